"""Drop-in for the mesh sampling stage of ``network/point_sample/pc_sample_sphere.py`` (:90-116, :125-206): ``load_obj``,
``uniform_sample``, ``farthest_point_sampling`` and ``sample_points_from_mesh`` with the reference's signatures, on the device.

The reference draws one sample per Python iteration from ``np.random`` and thins by an n x n distance matrix.  Here the uniforms
are drawn in one ``np.random.random_sample((n, 3))`` -- the same 3 n doubles in the same order, row i being sample i's
``np.random.random()`` then ``np.random.random(2)``, so ``np.random`` is left in the state the reference leaves it -- and every
sample is computed by one launch (``ops.mesh_sample``, ``csrc/meshsample.hip``) with the reference's float64 arithmetic: the
returned arrays equal the reference's bit for bit wherever no ``u * total`` falls within rounding of a cumulative-area boundary
(DESIGN.md section 3 "Mesh surface sampling").

Differences from the reference, all stated here: vertices are rounded to float32 on entry, as ``ops.MeshSet`` stores them; faces
must be triangles; ``farthest_point_sampling`` runs on ``tgp_fps`` (float32 coordinates, torch's ``pairwise_distance`` with its 1e-6
offset, the lowest index among equal maxima) where the reference takes float64 plain distances, so on near-ties the two can pick
different points; clouds above ``ops.fps_max_points()`` raise ValueError; with ``n_samples >= len(points)`` the indices are
``i % len(points)``.  There is no CPU path: a GPU is required.

The ball crop of the same file (:15-48, :209-280, :283-453): ``crop_ball_from_pts`` / ``crop_ball_from_depth_image`` with the
reference's signatures on ``ops.ball_cloud_pts`` (csrc/ballcrop.hip; DESIGN.md section 3 "Ball crop and tracking"), the index
plumbing round them (``backproject``, ``sample_bp_depth``, ``crop_mask_depth_image``, ``random_sample``) as torch code on the
inputs' device, ``farthest_point_sample`` on ``tgp_fps`` (the reference's device branch imports a module it does not ship), and
the host helpers (``occlude_obj_by_bboxes``, box corners / projection) in NumPy.  Differences, all stated here: points are
compared in float32; the square root of the distance is correctly rounded, where torch's CPU square root is not always -- a
point whose distance lies within an ulp of a radius can fall on the other side; a tensor radius is not multiplied in place;
``crop_ball_from_depth_image`` raises ValueError on a frame without a valid pixel (or whose balls never hold a point), where
the reference recurses until RecursionError -- an empty crop of a frame that has valid pixels is retried with the ratio grown by
1.2, as there; ``sample_bp_depth`` keeps (1, 3) shapes for a single valid pixel where the reference's ``squeeze`` drops the
axis; ``farthest_point_sample`` thins a list above ``ops.fps_max_points()`` evenly first; the batched, read-back-free form of all
this is ``evaluation.load_data_eval.clouds_from_poses``."""
import numpy as np
import torch

from ... import ops

DEVICE = "cuda"


def load_obj(path_to_file):
    """the ``v`` and ``f`` lines of an OBJ file -> vertices (V, 3) float64, faces (F, k) int, 0-based (``f a/b/c`` and ``f a//c``
    keep the vertex index a)"""
    vertices, faces = [], []
    with open(path_to_file, "r") as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                vertices.append([float(x) for x in tok[1:]])
            elif tok[0] == "f":
                faces.append([int(t.split("/")[0]) - 1 for t in tok[1:]])
    return np.asarray(vertices), np.asarray(faces)


def _meshset(vertices, faces):
    return ops.MeshSet([(np.asarray(vertices), np.asarray(faces))], device=DEVICE)


def uniform_sample(vertices, faces, n_samples, with_normal=False):
    """n_samples points on the surface, faces chosen by area -> float64 (n, 3), or (n, 6) with the face normals"""
    ms = _meshset(vertices, faces)
    u = torch.from_numpy(np.random.random_sample((1, int(n_samples), 3))).to(ms.device)
    out = ops.mesh_sample(ms, [0], int(n_samples), u=u, normals=bool(with_normal), dtype=torch.float64)
    return out["points"][0].cpu().numpy()


def farthest_point_sampling(points, n_samples):
    """indices (n_samples,) of the farthest point sampling that starts at point 0"""
    pts = np.ascontiguousarray(np.asarray(points)[:, :3], dtype=np.float32)
    if len(pts) > ops.fps_max_points():
        raise ValueError("farthest_point_sampling: %d points are above the cap of %d" % (len(pts), ops.fps_max_points()))
    idx = ops.farthest_points(torch.from_numpy(pts).to(DEVICE)[None], int(n_samples), init_center=False)
    return idx[0].cpu().numpy().astype(np.int64)


def sample_points_from_mesh(path, n_pts, with_normal=False, fps=False, ratio=2):
    """path: an OBJ file or a (vertices, faces) pair -> (n_pts, 3 | 6) float64; fps: ratio * n_pts samples thinned to n_pts"""
    vertices, faces = load_obj(path) if isinstance(path, str) else path
    if not fps:
        return uniform_sample(vertices, faces, n_pts, with_normal)
    ms = _meshset(vertices, faces)
    m = int(ratio) * int(n_pts)
    if m > ops.fps_max_points():
        raise ValueError("sample_points_from_mesh: ratio * n_pts = %d is above the cap of %d points" % (m, ops.fps_max_points()))
    u = torch.from_numpy(np.random.random_sample((1, m, 3))).to(ms.device)
    out = ops.mesh_sample_fps(ms, [0], int(n_pts), int(ratio), u=u, normals=bool(with_normal), dtype=torch.float64)
    return out["points"][0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ ball crop round a pose (:15-48, :209-453)
def occlude_obj_by_bboxes(bbox, mask):
    """Zero one quadrant-anchored three-quarter block of the box (x1, y1, x2, y2) in ``mask`` -- the first of the four (anchored right
    down, left down, left up, right up; the first index of ``mask`` runs along x, as in the reference) that removes anything ->
    (occluded mask, remaining share of the mask's sum).  When none does, the last one tried is returned with share 1.0."""
    x1, y1, x2, y2 = bbox.type(torch.int).tolist()
    xq, yq = int(x1 * 0.75 + x2 * 0.25), int(y1 * 0.75 + y2 * 0.25)          # a quarter of the way in
    xt, yt = int(x1 * 0.25 + x2 * 0.75), int(y1 * 0.25 + y2 * 0.75)          # three quarters
    total = mask.sum().item()
    for rows, cols in ((slice(xq, x2), slice(yq, y2)), (slice(x1, xt), slice(yq, y2)), (slice(x1, xt), slice(y1, yt)),
                       (slice(xq, x2), slice(y1, yt))):
        out = mask.clone()
        out[rows, cols] = 0
        out = out.contiguous()
        share = out.sum().item() / total
        if share < 1.0:
            break
    return out, share


def _valid_rows(depth_z, mask):
    ok = depth_z > 0
    if mask is not None:
        ok = torch.logical_and(mask, ok)
    return ok.flatten().nonzero()[:, 0]


def sample_bp_depth(image, depth, coord, mask=None):
    """rows of the (H,W,3) maps ``image`` / ``depth`` (back-projected points) / ``coord`` at the pixels with z > 0 inside ``mask``, in
    row-major order -> (rgb, pts, nocs); nocs None without coord"""
    rows = _valid_rows(depth[:, :, -1], mask)
    if coord is not None:
        assert coord.shape[-1] == 3
    return image.reshape(-1, 3)[rows], depth.reshape(-1, 3)[rows], None if coord is None else coord.reshape(-1, 3)[rows]


def backproject(depth, intrinsics, mask=None):
    """depth (H,W) -> the points ((x - cx) z / fx, (y - cy) z / fy, z) of the pixels with z > 0 inside ``mask``, row-major, (n,3)"""
    assert depth.ndim == 2, depth.ndim
    H, W = depth.shape
    ys = torch.arange(H, device=depth.device, dtype=depth.dtype) - intrinsics[1, 2]
    xs = torch.arange(W, device=depth.device, dtype=depth.dtype) - intrinsics[0, 2]
    pts = torch.stack((xs[None, :] * depth / intrinsics[0, 0], ys[:, None] * depth / intrinsics[1, 1], depth), dim=2)
    return pts.reshape(-1, 3)[_valid_rows(depth, mask)]


def random_sample(xyz, npoint):
    """npoint row numbers of xyz: a prefix of torch.randperm(len(xyz)) (the CPU generator, as the reference), and further
    permutations' prefixes while that is short"""
    if len(xyz) == 0 and npoint > 0:
        raise ValueError("random_sample: nothing to draw from")
    parts, have = [], 0
    while have < npoint:
        part = torch.randperm(len(xyz))[:npoint - have]
        parts.append(part)
        have += len(part)
    return torch.cat(parts, dim=0) if parts else torch.zeros(0, dtype=torch.long)


def farthest_point_sample(xyz, npoint, device=None):
    """farthest point sampling of xyz (N,3) from its centroid (the reference's farthest_points, init_center=True) on the device
    -> (npoint,) int64 row numbers on the CPU; every row once when npoint >= N, as there.  ``device``: kept for the signature."""
    xyz = torch.as_tensor(xyz)
    N = len(xyz)
    if npoint >= N:
        return torch.arange(N, dtype=torch.long)
    pts = xyz.detach().to(DEVICE, torch.float32).reshape(1, N, 3)
    rows = None
    if N > ops.fps_max_points():
        m = ops.fps_max_points()
        rows = (torch.arange(m, device=pts.device, dtype=torch.int64) * N) // m
        pts = pts[:, rows].contiguous()
    idx = ops.farthest_points(pts.contiguous(), int(npoint), init_center=True)[0].long()
    return (idx if rows is None else rows[idx]).cpu()


def _ladder(radius, num_points, dev):
    """the radii the reference's loop tests: ten rungs (ops.ball_ladder) with num_points, the first radius alone without"""
    if torch.is_tensor(radius):
        lad = ops.ball_ladder(radius.detach().reshape(1).to(dev, torch.float32))
    else:                                           # a Python number: max(radius, 0.05) and its products are doubles
        rungs, r = [], max(float(radius), 0.05)
        for _ in range(ops.BALL_LEVELS):
            rungs.append(r)
            r *= 1.10
        lad = torch.tensor([rungs], dtype=torch.float64).to(torch.float32).to(dev)
    return lad if num_points is not None else lad[:, :1].expand(-1, ops.BALL_LEVELS).contiguous()


def crop_ball_from_pts(pts, center, radius, num_points=None, device=None, fps_sample=False):
    """row numbers of pts (N,3) within ``max(radius, 0.05)`` of ``center``, ascending.  With num_points: the radius grows by 1.10 up
    to ten times until ten points are inside (every finite point when none is); the list is doubled until it holds num_points and
    num_points of it are drawn -- random_sample, or farthest_point_sample with fps_sample.  -> int64 tensor on pts' device."""
    src = torch.as_tensor(pts)
    empty = torch.zeros(0, dtype=torch.long, device=src.device)
    if len(src) == 0:
        return empty
    dev = torch.device(DEVICE)
    p = src.detach().to(dev, torch.float32).reshape(1, -1, 3).contiguous()
    c = torch.as_tensor(center).detach().to(dev, torch.float32).reshape(1, 3).contiguous()
    job = torch.zeros(1, dtype=torch.int32, device=dev)
    br = ops.ball_cloud_pts(p, job, c, _ladder(radius, num_points, dev))
    _, count, _, status = br.counts[0].tolist()
    if num_points is not None and status == 1:
        br = ops.ball_cloud_pts(p, job, c, torch.full((1, ops.BALL_LEVELS), 1e9, device=dev))
        count = br.counts[0, 1].item()
    idx = br.recs[0, :count].long()
    if num_points is None or count == 0:
        return idx.to(src.device)
    while len(idx) < num_points:
        idx = torch.cat([idx, idx], dim=0)
    pick = farthest_point_sample(p[0, idx], num_points, device) if fps_sample else random_sample(idx, num_points)
    return idx[pick.to(dev)].to(src.device)


def crop_mask_depth_image(image, depth, mask, coord=None, num_points=None):
    """num_points random rows (random_sample) of the valid pixels of ``mask`` -> (rgb, pts, nocs)"""
    assert depth.shape[-1] == 3
    rgb, pts, nocs = sample_bp_depth(image, depth, coord, mask)
    pick = random_sample(pts, num_points).to(pts.device)
    return rgb[pick], pts[pick], None if nocs is None else nocs[pick]


def crop_ball_from_depth_image(image, depth, mask, pose, scale, ratio, cam_intrinsics, coord=None, num_points=None, device=None,
                               fps_sample=False):
    """the valid pixels of the point map ``depth`` (H,W,3) within ``ratio * |pose[:, :3] @ scale|`` of the pose's translation
    (crop_ball_from_pts) -> (rgb, pts, nocs) rows.  An empty crop is tried again with the ratio grown by 1.2, as the reference's
    call of itself does, until a ball holds a point.  ValueError when no pixel is valid, or no ball up to an infinite radius
    holds one (the reference recurses without end in both cases)."""
    assert depth.shape[-1] == 3
    rgb, pts, nocs = sample_bp_depth(image, depth, coord, mask)
    if len(pts) == 0:
        raise ValueError("crop_ball_from_depth_image: no valid pixel (the reference recurses without end here)")
    extent = torch.norm(pose[:, :3] @ scale)
    for _ in range(600):                            # a float32 radius that grows at all is infinite well before this
        idx = crop_ball_from_pts(pts, pose[:, 3], ratio * extent, num_points, device=device, fps_sample=fps_sample)
        if len(idx):
            return rgb[idx], pts[idx], None if nocs is None else nocs[idx]
        ratio = ratio * 1.2
    raise ValueError("crop_ball_from_depth_image: no ball round the centre holds a point (the reference recurses without end here)")


def get_corners(points):
    """(..., N, 3) -> (..., 2, 3): the componentwise minimum and maximum"""
    if isinstance(points, torch.Tensor):
        points = points.detach().cpu().numpy()
    points = np.asarray(points)
    return np.stack([points.min(axis=-2), points.max(axis=-2)], axis=-2)


def bbox_from_corners(corners):
    """(..., 2, 3) minimum / maximum -> (..., 8, 3) box corners; corner i takes x from i % 4 // 2, y from i // 4, z from i % 2"""
    corners = np.asarray(corners)
    i = np.arange(8)
    return np.stack([corners[..., (i % 4) // 2, 0], corners[..., i // 4, 1], corners[..., i % 2, 2]], axis=-1).astype(np.float64)


def project(pts, intrinsics, scale=1000):
    """(N,3) camera-frame points -> (N,2) pixel coordinates of K @ (-x/z, -y/z, 1) (y not flipped)"""
    pts = np.asarray(pts) * scale
    pts = -pts / pts[:, -1:]
    pts[:, -1] = -pts[:, -1]
    return (intrinsics @ pts.T).T[:, :2]


def get_proj_corners(depth, center, radius, cam_intrinsics):
    """the (row, column) rectangle [[rmin, cmin], [rmax, cmax]] of the projected cube of half side max(radius, 0.05) round center,
    clipped to the (H,W) of ``depth``; rows are counted from the bottom (height - v), as in the reference"""
    radius = max(radius, 0.05)
    box = bbox_from_corners(get_corners([center - np.ones(3) * radius, center + np.ones(3) * radius]))
    height, width = depth.shape
    rc = project(box, cam_intrinsics).astype(np.int32)[:, [1, 0]]
    rc[:, 0] = height - rc[:, 0]
    out = np.stack([rc.min(axis=0), rc.max(axis=0)], axis=0)
    out[0] = np.maximum(out[0], 0)
    out[1] = np.minimum(out[1], np.array([height - 1, width - 1]))
    return out


def get_bbox_from_scale(scale):
    """(3,) extents -> (8,3) float32 corners of the centred box, +++ -++ --+ +-+ then the same with z negative"""
    hx, hy, hz = scale[0] / 2, scale[1] / 2, scale[2] / 2
    return np.array([[hx, hy, hz], [-hx, hy, hz], [-hx, -hy, hz], [hx, -hy, hz],
                     [hx, hy, -hz], [-hx, hy, -hz], [-hx, -hy, -hz], [hx, -hy, -hz]], dtype=np.float32)
