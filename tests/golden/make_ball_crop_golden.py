"""Regenerates tests/golden/ball_crop_ref.npz from the REFERENCE's own ``network/point_sample/pc_sample_sphere.py`` (loaded by path,
unmodified, with stand-in ``cv2`` / ``tqdm`` / ``matplotlib`` modules it imports and never calls here; its ``farthest_points_torch``
is found beside it), on the CPU.

Stored: small clouds and one small depth frame with their centres and radii, and what the reference returned --
  crop_ball_from_pts            num_points=None; num_points set under a recorded torch seed; fps_sample=True, device='cpu'
  crop_ball_from_depth_image    with and without a mask, random and farthest point selection (the image is the pixel index, so the
                                returned rgb rows are the chosen pixels); one case whose first balls are empty (num_points=None):
                                the reference's retries with the ratio grown by 1.2
  occlude_obj_by_bboxes, get_proj_corners / project / get_corners / bbox_from_corners / get_bbox_from_scale
  the radii the reference's loop compares with, for a radius on either side of 0.05, observed through a tensor subclass that logs
  the right-hand side of ``distance <= radius``.

The maker ASSERTS the conditions under which the contract (tests/ball_ref.py) and the reference must agree, and moves to the next
seed when one fails:
  1. no point's distance, computed in float64, lies within a relative 1e-6 of a radius it is compared with (torch's CPU square root
     is not correctly rounded; the contract's is);
  2. in every farthest point case the best running distance exceeds the best of the other distinct points by at least 2e-5 m at
     every step that still has a distinct point to choose: torch's 1e-6 offset (at most 1.8e-6) and float32 rounding of coordinates
     below 1 m (6e-8) cannot change the choice.  Copies of one point tie exactly and the lowest index wins on both sides.

Usage:  python tests/golden/make_ball_crop_golden.py REFERENCE_ROOT   (from the repo root; or set $TGP_REFERENCE)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_augment_golden as mag  # noqa: E402  (puts REF and the repo on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import ball_ref as br  # noqa: E402

REF = mag.REF
F = np.float32
N_CLOUD, NUM = 300, 64
H, W = 48, 64
CAMK = (60.0, 61.0, 31.5, 23.25)
GAP, MARGIN = 1e-6, 2e-5


def load_reference():
    for name in ("cv2", "tqdm", "matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.tqdm = lambda it, *a, **k: it
            sys.modules[name] = m
    sys.path.append(os.path.join(REF, "network", "point_sample"))
    return mag._load_by_path("ref_pc_sample_sphere_ball", os.path.join(REF, "network/point_sample/pc_sample_sphere.py"))


class Spy(torch.Tensor):
    """logs the right-hand side of every <= it takes part in"""
    seen = []

    @classmethod
    def __torch_function__(cls, func, types_, args=(), kwargs=None):
        if getattr(func, "__name__", "") in ("le", "__le__"):
            rhs = args[1]
            cls.seen.append(float(rhs) if not torch.is_tensor(rhs) else float(rhs.float()))
        return super().__torch_function__(func, types_, args, kwargs or {})


def d64(pts, center):
    return np.sqrt(((pts.astype(np.float64) - np.asarray(center, np.float64)) ** 2).sum(-1))


def clear_of(pts, center, radii):
    """condition 1 for the radii given"""
    d = d64(pts, center)
    return all(np.abs(d - float(r)).min() > GAP * float(r) for r in radii)


def fps_margin(pts, n):
    """condition 2: farthest_points' loop in float64 (from the mean), the smallest lead of the winner over every point that is not
    a copy of it, over the steps at which such a point still has a positive running distance"""
    p = pts.astype(np.float64)
    run = np.sqrt(((p - p.mean(0)) ** 2).sum(-1))
    worst = np.inf
    for _ in range(n):
        c = int(np.argmax(run))
        other = run[(p != p[c]).any(1)]
        if len(other) and other.max() > 1e-5:
            worst = min(worst, run[c] - other.max())
        run = np.minimum(run, np.sqrt(((p - p[c]) ** 2).sum(-1)))
    return worst


def cloud(seed):
    r = np.random.RandomState(seed)
    return (r.randn(N_CLOUD, 3) * 0.06 + np.array([0.03, -0.02, 0.8])).astype(F)


def pts_cases(pts):
    """name -> (centre, radius, expected (L, status) with num_points); radii placed between sorted distances"""
    near, far = np.array([0.03, -0.02, 0.8], F), np.array([0.03, -0.02, 1.6], F)
    dn, df = np.sort(d64(pts, near)), np.sort(d64(pts, far))
    mid = lambda d, k: 0.5 * (d[k - 1] + d[k])          # a radius that holds exactly k points
    return {
        "level0": (near, mid(dn, 40), 0, 0),
        "small": (near, 0.01, None, 0),                                     # below 0.05: the Python-float branch
        "twelve": (far, mid(df, 12), 0, 0),                                 # 12 points -> 64 samples draw only from those 12
        "exact10": (far, mid(df, 10), 0, 0),
        "exact9": (far, mid(df, 9), 1, 0),
        "level3": (far, mid(df, 14) / 1.1 ** 3, 3, 0),
        "few9": (far, mid(df, 4) / 1.1 ** 9, 9, 0),                         # 4 points at the tenth radius: kept, not grown further
        "none9": (far, 0.06, 9, 1),                                         # nothing within 0.06 * 1.1^9: every point
    }


def frame(seed):
    """a table plane with an object in front of it, holes (0) and one saturated pixel (65535)"""
    r = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    dep = 900.0 + 0.8 * ys + r.rand(H, W) * 3.0
    rr = (xs - 36.0) ** 2 + (ys - 20.0) ** 2
    obj = rr < 9.5 ** 2
    dep[obj] = 600.0 - np.sqrt(9.5 ** 2 - rr[obj]) * 6.0 + r.rand(int(obj.sum())) * 2.0
    dep[r.rand(H, W) < 0.05] = 0
    dep = dep.astype(np.uint16)
    dep[2, 3] = 65535
    return dep, obj


def main():
    ref = load_reference()
    out = {}
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    # ---- the ladder, as the reference's comparisons show it
    for name, radius in (("big", 0.0625), ("small", 0.03)):
        Spy.seen = []
        pts = T(np.zeros((4, 3), F) + F(50.0)).as_subclass(Spy)
        got = ref.crop_ball_from_pts(pts, torch.zeros(3), torch.tensor(radius, dtype=torch.float32), num_points=8)
        assert len(got) == 8 and len(Spy.seen) == 11, (len(got), len(Spy.seen))        # ten rungs, then the 1e9 fallback
        out["ladder.%s.radius" % name] = F(radius)
        out["ladder.%s.rungs" % name] = np.asarray(Spy.seen[:10], np.float64).astype(F)
        assert np.array_equal(out["ladder.%s.rungs" % name], br.ladder_of(F(radius))), name

    # ---- crop_ball_from_pts
    seed = 11
    while True:
        pts = cloud(seed)
        cases = pts_cases(pts)
        ok = True
        for name, (c, radius, L, status) in cases.items():
            lad = br.ladder_of(F(radius))
            _, counts = br.ball_cloud_pts(pts, c, lad)
            ok &= clear_of(pts, c, lad[:counts[2] + 1]) and (L is None or (counts[2], counts[3]) == (L, status))
        keep12, _ = br.ball_cloud_pts(pts, cases["twelve"][0], br.ladder_of(F(cases["twelve"][1])))
        keep40, _ = br.ball_cloud_pts(pts, cases["level0"][0], [F(0.2)] * 10)
        dbl = np.tile(pts[keep12.astype(np.int64)], (8, 1))
        ok &= len(keep12) == 12 and len(keep40) > NUM and fps_margin(dbl, NUM) >= MARGIN
        ok &= fps_margin(pts[keep40.astype(np.int64)], NUM) >= MARGIN and clear_of(pts, cases["level0"][0], [F(0.2)])
        if ok:
            break
        seed += 1
    print("cloud seed %d" % seed)
    out["pts.cloud"], out["pts.names"] = pts, np.asarray(list(cases))
    for k, (name, (c, radius, L, status)) in enumerate(cases.items()):
        rad = lambda: torch.tensor(float(radius), dtype=torch.float32)      # a fresh tensor: the reference multiplies it in place
        out["pts.%s.center" % name], out["pts.%s.radius" % name] = c, F(radius)
        out["pts.%s.all" % name] = ref.crop_ball_from_pts(T(pts), T(c), rad()).numpy()
        torch.manual_seed(100 + k)
        out["pts.%s.seed" % name] = np.int64(100 + k)
        out["pts.%s.drawn" % name] = ref.crop_ball_from_pts(T(pts), T(c), rad(), num_points=NUM).numpy()
        out["pts.%s.next" % name] = torch.randperm(5).numpy()            # the generator's state afterwards
    c, radius = cases["twelve"][:2]
    out["pts.twelve.fps"] = ref.crop_ball_from_pts(T(pts), T(c), torch.tensor(float(radius), dtype=torch.float32), num_points=NUM,
                                                   device="cpu", fps_sample=True).numpy()
    first = out["pts.twelve.fps"]
    assert len(set(first[:12].tolist())) == 12 and (first[12:] == first[12]).all() and first[12] == out["pts.twelve.all"][0]
    out["pts.level0.fps_radius"] = F(0.2)
    out["pts.level0.fps"] = ref.crop_ball_from_pts(T(pts), T(cases["level0"][0]), torch.tensor(0.2, dtype=torch.float32),
                                                   num_points=NUM, device="cpu", fps_sample=True).numpy()

    # ---- crop_ball_from_depth_image
    seed = 5
    pose = np.concatenate([mag.rot(3) * F(1.0), np.array([[0.075], [-0.055], [0.56]], F)], 1).astype(F)
    scale, ratio = np.array([0.10, 0.12, 0.08], F), 0.45
    radius = (ratio * torch.norm(T(pose)[:, :3] @ T(scale))).float().numpy()
    while True:
        dep, obj = frame(seed)
        pix_all = np.arange(H * W)
        cloud_all = br.pixel_points(pix_all % W, pix_all // W, dep.reshape(-1), CAMK)
        ok = True
        for mask in (None, obj):
            recs, counts = br.ball_cloud(dep, CAMK, pose[:, 3], br.ladder_of(radius), mask=mask)
            v = br.valid_pixels(dep, mask)
            ok &= clear_of(cloud_all[v], pose[:, 3], br.ladder_of(radius)[:counts[2] + 1]) and counts[3] == 0 and counts[1] > NUM
            ok &= fps_margin(cloud_all[recs.astype(np.int64)], NUM) >= MARGIN
        if ok:
            break
        seed += 1
    print("frame seed %d, %d pixels in the masked crop" % (seed, counts[1]))
    image = T(np.repeat(pix_all.reshape(H, W, 1), 3, axis=2))
    depth3 = T(cloud_all.reshape(H, W, 3))
    coord = T((cloud_all.reshape(H, W, 3) * F(0.5)).astype(F))
    out["img.depth"], out["img.mask"], out["img.camk"] = dep, obj, np.asarray(CAMK, F)
    out["img.pose"], out["img.scale"], out["img.ratio"], out["img.radius"] = pose, scale, np.float64(ratio), radius
    K = np.array([[CAMK[0], 0, CAMK[2]], [0, CAMK[1], CAMK[3]], [0, 0, 1]], F)
    for name, mask, kw in (("nomask_all", None, {}), ("mask_all", obj, {}), ("nomask_drawn", None, dict(num_points=NUM)),
                           ("mask_drawn", obj, dict(num_points=NUM)), ("mask_fps", obj, dict(num_points=NUM, device="cpu", fps_sample=True))):
        torch.manual_seed(7)
        rgb, p, nocs = ref.crop_ball_from_depth_image(image, depth3, None if mask is None else T(mask), T(pose), T(scale), ratio, K,
                                                      coord=coord, **kw)
        pix = rgb[:, 0].numpy()
        assert np.array_equal(p.numpy(), cloud_all[pix]) and np.array_equal(nocs.numpy(), coord.reshape(-1, 3).numpy()[pix])
        out["img.%s.pix" % name] = pix.astype(np.int32)
    out["img.seed"] = np.int64(7)
    # an empty first ball with num_points=None: the reference calls itself with ratio * 1.2 until a ball holds a point
    pose_g = pose.copy()
    pose_g[2, 3] -= F(0.2)                                    # 0.2 m in front of the object
    grown, r = [], ratio
    while True:
        rad = (r * torch.norm(T(pose_g)[:, :3] @ T(scale))).float().numpy()
        lad0 = np.repeat(br.ladder_of(rad)[:1], br.LEVELS)
        assert clear_of(cloud_all[br.valid_pixels(dep, obj)], pose_g[:, 3], lad0[:1]), "a distance too near a grown radius"
        recs, _ = br.ball_cloud(dep, CAMK, pose_g[:, 3], lad0, mask=obj)
        grown.append(rad)
        if len(recs):
            break
        r = r * 1.2
    assert len(grown) >= 3
    rgb, p, nocs = ref.crop_ball_from_depth_image(image, depth3, T(obj), T(pose_g), T(scale), ratio, K, coord=coord)
    out["img.grow.pose"], out["img.grow.radii"], out["img.grow.pix"] = pose_g, np.asarray(grown, F), rgb[:, 0].numpy().astype(np.int32)
    assert np.array_equal(out["img.grow.pix"], recs.astype(np.int32))

    # ---- host helpers
    m = torch.zeros(40, 48, dtype=torch.uint8)
    m[10:30, 12:40] = 1
    boxes = np.array([[8, 10, 32, 42], [0, 0, 10, 12], [25, 30, 40, 48], [9, 11, 13, 15]], np.float32)
    out["occ.mask"], out["occ.boxes"] = m.numpy(), boxes
    for k, b in enumerate(boxes):
        om, share = ref.occlude_obj_by_bboxes(T(b), m)
        out["occ.%d.mask" % k], out["occ.%d.share" % k] = om.numpy(), np.float64(share)
    c3 = np.array([0.05, -0.04, 0.7])
    out["geo.center"], out["geo.K"] = c3, K.astype(np.float64)
    out["geo.proj_corners"] = ref.get_proj_corners(np.zeros((H, W)), c3, 0.11, K.astype(np.float64))
    out["geo.proj_corners_small"] = ref.get_proj_corners(np.zeros((H, W)), c3, 0.01, K.astype(np.float64))
    cs = ref.get_corners(pts[:50])
    out["geo.corners"], out["geo.bbox"] = cs, ref.bbox_from_corners(cs)
    out["geo.project"] = ref.project(pts[:50].astype(np.float64), K.astype(np.float64))
    out["geo.bbox_from_scale"] = ref.get_bbox_from_scale(np.array([0.2, 0.1, 0.3]))
    path = os.path.join(HERE, "ball_crop_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote ball_crop_ref.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
