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
``i % len(points)``.  There is no CPU path: a GPU is required."""
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
