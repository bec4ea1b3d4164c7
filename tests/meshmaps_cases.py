"""The cases of the mesh maps (include/tgpose.h tgp_mesh_maps), shared by tests/test_meshmaps_cpu.py (the restatement alone) and
tests/test_meshmaps_gpu.py (the kernel against the restatement).  They are small: the kernel can go wrong at tile, chunk and record
edges, not at workload size.  A case is one call: dict(meshes, vnormals, camk (S,4), job_img, job_mesh (J), job_pose (J,3,4), window
(J,4), h, w, near); expected(name) is the restatement's result, computed once and shared (do not write to it)."""
import functools

import numpy as np

from tests import icp_ref
from tests import meshmaps_ref as mr
from tests.render_ref import pose34
from tgpose_amd.datasets import shapes

F = np.float32
FULL = (0.0, 0.0, 1.0, 1.0)
EYE = np.eye(3)


def call(meshes, camk, job_pose, window, h, w, job_img=None, job_mesh=None, near=0.01, vnormals=None):
    J = len(job_pose)
    camk = np.asarray(camk, F).reshape(-1, 4)
    return dict(meshes=[(np.ascontiguousarray(v, F), np.ascontiguousarray(f, np.int32).reshape(-1, 3)) for v, f in meshes], vnormals=vnormals,
                camk=camk, job_img=np.asarray(job_img if job_img is not None else [0] * J, np.int32),
                job_mesh=np.asarray(job_mesh if job_mesh is not None else [0] * J, np.int32),
                job_pose=np.ascontiguousarray(np.stack([np.asarray(p, F).reshape(3, 4) for p in job_pose])),
                window=np.ascontiguousarray(np.asarray(window, F).reshape(J, 4)), h=h, w=w, near=near)


def tilted_triangle():
    """one triangle that fills a small frame, its depth different at each corner"""
    return np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.2], [0.0, 1.2, 0.5]], F), np.array([[0, 1, 2]], np.int32)


def stack_of_triangles(n=700, seed=5):
    """n triangles far larger than the 16 x 16 frame they are seen in under K = (40, 40, 8, 8) at depth 1, their corners moved about
    so that each covers its own part of the frame, at n depths in no order, each with its own tilt: the box of every one of them
    meets the frame's only tile, so each is a record of it"""
    r = np.random.RandomState(seed)
    base = np.array([[-2.0, -1.5, 0.0], [2.0, -1.5, 0.0], [0.0, 2.5, 0.0]])
    v = np.concatenate([base + np.concatenate([r.uniform(-1.9, 1.9, (3, 2)), 0.2 * r.permutation(n)[t] / n + r.uniform(-0.4, 0.4, (3, 1))], 1)
                        for t in range(n)])
    return v.astype(F), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def sliver():
    """a triangle that is degenerate in the MODEL frame -- corners 0, d and 2 d: the cross product of its edges is an exact zero in
    float32 -- posed so that the snapping of its three corners gives it a snapped area that is not zero and one sample inside: the
    rasteriser has a winner there (tests/test_meshmaps_cpu.py holds that), the maps must not (no normal).  Behind it an honest triangle
    over the whole frame, which the sliver hides in that one cell."""
    r = np.random.RandomState(33)
    d = r.uniform(-0.12, 0.12, 3).astype(F)
    d[2] *= F(0.3)
    R = icp_ref.rot(r.uniform(-1, 1, 3), r.uniform(0, 40))
    t = np.array([r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05), 0.5])
    v = np.stack([np.zeros(3, F), d, F(2) * d, [-1, -1, 0.25], [1, -1, 0.25], [0, 1.5, 0.25]]).astype(F)
    return (v, np.array([[0, 1, 2], [3, 4, 5]], np.int32)), pose34(R, t)


SLIVER_K = (60.0, 60.0, 16.0, 16.0)


@functools.lru_cache(maxsize=None)
def calls():
    tri = tilted_triangle()
    sphere = shapes.icosphere(0.1, 1)                                                  # 80 faces
    front = pose34(EYE, [0, 0, 1.5])
    K16 = (6.0, 6.0, 7.6, 7.3)
    c = {}
    c["one_cell"] = call([tri], (6.0, 6.0, 0.2, 0.1), [front], [FULL], 1, 1)
    c["partial_tiles"] = call([sphere], (100.0, 90.0, 16.3, 8.2), [pose34(icp_ref.rot([1, 2, 3], 25.0), [0.01, -0.005, 0.7])], [FULL], 17, 33)
    # the only triangle lies between the samples of pixels (3, 3) and (4, 4)
    tiny = (np.array([[-0.048, -0.048, 0], [-0.042, -0.047, 0], [-0.045, -0.042, 0]], F), np.array([[0, 1, 2]], np.int32))
    c["no_sample"] = call([tiny], (100.0, 100.0, 8.0, 8.0), [pose34(EYE, [0, 0, 1.0])], [FULL], 16, 16)
    c["cap_sweep"] = call([stack_of_triangles()], (40.0, 40.0, 8.0, 8.0), [pose34(EYE, [0, 0, 1.0])], [FULL], 16, 16)
    c["coincident"] = call([(tri[0], np.array([[0, 1, 2], [0, 1, 2], [0, 2, 1]], np.int32))], K16, [front], [FULL], 16, 16)
    c["windings"] = call([tri, (tri[0], np.array([[0, 2, 1]], np.int32))], K16, [front, front], [FULL, FULL], 16, 16, job_mesh=[0, 1])
    # face 0 has a corner behind near, face 1 a corner beyond the guard band (u = 6 * 5000 / 1.5 px > 16384), face 2 is seen
    v = np.concatenate([tri[0], [[0, 0, -1.495]], [[5000.0, 0, 0]]]).astype(F)
    c["near_guard"] = call([(v, np.array([[0, 1, 3], [0, 4, 2], [0, 1, 2]], np.int32))], K16, [front], [FULL], 16, 16)
    sl, slp = sliver()
    c["sliver"] = call([sl], SLIVER_K, [slp], [FULL], 32, 32)
    sp = pose34(icp_ref.rot([0, 1, 0], 30.0), [0, 0, 0.6])
    Ksp = (120.0, 120.0, 24.0, 20.0)
    nan = float("nan")
    c["windows"] = call([sphere], Ksp, [sp] * 6, [(6.25, 3.5, 0.5, 0.5), (44.0, 0.0, -1.0, 1.0), (nan, 0, 1, 1), (0, 0, 0, 1), (4, 2, 2.5, 1.75),
                                                  (0, 0, 1, float("inf"))], 40, 48)
    c["bad_index"] = call([sphere], Ksp, [sp] * 5, [FULL] * 5, 20, 24, job_img=[-1, 0, 1, 0, 0], job_mesh=[0, -1, 0, 1, 0])
    box = shapes.box((0.12, 0.08, 0.1))
    c["three_jobs"] = call([sphere, box, tri], [Ksp, (90.0, 95.0, 15.5, 12.5), (6.0, 6.0, 9.0, 9.0)],
                           [sp, pose34(icp_ref.rot([1, 1, 0], 40.0), [0.02, 0.01, 0.5], 1.1), front],
                           [(10.0, 8.0, 1.0, 1.0), (3.0, 2.0, 0.75, 0.8), (0.0, 0.0, 0.6, 0.6)], 24, 28, job_img=[0, 1, 2], job_mesh=[0, 1, 2])
    ball = shapes.icosphere(0.1, 2)                                                    # 320 faces: more than one chunk of boxes
    unit = (ball[0].astype(np.float64) / np.linalg.norm(ball[0].astype(np.float64), axis=1, keepdims=True)).astype(F)
    c["vertex_normals"] = call([ball], Ksp, [sp], [(4.0, 0.0, 0.85, 0.85)], 40, 48, vnormals=[unit])
    for x in c.values():
        for a in list(x.values()) + [m for pair in x["meshes"] for m in pair] + (x["vnormals"] or []):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


def run(c):
    return mr.maps(c["meshes"], c["camk"], c["job_img"], c["job_mesh"], c["job_pose"], c["window"], c["h"], c["w"], c["near"], c["vnormals"])


@functools.lru_cache(maxsize=None)
def expected(name):
    out = run(calls()[name])
    for a in out.values():
        a.setflags(write=False)
    return out


def job_alone(c, j):
    """job j of a call as a call of its own"""
    return dict(c, job_img=c["job_img"][j:j + 1], job_mesh=c["job_mesh"][j:j + 1], job_pose=c["job_pose"][j:j + 1], window=c["window"][j:j + 1])
