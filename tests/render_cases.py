"""The depth renderer's test scenes, shared by tests/test_render_cpu.py (the restatement against closed forms) and
tests/test_render_gpu.py (the kernel against the restatement).  A case is a dict of the kernel's host arguments; ``reference`` renders
it with tests/render_ref.py once per process."""
import functools

import numpy as np

from tests import render_ref
from tgpose_amd.datasets import shapes

H, W = 120, 160
CAMK = (144.375, 144.375, 79.5, 59.5)                     # the NOCS intrinsics divided by 4
K33 = np.array([[CAMK[0], 0, CAMK[2]], [0, CAMK[1], CAMK[3]], [0, 0, 1]], dtype=np.float32)


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def case(meshes, scenes, camk=CAMK, h=H, w=W, near=0.01):
    """scenes: list of lists of (mesh, inst_id, R, t, s) -> the kernel's host arguments"""
    ptr, mesh, ids, pose = [0], [], [], []
    for sc in scenes:
        for m, i, R, t, s in sc:
            mesh.append(m), ids.append(i), pose.append(render_ref.pose34(R, t, s))
        ptr.append(len(mesh))
    camk = np.asarray(camk, dtype=np.float32)
    camk = np.broadcast_to(camk, (len(scenes), 4)) if camk.ndim == 1 else camk
    return dict(meshes=meshes, scene_ptr=np.asarray(ptr, dtype=np.int32), inst_mesh=np.asarray(mesh, dtype=np.int32),
                inst_id=np.asarray(ids, dtype=np.uint8), inst_pose=np.stack(pose) if pose else np.zeros((0, 3, 4), dtype=np.float32),
                camk=np.array(camk, dtype=np.float32, order="C"), H=h, W=w, near=near)


I3, Z3 = np.eye(3), np.zeros(3)
RECT_K = (128.0, 128.0, 0.0, 0.0)
RECT_SPLITS = {"diag02": [(0, 1, 2), (0, 2, 3)], "diag13": [(0, 1, 3), (1, 2, 3)], "reversed": [(2, 1, 0), (3, 2, 0)]}


def rectangle(split):
    """a fronto-parallel rectangle at z = 1 whose corners project to pixel (10, 5) - (40.5, 20) under RECT_K"""
    x0, x1, y0, y1 = 10 / 128.0, 40.5 / 128.0, 5 / 128.0, 20 / 128.0
    v = np.array([[x0, y0, 1], [x1, y0, 1], [x1, y1, 1], [x0, y1, 1]], dtype=np.float32)
    return case([(v, np.asarray(RECT_SPLITS[split], dtype=np.int32))], [[(0, 1, I3, Z3, 1.0)]], camk=RECT_K)


PLANE_R = rot("x", 20) @ rot("y", 50)                    # rotated 50 degrees about y and then 20 degrees about x
PLANE_T = np.array([0.01, -0.02, 0.9])


def slanted_plane(n):
    return case([shapes.plane(0.6, 0.6, n, n)], [[(0, 1, PLANE_R, PLANE_T, 1.0)]])


def plane_depth_analytic():
    """the ray-plane depth of every pixel's sample point (fp64), +inf where the ray is parallel"""
    nrm = PLANE_R[:, 2]
    jj, ii = np.mgrid[0:H, 0:W].astype(np.float64)
    fx, fy, cx, cy = (float(np.float32(k)) for k in CAMK)
    den = nrm[0] * (ii - cx) / fx + nrm[1] * (jj - cy) / fy + nrm[2]
    return float(nrm @ PLANE_T) / den


CUBE_R = rot("z", 25) @ rot("x", 35) @ rot("y", 40)
CUBE_T = np.array([0.02, -0.01, 0.8])
CUBE_S = 0.2


def cube():
    return case([shapes.box(1.0)], [[(0, 7, CUBE_R, CUBE_T, CUBE_S)]])


def closure_error(points, R, t, s, half=0.5):
    """camera-frame points (n,3) of a box of half-extent ``half`` model units posed by (R, t, s) -> (largest distance to the nearest
    face plane, largest excess over the half-extent), both in metres"""
    q = (np.asarray(points, dtype=np.float64) - np.asarray(t, dtype=np.float64)) @ np.asarray(R, dtype=np.float64) / float(s)
    d = np.abs(np.abs(q) - half)
    return float(d.min(1).max() * s), float((np.abs(q).max(1) - half).max() * s)


def backproject(depth, camk):
    """the loaders' back-projection of a uint16 millimetre depth image -> (n,3) points of its non-zero pixels"""
    fx, fy, cx, cy = (float(np.float32(k)) for k in camk)
    jj, ii = np.nonzero(depth)
    d = depth[jj, ii].astype(np.float64) / 1000.0
    return np.stack([(ii - cx) * d / fx, (jj - cy) * d / fy, d], 1)


def rules():
    """one scene per rule: 0 a vertex behind near, 1 beyond the guard band, 2 zero area, 3 coplanar duplicate instances (ids not in
    slot order), 4 duplicate faces, 5 a surface beyond 65.535 m"""
    tri = lambda *v: (np.asarray(v, dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32))
    front = tri((-0.1, -0.1, 0.5), (0.1, -0.1, 0.5), (0.0, 0.1, 0.5))
    meshes = [tri((-0.1, -0.1, 0.5), (0.1, -0.1, 0.5), (0.0, 0.1, 0.005)),            # one vertex at z = 5 mm <= near
              tri((-0.1, -0.1, 0.5), (0.1, -0.1, 0.5), (2.0, 0.0, 0.0125)),           # u = 144.375 * 160 px: beyond 2^22 / 256
              tri((-0.1, -0.1, 0.5), (0.0, 0.0, 0.5), (0.1, 0.1, 0.5)),               # collinear
              front,
              (front[0], np.array([[0, 1, 2], [0, 1, 2]], dtype=np.int32)),
              tri((-20, -20, 70.0), (20, -20, 70.0), (0.0, 20, 70.0))]
    one = lambda m, i=1: (m, i, I3, Z3, 1.0)
    return case(meshes, [[one(0)], [one(1)], [one(2)], [one(3, 9), one(3, 4)], [one(4)], [one(5)]])


def tails():
    """123 x 157: a two-triangle table overhanging all four borders, an icosphere (level 3) and a lathe bottle through it"""
    meshes = [shapes.plane(3.0, 1.6, 1, 1), shapes.icosphere(0.5, 3), shapes.lathe(shapes.PROFILES["bottle"], 24)]
    Rt = rot("x", 35)                                       # every corner stays in front of the camera: z in 0.54 .. 1.46
    sc = [(0, 3, Rt, (0.0, 0.12, 1.0), 1.0), (1, 200, rot("y", 10), (-0.12, 0.05, 0.85), 0.2), (2, 17, rot("x", 150) @ rot("z", 12), (0.15, 0.0, 0.8), 0.3)]
    return case(meshes, [sc], h=123, w=157)


def tiny_triangles():
    """an icosphere of level 5 (20 480 faces) at 3 m: about 12 x 12 pixels, thousands of triangles in one tile"""
    return case([shapes.icosphere(0.125, 5)], [[(0, 5, rot("x", 17), (0.011, -0.007, 3.0), 1.0)]])


def three_scenes():
    """0, 1 and 7 instances, a camk per scene, inst_id values not in slot order"""
    meshes = [shapes.box(1.0), shapes.icosphere(0.5, 2), shapes.lathe(shapes.PROFILES["mug"], 16), shapes.cylinder(0.3, 1.0, 12)]
    rng = np.random.RandomState(5)
    seven = []
    for k, i in enumerate((40, 3, 255, 1, 77, 12, 8)):
        R = rot("z", rng.uniform(0, 360)) @ rot("x", rng.uniform(0, 360)) @ rot("y", rng.uniform(0, 360))
        seven.append((k % 4, i, R, (rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.2)), rng.uniform(0.1, 0.3)))
    camk = np.array([CAMK, (150.0, 140.0, 70.25, 66.5), (130.5, 133.0, 85.0, 55.75)], dtype=np.float32)
    return case(meshes, [[], [(1, 9, rot("y", 30), (0.05, 0.0, 0.7), 0.3)], seven], camk=camk)


RASTER_THREADS, RASTER_CAP = 256, 512                     # csrc/raster.h: the boxes a tile walks per chunk, the records its list holds
CARRY_IDS = (11, 22)


def tile_walk(c, scene=0, tile=(0, 0)):
    """The record list of one 16 x 16 tile over its scene's instance slots, as csrc/raster.h walks it: per slot, the number of records
    held after the slot's last chunk, and the sizes of the lists swept inside the slot's walk -- a list is swept, and emptied, when
    it holds more than RASTER_CAP - RASTER_THREADS records after a chunk of RASTER_THREADS boxes.  The boxes are render_ref's."""
    tx0, ty0 = tile[0] * 16, tile[1] * 16
    held, n = [], 0
    for i in range(int(c["scene_ptr"][scene]), int(c["scene_ptr"][scene + 1])):
        verts, faces = c["meshes"][int(c["inst_mesh"][i])]
        X, Y, _, flag = render_ref.project(verts, c["inst_pose"][i], c["camk"][scene], c["near"])
        faces = np.asarray(faces, dtype=np.int64)
        x, y = X[faces], Y[faces]
        x0, x1 = np.maximum(-((-x.min(1)) // 256), 0), np.minimum(x.max(1) // 256, c["W"] - 1)
        y0, y1 = np.maximum(-((-y.min(1)) // 256), 0), np.minimum(y.max(1) // 256, c["H"] - 1)
        area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        meets = (flag[faces] == 0).all(1) & (area != 0) & (x0 <= x1) & (y0 <= y1) & (x0 <= tx0 + 15) & (x1 >= tx0) & (y0 <= ty0 + 15) & (y1 >= ty0)
        swept = []
        for base in range(0, len(faces), RASTER_THREADS):
            n += int(meets[base:base + RASTER_THREADS].sum())
            assert n <= RASTER_CAP
            if n > RASTER_CAP - RASTER_THREADS:
                swept.append(n)
                n = 0
        held.append((n, swept))
    return held


def slot_carry():
    """32 x 32, one scene of two instances of 200 small triangles each, every one in the tile at the origin: triangle k covers the one
    sample (1 + k % 14, 1 + k // 14 % 14) and lies at z = 1 m where k + slot is even, at 1.05 m where it is odd, so each instance
    wins every other column of the 14 x 14 block.  The tile's record list holds 200 records after the first slot -- below the sweep's
    threshold of 256 -- carries them into the second slot, holds 400 after that slot's only chunk and is swept there, inside the
    walk: asserted here, so that the case cannot stop crossing the threshold with records of both slots in the list."""
    f = 64.0
    meshes = []
    for slot in range(2):
        v = []
        for k in range(200):
            cx, cy, z = 1 + k % 14, 1 + k // 14 % 14, 1.0 + 0.05 * ((k + slot) % 2)
            v += [((cx - 0.6) * z / f, (cy - 0.6) * z / f, z), ((cx + 0.8) * z / f, (cy - 0.6) * z / f, z), ((cx - 0.6) * z / f, (cy + 0.8) * z / f, z)]
        meshes.append((np.asarray(v, dtype=np.float32), np.arange(600, dtype=np.int32).reshape(200, 3)))
    c = case(meshes, [[(0, CARRY_IDS[0], I3, Z3, 1.0), (1, CARRY_IDS[1], I3, Z3, 1.0)]], camk=(f, f, 0.0, 0.0), h=32, w=32)
    assert tile_walk(c) == [(200, []), (0, [400])]
    assert all(tile_walk(c, tile=t) == [(0, []), (0, [])] for t in ((1, 0), (0, 1), (1, 1)))
    return c


@functools.lru_cache(maxsize=None)
def _reference(name, arg):
    c = BUILDERS[name]() if arg is None else BUILDERS[name](arg)
    ref = render_ref.render(c["meshes"], c["scene_ptr"], c["inst_mesh"], c["inst_id"], c["inst_pose"], c["camk"], c["H"], c["W"], c["near"])
    for v in ref.values():
        v.setflags(write=False)
    return c, ref


def reference(name, arg=None):
    """(case, restatement's outputs) of a named case; computed once, read-only"""
    return _reference(name, arg)


BUILDERS = dict(rectangle=rectangle, slanted_plane=slanted_plane, cube=cube, rules=rules, tails=tails, tiny_triangles=tiny_triangles,
                three_scenes=three_scenes, slot_carry=slot_carry)
