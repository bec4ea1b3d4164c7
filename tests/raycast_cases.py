"""The cases of tests/test_raycast_cpu.py and tests/test_raycast_gpu.py (DESIGN.md section 3 "Ray casting and frame-to-model
tracking"): ray-cast calls on the analytic sphere and on hand-built plane volumes, one per rule, with the restatement's outputs
computed once and shared; the fused bottle of the accuracy test; and the smooth sequence scan_track is tested on."""
import functools

import numpy as np

from tests import raycast_ref as rr
from tests import tsdf_cases as tc
from tests import tsdf_ref as tr
from tests.render_ref import pose34

F = np.float32


def call(vsum, weight, meta, camk, job_img, job_model, job_pose, window, h, w, **kw):
    """one ray-cast call as a dict; vsum, weight (M,G,G,G), meta (M,4)"""
    job_pose = np.asarray(job_pose, dtype=F).reshape(-1, 3, 4)
    return dict(vsum=np.ascontiguousarray(vsum, dtype=np.int32), weight=np.ascontiguousarray(weight, dtype=np.int32),
                meta=np.ascontiguousarray(meta, dtype=F), camk=np.ascontiguousarray(camk, dtype=F).reshape(-1, 4),
                job_img=np.asarray(job_img, dtype=np.int32), job_model=np.asarray(job_model, dtype=np.int32), job_pose=job_pose,
                job_inv=rr.inverse_pose(job_pose), window=np.ascontiguousarray(window, dtype=F).reshape(-1, 4), h=h, w=w, kw=kw)


def run(c):
    """the restatement on a call"""
    return rr.raycast(c["vsum"], c["weight"], c["meta"], c["camk"], c["job_img"], c["job_model"], c["job_inv"], c["window"], c["h"], c["w"],
                      **c["kw"])


# ---------------------------------------------------------------------------------------------------------------------- the sphere
SPHERE_R, SPHERE_H, SPHERE_W = 0.4, 33, 65
SPHERE_K = np.array([280.0, 280.0, 159.5, 119.5], dtype=F)
SPHERE_POSES = (((1, 0, 0), 0.0, (0.0, 0.0, 0.6), 0.2), ((1, 2, -1), 40.0, (0.03, -0.02, 0.55), 0.2), ((-2, 1, 3), 115.0, (-0.05, 0.04, 0.8), 0.25))


@functools.lru_cache(maxsize=None)
def sphere_call(G):
    """tsdf_cases.sphere(G) seen from three poses (rotation, offset, scale differ), a 33 x 65 grid over the cube's image each"""
    vsum, weight, meta = tc.sphere(G)
    poses = [pose34(tc.rodrigues(axis, deg), t, s) for axis, deg, t, s in SPHERE_POSES]
    wins = []
    for (_, _, t, s), p in zip(SPHERE_POSES, poses):
        r = 0.6 * s / t[2] * float(SPHERE_K[0])                   # a little more than the cube's half edge in pixels
        u, v = SPHERE_K[2] + SPHERE_K[0] * t[0] / t[2], SPHERE_K[3] + SPHERE_K[1] * t[1] / t[2]
        wins.append((u - r, v - r, 2 * r / (SPHERE_W - 1), 2 * r / (SPHERE_H - 1)))
    return call(vsum[None], weight[None], meta[None], SPHERE_K, [0, 0, 0], [0, 0, 0], poses, wins, SPHERE_H, SPHERE_W)


def sphere_analytic(c):
    """per job and ray, float64: the depth of the ray's first intersection with the sphere (NaN without one), the distance of the
    ray's line from the sphere's centre in voxels minus the radius in voxels (negative inside the silhouette), the outward normal
    at the intersection in the model frame"""
    J, h, w = len(c["job_img"]), c["h"], c["w"]
    K = c["camk"][0].astype(np.float64)
    z, gap, normal = np.zeros((J, h, w)), np.zeros((J, h, w)), np.zeros((J, h, w, 3))
    for j in range(J):
        T = c["job_pose"][j].astype(np.float64)
        s = np.cbrt(np.linalg.det(T[:, :3]))
        win = c["window"][j].astype(np.float64)
        u = win[0] + np.arange(w)[None, :] * win[2] + np.zeros((h, 1))
        v = win[1] + np.arange(h)[:, None] * win[3] + np.zeros((1, w))
        d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1)
        ctr, R = T[:, 3], s * SPHERE_R
        a, b = (d * d).sum(-1), d @ ctr
        disc = b * b - a * (ctr @ ctr - R * R)
        with np.errstate(invalid="ignore"):
            z[j] = np.where(disc >= 0, (b - np.sqrt(disc)) / a, np.nan)
        line = np.sqrt(np.maximum(ctr @ ctr - b * b / a, 0))
        gap[j] = (line - R) / (s * float(c["meta"][0, 3]))
        p = z[j][..., None] * d - ctr
        normal[j] = (p / R) @ (T[:, :3] / s)                       # R^T n: the camera-frame normal in the model frame
    return z, gap, normal


# ---------------------------------------------------------------------------------------------------------------------- the rules
RULE_G = 16
RULE_K = np.array([[128, 128, 32, 24]], dtype=F)
RULE_VOXEL = 1.0 / 64


def plane(S, G=RULE_G, weight=1):
    """f(ix, iy, iz) = 256 (S - iz): the surface is the plane at voxel coordinate z = S, outside (positive) towards smaller z"""
    iz = np.arange(G, dtype=np.float64)
    w = np.full((G, G, G), weight, np.int32)
    vsum = (np.rint(256 * (S - iz)).astype(np.int32) * weight)[None, None, :] * np.ones((G, G, 1), np.int32)
    return vsum, w


def eye(*t):
    return pose34(np.eye(3), t)


AXIS = (32.0, 24.0, 1.0, 1.0)                                       # a window whose ray (0, 0) is the optical axis


@functools.lru_cache(maxsize=None)
def rule_calls():
    """name -> call.  The camera of eye(0, 0, 1) sits 64 voxels in front of the cube's centre plane and looks along +z of a cube of
    voxel 1/64 about the origin: the axis ray is g_z(z) = 64 z - 56.5, it enters at z = 0.8828125 and its samples sit at g_z = 0, 1,
    2, ... exactly."""
    meta = np.array([[0, 0, 0, RULE_VOXEL]], dtype=F)
    p75, p8 = plane(7.5), plane(8.0)
    one = lambda vol, pose=eye(0, 0, 1), win=AXIS, h=1, w=1, **kw: call(vol[0][None], vol[1][None], meta, RULE_K, [0], [0], [pose], [win], h, w, **kw)
    out = {}
    out["plane"] = one(p75)                                         # a hit at g_z = 7.5: z = 1, vertex (0, 0, 0), normal (0, 0, -1)
    out["boundary"] = one(p8)                                       # f = 0 at the sample g_z = 8 itself: z = 1.0078125 on the cell's face
    out["misses_cube"] = one(p75, win=(200.0, 24.0, 1.0, 1.0))
    out["inside"] = one(p75, pose=eye(0, 0, -0.02))                 # the camera sits at g_z = 8.78: the first known sample is negative
    layer = (p75[0] * 2, np.where(np.arange(RULE_G)[None, None, :] == 8, 1, 2).astype(np.int32) * np.ones((RULE_G, RULE_G, 1), np.int32))
    layer[0][:, :, 8] //= 2
    out["unknown_layer"] = one(layer, min_weight=2)                 # the cells at g_z = 7 and 8 are unknown: the sample at 9 has no past
    out["unknown_layer_low"] = one(layer, min_weight=1)             # ... and with every voxel known the plane's hit
    behind = pose34(tc.rodrigues((0, 1, 0), 180.0), (0, 0, 1))
    out["from_behind"] = one(p75, pose=behind)                      # enters at g_z = 15: negative first
    far_unknown = (p75[0], np.where(np.arange(RULE_G)[None, None, :] >= 12, 0, 1).astype(np.int32) * np.ones((RULE_G, RULE_G, 1), np.int32))
    out["exit"] = one(far_unknown, pose=behind)                     # unknown, then negative, then the - -> + change: a miss
    out["near_cuts"] = one(p75, near=0.95)                          # the march starts at g_z = 4.3: a hit at z = 1 all the same
    out["near_beyond"] = one(p75, near=1.05)                        # the march starts behind the surface
    bad = []
    for where, value in (((0, 0), np.nan), ((2, 3), np.nan), ((1, 1), np.inf), ((2, 3), np.inf), ((0, 3), -np.inf)):
        p = eye(0, 0, 1)
        p[where] = value
        bad.append(p)
    out["bad_pose"] = call(p75[0][None], p75[1][None], meta, RULE_K, [0] * 5, [0] * 5, bad, [AXIS] * 5, 1, 1)
    wins = [(np.nan, 24, 1, 1), (32, np.nan, 1, 1), (32, 24, np.nan, 1), (np.inf, 24, 1, 1), (32, -np.inf, 1, 1), (32, 24, 1, np.inf)]
    out["bad_window"] = call(p75[0][None], p75[1][None], meta, RULE_K, [0] * 6, [0] * 6, [eye(0, 0, 1)] * 6, wins, 2, 2)
    out["bad_index"] = call(p75[0][None], p75[1][None], meta, RULE_K, [0, 0, -1, 1, 0], [-1, 1, 0, 0, 0], [eye(0, 0, 1)] * 5, [AXIS] * 5, 1, 1)
    out["far"] = one(p75, pose=eye(0, 0, 70))                       # z = 70 m: kept in z, 0 in the 16-bit depth
    meta2 = np.array([[0, 0, 0, RULE_VOXEL], [0.01, -0.02, 0.03, 1.0 / 32]], dtype=F)
    vols = (np.stack([p75[0], p8[0]]), np.stack([p75[1], p8[1]]))
    for h, w in ((1, 1), (5, 7), (33, 65)):
        win = (32.0 - 24.0, 24.0 - 20.0, 48.0 / max(w - 1, 1), 40.0 / max(h - 1, 1)) if h > 1 else AXIS   # wider than the cube's image
        out["grid_%dx%d" % (h, w)] = call(vols[0], vols[1], meta2, RULE_K, [0, 0, 0], [0, 1, 0],
                                          [eye(0, 0, 1), eye(0.01, 0.02, 1.5), pose34(tc.rodrigues((1, 1, 0), 20.0), (0, 0, 1))], [win] * 3, h, w)
    for c in out.values():
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's outputs of rule_calls()[name] or of sphere16 / sphere24, computed once and shared (do not write to them)"""
    c = sphere_call(int(name[6:])) if name.startswith("sphere") else rule_calls()[name]
    out = run(c)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the fused object
QUALITY_G, QUALITY_H, QUALITY_W = 32, 120, 160
QUALITY_K = np.array([140, 140, 79.5, 59.5], dtype=F)


@functools.lru_cache(maxsize=None)
def fused_bottle():
    """tests/test_tsdf_cpu.py's case: the bottle rendered by tests/render_ref.py at 160 x 120 from the 12 turntable poses and fused by
    tests/tsdf_ref.py at G = 32 with a truncation of two voxels -> (verts, faces, meta, vsum, weight)"""
    from tests import render_ref
    v, f = tc.turntable_mesh()
    poses = [pose34(*tc.turntable_pose(k), s=tc.TURN_SCALE) for k in range(tc.TURN_FRAMES)]
    depth = np.stack([render_ref.render_scene([(v, f)], [(0, 1, p)], QUALITY_K, QUALITY_H, QUALITY_W)["depth"] for p in poses])
    meta = tr.tsdf_meta((v.max(0).astype(np.float64) + v.min(0)) / 2, v.max(0) - v.min(0), QUALITY_G)
    vsum, weight = np.zeros((1,) + (QUALITY_G,) * 3, np.int32), np.zeros((1,) + (QUALITY_G,) * 3, np.int32)
    tr.integrate(vsum, weight, meta[None], depth, np.tile(QUALITY_K, (len(poses), 1)), np.arange(len(poses)), np.zeros(len(poses), np.int64),
                 np.stack(poses), 2000.0 * float(meta[3]) * tc.TURN_SCALE)
    return v, f, meta, vsum, weight


# ---------------------------------------------------------------------------------------------------------------------- the sequence
SEQ_FRAMES, SEQ_STEP_DEG, SEQ_START_DEG = 24, 4.0, 30.0


def smooth_pose(k, scale=tc.TURN_SCALE, dist=tc.TURN_DIST):
    """view k of the smooth sequence: azimuth 30 + 4 k degrees about the model's y axis, elevation 25 + 5 sin(2 pi k / 24) degrees:
    (R, t) float64, model to camera, the model's y axis up (tsdf_cases.turntable_pose's frame).  The start is 30 degrees off the
    boxes' faces: seen face on (azimuth 0) a box shows two plane directions only, which leaves point-to-plane ICP a free slide, and
    the first frames, registered against a model made of one or two frames, must not be the degenerate ones."""
    el = 25.0 + 5.0 * np.sin(2 * np.pi * k / SEQ_FRAMES)
    flip = np.diag([1.0, -1.0, -1.0])
    return tc.rodrigues((1, 0, 0), el) @ flip @ tc.rodrigues((0, 1, 0), SEQ_START_DEG + SEQ_STEP_DEG * k), np.array([0.0, 0.0, dist])


def smooth_rts(n=SEQ_FRAMES):
    return np.stack([tc.pose44(*smooth_pose(k), tc.TURN_SCALE) for k in range(n)])
