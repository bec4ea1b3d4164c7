"""The cases of tests/test_icp_dense_cpu.py and tests/test_icp_dense_gpu.py (DESIGN.md section 3 "Dense projective registration"):
icp_dense calls on hand-built plane volumes, one per rule, and on the fused two-box object of the accuracy test, with the
restatement's results computed once and shared.

A case is a dict: depth (S,H,W) uint16, camk (S,4), mask (S,H,W) uint8 or None, job_mask_val (J) uint8 or None, z (J,h,w), vertex,
normal (J,h,w,3), window (J,4), ref (J,3,4), job_img (J), rect (J,4), stride, R (J,3,3), t (J,3), s (J), max_dist (J), kw (iters,
tolerances, min_inliers).  Every frame is the volume itself ray-cast over the full frame at the TRUE pose (raycast_ref.raycast with
window (0, 0, 1, 1), its 16-bit depth); the maps are cast at the START pose."""
import functools

import numpy as np

from tests import icp_dense_ref as dr
from tests import icp_ref
from tests import raycast_cases as rc
from tests import raycast_ref as rr
from tests import tsdf_cases as tc
from tests import tsdf_ref as tr
from tests.render_ref import pose34

F = np.float32
FULL = (0.0, 0.0, 1.0, 1.0)


def cast(vsum, weight, meta, camk, pose, window, h, w):
    """one volume from one pose -> raycast_ref's dict of a single job"""
    pose = np.asarray(pose, F).reshape(1, 3, 4)
    return rr.raycast(vsum[None], weight[None], np.asarray(meta, F)[None], np.asarray(camk, F)[None], [0], [0], rr.inverse_pose(pose),
                      np.asarray(window, F)[None], h, w)


def job(frame, camk, maps, window, ref, rect, R, t, s, max_dist, img=0):
    return dict(frame=frame, camk=np.asarray(camk, F), z=maps["z"][0], vertex=maps["vertex"][0], normal=maps["normal"][0],
                window=np.asarray(window, F), ref=np.asarray(ref, F).reshape(3, 4), rect=np.asarray(rect, np.int32), R=np.asarray(R, F),
                t=np.asarray(t, F), s=F(s), max_dist=F(max_dist), img=img)


def call(jobs, stride=1, mask=None, mask_val=None, frames=None, camk=None, **kw):
    """J jobs of equal map size as one call; frames / camk: the call's (S,H,W) and (S,4) when the jobs' ``img`` index them (default:
    the first job's frame as the only one)"""
    depth = np.stack(frames) if frames is not None else jobs[0]["frame"][None]
    camk = np.stack(camk) if camk is not None else jobs[0]["camk"][None]
    c = dict(depth=np.ascontiguousarray(depth, np.uint16), camk=np.ascontiguousarray(camk, F), mask=mask,
             job_mask_val=None if mask is None else np.full(len(jobs), mask_val, np.uint8), stride=stride, kw=kw,
             job_img=np.array([j["img"] for j in jobs], np.int32))
    for k in ("z", "vertex", "normal", "window", "ref", "rect", "R", "t", "s", "max_dist"):
        c[k] = np.ascontiguousarray(np.stack([j[k] for j in jobs]))
    return c


def run(c):
    """the restatement on every job of a call -> list of its dicts; a job whose job_img is out of range is status 3 by the rule"""
    out = []
    S = len(c["depth"])
    for j in range(len(c["job_img"])):
        img = int(c["job_img"][j])
        if not 0 <= img < S:
            out.append(dict(R=c["R"][j], t=c["t"][j], s=c["s"][j], R64=c["R"][j].astype(np.float64), t64=c["t"][j].astype(np.float64),
                            status=3, inliers=0, iters=0, candidates=0, rmse=F(np.nan), corr=np.zeros(0, np.int32)))
            continue
        maps = dict(z=c["z"][j], vertex=c["vertex"][j], normal=c["normal"][j])
        out.append(dr.refine(c["depth"][img], c["camk"][img], maps, c["window"][j], c["ref"][j], c["rect"][j], c["R"][j], c["t"][j], c["s"][j],
                             c["max_dist"][j], stride=c["stride"], mask=None if c["mask"] is None else c["mask"][img],
                             mask_val=None if c["mask"] is None else c["job_mask_val"][j], **c["kw"]))
    return out


def pixels(c, j):
    """how many source pixels job j of a call has"""
    return len(dr.grid(c["rect"][j], c["stride"], *c["depth"].shape[1:])[0])


# ---------------------------------------------------------------------------------------------------------------------- the rules
RULE_H, RULE_W = 48, 64
RULE_META = np.array([0, 0, 0, rc.RULE_VOXEL], dtype=F)
TRUE = (np.eye(3), np.array([0.0, 0.0, 1.0]), 1.0)                 # raycast_cases' camera: the plane z = 7.5 voxels lies at depth 1 m
WHOLE = (0, 0, RULE_W - 1, RULE_H - 1)


def off(deg=0.4, dz=0.003):
    """a start a little off the truth in the directions a plane holds: a tilt about (1, 2, 0) and a shift along z"""
    return icp_ref.rot([1, 2, 0], deg) @ TRUE[0], TRUE[1] + np.array([0.0, 0.0, dz]), 1.0


@functools.lru_cache(maxsize=None)
def rule_calls():
    """name -> call, on raycast_cases.plane(7.5) at G = 16 seen by raycast_cases.RULE_K in a 48 x 64 frame: the cube's image is about
    32 pixels a side, every hit is at 1000 mm exactly.  A plane holds three of the six freedoms; the rows of the other three are exact
    zeros (the normals are (0, 0, -1) and never mix), so the damped system solves them to an exact 0."""
    vsum, weight = rc.plane(7.5)
    K = rc.RULE_K[0]
    frame = cast(vsum, weight, RULE_META, K, pose34(*TRUE[:2], TRUE[2]), FULL, RULE_H, RULE_W)["depth"][0]
    assert (frame > 0).sum() > 800 and set(np.unique(frame)) == {0, 1000}

    def one(start=TRUE, window=FULL, h=RULE_H, w=RULE_W, rect=WHOLE, ref=None, gate=0.02, frame=frame, img=0, over_window=None):
        """over_window: the window the call is GIVEN, where it is not the one the maps were cast from"""
        R, t, s = start
        P = pose34(R, t, s)
        maps = cast(vsum, weight, RULE_META, K, P, window, h, w)
        return job(frame, K, maps, window if over_window is None else over_window, P if ref is None else ref, rect, R, t, s, gate, img)
    out = {}
    out["exact"] = call([one()])                                     # start = truth: every hit pixel meets its own cell
    out["shifted"] = call([one(off())], iters=20)
    out["rect_partly_outside"] = call([one(off(), rect=(-5, -7, 40, 30))], iters=20)
    out["rect_outside"] = call([one(rect=(70, 5, 90, 20)), one(rect=(-20, -20, -3, -3)), one(rect=(5, 48, 20, 60))])
    out["rect_empty"] = call([one(rect=(0, 0, -1, -1)), one(rect=(40, 30, 20, 10))])
    out["stride2"] = call([one(off(), rect=(-5, -7, 60, 45))], stride=2, iters=20)
    out["stride3"] = call([one(off(), rect=(1, 2, 63, 47))], stride=3, iters=20)
    out["zero_frame"] = call([one(frame=np.zeros_like(frame))])
    half = (np.where(np.arange(RULE_W)[None, :] % 2 == 0, 7, 9) * np.ones((RULE_H, 1), np.int64)).astype(np.uint8)
    out["mask_half"] = call([one(off())], mask=half[None], mask_val=7, iters=20)
    nan = np.nan
    out["nan_window"] = call([one(window=np.array([nan, nan, nan, nan], F)),         # tsdf_windows' empty window: maps without a hit
                              one(over_window=np.array([0, nan, 1, 1], F)), one(over_window=np.array([0, 0, 0, 1], F))])   # good maps, du = 0
    bad = []
    for what, where, value in (("R", (0, 0), nan), ("R", (1, 2), np.inf), ("t", (2,), nan), ("t", (0,), np.inf), ("t", (2,), -np.inf),
                               ("s", (), nan), ("s", (), np.inf), ("s", (), 0.0)):
        j = one()
        a = np.array(j[what], F)
        a[where] = value
        j[what] = a if what != "s" else F(a)
        bad.append(j)
    out["bad_pose"] = call(bad)
    out["bad_img"] = call([one(img=-1), one(img=1), one()])
    out["map_1x1"] = call([one(window=rc.AXIS, h=1, w=1)])
    flipped = np.array([[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, -1]], F)       # c_z = -q_z - 1 < 0 with the same u, v
    out["behind_ref"] = call([one(ref=flipped)])
    out["one_iteration"] = call([one(off())], iters=1, tol_rot=0.0, tol_trans=0.0)
    out["five_pixels"] = call([one(rect=(30, 24, 34, 24))], min_inliers=0)
    out["six_by_eight"] = call([one(off(), rect=(28, 20, 35, 26))], iters=20)   # 56 pixels: a single partial wave
    # three jobs of one call: two frames with their own intrinsics, two volumes, three rectangles
    v8, w8 = rc.plane(8.0)
    meta2 = np.array([0.01, -0.02, 0.03, 1.0 / 32], dtype=F)
    K2 = np.array([100, 110, 30, 20], F)
    true2 = (tc.rodrigues((1, 1, 0), 10.0), np.array([0.01, 0.02, 1.5]), 1.0)
    frame2 = cast(v8, w8, meta2, K2, pose34(*true2[:2], true2[2]), FULL, RULE_H, RULE_W)["depth"][0]
    assert (frame2 > 0).sum() > 800
    start2 = (icp_ref.rot([2, -1, 0], 0.5) @ true2[0], true2[1] + np.array([0.0, 0.0, -0.004]), 1.0)
    P2 = pose34(*start2[:2], start2[2])
    win2 = rr.windows(meta2[None], 16, K2[None], [0], [0], P2[None], 20, 28, RULE_H, RULE_W)[0]
    j2 = job(frame2, K2, cast(v8, w8, meta2, K2, P2, win2, 20, 28), win2, P2, dr.rects(win2[None], 20, 28, RULE_H, RULE_W)[0], *start2, 0.03, 1)
    win0 = rr.windows(RULE_META[None], 16, K[None], [0], [0], pose34(*off()[:2], 1.0)[None], 20, 28, RULE_H, RULE_W)[0]
    out["three_jobs"] = call([one(off(), window=win0, h=20, w=28, rect=(10, 3, 50, 40)), j2, one(off(0.2, -0.002), window=win0, h=20, w=28, rect=(0, 0, 37, 47))],
                             frames=[frame, frame2], camk=[K, K2], iters=20)
    for c in out.values():
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the object
OBJ_G, OBJ_H, OBJ_W, OBJ_MAP_H, OBJ_MAP_W, OBJ_GATE = 32, 120, 160, 60, 80, 0.02


@functools.lru_cache(maxsize=None)
def fused_two_boxes():
    """icp_ref.two_boxes (no symmetry: a surface of revolution would leave an angle free) rendered by tests/render_ref.py at 160 x 120
    from the 12 turntable poses and fused by tests/tsdf_ref.py at G = 32 with a truncation of two voxels, the way
    raycast_cases.fused_bottle is built -> (verts, faces, meta, vsum, weight)"""
    from tests import render_ref
    v, f = icp_ref.two_boxes()
    poses = [pose34(*tc.turntable_pose(k), s=tc.TURN_SCALE) for k in range(tc.TURN_FRAMES)]
    depth = np.stack([render_ref.render_scene([(v, f)], [(0, 1, p)], rc.QUALITY_K, OBJ_H, OBJ_W)["depth"] for p in poses])
    meta = tr.tsdf_meta((v.max(0).astype(np.float64) + v.min(0)) / 2, v.max(0) - v.min(0), OBJ_G)
    vsum, weight = np.zeros((1,) + (OBJ_G,) * 3, np.int32), np.zeros((1,) + (OBJ_G,) * 3, np.int32)
    tr.integrate(vsum, weight, meta[None], depth, np.tile(rc.QUALITY_K, (len(poses), 1)), np.arange(len(poses)), np.zeros(len(poses), np.int64),
                 np.stack(poses), 2000.0 * float(meta[3]) * tc.TURN_SCALE)
    return v, f, meta, vsum, weight


@functools.lru_cache(maxsize=None)
def object_case():
    """the accuracy case: the fused two boxes seen from a held-out pose (half a step between two of the turntable's), the start 5
    degrees and 10 mm off it as tests/test_raycast_gpu.py test_raycast_model_serves_icp starts -> (call, truth (R, t), sparse: the
    40 x 48 maps packed into a model and a 1024-point sample of the frame for icp_ref.refine)"""
    v, f, meta, vsum, weight = fused_two_boxes()
    K, s = rc.QUALITY_K, tc.TURN_SCALE
    R_true, t_true = tc.turntable_pose(2, offset=0.5)
    frame = cast(vsum[0], weight[0], meta, K, pose34(R_true, t_true, s), FULL, OBJ_H, OBJ_W)["depth"][0]
    R0, t0 = icp_ref.rot([1, 2, -1], 5.0) @ R_true, t_true + 0.010 * np.array([2.0, -1.0, 2.0]) / 3.0
    P = pose34(R0, t0, s)
    win = rr.windows(meta[None], OBJ_G, K[None], [0], [0], P[None], OBJ_MAP_H, OBJ_MAP_W, OBJ_H, OBJ_W)[0]
    maps = cast(vsum[0], weight[0], meta, K, P, win, OBJ_MAP_H, OBJ_MAP_W)
    c = call([job(frame, K, maps, win, P, dr.rects(win[None], OBJ_MAP_H, OBJ_MAP_W, OBJ_H, OBJ_W)[0], R0, t0, s, OBJ_GATE)], iters=50)
    wins = rr.windows(meta[None], OBJ_G, K[None], [0], [0], P[None], 40, 48, OBJ_H, OBJ_W)[0]
    model, count = rr.pack(cast(vsum[0], weight[0], meta, K, P, wins, 40, 48))
    ys, xs = np.nonzero(frame)
    keep = np.linspace(0, len(xs) - 1, 1024).astype(np.int64)
    from tests import ball_ref
    cloud = ball_ref.pixel_points(xs[keep], ys[keep], frame[ys[keep], xs[keep]], K)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, (R_true, t_true), dict(model=model[0, :int(count[0])], cloud=cloud, R=R0.astype(F), t=t0.astype(F), s=F(s), hits=int(count[0]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's results of rule_calls()[name] or of 'object', computed once and shared (do not write to them)"""
    return run(object_case()[0] if name == "object" else rule_calls()[name])
