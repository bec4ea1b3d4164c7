"""The pose-verification test cases, shared by tests/test_verify_cpu.py (the restatement against closed forms),
tests/test_verify_gpu.py (the kernel against the restatement) and tests/test_track_verify_gpu.py.  A case is a dict of
verify_ref.verify's arguments; ``reference`` runs the restatement on it once per process.  The geometry is tests/render_cases.py's
and tests/plane_cases.py's; a frame is a depth image one of their scenes renders to, changed as the case says."""
import functools

import numpy as np

from tests import icp_ref
from tests import plane_cases as pc
from tests import render_cases as rc
from tests import render_ref
from tests import verify_ref as vr

TAU = 5


def case(meshes, depth, camk, jobs, tau=TAU, near=0.01, mask=None):
    """jobs: list of (frame, mesh, pose (3,4), mask byte) -> verify_ref.verify's keyword arguments, mask bytes only with a mask"""
    depth = np.ascontiguousarray(depth, dtype=np.uint16)
    camk = np.asarray(camk, dtype=np.float32)
    camk = np.ascontiguousarray(np.broadcast_to(camk, (depth.shape[0], 4)) if camk.ndim == 1 else camk)
    c = dict(meshes=meshes, depth=depth, camk=camk, job_img=np.asarray([j[0] for j in jobs], dtype=np.int32),
             job_mesh=np.asarray([j[1] for j in jobs], dtype=np.int32), job_pose=np.stack([j[2] for j in jobs]).astype(np.float32),
             tau=tau, near=near, mask=None, job_mask_val=None)
    if mask is not None:
        c.update(mask=np.ascontiguousarray(mask, dtype=np.uint8), job_mask_val=np.asarray([j[3] for j in jobs], dtype=np.uint8))
    return c


def shifted(depth, mm):
    """the frame with every valid pixel moved by mm millimetres"""
    return np.where(depth > 0, depth.astype(np.int64) + mm, 0).astype(np.uint16)


RECT_FRAMES = ("own", "plus_tau", "plus_tau_1", "minus_tau_1", "zeroed")
RECT_MASK_X = 25                                             # the half-frame mask: byte 7 left of this column, byte 9 from it on


def rectangle(split="diag02"):
    """render_cases.rectangle against five frames: its own rendered depth, that shifted by +tau, +tau+1 and -tau-1 mm, and zeros;
    one job per frame, all with the mask byte 7 of the left part of the frame"""
    c, ref = rc.reference("rectangle", split)
    own = ref["depth"][0]
    frames = np.stack([own, shifted(own, TAU), shifted(own, TAU + 1), shifted(own, -TAU - 1), np.zeros_like(own)])
    mask = np.full(frames.shape, 9, dtype=np.uint8)
    mask[:, :, :RECT_MASK_X] = 7
    return case(c["meshes"], frames, c["camk"][0], [(s, 0, c["inst_pose"][0], 7) for s in range(len(RECT_FRAMES))], mask=mask)


def tails():
    """render_cases.tails at 123 x 157 (tile tails, a table larger than the image): each of its three instances against the frame
    the whole scene renders to -- the table is occluded where the objects stand -- then the sphere moved 20 mm towards the camera
    (violations) and 20 mm away (occluded by the frame's own sphere); the mask is the rendered instance mask"""
    c, ref = rc.reference("tails")
    jobs = [(0, int(c["inst_mesh"][i]), c["inst_pose"][i], int(c["inst_id"][i])) for i in range(3)]
    for dz in (-0.02, 0.02):
        p = c["inst_pose"][1].copy()
        p[2, 3] += np.float32(dz)
        jobs.append((0, 1, p, 200))
    return case(c["meshes"], ref["depth"], c["camk"], jobs, mask=ref["mask"])


def rules():
    """render_cases.rules' meshes against a flat frame at 1 m: 0 a job wholly off-screen (zeros), 1 a vertex behind near (dropped,
    nothing rendered), 2 the guard band (dropped), 3 the front triangle at 0.5 m (all violations), 4 a surface at 70 m: over range,
    d_r = 0, all nodata"""
    c = rc.rules()
    frame = np.full((1, rc.H, rc.W), 1000, dtype=np.uint16)
    eye = c["inst_pose"][0]
    off = eye.copy()
    off[0, 3] = 10.0
    return case(c["meshes"], frame, rc.CAMK, [(0, 3, off, 0), (0, 0, eye, 0), (0, 1, eye, 0), (0, 3, eye, 0), (0, 5, eye, 0)])


def tiny_triangles():
    """render_cases.tiny_triangles (20 480 triangles in about one tile: the record list is swept many times) against its own depth
    3 mm further"""
    c, ref = rc.reference("tiny_triangles")
    return case(c["meshes"], shifted(ref["depth"], 3), c["camk"], [(0, 0, c["inst_pose"][0], 0)])


def seven_jobs():
    """J = 7 over the S = 3 frames of render_cases.three_scenes, each with its own intrinsics: four instances of frame 2 as rendered
    (0 and 4 share mesh 0), one of them 15 mm nearer, frame 1's sphere, a box against the empty frame 0, and a job whose job_img
    is out of range; the mask is the rendered instance mask"""
    c, ref = rc.reference("three_scenes")
    P, ids, mesh = c["inst_pose"], c["inst_id"], c["inst_mesh"]
    near5 = P[6].copy()
    near5[2, 3] -= np.float32(0.015)
    jobs = [(2, int(mesh[1]), P[1], int(ids[1])), (2, int(mesh[2]), P[2], int(ids[2])), (2, int(mesh[5]), P[5], int(ids[5])),
            (2, int(mesh[6]), near5, int(ids[6])), (1, int(mesh[0]), P[0], int(ids[0])), (0, int(mesh[1]), P[1], 0), (3, 0, P[1], 1)]
    assert mesh[1] == mesh[5] == 0
    return case(c["meshes"], ref["depth"], c["camk"], jobs, mask=ref["mask"])


BUILDERS = dict(rectangle=rectangle, tails=tails, rules=rules, tiny_triangles=tiny_triangles, seven_jobs=seven_jobs)


@functools.lru_cache(maxsize=None)
def reference(name, arg=None):
    """(case, restatement's outputs) of a named case; computed once, read-only"""
    c = BUILDERS[name]() if arg is None else BUILDERS[name](arg)
    ref = vr.verify(**c)
    for v in ref.values():
        v.setflags(write=False)
    return c, ref


def without_mask(c):
    return dict(c, mask=None, job_mask_val=None)


# ---- the vanished object: plane_cases' six frames (icp_ref.table_scene, 240 x 320, the objects standing on the table), object
# VANISHED absent from frame GONE_FROM on
VANISHED, GONE_FROM = 2, 3


def present(k, o):
    return o != VANISHED or k < GONE_FROM


@functools.lru_cache(maxsize=None)
def vanished_rendered(k):
    """frame k of the vanished-object sequence -> (depth (H,W) uint16, mask (H,W) uint8)"""
    sc = icp_ref.table_scene(k, objects=tuple(o for o in range(3) if present(k, o)))
    inst = [(i["mesh"], i["inst_id"], render_ref.pose34(i["R"], i["t"], i["s"])) for i in sc]
    r = render_ref.render_scene(pc.meshes(), inst, pc.CAMK, pc.H, pc.W)
    return r["depth"], r["mask"]


def gt_pose34(k, o, move=(0.0, 0.0, 0.0)):
    """the ground-truth pose of object o in frame k as the kernel reads it, moved by ``move`` metres in the camera's frame"""
    R, t, s = pc.gt_pose(k, o)
    return render_ref.pose34(R, t + np.asarray(move, np.float64), s)


@functools.lru_cache(maxsize=None)
def vanished_scores():
    """every object at its ground-truth pose in every frame of the vanished-object sequence -> score (FRAMES, 3) float32"""
    depth = np.stack([vanished_rendered(k)[0] for k in range(pc.FRAMES)])
    jobs = [(k, 0, gt_pose34(k, o), 0) for k in range(pc.FRAMES) for o in range(3)]
    out = vr.verify(**case(pc.meshes(), depth, pc.CAMK, jobs))
    return out["score"].reshape(pc.FRAMES, 3)


def separation():
    """(the least score over the present (frame, object) pairs, the greatest over the absent ones, their midpoint: the tracking
    test's min_score)"""
    s = vanished_scores()
    here = np.array([[present(k, o) for o in range(3)] for k in range(pc.FRAMES)])
    lo, hi = float(s[here].min()), float(s[~here].max())
    return lo, hi, 0.5 * (lo + hi)
