"""The BOP pose-error test cases, shared by tests/test_bop_cpu.py (the restatement against closed forms), tests/test_bop_gpu.py (the
kernels against the restatement) and tests/test_bop_track_gpu.py.  A point case is a dict of bop_ref.pose_errors' arguments, a VSD
case one of bop_ref.pose_vsd's; ``reference`` runs the restatement once per process.  The VSD geometry is tests/render_cases.py's
and tests/verify_cases.py's."""
import functools

import numpy as np

from tests import plane_cases as pc
from tests import render_cases as rc
from tests import render_ref
from tests import verify_cases as vc
from tests import bop_ref

F = np.float32
CAMK = np.asarray(rc.CAMK, dtype=F)
STEP = 2.0 ** -6                                   # the translation of the closed forms, metres: exact in every format
SIZES = (1, 63, 64, 65, 257, 2500, 8300)           # vertices: one; around a wave; above a workgroup; above the LDS tile of 1024
                                                   # points (three tiles, the last partial); more than 256 points per workgroup
                                                   # slice (8300 / 32 = 260: two rounds)


def points(n, seed):
    """n random vertices in the cube of edge 1 about the origin, as a mesh of one degenerate face (the point errors read no face)"""
    v = np.random.RandomState(seed).uniform(-0.5, 0.5, (n, 3)).astype(F)
    return v, np.zeros((1, 3), dtype=np.int32)


def turn_z(k, n):
    """[R | 0] of k turns of 2 pi / n about z; exact for n = 1, 2, 4"""
    exact = {(0, 1): (1, 0), (0, 2): (1, 0), (1, 2): (-1, 0), (0, 4): (1, 0), (1, 4): (0, 1), (2, 4): (-1, 0), (3, 4): (0, -1)}
    c, s = exact.get((k, n), (np.cos(2 * np.pi * k / n), np.sin(2 * np.pi * k / n)))
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0]], dtype=np.float64)


def group_z(n):
    return np.stack([turn_z(k, n) for k in range(n)]).astype(F)


@functools.lru_cache(maxsize=None)
def groups():
    """groups of 1, 2, 4 and 315 transforms about z (the last is bop.symmetry_transformations at BOP's step 0.01); 4: eight turns about
    z, one of them with a translation; 5: (identity, half turn) three times over -- equal values at indices two workgroups hold"""
    from tgpose_amd.evaluation import bop
    cont = bop.symmetry_transformations(dict(symmetries_continuous=[dict(axis=[0, 0, 1], offset=[0, 0, 0])]), 0.01)
    assert len(cont) == 315
    eight = group_z(8)
    eight[PUSH, 2, 3] = -1.0                       # S_5 also moves the model one unit down its z: under pushed()'s poses, behind the camera
    return [group_z(1), group_z(2), group_z(4), cont.astype(F), eight, np.concatenate([group_z(2)] * 3)]


PUSH = 5                                            # the transform of group 4 that pushed() relies on: wave 1 of workgroup b = 1


@functools.lru_cache(maxsize=None)
def meshes():
    from tgpose_amd.datasets import shapes
    two = (np.array([[-0.25, 0, 0], [0.25, 0, 0]], dtype=F), np.zeros((1, 3), dtype=np.int32))
    return [points(n, 100 + n) for n in SIZES] + [shapes.box(1.0), shapes.plane(0.5, 0.5, 3, 3), two]


CUBE, PLANE, TWO = len(SIZES), len(SIZES) + 1, len(SIZES) + 2      # mesh indices: a cube, 16 points in the plane z = 0, two points


def pose(axis_deg, t, s=1.0):
    R = np.eye(3)
    for axis, deg in axis_deg:
        R = R @ rc.rot(axis, deg)
    return render_ref.pose34(R, t, s)


def pcase(jobs, near=0.01, camk=CAMK):
    """jobs: list of (mesh, group, pose_est (3,4), pose_gt (3,4)) -> bop_ref.pose_errors' keyword arguments"""
    return dict(meshes=meshes(), groups=groups(), job_mesh=np.asarray([j[0] for j in jobs], np.int32), job_sym=np.asarray([j[1] for j in jobs], np.int32),
                pose_est=np.stack([j[2] for j in jobs]).astype(F), pose_gt=np.stack([j[3] for j in jobs]).astype(F),
                camk=np.ascontiguousarray(np.broadcast_to(np.asarray(camk, F), (len(jobs), 4))), near=near)


GT = pose([("z", 25), ("x", 35)], (0.02, -0.01, 0.9), 0.2)
EST = pose([("z", 27), ("x", 33), ("y", 3)], (0.025, -0.012, 0.91), 0.2)


def sizes():
    """one job per vertex count of SIZES, the groups of 1, 2, 4, 315, 1, 2 and 4 transforms"""
    return pcase([(i, i % 4, EST, GT) for i in range(len(SIZES))])


def single():
    """J = 1: 257 vertices against the group of 315 -- more symmetries than the 128 waves a job gets, and no multiple of them"""
    return pcase([(4, 3, EST, GT)])


def mixed():
    """J = 7: mixed meshes and groups, job 2 with a mesh index out of range, job 4 with a group index out of range, job 5 with
    ground-truth points behind the camera (bit 2), each job with its own intrinsics"""
    behind = pose([("x", 10)], (0.0, 0.0, 0.05), 0.2)
    jobs = [(3, 3, EST, GT), (CUBE, 2, EST, GT), (len(meshes()), 0, EST, GT), (1, 1, GT, EST), (2, -1, EST, GT), (4, 2, EST, behind), (5, 0, GT, GT)]
    camk = np.stack([CAMK * F(1 + 0.125 * j) for j in range(len(jobs))])
    return pcase(jobs, camk=camk)


def cube():
    """the cube turned a quarter about z (the estimate's columns are the ground truth's, permuted: exact) with the identity group and
    with the 4-fold group: mssd > 0 and mssd = 0 at sym_best = 1"""
    gt = pose([("x", 20), ("y", 30)], (0.01, 0.02, 0.8), 0.25)
    est = gt.copy()
    est[:, 0], est[:, 1] = gt[:, 1], -gt[:, 0]                                    # G Rz(90): x -> y, y -> -x
    return pcase([(CUBE, 0, est, gt), (CUBE, 2, est, gt)])


def translated(mesh=3, z=1.0):
    """R = I and the estimate STEP further along x, against the 4-fold group: the identity is the best symmetry by a wide margin"""
    gt = render_ref.pose34(np.eye(3), (0.0, 0.0, z))
    est = gt.copy()
    est[0, 3] += F(STEP)
    return pcase([(mesh, 2, est, gt)])


def planar():
    """the 16 points of a plane at constant z = 2 m, R = I, the estimate STEP further along x: mspd = fx STEP / z"""
    return translated(PLANE, 2.0)


def swapped():
    """two points, the estimate the ground truth turned half about z: each lands on the other, adi = 0 with add > 0"""
    gt = pose([("x", 20), ("y", 30)], (0.01, 0.02, 0.8), 0.5)
    est = gt.copy()
    est[:, 0], est[:, 1] = -gt[:, 0], -gt[:, 1]
    return pcase([(TWO, 0, est, gt)])


HIGH = (200, 314, 130)                              # symmetries of the 315: second round, workgroup 18; third round, the tail 256 ..
                                                    # 314, workgroup 14; second round, workgroup 0
OFFSET = 2.0 ** -10                                 # metres


def high_sym():
    """the estimate is the ground truth composed with element q of the group of 315, then OFFSET further along x, for q in HIGH:
    S_q is the best symmetry for mssd and for mspd, by a margin the CPU test asserts -- found only by a kernel that runs every round
    of its symmetry loop, the tail included, and joins every workgroup's slot"""
    jobs = []
    for q, mesh in zip(HIGH, (4, 3, 2)):
        est = GT.astype(np.float64)
        est[:, :3] = est[:, :3] @ groups()[3][q, :, :3].astype(np.float64)
        est[0, 3] += OFFSET
        jobs.append((mesh, 3, est.astype(F), GT))
    return pcase(jobs)


def pushed():
    """R = I, t = (0, 0, 1): every E p and every G S p is in front of the camera except under transform PUSH of group 4, which only
    wave 1 of workgroup 1 sees: bit 2 has to come out of that workgroup's slot"""
    gt = render_ref.pose34(np.eye(3), (0.0, 0.0, 1.0))
    return pcase([(3, 4, moved(gt, dx=STEP), gt)])


def tied():
    """the estimate is the ground truth turned half about z, exactly; group 5 holds that half turn at 1, 3 and 5 -- workgroup 0 and
    workgroup 1 -- with equal computed values: the lowest index wins"""
    gt = pose([("x", 20), ("y", 30)], (0.01, 0.02, 0.8), 0.5)
    est = gt.copy()
    est[:, 0], est[:, 1] = -gt[:, 0], -gt[:, 1]
    return pcase([(3, 5, est, gt)])


def nonfinite():
    """a NaN in the estimate, an infinity in the ground truth, a NaN in the intrinsics, and a sound job after them"""
    nan_est, inf_gt = EST.copy(), GT.copy()
    nan_est[1, 2], inf_gt[2, 3] = np.nan, np.inf
    c = pcase([(3, 2, nan_est, GT), (4, 3, EST, inf_gt), (2, 1, EST, GT), (2, 1, EST, GT)])
    c["camk"][2, 0] = np.nan
    return c


POINT_BUILDERS = dict(high_sym=high_sym, pushed=pushed, tied=tied, nonfinite=nonfinite, planar=planar, swapped=swapped, sizes=sizes, single=single, mixed=mixed, cube=cube, translated=translated)


@functools.lru_cache(maxsize=None)
def point_reference(name):
    """(case, restatement's outputs, (J,2) [L, z_min]) of a named point case; computed once"""
    c = POINT_BUILDERS[name]()
    ref = bop_ref.pose_errors(**c)
    scale = bop_ref.scale_L(c["meshes"], c["groups"], c["job_mesh"], c["job_sym"], c["pose_est"], c["pose_gt"], c["camk"])
    return c, ref, scale


def tolerances(c, scale):
    """(J,4): the derived bound of tests/test_bop_gpu.py per job and column -- 2^-40 L for the three distances in metres, times
    max(fx, fy) / z_min * (1 + L / z_min) for mspd"""
    L, zmin = scale[:, 0], scale[:, 1]
    base = 2.0 ** -40 * L
    with np.errstate(all="ignore"):
        px = base * c["camk"][:, :2].astype(np.float64).max(1) / zmin * (1.0 + L / zmin)
    return np.stack([base, base, base, px], 1)


# ---- VSD
DELTA = 15
TAUS = {1: (8,), 3: (-5, 0, 70000), 10: tuple(range(1, 11)), 16: tuple(range(1, 14)) + (20, 21, 25)}   # 3: outside [1, 65535]


def vcase(meshes_, depth, camk, jobs, taus, delta=DELTA, near=0.01):
    """jobs: list of (frame, mesh, pose_est, pose_gt) -> bop_ref.pose_vsd's keyword arguments; taus: one tuple for every job, or a
    (J, n_tau) array"""
    depth = np.ascontiguousarray(depth, dtype=np.uint16)
    camk = np.asarray(camk, dtype=F)
    camk = np.ascontiguousarray(np.broadcast_to(camk, (depth.shape[0], 4)) if camk.ndim == 1 else camk)
    taus = np.asarray(taus, dtype=np.int32)
    job_tau = np.ascontiguousarray(np.broadcast_to(taus, (len(jobs), taus.shape[-1])))
    return dict(meshes=meshes_, depth=depth, camk=camk, job_img=np.asarray([j[0] for j in jobs], np.int32),
                job_mesh=np.asarray([j[1] for j in jobs], np.int32), pose_est=np.stack([j[2] for j in jobs]).astype(F),
                pose_gt=np.stack([j[3] for j in jobs]).astype(F), job_tau=job_tau, delta=delta, near=near)


def moved(p, dx=0.0, dy=0.0, dz=0.0):
    q = np.array(p, dtype=F)
    q[:, 3] += np.asarray([dx, dy, dz], dtype=F)
    return q


RECT_JOBS = ("same", "plus_7", "plus_20", "right_3px", "est_off", "both_off", "zeroed_plus_20")
RECT_N, RECT_SHIFT = 31 * 15, 3                     # the rectangle covers x = 10 .. 40, y = 5 .. 19 at 1000 mm (render_cases.rectangle)


def rectangle(n_tau=10, split="diag02"):
    """render_cases.rectangle against its own depth (frame 0) and a zeroed frame (1): the estimate at the ground truth, 7 and 20 mm
    farther, 3 whole pixels to the right (3 / 128 m at z = 1 under RECT_K), off-screen, both off-screen, and 20 mm farther on the
    zeroed frame"""
    c, ref = rc.reference("rectangle", split)
    own, gt = ref["depth"][0], c["inst_pose"][0]
    off = moved(gt, dx=10.0)
    jobs = [(0, 0, gt, gt), (0, 0, moved(gt, dz=0.007), gt), (0, 0, moved(gt, dz=0.02), gt), (0, 0, moved(gt, dx=RECT_SHIFT / 128.0), gt),
            (0, 0, off, gt), (0, 0, off, off), (1, 0, moved(gt, dz=0.02), gt)]
    return vcase(c["meshes"], np.stack([own, np.zeros_like(own)]), c["camk"][0], jobs, TAUS[n_tau])


MM = (5, 10, 15, 20, 25, 30, 40, 50, 75, 100)


def tails():
    """verify_cases.tails at 123 x 157 (occluders, tile tails, a table larger than the image): each instance's pose as ground truth
    and estimate, then the sphere's estimate 20 mm nearer and 20 mm farther"""
    c, _ = vc.reference("tails")
    gt = c["job_pose"]
    jobs = [(0, int(c["job_mesh"][i]), gt[i], gt[i]) for i in range(3)] + [(0, 1, gt[3], gt[1]), (0, 1, gt[4], gt[1])]
    return vcase(c["meshes"], c["depth"], c["camk"], jobs, MM)


def rules():
    """verify_cases.rules: an estimate wholly off-screen against the front triangle; the near rule and the guard band in both
    dropped counts; the front triangle at 0.5 m before a frame at 1 m; a surface at 70 m, never rendered"""
    c, _ = vc.reference("rules")
    eye = c["job_pose"][1]
    return vcase(c["meshes"], c["depth"], c["camk"], [(0, int(m), p, eye) for m, p in zip(c["job_mesh"], c["job_pose"])], MM)


def tiny_triangles():
    """verify_cases.tiny_triangles (20 480 triangles in about one tile, the record list swept many times for both poses): the
    ground truth 3 mm farther than the estimate, the frame at the ground truth"""
    c, _ = vc.reference("tiny_triangles")
    return vcase(c["meshes"], c["depth"], c["camk"], [(0, 0, c["job_pose"][0], moved(c["job_pose"][0], dz=0.003))], MM)


def seven_jobs():
    """verify_cases.seven_jobs: S = 3 frames with their own intrinsics, two jobs sharing a frame and a mesh, the fourth job's
    estimate 15 mm nearer than its ground truth, a job against the empty frame 0, and job_img out of range; a tau row per job"""
    c, _ = vc.reference("seven_jobs")
    three, _ = rc.reference("three_scenes")
    gt = c["job_pose"].copy()
    gt[3] = three["inst_pose"][6]
    jobs = [(int(c["job_img"][j]), int(c["job_mesh"][j]), c["job_pose"][j], gt[j]) for j in range(7)]
    taus = np.asarray(MM, np.int32)[None, :] + np.arange(7, dtype=np.int32)[:, None]
    return vcase(c["meshes"], c["depth"], c["camk"], jobs, taus)


VSD_BUILDERS = dict(rectangle=rectangle, tails=tails, rules=rules, tiny_triangles=tiny_triangles, seven_jobs=seven_jobs)


@functools.lru_cache(maxsize=None)
def vsd_reference(name, *args):
    """(case, restatement's outputs) of a named VSD case; computed once, read-only"""
    c = VSD_BUILDERS[name](*args)
    ref = bop_ref.pose_vsd(**c)
    for v in ref.values():
        v.setflags(write=False)
    return c, ref


# ---- the tracked sequence: plane_cases' six frames, every object at its ground-truth pose
def track_gts():
    """(FRAMES, 3, 4, 4) float32: the ground-truth poses [s R | t] of the three objects of plane_cases' sequence"""
    out = np.zeros((pc.FRAMES, 3, 4, 4), dtype=F)
    for k in range(pc.FRAMES):
        for o in range(3):
            out[k, o, :3, :4] = vc.gt_pose34(k, o)
            out[k, o, 3, 3] = 1
    return out
