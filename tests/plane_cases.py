"""The scenes of the supporting-plane tests, on the CPU: icp_ref.table_scene rendered by tests/render_ref.py at 240 x 320 with the
objects standing ON the table (gap = 0), the table's plane as the scene's pose gives it, and the tracking simulation both
tests/test_plane_cpu.py and tests/test_track_plane_gpu.py rely on: per frame plane_ref.fit + plane_ref.cut, the ball crop and the
keyed draw of 512 points restated (tests/ball_ref.py), icp_ref.refine (point-to-plane, gate 1 cm) started from the previous pose."""
import functools

import numpy as np

from tests import ball_ref, icp_ref, mesh_sample_ref, plane_ref, render_ref

H, W, N_PTS, RATIO, GATE = 240, 320, 512, 0.5, 0.01
K = np.array([[288.8, 0, 159.5], [0, 288.8, 119.5], [0, 0, 1]], np.float32)
CAMK = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
FRAMES = 6
TOL, MARGIN, HYPOTHESES = 0.004, 0.006, 256
SEED = 5                     # the evaluater's seed in the tracking tests


def meshes():
    from tgpose_amd.datasets import shapes
    return [icp_ref.two_boxes(), shapes.plane(3.0, 3.0, 4, 4)]


@functools.lru_cache(maxsize=None)
def rendered(k, gap=0.0):
    """frame k of the sequence -> depth (H,W) uint16"""
    sc = icp_ref.table_scene(k, gap=gap)
    inst = [(i["mesh"], i["inst_id"], render_ref.pose34(i["R"], i["t"], i["s"])) for i in sc]
    return render_ref.render_scene(meshes(), inst, CAMK, H, W)["depth"]


def table_plane(k, gap=0.0):
    """(n (3,), d) float64 of the scene's table: the plane mesh's z = 0 under its pose, oriented to d >= 0"""
    tb = icp_ref.table_scene(k, gap=gap)[-1]
    n = np.asarray(tb["R"], np.float64)[:, 2]
    d = -float(n @ np.asarray(tb["t"], np.float64))
    return (-n, -d) if d < 0 else (n, d)


def plane_error(plane, k, gap=0.0):
    """(degrees between the normals, millimetres between the offsets) of a fitted plane against frame k's table"""
    n, d = table_plane(k, gap)
    p = np.asarray(plane, np.float64)
    c = float(np.clip(p[:3] @ n / np.linalg.norm(p[:3]), -1.0, 1.0))
    return np.rad2deg(np.arccos(c)), 1000.0 * abs(p[3] - d)


def gt_pose(k, o):
    ob = icp_ref.table_scene(k)[o]
    return np.asarray(ob["R"], np.float64), np.asarray(ob["t"], np.float64), float(ob["s"])


@functools.lru_cache(maxsize=None)
def model():
    """the model ops.IcpModels.from_meshset(meshset, [0], 1024) samples: key 0 under seed 0, rounded once to float32"""
    v, f = icp_ref.two_boxes()
    return mesh_sample_ref.sample(v, f, mesh_sample_ref.device_uniforms(0, 0, 1024))[0].astype(np.float32)


def extent():
    v = icp_ref.two_boxes()[0].astype(np.float64)
    return v.max(0) - v.min(0)


@functools.lru_cache(maxsize=None)
def fitted(k, seed=SEED):
    """plane_ref.fit of frame k as the tracker asks for it: key = the frame's index, seed = the evaluater's"""
    return plane_ref.fit(rendered(k), CAMK, key=k, seed=seed, hypotheses_n=HYPOTHESES, tol=TOL, refine_iters=2, min_inliers=100)


@functools.lru_cache(maxsize=None)
def simulate(with_cut):
    """The tracker on the CPU: the crop is the ball crop's restatement (tests/ball_ref.py) with the device's keyed draw of N_PTS points
    under seed SEED + frame, the refinement icp_ref.refine from the previous pose (float32 between frames, as the device keeps it).
    -> list over frames of list over objects of (rotation error degrees, translation error mm, inliers, status)"""
    f32 = np.float32
    poses = [gt_pose(0, o) for o in range(3)]
    ext = extent().astype(f32)
    out = []
    for k in range(FRAMES):
        depth = rendered(k)
        if with_cut:
            ft = fitted(k)
            assert ft["info"][0] == 0
            depth = plane_ref.cut(depth, ft["plane"], 0, CAMK, MARGIN)[0]
        row = []
        for o in range(3):
            R, t, s = poses[o]
            radius = f32(np.linalg.norm(((R * s).astype(f32) @ ext).astype(f32)).astype(f32) * f32(RATIO))
            recs, counts = ball_ref.ball_cloud(depth, CAMK, t.astype(f32), ball_ref.ladder_of(radius))
            sel = ball_ref.sample_selection(int(counts[1]), N_PTS, SEED + k, o)
            src, _ = ball_ref.ball_select(recs, counts[1], H * W, sel, ball_ref.depth_points_of(depth, CAMK))
            r = icp_ref.refine(model(), src, R.astype(f32), t.astype(f32), f32(s), GATE, mode=1)
            if r["status"] == 0:
                poses[o] = (r["R"].astype(np.float64), r["t"].astype(np.float64), s)
            Rg, tg, _ = gt_pose(k, o)
            e = icp_ref.pose_error(poses[o][0], poses[o][1], Rg, tg)
            row.append((e[0], e[1], r["inliers"], r["status"]))
        out.append(row)
    return out


def worst(sim):
    """(largest rotation error, largest translation error, fewest inliers) over a simulation's frames and objects"""
    flat = [e for row in sim for e in row]
    return max(e[0] for e in flat), max(e[1] for e in flat), min(e[2] for e in flat)


# ---- the small frames of tests/test_plane_gpu.py: 37 x 53 (1961 pixels: not a multiple of 8, so the scalar loads and the tail
# group; fewer pixels than one scoring tile), 70 hypotheses (not a multiple of 64)
SH, SW, SMALL_HYPOTHESES = 37, 53, 70
SMALL_CAMK = (60.0, 61.0, 26.0, 18.25)
SMALL_KEYS = (11, 12, 13, 14, 2 ** 40 + 15)


def _plane_depth(n, d, r, noise_mm):
    """the depth image (millimetres, float) of the plane n.p + d = 0 seen through SMALL_CAMK, plus uniform noise"""
    ys, xs = np.mgrid[0:SH, 0:SW]
    ray = np.stack([(xs - SMALL_CAMK[2]) / SMALL_CAMK[0], (ys - SMALL_CAMK[3]) / SMALL_CAMK[1], np.ones((SH, SW))], -1)
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    return 1000.0 * (-d / (ray @ n)) + r.uniform(-noise_mm, noise_mm, (SH, SW))


def small_frames():
    """(5, 37, 53) uint16: 0 a tilted plane with a bump in front of it, holes and one saturated pixel (65535); 1 all invalid; 2 two
    valid pixels; 3 two fronto-parallel planes of 26 x 37 pixels each (any three pixels of one give that plane exactly, so the two
    planes' hypotheses tie at 962 inliers); 4 another tilted plane, noisier, half of it missing"""
    r = np.random.RandomState(7)
    ys, xs = np.mgrid[0:SH, 0:SW]
    f0 = _plane_depth([0.1, -0.8, -0.6], 0.55, r, 1.0)
    bump = (xs - 30.0) ** 2 + (ys - 15.0) ** 2 < 7.0 ** 2
    f0[bump] -= 60.0 + r.uniform(0, 30.0, int(bump.sum()))
    f0[r.rand(SH, SW) < 0.06] = 0
    f0 = np.rint(f0).astype(np.uint16)
    f0[3, 5] = 65535
    f1 = np.zeros((SH, SW), np.uint16)
    f2 = np.zeros((SH, SW), np.uint16)
    f2[4, 7], f2[30, 41] = 700, 900
    f3 = np.zeros((SH, SW), np.uint16)
    f3[:, :26], f3[:, 27:] = 800, 1000
    f4 = _plane_depth([-0.2, -0.5, -0.85], 0.7, r, 2.0)
    f4[xs + ys > 60] = 0
    f4 = np.rint(f4).astype(np.uint16)
    return np.stack([f0, f1, f2, f3, f4])
