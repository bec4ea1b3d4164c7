"""Times the TSDF ray caster (ops.tsdf_raycast: csrc/raycast.hip) and myEvaluater.scan_track.  Writes profiles/raycast_time.json:

  * tsdf_raycast: device time of ONE call of 6 and of 192 jobs at 40 x 48 rays (the frame-to-model tracker's shape: every object of
    the six-object rendered scene of scripts/tsdf_time.py at its ground-truth pose, in one and in 32 frames, against the six volumes
    fused from the 32 frames at G = 64), and of one 480 x 640 depth map of one volume at G = 64 and at G = 32.
  * composed: the same rule from torch operations (`torch_raycast` below: every float32 step an operation of its own, all jobs and
    rays at once, one pass over the ray's samples per march step).  Its outputs are compared with the kernel's in the same run
    (`equal`: z, depth, vertex, normal, count and status, byte for byte).
  * windows_pack: device time of the torch glue round the kernel in the tracker: ops.tsdf_windows before and
    ops.IcpModels.from_raycast after it, 6 jobs.
  * scan_track: host-clock milliseconds per frame of myEvaluater.scan_track on the six objects over the 32 frames (crop, windows, ray
    cast, packing, ICP and fusion per frame, nothing read back between frames), beside myEvaluater.track(init_from='previous',
    refine=IcpRefine(the true meshes' models)) on the same frames, and the shares of frames x objects tracked and fused.
  * sequence: the worst pose errors of both trackers on the 24-frame sequence tests/test_raycast_gpu.py bounds (icp_ref.two_boxes
    turning 4 degrees a frame), with the voxel's size, and the worst vertex-to-surface distance of both meshes.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/raycast_time.py [--reps 10] [--warmup 3] [--out profiles/raycast_time.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

KEYS = ("z", "depth", "vertex", "normal", "count", "status")


def _median_ms(fn, warmup, reps, calls):
    times = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(s.elapsed_time(e) / calls)
    return dict(calls_per_window=calls, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))


def _div(a, b):
    """the correctly rounded float32 quotient whatever the build of torch's own: float64, rounded once (53 >= 2 x 24 + 2 bits)"""
    return (a.double() / b.double()).float()


def _sqrt(a):
    return a.double().sqrt().float()


def torch_raycast(volumes, camk, job_img, job_model, job_inv, window, h, w, min_weight=1, step=1.0, near=0.01):
    """tgp_tsdf_raycast's outputs from torch operations, all jobs and rays at once: (J, h w) tensors, one pass per march step"""
    dev, G, M, S = volumes.sum.device, volumes.G, len(volumes), camk.shape[0]
    J, n = job_img.numel(), h * w
    f32 = lambda v: torch.tensor(np.float32(v), device=dev)
    job_ok = (job_model >= 0) & (job_model < M) & (job_img >= 0) & (job_img < S)
    mdl, img = job_model.long().clamp(0, M - 1), job_img.long().clamp(0, S - 1)
    meta, K, inv, win = volumes.meta[mdl], camk[img], job_inv, window
    vsum, vweight = volumes.sum.reshape(-1), volumes.weight.reshape(-1)
    base = (mdl * (G * G * G))[:, None]
    voxel, half, last = meta[:, 3:4], f32(G // 2) - f32(0.5), f32(G - 1)
    cc = torch.arange(w, device=dev, dtype=torch.float32).repeat(h)[None]
    rr = torch.arange(h, device=dev, dtype=torch.float32).repeat_interleave(w)[None]
    u, v = win[:, 0:1] + cc * win[:, 2:3], win[:, 1:2] + rr * win[:, 3:4]
    dx, dy = _div(u - K[:, 2:3], K[:, 0:1]), _div(v - K[:, 3:4], K[:, 1:2])
    e = [_div((inv[:, q, 0:1] * dx + inv[:, q, 1:2] * dy) + inv[:, q, 2:3], voxel) for q in range(3)]
    o = [(_div(inv[:, q, 3:4] - meta[:, q:q + 1], voxel) + half).expand(J, n) for q in range(3)]
    inf = f32(np.inf)
    zin, zout = f32(near).expand(J, n), inf.expand(J, n)
    ok = job_ok[:, None].expand(J, n)
    for q in range(3):
        moving = e[q] != 0
        t0, t1 = _div(f32(0) - o[q], e[q]), _div(last - o[q], e[q])
        zin = torch.where(moving, torch.fmax(zin, torch.fmin(t0, t1)), zin)
        zout = torch.where(moving, torch.fmin(zout, torch.fmax(t0, t1)), zout)
        ok = ok & torch.where(moving, (t0 == t0) & (t1 == t1), (o[q] >= 0) & (o[q] <= last))
    length = _sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    dz = _div(f32(step).expand(J, n), length)
    ok = ok & (length > 0) & (length < inf) & (dz > 0) & (dz < inf) & (zin <= zout) & (zin < inf) & (zout < inf)

    def cell(g):
        inside = torch.ones_like(ok)
        for q in range(3):
            inside = inside & (g[q] >= -1) & (g[q] <= G)
        idx, t = [], []
        for q in range(3):
            i = torch.floor(torch.where(inside, g[q], torch.zeros_like(g[q]))).long().clamp(0, G - 2)
            idx.append(i)
            t.append(g[q] - i.float())
        known, f = inside, []
        for k in range(8):
            flat = base + ((idx[0] + (k >> 2)) * G + idx[1] + ((k >> 1) & 1)) * G + idx[2] + (k & 1)
            wk, sk = vweight[flat], vsum[flat]
            known = known & (wk >= min_weight)
            f.append(_div(sk.float(), wk.float()))
        return known, f, t

    lerp = lambda a, b, t: a + t * (b - a)

    def trilinear(f, t):
        c00, c01, c10, c11 = lerp(f[0], f[1], t[2]), lerp(f[2], f[3], t[2]), lerp(f[4], f[5], t[2]), lerp(f[6], f[7], t[2])
        c0, c1 = lerp(c00, c01, t[1]), lerp(c10, c11, t[1])
        return lerp(c0, c1, t[0]), (c00, c01, c10, c11, c0, c1)

    alive, have, hit = ok.clone(), torch.zeros_like(ok), torch.zeros_like(ok)
    fprev, zs = torch.zeros(J, n, device=dev), torch.zeros(J, n, device=dev)
    for k in range(int(math.ceil(1.7320508075688772 * float(G - 1) / float(np.float32(step)))) + 2):   # no early exit: nothing is read back
        zk = zin + f32(k) * dz
        alive = alive & (zk <= zout)
        known, f8, t = cell([o[q] + zk * e[q] for q in range(3)])
        f, _ = trilinear(f8, t)
        pos = alive & known & (f > 0)
        have = (have & ~(alive & ~known)) | pos
        fprev = torch.where(pos, f, fprev)
        end = alive & known & ~(f > 0)
        now = end & have
        zs = torch.where(now, (zin + f32(k - 1) * dz) + dz * _div(fprev, fprev - f), zs)
        hit = hit | now
        alive = alive & ~end
    g = [o[q] + zs * e[q] for q in range(3)]
    known, f8, t = cell(g)
    hit = hit & known
    _, (c00, c01, c10, c11, c0, c1) = trilinear(f8, t)
    nx, ny = c1 - c0, lerp(c01 - c00, c11 - c10, t[0])
    nz = lerp(lerp(f8[1] - f8[0], f8[3] - f8[2], t[1]), lerp(f8[5] - f8[4], f8[7] - f8[6], t[1]), t[0])
    size = _sqrt((nx * nx + ny * ny) + nz * nz)
    hit = hit & (size > 0) & (size < inf)
    zero = torch.zeros((), device=dev)
    normal = torch.stack([torch.where(hit, _div(c, size), zero) for c in (nx, ny, nz)], 2)
    vertex = torch.stack([torch.where(hit, meta[:, q:q + 1] + ((g[q] + f32(0.5)) - f32(G // 2)) * voxel, zero) for q in range(3)], 2)
    zs = torch.where(hit, zs, zero)
    mm = torch.round(zs * f32(1000))
    depth = torch.where(hit & (mm <= 65535), mm, zero).to(torch.int32).to(torch.int16)        # the low 16 bits: uint16's
    return dict(z=zs.reshape(J, h, w), depth=depth.reshape(J, h, w), vertex=vertex.reshape(J, h, w, 3), normal=normal.reshape(J, h, w, 3),
                count=hit.sum(1).to(torch.int32), status=(~job_ok).to(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raycast_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tests import icp_ref
    from tests import raycast_cases as rc
    from tests import tsdf_cases as tc
    from tgpose_amd import PoseNet9D, ops, pose
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": bct.H, "W": bct.W,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so"}
    K = lde.CAMERA_INTRINSICS
    shapes_ms = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    objects = ops.MeshSet([shapes.lathe(shapes.PROFILES[bct.NAMES[o % 4]], 24) for o in range(6)], device=dev)
    sc = bct.scenes(a.frames)
    rendered = synthetic.render_scenes(shapes_ms, sc, K, bct.H, bct.W)
    frames = [synthetic.scene_frame(shapes_ms, sc, rendered, i) for i in range(a.frames)]
    seq = [dict(depth=fr["depth"], inst_mask=rendered["mask"][i]) for i, fr in enumerate(frames)]
    RTs = np.stack([fr["gt_RTs"][:6] for fr in frames]).astype(np.float32)
    camk_all = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]] * a.frames, dtype=torch.float32, device=dev)
    ev = myEvaluater(PoseNet9D().to(dev).eval(), sampler="device", seed=1)
    filled = {}
    for G in (64, 32):
        filled[G] = ops.TsdfVolumes.from_meshset(objects, G)
        ev.scan(seq, list(RTs), K, volumes=filled[G], trunc_mm=2000.0 * float(filled[G].meta_host[:, 3].max()) * 0.14, inst_ids=[1, 2, 3, 4, 5, 6])
    res["tsdf_raycast"], res["composed"] = [], []

    def measure(what, vol, camk, job_img, job_model, job_pose, win, h, w, calls):
        inv = ops.pose_inverse(job_pose)
        run = lambda: ops.tsdf_raycast(vol, camk, job_img, job_model, job_pose, win, h, w, job_inv=inv)
        comp = lambda: torch_raycast(vol, camk, job_img, job_model, inv, win, h, w)
        got, want = run(), comp()
        row = dict(what=what, jobs=job_img.numel(), h=h, w=w, G=vol.G, launches=1, hits=int(got["count"].sum()), **_median_ms(run, a.warmup, a.reps, calls))
        res["tsdf_raycast"].append(row)
        print(json.dumps(row), flush=True)
        crow = dict(what=what, jobs=job_img.numel(), h=h, w=w, G=vol.G, equal={k: bool(torch.equal(got[k], want[k])) for k in KEYS}, **_median_ms(comp, 1, 3, 1))
        crow["ratio_to_kernel"] = crow["median_ms"] / row["median_ms"]
        res["composed"].append(crow)
        print(json.dumps(crow), flush=True)
    for S in (1, a.frames):
        J = 6 * S
        job_img = torch.from_numpy(np.repeat(np.arange(S), 6).astype(np.int32)).to(dev)
        job_model = torch.from_numpy(np.tile(np.arange(6), S).astype(np.int32)).to(dev)
        job_pose = pose.verify_job_pose(torch.from_numpy(RTs[:S].reshape(J, 4, 4)).to(dev))
        camk = camk_all[:S].contiguous()
        win = ops.tsdf_windows(filled[64], camk, job_img, job_model, job_pose, 40, 48, bct.H, bct.W)
        measure("models", filled[64], camk, job_img, job_model, job_pose, win, 40, 48, 50 if S == 1 else 10)
        if S == 1:
            cast = ops.tsdf_raycast(filled[64], camk, job_img, job_model, job_pose, win, 40, 48)
            glue = lambda: (ops.tsdf_windows(filled[64], camk, job_img, job_model, job_pose, 40, 48, bct.H, bct.W), ops.IcpModels.from_raycast(cast))
            res["windows_pack"] = dict(jobs=J, **_median_ms(glue, a.warmup, a.reps, 20))
            print(json.dumps(res["windows_pack"]), flush=True)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    full = torch.tensor([[0.0, 0.0, 1.0, 1.0]], device=dev)
    for G in (64, 32):
        measure("depth map", filled[G], camk_all[:1].contiguous(), one, one, pose.verify_job_pose(torch.from_numpy(RTs[0, :1]).to(dev)), full,
                bct.H, bct.W, 10)
    # the two trackers on the 32 frames
    init = dict(class_ids=frames[0]["gt_class_ids"][:6], RTs=frames[0]["gt_RTs"][:6], scales=frames[0]["gt_scales"][:6], inst_ids=[1, 2, 3, 4, 5, 6])
    refine = pose.IcpRefine(ops.IcpModels.from_meshset(shapes_ms, [0, 1, 2, 3], 1024), [o % 4 for o in range(6)], 0.01, mode="plane")
    res["scan_track"] = []
    for name in ("scan_track", "track previous+icp (true models)"):
        def go(frames_):
            if name == "scan_track":
                return ev.scan_track(frames_, init, K, bct.RATIO, volumes=ops.TsdfVolumes.from_meshset(objects, 64))[0]
            return ev.track(frames_, init, K, bct.RATIO, refine=refine, init_from="previous")
        go(seq[:4])
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            out = go(seq)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t_0) * 1e3 / len(seq))
        row = dict(path=name, frames=len(seq), objects=6, n_pts=bct.N_PTS, host_clock=True, ms_per_frame=statistics.median(t), min_ms=min(t), max_ms=max(t),
                   tracked_share=float(np.mean([o["tracked"].mean() for o in out])), icp_ok_share=float(np.mean([(o["icp_status"] == 0).mean() for o in out])))
        if "fused" in out[0]:
            row.update(fused_share=float(np.mean([o["fused"].mean() for o in out])), mean_ray_hits=float(np.mean([o["ray_hits"].mean() for o in out[1:]])))
        res["scan_track"].append(row)
        print(json.dumps(row), flush=True)
    # the sequence of tests/test_raycast_gpu.py: both trackers' worst errors, both meshes' worst vertex
    mesh = icp_ref.two_boxes()
    true = ops.MeshSet([mesh], device=dev)
    n = rc.SEQ_FRAMES
    rts = rc.smooth_rts(n)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    camk = up(np.tile(np.array([tc.LOOP_K[0, 0], tc.LOOP_K[1, 1], tc.LOOP_K[0, 2], tc.LOOP_K[1, 2]], dtype=np.float32), (n, 1)))
    ren = ops.render_depth(true, torch.arange(n + 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                           torch.ones(n, dtype=torch.uint8, device=dev), up(rts[:, :3, :4]), camk, tc.LOOP_H, tc.LOOP_W)
    depth = ren["depth"].cpu().numpy().view(np.uint16)
    two = [dict(depth=depth[k]) for k in range(n)]
    init2 = dict(class_ids=[3], RTs=rts[:1].astype(np.float32), scales=(mesh[0].max(0) - mesh[0].min(0)).astype(np.float32)[None])
    with_model = ev.track(two, init2, tc.LOOP_K, 0.6, n_pts=1024, use_mask=False, init_from="previous",
                          refine=pose.IcpRefine(ops.IcpModels.from_meshset(true, [0], 1024), [0], 0.01, mode="plane"))
    got, vol = ev.scan_track(two, init2, tc.LOOP_K, 0.6, volumes=ops.TsdfVolumes.from_meshset(true, 64), n_pts=1024, use_mask=False)
    _, posed = ev.scan(two, [rts[k][None] for k in range(n)], tc.LOOP_K, volumes=ops.TsdfVolumes.from_meshset(true, 64))

    def error(rt, k):
        rt, g = np.asarray(rt, dtype=np.float64), rts[k].astype(np.float64)
        s = np.cbrt(np.linalg.det(rt[:3, :3]))
        return icp_ref.pose_error(rt[:3, :3] / s, rt[:3, 3], g[:3, :3] / tc.TURN_SCALE, g[:3, 3])
    voxel = float(vol.meta_host[0, 3])
    centre = (mesh[0].max(0).astype(np.float64) + mesh[0].min(0)) / 2
    worst = lambda ms: float(tc.surface_distance(ms.verts.cpu().numpy()[:3 * ms.n_faces[0]], *mesh).max()) / voxel
    res["sequence"] = dict(frames=n, step_deg=rc.SEQ_STEP_DEG, start_deg=rc.SEQ_START_DEG, G=64, voxel_mm=1000 * voxel * tc.TURN_SCALE,
                           voxel_angle_deg=float(np.rad2deg(np.arctan(voxel / np.linalg.norm(mesh[0].astype(np.float64) - centre, axis=1).max()))),
                           scan_track_worst_deg=max(error(g["pred_RTs"][0], k)[0] for k, g in enumerate(got)),
                           scan_track_worst_mm=max(error(g["pred_RTs"][0], k)[1] for k, g in enumerate(got)),
                           true_model_worst_deg=max(error(g["pred_RTs"][0], k)[0] for k, g in enumerate(with_model)),
                           true_model_worst_mm=max(error(g["pred_RTs"][0], k)[1] for k, g in enumerate(with_model)),
                           fused_share=float(np.mean([g["fused"].mean() for g in got])),
                           mesh_worst_vertex_voxels=dict(scan_track=worst(ops.tsdf_meshset(vol)), scan_true_poses=worst(posed)))
    print(json.dumps(res["sequence"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, default=float)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
