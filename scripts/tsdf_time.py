"""Times TSDF fusion and meshing (ops.tsdf_integrate, ops.tsdf_mesh: csrc/tsdf.hip) and myEvaluater.scan.  Writes
profiles/tsdf_time.json:

  * tsdf_integrate: device time of ONE call that fuses 32 frames of 480 x 640 into M = 6 volumes of G = 64 (192 jobs) on the
    six-object rendered scene scripts/verify_time.py checks (the scenes of scripts/ball_crop_time.py), every object at its
    ground-truth pose with the rendered instance mask; and the same with one frame (6 jobs).
  * composed: the same integers from torch operations, job by job (`torch_integrate` below: every float32 step an operation of
    its own).  Its volumes are compared with the kernel's in the same run (sum_equal, weight_equal).
  * tsdf_mesh: device time of the count launch, the prefix sum and the emit launch on one fused volume with a face_cap (nothing read
    back), and the host-clock time of ops.tsdf_meshset over the six volumes (it reads every count and soup back).
  * scan: host-clock milliseconds of the whole of myEvaluater.scan on the 32 frames: upload, one integrate call, meshing.
  * loop: tests/tsdf_cases.scan_loop -- a model scanned from 12 rendered turntable frames, then ICP from 5 degrees / 10 mm off on
    a held-out view with the scanned and with the true model, and both meshes' render-and-compare scores: the errors
    tests/test_tsdf_gpu.py bounds by the volume's resolution.
  * downstream: tests/tsdf_cases.scan_downstream -- the same scan at G = 32 through pose.ModelSearch (search, ICP, verify) and
    evaluation.bop.score_track, with the scanned and with the true model.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/tsdf_time.py [--reps 10] [--warmup 3] [--out profiles/tsdf_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def torch_integrate(vsum, weight, meta_host, depth, camk, job_img, job_model, job_pose, mask, job_mask_val, trunc, near):
    """tgp_tsdf_integrate's integers from torch operations: one job at a time over its volume's G^3 voxels.  The host lists
    (job_img, job_model, job_mask_val) steer the loop; everything else stays on the device."""
    G, dev = vsum.shape[1], vsum.device
    S, H, W = depth.shape
    wide = lambda t: t.view(torch.int16).to(torch.int32) & 0xffff
    trunc_t = torch.tensor(np.float32(trunc), device=dev)
    inv = torch.tensor(np.float32(1024.0 / float(np.float32(trunc))), device=dev)
    idx = (torch.arange(G, device=dev, dtype=torch.float32) + 0.5) - float(G // 2)
    for j, (s, m) in enumerate(zip(job_img, job_model)):
        c = [torch.tensor(meta_host[m, a], device=dev) + idx * torch.tensor(meta_host[m, 3], device=dev) for a in range(3)]
        x, y, z = c[0][:, None, None], c[1][None, :, None], c[2][None, None, :]
        T = job_pose[j]
        p = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
        ok = p[2] > near
        u = camk[s, 0] * (p[0] / p[2]) + camk[s, 2]
        v = camk[s, 1] * (p[1] / p[2]) + camk[s, 3]
        ru, rv = torch.round(u), torch.round(v)
        ok = ok & (ru >= 0) & (ru <= W - 1) & (rv >= 0) & (rv <= H - 1)
        pix = torch.where(ok, rv, torch.zeros_like(rv)).long() * W + torch.where(ok, ru, torch.zeros_like(ru)).long()
        d = wide(depth[s]).reshape(-1)[pix]
        ok = ok & (d != 0)
        if mask is not None:
            ok = ok & (mask[s].reshape(-1)[pix] == job_mask_val[j])
        sdf = d.float() - p[2] * 1000.0
        ok = ok & ~(sdf < -trunc_t)
        q = torch.round(torch.minimum(sdf, trunc_t) * inv)
        vsum[m] += torch.where(ok, q, torch.zeros_like(q)).to(torch.int32)
        weight[m] += ok.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsdf_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tests import tsdf_cases as tc
    from tgpose_amd import PoseNet9D, ops, pose
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": bct.H, "W": bct.W, "G": a.G,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so"}
    K = lde.CAMERA_INTRINSICS
    shapes_ms = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    objects = ops.MeshSet([shapes.lathe(shapes.PROFILES[bct.NAMES[o % 4]], 24) for o in range(6)], device=dev)      # one cube per object
    sc = bct.scenes(a.frames)
    rendered = synthetic.render_scenes(shapes_ms, sc, K, bct.H, bct.W)
    frames = [synthetic.scene_frame(shapes_ms, sc, rendered, i) for i in range(a.frames)]
    depth_all = torch.from_numpy(np.stack([fr["depth"] for fr in frames]).view(np.int16)).to(dev)
    mask_all = torch.from_numpy(np.stack([rendered["mask"][i] for i in range(a.frames)])).to(dev)
    camk_all = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]] * a.frames, dtype=torch.float32, device=dev)
    RTs = np.stack([fr["gt_RTs"][:6] for fr in frames]).astype(np.float32)                                          # (frames, 6, 4, 4)
    volumes = ops.TsdfVolumes.from_meshset(objects, a.G)
    trunc = 2000.0 * float(volumes.meta_host[:, 3].max()) * 0.14
    res["trunc_mm"] = trunc
    res["tsdf_integrate"], res["composed"] = [], []
    for S in (1, a.frames):
        J = 6 * S
        depth, mask, camk = depth_all[:S].contiguous(), mask_all[:S].contiguous(), camk_all[:S].contiguous()
        img_host, model_host, val_host = np.repeat(np.arange(S), 6), np.tile(np.arange(6), S), np.tile(np.arange(1, 7), S)
        job_img = torch.from_numpy(img_host.astype(np.int32)).to(dev)
        job_model = torch.from_numpy(model_host.astype(np.int32)).to(dev)
        job_val = torch.from_numpy(val_host.astype(np.uint8)).to(dev)
        job_pose = pose.verify_job_pose(torch.from_numpy(RTs[:S].reshape(J, 4, 4)).to(dev))

        def run():
            return ops.tsdf_integrate(volumes, depth, camk, job_img, job_model, job_pose, trunc, mask=mask, job_mask_val=job_val)
        volumes.zero_()
        run()
        got_sum, got_weight = volumes.sum.clone(), volumes.weight.clone()
        want_sum, want_weight = torch.zeros_like(got_sum), torch.zeros_like(got_weight)

        def comp():
            torch_integrate(want_sum, want_weight, volumes.meta_host, depth, camk, img_host.tolist(), model_host.tolist(), job_pose, mask,
                            val_host.tolist(), trunc, 0.01)
        comp()
        row = dict(jobs=J, frames=S, volumes=6, launches=1, voxels_seen=int((got_weight > 0).sum()), observations=int(got_weight.sum()),
                   **_median_ms(run, a.warmup, a.reps, 20 if S == 1 else 5))
        res["tsdf_integrate"].append(row)
        print(json.dumps(row), flush=True)
        crow = dict(jobs=J, frames=S, sum_equal=bool(torch.equal(got_sum, want_sum)), weight_equal=bool(torch.equal(got_weight, want_weight)),
                    **_median_ms(comp, 1, 3, 1))
        crow["ratio_to_kernel"] = crow["median_ms"] / row["median_ms"]
        res["composed"].append(crow)
        print(json.dumps(crow), flush=True)
    # meshing: the volumes hold the frames fused once (run() above added to them again and again: fuse afresh)
    volumes.zero_()
    run()
    total = int(ops.tsdf_mesh(volumes, 0)["n_faces"])
    row = dict(G=a.G, faces=total, read_back=False, **_median_ms(lambda: ops.tsdf_mesh(volumes, 0, face_cap=total), a.warmup, a.reps, 10))
    res["tsdf_mesh"] = [row]
    print(json.dumps(row), flush=True)
    t = []
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t_0 = time.perf_counter()
        scanned = ops.tsdf_meshset(volumes)
        torch.cuda.synchronize()
        if r >= a.warmup:
            t.append((time.perf_counter() - t_0) * 1e3)
    row = dict(what="tsdf_meshset", volumes=6, faces=scanned.n_faces, host_clock=True, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
    res["tsdf_mesh"].append(row)
    print(json.dumps(row), flush=True)
    # the whole of scan
    seq = [dict(depth=fr["depth"], inst_mask=rendered["mask"][i]) for i, fr in enumerate(frames)]
    ev = myEvaluater(PoseNet9D().to(dev).eval(), sampler="device")
    t = []
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t_0 = time.perf_counter()
        ev.scan(seq, list(RTs), K, volumes=ops.TsdfVolumes.from_meshset(objects, a.G), trunc_mm=trunc, inst_ids=[1, 2, 3, 4, 5, 6])
        torch.cuda.synchronize()
        if r >= a.warmup:
            t.append((time.perf_counter() - t_0) * 1e3)
    row = dict(frames=len(seq), objects=6, G=a.G, host_clock=True, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
    res["scan"] = row
    print(json.dumps(row), flush=True)
    res["loop"] = json.loads(json.dumps(tc.scan_loop(dev), default=float))
    print(json.dumps(res["loop"]), flush=True)
    res["downstream"] = json.loads(json.dumps(tc.scan_downstream(dev), default=float))
    print(json.dumps(res["downstream"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
