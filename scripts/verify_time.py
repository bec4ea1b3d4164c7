"""Times pose verification (ops.pose_verify: csrc/verify.hip, four launches, no frame written).  Writes profiles/verify_time.json:

  * pose_verify: device time of one call at 480 x 640 on the six-object rendered scene scripts/icp_time.py tracks (the scenes of
    scripts/ball_crop_time.py), every object at its ground-truth pose against its frame with the rendered instance mask: J = 6 jobs
    on one frame, and 32 x 6 = 192 jobs over 32 frames.
  * composed: the only way to the same counts without the kernel -- ops.render_depth with one scene per job (J full frames written)
    and the classification with torch operations, `torch_classify` below.  Its counts are compared with the kernel's
    (counts_equal) in the same run.
  * track: milliseconds per frame, host clock, of myEvaluater.track(refine=..., init_from='previous') on the same 32 frames with
    and without verify=pose.Verify(...), alternated.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/verify_time.py [--reps 10] [--warmup 3] [--out profiles/verify_time.json]
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


def torch_classify(ren, depth, job_img, mask, job_mask_val, tau):
    """the counts of ops.pose_verify from ops.render_depth's output for one scene per job (J,H,W), with torch operations"""
    wide = lambda t: t.view(torch.int16).to(torch.int32) & 0xffff
    idx = job_img.long()
    d_r, d_o, covered = wide(ren["depth"]), wide(depth)[idx], ren["mask"] > 0
    nodata = covered & ((d_o == 0) | (d_r == 0))
    rest = covered & ~nodata
    diff = (d_o - d_r).abs()
    occluded = rest & (d_o + tau < d_r)
    match = rest & (diff <= tau)
    violation = rest & (d_o > d_r + tau)
    in_mask = covered & (mask[idx] == job_mask_val[:, None, None])
    cols = [x.sum((1, 2)) for x in (covered, match, violation, occluded, nodata, in_mask)] + [(diff * match).sum((1, 2)), ren["dropped"].sum(1)]
    counts = torch.stack(cols, 1).to(torch.int32)
    den = (counts[:, 0] - counts[:, 3]).float()
    return counts, torch.where(den > 0, counts[:, 1].float() / den.clamp(min=1), torch.zeros_like(den))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--tau", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("verify_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": bct.H, "W": bct.W, "tau": a.tau,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so"}
    K = lde.CAMERA_INTRINSICS
    ms = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    sc = bct.scenes(a.frames)
    rendered = synthetic.render_scenes(ms, sc, K, bct.H, bct.W)
    frames = [synthetic.scene_frame(ms, sc, rendered, i) for i in range(a.frames)]
    depth_all = torch.from_numpy(np.stack([fr["depth"] for fr in frames]).view(np.int16)).to(dev)
    mask_all = torch.from_numpy(np.stack([rendered["mask"][i] for i in range(a.frames)])).to(dev)
    camk_all = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]] * a.frames, dtype=torch.float32, device=dev)
    RTs = torch.from_numpy(np.stack([fr["gt_RTs"][:6] for fr in frames]).astype(np.float32)).to(dev)           # (frames, 6, 4, 4)
    res["pose_verify"], res["composed"] = [], []
    for S in (1, a.frames):
        J = 6 * S
        depth, mask, camk = depth_all[:S].contiguous(), mask_all[:S].contiguous(), camk_all[:S].contiguous()
        job_img = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(6).contiguous()
        job_mesh = torch.tensor([o % 4 for o in range(6)] * S, dtype=torch.int32, device=dev)
        job_val = torch.tensor([o + 1 for o in range(6)] * S, dtype=torch.uint8, device=dev)
        job_pose = pose.verify_job_pose(RTs[:S].reshape(J, 4, 4))

        def run():
            return ops.pose_verify(ms, depth, camk, job_img, job_mesh, job_pose, tau=a.tau, mask=mask, job_mask_val=job_val)
        scene_ptr = torch.arange(J + 1, device=dev, dtype=torch.int32)
        ones = torch.ones(J, device=dev, dtype=torch.uint8)
        camk_job = camk[job_img.long()].contiguous()

        def comp():
            ren = ops.render_depth(ms, scene_ptr, job_mesh, ones, job_pose, camk_job, bct.H, bct.W)
            return torch_classify(ren, depth, job_img, mask, job_val, a.tau)
        out, (want, wscore) = run(), comp()
        counts = out["counts"].cpu().numpy()
        row = dict(jobs=J, frames=S, launches=4, rendered_pixels=int(counts[:, 0].sum()), frame_pixels=J * bct.H * bct.W,
                   mean_score=float(out["score"].mean()), **_median_ms(run, a.warmup, a.reps, 20 if S == 1 else 5))
        res["pose_verify"].append(row)
        print(json.dumps(row), flush=True)
        crow = dict(jobs=J, frames=S, counts_equal=bool(torch.equal(out["counts"], want)), score_equal=bool(torch.equal(out["score"], wscore)),
                    **_median_ms(comp, a.warmup, a.reps, 5 if S == 1 else 2))
        crow["ratio_to_kernel"] = crow["median_ms"] / row["median_ms"]
        res["composed"].append(crow)
        print(json.dumps(crow), flush=True)
    # the model-based tracker with and without the check
    seq = [dict(depth=fr["depth"], inst_mask=rendered["mask"][i]) for i, fr in enumerate(frames)]
    init = dict(class_ids=frames[0]["gt_class_ids"][:6], RTs=frames[0]["gt_RTs"][:6], scales=frames[0]["gt_scales"][:6], inst_ids=[1, 2, 3, 4, 5, 6])
    net = PoseNet9D().to(dev).eval()
    net.load_state_dict(seeded_state_dict(0))
    refine = pose.IcpRefine(ops.IcpModels.from_meshset(ms, [0, 1, 2, 3], 1024), [o % 4 for o in range(6)], 0.01, mode="plane")
    verify = pose.Verify(ms, [o % 4 for o in range(6)], tau=a.tau)
    ev = myEvaluater(net, sampler="device", seed=1)
    paths = (("previous+icp", {}), ("previous+icp+verify", dict(verify=verify)))
    ms_per_frame = {name: [] for name, _ in paths}
    last = {}
    for r in range(a.warmup + a.reps):
        for name, kw in paths:                               # alternated: the two share whatever else the machine does
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            last[name] = ev.track(seq, init, K, bct.RATIO, refine=refine, init_from="previous", **kw)
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms_per_frame[name].append((time.perf_counter() - t_0) * 1e3 / len(seq))
    res["track"] = []
    for name, _ in paths:
        t = ms_per_frame[name]
        row = dict(path=name, frames=len(seq), objects=6, n_pts=bct.N_PTS, host_clock=True, ms_per_frame=statistics.median(t), min_ms=min(t), max_ms=max(t))
        if "verified" in last[name][0]:
            row.update(verified_share=float(np.mean([o["verified"].mean() for o in last[name]])),
                       mean_score=float(np.mean([o["verify_score"].mean() for o in last[name]])))
        res["track"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
