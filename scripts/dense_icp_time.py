"""Times dense projective ICP (ops.icp_dense: csrc/icp_dense.hip), pose.DenseRefine and myEvaluater.scan_track(register='dense')
beside the sparse path they stand next to.  Writes profiles/dense_icp_time.json:

  * icp_dense: device time of ONE call of 6 and of 192 jobs (every object of the six-object rendered 480 x 640 scene of
    scripts/tsdf_time.py, in one and in 32 frames, against the six volumes fused from the 32 frames at G = 64) with 96 x 128 maps cast
    at the start poses, stride 1 and 2; the start is each object's ground-truth pose turned 2 degrees and moved 3 mm; with the
    source pixels, candidates, inliers and iterations per job.
  * refine: pose.DenseRefine (windows, ray cast, rectangles, dense ICP) against today's path on the same jobs:
    load_data_eval.clouds_from_poses (the ball crop and its 1024-point sample) plus pose.RaycastRefine (windows, 40 x 48 ray cast,
    packing, icp_refine); device time of the whole chain, and the inliers per object of both.
  * scan_track: host-clock milliseconds per frame of myEvaluater.scan_track on the six objects over the 32 frames with
    register='dense' and with register='sparse', and the shares of frames x objects fused.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/dense_icp_time.py [--reps 10] [--warmup 3] [--out profiles/dense_icp_time.json]
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

from raycast_time import _median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_icp_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dense_icp_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tests import icp_ref
    from tgpose_amd import PoseNet9D, ops, pose
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": bct.H, "W": bct.W, "map": [96, 128],
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
    scales = np.stack([fr["gt_scales"][:6] for fr in frames]).astype(np.float32)
    ev = myEvaluater(PoseNet9D().to(dev).eval(), sampler="device", seed=1)
    vol = ops.TsdfVolumes.from_meshset(objects, 64)
    ev.scan(seq, list(RTs), K, volumes=vol, trunc_mm=2000.0 * float(vol.meta_host[:, 3].max()) * 0.14, inst_ids=[1, 2, 3, 4, 5, 6])
    depth_all, inst_all, camk_all = lde._depth_frames(seq, K, dev)
    inst_all = inst_all.view(torch.uint8)
    turn = icp_ref.rot([1, 2, -1], 2.0)
    start = RTs.astype(np.float64).copy()
    start[:, :, :3, :3] = turn @ start[:, :, :3, :3]
    start[:, :, :3, 3] += 0.003 * np.array([2.0, -1.0, 2.0]) / 3.0
    s0 = np.cbrt(np.abs(np.linalg.det(RTs[0, :, :3, :3].astype(np.float64))))
    gate = 3.0 * float((vol.meta_host[:, 3].astype(np.float64) * s0).max())
    res["gate_m"] = gate
    res["icp_dense"], res["refine"] = [], []
    for S in (1, a.frames):
        J = 6 * S
        job_img = torch.from_numpy(np.repeat(np.arange(S), 6).astype(np.int32)).to(dev)
        job_model = torch.from_numpy(np.tile(np.arange(6), S).astype(np.int32)).to(dev)
        vals = (job_model + 1).to(torch.uint8)
        rts = torch.from_numpy(start[:S].reshape(J, 4, 4).astype(np.float32)).to(dev)
        scl = torch.from_numpy(scales[:S].reshape(J, 3)).to(dev)
        depth, inst, camk = depth_all[:S].contiguous(), inst_all[:S].contiguous(), camk_all[:S].contiguous()
        P = pose.verify_job_pose(rts)
        win = ops.tsdf_windows(vol, camk, job_img, job_model, P, 96, 128, bct.H, bct.W)
        cast = ops.tsdf_raycast(vol, camk, job_img, job_model, P, win, 96, 128)
        rect = ops.dense_rects(win, 96, 128, bct.H, bct.W)
        R, t, s = pose.split_RT(rts)
        for stride in (1, 2):
            run = lambda: ops.icp_dense(depth, camk, job_img, rect, cast, win, P, R, t, s, gate, stride=stride, mask=inst, job_mask_val=vals)
            info = run()[3].cpu().numpy()
            box = rect.cpu().numpy().astype(np.int64)
            pix = ((box[:, 2] - box[:, 0]) // stride + 1) * ((box[:, 3] - box[:, 1]) // stride + 1)
            row = dict(jobs=J, stride=stride, launches=1, ok=int((info[:, 0] == 0).sum()), mean_source_pixels=float(pix.mean()),
                       mean_candidates=float(info[:, 3].mean()), mean_inliers=float(info[:, 1].mean()), mean_iterations=float(info[:, 2].mean()),
                       **_median_ms(run, a.warmup, a.reps, 20 if S == 1 else 5))
            res["icp_dense"].append(row)
            print(json.dumps(row), flush=True)
        dense = pose.DenseRefine(vol, gate, job_model=job_model)
        sparse = pose.RaycastRefine(vol, gate, job_model=job_model, mode="plane")
        crop = dict(depth=depth, inst_mask=inst)
        ids = (job_model + 1).cpu().tolist()

        def today():
            pts = lde.clouds_from_poses(crop, job_img, rts, scl, bct.RATIO, K, n_pts=bct.N_PTS, sampler="device", masks=ids, seed=1, device=dev)[0]
            return sparse(pts, rts, camk, job_img, bct.H, bct.W)
        for name, fn in (("DenseRefine", lambda: dense(depth, rts, camk, job_img, mask=inst, job_mask_val=vals)),
                         ("clouds_from_poses + RaycastRefine", today)):
            _, info, rmse, hits = fn()
            info = info.cpu().numpy()
            row = dict(path=name, jobs=J, ok=int((info[:, 0] == 0).sum()), mean_inliers=float(info[:, 1].mean()), mean_ray_hits=float(hits.float().mean()),
                       inliers_first_frame=info[:6, 1].tolist(), **_median_ms(fn, a.warmup, a.reps, 10 if S == 1 else 3))
            res["refine"].append(row)
            print(json.dumps(row), flush=True)
    init = dict(class_ids=frames[0]["gt_class_ids"][:6], RTs=frames[0]["gt_RTs"][:6], scales=frames[0]["gt_scales"][:6], inst_ids=[1, 2, 3, 4, 5, 6])
    res["scan_track"] = []
    for register in ("dense", "sparse"):
        go = lambda frames_: ev.scan_track(frames_, init, K, bct.RATIO, volumes=ops.TsdfVolumes.from_meshset(objects, 64), register=register)[0]
        go(seq[:4])
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            out = go(seq)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t_0) * 1e3 / len(seq))
        row = dict(register=register, frames=len(seq), objects=6, host_clock=True, ms_per_frame=statistics.median(t), min_ms=min(t), max_ms=max(t),
                   fused_share=float(np.mean([o["fused"].mean() for o in out])), icp_ok_share=float(np.mean([(o["icp_status"] == 0).mean() for o in out[1:]])),
                   mean_inliers=float(np.mean([o["icp_inliers"].mean() for o in out[1:]])), mean_ray_hits=float(np.mean([o["ray_hits"].mean() for o in out[1:]])))
        res["scan_track"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, default=float)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
