"""Times the ball crop (ops.ball_cloud + ops.ball_sample: csrc/ballcrop.hip, two launches) on rendered 480 x 640 frames of six
objects each.  Writes profiles/ball_crop_time.json:

  * crop_sample: device time of the crop and the keyed draw of 1024 points for 1, 6 and 32 x 6 jobs, with the rectangle and with
    full_scan=True, inputs already on the device; `hbm_bytes_per_job` is what a job must move: the frame's depth once (2 H W; a
    second pass over the rectangle hits L2), 4 bytes per kept pixel out, 16 bytes per selected point;
  * roi_path: ops.roi_cloud + ops.cloud_sample (what clouds_from_frames(sampler='device') launches) for the same objects from the
    renderer's masks and boxes, inputs already on the device, and clouds_from_frames itself on the host clock (packing and upload
    included);
  * reference_method_cpu: the reference's per-object method (back-project the frame, nonzero(), distances, the radius loop,
    randperm) as torch CPU code for ONE object, host clock, one run -- indicative only;
  * track: milliseconds per frame of myEvaluater.track over a rendered sequence (randomly initialised network: a time, no accuracy).
Device times are per call: a window is --calls back-to-back calls between two HIP events, divided by the number of calls; median
of --reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/ball_crop_time.py [--reps 7] [--warmup 3] [--calls 50] [--out profiles/ball_crop_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, N_PTS, RATIO = 480, 640, 1024, 0.5
NAMES = ("bottle", "bowl", "can", "mug")


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


def _rot_x(deg):
    a = np.deg2rad(deg)
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def scenes(n):
    """n frames: six objects in two rows on a table, moved 2 mm per frame"""
    out = []
    for k in range(n):
        sc = []
        for o in range(6):
            t = np.array([-0.3 + 0.3 * (o % 3), -0.12 + 0.22 * (o // 3), 0.8 + 0.1 * (o // 3)]) + k * np.array([0.002, 0.0, 0.001])
            sc.append(dict(mesh=o % 4, inst_id=o + 1, R=_rot_x(-160.0), t=t, s=0.14, labels=dict(cat_id=(0, 1, 3, 5)[o % 4])))
        sc.append(dict(mesh=4, inst_id=200, R=_rot_x(-70.0), t=np.array([0.0, 0.25, 1.0]), s=1.0))
        out.append(sc)
    return out


def reference_method_cpu(depth, K, center, radius, n_pts):
    """crop_ball_from_depth_image's steps for one object, on the CPU"""
    z = torch.from_numpy(depth.astype(np.float32) / 1000.0)
    ys = torch.arange(H, dtype=torch.float32) - float(K[1, 2])
    xs = torch.arange(W, dtype=torch.float32) - float(K[0, 2])
    pts = torch.stack((xs[None, :] * z / float(K[0, 0]), ys[:, None] * z / float(K[1, 1]), z), 2).reshape(-1, 3)
    pts = pts[(z > 0).flatten().nonzero()[:, 0]]
    d = torch.sqrt(((pts - center) ** 2).sum(-1))
    for _ in range(10):
        idx = torch.where(d <= radius)[0]
        if len(idx) >= 10:
            break
        radius *= 1.10
    while len(idx) < n_pts:
        idx = torch.cat([idx, idx])
    return pts[idx[torch.randperm(len(idx))[:n_pts]]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_crop_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ball_crop_time.py measures on a GPU; none is visible")
    from tgpose_amd import PoseNet9D, ops, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    K = lde.CAMERA_INTRINSICS
    ms = ops.MeshSet([shapes.lathe(shapes.PROFILES[n], 24) for n in NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    sc = scenes(a.frames)
    rendered = synthetic.render_scenes(ms, sc, K, H, W)
    frames = [synthetic.scene_frame(ms, sc, rendered, i) for i in range(a.frames)]
    for i, fr in enumerate(frames):
        assert fr["pred_masks"].shape[2] == 7, "every instance must be visible"
        fr["inst_mask"] = rendered["mask"][i]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": H, "W": W, "n_pts": N_PTS, "ratio": RATIO,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so"}
    depth, inst, camk = lde._depth_frames(frames, K, torch.device(dev))
    RTs = torch.from_numpy(np.concatenate([fr["gt_RTs"][:6] for fr in frames]).astype(np.float32)).to(dev)
    scales = torch.from_numpy(np.concatenate([fr["gt_scales"][:6] for fr in frames]).astype(np.float32)).to(dev)
    job_img = torch.arange(a.frames, dtype=torch.int32, device=dev).repeat_interleave(6)
    centers, ladder = lde.pose_balls(RTs, scales, RATIO)
    res["crop_sample"] = []
    for J in (1, 6, 6 * a.frames):
        for full in (False, True):
            def run():
                br = ops.ball_cloud(depth, job_img[:J], centers[:J], ladder[:J], camk, full_scan=full)
                return br, ops.ball_sample(br, N_PTS, 1)
            br, _ = run()
            counts = br.counts.cpu().numpy()
            assert (counts[:, 3] == 0).all()
            row = dict(jobs=J, full_scan=full, launches=2, mean_count=float(counts[:, 1].mean()), mean_level=float(counts[:, 2].mean()),
                       hbm_bytes_per_job=int(2 * H * W + 4 * counts[:, 1].mean() + 16 * N_PTS),
                       **_median_ms(run, a.warmup, a.reps, a.calls if J <= 6 else max(1, a.calls // 10)))
            res["crop_sample"].append(row)
            print(json.dumps(row), flush=True)
    # the ROI path on the same objects (the table's channel left out: six detections per frame)
    for fr in frames:
        fr.update(pred_masks=fr["pred_masks"][:, :, :6], pred_bboxes=fr["pred_bboxes"][:6], pred_class_ids=fr["pred_class_ids"][:6],
                  pred_scores=fr["pred_scores"][:6])
    res["roi_path"] = []
    for n in (1, a.frames):
        up = lde.upload(frames[:n], K, dev)
        torch.cuda.synchronize()

        def roi():
            return ops.cloud_sample(ops.roi_cloud(*up), N_PTS, 1)
        row = dict(detections=6 * n, launches=2, **_median_ms(roi, a.warmup, a.reps, a.calls if n == 1 else max(1, a.calls // 10)))
        t0 = time.perf_counter()
        lde.clouds_from_frames(frames[:n], K, sampler="device", seed=1, device=dev)
        torch.cuda.synchronize()
        row["clouds_from_frames_host_ms"] = (time.perf_counter() - t0) * 1e3
        res["roi_path"].append(row)
        print(json.dumps(row), flush=True)
    c0, lad0 = centers[0].cpu(), ladder[0, 0].cpu().clone()
    t0 = time.perf_counter()
    reference_method_cpu(frames[0]["depth"], K, c0, lad0, N_PTS)
    res["reference_method_cpu"] = dict(objects=1, ms=(time.perf_counter() - t0) * 1e3, threads=torch.get_num_threads())
    print(json.dumps(res["reference_method_cpu"]), flush=True)
    net = PoseNet9D().to(dev).eval()
    net.load_state_dict(seeded_state_dict(0))
    init = dict(class_ids=frames[0]["gt_class_ids"][:6], RTs=frames[0]["gt_RTs"][:6], scales=frames[0]["gt_scales"][:6],
                inst_ids=[1, 2, 3, 4, 5, 6])
    res["track"] = []
    for sampler in ("device", "fps"):
        ev = myEvaluater(net, sampler=sampler, seed=1)
        seq = [dict(depth=fr["depth"], inst_mask=fr["inst_mask"]) for fr in frames]
        ev.track(seq[:4], init, K, RATIO)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ev.track(seq, init, K, RATIO)
        torch.cuda.synchronize()
        row = dict(sampler=sampler, frames=len(seq), objects=6, host_clock=True, ms_per_frame=(time.perf_counter() - t0) * 1e3 / len(seq),
                   tracked_share=float(np.mean([o["tracked"].mean() for o in out])))
        res["track"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
