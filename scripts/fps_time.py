"""Times farthest point sampling on the device (ops.farthest_points: csrc/fps.hip, all n steps of every cloud in one launch) and the
two loaders with it.  Writes profiles/fps_time.json:

  * kernel: device time by HIP events around the call (output allocation and the ctypes call included), median of --reps calls after
    --warmup, for B = 32 and 192 uniform random clouds of M = 2048, 4096 and the cap, n = 1024;
  * eval: the evaluation input side, clouds_from_frames(sampler='fps') against sampler='device', on 32 synthetic frames of 6
    detections held in host memory (host clock from the call to a device synchronise: upload, ROI kernel, sampling);
  * train: train_batch of 32 synthetic items with pcl_select='fps' against the default (host clock to a synchronise);
  * reference_cpu: the reference's own farthest_points on a CPU for one cloud of the same sizes, as recorded in
    tests/golden/fps_ref.npz (one run, one thread; indicative only);
  * coverage: the coverage radius -- the maximum over the cloud of the distance to the nearest selected point -- of the FPS
    selection against random selections of the same size (np.random.permutation prefixes, --draws of them) on the fixture's clouds.

    python scripts/fps_time.py [--reps 5] [--warmup 2] [--out profiles/fps_time.json]
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


def _median_ms(fn, warmup, reps, events=True):
    times = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        if events:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            dt = s.elapsed_time(e)
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            times.append(dt)
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--draws", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_time.json"))
    a = ap.parse_args()
    from tests import fps_ref
    from tests.util import golden, synth_depth_scene
    from tgpose_amd import ops
    from tgpose_amd.datasets import load_data as ld
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    cap = ops.fps_max_points()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "cap": cap, "kernel": [], "eval": [], "train": [],
           "reference_cpu": [], "coverage": [],
           "note": "kernel: HIP events around ops.farthest_points; eval / train: host clock from the call to a device synchronise; "
                   "median of `reps` calls after `warmup`"}
    for B in (32, 192):
        for M in (2048, 4096, cap):
            x = torch.from_numpy(np.random.default_rng(M).random((B, M, 3), dtype=np.float32)).to(dev)
            run = dict(B=B, M=M, n=1024, launches=1, **_median_ms(lambda: ops.farthest_points(x, 1024), a.warmup, a.reps))
            res["kernel"].append(run)
            print(json.dumps(run), flush=True)

    frames = [synth_depth_scene(7000 + i, 6) for i in range(32)]
    for sampler in ("device", "fps"):
        run = dict(frames=32, detections=192, sampler=sampler,
                   **_median_ms(lambda: lde.clouds_from_frames(frames, sampler=sampler, seed=1, device=dev), a.warmup, a.reps, events=False))
        res["eval"].append(run)
        print(json.dumps(run), flush=True)

    from tests.test_train_loop_gpu import _items
    items = [{k: v for k, v in it.items() if k not in ("pdh1", "pdh2")} for i, it in enumerate(_items(33)) if i != 1]
    for sel in ("random", "fps"):
        rng, gen = np.random.RandomState(1), torch.Generator().manual_seed(1)
        run = dict(B=len(items), pcl_select=sel,
                   **_median_ms(lambda: ld.train_batch(items, rng=rng, gen=gen, device=dev, pcl_select=sel), a.warmup, a.reps, events=False))
        res["train"].append(run)
        print(json.dumps(run), flush=True)

    g = golden("fps_ref.npz")
    for M, sec in zip(g["time_M"].tolist(), g["time_seconds"].tolist()):
        res["reference_cpu"].append(dict(M=M, n=1024, clouds=1, seconds=sec))
    rng = np.random.RandomState(0)
    for name, n in zip(g["names"].tolist(), g["n"].tolist()):
        xyz = g[name + "_xyz"]
        idx = ops.farthest_points(torch.from_numpy(xyz).to(dev)[None], n)[0].cpu().numpy()
        assert np.array_equal(idx, g[name + "_centers"])
        rand = [fps_ref.coverage_radius(xyz, rng.permutation(len(xyz))[:n]) for _ in range(a.draws)]
        run = dict(cloud=name, M=len(xyz), n=n, fps_radius=fps_ref.coverage_radius(xyz, idx), random_radius_mean=float(np.mean(rand)),
                   random_radius_min=float(np.min(rand)), random_draws=a.draws, reference_cpu_seconds=float(g[name + "_seconds"]))
        res["coverage"].append(run)
        print(json.dumps(run), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
