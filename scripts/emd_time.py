"""Times the EMD forward (ops.emd_fwd: csrc/emd.hip, every auction iteration in one launch) on uniform clouds in [0,1]^3.

For B = 32 at n = 1024, 1028 and 2048 and (eps, iters) = (0.005, 50) -- calc_emd's defaults -- and (0.004, 3000): device time by HIP
events around the call, median of --reps calls after --warmup, with the share of points still unassigned before the last iteration
(a property of the input, read from the result) and the launch counts: 1 here, 7 * iters + 1 in the reference's emd_cuda.cu
(which cannot run on this hardware and refuses n = 1028, so only the count is compared).
Writes profiles/emd_time.json.

    python scripts/emd_time.py [--reps 5] [--warmup 1] [--out profiles/emd_time.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emd_time.json"))
    a = ap.parse_args()
    from tgpose_amd import ops
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "runs": [],
           "note": "HIP events around ops.emd_fwd (output allocation and the ctypes call included), median of `reps` calls; "
                   "duplicate_share: points of xyz1 whose object is also another point's (0 = the auction converged)"}
    B = a.batch
    for n in (1024, 1028, 2048):
        rng = np.random.default_rng(n)
        x1 = torch.from_numpy(rng.random((B, n, 3), dtype=np.float32)).cuda()
        x2 = torch.from_numpy(rng.random((B, n, 3), dtype=np.float32)).cuda()
        for eps, iters in ((0.005, 50), (0.004, 3000)):
            times = []
            for r in range(a.warmup + a.reps):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                dist, asg = ops.emd_fwd(x1, x2, eps, iters)
                e.record()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times.append(s.elapsed_time(e))
            distinct = sum(int(row.unique().numel()) for row in asg)
            run = dict(B=B, n=n, eps=eps, iters=iters, device_ms=statistics.median(times), min_ms=min(times), max_ms=max(times),
                       duplicate_share=1.0 - distinct / (B * n), mean_emd=float(torch.sqrt(dist).mean()),
                       launches=1, reference_launches=7 * iters + 1)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
