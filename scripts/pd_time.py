"""Device time of tgp_persistence (ops.persistence_images: the diagram and image launches) at B = 32 and B = 256 on realistic
clouds (the reference's seven training pcl_in clouds of tests/golden/pd.npz, cycled), and the float64 CPU restatement's time per
cloud (tests/pd_ref.py: scipy Delaunay, Python filtration and reduction) for contrast.  Writes profiles/pd_time.json.

    python scripts/pd_time.py [--reps 5] [--out profiles/pd_time.json]

The per-kernel split comes from a separate run: rocprofv3 --kernel-trace --stats -- python scripts/pd_time.py --reps 2 --cpu-clouds 0
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pd_time.json"))
    ap.add_argument("--cpu-clouds", type=int, default=2)
    a = ap.parse_args()
    from tgpose_amd import ops
    fx = np.load(os.path.join(ROOT, "tests", "golden", "pd.npz"))
    clouds = [fx["cloud.ref%d" % k] for k in range(7)]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "clouds": "reference training pcl_in (pd.npz ref0-ref6), cycled"}
    for B in (32, 256):
        pc = torch.from_numpy(np.stack([clouds[i % 7] for i in range(B)])).cuda()
        ops.persistence_images(pc)                     # warm-up, with the status check
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.persistence_images(pc, check_status=False)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        res["B%d_ms" % B] = {"median": float(np.median(ms)), "min": float(np.min(ms)), "all": ms}
        print("B=%d: %.3f ms median (%s)" % (B, np.median(ms), ", ".join("%.3f" % m for m in ms)), flush=True)
    if a.cpu_clouds:
        from tests import pd_ref
        t = []
        for k in range(a.cpu_clouds):
            t0 = time.perf_counter()
            pd_ref.compute_pd(clouds[k + 1])
            t.append(time.perf_counter() - t0)
        res["cpu_restatement_s_per_cloud"] = t
        print("CPU restatement: %s s per cloud" % ", ".join("%.2f" % x for x in t), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
