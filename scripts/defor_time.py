"""Times the training loader's mask deformation (load_data.train_batch(..., roi_mask_pro)) at B = 32 and B = 256 on synthetic frames,
with roi_mask_pro = None and 0.5 alternating in one run.

Recorded per (B, roi_mask_pro), median over --reps calls after --warmup:
  * device time of the ROI launches by HIP events around each: tgp_roi_cloud_ex (None), or tgp_roi_band + tgp_roi_cloud_defor (0.5);
  * host time of the deformation draws (load_data.defor_draws);
  * device-to-host read-backs per call;
  * the wall time of the whole train_batch call.
The events bracket the ops.* calls (argument checks and the ctypes call included); kernel-only times come from a run under
``rocprofv3 --kernel-trace --stats`` with one size per run (``--sizes 32``), recorded beside them in profiles/defor_time.json.
Writes profiles/defor_time.json.

    python scripts/defor_time.py [--reps 10] [--warmup 2] [--out profiles/defor_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defor_time.json"))
    ap.add_argument("--sizes", default="32,256", help="batch sizes, comma-separated (one per run for a per-size kernel trace)")
    a = ap.parse_args()
    from augment_time import items_for
    from tgpose_amd import ops
    from tgpose_amd.datasets import load_data as ld
    rec = {"band": [], "cloud": [], "draws": 0.0, "readbacks": 0}

    def timed_launch(name, fn):
        def w(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*args, **kw)
            e.record()
            rec[name].append((s, e))
            return r
        return w
    real_band, real_cloud, real_draws, real_cpu = ops.roi_band, ops.roi_cloud, ld.defor_draws, torch.Tensor.cpu
    ops.roi_band, ops.roi_cloud = timed_launch("band", real_band), timed_launch("cloud", real_cloud)

    def draws(*args, **kw):
        t0 = time.perf_counter()
        r = real_draws(*args, **kw)
        rec["draws"] += time.perf_counter() - t0
        return r
    ld.defor_draws = draws

    def cpu(self, *args, **kw):
        if self.is_cuda:
            rec["readbacks"] += 1
        return real_cpu(self, *args, **kw)
    torch.Tensor.cpu = cpu
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "runs": []}
    for B in [int(v) for v in a.sizes.split(",")]:
        items = [{k: v for k, v in it.items()} for it in items_for(B)]
        stats = {None: [], 0.5: []}
        for r in range(a.warmup + a.reps):
            for pro in (None, 0.5):                                   # alternating in one run
                rec.update(band=[], cloud=[], draws=0.0, readbacks=0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                db = ld.train_batch(items, rng=np.random.RandomState(r), gen=torch.Generator().manual_seed(r), device="cuda",
                                    roi_mask_pro=pro)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                if r >= a.warmup:
                    stats[pro].append(dict(wall_ms=wall * 1e3, band_us=sum(s.elapsed_time(e) for s, e in rec["band"]) * 1e3,
                                           cloud_us=sum(s.elapsed_time(e) for s, e in rec["cloud"]) * 1e3, draws_ms=rec["draws"] * 1e3,
                                           readbacks=rec["readbacks"], kept=int(db["pcl_in"].shape[0])))
        for pro, runs in stats.items():
            med = lambda k: statistics.median(x[k] for x in runs)
            res["runs"].append(dict(B=B, roi_mask_pro=pro, wall_ms=med("wall_ms"), band_launch_us=med("band_us"),
                                    roi_cloud_launch_us=med("cloud_us"), defor_draws_ms=med("draws_ms"), readbacks=med("readbacks"),
                                    items_kept=med("kept")))
            print(json.dumps(res["runs"][-1]))
    ops.roi_band, ops.roi_cloud, ld.defor_draws, torch.Tensor.cpu = real_band, real_cloud, real_draws, real_cpu
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
