"""Times mesh surface sampling on the device (ops.mesh_sample / mesh_sample_fps: csrc/meshsample.hip, one launch per call once the
mesh set's area table exists).  Writes profiles/mesh_sample_time.json:

  * area_table: the one-off table of a set of 32 meshes of 5120 faces (icosphere level 4): MeshSet.area_cdf() with the kept table
    dropped before every call (the allocation, the tgp_mesh_area_cdf launch and the one-off stream synchronise);
  * sample: B = 32 jobs x 2048 samples (points + normals, float32) with device draws, and with host draws already on the device;
  * sample_fps: B = 6 jobs x 1024 points kept of 2048 by farthest point sampling (sampling, tgp_fps, the gather);
  * python_loop_cpu: the reference's per-sample Python loop of the same arithmetic (np.searchsorted, the barycentric map) for ONE
    mesh and 2048 samples on a CPU, one run -- what the reference does per model; indicative only.
Device times are per call: a window is --calls back-to-back calls (output allocation and the ctypes call included) between two
HIP events, divided by the number of calls; median of --reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/mesh_sample_time.py [--reps 7] [--warmup 3] [--calls 200] [--out profiles/mesh_sample_time.json]
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


def _median_ms(fn, warmup, reps, calls):
    """per-call device time: each window is `calls` back-to-back calls between two HIP events, divided by `calls`"""
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


def python_loop(vertices, faces, n, rng):
    """the reference's uniform_sample loop restated: one face search and one point per Python iteration"""
    tri = vertices.astype(np.float64)[faces]
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    cum = np.cumsum(0.5 * np.linalg.norm(cross, axis=1))
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        k = np.searchsorted(cum, rng.random_sample() * cum[-1])
        r1, r2 = rng.random_sample(2)
        s = np.sqrt(r1)
        pts[i] = (1 - s) * tri[k, 0] + s * (1 - r2) * tri[k, 1] + s * r2 * tri[k, 2]
        nrm[i] = cross[k]
    return pts, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sample_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_sample_time.py measures on a GPU; none is visible")
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes
    dev = "cuda:0"
    v, f = shapes.icosphere(0.5, 4)
    meshes = [(v * (1.0 + 0.01 * k), f) for k in range(32)]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "faces_per_mesh": int(len(f)), "meshes": 32,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; python_loop_cpu: host clock, one run"}
    ms = ops.MeshSet(meshes, device=dev)

    def table():
        ms._area_cdf = None
        ms.area_cdf()
    res["area_table"] = dict(launches=1, **_median_ms(table, a.warmup, a.reps, max(1, a.calls // 4)))
    print(json.dumps(res["area_table"]), flush=True)
    jobs = torch.arange(32, dtype=torch.int32, device=dev)
    keys = torch.arange(32, dtype=torch.int64, device=dev)
    u = torch.from_numpy(np.random.RandomState(0).random_sample((32, 2048, 3))).to(dev)
    res["sample"] = []
    for draws, kw in (("device", dict(keys=keys, seed=1)), ("host", dict(u=u))):
        run = dict(B=32, n=2048, draws=draws, normals=True, dtype="float32", launches=1,
                   **_median_ms(lambda: ops.mesh_sample(ms, jobs, 2048, normals=True, **kw), a.warmup, a.reps, a.calls))
        res["sample"].append(run)
        print(json.dumps(run), flush=True)
    run = dict(B=6, n=1024, ratio=2, draws="device",
               **_median_ms(lambda: ops.mesh_sample_fps(ms, jobs[:6], 1024, 2, keys=keys[:6], seed=1), a.warmup, a.reps,
                             max(1, a.calls // 10)))
    res["sample_fps"] = run
    print(json.dumps(run), flush=True)
    t0 = time.perf_counter()
    python_loop(v, f, 2048, np.random.RandomState(0))
    res["python_loop_cpu"] = dict(meshes=1, n=2048, ms=(time.perf_counter() - t0) * 1e3)
    print(json.dumps(res["python_loop_cpu"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
