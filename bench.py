#!/usr/bin/env python3
"""bench.py -- objects/s of PoseNet9D.forward (eval, B=32 per GPU, N=1028) on the HIP path.

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: starts its N ranks as child processes)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one full forward of the hot path (kNN graphs, 3D-GCN encoder, PH predictor, decoder,
three heads, pose post-processing) over one batch of B synthetic clouds already resident in HBM
(BASELINE.json configs[1] extended to the whole forward, which is what `metric` is quoted on).
The forward is replayed as a captured hipGraph; by default four batches are in flight (`--streams 4`:
one captured forward per HIP stream, step i on stream i % 4 over its own batch; with three or more in
flight the captured forwards are branch-free -- see `--branch-streams`), `--streams 1` keeps one.  Objects are independent in eval mode, so N GPUs run N replicas on their own batches with no
data-path collective (weak scaling); the only RCCL traffic is the barrier / max-time reduction
around the timed region.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times exactly --steps steps once, writes the last step's outputs if --dump-outputs DIR is
given (DIR/<name>.npy, float32 / float64, at most 64 MB in all) and prints the line: metric, value, unit, ms_per_step,
higher_is_better, dtype, the configuration.  Everything else moves behind --full: the timed region repeated until
--min-seconds have been measured (value from the median region), the roofline objects with the serial eager steps and the
one / two in flight replays they need, and the CPU baseline.

Extra objects in the line (--full):
  roofline      the dominant kernel class (the operand-split GEMMs on the fp16 matrix cores that hold the
                per-point MLPs, 95 % of the FLOPs: hs_proj_kernel / gemm_pp_kernel and the fused heads /
                conv_5 / decoder kernels), timed with HIP events on the launch stream around every one of
                its launches: achieved = algorithmic fp32 FLOPs / time; `per_launch` prices each launch
                at its own bound (MFMA or HBM).  Replayed graphs have no launch to bracket, so the
                events go around serial eager launches of the same steps right after the timed region
                (`roofline.measured` says which).
  cpu_baseline  the CPU oracle (the build's restatement of the reference's torch op sequence,
                oracle/posenet_ref.py mode='torch') timed on this host's cores on a bounded sample.

`--workload train_step` times the reference's trainer step instead (trainer/RL_TDA.py:110-226 as composed by
tgpose_amd.trainer.RL_TDA: net1 with autograd, net2 under no_grad on the augmented cloud, the three consistency
terms, the fourteen-term TDA loss, total, backward, gradient all-reduce, clip, SGD), forward + loss + backward
replayed as one hipGraph.
The timed region is exactly --steps steps between fences; with --full it is repeated until --min-seconds have been
measured and `value` is taken from the median region (`timed_regions` carries min / median / max).
`--workload input_side` times the evaluation loader's input side: `--frames` synthetic depth frames with 6
detections each, resident in HBM, -> (1024,3) clouds (tgp_roi_cloud + tgp_cloud_sample); detections/s, with an HBM roofline
block for roi_cloud_kernel and the numpy port as cpu_baseline.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs x 4 SIMD x 64 FLOP/clk x 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2500.0 # dense bf16 MFMA; the split kernel issues 6 bf16 MFMA terms per fp32 product
B_PER_GPU = 32
N_POINTS = 1028


def synth_batch(B, N, seed):
    """0.1*randn clouds + camera-frame offsets, random categories."""
    g = torch.Generator().manual_seed(seed)
    pts = 0.1 * torch.randn(B, N, 3, generator=g)
    off = torch.rand(B, 1, 3, generator=g) * torch.tensor([0.4, 0.4, 1.0]) + torch.tensor([-0.2, -0.2, 0.5])
    obj = torch.randint(0, 6, (B, 1), generator=g).float()
    return (pts + off).contiguous(), obj


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out, path):
    """--dump-outputs: the arrays a caller of the timed path receives from its last step, as path/<name>.npy -- floating arrays in
    float32 (float64 stays float64), integer and boolean ones in float64 (exact for int32).  Above 64 MB in all, every array is cut
    to the same fraction of its elements by a fixed, seeded choice of flat indices (ascending; the same for the same shapes), and
    <name>.npy holds that flat sample."""
    import numpy as np
    if torch.is_tensor(out):
        named = [("out", out)]
    elif isinstance(out, dict):
        named = list(out.items())
    else:
        named = [("out_%d" % i, t) for i, t in enumerate(out)]
    arrays = {}
    for name, t in named:
        if not torch.is_tensor(t):
            continue
        t = t.detach()
        dt = torch.float64 if (t.dtype == torch.float64 or not t.dtype.is_floating_point) else torch.float32
        arrays[str(name)] = t.to(dt).cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        if total > DUMP_LIMIT_BYTES:
            keep = max(1, int(a.size * (DUMP_LIMIT_BYTES - (1 << 20)) / total))      # (1 MB left for the .npy headers)
            a = a.reshape(-1)[np.sort(np.random.RandomState(0).choice(a.size, size=keep, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def cpu_baseline(sd):
    """SURVEY 8(d) protocol: the oracle forward (the reference's op sequence on torch CPU ops) at B=32, N=1028, eval mode, one
    warm-up + three timed forwards (bounded to ~30 s: fewer timed forwards on a slow host).  The GPU box exposes every host core
    but grants a 16-core share per GPU, so at most 16 threads are used."""
    from oracle import posenet_ref
    threads = max(1, min(os.cpu_count() or 1, 16))
    torch.set_num_threads(threads)
    pts, obj = synth_batch(B_PER_GPU, N_POINTS, 1)
    with torch.no_grad():
        posenet_ref.posenet_forward(sd, pts[:2], obj[:2], mode="torch")           # thread pool, allocator
        t0 = time.perf_counter()
        posenet_ref.posenet_forward(sd, pts, obj, mode="torch")                   # warm-up at full size
        probe = time.perf_counter() - t0
        reps = int(max(1, min(3, 30.0 / max(probe, 1e-3) - 1)))
        t0 = time.perf_counter()
        for _ in range(reps):
            posenet_ref.posenet_forward(sd, pts, obj, mode="torch")
        dt = time.perf_counter() - t0
    return {"value": round(reps * pts.shape[0] / dt, 3), "unit": "objects/s", "cores": threads, "kind": "port",
            "sample": "1 warm-up + %d timed eval forward(s) of B=%d, N=%d on torch %s CPU ops with %d threads (oracle mode='torch': the "
                      "reference's op sequence, bit-identical to the imported reference in the build container), %.1f s timed"
                      % (reps, pts.shape[0], N_POINTS, torch.__version__, threads, dt)}


def _input_side_traffic(D):
    """Memory-side bytes per launch of roi_cloud_kernel from the latest committed PMC passes (per detection x D), or None."""
    try:
        import glob
        k = json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_input_side_pmc_traffic.json")))[-1]))["kernels"]
        k = next(v for n, v in k.items() if "roi_cloud" in n)
        return int(k["bytes_per_launch"] / k["detections_per_launch"] * D)
    except Exception:
        return None


def bench_input_side(args, dev, rank, world, dist, share):
    """a step turns `--frames` depth frames (480x640 uint16) with 6 detections each, already in HBM, into
    (1024,3) clouds: one tgp_roi_cloud launch (a workgroup per detection) + one tgp_cloud_sample launch.  HBM-bound byte
    work; algorithmic bytes per detection = 65536 ROI pixels x (2 B depth + 1 B mask) + 1024 x 12 B out = 208.9 KB."""
    import numpy as np
    from tgpose_amd import ops
    from tgpose_amd.evaluation import load_data_eval as lde
    from tests.util import synth_depth_scene
    per_frame = 6
    frames = [synth_depth_scene(1000 * rank + i, per_frame) for i in range(args.frames)]
    packed = lde.upload(frames, lde.REAL_INTRINSICS, dev)
    D = args.frames * per_frame
    ev = []

    def step(timed=False):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
        if timed:
            e[0].record()
        rr = ops.roi_cloud(*packed, roi_size=256)
        if timed:
            e[1].record()
        out = ops.cloud_sample(rr, 1024, 7)
        if timed:
            e[2].record()
            ev.append(e)
        return out

    def fence():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step(args.full)
    fence()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device="cpu" if share else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(out, args.dump_outputs)
    if rank == 0:
        line = {"metric": "detections/sec depth frame -> cloud (256x256 ROI, 1024 pts)", "value": round(world * D * args.steps / elapsed, 1),
                "unit": "detections/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(1e3 * elapsed / args.steps, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "u16/u8 in, f32 out", "data": "synthetic",
                "config": {"workload": "evaluation loader input side (load_data_eval.py:302-357): %d frames x %d detections per step, "
                                       "frames resident in HBM, device-drawn resampling" % (args.frames, per_frame),
                           "frames": args.frames, "detections": D, "replicas": world}}
    if rank == 0 and args.full:
        k_roi = sum(a.elapsed_time(b) for a, b, _ in ev) * 1e-3 / len(ev)
        k_smp = sum(b.elapsed_time(c) for _, b, c in ev) * 1e-3 / len(ev)
        alg = D * (65536 * 3 + 1024 * 12)
        line["roofline"] = {"bound": "hbm", "achieved": round(alg / k_roi / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                             "frac": round(alg / k_roi / 8e12, 4), "traffic": _input_side_traffic(D), "kernel": "roi_cloud_kernel",
                             "avg_launch_us": round(1e6 * k_roi, 1), "sample_launch_us": round(1e6 * k_smp, 1),
                             "algorithmic_bytes_per_launch": alg,
                             "note": "one workgroup per detection (%d workgroups on 256 CUs), each a chain of 16 + ~8 dependent "
                                     "ordered-compaction rounds: latency- and issue-bound (SQ counters under profiles/), far from the "
                                     "HBM roof by construction; 65536 pixels x ~40 VALU instructions per detection on one CU" % D}
        if world == 1 and not args.no_cpu_baseline:
            from oracle import input_ref as ir
            t1 = time.perf_counter()
            n = 0
            rs = np.random.RandomState(0)
            for fr in frames[:4]:
                ir.image_clouds(fr["depth"], fr["pred_masks"], fr["pred_bboxes"], lde.REAL_INTRINSICS, rng=rs)
                n += per_frame
            dt = time.perf_counter() - t1
            line["cpu_baseline"] = {"value": round(n / dt, 1), "unit": "detections/s", "cores": 1, "kind": "port",
                                    "sample": "%d detections of 4 frames through oracle/input_ref.py (numpy, one thread; the reference's "
                                              "loader runs the same passes per DataLoader worker), %.2f s" % (n, dt)}
    if rank == 0:
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


# algorithmic work per object at N = 1028
GRAPH_CLASS_BYTES = 45.03e6       # graph / HBM class: unique inputs read once + outputs written once
HBM_PEAK = 8.0e12                 # MI355X_MICROARCH.md: HBM3E ~8 TB/s
FP16_MFMA_PEAK = 2500.0e12        # dense fp16 / bf16 MFMA


def _latest_profile(pattern, skip=("input_side",)):
    import glob
    files = [f for f in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern))) if not any(s in f for s in skip)]
    return files[-1] if files else None


# Algorithmic bytes per launch (B = 32, N = 1028) of the kernels that serve ONE shape per forward: unique inputs read once + outputs
# written once (SURVEY.md 8d's rule), fp32 unless noted.  Kernels that serve several shapes (the tile GEMMs) carry no single figure.
# Keys are PREFIXES of the profiler's kernel names (template arguments that do not change the shape are left out).
ALGO_BYTES_B32 = {
    # fine (32896 x 272) + the heads' columns of both coarse products (8224 + 2048 rows x 3072) + fp16 weight planes
    # (3 x 1024 x 272 + 3 x 256 x 1024, two planes) + keys: 35.8 + 101.1 + 25.2 + 6.5 MB
    "void heads_fused_kernel": 35.8e6 + 101.1e6 + 25.2e6 + 6.5e6,
    # fine + conv_5's 1024 columns of the coarse products + weights: 35.8 + 33.7 + 8.4 + 1.1 MB
    "void conv_max_fused_kernel": 35.8e6 + 33.7e6 + 8.4e6 + 1.1e6,
    # the first decoder conv's activation as planes (32896 x 512 x 4 B), the three inner weights, the rows out + their map
    "dec_fused_kernel": 67.4e6 + 1.7e6 + 0.4e6 + 0.3e6,
    # fine + the decoder's 512 columns of the coarse products (8224 + 2048 rows) + weight planes + the activation out as fragments
    "dec_l1_kernel": 35.8e6 + 16.8e6 + 4.2e6 + 0.6e6 + 67.4e6,
    # the projection kernel serves two launches per forward and instance (operand planes + weight + result, 4 B per element): their mean
    "void hs_proj_kernel<8>": 0.5 * (169.0e6 + 81.1e6),                        # conv_1 (32896 x 1152 x 128), conv_2 (8224 x 2304 x 128)
    "void hs_proj_kernel<16>": 0.5 * (86.6e6 + 45.1e6),                        # conv_3 (8224 x 2304 x 256), conv_4 (2048 x 4608 x 256)
    "void hs_proj_kernel<32>": 0.5 * (177.9e6 + 51.4e6),                       # the coarse products (8224 / 2048 x 4608 x 512)
    "void gconv_kernel<128, false>": 4.83e6 * 32,       # conv_1's graph convolution, SURVEY 8d: 4.83 MB per object
    "void gconv_kernel<128, true>": 0.62e6 * 32,        # conv_0
    # conv_2 / conv_3 (n = 257, C = 256): centre + 7 support blocks of the projection (8224 x 2048 x 4 B), directions, lists, output
    "void gconv_lds_kernel<8>": 67.4e6 + 2.6e6 + 0.7e6 + 8.4e6,
    "void gconv_lds_kernel<16>": 33.6e6 + 0.3e6 + 4.2e6,                      # conv_4 (n = 64, C = 512)
    # five launches per forward (n = 1028 C = 128 twice, n = 257 C = 256 twice, n = 64 C = 512): table in, lists in, table out as planes;
    # their mean: (2 x 36.3 + 2 x 17.5 + 8.5) / 5 MB
    "orl_lds_kernel": 23.2e6,
    "void knn_feat_fused16_kernel<128, 17": 0.61e6 * 32,                      # conv_1's feature-space graph, SURVEY 8d: 0.61 MB per object
    "void knn_feat_fused16_kernel<256, 5": 0.28e6 * 32,                       # conv_3 (n = 257, d = 256)
    "void knn_feat_fused16_kernel<128, 5": 0.15e6 * 32,                       # conv_2 (n = 257, d = 128)
    "void knn_feat_fused16_kernel<256, 1": 0.07e6 * 32,                       # conv_4 (n = 64, d = 256)
    "void knn_feat_fused_kernel<128, 17, 8>": 0.61e6 * 32,
    "void knn_xyz_kernel<17>": 0.10e6 * 32,
}


def _algo_bytes(kernel_name):
    best = None
    for k, v in ALGO_BYTES_B32.items():
        if kernel_name.startswith(k) and (best is None or len(k) > len(best[0])):
            best = (k, v)
    return best[1] if best else None


# Compute floors of the graph / HBM class (B = 32, N = 1028), for the compute-aware bound beside the HBM one:
#   * feature-space kNN: the distance products must be exact fp32 in ascending k (bit-exact lists): v_mfma_f32_16x16x4_f32 at the
#     fp32 matrix peak 157.3 TFLOP/s; SURVEY 8d: 273.7 + 17.1 + 34.0 + 2.1 MFLOP per object;
#   * graph convolutions: relu(dir . support_dir) * support, max, mean on the vector pipes at the fp32 vector peak 157.3 TFLOP/s;
#     147.4 + 165.8 + 82.9 + 82.9 + 16.5 MFLOP per object (the formula's FLOPs: the instruction count is higher);
#   * everything else of the class (ORL pooling, pooling, up-sampling, gathers, sorts): HBM.
GRAPH_KNN_FLOP, GRAPH_KNN_BYTES = (273.7 + 17.1 + 34.0 + 2.1) * 1e6, (0.61 + 0.15 + 0.28 + 0.07) * 1e6
GRAPH_GCONV_FLOP, GRAPH_GCONV_BYTES = (147.4 + 165.8 + 82.9 + 82.9 + 16.5) * 1e6, (0.62 + 4.83 + 2.39 + 2.39 + 1.18) * 1e6
PEAK_F32_VECTOR = 157.3e12


def _kernel_traffic(gemm_algo=None):
    """Per-kernel HBM-side traffic from the latest COMMITTED PMC passes (FETCH_SIZE / WRITE_SIZE in separate rocprofv3 --pmc runs,
    corrected as MI355X_MICROARCH.md prescribes: bytes = (2 FETCH + WRITE) KB; scripts/pmc_traffic.py) -- not a measurement of this
    run, and labelled so in the line.  -> ([{kernel, launches, bytes_per_launch, algorithmic_bytes_per_launch, ratio}], source).
    gemm_algo = (launches per forward, algorithmic bytes per forward) of the tile-GEMM launches this run timed: the tile GEMM kernels
    serve many shapes each, so they get ONE family row -- the PMC bytes of every gemm_pp / gemm_split kernel per forward against the
    algorithmic bytes of the forward's tile-GEMM launches."""
    try:
        path = _latest_profile("r*_pmc_traffic.json")
        pmc = json.load(open(path))["kernels"]
        rows = []
        fam = [(k, v) for k, v in pmc.items() if "gemm_pp_kernel" in k or "gemm_split" in k]
        if fam and gemm_algo and gemm_algo[0]:
            fwd = max(1, round(sum(v["launches"] for _, v in fam) / gemm_algo[0]))            # forwards in the PMC passes
            per_fwd = sum(v["launches"] * v["bytes_per_launch_corrected"] for _, v in fam) / fwd
            rows.append({"kernel": "tile GEMM family (every gemm_pp_kernel<*> / gemm_split*_kernel launch of a forward)",
                         "launches": int(gemm_algo[0]), "bytes_per_launch": int(per_fwd / gemm_algo[0]),
                         "algorithmic_bytes_per_launch": int(gemm_algo[1] / gemm_algo[0]), "ratio": round(per_fwd / gemm_algo[1], 2)})
        for k, v in pmc.items():
            if "at::native" in k or "rocclr" in k or v["bytes_per_launch_corrected"] < 2e6:
                continue
            algo = _algo_bytes(k)
            rows.append({"kernel": k, "launches": v["launches"], "bytes_per_launch": v["bytes_per_launch_corrected"],
                         "algorithmic_bytes_per_launch": int(algo) if algo else None,
                         "ratio": round(v["bytes_per_launch_corrected"] / algo, 2) if algo else None})
        rows.sort(key=lambda r: -r["bytes_per_launch"] * r["launches"])
        return rows, os.path.relpath(path, ROOT)
    except Exception:
        return None, None


def train_batch(B, N, seed):
    """the trainer's batch dict (datasets/load_data.py:313-349) on BASELINE config 3/4's workload: the six obj_model category
    clouds with their pdh1 / pdh2 priors (data recorded in tests/golden/category_clouds.npz), posed, scaled and sampled to N"""
    import numpy as np
    from tests.util import synth_train_db
    gc = np.load(os.path.join(ROOT, "tests", "golden", "category_clouds.npz"))
    return synth_train_db(torch.from_numpy(gc["points_category"]), torch.from_numpy(gc["pdh1_category"]),
                          torch.from_numpy(gc["pdh2_category"]), gc["sym"].astype(int).tolist(), [i % 6 for i in range(B)], N, seed)


def rank_env(rank, world, port, base=None):
    """environment of rank `rank` of a one-node job of `world` ranks (what torch.distributed.run would set)"""
    env = dict(os.environ if base is None else base)
    env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL between processes needs it on this driver
    return env


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(world, argv=None, cmd=None, poll=0.2):
    """`python bench.py --gpus N` typed as it stands: start the N ranks as CHILD processes (never an exec: the parent has not touched
    the GPU and never will), one per GPU, wait for them, relay rank 0's standard output (the JSON line) and return 0, or the first
    non-zero exit code -- the other ranks are then terminated, so a rank that died cannot leave the rest waiting in a collective."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv) if cmd is None else list(cmd)
    port = free_port()
    procs = []
    for r in range(world):
        procs.append(subprocess.Popen(cmd, env=rank_env(r, world, port), stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    rc, out0 = 0, []
    import threading
    reader = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()))     # (drained while waiting: a full pipe would block rank 0)
    reader.start()
    live = set(range(world))
    while live and rc == 0:
        for r in sorted(live):
            code = procs[r].poll()
            if code is not None:
                live.discard(r)
                if code != 0:
                    rc = code
                    sys.stderr.write("bench.py: rank %d exited with code %d; stopping the other ranks\n" % (r, code))
                    break
        if live and rc == 0:
            time.sleep(poll)
    for r in live:                       # only after a failure: exactly the children started above
        procs[r].terminate()
    for r in live:
        try:
            procs[r].wait(timeout=20)
        except subprocess.TimeoutExpired:
            procs[r].kill()
            procs[r].wait()
    reader.join()
    if rc == 0:
        sys.stdout.write(b"".join(out0).decode())
        sys.stdout.flush()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=B_PER_GPU, help="objects per GPU per step")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: repeated timed regions (--min-seconds), the roofline "
                         "objects, the one / two in flight figures and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--min-seconds", type=float, default=1.0,
                    help="--full: the timed region (exactly --steps steps between fences) is repeated until this much time has been "
                         "measured; the line reports the median region and the spread")
    ap.add_argument("--streams", type=int, default=4,
                    help="batches in flight per GPU: step i runs on HIP stream i %% S over its own batch (independent batches "
                         "overlap each other's tail rounds and small kernels); 1 = one forward at a time")
    ap.add_argument("--branch-streams", choices=("auto", "on", "off"), default="auto",
                    help="side branches inside a forward (feature-space kNN beside the projection GEMM, PH tail + decoder beside the "
                         "heads).  hipGraph runs a graph's extra branches on ONE pool of internal streams per device, shared by every "
                         "graph in flight, so the branches of concurrent replays queue behind each other: with three or more batches "
                         "in flight branch-free (linear) graphs are faster (profiles/r03_streams_ab.txt).  auto: on up to 2 in flight")
    ap.add_argument("--no-branch-streams", action="store_true", help="same as --branch-streams off")
    ap.add_argument("--gemm", choices=("split16", "split", "fp32"), default="split16",
                    help="split16: fp32-accurate GEMM on the fp16 matrix cores (2-term operand split, 3 MFMA terms); "
                         "split: the same on the bf16 matrix cores (3-term split, 6 MFMA terms, full fp32 range); "
                         "fp32: v_mfma_f32_32x32x2_f32 kernels")
    ap.add_argument("--graph", type=int, choices=(0, 1, 2), default=1,
                    help="replay the forward as a captured hipGraph (default 1 = whole batch; 0 = eager launches; "
                         "2 = two half batches on forked streams, measured slower)")
    ap.add_argument("--frames", type=int, default=32, help="input_side: frames per step (6 detections each)")
    ap.add_argument("--eval-outputs-only", action="store_true",
                    help="forward: skip the PH predictor and the decoder, whose results the six-key eval dict does not return "
                         "(engine.EVAL_OUTPUTS_ONLY; a secondary, deployment figure -- the headline is the full forward)")
    ap.add_argument("--workload", choices=("forward", "train_step", "input_side"), default="forward",
                    help="forward: the headline metric (eval-mode forward).  train_step: BASELINE config 4's step on one rank's "
                         "share -- the reference's RL_TDA_train_step (net1 with gradients, net2 under no_grad on the augmented cloud, "
                         "three consistency terms, fourteen TDA terms, total as trainer/RL_TDA.py:214), backward, gradient all-reduce "
                         "over the ranks, clip, optimizer step; objects/s of whole steps.  input_side: SURVEY 8 f-4 -- depth frames "
                         "+ detection masks resident in HBM -> (1024,3) clouds; detections/s")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            # typed without a launcher: this process becomes the launcher (nothing above has touched the GPU)
            raise SystemExit(self_launch(args.gpus))
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    # TGP_BENCH_SHARE_GPU=1 is a rehearsal mode for a one-GPU box: every rank uses cuda:0 and the control plane
    # (barrier, max-time reduction) runs over gloo, because RCCL refuses two ranks on one device.
    share = os.environ.get("TGP_BENCH_SHARE_GPU") == "1"
    dev_index = 0 if share else local_rank
    if dev_index >= torch.cuda.device_count():
        raise SystemExit("rank %d: no cuda:%d on this node (%d GPUs visible)" % (rank, dev_index, torch.cuda.device_count()))
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    if args.workload == "input_side":
        return bench_input_side(args, dev, rank, world, dist, share)

    import tgpose_amd
    from tgpose_amd import PoseNet9D, FLAGS, ops, seeded_state_dict
    from tgpose_amd import engine as _engine
    sd = seeded_state_dict(0)
    ops.GEMM_MODE = args.gemm
    if args.no_branch_streams:
        args.branch_streams = "off"
    _engine.BRANCH_STREAMS = args.branch_streams == "on" or (args.branch_streams == "auto" and (args.streams <= 2 or args.workload != "forward"
                                                                                                  or args.graph != 1))
    _engine.EVAL_OUTPUTS_ONLY = bool(args.eval_outputs_only)      # (never from the environment: the default line is the full forward)
    B = args.batch
    torch.manual_seed(rank)
    step_no = [0]
    replayers, one_in_flight, two_in_flight, trainer = None, None, None, None
    streams = [torch.cuda.Stream(device=dev) for _ in range(args.streams)] if (args.streams > 1 and args.workload == "forward") else [None]

    if args.workload == "forward":
        net = PoseNet9D()
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        FLAGS.train = 0
        pts, obj = synth_batch(B, N_POINTS, 100 + rank)
        pts, obj = pts.to(dev), obj.to(dev)

        def step():
            st = streams[step_no[0] % len(streams)]
            step_no[0] += 1
            if st is None:
                return net(pts, obj)
            with torch.cuda.stream(st):
                return net(pts, obj)

        if args.graph == 1 and args.streams == 1:
            net.graph_replay = True                 # PoseNet9D.forward captures once, then replays
        elif args.graph == 1:
            # S batches in flight: one captured forward (own static buffers, own activation pool) per HIP stream; step i replays
            # graph i % S on stream i % S over its own batch, so one batch's tail rounds and small kernels overlap the other's
            # GEMMs.  Every step is still one whole forward of B objects; a batch's latency is S steps.
            batches = [tuple(t.to(dev) for t in synth_batch(B, N_POINTS, 100 + rank + 1000 * i)) for i in range(len(streams))]
            replayers = [_engine.GraphedForward(net.packed(dev), B, N_POINTS, dev, train_keys=False) for _ in streams]
            for st in streams:
                st.wait_stream(torch.cuda.current_stream(dev))

            def step():
                i = step_no[0] % len(streams)
                step_no[0] += 1
                with torch.cuda.stream(streams[i]):
                    return replayers[i](*batches[i])
        elif args.graph == 2:
            graphed = _engine.GraphedForward(net.packed(dev), B, N_POINTS, dev, train_keys=False, parts=2)

            def step():
                return graphed(pts, obj)
    else:
        # the reference's trainer step (trainer/RL_TDA.py:110-226) composed by tgpose_amd.trainer.RL_TDA on the category-cloud
        # workload; dropout active as in the trainer (net.train()); SGD stands in for Ranger (optimizer zoo: out of scope)
        from tgpose_amd.trainer.RL_TDA import RT_TDA_Trainer
        trainer = RT_TDA_Trainer(device=dev)
        trainer.init_network('RL_TDA')
        trainer.init_loss()
        trainer.net1.load_state_dict(sd, strict=True)
        trainer.net2.load_state_dict(seeded_state_dict(1, only_encoder=True), strict=True)
        trainer.net1.train(), trainer.net2.train()
        trainer.optimizer = torch.optim.SGD(trainer.net1.parameters(), lr=1e-5, momentum=0.9)
        net = trainer.net1
        db = {k: v.to(dev) for k, v in train_batch(B, N_POINTS, 7 + rank).items()}
        if args.graph:
            # both forwards + losses + backward replayed as one hipGraph; the collective, the clip and the optimizer step stay eager
            # (two graphs split at the encoder's output: the late layers' gradient bucket is exchanged while the encoder's backward runs)
            graphed_step = trainer.graphed_step(db, overlap=True)

            def step():
                loss = graphed_step()
                # total=loss: the reference loop's per-iteration NaN test (trainer/RL_TDA.py:217-220) with its host read of the loss is
                # part of the step, as in the reference (round-3 advisor: it was left out of the timed step)
                trainer.finish_step(total=loss)
                return loss
        else:
            def step():
                return trainer.train_iteration(db)[0]

    def fence():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    last = [None]                  # what the last timed step returned (--dump-outputs)

    def timed_region():
        """exactly --steps steps between fences; max over ranks"""
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last[0] = step()
        fence()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], device="cpu" if share else dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    for _ in range(max(args.warmup, len(streams))):
        step()
    ops.GEMM_TIMER = [] if args.full and replayers is None and not getattr(net, "graph_replay", False) and not (trainer and args.graph) else None
    regions = [timed_region()]
    timer, ops.GEMM_TIMER = ops.GEMM_TIMER, None
    # the same region again until --min-seconds have been measured (every rank takes the same decision: the times are reduced)
    while args.full and sum(regions) < args.min_seconds and len(regions) < 200:
        regions.append(timed_region())
    regions_sorted = sorted(regions)
    elapsed = regions_sorted[len(regions) // 2] if len(regions) % 2 else 0.5 * (regions_sorted[len(regions) // 2 - 1] + regions_sorted[len(regions) // 2])
    if rank == 0 and args.dump_outputs:
        dump_outputs(last[0], args.dump_outputs)

    # ---- roofline block: per-kernel durations need serial launches (graph replays have no launch to bracket, overlapping
    # streams stretch each other's kernels): the same steps once more as serial eager launches on one stream, HIP events
    # around every tile-kernel launch and every launch of the graph / HBM class
    roof_note = "HIP events around every tile-kernel launch of the timed region (eager launches)"
    graph_cls, roof_elapsed, k_roof = None, regions[0], args.steps
    if args.full and timer is None:
        branch, _engine.BRANCH_STREAMS = _engine.BRANCH_STREAMS, False
        replay_flag = getattr(net, "graph_replay", False)
        net.graph_replay = False
        if trainer is not None:
            def roof_step():
                return trainer.train_iteration(db)[0]
        else:
            def roof_step():
                return net(pts, obj)
        k_roof = min(args.steps, 10)
        roof_step()
        fence()
        ops.GEMM_TIMER, ops.CLASS_TIMER = [], {}
        t1 = time.perf_counter()
        for _ in range(k_roof):
            roof_step()
        fence()
        roof_elapsed = time.perf_counter() - t1
        timer, ops.GEMM_TIMER = ops.GEMM_TIMER, None
        graph_cls, ops.CLASS_TIMER = ops.CLASS_TIMER.get("graph", []), None
        _engine.BRANCH_STREAMS, net.graph_replay = branch, replay_flag
        roof_note = ("HIP events around every tile-kernel launch of %d serial eager steps (one stream, no side branches) run after the "
                     "timed region%s" % (k_roof, "" if replayers is None else " (%d graph replays in flight there)" % len(streams)))
        if replayers is not None:
            # for reference: the same replayed forward with ONE batch in flight (what a latency-bound caller sees) -- captured with
            # its side branches, which is the faster form when nothing else is in flight
            solo = replayers[0]
            if not branch:
                _engine.BRANCH_STREAMS = True
                solo = _engine.GraphedForward(net.packed(dev), B, N_POINTS, dev, train_keys=False)
                _engine.BRANCH_STREAMS = branch
            with torch.cuda.stream(streams[0]):
                for _ in range(3):
                    solo(*batches[0])
            fence()
            t2 = time.perf_counter()
            with torch.cuda.stream(streams[0]):
                for _ in range(args.steps):
                    solo(*batches[0])
            fence()
            one_in_flight = world * B * args.steps / (time.perf_counter() - t2)
            # ... and with TWO branched replays in flight, the bench's default until round 2: keeps rounds comparable across the
            # change of default (round-3 advisor)
            if len(streams) >= 2 and len(batches) >= 2:
                _engine.BRANCH_STREAMS = True
                pair = [solo, _engine.GraphedForward(net.packed(dev), B, N_POINTS, dev, train_keys=False)]
                _engine.BRANCH_STREAMS = branch
                for i in range(4):
                    with torch.cuda.stream(streams[i % 2]):
                        pair[i % 2](*batches[i % 2])
                fence()
                t3 = time.perf_counter()
                for i in range(args.steps):
                    with torch.cuda.stream(streams[i % 2]):
                        pair[i % 2](*batches[i % 2])
                fence()
                two_in_flight = world * B * args.steps / (time.perf_counter() - t3)
                del pair

    if rank == 0 and args.full:
        tile = [t for t in timer if len(t) > 6 and t[6] == "tile"]
        traffic, traffic_src = _kernel_traffic((len(tile) / max(k_roof, 1), sum(t[5] for t in tile) / max(k_roof, 1)) if tile and args.workload == "forward" else None)
        launches = len(timer)
        ksec = sum(e0.elapsed_time(e1) for e0, e1, *_ in timer) * 1e-3
        kflop = sum(f for _, _, f, *_ in timer)
        kflop_ref = sum(t[4] for t in timer)
        achieved = kflop / ksec / 1e12 if ksec > 0 else 0.0
        if args.gemm == "split":
            kernel_name = "gemm_split_kernel"
            peak = PEAK_BF16_MFMA_TFLOPS / 6.0
            peak_basis = ("algorithmic fp32 FLOPs; each fp32 product costs 6 bf16 MFMA terms (3-term operand split), so "
                          "the bound is the dense bf16 MFMA peak 2500 TFLOP/s / 6; for scale, the fp32 MFMA peak is 157.3")
        elif args.gemm == "split16":
            kernel_name = ("the fp16-split MFMA class of the forward: hs_proj_kernel<*> (projections, coarse products) / gemm_pp_kernel<*> "
                           "(the layers' last GEMMs; both operands as fp16 planes) / heads_fused_kernel / conv_max_fused_kernel / "
                           "dec_l1_kernel / dec_fused_kernel: the same 3-term fp16 MFMA arithmetic")
            peak = PEAK_BF16_MFMA_TFLOPS / 3.0
            peak_basis = ("algorithmic fp32 FLOPs; each fp32 product costs 3 fp16 MFMA terms (2-term operand split), so the "
                          "bound is the dense fp16 MFMA peak 2500 TFLOP/s / 3; for scale, the fp32 MFMA peak is 157.3")
        else:
            kernel_name = "gemm_main256_kernel / gemm_main_kernel"
            peak = PEAK_F32_MFMA_TFLOPS
            peak_basis = "fp32 MFMA (v_mfma_f32_32x32x2_f32) dense peak"
    if rank == 0:
        per_step = [1e3 * r / args.steps for r in regions]
        fwd = args.workload == "forward"
        line = {
            "metric": ("objects/sec forward (B=%d, N=%d pts)" % (B, N_POINTS) if fwd
                       else "objects/sec training step (forward x2 + loss + backward + optimizer, B=%d, N=%d pts)" % (B, N_POINTS)),
            "value": round(world * B * args.steps / elapsed, 2),
            "unit": "objects/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "timed_regions": {"count": len(regions), "steps_each": args.steps, "value_from": "median region",
                              "ms_per_step_min": round(min(per_step), 4), "ms_per_step_median": round(1e3 * elapsed / args.steps, 4),
                              "ms_per_step_max": round(max(per_step), 4), "total_s": round(sum(regions), 3)},
            "gemm_mode": {"split": "fp32-accurate 3xbf16 operand split on the bf16 matrix cores, fp32 accumulate",
                          "split16": "fp32-accurate 2xfp16 operand split on the fp16 matrix cores, fp32 accumulate",
                          "fp32": "fp32 MFMA"}[args.gemm],
            "config": {"workload": (("PoseNet9D.forward eval mode, full forward (kNN graphs + 3D-GCN encoder + PH predictor "
                                     "+ decoder + R/t/s heads), B=%d objects per GPU, N=%d points, seeded random weights "
                                     "of the reference architecture (27.43 M params)" % (B, N_POINTS)) if not args.eval_outputs_only else
                                    ("PoseNet9D.forward eval mode WITHOUT the PH predictor and the decoder, whose results the six-key "
                                     "eval dict does not return (reduced set: -4,968 MFLOP, -41.5 MB per object against SURVEY 8d's "
                                     "full-forward figures; NOT the headline configuration), B=%d objects per GPU, N=%d points, seeded "
                                     "random weights" % (B, N_POINTS))) if fwd
                       else ("the reference's RL_TDA_train_step (trainer/RL_TDA.py:110-226): net1 = PoseNet9D training-mode forward "
                             "with autograd, net2 = PoseNet9D(only_encoder) under no_grad on the augmented cloud, feat_consistency + 2x "
                             "prop_sym_matching, the 14 control_loss('TDA') terms, total = 0.1 (con + recon_1 + recon_cons) + 0.9 sum(TDA), "
                             "backward in two captured segments with the bucketed gradient exchange (reduce-scatter + all-gather) overlapping the second, "
                             "clip_grad_norm_(5), SGD step; B=%d objects per GPU, N=%d points sampled "
                             "from the six obj_model category clouds with their pdh1/pdh2 priors" % (B, N_POINTS)),
                       "objects_per_gpu": B, "points": N_POINTS, "replicas": world, "batches_in_flight": len(streams),
                       "full_forward": not (fwd and args.eval_outputs_only),
                       "side_branches_in_a_forward": bool(_engine.BRANCH_STREAMS),
                       **({} if fwd else {"nan_test_in_step": True}),
                       "hipgraph": {0: "off", 1: "whole batch" if replayers is None else "whole batch, one captured forward per stream",
                                    2: "two half batches on forked streams"}[args.graph]},
        }
        if args.full:
            line["roofline"] = {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                                "frac": round(achieved / peak, 4), "traffic": traffic,
                                "traffic_source": (traffic_src + " (committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over serial eager "
                                                                 "forwards of this workload, per kernel and launch, bytes = (2 FETCH + WRITE) KB; "
                                                                 "algorithmic bytes where a kernel serves one shape; not measured by this run)")
                                if traffic_src else None,
                                "kernel": kernel_name, "peak_basis": peak_basis,
                                "launches_timed": launches, "avg_launch_us": round(1e6 * ksec / max(launches, 1), 2),
                                "share_of_step": round(ksec / roof_elapsed, 4), "measured": roof_note}
        #  the same launches priced one by one at THEIR roof: a launch is bound by
        # max(executed FLOPs / MFMA roof of the GEMM mode, algorithmic bytes / HBM peak) -- the layers' last GEMMs (N = K = 128) and the
        # K = 128 projections are HBM-bound launches that the class-wide "mfma" fraction above prices on the wrong roof
        priced = [t for t in timer if len(t) > 5 and t[5]] if args.full else []
        if priced and ksec > 0:
            roof = peak * 1e12
            b_mfma = [t[2] / roof for t in priced]
            b_hbm = [t[5] / HBM_PEAK for t in priced]
            bound = sum(max(a, b) for a, b in zip(b_mfma, b_hbm))
            psec = sum(t[0].elapsed_time(t[1]) for t in priced) * 1e-3
            n_hbm = sum(1 for a, b in zip(b_mfma, b_hbm) if b > a)
            line["roofline"]["per_launch"] = {
                "frac": round(bound / psec, 4), "launches_priced": len(priced), "of_them_hbm_bound": n_hbm,
                "bound_us_per_forward": round(1e6 * bound / max(k_roof, 1), 1), "measured_us_per_forward": round(1e6 * psec / max(k_roof, 1), 1),
                "hbm_bound_launches_us_per_forward": round(1e6 * sum(t[0].elapsed_time(t[1]) * 1e-3 for t, a, b in zip(priced, b_mfma, b_hbm) if b > a) / max(k_roof, 1), 1),
                "basis": "per launch max(executed FLOPs / %.0f TFLOP/s, algorithmic bytes / 8 TB/s), summed, over the summed launch times "
                         "(tile GEMMs: A + W + result(s) + residuals once; fused kernels: their operands once)" % peak}
        if args.full and kflop_ref != kflop and ksec > 0:
            # the layers over the concat buffer run factored over the nearest-neighbour upsampling (DESIGN.md "Factored wide
            # layers"): `achieved` counts the FLOPs the kernels execute; for comparison, the same time priced in the FLOPs of
            # the reference's formulation (W x upsampled copies)
            line["roofline"]["flops_counted"] = "executed (factored formulation)"
            line["roofline"]["executed_over_reference_formulation_flops"] = round(kflop / kflop_ref, 4)
            line["roofline"]["rate_in_reference_formulation_flops"] = round(kflop_ref / ksec / 1e12, 2)
        if fwd and graph_cls:
            # second class: the graph / HBM-bound kernels (45.03 MB of unique traffic per object) and the bound of the
            # whole path as it now executes: executed dense FLOPs at the split kernels' roof + the graph class at HBM speed
            gsec = sum(e0.elapsed_time(e1) for e0, e1, _ in graph_cls) * 1e-3 / k_roof            # per forward
            ach = GRAPH_CLASS_BYTES * B / gsec
            line["roofline_graph_class"] = {
                "bound": "hbm", "achieved": round(ach / 1e9, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": round(ach / HBM_PEAK, 4),
                "algorithmic_bytes_per_object": GRAPH_CLASS_BYTES, "ms_per_forward": round(1e3 * gsec, 4), "launches_per_forward": len(graph_cls) // k_roof,
                "kernels": "kNN (xyz + feature space incl. the distance GEMM), graph convolution, ORL pooling, pooling, gathers, "
                           "row sort, tails, per-object post-processing; serial launches as for `roofline`"}
            # compute-aware bound of the class (item 7): the exact-fp32 distance products of the feature-space kNN on the fp32 matrix
            # peak, the graph convolutions' formula on the fp32 vector peak, the rest at HBM speed
            rest_bytes = GRAPH_CLASS_BYTES - GRAPH_KNN_BYTES - GRAPH_GCONV_BYTES
            cb = B * (max(GRAPH_KNN_FLOP / (PEAK_F32_MFMA_TFLOPS * 1e12), GRAPH_KNN_BYTES / HBM_PEAK)
                      + max(GRAPH_GCONV_FLOP / PEAK_F32_VECTOR, GRAPH_GCONV_BYTES / HBM_PEAK) + rest_bytes / HBM_PEAK)
            line["roofline_graph_class"]["compute_aware"] = {
                "bound_ms_per_forward": round(1e3 * cb, 4), "frac": round(cb / gsec, 4),
                "basis": "feature-space kNN: %.0f MFLOP per object of exact fp32 MFMA at 157.3 TFLOP/s; graph convolutions: %.0f MFLOP per object "
                         "at the fp32 vector peak 157.3 TFLOP/s; the other %.1f MB per object at 8 TB/s"
                         % (GRAPH_KNN_FLOP / 1e6, GRAPH_GCONV_FLOP / 1e6, rest_bytes / 1e6)}
            flop_fwd = kflop / k_roof
            mfma_roof = {"split16": FP16_MFMA_PEAK / 3.0, "split": FP16_MFMA_PEAK / 6.0, "fp32": PEAK_F32_MFMA_TFLOPS * 1e12}[args.gemm]
            bound_s = flop_fwd / mfma_roof + GRAPH_CLASS_BYTES * B / HBM_PEAK
            line["roofline_path"] = {
                "bound_ms_per_step": round(1e3 * bound_s, 4), "measured_ms_per_step": round(1e3 * elapsed / args.steps, 4),
                "frac": round(bound_s / (elapsed / args.steps), 4),
                "basis": "executed tile-kernel FLOPs per forward (%.1f GFLOP) / MFMA roof of the GEMM mode + %.0f MB x %d objects / 8 TB/s"
                         % (flop_fwd / 1e9, GRAPH_CLASS_BYTES / 1e6, B)}
        if one_in_flight is not None:
            line["config"]["objects_per_s_one_batch_in_flight"] = round(one_in_flight, 1)     # this rank's clock, not max-over-ranks
        if two_in_flight is not None:
            line["config"]["objects_per_s_two_batches_in_flight"] = round(two_in_flight, 1)   # (two branched replays: the default of rounds 1-2)
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(sd)
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
