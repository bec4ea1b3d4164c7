"""Cost of the gradients with respect to the points (B = 32, N = 1028, device events, medians):
  eval_fwd_bwd      eval-mode forward + backward to a cloud that requires grad (the six-key outputs)
  train_bwd_plain   training-mode backward, cloud without requires_grad
  train_bwd_points  the same with points.requires_grad (the extra kernels of csrc/xyz_bwd.hip); alternated with the plain run
Writes JSON to the path given (default profiles/xyz_grad_time.json).  Per-kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/xyz_grad_time.py --quick
then `python scripts/xyz_grad_time.py --merge-trace OUT [json]` adds the new kernels' dispatch statistics from the trace database
(OUT/**/*.db) to the JSON as "kernel_trace" (the committed profile was assembled this way)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


KERNELS = ["gconv_dirgrad_kernel", "dirs_to_xyz_kernel", "center_bwd_kernel", "bn_eval_bwd_kernel", "bn_eval_finish_kernel",
           "bn_eval_bwd_pooled_kernel", "neighbor_dirs_kernel"]


def merge_trace(trace_dir, json_path):
    """per-kernel dispatch statistics (us) of the new kernels from a rocprofv3 --kernel-trace database into the profile JSON"""
    import glob
    import sqlite3
    import statistics
    db = sorted(glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True))[0]
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info('rocpd_info_kernel_symbol')")]
    name = "kernel_name" if "kernel_name" in cols else "display_name"
    rows = c.execute("select s.%s, d.end - d.start from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id"
                     % name).fetchall()
    stats = {}
    for kname, dur in rows:
        for w in KERNELS:
            if w in kname:
                key = w + ("<HS>" if "ILb1E" in kname else "<surface>" if "ILb0E" in kname else "")
                stats.setdefault(key, []).append(dur / 1000.0)
    per = {k: {"calls": len(v), "total_us": round(sum(v), 1), "median_us": round(statistics.median(v), 1), "max_us": round(max(v), 1)}
           for k, v in sorted(stats.items())}
    with open(json_path) as f:
        res = json.load(f)
    res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, scripts/xyz_grad_time.py --quick in a run of its own: 4 eval-mode "
                           "and 4 training-mode forward + backward passes with points.requires_grad (the eval BatchNorm kernels run in "
                           "the eval passes only)", "per_kernel": per}
    with open(json_path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    from tgpose_amd import FLAGS, PoseNet9D, seeded_state_dict
    if "--merge-trace" in sys.argv:
        i = sys.argv.index("--merge-trace")
        rest = sys.argv[i + 2:]
        merge_trace(sys.argv[i + 1], rest[0] if rest else os.path.join(ROOT, "profiles", "xyz_grad_time.json"))
        return
    quick = "--quick" in sys.argv
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles", "xyz_grad_time.json"))
    dev, B, N = "cuda:0", 32, 1028
    reps = 3 if quick else 15
    net = PoseNet9D()
    net.load_state_dict(seeded_state_dict(0))
    net = net.to(dev)
    g = torch.Generator().manual_seed(0)
    pts = (0.1 * torch.randn(B, N, 3, generator=g) + torch.tensor([0.1, -0.1, 0.9])).to(dev)
    obj = (torch.arange(B) % 6).float().view(B, 1).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def eval_step():
        x = pts.clone().requires_grad_(True)
        out = net(x, obj)
        sum(v.sum() for v in out.values()).backward()

    res = {"B": B, "N": N, "reps": reps, "ms": {}}
    net.eval()
    FLAGS.train = 0
    eval_step()
    res["ms"]["eval_fwd_bwd"] = sorted(timed(eval_step) for _ in range(reps))[reps // 2]
    net.train()
    FLAGS.train = 1
    plain, withp = [], []
    try:
        for i in range(reps + 1):
            for req, acc in ((False, plain), (True, withp)):
                x = pts.clone().requires_grad_(req)
                net.zero_grad(set_to_none=True)
                out = net(x, obj)
                loss = sum(v.square().mean() for v in out.values())
                t = timed(loss.backward)
                if i:
                    acc.append(t)
    finally:
        FLAGS.train = 0
    res["ms"]["train_bwd_plain"] = sorted(plain)[len(plain) // 2]
    res["ms"]["train_bwd_points"] = sorted(withp)[len(withp) // 2]
    res["ms"]["train_bwd_points_minus_plain"] = res["ms"]["train_bwd_points"] - res["ms"]["train_bwd_plain"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if not quick:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
