"""Times the fused Ranger step (tgp_ranger_step, csrc/ranger.hip) over net1's parameters and sets it against its byte bound, a
torch-eager statement of the same algorithm, and SGD inside the graphed trainer step.

    python scripts/ranger_time.py [--out DIR] [--reps 10] [--window 12] [--trainer-steps 30] [--kernel-only]

(a) the fused step's time per step from device events over windows of --window steps after warm-up (a window of 12 holds two
    lookahead steps, as every 12 steps of training do), spread over --reps windows.  Kernel time: run once more under
    `rocprofv3 --kernel-trace --stats` with --kernel-only (the fused steps alone).
(b) the algorithm's bytes, counted over the tensors that have a gradient: read p, g, m, v and write p, m, v (28 B per element), + 4 B
    for the write of a centralised gradient, + 8 B (read and write of slow_buffer) on a lookahead step.
(c) the reference's per-tensor loop (ranger2020.py:139-244) in torch ops, timed the same way.
(d) the trainer's graphed step (graphed_step(overlap=True) + finish_step(total=loss)) with Ranger (set_optimizer_scheduler) and with
    bench.py's SGD, alternating windows in one process.
Prints one JSON line and writes it to DIR/ranger_time.json.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12          # achievable HBM rate of the MI355X: the byte bound is set against it


def net1_params(dev, seed=0):
    from tgpose_amd import seeded_state_dict
    from tgpose_amd.network.fs_net_repo.PoseNet9D import PoseNet9D
    net = PoseNet9D()
    net.load_state_dict(seeded_state_dict(seed), strict=True)
    return [p for p in net.to(dev).parameters() if p.requires_grad]


def seed_grads(params, seed):
    g = torch.Generator(device=params[0].device).manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=p.device) * 1e-3


def algorithm_bytes(params, gc_dims=1):
    n = sum(p.numel() for p in params if p.grad is not None)
    n_gc = sum(p.numel() for p in params if p.grad is not None and p.dim() > gc_dims)
    plain = 28 * n + 4 * n_gc
    return n, n_gc, plain, plain + 8 * n


def time_windows(fn, window, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(window):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / window)
    return out


def summary(ms):
    return dict(mean_ms=statistics.mean(ms), median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                stdev_ms=statistics.stdev(ms) if len(ms) > 1 else 0.0, n=len(ms))


class EagerRanger(object):
    """the reference's step as torch ops, one tensor at a time (gc_loc=True, use_gc=True, weight_decay=0): what running
    ranger2020.Ranger as it stands costs in launches"""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, betas=(0.95, 0.999), eps=1e-5, thr=5):
        self.params, self.lr, self.alpha, self.k, self.betas, self.eps, self.thr = params, lr, alpha, k, betas, eps, thr
        self.state = {}

    @torch.no_grad()
    def step(self):
        b1, b2 = self.betas
        for p in self.params:
            grad = p.grad
            st = self.state.get(p)
            if st is None:
                st = self.state[p] = dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p), slow=p.detach().clone())
            if grad.dim() > 1:
                grad.add_(-grad.mean(dim=tuple(range(1, grad.dim())), keepdim=True))
            st["step"] += 1
            t = st["step"]
            st["exp_avg_sq"].mul_(b2).addcmul_(grad, grad, value=1 - b2)
            st["exp_avg"].mul_(b1).add_(grad, alpha=1 - b1)
            b2t = b2 ** t
            nmax = 2 / (1 - b2) - 1
            nsma = nmax - 2 * t * b2t / (1 - b2t)
            if nsma > self.thr:
                ss = math.sqrt((1 - b2t) * (nsma - 4) / (nmax - 4) * (nsma - 2) / nsma * nmax / (nmax - 2)) / (1 - b1 ** t)
                G = st["exp_avg"] / st["exp_avg_sq"].sqrt().add_(self.eps)
            else:
                ss = 1.0 / (1 - b1 ** t)
                G = st["exp_avg"]
            p.data.add_(G, alpha=-ss * self.lr)
            if t % self.k == 0:
                st["slow"].add_(p.data - st["slow"], alpha=self.alpha)
                p.data.copy_(st["slow"])


def trainer_ab(dev, B, N, windows, window):
    from bench import train_batch
    from tgpose_amd import FLAGS, seeded_state_dict
    from tgpose_amd.trainer.RL_TDA import RT_TDA_Trainer
    torch.compiler.config.force_cudagraph_gc = True
    db = {k: v.to(dev) for k, v in train_batch(B, N, 7).items()}
    setups = {}
    for name in ("ranger", "sgd"):
        tr = RT_TDA_Trainer(device=dev)
        tr.init_network('RL_TDA')
        tr.init_loss()
        tr.net1.load_state_dict(seeded_state_dict(0), strict=True)
        tr.net2.load_state_dict(seeded_state_dict(1, only_encoder=True), strict=True)
        tr.net1.train(), tr.net2.train()
        if name == "ranger":
            tr.set_optimizer_scheduler()
        else:
            tr.optimizer = torch.optim.SGD(tr.net1.parameters(), lr=1e-5, momentum=0.9)       # bench.py's
        gs = tr.graphed_step(db, overlap=True)

        def step(tr=tr, gs=gs):
            tr.finish_step(total=gs())
        setups[name] = step
    try:
        for fn in setups.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        res = {k: [] for k in setups}
        for _ in range(windows):
            for name, fn in setups.items():
                res[name] += time_windows(fn, window, 1, 0)
    finally:
        FLAGS.train = 0
    return {k: summary(v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".", help="directory for ranger_time.json (default: the working directory)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--trainer-steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=1028)
    ap.add_argument("--kernel-only", action="store_true", help="only the fused steps (for a rocprofv3 --kernel-trace --stats run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ranger_time.py needs a GPU")
    from tgpose_amd.tools.torch_utils.solver.ranger2020 import Ranger
    dev = torch.device("cuda:0")
    params = net1_params(dev)
    seed_grads(params, 1)
    n, n_gc, plain, look = algorithm_bytes(params)
    opt = Ranger(params, lr=1e-3)
    fused = time_windows(opt.step, a.window, a.reps, warm=12)
    out = dict(tensors=len(params), elements=n, elements_gc=n_gc, bytes_plain_step=plain, bytes_lookahead_step=look,
               bytes_per_step_avg=plain + (look - plain) / 6.0, fused_step=summary(fused))
    out["fused_bytes_per_s_from_event_time"] = out["bytes_per_step_avg"] / (out["fused_step"]["median_ms"] * 1e-3)
    out["byte_bound_ms_plain"] = plain / HBM_BYTES_PER_S * 1e3
    if not a.kernel_only:
        ps = net1_params(dev)
        seed_grads(ps, 1)
        eager = EagerRanger(ps, lr=1e-3)
        out["eager_step"] = summary(time_windows(eager.step, a.window, max(3, a.reps // 2), warm=12))
        out["trainer"] = trainer_ab(dev, a.batch, a.points, a.trainer_steps // 5 or 1, 5)
        out["trainer"]["batch"], out["trainer"]["points"] = a.batch, a.points
        out["trainer"]["ranger_minus_sgd_ms"] = out["trainer"]["ranger"]["median_ms"] - out["trainer"]["sgd"]["median_ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ranger_time%s.json" % ("_kernel_only" if a.kernel_only else "")), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
