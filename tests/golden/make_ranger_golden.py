"""Regenerates tests/golden/ranger.npz by running the REFERENCE's Ranger and flat_and_anneal_lr_scheduler themselves
(tools/torch_utils/solver/ranger2020.py and lr_scheduler.py, loaded by file path, unmodified) on the cases of tests/ranger_cases.py,
on the CPU in fp32.

``lr_scheduler`` imports ``tools.logger``; a stand-in module of this repository (one ``warning`` function) is put into sys.modules
under that name first.  Nothing is copied from the reference: the fixture holds the reference's outputs only.

Stored: the lr sequence of the run; at the checkpoints of ranger_cases.STORED the state each configuration leaves (parameter,
exp_avg, exp_avg_sq, slow_buffer, step, and p.grad after the step, which the reference centralises in place); the reference
state_dict after step 7 of "default"; lr sequences of the reference scheduler for every anneal and warmup method; the reference's
constructor / argument errors.

Usage:  python tests/golden/make_ranger_golden.py REFERENCE_ROOT   (from the repo root; or set $TGP_REFERENCE)
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import ranger_cases as C  # noqa: E402


def load_reference(ref):
    tools = types.ModuleType("tools")
    tools.__path__ = []
    logger = types.ModuleType("tools.logger")
    logger.warning = lambda *a, **k: None
    tools.logger = logger
    sys.modules.setdefault("tools", tools)
    sys.modules["tools.logger"] = logger
    mods = {}
    for name in ("ranger2020", "lr_scheduler"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref, "tools", "torch_utils", "solver", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["ranger2020"], mods["lr_scheduler"]


def run_config(R, S, config, out):
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in C.init_params()]
    opt = R.Ranger(params, lr=C.BASE_LR, **C.CONFIGS[config]["kw"])
    sched = S.flat_and_anneal_lr_scheduler(opt, **C.SCHED)
    lrs = []
    for step in range(1, C.STEPS + 1):
        for i, p in enumerate(params):
            p.grad = torch.from_numpy(C.grad(step, i)) if C.has_grad(config, step, i) else None
        torch.nn.utils.clip_grad_norm_(params, C.MAX_NORM)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        if step in C.STORED[config]:
            for i, p in enumerate(params):
                st = opt.state[p]
                out["%s/%d/step/%d" % (config, step, i)] = np.int64(st.get("step", 0))
                for f in C.STORED[config][step]:
                    t = p.detach() if f == "p" else (p.grad if f == "grad" else st.get(f))
                    if t is not None:
                        out["%s/%d/%s/%d" % (config, step, f, i)] = t.numpy().copy()
        if config == "default" and step == C.SD_STEP:
            sd = opt.state_dict()
            out["sd/param_groups"] = np.array(json.dumps(sd["param_groups"]))
            for i, st in sd["state"].items():
                out["sd/step/%d" % i] = np.int64(st["step"])
                for f in ("exp_avg", "exp_avg_sq", "slow_buffer"):
                    out["sd/%s/%d" % (f, i)] = st[f].numpy().copy()
    out["%s/lr" % config] = np.array(lrs, dtype=np.float64)


def errors(R, S):
    p = [torch.nn.Parameter(torch.zeros(2))]
    bad = {"alpha": dict(alpha=1.5), "k": dict(k=0), "lr": dict(lr=0.0), "eps": dict(eps=0.0)}
    errs = {}
    for name, kw in bad.items():
        try:
            R.Ranger(p, **kw)
        except ValueError as e:
            errs["ranger/" + name] = str(e)
    opt = torch.optim.SGD(p, lr=1.0)
    sbad = {"warmup": dict(warmup_method="cubic"), "anneal": dict(anneal_method="sqrt"), "point": dict(anneal_point=1.5),
            "steps_range": dict(anneal_method="step", warmup_iters=50, steps=(0.2, 0.9)),
            "steps_order": dict(anneal_method="step", steps=(0.9, 0.5))}
    for name, kw in sbad.items():
        try:
            S.flat_and_anneal_lr_scheduler(opt, 100, **kw)
        except ValueError as e:
            errs["sched/" + name] = str(e)
    return errs


def sched_table(S):
    out = {}
    for warm in ("linear", "constant"):
        for ann in ("cosine", "linear", "poly", "exp", "step", "none"):
            p = [torch.nn.Parameter(torch.zeros(1))]
            opt = torch.optim.SGD(p, lr=0.5)
            sch = S.flat_and_anneal_lr_scheduler(opt, warmup_method=warm, anneal_method=ann, **C.SCHED_TABLE)
            lrs = []
            for _ in range(C.SCHED_TABLE["total_iters"] + 1):
                lrs.append(opt.param_groups[0]["lr"])
                opt.step()
                sch.step()
            out["table/%s/%s" % (warm, ann)] = np.array(lrs, dtype=np.float64)
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TGP_REFERENCE")
    if not ref:
        raise SystemExit("usage: python tests/golden/make_ranger_golden.py REFERENCE_ROOT (the reference checkout)")
    R, S = load_reference(ref)
    torch.set_num_threads(1)
    out = {}
    for config in C.CONFIGS:
        run_config(R, S, config, out)
    out.update(sched_table(S))
    out["errors"] = np.array(json.dumps(errors(R, S)))
    path = os.path.join(HERE, "ranger.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.2f MB)" % (path, len(out), os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
