"""Regenerates tests/golden/train_loop.npz by running the REFERENCE's own training loop, ``RT_TDA_Trainer.RL_TDA_train``
(trainer/RL_TDA.py, imported unmodified as make_golden.gen_train_step imports it), on the CPU (the trainer's device swapped as there).

One epoch of four B = 4, N = 256 batches (make_golden.synth_train_batch); batch 3 carries a NaN translation target in one item, so
its total is NaN through the translation terms only (the clouds and every neighbour search stay finite) and the loop skips it.
The optimizer and schedule are the reference's own Ranger and flat_and_anneal_lr_scheduler (tools/torch_utils/solver, loaded by
file path) built with the arguments of this package's tools/training_utils (the reference ships that module as bytecode only), at
lr 1e-3 and 2 warm-up iterations so that every update is well above the parameters' rounding.  Dropout p = 0.  torch's CPU
generator is seeded once before the loop; every torch.randperm of the loop (the forwards' subsamples) is recorded.

Stored: per step the loss terms and total, whether the optimizer stepped, the LR the step saw; per net1 parameter before the loop
and after every step its sum and norm (both in float64) and 16 samples; the subsample draws; the log lines; the key lists of the checkpoint
the loop wrote.  Nothing is copied from the reference: the fixture holds its outputs only.

Usage:  python tests/golden/make_train_loop_golden.py REFERENCE_ROOT   (from the repo root)
"""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

B, N, N_BATCHES, NAN_BATCH = 4, 256, 4, 3            # NAN_BATCH: 1-based, as the loop counts
CATS = [(0, 2, 3, 4), (1, 5, 0, 3), (2, 4, 1, 5), (3, 0, 5, 2)]
DATA_SEEDS = (61, 62, 63, 64)
WSEED, FSEED = 21, 77
LOOP_FLAGS = dict(lr=1e-3, warmup_iters=2, total_epoch=1, log_every=1, save_every=1)


def param_stats(net):
    out = {}
    for k, p in net.named_parameters():
        f = p.detach().reshape(-1)
        pick = torch.linspace(0, f.numel() - 1, 16).long()
        out[k] = torch.cat([f.double().sum().float().view(1), f.double().norm().float().view(1), f[pick]]).numpy()
    return out


def main():
    global torch
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TGP_REFERENCE")
    if not ref:
        raise SystemExit("usage: python tests/golden/make_train_loop_golden.py REFERENCE_ROOT (the reference checkout)")
    ref = os.path.abspath(ref)
    sys.path.insert(0, ref)
    sys.path.insert(0, HERE)
    import make_golden as G
    import torch
    G.REF = ref
    import importlib.util

    def by_path(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    try:
        import tools.logger  # noqa: F401
    except Exception:
        lg = types.ModuleType("tools.logger")
        lg.warning = lambda *a, **k: None
        sys.modules["tools.logger"] = lg
    R = by_path("ref_ranger2020", "tools/torch_utils/solver/ranger2020.py")
    S = by_path("ref_lr_scheduler", "tools/torch_utils/solver/lr_scheduler.py")
    ref_tr = G.load_reference_trainer()
    F = G.FLAGS
    F.train = 1
    F.fsnet_loss_type = "l1"
    for k, v in LOOP_FLAGS.items():
        setattr(F, k, v)
    torch.set_num_threads(8)

    tr = ref_tr.RT_TDA_Trainer(logger=None)
    tr.device = torch.device("cpu")
    tr.init_network("RL_TDA")
    tr.init_loss()
    tr.net1.load_state_dict(G.iw.seeded_state_dict(WSEED), strict=True)
    tr.net2.load_state_dict(G.iw.seeded_state_dict(WSEED + 1, only_encoder=True), strict=True)
    for net in (tr.net1, tr.net2):
        net.train()
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    # this package's build_optimizer / build_lr_rate (tools/training_utils.py) with the reference's classes
    params = [{"params": [p for p in tr.net1.parameters() if p.requires_grad], "lr": float(F.lr) * F.lr_pose}]
    tr.optimizer = R.Ranger(params=params, lr=float(F.lr) * F.lr_pose, weight_decay=F.weight_decay)
    tr.scheduler = S.flat_and_anneal_lr_scheduler(tr.optimizer, total_iters=F.train_steps * F.total_epoch // F.accumulate,
                                                  warmup_factor=F.warmup_factor, warmup_iters=F.warmup_iters,
                                                  warmup_method=F.warmup_method, anneal_method=F.anneal_method,
                                                  anneal_point=F.anneal_point, steps=(0.5, 0.75), target_lr_factor=0,
                                                  poly_power=F.poly_power, step_gamma=F.gamma)

    batches = [G.synth_train_batch(list(c), N, s) for c, s in zip(CATS, DATA_SEEDS)]
    batches[NAN_BATCH - 1]["translation"][1, 0] = float("nan")

    lines = []
    tr.logger = types.SimpleNamespace(info=lambda msg: lines.append(str(msg)))
    rec = {"lr": [], "loss": [], "stepped": [], "stats": [param_stats(tr.net1)], "draws": []}
    steps = [0]
    o_train_step, o_opt_step, o_randperm = tr.RL_TDA_train_step, tr.optimizer.step, torch.randperm

    def train_step(db, *a, **k):
        if len(rec["loss"]) > 0:
            rec["stepped"].append(steps[0] > 0)
            rec["stats"].append(param_stats(tr.net1))
            steps[0] = 0
        rec["lr"].append(tr.optimizer.param_groups[0]["lr"])
        out, ld = o_train_step(db, *a, **k)
        terms = {k_: float(v) for k_, v in ld.items() if k_ != "TDA_loss"}
        terms.update({"TDA." + k_: float(v) for k_, v in ld["TDA_loss"].items()})
        rec["loss"].append(terms)
        return out, ld

    def opt_step(*a, **k):
        steps[0] += 1
        return o_opt_step(*a, **k)

    def randperm(n, *a, **k):
        r = o_randperm(n, *a, **k)
        rec["draws"].append(r.clone())
        return r

    tr.RL_TDA_train_step, tr.optimizer.step = train_step, opt_step
    with tempfile.TemporaryDirectory() as tmp:
        F.model_save = tmp
        torch.manual_seed(FSEED)
        torch.randperm = randperm
        try:
            tr.RL_TDA_train(batches, 1)
        finally:
            torch.randperm = o_randperm
        rec["stepped"].append(steps[0] > 0)
        rec["stats"].append(param_stats(tr.net1))
        files = sorted(os.listdir(tmp))
        ck = torch.load(os.path.join(tmp, files[0]), map_location="cpu")
    keys = {"files": files, "top": list(ck), "epoch": ck["epoch"], "net1": list(ck["net1_state_dict"]),
            "net2": list(ck["net2_state_dict"]), "optimizer": list(ck["optimizer_state_dict"]),
            "optimizer.state": sorted(set(k for st in ck["optimizer_state_dict"]["state"].values() for k in st)),
            "optimizer.param_groups": sorted(ck["optimizer_state_dict"]["param_groups"][0]),
            "scheduler": sorted(ck["scheduler_state_dict"])}

    out = dict(weight_seed=np.int64(WSEED), forward_seed=np.int64(FSEED), n_points=np.int64(N), nan_batch=np.int64(NAN_BATCH),
               cat_ids=np.array(CATS), data_seeds=np.array(DATA_SEEDS), flags=np.array(json.dumps(LOOP_FLAGS)),
               lr=np.array(rec["lr"], dtype=np.float64), stepped=np.array(rec["stepped"]), log=np.array(json.dumps(lines)),
               checkpoint=np.array(json.dumps(keys)))
    names = sorted(rec["loss"][0])
    out["loss.names"] = np.array(json.dumps(names))
    out["loss"] = np.array([[t[k] for k in names] for t in rec["loss"]], dtype=np.float32)
    pnames = list(rec["stats"][0])
    out["param.names"] = np.array(json.dumps(pnames))
    for j, k in enumerate(pnames):
        out["param.%d" % j] = np.stack([s[k] for s in rec["stats"]]).astype(np.float32)      # (1 + steps, 18)
    assert len(rec["draws"]) == 4 * N_BATCHES
    for j, d in enumerate(rec["draws"]):
        out["draw.%d" % j] = d.numpy().astype(np.int16)
    path = os.path.join(HERE, "train_loop.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f kB); stepped %s; lr %s" % (path, len(out), os.path.getsize(path) / 1e3, rec["stepped"], rec["lr"]))


import numpy as np  # noqa: E402

if __name__ == "__main__":
    main()
