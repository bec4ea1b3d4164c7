"""GPU tests of the fused Ranger step (tgpose_amd.tools.torch_utils.solver.ranger2020.Ranger, csrc/ranger.hip): against the
reference's own optimizer (tests/golden/ranger.npz, recorded by tests/golden/make_ranger_golden.py), against an fp64 restatement of
the algorithm at net1's parameter shapes, bit-for-bit determinism, misaligned views, None gradients, loading a reference
state_dict, no host synchronisation, and the trainer's captured step with set_optimizer_scheduler().

Bars: exp_avg / exp_avg_sq within 1e-5 max|ref|; p and slow_buffer within 1e-4 max|p_ref - p_init| + 4 ulp(p) (the bar is set on the
update: an update of ~1e-4 |p| would hide inside any plain relative tolerance on p); step counters exact."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import ranger_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    from tgpose_amd import _lib
    _lib.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "ranger.npz"))


def _Ranger():
    from tgpose_amd.tools.torch_utils.solver.ranger2020 import Ranger
    return Ranger


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _close_state(got, want, name):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want).max() if want.size else 0.0
    assert err <= 1e-5 * np.abs(want).max() + 1e-30, (name, err, np.abs(want).max())


def _close_param(got, want, init, name):
    got, want, init = (np.asarray(a, dtype=np.float64) for a in (got, want, init))
    bar = 1e-4 * np.abs(want - init).max() + 4 * _ulp(want)
    assert np.all(np.abs(got - want) <= bar), (name, np.abs(got - want).max(), np.abs(want - init).max())


def _clipped_grads(config, step):
    """the step's gradients after clip_grad_norm_(5) on the CPU, as the recorder computed them; None where the case has none"""
    carriers = []
    for i, s in enumerate(C.SHAPES):
        t = torch.zeros(s)
        t.grad = torch.from_numpy(C.grad(step, i)) if C.has_grad(config, step, i) else None
        carriers.append(t)
    torch.nn.utils.clip_grad_norm_(carriers, C.MAX_NORM)
    return [c.grad for c in carriers]


def _run_fixture_case(config, opt_kw, params, opt, sched, first, last, fx, init):
    for step in range(first, last + 1):
        clipped = _clipped_grads(config, step)
        for p, g in zip(params, clipped):
            p.grad = None if g is None else g.to(DEV)
        if sched is not None:
            assert opt.param_groups[0]["lr"] == fx["%s/lr" % config][step - 1]
        else:
            opt.param_groups[0]["lr"] = float(fx["%s/lr" % config][step - 1])
        opt.step()
        if sched is not None:
            sched.step()
        if step in C.STORED[config]:
            torch.cuda.synchronize()
            for i, p in enumerate(params):
                tag = "%s/%d/%%s/%d" % (config, step, i)
                st = opt.state[p]
                if not C.CONFIGS[config]["kw"].get("use_gc", True) or C.CONFIGS[config]["kw"].get("gc_conv_only", False):
                    assert torch.equal(p.grad.cpu(), clipped[i]), tag      # no tensor here is centralised: grads left as they came
                assert st.get("step", 0) == int(fx[tag % "step"]), (tag, st.get("step"))
                for f in C.STORED[config][step]:
                    if (tag % f) not in fx.files:
                        assert f != "p" and (f == "grad" and p.grad is None or f != "grad" and f not in st), tag
                        continue
                    want = fx[tag % f]
                    if f == "p":
                        _close_param(p.detach().cpu().numpy(), want, init[i], tag % f)
                    elif f == "slow_buffer":
                        _close_param(st[f].cpu().numpy(), want, init[i], tag % f)
                    elif f == "grad":
                        _close_state(p.grad.cpu().numpy(), want, tag % f)
                    else:
                        _close_state(st[f].cpu().numpy(), want, tag % f)


@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_ranger_matches_reference_fixture(fx, config):
    from tgpose_amd.tools.torch_utils.solver.lr_scheduler import flat_and_anneal_lr_scheduler
    init = C.init_params()
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(DEV)) for p in init]
    opt = _Ranger()(params, lr=C.BASE_LR, **C.CONFIGS[config]["kw"])
    sched = flat_and_anneal_lr_scheduler(opt, **C.SCHED)
    _run_fixture_case(config, {}, params, opt, sched, 1, C.STEPS, fx, init)


def test_ranger_loads_reference_state_dict_and_continues(fx):
    """the reference's state_dict after step 7 (separate tensors, int step counters) loads, is flattened again, and steps 8-13
    end where the reference ended"""
    init = C.init_params()
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(DEV)) for p in init]
    # the parameters as they were after step 7: the reference's p is not in the state_dict, so replay steps 1-7 here first
    opt0 = _Ranger()(params, lr=C.BASE_LR)
    for step in range(1, C.SD_STEP + 1):
        for p, g in zip(params, _clipped_grads("default", step)):
            p.grad = g.to(DEV)
        opt0.param_groups[0]["lr"] = float(fx["default/lr"][step - 1])
        opt0.step()
    opt = _Ranger()(params, lr=C.BASE_LR)
    state = {i: {"step": int(fx["sd/step/%d" % i]), **{f: torch.from_numpy(fx["sd/%s/%d" % (f, i)]) for f in
                                                      ("exp_avg", "exp_avg_sq", "slow_buffer")}} for i in range(len(C.SHAPES))}
    opt.load_state_dict({"state": state, "param_groups": json.loads(str(fx["sd/param_groups"]))})
    _run_fixture_case("default", {}, params, opt, None, C.SD_STEP + 1, C.STEPS, fx, init)
    flat = opt._flat.untyped_storage().data_ptr()
    assert all(opt.state[p][f].untyped_storage().data_ptr() == flat for p in params for f in ("exp_avg", "exp_avg_sq", "slow_buffer"))


# ------------------------------------------------------------------------------------------------ fp64 restatement
class Ref64(object):
    """ranger2020.py:139-246 restated in fp64 over fp32 inputs (gc_loc=True): per parameter, step counter, GC, moments, the RAdam
    branch, weight decay (into exp_avg on the non-adaptive branch), update, lookahead"""

    def __init__(self, params, lr, weight_decay=0.0, alpha=0.5, k=6, betas=(0.95, 0.999), eps=1e-5, thr=5, use_gc=True):
        self.p = [p.detach().double().clone() for p in params]
        self.st = [None] * len(params)
        self.lr, self.wd, self.alpha, self.k, self.betas, self.eps, self.thr, self.use_gc = lr, weight_decay, alpha, k, betas, eps, thr, use_gc

    def step(self, grads):
        b1, b2 = self.betas
        out = []
        for i, g in enumerate(grads):
            if g is None:
                out.append(None)
                continue
            g = g.double().clone()
            p = self.p[i]
            if self.st[i] is None:
                self.st[i] = dict(step=0, m=torch.zeros_like(p), v=torch.zeros_like(p), slow=p.clone())
            st = self.st[i]
            if self.use_gc and g.dim() > 1:
                g = g - g.mean(dim=tuple(range(1, g.dim())), keepdim=True)
            st["step"] += 1
            t = st["step"]
            st["v"] = st["v"] * b2 + (1 - b2) * g * g
            st["m"] = st["m"] * b1 + (1 - b1) * g
            b2t = b2 ** t
            nmax = 2 / (1 - b2) - 1
            nsma = nmax - 2 * t * b2t / (1 - b2t)
            if nsma > self.thr:
                ss = math.sqrt((1 - b2t) * (nsma - 4) / (nmax - 4) * (nsma - 2) / nsma * nmax / (nmax - 2)) / (1 - b1 ** t)
                G = st["m"] / (st["v"].sqrt() + self.eps)
            else:
                ss = 1.0 / (1 - b1 ** t)
                G = st["m"]
            if self.wd != 0:
                G = G + self.wd * p
                if nsma <= self.thr:
                    st["m"] = G
            p = p - ss * self.lr * G
            if t % self.k == 0:
                st["slow"] = st["slow"] + self.alpha * (p - st["slow"])
                p = st["slow"].clone()
            self.p[i] = p
            out.append(g)
        return out


def _check_vs_ref64(params, opt, ref, init, what):
    for i, p in enumerate(params):
        st = opt.state[p]
        if ref.st[i] is None:
            assert len(st) == 0, (what, i)
            continue
        assert st["step"] == ref.st[i]["step"], (what, i)
        _close_param(p.detach().cpu().numpy(), ref.p[i].cpu().numpy(), init[i], "%s p %d" % (what, i))
        _close_param(st["slow_buffer"].cpu().numpy(), ref.st[i]["slow"].cpu().numpy(), init[i], "%s slow %d" % (what, i))
        _close_state(st["exp_avg"].cpu().numpy(), ref.st[i]["m"].cpu().numpy(), "%s m %d" % (what, i))
        _close_state(st["exp_avg_sq"].cpu().numpy(), ref.st[i]["v"].cpu().numpy(), "%s v %d" % (what, i))


def _net1_shapes():
    from tgpose_amd.network.fs_net_repo.PoseNet9D import PoseNet9D
    return [tuple(p.shape) for p in PoseNet9D().parameters()]


def _seeded(shape, seed, scale):
    rs = np.random.RandomState(seed)
    n = shape[0] if shape else 1
    g = rs.standard_normal(shape) + 0.3 * rs.standard_normal((n,) + (1,) * (len(shape) - 1))
    return torch.from_numpy((scale * g).astype(np.float32))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_ranger_net1_shapes_vs_fp64_restatement(fx, wd):
    shapes = _net1_shapes()
    init = [(0.05 * np.random.RandomState(500 + i).standard_normal(s)).astype(np.float32) for i, s in enumerate(shapes)]
    params = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in init]
    opt = _Ranger()(params, lr=3e-3, weight_decay=wd)
    ref = Ref64([torch.from_numpy(a).to(DEV) for a in init], 3e-3, weight_decay=wd)
    for step in range(1, 8):
        grads = [_seeded(s, 7919 * step + i, 1e-3).to(DEV) for i, s in enumerate(shapes)]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        gref = ref.step(grads)
        if step in (5, 6, 7):
            torch.cuda.synchronize()
            _check_vs_ref64(params, opt, ref, init, "step %d" % step)
            for i, p in enumerate(params):                     # p.grad is centralised in place, as the reference leaves it
                _close_state(p.grad.cpu().numpy(), gref[i].cpu().numpy(), "grad %d" % i)


def test_ranger_is_deterministic_and_independent_of_launch_company(fx):
    """two optimizers on the same inputs agree bit for bit; one launch over all tensors equals one launch per tensor"""
    shapes = C.SHAPES + [(1024, 1289, 1)]
    init = [(0.1 * np.random.RandomState(77 + i).standard_normal(s)).astype(np.float32) for i, s in enumerate(shapes)]
    runs = []
    for mode in ("joint", "joint", "apart"):
        params = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in init]
        opts = [_Ranger()(params, lr=1e-2)] if mode == "joint" else [_Ranger()([p], lr=1e-2) for p in params]
        for step in range(1, 8):
            for i, p in enumerate(params):
                p.grad = _seeded(shapes[i], 31 * step + i, 1e-2).to(DEV)
            for o in opts:
                o.step()
        state = [opts[0 if mode == "joint" else i].state[p] for i, p in enumerate(params)]
        runs.append([(p.detach().clone(), p.grad.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["slow_buffer"].clone())
                     for p, st in zip(params, state)])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for x, y in zip(a, b):
                assert torch.equal(x, y)


def test_ranger_misaligned_views_and_scalar_tails(fx):
    """parameters and gradients as views at odd 4-byte offsets of flat buffers (as shard.GradBuckets lays gradients out): the
    16-byte accesses give way to 4-byte ones where an array's phase differs from exp_avg's, heads and tails are scalar"""
    shapes = [(5, 7, 1), (3, 1289), (2, 4500), (257,), (128, 3, 1), (64, 130)]
    init = [(0.1 * np.random.RandomState(900 + i).standard_normal(s)).astype(np.float32) for i, s in enumerate(shapes)]
    n = sum(int(np.prod(s)) + 3 for s in shapes) + 8
    pflat = torch.zeros(n, device=DEV)
    gflat = torch.zeros(n, device=DEV)
    params, o_p, o_g = [], 1, 3
    for a in init:
        k = a.size
        view = pflat[o_p:o_p + k].view(a.shape)
        view.copy_(torch.from_numpy(a))
        params.append((view, o_g))
        o_p += k + 1 + (k % 2)
        o_g += k + 2
    leaves = [torch.nn.Parameter(v) for v, _ in params]        # Parameters sharing pflat's storage at odd offsets
    assert any(lf.data_ptr() % 16 for lf in leaves)
    opt = _Ranger()(leaves, lr=1e-2)
    ref = Ref64([torch.from_numpy(a).to(DEV) for a in init], 1e-2)
    for step in range(1, 8):
        grads = [_seeded(s, 4001 * step + i, 1e-2).to(DEV) for i, s in enumerate(shapes)]
        for lf, (_, og), g in zip(leaves, params, grads):
            lf.grad = gflat[og:og + g.numel()].view(g.shape)
            lf.grad.copy_(g)
        assert any(lf.grad.data_ptr() % 16 for lf in leaves)
        opt.step()
        ref.step(grads)
    torch.cuda.synchronize()
    _check_vs_ref64(leaves, opt, ref, init, "misaligned")
    # nothing outside the views was written
    used_p = torch.zeros(n, dtype=torch.bool, device=DEV)
    for lf in leaves:
        o = (lf.data_ptr() - pflat.data_ptr()) // 4
        used_p[o:o + lf.numel()] = True
    assert (pflat[~used_p] == 0).all()
    used_g = torch.zeros(n, dtype=torch.bool, device=DEV)
    for lf in leaves:
        o = (lf.grad.data_ptr() - gflat.data_ptr()) // 4
        used_g[o:o + lf.numel()] = True
    assert (gflat[~used_g] == 0).all()


def test_ranger_none_grad_gets_no_state_and_no_step(fx):
    params = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(3)).to(DEV)) for s in [(16, 9), (33,), (4, 5)]]
    before = [p.detach().clone() for p in params]
    opt = _Ranger()(params, lr=1e-2)
    params[0].grad = torch.ones(16, 9, device=DEV)
    params[2].grad = torch.ones(4, 5, device=DEV)
    opt.step()
    assert len(opt.state[params[1]]) == 0 and torch.equal(params[1].detach(), before[1])
    assert opt.state[params[0]]["step"] == 1 and opt.state[params[2]]["step"] == 1
    params[1].grad, params[2].grad = torch.full((33,), 0.5, device=DEV), None
    opt.step()                                  # a new parameter gets state: the flat buffer grows, the old state is kept
    assert [opt.state[p]["step"] for p in params] == [2, 1, 1]
    ref = Ref64(before, 1e-2)
    ref.step([torch.ones(16, 9, device=DEV), None, torch.ones(4, 5, device=DEV)])
    ref.step([torch.ones(16, 9, device=DEV), torch.full((33,), 0.5, device=DEV), None])
    torch.cuda.synchronize()
    _check_vs_ref64(params, opt, ref, [b.cpu().numpy() for b in before], "none")


def test_ranger_step_makes_no_host_sync(fx):
    shapes = [(64, 128, 1), (256,), (2, 4500)]
    params = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in shapes]
    opt = _Ranger()(params, lr=1e-3)
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()                                  # the first step builds the state and the table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert all(opt.state[p]["step"] == 4 for p in params)


# ------------------------------------------------------------------------------------------------------ the trainer
def test_trainer_graphed_overlap_step_with_ranger(fx):
    """RT_TDA_Trainer at B = 4, N = 256: graphed_step(overlap=True), set_optimizer_scheduler(), seven finish_step(total=loss).
    Each step's update (from the clipped gradients and the state before it) agrees with the fp64 restatement; proj_layer, whose
    gradients GradBuckets keeps at zero instead of None (shard.py), gets state and stays bit-unchanged with weight_decay 0."""
    from tgpose_amd import FLAGS, seeded_state_dict
    from tgpose_amd.trainer.RL_TDA import RT_TDA_Trainer
    from tests.test_gpu_parity import _step_db
    B, N = 4, 256
    tr = RT_TDA_Trainer(device=DEV)
    tr.init_network('RL_TDA')
    tr.init_loss()
    tr.net1.load_state_dict(seeded_state_dict(13), strict=True)
    tr.net2.load_state_dict(seeded_state_dict(14, only_encoder=True), strict=True)
    for net in (tr.net1, tr.net2):
        net.train()
    old = {k: getattr(FLAGS, k) for k in ("warmup_iters", "lr")}
    torch.compiler.config.force_cudagraph_gc, old_gc = True, torch.compiler.config.force_cudagraph_gc
    try:
        FLAGS.warmup_iters, FLAGS.lr = 3, 1e-3          # updates well above the parameters' rounding from the first step
        tr.set_optimizer_scheduler()
        db = {k: torch.as_tensor(v).to(DEV) for k, v in _step_db([0, 1, 2, 3], N, 47).items()}
        step = tr.graphed_step(db, overlap=True)
        named = list(tr.net1.named_parameters())
        proj = [p for n, p in named if "proj_layer" in n]
        proj0 = [p.detach().clone() for p in proj]
        torch.manual_seed(3)
        for it in range(7):
            total = step()
            # what the optimizer will see: the clip runs inside finish_step; reproduce its clipped gradients for the check
            torch.cuda.synchronize()
            grads = [p.grad.detach().clone() for _, p in named]
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
            coef = torch.clamp(5.0 / (norm + 1e-6), max=1.0)
            clipped = [g * coef for g in grads]
            st_before = [dict(tr.optimizer.state[p]) for _, p in named]
            snap = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()} for s in st_before]
            p_before = [p.detach().clone() for _, p in named]
            lr = tr.optimizer.param_groups[0]["lr"]
            assert tr.finish_step(total=total) is True
            torch.cuda.synchronize()
            ref = Ref64(p_before, lr)
            for i, s in enumerate(snap):
                if s:
                    ref.st[i] = dict(step=s["step"], m=s["exp_avg"].double(), v=s["exp_avg_sq"].double(), slow=s["slow_buffer"].double())
            ref.step(clipped)
            for i, (n_, p) in enumerate(named):
                st = tr.optimizer.state[p]
                assert st["step"] == it + 1, n_
                d_ref = (ref.p[i] - p_before[i].double()).abs().max().item()
                err = (p.detach().double() - ref.p[i]).abs()
                bar = 1e-4 * d_ref + 4 * torch.from_numpy(_ulp(ref.p[i].cpu().numpy())).to(DEV)
                # the clip coefficient here and inside finish_step differ by rounding: allow its relative effect on the update
                bar = bar + 1e-5 * d_ref
                assert bool((err <= bar).all()), (it, n_, err.max().item(), d_ref)
                _close_state(st["exp_avg"].cpu().numpy(), ref.st[i]["m"].cpu().numpy(), "%d %s m" % (it, n_))
        assert len(proj) > 0
        for p, p0 in zip(proj, proj0):
            assert torch.equal(p.detach(), p0) and len(tr.optimizer.state[p]) == 4
        assert tr.scheduler.last_epoch == 7
    finally:
        for k, v in old.items():
            setattr(FLAGS, k, v)
        torch.compiler.config.force_cudagraph_gc = old_gc
        FLAGS.train = 0
