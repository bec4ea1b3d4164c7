"""tests/bn_ref.py held to PyTorch, and the conditions that keep tests/test_bn_kernels_gpu.py from hiding a failure.  No GPU.

* ref64 against F.batch_norm(training=True) and torch autograd in float64 -- every activation, the running buffers, the pooled form --
  on benign data: the reference is pinned to PyTorch, not to the kernels.
* oracle32 against ref64 within float32 accuracy on benign data, both forms, at shapes with tails and an empty chunk group.
* For every (rows, C, kinds) the GPU file uses: `ambiguous` marks at most 1e-3 of any tensor and nothing in the sign-exact kinds;
  for every kind but the K-outlier and the scale kinds Q_c <= 4 var_c, so that a bound expressed through oracle32's error stays a
  bound relative to the problem itself.
* The conditioning table (recorded in DESIGN.md, "Training-mode forward") is printed, nothing about it is asserted.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

F64, F32 = torch.float64, torch.float32
ACTS = [(0, 0.0, False), (1, 0.0, False), (1, 0.2, False), (1, 0.0, True)]


def _benign(rows, C, seed):
    ge = R.gen(rows, C, seed)
    x = (2 * torch.randn(rows, C, generator=ge) + 0.5 * torch.randn(C, generator=ge)).to(F32)
    gamma, beta = torch.rand(C, generator=ge) + 0.5, torch.randn(C, generator=ge)
    slope_vec = torch.tensor([(0.2, 0.0, 0.01, 1.0)[c % 4] for c in range(C)])
    return x, gamma, beta, slope_vec, ge


def _torch_act(z, act, slope, sv):
    return torch.where(z > 0, z, z * (sv.to(z.dtype) if sv is not None else slope)) if act else z


@pytest.mark.parametrize("act,slope,vec", ACTS)
@pytest.mark.parametrize("rows,C,momentum", [(2, 5, 0.1), (37, 8, 0.0), (300, 7, 1.0)])
def test_ref64_forward_is_pytorch(rows, C, momentum, act, slope, vec):
    x, gamma, beta, sv, ge = _benign(rows, C, 1)
    sv = sv if vec else None
    rm, rv, nbt = torch.randn(C, generator=ge).double(), torch.rand(C, generator=ge).double() + 0.5, torch.tensor(7)
    trm, trv = rm.clone(), rv.clone()
    want = _torch_act(F.batch_norm(x.double(), trm, trv, gamma.double(), beta.double(), True, momentum, R.BN_EPS), act, slope, sv)
    got = R.ref64(x, gamma, beta, R.BN_EPS, act, slope, sv, running=(rm, rv, momentum, nbt))
    assert torch.allclose(got["y"], want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(got["rm"], trm, rtol=1e-13, atol=1e-13) and torch.allclose(got["rv"], trv, rtol=1e-13, atol=1e-13)
    assert int(got["nbt"]) == 8 and got["y"].dtype == F64
    assert torch.allclose(got["mean"], x.double().mean(0), rtol=1e-13, atol=1e-13)
    assert torch.allclose(got["var"], x.double().var(0, unbiased=False), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("act,slope,vec", ACTS)
@pytest.mark.parametrize("rows,C", [(2, 5), (37, 8), (300, 7)])
def test_ref64_backward_is_autograd(rows, C, act, slope, vec):
    x, gamma, beta, sv, ge = _benign(rows, C, 2)
    sv = sv if vec else None
    dy = torch.randn(rows, C, generator=ge).double()
    xd, gd, bd = (t.double().requires_grad_() for t in (x, gamma, beta))
    _torch_act(F.batch_norm(xd, None, None, gd, bd, True, 0.0, R.BN_EPS), act, slope, sv).backward(dy)
    got = R.ref64_bwd(dy, x, gamma, beta, R.BN_EPS, act, slope, sv)
    for name, want in (("dx", xd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad)):
        assert torch.allclose(got[name], want, rtol=1e-10, atol=1e-11), name


@pytest.mark.parametrize("act,slope,vec", ACTS)
@pytest.mark.parametrize("objects,n,C,cm", [(3, 17, 8, 8), (5, 1, 6, 4), (1, 40, 5, 5)])
def test_ref64_pooled_is_autograd(objects, n, C, cm, act, slope, vec):
    x, gamma, beta, sv, ge = _benign(objects * n, C, 3)
    sv = sv if vec else None
    dpool = torch.randn(objects, cm, generator=ge).double()
    xd, gd, bd = (t.double().requires_grad_() for t in (x, gamma, beta))
    y = _torch_act(F.batch_norm(xd, None, None, gd, bd, True, 0.0, R.BN_EPS), act, slope, sv)
    pooled, where = y.view(objects, n, C)[:, :, :cm].max(1)
    pooled.backward(dpool)
    fwd = R.ref64(x, gamma, beta, R.BN_EPS, act, slope, sv, rows_per_obj=n, cm_cols=cm)
    assert torch.allclose(fwd["colmax"], pooled.detach(), rtol=1e-12, atol=1e-12)
    assert torch.equal(fwd["argrow"].long(), where + torch.arange(objects).unsqueeze(1) * n)
    # the pooled backward takes (objects, C): columns past cm_cols get no gradient
    full = torch.zeros(objects, C, dtype=F64)
    full[:, :cm] = dpool
    arg = torch.zeros(objects, C, dtype=torch.int32) + (torch.arange(objects).unsqueeze(1) * n).int()
    arg[:, :cm] = fwd["argrow"]
    got = R.ref64_bwd_pooled(full, arg, x, gamma, beta, R.BN_EPS, act, slope, sv)
    for name, want in (("dx", xd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad)):
        assert torch.allclose(got[name], want, rtol=1e-10, atol=1e-11), name
    dy = torch.randn(objects, n, C, generator=ge)
    assert torch.allclose(R.colsum_objects(dy), dy.double().sum(1)) and torch.allclose(R.colsum(dy.view(-1, C)), dy.double().sum((0, 1)))


@pytest.mark.parametrize("form", ["v4", "s"])
@pytest.mark.parametrize("rows", [2, 5, 257, 1025, 1281, 2049])
def test_oracle32_is_the_same_operation(rows, form):
    """within float32 accuracy of ref64 on benign data: 1281 rows give the one-pass form groups of 2, 2, 1 and 0 chunks"""
    C = 12
    x, gamma, beta, sv, ge = _benign(rows, C, 4)
    run = (torch.randn(C, generator=ge), torch.rand(C, generator=ge) + 0.5, 0.1, torch.tensor(3))
    a = R.ref64(x, gamma, beta, act=1, slope_vec=sv, rows_per_obj=1, running=run)
    b = R.oracle32(x, gamma, beta, act=1, slope_vec=sv, rows_per_obj=1, running=run, form=form)
    for k in ("mean", "var", "y", "colmax", "rm", "rv"):
        assert b[k].dtype == F32 and torch.allclose(b[k].double(), a[k], rtol=2e-5, atol=2e-5), k
    assert int(b["nbt"]) == 4 and torch.equal(a["argrow"], b["argrow"])
    dy = torch.randn(rows, C, generator=ge)
    stats = (b["mean"], b["var"])
    a, b = R.ref64_bwd(dy, x, gamma, beta, stats=stats), R.oracle32_bwd(dy, x, gamma, beta, stats=stats, form=form)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.allclose(b[k].double(), a[k], rtol=1e-4, atol=1e-4), k
    assert torch.allclose(R.colsum32(dy, form).double(), R.colsum(dy), rtol=1e-5, atol=1e-4)
    if rows % 5 == 0 or rows == 2:
        d3 = dy.view(-1, rows // (5 if rows % 5 == 0 else 2), C)
        assert torch.allclose(R.colsum_objects32(d3).double(), R.colsum_objects(d3), rtol=1e-5, atol=1e-4)


def test_oracle32_constant_columns_are_exact():
    """both forms shift by a first row: a constant column has mean == the constant and variance == 0"""
    for rows in R.ROWS:
        x = torch.tensor([0.1, 0.0, -3.3, 1e3 + 0.1]).to(F32).expand(rows, 4).contiguous()
        for form in ("v4", "s"):
            mean, var = R.stats32(x, form)
            assert torch.equal(mean, x[0]) and torch.equal(var, torch.zeros(4)), (rows, form)


@functools.lru_cache(maxsize=None)
def _case(rows, C, kinds):
    return R.case(rows, C, kinds)


def _form(C):
    return "v4" if C % 4 == 0 else "s"


@pytest.mark.parametrize("rows,C,kinds", R.all_cases(), ids=lambda v: str(v) if isinstance(v, int) else "k%d" % len(v))
def test_gpu_cases_hide_nothing(rows, C, kinds):
    cs = _case(rows, C, kinds)
    x, gamma, beta, kd = cs["x"], cs["gamma"], cs["beta"], cs["kinds"]
    assert bool(torch.isfinite(x).all())
    # the activation decision: against the statistics either form hands to the backward, and against the forward's own float64 ones
    for form in ("v4", "s"):
        amb = R.ambiguous(x, gamma, beta, stats=R.stats32(x, form), stats_other=None if rows < 2 else
                          tuple(R.ref64(x, gamma, beta)[k] for k in ("mean", "var")))
        assert R.excluded_share_ok(amb["z"]) and R.excluded_share_ok(amb["cols"]), (form, int(amb["z"].sum()), int(amb["cols"].sum()))
        for k in R.SIGN_EXACT:
            assert not bool(amb["z"][:, R.columns_of(kd, k)].any()), k
    # the argmax: cases the GPU file pools
    for prow, rpo, pC, cm in R.POOL_CASES:
        if (prow, pC) == (rows, C) and kinds == R.NO_TIES:
            st = R.stats32(x, _form(C))
            for act, slope in ((0, 0.0), (1, 0.0), (1, 0.2)):      # test_colmax_arg's activations, over all C columns
                amb = R.ambiguous(x, gamma, beta, stats=st, rows_per_obj=rpo, act=act, slope=slope)
                if rpo > 1:
                    assert R.excluded_share_ok(amb["arg"]), (rpo, cm, int(amb["arg"].sum()))
                else:
                    assert not bool(amb["arg"].any())
    # the one-pass form's conditioning
    q, var = R.q_over_var(x)
    for k in R.KINDS:
        cols = R.columns_of(kd, k)
        if k not in R.Q_FREE and bool(cols.any()):
            assert bool((q[cols] <= 4.0 * var[cols]).all()), (k, (q[cols] / var[cols]).max())


def test_conditioning_table(capsys):
    """oracle32's error against ref64 per kind, both forms, next to a plain float32 two-pass in torch: printed, nothing asserted"""
    rows, C = 2049, 40
    cs = R.make_case(rows, C)
    x, gamma, beta, kd = cs["x"], cs["gamma"], cs["beta"], cs["kinds"]
    r = R.ref64(x, gamma, beta)
    forms = {"one-pass (16-byte form)": R.oracle32(x, gamma, beta, form="v4"), "two-pass (4-byte form)": R.oracle32(x, gamma, beta, form="s"),
             "float32 two-pass in torch": R.oracle32(x, gamma, beta, stats=R.two_pass32(x))}
    with capsys.disabled():
        print("\nrelative error of the variance / error of y relative to max|y|, %d rows, float32 against float64 on the same inputs" % rows)
        print("%-8s" % "kind" + "".join(" | %-27s" % n for n in forms))
        for k in R.KINDS:
            cols = R.columns_of(kd, k)
            line = "%-8s" % k
            for o in forms.values():
                v64, y64 = r["var"][cols], r["y"][:, cols]
                ev = (o["var"][cols].double() - v64).abs()
                ev = float((ev / v64).max()) if bool((v64 > 0).all()) else float(ev.max())
                ey = float((o["y"][:, cols].double() - y64).abs().max() / y64.abs().max())
                line += " | %-12.1e / %-12.1e" % (ev, ey)
            print(line)
