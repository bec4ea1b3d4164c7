"""The training-mode BatchNorm kernels on an MI355X, called through their ops.* wrappers, against the float64 reference of
tests/bn_ref.py at the shapes where they can go wrong: one short of, at and one past the 256-row chunks of the 16-byte form and the
1024-row chunks of the 4-byte form, 1281 rows (five one-pass chunks: chunk groups of 2, 2, 1 and 0), C on both sides of the 256-column
workgroup, both forms and calls that mix them (x, out, dy, dx aligned differently), object boundaries inside, at and across chunks.

Kernels: bn_stats_partial_v4 / bn_stats_finish_v4, bn_partial / bn_finish / bn_running_update, bn_apply / bn_apply_v4,
dropout_apply (csrc/bn.hip); bw_partial / bw_partial_v4, bw_finish / bw_finish2, bn_bwd_apply / bn_bwd_apply_v4, bn_bwd_pooled_sums,
bn_bwd_pooled_apply / _v4, colmax_arg, colsum_objects (csrc/backward.hip).

The inputs lay ten kinds of column side by side (bn_ref.make_case), so that one launch covers all of them and a 16-byte quad mixes
kinds: benign, mean = 1e3 std, constant 0.1, constant 0, one nonzero row, every chunk's first row an outlier, scale 1e-20, scale 1e15,
all-negative after BN, gamma = 0; a NaN and a +Inf element in tests of their own.

The bar is derived, not measured: per output tensor and per column kind |kernel - ref64| <= 4 max|oracle32 - ref64| + 4 eps32 max|ref64|,
oracle32 being the kernels' documented algorithm in float32 on the CPU; each kind is held to the bound its own columns give.  The
backward takes the statistics as operands, so both restatements get the ones the kernel gets.  Exact things are compared exactly:
constant and gamma = 0 columns, num_batches_tracked, the keys against the written activation, argmax rows outside bn_ref.ambiguous,
two runs of every call, the words around every tensor a wrapper allocates (`Guard`), the neighbours of a column slice, the columns next
to a NaN / Inf column, the absmax words.  Each comparison prints its error / bound ratio, each test the largest per kernel so far.

Headroom when this file was written (largest error / bound per wrapper and form over all cases): bn_bwd 4-byte form 0.90 (dx of the
K-outlier column at a handful of rows, where the bound rests on the two or three elements of one column; every other dx at most
0.42), bn_bwd 16-byte form 0.50 (dgamma, mean = 1e3 std), bn_bwd_pooled 0.41, bn_train 0.25 in both forms (the kernels
give oracle32's bits in most cases: error = oracle's error = a quarter of the bound), colsum 0.24 / 0.21, colsum_objects 0.18,
colmax_arg 0.17, bn_apply 0.13.  Against the kernels as they were before this file, 31 cases failed, all of them on the constant
columns of the 4-byte form, whose mean pass summed the raw values: mean 0.1 came back up to 2.4e-7 off (five times the bound) and the
variance nonzero; bn_finish_kernel now adds the first row back to a shifted sum.
"""
import pytest
import torch

from tests import bn_ref as R
from tests.test_loss_kernels_gpu import Guard, guarded, POISON

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
EPS = R.BN_EPS
RATIOS = {}
MODES = {0: (0, 0.0, False), 1: (1, 0.0, False), 2: (1, 0.2, False), 3: (1, 0.0, True)}   # act, slope, per-column slopes


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    from tgpose_amd import ops as _ops, _lib
    _lib.lib()  # raises if libtgpose_hip.so is missing: there is no fallback
    return _ops


def g(t):
    return None if t is None else t.to(DEV).contiguous()


def place(t, layout):
    """a CPU (rows, C) tensor on the device in one of the layouts -> (view, buffer); everything else in the buffer holds POISON"""
    rows, C = t.shape
    if layout == "C":
        buf = g(t)
        return buf, buf
    if layout in ("C+4", "C+1"):
        buf = torch.full((rows, C + int(layout[2:])), POISON, device=DEV, dtype=t.dtype)
        buf[:, :C] = t.to(DEV)
        return buf[:, :C], buf
    assert layout == "off1"
    buf = torch.full((rows * C + 8,), POISON, device=DEV, dtype=t.dtype)
    view = buf[1:1 + rows * C].view(rows, C)
    view.copy_(t.to(DEV))
    return view, buf


def neighbours_untouched(view, buf, layout):
    rows, C = view.shape
    if layout in ("C+4", "C+1"):
        return bool((buf[:, C:] == POISON).all())
    if layout == "off1":
        return bool((buf[:1] == POISON).all()) and bool((buf[1 + rows * C:] == POISON).all())
    return True


def vec_ok(C, *views):
    """the rule bn_vec_ok / bw_vec_ok state: C % 4, every row stride % 4, every pointer 16-byte aligned"""
    return C % 4 == 0 and all((v.stride(0) if v.dim() > 1 else 0) % 4 == 0 and v.data_ptr() % 16 == 0 for v in views)


def form_of(C, *views):
    return "v4" if vec_ok(C, *views) else "s"


def act32(beta, act, slope, sv):
    """act(beta) in float32, the value a constant or gamma = 0 column must hold in every row"""
    b = beta.to(F32)
    return torch.where(b > 0, b, b * (sv if sv is not None else torch.tensor(slope, dtype=F32))) if act else b


def held(kernel, name, got, ref64, ora32, kinds, skip_cols=None):
    """per column kind (the last dim is the columns): |got - ref64| within bn_ref.bound of that kind's columns; where both restatements
    give exactly 0 the kernel must.  skip_cols: columns bn_ref.ambiguous marks (their share is held to 1e-3)"""
    got = got.detach().cpu().double().reshape(ref64.shape)
    ref64, ora32 = ref64.detach().double(), ora32.detach().double()
    C = ref64.shape[-1]
    keep = torch.ones(C, dtype=torch.bool) if skip_cols is None else ~skip_cols[:C]
    assert R.excluded_share_ok(~keep), (kernel, name, "excluded share", int((~keep).sum()), C)
    for kind in R.KINDS:
        cols = R.columns_of(kinds[:C], kind) & keep
        if not bool(cols.any()):
            continue
        a, r, o = got[..., cols], ref64[..., cols], ora32[..., cols]
        assert bool(torch.isfinite(a).all()), (kernel, name, kind, "not finite")
        zero = (r == 0) & (o == 0)                                                    # a structural zero, not a cancellation
        assert bool((a[zero] == 0).all()), (kernel, name, kind, "both restatements are exactly 0, the kernel is not")
        b = R.bound(r, o)
        err = float((a - r).abs().max())
        ratio = err / b if b > 0 else (0.0 if err == 0 else float("inf"))
        RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
        print("%-14s %-10s %-8s err %.3e  bound %.3e  ratio %.3f" % (kernel, name, kind, err, b, ratio))
        assert ratio <= 1.0, (kernel, name, kind, err, b)


def headroom(*kernels):
    for k in kernels:
        print("largest error / bound so far: %-14s %.3f" % (k, RATIOS.get(k, 0.0)))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def exact_columns(kd, x, beta, mean, var, y, act, slope, sv):
    """constant columns: var == 0, mean == the constant, y == act(beta) in every row; gamma = 0 columns: y == act(beta)"""
    want = act32(beta, act, slope, sv)
    for kind in ("const", "zero", "gamma0"):
        cols = R.columns_of(kd, kind)
        if not bool(cols.any()):
            continue
        if kind != "gamma0" and mean is not None:
            assert torch.equal(var.cpu()[cols], torch.zeros(int(cols.sum()))), (kind, "variance", var.cpu()[cols])
            assert torch.equal(mean.cpu()[cols], x[0, cols]), (kind, "mean")
        assert torch.equal(y.cpu()[:, cols], want[cols].expand(y.shape[0], -1)), (kind, "y != act(beta)")


# ------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("C,layout,mode", R.C_CONFIGS)
@pytest.mark.parametrize("rows", R.ROWS)
def test_bn_train(ops, rows, C, layout, mode):
    cs = R.case(rows, C)
    x, gamma, beta, kd = cs["x"], cs["gamma"], cs["beta"], cs["kinds"]
    act, slope, vec = MODES[mode]
    sv = cs["slope_vec"] if vec else None
    momentum = (0.0, 0.1, 1.0)[(rows + C) % 3]
    ge = R.gen(rows, C, 11)
    rm0, rv0 = torch.randn(C, generator=ge), torch.rand(C, generator=ge) + 0.5
    xv, xbuf = place(x, layout)
    form = form_of(C, xv)
    assert form == ("v4" if C % 4 == 0 and layout in ("C", "C+4") else "s")
    dg_, db_, dsv = g(gamma), g(beta), g(sv)

    def run():
        rm, rv, nbt = g(rm0), g(rv0), torch.tensor([7], device=DEV)
        out = torch.empty(rows, C, device=DEV, dtype=F32)
        o, mean, var = ops.bn_train(xv, dg_, db_, EPS, act, slope, slope_vec=dsv, out=out, running=(rm, rv, momentum, nbt))
        assert o.data_ptr() == out.data_ptr()
        return o, mean, var, rm, rv, nbt

    out, mean, var, rm, rv, nbt = guarded(run)
    assert torch.equal(xv.cpu(), x) and neighbours_untouched(xv, xbuf, layout)              # out of place: x is an input
    args = (x, gamma, beta, EPS, act, slope, sv)
    r64 = R.ref64(*args, running=(rm0, rv0, momentum, torch.tensor(7)))
    o32 = R.oracle32(*args, running=(rm0, rv0, momentum, torch.tensor(7)), form=form)
    for name, got in (("mean", mean), ("var", var), ("y", out), ("rm", rm), ("rv", rv)):
        held("bn_train " + form, name, got, r64[name], o32[name], kd)
    assert int(nbt) == 8 == int(r64["nbt"])
    exact_columns(kd, x, beta, mean, var, out, act, slope, sv)
    # in place, no running buffers: the same bits
    xv2, xbuf2 = place(x, layout)
    o2, m2, v2 = ops.bn_train(xv2, dg_, db_, EPS, act, slope, slope_vec=dsv)
    assert o2.data_ptr() == xv2.data_ptr() and same_bits(o2, out) and same_bits(m2, mean) and same_bits(v2, var)
    assert neighbours_untouched(xv2, xbuf2, layout)
    headroom("bn_train v4", "bn_train s")


@pytest.mark.parametrize("x_layout,out_layout", [("C+4", "C"), ("C+1", "C"), ("off1", "C"), ("C", "off1"), ("C", "C+1"), ("C", "C+4"),
                                                 ("C+1", "C+1"), ("off1", "off1")])
@pytest.mark.parametrize("rows", R.LAYOUT_ROWS)
def test_bn_train_mixed_forms(ops, rows, x_layout, out_layout):
    """statistics and apply pick their form separately: x decides the first, x and out (and cm_cols) the second"""
    C = R.LAYOUT_C
    cs = R.case(rows, C)
    x, gamma, beta, kd, sv = cs["x"], cs["gamma"], cs["beta"], cs["kinds"], cs["slope_vec"]
    xv, xbuf = place(x, x_layout)
    form = form_of(C, xv)
    dg_, db_, dsv = g(gamma), g(beta), g(sv)
    res = []
    for _ in range(2):
        ov, obuf = place(torch.full((rows, C), POISON), out_layout)
        keys = torch.zeros(1, C + 3, dtype=torch.int32, device=DEV)
        o, mean, var = ops.bn_train(xv, dg_, db_, EPS, 1, 0.0, slope_vec=dsv, out=ov, colmax_keys=keys[:, :C], cm_cols=C, rows_per_obj=rows)
        torch.cuda.synchronize()
        assert neighbours_untouched(ov, obuf, out_layout) and bool((keys[:, C:] == 0).all())
        res.append((o, mean, var, keys))
    assert all(same_bits(a, b) for a, b in zip(*res))
    out, mean, var, keys = res[0]
    assert torch.equal(xv.cpu(), x) and neighbours_untouched(xv, xbuf, x_layout)
    r64, o32 = R.ref64(x, gamma, beta, EPS, 1, 0.0, sv), R.oracle32(x, gamma, beta, EPS, 1, 0.0, sv, form=form)
    for name, got in (("mean", mean), ("var", var), ("y", out)):
        held("bn_train " + form, name, got, r64[name], o32[name], kd)
    exact_columns(kd, x, beta, mean, var, out, 1, 0.0, sv)
    assert torch.equal(ops.colmax_decode(keys[:, :C].contiguous()).cpu(), out.cpu().max(0, keepdim=True)[0])
    headroom("bn_train v4", "bn_train s")


@pytest.mark.parametrize("rows,rpo,C,cm", R.POOL_CASES)
def test_bn_train_colmax_keys(ops, rows, rpo, C, cm):
    """in place with the per-object maxima as keys: they decode to exactly the max of the written activation -- all-negative columns
    (ReLU leaves -0, LeakyReLU negatives), objects that end inside, at and across chunks, cm_cols < C, cm_cols % 4 != 0 (16-byte
    statistics, 4-byte apply); want_out = False leaves x alone and gives the same keys"""
    cs = R.case(rows, C)
    x, gamma, beta, kd, sv = cs["x"], cs["gamma"], cs["beta"], cs["kinds"], cs["slope_vec"]
    objects = rows // rpo
    dg_, db_, dsv = g(gamma), g(beta), g(sv)
    form = form_of(C, g(x))
    res = []
    for want_out in (True, True, False):
        xv = g(x)
        keys = torch.zeros(objects, cm + 5, dtype=torch.int32, device=DEV)
        o, mean, var = ops.bn_train(xv, dg_, db_, EPS, 1, 0.0, slope_vec=dsv, colmax_keys=keys[:, :cm], cm_cols=cm, rows_per_obj=rpo,
                                    want_out=want_out)
        torch.cuda.synchronize()
        assert bool((keys[:, cm:] == 0).all())
        assert (o is None and torch.equal(xv.cpu(), x)) if not want_out else o.data_ptr() == xv.data_ptr()
        res.append((o, mean, var, keys))
    assert all(same_bits(a, b) for a, b in zip(res[0], res[1]))
    assert all(same_bits(a, b) for a, b in zip(res[0][1:], res[2][1:]))
    out, mean, var, keys = res[0]
    got = ops.colmax_decode(keys[:, :cm].contiguous()).cpu()
    assert torch.equal(got, out.cpu().view(objects, rpo, C)[:, :, :cm].max(1)[0])            # exactly the written values
    r64 = R.ref64(x, gamma, beta, EPS, 1, 0.0, sv, rows_per_obj=rpo, cm_cols=cm)
    o32 = R.oracle32(x, gamma, beta, EPS, 1, 0.0, sv, rows_per_obj=rpo, cm_cols=cm, form=form)
    held("bn_train " + form, "y", out, r64["y"], o32["y"], kd)
    held("bn_train " + form, "colmax", got, r64["colmax"], o32["colmax"], kd)
    neg = R.columns_of(kd, "neg")[:cm]
    if bool(neg.any()):
        assert bool((got[:, neg] <= 0).all()) and bool((r64["colmax"][:, neg] <= 0).all())
    exact_columns(kd, x, beta, mean, var, out, 1, 0.0, sv)
    headroom("bn_train v4", "bn_train s")


@pytest.mark.parametrize("rows,C,layout", [(3, 4, "C"), (257, 64, "C+4"), (1025, 63, "C"), (1281, 260, "C"), (2049, 3, "C+1")])
def test_bn_apply(ops, rows, C, layout):
    """fixed statistics (eval mode): no statistics kernel in the way of the apply kernel's own error"""
    cs = R.case(rows, C)
    x, gamma, beta, kd = cs["x"], cs["gamma"], cs["beta"], cs["kinds"]
    stats = R.stats32(x, "v4")
    xv, xbuf = place(x, layout)
    for act, slope in ((0, 0.0), (1, 0.0), (1, 0.2)):
        y = guarded(lambda: ops.bn_apply(xv, g(stats[0]), g(stats[1]), g(gamma), g(beta), EPS, act, slope))
        r64, o32 = R.ref64(x, gamma, beta, EPS, act, slope, stats=stats), R.oracle32(x, gamma, beta, EPS, act, slope, stats=stats)
        held("bn_apply", "y", y, r64["y"], o32["y"], kd)
        exact_columns(kd, x, beta, None, None, y, act, slope, None)
    assert torch.equal(xv.cpu(), x) and neighbours_untouched(xv, xbuf, layout)
    headroom("bn_apply")


# ------------------------------------------------------------------------------------------------------------------- backward
def _bwd_case(rows, C, kinds=R.KINDS):
    cs = R.case(rows, C, kinds)
    dy = torch.randn(rows, C, generator=R.gen(rows, C, 21))
    return cs, dy


def _check_bwd(kernel, got, r64, o32, kd, skip):
    for name, t in zip(("dx", "dgamma", "dbeta"), got):
        held(kernel, name, t, r64[name], o32[name], kd, skip_cols=skip)


@pytest.mark.parametrize("C,layout,mode", R.C_CONFIGS)
@pytest.mark.parametrize("rows", R.ROWS)
def test_bn_bwd(ops, rows, C, layout, mode):
    cs, dy = _bwd_case(rows, C)
    x, gamma, beta, kd = cs["x"], cs["gamma"], cs["beta"], cs["kinds"]
    act, slope, vec = MODES[mode]
    sv = cs["slope_vec"] if vec else None
    xv, xbuf = place(x, layout)
    dyv, dybuf = place(dy, layout)
    form = form_of(C, xv, dyv)
    stats = R.stats32(x, form)                                   # operands of the backward: what the forward of this form hands over
    dm, dv, dg_, db_, dsv = g(stats[0]), g(stats[1]), g(gamma), g(beta), g(sv)

    def run():
        dx = torch.empty(rows, C, device=DEV, dtype=F32)
        r = ops.bn_bwd(dyv, xv, dm, dv, dg_, db_, EPS, act, slope, slope_vec=dsv, dx=dx, want_scale=True)
        assert r[0].data_ptr() == dx.data_ptr()
        return r + ((getattr(r[0], "_tgp_scale", None),))

    dx, dgam, dbet, sc = guarded(run)
    assert torch.equal(xv.cpu(), x) and torch.equal(dyv.cpu(), dy)
    assert neighbours_untouched(xv, xbuf, layout) and neighbours_untouched(dyv, dybuf, layout)
    args = (dy, x, gamma, beta, EPS, act, slope, sv)
    r64, o32 = R.ref64_bwd(*args, stats=stats), R.oracle32_bwd(*args, stats=stats, form=form)
    skip = R.ambiguous(x, gamma, beta, EPS, stats=stats)["cols"] if act else None
    _check_bwd("bn_bwd " + form, (dx, dgam, dbet), r64, o32, kd, skip)
    assert (sc is not None) == (form == "v4")                    # the scale rides on the 16-byte form only
    if sc is not None:
        top = dx.abs().max()
        assert sc[2].item() == top.item() and sc[0].item() * sc[1].item() == 1.0 and top.item() * sc[0].item() <= 32768.0
    # in place on dy (the default): the same bits, the neighbours of dy untouched
    dyv2, dybuf2 = place(dy, layout)
    dx2, dg2, db2 = ops.bn_bwd(dyv2, xv, dm, dv, dg_, db_, EPS, act, slope, slope_vec=dsv)
    assert dx2.data_ptr() == dyv2.data_ptr() and same_bits(dx2, dx) and same_bits(dg2, dgam) and same_bits(db2, dbet)
    assert neighbours_untouched(dyv2, dybuf2, layout)
    headroom("bn_bwd v4", "bn_bwd s")


@pytest.mark.parametrize("dy_layout,x_layout,dx_layout", [("C", "C", "off1"), ("C", "C", "C+1"), ("C", "C+1", "C"), ("off1", "C", "C"),
                                                          ("C+4", "C", "C+4"), ("C+4", "C+4", "C+1")])
@pytest.mark.parametrize("rows", R.LAYOUT_ROWS)
def test_bn_bwd_mixed_forms(ops, rows, dy_layout, x_layout, dx_layout):
    """dy, x, dx and the workspace must all qualify for the 16-byte form: one misaligned operand sends the call to the 4-byte kernels"""
    C = R.LAYOUT_C
    cs, dy = _bwd_case(rows, C)
    x, gamma, beta, kd, sv = cs["x"], cs["gamma"], cs["beta"], cs["kinds"], cs["slope_vec"]
    xv, _ = place(x, x_layout)
    dyv, _ = place(dy, dy_layout)
    stats = R.stats32(x, form_of(C, xv))
    res = []
    for _ in range(2):
        dxv, dxbuf = place(torch.full((rows, C), POISON), dx_layout)
        form = form_of(C, xv, dyv, dxv)
        r = ops.bn_bwd(dyv, xv, g(stats[0]), g(stats[1]), g(gamma), g(beta), EPS, 1, 0.0, slope_vec=g(sv), dx=dxv, want_scale=True)
        torch.cuda.synchronize()
        assert neighbours_untouched(dxv, dxbuf, dx_layout) and (getattr(r[0], "_tgp_scale", None) is not None) == (form == "v4")
        res.append(r)
    assert all(same_bits(a, b) for a, b in zip(*res))
    assert torch.equal(xv.cpu(), x) and torch.equal(dyv.cpu(), dy)
    args = (dy, x, gamma, beta, EPS, 1, 0.0, sv)
    _check_bwd("bn_bwd " + form, res[0], R.ref64_bwd(*args, stats=stats), R.oracle32_bwd(*args, stats=stats, form=form), kd,
               R.ambiguous(x, gamma, beta, EPS, stats=stats)["cols"])
    headroom("bn_bwd v4", "bn_bwd s")


def _raw_bn_bwd(dy, x, stats, gamma, beta, act, slope, dx, bits):
    """tgp_bn_bwd itself (ops.bn_bwd only asks for the absmax words where the 16-byte form will run) -> return code, dgamma, dbeta"""
    from tgpose_amd import _lib
    from tgpose_amd.ops import _p, _stream
    rows, C = x.shape
    dg, db = torch.full((C,), POISON, device=DEV), torch.full((C,), POISON, device=DEV)
    ws = torch.empty(max(int(_lib.lib().tgp_bw_workspace_floats(rows, C)), 1), device=DEV, dtype=F32)
    rc = _lib.lib().tgp_bn_bwd(_p(dy), dy.stride(0), _p(x), x.stride(0), rows, C, _p(stats[0]), _p(stats[1]), float(EPS), _p(gamma), _p(beta),
                               act, float(slope), None, _p(dx), dx.stride(0), _p(dg), _p(db), _p(ws), _p(bits), _stream(x))
    torch.cuda.synchronize()
    return rc, dg, db


def _tile_bits(dx, words):
    """the word of workgroup (bx, by): the bits of max |dx| over its 256 rows x 256 columns, 0x7fc00000 once one of them is not finite"""
    rows, C = dx.shape
    gx = -(-C // 256)
    want = torch.zeros_like(words)
    for by in range(-(-rows // 256)):
        for bx in range(gx):
            tile = dx[by * 256:(by + 1) * 256, bx * 256:(bx + 1) * 256]
            want[by * gx + bx] = 0x7fc00000 if not bool(torch.isfinite(tile).all()) else int(tile.abs().max().view(torch.int32))
    return want


@pytest.mark.parametrize("bad", [None, "nan", "inf"])
@pytest.mark.parametrize("rows,C", [(257, 64), (1281, 260)])
def test_bn_bwd_absmax_words(ops, rows, C, bad):
    from tgpose_amd import _lib
    cs, dy = _bwd_case(rows, C)
    x, gamma, beta = cs["x"], cs["gamma"], cs["beta"]
    if bad:
        dy[rows - 2, C - 3] = float(bad)                         # (at C = 260: in the second workgroup's only live quad)
    stats = R.stats32(x, "v4")
    n = int(_lib.lib().tgp_bn_bwd_absmax_words(rows, C))
    assert n == -(-C // 256) * -(-rows // 256)
    dev = [g(t) for t in (dy, x, stats[0], stats[1], gamma, beta)]
    res = []
    for _ in range(2):
        bits = torch.full((n + 2,), 0x55555555, dtype=torch.int32, device=DEV)
        dx = torch.full((rows, C), POISON, device=DEV)
        rc, dg, db = _raw_bn_bwd(dev[0], dev[1], dev[2:4], dev[4], dev[5], 1, 0.2, dx, bits[1:1 + n])
        assert rc == 0 and bits[0].item() == 0x55555555 == bits[-1].item()
        res.append((dx, dg, db, bits))
    assert all(same_bits(a, b) for a, b in zip(*res))
    dx, _, _, bits = res[0]
    words = bits[1:1 + n].cpu()
    assert torch.equal(words, _tile_bits(dx.cpu(), words))
    finite = bool(torch.isfinite(dx).all())
    assert finite == (bad is None)
    assert int(words.max()) == (int(dx.abs().max().view(torch.int32)) if finite else 0x7fc00000)
    if bad:                                                      # the bad column is not finite from top to bottom, every other one is
        nf = ~torch.isfinite(dx.cpu())
        assert bool(nf[:, C - 3].all()) and int(nf.sum()) == rows


@pytest.mark.parametrize("rows,rpo,C,cm", R.POOL_CASES)
@pytest.mark.parametrize("layout", ["C", "C+4", "C+1"])
def test_bn_bwd_pooled(ops, rows, rpo, C, cm, layout):
    """the gradient of the per-object maxima lands on the recorded row; argrow is an operand (the reference's own argmax)"""
    cs = R.case(rows, C)
    x, gamma, beta, kd, sv = cs["x"], cs["gamma"], cs["beta"], cs["kinds"], cs["slope_vec"]
    objects = rows // rpo
    xv, xbuf = place(x, layout)
    stats = R.stats32(x, form_of(C, xv))
    fwd = R.ref64(x, gamma, beta, EPS, 1, 0.0, sv, rows_per_obj=rpo, stats=stats)
    arg = fwd["argrow"]
    dpool = torch.randn(objects, C, generator=R.gen(rows, rpo, C))
    dev = [g(t) for t in (dpool, arg, stats[0], stats[1], gamma, beta, sv)]

    def run():
        return ops.bn_bwd_pooled(dev[0], dev[1], xv, rpo, dev[2], dev[3], dev[4], dev[5], EPS, 1, 0.0, slope_vec=dev[6])

    got = guarded(run)
    assert torch.equal(xv.cpu(), x) and neighbours_untouched(xv, xbuf, layout)
    args = (dpool, arg, x, gamma, beta, EPS, 1, 0.0, sv)
    r64, o32 = R.ref64_bwd_pooled(*args, stats=stats), R.oracle32_bwd_pooled(*args, stats=stats)
    amb = R.ambiguous(x, gamma, beta, EPS, stats=stats)["z"]
    skip = torch.gather(amb, 0, arg.long()).any(0)               # only the decisions on the recorded rows enter
    _check_bwd("bn_bwd_pooled", got, r64, o32, kd, skip)
    # into a column slice of a wider buffer
    dxv, dxbuf = place(torch.full((rows, C), POISON), layout)
    again = ops.bn_bwd_pooled(dev[0], dev[1], xv, rpo, dev[2], dev[3], dev[4], dev[5], EPS, 1, 0.0, slope_vec=dev[6], dx=dxv)
    assert all(same_bits(a, b) for a, b in zip(again, got)) and neighbours_untouched(dxv, dxbuf, layout)
    headroom("bn_bwd_pooled")


@pytest.mark.parametrize("rows,rpo,C,cm", R.POOL_CASES)
def test_colmax_arg(ops, rows, rpo, C, cm):
    """the per-object max with its row: the value is exactly the activation bn_apply writes, the row the reference's outside near-ties"""
    cs = R.case(rows, C, R.NO_TIES)
    x, gamma, beta, kd = cs["x"], cs["gamma"], cs["beta"], cs["kinds"]
    objects = rows // rpo
    xv, xbuf = place(x, "C+4" if C % 2 == 0 else "C+1")
    stats = R.stats32(x, form_of(C, xv))
    dev = [g(t) for t in (stats[0], stats[1], gamma, beta)]
    for act, slope in ((0, 0.0), (1, 0.0), (1, 0.2)):
        out, arg = guarded(lambda: ops.colmax_arg(xv, objects, rpo, bn=tuple(dev), act=act, slope=slope, eps=EPS))
        r64 = R.ref64(x, gamma, beta, EPS, act, slope, rows_per_obj=rpo, stats=stats)
        o32 = R.oracle32(x, gamma, beta, EPS, act, slope, rows_per_obj=rpo, stats=stats)
        held("colmax_arg", "max", out, r64["colmax"], o32["colmax"], kd)
        y = ops.bn_apply(xv, dev[0], dev[1], dev[2], dev[3], EPS, act, slope).cpu()
        val, where = R._pool(y, rpo, C)
        assert torch.equal(out.cpu(), val) and torch.equal(arg.cpu(), where)                    # against the written activation: exactly
        amb = R.ambiguous(x, gamma, beta, EPS, stats=stats, rows_per_obj=rpo, act=act, slope=slope)["arg"]
        assert R.excluded_share_ok(amb)
        assert torch.equal(arg.cpu()[~amb], r64["argrow"][~amb])
    out, arg = guarded(lambda: ops.colmax_arg(xv, objects, rpo))
    val, where = R._pool(x, rpo, C)
    assert torch.equal(out.cpu(), val) and torch.equal(arg.cpu(), where)                        # no BatchNorm: a plain max, first row on ties
    assert neighbours_untouched(xv, xbuf, "C+4" if C % 2 == 0 else "C+1")
    headroom("colmax_arg")


@pytest.mark.parametrize("C,layout", [(64, "C"), (63, "C"), (260, "C+4"), (3, "C+1"), (64, "off1")])
@pytest.mark.parametrize("rows", R.ROWS)
def test_colsum(ops, rows, C, layout):
    cs = R.case(rows, C)
    dy, kd = cs["x"], cs["kinds"]
    dyv, dybuf = place(dy, layout)
    form = form_of(C, dyv)
    r64, o32 = R.colsum(dy), R.colsum32(dy, form)
    got = guarded(lambda: ops.colsum(dyv))
    held("colsum " + form, "sum", got, r64, o32, kd)
    base = torch.randn(C, generator=R.gen(rows, C, 31))
    acc = g(base)
    assert ops.colsum(dyv, out=acc, accumulate=True).data_ptr() == acc.data_ptr()
    held("colsum " + form, "accumulate", acc, base.double() + r64, base + o32, kd)
    assert torch.equal(dyv.cpu(), dy) and neighbours_untouched(dyv, dybuf, layout)
    headroom("colsum v4", "colsum s")


@pytest.mark.parametrize("rows,rpo,C,cm", R.POOL_CASES)
def test_colsum_objects(ops, rows, rpo, C, cm):
    cs = R.case(rows, C)
    dy, kd = cs["x"].view(rows // rpo, rpo, C), cs["kinds"]
    got = guarded(lambda: ops.colsum_objects(g(dy)))
    held("colsum_objects", "sum", got, R.colsum_objects(dy), R.colsum_objects32(dy), kd)
    wide = torch.full((rows, C + 3), POISON, device=DEV)
    wide[:, :C] = g(cs["x"])
    sliced = torch.as_strided(wide, (rows // rpo, rpo, C), (rpo * (C + 3), C + 3, 1))
    assert same_bits(ops.colsum_objects(sliced), got) and bool((wide[:, C:] == POISON).all())
    headroom("colsum_objects")


# ------------------------------------------------------------------------------------------------------------------- NaN / Inf
@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("row", [0, 256, 700, 1280])
@pytest.mark.parametrize("rows,C", R.NAN_CASES)
def test_nan_inf_stay_in_their_column(ops, rows, C, row, bad):
    """one bad element in column 5 (row 0 and 256 are a chunk's K, 1280 the lone row of the last one-pass chunk): the column is NaN
    where PyTorch's is (mean, variance, y, the running buffers, dx, dgamma, dbeta; where PyTorch keeps an Inf -- the mean of the Inf
    column -- it is not finite), every other column holds the bits of the run without the bad element, and the key of the column's
    maximum decodes to NaN"""
    cs, dy = _bwd_case(rows, C)
    x, gamma, beta, sv = cs["x"], cs["gamma"], cs["beta"], cs["slope_vec"]
    col = 5
    xb = x.clone()
    xb[row, col] = float(bad)
    ge = R.gen(rows, C, 41)
    rm0, rv0 = torch.randn(C, generator=ge), torch.rand(C, generator=ge) + 0.5
    dev = [g(t) for t in (gamma, beta, sv, dy)]

    def run(xin):
        rm, rv, nbt = g(rm0), g(rv0), torch.tensor([0], device=DEV)
        xv = g(xin)
        keys = torch.zeros(1, C - C % 4, dtype=torch.int32, device=DEV)
        y, mean, var = ops.bn_train(xv, dev[0], dev[1], EPS, 1, 0.0, slope_vec=dev[2], out=torch.empty_like(xv), running=(rm, rv, 0.1, nbt),
                                    colmax_keys=keys, cm_cols=C - C % 4, rows_per_obj=rows)
        dx, dgam, dbet = ops.bn_bwd(dev[3], xv, mean, var, dev[0], dev[1], EPS, 1, 0.0, slope_vec=dev[2], dx=torch.empty_like(xv),
                                    want_scale=True)
        return dict(mean=mean, var=var, y=y, rm=rm, rv=rv, dx=dx, dgamma=dgam, dbeta=dbet, colmax=ops.colmax_decode(keys),
                    scale=getattr(dx, "_tgp_scale", None), nbt=nbt)

    clean, dirty = run(x), run(xb)
    torch.cuda.synchronize()
    assert int(dirty["nbt"]) == 1
    # PyTorch on the same input, float32 on the CPU
    xt, gt, bt = xb.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    trm, trv = rm0.clone(), rv0.clone()
    z = torch.nn.functional.batch_norm(xt, trm, trv, gt, bt, True, 0.1, EPS)
    yt = torch.where(z > 0, z, z * sv)
    yt.backward(dy)
    want = dict(mean=xb.mean(0), var=xb.var(0, unbiased=False), y=yt.detach(), rm=trm, rv=trv, dx=xt.grad, dgamma=gt.grad, dbeta=bt.grad)
    others = torch.arange(C) != col
    for name, w in want.items():
        got_c, got_d = clean[name].cpu(), dirty[name].cpu()
        assert same_bits(got_c[..., others], got_d[..., others]), (name, "a neighbour of the bad column moved")
        assert bool(torch.isfinite(got_c).all()), name
        wc, gc = w[..., col], got_d[..., col]
        assert bool(torch.isnan(gc)[torch.isnan(wc)].all()), (name, "PyTorch has NaN, the kernel has not")
        assert bool((~torch.isfinite(gc))[~torch.isfinite(wc)].all()), (name, "PyTorch is not finite, the kernel is")
    assert bool(torch.isnan(want["y"][:, col]).all()) and bool(torch.isnan(want["dx"][:, col]).all())          # what the above demanded
    assert bool(torch.isnan(want["var"][col])) and bool(torch.isnan(want["rv"][col])) and not bool(torch.isfinite(want["rm"][col]))
    if col < C - C % 4:
        km_c, km_d = clean["colmax"].cpu()[0], dirty["colmax"].cpu()[0]
        assert bool(torch.isnan(km_d[col])) and same_bits(km_c[others[:km_c.numel()]], km_d[others[:km_c.numel()]])
    if clean["scale"] is not None:                               # the word is 0x7fc00000: the scale kernel answers 1 and hands the NaN on
        sc = dirty["scale"].cpu()
        assert bool(torch.isnan(sc[2])) and sc[0].item() == 1.0 and clean["scale"][2].item() == clean["dx"].abs().max().item()


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(ops):
    from tgpose_amd import _lib
    C = 8
    x = torch.randn(6, C, generator=R.gen(1)).to(DEV)
    gamma, beta, mean, var = (torch.ones(C, device=DEV) for _ in range(4))
    narrow = torch.as_strided(x, (6, C), (C - 1, 1))             # ld < C
    empty_rows = torch.empty(0, C, device=DEV)
    out = torch.full((6, C), POISON, device=DEV)
    rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.tensor([3], device=DEV)
    calls = [lambda: ops.bn_train(narrow, gamma, beta, out=out), lambda: ops.bn_train(empty_rows, gamma, beta, out=out),
             lambda: ops.bn_train(x[:1], gamma, beta, out=out, running=(rm, rv, 0.1, nbt)),       # one row has no unbiased variance
             lambda: ops.bn_train(x, gamma, beta, out=out, running=(rm, rv, 1.5, nbt)),
             lambda: ops.bn_apply(narrow, mean, var, gamma, beta), lambda: ops.bn_apply(empty_rows, mean, var, gamma, beta),
             lambda: ops.bn_bwd(narrow, x, mean, var, gamma, beta, dx=out), lambda: ops.bn_bwd(x, narrow, mean, var, gamma, beta, dx=out),
             lambda: ops.bn_bwd(x, x, mean, var, gamma, beta, dx=narrow), lambda: ops.bn_bwd(empty_rows, empty_rows, mean, var, gamma, beta),
             lambda: ops.colsum(narrow), lambda: ops.colsum(empty_rows),
             lambda: ops.bn_bwd_pooled(torch.ones(2, C, device=DEV), torch.zeros(2, C, dtype=torch.int32, device=DEV), narrow, 3,
                                       mean, var, gamma, beta, dx=out),
             lambda: ops.colmax_arg(narrow, 2, 3), lambda: ops.dropout(x, 1.0)]
    for call in calls:
        with pytest.raises(_lib.TgpError, match="TGP_EINVAL"):
            call()
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and int(nbt) == 3 and bool((rm == 0).all()) and bool((rv == 1).all())
    assert ops.bn_train(x[:2].clone(), gamma, beta, running=(rm, rv, 0.1, nbt))[0].shape == (2, C) and int(nbt) == 4   # two rows: accepted
    # the absmax words on the 4-byte form: TGP_EUNSUPPORTED, nothing written
    rows, C = 6, 6
    t = [torch.ones(rows, C, device=DEV), torch.ones(rows, C, device=DEV)]
    stats = (torch.zeros(C, device=DEV), torch.ones(C, device=DEV))
    bits = torch.full((4,), 0x55555555, dtype=torch.int32, device=DEV)
    dx = torch.full((rows, C), POISON, device=DEV)
    rc, dg, db = _raw_bn_bwd(t[0], t[1], stats, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), 0, 0.0, dx, bits)
    assert rc == _lib.EUNSUPPORTED
    assert bool((dx == POISON).all()) and bool((dg == POISON).all()) and bool((db == POISON).all()) and bool((bits == 0x55555555).all())
    # ... and so does ops.bn_bwd there: no scale attached, the gradients computed
    dx, _, _ = ops.bn_bwd(t[0].clone(), t[1], stats[0], stats[1], torch.ones(C, device=DEV), torch.zeros(C, device=DEV), want_scale=True)
    assert getattr(dx, "_tgp_scale", None) is None and bool(torch.isfinite(dx).all())


# ------------------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("p", [0.5, 0.75, 0.2])
@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_dropout(ops, count, p):
    """kept elements are x / (1 - p) in float32 exactly, formed as nn.Dropout forms it -- x * (1 / (1 - p)), the factor rounded to
    float32 (for p = 0.5 and 0.75 that is the quotient itself) --, dropped ones exactly 0; the mask is the generator's"""
    x = torch.randn(count, generator=R.gen(count)) + 3.0          # (no zeros among the inputs: a 0 in y is a dropped element)
    gen = torch.Generator(device=DEV).manual_seed(count)
    y = guarded(lambda: ops.dropout(g(x), p, gen.manual_seed(count)))
    keep = (torch.rand(x.shape, device=DEV, generator=gen.manual_seed(count)) >= p).cpu()
    one = torch.tensor(1.0, dtype=F32)
    want = torch.where(keep, x * (one / (one - torch.tensor(p, dtype=F32))), torch.zeros(()))
    assert same_bits(y.cpu(), want)
    if p in (0.5, 0.75):
        assert torch.equal(y.cpu()[keep], (x / (1.0 - p))[keep])
    other = ops.dropout(g(x), p, gen.manual_seed(count + 1))
    assert count < 255 or not torch.equal(other, y)              # another seed, another mask
    xd = g(x)
    assert ops.dropout(xd, 0.0) is xd                            # p = 0: the input itself
