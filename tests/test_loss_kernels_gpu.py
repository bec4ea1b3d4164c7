"""The loss and pose-glue kernels on an MI355X, called through their ops.* wrappers, against the float64 reference of
tests/loss_kernels_ref.py at the shapes where they can go wrong: one short of, at and one past every workgroup stride (256 objects,
256 points, 64 objects), the N = 1024 switch of the symmetric-reconstruction workspace, the 4096-point LDS histograms of dcd, all five
symmetry modes by every route, batches whose objects are all symmetric, exact ties (pred == gt, |pred - gt| == beta, all-zero feature
rows, a zero axis), NaN / Inf operands.

Kernels: tgp_pose_terms_fwd/bwd, tgp_sym_recon_fwd/bwd, tgp_rowl1_fwd/bwd, tgp_feat_consistency_fwd/bwd (csrc/tdaloss.hip),
tgp_dcd_fwd/bwd, tgp_canonicalize, tgp_generate_rt, tgp_pose_transform_fwd/bwd (csrc/dcd.hip), tgp_pose_rotation_fwd/bwd,
tgp_head_post_bwd (csrc/poserot.hip) and tgp_head_post.

The bar is derived, not measured: per output tensor |kernel - ref64| <= 4 max|oracle32 - ref64| + 4 eps32 max|ref64|, oracle32 being the
same restatement in float32 on the CPU (the factor covers the kernels' fixed summation trees and the device's expf / powf / acosf).
Where one tensor mixes rows of very different conditioning -- axis pairs 1e-3 apart, rows F.normalize floors, a zero axis -- the rows
are held group by group, each to the bound its own rows give.  Exact things are compared exactly: the valid count, every gradient the
reference gives as 0, the NaN / 0 branches, the loss bits with and without weights, two runs of each kernel, and the words around
every tensor a wrapper allocates (`Guard`).  Sign-dependent gradients leave out the elements loss_kernels_ref.ambiguous marks, at
most 1e-3 of a tensor.  Each comparison prints its error / bound ratio, each test the largest per kernel so far.

Headroom when this file was written (largest error / bound per kernel over all cases): pose_transform_bwd 0.96 (d s at B = 1: the
kernel adds its 256 per-thread partials one after the other, a sum whose terms cancel, while the float32 restatement's pairwise sum
happens to be nearly exact there), generate_rt 0.59, pose_rotation_fwd and canonicalize 0.54, pose_rotation_bwd 0.44,
pose_terms_bwd 0.37, sym_recon_fwd 0.36, every other kernel at most 0.27.
"""
import ctypes
import math

import pytest
import torch

from tests import loss_kernels_ref as K
from tests.util import rand_rotations

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
POISON = 12345.0
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    from tgpose_amd import ops as _ops, _lib
    _lib.lib()  # raises if libtgpose_hip.so is missing: there is no fallback
    return _ops


def g(t):
    return None if t is None else t.to(DEV).contiguous()


def gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


class Guard(object):
    """Inside the block every tensor a wrapper allocates with torch.empty / torch.empty_like lies in the middle of a poisoned buffer;
    check() asserts that the words in front of it and after it (the tail beyond n) were left alone.  The tensor itself starts out
    poisoned too, so an element a kernel skips shows up in the comparison."""
    WORDS = 64

    def __enter__(self):
        self.bufs, self._empty, self._like = [], torch.empty, torch.empty_like
        real = self._empty

        def empty(*size, **kw):
            shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
            n = int(math.prod(shape))
            buf = real(n + 2 * Guard.WORDS, device=kw.get("device"), dtype=kw.get("dtype", F32))
            buf.fill_(POISON)
            self.bufs.append((buf, n))
            return buf[Guard.WORDS:Guard.WORDS + n].view(shape)

        torch.empty, torch.empty_like = empty, lambda t, **kw: empty(t.shape, device=t.device, dtype=t.dtype)
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self._empty, self._like
        return False

    def check(self):
        assert self.bufs
        for buf, n in self.bufs:
            assert bool((buf[:Guard.WORDS] == POISON).all()) and bool((buf[Guard.WORDS + n:] == POISON).all()), (tuple(buf.shape), n)


def guarded(fn):
    """fn() twice under a Guard: the words around every output untouched, the two runs bit for bit alike -> the first run's outputs"""
    res = []
    for _ in range(2):
        with Guard() as gd:
            out = fn()
        torch.cuda.synchronize()
        gd.check()
        res.append(out)
    flat = lambda o: [t for t in (o if isinstance(o, (tuple, list)) else (o,)) if torch.is_tensor(t)]
    for a, b in zip(flat(res[0]), flat(res[1])):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), "two runs differ"
    return res[0]


def held(kernel, name, got, ref64, ora32, exclude=None, rows=None):
    """|got - ref64| within loss_kernels_ref.bound of the tensor (of its `rows`, when given); where the reference is exactly 0 the
    kernel must be; `exclude` marks sign-ambiguous elements (their share is held to 1e-3)"""
    got = got.detach().cpu().double().reshape(ref64.shape)
    ref64, ora32 = ref64.detach().double(), ora32.detach().double()
    if rows is not None:
        if int(rows.sum()) == 0:
            return
        got, ref64, ora32 = got[rows], ref64[rows], ora32[rows]
        exclude = None if exclude is None else exclude[rows]
    keep = torch.ones_like(ref64, dtype=torch.bool) if exclude is None else ~exclude
    assert K.excluded_share_ok(~keep), (kernel, name, "excluded share", float((~keep).double().mean()))
    assert bool(torch.isfinite(got[keep]).all()), (kernel, name, "not finite")
    zero = keep & (ref64 == 0) & (ora32 == 0)                                        # a structural zero, not a cancellation
    assert bool((got[zero] == 0).all()), (kernel, name, "the reference is exactly 0, the kernel is not", int((got[zero] != 0).sum()))
    b = K.bound(ref64, ora32)
    err = float(((got - ref64).abs() * keep).max()) if got.numel() else 0.0
    ratio = err / b if b > 0 else (0.0 if err == 0 else float("inf"))
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print("%-22s %-28s err %.3e  bound %.3e  ratio %.3f  excluded %d of %d" % (kernel, name, err, b, ratio, int((~keep).sum()), keep.numel()))
    assert ratio <= 1.0, (kernel, name, err, b)


def headroom(*kernels):
    for k in kernels:
        print("largest error / bound so far: %-22s %.3f" % (k, RATIOS.get(k, 0.0)))


# ---------------------------------------------------------------------------------------------------------------- pose terms
def _pose_case(B, width, pattern):
    """operands near their targets; for B >= 2 row 0 sits exactly on the smooth-L1 knee (pred - gt == +-beta in every field, gt on a 1/8
    grid so the subtraction is exact) and row B - 1 has pred == gt in every field with confidences exp(0) = 1"""
    ge = gen(B, width, len(pattern))
    unit = lambda v: v / v.norm(dim=1, keepdim=True)
    g1, g2 = unit(torch.randn(B, 3, generator=ge)), unit(torch.randn(B, 3, generator=ge))
    gt_, gs = torch.randint(-8, 9, (B, 3), generator=ge) / 8.0, torch.randint(1, 9, (B, 3), generator=ge) / 8.0
    r1, r2 = unit(g1 + 0.15 * torch.randn(B, 3, generator=ge)), unit(g2 + 0.15 * torch.randn(B, 3, generator=ge))
    f1, f2 = torch.rand(B, generator=ge), torch.rand(B, generator=ge)
    tr, sz = gt_ + 0.3 * torch.randn(B, 3, generator=ge), gs + 0.3 * torch.randn(B, 3, generator=ge)
    if B >= 2:
        step = torch.tensor([0.5, -0.5, 0.5])
        g1[0], g2[0] = torch.tensor([0.5, -0.25, 0.125]), torch.tensor([-0.375, 0.625, 0.25])
        r1[0], r2[0], tr[0], sz[0] = g1[0] + step, g2[0] - step, gt_[0] - step, gs[0] + step
        r1[-1], r2[-1], tr[-1], sz[-1], f1[-1], f2[-1] = g1[-1], g2[-1], gt_[-1], gs[-1], 1.0, 1.0
    s0 = {"all1": [1], "all0": [0], "mixed": [0, 1, 2, -1, 0]}[pattern]
    sym = torch.randint(0, 2, (B, width), generator=ge)
    sym[:, 0] = torch.tensor([s0[i % len(s0)] for i in range(B)])
    return (r1, r2, f1, f2, tr, sz), (g1, g2, gt_, gs), sym


@pytest.mark.parametrize("pattern", ["all1", "all0", "mixed"])
@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 513])
def test_pose_terms(ops, B, kind, width, pattern):
    pred, gt, sym = _pose_case(B, width, pattern)
    dp, dg, dsym = [g(t) for t in pred], [g(t) for t in gt], ops.sym_i32(g(sym))
    out = guarded(lambda: ops.pose_terms_fwd(dp, dg, dsym, kind, 0.5))
    r64, r32 = K.pose_terms(pred, gt, sym, kind, 0.5), K.pose_terms(pred, gt, sym, kind, 0.5, dtype=F32)
    held("pose_terms_fwd", "out[0:8]", out[:8], r64[:8], r32[:8])
    assert out[8].item() == r64[8].item() == int((sym[:, 0] != 1).sum())                          # exactly
    gws = [torch.randn(8, generator=gen(B, kind))] + [torch.eye(8)[k] for k in range(8)]
    for j, gw in enumerate(gws):
        grads = guarded(lambda: ops.pose_terms_bwd(dp, dg, dsym, kind, 0.5, out, g(gw)))
        _, w64, amb = K.pose_terms(pred, gt, sym, kind, 0.5, gw)
        _, w32, _ = K.pose_terms(pred, gt, sym, kind, 0.5, gw, dtype=F32)
        for name, got, a, b, ex in zip(("rot1", "rot2", "f1", "f2", "tran", "size"), grads, w64, w32, amb):
            held("pose_terms_bwd", "d %s gw %s" % (name, "random" if j == 0 else "e%d" % (j - 1)), got, a, b, exclude=ex)
    headroom("pose_terms_fwd", "pose_terms_bwd")


# ---------------------------------------------------------------------------------------------- symmetric reconstruction loss
SYM_ROWS = [[0, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0], [2, 0, 1, 0], [1, -1, 0, 0], [0, 0, 1, 1], [1, 0, 1, 0], [-1, 1, 1, 1]]


def _cloud_case(B, N, cols):
    ge = gen(B, N, cols)
    R, t = rand_rotations(B, 100 + N), 0.1 * torch.randn(B, 3, generator=ge) + torch.tensor([0.0, 0.0, 0.8])
    s = 0.2 + 0.3 * torch.rand(B, 3, generator=ge)
    PC = ((torch.rand(B, N, 3, generator=ge) - 0.5) * s.unsqueeze(1)) @ R.transpose(1, 2) + t.unsqueeze(1)
    re = PC + 0.02 * torch.randn(B, N, 3, generator=ge)
    re[:, ::7] = PC[:, ::7]                                                        # equal to the identity target exactly: gradient 0
    rows = SYM_ROWS if B > 1 else [SYM_ROWS[N % 9]]
    sym = torch.tensor([rows[i % len(rows)] for i in range(B)])[:, :cols]
    return PC.contiguous(), re.contiguous(), R.contiguous(), t, sym


@pytest.mark.parametrize("cols", [1, 4])
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_sym_recon(ops, N, B, cols):
    from tgpose_amd import _lib
    PC, re, R, t, sym = _cloud_case(B, N, cols)
    if B > 1:
        assert set(K.sym_mode(sym, cols).tolist()) == ({0, 1, 2, 3, 4} if cols == 4 else {0, 3, 4})
    d = [g(PC), g(re), g(R), g(t), ops.sym_i32(g(sym))]
    # the workspace: exactly tgp_sym_recon_workspace_floats(B, N) floats (Guard checks the words on both sides of the wrapper's)
    ws = int(_lib.lib().tgp_sym_recon_workspace_floats(B, N))
    assert ws == B * (4 if N >= 1024 else -(-N // 256))
    with Guard() as gd:
        ops.sym_recon_fwd(*d)
    assert sorted(n for _, n in gd.bufs) == [1, ws]
    loss = guarded(lambda: ops.sym_recon_fwd(*d))
    held("sym_recon_fwd", "loss", loss, K.sym_recon(PC, re, R, t, sym).reshape(1), K.sym_recon(PC, re, R, t, sym, dtype=F32).reshape(1))
    gl = torch.tensor([1.75])
    _, w64, amb = K.sym_recon(PC, re, R, t, sym, gloss=gl)
    _, w32, _ = K.sym_recon(PC, re, R, t, sym, gloss=gl, dtype=F32)
    for need_pc, need_re in ((True, True), (True, False), (False, True)):
        dPC, dRe = guarded(lambda: ops.sym_recon_bwd(*d, g(gl), need_pc, need_re))
        assert (dPC is None) == (not need_pc) and (dRe is None) == (not need_re)
        tag = "pc%d re%d" % (need_pc, need_re)
        if need_pc:
            held("sym_recon_bwd", "d PC " + tag, dPC, w64[0], w32[0], exclude=amb[0])
        if need_re:
            held("sym_recon_bwd", "d PC_re " + tag, dRe, w64[1], w32[1], exclude=amb[1])
    ident = (K.sym_mode(sym, cols) == 0).nonzero().flatten()
    if ident.numel():
        assert float(w64[0][ident][:, ::7].abs().max()) == 0.0 and float(w64[1][ident][:, ::7].abs().max()) == 0.0   # held exactly above
    headroom("sym_recon_fwd", "sym_recon_bwd")


# ---------------------------------------------------------------------------------------------------------------- ph_loss
@pytest.mark.parametrize("bad", ["clean", "a_last", "b_last", "both_last", "a_zero_row", "b_zero_row"])
@pytest.mark.parametrize("B,D", [(1, 1), (3, 255), (3, 257), (257, 50), (300, 2500)])
def test_rowl1(ops, B, D, bad):
    ge = gen(B, D)
    b = torch.relu(torch.randn(B, D, generator=ge))
    a = b + 0.3 * torch.randn(B, D, generator=ge)
    w = torch.relu(torch.randn(B, D, generator=ge))
    zero_row = 1 if B > 1 else 0
    if B > 1:
        w[1::4] = 0.0                                                               # rows without weight
        w[2] = 0.0
        w[2, D - 1] = 1e-30                                                         # a row that counts by one tiny element in the last column
    else:
        w[0] = 0.0
        w[0, D - 1] = 0.0 if bad.endswith("zero_row") else 1e-30
    r, c = (B - 1, D - 1) if bad.endswith("last") else (zero_row, D - 1)
    if bad.startswith("a") or bad.startswith("both"):
        a[r, c] = float("inf")
    if bad.startswith("b"):
        b[r, c] = float("nan")
    da_, db_, dw_ = g(a), g(b), g(w)
    out, rows = guarded(lambda: ops.rowl1_fwd(da_, db_, dw_))
    gout = torch.tensor([1.75])
    loss64, live, w64, g64, amb = K.rowl1(a, b, w, gout=gout)
    loss32, _, _, g32, _ = K.rowl1(a, b, w, gout=gout, dtype=F32)
    assert torch.equal(rows[:, 1].cpu().double(), w64) and out[1].item() == live           # out[1]: 1 when the backward is live
    if bad == "clean":
        assert live == 1.0
        held("rowl1_fwd", "loss", out[:1], loss64.reshape(1), loss32.reshape(1))
    elif bad.startswith("b_"):
        assert live == 0.0 and out[0].item() == 0.0 == loss64.item()                       # only b is bad: exactly 0
    else:
        assert live == 0.0 and math.isnan(out[0].item()) and math.isnan(loss64.item())     # a is bad: NaN
    da = guarded(lambda: ops.rowl1_bwd(da_, db_, rows, out, g(gout)))
    if live:
        held("rowl1_bwd", "d a", da, g64, g32, exclude=amb)
        assert float(da.cpu()[w64 == 0].abs().max() if bool((w64 == 0).any()) else 0.0) == 0.0
    else:
        assert float(g64.abs().max()) == 0.0 and bool((da == 0).all())                     # a dead backward: zeros, not NaN
    headroom("rowl1_fwd", "rowl1_bwd")


# ---------------------------------------------------------------------------------------------------------------- feature consistency
@pytest.mark.parametrize("B,C", [(1, 1), (2, 255), (3, 257), (257, 70), (32, 1286)])
def test_feat_consistency(ops, B, C):
    ge = gen(B, C)
    spread = lambda: 10.0 ** (6.0 * torch.rand(B, 1, generator=ge) - 3.0)                   # row norms between 1e-3 and 1e3
    unit = lambda v: v / v.norm(dim=1, keepdim=True)
    base1, base2 = unit(torch.randn(B, C, generator=ge)) * spread(), unit(torch.randn(B, C, generator=ge)) * spread()
    if C == 1:          # d (x / |x|) / dx is identically 0 for a scalar: powers of two keep every evaluation of it exact
        base1, base2 = torch.tensor([[0.5]]), torch.tensor([[-2.0]])
    # all-zero rows in x1, in x2 and in both: side by side where the batch has three rows, else one layout after the other
    layouts = [((0,), (1,), (2,))] if B >= 3 else [((), (), ()), ((0,), (), ()), ((), (B - 1,), ()), ((), (), (0,))]
    for z1, z2, zb in layouts:
        x1, x2 = base1.clone(), base2.clone()
        for r in z1 + zb:
            x1[r] = 0.0
        for r in z2 + zb:
            x2[r] = 0.0
        floored = torch.zeros(B, dtype=torch.bool)
        for r in z1 + z2 + zb:
            floored[r] = True
        tag = "zero x1 %s x2 %s both %s" % (list(z1), list(z2), list(zb))
        d1_, d2_ = g(x1), g(x2)
        loss, rows = guarded(lambda: ops.feat_consistency_fwd(d1_, d2_))
        held("feat_consistency_fwd", "loss " + tag, loss, K.feat_consistency(x1, x2).reshape(1), K.feat_consistency(x1, x2, dtype=F32).reshape(1))
        gl = torch.tensor([1.25])
        _, w64 = K.feat_consistency(x1, x2, gloss=gl)
        _, w32 = K.feat_consistency(x1, x2, gloss=gl, dtype=F32)
        for need1, need2 in ((True, True), (True, False), (False, True)):
            got = guarded(lambda: ops.feat_consistency_bwd(d1_, d2_, rows, g(gl), need1, need2))
            assert (got[0] is None) == (not need1) and (got[1] is None) == (not need2)
            for i in range(2):
                if got[i] is not None:
                    for grp, sel in (("floored rows", floored), ("other rows", ~floored)):
                        held("feat_consistency_bwd", "d x%d %s %d%d" % (i + 1, grp, need1, need2), got[i], w64[i], w32[i], rows=sel)
    headroom("feat_consistency_fwd", "feat_consistency_bwd")


# ---------------------------------------------------------------------------------------------------------------- dcd
def _dcd_case(B, n, m, pattern):
    ge = gen(B, n, m, len(pattern))

    def idx(rows, top):                                                              # `rows` indices in [0, top)
        if pattern == "permutation":                                                # every count 1 wherever rows <= top
            return torch.stack([torch.randperm(max(rows, top), generator=ge)[:rows] % top for _ in range(B)])
        if pattern == "all_equal":                                                  # one count of `rows`
            return torch.stack([torch.full((rows,), int(torch.randint(0, top, (1,), generator=ge))) for _ in range(B)])
        return (top * torch.rand(B, rows, generator=ge) ** 3).long().clamp(0, top - 1)   # skewed

    def dist(rows):
        d = 0.05 * torch.rand(B, rows, generator=ge) ** 2
        d[:, ::5] = 0.0                                                             # exact zeros
        d[:, 3::7] = 50.0 + torch.rand(B, len(range(3, rows, 7)), generator=ge)     # exp(-70 d) is 0 in float32 and in float64
        d[:, 4::11] = 1.3                                                           # exp(-70 d) = 3e-40: below float32's normal range
        return d
    i1, i2 = idx(n, m), idx(m, n)
    assert 0 <= int(i1.min()) and int(i1.max()) < m and 0 <= int(i2.min()) and int(i2.max()) < n
    return dist(n), dist(m), i1.int(), i2.int()


@pytest.mark.parametrize("pattern", ["permutation", "all_equal", "skewed"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n,m", [(1, 1), (1, 5), (5, 1), (255, 257), (1028, 1024), (4096, 1), (4096, 4096)])
def test_dcd(ops, n, m, B, pattern):
    d1, d2, i1, i2 = _dcd_case(B, n, m, pattern)
    if pattern == "permutation" and n == m:
        assert all(int(torch.bincount(i1[b].long(), minlength=m).max()) == 1 for b in range(B))
    dev = [g(d1), g(d2), g(i1), g(i2)]
    gloss = torch.tensor([1.0, -0.5, 2.25])[:B]
    for alpha in (0.1, 70.0):
        for lam in (0.0, 0.3, 1.0):
            ws = {}
            for non_reg in (False, True):
                tag = "alpha %g lambda %g non_reg %d" % (alpha, lam, non_reg)
                loss, w1, w2 = guarded(lambda: ops.dcd_fwd(*dev, alpha, lam, non_reg))
                l64, a64, b64, g64 = K.dcd(d1, d2, i1, i2, alpha, lam, non_reg, gloss=gloss)
                l32, a32, b32, g32 = K.dcd(d1, d2, i1, i2, alpha, lam, non_reg, gloss=gloss, dtype=F32)
                held("dcd_fwd", "loss " + tag, loss, l64, l32)
                held("dcd_fwd", "w1 " + tag, w1, a64, a32)
                held("dcd_fwd", "w2 " + tag, w2, b64, b32)
                bare, n1, n2 = ops.dcd_fwd(*dev, alpha, lam, non_reg, want_weights=False)
                assert n1 is None and n2 is None and torch.equal(bare.view(torch.int32), loss.view(torch.int32))   # the same loss bits
                gd1, gd2 = guarded(lambda: ops.dcd_bwd(dev[0], dev[1], w1, w2, g(gloss), alpha))
                held("dcd_bwd", "d dist1 " + tag, gd1, g64[0], g32[0])
                held("dcd_bwd", "d dist2 " + tag, gd2, g64[1], g32[1])
                ws[non_reg] = (w1, w2)
            # non_reg clamps frac_21 = m / n (in w1) and frac_12 = n / m (in w2) to >= 1: with n != m exactly one of them moves
            moved = [not torch.equal(ws[False][k], ws[True][k]) for k in range(2)]
            assert moved == [m < n, n < m], (moved, n, m)
    headroom("dcd_fwd", "dcd_bwd")


def test_dcd_above_the_lds_histograms_is_refused(ops):
    """n = 4097: the library's TGP_EUNSUPPORTED, raised by the wrapper, and nothing is launched (no output is written)"""
    from tgpose_amd import _lib
    for n, m in ((4097, 8), (8, 4097)):
        d1, d2 = torch.rand(1, n, device=DEV), torch.rand(1, m, device=DEV)
        i1, i2 = torch.zeros(1, n, device=DEV, dtype=torch.int32), torch.zeros(1, m, device=DEV, dtype=torch.int32)
        with Guard() as gd:
            with pytest.raises(_lib.TgpError, match="TGP_EUNSUPPORTED"):
                ops.dcd_fwd(d1, d2, i1, i2, 70.0, 0.3)
        torch.cuda.synchronize()
        assert sorted(k for _, k in gd.bufs) == sorted([1, n, m])
        for buf, _ in gd.bufs:
            assert bool((buf == POISON).all())                                      # loss, w1 and w2 as they were allocated
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        loss = torch.full((1,), POISON, device=DEV)
        rc = _lib.lib().tgp_dcd_fwd(p(d1), p(d2), p(i1), p(i2), 1, n, m, 70.0, 0.3, 0, p(loss), None, None,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == _lib.EUNSUPPORTED and loss.item() == POISON


# ---------------------------------------------------------------------------------------------------------------- pose transform
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 257, 1028])
def test_pose_transform(ops, n, B):
    ge = gen(B, n)
    R = rand_rotations(B, 7 + n).contiguous()
    t = torch.randn(B, 3, generator=ge)
    t = t / t.norm(dim=1, keepdim=True)                                             # |t| = 1
    s = 0.5 + 2.0 * torch.rand(B, 3, generator=ge)                                  # non-unit scales
    pts = 0.3 * torch.randn(B, n, 3, generator=ge) + t.unsqueeze(1)
    dout = torch.randn(B, n, 3, generator=ge)
    dev = [g(pts), g(R), g(t), g(s)]
    out = guarded(lambda: ops.pose_transform(*dev))
    o64, w64 = K.pose_transform(pts, R, t, s, dout)
    o32, w32 = K.pose_transform(pts, R, t, s, dout, dtype=F32)
    held("pose_transform_fwd", "out", out, o64, o32)
    for need_points in (True, False):
        got = guarded(lambda: ops.pose_transform_bwd(*dev, g(dout), need_points=need_points))
        assert (got[0] is None) == (not need_points)
        for name, x, a, b in zip(("d points", "d R", "d t", "d s"), got, w64, w32):
            if x is not None:
                held("pose_transform_bwd", "%s need_points %d" % (name, need_points), x, a, b)
    headroom("pose_transform_fwd", "pose_transform_bwd")


# ------------------------------------------------------------------------------------- pose rotation, canonicalize, generate_RT
def _axes_case(B, ld):
    """axis pairs by row: perpendicular, at 30 / 150 degrees, 1e-3 rad apart (clamp active; the common normal is a difference of nearly
    equal products, so these rows are held to their own conditioning); both the predicted red axis and the ground truth's x axis are
    built that way, so symmetric and non-symmetric objects (interleaved) meet every kind"""
    ge = gen(B, ld)
    unit = lambda v: v / v.norm(dim=1, keepdim=True)
    p_g = unit(torch.randn(B, 3, generator=ge))
    kind = (torch.arange(B) + B) % 3
    ang = torch.where(kind == 0, torch.full((B,), math.pi / 2), torch.where(kind == 1, torch.full((B,), math.pi / 6), torch.full((B,), 1e-3)))
    ang = torch.where((kind == 1) & ((torch.arange(B) // 6) % 2 == 1), torch.full((B,), 5 * math.pi / 6), ang)

    def at_angle():
        u = unit(torch.cross(p_g, torch.randn(B, 3, generator=ge), dim=1))
        return (p_g.double() * torch.cos(ang.double()).unsqueeze(1) + u.double() * torch.sin(ang.double()).unsqueeze(1)).float()
    p_r, gR0 = at_angle(), at_angle()
    f_g, f_r = torch.rand(B, generator=ge) * 0.9 + 0.05, torch.rand(B, generator=ge) * 0.9 + 0.05
    sym = torch.randint(0, 2, (B, ld), generator=ge).float()
    sym[:, 0] = (torch.arange(B) % 2).float()
    gR = torch.randn(B, 3, 3, generator=ge)
    gR[:, :, 0] = gR0
    return gR.contiguous(), p_g, f_g, p_r, f_r, sym, kind == 2


ORTHO = 64 * K.EPS32     # R^T R - I: each entry of R carries a few roundings of two normalisations and two cross products


def _orthonormal(R):
    R = R.cpu().double()
    dev = (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max().item()
    print("orthonormality %.2e of %.2e" % (dev, ORTHO))
    assert dev <= ORTHO


@pytest.mark.parametrize("ld", [1, 4])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_pose_rotation_canonicalize_generate_rt(ops, B, ld):
    gR, p_g, f_g, p_r, f_r, sym, near = _axes_case(B, ld)
    ge = gen(B, ld, 1)
    groups = (("well conditioned", ~near), ("1e-3 apart", near))
    gR0, sym0 = gR[:, :, 0].contiguous(), sym[:, 0].contiguous()
    dev = [g(gR0), g(p_g), g(f_g), g(p_r), g(f_r), g(sym0)]
    R, J = guarded(lambda: ops.pose_rotation_fwd(*dev))
    dR = torch.randn(B, 3, 3, generator=ge)
    R64, d64 = K.pose_rotation(gR0, p_g, f_g, p_r, f_r, sym0, dR=dR)
    R32, d32 = K.pose_rotation(gR0, p_g, f_g, p_r, f_r, sym0, dR=dR, dtype=F32)
    din = guarded(lambda: ops.pose_rotation_bwd(g(dR), J))
    for tag, sel in groups:
        held("pose_rotation_fwd", "R " + tag, R, R64, R32, rows=sel)
        held("pose_rotation_bwd", "d in " + tag, din, d64, d32, rows=sel)
    _orthonormal(R)
    symmetric = sym0 == 1
    if bool(symmetric.any()):
        assert float(din.cpu()[symmetric][:, 4:].abs().max()) == 0.0                # nothing flows to the red axis of a symmetric object
    # canonicalize: the same rotation, then (R^T (p - t)) * s over a cloud of more than one block with a tail
    n = 257
    pts = 0.3 * torch.randn(B, n, 3, generator=ge) + torch.tensor([0.0, 0.0, 0.8])
    p_t, p_s = 0.1 * torch.randn(B, 3, generator=ge) + torch.tensor([0.0, 0.0, 0.8]), 0.5 + 2.0 * torch.rand(B, 3, generator=ge)
    canon, Rc = guarded(lambda: ops.canonicalize(g(pts), g(gR), g(p_g), g(f_g), g(p_r), g(f_r), g(p_t), g(p_s), g(sym)))
    c64, Rc64 = K.canonicalize(pts, gR, p_g, f_g, p_r, f_r, p_t, p_s, sym)
    c32, Rc32 = K.canonicalize(pts, gR, p_g, f_g, p_r, f_r, p_t, p_s, sym, dtype=F32)
    assert torch.equal(Rc64, R64)
    for tag, sel in groups:
        held("canonicalize", "R " + tag, Rc, Rc64, Rc32, rows=sel)
        held("canonicalize", "points " + tag, canon, c64, c32, rows=sel)
        if int(sel.sum()):                                                          # the two kernels' rotations agree to rounding
            assert float((Rc.cpu().double() - R.cpu().double())[sel].abs().max()) <= 2 * K.bound(R64[sel], R32[sel])
    _orthonormal(Rc)
    # generate_RT: the red confidence zeroed for symmetric objects (sym given) or used as it is (sym=None)
    T = torch.randn(B, 3, generator=ge)
    for label, s_ in (("sym", sym), ("sym=None", None)):
        rt = guarded(lambda: ops.generate_rt(g(p_g), g(p_r), g(f_g), g(f_r), g(T), g(s_)))
        rt64, rt32 = K.generate_rt(p_g, p_r, f_g, f_r, T, s_), K.generate_rt(p_g, p_r, f_g, f_r, T, s_, dtype=F32)
        for tag, sel in groups:
            held("generate_rt", "R %s %s" % (label, tag), rt[:, :3, :3], rt64[:, :3, :3], rt32[:, :3, :3], rows=sel)
        assert torch.equal(rt[:, :3, 3].cpu(), T) and torch.equal(rt[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 4))
        _orthonormal(rt[:, :3, :3])
    headroom("pose_rotation_fwd", "pose_rotation_bwd", "canonicalize", "generate_rt")


# ---------------------------------------------------------------------------------------------------------------- head_post
@pytest.mark.parametrize("stride", [4, 8])
@pytest.mark.parametrize("B", [1, 65])
def test_head_post_bwd(ops, B, stride):
    """a zero axis: torch's norm backward contributes 0 at the origin, so that row's gradient is what the division alone gives,
    g / (0 + 1e-6) -- held as its own group, the other rows to their own bound"""
    ge = gen(B, stride)
    green, red, ts, mean = (torch.randn(B, 4, generator=ge), torch.randn(B, 4, generator=ge), torch.randn(B, 6, generator=ge),
                            torch.randn(B, 3, generator=ge))
    green[7 % B, 1:] = 0.0
    zg, zr = torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)
    zg[7 % B] = True
    if B > 1:
        red[B - 1, 1:] = 0.0
        zr[B - 1] = True

    def strided(t, width):                                                          # rows of a wider buffer whose other columns are NaN
        buf = torch.full((B, width), float("nan"), device=DEV)
        buf[:, :t.shape[1]] = g(t)
        return buf[:, :t.shape[1]]
    dgreen, dred, dts = strided(green, stride), strided(red, stride), strided(ts, 8 if stride == 8 else 6)
    outs = guarded(lambda: ops.head_post(dgreen, dred, dts, g(mean)))
    o64, o32 = K.head_post(green, red, ts, mean), K.head_post(green, red, ts, mean, dtype=F32)
    for name, x, a, b in zip(("p_green", "p_red", "f_green", "f_red", "T", "s"), outs, o64, o32):
        held("head_post", name, x, a, b)
    full = [torch.randn(B, 3, generator=ge), torch.randn(B, 3, generator=ge), torch.randn(B, generator=ge), torch.randn(B, generator=ge),
            torch.randn(B, 3, generator=ge), torch.randn(B, 3, generator=ge)]
    for missing in [None] + list(range(6)):
        grads = [None if i == missing else t for i, t in enumerate(full)]
        got = guarded(lambda: ops.head_post_bwd(dgreen, dred, [g(t) for t in grads]))
        _, w64 = K.head_post(green, red, ts, mean, grads)
        _, w32 = K.head_post(green, red, ts, mean, grads, dtype=F32)
        tag = "all six" if missing is None else "without %d" % missing
        for name, x, a, b, zero in zip(("d green", "d red", "d ts"), got, w64, w32, (zg, zr, None)):
            if zero is None:
                held("head_post_bwd", "%s %s" % (name, tag), x, a, b)
            else:
                held("head_post_bwd", "%s %s, zero axis" % (name, tag), x, a, b, rows=zero)
                held("head_post_bwd", "%s %s, other rows" % (name, tag), x, a, b, rows=~zero)
    headroom("head_post", "head_post_bwd")
