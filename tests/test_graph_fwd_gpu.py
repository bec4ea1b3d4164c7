"""The encoder's forward graph kernels (csrc/gconv.hip) on an MI355X against the fp64 reference of tests/graph_fwd_ref.py, on both
sides of every shape at which a launch switches its kernel form, and on graphs built so that a mishandled slot or row shows.

Forms and their boundaries (graph_fwd_ref.gconv_form / orl_form; tests/test_graph_fwd_cpu.py recomputes them from the byte formulas):

    tgp_gconv_hs_fwd     n <= 164 LDS table of 16-channel slices | 165..329 of 8-channel slices | n >= 330 wave-per-point gather;
                         the launch opts in to more than 64 KiB of LDS from n = 147 (16) and n = 293 (8)
    ORL pooling          LDS table up to n = 1084 (1081 with planes and for the one-launch form), beyond it orl_partial_kernel;
                         inside the LDS form the lists go to LDS as 16-bit ids when (n k) % 4 == 0, the list is 16-byte aligned
                         and all fits 150 KiB (k = 64: up to n = 782), else they are read from memory; 256 threads up to n = 704,
                         512 from 705

Observable from outside, and asserted here per case: tgp_gconv_hs_fwd_dirs answers TGP_EUNSUPPORTED exactly where gconv_form is 0;
ops.orl_rowbias(planes=P) returns P exactly where orl_form(planes=True) is the LDS form; tgp_orl_rowbias_fused answers
TGP_EUNSUPPORTED exactly where that form (or n >= 2) does not hold.  The other switches are run on both sides and judged by the
results alone.

Graph families: slot_wins (k different neighbours, operands shaped so that every slot is the decisive winner of its share of the
entries: a kernel that drops or misreads one slot fails, tests/test_graph_fwd_cpu.py shows it on the reference), base (self at slot
0: a zero direction), repeats, coincident, no_self (graph_bwd_ref) and ends (only ids 0 and n - 1: the table's first and last row).

The bars are derived, not measured (graph_fwd_ref's docstring): (12 + 7) 2^-24 abs_terms for the graph convolutions with abs_terms
taken over the largest candidate per support, so NO element is excluded; (2 + chain) 2^-24 abs_terms for ORL with chain from the
kernels' fixed summation order.  Pool, gathers, planes and every "same result by another route" comparison are bit for bit.

Largest |error| / bar measured on the MI355X, per kernel form (every case prints its own):

    gconv_hs       lds16 0.12, lds16 + opt-in 0.14, lds8 0.16, lds8 + opt-in 0.17, gather 0.15       (52 cases)
    gconv_surface  C = 128 0.16, C = 256 0.17, C = 512 0.17                                           (48 cases)
    ORL g          LDS, lists in LDS, 256 / 512 threads 0.24 / 0.20; lists from memory 0.10 / 0.22; L2 gather 0.20;
                   the one-launch form the same figures (its g is the two-launch form's bit for bit)
    ORL rb         two launches 0.010, with planes 0.010, one launch 0.011 (its own summation order)   (32 cases)
    normalize_dirs 0.39 of the absolute bar, 0.59 of the bar taken relative to each component
"""
import ctypes
import functools

import pytest
import torch

from tests import graph_fwd_ref as F
from tests import test_graph_bwd_gpu as BW
from tests.graph_fwd_ref import case, case_id

pytestmark = pytest.mark.gpu

DEV = BW.DEV
g, FILL = BW.g, BW.FILL
EUNSUPPORTED = -2
SW = "slot_wins"

# ----------------------------------------------------------------------------------------------------------------------- the cases
# HS_layer.graph_conv: (family, B, n, k, C).  Both sides of 146|147 (opt-in, 16), 164|165 (16 -> 8), 292|293 (opt-in, 8), 329|330
# (8 -> gather) at C = 128, B = 1 and 3 in every form; every family in every form; the form switches again at C = 256 and 512; the
# neighbour counts at n = 165 (LDS) and n = 330 (gather: odd k leaves the second half-wave a spare slot at C = 128); views.
HS_FAMILIES = ("base", "repeats", "coincident", "no_self", "ends")
HS_CASES = ([case(SW, 3, 146, 8, 128), case(SW, 1, 147, 8, 128), case(SW, 3, 164, 20, 128), case(SW, 1, 165, 20, 128),
             case(SW, 3, 292, 8, 128), case(SW, 1, 293, 8, 128), case(SW, 3, 329, 20, 128), case(SW, 1, 330, 20, 128),
             case(SW, 1, 164, 7, 128), case(SW, 3, 165, 7, 128), case(SW, 1, 329, 7, 128), case(SW, 3, 330, 7, 128)]
            + [case(f, 1 + 2 * (i % 2), n, 6, 128) for n in (164, 165, 330) for i, f in enumerate(HS_FAMILIES)]
            + [case(SW, 1 + (n % 2), n, 8, C) for C in (256, 512) for n in (164, 165, 329, 330)]
            + [case(SW, 1, n, k, 128) for n in (165, 330) for k in (1, 2, 7, 63, 64)]
            + [case(SW, 3, 330, 5, 256), case("repeats", 2, 330, 7, 512), case("ends", 1, 165, 63, 256)]
            + [case(SW, 3, 164, 8, 128, view=True), case(SW, 1, 165, 8, 256, view=True), case(SW, 3, 330, 7, 128, view=True),
               case("base", 1, 330, 8, 512, view=True)])

# HSlayer_surface.graph_conv: n in {1, 15, 16, 17, 330} x C in {128, 256, 512} x k in {1, 7, 64}; view = the xyz_pad form
SURFACE_CASES = ([case("base", 1 + 2 * ((n + k) % 2), n, k, C, view=(k == 7)) for n in (1, 15, 16, 17) for C in (128, 256, 512)
                  for k in (1, 7, 64)]
                 + [case("base", 1, 330, k, C, view=(k == 1)) for C in (128, 256, 512) for k in (1, 7, 64)]
                 + [case("ends", 3, 330, 7, 128), case("coincident", 3, 330, 7, 256), case("repeats", 1, 17, 7, 512)])

# ORL pooling: (family, B, n, k, C); view = the list's storage starts 4 bytes past a 16-byte boundary
ORL_EDGES = (2, 63, 64, 65, 704, 705, 1081, 1082, 1084, 1085)
ORL_CASES = ([case(SW if n > 20 else "base", 3, n, 20, 128) for n in ORL_EDGES]
             + [case(SW, 2, n, 20, 512) for n in (1081, 1082, 1084, 1085)]
             + [case(SW, 3, 257, 7, 128), case(SW, 2, 1028, 7, 128), case(SW, 1, 782, 64, 128), case(SW, 1, 783, 64, 128),
                case(SW, 3, 300, 20, 128, view=True), case("repeats", 2, 1084, 20, 256, view=True)]
             + [case("repeats", 3, n, 20, 128) for n in (2, 65, 705, 1085)]
             + [case("ends", 3, n, 20, 128) for n in (64, 704, 1081, 1082, 1085)] + [case("ends", 1, 783, 64, 256)]
             + [case("base", 3, 1, 20, 128), case("base", 2, 1, 1, 512)])

POOL_WIDTHS = (4, 16, 64, 256, 512)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    from tgpose_amd import ops as _ops, _lib
    _lib.lib()  # raises if libtgpose_hip.so is missing: there is no fallback
    return _ops


@functools.lru_cache(maxsize=None)
def hs_reference(c, surface=False):
    """the operands of a case and their fp64 forward: built once, shared, never written to"""
    inp = F.hs_inputs(c, surface)
    return inp, F.hs_terms(inp["xyz"], inp["idx"], inp["proj"], inp["sdn"], c.C, surface)


@functools.lru_cache(maxsize=None)
def orl_reference(c):
    inp = F.orl_inputs(c)
    return inp, F.orl_terms(inp["feat"], inp["idx"], inp["w2t"])


def hs_form_name(c):
    ch = F.gconv_form(c.n, c.C)
    return "gather" if not ch else "lds%d%s" % (ch, "+optin" if F.gconv_opt_in(c.n, c.C) else "")


def orl_form_name(c, planes=False):
    form, lists, threads = F.orl_form(c.n, c.k, c.C, planes, aligned=not c.view)
    return form if form == "gather" else "lds/%s/%d" % ("lists-in-lds" if lists else "lists-from-memory", threads)


class _Report(object):
    """collects every comparison of a case, prints each figure, asserts once"""

    def __init__(self, tag, mismatch):
        self.tag, self.mismatch, self.failed = tag, mismatch, []

    def check(self, name, got, term):
        assert got.numel() == term.value.numel(), name
        bad, worst = self.mismatch(got, term)
        print("%s  %-30s max |err| / bar %.3f   outside %d of %d" % (self.tag, name, worst, int(bad.sum()), bad.numel()))
        if bool(bad.any()):
            self.failed.append((name, worst, int(bad.sum())))

    def done(self):
        assert not self.failed, (self.tag, self.failed)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _planes_match(P, table, rows):
    """the planes' bytes of the first `rows` rows and every magnitude word equal the stand-alone split of `table` (rows, K); what
    lies in the last row block past `rows` is nobody's"""
    from tests.test_gpu_parity import _ref_planes
    want, amax = _ref_planes(table, P.K)
    nblk = want.shape[0]
    rows_ok = (torch.arange(nblk * 32, device=DEV) < rows).view(nblk, 1, 1, 1, 32, 1)
    same = (P.buf.view(nblk, P.kt, 2, 2, 32, 16) == want.view(nblk, P.kt, 2, 2, 32, 16)) | ~rows_ok
    return bool(same.all()) and torch.equal(P.amax, amax)


# ------------------------------------------------------------------------------------------------------------ HS graph convolution
@pytest.mark.parametrize("c", HS_CASES, ids=case_id)
def test_gconv_hs_vs_fp64(ops, c):
    """ops.gconv_hs against hs_terms at every element; the same bits on a second call, from gconv_hs_slots (k <= 63) and from the
    dirs entry wherever the LDS kernel serves the shape; tgp_gconv_hs_fwd_dirs' return code says which side of 329 | 330 the launch
    took, and a refusal leaves the output alone.  View cases: proj and out are column slices (ldp > 9 C, ldo > C) of buffers whose
    other columns come back untouched."""
    from tgpose_amd import _lib
    inp, want = hs_reference(c)
    x, idx, sdn = g(inp["xyz"]), g(inp["idx"]), g(inp["sdn"])
    if c.view:
        proj, proj_buf = BW._slice(inp["proj"], 8, c.C + 12)                 # ldp = 9 C + 20
        out, out_buf = BW._slice(torch.zeros(c.B, c.n, c.C), 4, 8)
        fresh = lambda: BW._slice(torch.zeros(c.B, c.n, c.C), 4, 8)[0]
    else:
        proj, out = g(inp["proj"]), None
        fresh = lambda: None
    rep = _Report("hs %s %s" % (hs_form_name(c), case_id(c)), F.R.mismatch)
    got = ops.gconv_hs(x, idx, proj, sdn, 7, c.C, out=out)
    rep.check("out (gconv_hs)", got, want)
    assert torch.equal(ops.gconv_hs(x, idx, proj, sdn, 7, c.C, out=fresh()), got)
    if c.k <= 63:
        assert torch.equal(ops.gconv_hs_slots(x, idx, proj, sdn, 7, c.C)[0], got), "gconv_hs_slots' output differs"

    dirs = torch.zeros(c.B, c.n, c.k, 4, device=DEV)
    dirs[..., :3] = ops.neighbor_dirs(x, idx)
    lds = F.gconv_form(c.n, c.C) != 0
    direct = torch.full((c.B, c.n, c.C), FILL, device=DEV)
    ldp = proj.stride(1)
    rc = _lib.lib().tgp_gconv_hs_fwd_dirs(_p(x), _p(idx), _p(proj), ldp, _p(sdn), c.B, c.n, c.k, 7, c.C, _p(direct), c.C, _p(dirs), _stream())
    torch.cuda.synchronize()
    assert rc == (0 if lds else EUNSUPPORTED), (rc, hs_form_name(c))
    assert torch.equal(direct, got) if lds else bool((direct == FILL).all())
    assert torch.equal(ops.gconv_hs(x, idx, proj, sdn, 7, c.C, dirs=dirs), got)
    if c.view:
        BW._outside_unchanged(proj_buf, 8, 8 * c.C, inp["proj"])
        BW._outside_unchanged(out_buf, 4, c.C)
    rep.done()


# ------------------------------------------------------------------------------------------------------- surface graph convolution
@pytest.mark.parametrize("c", SURFACE_CASES, ids=case_id)
def test_gconv_surface_vs_fp64(ops, c):
    """ops.gconv_surface against hs_terms(surface=True) at every element, tiles of 16 points with 1, 15, 16 and 17 of them and 21
    tiles, k = 1 (both half-waves repeat slot 0 at C = 128), 7 and 64.  View cases: out is a (B, n, C) slice of rows C + 12 wide and
    xyz_pad leaves (x, y, z, 0) bit for bit in columns C .. C + 3, the sentinel in the eight behind them."""
    inp, want = hs_reference(c, True)
    x, idx, sdn = g(inp["xyz"]), g(inp["idx"]), g(inp["sdn"])
    rep = _Report("surface %s" % case_id(c), F.R.mismatch)
    got = ops.gconv_surface(x, idx, sdn, 7, c.C)
    rep.check("out (gconv_surface)", got, want)
    assert torch.equal(ops.gconv_surface(x, idx, sdn, 7, c.C), got)
    if c.view:
        buf = torch.full((c.B, c.n, c.C + 12), FILL, device=DEV)
        padded = ops.gconv_surface(x, idx, sdn, 7, c.C, out=buf[..., :c.C], xyz_pad=True)
        torch.cuda.synchronize()
        assert torch.equal(padded, got)
        xyz0 = torch.cat([x, torch.zeros(c.B, c.n, 1, device=DEV)], 2)
        assert torch.equal(buf[..., c.C:c.C + 4].contiguous().view(torch.int32), xyz0.view(torch.int32))
        assert bool((buf[..., c.C + 4:] == FILL).all())
    rep.done()


# ------------------------------------------------------------------------------------------------------------------------------ ORL
def _fused_direct(lib, c, feat, idx, w2t, planes, xyz_tile):
    """tgp_orl_rowbias_fused itself -> (return code, rb, g, tickets)"""
    rb = torch.full((c.B, c.C), FILL, device=DEV)
    g_out = torch.full((c.B, c.C), FILL, device=DEV)
    contrib = torch.empty(c.B * (c.C // 16) * c.C, device=DEV)
    tickets = torch.zeros(c.B, device=DEV, dtype=torch.int32)
    rc = lib.tgp_orl_rowbias_fused(_p(feat), feat.stride(1), _p(idx), c.B, c.n, c.k, c.C, _p(w2t), _p(g_out), _p(rb),
                                   _p(planes.buf) if planes is not None else None, planes.kt if planes is not None else 0,
                                   _p(planes.amax) if planes is not None else None, _p(xyz_tile), _p(contrib), _p(tickets), _stream())
    torch.cuda.synchronize()
    return rc, rb, g_out, tickets


@pytest.mark.parametrize("c", ORL_CASES, ids=case_id)
def test_orl_vs_fp64(ops, c):
    """ops.orl_global and ops.orl_rowbias (plain, with planes [and the xyz K-tile at odd n], with tickets) against orl_terms, every
    entry point twice with the same bits.  planes=P comes back as P exactly where orl_form says the planes budget fits (n <= 1081):
    then its bytes and magnitude words equal the stand-alone split of the table, else nothing was written.  The one-launch entry
    point answers TGP_EUNSUPPORTED exactly where that budget (or n >= 2) fails; a tickets= call lands within the bar either way with
    the tickets back at zero, and agrees with the two-launch form within the rb bar."""
    from tgpose_amd import _lib
    inp, (want_g, want_rb) = orl_reference(c)
    feat, w2t = g(inp["feat"]), g(inp["w2t"])
    if c.view:                                                              # the list 4 bytes past a 16-byte boundary
        flat = torch.zeros(c.B * c.n * c.k + 8, device=DEV, dtype=torch.int32)
        idx = flat[1:1 + c.B * c.n * c.k].view(c.B, c.n, c.k)
        idx.copy_(inp["idx"])
        assert idx.data_ptr() % 16 == 4 and idx.is_contiguous()
    else:
        idx = g(inp["idx"])
        assert idx.data_ptr() % 16 == 0
    xyz = g(torch.randn(c.B, c.n, 3, generator=torch.Generator().manual_seed(c.n))) if c.n % 2 else None
    rep = _Report("orl %s %s" % (orl_form_name(c), case_id(c)), F.orl_mismatch)

    got_g = ops.orl_global(feat, idx)
    rep.check("g (orl_global)", got_g, want_g)
    assert torch.equal(ops.orl_global(feat, idx), got_g)
    rb = ops.orl_rowbias(feat, idx, w2t)
    rep.check("rb (orl_rowbias)", rb, want_rb)
    assert torch.equal(ops.orl_rowbias(feat, idx, w2t), rb)

    fits = F.orl_form(c.n, c.k, c.C, planes=True, aligned=not c.view)[0] == "lds"
    K = c.C + 4 if xyz is not None else c.C
    table = feat.view(c.B * c.n, c.C)
    if xyz is not None:
        table = torch.cat([table, xyz.view(-1, 3), torch.zeros(c.B * c.n, 1, device=DEV)], 1)

    def new_planes():
        P = ops.Planes(c.B * c.n, K, DEV)
        P.buf.fill_(0xAB)
        return P

    P = new_planes()
    rb_p, back = ops.orl_rowbias(feat, idx, w2t, planes=P, xyz_tile=xyz)
    assert (back is P) == fits, (orl_form_name(c, True), back is P)
    rep.check("rb (planes%s)" % ("" if fits else " refused"), rb_p, want_rb)
    assert torch.equal(rb_p, rb)
    if fits:
        assert _planes_match(P, table, c.B * c.n)
        P2 = new_planes()
        ops.orl_rowbias(feat, idx, w2t, planes=P2, xyz_tile=xyz)
        assert torch.equal(P2.buf, P.buf) and torch.equal(P2.amax, P.amax)
    else:
        assert bool((P.buf == 0xAB).all()) and bool((P.amax == 0).all())

    # the one-launch form: the entry point itself, then through ops (which falls back where it is refused)
    P = new_planes()
    rc, rb_f, g_f, tickets = _fused_direct(_lib.lib(), c, feat, idx, w2t, P, xyz)
    assert rc == (0 if fits and c.n >= 2 else EUNSUPPORTED), (rc, orl_form_name(c, True))
    if rc == 0:
        rep.check("rb (one launch)", rb_f, want_rb)
        rep.check("g (one launch)", g_f, want_g)
        assert torch.equal(g_f, got_g), "the fused finish adds the tile sums as orl_finish_kernel does, term by term"
        assert int(tickets.abs().sum()) == 0
        assert _planes_match(P, table, c.B * c.n)
        assert bool(((rb_f.double() - rb.double()).abs().cpu() <= F.orl_bound(want_rb)).all()), "one launch against two"
        again = _fused_direct(_lib.lib(), c, feat, idx, w2t, None, None)
        assert again[0] == 0 and torch.equal(again[1], rb_f) and torch.equal(again[2], g_f)
    else:
        assert bool((rb_f == FILL).all()) and bool((P.buf == 0xAB).all()) and int(tickets.abs().sum()) == 0
    tickets = torch.zeros(c.B, device=DEV, dtype=torch.int32)
    rb_t = ops.orl_rowbias(feat, idx, w2t, tickets=tickets)
    rep.check("rb (tickets=%s)" % ("one launch" if rc == 0 else "fallback"), rb_t, want_rb)
    assert int(tickets.abs().sum()) == 0
    assert torch.equal(rb_t, rb_f if rc == 0 else rb)
    rep.done()


# ----------------------------------------------------------------------------------------------------------------- pool and gathers
@pytest.mark.parametrize("family", [SW, "repeats"])
@pytest.mark.parametrize("C", POOL_WIDTHS)
def test_pool_bit_equal(ops, C, family):
    """ops.pool, with and without planes, bit for bit pool_ref: n_out = 1, 77 (B n_out C / 4 no multiple of 256 at any width; with
    B = 3 the objects' rows straddle the planes' 32-row blocks) and n, kpool = 1 and k, a sample with repeats in no order, feat and
    out_f as slices of wider buffers.  C = 4 has no planes; C = 512 is refused by the planes kernel and the wrapper's split of the
    result must give the same planes."""
    B, n, k = 3, 100, 8
    c = case(family, B, n, k, C)
    inp = F.orl_inputs(c)
    gen = torch.Generator().manual_seed(C + n)
    xyz = torch.randn(B, n, 3, generator=gen)
    feat, feat_buf = BW._slice(inp["feat"], 4, 8)
    idx = g(inp["idx"])
    for n_out in (1, 77, n):
        assert n_out == 1 or n_out == n or (B * n_out * C // 4) % 256
        sample = torch.randint(0, n, (n_out,), generator=gen, dtype=torch.int32)
        if n_out == n:
            sample[1] = sample[0]
        for kpool in (1, k):
            want_xyz, want_f = F.pool_ref(xyz, inp["feat"], inp["idx"], sample, kpool)
            out_f, out_buf = BW._slice(torch.zeros(B, n_out, C), 8, 4)
            got_xyz, got_f = ops.pool(g(xyz), feat, idx, g(sample), kpool=kpool, out_f=out_f)
            torch.cuda.synchronize()
            assert torch.equal(got_xyz.cpu(), want_xyz) and torch.equal(got_f.cpu(), want_f), (n_out, kpool)
            BW._outside_unchanged(out_buf, 8, C)
            if C >= 16:
                P = ops.Planes(B * n_out, C, DEV)
                P.buf.fill_(0xAB)
                out_f, out_buf = BW._slice(torch.zeros(B, n_out, C), 8, 4)
                got_xyz, got_f = ops.pool(g(xyz), feat, idx, g(sample), kpool=kpool, out_f=out_f, planes=P)
                torch.cuda.synchronize()
                assert torch.equal(got_xyz.cpu(), want_xyz) and torch.equal(got_f.cpu(), want_f), (n_out, kpool, "planes")
                assert _planes_match(P, g(want_f).view(B * n_out, C), B * n_out), (n_out, kpool)
                BW._outside_unchanged(out_buf, 8, C)
    BW._outside_unchanged(feat_buf, 4, C, inp["feat"])


@pytest.mark.parametrize("C", POOL_WIDTHS)
def test_gather_rows_bit_equal(ops, C):
    """ops.gather_rows bit for bit gather_ref: n_out = 1, 77 and 4 n, ids with repeats and both ends of the table, src and dst as
    slices of wider buffers whose other columns keep their sentinel"""
    B, n = 3, 100
    gen = torch.Generator().manual_seed(C)
    src0 = torch.randn(B, n, C, generator=gen)
    src, src_buf = BW._slice(src0, 8, 4)
    for n_out in (1, 77, 4 * n):
        idx = torch.randint(0, n, (B, n_out), generator=gen, dtype=torch.int32)
        idx[:, 0] = n - 1
        idx[:, -1] = 0 if n_out > 1 else n - 1
        dst, dst_buf = BW._slice(torch.zeros(B, n_out, C), 4, 12)
        ops.gather_rows(src, g(idx), dst)
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), F.gather_ref(src0, idx)), n_out
        BW._outside_unchanged(dst_buf, 4, C)
    BW._outside_unchanged(src_buf, 8, C, src0)


# ------------------------------------------------------------------------------------------------------------------ normalize_dirs
def test_normalize_dirs_vs_fp64(ops):
    """ops.normalize_dirs against F.normalize(dim=0, eps=1e-12) in fp64: every component within 4 * 2^-24, on columns that are zero,
    of length 1e-20 and 1e-7 (the eps clamp: 1e-20 / 1e-12), 1 and 1e6, among ordinary ones; SC = 901, no multiple of the 256-thread
    workgroup.  A zero column stays exactly zero."""
    SC = 901
    gen = torch.Generator().manual_seed(SC)
    d = torch.randn(3, SC, generator=gen)
    unit = torch.nn.functional.normalize(torch.randn(3, 10, generator=gen), dim=0)
    for j, length in enumerate((0.0, 1e-20, 1e-7, 1.0, 1e6)):
        d[:, j] = unit[:, j] * length
        d[:, SC - 1 - j] = unit[:, 5 + j] * length                          # and in the last, partly filled workgroup
    got = ops.normalize_dirs(g(d)).cpu().double()
    want = F.normalize_dirs_ref(d)
    err = (got - want).abs()
    print("normalize_dirs  max |err| / bar %.3f   (relative to the component: %.3f of 4 * 2^-24)"
          % (float(err.max() / F.NORMALIZE_BAR), float((err / want.abs().clamp_min(1e-30)).max() / F.NORMALIZE_BAR)))
    assert bool((err <= F.NORMALIZE_BAR).all())
    # the same four roundings are relative to the component itself (3.5: the squares and their sum, halved by the root, the root,
    # the division), the clamped columns included: x / 1e-12 is one division
    assert bool((err <= F.NORMALIZE_BAR * want.abs() + 1e-30).all())
    assert bool((got[:, 0] == 0).all()) and bool((got[:, SC - 1] == 0).all())
    assert torch.equal(ops.normalize_dirs(g(d)).cpu().double(), got)
