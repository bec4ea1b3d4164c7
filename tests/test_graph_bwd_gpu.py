"""The graph layers' backward kernels on an MI355X against the fp64 reference of tests/graph_bwd_ref.py, on graphs built to reach
what random kNN-like lists do not: reverse lists that end at, one past and two slabs past the 224-entry LDS slab of
gconv_bwd_gather_kernel (hubs), sources nobody lists, sources listed twice or three times in one row, coincident points, and the
edges of the 16-point tiles (n = 1, 15, 16, 17, 33; k = 1, 2, 63, 64; several objects with a ragged last tile).

Kernels: tgp_gconv_hs_bwd_gather (slots recomputed and taken from tgp_gconv_hs_fwd_slots), tgp_gconv_hs_bwd (atomic scatter),
tgp_gconv_hs_fwd_slots / tgp_gconv_hs_fwd, tgp_gconv_surface_bwd / tgp_gconv_surface_fwd, tgp_gconv_dirgrad, tgp_dirs_to_xyz (over
tgp_reverse_graph's lists and over tgp_child_lists'), tgp_nbrmax_bwd_gather and tgp_nbrmax_bwd.

The bar is derived, not measured (graph_bwd_ref's docstring): per element |got - want| <= (12 + chain) * 2^-24 * abs_terms + 1e-30,
with abs_terms and chain from the reference, chain capped for d sdn by the longest addition path through the kernels' partials
(graph_bwd_ref.dsdn_path) and 7 for the forward output.  d g is zeroed where fp32 and fp64 may legitimately pick different winners
(graph_bwd_ref.ambiguous; at most 1 % of the entries, asserted on the CPU in tests/test_graph_bwd_cpu.py).  A dropped or misdirected
list entry moves an element by a whole term, at least abs_terms / chain: on the 449-entry hub 2e-3 of abs_terms against a bar of
3e-5.  The two test_*_wrong_reverse_list_is_caught tests show it on a valid but wrong list.
"""
import ctypes

import pytest
import torch

from tests import graph_bwd_ref as R
from tests.graph_bwd_ref import case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_HUB = 460

# HS_layer.graph_conv: (family, B, n, k, C)
HS_CASES = [case("hub", 1, N_HUB, 4, 128, L=223), case("hub", 1, N_HUB, 4, 128, L=224), case("hub", 3, N_HUB, 4, 128, L=225),
            case("hub", 1, N_HUB, 4, 128, L=448), case("hub", 2, N_HUB, 4, 128, L=449),
            case("hub", 1, N_HUB, 4, 256, L=225), case("hub", 1, N_HUB, 4, 512, L=225),
            case("everyone_lists_2", 1, 300, 20, 128),
            case("no_self", 2, 72, 8, 128), case("no_self", 3, 40, 5, 256),
            case("repeats", 2, 50, 6, 128), case("repeats", 1, 33, 20, 256),
            case("coincident", 2, 40, 8, 128),
            case("base", 1, 1, 1, 128), case("base", 3, 1, 2, 256), case("base", 3, 15, 2, 128), case("base", 1, 16, 20, 256),
            case("base", 3, 17, 20, 128), case("base", 3, 33, 63, 128), case("base", 1, 33, 1, 512), case("base", 1, 17, 63, 512),
            case("base", 2, 33, 64, 128), case("base", 2, 72, 20, 128),
            case("base", 2, 33, 20, 128, view=True), case("base", 3, 17, 8, 256, view=True)]

# HSlayer_surface.graph_conv
SURFACE_CASES = [case("hub", 1, N_HUB, 4, 128, L=449), case("base", 3, 33, 20, 128), case("base", 1, 17, 63, 256),
                 case("base", 1, 1, 1, 128), case("base", 2, 33, 64, 128), case("repeats", 2, 50, 6, 512),
                 case("coincident", 2, 40, 8, 128), case("base", 3, 17, 20, 256, view=True)]

# y = max_j src[idx]: (family, B, n, k, C), each with per_object both ways
NBRMAX_CASES = [case("hub", 2, N_HUB, 4, 128, L=449), case("no_self", 3, 72, 8, 256), case("base", 3, 33, 1, 128),
                case("base", 2, 33, 64, 512)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    from tgpose_amd import ops as _ops, _lib
    _lib.lib()  # raises if libtgpose_hip.so is missing: there is no fallback
    return _ops


def g(t):
    return torch.as_tensor(t).to(DEV)


FILL = 7.0


def _slice(t, lead, trail):
    """t on the device as a column slice of a wider buffer (row stride a multiple of 4 floats, the slice 16-byte aligned), the
    other columns holding FILL -> (view, buffer)"""
    assert lead % 4 == 0 and (lead + t.shape[-1] + trail) % 4 == 0
    buf = torch.full(t.shape[:-1] + (lead + t.shape[-1] + trail,), FILL, device=DEV)
    view = buf[..., lead:lead + t.shape[-1]]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view, buf


def _outside_unchanged(buf, lead, width, inside=None):
    assert bool((buf[..., :lead] == FILL).all()) and bool((buf[..., lead + width:] == FILL).all())
    if inside is not None:
        assert torch.equal(buf[..., lead:lead + width].cpu(), inside)


class _Report(object):
    """collects every comparison of a case, prints each figure, asserts once"""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def check(self, name, got, term, chain=None):
        assert tuple(got.shape) == tuple(term.value.shape) or got.numel() == term.value.numel(), name
        bad, worst = R.mismatch(got, term, chain)
        print("%s  %-34s max |err| / bound %.3f   outside %d of %d" % (self.tag, name, worst, int(bad.sum()), bad.numel()))
        if bool(bad.any()):
            self.failed.append((name, worst, int(bad.sum())))
        return bad

    def done(self):
        assert not self.failed, (self.tag, self.failed)


def _device_inputs(c, inp, surface=False):
    d = {k: (None if v is None else g(v)) for k, v in inp.items()}
    bufs = {}
    if c.view:
        d["dg"], bufs["dg"] = _slice(inp["dg"], 8, 4)
        if not surface:
            d["proj"], bufs["proj"] = _slice(inp["proj"], 4, 4)
    return d, bufs


def _check_views(c, inp, bufs):
    if "dg" in bufs:
        _outside_unchanged(bufs["dg"], 8, c.C, inp["dg"])
    if "proj" in bufs:
        _outside_unchanged(bufs["proj"], 4, 8 * c.C, inp["proj"])


def _dxyz_both_lists(ops, rep, d, c, ddir, want, tag):
    """tgp_dirs_to_xyz over tgp_reverse_graph's lists and over tgp_child_lists' (global entries)"""
    rev = ops.reverse_graph(d["idx"], c.n)
    rep.check("dxyz (reverse_graph) " + tag, ops.dirs_to_xyz(d["xyz"], d["idx"], ddir, rev=rev), want)
    ptr, ent = ops.child_lists(d["idx"].view(c.B, c.n * c.k), c.n)
    rep.check("dxyz (child_lists) " + tag, ops.dirs_to_xyz(d["xyz"], d["idx"], ddir, rev=(ptr, ent, 1)), want)


@pytest.mark.parametrize("c", HS_CASES, ids=R.case_id)
def test_hs_kernels_vs_fp64(ops, c):
    """forward (both kernels), d proj and d sdn from the gather form (slots recomputed / recorded) and from the atomic scatter,
    d dir (slots recorded / recomputed), d xyz over both kinds of reverse list: each against the explicit fp64 backward.  k = 64:
    the gather form must decline (tests below), the scatter form, d dir and d xyz are still checked.  Hubs: two runs agree bit for
    bit.  View cases: proj and d g are column slices of wider buffers, whose other columns must come back untouched."""
    inp, share, pre = R.case_inputs(c)
    assert share <= 0.01, share
    want = R.hs_backward_explicit(inp["xyz"], inp["idx"], inp["proj"], inp["sdn"], inp["dg"], c.C, pre=pre)
    fwd = R.forward_terms(None, None, None, None, c.C, pre=pre)
    d, bufs = _device_inputs(c, inp)
    x, idx, proj, sdn, dg = d["xyz"], d["idx"], d["proj"], d["sdn"], d["dg"]
    rep = _Report(R.case_id(c))
    path = R.dsdn_path(c.B, c.n)

    rep.check("out (gconv_hs)", ops.gconv_hs(x, idx, proj, sdn, 7, c.C), fwd, chain=7)
    dproj, dsdn = ops.gconv_hs_bwd(x, idx, proj, sdn, dg, 7, c.C)
    rep.check("dproj (scatter)", dproj, want["dproj"])
    rep.check("dsdn (scatter)", dsdn, want["dsdn"], chain=path)

    gather = ops.gconv_gather_ok(c.C, c.k, proj, sdn)
    assert gather == (c.k <= 63)
    if gather:
        rev = ops.reverse_graph(idx, c.n)
        dproj, dsdn = ops.gconv_hs_bwd_gather(x, idx, rev, proj, sdn, dg, 7, c.C)
        rep.check("dproj (gather)", dproj, want["dproj"])
        rep.check("dsdn (gather)", dsdn, want["dsdn"], chain=path)
        out, slots = ops.gconv_hs_slots(x, idx, proj, sdn, 7, c.C)
        rep.check("out (gconv_hs_slots)", out, fwd, chain=7)
        ddir_s = ops.gconv_dirgrad(x, idx, sdn, dg, 7, c.C, proj=proj, slots=slots)      # before the backward consumes the slots
        rep.check("ddir (slots)", ddir_s, want["ddir"])
        dproj_s, dsdn_s = ops.gconv_hs_bwd_gather(x, idx, rev, proj, sdn, dg, 7, c.C, slots=slots)
        rep.check("dproj (gather, slots)", dproj_s, want["dproj"])
        rep.check("dsdn (gather, slots)", dsdn_s, want["dsdn"], chain=path)
        if c.family == "hub":
            again = ops.gconv_hs_bwd_gather(x, idx, rev, proj, sdn, dg, 7, c.C)
            assert torch.equal(again[0], dproj) and torch.equal(again[1], dsdn)
            assert torch.equal(ops.gconv_dirgrad(x, idx, sdn, dg, 7, c.C, proj=proj, slots=ops.gconv_hs_slots(x, idx, proj, sdn, 7, c.C)[1]),
                               ddir_s)
    ddir = ops.gconv_dirgrad(x, idx, sdn, dg, 7, c.C, proj=proj)
    rep.check("ddir (recomputed)", ddir, want["ddir"])
    if c.family != "coincident":       # (zero directions: test_seam_neighbor_direction_norm_coincident_points)
        _dxyz_both_lists(ops, rep, d, c, ddir, want["dxyz"], "")
    torch.cuda.synchronize()
    _check_views(c, inp, bufs)
    rep.done()


@pytest.mark.parametrize("c", SURFACE_CASES, ids=R.case_id)
def test_surface_kernels_vs_fp64(ops, c):
    """HSlayer_surface.graph_conv: the forward, d sdn (tgp_gconv_surface_bwd: the scatter kernel's two 16-point streams at C = 128,
    k up to 64), d dir and d xyz against the explicit fp64 backward."""
    inp, share, pre = R.case_inputs(c, surface=True)
    assert share <= 0.01, share
    want = R.hs_backward_explicit(inp["xyz"], inp["idx"], None, inp["sdn"], inp["dg"], c.C, surface=True, pre=pre)
    fwd = R.forward_terms(None, None, None, None, c.C, surface=True, pre=pre)
    d, bufs = _device_inputs(c, inp, surface=True)
    x, idx, sdn, dg = d["xyz"], d["idx"], d["sdn"], d["dg"]
    rep = _Report("surface " + R.case_id(c))
    rep.check("out (gconv_surface)", ops.gconv_surface(x, idx, sdn, 7, c.C), fwd, chain=7)
    rep.check("dsdn", ops.gconv_surface_bwd(x, idx, sdn, dg, 7, c.C), want["dsdn"], chain=R.dsdn_path(c.B, c.n))
    ddir = ops.gconv_dirgrad(x, idx, sdn, dg, 7, c.C)
    rep.check("ddir", ddir, want["ddir"])
    if c.family == "hub":
        assert torch.equal(ops.gconv_dirgrad(x, idx, sdn, dg, 7, c.C), ddir)
    if c.family != "coincident":
        _dxyz_both_lists(ops, rep, d, c, ddir, want["dxyz"], "")
    torch.cuda.synchronize()
    _check_views(c, inp, bufs)
    rep.done()


def _nbrmax_inputs(c, per_object, n_rows=None):
    gen = torch.Generator().manual_seed(c.seed + c.n + c.k + c.C + int(per_object))
    src = torch.randn(c.B, c.n, c.C, generator=gen)
    src[:, c.n // 2] = src[:, 0]                                 # exact ties between two sources: the first slot takes them
    idx = R.case_graph(c)
    dy = torch.randn(c.B, c.C, generator=gen) if per_object else torch.randn(c.B, c.n, c.C, generator=gen)
    return src, idx, dy, (1.0 / c.n if per_object else 1.0)


@pytest.mark.parametrize("per_object", [False, True], ids=["rows", "per_object"])
@pytest.mark.parametrize("c", NBRMAX_CASES, ids=R.case_id)
def test_nbrmax_bwd_vs_fp64(ops, c, per_object):
    """the neighbourhood max's backward (Pool_layer; ORL pooling with per_object): the gather form's long walk over a hub's list and
    its dense zero rows for unlisted sources, k = 1 and k = 64, and the atomic scatter, against the fp64 reference; two gather runs
    agree bit for bit."""
    src, idx, dy, scale = _nbrmax_inputs(c, per_object)
    want = R.nbrmax_backward(src, idx, dy, per_object, scale)
    rep = _Report("nbrmax " + R.case_id(c))
    assert ops.nbrmax_gather_ok(c.C, g(src), g(dy))
    rev = ops.reverse_graph(g(idx), c.n)
    got = ops.nbrmax_bwd_gather(g(src), g(idx), rev, g(dy), per_object=per_object, scale=scale)
    rep.check("dsrc (gather)", got, want)
    assert torch.equal(ops.nbrmax_bwd_gather(g(src), g(idx), rev, g(dy), per_object=per_object, scale=scale), got)
    rep.check("dsrc (scatter)", ops.nbrmax_bwd(g(src), g(idx), g(dy), per_object=per_object, scale=scale), want)
    if c.family == "no_self":
        assert bool((got[:, 1::2] == 0).all())                   # nobody lists an odd source: zeros, written densely
    rep.done()


def test_nbrmax_bwd_views(ops):
    """src and d y as column slices of wider buffers, the scatter form's d src a zeroed slice of one: results as before, every
    column outside the slices untouched."""
    c = case("base", 3, 33, 8, 128)
    src, idx, dy, scale = _nbrmax_inputs(c, False)
    want = R.nbrmax_backward(src, idx, dy)
    src_v, src_b = _slice(src, 4, 8)
    dy_v, dy_b = _slice(dy, 8, 4)
    rep = _Report("nbrmax views")
    rev = ops.reverse_graph(g(idx), c.n)
    assert ops.nbrmax_gather_ok(c.C, src_v, dy_v)
    rep.check("dsrc (gather)", ops.nbrmax_bwd_gather(src_v, g(idx), rev, dy_v), want)
    out_v, out_b = _slice(torch.zeros(c.B, c.n, c.C), 4, 4)
    rep.check("dsrc (scatter)", ops.nbrmax_bwd(src_v, g(idx), dy_v, dsrc=out_v), want)
    torch.cuda.synchronize()
    _outside_unchanged(src_b, 4, c.C, src)
    _outside_unchanged(dy_b, 8, c.C, dy)
    _outside_unchanged(out_b, 4, c.C)
    rep.done()


def test_gather_form_declines_k64_without_launching(ops):
    """k = 64 is the scatter kernel's cap and one past the gather form's (slot 255 / 6-bit entries leave 63): gconv_gather_ok is false
    and the entry point returns TGP_EUNSUPPORTED with its outputs untouched."""
    from tgpose_amd import _lib
    c = case("base", 2, 33, 64, 128)
    inp, _, _ = R.case_inputs(c)
    d = {k: g(v) for k, v in inp.items()}
    assert not ops.gconv_gather_ok(c.C, c.k, d["proj"], d["sdn"])
    assert ops.gconv_gather_ok(c.C, 63, d["proj"], d["sdn"])
    rev = ops.reverse_graph(d["idx"], c.n)
    E = c.B * c.n * 7 * c.C
    dproj = torch.full((c.B, c.n, 8 * c.C), FILL, device=DEV)
    dsdn = torch.full((3, 7 * c.C), FILL, device=DEV)
    ws = torch.empty(_lib.lib().tgp_gconv_bwd_workspace_floats(c.B, c.n, c.C), device=DEV)
    arg = torch.full((E,), 9, device=DEV, dtype=torch.uint8)
    contrib = torch.full((E,), FILL, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for have_slots in (0, 1):
        rc = _lib.lib().tgp_gconv_hs_bwd_gather(p(d["xyz"]), p(d["idx"]), p(rev[0]), p(rev[1]), p(d["proj"]), 8 * c.C, p(d["sdn"]), p(d["dg"]),
                                                c.C, c.B, c.n, c.k, 7, c.C, p(dproj), 8 * c.C, p(dsdn), p(ws), p(arg), p(contrib), have_slots,
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == -2
    torch.cuda.synchronize()
    assert bool((dproj == FILL).all()) and bool((dsdn == FILL).all()) and bool((arg == 9).all()) and bool((contrib == FILL).all())
    with pytest.raises(_lib.TgpError):
        ops.gconv_hs_bwd_gather(d["xyz"], d["idx"], rev, d["proj"], d["sdn"], d["dg"], 7, c.C)
    with pytest.raises(_lib.TgpError):
        ops.gconv_hs_slots(d["xyz"], d["idx"], d["proj"], d["sdn"], 7, c.C)


def _move_hub_tail(rev, b, n):
    """a valid but WRONG reverse list: the last entry of the hub's list in object b (its 225th, the first of the second slab) handed
    to the next source's list -- rptr stays monotone, every id stays in range"""
    rptr = rev[0].clone()
    rptr[b * n + R.HUB + 1] -= 1
    return rptr, rev[1]


def test_gconv_hs_bwd_gather_wrong_reverse_list_is_caught(ops):
    """the comparator's teeth: with the hub's 225th entry moved to another source's list the comparison fails on exactly the hub's
    and the recipient's d proj rows -- what a slab-boundary bug (an entry dropped or walked twice) would look like."""
    c = case("hub", 2, N_HUB, 4, 128, L=225)
    inp, _, pre = R.case_inputs(c)
    want = R.hs_backward_explicit(inp["xyz"], inp["idx"], inp["proj"], inp["sdn"], inp["dg"], c.C, pre=pre)
    d = {k: g(v) for k, v in inp.items()}
    rev = ops.reverse_graph(d["idx"], c.n)
    lens = (rev[0][1:] - rev[0][:-1]).view(c.B, c.n)
    assert lens[:, R.HUB].tolist() == [225] * c.B
    good, _ = ops.gconv_hs_bwd_gather(d["xyz"], d["idx"], rev, d["proj"], d["sdn"], d["dg"], 7, c.C)
    assert not bool(R.mismatch(good, want["dproj"])[0].any())
    wrong, _ = ops.gconv_hs_bwd_gather(d["xyz"], d["idx"], _move_hub_tail(rev, 1, c.n), d["proj"], d["sdn"], d["dg"], 7, c.C)
    bad, worst = R.mismatch(wrong, want["dproj"])
    print("wrong list: max |err| / bound %.1f, %d elements outside" % (worst, int(bad.sum())))
    rows = bad.any(-1).nonzero().tolist()
    assert rows == [[1, R.HUB], [1, R.HUB + 1]], rows


def test_nbrmax_bwd_gather_wrong_reverse_list_is_caught(ops):
    """the same for the neighbourhood max's gather form"""
    c = case("hub", 2, N_HUB, 4, 128, L=225)
    src, idx, dy, scale = _nbrmax_inputs(c, False)
    want = R.nbrmax_backward(src, idx, dy)
    rev = ops.reverse_graph(g(idx), c.n)
    good = ops.nbrmax_bwd_gather(g(src), g(idx), rev, g(dy))
    assert not bool(R.mismatch(good, want)[0].any())
    wrong = ops.nbrmax_bwd_gather(g(src), g(idx), _move_hub_tail(rev, 1, c.n), g(dy))
    bad, worst = R.mismatch(wrong, want)
    print("wrong list: max |err| / bound %.1f, %d elements outside" % (worst, int(bad.sum())))
    rows = bad.any(-1).nonzero().tolist()
    assert rows == [[1, R.HUB], [1, R.HUB + 1]], rows
