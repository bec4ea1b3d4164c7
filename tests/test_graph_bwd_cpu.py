"""CPU checks of the fp64 reference that judges the graph layers' backward kernels (tests/graph_bwd_ref.py) and of the cases
tests/test_graph_bwd_gpu.py runs: the hand-derived backward against torch autograd and against the oracle's layers, the share of
d g that the ambiguity mask zeroes (at most 1 % in every GPU case), the graph builders, and the refusal of widths below 128 by the
scatter backward's entry points."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import graph_bwd_ref as R
from tests import test_graph_bwd_gpu as G
from tests.graph_bwd_ref import case

# one small case per graph family (the GPU file's shapes, shrunk where that loses nothing), surface and HS
FAMILY_CASES = [case("hub", 1, G.N_HUB, 4, 128, L=225), case("everyone_lists_2", 1, 60, 20, 128), case("no_self", 2, 40, 5, 128),
                case("repeats", 2, 50, 6, 128), case("coincident", 2, 40, 8, 128), case("base", 3, 17, 20, 128), case("base", 1, 1, 2, 128)]


def _rel(a, b):
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())


@pytest.mark.parametrize("surface", [False, True], ids=["hs", "surface"])
@pytest.mark.parametrize("c", FAMILY_CASES, ids=R.case_id)
def test_explicit_backward_matches_autograd(c, surface):
    """two derivations that must agree before either judges a kernel: hs_backward_explicit against torch float64 autograd of
    hs_forward, to 1e-12 relative, on every graph family with the mask applied; the explicit forward equals hs_forward."""
    inp, share, pre = R.case_inputs(c, surface)
    ex = R.hs_backward_explicit(inp["xyz"], inp["idx"], inp["proj"], inp["sdn"], inp["dg"], c.C, surface, pre=pre)
    x = inp["xyz"].double().requires_grad_(True)
    sd = inp["sdn"].double().requires_grad_(True)
    pj = None if surface else inp["proj"].double().requires_grad_(True)
    out = R.hs_forward(x, inp["idx"], pj, sd, c.C, surface)
    assert _rel(out.detach(), R.forward_terms(None, None, None, None, c.C, surface, pre=pre).value) <= 1e-14
    grads = torch.autograd.grad(out, [x, sd] + ([] if surface else [pj]), inp["dg"].double(), allow_unused=True)
    got = {"dxyz": ex["dxyz"].value, "dsdn": ex["dsdn"].value}
    want = {"dxyz": grads[0] if grads[0] is not None else torch.zeros_like(x), "dsdn": grads[1]}
    if not surface:
        got["dproj"], want["dproj"] = ex["dproj"].value, grads[2]
    # d dir: autograd of the same forward with the unit directions as the leaf
    B, n, k = inp["idx"].shape
    b = torch.arange(B).view(B, 1, 1)
    u = (inp["xyz"].double()[b, inp["idx"].long()] - inp["xyz"].double().unsqueeze(2))
    dleaf = F.normalize(u, dim=-1, eps=1e-12).requires_grad_(True)
    val = torch.relu(dleaf @ inp["sdn"].double()).view(B, n, k, R.S, c.C)
    if not surface:
        val = val * inp["proj"].double()[..., c.C:].reshape(B, n, R.S, c.C)[b, inp["idx"].long()]
    m = val.gather(2, val.argmax(2, keepdim=True)).squeeze(2).sum(2) / 7.0
    got["ddir"], want["ddir"] = ex["ddir"].value, torch.autograd.grad(m, dleaf, inp["dg"].double())[0]
    for name in got:
        rel = _rel(got[name], want[name])
        print("%s %s %s: |explicit - autograd| / |autograd| = %.2e" % (R.case_id(c), "surface" if surface else "hs", name, rel))
        assert rel <= 1e-12, (name, rel)
    for name, t in ex.items():       # the bound's ingredients: |value| can never exceed the sum of its terms' absolute values
        assert bool((t.value.abs() <= t.abs_terms * (1 + 1e-12) + 1e-300).all()), name
        assert bool((t.chain >= 0).all()) and bool(((t.chain == 0) <= (t.value == 0)).all()), name


def test_explicit_backward_matches_oracle_layers():
    """the oracle's own layers (oracle/gcn_ref.py hs_conv / surface_conv: the reference's op sequence) in float64 on an injected
    graph, reduced to their graph convolution (zero STE and ORL weights, an identity projection): d proj, d directions (through
    F.normalize, which the explicit form leaves to its caller) and d xyz."""
    from oracle import gcn_ref
    c = case("base", 2, 40, 8, 128)
    for surface in (False, True):
        inp, _, _ = R.case_inputs(c, surface)
        x = inp["xyz"].double().requires_grad_(True)
        raw = (inp["sdn"].double() * (0.5 + torch.rand(1, 7 * c.C, dtype=torch.float64))).requires_grad_(True)   # unnormalised
        # the layer normalises its directions itself, in float64: the explicit form gets exactly those (inp["sdn"] is unit to fp32)
        sdn = F.normalize(raw.detach(), dim=0)
        pre = R._setup(inp["xyz"], inp["idx"], inp["proj"], sdn, c.C, surface)
        ex = R.hs_backward_explicit(inp["xyz"], inp["idx"], inp["proj"], sdn, inp["dg"], c.C, surface, pre=pre)
        cache = gcn_ref.GraphCache(mode="torch", inject={"L.rf": inp["idx"].long(), "L.orl_xyz": inp["idx"].long()})
        P = {"_support_num": 7, "L.directions": raw}
        if surface:
            P["L.STE_layer.weight"] = torch.zeros(c.C, 3, 1, dtype=torch.float64)
            P["L.conv2.weight"] = torch.zeros(c.C, 2 * c.C, 1, dtype=torch.float64)
            out = gcn_ref.surface_conv(P, "L", x, c.k, cache)
            leaves = [x, raw]
        else:
            fmap = inp["proj"].double().requires_grad_(True)
            P.update({"L.weights": torch.eye(8 * c.C, dtype=torch.float64), "L.bias": torch.zeros(8 * c.C, dtype=torch.float64),
                      "L.STE_layer.weight": torch.zeros(c.C, 8 * c.C, 1, dtype=torch.float64),
                      "L.conv2.weight": torch.zeros(c.C, 2 * c.C, 1, dtype=torch.float64)})
            out = gcn_ref.hs_conv(P, "L", x, fmap, c.k, cache)
            leaves = [x, raw, fmap]
        assert _rel(out.detach(), R.forward_terms(None, None, None, None, c.C, surface, pre=pre).value) <= 1e-12
        grads = torch.autograd.grad(out, leaves, inp["dg"].double())
        # push the explicit d sdn through F.normalize's backward
        raw2 = raw.detach().clone().requires_grad_(True)
        (draw,) = torch.autograd.grad(F.normalize(raw2, dim=0), raw2, ex["dsdn"].value)
        assert _rel(ex["dxyz"].value, grads[0]) <= 1e-12
        assert _rel(draw, grads[1]) <= 1e-12
        if not surface:
            assert _rel(ex["dproj"].value, grads[2]) <= 1e-12


def test_zeroed_share_of_every_gpu_case_is_at_most_one_percent():
    """the condition under which the masked comparison still says something: in every parametrised GPU case the ambiguity mask zeroes
    at most 1 % of d g's entries (measured on the reference alone; a case that exceeds it gets another seed, never another cap)"""
    worst = 0.0
    for surface, cases in ((False, G.HS_CASES), (True, G.SURFACE_CASES)):
        for c in cases:
            _, share, _ = R.case_inputs(c, surface)
            print("%-8s %-40s zeroed share %.3f %%" % ("surface" if surface else "hs", R.case_id(c), 100 * share))
            assert share <= 0.01, (R.case_id(c), share)
            worst = max(worst, share)
    assert len(G.HS_CASES) + len(G.SURFACE_CASES) + 2 * len(G.NBRMAX_CASES) <= 48
    print("largest share %.3f %%" % (100 * worst))


def test_ambiguous_marks_close_calls_and_leaves_exact_ties():
    """the mask on constructed inputs: a margin below 1e-5 max|proj| between two different sources and a |theta| below 1e-6 are
    marked; a source listed twice and an all-zero maximum (exact ties) are not."""
    C = 128
    xyz = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]])
    sdn = torch.zeros(3, 7 * C)
    sdn[0] = 1.0                                                     # every support direction is +x
    proj = torch.ones(1, 4, 8 * C)
    idx = torch.tensor([[[1, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]], dtype=torch.int32)
    # row 0 lists source 1 twice (theta = 1, an exact tie); rows 1..3 see only directions with theta <= 0: maxima exactly zero
    assert not bool(R.ambiguous(xyz, idx, proj, sdn, C).any())
    idx2 = torch.tensor([[[1, 2, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]], dtype=torch.int32)
    xyz2 = xyz.clone()
    xyz2[0, 2] = torch.tensor([1.0, 0.001, 0.0])                     # source 2's direction: theta = 1 - 5e-7, another source
    amb = R.ambiguous(xyz2, idx2, proj, sdn, C)
    assert bool(amb[0, 0].all()) and not bool(amb[0, 1:].any())
    xyz3 = xyz.clone()
    xyz3[0, 1] = torch.tensor([1e-7, 1.0, 0.0])                      # theta = 1e-7
    amb = R.ambiguous(xyz3, idx, proj, sdn, C)
    assert bool(amb[0, 0].all())


def test_graph_builders_build_what_they_claim():
    for L in (223, 224, 225, 448, 449):
        idx = R.graph_hub(2, G.N_HUB, 4, L, 5)
        assert (idx == R.HUB).sum((1, 2)).tolist() == [L, L]        # exactly L entries, the hub's own self entry included
        assert bool((idx[:, :, 0] == torch.arange(G.N_HUB)).all())
        assert int((idx == R.HUB).sum(2).max()) == 1                 # by L distinct rows
        assert int(idx.min()) >= 0 and int(idx.max()) < G.N_HUB
    hub_cases = [c for c in G.HS_CASES if c.family == "hub"]
    assert sorted({c.L for c in hub_cases if c.C == 128}) == [223, 224, 225, 448, 449]
    assert {c.C for c in hub_cases if c.L == 225} == {128, 256, 512}
    for c in hub_cases:
        assert (R.case_graph(c) == R.HUB).sum((1, 2)).tolist() == [c.L] * c.B
    idx = R.graph_everyone_lists_2(2, 300, 20, 1)
    assert bool((idx[:, :, 1] == 2).all()) and bool((idx[:, :, 0] == torch.arange(300)).all()) and int((idx == 2).sum()) > 2 * 300
    idx = R.graph_no_self(3, 41, 5, 2)
    assert not bool((idx == torch.arange(41).view(1, 41, 1)).any()) and bool((idx % 2 == 0).all())
    assert int(idx.min()) >= 0 and int(idx.max()) < 41
    idx = R.graph_repeats(2, 50, 6, 3)
    assert bool((idx[:, :, 1] == idx[:, :, 2]).all()) and bool((idx[:, ::3, 4] == idx[:, ::3, 1]).all())
    idx = R.graph_coincident(2, 40, 8, 4)
    assert idx[0, :10, 1].tolist() == list(range(10, 20)) and idx[1, 10:20, 1].tolist() == list(range(10))
    inp, _, _ = R.case_inputs(case("coincident", 2, 40, 8, 128))
    assert torch.equal(inp["xyz"][:, 10:20], inp["xyz"][:, :10])
    for c in G.HS_CASES + G.SURFACE_CASES + G.NBRMAX_CASES:
        idx = R.case_graph(c)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (c.B, c.n, c.k) and int(idx.min()) >= 0 and int(idx.max()) < c.n


def test_nbrmax_backward_matches_autograd():
    gen = torch.Generator().manual_seed(3)
    src = torch.randn(2, 30, 16, generator=gen)
    src[:, 7] = src[:, 2]
    idx = R.graph_base(2, 30, 5, 9)
    for per_object in (False, True):
        dy = torch.randn(2, 16, generator=gen) if per_object else torch.randn(2, 30, 16, generator=gen)
        t = R.nbrmax_backward(src, idx, dy, per_object, 1.0 / 30 if per_object else 1.0)
        s = src.double().requires_grad_(True)
        v = s[torch.arange(2).view(2, 1, 1), idx.long()]
        y = v.gather(2, v.argmax(2, keepdim=True)).squeeze(2)
        gy = (dy.double().unsqueeze(1).expand(2, 30, 16) / 30) if per_object else dy.double()
        (want,) = torch.autograd.grad(y, s, gy)
        assert _rel(t.value, want) <= 1e-12
        assert bool((t.value.abs() <= t.abs_terms * (1 + 1e-12)).all())


def test_scatter_backward_refuses_widths_below_128_without_launching():
    """tgp_gconv_surface_bwd / tgp_gconv_hs_bwd stage two 16-point streams per workgroup; C = 64 or 32 would launch four or eight
    (256 / C) into the same arrays.  The entry points return TGP_EUNSUPPORTED before any launch (the pointers here are not device
    memory), the ops wrappers raise before they touch a tensor, and a width the kernels do serve still passes the argument checks
    that follow (a null pointer: TGP_EINVAL)."""
    from tgpose_amd import _lib, ops
    lib = _lib.lib()
    fake = ctypes.c_void_p(1 << 20)
    for C in (64, 32, 16):
        assert lib.tgp_gconv_surface_bwd(fake, fake, fake, fake, C, 2, 40, 8, 7, C, fake, fake, None) == -2, C
        assert lib.tgp_gconv_hs_bwd(fake, fake, fake, 8 * C, fake, fake, C, 2, 40, 8, 7, C, fake, 8 * C, fake, fake, None) == -2, C
        z = torch.zeros(1)
        with pytest.raises(ValueError, match="C >= 128"):
            ops.gconv_surface_bwd(z, z, z, z, 7, C)
        with pytest.raises(ValueError, match="C >= 128"):
            ops.gconv_hs_bwd(z, z, z, z, z, 7, C)
    assert lib.tgp_gconv_surface_bwd(None, fake, fake, fake, 128, 2, 40, 8, 7, 128, fake, fake, None) == -1
    assert lib.tgp_gconv_hs_bwd(fake, fake, None, 1024, fake, fake, 128, 2, 40, 8, 7, 128, fake, 1024, fake, fake, None) == -1
    # the gather form's own cap, checked the same way: k = 64 is refused before any launch
    a16 = ctypes.c_void_p(1 << 20)
    assert lib.tgp_gconv_hs_bwd_gather(a16, a16, a16, a16, a16, 1024, a16, a16, 128, 2, 40, 64, 7, 128, a16, 1024, a16, a16, a16, a16, 0,
                                       None) == -2
    assert not ops.gconv_gather_ok(128, 64) and ops.gconv_gather_ok(128, 63)
