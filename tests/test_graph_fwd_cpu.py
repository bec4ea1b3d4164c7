"""CPU checks of what judges the forward graph kernels (tests/graph_fwd_ref.py) and of the cases tests/test_graph_fwd_gpu.py runs:
the launch-form rules on both sides of every boundary, each boundary recomputed from the byte formulas of csrc/gconv.hip's launch
code; the fp64 forward against graph_bwd_ref.hs_forward and the oracle; the slot_wins shares; that a reference with a slot dropped
lands outside the bar; and that every GPU case's reference is small and quick to build."""
import time

import pytest
import torch

from tests import graph_bwd_ref as R
from tests import graph_fwd_ref as F
from tests import test_graph_fwd_gpu as G
from tests.graph_fwd_ref import case, case_id

KIB = 1024


def _last(fits, lo=1, hi=1 << 20):
    """the largest n in [lo, hi) with fits(n), by bisection, checked to be a boundary: fits(n) and not fits(n + 1)"""
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    assert fits(lo) and not fits(lo + 1)
    return lo


# ------------------------------------------------------------------------------------------------------------------ the form rules
def test_gconv_form_boundaries():
    """gconv_lds_launch: the table is n * 7 * ch * 4 bytes, the widest slice of 16 / 8 channels that fits 72 KiB is taken, none
    means the gather kernel; gconv_lds_go opts in above 64 KiB"""
    last16 = _last(lambda n: n * 7 * 16 * 4 <= 72 * KIB)
    last8 = _last(lambda n: n * 7 * 8 * 4 <= 72 * KIB)
    plain16 = _last(lambda n: n * 7 * 16 * 4 <= 64 * KIB)
    plain8 = _last(lambda n: n * 7 * 8 * 4 <= 64 * KIB)
    assert (plain16, last16, plain8, last8) == (146, 164, 292, 329)
    for C in (128, 256, 512):
        for n in range(1, 400):
            want = 16 if n <= last16 else 8 if n <= last8 else 0
            assert F.gconv_form(n, C) == want, (n, C)
            assert F.gconv_opt_in(n, C) == (plain16 < n <= last16 or plain8 < n <= last8), (n, C)
    assert [F.gconv_form(n, 128) for n in (146, 147, 164, 165, 292, 293, 329, 330)] == [16, 16, 16, 8, 8, 8, 8, 0]
    assert [F.gconv_opt_in(n, 128) for n in (146, 147, 164, 165, 292, 293, 329, 330)] == [False, True, True, False, False, True, True, False]


def _orl_bytes(n, planes):
    ptiles = (n + 63) // 64
    return 4 * (16 * n + 64 * ptiles + ((n // 32 + 4) if planes else 0))


def test_orl_form_boundaries():
    """orl_lds_launch: 4 (16 n + 64 ceil(n / 64) [+ n / 32 + 4]) <= 72 KiB for the LDS form; the lists beside it as 16-bit ids when
    (n k) % 4 == 0, the pointer is aligned and all fits 150 KiB; threads from the slot count 32 ceil(n / 64)"""
    last_plain = _last(lambda n: _orl_bytes(n, False) <= 72 * KIB, hi=4096)
    last_planes = _last(lambda n: _orl_bytes(n, True) <= 72 * KIB, hi=4096)
    assert (last_plain, last_planes) == (1084, 1081)
    # the budget is not monotone in n (a tile's 64 floats arrive at once): no n below the boundary may fail, none above it fit
    assert all(_orl_bytes(n, p) <= 72 * KIB for p, last in ((False, last_plain), (True, last_planes)) for n in range(1, last + 1))
    assert not any(_orl_bytes(n, p) <= 72 * KIB for p, last in ((False, last_plain), (True, last_planes)) for n in range(last + 1, 4096))
    for n in range(1, 1200):
        for planes in (False, True):
            assert (F.orl_form(n, 20, 128, planes)[0] == "lds") == (n <= (last_planes if planes else last_plain)), (n, planes)
            assert F.orl_lds_bytes(n, planes) == _orl_bytes(n, planes)
    assert [F.orl_form(n, 20, 128)[0] for n in (1084, 1085)] == ["lds", "gather"]
    assert [F.orl_form(n, 20, 512, planes=True)[0] for n in (1081, 1082)] == ["lds", "gather"]

    last_lists64 = _last(lambda n: _orl_bytes(n, False) + 2 * n * 64 <= 150 * KIB, hi=4096)
    assert last_lists64 == 782
    assert _orl_bytes(782, True) + 2 * 782 * 64 <= 150 * KIB                 # (the planes' words do not move this boundary)
    assert [F.orl_form(n, 64, 128)[1] for n in (782, 783)] == [True, False]
    assert [F.orl_form(n, 64, 128, planes=True)[1] for n in (782, 783)] == [True, False]
    assert F.orl_form(257, 7, 128)[1] is False and (257 * 7) % 4 != 0          # lists read from memory: n k no multiple of 4
    assert F.orl_form(1028, 7, 128)[1] is True and F.orl_form(257, 20, 128)[1] is True
    assert F.orl_form(300, 20, 128, aligned=False)[1] is False                 # ... or a list off the 16-byte grid
    assert F.orl_form(1085, 20, 128) == ("gather", False, 256)

    last256 = _last(lambda n: 32 * ((n + 63) // 64) < 384, hi=4096)
    last512 = _last(lambda n: 32 * ((n + 63) // 64) < 768, hi=4096)
    assert (last256, last512) == (704, 1472)                                   # 1024 threads would need n >= 1473: never an LDS shape
    assert [F.orl_form(n, 20, 128)[2] for n in (704, 705, 1084)] == [256, 512, 512]
    assert F.orl_chain(1) == 21 and F.orl_chain(64) == 21 and F.orl_chain(65) == 22 and F.orl_chain(1085) == 37


def test_gpu_cases_reach_both_sides_of_every_switch():
    """the case lists of tests/test_graph_fwd_gpu.py, read through the form rules: every form and both sides of every boundary"""
    hs = {(c.n, c.C, c.B) for c in G.HS_CASES}
    for n in (146, 147, 164, 165, 292, 293, 329, 330):
        assert any(m == n and C == 128 for m, C, _ in hs), n
    for C in (256, 512):
        assert {164, 165, 329, 330} <= {m for m, CC, _ in hs if CC == C}
    for form in (16, 8, 0):
        for B in (1, 3):
            assert any(F.gconv_form(c.n, c.C) == form and c.B == B for c in G.HS_CASES), (form, B)
        for fam in (G.SW,) + G.HS_FAMILIES:
            assert any(F.gconv_form(c.n, c.C) == form and c.family == fam for c in G.HS_CASES), (form, fam)
        assert any(F.gconv_form(c.n, c.C) == form and c.view for c in G.HS_CASES), form
    for n in (165, 330):
        assert {1, 2, 7, 20, 63, 64} <= {c.k for c in G.HS_CASES if c.n == n and c.C == 128}
    assert all(c.B * c.k <= 16 for c in G.HS_CASES if c.C == 512)
    assert {(c.n, c.C, c.k) for c in G.SURFACE_CASES} >= {(n, C, k) for n in (1, 15, 16, 17, 330) for C in (128, 256, 512) for k in (1, 7, 64)}

    forms = {F.orl_form(c.n, c.k, c.C, aligned=not c.view) for c in G.ORL_CASES}
    assert forms >= {("lds", True, 256), ("lds", True, 512), ("lds", False, 256), ("lds", False, 512), ("gather", False, 256)}
    assert {c.n for c in G.ORL_CASES if c.C == 128 and c.k == 20 and c.B == 3} >= set(G.ORL_EDGES)
    assert {c.n for c in G.ORL_CASES if c.C == 512} >= {1081, 1082, 1084, 1085}
    assert {(c.n, c.k) for c in G.ORL_CASES} >= {(257, 7), (1028, 7), (782, 64), (783, 64)}
    assert any(c.view for c in G.ORL_CASES) and any(c.n == 1 for c in G.ORL_CASES)
    for lists in (G.HS_CASES, G.SURFACE_CASES, G.ORL_CASES):
        assert len({case_id(c) for c in lists}) == len(lists)


# ------------------------------------------------------------------------------------------------------------------ the references
FAMILY_CASES = [case(G.SW, 2, 40, 8, 128), case("base", 3, 17, 20, 128), case("repeats", 2, 50, 6, 128), case("coincident", 2, 40, 8, 128),
                case("no_self", 2, 40, 5, 128), case("ends", 2, 33, 7, 128), case("base", 1, 1, 2, 128)]


@pytest.mark.parametrize("surface", [False, True], ids=["hs", "surface"])
@pytest.mark.parametrize("c", FAMILY_CASES, ids=case_id)
def test_hs_terms_match_hs_forward(c, surface, monkeypatch):
    """hs_terms' value is graph_bwd_ref.hs_forward's to 1e-12 (in one piece and in slices of three points), its bound is nowhere below
    forward_terms', and the value lies within its own abs_terms"""
    inp = F.hs_inputs(c, surface)
    args = (inp["xyz"], inp["idx"], inp["proj"], inp["sdn"], c.C, surface)
    want = R.hs_forward(*args)
    whole = F.hs_terms(*args)
    monkeypatch.setattr(F, "BUDGET", 3 * 8 * 8 * c.B * c.k * F.S * c.C)
    sliced = F.hs_terms(*args)
    for t in (whole, sliced):
        assert tuple(t.value.shape) == (c.B, c.n, c.C)
        assert float((t.value - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert torch.equal(whole.value, sliced.value) and torch.equal(whole.abs_terms, sliced.abs_terms)
    old = R.forward_terms(*args)
    assert bool((R.bound(whole, 7) >= R.bound(old, 7)).all())
    assert bool((whole.value.abs() <= whole.abs_terms * (1 + 1e-12) + 1e-300).all())


@pytest.mark.parametrize("c", [case(G.SW, 3, 65, 20, 128), case("repeats", 2, 130, 7, 256), case("ends", 2, 64, 5, 128), case("base", 3, 1, 3, 128)],
                         ids=case_id)
def test_orl_terms_match_the_oracle(c):
    """orl_terms' g is the oracle's gather_rows(...).max(2)[0].mean(1) in fp64 to 1e-12, rb its product with W2^T; pool_ref and
    gather_ref are the oracle's selections"""
    from oracle import gcn_ref
    inp = F.orl_inputs(c)
    g, rb = F.orl_terms(inp["feat"], inp["idx"], inp["w2t"])
    want = gcn_ref.gather_rows(inp["feat"].double(), inp["idx"].long()).max(2)[0].mean(1)
    assert float((g.value - want).abs().max()) <= 1e-12
    assert float((rb.value - want @ inp["w2t"].double()).abs().max()) <= 1e-12
    assert bool((g.value.abs() <= g.abs_terms + 1e-300).all()) and bool((rb.value.abs() <= rb.abs_terms * (1 + 1e-12)).all())
    assert float(g.chain.max()) == F.orl_chain(c.n) and float(rb.chain.max()) == F.orl_chain(c.n) + c.C
    sample = torch.randint(0, c.n, (max(1, c.n // 3),), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    xyz = torch.randn(c.B, c.n, 3, generator=torch.Generator().manual_seed(2))
    kp = min(4, c.k)
    v, f = F.pool_ref(xyz, inp["feat"], inp["idx"], sample, kp)
    assert torch.equal(f, gcn_ref.gather_rows(inp["feat"], inp["idx"].long()[:, sample.long(), :kp]).max(2)[0])
    assert torch.equal(v, xyz[:, sample.long()])
    near = torch.randint(0, c.n, (c.B, 2 * c.n), generator=torch.Generator().manual_seed(3))
    assert torch.equal(F.gather_ref(inp["feat"], near), gcn_ref.gather_rows(inp["feat"], near.unsqueeze(-1)).squeeze(2))


def test_normalize_dirs_ref():
    d = torch.randn(3, 9, generator=torch.Generator().manual_seed(0))
    d[:, 0], d[:, 1] = 0.0, d[:, 1] * 1e-20
    want = F.normalize_dirs_ref(d)
    assert bool((want[:, 0] == 0).all()) and float(want[:, 1].norm()) < 1e-7
    assert float((want[:, 2:].norm(dim=0) - 1).abs().max()) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- slot_wins' teeth
HS_SLOT_CASES = [c for c in G.HS_CASES if c.family == G.SW]
ORL_SLOT_CASES = [c for c in G.ORL_CASES if c.family == G.SW]


@pytest.mark.parametrize("c", HS_SLOT_CASES, ids=case_id)
def test_hs_slot_wins_shares_and_dropped_slots(c):
    """on every slot_wins case the GPU file runs: each slot is the strict winner of at least 1 / (4 k) of the (point, support,
    channel) entries by at least 100 bars, and a forward that leaves out slot 0 or slot k - 1 lands outside the bar"""
    inp, want = G.hs_reference(c)
    shares = F.hs_slot_shares(inp["xyz"], inp["idx"], inp["proj"], inp["sdn"], c.C)
    print("%s  smallest share x k = %.3f" % (case_id(c), float(shares.min()) * c.k))
    assert float(shares.min()) >= 1.0 / (4 * c.k), shares
    for name, keep in (("slot 0", slice(1, None)), ("slot k - 1", slice(0, c.k - 1))):
        if c.k == 1:
            continue
        wrong = F.hs_terms(inp["xyz"], inp["idx"][:, :, keep].contiguous(), inp["proj"], inp["sdn"], c.C).value
        bad, worst = R.mismatch(wrong, want)
        print("%s  without %s: %d of %d elements outside, largest %.0f bars" % (case_id(c), name, int(bad.sum()), bad.numel(), worst))
        assert float(bad.double().mean()) >= 1.0 / (4 * c.k), name


@pytest.mark.parametrize("c", ORL_SLOT_CASES, ids=case_id)
def test_orl_slot_wins_shares_and_dropped_slots(c):
    """the same for ORL's (point, channel) entries; without a slot most of g and of rb leaves its bar"""
    inp, (want_g, want_rb) = G.orl_reference(c)
    shares = F.orl_slot_shares(inp["feat"], inp["idx"])
    print("%s  smallest share x k = %.3f" % (case_id(c), float(shares.min()) * c.k))
    assert float(shares.min()) >= 1.0 / (4 * c.k), shares
    for name, keep in (("slot 0", slice(1, None)), ("slot k - 1", slice(0, c.k - 1))):
        g, rb = F.orl_terms(inp["feat"], inp["idx"][:, :, keep].contiguous(), inp["w2t"])
        bad_g, worst_g = F.orl_mismatch(g.value, want_g)
        bad_rb, worst_rb = F.orl_mismatch(rb.value, want_rb)
        print("%s  without %s: g %.0f bars, rb %.0f bars" % (case_id(c), name, worst_g, worst_rb))
        # (a channel escapes only if none of its n points has its maximum at that slot: (1 - 1 / k)^n of the channels, 4 % at worst)
        assert float(bad_g.double().mean()) >= 0.5 and float(bad_rb.double().mean()) >= 0.5, name


# ------------------------------------------------------------------------------------------------------------------ cost of a case
def test_gpu_references_are_small_and_quick():
    """every GPU case's reference stays under the float64 budget by construction (slices of points) and is built in about two
    seconds at the most (built afresh here, past the cache the tests share); the slowest are printed"""
    assert F.BUDGET <= 300e6
    cost = []
    for c in G.HS_CASES:
        assert 8 * 8 * c.B * c.k * F.S * c.C <= F.BUDGET, c                  # one point's slice fits
        t = time.perf_counter()
        G.hs_reference.__wrapped__(c)
        cost.append((time.perf_counter() - t, "hs " + case_id(c)))
    for c in G.SURFACE_CASES:
        assert 8 * 8 * c.B * c.k * F.S * c.C <= F.BUDGET, c
        t = time.perf_counter()
        G.hs_reference.__wrapped__(c, True)
        cost.append((time.perf_counter() - t, "surface " + case_id(c)))
    for c in G.ORL_CASES:
        assert 3 * 8 * c.B * c.n * c.C <= F.BUDGET, c
        t = time.perf_counter()
        G.orl_reference.__wrapped__(c)
        cost.append((time.perf_counter() - t, "orl " + case_id(c)))
    cost.sort(reverse=True)
    print("slowest references: " + ", ".join("%s %.2f s" % (name, t) for t, name in cost[:5]))
    assert cost[0][0] <= 4.0, cost[0]                                        # (two seconds, with room for a busy machine)
