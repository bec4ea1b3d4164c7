"""The range-guard cases of tests/range_cases.py bite: on the CPU, with a model of the UNGUARDED split arithmetic against fp64.

tests/test_range_guard_gpu.py demands `flag == 1` of the kernels for the cases marked must_flag.  That demand has teeth only if a
kernel that computed on regardless were wrong there -- which is what this file shows, case by case: the modelled unguarded result
misses the project's bar at the affected rows by at least 10 x, while the operand the kernel reads has every 32-row magnitude word
inside [2^-4, 65504) (so the input-side guard cannot be what fires).  For the cases that are NOT marked (the base operands, a value
in [65504, 65519] that fp16 still holds, anything at layer 4, whose activation is consumed in fp32) it shows the opposite: the
unguarded arithmetic is within the bar, so a kernel may keep its flag at 0 there.
"""
import pytest
import torch

from tests import range_cases as rc


def _check(c, x, layers, last, bar, operand, layer_index):
    acts = []
    ref = rc.chain_fp64(x, layers, last, acts=acts)
    got = rc.chain_split_model(x, layers, last)
    # the operand of the kernel is in range in every case: its input-side guard stays quiet
    assert rc.in_range(rc.block_amax(operand)), "operand out of range"
    err = rc.rel_err(got, ref, c["rows"])
    print("%s layer %s p %s ch %s: modelled unguarded error %.3g of the output's scale (bar %.1g)" % (c["kind"], c.get("layer"), c["p"], c["ch"], err, bar))
    if c["must_flag"]:
        assert err >= 10 * bar, err
    else:
        assert rc.rel_err(got, ref) <= bar, rc.rel_err(got, ref)
    if layer_index is None:
        return ref, got
    v = acts[layer_index]
    if c["kind"] in ("big-one", "edge-finite"):
        over = torch.nonzero(v >= rc.FP16_MAX)
        assert over.tolist() == [[c["p"], c["ch"]]], over.tolist()              # exactly one (point, channel) of the layer
        top = v[c["p"], c["ch"]].item()
        assert (top >= rc.FP16_INF) if c["kind"] == "big-one" else (rc.FP16_MAX <= top <= 65519.0), top
        v2 = v.clone()
        v2[c["p"], c["ch"]] = 0
        assert v2.max().item() < 60000.0
    elif c["kind"] == "big-all":
        assert (torch.relu(v).view(v.shape[0], -1).max(1)[0] >= rc.FP16_INF).all()     # every point has a channel beyond fp16
    elif c["kind"] == "tiny":
        a = rc.block_amax(torch.relu(v))
        assert (a < rc.FP16_MIN).all() and (a > 0).all()                        # every block of the activation is under 2^-4, none all zero
    return ref, got


DEC_CASES = ([("base", None, None, None)] + [(k, l, None, None) for k in ("big-all", "tiny") for l in (2, 3, 4)]
             + [(k,) + pl for k in ("big-one", "edge-finite") for pl in rc.dec_big_one_placements()])


@pytest.mark.parametrize("kind,layer,p,ch", DEC_CASES)
def test_decoder_chain_cases(kind, layer, p, ch):
    """tgp_dec_fused on an operand from planes_split: layers 2 / 3 are split again inside the kernel, layer 4 is not."""
    c = rc.dec_case(kind, layer, p, ch)
    x, layers, last = rc.dec_chain(c)
    ref, _ = _check(c, x, layers, last, rc.BAR_DEC, rc.dec_operand(c), None if layer is None else rc.dec_layer_index(c, layer))
    if kind == "tiny":                                             # powers of two: the fp64 result is the base case's, bit for bit
        assert torch.equal(ref, rc.chain_fp64(*rc.dec_chain(rc.dec_case("base"))))
    assert c["must_flag"] == (kind in ("big-all", "big-one", "tiny") and layer < 4)


DEC_L1_CASES = ([("base", None, None, None, None), ("big-all", 1, None, None, None), ("tiny", 1, None, None, None)]
                + [("big-one", 1, p, ch, None) for p, ch in zip(rc.DEC_POINTS, rc.DEC_CHANNELS[1] * 2)]
                + [("edge-finite", 1, 300, 77, None)]
                + [("big-one",) + pl + (None,) for pl in rc.dec_edge_placements((2, 3))]
                + [("nan-addend", 1, p, ch, (what, value)) for what, p, ch in (("p1", 300, 77), ("rowbias", 898, 470))
                   for value in (float("nan"), float("inf"))])


@pytest.mark.parametrize("kind,layer,p,ch,extra", DEC_L1_CASES)
def test_decoder_first_conv_cases(kind, layer, p, ch, extra):
    """tgp_dec_l1 -> tgp_dec_fused: the first conv's activation travels as fp16 planes whose magnitude words are dec_l1's to record."""
    what, value = extra or (None, None)
    c = rc.dec_case(kind, layer, p, ch, l1=True, what=what, value=value)
    x, layers, last = rc.dec_chain(c)
    ref, got = _check(c, x, layers, last, rc.BAR_DEC, rc.dec_operand(c), None if kind in ("base", "nan-addend") else rc.dec_layer_index(c, layer))
    if kind == "nan-addend":
        # the unguarded kernel's rows are finite (ReLU as fmax turns the NaN sums into zeros): silently wrong, not loudly
        assert torch.isfinite(got[c["rows"]]).all() and not torch.isfinite(ref[c["rows"]]).all()


HEADS_CASES = [(B, N, kind, which) for B, N in rc.HEADS_SHAPES
               for kind, which in (("base", None), ("big-all", None), ("tiny", None), ("big-one", 0), ("big-one", 1), ("edge-finite", 0), ("edge-finite", 1))
               if which is None or which < len(rc.heads_points(B, N))]


@pytest.mark.parametrize("B,N,kind,which", HEADS_CASES)
def test_heads_cases(B, N, kind, which):
    """tgp_heads_fused: conv1's activation (1024 channels of a head) is split inside the kernel for conv2."""
    p = None if which is None else rc.heads_points(B, N)[which]
    c = rc.heads_case(kind, B, N, hd=1, p=p, ch=None if which is None else 333 + 300 * which)
    x, layers, last = rc.heads_chain(c, c["hd"])
    _check(c, x, layers, last, rc.BAR_HEADS, x, None if kind == "base" else 0)
    # the coarse products the kernel gathers are in range too (they are added in fp32, never split)
    assert torch.isfinite(c["P1"]).all() and torch.isfinite(c["P2"]).all()


@pytest.mark.parametrize("kind", ["base", "big-one", "edge-finite"])
def test_hs_chain_cases(kind):
    """tgp_hs_chain: one row of the partial last tile (rows 1024 .. 1027 of 1028)"""
    c = rc.hs_case(kind, p=None if kind == "base" else 1026, ch=None if kind == "base" else 100)
    x, layers, last = rc.hs_chain_layers(c)
    _check(c, x, layers, last, 2 * rc.BAR_HS, x, None if kind == "base" else 0)
