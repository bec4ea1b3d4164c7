"""The fused kernels' fp16 range guards at every INNER layer (run on the MI355X with ``-m gpu``).

The contract asserted everywhere (tests/range_cases.py states it and builds the cases):

    the range flag stays 0  =>  the output is within the bar of fp64 at every live row;  otherwise the flag is 1.

For the cases marked must_flag the flag has to be 1: tests/test_range_guard_cpu.py shows that arithmetic that splits on regardless
misses the bar there by more than 10 x, with the kernel's operand in range -- so a kernel that leaves its flag at 0 returns a wrong
(and finite, so silently wrong) result.
"""
import pytest
import torch

from tests import range_cases as rc
from tests.util import fused_kernels_fp64, run_fused_kernels, synth_points

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT_OF_RANGE = lambda am: am >= 0x477fe000 or (am != 0 and am < 0x3d800000)       # TGP_FP16_OUT_OF_RANGE over a magnitude word


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    from tgpose_amd import ops as _ops, _lib
    _lib.lib()  # raises if libtgpose_hip.so is missing: there is no fallback
    return _ops


def d(t):
    return t.contiguous().to(DEV)


def _contract(c, out, flag, ref, bar, what):
    """flag 0 => within the bar at every row; must_flag => flag 1"""
    assert flag in (0, 1)
    err = rc.rel_err(out, ref) if flag == 0 else float("nan")
    print("%s: %s layer %s p %s ch %s: flag %d, |err| / scale %.3g (bar %.1g)" % (what, c["kind"], c.get("layer"), c["p"], c["ch"], flag, err, bar))
    if c["must_flag"]:
        assert flag == 1, "%s kept its flag at 0 where the unguarded arithmetic is wrong" % what
    if flag == 0:
        assert err <= bar, err
    if c["kind"] == "base":
        assert flag == 0


# ------------------------------------------------------------------------------------------------------------- the decoder
def _dec_ref(c):
    return rc.dec_rows_out(c, rc.chain_fp64(*rc.dec_chain(c)))


def _dec_l1(ops, c, flag):
    """tgp_dec_l1 of an l1 case -> the first conv's activation as planes in accumulator order"""
    P1, P2, rowbias = rc.dec_l1_views(c, d)
    h1 = ops.Planes(c["M"], 512, DEV)
    ops.dec_l1(ops.planes_split(d(c["fine"]), K=c["K"]), ops.heads_planes_w(d(c["Wa"])), P1, d(c["idx1"]), P2, d(c["idx2"]),
               *[d(v) for v in c["vec1"]], rowbias, c["N"], h1, flag)
    return h1


def _dec_fused(ops, c):
    """the case through tgp_dec_fused (behind tgp_dec_l1 for an l1 case) -> (B, N, 3) fp64 on the host, the flag, the operand planes"""
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    h1 = _dec_l1(ops, c, flag) if c["l1"] else ops.planes_split(d(c["H1"]), K=512)
    units = ops.dec_pack(*[d(w) for w in c["Ws"]], h1_permuted=c["l1"])
    out = ops.dec_fused(h1, units, [[d(v) for v in vv] for vv in c["vecs"]], d(c["w5"]), d(c["b5"]), d(c["order"]), c["N"], flag)
    return out.view(c["B"], c["N"], 3).cpu().double(), int(flag.item()), h1


def _dec_tiles(ops, c):
    """the same layers as three tile-kernel launches on planes-only operands (engine.DEC_PLANES_ONLY without engine.DEC_FUSED) and
    tgp_rows_out: the form the fused kernel replaced, which sees every inner activation's magnitude words"""
    M, B, N = c["M"], c["B"], c["N"]
    assert all(ops._routes_to_big_tile(M, n, 1, True) for n in (512, 256, 128))     # (else ops.gemm refuses a planes-only operand)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    xp = ops.planes_split(d(c["H1"]), K=512)
    x = torch.empty(M, 128, device=DEV)
    planes = [ops.Planes(M, 512, DEV), ops.Planes(M, 256, DEV), None]
    for i, (W, (b, sc, sh)) in enumerate(zip(c["Ws"], c["vecs"])):
        W = d(W)
        n, k = W.shape
        ops.gemm(None, W, x if i == 2 else None, M=M, N=n, K=k, lda=0, ldw=k, ldc=n, bias=d(b), scale=d(sc), shift=d(sh), act=1,
                 w_split=ops.split_w(W), a_planes=xp, w_planes=ops.planes_w(W), c_planes=planes[i], range_flag=flag)
        xp = planes[i]
    out = ops.rows_out(x.view(B, N, 128), d(c["w5"]), d(c["b5"]), d(c["order"]))
    return out.cpu().double(), int(flag.item())


DEC_CASES = ([("base", None, None, None)] + [(k, l, None, None) for k in ("big-all", "tiny") for l in (2, 3, 4)]
             + [(k,) + pl for k in ("big-one", "edge-finite") for pl in rc.dec_big_one_placements()])


@pytest.mark.parametrize("kind,layer,p,ch", DEC_CASES)
def test_dec_fused_inner_layers(ops, kind, layer, p, ch):
    """tgp_dec_fused on an operand from planes_split, M = 903: one inner layer out of range, at every place where the kernel's own
    structure changes (which wave, which half of layer 2, converted before or inside the next layer's units).  Layer 4 is the control:
    its activation is consumed in fp32, so the kernel may stay quiet there -- and must then be right."""
    c = rc.dec_case(kind, layer, p, ch)
    out, flag, h1 = _dec_fused(ops, c)
    assert not any(OUT_OF_RANGE(int(a) & 0xffffffff) for a in h1.amax.cpu().tolist())        # the input guard is not what fires
    _contract(c, out, flag, _dec_ref(c), rc.BAR_DEC, "dec_fused")


TILE_CASES = ([("base", None, None, None)] + [(k, l, None, None) for k in ("big-all", "tiny") for l in (2, 3, 4)]
              + [(k,) + pl for k in ("big-one", "edge-finite") for pl in rc.dec_edge_placements()])


@pytest.mark.parametrize("kind,layer,p,ch", TILE_CASES)
def test_tile_chain_on_planes_only_is_the_comparator(ops, kind, layer, p, ch):
    """The tile chain on planes-only operands owes the same contract, and is what the fused kernel replaced: where it raises the flag,
    the fused kernel must too.  B = 7 objects of 301 points: the 128-channel layer reaches the tile kernel from 32 tiles of 64 rows
    on (ops._routes_to_big_tile), so M = 903 cannot run this form."""
    c = rc.dec_case(kind, layer, p, ch, B=7)
    ref = _dec_ref(c)
    out_t, flag_t = _dec_tiles(ops, c)
    _contract(c, out_t, flag_t, ref, rc.BAR_DEC, "tile chain")
    out_f, flag_f, _ = _dec_fused(ops, c)
    _contract(c, out_f, flag_f, ref, rc.BAR_DEC, "dec_fused")
    assert flag_f >= flag_t


DEC_L1_CASES = ([("base", None, None, None, None), ("big-all", 1, None, None, None), ("tiny", 1, None, None, None)]
                + [("big-one", 1, p, ch, None) for p, ch in zip(rc.DEC_POINTS, rc.DEC_CHANNELS[1] * 2)]
                + [("edge-finite", 1, 300, 77, None)]
                + [("big-one",) + pl + (None,) for pl in rc.dec_edge_placements((2, 3))]
                + [("nan-addend", 1, p, ch, (what, value)) for what, p, ch in (("p1", 300, 77), ("rowbias", 898, 470))
                   for value in (float("nan"), float("inf"))])


@pytest.mark.parametrize("kind,layer,p,ch,extra", DEC_L1_CASES)
def test_dec_l1_then_dec_fused(ops, kind, layer, p, ch, extra):
    """tgp_dec_l1 -> tgp_dec_fused (dec_pack(h1_permuted=True)), the engine's default decoder.  dec_l1's own BatchNorm out of range: the
    magnitude word it records for the block must say so (the consumer has nothing else to go by), and the consumer raises the flag.  A
    NaN or an infinity in a gathered addend must not vanish in the ReLU.  big-one at layers 2 / 3: the fused kernel's inner guard on the
    permuted operand."""
    what, value = extra or (None, None)
    c = rc.dec_case(kind, layer, p, ch, l1=True, what=what, value=value)
    out, flag, h1 = _dec_fused(ops, c)
    amax = [int(a) & 0xffffffff for a in h1.amax.cpu().tolist()]
    if layer == 1 and kind in ("big-all", "big-one", "nan-addend"):
        blocks = range(len(amax)) if kind == "big-all" else sorted({int(r) // 32 for r in c["rows"]})
        assert all(OUT_OF_RANGE(amax[b]) for b in blocks), [hex(amax[b]) for b in blocks]
    elif layer != 1:
        assert not any(OUT_OF_RANGE(a) for a in amax)
    if kind == "tiny":
        c["must_flag"] = False          # contract only: the first conv's activation is an operand with magnitude words, not an inner layer
    _contract(c, out, flag, _dec_ref(c), rc.BAR_DEC, "dec_l1 -> dec_fused")


# ------------------------------------------------------------------------------------------------------------- the heads
HEADS_CASES = [(B, N, kind, which) for B, N in rc.HEADS_SHAPES
               for kind, which in (("big-all", None), ("tiny", None), ("big-one", 0), ("big-one", 1), ("edge-finite", 0), ("edge-finite", 1))
               if which is None or which < len(rc.heads_points(B, N))]


@pytest.mark.parametrize("B,N,kind,which", HEADS_CASES)
def test_heads_fused_conv1_activation(ops, B, N, kind, which):
    """tgp_heads_fused with the conv1 BatchNorm of ONE head out of range and the features and coarse products in range: in a plain
    wave and in a wave that straddles two objects (the kernel's two epilogue paths).  A flagged wave writes no keys: the head's maxima
    are those of the other waves' points; the other heads and conv_5 (tgp_conv_max_fused on the same operands) are untouched."""
    p = None if which is None else rc.heads_points(B, N)[which]
    c = rc.heads_case(kind, B, N, hd=1, p=p, ch=None if which is None else 333 + 300 * which)
    hd, heads = c["hd"], c["heads"]
    operands = rc.heads_operands(c)
    dev_ops = [d(t) if torch.is_tensor(t) else t for t in operands]
    got5, got2, over5, over = run_fused_kernels(ops, *dev_ops, B, N)
    c5, y = fused_kernels_fp64(*operands, N, range(B))
    assert over5 == 0 and (got5 - c5).abs().max().item() <= 3e-6 * c5.abs().max().item()
    print("heads_fused: %s p %s: over %d" % (kind, p, over))
    if kind in ("big-all", "big-one"):
        assert over == 1
        for o in range(heads):
            if o != hd:
                assert (got2[o] - y[o]).abs().max().item() <= rc.BAR_HEADS * y[o].abs().max().item(), o
        keys2, _ = ops.heads_fused(dev_ops[0], c["K"], ops.heads_planes_w(dev_ops[2][1024:]), dev_ops[3][:, 1024:], dev_ops[4], dev_ops[5][:, 1024:],
                                   dev_ops[6], ops.heads_pack_w2(dev_ops[10], dev_ops[7][1024:], dev_ops[8][1024:], dev_ops[9][1024:]),
                                   dev_ops[11], dev_ops[12], dev_ops[13], B, N)
        if kind == "big-all":
            assert int(keys2[hd].abs().max().item()) == 0                  # every wave of the head flagged: no key written
        else:
            # the flagged wave's 32 points are missing from the maxima of the objects it touches, everybody else's are there
            yp = rc.chain_fp64(*rc.heads_chain(c, hd)[:2])
            keep = torch.ones(c["M"], dtype=torch.bool)
            keep[p // 32 * 32: p // 32 * 32 + 32] = False
            yp = torch.relu(yp).masked_fill(~keep.view(-1, 1), float("-inf")).view(B, N, 256).max(1)[0]
            assert (got2[hd] - yp).abs().max().item() <= rc.BAR_HEADS * yp.abs().max().item()
    elif over == 0:
        for o in range(heads):
            err = (got2[o] - y[o]).abs().max().item() / y[o].abs().max().item()
            print("  head %d: |err| / scale %.3g (bar %.1g)" % (o, err, rc.BAR_HEADS))
            assert err <= rc.BAR_HEADS, (o, err)
    else:
        assert over == 1


# ------------------------------------------------------------------------------------------------------------- tgp_hs_chain
@pytest.mark.parametrize("kind", ["base", "big-one", "edge-finite"])
def test_hs_chain_intermediate(ops, kind):
    """tgp_hs_chain with one value of its intermediate (the first layer's result, which it splits for the second) beyond fp16's range,
    in a row of the partial last tile"""
    c = rc.hs_case(kind, p=None if kind == "base" else 1026, ch=None if kind == "base" else 100)
    M, n = c["M"], c["n"]
    units = ops.hs_chain_pack(d(c["W1"]), d(c["W2"]))
    assert units is not None
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    c1 = torch.empty(M, c["N1"], device=DEV)
    c2 = ops.hs_chain(ops.planes_split(d(c["A"]), K=c["K1"]), units, c1, d(c["b2"]), flag, rowbias=d(c["rowbias"]), rows_per_obj=n,
                      res1=d(c["res1"]), scale1=d(c["scale1"]), shift1=d(c["shift1"]), relu=True)
    x, layers, _ = rc.hs_chain_layers(c)
    _contract(c, c2.cpu().double(), int(flag.item()), rc.chain_fp64(x, layers), 2 * rc.BAR_HS, "hs_chain")
    if int(flag.item()) == 0:
        ref1 = rc.chain_fp64(x, layers[:1])
        assert rc.rel_err(c1.cpu().double(), ref1) <= rc.BAR_HS


# ------------------------------------------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("scale", [1e6, 1e-5])
@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("bn", ["conv1d_block.4", "conv1d_block.7", "recon_head.1"])
def test_decoder_chain_on_planes_only_inner_layers(ops, monkeypatch, bn, fused, scale):
    """tests/test_gpu_parity.py::test_decoder_chain_on_planes_only with the scale on the BatchNorm of an INNER decoder layer (512 -> 512,
    512 -> 256, 256 -> 128) instead of the first: in every form of the planes-only chain the reconstruction is finite and, whenever the
    chain's flag was raised (the predicated fp32 chain ran), the bits of the forward without planes; where it was not (the layer's
    activation is still a faithful operand, or is never split), within that test's 2e-6 of the output's scale."""
    from tgpose_amd import PoseNet9D, seeded_state_dict, FLAGS, engine
    sd = seeded_state_dict(16)
    for k in ("weight", "bias"):
        sd["face_all.decoder." + bn + "." + k] = sd["face_all.decoder." + bn + "." + k] * scale
    net = PoseNet9D()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    FLAGS.train = 0
    B, N = 3, 1028
    pts, obj = synth_points(B, N, 45)
    torch.manual_seed(10)
    i1 = torch.randperm(N)[: N // 4]
    smp = (i1, torch.randperm(N // 4)[: N // 16])
    pk = net.packed(DEV)
    assert pk.dec_units is not None
    arenas = []

    class Arena(engine.Arena):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            arenas.append(self)
    monkeypatch.setattr(engine, "Arena", Arena)
    got = []
    for planes, only in ((True, True), (False, False)):
        old = ops.PLANES, engine.DEC_PLANES_ONLY, engine.DEC_FUSED, engine.DEC_L1
        ops.PLANES, engine.DEC_PLANES_ONLY, engine.DEC_FUSED, engine.DEC_L1 = planes, only, fused > 0, fused > 1
        try:
            probe = {}
            with torch.no_grad():
                engine.posenet_forward(pk, pts.to(DEV), obj.to(DEV), False, sample_idx=smp, probe=probe)
            got.append(probe["recon"].clone())
        finally:
            ops.PLANES, engine.DEC_PLANES_ONLY, engine.DEC_FUSED, engine.DEC_L1 = old
    flag = int(arenas[0].dec_flag.item())
    assert torch.isfinite(got[0]).all()
    mean = pts.to(DEV).mean(1, keepdim=True)
    err = (got[0] - got[1]).abs().max().item()
    print("%s x %g, fused %d: flag %d, |planes - without| %.3g (scale %.3g)" % (bn, scale, fused, flag, err, (got[1] - mean).abs().max().item()))
    if flag:
        assert torch.equal(got[0], got[1])
    else:
        assert err <= 2e-6 * max(1.0, (got[1] - mean).abs().max().item()), err
