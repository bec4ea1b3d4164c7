"""Cases for the fused kernels' fp16 range guards at their INNER layers (tests/test_range_guard_cpu.py, tests/test_range_guard_gpu.py).

The forward's hot kernels emulate fp32 with a two-term fp16 operand split (hi = fp16(v), lo = fp16(v - hi)), faithful only while a
32-row operand block lies in [2^-4, 65504) (TGP_FP16_OUT_OF_RANGE, csrc/mfma_unit.h).  The fused kernels keep their inner activations
in registers, so no magnitude word of those exists for a consumer to look at.  The contract they owe their callers all the same:

    the range flag stays 0  =>  every live row of the output lies within the bar of an fp64 restatement;  otherwise the flag is 1.

Every case here starts from in-range base operands and changes BatchNorm scale / shift entries or weights only, so that ONE inner
layer leaves the range while the operand the kernel reads (and its magnitude words) stays inside it: the input-side guard cannot be what
fires.  The layers are numbered as csrc/dec_fused.hip numbers them: 1 = the decoder's first conv (fine -> 512, tgp_dec_l1), 2 =
512 -> 512, 3 = 512 -> 256, 4 = 256 -> 128 (its activation is consumed in fp32 by the last conv: never split), then conv 128 -> 3.

  chain_fp64          the fp64 restatement relu(bn(conv)) x L -> conv
  chain_split_model   a CPU model of the UNGUARDED arithmetic: what a kernel computes that splits whatever it is given
  dec_case / heads_case / hs_case     the operands of a case, on the CPU
"""
import functools

import torch

FP16_MAX = 65504.0            # the range rule's upper end (0x477fe000): at and above it a block is out of range
FP16_INF = 65520.0            # the smallest magnitude fp16 rounds to infinity
FP16_MIN = 2.0 ** -4          # the range rule's lower end (0x3d800000)
BAR_DEC = 1e-5                # tests/test_gpu_parity.py::test_dec_fused_vs_fp64_and_partial_tiles: of the output's scale, the whole chain
BAR_HEADS = 6e-6              # ...::test_fused_kernels_vs_fp64: two layers
BAR_HS = 3e-6                 # per layer of tgp_hs_chain (the split GEMM's bar)

# big-one placements.  Points (M = 903 = 3 objects of 301): the first wave of tile 0; a wave that straddles two objects (rows 288-319,
# object boundary at 301); the partial last 32-row block (rows 896-902); the last live row.
DEC_POINTS = (5, 300, 898, 902)
# Channels.  Layer 2 is produced in two halves of 256 channels = 8 blocks of 32: blocks 0 / 1 of a half are converted before layer 3
# starts, blocks 2-7 inside layer 3's MFMA gaps.  Layer 3: blocks 0-3 before layer 4 starts, 4-7 inside its first unit.
DEC_CHANNELS = {1: (77, 470), 2: (40, 200, 300, 500), 3: (70, 200), 4: (77,)}


# ------------------------------------------------------------------------------------------------------------- arithmetic
def chain_fp64(x, layers, last=None, acts=None):
    """relu(bn(conv(x))) for every layer, then the plain conv `last` = (W, b): the fp64 restatement the operator tests hold the
    kernels against.  A layer is a dict: W (C, K), bias (C) or None, addends (a list of (M, C) row terms added before the BatchNorm
    fold, in the kernels' order), scale / shift (C) or None, act (ReLU unless False).  acts (a list) receives each layer's value
    BEFORE its ReLU."""
    h = x.double()
    for L in layers:
        v = h @ L["W"].double().t()
        if L.get("bias") is not None:
            v = v + L["bias"].double()
        for a in L.get("addends", ()):
            v = v + a.double()
        if L.get("scale") is not None:
            v = v * L["scale"].double() + L["shift"].double()
        if acts is not None:
            acts.append(v)
        h = torch.relu(v) if L.get("act", True) else v
    if last is not None:
        h = h @ last[0].double().t() + last[1].double()
    return h


def _split(v):
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    return hi.float(), lo.float()


def chain_split_model(x, layers, last=None):
    """The chain as a kernel WITHOUT a range guard computes it: every operand (the input, each layer's activation, the weights) is
    split into fp16 hi / lo, the three products hi hi + hi lo + lo hi are accumulated in fp32, the epilogue runs in fp32, ReLU is
    fmax(v, -0) -- which turns a NaN into -0, as v_max_f32 does -- and the last conv reads the last activation in fp32 (as the fused
    decoder kernel and tgp_rows_out do).  A model: torch's fp32 matmul adds in another order than the MFMA units, so not bit-exact."""
    h = x.float()
    for L in layers:
        hh, hl = _split(h)
        wh, wl = _split(L["W"].float())
        v = hl @ wh.t() + hh @ wl.t() + hh @ wh.t()
        if L.get("bias") is not None:
            v = v + L["bias"].float()
        for a in L.get("addends", ()):
            v = v + a.float()
        if L.get("scale") is not None:
            v = v * L["scale"].float() + L["shift"].float()
        h = torch.fmax(v, torch.tensor(-0.0)) if L.get("act", True) else v
    if last is not None:
        h = h @ last[0].float().t() + last[1].float()
    return h


def rel_err(got, ref, rows=None):
    """largest |got - ref| over `rows` (all rows when None) in units of the reference's scale (its largest finite magnitude); a
    difference that is not finite counts as infinite"""
    fin = torch.isfinite(ref)
    scale = ref[fin].abs().max().item() if fin.any() else 1.0
    d = (got.double() - ref).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    if rows is not None:
        d = d[rows]
    return d.max().item() / scale


def block_amax(x, rows=32):
    """max |x| per block of 32 rows: what a producer records as the block's magnitude word"""
    M = x.shape[0]
    pad = (-M) % rows
    a = torch.cat([x.abs().float(), torch.zeros(pad, x.shape[1])]).view(-1, rows * x.shape[1])
    return a.max(1)[0]


def in_range(amax):
    """the range rule over magnitude words given as floats"""
    return bool(((amax < FP16_MAX) & ((amax >= FP16_MIN) | (amax == 0))).all()) and bool(torch.isfinite(amax).all())


def _aim(a, layer, p, c, target):
    """Point p, channel c of `layer` (its W / bias / addends / scale / shift are edited in place) gets the value `target` before the
    ReLU and is the channel's largest by a wide margin: the channel's weight row is pointed along what distinguishes point p's input
    `a[p]` from the mean input, then scale[c] / shift[c] map the largest pre-activation to `target` and the second largest to
    target - 20000 (so big-one's other points stay below 50000 < 60000)."""
    a = a.double()
    d = a[p] - a.mean(0)
    layer["W"][c] = (4.0 * d / d.norm()).float()
    u = a @ layer["W"][c].double()
    if layer.get("bias") is not None:
        u = u + layer["bias"][c].double()
    for t in layer.get("addends", ()):
        u = u + t[:, c].double()
    top = torch.topk(u, 2)
    assert int(top.indices[0]) == p, "point %d is not the largest of channel %d" % (p, c)
    s = 20000.0 / (top.values[0] - top.values[1]).item()
    layer["scale"][c] = s
    layer["shift"][c] = target - float(torch.tensor(s, dtype=torch.float32).double() * top.values[0])


# ------------------------------------------------------------------------------------------------------------- the decoder
@functools.lru_cache(maxsize=None)
def _dec_base(B, l1):
    """in-range operands of tgp_dec_fused (and of tgp_dec_l1 in front of it): tests/test_gpu_parity.py's operator-test operands"""
    gen = torch.Generator().manual_seed(9 + B + (100 if l1 else 0))
    N = 301
    M = B * N
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    c = dict(B=B, N=N, M=M, l1=l1)
    if l1:
        K = 268
        fine = rn(M, 272)
        fine[:, K:] = float("nan")                                 # the padding columns are not the caller's to define
        Wa = rn(512, 272) / K ** 0.5
        Wa[:, K:] = 0
        n1, n2 = M // 4, M // 16
        # the coarse products and the per-object bias are columns of wider rows (dec_l1_views), as in the engine
        c.update(K=K, fine=fine, Wa=Wa, P1w=rn(n1, 640), P2w=rn(n2, 640), idx1=torch.randint(0, n1, (M,), generator=gen, dtype=torch.int32),
                 idx2=torch.randint(0, n2, (M,), generator=gen, dtype=torch.int32), rbw=rn(B, 516) * 0.3,
                 vec1=[rn(512) * 0.1, ru(512) + 0.5, rn(512) * 0.1])
    else:
        c["H1"] = torch.relu(rn(M, 512))
    c["Ws"] = [rn(n, k) / k ** 0.5 for n, k in ((512, 512), (256, 512), (128, 256))]
    c["vecs"] = [[rn(n) * 0.1, ru(n) + 0.5, rn(n) * 0.1] for n in (512, 256, 128)]
    c["w5"], c["b5"] = rn(3, 128) / 11.0, rn(3)
    c["order"] = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)])
    return c


def _clone(c):
    out = {}
    for k, v in c.items():
        if torch.is_tensor(v):
            out[k] = v.clone()
        elif isinstance(v, list):
            out[k] = [[t.clone() for t in e] if isinstance(e, list) else e.clone() for e in v]
        else:
            out[k] = v
    return out


def dec_l1_views(c, to=lambda t: t):
    """P1, P2 (row stride 640) and the per-object bias (row stride 516) of an l1 case; `to` moves the wide tensors first"""
    return to(c["P1w"])[:, 128:], to(c["P2w"])[:, 128:], to(c["rbw"])[:, :512]


def dec_chain(c):
    """(x, layers, last) of a decoder case for chain_fp64 / chain_split_model; the layers hold the case's own tensors (edits show)"""
    layers = []
    if c["l1"]:
        obj = torch.arange(c["M"]) // c["N"]
        P1, P2, rowbias = dec_l1_views(c)
        layers.append(dict(W=c["Wa"][:, :c["K"]], bias=c["vec1"][0], scale=c["vec1"][1], shift=c["vec1"][2],
                           addends=[P1[c["idx1"].long()], P2[c["idx2"].long()], rowbias[obj]]))
        x = c["fine"][:, :c["K"]]
    else:
        x = c["H1"]
    for W, (b, sc, sh) in zip(c["Ws"], c["vecs"]):
        layers.append(dict(W=W, bias=b, scale=sc, shift=sh))
    return x, layers, (c["w5"], c["b5"])


def dec_layer_index(c, layer):
    """index of dec_fused.hip's layer number in dec_chain's list"""
    return layer - 1 if c["l1"] else layer - 2


def dec_operand(c):
    """the operand whose magnitude words the case's FIRST kernel checks on its input side"""
    return c["fine"][:, :c["K"]] if c["l1"] else c["H1"]


def dec_rows_out(c, y):
    """(M, 3) rows in sorted order -> (B, N, 3) in point order, through the case's permutation (tgp_rows_out's `map`)"""
    B, N = c["B"], c["N"]
    y = y.view(B, N, 3)
    return torch.empty_like(y).scatter_(1, c["order"].unsqueeze(-1).expand(-1, -1, 3), y)


def dec_case(kind, layer=None, p=None, ch=None, l1=False, B=3, what=None, value=None):
    """A decoder case.  kind: base | big-all | big-one | edge-finite | tiny | nan-addend (l1 only; what = "p1" / "rowbias", value = the
    non-finite entry).  -> the operands, plus: layer, rows (the affected rows, sorted order; None = all), must_flag (an unguarded kernel
    is wrong there -- tests/test_range_guard_cpu.py proves it --, so the flag has to be 1), split (is the layer's activation ever split
    into fp16? layer 4's is not)."""
    c = _clone(_dec_base(B, l1))
    c.update(kind=kind, layer=layer, p=p, ch=ch, rows=None, split=layer is None or layer < 4)
    c["must_flag"] = kind in ("big-all", "big-one", "tiny", "nan-addend") and c["split"]
    if kind == "base":
        c["must_flag"] = False
        return c
    if kind == "nan-addend":
        c["layer"], c["split"], c["must_flag"] = 1, True, True
        P1, _, rowbias = dec_l1_views(c)
        if what == "p1":                                            # the entry point p gathers (and whoever else gathers that row)
            P1[c["idx1"][p].long(), ch] = value
            c["rows"] = torch.nonzero(c["idx1"] == c["idx1"][p]).view(-1)
        else:                                                       # the entry of point p's object
            rowbias[p // c["N"], ch] = value
            c["rows"] = torch.arange(p // c["N"] * c["N"], (p // c["N"] + 1) * c["N"])
        return c
    x, layers, last = dec_chain(c)
    li = dec_layer_index(c, layer)
    L = layers[li]
    if kind == "big-all":
        L["scale"] *= 2.0 ** 20
    elif kind == "tiny":
        # exact powers of two: the fp64 result is the base case's, bit for bit
        L["scale"] *= 2.0 ** -16
        L["shift"] *= 2.0 ** -16
        (layers[li + 1]["W"] if li + 1 < len(layers) else last[0]).mul_(2.0 ** 16)
    elif kind in ("big-one", "edge-finite"):
        acts = []
        chain_fp64(x, layers[:li], acts=acts)
        a = torch.relu(acts[-1]) if li else x.double()
        _aim(a, L, p, ch, 70000.0 if kind == "big-one" else 65510.0)
        c["rows"] = torch.tensor([p])
    else:
        raise ValueError(kind)
    return c


def dec_big_one_placements(layers=(2, 3, 4)):
    return [(layer, p, ch) for layer in layers for p in DEC_POINTS for ch in DEC_CHANNELS[layer]]


def dec_edge_placements(layers=(2, 3, 4)):
    """one point per (layer, channel), walking through DEC_POINTS"""
    out = []
    for layer in layers:
        for ch in DEC_CHANNELS[layer]:
            out.append((layer, DEC_POINTS[len(out) % len(DEC_POINTS)], ch))
    return out


# ------------------------------------------------------------------------------------------------------------- the heads
HEADS_SHAPES = ((2, 160), (3, 301))


@functools.lru_cache(maxsize=None)
def _heads_base(B, N):
    """tests/test_gpu_parity.py::test_fused_kernels_vs_fp64's operands: K = 268 of 272 columns, garbage in the padding"""
    gen = torch.Generator().manual_seed(B * 1000 + N)
    M, K, heads = B * N, 268, 3
    fine = torch.randn(M, 272, generator=gen)
    fine[:, K:] = float("nan")
    fine[:, :K][:, ::9] *= 30.0
    Wa = torch.randn((heads + 1) * 1024, 272, generator=gen) / K ** 0.5
    Wa[:, K:] = 0
    n1, n2 = max(M // 4, 1), max(M // 16, 1)
    P1, P2 = torch.randn(n1, 4096, generator=gen), torch.randn(n2, 4096, generator=gen)
    idx1 = torch.randint(0, n1, (M,), generator=gen, dtype=torch.int32)
    idx2 = torch.randint(0, n2, (M,), generator=gen, dtype=torch.int32)
    bias, scale, shift = (torch.randn(4096, generator=gen) * 0.1, torch.rand(4096, generator=gen) + 0.5, torch.randn(4096, generator=gen) * 0.1)
    W2 = torch.randn(heads, 256, 1024, generator=gen) / 32.0
    b2, sc2, sh2 = (torch.randn(heads, 256, generator=gen) * 0.1, torch.rand(heads, 256, generator=gen) + 0.5, torch.randn(heads, 256, generator=gen) * 0.1)
    return dict(B=B, N=N, M=M, K=K, heads=heads, fine=fine, Wa=Wa, P1=P1, idx1=idx1, P2=P2, idx2=idx2, bias=bias, scale=scale, shift=shift,
                W2=W2, b2=b2, sc2=sc2, sh2=sh2)


def heads_operands(c):
    """the positional operands of tests.util.run_fused_kernels / fused_kernels_fp64"""
    return [c[k] for k in ("fine", "K", "Wa", "P1", "idx1", "P2", "idx2", "bias", "scale", "shift", "W2", "b2", "sc2", "sh2")]


def heads_chain(c, hd):
    """(x, layers, None) of head hd, per point (before the max over an object's points)"""
    lo, hi = 1024 * (hd + 1), 1024 * (hd + 2)
    l1 = dict(W=c["Wa"][lo:hi, :c["K"]], bias=c["bias"][lo:hi], scale=c["scale"][lo:hi], shift=c["shift"][lo:hi],
              addends=[c["P1"][c["idx1"].long(), lo:hi], c["P2"][c["idx2"].long(), lo:hi]])
    l2 = dict(W=c["W2"][hd], bias=c["b2"][hd], scale=c["sc2"][hd], shift=c["sh2"][hd])
    return c["fine"][:, :c["K"]], [l1, l2], None


def heads_points(B, N):
    """a point in a plain wave (32 live points of one object) and, where N % 32 != 0, one in the wave that holds object 0's last
    points and object 1's first (the kernel's other epilogue path)"""
    return (40, N // 32 * 32 + 3) if N % 32 and B > 1 else (40,)


def heads_case(kind, B, N, hd=1, p=None, ch=None):
    """A case on the conv1 BatchNorm of head hd; the views heads_chain returns alias the case's tensors, so edits through them show"""
    c = _clone(_heads_base(B, N))
    c.update(kind=kind, hd=hd, p=p, ch=ch, rows=None, must_flag=kind in ("big-all", "big-one", "tiny"))
    if kind == "base":
        return c
    x, (l1, l2), _ = heads_chain(c, hd)
    if kind == "big-all":
        l1["scale"] *= 2.0 ** 20
    elif kind == "tiny":
        l1["scale"] *= 2.0 ** -16
        l1["shift"] *= 2.0 ** -16
        l2["W"].mul_(2.0 ** 16)
    elif kind in ("big-one", "edge-finite"):
        _aim(x, l1, p, ch, 70000.0 if kind == "big-one" else 65510.0)
        c["rows"] = torch.tensor([p])
    else:
        raise ValueError(kind)
    return c


# ------------------------------------------------------------------------------------------------------------- tgp_hs_chain
HS_SHAPE = (4, 257, 256, 256, 2304)       # the smallest (B, n, K1, N1, N2) of test_hs_chain_bit_identical_to_two_tile_launches: M = 1028


@functools.lru_cache(maxsize=None)
def _hs_base():
    B, n, K1, N1, N2 = HS_SHAPE
    gen = torch.Generator().manual_seed(B * 7 + n + K1)
    M = B * n
    rn = lambda *s: torch.randn(*s, generator=gen)
    return dict(B=B, n=n, M=M, K1=K1, N1=N1, N2=N2, A=rn(M, K1), W1=rn(N1, K1) / K1 ** 0.5, W2=rn(N2, N1) / N1 ** 0.5, rowbias=rn(B, N1),
                b2=rn(N2), res1=rn(M, N1), scale1=torch.rand(N1, generator=gen) + 0.5, shift1=rn(N1))


def hs_chain_layers(c):
    obj = torch.arange(c["M"]) // c["n"]
    return c["A"], [dict(W=c["W1"], bias=None, addends=[c["rowbias"][obj], c["res1"]], scale=c["scale1"], shift=c["shift1"]),
                    dict(W=c["W2"], bias=c["b2"], act=False)], None


def hs_case(kind, p=None, ch=None):
    """base | big-one | edge-finite on the first layer's result (the intermediate the kernel splits for its second layer)"""
    c = _clone(_hs_base())
    c.update(kind=kind, p=p, ch=ch, rows=None, must_flag=kind == "big-one")
    if kind != "base":
        x, layers, _ = hs_chain_layers(c)
        _aim(x, layers[0], p, ch, 70000.0 if kind == "big-one" else 65510.0)
        c["rows"] = torch.tensor([p])
    return c
