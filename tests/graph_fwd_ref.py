"""fp64 reference of the graph layers' FORWARD kernels (csrc/gconv.hip) and the rules by which their launches pick a kernel form
(TEST INFRASTRUCTURE), plain torch on the CPU.  It stands on tests/graph_bwd_ref.py: `_setup`, `forward_terms`, `bound`, `mismatch`,
the graph families and `Case` are that module's, used and not restated.

    hs_terms            HS_layer.graph_conv / HSlayer_surface.graph_conv, value and a bound that holds at EVERY element
    orl_terms           ORL pooling g = mean_i max_j feat[idx_ij] and its projection rb = g @ W2^T
    pool_ref            Pool_layer: neighbour max at the sampled rows, the sampled points         (exact: torch.equal)
    gather_ref          dst[b, i] = src[b, idx[b, i]]                                             (exact: torch.equal)
    normalize_dirs_ref  F.normalize(directions, dim=0, eps=1e-12)

The graph convolution's bound.  graph_bwd_ref.forward_terms takes abs_terms at the fp64 winner; fp32 may legitimately pick another
slot where two candidates are closer than its arithmetic resolves, so that bound needs the `ambiguous` mask beside it.  Here no
element is excluded: the maximum is 1-Lipschitz in the largest candidate error, |max_j a_j - max_j b_j| <= max_j |a_j - b_j|, and
candidate j's error is relative to |dir_j| . |D_s| |support_j| (surface: |dir_j| . |D_s|).  So per (point, support, channel) the
LARGEST candidate term over the k slots stands for the support's maximum, whichever slot either side picked:

    abs_terms = |centre| + sum_s max_j (sum_a |dir_ja D_sa|) |support_js| / 7,     chain = 7,
    |got - want| <= (12 + 7) * 2^-24 * abs_terms + 1e-30                            (graph_bwd_ref.bound: the project's bar)

It is never below forward_terms' (the winner is one of the candidates; tests/test_graph_fwd_cpu.py asserts it).

ORL's bound.  The neighbour maxima are exact selections; only the mean rounds.  Both pooling kernels add in ONE fixed order
(orl_lds_kernel reproduces orl_partial_kernel's, its comment says so and the partials are bit-identical): wave slot w of a 64-point
tile adds the maxima of points w, w + 4, .. -- at most 16 of them, into a zero -- then ((s0 + s1) + s2) + s3 joins the four slots (3
additions), orl_finish_kernel / orl_finish_project_kernel / the fused finish add the ceil(n / 64) tile sums in tile order into a
zero, and one division by n follows.  The longest path a value travels:

    chain(n) = 16 + 3 + ceil(n / 64) + 1,      abs_terms = sum_i |max_j ..| / n,
    |g - want| <= (2 + chain) * 2^-24 * abs_terms + 1e-30

(two additions into an exact zero round nothing, so the path is two shorter than counted; the 2 in front covers the second-order
terms of (1 + u)^chain).  rb[b, o] = sum_c g[b, c] w2t[c, o]: abs_terms = sum_c |g_c| |w_co| and chain = chain(n) + C, the g entries'
own error and a C-term sum in any order -- orl_finish_project_kernel's four fmaf chains of C / 4 joined in order, the fused form's
C / 16 chains of 16 joined in chunk order, or whatever a later rewrite picks: one bar for all.

Launch forms (gconv_form, orl_form) restate csrc/gconv.hip's gconv_lds_launch and orl_lds_launch.  What can be seen from outside is
tied to them by tests/test_graph_fwd_gpu.py: tgp_gconv_hs_fwd_dirs answers TGP_EUNSUPPORTED exactly where gconv_form is 0, and
ops.orl_rowbias(planes=P) hands P back exactly where orl_form(planes=True) says "lds".  NOT observable from outside: which of the
16- and 8-channel slices the LDS graph convolution took, whether its launch went through the opt-in LDS attribute, whether ORL's
neighbour lists went to LDS as 16-bit ids, and the workgroup size.  The tests run both sides of each of those switches and judge
the results; a changed rule moves the switch away from the tested shapes without failing anything, which is why
tests/test_graph_fwd_cpu.py recomputes every boundary from the byte formulas and pins the numbers.
"""
import torch
import torch.nn.functional as F

from tests import graph_bwd_ref as R
from tests.graph_bwd_ref import S, U, Term, case, case_id  # noqa: F401  (re-exported for the tests)

KIB = 1024
LDS_TWO_PER_CU = 72 * KIB            # a table that leaves room for two workgroups per CU
LDS_OPT_IN = 64 * KIB                # above this the launch needs the opt-in attribute
LDS_MAX = 150 * KIB                  # what the opt-in asks for
ORL_PTS, ORL_CH = 64, 16
BUDGET = 300e6                       # bytes of float64 a reference may hold at once


# ------------------------------------------------------------------------------------------------------------------ launch forms
def gconv_lds_bytes(n, ch):
    """the LDS table of gconv_lds_kernel<ch>: [n][7][ch] floats"""
    return n * S * ch * 4


def gconv_form(n, C):
    """the channel slice tgp_gconv_hs_fwd stages in LDS: 16, 8, or 0 = the wave-per-point gather kernel (release builds never take
    the 4-channel slice)"""
    for ch in (16, 8):
        if gconv_lds_bytes(n, ch) <= LDS_TWO_PER_CU and C % ch == 0:
            return ch
    return 0


def gconv_opt_in(n, C):
    """the LDS launch asks for more than 64 KiB"""
    ch = gconv_form(n, C)
    return bool(ch) and gconv_lds_bytes(n, ch) > LDS_OPT_IN


def orl_lds_bytes(n, planes):
    """orl_lds_kernel's table [n][16], its per-slot sums [ceil(n / 64)][4][16] and, with planes, n / 32 + 4 magnitude words"""
    ptiles = -(-n // ORL_PTS)
    return 4 * (n * ORL_CH + ptiles * 4 * ORL_CH + ((n // 32 + 4) if planes else 0))


def orl_form(n, k, C, planes=False, aligned=True):
    """-> ("lds" | "gather", neighbour lists in LDS, threads per workgroup).  planes: the budget counts the magnitude words -- the
    planes entry point AND the one-launch form (which counts them with or without planes); aligned: the list pointer is 16-byte
    aligned.  "gather" under planes means the entry point answers TGP_EUNSUPPORTED and the caller falls back."""
    lds = orl_lds_bytes(n, planes)
    if lds > LDS_TWO_PER_CU or C % ORL_CH:
        return ("gather", False, 256)
    lists = n <= 65535 and (n * k) % 4 == 0 and aligned and lds + 2 * n * k <= LDS_MAX
    slots = -(-n // ORL_PTS) * 4 * (ORL_CH // 2)
    return ("lds", lists, 1024 if slots >= 768 else 512 if slots >= 384 else 256)


def orl_chain(n):
    """the longest addition path of g (module docstring)"""
    return 16 + 3 + -(-n // ORL_PTS) + 1


# ------------------------------------------------------------------------------------------------------------------ graph convolution
def _hs_chunks(xyz, idx, proj, sdn, C, surface):
    """the shared setup in slices of points that keep about eight (B, m, k, 7, C) float64 arrays under BUDGET"""
    B, n, k = idx.shape
    m = max(1, int(BUDGET // (8 * 8 * B * k * S * C)))
    for i0 in range(0, n, m):
        yield R._setup(xyz, idx, proj, sdn, C, surface, rows=slice(i0, min(n, i0 + m)))


def _hs_chunk_terms(p, C, surface):
    t = R.forward_terms(None, None, None, None, C, surface, pre=p)
    cand = p["absth"] if surface else p["absth"] * p["sup"].abs()
    ab = cand.amax(2).sum(2) / 7.0
    if not surface:
        ab = ab + p["proj"][..., :C].abs()
    return Term(t.value, ab, t.chain)


def hs_terms(xyz, idx, proj, sdn, C, surface=False):
    """the fp64 forward (B, n, C) with the every-element bound of the module docstring"""
    parts = [_hs_chunk_terms(p, C, surface) for p in _hs_chunks(xyz, idx, proj, sdn, C, surface)]
    return Term(*(torch.cat([t[i] for t in parts], 1) for i in range(3)))


def _strict_wins(val, need, k):
    """val (.., k, ..) candidates along dim 2, need broadcastable to val without dim 2 -> per slot, how many entries it wins by at
    least `need` over the runner-up"""
    best, jw = val.max(2, keepdim=True)
    second = val.masked_fill(torch.zeros_like(val, dtype=torch.bool).scatter_(2, jw, True), float("-inf")).amax(2)
    ok = (best.squeeze(2) - second) >= need
    return torch.bincount(jw.squeeze(2)[ok].reshape(-1), minlength=k).double()


def hs_slot_shares(xyz, idx, proj, sdn, C):
    """per slot j: the share of the (point, support, channel) entries whose maximum is slot j's alone, by at least 100 times the
    bar of the output element the entry is added into"""
    k = idx.shape[2]
    wins, total = torch.zeros(k, dtype=torch.float64), 0
    for p in _hs_chunks(xyz, idx, proj, sdn, C, False):
        need = 100.0 * R.bound(_hs_chunk_terms(p, C, False), 7).unsqueeze(2)            # (B, m, 1, C) over the supports
        wins += _strict_wins(p["val"], need, k)
        total += p["val"].numel() // k
    return wins / total


# ------------------------------------------------------------------------------------------------------------------ ORL, pool, gathers
def _rows_of(t, idx):
    """t (B, n, C), idx (B, m) -> (B, m, C)"""
    return t[torch.arange(t.shape[0]).view(-1, 1), idx]


def _nbr_max(feat, idx):
    """max_j feat[b, idx[b, i, j]] slot by slot: nothing of size k is held"""
    m = _rows_of(feat, idx[:, :, 0])
    for j in range(1, idx.shape[2]):
        m = torch.maximum(m, _rows_of(feat, idx[:, :, j]))
    return m


def orl_terms(feat, idx, w2t=None):
    """g (B, C) as a Term; with w2t (C, C) = W2^T: (g, rb) with rb = g @ w2t (B, C) a Term too.  Compare with orl_bound."""
    feat, idx = R._up(feat), idx.detach().cpu().long()
    n = feat.shape[1]
    m = _nbr_max(feat, idx)
    g = Term(m.sum(1) / n, m.abs().sum(1) / n, torch.full(m.shape[::2], float(orl_chain(n)), dtype=torch.float64))
    if w2t is None:
        return g
    w = R._up(w2t)
    return g, Term(g.value @ w, g.value.abs() @ w.abs(), g.chain + float(w.shape[0]))


def orl_bound(term):
    return (2.0 + term.chain) * U * term.abs_terms + 1e-30


def orl_mismatch(got, term):
    """-> (bool tensor of the elements outside orl_bound, the largest |error| / bound)"""
    got = got.detach().cpu().double().reshape(term.value.shape)
    err, bd = (got - term.value).abs(), orl_bound(term)
    return ~(err <= bd), float((err / bd).max())


def orl_slot_shares(feat, idx):
    """per slot j: the share of the (point, channel) entries whose maximum is slot j's alone, by at least 100 times g's bar"""
    feat, idx = R._up(feat), idx.detach().cpu().long()
    B, n, k = idx.shape
    need = 100.0 * orl_bound(orl_terms(feat, idx)).view(B, 1, -1)
    step = max(1, int(BUDGET // (4 * 8 * B * k * feat.shape[2])))
    wins = torch.zeros(k, dtype=torch.float64)
    for i0 in range(0, n, step):
        part = idx[:, i0:i0 + step]
        vals = feat[torch.arange(B).view(B, 1, 1), part]                                # (B, m, k, C)
        wins += _strict_wins(vals, need, k)
    return wins / (B * n * feat.shape[2])


def pool_ref(xyz, feat, idx, sample, kpool):
    """-> (xyz[:, sample], max_{j < kpool} feat[b, idx[b, sample, j]]) in the operands' own type: selections, no rounding"""
    sample, idx = sample.detach().cpu().long(), idx.detach().cpu().long()
    return xyz.detach().cpu()[:, sample], _nbr_max(feat.detach().cpu(), idx[:, sample, :kpool])


def gather_ref(src, idx):
    return _rows_of(src.detach().cpu(), idx.detach().cpu().long())


def normalize_dirs_ref(directions):
    """(3, SC) -> columns of unit length, float64; the kernel's squares, two additions, square root and division leave each component
    within 4 * 2^-24 of it (components are at most 1)"""
    return F.normalize(R._up(directions), dim=0, eps=1e-12)


NORMALIZE_BAR = 4.0 * U


# ------------------------------------------------------------------------------------------------------------------ graphs and inputs
def _distinct(B, n, k, gen, no_self):
    """k different ids per row, in random order (no_self: never the row itself)"""
    assert k <= n - (1 if no_self else 0)
    key = torch.rand(B, n, n, generator=gen)
    if no_self:
        key.diagonal(dim1=1, dim2=2).fill_(2.0)
    return key.argsort(-1)[:, :, :k].to(torch.int32).contiguous()


def graph_slot_wins(B, n, k, seed):
    """k different neighbours per row, never the row itself: a row that wins does so at ONE slot, and `hs_inputs` / `orl_inputs`
    shape the operands so that every slot wins its share decisively"""
    return _distinct(B, n, k, R._gen(seed), True)


def graph_ends(B, n, k, seed):
    """lists that name only ids 0 and n - 1: the first and the last row of every table"""
    pick = torch.rand(B, n, k, generator=R._gen(seed)) < 0.5
    return torch.where(pick, 0, n - 1).to(torch.int32).contiguous()


FAMILIES = dict(R.FAMILIES, slot_wins=graph_slot_wins, ends=graph_ends)


def case_graph(c):
    return FAMILIES[c.family](c.B, c.n, c.k, 2000 + c.seed)


def hs_inputs(c, surface=False):
    """the fp32 operands of a graph-convolution case on the CPU.  slot_wins: the support row of every point's neighbour at slot
    (i mod k) is scaled by 8, so that each slot in turn carries candidates no other slot of the row can reach."""
    gen = R._gen(104729 * c.seed + 31 * c.n + c.C + c.k + (1 if surface else 0))
    xyz = torch.randn(c.B, c.n, 3, generator=gen)
    if c.family == "coincident":
        xyz[:, 10:20] = xyz[:, 0:10]
    idx = case_graph(c)
    sdn = F.normalize(torch.randn(3, S * c.C, generator=gen), dim=0)
    proj = None
    if not surface:
        proj = torch.randn(c.B, c.n, 8 * c.C, generator=gen)
        if c.family == "slot_wins":
            i = torch.arange(c.n)
            q = idx[:, i, i % c.k].long()                                               # (B, n)
            big = torch.zeros(c.B, c.n, dtype=torch.bool).scatter_(1, q, True)
            proj[..., c.C:] = torch.where(big.unsqueeze(-1), 8.0 * proj[..., c.C:], proj[..., c.C:])
    return dict(xyz=xyz, idx=idx, proj=proj, sdn=sdn)


def orl_inputs(c):
    """feat (B, n, C), idx, w2t of an ORL / pool case.  slot_wins: features drawn from [-1, 0], a margin of 2 added to one entry
    in k of every channel: a point that lists exactly one raised row at a channel has its maximum there, at that row's slot alone
    and by more than 1 (1 / e of the entries at large k, spread evenly over the slots because the lists are in random order)."""
    gen = R._gen(15485863 * c.seed + 17 * c.n + c.C + c.k)
    if c.family == "slot_wins":
        feat = -torch.rand(c.B, c.n, c.C, generator=gen)
        feat = feat + 2.0 * (torch.rand(c.B, c.n, c.C, generator=gen) < 1.0 / c.k).float()
    else:
        feat = torch.randn(c.B, c.n, c.C, generator=gen)
        if c.n > 1:
            feat[:, c.n // 2] = feat[:, 0]                                              # exact ties between two rows
    idx = case_graph(c)
    w2t = torch.randn(c.C, c.C, generator=gen) / c.C ** 0.5
    return dict(feat=feat, idx=idx, w2t=w2t)
