"""fp64 reference of the graph layers' forward and backward (TEST INFRASTRUCTURE), plain torch on the CPU.

    HS_layer.graph_conv        out = centre + mean_s max_j relu(dir_ij . D_s) * support[idx_ij][s]         (gcn3d.py:157-180)
    HSlayer_surface.graph_conv out =          mean_s max_j relu(dir_ij . D_s)                               (gcn3d.py:91-106)
    Pool_layer / ORL pooling   y   = max_j src[idx_ij]                                                      (gcn3d.py:210-245)

with dir_ij = F.normalize(x[idx_ij] - x_i, eps=1e-12), proj = [centre (C) | support (7 x C)] per point and D = sdn (3, 7C) the unit
support directions, as oracle/gcn_ref.py and DESIGN.md state them.  Every function takes the kernels' fp32 operands, casts them up and
computes nothing in fp32.

Two derivations of the backward live here: torch autograd of `hs_forward`, and `hs_backward_explicit`, written out by hand with
explicit winners (the first slot of the maximum, as the kernels take it).  tests/test_graph_bwd_cpu.py makes the two agree to 1e-12
before tests/test_graph_bwd_gpu.py lets either judge a kernel.

The explicit form also returns, for every output element, what the comparison's bound is made of:

    abs_terms  the sum of the absolute values of the terms added into the element.  theta = dir . D is itself a sum of three
               products, so a term g / 7 * theta* counts as |g / 7| * sum_a |dir_a D_a|: the fmaf chain's error is relative to that
               sum, not to theta
    chain      the number of non-zero terms.  A sum of m non-zero terms in ANY order or tree passes each term through at most m - 1
               rounded additions (adding an exact zero rounds nothing), so |error| <= (m - 1) 2^-24 abs_terms whatever the kernel's
               summation order (slab walk, atomics, per-workgroup partials)

and the comparison is |got - want| <= (12 + chain) * 2^-24 * abs_terms + 1e-30 per element (`bound`, `mismatch`); 12 covers the
roundings inside one term: three in the normalisation, three in the fmaf chain, the division by 7, the products, the fp32 storage
of the travelling value.  For d xyz the terms are F.normalize's backward of d dir: its inputs carry d dir's own error, so its
abs_terms are propagated from d dir's (not taken from |d dir|, which may have cancelled), and its chain is the number of terms plus the
longest chain among the d dir entries that reach the element plus the 12 roundings of the normalisation's backward (dot product,
den^2, two divisions, the rank-one update).

fp32 and fp64 may legitimately choose different winners where two candidates are closer than the fp32 arithmetic resolves.
`ambiguous` marks those (point, channel) pairs; the tests zero d g there BEFORE the arrays reach either side, so such an entry
contributes nothing to any output, the full reduction of d sdn included, and what remains can be compared tightly.
"""
import collections

import torch
import torch.nn.functional as F

S = 7
U = 2.0 ** -24                       # fp32 unit roundoff
AMBIG_REL = 1e-5                     # winner margin, relative to max |proj| (surface: to 1, theta's range)
AMBIG_THETA = 1e-6                   # |theta| below this may change sign in fp32
ROUNDINGS = 12

Term = collections.namedtuple("Term", "value abs_terms chain")


def _up(t):
    return None if t is None else t.detach().cpu().double()


def _dot3(d, s):
    """d (..., 3) . s (3, E) -> (..., E), written out: the same source listed at two slots must give bit-identical values, so that
    argmax takes the first as the kernels do.  A BLAS product does not promise that: its edge tiles and thread shares may round
    equal rows differently, and the tie's gradient then lands on the later slot of d dir."""
    return d[..., 0:1] * s[0] + d[..., 1:2] * s[1] + d[..., 2:3] * s[2]


def _setup(xyz, idx, proj, sdn, C, surface, rows=None):
    """the quantities the forward, the mask and the explicit backward share, all float64.  rows (a slice of points): those points'
    share alone -- n is then the slice's length and 'proj' holds their rows -- for forwards too large to hold whole
    (tests/graph_fwd_ref.py); the backward needs every point."""
    xyz, sdn, idx = _up(xyz), _up(sdn), idx.detach().cpu().long()
    own = xyz
    if rows is not None:
        idx, own = idx[:, rows], xyz[:, rows]
    B, n, k = idx.shape
    b = torch.arange(B).view(B, 1, 1)
    u = xyz[b, idx] - own.unsqueeze(2)                               # (B, n, k, 3)
    r = u.square().sum(-1, keepdim=True).sqrt()
    dirs = u / r.clamp_min(1e-12)                                    # F.normalize(u, eps=1e-12)
    raw = _dot3(dirs, sdn).view(B, n, k, S, C)                       # theta before the ReLU
    absth = _dot3(dirs.abs(), sdn.abs()).view(B, n, k, S, C)         # sum_a |dir_a D_a|
    th = raw.clamp_min(0.0)
    if surface:
        sup, val = None, th
    else:
        sup = _up(proj)[..., C:].reshape(B, -1, S, C)[b, idx]       # (B, n, k, S, C)
        val = th * sup
    own_proj = None if surface else (_up(proj) if rows is None else _up(proj)[:, rows])
    return dict(xyz=xyz, sdn=sdn, idx=idx, u=u, r=r, dirs=dirs, raw=raw, absth=absth, th=th, sup=sup, val=val, B=B, n=n, k=k, C=C,
                surface=surface, proj=own_proj)


def hs_forward(xyz, idx, proj, sdn, C, surface=False):
    """float64 (B, n, C); differentiable in xyz, proj and sdn when they are float64 leaves.  The maximum is taken at argmax's
    index (the FIRST maximal slot) so that autograd sends a tie's gradient where the kernels send it."""
    idx = idx.long()
    B, n, k = idx.shape
    b = torch.arange(B).view(B, 1, 1)
    xyz, sdn = xyz.double(), sdn.double()
    dirs = F.normalize(xyz[b, idx] - xyz.unsqueeze(2), dim=-1, eps=1e-12)
    val = torch.relu(_dot3(dirs, sdn)).view(B, n, k, S, C)
    if not surface:
        proj = proj.double()
        val = val * proj[..., C:].reshape(B, n, S, C)[b, idx]
    m = val.gather(2, val.argmax(2, keepdim=True)).squeeze(2)       # (B, n, S, C)
    out = m.sum(2) / 7.0
    return out if surface else proj[..., :C] + out


def forward_terms(xyz, idx, proj, sdn, C, surface=False, pre=None):
    """the forward output with its abs_terms (|centre| + sum_s sum_a |dir_a D_a| |support| / 7 at the winners) and chain = 7"""
    p = pre or _setup(xyz, idx, proj, sdn, C, surface)
    jw = p["val"].argmax(2, keepdim=True)
    m = p["val"].gather(2, jw).squeeze(2)
    a = p["absth"].gather(2, jw).squeeze(2)
    if not surface:
        a = a * p["sup"].gather(2, jw).squeeze(2).abs()
    out, ab = m.sum(2) / 7.0, a.sum(2) / 7.0
    if not surface:
        out, ab = p["proj"][..., :C] + out, p["proj"][..., :C].abs() + ab
    return Term(out, ab, torch.full_like(out, 7.0))


def ambiguous(xyz, idx, proj, sdn, C, surface=False, pre=None):
    """(B, n, C) bool: for some support s, the best value and the best among candidates naming a DIFFERENT source row differ by more
    than 0 and less than 1e-5 max|proj|, or some candidate has 0 < |theta| < 1e-6.  Exactly equal values are not ambiguous: the same
    source listed twice (both sides take the first slot, the gradient lands on the same row) and maxima that are exactly zero (no
    gradient).  The thresholds are 40 to 80 ulp of what they guard, far above what the fp32 fmaf chain moves."""
    p = pre or _setup(xyz, idx, proj, sdn, C, surface)
    val, idx = p["val"], p["idx"]
    B, n, k = idx.shape
    best, jw = val.amax(2, keepdim=True), val.argmax(2, keepdim=True)
    ids = idx.view(B, n, k, 1, 1).expand(B, n, k, S, C)
    qw = ids.gather(2, jw)
    other = val.masked_fill(ids == qw, float("-inf")).max(2, keepdim=True)[0]
    diff = best - other
    scale = 1.0 if surface else float(p["proj"].abs().max())
    close = (diff > 0) & (diff < AMBIG_REL * scale)
    a = p["raw"].abs()
    tiny = ((a > 0) & (a < AMBIG_THETA)).any(2, keepdim=True)
    return (close | tiny).squeeze(2).any(2)


def hs_backward_explicit(xyz, idx, proj, sdn, dg, C, surface=False, pre=None):
    """hand-derived backward with explicit winners -> dict of Term: 'dproj' (B, n, 8C) = [d centre | d support] (HS only), 'dsdn'
    (3, 7C), 'ddir' (B, n, k, 3), 'dxyz' (B, n, 3)."""
    p = pre or _setup(xyz, idx, proj, sdn, C, surface)
    B, n, k, idx = p["B"], p["n"], p["k"], p["idx"]
    dg = _up(dg)
    jw = p["val"].argmax(2, keepdim=True)                            # (B, n, 1, S, C): the first maximal slot
    take = lambda t: t.gather(2, jw).squeeze(2)
    thw, athw = take(p["th"]), take(p["absth"])
    supw = None if surface else take(p["sup"])
    qw = take(idx.view(B, n, k, 1, 1).expand(B, n, k, S, C))         # the winning source row
    jw = jw.squeeze(2)
    g7 = (dg / 7.0).unsqueeze(2)                                     # (B, n, 1, C): the mean over the supports
    pos = (thw > 0).double()                                         # ReLU'(0) = 0
    out = {}

    if not surface:
        # d centre = d g;  d support[winner's row][s][c] += g / 7 * theta*
        send = g7 * thw
        sup_t = [torch.zeros(B, n, S, C, dtype=torch.float64).scatter_add_(1, qw, t)
                 for t in (send, g7.abs() * athw * pos, (send != 0).double())]
        flat = lambda c, s_: torch.cat([c, s_.reshape(B, n, S * C)], 2)
        out["dproj"] = Term(flat(dg, sup_t[0]), flat(dg.abs(), sup_t[1]), flat((dg != 0).double(), sup_t[2]))

    # the gradient that reaches theta at the winner, and through it D_s and the winner's direction
    w = pos * g7 * (1.0 if surface else supw)                        # (B, n, S, C)
    bI, nI = torch.arange(B).view(B, 1, 1, 1), torch.arange(n).view(1, n, 1, 1)
    dirw = p["dirs"][bI, nI, jw]                                     # (B, n, S, C, 3)
    t = w.unsqueeze(-1) * dirw
    red = lambda x: x.sum((0, 1)).permute(2, 0, 1).reshape(3, S * C)
    out["dsdn"] = Term(red(t), red(t.abs()), red((t != 0).double()))

    sd = p["sdn"].view(3, S * C).t().reshape(1, 1, S * C, 3)         # D as (e, component)
    t = w.reshape(B, n, S * C, 1) * sd                               # (B, n, 7C, 3)
    ji = jw.reshape(B, n, S * C, 1).expand(B, n, S * C, 3)
    dd = [torch.zeros(B, n, k, 3, dtype=torch.float64).scatter_add_(2, ji, x) for x in (t, t.abs(), (t != 0).double())]
    out["ddir"] = Term(*dd)

    # F.normalize's backward as torch differentiates it (norm -> clamp_min -> div), then the difference's: -du to the point, +du to
    # the neighbour
    u, r = p["u"], p["r"]
    den = r.clamp_min(1e-12)
    live, rr = r >= 1e-12, r.clamp_min(1e-12)                        # (the norm's own backward is 0 below eps)
    zero = torch.zeros((), dtype=torch.float64)
    du = dd[0] / den - torch.where(live, u * (dd[0] * u).sum(-1, keepdim=True) / (den * den * rr), zero)
    du_abs = dd[1] / den + torch.where(live, u.abs() * (dd[1] * u.abs()).sum(-1, keepdim=True) / (den * den * rr), zero)
    ii = idx.reshape(B, n * k, 1).expand(B, n * k, 3)
    gather_in = lambda x: torch.zeros(B, n, 3, dtype=torch.float64).scatter_add_(1, ii, x.reshape(B, n * k, 3))
    cd = dd[2].amax(-1)                                              # (B, n, k): d dir's longest chain per entry
    cmax = torch.maximum(cd.amax(2), torch.zeros(B, n, dtype=torch.float64).scatter_reduce_(1, idx.reshape(B, n * k),
                                                                                           cd.reshape(B, n * k), "amax"))
    nz = (du_abs != 0).double()
    count = nz.sum(2) + gather_in(nz)
    out["dxyz"] = Term(gather_in(du) - du.sum(2), gather_in(du_abs) + du_abs.sum(2), count + cmax.unsqueeze(-1) + ROUNDINGS)
    return out


def nbrmax_backward(src, idx, dy, per_object=False, scale=1.0):
    """y[b, p] = max_j src[b, idx[b, p, j]] (first maximal slot): d src as a Term.  dy (B, n_rows, C), or (B, C) when per_object: every
    row of the object then receives dy[b] * scale.  No ambiguity mask is needed here: both sides compare the same fp32 numbers."""
    src, dy, idx = _up(src), _up(dy), idx.detach().cpu().long()
    B, n_src, C = src.shape
    n_rows, k = idx.shape[1], idx.shape[2]
    b = torch.arange(B).view(B, 1, 1)
    vals = src[b, idx]                                               # (B, n_rows, k, C)
    jw = vals.argmax(2, keepdim=True)
    qw = idx.view(B, n_rows, k, 1).expand(B, n_rows, k, C).gather(2, jw).squeeze(2)
    g = (dy.unsqueeze(1).expand(B, n_rows, C) * scale) if per_object else dy
    z = lambda: torch.zeros(B, n_src, C, dtype=torch.float64)
    return Term(z().scatter_add_(1, qw, g), z().scatter_add_(1, qw, g.abs()), z().scatter_add_(1, qw, (g != 0).double()))


def bound(term, chain=None):
    """(12 + chain) * 2^-24 * abs_terms + 1e-30; chain: overrides the term's (the d sdn partials' longest addition path)"""
    c = term.chain if chain is None else torch.minimum(term.chain, torch.as_tensor(float(chain), dtype=torch.float64))
    return (ROUNDINGS + c) * U * term.abs_terms + 1e-30


def mismatch(got, term, chain=None):
    """-> (bool tensor of the elements outside the bound, the largest |error| / bound)"""
    got = got.detach().cpu().double().reshape(term.value.shape)
    err, bd = (got - term.value).abs(), bound(term, chain)
    bad = ~(err <= bd)                                               # a NaN is a mismatch
    return bad, float((err / bd).max()) if err.numel() else 0.0


def dsdn_path(B, n):
    """the longest addition path through the d sdn partials: 16 points per workgroup partial (GG_PTS / GB_PTS), 32 partials per group
    (GB_GROUP, and the same literal in gg_partial_sum_kernel), then the groups.  The scatter kernel at C = 128 runs two 16-point
    streams per workgroup, each with a partial of its own: B * ceil(n / 32) * 2 partials, never fewer than the gather form's."""
    parts = B * ((n + 31) // 32) * 2
    return 16 + 32 + (parts + 31) // 32


# ------------------------------------------------------------------------------------------------------------------ graph builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def graph_base(B, n, k, seed):
    """random ids within the object, slot 0 the point itself (as kNN gives it: a zero direction)"""
    idx = torch.randint(0, n, (B, n, k), generator=_gen(seed), dtype=torch.int32)
    idx[:, :, 0] = torch.arange(n, dtype=torch.int32)
    return idx


HUB = 5


def graph_hub(B, n, k, L, seed):
    """row HUB is listed exactly L times in every object, its own self entry included: by L - 1 other rows, once each, at a slot
    past 0.  Stray random hits are replaced by another id."""
    assert k >= 2 and L - 1 <= n - 1 and n > HUB + 2
    gen = _gen(seed)
    idx = graph_base(B, n, k, seed + 1)
    rest = idx[:, :, 1:]
    rest[rest == HUB] = HUB + 2                                      # stray hits
    others = torch.tensor([i for i in range(n) if i != HUB])
    for b in range(B):
        rows = others[torch.randperm(n - 1, generator=gen)[: L - 1]]
        slots = torch.randint(1, k, (L - 1,), generator=gen)
        idx[b, rows, slots] = HUB
    return idx


def graph_everyone_lists_2(B, n, k, seed):
    """every row lists source 2 at slot 1 (row 2 itself: twice), among ordinary lists"""
    idx = graph_base(B, n, k, seed)
    idx[:, :, 1] = 2
    return idx


def graph_no_self(B, n, k, seed):
    """no row lists itself, and only even ids are listed: every odd source has an empty reverse list"""
    assert n >= 4
    m = (n + 1) // 2                                                 # even ids 0, 2, .., 2 (m - 1)
    idx = 2 * torch.randint(0, m, (B, n, k), generator=_gen(seed), dtype=torch.int32)
    own = torch.arange(n, dtype=torch.int32).view(1, n, 1)
    return torch.where(idx == own, (idx + 2) % (2 * m), idx).to(torch.int32).contiguous()


def graph_repeats(B, n, k, seed):
    """every row lists the source of slot 1 again at slot 2 (slots of different parity: the two lane groups of the C = 128 slot kernel
    meet it in their merge), every third row a third time at slot 4"""
    assert k >= 5
    idx = graph_base(B, n, k, seed)
    idx[:, :, 2] = idx[:, :, 1]
    idx[:, ::3, 4] = idx[:, ::3, 1]
    return idx


def graph_coincident(B, n, k, seed):
    """ordinary lists in which rows 0:10 and 10:20 (the caller makes their points coincide) list each other at slot 1"""
    assert n >= 20 and k >= 2
    idx = graph_base(B, n, k, seed)
    idx[:, 0:10, 1] = torch.arange(10, 20, dtype=torch.int32)
    idx[:, 10:20, 1] = torch.arange(0, 10, dtype=torch.int32)
    return idx


FAMILIES = {"base": graph_base, "hub": graph_hub, "everyone_lists_2": graph_everyone_lists_2, "no_self": graph_no_self,
            "repeats": graph_repeats, "coincident": graph_coincident}

Case = collections.namedtuple("Case", "family B n k C seed L view")


def case(family, B, n, k, C, seed=0, L=0, view=False):
    return Case(family, B, n, k, C, seed, L, view)


def case_id(c):
    return "%s%s-B%d-n%d-k%d-C%d%s" % (c.family, c.L or "", c.B, c.n, c.k, c.C, "-view" if c.view else "")


def case_graph(c):
    args = (c.B, c.n, c.k) + ((c.L,) if c.family == "hub" else ()) + (1000 + c.seed,)
    return FAMILIES[c.family](*args)


def case_inputs(c, surface=False):
    """the fp32 operands of a case on the CPU, d g already zeroed where `ambiguous` says so -> (dict, zeroed share, shared setup)"""
    gen = _gen(7919 * c.seed + 31 * c.n + c.C + c.k + (1 if surface else 0))
    xyz = torch.randn(c.B, c.n, 3, generator=gen)
    if c.family == "coincident":
        xyz[:, 10:20] = xyz[:, 0:10]
    idx = case_graph(c)
    proj = None if surface else torch.randn(c.B, c.n, 8 * c.C, generator=gen)
    sdn = F.normalize(torch.randn(3, S * c.C, generator=gen), dim=0)
    dg = torch.randn(c.B, c.n, c.C, generator=gen)
    pre = _setup(xyz, idx, proj, sdn, c.C, surface)
    amb = ambiguous(xyz, idx, proj, sdn, c.C, surface, pre=pre)
    dg[amb] = 0.0
    return dict(xyz=xyz, idx=idx, proj=proj, sdn=sdn, dg=dg), float(amb.double().mean()), pre
