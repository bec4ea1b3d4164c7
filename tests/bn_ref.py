"""Training-mode BatchNorm (csrc/bn.hip and the BatchNorm half of csrc/backward.hip) restated on the CPU: `ref64`, the operation in
float64, and `oracle32`, the kernels' documented algorithm and summation order in float32.  numpy / torch only, no project import.

    forward   mu = E[x], var = E[(x - mu)^2] (biased), z = (x - mu) * gamma / sqrt(var + eps) + beta, y = act(z) with act none or
              z > 0 ? z : z * slope (slope a scalar or a per-column vector; 0 is ReLU), the max of y over each object's rows for the
              first cm_cols columns with the winning row (the first on ties), running <- (1 - m) running + m batch (the variance
              with n / (n - 1)), num_batches_tracked + 1
    backward  xhat = (x - mu) / sqrt(var + eps), z = xhat * gamma + beta, dz = dy * (z > 0 ? 1 : slope), dbeta = sum dz,
              dgamma = sum dz * xhat, dx = gamma * inv * ((dz - mean dz) - xhat * mean(dz * xhat));  mu and var are operands of the
              backward kernels, so the reference takes them as given (the batch statistics in float64 when none are passed)
    pooled    the same with dz nonzero only on the recorded argmax row of each (object, column)

oracle32 follows the two forms the library picks between (`form`): "v4", a column quad per thread with 256-row chunks -- one pass of
shifted sums (K = the chunk's first row) and a Chan merge in chunk order, four chunk groups merged in group order -- and "s", one
column per thread with 1024-row chunks, the first row as the shift of the mean pass, then the centred squares.  In both a chunk's rows
go to four slices (row r to slice r % 4) that are combined as ((s0 + s1) + s2) + s3.

The bar of the GPU tests, per output tensor and per column kind: |kernel - ref64| <= 4 max|oracle32 - ref64| + 4 eps32 max|ref64|.
"""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
EPS32 = float(np.finfo(np.float32).eps)
BN_EPS = float(np.float32(1e-5))        # the kernels take eps as a float: both restatements use the value they see
MAX_EXCLUDED = 1e-3

KINDS = ("benign", "far", "const", "zero", "onerow", "kout", "tiny", "huge", "neg", "gamma0")
SIGN_EXACT = ("const", "zero", "gamma0")        # z == beta exactly: nothing about these columns may be called ambiguous
Q_FREE = ("kout", "tiny", "huge")               # kinds the conditioning check of the one-pass form leaves out
NO_TIES = tuple(k for k in KINDS if k != "tiny")  # (float32 cannot tell the rows of a 1e-20 column apart: every argmax would be a tie)


def gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def kinds_of(C, shift=0, kinds=KINDS):
    """column c is of kind kinds[(c + shift) % len]: 10 kinds against quads of 4, so every 16-byte quad mixes kinds"""
    return [kinds[(c + shift) % len(kinds)] for c in range(C)]


def onerow_row(rows):
    r = rows // 2
    return r + 1 if r % 256 == 0 and r + 1 < rows else r


def make_case(rows, C, shift=0, kinds=KINDS, seed=0):
    """-> dict(x (rows, C) float32, gamma, beta, slope_vec (C,) float32, kinds [C]).  Columns lie side by side, one kind each:
       benign   2 N(0,1) + 0.5 N(0,1)            far     1e3 + N(0,1): mean = 1e3 std
       const    0.1 in every row                 zero    0 in every row
       onerow   0 but for one row of 3           kout    N(0,1), every 256th row (each one-pass chunk's K) 1e3
       tiny     1e-20 N(0,1): var << eps, the squares are denormal        huge    1e15 N(0,1)
       neg      benign with beta = -50: ReLU kills the column             gamma0  benign with gamma = 0
    The first row of every 256-row chunk of a benign / far / neg / gamma0 column lies within half a standard deviation of the mean of the
    chunk's other rows (q_over_var below), and elements whose pre-activation would fall within 2e-4 gamma of 0 are moved by 1e-3 std
    (`ambiguous`: the backward sums make one undecided element the whole column's business)."""
    ge = gen(rows, C, shift, seed, len(kinds))
    kd = kinds_of(C, shift, kinds)
    x = torch.zeros(rows, C, dtype=F64)
    gamma = torch.rand(C, generator=ge, dtype=F64) + 0.5
    beta = torch.randn(C, generator=ge, dtype=F64)
    nom = {}
    for c, k in enumerate(kd):
        n = torch.randn(rows, generator=ge, dtype=F64)
        first = torch.arange(0, rows, 256)
        if k in ("benign", "neg", "gamma0"):
            m, s = 0.5 * float(torch.randn(1, generator=ge, dtype=F64)), 2.0
        elif k == "far":
            m, s = 1e3, 1.0
        if k in ("benign", "neg", "gamma0", "far"):
            for r0 in first.tolist():                               # K: within half a deviation of the mean of its chunk's other rows
                rest = n[r0 + 1:min(r0 + 256, rows)]
                if rest.numel() >= 2:
                    n[r0] = rest.mean() + 0.5 * n[r0].clamp(-1.0, 1.0) * rest.std(unbiased=False)
            x[:, c] = m + s * n
            nom[c] = s
        elif k == "const":
            x[:, c] = 0.1
        elif k == "onerow":
            x[onerow_row(rows), c] = 3.0
        elif k == "kout":
            x[:, c] = n
            x[first, c] = 1e3
            nom[c] = 62.0
        elif k == "tiny":
            x[:, c] = 1e-20 * n
        elif k == "huge":
            x[:, c] = 1e15 * n
            nom[c] = 1e15
        if k == "neg":
            beta[c] = -50.0
        if k == "gamma0":
            gamma[c] = 0.0
    x = x.to(F32)
    gamma, beta = gamma.to(F32), beta.to(F32)
    # keep the activation decision away from 0 where it is a matter of chance (see ambiguous): a float32 step of the column's scale
    if rows > 1:
        z = ref64(x, gamma, beta)["z"]
        for c, s in nom.items():
            if kd[c] == "gamma0":
                continue
            near = z[:, c].abs() < 2e-4 * float(gamma[c])
            if bool(near.any()):
                step = torch.where(z[:, c] >= 0, 1.0, -1.0) * 1e-3 * s
                x[:, c] = torch.where(near, (x[:, c].double() + step).to(F32), x[:, c])
    slope_vec = torch.tensor([(0.2, 0.0, 0.01, 1.0)[(c // 3) % 4] for c in range(C)], dtype=F32)
    return dict(x=x, gamma=gamma, beta=beta, slope_vec=slope_vec, kinds=kd)


def columns_of(kinds, kind):
    return torch.tensor([k == kind for k in kinds], dtype=torch.bool)


def bound(ref, ora):
    """the allowed deviation of a float32 kernel from ref64, for one tensor (one kind's columns of it)"""
    ref, ora = ref.detach().to(F64), ora.detach().to(F64)
    if ref.numel() == 0:
        return 0.0
    return 4.0 * float((ora - ref).abs().max()) + 4.0 * EPS32 * float(ref.abs().max())


def excluded_share_ok(mask):
    return mask.numel() == 0 or float(mask.double().mean()) <= MAX_EXCLUDED


# ---------------------------------------------------------------------------------------------------------------- shared pieces
def _slope(C, slope, slope_vec, T):
    return slope_vec.to(T) if slope_vec is not None else torch.full((C,), float(slope), dtype=T)


def _act(z, act, sl):
    return torch.where(z > 0, z, z * sl) if act else z            # (a NaN is not > 0: NaN * slope stays NaN)


def _act_grad(z, act, sl):
    return torch.where(z > 0, torch.ones_like(z), sl.expand_as(z)) if act else torch.ones_like(z)


def _pool(y, rows_per_obj, cm_cols):
    """max over each object's rows and the winning global row, the first on ties (NaN wins, as torch.max)"""
    rows, C = y.shape
    yo = y[:, :cm_cols].reshape(rows // rows_per_obj, rows_per_obj, cm_cols)
    val, arg = yo.max(1)
    first = (yo == val.unsqueeze(1)) | (torch.isnan(yo) & torch.isnan(val).unsqueeze(1))
    arg = torch.where(first, torch.arange(rows_per_obj).view(1, -1, 1), rows_per_obj).min(1)[0]
    return val, (arg + torch.arange(rows // rows_per_obj).unsqueeze(1) * rows_per_obj).to(torch.int32)


def _running(T, running, mean, var, rows):
    rm, rv, m, nbt = running
    m_, keep = torch.tensor(float(m), dtype=T), torch.tensor(1.0, dtype=T) - torch.tensor(float(m), dtype=T)
    unbias = torch.tensor(rows / (rows - 1.0), dtype=T)
    return rm.to(T) * keep + m_ * mean, rv.to(T) * keep + (m_ * unbias) * var, None if nbt is None else nbt + 1


def _finish_fwd(T, x, mean, var, gamma, beta, eps, act, slope, slope_vec, rows_per_obj, cm_cols, running):
    rows, C = x.shape
    sl = _slope(C, slope, slope_vec, T)
    a = gamma.to(T) / torch.sqrt(var + torch.tensor(eps, dtype=T))
    z = (x.to(T) - mean) * a + beta.to(T)
    out = dict(mean=mean, var=var, z=z, y=_act(z, act, sl))
    if rows_per_obj:
        out["colmax"], out["argrow"] = _pool(out["y"], rows_per_obj, cm_cols or C)
    if running is not None:
        out["rm"], out["rv"], out["nbt"] = _running(T, running, mean, var, rows)
    return out


# ---------------------------------------------------------------------------------------------------------------- float64
def ref64(x, gamma, beta, eps=BN_EPS, act=0, slope=0.0, slope_vec=None, rows_per_obj=0, cm_cols=0, running=None, stats=None):
    """the forward in float64; stats = (mean, var) given instead of the batch's (ops.bn_apply)"""
    xd = x.to(F64)
    if stats is None:
        mean = xd.mean(0)
        var = ((xd - mean) ** 2).mean(0)
    else:
        mean, var = stats[0].to(F64), stats[1].to(F64)
    return _finish_fwd(F64, x, mean, var, gamma, beta, eps, act, slope, slope_vec, rows_per_obj, cm_cols, running)


def _bwd_terms(T, x, mean, var, gamma, beta, eps, act, sl):
    inv = 1.0 / torch.sqrt(var.to(T) + torch.tensor(eps, dtype=T))
    xh = (x.to(T) - mean.to(T)) * inv
    z = xh * gamma.to(T) + beta.to(T)
    return inv, xh, z, _act_grad(z, act, sl)


def ref64_bwd(dy, x, gamma, beta, eps=BN_EPS, act=0, slope=0.0, slope_vec=None, stats=None):
    """-> dict(dx, dgamma, dbeta, z)"""
    xd = x.to(F64)
    mean, var = (xd.mean(0), ((xd - xd.mean(0)) ** 2).mean(0)) if stats is None else stats
    inv, xh, z, ag = _bwd_terms(F64, x, mean, var, gamma, beta, eps, act, _slope(x.shape[1], slope, slope_vec, F64))
    dz = dy.to(F64) * ag
    db, dg = dz.sum(0), (dz * xh).sum(0)
    n = x.shape[0]
    return dict(dx=gamma.to(F64) * inv * ((dz - db / n) - xh * (dg / n)), dgamma=dg, dbeta=db, z=z, xhat=xh)


def _scatter(T, dpool, argrow, rows):
    """(objects, C) values onto their recorded rows of a dense (rows, C) tensor, and the mask of those rows"""
    objects, C = dpool.shape
    dense, hit = torch.zeros(rows, C, dtype=T), torch.zeros(rows, C, dtype=torch.bool)
    cols = torch.arange(C).expand(objects, C)
    dense[argrow.long(), cols] = dpool.to(T)
    hit[argrow.long(), cols] = True
    return dense, hit


def ref64_bwd_pooled(dpool, argrow, x, gamma, beta, eps=BN_EPS, act=0, slope=0.0, slope_vec=None, stats=None):
    dense, _ = _scatter(F64, dpool, argrow, x.shape[0])
    return ref64_bwd(dense, x, gamma, beta, eps, act, slope, slope_vec, stats)


def colsum(dy):
    return dy.to(F64).sum(0)


def colsum_objects(dy):
    """(B, n, C) -> (B, C)"""
    return dy.to(F64).sum(1)


# ---------------------------------------------------------------------------------------------------------------- float32
def _sliced(t, chunk, pad_with=None):
    """(rows, C) -> (chunks, chunk / 4, 4, C): [k, i, s] is row k * chunk + 4 i + s; rows past the end hold `pad_with` (per chunk and
    column) or 0 -- values that add an exact 0 to the sums below"""
    rows, C = t.shape
    chunks = -(-rows // chunk)
    full = torch.zeros(chunks * chunk, C, dtype=t.dtype)
    full[:rows] = t
    full = full.view(chunks, chunk // 4, 4, C)
    if pad_with is not None:
        live = (torch.arange(chunks * chunk) < rows).view(chunks, chunk // 4, 4, 1)
        full = torch.where(live, full, pad_with.view(chunks, 1, 1, C).expand_as(full))
    return full


def _slice_sums(terms):
    """terms (chunks, steps, 4, C) float32: every slice adds its rows one after the other, the slices combine as ((0 + 1) + 2) + 3"""
    acc = torch.zeros_like(terms[:, 0])
    for i in range(terms.shape[1]):
        acc = acc + terms[:, i]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]      # (chunks, C)


def _in_order(parts):
    s = torch.zeros_like(parts[0])
    for k in range(parts.shape[0]):
        s = s + parts[k]
    return s


def _four_groups(parts):
    """bw_finish2_kernel: four groups of (chunks + 3) / 4 chunks, each in chunk order, then ((g0 + g1) + g2) + g3"""
    chunks = parts.shape[0]
    per = (chunks + 3) // 4
    g = [_in_order(parts[q * per:min((q + 1) * per, chunks)]) if q * per < chunks else torch.zeros_like(parts[0]) for q in range(4)]
    return ((g[0] + g[1]) + g[2]) + g[3]


def _chan(n_a, mean_a, m2_a, n_b, mean_b, m2_b):
    n = n_a + n_b
    delta = mean_b - mean_a
    return n, mean_a + delta * (n_b / n), (m2_a + m2_b) + delta * delta * (n_a * (n_b / n))


def stats32(x, form):
    """(mean, var) as bn_stats_partial_v4 + bn_stats_finish_v4 ("v4") or bn_partial x 2 + bn_finish x 2 ("s") form them"""
    x = x.to(F32)
    rows, C = x.shape
    f = lambda v: torch.tensor(float(v), dtype=F32)
    if form == "s":
        K = x[0]
        inv = f(1.0 / rows)
        mean = K + _in_order(_slice_sums(_sliced(x, 1024, K.expand(-(-rows // 1024), C)) - K)) * inv
        d = _sliced(x, 1024, mean.expand(-(-rows // 1024), C)) - mean
        return mean, _in_order(_slice_sums(d * d)) * inv
    chunks = -(-rows // 256)
    K = x[0::256]                                                   # (chunks, C): each chunk's first row
    d = _sliced(x, 256, K) - K.view(chunks, 1, 1, C)
    s1, s2 = _slice_sums(d), _slice_sums(d * d)
    per = (chunks + 3) // 4
    groups = []
    for q in range(4):
        n_a, mean_a, m2_a = f(0), torch.zeros(C), torch.zeros(C)
        for k in range(q * per, min((q + 1) * per, chunks)):
            n_b = f(min(256, rows - k * 256))
            n_a, mean_a, m2_a = _chan(n_a, mean_a, m2_a, n_b, K[k] + s1[k] / n_b, s2[k] - s1[k] * (s1[k] / n_b))
        groups.append((n_a, mean_a, m2_a))
    n_a, mean_a, m2_a = groups[0]
    for q in range(1, 4):
        if float(groups[q][0]) > 0:
            n_a, mean_a, m2_a = _chan(n_a, mean_a, m2_a, *groups[q])
    v = m2_a / n_a
    return mean_a, torch.where(v < 0, torch.zeros_like(v), v)


def oracle32(x, gamma, beta, eps=BN_EPS, act=0, slope=0.0, slope_vec=None, rows_per_obj=0, cm_cols=0, running=None, stats=None,
             form="v4"):
    """the forward as the kernels compute it: `form` is the statistics' (both apply kernels evaluate one expression per element)"""
    mean, var = stats32(x, form) if stats is None else (stats[0].to(F32), stats[1].to(F32))
    return _finish_fwd(F32, x, mean, var, gamma, beta, eps, act, slope, slope_vec, rows_per_obj, cm_cols, running)


def _bwd_sums32(dz, xh, form):
    if form == "s":
        return _in_order(_slice_sums(_sliced(dz, 1024))), _in_order(_slice_sums(_sliced(dz * xh, 1024)))
    return _four_groups(_slice_sums(_sliced(dz, 256))), _four_groups(_slice_sums(_sliced(dz * xh, 256)))


def _bwd_apply32(x, dz, xh, inv, gamma, s1, s2):
    inv_n = torch.tensor(1.0 / x.shape[0], dtype=F32)
    return (gamma.to(F32) * inv) * ((dz - s1 * inv_n) - xh * (s2 * inv_n))


def oracle32_bwd(dy, x, gamma, beta, eps=BN_EPS, act=0, slope=0.0, slope_vec=None, stats=None, form="v4"):
    mean, var = stats32(x, form) if stats is None else stats
    inv, xh, z, ag = _bwd_terms(F32, x, mean, var, gamma, beta, eps, act, _slope(x.shape[1], slope, slope_vec, F32))
    dz = dy.to(F32) * ag
    s1, s2 = _bwd_sums32(dz, xh, form)
    return dict(dx=_bwd_apply32(x, dz, xh, inv, gamma, s1, s2), dgamma=s2, dbeta=s1, z=z, xhat=xh)


def oracle32_bwd_pooled(dpool, argrow, x, gamma, beta, eps=BN_EPS, act=0, slope=0.0, slope_vec=None, stats=None, form="v4"):
    """bn_bwd_pooled_sums_kernel adds the objects one after the other; the apply pass is the dense one's"""
    mean, var = stats32(x, form) if stats is None else stats
    inv, xh, z, ag = _bwd_terms(F32, x, mean, var, gamma, beta, eps, act, _slope(x.shape[1], slope, slope_vec, F32))
    dense, _ = _scatter(F32, dpool, argrow, x.shape[0])
    dz = dense * ag
    cols = torch.arange(x.shape[1]).expand(argrow.shape)
    dzo, xho = dz[argrow.long(), cols], xh[argrow.long(), cols]
    return dict(dx=_bwd_apply32(x, dz, xh, inv, gamma, _in_order(dzo), _in_order(dzo * xho)), dgamma=_in_order(dzo * xho),
                dbeta=_in_order(dzo), z=z, xhat=xh)


def colsum32(dy, form):
    dy = dy.to(F32)
    return _in_order(_slice_sums(_sliced(dy, 1024))) if form == "s" else _four_groups(_slice_sums(_sliced(dy, 256)))


def colsum_objects32(dy):
    """colsum_objects_kernel: S = 1024 / CW contiguous row slices [n s / S, n (s + 1) / S), each in row order, combined in slice order;
    CW = 32 channels per workgroup while ceil(C / 64) * objects < 512, else 64"""
    dy = dy.to(F32)
    B, n, C = dy.shape
    S = 32 if -(-C // 64) * B < 512 else 16
    acc = None
    for s in range(S):
        part = torch.zeros(B, C, dtype=F32)
        for r in range(n * s // S, n * (s + 1) // S):
            part = part + dy[:, r]
        acc = part if acc is None else acc + part
    return acc


def two_pass32(x):
    """a plain float32 two-pass in torch (the yardstick next to oracle32 in the conditioning table)"""
    x = x.to(F32)
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


# ---------------------------------------------------------------------------------------------------------------- ambiguity
def ambiguous_z(z64, xhat64, gamma, beta):
    """elements whose activation decision float32 may not reproduce: z = xhat * gamma + beta nonzero and within 16 float32 roundings of
    its own terms of 0 (the kernels form z in three or four rounded operations)"""
    scale = (xhat64 * gamma.to(F64)).abs() + beta.to(F64).abs()
    return (z64 != 0) & (z64.abs() <= 16.0 * EPS32 * scale)


def ambiguous(x, gamma, beta, eps=BN_EPS, stats=None, stats_other=None, rows_per_obj=0, cm_cols=0, act=0, slope=0.0, slope_vec=None,
              tie_tol=None):
    """-> dict(z (rows, C) bool, cols (C,) bool, arg (objects, cm_cols) bool or None)
    z: the activation decision is not decided in float32 -- |z64| within a few float32 roundings of 0 (ambiguous_z), or z64 formed with
       the statistics `stats` and with `stats_other` (the forward's (x - mu) a + beta with float32 statistics against the backward's
       xhat gamma + beta, say) on different sides of 0;
    cols: columns that hold such an element (dbeta, dgamma and the column's dx depend on every decision of the column);
    arg: argmax rows whose runner-up -- the largest value different from the maximum -- lies within tie_tol of it: by default
       64 eps32 (|z| + |beta|) of the maximum, the rounding of the two values' own formation."""
    r = ref64_bwd(torch.zeros_like(x), x, gamma, beta, eps, 0, 0.0, None, stats)
    amb = ambiguous_z(r["z"], r["xhat"], gamma, beta)
    if stats_other is not None:
        o = ref64_bwd(torch.zeros_like(x), x, gamma, beta, eps, 0, 0.0, None, stats_other)
        amb |= ambiguous_z(o["z"], o["xhat"], gamma, beta) | ((r["z"] > 0) != (o["z"] > 0))
    out = dict(z=amb, cols=amb.any(0), arg=None)
    if rows_per_obj:
        rows, C = x.shape
        cm = cm_cols or C
        sl = _slope(C, slope, slope_vec, F64)
        shape = (rows // rows_per_obj, rows_per_obj, cm)
        y = _act(r["z"], act, sl)[:, :cm].reshape(shape)
        # the rounding of a value's own formation: its terms, times the slope the activation applied to it
        err = (((r["xhat"] * gamma.to(F64)).abs() + beta.to(F64).abs()) * _act_grad(r["z"], act, sl).abs())[:, :cm].reshape(shape)
        top = y.max(1)[0]
        at_top = y == top.unsqueeze(1)
        rest = torch.where(at_top, torch.full_like(y, -float("inf")), y).max(1)[0]
        tol = 64.0 * EPS32 * torch.where(at_top, err, torch.zeros_like(err)).max(1)[0] if tie_tol is None else tie_tol
        out["arg"] = (top - rest) <= tol
    return out


def q_over_var(x):
    """the conditioning quantity of the one-pass form: Q_c = (1 / rows) sum over chunks and rows of (x - K_chunk)^2, and var_c, float64"""
    xd = x.to(F64)
    rows = xd.shape[0]
    K = xd[0::256].repeat_interleave(256, 0)[:rows]
    return ((xd - K) ** 2).mean(0), ((xd - xd.mean(0)) ** 2).mean(0)


# ---------------------------------------------------------------------------------------------------------------- the GPU file's cases
ROWS = (2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 1281, 2049)
# (C, layout of x, activation mode): modes 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 per-column slopes.  Layouts: "C" ld = C, "C+4", "C+1",
# "off1" a view one float into an aligned buffer.  C = 4 .. 260 with ld % 4 == 0 take the 16-byte form, the others the 4-byte form.
C_CONFIGS = ((4, "C", 1), (64, "C+4", 2), (252, "C", 3), (256, "C", 0), (260, "C", 1), (1, "C", 1), (3, "C+1", 2), (63, "C", 3),
             (65, "C", 0))
LAYOUT_ROWS = (5, 257, 1281)
LAYOUT_C = 64
# (rows, rows_per_obj, C, cm_cols): object boundaries inside, at and across the 256- and 1024-row chunks
POOL_CASES = ((1281, 1, 64, 32), (1281, 3, 64, 64), (1281, 1281, 260, 128), (1285, 257, 64, 64), (257, 257, 63, 40), (1023, 3, 252, 250),
              (5, 1, 4, 4), (2049, 3, 65, 65), (1025, 1, 64, 64))
NAN_CASES = ((1281, 64), (1281, 63))


def case(rows, C, kinds=KINDS):
    return make_case(rows, C, shift=rows % 10, kinds=kinds)


def all_cases():
    """every (rows, C, kinds) the GPU file builds its inputs from"""
    seen = []
    for rows in ROWS:
        for C, _, _ in C_CONFIGS:
            seen.append((rows, C, KINDS))
    for rows in LAYOUT_ROWS:
        seen.append((rows, LAYOUT_C, KINDS))
    for rows, _, C, _ in POOL_CASES:
        seen.append((rows, C, KINDS))
        seen.append((rows, C, NO_TIES))
    for rows, C in NAN_CASES:
        seen.append((rows, C, KINDS))
    return sorted(set(seen))
