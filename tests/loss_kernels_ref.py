"""TEST INFRASTRUCTURE: the loss and pose-glue operations of csrc/tdaloss.hip, csrc/dcd.hip and csrc/poserot.hip restated as plain
vectorised CPU torch, written from the reference's formulas that the kernel headers cite (losses/TDA_loss_sym_recon.py:205-450,
losses/consistency_loss.py:11-81, PoseNet9D.py:57-66), with every gradient by autograd.  Nothing here imports the project's losses.

Every operand is float32 data.  Each function evaluates in `dtype`: torch.float64 is the reference, torch.float32 the same
restatement at the kernels' precision ("oracle32"), which measures how far two correct float32 evaluations of that case may lie
apart.  The bar of the GPU tests is `bound()`: 4 * max|oracle32 - ref64| + 4 * eps32 * max|ref64| per output tensor.

Where float32 semantics decide a branch -- the smooth-L1 knee |x| >= beta, F.normalize's 1e-12 floor, the clamp to [-1 + 1e-6,
1 - 1e-6] in front of acos, "the row's weights sum to more than 0" -- the branch is decided ONCE, on a float32 evaluation, and the
float64 evaluation takes the same side (`Branches`).  Constants a kernel receives or holds as float32 (alpha, lambda, the clamp
bounds, the floors, n / m) are promoted from their float32 values.

Sign-dependent gradients (L1 terms): an element whose float64 difference is nonzero but within 16 * eps32 * max|operand| of zero may
take either sign in float32; `ambiguous()` marks those, and `excluded_share_ok` holds their share to 1e-3 per tensor.  A difference
that is exactly zero is NOT ambiguous: its gradient is exactly 0.
"""
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
EPS32 = float(torch.finfo(torch.float32).eps)
f32c = lambda v: float(np.float32(v))                                     # a constant as the float32 the kernels hold
FLOOR = f32c(1e-12)                                                        # F.normalize's eps
CLAMP_LO, CLAMP_HI = float(np.float32(-1.0) + np.float32(1e-6)), float(np.float32(1.0) - np.float32(1e-6))
SYM_CONF = f32c(1e-5)                                                      # the ground-truth x axis' confidence for symmetric objects
MAX_EXCLUDED = 1e-3


class Branches(object):
    """records each data-dependent branch mask of a float32 evaluation, replays them in order for the evaluation that counts"""

    def __init__(self):
        self.rec, self.pos, self.replay = [], 0, False

    def __call__(self, cond):
        if self.replay:
            m = self.rec[self.pos]
            self.pos += 1
            return m
        m = cond().detach()
        self.rec.append(m)
        return m


def _run(fn, floats, dtype, wrt=(), **kw):
    """fn(br, *floats, **kw) once in float32 to decide the branches, then in `dtype` with the tensors `wrt` as autograd leaves"""
    br = Branches()
    with torch.no_grad():
        fn(br, *[None if t is None else t.detach().to(F32) for t in floats], **kw)
    br.pos, br.replay = 0, True
    xs = [None if t is None else t.detach().to(F32).to(dtype) for t in floats]
    for i in wrt:
        xs[i].requires_grad_(True)
    return fn(br, *xs, **kw), xs


def _grads(scalar, leaves):
    gs = torch.autograd.grad(scalar, leaves, allow_unused=True)
    return [torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves)]


def bound(ref64, ora32):
    """the allowed deviation of a float32 kernel from ref64, per output tensor"""
    ref64, ora32 = ref64.detach().to(F64), ora32.detach().to(F64)
    if ref64.numel() == 0:
        return 0.0
    return 4.0 * float((ora32 - ref64).abs().max()) + 4.0 * EPS32 * float(ref64.abs().max())


def ambiguous(diff, *operands):
    """elements of a float64 difference whose sign float32 may not resolve: nonzero, within 16 eps32 max|operand| of zero"""
    top = max(float(o.detach().abs().max()) for o in operands)
    d = diff.detach()
    return (d != 0) & (d.abs() <= 16.0 * EPS32 * top)


def excluded_share_ok(mask):
    return mask.numel() == 0 or float(mask.double().mean()) <= MAX_EXCLUDED


# ---- pose terms (TDA_loss_sym_recon.py:205-290) ---------------------------------------------------------------------------------
def _rho(br, x, kind, beta):
    """nn.L1Loss (kind 0) / nn.SmoothL1Loss(beta) (kind 1), elementwise"""
    if kind == 0:
        return x.abs()
    knee = br(lambda: x.abs() >= beta)
    return torch.where(knee, x.abs() - 0.5 * beta, 0.5 * x * x / beta)


def _pose_terms(br, rot1, rot2, f1, f2, tran, size, g1, g2, gt, gs, sym=None, kind=0, beta=0.5):
    B, dt = rot1.shape[0], rot1.dtype
    s0 = sym[:, 0]
    valid = (s0 != 1).to(dt)                                  # Rot2 / Rot2_cos / Rot_regular skip the objects symmetric about y ...
    red = (s0 == 0).to(dt)                                    # ... the red half of R_con takes sym0 == 0 only, over the whole batch
    nv = valid.sum()
    dv = torch.clamp(nv, min=1.0)
    rho = lambda x: _rho(br, x, kind, beta)
    d12 = (rot1 * rot2).sum(1)
    cg = torch.exp(-13.7 * (rot1 - g1).norm(dim=1) ** 2) - f1
    cr = torch.exp(-13.7 * (rot2 - g2).norm(dim=1) ** 2) - f2
    out = torch.stack([rho(rot1 - g1).mean(), ((1 - (rot1 * g1).sum(1)) * 2).mean(), (valid * rho(rot2 - g2).mean(1)).sum() / dv,
                       (valid * (1 - (rot2 * g2).sum(1)) * 2).sum() / dv, (valid * d12.abs()).sum() / dv, rho(tran - gt).mean(),
                       rho(size - gs).mean(), rho(cg).mean() + (red * rho(cr)).sum() / B, nv])
    return out, {"d12": d12, "cg": cg, "cr": cr}


def pose_terms(pred, gt, sym, kind=0, beta=0.5, gw=None, dtype=F64):
    """pred = (rot1, rot2, f1, f2, tran, size), gt = (rot1, rot2, tran, size), sym (B, S) integers -> out (9,): Rot1, Rot1_cos, Rot2,
    Rot2_cos, Rot_regular, Tran, Size, R_con and the number of objects with sym0 != 1; with gw (8,) also the gradients of
    sum_k gw[k] out[k] w.r.t. the six predictions and, per gradient, the mask of elements whose sign is ambiguous"""
    (out, aux), xs = _run(_pose_terms, list(pred) + list(gt), dtype, wrt=range(6) if gw is not None else (), sym=sym, kind=kind,
                          beta=f32c(beta))
    if gw is None:
        return out.detach()
    grads = _grads((out[:8] * gw.detach().to(F32).to(dtype)).sum(), xs[:6])
    rot1, rot2, f1, f2, tran, size, g1, g2, gt_, gs = [x.detach() for x in xs]
    reg = ambiguous(aux["d12"], rot1, rot2).unsqueeze(1)
    amb = [reg.expand(-1, 3).clone(), reg.expand(-1, 3).clone(), torch.zeros_like(f1, dtype=torch.bool),
           torch.zeros_like(f2, dtype=torch.bool), torch.zeros_like(tran, dtype=torch.bool), torch.zeros_like(size, dtype=torch.bool)]
    if kind == 0:
        ag, ar = ambiguous(aux["cg"], f1, torch.ones(1)), ambiguous(aux["cr"], f2, torch.ones(1))
        amb[0] |= ambiguous(rot1 - g1, rot1, g1) | ag.unsqueeze(1)
        amb[1] |= ambiguous(rot2 - g2, rot2, g2) | ar.unsqueeze(1)
        amb[2], amb[3] = ag, ar
        amb[4], amb[5] = ambiguous(tran - gt_, tran, gt_), ambiguous(size - gs, size, gs)
    return out.detach(), grads, amb


# ---- prop_sym_matching_loss (consistency_loss.py:19-81) ---------------------------------------------------------------------------
def sym_mode(sym, sym_cols):
    """per object: 0 identity, 1 half turn about y, 2 mirror z -> -z, 3 target zero and the reconstruction kept, 4 both sides zero"""
    sym = sym.long()
    s0, rest = sym[:, 0], sym[:, 1:sym_cols].sum(1)
    s1 = sym[:, 1] if sym_cols > 1 else torch.zeros_like(s0)
    mode = torch.full_like(s0, 3)
    mode[(s0 == 1) & (rest > 0)] = 1
    mode[(s0 == 1) & (rest == 0)] = 4
    mode[(s0 == 0) & (s1 == 1)] = 2
    mode[(s0 == 0) & (s1 != 1)] = 0
    return mode


_FLIPS = [[1.0, 1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, 1.0, -1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]


def _sym_recon(br, PC, PC_re, R, t, sym=None, sym_cols=4):
    mode = sym_mode(sym, sym_cols)
    cano = torch.matmul(PC - t.unsqueeze(1), R)                                        # rows = R^T (p - t)
    flip = torch.tensor(_FLIPS, dtype=PC.dtype)[mode].unsqueeze(1)
    posed = torch.matmul(cano * flip, R.transpose(1, 2)) + t.unsqueeze(1)
    m = mode.view(-1, 1, 1)
    zero = torch.zeros_like(PC)
    tgt = torch.where(m == 0, PC, torch.where(m >= 3, zero, posed))
    rec = torch.where(m == 4, zero, PC_re)
    return (tgt - rec).abs().mean(), tgt, rec, mode


def sym_recon(PC, PC_re, gt_R, gt_t, sym, sym_cols=None, gloss=None, dtype=F64):
    """-> loss (scalar); with gloss (1,) also d PC, d PC_re and the masks of their sign-ambiguous elements"""
    sym_cols = sym.shape[1] if sym_cols is None else sym_cols
    (loss, tgt, rec, mode), xs = _run(_sym_recon, [PC, PC_re, gt_R, gt_t], dtype, wrt=(0, 1) if gloss is not None else (), sym=sym,
                                      sym_cols=sym_cols)
    if gloss is None:
        return loss.detach()
    grads = _grads(loss * gloss.detach().to(F32).to(dtype).reshape(()), xs[:2])
    live = (mode != 4).view(-1, 1, 1)
    amb_re = ambiguous(tgt - rec, tgt, rec) & live
    m = mode.view(-1, 1, 1)
    amb_pc = torch.where(m == 0, amb_re, torch.where(m >= 3, torch.zeros_like(amb_re), amb_re.any(dim=2, keepdim=True).expand_as(amb_re)))
    return loss.detach(), grads, [amb_pc, amb_re]


# ---- ph_loss_fn (TDA_loss_sym_recon.py:292-298) ----------------------------------------------------------------------------------
def _rowl1(br, a, b, wsrc):
    w = br(lambda: wsrc.sum(1, keepdim=True) > 0).to(a.dtype)
    return ((a - b).abs() * w).mean(), w


def rowl1(a, b, wsrc, gout=None, dtype=F64):
    """mean(|a - b| * w), w = 1 on the rows whose wsrc sums to more than 0 -> (loss, live, w (B,)[, d a, ambiguous]).  As the kernel
    header states the reference's NaN / Inf branch: the loss is NaN when `a` holds a NaN / Inf, 0 when only `b` does; in both the
    backward is dead (live = 0, d a = 0)."""
    bad_a, bad_b = not bool(torch.isfinite(a).all()), not bool(torch.isfinite(b).all())
    clean = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    (loss, w), xs = _run(_rowl1, [clean(a), clean(b), wsrc], dtype, wrt=(0,) if gout is not None else ())
    live = 0.0 if (bad_a or bad_b) else 1.0
    if bad_a or bad_b:
        value = torch.tensor(float("nan") if bad_a else 0.0, dtype=dtype)
    else:
        value = loss.detach()
    res = (value, live, w.detach().reshape(-1))
    if gout is None:
        return res
    if live:
        da = _grads(loss * gout.detach().to(F32).to(dtype).reshape(()), xs[:1])[0]
    else:
        da = torch.zeros_like(xs[0])
    amb = ambiguous(xs[0] - xs[1], xs[0], xs[1]) & (w.detach() > 0) & bool(live)
    return res + (da, amb)


# ---- feat_consistency_loss (consistency_loss.py:11-16) -----------------------------------------------------------------------------
def _feat(br, x1, x2):
    def normalize(x):                                                                 # F.normalize: x / max(|x|, 1e-12)
        n = x.norm(dim=1, keepdim=True)
        floor = br(lambda: n <= FLOOR)
        return x / torch.where(floor, torch.full_like(n, FLOOR), n)
    return 2 - 2 * (normalize(x1) * normalize(x2)).sum() / x1.shape[0]


def feat_consistency(x1, x2, gloss=None, dtype=F64):
    loss, xs = _run(_feat, [x1, x2], dtype, wrt=(0, 1) if gloss is not None else ())
    if gloss is None:
        return loss.detach()
    return loss.detach(), _grads(loss * gloss.detach().to(F32).to(dtype).reshape(()), xs)


# ---- calc_dcd after the Chamfer search (TDA_loss_sym_recon.py:411-450) ---------------------------------------------------------------
def _dcd(br, d1, d2, idx1=None, idx2=None, alpha=70.0, lam=0.3, non_reg=False):
    (B, n), m, dt = d1.shape, d2.shape[1], d1.dtype
    frac_12, frac_21 = n / m, m / n
    if non_reg:
        frac_12, frac_21 = max(1.0, frac_12), max(1.0, frac_21)
    idx1, idx2 = idx1.long(), idx2.long()
    cnt1 = torch.stack([torch.bincount(idx1[b], minlength=m)[idx1[b]] for b in range(B)]).to(dt)
    cnt2 = torch.stack([torch.bincount(idx2[b], minlength=n)[idx2[b]] for b in range(B)]).to(dt)
    w1 = (1.0 / (cnt1 ** lam + 1e-6) * f32c(frac_21)).detach()
    w2 = (1.0 / (cnt2 ** lam + 1e-6) * f32c(frac_12)).detach()
    loss = (1.0 - torch.exp(-d1 * alpha) * w1).mean(1) + 0.5 * (1.0 - torch.exp(-d2 * alpha) * w2).mean(1)
    return loss, w1, w2


def dcd(dist1, dist2, idx1, idx2, alpha, lam, non_reg=False, gloss=None, dtype=F64):
    """-> loss (B,), w1 (B, n), w2 (B, m) [, d dist1, d dist2 of sum_b gloss[b] loss[b], the weights detached]"""
    (loss, w1, w2), xs = _run(_dcd, [dist1, dist2], dtype, wrt=(0, 1) if gloss is not None else (), idx1=idx1, idx2=idx2,
                              alpha=f32c(alpha), lam=f32c(lam), non_reg=non_reg)
    if gloss is None:
        return loss.detach(), w1, w2
    return loss.detach(), w1, w2, _grads((loss * gloss.detach().to(F32).to(dtype)).sum(), xs)


# ---- R_DCD's canonicalisation (TDA_loss_sym_recon.py:326-408) -------------------------------------------------------------------------
def _pose_transform(br, points, R, t, s):
    return torch.matmul(points - t.unsqueeze(1), R) * s.unsqueeze(1)                  # rows = (R^T (p - t)) * s


def pose_transform(points, R, t, s, dout=None, dtype=F64):
    """-> out (B, n, 3) [, (d points, d R, d t, d s)]"""
    out, xs = _run(_pose_transform, [points, R, t, s], dtype, wrt=range(4) if dout is not None else ())
    if dout is None:
        return out.detach()
    return out.detach(), _grads((out * dout.detach().to(F32).to(dtype)).sum(), xs)


def _axis_angle_matrix(k, s, c):
    """to_rot_matrix_in_batch (:398-408)"""
    kx, ky, kz = k[:, 0:1], k[:, 1:2], k[:, 2:3]
    oc = 1 - c
    rows = [torch.cat([kx * kx * oc + c, kx * ky * oc - kz * s, kx * kz * oc + ky * s], -1),
            torch.cat([ky * kx * oc + kz * s, ky * ky * oc + c, ky * kz * oc - kx * s], -1),
            torch.cat([kx * kz * oc - ky * s, kz * ky * oc + kx * s, kz * kz * oc + c], -1)]
    return torch.stack(rows, dim=-2)


def _vertical_axes(br, c1, c2, y, z):
    """get_vertical_rot_vec_in_batch (:370-395): rotate y and z about their common normal until they are perpendicular, each by the
    share of the OTHER axis' confidence"""
    c1, c2 = c1.unsqueeze(-1), c2.unsqueeze(-1)
    k = torch.cross(y, z, dim=-1)
    k = k / (torch.norm(k, dim=-1, keepdim=True) + 1e-8)
    dot = (y * z).sum(-1, keepdim=True)
    lo, hi = br(lambda: dot < CLAMP_LO), br(lambda: dot > CLAMP_HI)
    cs = torch.where(lo, torch.full_like(dot, CLAMP_LO), torch.where(hi, torch.full_like(dot, CLAMP_HI), dot))
    theta = torch.acos(cs)
    th2 = c1 / (c1 + c2) * (theta - math.pi / 2)
    th1 = c2 / (c1 + c2) * (theta - math.pi / 2)
    ny = torch.matmul(_axis_angle_matrix(k, torch.sin(th1), torch.cos(th1)), y.unsqueeze(-1)).squeeze(-1)
    nz = torch.matmul(_axis_angle_matrix(k, torch.sin(-th2), torch.cos(-th2)), z.unsqueeze(-1)).squeeze(-1)
    return ny, nz


def _normalize3(br, v):
    n = v.norm(dim=-1, keepdim=True)
    floor = br(lambda: n < FLOOR)
    return v / torch.where(floor, torch.full_like(n, FLOOR), n)


def _rot_from_y_x(br, y, x):
    """get_rot_mat_y_first (:351-360)"""
    y = _normalize3(br, y)
    z = _normalize3(br, torch.cross(x, y, dim=-1))
    return torch.stack((torch.cross(y, z, dim=-1), y, z), dim=-1)


def _pose_rotation(br, gR0, p_g, f_g, p_r, f_r, sym0=None):
    """:327-333: objects symmetric about y pair the green axis with the ground truth's x axis at confidence 1e-5"""
    flag = sym0 == 1
    x_in = torch.where(flag.unsqueeze(-1), gR0, p_r)
    c2 = torch.where(flag, torch.full_like(f_r, SYM_CONF), f_r)
    y, x = _vertical_axes(br, f_g, c2, p_g, x_in)
    return _rot_from_y_x(br, y, x)


def vertical_axes(c1, c2, y, z, dtype=F64):
    (ny, nz), _ = _run(_vertical_axes, [c1, c2, y, z], dtype)
    return ny, nz


def pose_rotation(gR0, p_g, f_g, p_r, f_r, sym0, dR=None, dtype=F64):
    """gR0 (B, 3) = g_R[:, :, 0], sym0 (B,) -> R (B, 3, 3) [, d in (B, 8) = (d p_g, d f_g, d p_r, d f_r) of sum(R * dR)]"""
    R, xs = _run(_pose_rotation, [gR0, p_g, f_g, p_r, f_r], dtype, wrt=range(1, 5) if dR is not None else (), sym0=sym0)
    if dR is None:
        return R.detach()
    g = _grads((R * dR.detach().to(F32).to(dtype)).sum(), xs[1:])
    return R.detach(), torch.cat([g[0], g[1].unsqueeze(1), g[2], g[3].unsqueeze(1)], dim=1)


def _canonicalize(br, points, gR0, p_g, f_g, p_r, f_r, p_t, p_s, sym0=None):
    R = _pose_rotation(br, gR0, p_g, f_g, p_r, f_r, sym0=sym0)
    return _pose_transform(br, points, R, p_t, p_s), R


def canonicalize(points, gR, p_g, f_g, p_r, f_r, p_t, p_s, sym, dtype=F64):
    """R_DCD's pose normalisation -> (points_re_n (B, n, 3), R (B, 3, 3))"""
    (out, R), _ = _run(_canonicalize, [points, gR[..., 0], p_g, f_g, p_r, f_r, p_t, p_s], dtype, sym0=sym.reshape(sym.shape[0], -1)[:, 0])
    return out, R


def _generate_rt(br, p_g, p_r, f_g, f_r, T, sym0=None):
    """generate_RT(mode='vec'): the red confidence is zeroed for objects symmetric about y; RT = [[R, T], [0 0 0 1]]"""
    if sym0 is not None:
        f_r = torch.where(sym0 == 1, torch.zeros_like(f_r), f_r)
    y, x = _vertical_axes(br, f_g, f_r, p_g, p_r)
    R = _rot_from_y_x(br, y, x)
    B = R.shape[0]
    top = torch.cat([R, T.unsqueeze(-1)], dim=-1)
    last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=R.dtype).expand(B, 1, 4)
    return torch.cat([top, last], dim=1)


def generate_rt(p_g, p_r, f_g, f_r, T, sym=None, dtype=F64):
    rt, _ = _run(_generate_rt, [p_g, p_r, f_g, f_r, T], dtype, sym0=None if sym is None else sym.reshape(sym.shape[0], -1)[:, 0])
    return rt


# ---- PoseNet9D.py:57-66 ----------------------------------------------------------------------------------------------------------
def _head_post(br, green, red, ts, mean):
    axis = lambda v: v[:, 1:4] / (torch.norm(v[:, 1:4], dim=1, keepdim=True) + 1e-6)
    return (axis(green), axis(red), torch.sigmoid(green[:, 0]), torch.sigmoid(red[:, 0]), ts[:, :3] + mean, ts[:, 3:6])


def head_post(green, red, ts, mean, grads=None, dtype=F64):
    """green / red (B, 4) = (confidence logit, x, y, z), ts (B, 6) -> (p_green, p_red, f_green, f_red, T, s)
    [, (d green, d red, d ts) for the gradients `grads` of the six outputs, None = zero]"""
    outs, xs = _run(_head_post, [green, red, ts, mean], dtype, wrt=range(3) if grads is not None else ())
    if grads is None:
        return tuple(o.detach() for o in outs)
    total = sum((o * g.detach().to(F32).to(dtype)).sum() for o, g in zip(outs, grads) if g is not None)
    return tuple(o.detach() for o in outs), _grads(total + 0.0 * xs[0].sum(), xs[:3])
