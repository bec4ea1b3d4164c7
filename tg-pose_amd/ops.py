"""Tensor-level wrappers over the C ABI: pointer/stride plumbing only, no compute.

Every function enqueues HIP kernels on torch's current stream of the tensors' device and returns
device tensors; nothing synchronises.  Inputs must be fp32 (indices int32), on a GPU, with the
layouts documented in include/tgpose.h -- violations raise instead of being silently copied.
"""
import ctypes
import functools
import os
import math

import torch

from . import _lib
from ._lib import GemmArgs, check


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


# bench.py sets this to a dict to time, with HIP events on the launch stream, every launch of the graph / HBM-bound kernel
# class (kNN, graph convolution, ORL pooling, pooling, gathers, row sort, tails, per-object post-processing): class name ->
# list of (start event, end event).  None (the default) adds nothing to a call.
CLASS_TIMER = None


def _timed(cls):
    def deco(fn):
        @functools.wraps(fn)
        def wrap(*a, **kw):
            if CLASS_TIMER is None:
                return fn(*a, **kw)
            st = torch.cuda.current_stream(next(t for t in a if torch.is_tensor(t)).device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            r = fn(*a, **kw)
            e1.record(st)
            CLASS_TIMER.setdefault(cls, []).append((e0, e1, fn.__name__))
            return r
        return wrap
    return deco


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _f32(t, name, dims=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise TypeError("%s must be a float32 GPU tensor" % name)
    if dims is not None and t.dim() != dims:
        raise ValueError("%s must have %d dims" % (name, dims))
    return t


def _rows(t, name):
    """(…, C) tensor whose rows are contiguous; returns (tensor, row stride in elements)."""
    _f32(t, name)
    if t.stride(-1) != 1:
        raise ValueError("%s: last dim must be contiguous" % name)
    ld = t.stride(-2)
    if t.dim() == 3 and t.stride(0) != t.shape[1] * ld:
        raise ValueError("%s: batch stride must equal n * row stride" % name)
    return t, ld


def _i32(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise TypeError("%s must be a contiguous int32 GPU tensor" % name)
    return t


def graph_node_counts(raw_graph):
    """(kernel, memcpy, memset, other) node counts of a captured hipGraph; raw_graph = torch.cuda.CUDAGraph(keep_graph=True)
    .raw_cuda_graph() after the capture (host-only census, tgp_graph_node_counts)"""
    counts = (ctypes.c_int * 4)()
    check(_lib.lib().tgp_graph_node_counts(ctypes.c_void_p(int(raw_graph)), counts), "tgp_graph_node_counts")
    return tuple(int(c) for c in counts)


@_timed("graph")
def center(points, zero=None):
    """points (B,n,3) -> (xyz_c (B,n,3), mean (B,3)); zero (a contiguous 4-byte tensor): cleared by the same launch"""
    _f32(points, "points", 3)
    points = points.contiguous()
    B, n, _ = points.shape
    xyz = torch.empty_like(points)
    mean = torch.empty(B, 3, device=points.device, dtype=torch.float32)
    if zero is not None:
        if not zero.is_contiguous() or zero.element_size() != 4 or zero.device != points.device:
            raise ValueError("center: zero must be a contiguous 4-byte tensor on the points' device")
        check(_lib.lib().tgp_center_zero(_p(points), B, n, _p(xyz), _p(mean), _p(zero), zero.numel(), _stream(points)), "tgp_center_zero")
        return xyz, mean
    check(_lib.lib().tgp_center(_p(points), B, n, _p(xyz), _p(mean), _stream(points)), "tgp_center")
    return xyz, mean


@_timed("graph")
def knn_xyz(xyz, k):
    """xyz (B,n,3) contiguous -> idx (B,n,k) int32"""
    _f32(xyz, "xyz", 3)
    if not xyz.is_contiguous() or xyz.shape[2] != 3:
        raise ValueError("xyz must be contiguous (B,n,3)")
    B, n, _ = xyz.shape
    idx = torch.empty(B, n, k, device=xyz.device, dtype=torch.int32)
    check(_lib.lib().tgp_knn_xyz(_p(xyz), B, n, int(k), _p(idx), _stream(xyz)), "tgp_knn_xyz")
    return idx


@_timed("graph")
def knn_feat(feat, k, workspace=None, xyz=None):
    """feat (B,n,d) rows contiguous (row stride may exceed d) -> idx (B,n,k) int32.
    xyz (B,n,3): returns (idx, dirs) -- dirs (B,n,k,4) the unit directions to the selected neighbours (tgp_knn_feat_dirs: written by
    the selecting waves; gconv_hs(dirs=...) takes them) or None where the fused kernel does not serve the shape."""
    feat, ld = _rows(feat, "feat")
    B, n, d = feat.shape
    need = _lib.lib().tgp_knn_feat_workspace_bytes(B, n, d)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 3) // 4, device=feat.device, dtype=torch.float32)
    idx = torch.empty(B, n, k, device=feat.device, dtype=torch.int32)
    if xyz is not None:
        _f32(xyz, "xyz", 3)
        dirs = torch.empty(B, n, k, 4, device=feat.device, dtype=torch.float32)
        rc = _lib.lib().tgp_knn_feat_dirs(_p(feat), ld, B, n, d, int(k), _p(idx), _p(workspace), workspace.numel() * workspace.element_size(),
                                          _p(xyz.contiguous()), _p(dirs), _stream(feat))
        if rc == 0:
            return idx, dirs
        if rc != -2:
            check(rc, "tgp_knn_feat_dirs")
        dirs = None
    check(_lib.lib().tgp_knn_feat(_p(feat), ld, B, n, d, int(k), _p(idx), _p(workspace), workspace.numel() * workspace.element_size(),
                                  _stream(feat)), "tgp_knn_feat")
    return idx if xyz is None else (idx, None)


@_timed("graph")
def nn1(target, source):
    """(B,n,3),(B,m,3) -> idx (B,n) int32"""
    _f32(target, "target", 3), _f32(source, "source", 3)
    target, source = target.contiguous(), source.contiguous()
    B, n, _ = target.shape
    m = source.shape[1]
    idx = torch.empty(B, n, device=target.device, dtype=torch.int32)
    check(_lib.lib().tgp_nn1(_p(target), _p(source), B, n, m, _p(idx), _stream(target)), "tgp_nn1")
    return idx


def nn1_pair(target, source1, source2, tail=None):
    """nn1(target, source1), nn1(target, source2) in one launch; tail = (obj_id (B,) float, feat (B,n,ld), col0, n_cls): the launch
    also writes fill_tail(obj_id, target, feat, col0, n_cls)"""
    for t, nm in ((target, "target"), (source1, "source1"), (source2, "source2")):
        _f32(t, nm, 3)
    target, source1, source2 = target.contiguous(), source1.contiguous(), source2.contiguous()
    B, n, _ = target.shape
    i1 = torch.empty(B, n, device=target.device, dtype=torch.int32)
    i2 = torch.empty(B, n, device=target.device, dtype=torch.int32)
    obj_id, feat, col0, n_cls, ld = None, None, 0, 0, 0
    if tail is not None:
        obj_id, feat, col0, n_cls = tail
        feat, ld = _rows(feat, "feat")
        if tuple(feat.shape[:2]) != (B, n) or obj_id.numel() != B or not obj_id.is_contiguous() or obj_id.dtype != torch.float32:
            raise ValueError("nn1_pair: tail = (obj_id (B,) float32, feat (B,n,ld), col0, n_cls)")
    check(_lib.lib().tgp_nn1_pair_tail(_p(target), _p(source1), _p(source2), B, n, source1.shape[1], source2.shape[1], _p(i1), _p(i2),
                                       _p(obj_id), int(n_cls), _p(feat), ld, int(col0), _stream(target)), "tgp_nn1_pair_tail")
    return i1, i2


def normalize_dirs(directions):
    _f32(directions, "directions", 2)
    directions = directions.contiguous()
    out = torch.empty_like(directions)
    check(_lib.lib().tgp_normalize_dirs(_p(directions), directions.shape[1], _p(out), _stream(directions)),
          "tgp_normalize_dirs")
    return out


def normalize_dirs_bwd(directions, grad):
    directions, grad = directions.contiguous(), grad.contiguous()
    out = torch.empty_like(directions)
    check(_lib.lib().tgp_normalize_dirs_bwd(_p(directions), _p(grad), directions.shape[1], _p(out), _stream(directions)),
          "tgp_normalize_dirs_bwd")
    return out


@_timed("graph")
def gconv_surface(xyz, idx, sdn, S, C, out=None, xyz_pad=False):
    """xyz_pad: `out` is a (B, n, C) view of a buffer whose rows are at least C + 4 floats long; columns C..C+3 of every row
    receive the point (x, y, z, 0) -- the STE convolution's operand for the layer's last GEMM"""
    _f32(xyz, "xyz", 3), _i32(idx, "idx")
    B, n, k = idx.shape
    if out is None:
        out = torch.empty(B, n, C, device=xyz.device, dtype=torch.float32)
    out, ldo = _rows(out, "out")
    check(_lib.lib().tgp_gconv_surface_fwd(_p(xyz), _p(idx), _p(sdn), B, n, k, S, C, _p(out), ldo, 1 if xyz_pad else 0,
                                           _stream(xyz)), "tgp_gconv_surface_fwd")
    return out


@_timed("graph")
def gconv_hs(xyz, idx, proj, sdn, S, C, out=None, dirs=None):
    """dirs (B,n,k,4): the unit neighbour directions knn_feat(xyz=...) left beside idx (no direction launch)"""
    _f32(xyz, "xyz", 3), _i32(idx, "idx")
    proj, ldp = _rows(proj, "proj")
    B, n, k = idx.shape
    if out is None:
        out = torch.empty(B, n, C, device=xyz.device, dtype=torch.float32)
    out, ldo = _rows(out, "out")
    if dirs is not None:
        if tuple(dirs.shape) != (B, n, k, 4) or not dirs.is_contiguous():
            raise ValueError("gconv_hs: dirs (B,n,k,4) contiguous expected")
        rc = _lib.lib().tgp_gconv_hs_fwd_dirs(_p(xyz), _p(idx), _p(proj), ldp, _p(sdn), B, n, k, S, C, _p(out), ldo, _p(dirs), _stream(xyz))
        if rc == 0:
            return out
        if rc != -2:
            check(rc, "tgp_gconv_hs_fwd_dirs")
    # scratch for the unit neighbour directions: only the LDS-staged kernel (pooled levels) uses it
    dirs = torch.empty(B * n * k * 4, device=xyz.device, dtype=torch.float32) if n * 7 * 8 * 4 <= 72 * 1024 else None
    check(_lib.lib().tgp_gconv_hs_fwd(_p(xyz), _p(idx), _p(proj), ldp, _p(sdn), B, n, k, S, C, _p(out), ldo,
                                      _p(dirs), _stream(xyz)), "tgp_gconv_hs_fwd")
    return out


@_timed("graph")
def orl_global(feat, idx):
    """feat (B,n,C), idx (B,n,k) -> (B,C)"""
    feat, ldf = _rows(feat, "feat")
    _i32(idx, "idx")
    B, n, C = feat.shape
    k = idx.shape[2]
    partial = torch.empty(_lib.lib().tgp_orl_partial_floats(B, n, C), device=feat.device, dtype=torch.float32)
    out = torch.empty(B, C, device=feat.device, dtype=torch.float32)
    check(_lib.lib().tgp_orl_global(_p(feat), ldf, _p(idx), B, n, k, C, _p(partial), _p(out), _stream(feat)),
          "tgp_orl_global")
    return out


@_timed("graph")
def orl_rowbias(feat, idx, w2t, planes=None, xyz_tile=None, tickets=None):
    """feat (B,n,C), idx (B,n,k), w2t (C,C) = W2^T -> rb (B,C) = mean_i max_j feat[idx] @ W2^T.
    planes (a Planes of B*n rows): feat is also written as fp16 planes -- it is the A operand of the layer's last GEMM -- by the
    kernel that stages it in LDS anyway (tgp_orl_rowbias_planes; xyz_tile (B,n,3): one more K-tile (x, y, z, 0 ...) behind the C
    channels).  Returns (rb, planes or None): None where that form does not serve the shape and nothing was written.
    tickets (B int32 zeros, handed back as zeros): the one-launch form (tgp_orl_rowbias_fused) where the shape allows."""
    feat, ldf = _rows(feat, "feat")
    _i32(idx, "idx")
    B, n, C = feat.shape
    k = idx.shape[2]
    rb = torch.empty(B, C, device=feat.device, dtype=torch.float32)
    if tickets is not None and ORL_FUSED:
        contrib = torch.empty(B * (C // 16) * C, device=feat.device, dtype=torch.float32)
        rc = _lib.lib().tgp_orl_rowbias_fused(_p(feat), ldf, _p(idx), B, n, k, C, _p(w2t), None, _p(rb),
                                              _p(planes.buf) if planes is not None else None, planes.kt if planes is not None else 0,
                                              _p(planes.amax) if planes is not None else None, _p(xyz_tile), _p(contrib), _p(tickets),
                                              _stream(feat))
        if rc == 0:
            return (rb, planes) if planes is not None else rb
        if rc != -2:
            check(rc, "tgp_orl_rowbias_fused")
    partial = torch.empty(_lib.lib().tgp_orl_partial_floats(B, n, C), device=feat.device, dtype=torch.float32)
    if planes is not None:
        rc = _lib.lib().tgp_orl_rowbias_planes(_p(feat), ldf, _p(idx), B, n, k, C, _p(partial), _p(w2t), None, _p(rb), _p(planes.buf),
                                               planes.kt, _p(planes.amax), _p(xyz_tile), _stream(feat))
        if rc == 0:
            return rb, planes
        if rc != -2:
            check(rc, "tgp_orl_rowbias_planes")
    check(_lib.lib().tgp_orl_rowbias(_p(feat), ldf, _p(idx), B, n, k, C, _p(partial), _p(w2t), None, _p(rb), _stream(feat)),
          "tgp_orl_rowbias")
    return (rb, None) if planes is not None else rb


@_timed("graph")
def pool(xyz, feat, idx, sample, kpool=4, out_f=None, planes=None):
    """xyz (B,n,3), feat (B,n,C), idx (B,n,>=kpool) int32, sample (n_out,) int32 -> (xyz_p, feat_p); planes (a Planes of B*n_out
    rows): feat_p also as fp16 planes, by the same kernel where the shape allows, else by a split of the result"""
    _f32(xyz, "xyz", 3)
    feat, ldf = _rows(feat, "feat")
    _i32(idx, "idx"), _i32(sample, "sample")
    B, n, C = feat.shape
    n_out = sample.numel()
    out_xyz = torch.empty(B, n_out, 3, device=xyz.device, dtype=torch.float32)
    if out_f is None:
        out_f = torch.empty(B, n_out, C, device=xyz.device, dtype=torch.float32)
    out_f, ldo = _rows(out_f, "out_f")
    if planes is not None:
        rc = _lib.lib().tgp_pool_fwd_planes(_p(xyz), _p(feat), ldf, _p(idx), idx.shape[2], _p(sample), B, n, n_out, kpool, C,
                                            _p(out_xyz), _p(out_f), ldo, _p(planes.buf), planes.kt, _p(planes.amax), _stream(xyz))
        if rc == 0:
            return out_xyz, out_f
        if rc != -2:
            check(rc, "tgp_pool_fwd_planes")
    check(_lib.lib().tgp_pool_fwd(_p(xyz), _p(feat), ldf, _p(idx), idx.shape[2], _p(sample), B, n, n_out, kpool, C,
                                  _p(out_xyz), _p(out_f), ldo, _stream(xyz)), "tgp_pool_fwd")
    if planes is not None:
        planes_split.__wrapped__(out_f.view(B * n_out, -1), K=C, out=planes)
    return out_xyz, out_f


@_timed("graph")
def gather_rows(src, idx, dst):
    """dst[b,i,:C] = src[b, idx[b,i], :C]; src (B,n_src,C), idx (B,n_out) int32, dst (B,n_out,C) view"""
    src, lds = _rows(src, "src")
    dst, ldd = _rows(dst, "dst")
    _i32(idx, "idx")
    B, n_src, C = src.shape
    n_out = idx.shape[1]
    check(_lib.lib().tgp_gather_rows(_p(src), lds, _p(idx), B, n_src, n_out, C, _p(dst), ldd, _stream(src)),
          "tgp_gather_rows")
    return dst


@_timed("graph")
def sort_by_parent(near1, near2, n1, n2):
    """Rows of each object sorted by (near2, near1), ties in point order (= torch.argsort(near2 * n1 + near1, stable=True)).
    near1, near2 (B,n) int32 -> order (B,n) int32, order64 (B,n) int64, near1 + b*n1 and near2 + b*n2 in the sorted order."""
    _i32(near1, "near1"), _i32(near2, "near2")
    B, n = near1.shape
    if near2.shape != (B, n):
        raise ValueError("sort_by_parent: near1 and near2 must both be (B,n)")
    order, o1, o2 = torch.empty_like(near1), torch.empty_like(near1), torch.empty_like(near1)
    order64 = torch.empty(B, n, device=near1.device, dtype=torch.int64)
    check(_lib.lib().tgp_sort_by_parent(_p(near1), _p(near2), B, n, n1, n2, _p(order), _p(order64), _p(o1), _p(o2), _stream(near1)),
          "tgp_sort_by_parent")
    return order, order64, o1, o2


@_timed("graph")
def fill_tail(obj_id, xyz_c, feat, col0, n_cls):
    _f32(obj_id, "obj_id"), _f32(xyz_c, "xyz_c", 3)
    feat, ld = _rows(feat, "feat")
    B, n, _ = xyz_c.shape
    check(_lib.lib().tgp_fill_tail(_p(obj_id.contiguous()), _p(xyz_c), B, n, n_cls, _p(feat), ld, col0, _stream(feat)),
          "tgp_fill_tail")


# How launches large enough for the tile kernels run when the caller supplies pre-split weights:
#   "split16"  two-term fp16 operand split, 3 MFMA terms (products to ~2^-22; operands must stay below 65504)
#   "split"    three-term bf16 operand split, 6 MFMA terms (fp32 range, products to ~2^-23)
#   "fp32"     always the fp32 MFMA kernels
# split_w() packs weights for the mode current at pack time; gemm() reads the kind off the packed tensor's shape.
GEMM_MODE = "split16"
PLANES = os.environ.get("TGP_PLANES", "1") != "0"     # activations also as fp16 planes, consumers on the pre-split kernel (split16 mode)
ORL_FUSED = os.environ.get("TGP_ORL_FUSED", "1") != "0"      # the ORL pooling, its mean and its projection as one launch
HEADS_PLANES = os.environ.get("TGP_HEADS_PLANES", "1") != "0"   # measurement switch of the fused kernels: fragments from the fine planes


FP16_SAFE = 32768.0          # |w| at or above this is pre-scaled before the fp16 split (fp16's largest finite value is 65504)


def split_w(W, check=True):
    """Pack-time operand split of a weight for the tile GEMM kernels, in the current GEMM_MODE.
    check (fp16 split only): fp16 holds magnitudes below 65504, so the weight's largest magnitude is read back ONCE here (pack time
    is outside every timed or captured region) and a weight that reaches 2^15 is split as W * 2^-k with the power of two 2^k
    attached to the result (``.tgp_unscale``, a device scalar that ops.gemm hands to the kernel as c_scale: the accumulated sums
    are multiplied back, exactly).  check=False is for splits made INSIDE a captured step (the training path splits the live
    parameters every step): nothing may be read back there, and a parameter beyond fp16's range gives inf / NaN, which the
    trainer's NaN test (trainer/RL_TDA.py:217) sees.  Activations need no such care: the kernels guard them tile by tile."""
    if GEMM_MODE != "split16":
        return split_bf16(W)
    if not check:
        return split_f16(W)
    amax = float(W.detach().abs().max()) if W.numel() else 0.0
    if not (amax >= FP16_SAFE) or not math.isfinite(amax):
        return split_f16(W)
    k = math.frexp(amax)[1] - 15                     # amax * 2^-k lies in [2^14, 2^15)
    out = split_f16(W * (2.0 ** -k))
    out.tgp_unscale = torch.full((1,), 2.0 ** k, device=W.device, dtype=torch.float32)
    return out


def split_rows(ws, a, b=None):
    """rows [a, b) of a pack-time split weight, keeping the power of two a pre-scaled weight carries (split_w's .tgp_unscale is a
    Python attribute that plain slicing would drop: the product would silently come out 2^k too small)"""
    out = ws[a:b]
    unscale = getattr(ws, "tgp_unscale", None)
    if unscale is not None:
        out.tgp_unscale = unscale
    return out


def split_f16(W):
    """W (..., rows, K) fp32 -> int16 tensor (..., rows, ldo // 16, 2, 16) of fp16 bit patterns (hi, lo per K-tile)."""
    W = W.contiguous()
    K = W.shape[-1]
    rows = W.numel() // K
    ldo = (K + 15) // 16 * 16
    out = torch.empty(tuple(W.shape[:-1]) + (ldo // 16, 2, 16), device=W.device, dtype=torch.int16)
    check(_lib.lib().tgp_split_f16(_p(W), rows, K, K, _p(out), ldo, _stream(W)), "tgp_split_f16")
    return out


def split_bf16(W):
    """W (..., rows, K) fp32 -> int16 tensor (..., rows, ldo // 16, 3, 16) of bf16 bit patterns: per 16-wide K-tile the
    hi / mid / lo terms consumed by the split GEMM kernel (ldo = K rounded up to 16, zero padded)."""
    W = W.contiguous()
    K = W.shape[-1]
    rows = W.numel() // K
    ldo = (K + 15) // 16 * 16
    out = torch.empty(tuple(W.shape[:-1]) + (ldo // 16, 3, 16), device=W.device, dtype=torch.int16)
    check(_lib.lib().tgp_split_bf16(_p(W), rows, K, K, _p(out), ldo, _stream(W)), "tgp_split_bf16")
    return out


class Planes(object):
    """A (rows, K) fp32 matrix as BLOCKED fp16 hi / lo planes (include/tgpose.h, tgp_gemm_args.A_planes): what the pre-split GEMM
    kernel (csrc/gemm_pp.hip) stages by LDS-DMA.  buf: uint8 (ceil(rows / 32), kt, 2048); amax: int32 (ceil(rows / 32),) bits of the
    largest magnitude per row block (the fp16 range guard of the consumer), or None for weights (checked once at pack time)."""

    __slots__ = ("buf", "amax", "rows", "K", "kt", "tgp_unscale")

    def __init__(self, rows, K, device, kt=None, amax=True, buf=None, amax_buf=None):
        self.rows, self.K = int(rows), int(K)
        self.kt = int(kt) if kt is not None else (self.K + 15) // 16
        nblk = (self.rows + 31) // 32
        self.buf = buf if buf is not None else torch.empty(nblk, self.kt, 2048, device=device, dtype=torch.uint8)
        self.amax = (amax_buf if amax_buf is not None else torch.zeros(nblk, device=device, dtype=torch.int32)) if amax else None
        self.tgp_unscale = None

    def to_float(self):
        """(tests) the fp32 matrix hi + lo the planes stand for, (rows, K)"""
        nblk = self.buf.shape[0]
        h = self.buf.view(torch.float16).view(nblk, self.kt, 2, 2, 32, 8).float()      # [rb][kt][plane][h][r][8]
        x = (h[:, :, 0] + h[:, :, 1]).permute(0, 3, 1, 2, 4).reshape(nblk * 32, self.kt * 16)
        return x[: self.rows, : self.K]


def planes_on():
    """activations also travel as fp16 planes and their consumers run on the pre-split kernel (the default arithmetic only)"""
    return PLANES and GEMM_MODE == "split16"


@_timed("graph")
def planes_split(X, K=None, kt=None, amax=True, out=None):
    """X (..., K) fp32 rows (row stride >= K) -> Planes (tgp_planes_split).  Weights at pack time (amax=False), activations whose
    producer does not write planes itself."""
    X, ld = _rows(X, "X")
    K = X.shape[-1] if K is None else K
    rows = math.prod(X.shape[:-1])
    P = out if out is not None else Planes(rows, K, X.device, kt=kt, amax=amax)
    check(_lib.lib().tgp_planes_split(_p(X), rows, K, ld, _p(P.buf), P.kt, _p(P.amax), _stream(X)), "tgp_planes_split")
    return P


@_timed("graph")
def planes_gather(src, idx, dst, K, planes):
    """gather_rows(src, idx, dst) that also writes the planes of the gathered rows' first K columns (tgp_planes_gather)"""
    src, lds = _rows(_f32(src, "src", 3), "src")
    dst, ldd = _rows(_f32(dst, "dst", 3), "dst")
    B, n_src, C = src.shape
    n_out = dst.shape[1]
    check(_lib.lib().tgp_planes_gather(_p(src), lds, _p(_i32(idx, "idx")), B, n_src, n_out, K, C, _p(dst), ldd, _p(planes.buf),
                                       planes.kt, _p(planes.amax), _stream(src)), "tgp_planes_gather")
    return dst


def planes_w(W):
    """pack-time planes of a weight (N, K) for the pre-split kernel, with split_w's range rule: a weight that reaches 2^15 is split
    as W * 2^-k and the power of two rides along as .tgp_unscale (c_scale of the launch)."""
    amax = float(W.detach().abs().max()) if W.numel() else 0.0
    if not (amax >= FP16_SAFE) or not math.isfinite(amax):
        return planes_split(W.contiguous(), amax=False)
    k = math.frexp(amax)[1] - 15
    P = planes_split((W * (2.0 ** -k)).contiguous(), amax=False)
    P.tgp_unscale = torch.full((1,), 2.0 ** k, device=W.device, dtype=torch.float32)
    return P


# bench.py sets this to a list to time, with HIP events on the launch stream, every launch that the
# library routes to its 128x128-tile MFMA kernel (same rule as tgp_gemm_f32 in csrc/gemm.hip).
GEMM_TIMER = None
GEMM_TIMER_ALL = False      # development: time the small-tile and skinny launches too (scripts/gemm_shapes.py)


def _routes_to_big_tile(M, N, batch=1, split16=False):
    """does tgp_gemm_f32 send this launch to a tile kernel that reads the SPLIT weight (rather than to the exact-fp32 64 x 64 or the
    skinny kernel, which read the fp32 weight)?  split16: a two-term fp16 split weight is passed -- such launches also take the
    64 x 128 small-tile split kernel from 32 tiles on (round 3, csrc/gemm.hip `small_split`)."""
    if not (M > 32 and N > 64):
        return False
    if ((M + 127) // 128) * ((N + 127) // 128) * batch >= _big_tile_threshold():
        return True
    return bool(split16) and ((M + 63) // 64) * ((N + 127) // 128) * batch >= 32


_BIG_THR = None


def _big_tile_threshold():
    """resident_slots() / 2 of csrc/gemm.hip (slots = CUs: one 1024-thread workgroup per CU)"""
    global _BIG_THR
    if _BIG_THR is None:
        _BIG_THR = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count // 2
    return _BIG_THR


def gemm(A, W, C=None, *, M=None, N=None, K=None, lda=None, ldw=None, ldc=None, bias=None, rowbias=None,
         rows_per_obj=0, res1=None, ldr1=0, res2=None, ldr2=0, scale=None, shift=None, act=0, slope=0.0,
         colmax_keys=None, k_alg=None, slope_vec=None, cm_cols=0, c_col0=0, batch=1, batch_strides=None, w_split=None,
         a_scale=None, c_scale=None, ksplit_chunk=0, gather1=None, gather2=None, flops_ref=None, epilogue=0, pred=None,
         row_base=0, a_planes=None, w_planes=None, c_planes=None, cp_col0=0, pp_config=0, range_flag=None, a_keys=False, a_wrap=0,
         c_sigmoid=None):
    """Raw call into tgp_gemm_f32.  A/W/C/res* are tensors whose data_ptr is the first element of the
    operand (views into wider buffers are fine); all sizes/strides are explicit.  k_alg: the layer's
    true input width when K includes zero padding (only used for FLOP accounting in bench.py)."""
    split16 = w_split is not None and GEMM_MODE != "fp32" and w_split.shape[-2] == 2 and not ksplit_chunk
    # the pre-split kernel serves the launches the split tile kernels serve (so that results do not depend on whether planes were
    # handed in: launches too small for them run on the exact-fp32 small kernel either way)
    tile = _routes_to_big_tile(M, N, batch, True) and not ksplit_chunk
    pp = a_planes is not None and w_planes is not None and GEMM_MODE == "split16" and PLANES and tile and w_split is not None
    late_planes = None
    if c_planes is not None and GEMM_MODE == "split16" and PLANES and not (tile and w_split is not None):
        late_planes, c_planes = c_planes, None          # a small launch: its result is split by a launch of its own below
    timed = GEMM_TIMER is not None and pred is None and (GEMM_TIMER_ALL or pp or _routes_to_big_tile(M, N, batch, split16))   # (a predicated
    # launch is a repair path that normally does nothing: it has no place in a FLOP rate)
    if A is None:                                # a planes-only operand (tgp_gemm_args.range_flag)
        if not pp or range_flag is None:
            raise ValueError("gemm: an operand without its fp32 form needs both operands' planes, a tile-kernel launch and a range flag")
        A = a_planes.buf                         # (device / stream of the launch)
        a_ptr, lda = None, 0
    else:
        a_ptr = _p(A)
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(A.device))
    a = GemmArgs()
    a.A, a.lda, a.W, a.ldw = a_ptr, lda, _p(W), ldw
    a.C, a.ldc = (_p(C), ldc) if C is not None else (None, 0)
    a.M, a.N, a.K = M, N, K
    a.bias = _p(bias)
    a.rowbias, a.ldrb = (_p(rowbias), rowbias.stride(0)) if rowbias is not None else (None, 0)
    a.rows_per_obj = rows_per_obj
    a.res1, a.ldr1 = _p(res1), ldr1
    a.res2, a.ldr2 = _p(res2), ldr2
    a.scale, a.shift = _p(scale), _p(shift)
    a.act, a.slope = act, slope
    a.colmax_keys, a.ldcm = (_p(colmax_keys), colmax_keys.stride(-2)) if colmax_keys is not None else (None, 0)
    a.slope_vec, a.cm_cols, a.c_col0, a.batch = _p(slope_vec), cm_cols, c_col0, batch
    if batch_strides is not None:
        (a.batch_stride_a, a.batch_stride_w, a.batch_stride_c, a.batch_stride_vec, a.batch_stride_colmax) = batch_strides
    if w_split is not None and GEMM_MODE != "fp32":
        a.W_split, a.ldws = _p(w_split), w_split.shape[-3] * 16
        a.w_split_kind = 1 if w_split.shape[-2] == 2 else 0
        unscale = getattr(w_split, "tgp_unscale", None)       # a weight that was pre-scaled into fp16's range (split_w)
        if unscale is not None and not pp and _routes_to_big_tile(M, N, batch, split16):
            c_scale = unscale if c_scale is None else c_scale * unscale
    if pp and w_planes.tgp_unscale is not None:
        c_scale = w_planes.tgp_unscale if c_scale is None else c_scale * w_planes.tgp_unscale
    a.a_scale, a.c_scale, a.ksplit_chunk = _p(a_scale), _p(c_scale), int(ksplit_chunk)
    if gather1 is not None:                      # (rows tensor whose data_ptr is the first column wanted, row stride, int32 row ids)
        a.gres1, a.ldg1, a.gidx1 = _p(gather1[0]), int(gather1[1]), _p(gather1[2])
    if gather2 is not None:
        a.gres2, a.ldg2, a.gidx2 = _p(gather2[0]), int(gather2[1]), _p(gather2[2])
    a.epilogue = int(epilogue)
    a.pred = _p(pred)
    a.row_base = int(row_base)
    if pp:                                       # both operands as blocked fp16 planes: the pre-split kernel (bit-identical results)
        a.A_planes, a.a_kt, a.a_amax = _p(a_planes.buf), a_planes.kt, _p(a_planes.amax)
        a.W_planes, a.w_kt = _p(w_planes.buf), w_planes.kt
        a.pp_config = int(pp_config)
        a.range_flag = _p(range_flag)
    if c_planes is not None and GEMM_MODE == "split16" and PLANES:
        a.C_planes, a.c_kt, a.cp_col0, a.c_amax = _p(c_planes.buf), c_planes.kt, int(cp_col0), _p(c_planes.amax)
    a.a_keys, a.a_wrap, a.C_sigmoid = int(bool(a_keys)), int(a_wrap), _p(c_sigmoid)
    check(_lib.lib().tgp_gemm_f32(ctypes.byref(a), _stream(A)), "tgp_gemm_f32")
    if late_planes is not None:
        if C is None or batch != 1 or (cp_col0 & 15):
            raise ValueError("gemm: result planes of a small launch need its fp32 result")
        Kc = N - c_col0
        if Kc % 16 and (cp_col0 // 16 + (Kc + 15) // 16) < late_planes.kt:
            # the split kernel zero-fills the tail of its last K-tile: inside a wider planes buffer (fm2 | fm3) that tile belongs to
            # the neighbouring column range (the C-side rule of the C_planes path, csrc/gemm.hip)
            raise ValueError("gemm: result planes into a column range of a wider buffer need a multiple of 16 columns")
        check(_lib.lib().tgp_planes_split_cols(_p(C), M, Kc, ldc, _p(late_planes.buf), late_planes.kt, int(cp_col0), _p(late_planes.amax),
                                               _stream(A)), "tgp_planes_split_cols")
    if timed:
        e1.record(torch.cuda.current_stream(A.device))
        # flops_ref: what this launch stands for in the reference's formulation (the factored wide layers run fewer FLOPs)
        fl = 2.0 * M * N * (k_alg or K) * batch
        # algorithmic bytes of the launch (SURVEY 8d's rule: every operand once): A, W, the stored result (and its planes), plain and
        # gathered residuals -- bench.py sets them against the PMC traffic of the tile-GEMM kernel family
        nb = batch * 4.0 * (M * K + N * K + (M * (N - c_col0) if C is not None else 0) + (M * (N - c_col0) if c_planes is not None else 0)
                            + (M * N if res1 is not None else 0) + (M * N if res2 is not None else 0)
                            + (gather1[0].shape[0] * N if gather1 is not None else 0) + (gather2[0].shape[0] * N if gather2 is not None else 0))
        GEMM_TIMER.append((e0, e1, fl, (M, N, K, batch), fl if flops_ref is None else float(flops_ref), nb, "tile"))
    return C


def linear_rows(x, weight, bias=None, scale=None, shift=None, act=0, slope=0.0, out=None, rowbias=None,
                rows_per_obj=0, res1=None, res2=None, colmax_keys=None, want_out=True, k_alg=None, w_split=None,
                a_scale=None, c_scale=None, flops_ref=None, a_planes=None, w_planes=None, c_planes=None, cp_col0=0, pred=None):
    """x (..., K) rows (row stride >= K), weight (N, Kw>=K) -> (..., N).  Convenience over gemm()."""
    x, lda = _rows(x, "x")
    weight, ldw = _rows(weight, "weight")
    K = x.shape[-1]
    M = math.prod(x.shape[:-1])
    N = weight.shape[0]
    ldc = 0
    if want_out:
        if out is None:
            out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        out, ldc = _rows(out, "out")
    r1 = r2 = None
    l1 = l2 = 0
    if res1 is not None:
        r1, l1 = _rows(res1, "res1")
    if res2 is not None:
        r2, l2 = _rows(res2, "res2")
    gemm(x, weight, out if want_out else None, M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, bias=bias, rowbias=rowbias,
         rows_per_obj=rows_per_obj, res1=r1, ldr1=l1, res2=r2, ldr2=l2, scale=scale, shift=shift, act=act, slope=slope,
         colmax_keys=colmax_keys, k_alg=k_alg, w_split=w_split, a_scale=a_scale, c_scale=c_scale, flops_ref=flops_ref,
         a_planes=a_planes, w_planes=w_planes, c_planes=c_planes, cp_col0=cp_col0, pred=pred)
    return out


def heads_pack_w2(W2, bias1, scale1, shift1):
    """conv2 weights of the heads (heads, 256, 1024) fp32 and the heads' conv1 bias / BatchNorm scale / shift (heads * 1024 each) ->
    the fused heads kernel's operand: per (head, 32-channel block) conv2's fp16 hi / lo planes in MFMA fragment order (K permuted)
    and the block's three vectors (tgp_heads_pack_w2, ABI 7)"""
    W2 = W2.contiguous()
    heads = W2.shape[0]
    if tuple(W2.shape[1:]) != (256, 1024):
        raise ValueError("heads_pack_w2: (heads, 256, 1024) expected")
    vec = [v.contiguous() for v in (bias1, scale1, shift1)]
    if any(v.numel() != heads * 1024 for v in vec):
        raise ValueError("heads_pack_w2: bias1 / scale1 / shift1 of heads * 1024 channels expected")
    out = torch.empty(_lib.lib().tgp_heads_w2_bytes(heads), device=W2.device, dtype=torch.uint8)
    check(_lib.lib().tgp_heads_pack_w2(_p(W2), _p(vec[0]), _p(vec[1]), _p(vec[2]), heads, _p(out), _stream(W2)), "tgp_heads_pack_w2")
    out.tgp_heads = heads
    return out


def heads_repack_vectors(w2p, bias1, scale1, shift1):
    """rewrite, in place, the conv1 bias / BatchNorm scale / shift inside a heads_pack_w2 operand (the fold moved with the running
    statistics; the weights did not): a captured forward that holds the operand's address follows"""
    vec = [v.contiguous() for v in (bias1, scale1, shift1)]
    check(_lib.lib().tgp_heads_pack_w2(None, _p(vec[0]), _p(vec[1]), _p(vec[2]), w2p.tgp_heads, _p(w2p), _stream(w2p)), "tgp_heads_pack_w2")


def heads_planes_w(Wa_heads):
    """conv1 weights of the heads over the fine buffer (heads * 1024, ld >= 268) -> blocked fp16 planes with 17 K-tiles (the fused heads
    kernel's wa_planes)"""
    Wa_heads, ld = _rows(Wa_heads, "Wa_heads")
    return planes_split(Wa_heads, K=min(Wa_heads.shape[-1], 272), kt=17, amax=False)


def heads_fused(fine, K, wa_planes, p1, idx1, p2, idx2, w2p, bias2, scale2, shift2, B, rows_per_obj, k_alg=None,
                keys=None, overflow=None, rows=0, fine_planes=None):
    """conv1 -> BN -> ReLU -> conv2 -> BN -> ReLU -> max over points of the three heads (tgp_heads_fused): keys (heads, B, 256)
    and the device flag (1,) int32 that a wave raises instead of writing keys when it met a magnitude beyond fp16's range.
    fine (M, ldf); wa_planes: heads_planes_w(conv1 weights of the heads); w2p: heads_pack_w2(...) (conv2 weights + conv1's bias /
    scale / shift); p1 / p2: 2-D views whose column 0 is the first head's first channel (row stride = their .stride(0))."""
    fine, ldf = _rows(fine, "fine")
    heads = w2p.tgp_heads
    M = B * rows_per_obj
    if wa_planes.kt != 17 or wa_planes.rows != heads * 1024:
        raise ValueError("heads_fused: wa_planes must hold heads * 1024 rows in 17 K-tiles (ops.heads_planes_w)")
    if keys is None:          # (the eval forward hands in zeroed slices of its one per-forward arena instead)
        keys = torch.zeros(heads, B, 256, device=fine.device, dtype=torch.int32)
    if overflow is None:
        overflow = torch.zeros(1, device=fine.device, dtype=torch.int32)
    timed = GEMM_TIMER is not None
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(fine.device))
    a = _lib.HeadsFusedArgs()
    a.fine, a.ldf, a.K = _p(fine), ldf, K
    a.wa_planes = _p(wa_planes.buf)
    a.p1, a.ldp1, a.idx1 = _p(p1), p1.stride(0), _p(idx1)
    a.p2, a.ldp2, a.idx2 = _p(p2), p2.stride(0), _p(idx2)
    a.w2p = _p(w2p)
    a.bias2, a.scale2, a.shift2 = _p(bias2), _p(scale2), _p(shift2)
    a.keys = _p(keys)
    a.M, a.rows_per_obj, a.B, a.heads = M, rows_per_obj, B, heads
    a.overflow = _p(overflow)
    a.rows = int(rows)
    if fine_planes is not None and planes_on() and HEADS_PLANES:      # the points' features as fp16 planes: operand fragments load as they lie
        a.fine_planes, a.fine_kt, a.fine_amax = _p(fine_planes.buf), fine_planes.kt, _p(fine_planes.amax)
    check(_lib.lib().tgp_heads_fused(ctypes.byref(a), _stream(fine)), "tgp_heads_fused")
    if timed:
        e1.record(torch.cuda.current_stream(fine.device))
        Mk = rows if rows else M                                     # rows this launch processed
        conv2 = 2.0 * Mk * 256 * 1024 * heads
        # algorithmic bytes (SURVEY 8d's rule, every operand once): the points' features, the heads' columns of both coarse products,
        # the weights (conv1 planes + the packed conv2 image), the keys
        nb = 4.0 * (Mk * 272 + (p1.shape[0] + p2.shape[0]) * heads * 1024 + heads * 1024 * 272 + heads * 256 * 1024 + heads * B * 256)
        GEMM_TIMER.append((e0, e1, 2.0 * Mk * heads * 1024 * K + conv2, (Mk, heads * 1024, K, 1),
                           2.0 * Mk * heads * 1024 * (k_alg or K) + conv2, nb, "fused"))
    return keys, overflow


def dec_pack(w2, w3, w4, h1_permuted=False):
    """the decoder's 512 -> 512, 512 -> 256, 256 -> 128 weights -> the fused decoder kernel's staging image (tgp_dec_pack).
    h1_permuted: the operand will come from dec_l1 (channels in accumulator order) instead of a tile GEMM's C_planes"""
    if tuple(w2.shape) != (512, 512) or tuple(w3.shape) != (256, 512) or tuple(w4.shape) != (128, 256):
        raise ValueError("dec_pack: weights of (512, 512), (256, 512), (128, 256) expected")
    out = torch.empty(_lib.lib().tgp_dec_pack_bytes(), device=w2.device, dtype=torch.uint8)
    check(_lib.lib().tgp_dec_pack(_p(w2.contiguous()), _p(w3.contiguous()), _p(w4.contiguous()), int(bool(h1_permuted)), _p(out),
                                  _stream(w2)), "tgp_dec_pack")
    out.tgp_h1_permuted = bool(h1_permuted)
    return out


def proj_pack(w):
    """W (N, K) of a projection GEMM -> the staging image of tgp_proj_planes; None for shapes the kernel does not serve
    (K = 128 / 256 / 512, N % 128 == 0)"""
    N, K = w.shape
    nbytes = _lib.lib().tgp_proj_pack_bytes(int(K), int(N))
    if nbytes < 0:
        return None
    w = w.contiguous()
    out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    check(_lib.lib().tgp_proj_pack(_p(w), K, K, N, _p(out), _stream(w)), "tgp_proj_pack")
    out.tgp_shape = (int(K), int(N))
    return out


def proj_planes(a_planes, units, bias, x, weight, out=None, flops_ref=None):
    """x W^T (+ bias) on the projection kernel (tgp_proj_planes): a_planes = the planes of x (its first K columns), units =
    proj_pack(weight); x (..., K) fp32 rows and weight (N, K) are read only by tiles the fp16 range rule sends to the exact path."""
    K, N = units.tgp_shape
    x, lda = _rows(x, "x")
    weight, ldw = _rows(weight, "weight")
    M = a_planes.rows
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
    o, ldc = _rows(out, "out")
    timed = GEMM_TIMER is not None
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(x.device))
    a = _lib.ProjPlanesArgs()
    a.a_planes, a.a_kt, a.a_amax = _p(a_planes.buf), a_planes.kt, _p(a_planes.amax)
    a.a, a.lda, a.M, a.K, a.N = _p(x), lda, M, K, N
    a.units, a.w, a.ldw, a.bias = _p(units), _p(weight), ldw, _p(bias)
    a.c, a.ldc = _p(o), ldc
    check(_lib.lib().tgp_proj_planes(ctypes.byref(a), _stream(x)), "tgp_proj_planes")
    if timed:
        e1.record(torch.cuda.current_stream(x.device))
        fl = 2.0 * M * N * K
        GEMM_TIMER.append((e0, e1, fl, (M, N, K, 1), fl if flops_ref is None else float(flops_ref), 4.0 * (M * K + N * K + M * N), "fused"))
    return out


def hs_chain_pack(w1, w2):
    """W1 (N1, K1) of an HS layer's last GEMM and W2 (N2, N1) of the next layer's projection -> the fused pair's staging image
    (tgp_hs_chain_pack); None for shapes the kernel does not serve"""
    (N1, K1), (N2, k2) = w1.shape, w2.shape
    nbytes = _lib.lib().tgp_hs_chain_pack_bytes(int(K1), int(N1), int(N2)) if k2 == N1 else -1
    if nbytes < 0:
        return None
    w1, w2 = w1.contiguous(), w2.contiguous()
    out = torch.empty(nbytes, device=w1.device, dtype=torch.uint8)
    check(_lib.lib().tgp_hs_chain_pack(_p(w1), K1, K1, N1, _p(w2), N1, N2, _p(out), _stream(w1)), "tgp_hs_chain_pack")
    out.tgp_shape = (int(K1), int(N1), int(N2))
    return out


def hs_chain(a_planes, units, c1, bias2, flag, rowbias=None, rows_per_obj=0, res1=None, res2=None, scale1=None, shift1=None, relu=True,
             c1_planes=None, c1_col0=0, c2=None):
    """c1 = act(bn(A W1^T + rowbias[object] + res1 + res2)), c2 = c1 W2^T + bias2 in ONE launch (tgp_hs_chain): an HS layer's last
    GEMM and the next layer's projection.  a_planes: Planes of A (M rows); units: hs_chain_pack(W1, W2); c1 (M, N1) view (row stride
    = its .stride(-2)), written; c1_planes: Planes that also receive c1 from K-column c1_col0; c2 (M, N2) (allocated when None); flag:
    (1,) int32 zeroed by the caller, raised when the fp16 split's range is left -- the caller's two tile-kernel launches must follow,
    predicated on it.  Returns c2."""
    K1, N1, N2 = units.tgp_shape
    M = a_planes.rows
    c1r, ldc1 = _rows(c1, "c1")
    if c2 is None:
        c2 = torch.empty(M, N2, device=c1.device, dtype=torch.float32)
    timed = GEMM_TIMER is not None
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(c1.device))
    a = _lib.HsChainArgs()
    a.a_planes, a.a_kt, a.a_amax = _p(a_planes.buf), a_planes.kt, _p(a_planes.amax)
    a.M, a.K1, a.N1, a.N2 = M, K1, N1, N2
    a.units = _p(units)
    if rowbias is not None:
        a.rowbias, a.ldrb, a.rows_per_obj = _p(rowbias), rowbias.stride(0), rows_per_obj
    if res1 is not None:
        res1, a.ldr1 = _rows(res1, "res1")
        a.res1 = _p(res1)
    if res2 is not None:
        res2, a.ldr2 = _rows(res2, "res2")
        a.res2 = _p(res2)
    a.scale1, a.shift1, a.relu = _p(scale1), _p(shift1), int(bool(relu))
    a.c1, a.ldc1 = _p(c1r), ldc1
    if c1_planes is not None:
        if c1_col0 % 16:
            raise ValueError("hs_chain: c1_col0 must be a multiple of 16")
        a.c1_planes, a.c1_kt, a.c1_kt0, a.c1_amax = _p(c1_planes.buf), c1_planes.kt, c1_col0 // 16, _p(c1_planes.amax)
    a.bias2, a.c2, a.ldc2, a.flag = _p(bias2), _p(c2), c2.stride(-2), _p(flag)
    check(_lib.lib().tgp_hs_chain(ctypes.byref(a), _stream(c1)), "tgp_hs_chain")
    if timed:
        e1.record(torch.cuda.current_stream(c1.device))
        nb = 4.0 * (M * 16 * a_planes.kt + M * N1 * (2 + (res1 is not None) + (res2 is not None)) + M * N2 + N1 * K1 + N2 * N1)
        fl = 2.0 * M * (N1 * K1 + N2 * N1)
        GEMM_TIMER.append((e0, e1, fl, (M, N1 + N2, K1, 1), fl, nb, "fused"))
    return c2


def dec_l1(fine_planes, wa_planes, p1, idx1, p2, idx2, bias, scale, shift, rowbias, rows_per_obj, h1_planes, flag, k_alg=None):
    """The decoder's first conv on the factored form (tgp_dec_l1): fine_planes (M rows) x wa_planes (512 x 272 as planes, 17 K-tiles:
    heads_planes_w) + p1[idx1] + p2[idx2] + rowbias[object], BatchNorm fold, ReLU -> h1_planes (M, 512) in ACCUMULATOR channel order
    (for dec_fused with dec_pack(h1_permuted=True) only).  p1 / p2: 2-D views whose column 0 is the conv's first channel."""
    M = fine_planes.rows
    if wa_planes.kt != 17 or wa_planes.rows != 512 or h1_planes.rows != M or h1_planes.K != 512:
        raise ValueError("dec_l1: wa_planes (512 rows, 17 K-tiles) and h1_planes (M, 512) expected")
    a = _lib.DecL1Args()
    a.fine_planes, a.fine_kt, a.fine_amax = _p(fine_planes.buf), fine_planes.kt, _p(fine_planes.amax)
    a.wa_planes = _p(wa_planes.buf)
    a.p1, a.ldp1, a.idx1 = _p(p1), p1.stride(0), _p(idx1)
    a.p2, a.ldp2, a.idx2 = _p(p2), p2.stride(0), _p(idx2)
    a.bias, a.scale, a.shift = _p(bias), _p(scale), _p(shift)
    if rowbias is not None:
        a.rowbias, a.ldrb = _p(rowbias), rowbias.stride(0)
    a.rows_per_obj = int(rows_per_obj)
    a.h1_planes, a.h1_kt, a.h1_amax = _p(h1_planes.buf), h1_planes.kt, _p(h1_planes.amax)
    a.flag, a.M = _p(flag), M
    timed = GEMM_TIMER is not None
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(p1.device))
    check(_lib.lib().tgp_dec_l1(ctypes.byref(a), _stream(p1)), "tgp_dec_l1")
    if timed:
        e1.record(torch.cuda.current_stream(p1.device))
        nb = 4.0 * (M * 272 + (p1.shape[0] + p2.shape[0]) * 512 + 512 * 272 + M * 512)
        GEMM_TIMER.append((e0, e1, 2.0 * M * 512 * 268, (M, 512, 268, 1), 2.0 * M * 512 * (k_alg or 268), nb, "fused"))
    return h1_planes


def dec_fused(h1_planes, units, vecs, w5, b5, order, rows_per_obj, flag, out=None):
    """The decoder behind its first conv as one launch (tgp_dec_fused): h1_planes = the first conv's activation (M, 512) as planes;
    vecs = ((bias, scale, shift) of the 512 -> 512 layer, of 512 -> 256, of 256 -> 128); w5 (3, 128), b5 (3); order (B, n) int64 (the
    sort's permutation) or None; flag (1,) int32 (zeroed by the caller).  -> (M, 3) rows in point order"""
    M = h1_planes.rows
    if h1_planes.K != 512:
        raise ValueError("dec_fused: a (M, 512) operand expected")
    if out is None:
        out = torch.empty(M, 3, device=units.device, dtype=torch.float32)
    a = _lib.DecFusedArgs()
    a.h1_planes, a.h1_kt, a.h1_amax = _p(h1_planes.buf), h1_planes.kt, _p(h1_planes.amax)
    a.units = _p(units)
    keep = []
    for l in range(3):
        for v in range(3):
            t = vecs[l][v].contiguous()
            keep.append(t)
            a.vec[l][v] = t.data_ptr()
    w5c, b5c = w5.contiguous(), b5.contiguous()
    a.w5, a.b5 = _p(w5c), _p(b5c)
    a.map, a.rows_per_obj = _p(order), int(rows_per_obj)
    a.out, a.flag, a.M = _p(out), _p(flag), M
    timed = GEMM_TIMER is not None
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(units.device))
    check(_lib.lib().tgp_dec_fused(ctypes.byref(a), _stream(units)), "tgp_dec_fused")
    if timed:
        e1.record(torch.cuda.current_stream(units.device))
        fl = 2.0 * M * (512 * 512 + 256 * 512 + 128 * 256 + 3 * 128)
        nb = 4.0 * (M * 512 + 512 * 512 + 256 * 512 + 128 * 256 + M * 3) + 8.0 * M
        GEMM_TIMER.append((e0, e1, fl, (M, 512 + 256 + 128 + 3, 512, 1), fl, nb, "fused"))
    return out


def conv_max_fused(fine, K, wa_planes, p1, idx1, p2, idx2, bias, scale, shift, slope, B, rows_per_obj, k_alg=None, keys=None, overflow=None,
                   fine_planes=None):
    """conv -> BN -> LeakyReLU -> max over points of a factored layer (tgp_conv_max_fused): keys (B, C) and the overflow flag.
    wa_planes: heads_planes_w(the layer's (C, ld >= 268) weight over the fine buffer)."""
    fine, ldf = _rows(fine, "fine")
    C = bias.numel()
    M = B * rows_per_obj
    if keys is None:
        keys = torch.zeros(B, C, device=fine.device, dtype=torch.int32)
    if overflow is None:
        overflow = torch.zeros(1, device=fine.device, dtype=torch.int32)
    timed = GEMM_TIMER is not None
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(fine.device))
    a = _lib.ConvMaxFusedArgs()
    a.fine, a.ldf, a.K = _p(fine), ldf, K
    if wa_planes.kt != 17 or wa_planes.rows != C:
        raise ValueError("conv_max_fused: wa_planes must hold the layer's C rows in 17 K-tiles (ops.heads_planes_w)")
    a.wa_planes = _p(wa_planes.buf)
    a.p1, a.ldp1, a.p1_rows, a.idx1 = _p(p1), p1.stride(0), p1.shape[0], _p(idx1)
    a.p2, a.ldp2, a.p2_rows, a.idx2 = _p(p2), p2.stride(0), p2.shape[0], _p(idx2)
    a.bias, a.scale, a.shift, a.slope = _p(bias), _p(scale), _p(shift), float(slope)
    a.keys, a.ldk = _p(keys), C
    a.M, a.rows_per_obj, a.C = M, rows_per_obj, C
    a.overflow = _p(overflow)
    if fine_planes is not None and planes_on() and HEADS_PLANES:
        a.fine_planes, a.fine_kt, a.fine_amax = _p(fine_planes.buf), fine_planes.kt, _p(fine_planes.amax)
    check(_lib.lib().tgp_conv_max_fused(ctypes.byref(a), _stream(fine)), "tgp_conv_max_fused")
    if timed:
        e1.record(torch.cuda.current_stream(fine.device))
        nb = 4.0 * (M * 272 + (p1.shape[0] + p2.shape[0]) * C + C * 272 + B * C)
        GEMM_TIMER.append((e0, e1, 2.0 * M * C * K, (M, C, K, 1), 2.0 * M * C * (k_alg or K), nb, "fused"))
    return keys, overflow


@_timed("graph")
def colmax_decode(keys, out2=False):
    rows, N = keys.shape
    out = torch.empty(rows, 2 * N if out2 else N, device=keys.device, dtype=torch.float32)
    second = out[:, N:] if out2 else None
    check(_lib.lib().tgp_colmax_decode(_p(keys), keys.stride(0), rows, N, _p(out), out.stride(0), _p(second),
                                       _stream(keys)), "tgp_colmax_decode")
    return out


@_timed("graph")
def colmax(x):
    """x (B,n,C) rows -> (B,C) max over n"""
    x, ld = _rows(x, "x")
    B, n, C = x.shape
    out = torch.empty(B, C, device=x.device, dtype=torch.float32)
    check(_lib.lib().tgp_colmax(_p(x), ld, B, n, C, _p(out), _stream(x)), "tgp_colmax")
    return out


@_timed("graph")
def sigmoid(x):
    _f32(x, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().tgp_sigmoid(_p(x), _p(y), x.numel(), _stream(x)), "tgp_sigmoid")
    return y


@_timed("graph")
def head_post(green, red, ts, mean):
    """green / red (B, >=4), ts (B, >=6): 2-D views with contiguous rows (their row strides are passed on)"""
    B = green.shape[0]
    dev = green.device
    for t in (green, red, ts):
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError("head_post: 2-D inputs with contiguous rows expected")
    pg, pr = torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
    fg, fr = torch.empty(B, device=dev), torch.empty(B, device=dev)
    pT, ps = torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
    check(_lib.lib().tgp_head_post(_p(green), _p(red), _p(ts), green.stride(0), red.stride(0), ts.stride(0), _p(mean), B, _p(pg),
                                   _p(pr), _p(fg), _p(fr), _p(pT), _p(ps), _stream(green)), "tgp_head_post")
    return pg, pr, fg, fr, pT, ps


def rows_out(x, w, bias=None, order=None, out=None, pred=None):
    """x (B,n,K), w (n_out <= 4, K), order (B,n) int64 or None -> out (B,n,n_out) with out[b, order[b,i]] = x[b,i] @ w^T + bias
    (tgp_rows_out: a narrow last layer and the scatter that undoes a row sort, one launch).  pred: device int -- the launch returns at
    once while it is 0 (the last step of a repair chain, writing into `out`)"""
    x, ld = _rows(x, "x")
    B, n, K = x.shape
    if not w.is_contiguous() or w.shape[1] != K:
        raise ValueError("rows_out: w (n_out, K) contiguous expected")
    if order is not None and (order.dtype != torch.int64 or not order.is_contiguous() or tuple(order.shape) != (B, n)):
        raise ValueError("rows_out: order (B,n) int64 contiguous expected")
    if out is None:
        out = torch.empty(B, n, w.shape[0], device=x.device, dtype=torch.float32)
    check(_lib.lib().tgp_rows_out_pred(_p(x), ld, B * n, K, _p(w), w.stride(0), _p(bias), w.shape[0], _p(order), n, _p(out), _p(pred),
                                       _stream(x)), "tgp_rows_out")
    return out


def pose_tail(keys2, w3t, b3, scale3, shift3, w4, b4, mean, raw=None):
    """keys2 (3,B,256) int32 max keys of the heads' conv2 -> the six pose outputs (tgp_pose_tail: conv3, conv4 and head_post as one
    launch); raw (3,B,8): conv4's outputs"""
    B, dev = keys2.shape[1], keys2.device
    pg, pr = torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
    fg, fr = torch.empty(B, device=dev), torch.empty(B, device=dev)
    pT, ps = torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
    for t in (keys2, w3t, b3, scale3, shift3, w4, b4, mean):
        if not t.is_contiguous():
            raise ValueError("pose_tail: contiguous operands expected")
    if tuple(w3t.shape) != (3, 256, 256) or tuple(w4.shape) != (3, 8, 256) or tuple(keys2.shape) != (3, B, 256):
        raise ValueError("pose_tail: shapes")
    check(_lib.lib().tgp_pose_tail(_p(keys2), _p(w3t), _p(b3), _p(scale3), _p(shift3), _p(w4), _p(b4), _p(mean), B, _p(pg), _p(pr),
                                   _p(fg), _p(fr), _p(pT), _p(ps), _p(raw), _stream(keys2)), "tgp_pose_tail")
    return pg, pr, fg, fr, pT, ps


def head_post_bwd(green, red, grads):
    """grads: gradients of head_post's six outputs (None = zero) -> d green (B,4), d red (B,4), d ts (B,6)"""
    B, dev = green.shape[0], green.device
    gs = [None if t is None else t.float().contiguous() for t in grads]
    dg, dr, dt = torch.empty(B, 4, device=dev), torch.empty(B, 4, device=dev), torch.empty(B, 6, device=dev)
    check(_lib.lib().tgp_head_post_bwd(_p(green), _p(red), green.stride(0), red.stride(0), B, *[_p(t) for t in gs], _p(dg), _p(dr),
                                       _p(dt), _stream(green)), "tgp_head_post_bwd")
    return dg, dr, dt


@_timed("graph")
def add_mean_(recon, mean):
    B, n, _ = recon.shape
    check(_lib.lib().tgp_add_mean(_p(recon), _p(mean), B, n, _stream(recon)), "tgp_add_mean")
    return recon


def chamfer_fwd(xyz1, xyz2, dist1, dist2, idx1, idx2):
    """chamfer_3D.forward convention: caller allocates every output (dist_chamfer_3D.py:33-45)."""
    _f32(xyz1, "xyz1", 3), _f32(xyz2, "xyz2", 3)
    if not (xyz1.is_contiguous() and xyz2.is_contiguous()):
        raise ValueError("chamfer inputs must be contiguous (dist_chamfer_3D.py:72-73)")
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    check(_lib.lib().tgp_chamfer_fwd(_p(xyz1), _p(xyz2), B, n, m, _p(dist1), _p(dist2), _p(_i32(idx1, "idx1")),
                                     _p(_i32(idx2, "idx2")), _stream(xyz1)), "tgp_chamfer_fwd")
    return 1


def chamfer_bwd(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2):
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    check(_lib.lib().tgp_chamfer_bwd(_p(xyz1), _p(xyz2), B, n, m, _p(graddist1), _p(graddist2), _p(idx1), _p(idx2),
                                     _p(gradxyz1), _p(gradxyz2), _stream(xyz1)), "tgp_chamfer_bwd")
    return 1


def dcd_fwd(dist1, dist2, idx1, idx2, alpha, n_lambda, non_reg=False, want_weights=True):
    """calc_dcd after the Chamfer search -> (loss (B,), w1 (B,n), w2 (B,m))"""
    B, n = dist1.shape
    m = dist2.shape[1]
    dev = dist1.device
    loss = torch.empty(B, device=dev, dtype=torch.float32)
    w1 = torch.empty(B, n, device=dev, dtype=torch.float32) if want_weights else None
    w2 = torch.empty(B, m, device=dev, dtype=torch.float32) if want_weights else None
    check(_lib.lib().tgp_dcd_fwd(_p(dist1.contiguous()), _p(dist2.contiguous()), _p(_i32(idx1, "idx1")), _p(_i32(idx2, "idx2")),
                                 B, n, m, float(alpha), float(n_lambda), int(bool(non_reg)), _p(loss), _p(w1), _p(w2),
                                 _stream(dist1)), "tgp_dcd_fwd")
    return loss, w1, w2


def dcd_bwd(dist1, dist2, w1, w2, gloss, alpha):
    B, n = dist1.shape
    m = dist2.shape[1]
    gd1, gd2 = torch.empty_like(dist1), torch.empty_like(dist2)
    check(_lib.lib().tgp_dcd_bwd(_p(dist1), _p(dist2), _p(w1), _p(w2), _p(gloss.contiguous()), B, n, m, float(alpha), _p(gd1),
                                 _p(gd2), _stream(dist1)), "tgp_dcd_bwd")
    return gd1, gd2


def emd_max_points():
    return int(_lib.lib().tgp_emd_max_points())


def emd_fwd(xyz1, xyz2, eps, iters):
    """Auction matching of xyz1 (B,n,3) onto xyz2 (B,n,3), every iteration in one launch (csrc/emd.hip)
    -> (dist (B,n) float32 squared distances, assignment (B,n) int32)"""
    _f32(xyz1, "xyz1", 3), _f32(xyz2, "xyz2", 3)
    if not (xyz1.is_contiguous() and xyz2.is_contiguous()):
        raise ValueError("emd inputs must be contiguous")
    if xyz1.shape != xyz2.shape or xyz1.shape[2] != 3:
        raise ValueError("emd: the two clouds must both be (B, n, 3) (emd_module.py:45)")
    B, n, _ = xyz1.shape
    dist = torch.empty(B, n, device=xyz1.device, dtype=torch.float32)
    assignment = torch.empty(B, n, device=xyz1.device, dtype=torch.int32)
    nbytes = int(_lib.lib().tgp_emd_workspace_bytes(B, n))
    ws = torch.empty(nbytes, device=xyz1.device, dtype=torch.uint8) if nbytes > 0 else None
    check(_lib.lib().tgp_emd_fwd(_p(xyz1), _p(xyz2), B, n, float(eps), int(iters), _p(dist), _p(assignment), _p(ws),
                                 _stream(xyz1)), "tgp_emd_fwd")
    return dist, assignment


def emd_bwd(xyz1, xyz2, grad_dist, assignment):
    """-> grad_xyz1 (B,n,3) = (grad_dist * 2) * (xyz1 - xyz2[assignment]); the gradient for xyz2 is zero"""
    B, n, _ = xyz1.shape
    grad = torch.empty_like(xyz1)
    check(_lib.lib().tgp_emd_bwd(_p(xyz1), _p(xyz2), _p(_f32(grad_dist.contiguous(), "grad_dist", 2)),
                                 _p(_i32(assignment, "assignment")), B, n, _p(grad), _stream(xyz1)), "tgp_emd_bwd")
    return grad


def fps_max_points():
    return int(_lib.lib().tgp_fps_max_points())


def farthest_points(xyz, n, counts=None, start=None, init_center=True, return_distances=False, return_clusters=False):
    """Farthest point sampling of a batch of clouds in one launch (tgp_fps, csrc/fps.hip; the reference's farthest_points bit for bit,
    DESIGN.md section 3 "Farthest point sampling").

    xyz (B,M,3) or (B,M,4) float32 whose rows are 3 or 4 floats apart (a [..., :3] view of padded rows is read in place; a fourth
    column is not read), M <= fps_max_points().  counts (B,) int32: each cloud's live prefix, 1 <= counts[b] <= M (default M).
    start (B,3): the virtual first centre; None with init_center: the cloud's centroid (pairwise-tree sum); init_center=False: the
    first centre is row 0.  -> idx (B,n) int32: the centres in selection order where counts[b] > n, else i % counts[b]
    [, distances (B,M) float32][, clusters (B,M) int32]; rows at and beyond counts[b] are NaN / -1."""
    _f32(xyz, "xyz", 3)
    B, M, C = xyz.shape
    ld = xyz.stride(1) if M > 1 else C                       # the stride of a dimension of size 1 says nothing
    if C not in (3, 4) or ld not in (3, 4) or C > ld or xyz.stride(2) != 1 or (B > 1 and xyz.stride(0) != M * ld):
        raise ValueError("farthest_points: xyz must be (B, M, 3 or 4) with rows 3 or 4 floats apart and clouds M rows apart")
    n = int(n)
    if B < 1 or M < 1 or n < 1:
        raise ValueError("farthest_points: B, M and n must be at least 1")
    if M > fps_max_points():
        raise ValueError("farthest_points: M = %d is above the cap of %d points; thin the cloud first" % (M, fps_max_points()))
    if counts is not None and _i32(counts, "counts").shape != (B,):
        raise ValueError("farthest_points: counts must be (B,)")
    if start is not None and (not _f32(start, "start").is_contiguous() or start.shape != (B, 3)):
        raise ValueError("farthest_points: start must be a contiguous (B,3) tensor")
    dev = xyz.device
    idx = torch.empty(B, n, device=dev, dtype=torch.int32)
    dist = torch.full((B, M), float("nan"), device=dev) if return_distances else None
    clusters = torch.full((B, M), -1, device=dev, dtype=torch.int32) if return_clusters else None
    check(_lib.lib().tgp_fps(_p(xyz), ld, _p(counts), B, M, n, _p(start), 1 if init_center else 0, _p(idx), _p(dist), _p(clusters),
                             _stream(xyz)), "tgp_fps")
    out = (idx,) + ((dist,) if return_distances else ()) + ((clusters,) if return_clusters else ())
    return out[0] if len(out) == 1 else out


class MeshSet(object):
    """Triangle meshes packed once for ops.render_depth (tgp_render_depth's mesh set): ``meshes`` is a list of (verts (V,3) float,
    faces (F,3) int, local to their mesh).  Holds verts (sum V,3) float32, faces (sum F,3) int32 and the prefix sums vptr / fptr
    (M+1) int32 on ``device``, and on the host the counts, the largest mesh and each mesh's axis-aligned extent.  ops.mesh_sample
    reads the same set; its cumulative-area table is built on first use (area_cdf).  from_device takes meshes that are packed on
    the GPU already (ops.tsdf_meshset(indexed=True) makes its set that way)."""

    def __init__(self, meshes, device="cuda"):
        import numpy as np
        if not meshes:
            raise ValueError("MeshSet: at least one mesh")
        vs, fs = [], []
        for i, (v, f) in enumerate(meshes):
            v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or not len(v) or not len(f):
                raise ValueError("MeshSet: mesh %d must be (verts (V,3), faces (F,3)) with V, F >= 1" % i)
            if f.min() < 0 or f.max() >= len(v):
                raise ValueError("MeshSet: mesh %d has a face index outside its %d vertices" % (i, len(v)))
            if len(f) >= render_max_faces():
                raise ValueError("MeshSet: mesh %d has %d faces; the cap is %d" % (i, len(f), render_max_faces() - 1))
            vs.append(v), fs.append(f)
        self.n_verts = [len(v) for v in vs]
        self.n_faces = [len(f) for f in fs]
        self.extent = np.stack([v.max(0) - v.min(0) for v in vs])
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.verts, self.faces = up(np.concatenate(vs)), up(np.concatenate(fs))
        self.vptr = up(np.concatenate([[0], np.cumsum(self.n_verts)]).astype(np.int32))
        self.fptr = up(np.concatenate([[0], np.cumsum(self.n_faces)]).astype(np.int32))
        self._area_cdf = None
        self._fields = {}                # fields()' dicts
        self._diameter = None            # (M) float64, each mesh's largest vertex-to-vertex distance: evaluation.bop.diameter fills it
        self.vert_normals = None         # (sum V,3) float32 unit vertex normals: mesh_vertex_normals makes them, tsdf_meshset(normals=True) keeps them
        self.normal_scale = None         # (M) float64 quantisation of mesh_vertex_normals; None: 2^40 / (largest extent)^2

    @classmethod
    def from_device(cls, verts, faces, n_verts, n_faces):
        """The set of meshes that are already packed on a GPU: verts (sum V,3) float32 and faces (sum F,3) int32, local to their
        mesh, contiguous, with the host lists n_verts and n_faces (M ints each).  The meshes are not read back: each mesh's extent
        and its smallest and largest face index are made on the device and M x 5 numbers are read once.  An empty mesh, a mesh at
        the renderer's face cap and a face index outside its mesh are refused by name, as __init__ refuses them."""
        import numpy as np
        if not (torch.is_tensor(verts) and verts.is_cuda and verts.dtype == torch.float32 and verts.is_contiguous() and verts.dim() == 2
                and verts.shape[1] == 3):
            raise TypeError("MeshSet.from_device: verts must be a contiguous (sum V,3) float32 GPU tensor")
        if not (torch.is_tensor(faces) and faces.is_cuda and faces.dtype == torch.int32 and faces.is_contiguous() and faces.dim() == 2
                and faces.shape[1] == 3 and faces.device == verts.device):
            raise TypeError("MeshSet.from_device: faces must be a contiguous (sum F,3) int32 tensor on verts' device")
        n_verts, n_faces = [int(n) for n in n_verts], [int(n) for n in n_faces]
        if not n_verts or len(n_verts) != len(n_faces):
            raise ValueError("MeshSet.from_device: n_verts and n_faces must list the same M >= 1 meshes")
        for i, (nv, nf) in enumerate(zip(n_verts, n_faces)):
            if nv < 1 or nf < 1:
                raise ValueError("MeshSet.from_device: mesh %d is empty (%d vertices, %d faces)" % (i, nv, nf))
            if nf >= render_max_faces():
                raise ValueError("MeshSet.from_device: mesh %d has %d faces; the cap is %d" % (i, nf, render_max_faces() - 1))
        if sum(n_verts) != verts.shape[0] or sum(n_faces) != faces.shape[0]:
            raise ValueError("MeshSet.from_device: the counts must add up to the rows of verts and faces")
        vp, fp = np.concatenate([[0], np.cumsum(n_verts)]), np.concatenate([[0], np.cumsum(n_faces)])
        rows = []
        for m in range(len(n_verts)):
            v, f = verts[vp[m]:vp[m + 1]], faces[fp[m]:fp[m + 1]]
            rows.append(torch.cat([(v.amax(0) - v.amin(0)).double(), torch.stack([f.min(), f.max()]).double()]))
        host = torch.stack(rows).cpu().numpy()                # the read-back: M x 5 numbers
        for i in range(len(n_verts)):
            if host[i, 3] < 0 or host[i, 4] >= n_verts[i]:
                raise ValueError("MeshSet.from_device: mesh %d has a face index outside its %d vertices" % (i, n_verts[i]))
        self = cls.__new__(cls)
        self.n_verts, self.n_faces = n_verts, n_faces
        self.extent = host[:, :3].astype(np.float32)
        self.device = verts.device
        self.verts, self.faces = verts, faces
        self.vptr = torch.from_numpy(vp.astype(np.int32)).to(self.device)
        self.fptr = torch.from_numpy(fp.astype(np.int32)).to(self.device)
        self._area_cdf = None
        self._fields = {}
        self._diameter = None
        self.vert_normals = None
        self.normal_scale = None
        return self

    def __len__(self):
        return len(self.n_verts)

    def fields(self, faces=True, maxima=False):
        """the set as the keyword arguments of an argument struct (tgp_*_args): verts, vptr, M, n_verts; with ``faces`` faces, fptr,
        n_faces; with ``maxima`` the largest mesh's max_verts (and max_faces).  The set does not change once it is packed, so each
        dict is made once and kept (every call of an op asks for one): read it, do not write to it."""
        kw = self._fields.get((faces, maxima))
        if kw is None:
            kw = dict(verts=_p(self.verts), vptr=_p(self.vptr), M=len(self), n_verts=self.verts.shape[0])
            if faces:
                kw.update(faces=_p(self.faces), fptr=_p(self.fptr), n_faces=self.faces.shape[0])
            if maxima:
                kw.update(max_verts=max(self.n_verts))
            if maxima and faces:
                kw.update(max_faces=max(self.n_faces))
            self._fields[(faces, maxima)] = kw
        return kw

    def bounds(self):
        """(M,2,3) float32 on the device: each mesh's least and greatest vertex coordinates (ops.mesh_windows frames a mesh by this
        box).  Made by torch reductions on the device at first use and kept; nothing is read back."""
        b = getattr(self, "_bounds", None)
        if b is None:
            rows, lo = [], 0
            for nv in self.n_verts:
                v = self.verts[lo:lo + nv]
                rows.append(torch.stack([v.amin(0), v.amax(0)]))
                lo += nv
            b = self._bounds = torch.stack(rows).contiguous()
        return b

    def area_cdf(self):
        """(sum F) float64 on the device: each mesh's cumulative triangle area over its own faces in tgp_mesh_area_cdf's fixed
        order (chunks of 64 faces; DESIGN.md section 3 "Mesh surface sampling").  Built by one launch on the current stream at
        first use and kept; that stream is synchronised once, there, so that later calls may read the table from any stream
        (call it before a graph capture that samples from the set)."""
        if self._area_cdf is None:
            if self.verts.device.type != "cuda":
                raise TypeError("MeshSet.area_cdf: the mesh set must be on a GPU")
            cdf = torch.zeros(self.faces.shape[0], device=self.verts.device, dtype=torch.float64)
            check(_lib.lib().tgp_mesh_area_cdf(_p(self.verts), _p(self.faces), _p(self.vptr), _p(self.fptr), len(self),
                                               self.verts.shape[0], self.faces.shape[0], _p(cdf), _stream(self.verts)), "tgp_mesh_area_cdf")
            torch.cuda.current_stream(self.verts.device).synchronize()
            self._area_cdf = cdf
        return self._area_cdf


def _mesh_jobs(meshset, job_mesh, what):
    """job_mesh as a (B) int32 tensor on the mesh set's device.  A host list / array / tensor is checked against the set here; a GPU
    tensor is not read back: an index outside the set gives status 2 and rows of zeros."""
    import numpy as np
    if not isinstance(meshset, MeshSet):
        raise TypeError("%s: meshset must be an ops.MeshSet" % what)
    dev = meshset.verts.device
    if torch.is_tensor(job_mesh) and job_mesh.is_cuda:
        if job_mesh.dtype != torch.int32 or not job_mesh.is_contiguous() or job_mesh.dim() != 1:
            raise TypeError("%s: job_mesh on the GPU must be a contiguous (B) int32 tensor" % what)
        if job_mesh.device != dev:
            raise ValueError("%s: job_mesh is not on the mesh set's device" % what)
        jm = job_mesh
    else:
        a = np.asarray(job_mesh.numpy() if torch.is_tensor(job_mesh) else job_mesh)
        if a.size == 0:
            raise ValueError("%s: at least one job" % what)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise TypeError("%s: job_mesh must be a (B) sequence of integer mesh indices" % what)
        if a.size and (a.min() < 0 or a.max() >= len(meshset)):
            raise ValueError("%s: a mesh index is outside the set of %d meshes" % (what, len(meshset)))
        jm = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    if jm.numel() < 1:
        raise ValueError("%s: at least one job" % what)
    return jm


def _gpu_args(who, dev, given, where="the mesh set's device"):
    """every (tensor, name, dtype) of ``given`` is a contiguous GPU tensor of that dtype on ``dev``"""
    for t, name, dt in given:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise TypeError("%s: %s must be a contiguous %s GPU tensor" % (who, name, str(dt).replace("torch.", "")))
        if t.device != dev:
            raise ValueError("%s: %s is not on %s" % (who, name, where))


def _frame_jobs(who, dev, depth, camk, job_img, job_tensors, mask=None, job_mask_val=None, where="the mesh set's device"):
    """The depth frames and the job table of pose_verify, pose_vsd and tsdf_integrate: depth (S,H,W) 16-bit and not empty, camk
    (S,4) float32, job_img (J) int32, each (tensor, name, dtype, trailing shape[, the shape's text in the message]) of ``job_tensors``
    a (J, ...) tensor, mask (S,H,W) uint8 with job_mask_val (J) uint8 or neither; all contiguous on ``dev``.  -> (S, H, W, J)"""
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype in (torch.int16, torch.uint16) and depth.is_contiguous()):
        raise TypeError("%s: depth must be a contiguous 16-bit GPU tensor" % who)
    if (mask is None) != (job_mask_val is None):
        raise ValueError("%s: mask and job_mask_val come together" % who)
    given = [(depth, "depth", depth.dtype), (camk, "camk", torch.float32), (job_img, "job_img", torch.int32)] + [g[:3] for g in job_tensors]
    if mask is not None:
        given += [(mask, "mask", torch.uint8), (job_mask_val, "job_mask_val", torch.uint8)]
    _gpu_args(who, dev, given, where)
    if depth.dim() != 3 or depth.numel() == 0:
        raise ValueError("%s: depth must be (S,H,W)" % who)
    S, H, W = depth.shape
    J = job_img.numel()
    if camk.shape != (S, 4) or job_img.dim() != 1 or any(g[0].shape != (J,) + g[3] for g in job_tensors):
        shapes = ["%s (%s)" % (g[1], g[4] if len(g) > 4 else ",".join(["J"] + ["%d" % d for d in g[3]])) for g in job_tensors]
        raise ValueError("%s: %s are expected" % (who, ", ".join(["camk (S,4)", "job_img (J)"] + shapes)))
    if mask is not None and (mask.shape != (S, H, W) or job_mask_val.shape != (J,)):
        raise ValueError("%s: mask (S,H,W) and job_mask_val (J) are expected" % who)
    return S, H, W, J


def _workspace(dev, nbytes, who, dtype=torch.uint8):
    """the workspace a tgp_*_workspace_bytes call asks for, in elements of ``dtype``; a negative size is that call's error code"""
    if nbytes < 0:
        check(nbytes, who)
    return torch.empty(nbytes // dtype.itemsize, device=dev, dtype=dtype)


def mesh_check_status(status, what="mesh_sample"):
    """one read of the (B) status words; raises TgpError naming the first failed job"""
    st = status.cpu().tolist()
    bad = [(b, s) for b, s in enumerate(st) if s != 0]
    if bad:
        raise _lib.TgpError("%s: job %d failed: %s (%d of %d jobs failed)" % (what, bad[0][0], _lib.MESH_STATUS.get(bad[0][1], bad[0][1]),
                                                                             len(bad), len(st)))


def mesh_sample(meshset, job_mesh, n, *, u=None, keys=None, seed=0, normals=False, dtype=torch.float32, return_face=False,
                check_status=False):
    """Area-weighted surface samples of B jobs in one launch (tgp_mesh_sample, csrc/meshsample.hip; the reference's uniform_sample,
    DESIGN.md section 3 "Mesh surface sampling").  job_mesh (B): each job's mesh in the set; every job draws n samples from three
    float64 uniforms per sample: ``u`` (B,n,3) float64 on the device (row i = np.random.random(), np.random.random(2) of the
    reference's sample i), or Philox words keyed by ``keys`` (B) 64-bit integers under ``seed`` -- exactly one of the two.
    -> dict: points (B,n,3), or (B,n,6) [point, unit normal] with normals, float64 or rounded once to float32 (dtype); status (B)
    int32 (0; 1: the mesh has no positive finite area; 2: no such mesh); with return_face face (B,n) int32 within the mesh.
    Nothing synchronises unless check_status, which reads status once and raises TgpError."""
    import numpy as np
    jm = _mesh_jobs(meshset, job_mesh, "mesh_sample")
    dev = meshset.verts.device
    B, n = jm.numel(), int(n)
    if n < 1:
        raise ValueError("mesh_sample: n must be at least 1")
    if (u is None) == (keys is None):
        raise ValueError("mesh_sample: exactly one of u (host draws) and keys (device draws) is expected")
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("mesh_sample: dtype must be torch.float32 or torch.float64")
    if u is not None:
        if not (torch.is_tensor(u) and u.is_cuda and u.dtype == torch.float64 and u.is_contiguous()):
            raise TypeError("mesh_sample: u must be a contiguous float64 GPU tensor")
        if u.device != dev:
            raise ValueError("mesh_sample: u is not on the mesh set's device")
        if tuple(u.shape) != (B, n, 3):
            raise ValueError("mesh_sample: u must be (B, n, 3) = (%d, %d, 3)" % (B, n))
        kt = None
    else:
        if torch.is_tensor(keys):
            if keys.dtype != torch.int64 or not keys.is_contiguous():
                raise TypeError("mesh_sample: keys as a tensor must be contiguous int64 (the 64-bit keys' bits)")
            if keys.is_cuda and keys.device != dev:
                raise ValueError("mesh_sample: keys is not on the mesh set's device")
            kt = keys.to(dev)
        else:
            kt = torch.from_numpy(np.asarray([int(k) & (2 ** 64 - 1) for k in keys], dtype=np.uint64).view(np.int64)).to(dev)
        if tuple(kt.shape) != (B,):
            raise ValueError("mesh_sample: keys must be (B) = (%d)" % B)
    out = {"points": torch.empty(B, n, 6 if normals else 3, device=dev, dtype=dtype), "status": torch.empty(B, device=dev, dtype=torch.int32)}
    if return_face:
        out["face"] = torch.empty(B, n, device=dev, dtype=torch.int32)
    a = _lib.MeshSampleArgs(cdf=_p(meshset.area_cdf()), job_mesh=_p(jm), B=B, n=n, u=_p(u), keys=_p(kt), seed=int(seed) & (2 ** 64 - 1),
                            normals=int(bool(normals)), f32=int(dtype == torch.float32), out=_p(out["points"]), face=_p(out.get("face")),
                            status=_p(out["status"]), **meshset.fields())
    check(_lib.lib().tgp_mesh_sample(ctypes.byref(a), _stream(meshset.verts)), "tgp_mesh_sample")
    if check_status:
        mesh_check_status(out["status"])
    return out


def mesh_sample_fps(meshset, job_mesh, n, ratio=2, *, u=None, keys=None, seed=0, normals=False, dtype=torch.float32, check_status=False):
    """sample_points_from_mesh(fps=True): ratio * n surface samples per job (mesh_sample), thinned to the n that
    farthest_points(init_center=False) selects from their float32 coordinates (row 0 is the first centre, as in the reference), and
    the rows gathered in selection order -- three launches and a gather, nothing read back.  u, when given, is (B, ratio * n, 3).
    -> dict: points (B,n,3|6), index (B,n) int32 into the ratio * n samples, status (B)."""
    n, ratio = int(n), int(ratio)
    if n < 1 or ratio < 1:
        raise ValueError("mesh_sample_fps: n and ratio must be at least 1")
    if ratio * n > fps_max_points():
        raise ValueError("mesh_sample_fps: ratio * n = %d is above the cap of %d points" % (ratio * n, fps_max_points()))
    dense = mesh_sample(meshset, job_mesh, ratio * n, u=u, keys=keys, seed=seed, normals=normals, dtype=dtype, check_status=check_status)
    pts = dense["points"]
    xyz = pts[..., :3].to(torch.float32).contiguous()
    idx = farthest_points(xyz, n, init_center=False)
    rows = torch.gather(pts, 1, idx.long().unsqueeze(-1).expand(-1, -1, pts.shape[-1]))
    return {"points": rows, "index": idx, "status": dense["status"]}


def render_max_faces():
    return int(_lib.lib().tgp_render_max_faces())


def render_max_instances():
    return int(_lib.lib().tgp_render_max_instances())


def render_depth(meshset, scene_ptr, inst_mesh, inst_id, inst_pose, camk, H, W, near=0.01, return_z=False, return_face=False):
    """Depth frames and instance masks of posed meshes, S scenes in one call (tgp_render_depth, csrc/render.hip; the arithmetic is
    DESIGN.md section 3 "The depth renderer").  All tensors on the mesh set's GPU: scene_ptr (S+1) int32 into the instance arrays,
    inst_mesh (I) int32, inst_id (I) uint8 in 1..255, inst_pose (I,3,4) float32 [s R | t] (model -> camera, metres), camk (S,4)
    float32 = fx, fy, cx, cy.  -> dict: depth (S,H,W) uint16 millimetres and mask (S,H,W) uint8, 0 where no surface; visible (I)
    int32; bbox (I,4) int32 (y1,x1,y2,x2), exclusive ends, zeros when invisible; dropped (S,2) int32 (near rule, guard band);
    with return_z z (S,H,W) float32 metres, +inf where empty; with return_face face (S,H,W) int32, -1 where empty.
    Nothing synchronises, except that with more than render_max_instances() instances in all, scene_ptr is read back once to
    refuse a scene above the cap."""
    if not isinstance(meshset, MeshSet):
        raise TypeError("render_depth: meshset must be an ops.MeshSet")
    _gpu_args("render_depth", meshset.verts.device, [(scene_ptr, "scene_ptr", torch.int32), (inst_mesh, "inst_mesh", torch.int32),
                                                     (inst_id, "inst_id", torch.uint8), (inst_pose, "inst_pose", torch.float32),
                                                     (camk, "camk", torch.float32)])
    S, I = scene_ptr.numel() - 1, inst_mesh.numel()
    H, W = int(H), int(W)
    if S < 1 or scene_ptr.dim() != 1 or camk.shape != (S, 4) or inst_mesh.dim() != 1 or inst_id.shape != (I,) or inst_pose.shape != (I, 3, 4):
        raise ValueError("render_depth: scene_ptr (S+1), inst_mesh (I), inst_id (I), inst_pose (I,3,4), camk (S,4) are expected")
    if H < 1 or W < 1 or not float(near) > 0.0:
        raise ValueError("render_depth: H, W and near must be positive")
    cap = render_max_instances()
    longest = I if I <= cap else int((scene_ptr[1:] - scene_ptr[:-1]).max().item())
    if longest > cap:
        raise ValueError("render_depth: a scene of %d instances; the cap is %d" % (longest, cap))
    dev = inst_pose.device
    out = {"depth": torch.empty(S, H, W, device=dev, dtype=torch.uint16), "mask": torch.empty(S, H, W, device=dev, dtype=torch.uint8),
           "visible": torch.empty(I, device=dev, dtype=torch.int32), "bbox": torch.empty(I, 4, device=dev, dtype=torch.int32),
           "dropped": torch.empty(S, 2, device=dev, dtype=torch.int32)}
    if return_z:
        out["z"] = torch.empty(S, H, W, device=dev, dtype=torch.float32)
    if return_face:
        out["face"] = torch.empty(S, H, W, device=dev, dtype=torch.int32)
    mesh = meshset.fields(maxima=True)
    ws = _workspace(dev, _lib.lib().tgp_render_workspace_bytes(I, mesh["max_verts"], mesh["max_faces"]), "tgp_render_workspace_bytes")
    a = _lib.RenderArgs(scene_ptr=_p(scene_ptr), inst_mesh=_p(inst_mesh), inst_id=_p(inst_id), inst_pose=_p(inst_pose), camk=_p(camk),
                        S=S, I=I, max_scene_inst=longest, H=H, W=W, near=float(near), workspace=_p(ws), depth=_p(out["depth"]),
                        mask=_p(out["mask"]), z=_p(out.get("z")), face=_p(out.get("face")), visible=_p(out["visible"]),
                        bbox=_p(out["bbox"]), dropped=_p(out["dropped"]), **mesh)
    check(_lib.lib().tgp_render_depth(ctypes.byref(a), _stream(inst_pose)), "tgp_render_depth")
    return out


# the columns of pose_verify's counts
VERIFY_COUNTS = ("rendered", "match", "violation", "occluded", "nodata", "in_mask", "abs_sum", "dropped")
VERIFY_MAX_JOBS, VERIFY_MAX_TAU = _lib.VERIFY_MAX_JOBS, _lib.VERIFY_MAX_TAU


def pose_verify(meshset, depth, camk, job_img, job_mesh, job_pose, tau=5, near=0.01, mask=None, job_mask_val=None):
    """Render-and-compare of J poses against depth frames in one call (tgp_pose_verify, csrc/verify.hip; DESIGN.md section 3 "Pose
    verification").  Job j renders mesh job_mesh[j] of the set at job_pose[j] -- exactly render_depth's surface for that one instance
    -- inside its own projected box only, and compares it with frame job_img[j] pixel by pixel; no frame is written.  All tensors on
    the mesh set's GPU: depth (S,H,W) 16-bit millimetres (0: no data), camk (S,4) float32 = fx, fy, cx, cy, job_img and job_mesh (J)
    int32, job_pose (J,3,4) float32 [s R | t] (model -> camera, metres), mask (S,H,W) uint8 with job_mask_val (J) uint8, or neither.
    tau: the tolerance in millimetres, an int in [0, VERIFY_MAX_TAU].
    -> dict: counts (J,8) int32 in the order of VERIFY_COUNTS -- with d_r the rendered and d_o the frame's depth a covered pixel is
    nodata (d_o or d_r is 0), else occluded (d_o + tau < d_r), else match (|d_o - d_r| <= tau), else violation; in_mask: covered
    pixels whose mask byte is the job's; abs_sum: the sum of |d_o - d_r| over the match pixels; dropped: triangles the near rule and
    the guard band dropped -- and score (J) float32 = match / (rendered - occluded), 0 where nothing is left to compare.  A job whose
    frame or mesh index is out of range gives zeros.  Nothing synchronises."""
    if not isinstance(meshset, MeshSet):
        raise TypeError("pose_verify: meshset must be an ops.MeshSet")
    dev = meshset.verts.device
    S, H, W, J = _frame_jobs("pose_verify", dev, depth, camk, job_img, [(job_mesh, "job_mesh", torch.int32, ()),
                                                                         (job_pose, "job_pose", torch.float32, (3, 4))], mask, job_mask_val)
    if not (isinstance(tau, int) and 0 <= tau <= VERIFY_MAX_TAU):
        raise ValueError("pose_verify: tau must be an int in [0, %d] (millimetres)" % VERIFY_MAX_TAU)
    if not float(near) > 0.0:
        raise ValueError("pose_verify: near must be positive")
    if J > VERIFY_MAX_JOBS or H * W >= 2 ** 24:
        raise ValueError("pose_verify: at most %d jobs and frames of fewer than 2^24 pixels" % VERIFY_MAX_JOBS)
    out = {"counts": torch.empty(J, len(VERIFY_COUNTS), device=dev, dtype=torch.int32), "score": torch.empty(J, device=dev, dtype=torch.float32)}
    if J == 0:
        return out
    mesh = meshset.fields(maxima=True)
    ws = _workspace(dev, _lib.lib().tgp_verify_workspace_bytes(J, mesh["max_verts"], mesh["max_faces"]), "tgp_verify_workspace_bytes")
    a = _lib.VerifyArgs(depth=_p(depth), camk=_p(camk), job_img=_p(job_img), job_mesh=_p(job_mesh), job_pose=_p(job_pose), mask=_p(mask),
                        job_mask_val=_p(job_mask_val), S=S, H=H, W=W, J=J, tau=tau, near=float(near), counts=_p(out["counts"]),
                        score=_p(out["score"]), workspace=_p(ws), workspace_bytes=ws.numel(), **mesh)
    check(_lib.lib().tgp_pose_verify(ctypes.byref(a), _stream(job_pose)), "tgp_pose_verify")
    return out


# the columns of pose_errors' err and of pose_vsd's counts
POSE_ERRORS = ("add", "adi", "mssd", "mspd")
VSD_COUNTS = ("rendered_gt", "rendered_est", "visib_gt", "visib_est", "inter", "union", "dropped_gt", "dropped_est")
POSEERR_MAX_JOBS, POSEERR_MAX_SYMS, VSD_MAX_TAUS = _lib.POSEERR_MAX_JOBS, _lib.POSEERR_MAX_SYMS, _lib.VSD_MAX_TAUS
POSEERR_STATUS = {1: "mesh or symmetry index out of range", 2: "a projected point at or behind near (mspd is +inf)",
                  4: "a transformed point or an intrinsic is not finite (err is NaN)"}


class SymmetrySet(object):
    """Symmetry groups packed once for ops.pose_errors (tgp_pose_errors' table): ``groups`` is a list of (Q,3,4) arrays [R | t] in
    model units, 1 <= Q <= POSEERR_MAX_SYMS.  Group 0 is conventionally the identity alone (SymmetrySet.identity()).  Holds sym
    (sum Q,3,4) float32 and the prefix sums sptr (G+1) int32 on ``device``, and on the host the sizes."""

    def __init__(self, groups, device="cuda"):
        import numpy as np
        if not len(groups):
            raise ValueError("SymmetrySet: at least one group")
        gs = []
        for i, g in enumerate(groups):
            g = np.ascontiguousarray(g, dtype=np.float32)
            if g.ndim != 3 or g.shape[1:] != (3, 4) or not len(g):
                raise ValueError("SymmetrySet: group %d must be (Q,3,4) with Q >= 1" % i)
            if len(g) > POSEERR_MAX_SYMS:
                raise ValueError("SymmetrySet: group %d has %d transforms; the cap is %d" % (i, len(g), POSEERR_MAX_SYMS))
            gs.append(g)
        self.sizes = [len(g) for g in gs]
        self.device = torch.device(device)
        self.sym = torch.from_numpy(np.concatenate(gs)).to(self.device)
        self.sptr = torch.from_numpy(np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)).to(self.device)

    def __len__(self):
        return len(self.sizes)

    @staticmethod
    def identity():
        import numpy as np
        return np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None].astype(np.float32)


def pose_errors(meshset, job_mesh, pose_est, pose_gt, symset, job_sym, camk, near=0.01):
    """The point-based BOP pose errors of J (estimate, ground truth) pairs in one call (tgp_pose_errors, csrc/poseerr.hip;
    DESIGN.md section 3 "BOP pose errors").  Job j: the vertices of mesh job_mesh[j] of the set, pose_est[j] and pose_gt[j]
    (3,4) float32 [s R | t] (model -> camera, metres), group job_sym[j] of ``symset`` (ops.SymmetrySet) and camk[j] (4) float32
    = fx, fy, cx, cy -- one row per job.  All tensors on the mesh set's GPU; job_mesh, job_sym (J) int32.
    -> dict: err (J,4) float64 in the order of POSE_ERRORS -- add = mean |E p - G p|, adi = mean of the distance to the nearest
    ground-truth point, mssd = min over the group's S of max |E p - G S p|, mspd the same of the projections, in pixels;
    sym_best (J,2) int32: the group-local index that attains mssd and mspd; status (J) int32 bits: 1 an index out of range (NaN
    and -1), 2 a projected point without z > near (mspd = +inf); or 4 alone: a pose, a transform, a vertex or an intrinsic is not
    finite (NaN and -1: no threshold counts such a job as correct).  float64 throughout, fixed summation order, no atomics: two calls
    give identical bytes.  Nothing synchronises."""
    if not isinstance(meshset, MeshSet):
        raise TypeError("pose_errors: meshset must be an ops.MeshSet")
    if not isinstance(symset, SymmetrySet):
        raise TypeError("pose_errors: symset must be an ops.SymmetrySet")
    dev = meshset.verts.device
    _gpu_args("pose_errors", dev, [(job_mesh, "job_mesh", torch.int32), (pose_est, "pose_est", torch.float32), (pose_gt, "pose_gt", torch.float32),
                                   (job_sym, "job_sym", torch.int32), (camk, "camk", torch.float32), (symset.sym, "symset", torch.float32)])
    J = job_mesh.numel()
    if job_mesh.dim() != 1 or job_sym.shape != (J,) or pose_est.shape != (J, 3, 4) or pose_gt.shape != (J, 3, 4) or camk.shape != (J, 4):
        raise ValueError("pose_errors: job_mesh (J), job_sym (J), pose_est (J,3,4), pose_gt (J,3,4), camk (J,4) are expected")
    if not 0.0 < float(near) < float("inf"):
        raise ValueError("pose_errors: near must be positive and finite")
    if J > POSEERR_MAX_JOBS:
        raise ValueError("pose_errors: at most %d jobs" % POSEERR_MAX_JOBS)
    out = {"err": torch.empty(J, len(POSE_ERRORS), device=dev, dtype=torch.float64), "sym_best": torch.empty(J, 2, device=dev, dtype=torch.int32),
           "status": torch.empty(J, device=dev, dtype=torch.int32)}
    if J == 0:
        return out
    ws = _workspace(dev, _lib.lib().tgp_pose_errors_workspace_bytes(J), "tgp_pose_errors_workspace_bytes")
    a = _lib.PoseerrArgs(sym=_p(symset.sym), sptr=_p(symset.sptr), G=len(symset), n_syms=symset.sym.shape[0], max_syms=max(symset.sizes),
                         job_mesh=_p(job_mesh), job_sym=_p(job_sym), pose_est=_p(pose_est), pose_gt=_p(pose_gt), camk=_p(camk), J=J,
                         near=float(near), err=_p(out["err"]), sym_best=_p(out["sym_best"]), status=_p(out["status"]), workspace=_p(ws),
                         workspace_bytes=ws.numel(), **meshset.fields(faces=False))
    check(_lib.lib().tgp_pose_errors(ctypes.byref(a), _stream(pose_est)), "tgp_pose_errors")
    return out


def pose_vsd(meshset, depth, camk, job_img, job_mesh, pose_est, pose_gt, job_tau, delta=15, near=0.01):
    """Two-pose visible surface discrepancy of J jobs in one call (tgp_pose_vsd, csrc/vsd.hip; DESIGN.md section 3 "BOP pose
    errors").  Job j renders mesh job_mesh[j] at pose_est[j] and at pose_gt[j] -- each exactly render_depth's surface for that one
    instance, d_e and d_g in millimetres, 0 = not rendered -- and compares both with frame job_img[j]; no frame is written.  All
    tensors on the mesh set's GPU: depth (S,H,W) 16-bit millimetres (0: no data), camk (S,4) float32, job_img, job_mesh (J) int32,
    the poses (J,3,4) float32 [s R | t], job_tau (J,n_tau) int32 millimetres with 1 <= n_tau <= VSD_MAX_TAUS; delta: an int in
    [0, 65535], millimetres.
    -> dict: counts (J,8) int32 in the order of VSD_COUNTS -- vis(d) = d > 0 and (d_o == 0 or d - d_o <= delta); visib_gt =
    vis(d_g); visib_est = vis(d_e) or (visib_gt and d_e > 0); inter / union their AND / OR; dropped_*: triangles the near rule and
    the guard band dropped -- within (J,n_tau) int32: the inter pixels with |d_g - d_e| < tau; err (J,n_tau) float32 =
    (union - within) / union, 1 when union is 0.  BOP's vsd with visib_mode 'bop19' and cost_type 'step', on depth along the
    optical axis.  A job whose frame or mesh index is out of range gives zeros and err 1.  Nothing synchronises."""
    if not isinstance(meshset, MeshSet):
        raise TypeError("pose_vsd: meshset must be an ops.MeshSet")
    dev = meshset.verts.device
    n_tau = job_tau.shape[1] if torch.is_tensor(job_tau) and job_tau.dim() == 2 else 0                 # not a tensor: refused below
    if torch.is_tensor(job_tau) and not 1 <= n_tau <= VSD_MAX_TAUS:
        raise ValueError("pose_vsd: job_tau must be (J, n_tau) with n_tau in [1, %d]" % VSD_MAX_TAUS)
    S, H, W, J = _frame_jobs("pose_vsd", dev, depth, camk, job_img, [(job_mesh, "job_mesh", torch.int32, ()),
                                                                      (pose_est, "pose_est", torch.float32, (3, 4)),
                                                                      (pose_gt, "pose_gt", torch.float32, (3, 4)),
                                                                      (job_tau, "job_tau", torch.int32, (n_tau,), "J,n_tau")])
    if not (isinstance(delta, int) and 0 <= delta <= 65535):
        raise ValueError("pose_vsd: delta must be an int in [0, 65535] (millimetres)")
    if not 0.0 < float(near) < float("inf"):
        raise ValueError("pose_vsd: near must be positive and finite")
    if J > VERIFY_MAX_JOBS or H * W >= 2 ** 24:
        raise ValueError("pose_vsd: at most %d jobs and frames of fewer than 2^24 pixels" % VERIFY_MAX_JOBS)
    out = {"counts": torch.empty(J, len(VSD_COUNTS), device=dev, dtype=torch.int32), "within": torch.empty(J, n_tau, device=dev, dtype=torch.int32),
           "err": torch.empty(J, n_tau, device=dev, dtype=torch.float32)}
    if J == 0:
        return out
    mesh = meshset.fields(maxima=True)
    ws = _workspace(dev, _lib.lib().tgp_vsd_workspace_bytes(J, mesh["max_verts"], mesh["max_faces"]), "tgp_vsd_workspace_bytes")
    a = _lib.VsdArgs(depth=_p(depth), camk=_p(camk), job_img=_p(job_img), job_mesh=_p(job_mesh), pose_est=_p(pose_est), pose_gt=_p(pose_gt),
                     job_tau=_p(job_tau), S=S, H=H, W=W, J=J, n_tau=n_tau, delta=delta, near=float(near), counts=_p(out["counts"]),
                     within=_p(out["within"]), err=_p(out["err"]), workspace=_p(ws), workspace_bytes=ws.numel(), **mesh)
    check(_lib.lib().tgp_pose_vsd(ctypes.byref(a), _stream(pose_est)), "tgp_pose_vsd")
    return out


def canonicalize(points, gR, p_g, f_g, p_r, f_r, p_t, p_s, sym):
    """R_DCD pose normalisation -> (points_re_n (B,n,3), R (B,3,3))"""
    c = lambda t: _f32(t.contiguous(), "arg")
    points, gR, p_g, f_g, p_r, f_r, p_t, p_s, sym = map(c, (points, gR, p_g, f_g, p_r, f_r, p_t, p_s, sym))
    B, n, _ = points.shape
    out = torch.empty_like(points)
    R = torch.empty(B, 3, 3, device=points.device, dtype=torch.float32)
    check(_lib.lib().tgp_canonicalize(_p(points), _p(gR), _p(p_g), _p(f_g), _p(p_r), _p(f_r), _p(p_t), _p(p_s), _p(sym),
                                      sym.shape[1] if sym.dim() > 1 else 1, B, n, _p(out), _p(R), _stream(points)),
          "tgp_canonicalize")
    return out, R


def generate_rt(p_green, p_red, f_green, f_red, T, sym=None):
    """-> (B,4,4) pose matrices"""
    c = lambda t: _f32(t.contiguous(), "arg")
    p_green, p_red, f_green, f_red, T = map(c, (p_green, p_red, f_green.reshape(-1), f_red.reshape(-1), T))
    B = p_green.shape[0]
    out = torch.empty(B, 4, 4, device=p_green.device, dtype=torch.float32)
    sld = 0
    if sym is not None:
        sym = c(sym.float())
        sld = sym.shape[1] if sym.dim() > 1 else 1
    check(_lib.lib().tgp_generate_rt(_p(p_green), _p(p_red), _p(f_green), _p(f_red), _p(T), _p(sym), sld, B, _p(out),
                                     _stream(p_green)), "tgp_generate_rt")
    return out


def bn_train(x, gamma, beta, eps=1e-5, act=0, slope=0.0, slope_vec=None, out=None, colmax_keys=None, cm_cols=0,
             rows_per_obj=0, want_out=True, running=None):
    """Training-mode BatchNorm over rows: x (..., C) rows (row stride may exceed C).  Normalises (in place unless `out`),
    applies the activation, optionally feeds colmax keys.  Returns (out, batch_mean (C,), biased batch_var (C,)).
    running = (running_mean (C,), running_var (C,), momentum, num_batches_tracked or None): the module's buffers, updated by the
    statistics kernel itself (tgp_bn_stats_running) instead of by four torch launches."""
    x, ld = _rows(x, "x")
    C = x.shape[-1]
    rows = math.prod(x.shape[:-1])
    dev = x.device
    mean = torch.empty(C, device=dev, dtype=torch.float32)
    var = torch.empty(C, device=dev, dtype=torch.float32)
    ws = torch.empty(_lib.lib().tgp_bn_workspace_floats(rows, C), device=dev, dtype=torch.float32)
    if running is None:
        check(_lib.lib().tgp_bn_stats(_p(x), ld, rows, C, _p(mean), _p(var), _p(ws), _stream(x)), "tgp_bn_stats")
    else:
        rm, rv, momentum, nbt = running
        if not (rm.is_contiguous() and rv.is_contiguous() and rm.numel() == C and rv.numel() == C and rm.dtype == torch.float32):
            raise ValueError("bn_train: running statistics must be contiguous float32 (C,) tensors")
        if nbt is not None and nbt.dtype != torch.int64:
            raise ValueError("bn_train: num_batches_tracked must be int64")
        check(_lib.lib().tgp_bn_stats_running(_p(x), ld, rows, C, _p(mean), _p(var), _p(ws), _p(rm), _p(rv), float(momentum), _p(nbt),
                                              _stream(x)), "tgp_bn_stats_running")
    ldo = 0
    if want_out:
        out = x if out is None else out
        out, ldo = _rows(out, "out")
    else:
        out = None
    check(_lib.lib().tgp_bn_apply(_p(x), ld, rows, C, _p(mean), _p(var), _p(gamma), _p(beta), float(eps), act, float(slope),
                                  _p(slope_vec), _p(out), ldo, _p(colmax_keys),
                                  colmax_keys.stride(-2) if colmax_keys is not None else 0, cm_cols, rows_per_obj, _stream(x)),
          "tgp_bn_apply")
    return out, mean, var


def dropout(x, p, generator=None):
    """nn.Dropout(p) in train mode: the keep mask comes from torch's generator on the tensor's device."""
    if p <= 0.0:
        return x
    x = x.contiguous()
    keep = (torch.rand(x.shape, device=x.device, generator=generator) >= p).to(torch.uint8)
    y = torch.empty_like(x)
    check(_lib.lib().tgp_dropout_apply(_p(x), _p(keep), float(p), x.numel(), _p(y), _stream(x)), "tgp_dropout_apply")
    return y


# ------------------------------------------------------------------------------------------------- backward pass
def _ws(floats, dev):
    return torch.empty(max(int(floats), 1), device=dev, dtype=torch.float32)


FP16_TOP = 32768.0           # scaled gradients peak in [2^14, 2^15): a factor of two under fp16's largest finite value
TN_SPLIT = os.environ.get("TGP_TN_SPLIT", "1") != "0"    # backward GEMMs of large layers on the scaled fp16 split (0: bf16x3 / fp32 MFMA)
TN_SPLIT_MIN = 128 * 256     # smallest N * K routed to the split path
TN_NATIVE = os.environ.get("TGP_TN_NATIVE", "1") != "0"  # dW of the split path without transposed copies (0: transpose + NT kernel)


def absmax_scale(x, target=FP16_TOP):
    """-> device tensor {s, 1/s, max|x|}: s the largest power of two with max|x| * s <= target (chosen on the device)"""
    x, ld = _rows(x, "x")
    rows, cols = math.prod(x.shape[:-1]), x.shape[-1]
    ws = torch.empty(2048, device=x.device, dtype=torch.int32)
    out = torch.empty(3, device=x.device, dtype=torch.float32)
    check(_lib.lib().tgp_absmax_scale(_p(x), ld, rows, cols, float(target), _p(ws), _p(out), _stream(x)), "tgp_absmax_scale")
    return out


def _ksplit_plan(rows, tiles):
    """number of K-chunks Z and chunk length for a reduction over `rows` feeding `tiles` output tiles: fill whole rounds of the
    256 resident workgroups, keep a chunk >= 512 rows"""
    best, best_eff = 1, 0.0
    for Z in range(1, max(1, rows // 512) + 1):
        t = tiles * Z
        eff = t / (256.0 * ((t + 255) // 256))
        if eff > best_eff + 0.02:
            best, best_eff = Z, eff
        if t >= 1024:
            break
    chunk = ((rows + best - 1) // best + 15) // 16 * 16
    return best, chunk


def gemm_tn_split(a, b, scale, out=None, accumulate=False):
    """gemm_tn on the fp16 split kernels: out (N, K) (+)= a^T b, a = dy (rows, N) scaled into fp16's range by scale[0]
    (absmax_scale(a)), b = x (rows, K) activations.  a^T is transposed + scaled in fp32 and split on the fly as the GEMM's A
    operand, b^T transposed straight into fp16 planes; the reduction over the rows is cut into Z chunks whose partial
    products are added in order and unscaled by scale[1]."""
    a, lda = _rows(a.reshape(-1, a.shape[-1]) if a.dim() > 2 and a.is_contiguous() else a, "a")
    b, ldb = _rows(b.reshape(-1, b.shape[-1]) if b.dim() > 2 and b.is_contiguous() else b, "b")
    rows, N, K = math.prod(a.shape[:-1]), a.shape[-1], b.shape[-1]
    dev = a.device
    Z, chunk = _ksplit_plan(rows, ((N + 255) // 256) * ((K + 255) // 256))
    if TN_NATIVE and N % 4 == 0 and K % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0:
        # (round 3) the operands as they lie: transposed LDS reads instead of transposed copies (csrc/gemm_tn_split.hip)
        parts = torch.empty(Z, N, K, device=dev, dtype=torch.float32)
        check(_lib.lib().tgp_gemm_tn_split(_p(a), lda, _p(b), ldb, rows, N, K, _p(scale), Z, chunk, _p(parts), _stream(a)),
              "tgp_gemm_tn_split")
        if out is None:
            out = torch.empty(N, K, device=dev, dtype=torch.float32)
        if not out.is_contiguous():
            raise ValueError("gemm_tn_split: out must be contiguous")
        check(_lib.lib().tgp_sum_slabs(_p(parts), Z, N * K, _p(scale[1:]), _p(out), int(accumulate), _stream(a)), "tgp_sum_slabs")
        return out
    pad = Z * chunk
    at = torch.empty(N, pad, device=dev, dtype=torch.float32)
    check(_lib.lib().tgp_transpose_scaled(_p(a), lda, rows, N, _p(scale), _p(at), pad, _stream(a)), "tgp_transpose_scaled")
    bt = torch.empty(K, pad // 16, 2, 16, device=dev, dtype=torch.int16)
    check(_lib.lib().tgp_transpose_split_f16(_p(b), ldb, rows, K, None, _p(bt), pad, _stream(a)), "tgp_transpose_split_f16")
    parts = torch.empty(Z, N, K, device=dev, dtype=torch.float32)
    gemm(at, at, parts, M=N, N=K, K=chunk, lda=pad, ldw=pad, ldc=K, batch=Z, batch_strides=(chunk, 0, N * K, 0, 0), w_split=bt,
         ksplit_chunk=chunk)
    if out is None:
        out = torch.empty(N, K, device=dev, dtype=torch.float32)
    if not out.is_contiguous():
        raise ValueError("gemm_tn_split: out must be contiguous")
    check(_lib.lib().tgp_sum_slabs(_p(parts), Z, N * K, _p(scale[1:]), _p(out), int(accumulate), _stream(a)), "tgp_sum_slabs")
    return out


def sum_slabs(parts, scale, out=None, accumulate=False):
    """out (+)= scale[0] * sum over the leading dim of parts (Z, ...), slabs added in order (tgp_sum_slabs)"""
    Z = parts.shape[0]
    n = parts.numel() // Z
    if out is None:
        out = torch.empty(parts.shape[1:], device=parts.device, dtype=torch.float32)
    if not out.is_contiguous():
        raise ValueError("sum_slabs: out must be contiguous")
    check(_lib.lib().tgp_sum_slabs(_p(parts), Z, n, _p(scale), _p(out), int(accumulate), _stream(parts)), "tgp_sum_slabs")
    return out


def tn_split_ok(rows, N, K):
    """does gemm_tn route (rows, N)^T (rows, K) to the fp16 split path?  Large enough for the tile kernels in both output dims."""
    if not (TN_SPLIT and GEMM_MODE == "split16" and rows >= 2048 and N * K >= TN_SPLIT_MIN and N > 32 and K > 64):
        return False
    Z, _ = _ksplit_plan(rows, ((N + 255) // 256) * ((K + 255) // 256))
    return _routes_to_big_tile(N, K, Z)


def gemm_tn(a, b, out=None, accumulate=False, scale=None):
    """out (N, K) (+)= a^T b over the rows: a (rows, N), b (rows, K) row views (row stride >= width).  dW = dx^T x.
    scale: absmax_scale(a) if the caller already has it (the same dy feeds the dx GEMM)."""
    a, lda = _rows(a.reshape(-1, a.shape[-1]) if a.dim() > 2 and a.is_contiguous() else a, "a")
    b, ldb = _rows(b.reshape(-1, b.shape[-1]) if b.dim() > 2 and b.is_contiguous() else b, "b")
    rows, N, K = math.prod(a.shape[:-1]), a.shape[-1], b.shape[-1]
    if math.prod(b.shape[:-1]) != rows:
        raise ValueError("gemm_tn: row counts differ")
    if tn_split_ok(rows, N, K) and (out is None or out.is_contiguous()):
        return gemm_tn_split(a, b, absmax_scale(a) if scale is None else scale, out, accumulate)
    if out is None:
        out = torch.empty(N, K, device=a.device, dtype=torch.float32)
    out, ldc = _rows(out, "out")
    ws = _ws(_lib.lib().tgp_gemm_tn_workspace_floats(rows, N, K), a.device)
    check(_lib.lib().tgp_gemm_tn_f32(_p(a), lda, _p(b), ldb, rows, N, K, _p(out), ldc, int(accumulate), _p(ws), _stream(a)),
          "tgp_gemm_tn_f32")
    return out


def colsum(dy, out=None, accumulate=False):
    dy, ld = _rows(dy, "dy")
    rows, C = math.prod(dy.shape[:-1]), dy.shape[-1]
    if out is None:
        out = torch.empty(C, device=dy.device, dtype=torch.float32)
    ws = _ws(_lib.lib().tgp_bw_workspace_floats(rows, C), dy.device)
    check(_lib.lib().tgp_colsum(_p(dy), ld, rows, C, _p(out), int(accumulate), _p(ws), _stream(dy)), "tgp_colsum")
    return out


def bn_bwd(dy, x, mean, var, gamma, beta, eps=1e-5, act=0, slope=0.0, slope_vec=None, dx=None, want_scale=False):
    """Backward of y = act(BatchNorm_train(x)) over rows.  Returns (dx, dgamma, dbeta); dx defaults to in place on dy.
    want_scale: also absmax_scale(dx), collected by the apply pass itself (attached to dx as ``_tgp_scale`` for the linear layer
    whose backward consumes dx next; skipped when the operands do not take the 16-byte form)."""
    dy, lddy = _rows(dy, "dy")
    x, ld = _rows(x, "x")
    rows, C = math.prod(x.shape[:-1]), x.shape[-1]
    dx = dy if dx is None else dx
    dx, lddx = _rows(dx, "dx")
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws = _ws(_lib.lib().tgp_bw_workspace_floats(rows, C), x.device)
    bits = None
    if want_scale and C % 4 == 0 and lddy % 4 == 0 and ld % 4 == 0 and lddx % 4 == 0 and \
            all(t.data_ptr() % 16 == 0 for t in (dy, x, dx, ws)):
        bits = torch.empty(int(_lib.lib().tgp_bn_bwd_absmax_words(rows, C)), device=x.device, dtype=torch.int32)
    check(_lib.lib().tgp_bn_bwd(_p(dy), lddy, _p(x), ld, rows, C, _p(mean), _p(var), float(eps), _p(gamma), _p(beta), act,
                                float(slope), _p(slope_vec), _p(dx), lddx, _p(dg), _p(db), _p(ws), _p(bits), _stream(x)), "tgp_bn_bwd")
    if bits is not None:
        sc = torch.empty(3, device=x.device, dtype=torch.float32)
        check(_lib.lib().tgp_absmax_scale_from_bits(_p(bits), bits.numel(), float(FP16_TOP), _p(sc), _stream(x)),
              "tgp_absmax_scale_from_bits")
        dx._tgp_scale = sc
    return dx, dg, db


def bn_bwd_pooled(dpool, argrow, x, rows_per_obj, mean, var, gamma, beta, eps=1e-5, act=0, slope=0.0, slope_vec=None, dx=None):
    """Backward of max-over-points(act(BatchNorm_train(x))): dpool (objects, C), argrow (objects, C) int32 -> dense dx."""
    x, ld = _rows(x, "x")
    objects, C = dpool.shape
    if dx is None:
        dx = torch.empty(objects * rows_per_obj, C, device=x.device, dtype=torch.float32)
    dx, lddx = _rows(dx, "dx")
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    check(_lib.lib().tgp_bn_bwd_pooled(_p(dpool), dpool.stride(0), _p(argrow), argrow.stride(0), _p(x), ld, objects, rows_per_obj,
                                       C, _p(mean), _p(var), float(eps), _p(gamma), _p(beta), act, float(slope), _p(slope_vec),
                                       _p(dx), lddx, _p(dg), _p(db), _stream(x)), "tgp_bn_bwd_pooled")
    return dx, dg, db


def colmax_arg(x, objects, n, bn=None, act=0, slope=0.0, slope_vec=None, eps=1e-5):
    """max over each object's n rows (+ winning global row, int32) of act(BN(x)); bn = (mean, var, gamma, beta) or None."""
    x, ld = _rows(x, "x")
    C = x.shape[-1]
    out = torch.empty(objects, C, device=x.device, dtype=torch.float32)
    arg = torch.empty(objects, C, device=x.device, dtype=torch.int32)
    mean, var, gamma, beta = bn if bn is not None else (None, None, None, None)
    check(_lib.lib().tgp_colmax_arg(_p(x), ld, objects, n, C, _p(mean), _p(var), float(eps), _p(gamma), _p(beta), act,
                                    float(slope), _p(slope_vec), _p(out), out.stride(0), _p(arg), arg.stride(0), _stream(x)),
          "tgp_colmax_arg")
    return out, arg


def colsum_objects(dy):
    """dy (B, n, C) rows -> (B, C): sum over each object's points, fixed order"""
    dy, ld = _rows(dy, "dy")
    B, n, C = dy.shape
    out = torch.empty(B, C, device=dy.device, dtype=torch.float32)
    check(_lib.lib().tgp_colsum_objects(_p(dy), ld, B, n, C, _p(out), C, _stream(dy)), "tgp_colsum_objects")
    return out


def colmax_bwd(dpool, argrow, rows_per_obj, dx=None):
    """backward of colmax_arg(x) without BatchNorm: dpool (objects, C), argrow (objects, C) int32 -> dense dx (objects * n, C)"""
    objects, C = dpool.shape
    if dx is None:
        dx = torch.empty(objects * rows_per_obj, C, device=dpool.device, dtype=torch.float32)
    dx, lddx = _rows(dx, "dx")
    check(_lib.lib().tgp_colmax_bwd(_p(dpool), dpool.stride(0), _p(argrow), argrow.stride(0), objects, rows_per_obj, C, _p(dx), lddx,
                                    _stream(dpool)), "tgp_colmax_bwd")
    return dx


def transpose(w):
    """(rows, cols) -> contiguous (cols, rows)"""
    w, ld = _rows(w, "w")
    rows, cols = w.shape
    out = torch.empty(cols, rows, device=w.device, dtype=torch.float32)
    check(_lib.lib().tgp_transpose(_p(w), ld, rows, cols, _p(out), rows, _stream(w)), "tgp_transpose")
    return out


def transpose_both(w):
    """w (rows, cols) -> (wt (cols, rows16) fp32 = w^T zero padded to a multiple of 16 columns, split_f16(wt)) in one launch"""
    w, ld = _rows(w, "w")
    rows, cols = w.shape
    pad = (rows + 15) // 16 * 16
    wt = torch.empty(cols, pad, device=w.device, dtype=torch.float32)
    planes = torch.empty(cols, pad // 16, 2, 16, device=w.device, dtype=torch.int16)
    check(_lib.lib().tgp_transpose_both(_p(w), ld, rows, cols, _p(wt), _p(planes), pad, _stream(w)), "tgp_transpose_both")
    return wt, planes


def _gconv_bwd_width(C, name):
    # tgp_gconv_surface_bwd / tgp_gconv_hs_bwd stage two 16-point streams per workgroup: 256 / C <= 2
    if C < 128:
        raise ValueError("%s: C = %d is not supported, the scatter backward needs C >= 128 (and 256 %% C == 0 or C %% 256 == 0)" % (name, C))


def gconv_surface_bwd(xyz, idx, sdn, dg, S, C):
    """-> dsdn (3, S*C)"""
    _gconv_bwd_width(C, "gconv_surface_bwd")
    dg, ldg = _rows(dg, "dg")
    B, n, k = idx.shape
    dsdn = torch.empty(3, S * C, device=xyz.device, dtype=torch.float32)
    ws = _ws(_lib.lib().tgp_gconv_bwd_workspace_floats(B, n, C), xyz.device)
    check(_lib.lib().tgp_gconv_surface_bwd(_p(xyz), _p(idx), _p(sdn), _p(dg), ldg, B, n, k, S, C, _p(dsdn), _p(ws), _stream(xyz)),
          "tgp_gconv_surface_bwd")
    return dsdn


def gconv_hs_bwd(xyz, idx, proj, sdn, dg, S, C):
    """-> (dproj (B,n,8C) = [d centre | d support], dsdn (3, S*C))"""
    _gconv_bwd_width(C, "gconv_hs_bwd")
    proj, ldp = _rows(proj, "proj")
    dg, ldg = _rows(dg, "dg")
    B, n, k = idx.shape
    dproj = torch.zeros(B, n, 8 * C, device=xyz.device, dtype=torch.float32)
    dsdn = torch.empty(3, S * C, device=xyz.device, dtype=torch.float32)
    ws = _ws(_lib.lib().tgp_gconv_bwd_workspace_floats(B, n, C), xyz.device)
    check(_lib.lib().tgp_gconv_hs_bwd(_p(xyz), _p(idx), _p(proj), ldp, _p(sdn), _p(dg), ldg, B, n, k, S, C, _p(dproj), 8 * C,
                                      _p(dsdn), _p(ws), _stream(xyz)), "tgp_gconv_hs_bwd")
    return dproj, dsdn


def nbrmax_bwd(src, idx, dy, per_object=False, scale=1.0, dsrc=None):
    """backward of y[b,p] = max_j src[b, idx[b,p,j]]: idx (B, n_rows, k) int32; dy (B,n_rows,C) or (B,C) when per_object."""
    src, lds = _rows(src, "src")
    _i32(idx, "idx")
    B, n_src, C = src.shape
    n_rows, k = idx.shape[1], idx.shape[2]
    dy, lddy = _rows(dy, "dy")
    if dsrc is None:
        dsrc = torch.zeros(B, n_src, C, device=src.device, dtype=torch.float32)
    dsrc, ldds = _rows(dsrc, "dsrc")
    check(_lib.lib().tgp_nbrmax_bwd(_p(src), lds, _p(idx), B, n_src, n_rows, k, C, _p(dy), lddy, int(per_object), float(scale),
                                    _p(dsrc), ldds, _stream(src)), "tgp_nbrmax_bwd")
    return dsrc


def gather_rows_bwd(dy, idx, n_src):
    """backward of gather_rows: dy (B,n_out,C) rows, idx (B,n_out) int32 -> dsrc (B,n_src,C)"""
    dy, lddy = _rows(dy, "dy")
    _i32(idx, "idx")
    B, n_out, C = dy.shape
    dsrc = torch.zeros(B, n_src, C, device=dy.device, dtype=torch.float32)
    check(_lib.lib().tgp_gather_rows_bwd(_p(dy), lddy, _p(idx), B, n_src, n_out, C, _p(dsrc), C, _stream(dy)),
          "tgp_gather_rows_bwd")
    return dsrc


def pose_rotation_fwd(gR0, p_g, f_g, p_r, f_r, sym0):
    """-> R (B,3,3), J (B,9,8): tgp_pose_rotation_fwd (all inputs float32, contiguous, on the device)"""
    B = p_g.shape[0]
    R = torch.empty(B, 3, 3, device=p_g.device, dtype=torch.float32)
    J = torch.empty(B, 9, 8, device=p_g.device, dtype=torch.float32)
    check(_lib.lib().tgp_pose_rotation_fwd(_p(gR0), _p(p_g), _p(f_g), _p(p_r), _p(f_r), _p(sym0), B, _p(R), _p(J), _stream(p_g)),
          "tgp_pose_rotation_fwd")
    return R, J


def pose_rotation_bwd(dR, J):
    B = J.shape[0]
    din = torch.empty(B, 8, device=J.device, dtype=torch.float32)
    check(_lib.lib().tgp_pose_rotation_bwd(_p(dR), _p(J), B, _p(din), _stream(J)), "tgp_pose_rotation_bwd")
    return din


def reverse_graph(idx, n_src):
    """idx (B, n_rows, k) int32 ids in [0, n_src) -> (rptr (B*n_src + 1,), rent (B*n_rows*k,)) int32: for every source row the
    ascending (row << 6 | slot) pairs that list it; None when the shape is outside what tgp_reverse_graph sorts in LDS"""
    _i32(idx, "idx")
    idx = idx.contiguous()
    B, n_rows, k = idx.shape
    if k > 64 or n_src > 8192 or (n_rows * k + 2 * n_src) * 4 > 150 * 1024:
        return None
    rptr = torch.empty(B * n_src + 1, device=idx.device, dtype=torch.int32)
    rent = torch.empty(B * n_rows * k, device=idx.device, dtype=torch.int32)
    check(_lib.lib().tgp_reverse_graph(_p(idx), B, n_rows, k, n_src, _p(rptr), _p(rent), _stream(idx)), "tgp_reverse_graph")
    return rptr, rent


def nbrmax_gather_ok(C, *tensors):
    lanes = C // 4
    return C % 4 == 0 and 0 < lanes <= 256 and 256 % lanes == 0 and all(t.data_ptr() % 16 == 0 for t in tensors)


@_timed("graph")
def nbrmax_bwd_gather(src, idx, rev, dy, per_object=False, scale=1.0):
    """nbrmax_bwd without atomics (rev = reverse_graph(idx, n_src)); dsrc is written densely"""
    src, lds = _rows(src, "src")
    _i32(idx, "idx")
    B, n_src, C = src.shape
    n_rows, k = idx.shape[1], idx.shape[2]
    dy, lddy = _rows(dy, "dy")
    dsrc = torch.empty(B, n_src, C, device=src.device, dtype=torch.float32)
    arg = torch.empty(B * n_rows * C, device=src.device, dtype=torch.uint8)
    check(_lib.lib().tgp_nbrmax_bwd_gather(_p(src), lds, _p(idx), _p(rev[0]), _p(rev[1]), B, n_src, n_rows, k, C, _p(dy), lddy,
                                           int(per_object), float(scale), _p(arg), _p(dsrc), C, _stream(src)), "tgp_nbrmax_bwd_gather")
    return dsrc


def gconv_gather_ok(C, k, *tensors):
    return C in (128, 256, 512) and k <= 63 and all(t.data_ptr() % 16 == 0 for t in tensors)


@_timed("graph")
def gconv_hs_slots(xyz, idx, proj, sdn, S, C):
    """gconv_hs that also records the winning slots for gconv_hs_bwd_gather(slots=...): -> (out (B,n,C), slots uint8 (B*n*S*C,))"""
    _f32(xyz, "xyz", 3), _i32(idx, "idx")
    proj, ldp = _rows(proj, "proj")
    B, n, k = idx.shape
    out = torch.empty(B, n, C, device=xyz.device, dtype=torch.float32)
    slots = torch.empty(B * n * S * C, device=xyz.device, dtype=torch.uint8)
    check(_lib.lib().tgp_gconv_hs_fwd_slots(_p(xyz), _p(idx), _p(proj), ldp, _p(sdn), B, n, k, S, C, _p(out), C, _p(slots),
                                            _stream(xyz)), "tgp_gconv_hs_fwd_slots")
    return out, slots


@_timed("graph")
def gconv_hs_bwd_gather(xyz, idx, rev, proj, sdn, dg, S, C, slots=None):
    """gconv_hs_bwd without atomics (rev = reverse_graph(idx, n)) -> (dproj (B,n,8C), dsdn (3, S*C)).  slots: as recorded by
    gconv_hs_slots in the forward (CONSUMED: entries that carry no gradient are rewritten); None: recomputed here."""
    proj, ldp = _rows(proj, "proj")
    dg, ldg = _rows(dg, "dg")
    B, n, k = idx.shape
    dproj = torch.empty(B, n, 8 * C, device=xyz.device, dtype=torch.float32)
    dsdn = torch.empty(3, S * C, device=xyz.device, dtype=torch.float32)
    ws = _ws(_lib.lib().tgp_gconv_bwd_workspace_floats(B, n, C), xyz.device)
    arg = slots if slots is not None else torch.empty(B * n * S * C, device=xyz.device, dtype=torch.uint8)
    contrib = torch.empty(B * n * S * C, device=xyz.device, dtype=torch.float32)
    check(_lib.lib().tgp_gconv_hs_bwd_gather(_p(xyz), _p(idx), _p(rev[0]), _p(rev[1]), _p(proj), ldp, _p(sdn), _p(dg), ldg, B, n, k, S, C,
                                             _p(dproj), 8 * C, _p(dsdn), _p(ws), _p(arg), _p(contrib), int(slots is not None),
                                             _stream(xyz)), "tgp_gconv_hs_bwd_gather")
    return dproj, dsdn


def child_lists(near, R, global_ids=False):
    """near (B, n) int32 parent of every point, in [0, R) (global_ids: b * R + that) -> (ptr (B*R + 1,), idx (B*n,)) int32: CSR
    child lists over the B*R global parent rows, idx = global point rows b*n + i, children in point order"""
    _i32(near, "near")
    near = near.contiguous()
    B, n = near.shape
    ptr = torch.empty(B * R + 1, device=near.device, dtype=torch.int32)
    idx = torch.empty(B * n, device=near.device, dtype=torch.int32)
    check(_lib.lib().tgp_child_lists(_p(near), B, n, R, 1 if global_ids else 0, _p(ptr), _p(idx), _stream(near)), "tgp_child_lists")
    return ptr, idx


@_timed("graph")
def segsum_rows(g, ptr, idx, out=None):
    """g (M, C) rows -> out (R, C), R = ptr.numel() - 1: out[r] = sum of g[idx[k]] over k in [ptr[r], ptr[r+1]); out may be a
    column slice of a wider buffer"""
    g, ldg = _rows(g, "g")
    C = g.shape[-1]
    R = ptr.numel() - 1
    if out is None:
        out = torch.empty(R, C, device=g.device, dtype=torch.float32)
    out, ldo = _rows(out, "out")
    if tuple(out.shape) != (R, C):
        raise ValueError("segsum_rows: out must be (%d, %d)" % (R, C))
    check(_lib.lib().tgp_segsum_rows(_p(g), ldg, C, _p(ptr), _p(idx), R, _p(out), ldo, _stream(g)), "tgp_segsum_rows")
    return out


def pose_transform(points, R, t, s):
    """out = (R^T (points - t)) * s per object: points (B,n,3), R (B,3,3), t, s (B,3)"""
    points, R, t, s = points.contiguous(), R.contiguous(), t.contiguous(), s.contiguous()
    B, n, _ = points.shape
    out = torch.empty_like(points)
    check(_lib.lib().tgp_pose_transform_fwd(_p(points), _p(R), _p(t), _p(s), B, n, _p(out), _stream(points)), "tgp_pose_transform_fwd")
    return out


def pose_transform_bwd(points, R, t, s, dout, need_points=True):
    points, R, t, s, dout = points.contiguous(), R.contiguous(), t.contiguous(), s.contiguous(), dout.contiguous()
    B, n, _ = points.shape
    dev = points.device
    dp = torch.empty_like(points) if need_points else None
    dR = torch.empty(B, 3, 3, device=dev, dtype=torch.float32)
    dt = torch.empty(B, 3, device=dev, dtype=torch.float32)
    ds = torch.empty(B, 3, device=dev, dtype=torch.float32)
    check(_lib.lib().tgp_pose_transform_bwd(_p(points), _p(R), _p(t), _p(s), _p(dout), B, n, _p(dp), _p(dR), _p(dt), _p(ds),
                                            _stream(points)), "tgp_pose_transform_bwd")
    return dp, dR, dt, ds


# ---- the regression terms of the training loss (csrc/tdaloss.hip) ---------------------------------------------------------

def sym_i32(sym):
    """sym_info as the kernels read it: (B, S) int32, contiguous"""
    if sym.dim() != 2:
        raise ValueError("sym must be (B, S)")
    return sym.to(torch.int32).contiguous()


def _pose_args(pred, gt, sym, kind, beta):
    B = pred[0].shape[0]
    for t in tuple(pred) + tuple(gt):
        _f32(t, "pose term operand")
        if t.shape[0] != B or not t.is_contiguous():
            raise ValueError("pose term operands must be contiguous with %d rows" % B)
    if sym.dtype != torch.int32 or sym.shape[0] != B or not sym.is_contiguous():
        raise ValueError("sym must be (B, S) int32 contiguous (ops.sym_i32)")
    return [_p(t) for t in pred] + [_p(t) for t in gt] + [_p(sym), sym.shape[1], B, int(kind), float(beta)]


def pose_terms_fwd(pred, gt, sym, kind=0, beta=0.5):
    """pred = (rot1, rot2, f1, f2, tran, size), gt = (rot1, rot2, tran, size) -> 9 floats: the eight unweighted terms + valid count"""
    out = torch.empty(9, device=pred[0].device, dtype=torch.float32)
    check(_lib.lib().tgp_pose_terms_fwd(*_pose_args(pred, gt, sym, kind, beta), _p(out), _stream(out)), "tgp_pose_terms_fwd")
    return out


def pose_terms_bwd(pred, gt, sym, kind, beta, fwd_out, gw):
    grads = [torch.empty_like(t) for t in pred]
    d = dict(zip(("rot1", "rot2", "f1", "f2", "tran", "size"), grads))
    check(_lib.lib().tgp_pose_terms_bwd(*_pose_args(pred, gt, sym, kind, beta), _p(fwd_out), _p(gw), _p(d["rot1"]), _p(d["rot2"]),
                                        _p(d["f1"]), _p(d["f2"]), _p(d["tran"]), _p(d["size"]), _stream(fwd_out)), "tgp_pose_terms_bwd")
    return grads


def _sym_recon_args(PC, PC_re, gt_R, gt_t, sym):
    for t, n in ((PC, "PC"), (PC_re, "PC_re"), (gt_R, "gt_R"), (gt_t, "gt_t")):
        _f32(t, n)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % n)
    B, N, _ = PC.shape
    if PC_re.shape != PC.shape or gt_R.shape != (B, 3, 3) or gt_t.shape != (B, 3) or sym.shape[0] != B or sym.dtype != torch.int32:
        raise ValueError("prop_sym_matching_loss operand shapes")
    return [_p(PC), _p(PC_re), _p(gt_R), _p(gt_t), _p(sym), sym.shape[1], sym.shape[1], B, N]


def sym_recon_fwd(PC, PC_re, gt_R, gt_t, sym):
    B, N, _ = PC.shape
    ws = torch.empty(int(_lib.lib().tgp_sym_recon_workspace_floats(B, N)), device=PC.device, dtype=torch.float32)
    loss = torch.empty(1, device=PC.device, dtype=torch.float32)
    check(_lib.lib().tgp_sym_recon_fwd(*_sym_recon_args(PC, PC_re, gt_R, gt_t, sym), _p(ws), _p(loss), _stream(PC)), "tgp_sym_recon_fwd")
    return loss


def sym_recon_bwd(PC, PC_re, gt_R, gt_t, sym, gloss, need_pc, need_re):
    dPC = torch.empty_like(PC) if need_pc else None
    dRe = torch.empty_like(PC_re) if need_re else None
    check(_lib.lib().tgp_sym_recon_bwd(*_sym_recon_args(PC, PC_re, gt_R, gt_t, sym), _p(gloss), _p(dPC), _p(dRe), _stream(PC)),
          "tgp_sym_recon_bwd")
    return dPC, dRe


def rowl1_fwd(a, b, wsrc):
    for t in (a, b, wsrc):
        _f32(t, "rowl1 operand", 2)
    if a.shape != b.shape or a.shape != wsrc.shape or not (a.is_contiguous() and b.is_contiguous() and wsrc.is_contiguous()):
        raise ValueError("rowl1 operands must be contiguous and of one shape")
    B, D = a.shape
    rows = torch.empty(B, 4, device=a.device, dtype=torch.float32)
    out = torch.empty(2, device=a.device, dtype=torch.float32)
    check(_lib.lib().tgp_rowl1_fwd(_p(a), _p(b), _p(wsrc), B, D, _p(rows), _p(out), _stream(a)), "tgp_rowl1_fwd")
    return out, rows


def rowl1_bwd(a, b, rows, fwd_out, gout):
    B, D = a.shape
    da = torch.empty_like(a)
    check(_lib.lib().tgp_rowl1_bwd(_p(a), _p(b), _p(rows), _p(fwd_out), _p(gout), B, D, _p(da), _stream(a)), "tgp_rowl1_bwd")
    return da


def feat_consistency_fwd(x1, x2):
    _f32(x1, "x1", 2), _f32(x2, "x2", 2)
    if x1.shape != x2.shape or not (x1.is_contiguous() and x2.is_contiguous()):
        raise ValueError("feat_consistency operands must be contiguous and of one shape")
    B, C = x1.shape
    rows = torch.empty(B, 3, device=x1.device, dtype=torch.float32)
    loss = torch.empty(1, device=x1.device, dtype=torch.float32)
    check(_lib.lib().tgp_feat_consistency_fwd(_p(x1), _p(x2), B, C, _p(rows), _p(loss), _stream(x1)), "tgp_feat_consistency_fwd")
    return loss, rows


def feat_consistency_bwd(x1, x2, rows, gloss, need1, need2):
    B, C = x1.shape
    d1 = torch.empty_like(x1) if need1 else None
    d2 = torch.empty_like(x2) if need2 else None
    check(_lib.lib().tgp_feat_consistency_bwd(_p(x1), _p(x2), _p(rows), _p(gloss), B, C, _p(d1), _p(d2), _stream(x1)),
          "tgp_feat_consistency_bwd")
    return d1, d2


# ----------------------------------------------------------------------------- input side (depth image -> cloud)
class RoiRecords:
    """What tgp_roi_cloud leaves in HBM: ``recs`` (D, roi^2) int32-viewed records (ROI pixel index << 16 | depth), ``counts``
    (D,3) int32, and the descriptor tensors a record needs to become a point (``det_img``, ``window``, ``camk``)."""

    def __init__(self, recs, counts, det_img, window, camk, roi_size, tables=None):
        self.recs, self.counts, self.det_img, self.window, self.camk, self.roi_size = recs, counts, det_img, window, camk, roi_size
        self.tables = tables


def _roi_args(depth, masks, mask_off, mask_stride, det_img, window, camk, roi_size, tables, mask_val, who):
    """the checks roi_cloud and roi_band share -> (I, H, W, D)"""
    if not (depth.is_cuda and depth.dtype in (torch.int16, torch.uint16) and depth.dim() == 3 and depth.is_contiguous()):
        raise TypeError("depth must be a contiguous (I,H,W) 16-bit GPU tensor")
    if not (masks.is_cuda and masks.dtype in (torch.uint8, torch.bool) and masks.is_contiguous()):
        raise TypeError("masks must be a contiguous uint8 / bool GPU tensor")
    if not (mask_off.is_cuda and mask_off.dtype == torch.int64 and mask_off.is_contiguous()):
        raise TypeError("mask_off must be a contiguous int64 GPU tensor")
    _i32(mask_stride, "mask_stride"), _i32(det_img, "det_img")
    I, H, W = depth.shape
    D = det_img.numel()
    if window is None and tables is None:
        raise ValueError("%s: a window or source tables are needed" % who)
    if window is not None and _i32(window, "window").shape != (D, 3):
        raise ValueError("%s: window must be (D,3)" % who)
    if tables is not None and _i32(tables, "tables").shape != (D, 2, roi_size):
        raise ValueError("%s: tables must be (D,2,roi_size)" % who)
    if mask_val is not None and _i32(mask_val, "mask_val").numel() != D:
        raise ValueError("%s: mask_val must be (D,)" % who)
    if mask_off.numel() != D or mask_stride.numel() != D or (camk is not None and (camk.shape != (I, 4) or not camk.is_contiguous())):
        raise ValueError("%s: inconsistent shapes" % who)
    return I, H, W, D


def roi_band(depth, masks, mask_off, mask_stride, det_img, window, roi_size=256, tables=None, mask_val=None):
    """tgp_roi_band: the band launch of the mask deformation (defor_2D).  Arguments as roi_cloud.  -> (D,3) int32 GPU tensor:
    depth-valid ROI pixels, valid points with the undeformed mask, band size l (pixels whose mask differs from the up or left
    ROI neighbour's)"""
    _, H, W, D = _roi_args(depth, masks, mask_off, mask_stride, det_img, window, None, roi_size, tables, mask_val, "roi_band")
    out = torch.empty(D, 3, device=depth.device, dtype=torch.int32)
    check(_lib.lib().tgp_roi_band(_p(depth), _p(masks), _p(mask_off), _p(mask_stride), _p(det_img), _p(window), D, H, W, roi_size,
                                  _p(out), _p(tables), _p(mask_val), _stream(depth)), "tgp_roi_band")
    return out


def roi_cloud(depth, masks, mask_off, mask_stride, det_img, window, camk, roi_size=256, tables=None, mask_val=None, cut_frac=0.25,
              defor=None):
    """tgp_roi_cloud / tgp_roi_cloud_ex.  depth (I,H,W) int16-viewed uint16, masks flat uint8, mask_off (D,) int64, mask_stride /
    det_img (D,) int32, window (D,3) int32 (None with tables), camk (I,4) float32 -- all on the GPU.  tables (D,2,roi_size) int32:
    host-evaluated source pixels (the training loader's augmented windows); mask_val (D,) int32: mask byte to match (ground-truth
    instance masks); cut_frac: the outlier cut's share of the diagonal (0.25 evaluation, 0.15 training).
    defor = (defor_on (D,) int32, drop_bits (D, words) int32 viewed as uint32 bitmaps over band ranks): the mask deformation
    (tgp_roi_cloud_defor); cut_frac may then be -1 (no cut).  -> RoiRecords"""
    _f32(camk, "camk", 2)
    I, H, W, D = _roi_args(depth, masks, mask_off, mask_stride, det_img, window, camk, roi_size, tables, mask_val, "roi_cloud")
    if defor is not None:
        on, bits = defor
        _i32(on, "defor_on"), _i32(bits, "drop_bits")
        if on.numel() != D or bits.dim() != 2 or bits.shape[0] != D or bits.shape[1] > 2048:
            raise ValueError("roi_cloud: defor must be (defor_on (D,), drop_bits (D, words <= 2048))")
        if not (0.0 <= cut_frac <= 1.0 or cut_frac == -1.0):
            raise ValueError("roi_cloud: cut_frac must be in [0, 1] or -1 (no cut)")
    recs = torch.empty(D, roi_size * roi_size, device=depth.device, dtype=torch.int32)
    counts = torch.empty(D, 3, device=depth.device, dtype=torch.int32)
    if defor is not None:
        check(_lib.lib().tgp_roi_cloud_defor(_p(depth), _p(masks), _p(mask_off), _p(mask_stride), _p(det_img), _p(window), _p(camk), D,
                                             H, W, roi_size, _p(recs), _p(counts), _p(tables), _p(mask_val), float(cut_frac), _p(on),
                                             _p(bits), bits.shape[1], _stream(depth)), "tgp_roi_cloud_defor")
    elif tables is None and mask_val is None and cut_frac == 0.25:
        check(_lib.lib().tgp_roi_cloud(_p(depth), _p(masks), _p(mask_off), _p(mask_stride), _p(det_img), _p(window), _p(camk), D, H, W,
                                       roi_size, _p(recs), _p(counts), _stream(depth)), "tgp_roi_cloud")
    else:
        check(_lib.lib().tgp_roi_cloud_ex(_p(depth), _p(masks), _p(mask_off), _p(mask_stride), _p(det_img), _p(window), _p(camk), D, H, W,
                                          roi_size, _p(recs), _p(counts), _p(tables), _p(mask_val), float(cut_frac), _stream(depth)),
              "tgp_roi_cloud_ex")
    return RoiRecords(recs, counts, det_img, window, camk, roi_size, tables)


def cloud_select(rr, sel):
    """out[d, i] = point(recs[d, sel[d, i]]); rr RoiRecords, sel (D,n_pts) int32 -> (D,n_pts,3) float32"""
    _i32(sel, "sel")
    D = rr.recs.shape[0]
    if sel.dim() != 2 or sel.shape[0] != D:
        raise ValueError("cloud_select: sel must be (D,n_pts)")
    out = torch.empty(D, sel.shape[1], 3, device=rr.recs.device, dtype=torch.float32)
    if getattr(rr, "tables", None) is None:
        check(_lib.lib().tgp_cloud_select(_p(rr.recs), _p(sel), _p(rr.det_img), _p(rr.window), _p(rr.camk), D, rr.roi_size, sel.shape[1],
                                          _p(out), _stream(rr.recs)), "tgp_cloud_select")
    else:
        check(_lib.lib().tgp_cloud_select_ex(_p(rr.recs), _p(sel), _p(rr.det_img), _p(rr.window), _p(rr.camk), D, rr.roi_size,
                                             sel.shape[1], _p(out), _p(rr.tables), _stream(rr.recs)), "tgp_cloud_select_ex")
    return out


def cloud_sample(rr, n_pts, seed, counts=None):
    """Device-drawn resampling (tgp_cloud_sample) -> (D,n_pts,3); ``counts`` overrides rr.counts (tests)."""
    counts = rr.counts if counts is None else _i32(counts, "counts")
    D = rr.recs.shape[0]
    if getattr(rr, "tables", None) is not None:
        raise ValueError("cloud_sample: records built from source tables are resampled with cloud_select (tgp_cloud_select_ex)")
    if counts.shape != (D, 3):
        raise ValueError("cloud_sample: counts must be (D,3)")
    out = torch.empty(D, n_pts, 3, device=rr.recs.device, dtype=torch.float32)
    check(_lib.lib().tgp_cloud_sample(_p(rr.recs), _p(counts), _p(rr.det_img), _p(rr.window), _p(rr.camk), D, rr.roi_size, n_pts,
                                      int(seed) & (2 ** 64 - 1), _p(out), _stream(rr.recs)), "tgp_cloud_sample")
    return out


# ------------------------------------------------------------------------------------------- ball crop (depth frame + pose -> cloud)
BALL_LEVELS, BALL_THREADS = _lib.BALL_LEVELS, _lib.BALL_THREADS


class BallRecords:
    """What tgp_ball_cloud leaves in HBM: ``recs`` (J, cap) int32-viewed pixel (or point) indices in row-major order, ``counts``
    (J,4) int32 = valid pixels of the frame, the crop's true count, the ladder level L, status (0 ok, 1 nothing within the last
    radius, 2 no valid pixel, 3 bad frame index), and what a record needs to become a point: ``job_img`` and either ``depth`` +
    ``camk`` or the point lists ``pts`` (I,N,3)."""

    def __init__(self, recs, counts, job_img, depth=None, camk=None, pts=None):
        self.recs, self.counts, self.job_img, self.depth, self.camk, self.pts = recs, counts, job_img, depth, camk, pts

    @property
    def cap(self):
        return self.recs.shape[1]

    def _src(self):
        """(depth, camk, pts, I, H, W) as tgp_ball_select takes them"""
        if self.pts is not None:
            return None, None, self.pts, self.pts.shape[0], 1, self.pts.shape[1]
        return (self.depth, self.camk, None) + tuple(self.depth.shape)


def ball_ladder(radius):
    """The ten radii crop_ball_from_pts (pc_sample_sphere.py:260-265) tests, for radius (J,) float32 -> (J,10) float32, as torch
    ops on the radius' device (no read-back).  The reference keeps a tensor radius >= 0.05 and multiplies it in place by 1.10
    (float32 products); a smaller one becomes the Python float 0.05, whose products are doubles, rounded to float32 when compared."""
    if not (torch.is_tensor(radius) and radius.dtype == torch.float32 and radius.dim() == 1):
        raise TypeError("ball_ladder: radius must be a (J,) float32 tensor")
    rungs, r = [], radius
    for _ in range(BALL_LEVELS):
        rungs.append(r)
        r = r * 1.10
    small, s = [], 0.05
    for _ in range(BALL_LEVELS):
        small.append(s)
        s *= 1.10
    small = torch.tensor(small, dtype=torch.float64).to(torch.float32).to(radius.device)
    return torch.where((radius < 0.05)[:, None], small[None, :], torch.stack(rungs, 1)).contiguous()


def _ball_jobs(job_img, centers, ladder, cap, who):
    _i32(job_img, "job_img"), _f32(centers, "centers"), _f32(ladder, "ladder")
    J = job_img.numel()
    if J < 1 or job_img.dim() != 1 or centers.shape != (J, 3) or ladder.shape != (J, BALL_LEVELS):
        raise ValueError("%s: job_img (J,), centers (J,3) and ladder (J,%d) are needed, J >= 1" % (who, BALL_LEVELS))
    if not (centers.is_contiguous() and ladder.is_contiguous()):
        raise ValueError("%s: centers and ladder must be contiguous" % who)
    if not (isinstance(cap, int) and 1 <= cap <= 2 ** 29):
        raise ValueError("%s: cap must be an int in [1, 2^29]" % who)
    return J


def ball_cloud(depth, job_img, centers, ladder, camk, cap=None, masks=None, mask_off=None, mask_stride=None, mask_val=None,
               full_scan=False):
    """tgp_ball_cloud: job j crops frame job_img[j] of depth (I,H,W) (int16-viewed uint16 millimetres) round centers[j] with the radii
    ladder[j] (ball_ladder).  masks (flat uint8 / bool) with mask_off (J,) int64, mask_stride (J,) int32 and optionally mask_val (J,)
    int32 address a mask per job as roi_cloud does; None: no mask.  cap: records kept per job (default H*W).  full_scan: evaluate
    every pixel instead of the ball's rectangle (same result; for tests).  -> BallRecords"""
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype in (torch.int16, torch.uint16) and depth.dim() == 3
            and depth.is_contiguous()):
        raise TypeError("depth must be a contiguous (I,H,W) 16-bit GPU tensor")
    I, H, W = depth.shape
    cap = H * W if cap is None else cap
    J = _ball_jobs(job_img, centers, ladder, cap, "ball_cloud")
    if _f32(camk, "camk", 2).shape != (I, 4) or not camk.is_contiguous():
        raise ValueError("ball_cloud: camk must be a contiguous (I,4) tensor")
    if masks is not None:
        if not (masks.is_cuda and masks.dtype in (torch.uint8, torch.bool) and masks.is_contiguous()):
            raise TypeError("masks must be a contiguous uint8 / bool GPU tensor")
        if mask_off is None or mask_stride is None:
            raise ValueError("ball_cloud: masks need mask_off and mask_stride")
        if not (mask_off.is_cuda and mask_off.dtype == torch.int64 and mask_off.is_contiguous()):
            raise TypeError("mask_off must be a contiguous int64 GPU tensor")
        if mask_off.numel() != J or _i32(mask_stride, "mask_stride").numel() != J:
            raise ValueError("ball_cloud: mask_off and mask_stride must be (J,)")
        if mask_val is not None and _i32(mask_val, "mask_val").numel() != J:
            raise ValueError("ball_cloud: mask_val must be (J,)")
    elif mask_off is not None or mask_stride is not None or mask_val is not None:
        raise ValueError("ball_cloud: mask_off / mask_stride / mask_val without masks")
    recs = torch.empty(J, cap, device=depth.device, dtype=torch.int32)
    counts = torch.empty(J, 4, device=depth.device, dtype=torch.int32)
    check(_lib.lib().tgp_ball_cloud(_p(depth), _p(masks), _p(mask_off), _p(mask_stride), _p(mask_val), _p(job_img), _p(centers),
                                    _p(ladder), _p(camk), J, I, H, W, cap, int(bool(full_scan)), _p(recs), _p(counts), _stream(depth)),
          "tgp_ball_cloud")
    return BallRecords(recs, counts, job_img, depth=depth, camk=camk)


def ball_cloud_pts(pts, job_img, centers, ladder, cap=None):
    """tgp_ball_cloud_pts: the crop of point lists pts (I,N,3) float32 (crop_ball_from_pts); records are point indices -> BallRecords"""
    if _f32(pts, "pts", 3).shape[2] != 3 or not pts.is_contiguous() or pts.shape[1] < 1:
        raise ValueError("ball_cloud_pts: pts must be a contiguous (I,N,3) tensor, N >= 1")
    I, N = pts.shape[:2]
    cap = N if cap is None else cap
    J = _ball_jobs(job_img, centers, ladder, cap, "ball_cloud_pts")
    recs = torch.empty(J, cap, device=pts.device, dtype=torch.int32)
    counts = torch.empty(J, 4, device=pts.device, dtype=torch.int32)
    check(_lib.lib().tgp_ball_cloud_pts(_p(pts), _p(job_img), _p(centers), _p(ladder), J, I, N, cap, _p(recs), _p(counts), _stream(pts)),
          "tgp_ball_cloud_pts")
    return BallRecords(recs, counts, job_img, pts=pts)


def ball_select(br, sel):
    """tgp_ball_select: sel (J,n_pts) int32 indexes the crop's doubled list (length count * 2^m >= n_pts, element e = entry
    e mod count) -> (points (J,n_pts,3) float32, pix (J,n_pts) int32); an index outside the list gives NaNs and -1"""
    _i32(sel, "sel")
    J = br.recs.shape[0]
    if sel.dim() != 2 or sel.shape[0] != J or sel.shape[1] < 1:
        raise ValueError("ball_select: sel must be (J,n_pts)")
    n_pts = sel.shape[1]
    depth, camk, pts, I, H, W = br._src()
    out = torch.empty(J, n_pts, 3, device=br.recs.device, dtype=torch.float32)
    pix = torch.empty(J, n_pts, device=br.recs.device, dtype=torch.int32)
    check(_lib.lib().tgp_ball_select(_p(br.recs), _p(br.counts), _p(sel), _p(br.job_img), _p(depth), _p(camk), _p(pts), J, I, H, W,
                                     br.cap, n_pts, _p(out), _p(pix), _stream(br.recs)), "tgp_ball_select")
    return out, pix


def ball_sample(br, n_pts, seed, counts=None):
    """tgp_ball_sample: the first n_pts of the keyed permutation of each crop's doubled list, drawn on the device -> (points
    (J,n_pts,3), pix (J,n_pts)); rows of jobs whose status is not 0 are NaN / -1.  ``counts`` overrides br.counts (tests)."""
    counts = br.counts if counts is None else _i32(counts, "counts")
    J = br.recs.shape[0]
    if counts.shape != (J, 4):
        raise ValueError("ball_sample: counts must be (J,4)")
    if not (isinstance(n_pts, int) and 1 <= n_pts <= 2 ** 29):
        raise ValueError("ball_sample: n_pts must be an int in [1, 2^29]")
    depth, camk, pts, I, H, W = br._src()
    out = torch.empty(J, n_pts, 3, device=br.recs.device, dtype=torch.float32)
    pix = torch.empty(J, n_pts, device=br.recs.device, dtype=torch.int32)
    check(_lib.lib().tgp_ball_sample(_p(br.recs), _p(counts), _p(br.job_img), _p(depth), _p(camk),
                                     _p(pts), J, I, H, W, br.cap, n_pts, int(seed) & (2 ** 64 - 1), _p(out), _p(pix),
                                     _stream(br.recs)), "tgp_ball_sample")
    return out, pix


# ------------------------------------------------------------------------------------------------------------ ICP pose refinement
ICP_MAX_POINTS = _lib.ICP_MAX_POINTS
ICP_MODES = {"point": 0, "plane": 1}
ICP_STATUS = {1: "too few inliers", 2: "singular system", 3: "job_model or a count out of range"}


def icp_max_points():
    """most model points per model / source points per job that icp_refine takes"""
    return int(_lib.lib().tgp_icp_max_points())


class IcpModels(object):
    """The padded model set icp_refine registers against: ``points_normals`` (M, m_cap, 6) float32 on the GPU, rows [point, unit
    normal] in model units (what mesh_sample(..., normals=True) writes), and ``counts`` (M) int32 live rows per model (None: m_cap)."""

    def __init__(self, points_normals, counts=None):
        _f32(points_normals, "points_normals", 3)
        if points_normals.shape[2] != 6 or not points_normals.is_contiguous() or points_normals.shape[0] < 1:
            raise ValueError("IcpModels: points_normals must be a contiguous (M, m_cap, 6) tensor")
        if not 1 <= points_normals.shape[1] <= ICP_MAX_POINTS:
            raise ValueError("IcpModels: m_cap must be in [1, %d]" % ICP_MAX_POINTS)
        if counts is not None:
            counts = torch.as_tensor(counts, dtype=torch.int32).to(points_normals.device).contiguous()
            if counts.shape != (points_normals.shape[0],):
                raise ValueError("IcpModels: counts must be (M,)")
        self.points_normals, self.counts = points_normals, counts

    def __len__(self):
        return self.points_normals.shape[0]

    @property
    def m_cap(self):
        return self.points_normals.shape[1]

    @classmethod
    def from_meshset(cls, meshset, meshes, n, seed=0):
        """n surface samples with normals of each of ``meshes`` (mesh indices of the set), drawn on the device: model k's draws are
        keyed k under ``seed`` (mesh_sample)"""
        meshes = [int(m) for m in meshes]
        out = mesh_sample(meshset, meshes, n, keys=list(range(len(meshes))), seed=seed, normals=True, check_status=True)
        return cls(out["points"])

    @classmethod
    def from_vertices(cls, meshset, meshes, n):
        """each of ``meshes`` (mesh indices of the set) thinned to n of its own vertices by ops.farthest_points, with their vertex
        normals (``meshset.vert_normals``: ops.tsdf_meshset(..., indexed=True, normals=True), or ops.mesh_vertex_normals): the model
        points of a welded or decimated scan.  A mesh of more vertices than farthest_points takes is first thinned to that many at
        an even stride.  Nothing is read back.  Raises if the set has no vert_normals or a mesh has fewer than n vertices."""
        if not isinstance(meshset, MeshSet):
            raise TypeError("IcpModels.from_vertices: meshset must be an ops.MeshSet")
        if getattr(meshset, "vert_normals", None) is None:
            raise ValueError("IcpModels.from_vertices: the mesh set has no vert_normals (ops.mesh_vertex_normals makes them)")
        meshes, n = [int(m) for m in meshes], int(n)
        if not meshes or not 1 <= n <= ICP_MAX_POINTS:
            raise ValueError("IcpModels.from_vertices: at least one mesh and n in [1, %d]" % ICP_MAX_POINTS)
        rows, first, cap = [], [0], fps_max_points()
        for nv in meshset.n_verts:
            first.append(first[-1] + nv)
        for m in meshes:
            if not 0 <= m < len(meshset):
                raise ValueError("IcpModels.from_vertices: mesh %d is outside the set of %d meshes" % (m, len(meshset)))
            nv = meshset.n_verts[m]
            if nv < n:
                raise ValueError("IcpModels.from_vertices: mesh %d has %d vertices, fewer than n = %d" % (m, nv, n))
            pn = torch.cat([meshset.verts[first[m]:first[m + 1]], meshset.vert_normals[first[m]:first[m + 1]]], 1)
            if nv > cap:
                pn = pn[(torch.arange(cap, device=pn.device, dtype=torch.int64) * nv) // cap]
            idx = farthest_points(pn[None, :, :3].contiguous(), n)
            rows.append(pn[idx[0].long()])
        return cls(torch.stack(rows).contiguous())

    @classmethod
    def from_raycast(cls, rc):
        """one model per job of a tsdf_raycast result: the job's hits [vertex, normal] packed to the front in ray order (a stable sort
        of the miss mask and a gather, on the device), counts = rc['count']; rows past the count are the misses' zeros.  Nothing is
        read back.  h w must not exceed ICP_MAX_POINTS."""
        z = rc["z"]
        J, n = z.shape[0], z.shape[1] * z.shape[2]
        if not 1 <= n <= ICP_MAX_POINTS:
            raise ValueError("IcpModels.from_raycast: h w = %d rays a job, at most %d make a model" % (n, ICP_MAX_POINTS))
        if J < 1:
            raise ValueError("IcpModels.from_raycast: no job")
        miss = (z.reshape(J, n) <= 0).to(torch.uint8)
        order = torch.sort(miss, dim=1, stable=True).indices
        rows = torch.cat([rc["vertex"].reshape(J, n, 3), rc["normal"].reshape(J, n, 3)], 2)
        return cls(torch.gather(rows, 1, order[:, :, None].expand(J, n, 6)).contiguous(), rc["count"])


def icp_check_status(info, what="icp_refine"):
    """one read of the (J,4) info words; raises TgpError naming the first failed job"""
    st = info[:, 0].cpu().tolist()
    bad = [(j, s) for j, s in enumerate(st) if s != 0]
    if bad:
        raise _lib.TgpError("%s: job %d failed: %s (%d of %d jobs failed)" % (what, bad[0][0], ICP_STATUS.get(bad[0][1], bad[0][1]),
                                                                             len(bad), len(st)))


def icp_refine(models, job_model, src, R, t, s, max_dist, *, src_count=None, mode="plane", with_scale=False, iters=30, tol_rot=1e-5,
               tol_trans=1e-6, min_inliers=6, return_corr=False):
    """tgp_icp_refine (csrc/icp.hip; DESIGN.md section 3 "ICP refinement and model-based tracking"): J poses made to fit J clouds in
    one launch, every iteration on the device.  models: IcpModels; job_model (J) int32; src (J, n_cap, 3) float32 camera-frame
    metres (NaN rows are never inliers), src_count (J) int32 or None; R (J,3,3), t (J,3), s (J): the start x = s R y + t from model
    to camera; max_dist (J) float32 (or one number): the gate in metres.  mode 'plane' (point-to-plane Gauss-Newton) or 'point'
    (closed form; with_scale: the scale moves too); iters the cap; tol_rot / tol_trans: stop when an update is within both (both 0:
    exactly iters iterations).  -> (R, t, s, info (J,4) int32 = status, final inliers, iterations, 0; rmse (J)[, corr (J, n_cap)
    int32 with return_corr]).  Nothing is read back (icp_check_status does)."""
    if mode not in ICP_MODES:
        raise ValueError("icp_refine: mode must be 'plane' or 'point'")
    if with_scale and mode != "point":
        raise ValueError("icp_refine: with_scale needs mode='point'")
    if not (isinstance(iters, int) and iters >= 1):
        raise ValueError("icp_refine: iters must be an int >= 1")
    if not (tol_rot >= 0 and tol_trans >= 0 and isinstance(min_inliers, int) and min_inliers >= 0):
        raise ValueError("icp_refine: tol_rot, tol_trans and min_inliers must not be negative")
    _f32(src, "src", 3), _i32(job_model, "job_model"), _f32(R, "R", 3), _f32(t, "t", 2), _f32(s, "s", 1)
    if not isinstance(models, IcpModels):
        raise TypeError("icp_refine: models must be an ops.IcpModels")
    J, n_cap = src.shape[0], src.shape[1]
    dev = src.device
    if J < 1 or not 1 <= n_cap <= ICP_MAX_POINTS or src.shape[2] != 3:
        raise ValueError("icp_refine: src must be (J, n_cap, 3) with J >= 1 and 1 <= n_cap <= %d" % ICP_MAX_POINTS)
    if J > 65535:
        raise ValueError("icp_refine: at most 65535 jobs a call")
    if job_model.shape != (J,) or R.shape != (J, 3, 3) or t.shape != (J, 3) or s.shape != (J,):
        raise ValueError("icp_refine: job_model (J,), R (J,3,3), t (J,3) and s (J,) are needed for the %d jobs" % J)
    if not torch.is_tensor(max_dist):
        max_dist = torch.full((J,), float(max_dist), device=dev, dtype=torch.float32)
    if _f32(max_dist, "max_dist", 1).shape != (J,):
        raise ValueError("icp_refine: max_dist must be (J,)")
    if src_count is not None and _i32(src_count, "src_count").shape != (J,):
        raise ValueError("icp_refine: src_count must be (J,)")
    tensors = [src, job_model, R, t, s, max_dist, models.points_normals] + [x for x in (src_count, models.counts) if x is not None]
    if not all(x.is_contiguous() for x in tensors):
        raise ValueError("icp_refine: every tensor must be contiguous")
    if any(x.device != dev for x in tensors):
        raise ValueError("icp_refine: every tensor must be on one device")
    R_out, t_out, s_out = torch.empty_like(R), torch.empty_like(t), torch.empty_like(s)
    info = torch.empty(J, 4, device=dev, dtype=torch.int32)
    rmse = torch.empty(J, device=dev, dtype=torch.float32)
    corr = torch.empty(J, n_cap, device=dev, dtype=torch.int32) if return_corr else None
    a = _lib.IcpArgs(models=_p(models.points_normals), model_count=_p(models.counts), M=len(models), m_cap=models.m_cap, src=_p(src),
                     src_count=_p(src_count), job_model=_p(job_model), J=J, n_cap=n_cap, R=_p(R), t=_p(t), s=_p(s), max_dist=_p(max_dist),
                     mode=ICP_MODES[mode], with_scale=int(bool(with_scale)), iters=iters, tol_rot=float(tol_rot), tol_trans=float(tol_trans),
                     min_inliers=min_inliers, R_out=_p(R_out), t_out=_p(t_out), s_out=_p(s_out), info=_p(info), rmse=_p(rmse), corr=_p(corr))
    check(_lib.lib().tgp_icp_refine(ctypes.byref(a), _stream(src)), "tgp_icp_refine")
    out = (R_out, t_out, s_out, info, rmse)
    return out + (corr,) if return_corr else out


# ------------------------------------------------------------------------------------------------------------ distance-field pose search
SEARCH_MAX_POINTS, SEARCH_MAX_ROTATIONS, SEARCH_MAX_TOP, SEARCH_MAX_K = (_lib.SEARCH_MAX_POINTS, _lib.SEARCH_MAX_ROTATIONS,
                                                                          _lib.SEARCH_MAX_TOP, _lib.SEARCH_MAX_K)
SEARCH_MAX_REACH = _lib.SEARCH_MAX_REACH
SEARCH_GRIDS = (16, 32, 48)
SEARCH_REFUSED = 2 ** 31 - 1        # the cost of a row beyond R, and of every row of a refused job


def field_meta(points, G, cap):
    """The host's part of one model's distance field, from its (m,3) float32 points: (meta (4,) float32 = the cube's centre and the
    voxel edge, thresholds (cap,) float32).  centre = the midpoint of the bounding box, half edge = 0.575 x the largest extent,
    voxel = 2 half / G, T_l = (l voxel / 4)^2 for l = 1..cap: float64 on the float32 inputs, each rounded to float32 once."""
    import numpy as np
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    ctr = ((lo + hi) * 0.5).astype(np.float32)
    half = np.float32(0.575 * (hi - lo).max())
    voxel = np.float32(2.0 * float(half) / G)
    edge = np.arange(1, cap + 1, dtype=np.float64) * float(voxel) / 4.0
    return np.concatenate([ctr, [voxel]]).astype(np.float32), (edge * edge).astype(np.float32)


class DistanceFields(object):
    """The quantised distance fields pose_search looks poses up in (tgp_field_build, csrc/search.hip; DESIGN.md section 3
    "Model-based acquisition"): one cube of G^3 voxels per model of an ops.IcpModels, byte (ix G + iy) G + iz = how many of the
    thresholds (l voxel / 4)^2, l = 1..cap, the squared distance from the voxel's centre to the nearest model point reaches
    (tgp_nn1's float32 arithmetic).  ``field`` (M,G,G,G) uint8, ``meta`` (M,4) float32 = centre, voxel edge (model units), both on
    the models' device; ``meta_host`` is the same on the host.  The model's points are read back once, here, for the cube."""

    def __init__(self, models, G=32, cap=32):
        import numpy as np
        if not isinstance(models, IcpModels):
            raise TypeError("DistanceFields: models must be an ops.IcpModels")
        if G not in SEARCH_GRIDS:
            raise ValueError("DistanceFields: G must be one of %s" % (SEARCH_GRIDS,))
        if not (isinstance(cap, int) and 1 <= cap <= 255):
            raise ValueError("DistanceFields: cap must be an int in [1, 255]")
        pn = models.points_normals
        M, dev = len(models), pn.device
        counts = [models.m_cap] * M if models.counts is None else models.counts.cpu().tolist()
        if not all(1 <= c <= models.m_cap for c in counts):
            raise ValueError("DistanceFields: every model needs between 1 and m_cap points")
        pts = pn[:, :, :3].cpu().numpy()
        if not all(np.isfinite(pts[m, :c]).all() for m, c in enumerate(counts)):
            raise ValueError("DistanceFields: a model point is not finite")
        made = [field_meta(pts[m, :c], G, cap) for m, c in enumerate(counts)]
        self.meta_host = np.stack([m for m, _ in made])
        self.meta = torch.from_numpy(self.meta_host).to(dev)
        self.thresholds = torch.from_numpy(np.stack([t for _, t in made])).to(dev)
        self.G, self.cap, self.models = G, cap, models
        self.field = torch.empty(M, G, G, G, device=dev, dtype=torch.uint8)
        a = _lib.FieldArgs(models=_p(pn), model_count=_p(models.counts), M=M, m_cap=models.m_cap, meta=_p(self.meta),
                           thresholds=_p(self.thresholds), G=G, cap=cap, field=_p(self.field))
        check(_lib.lib().tgp_field_build(ctypes.byref(a), _stream(pn)), "tgp_field_build")

    def __len__(self):
        return self.field.shape[0]


def search_shifts(K, stride):
    """the (D,3) int64 lattice shifts of pose_search in voxels, in shift-index order, on the host"""
    r = torch.arange(-K, K + 1, dtype=torch.int64) * stride
    return torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def pose_search(fields, job_model, clouds, counts, anchors, scales, rotations, K=5, stride=2, top=16, return_table=False):
    """tgp_pose_search (csrc/search.hip; DESIGN.md section 3 "Model-based acquisition"): for each of J clouds, every one of R rotations
    x (2K+1)^3 lattice translations is scored against the distance field of the job's model, and the ``top`` rotations of least cost
    come back, each with its best translation.  fields: ops.DistanceFields; job_model (J) int32; clouds (J, n_cap <= 1024, 3)
    float32 camera-frame metres (non-finite rows and rows at or beyond counts[j] contribute nothing); counts (J) int32 or None;
    anchors (J,3) float32: the point of each cloud tried at the cube's centre; scales (J) float32 metres per model unit; rotations
    (R,3,3) float32.  The shifts are stride x {-K..K}^3 voxels (search_shifts).
    -> dict: cost, rot, shift (J, top) int32 and poses (J, top, 3, 4) float32 [R | t] (model units to metres takes the scale:
    x = s R y + t); rows beyond R, and a job whose model index or count is out of range, give cost = SEARCH_REFUSED, rot = shift = -1
    and a NaN pose.  return_table adds table (J, R, 2) int32 = each rotation's least cost and its shift.  Nothing synchronises."""
    if not isinstance(fields, DistanceFields):
        raise TypeError("pose_search: fields must be an ops.DistanceFields")
    _f32(clouds, "clouds", 3), _i32(job_model, "job_model"), _f32(anchors, "anchors", 2), _f32(scales, "scales", 1), _f32(rotations, "rotations", 3)
    J, n_cap = clouds.shape[0], clouds.shape[1]
    if J < 1 or not 1 <= n_cap <= SEARCH_MAX_POINTS or clouds.shape[2] != 3:
        raise ValueError("pose_search: clouds must be (J, n_cap, 3) with J >= 1 and 1 <= n_cap <= %d" % SEARCH_MAX_POINTS)
    if J > 65535:
        raise ValueError("pose_search: at most 65535 jobs a call")
    R = rotations.shape[0]
    if rotations.shape[1:] != (3, 3) or not 1 <= R <= SEARCH_MAX_ROTATIONS:
        raise ValueError("pose_search: rotations must be (R,3,3) with 1 <= R <= %d" % SEARCH_MAX_ROTATIONS)
    if job_model.shape != (J,) or anchors.shape != (J, 3) or scales.shape != (J,):
        raise ValueError("pose_search: job_model (J,), anchors (J,3) and scales (J,) are needed for the %d jobs" % J)
    if counts is not None and _i32(counts, "counts").shape != (J,):
        raise ValueError("pose_search: counts must be (J,)")
    if not (isinstance(K, int) and 0 <= K <= SEARCH_MAX_K and isinstance(stride, int) and stride >= 1 and K * stride <= SEARCH_MAX_REACH):
        raise ValueError("pose_search: K must be an int in [0, %d], stride an int >= 1 and K * stride <= %d" % (SEARCH_MAX_K, SEARCH_MAX_REACH))
    if not (isinstance(top, int) and 1 <= top <= SEARCH_MAX_TOP):
        raise ValueError("pose_search: top must be an int in [1, %d]" % SEARCH_MAX_TOP)
    dev = clouds.device
    tensors = [clouds, job_model, anchors, scales, rotations, fields.field] + ([] if counts is None else [counts])
    if not all(x.is_contiguous() for x in tensors):
        raise ValueError("pose_search: every tensor must be contiguous")
    if any(x.device != dev for x in tensors):
        raise ValueError("pose_search: every tensor must be on one device")
    out = {"cost": torch.empty(J, top, device=dev, dtype=torch.int32), "rot": torch.empty(J, top, device=dev, dtype=torch.int32),
           "shift": torch.empty(J, top, device=dev, dtype=torch.int32), "poses": torch.empty(J, top, 3, 4, device=dev, dtype=torch.float32)}
    table = _workspace(dev, _lib.lib().tgp_pose_search_workspace_bytes(J, R), "tgp_pose_search_workspace_bytes", torch.int32).view(J, R, 2)
    a = _lib.PoseSearchArgs(field=_p(fields.field), meta=_p(fields.meta), M=len(fields), G=fields.G, cap=fields.cap, job_model=_p(job_model),
                            clouds=_p(clouds), counts=_p(counts), anchors=_p(anchors), scales=_p(scales), J=J, n_cap=n_cap,
                            rotations=_p(rotations), R=R, K=K, stride=stride, top=top, cost=_p(out["cost"]), rot=_p(out["rot"]),
                            shift=_p(out["shift"]), poses=_p(out["poses"]), workspace=_p(table), workspace_bytes=table.numel() * 4)
    check(_lib.lib().tgp_pose_search(ctypes.byref(a), _stream(clouds)), "tgp_pose_search")
    if return_table:
        out["table"] = table
    return out


# ------------------------------------------------------------------------------------------------------------ models from depth sequences
TSDF_MIN_G, TSDF_MAX_G, TSDF_MAX_JOBS, TSDF_MAX_FACES = _lib.TSDF_MIN_G, _lib.TSDF_MAX_G, _lib.TSDF_MAX_JOBS, _lib.TSDF_MAX_FACES


def tsdf_meta(center, extent, G):
    """One volume's cube from its object's centre (3,) and extents (3,), in model units: (4,) float32 = the centre and the voxel
    edge.  field_meta's rule: half edge = 0.575 x the largest extent, voxel = 2 half / G, float64 on the float32 inputs, each
    rounded to float32 once -- a scanned model's distance field and its volume share a cube rule."""
    import numpy as np
    ctr = np.asarray(center, dtype=np.float32).reshape(3)
    half = np.float32(0.575 * float(np.asarray(extent, dtype=np.float32).reshape(3).astype(np.float64).max()))
    return np.concatenate([ctr, [np.float32(2.0 * float(half) / G)]]).astype(np.float32)


class TsdfVolumes(object):
    """M truncated-signed-distance volumes, one cube of G^3 voxels per object in the object's model units (csrc/tsdf.hip; DESIGN.md
    section 3 "Models from depth sequences").  ``sum`` and ``weight`` (M,G,G,G) int32 on ``device``: the voxel's summed quantised
    distances (1024 = the truncation) and how many frames it was seen in, voxel (ix, iy, iz) at (ix G + iy) G + iz; ``meta`` (M,4)
    float32 = the cube's centre and the voxel edge, as DistanceFields.meta; ``meta_host`` the same on the host.  A voxel's centre
    along an axis is c + (((float)i + 0.5f) - G/2) * voxel in float32.  centers, extents: (M,3) model units (tsdf_meta's rule)."""

    def __init__(self, centers, extents, G=64, device="cuda"):
        import numpy as np
        if not (isinstance(G, int) and TSDF_MIN_G <= G <= TSDF_MAX_G and G % 8 == 0):
            raise ValueError("TsdfVolumes: G must be a multiple of 8 in [%d, %d]" % (TSDF_MIN_G, TSDF_MAX_G))
        centers, extents = np.asarray(centers, dtype=np.float32), np.asarray(extents, dtype=np.float32)
        if centers.ndim != 2 or centers.shape[1] != 3 or centers.shape[0] < 1 or extents.shape != centers.shape:
            raise ValueError("TsdfVolumes: centers and extents must be (M,3) with M >= 1")
        if not (np.isfinite(centers).all() and np.isfinite(extents).all() and (extents.max(1) > 0).all()):
            raise ValueError("TsdfVolumes: centers and extents must be finite and every object's largest extent positive")
        self._alloc(np.stack([tsdf_meta(c, e, G) for c, e in zip(centers, extents)]), G, device)

    def _alloc(self, meta, G, device):
        import numpy as np
        self.G = G
        self.meta_host = np.ascontiguousarray(meta, dtype=np.float32)
        self.meta = torch.from_numpy(self.meta_host).to(device)
        M = len(self.meta_host)
        self.sum = torch.zeros(M, G, G, G, device=device, dtype=torch.int32)
        self.weight = torch.zeros(M, G, G, G, device=device, dtype=torch.int32)

    @classmethod
    def from_meta(cls, meta, G, device="cuda"):
        """volumes on given cubes: meta (M,4) float32 = each cube's centre and its voxel edge (finite, the edge positive), for
        instance an ops.DistanceFields' meta_host, so that a field and a volume cover the same cube"""
        import numpy as np
        meta = np.asarray(meta, dtype=np.float32)
        if not (isinstance(G, int) and TSDF_MIN_G <= G <= TSDF_MAX_G and G % 8 == 0):
            raise ValueError("TsdfVolumes: G must be a multiple of 8 in [%d, %d]" % (TSDF_MIN_G, TSDF_MAX_G))
        if meta.ndim != 2 or meta.shape[1] != 4 or meta.shape[0] < 1 or not np.isfinite(meta).all() or not (meta[:, 3] > 0).all():
            raise ValueError("TsdfVolumes.from_meta: meta must be (M,4) finite rows with a positive voxel edge")
        self = cls.__new__(cls)
        self._alloc(meta, G, device)
        return self

    @classmethod
    def from_meshset(cls, meshset, G=64, pad=1.0):
        """volumes around the meshes of an ops.MeshSet: each mesh's bounding box, its extents times ``pad``"""
        import numpy as np
        if not isinstance(meshset, MeshSet):
            raise TypeError("TsdfVolumes.from_meshset: meshset must be an ops.MeshSet")
        v, vptr = meshset.verts.cpu().numpy(), meshset.vptr.cpu().numpy()
        lo = np.stack([v[vptr[m]:vptr[m + 1]].min(0) for m in range(len(meshset))]).astype(np.float64)
        hi = np.stack([v[vptr[m]:vptr[m + 1]].max(0) for m in range(len(meshset))]).astype(np.float64)
        return cls(((lo + hi) * 0.5).astype(np.float32), ((hi - lo) * float(pad)).astype(np.float32), G, meshset.device)

    def __len__(self):
        return self.sum.shape[0]

    def zero_(self):
        self.sum.zero_(), self.weight.zero_()
        return self


def tsdf_integrate(volumes, depth, camk, job_img, job_model, job_pose, trunc_mm, near=0.01, mask=None, job_mask_val=None):
    """Fuse J posed depth frames into truncated-signed-distance volumes in one call (tgp_tsdf_integrate, csrc/tsdf.hip; DESIGN.md
    section 3 "Models from depth sequences").  Job j projects every voxel centre of volume job_model[j] at job_pose[j] into frame
    job_img[j]; a voxel in front of near whose pixel (rounded, ties to even) lies in the frame, holds a depth, carries the job's
    mask byte when a mask is given, and is not more than trunc_mm behind the surface adds q = rint(1024 min(sdf, trunc) / trunc) to
    its sum and 1 to its weight, sdf = depth - 1000 z in millimetres.  All tensors on the volumes' GPU, as pose_verify takes them:
    depth (S,H,W) 16-bit millimetres, camk (S,4) float32, job_img and job_model (J) int32, job_pose (J,3,4) float32 [s R | t] (model
    -> camera, metres), mask (S,H,W) uint8 with job_mask_val (J) uint8, or neither.  The volumes are added to in place; integer
    sums, so neither the order of the jobs nor their split over calls matters.  -> status (J) int32: 1 for a job whose frame or
    volume index is out of range (it adds nothing), else 0.  Nothing is read back."""
    if not isinstance(volumes, TsdfVolumes):
        raise TypeError("tsdf_integrate: volumes must be an ops.TsdfVolumes")
    dev = volumes.sum.device
    S, H, W, J = _frame_jobs("tsdf_integrate", dev, depth, camk, job_img, [(job_model, "job_model", torch.int32, ()),
                                                                            (job_pose, "job_pose", torch.float32, (3, 4))],
                             mask, job_mask_val, where="the volumes' device")
    import numpy as np
    trunc = np.float32(trunc_mm)
    if not (np.isfinite(trunc) and trunc > 0):
        raise ValueError("tsdf_integrate: trunc_mm must be positive (millimetres)")
    inv = np.float32(1024.0 / float(trunc))
    if not (np.isfinite(inv) and inv > 0):
        raise ValueError("tsdf_integrate: trunc_mm is out of range")
    if not float(near) > 0.0:
        raise ValueError("tsdf_integrate: near must be positive")
    if J > TSDF_MAX_JOBS or H > 16384 or W > 16384:
        raise ValueError("tsdf_integrate: at most %d jobs and frames of at most 16384 pixels a side" % TSDF_MAX_JOBS)
    status = torch.empty(J, device=dev, dtype=torch.int32)
    if J == 0:
        return status
    a = _lib.TsdfIntegrateArgs(depth=_p(depth), camk=_p(camk), S=S, H=H, W=W, sum=_p(volumes.sum), weight=_p(volumes.weight),
                               meta=_p(volumes.meta), M=len(volumes), G=volumes.G, job_img=_p(job_img), job_model=_p(job_model),
                               job_pose=_p(job_pose), mask=_p(mask), job_mask_val=_p(job_mask_val), J=J, trunc=float(trunc), inv=float(inv),
                               near=float(near), status=_p(status))
    check(_lib.lib().tgp_tsdf_integrate(ctypes.byref(a), _stream(job_pose)), "tgp_tsdf_integrate")
    return status


def _tsdf_mesh_args(volumes, model, min_weight, who):
    if not isinstance(volumes, TsdfVolumes):
        raise TypeError("%s: volumes must be an ops.TsdfVolumes" % who)
    if not (isinstance(model, int) and 0 <= model < len(volumes)):
        raise ValueError("%s: model must index the %d volumes" % (who, len(volumes)))
    if not (isinstance(min_weight, int) and min_weight >= 1):
        raise ValueError("%s: min_weight must be an int >= 1" % who)
    G, dev = volumes.G, volumes.sum.device
    counts = torch.empty(G * G * G, device=dev, dtype=torch.int32)
    a = _lib.TsdfMeshArgs(sum=_p(volumes.sum), weight=_p(volumes.weight), meta=_p(volumes.meta), M=len(volumes), G=G, model=model,
                          min_weight=min_weight, counts=_p(counts))
    check(_lib.lib().tgp_tsdf_mesh_count(ctypes.byref(a), _stream(volumes.sum)), "tgp_tsdf_mesh_count")
    return a, counts, torch.cumsum(counts, 0, dtype=torch.int64)


def tsdf_mesh(volumes, model, min_weight=1, face_cap=None):
    """The surface of one volume as a triangle soup by marching tetrahedra (tgp_tsdf_mesh_count / _emit, csrc/tsdf.hip; DESIGN.md
    section 3 "Models from depth sequences").  A cube of eight voxel centres takes part iff all eight have weight >= min_weight; a
    corner is inside iff its sum is negative; the cube is cut into the six Kuhn tetrahedra and every cut edge's vertex is
    interpolated from the end with the smaller flat index, so shared edges share bits.  Triangles are ordered by cube flat index,
    tetrahedron, triangle, and wind so that their normals point outward (from inside to outside corners).
    face_cap None: the triangle count is read back once and ``verts`` is exactly (3 F,3).  face_cap an int: nothing is read back,
    ``verts`` is (3 face_cap,3), its rows beyond 3 n_faces zero, and triangles beyond the cap are dropped in that order.
    -> dict: verts float32 (model units), faces (rows/3, 3) int32 = arange, n_faces () int64 = min(total, face_cap), status () int64
    = 1 iff triangles were dropped, counts (G^3) int32 = each cube's triangles; all on the volumes' device."""
    a, counts, offsets = _tsdf_mesh_args(volumes, model, min_weight, "tsdf_mesh")
    dev = counts.device
    if face_cap is None:
        cap = int(offsets[-1].item())                        # the read-back
    elif isinstance(face_cap, int) and 0 <= face_cap <= TSDF_MAX_FACES:
        cap = face_cap
    else:
        raise ValueError("tsdf_mesh: face_cap must be None or an int in [0, %d]" % TSDF_MAX_FACES)
    if cap > TSDF_MAX_FACES:
        raise ValueError("tsdf_mesh: the volume has %d triangles, above the cap of %d; pass a face_cap" % (cap, TSDF_MAX_FACES))
    verts = torch.zeros(3 * cap, 3, device=dev, dtype=torch.float32)
    info = torch.zeros(2, device=dev, dtype=torch.int64)
    a.offsets, a.verts, a.face_cap, a.info = _p(offsets), _p(verts) if cap else None, cap, _p(info)
    check(_lib.lib().tgp_tsdf_mesh_emit(ctypes.byref(a), _stream(volumes.sum)), "tgp_tsdf_mesh_emit")
    return {"verts": verts, "faces": torch.arange(3 * cap, device=dev, dtype=torch.int32).reshape(cap, 3), "n_faces": info[0],
            "status": info[1], "counts": counts}


# ------------------------------------------------------------------------------------------------------------ indexed meshes from volumes
WELD_MAX_VERTS = _lib.WELD_MAX_VERTS
WELD_CLUSTERS = (1, 2, 4, 8)


def volume_normal_scale(voxel):
    """mesh_vertex_normals' quantisation for a volume's mesh: 2^30 / voxel^2 in float64 on the float32 voxel edge (a face's cross
    product is at most a few voxel^2)"""
    v = float(voxel)
    return 2.0 ** 30 / (v * v)


def tsdf_mesh_indexed(volumes, model, min_weight=1, face_cap=None, vert_cap=None, cluster=1):
    """The surface of one volume as an INDEXED mesh (tgp_tsdf_weld_*, csrc/weld.hip; DESIGN.md section 3 "Indexed meshes from
    volumes"): tsdf_mesh's triangles in tsdf_mesh's order, with every vertex once.  A vertex is named by the voxel edge it cuts --
    key = flat(A) 8 + d, A the edge's smaller end, d = dx << 2 | dy << 1 | dz the step to the other -- and vertices are numbered in
    ascending key: a bit mask per voxel, a prefix sum and a rank, no float is compared.  verts[faces].reshape(-1, 3) is tsdf_mesh's
    soup byte for byte.  Vertices at a corner whose sum is 0 have equal positions and different names; they stay distinct.
    Both caps None: the two counts are read back once and verts, faces are exactly (V,3), (F,3).  Both caps ints: nothing is read
    back, verts is (vert_cap,3) and faces (face_cap,3), rows beyond the counts zero; a face that names a vertex at or beyond
    vert_cap is dropped (status bit 2), then faces beyond face_cap are dropped in order (status bit 1).
    cluster c in (2, 4, 8) decimates: the vertices whose A lies in one cell of c^3 voxels become their mean (in 2^-16 voxel
    fixed point, integer sums), occupied cells are numbered in ascending flat cell index, faces are renamed, those with two equal
    names dropped, the rest rotated to start at their smallest name (winding kept), exact duplicates removed and the survivors
    sorted by that triple; this path reads the cell count back and torch.unique sizes its result on the host.
    -> dict: verts float32 (model units), faces int32, n_verts, n_faces, status () int64, mask (G^3) uint8 (bit d of mask[A]: vertex
    (A, d) exists), normal_scale (mesh_vertex_normals' quantisation for this mesh); all tensors on the volumes' device."""
    who = "tsdf_mesh_indexed"
    if not isinstance(volumes, TsdfVolumes):
        raise TypeError("%s: volumes must be an ops.TsdfVolumes" % who)
    if not (isinstance(model, int) and 0 <= model < len(volumes)):
        raise ValueError("%s: model must index the %d volumes" % (who, len(volumes)))
    if not (isinstance(min_weight, int) and min_weight >= 1):
        raise ValueError("%s: min_weight must be an int >= 1" % who)
    if cluster not in WELD_CLUSTERS:
        raise ValueError("%s: cluster must be 1, 2, 4 or 8" % who)
    if (face_cap is None) != (vert_cap is None):
        raise ValueError("%s: face_cap and vert_cap come together" % who)
    if face_cap is not None and not (isinstance(face_cap, int) and 0 <= face_cap <= TSDF_MAX_FACES):
        raise ValueError("%s: face_cap must be None or an int in [0, %d]" % (who, TSDF_MAX_FACES))
    if vert_cap is not None and not (isinstance(vert_cap, int) and 0 <= vert_cap <= WELD_MAX_VERTS):
        raise ValueError("%s: vert_cap must be None or an int in [0, %d]" % (who, WELD_MAX_VERTS))
    G, dev, lib, st = volumes.G, volumes.sum.device, _lib.lib(), _stream(volumes.sum)
    cells = G * G * G
    mask = torch.empty(cells, device=dev, dtype=torch.uint8)
    vcounts = torch.empty(cells, device=dev, dtype=torch.int32)
    fcounts = torch.empty(cells, device=dev, dtype=torch.int32)
    a = _lib.TsdfWeldArgs(sum=_p(volumes.sum), weight=_p(volumes.weight), meta=_p(volumes.meta), M=len(volumes), G=G, model=model,
                          min_weight=min_weight, mask=_p(mask), vcounts=_p(vcounts), fcounts=_p(fcounts),
                          vert_cap=WELD_MAX_VERTS if vert_cap is None else vert_cap)
    check(lib.tgp_tsdf_weld_mark(ctypes.byref(a), st), "tgp_tsdf_weld_mark")
    voffsets = torch.cumsum(vcounts, 0, dtype=torch.int64)
    a.voffsets = _p(voffsets)
    check(lib.tgp_tsdf_weld_count(ctypes.byref(a), st), "tgp_tsdf_weld_count")
    foffsets = torch.cumsum(fcounts, 0, dtype=torch.int64)
    if vert_cap is None:
        vcap, fcap = torch.stack([voffsets[-1], foffsets[-1]]).cpu().tolist()       # the read-back
        if fcap > TSDF_MAX_FACES:
            raise ValueError("%s: the volume has %d triangles, above the cap of %d; pass caps" % (who, fcap, TSDF_MAX_FACES))
    else:
        vcap, fcap = vert_cap, face_cap
    verts = torch.zeros(vcap, 3, device=dev, dtype=torch.float32)
    faces = torch.zeros(fcap, 3, device=dev, dtype=torch.int32)
    info = torch.zeros(3, device=dev, dtype=torch.int64)
    a.foffsets, a.vert_cap, a.face_cap, a.info = _p(foffsets), vcap, fcap, _p(info)
    a.verts, a.faces = _p(verts) if vcap else None, _p(faces) if fcap else None
    check(lib.tgp_tsdf_weld_verts(ctypes.byref(a), st), "tgp_tsdf_weld_verts")
    check(lib.tgp_tsdf_weld_faces(ctypes.byref(a), st), "tgp_tsdf_weld_faces")
    out = {"verts": verts, "faces": faces, "n_verts": info[0], "n_faces": info[1], "status": info[2], "mask": mask,
           "normal_scale": volume_normal_scale(volumes.meta_host[model, 3])}
    if cluster == 1:
        return out
    side = -(-G // cluster)
    vcell = torch.zeros(vcap, device=dev, dtype=torch.int32)
    sums = torch.empty(side ** 3, 3, device=dev, dtype=torch.int64)
    counts = torch.empty(side ** 3, device=dev, dtype=torch.int32)
    c = _lib.WeldClusterArgs(mask=_p(mask), voffsets=_p(voffsets), verts=_p(verts) if vcap else None, meta=_p(volumes.meta), M=len(volumes),
                             G=G, model=model, cluster=cluster, vert_cap=vcap, vcell=_p(vcell) if vcap else None, cell_sums=_p(sums),
                             cell_counts=_p(counts))
    check(lib.tgp_weld_cluster(ctypes.byref(c), st), "tgp_weld_cluster")
    occupied = counts > 0
    number = torch.cumsum(occupied, 0, dtype=torch.int64) - 1                       # a cell's name: its rank among the occupied ones
    n_cells = int(number[-1].item()) + 1                                            # the read-back
    order = torch.sort((~occupied).to(torch.uint8), stable=True).indices[:n_cells]  # the occupied cells, ascending
    meta = volumes.meta[model]
    first = meta[:3] + torch.tensor(0.5 - (G // 2), device=dev, dtype=torch.float32) * meta[3]      # voxel 0's centre, float32
    mean = sums[order].double() / counts[order].double()[:, None]
    rep = (first.double() + (mean * meta[3].double()) / 65536.0).float()
    names = number[vcell.long()[faces.long()]]                                     # (fcap,3); rows beyond n_faces name one cell thrice
    keep = (names[:, 0] != names[:, 1]) & (names[:, 1] != names[:, 2]) & (names[:, 2] != names[:, 0])
    turn = (names.argmin(1)[:, None] + torch.arange(3, device=dev)[None]) % 3
    r = torch.gather(names, 1, turn)
    packed = torch.unique(((r[:, 0] << 42) | (r[:, 1] << 21) | r[:, 2])[keep])      # names are below 2^21; sorted = lexicographic
    low = (1 << 21) - 1
    cfaces = torch.stack([packed >> 42, (packed >> 21) & low, packed & low], 1).to(torch.int32)
    out.update(verts=rep, faces=cfaces, n_verts=torch.tensor(n_cells, device=dev), n_faces=torch.tensor(cfaces.shape[0], device=dev))
    return out


def mesh_vertex_normals(mesh, scale=None):
    """Area-weighted unit vertex normals (tgp_mesh_vertex_normals, csrc/weld.hip; DESIGN.md section 3 "Indexed meshes from
    volumes") of an ops.MeshSet -- CAD meshes too -- or of a tsdf_mesh_indexed result.  Per face the float32 cross product (p1 -
    p0) x (p2 - p0), times the mesh's ``scale`` in float64, rounded to an integer and added to its three vertices' int64 sums by
    integer atomics; each sum is normalised in float64 and rounded to float32 once.  Integer sums: two calls give identical bytes.
    A vertex that no face with area uses gets (0, 0, 0).  scale: (M) floats; None: the set's ``normal_scale`` (2^30 / voxel^2 for a
    volume's mesh), else 2^40 / (the mesh's largest extent)^2.  -> (sum V,3) float32 on the mesh's device; nothing is read back."""
    if isinstance(mesh, MeshSet):
        verts, faces, vptr, fptr, M = mesh.verts, mesh.faces, mesh.vptr, mesh.fptr, len(mesh)
        if scale is None:
            scale = mesh.normal_scale
        if scale is None:
            ext = [float(e.max()) for e in mesh.extent]
            scale = [2.0 ** 40 / (e * e) if e > 0 else 1.0 for e in ext]
    elif isinstance(mesh, dict) and all(k in mesh for k in ("verts", "faces", "n_verts", "n_faces")):
        verts, faces, M = mesh["verts"], mesh["faces"], 1
        zero = torch.zeros((), device=verts.device, dtype=torch.int64)
        vptr, fptr = torch.stack([zero, mesh["n_verts"]]).to(torch.int32), torch.stack([zero, mesh["n_faces"]]).to(torch.int32)
        if scale is None:
            scale = [mesh["normal_scale"]]
    else:
        raise TypeError("mesh_vertex_normals: an ops.MeshSet or a tsdf_mesh_indexed result is expected")
    if not verts.is_cuda:
        raise TypeError("mesh_vertex_normals: the mesh must be on a GPU")
    scale = [float(x) for x in scale]
    if len(scale) != M or not all(math.isfinite(x) and x > 0 for x in scale):
        raise ValueError("mesh_vertex_normals: scale must be %d positive finite numbers" % M)
    dev, V, F = verts.device, verts.shape[0], faces.shape[0]
    scale_t = torch.tensor(scale, device=dev, dtype=torch.float64)
    sums = torch.empty(V, 3, device=dev, dtype=torch.int64)
    normals = torch.zeros(V, 3, device=dev, dtype=torch.float32)
    a = _lib.MeshNormalsArgs(verts=_p(verts) if V else None, faces=_p(faces) if F else None, vptr=_p(vptr), fptr=_p(fptr), M=M, V=V, F=F,
                             scale=_p(scale_t), sums=_p(sums) if V else None, normals=_p(normals) if V else None)
    check(_lib.lib().tgp_mesh_vertex_normals(ctypes.byref(a), _stream(verts)), "tgp_mesh_vertex_normals")
    return normals


def tsdf_meshset(volumes, min_weight=1, indexed=False, cluster=1, normals=False):
    """Every volume's surface as one ops.MeshSet on the volumes' device: what IcpModels.from_meshset, pose.Verify, DistanceFields
    (through IcpModels) and evaluation.bop take.  A volume without a face is refused by name.
    indexed False (the default): tsdf_mesh's soups; each volume's triangle count is read back once, and its soup once (MeshSet
    packs on the host).  indexed True: tsdf_mesh_indexed's welded meshes -- the same triangles in the same order over shared
    vertices -- packed on the device (MeshSet.from_device): per volume only the two counts are read back, and M x 5 numbers for the
    set.  cluster (2, 4 or 8, with indexed) decimates by voxel clusters.  normals: the set carries ``vert_normals`` (sum V,3)
    float32 (mesh_vertex_normals), which IcpModels.from_vertices needs."""
    if not isinstance(volumes, TsdfVolumes):
        raise TypeError("tsdf_meshset: volumes must be an ops.TsdfVolumes")
    if cluster not in WELD_CLUSTERS:
        raise ValueError("tsdf_meshset: cluster must be 1, 2, 4 or 8")
    if cluster != 1 and not indexed:
        raise ValueError("tsdf_meshset: cluster needs indexed=True")
    empty = "tsdf_meshset: volume %d has no face (no cube with all eight corners seen %d times and a sign change)"
    if indexed:
        vs, fs = [], []
        for m in range(len(volumes)):
            out = tsdf_mesh_indexed(volumes, m, min_weight, cluster=cluster)
            if out["faces"].shape[0] == 0:
                raise ValueError(empty % (m, min_weight))
            vs.append(out["verts"]), fs.append(out["faces"])
        ms = MeshSet.from_device(torch.cat(vs), torch.cat(fs), [v.shape[0] for v in vs], [f.shape[0] for f in fs])
        ms.normal_scale = [volume_normal_scale(v) for v in volumes.meta_host[:, 3]]
    else:
        meshes = []
        for m in range(len(volumes)):
            out = tsdf_mesh(volumes, m, min_weight)
            if out["verts"].shape[0] == 0:
                raise ValueError(empty % (m, min_weight))
            meshes.append((out["verts"].cpu().numpy(), out["faces"].cpu().numpy()))
        ms = MeshSet(meshes, device=volumes.sum.device)
    if normals:
        ms.vert_normals = mesh_vertex_normals(ms)
    return ms


# ------------------------------------------------------------------------------------------------------------ ray casting of the volumes
RAYCAST_MAX_SIDE = _lib.RAYCAST_MAX_SIDE


def pose_inverse(job_pose):
    """(J,3,4) float32 [s R | t] on the GPU -> (J,3,4) float32: the inverse map (camera -> model), by cofactors in float64 on the
    device in a fixed order of single operations, rounded to float32 once (tests/raycast_ref.py inverse_pose does the same
    operations in NumPy).  Nothing is read back; a NaN stays a NaN."""
    T = job_pose.to(torch.float64)
    a, b, c, d, e, f, g, h, i = (T[:, r, k] for r in range(3) for k in range(3))
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = (a * c00 + b * c10) + c * c20
    A = torch.stack([torch.stack([c00, c01, c02], 1), torch.stack([c10, c11, c12], 1), torch.stack([c20, c21, c22], 1)], 1) / det[:, None, None]
    t = T[:, :, 3]
    back = -((A[:, :, 0] * t[:, None, 0] + A[:, :, 1] * t[:, None, 1]) + A[:, :, 2] * t[:, None, 2])
    return torch.cat([A, back[:, :, None]], 2).to(torch.float32).contiguous()


def _raycast_jobs(volumes, camk, job_img, job_model, job_pose, who):
    if not isinstance(volumes, TsdfVolumes):
        raise TypeError("%s: volumes must be an ops.TsdfVolumes" % who)
    dev = volumes.sum.device
    _gpu_args(who, dev, [(camk, "camk", torch.float32), (job_img, "job_img", torch.int32), (job_model, "job_model", torch.int32),
                         (job_pose, "job_pose", torch.float32)], where="the volumes' device")
    J = job_img.numel()
    if camk.dim() != 2 or camk.shape[1] != 4 or camk.shape[0] < 1 or job_img.dim() != 1 or job_model.shape != (J,) or job_pose.shape != (J, 3, 4):
        raise ValueError("%s: camk (S,4), job_img (J), job_model (J), job_pose (J,3,4) are expected" % who)
    if J > TSDF_MAX_JOBS:
        raise ValueError("%s: at most %d jobs" % (who, TSDF_MAX_JOBS))
    return dev, J


def tsdf_raycast(volumes, camk, job_img, job_model, job_pose, window, h, w, *, min_weight=1, step=1.0, near=0.01, job_inv=None):
    """The surface of TSDF volumes as cameras see it (tgp_tsdf_raycast, csrc/raycast.hip; DESIGN.md section 3 "Ray casting and
    frame-to-model tracking").  Job j casts h x w rays into volume job_model[j] from the camera of job_pose[j] (3,4) [s R | t] (model
    -> camera, metres) with the intrinsics camk[job_img[j]]; ray (r, c) goes through the pixel coordinates (u0 + c du, v0 + r dv) of
    window[j] = (u0, v0, du, dv).  It is marched in steps of ``step`` voxels from where it enters the cube (not before ``near``
    metres); a sample is the trilinear value of sum / weight over its cell, known when all eight voxels have weight >= min_weight;
    the first known sample <= 0 ends the ray, as a hit where the sample before it was known and positive.  All tensors on the
    volumes' GPU: camk (S,4) float32, job_img, job_model (J) int32, job_pose (J,3,4), window (J,4) float32; job_inv (J,3,4) float32:
    the poses' inverses if the caller has them (default pose_inverse(job_pose)).
    -> dict: z (J,h,w) float32 camera depth in metres (0: a miss), depth (J,h,w) int16-viewed uint16 millimetres, vertex, normal
    (J,h,w,3) float32 in the MODEL frame (zeros on a miss), count (J) int32 hits, status (J) int32: 1 for a job whose volume or
    camera index is out of range (all its rays miss).  Nothing is read back."""
    dev, J = _raycast_jobs(volumes, camk, job_img, job_model, job_pose, "tsdf_raycast")
    if not (torch.is_tensor(window) and window.is_cuda and window.dtype == torch.float32 and window.is_contiguous() and window.device == dev
            and window.shape == (J, 4)):
        raise ValueError("tsdf_raycast: window must be a contiguous (J,4) float32 tensor on the volumes' device")
    if job_inv is None:
        job_inv = pose_inverse(job_pose)
    elif not (torch.is_tensor(job_inv) and job_inv.dtype == torch.float32 and job_inv.is_contiguous() and job_inv.device == dev
              and job_inv.shape == (J, 3, 4)):
        raise ValueError("tsdf_raycast: job_inv must be a contiguous (J,3,4) float32 tensor on the volumes' device")
    if not (isinstance(h, int) and isinstance(w, int) and 1 <= h <= RAYCAST_MAX_SIDE and 1 <= w <= RAYCAST_MAX_SIDE):
        raise ValueError("tsdf_raycast: h and w must be ints in [1, %d]" % RAYCAST_MAX_SIDE)
    if not (isinstance(min_weight, int) and min_weight >= 1):
        raise ValueError("tsdf_raycast: min_weight must be an int >= 1")
    if not (0.0625 <= float(step) < math.inf):
        raise ValueError("tsdf_raycast: step must be a finite number of voxels >= 1/16")
    if not (0.0 < float(near) < math.inf):
        raise ValueError("tsdf_raycast: near must be positive and finite")
    out = {"z": torch.empty(J, h, w, device=dev, dtype=torch.float32), "depth": torch.empty(J, h, w, device=dev, dtype=torch.int16),
           "vertex": torch.empty(J, h, w, 3, device=dev, dtype=torch.float32), "normal": torch.empty(J, h, w, 3, device=dev, dtype=torch.float32),
           "count": torch.empty(J, device=dev, dtype=torch.int32), "status": torch.empty(J, device=dev, dtype=torch.int32)}
    if J == 0:
        return out
    a = _lib.TsdfRaycastArgs(sum=_p(volumes.sum), weight=_p(volumes.weight), meta=_p(volumes.meta), M=len(volumes), G=volumes.G, camk=_p(camk),
                             S=camk.shape[0], job_img=_p(job_img), job_model=_p(job_model), job_inv=_p(job_inv), job_window=_p(window), J=J,
                             h=h, w=w, min_weight=min_weight, step=float(step), near=float(near), z=_p(out["z"]), depth=_p(out["depth"]),
                             vertex=_p(out["vertex"]), normal=_p(out["normal"]), count=_p(out["count"]), status=_p(out["status"]))
    check(_lib.lib().tgp_tsdf_raycast(ctypes.byref(a), _stream(job_pose)), "tgp_tsdf_raycast")
    return out


def tsdf_windows(volumes, camk, job_img, job_model, job_pose, h, w, H, W, pad=1.0):
    """The ray-cast windows that frame each job's cube: (J,4) float32 (u0, v0, du, dv) on the device, an h x w grid that spans the box
    of the cube's eight projected corners grown by ``pad`` pixels and clamped to the frame [0, W-1] x [0, H-1] (du = (u1 - u0) / (w
    - 1); 1 for a single column).  A cube with a corner at or behind the camera (z <= 1e-6), or whose projection is not finite,
    gets four NaN: every ray of it misses.  Indices out of range are clamped here (tsdf_raycast refuses the job).  Made of torch
    operations, float32 one operation at a time (tests/raycast_ref.py windows); nothing is read back."""
    dev, J = _raycast_jobs(volumes, camk, job_img, job_model, job_pose, "tsdf_windows")
    if not all(isinstance(v, int) and v >= 1 for v in (h, w, H, W)):
        raise ValueError("tsdf_windows: h, w, H, W must be ints >= 1")
    meta = volumes.meta[job_model.long().clamp(0, len(volumes) - 1)]                  # (J,4)
    K = camk[job_img.long().clamp(0, camk.shape[0] - 1)]
    halfe = (meta[:, 3] * float(volumes.G)) * 0.5
    k = torch.arange(8, device=dev)
    signs = torch.stack([k // 4 % 2, k // 2 % 2, k % 2], 1).float() * 2.0 - 1.0              # (8,3) of +-1, made on the device
    p = meta[:, None, :3] + signs[None] * halfe[:, None, None]                          # (J,8,3): +- halfe is exact
    T = job_pose
    c = [((T[:, None, r, 0] * p[:, :, 0] + T[:, None, r, 1] * p[:, :, 1]) + T[:, None, r, 2] * p[:, :, 2]) + T[:, None, r, 3] for r in range(3)]
    us = K[:, None, 0] * (c[0] / c[2]) + K[:, None, 2]
    vs = K[:, None, 1] * (c[1] / c[2]) + K[:, None, 3]
    good = (c[2] > 1e-6).all(1) & torch.isfinite(us).all(1) & torch.isfinite(vs).all(1)
    u0 = (us.min(1).values - float(pad)).clamp(0.0, float(W - 1))
    u1 = (us.max(1).values + float(pad)).clamp(0.0, float(W - 1))
    v0 = (vs.min(1).values - float(pad)).clamp(0.0, float(H - 1))
    v1 = (vs.max(1).values + float(pad)).clamp(0.0, float(H - 1))
    du = (u1 - u0) / float(w - 1) if w > 1 else torch.ones_like(u0)
    dv = (v1 - v0) / float(h - 1) if h > 1 else torch.ones_like(v0)
    win = torch.stack([u0, v0, du, dv], 1)
    return torch.where(good[:, None], win, torch.full_like(win, float("nan"))).contiguous()


# ------------------------------------------------------------------------------------------------------------ dense projective ICP
def dense_rects(window, h, w, H, W):
    """The frame pixels that the h x w ray grids of ``window`` (J,4) float32 = (u0, v0, du, dv) cover, as icp_dense's job_rect: (J,4)
    int32 (x0, y0, x1, y1) inclusive = the floor of the smaller and the ceil of the larger of each axis' two ends (u0 and u0 +
    (w - 1) du, float32), clamped to the frame [0, W-1] x [0, H-1].  A window with a NaN in an end (tsdf_windows' empty window)
    gives the empty rectangle (0, 0, -1, -1).  Torch operations on the window's device (tests/icp_dense_ref.py rects); nothing is
    read back."""
    if not (torch.is_tensor(window) and window.dtype == torch.float32 and window.dim() == 2 and window.shape[1] == 4):
        raise ValueError("dense_rects: window must be a (J,4) float32 tensor")
    if not all(isinstance(v, int) and v >= 1 for v in (h, w, H, W)):
        raise ValueError("dense_rects: h, w, H, W must be ints >= 1")
    ua, va = window[:, 0], window[:, 1]
    ub, vb = ua + float(w - 1) * window[:, 2], va + float(h - 1) * window[:, 3]
    bad = torch.isnan(ua) | torch.isnan(ub) | torch.isnan(va) | torch.isnan(vb)
    box = torch.stack([torch.minimum(ua, ub).floor().clamp(0.0, float(W - 1)), torch.minimum(va, vb).floor().clamp(0.0, float(H - 1)),
                       torch.maximum(ua, ub).ceil().clamp(0.0, float(W - 1)), torch.maximum(va, vb).ceil().clamp(0.0, float(H - 1))], 1)
    empty = -(torch.arange(4, dtype=torch.int32, device=window.device) // 2)               # (0, 0, -1, -1), made on the device
    box = torch.where(bad[:, None], torch.zeros_like(box), box).to(torch.int32)           # a NaN has no integer
    return torch.where(bad[:, None], empty[None], box).contiguous()


def icp_dense(depth, camk, job_img, rect, rc, window, ref_pose, R, t, s, max_dist, *, stride=1, mask=None, job_mask_val=None, iters=30,
              tol_rot=1e-5, tol_trans=1e-6, min_inliers=6, corr_cap=0):
    """tgp_icp_dense (csrc/icp_dense.hip; DESIGN.md section 3 "Dense projective registration"): J poses registered to depth frames
    against the maps of one tsdf_raycast call, in one launch, every iteration on the device.  A source pixel finds its model point
    by projecting into the map (no search), so every depth pixel of the object can take part.  depth (S,H,W) 16-bit millimetres,
    camk (S,4), job_img (J) int32, mask (S,H,W) uint8 with job_mask_val (J) uint8 or neither, as tsdf_integrate takes them; rect
    (J,4) int32 (x0, y0, x1, y1) inclusive (dense_rects) and ``stride``: the job's source pixels (x0 + i stride, y0 + k stride)
    inside the frame; rc: tsdf_raycast's dict (z, vertex, normal of J jobs), window (J,4) and ref_pose (J,3,4) [s R | t]: the window
    and pose that call cast from; R (J,3,3), t (J,3), s (J): the start x = s R y + t; max_dist (J) float32 (or one number): the
    gate in metres; iters, tol_rot, tol_trans, min_inliers as icp_refine takes them.
    -> (R, t, s, info (J,4) int32 = status, final inliers, iterations, candidates (pixels associated at the start pose before the
    gate); rmse (J)[, corr (J, corr_cap) int32 with corr_cap > 0: source pixel e's final map cell, -1 for a non-inlier]).  A job that
    fails (ICP_STATUS; 3: job_img out of range) returns the pose it came with.  Nothing is read back (icp_check_status does)."""
    if not (isinstance(stride, int) and stride >= 1):
        raise ValueError("icp_dense: stride must be an int >= 1")
    if not (isinstance(iters, int) and iters >= 1):
        raise ValueError("icp_dense: iters must be an int >= 1")
    if not (tol_rot >= 0 and tol_trans >= 0 and isinstance(min_inliers, int) and min_inliers >= 0):
        raise ValueError("icp_dense: tol_rot, tol_trans and min_inliers must not be negative")
    if not (isinstance(corr_cap, int) and corr_cap >= 0):
        raise ValueError("icp_dense: corr_cap must be an int >= 0")
    if not (isinstance(rc, dict) and all(k in rc for k in ("z", "vertex", "normal"))):
        raise TypeError("icp_dense: rc must be tsdf_raycast's dict (z, vertex, normal)")
    if not (torch.is_tensor(job_img) and job_img.is_cuda):
        raise TypeError("icp_dense: job_img must be a contiguous int32 GPU tensor")
    dev = job_img.device
    J = job_img.numel()
    if not torch.is_tensor(max_dist):
        max_dist = torch.full((J,), float(max_dist), device=dev, dtype=torch.float32)
    S, H, W, J = _frame_jobs("icp_dense", dev, depth, camk, job_img,
                             [(rect, "rect", torch.int32, (4,)), (window, "window", torch.float32, (4,)),
                              (ref_pose, "ref_pose", torch.float32, (3, 4)), (R, "R", torch.float32, (3, 3)), (t, "t", torch.float32, (3,)),
                              (s, "s", torch.float32, ()), (max_dist, "max_dist", torch.float32, ())],
                             mask, job_mask_val, where="job_img's device")
    z, vertex, normal = rc["z"], rc["vertex"], rc["normal"]
    _gpu_args("icp_dense", dev, [(z, "rc['z']", torch.float32), (vertex, "rc['vertex']", torch.float32), (normal, "rc['normal']", torch.float32)],
              where="job_img's device")
    if z.dim() != 3 or z.shape[0] != J or vertex.shape != z.shape + (3,) or normal.shape != z.shape + (3,):
        raise ValueError("icp_dense: rc must hold z (J,h,w), vertex and normal (J,h,w,3) of the %d jobs" % J)
    h, w = z.shape[1:]
    if not (1 <= h <= RAYCAST_MAX_SIDE and 1 <= w <= RAYCAST_MAX_SIDE):
        raise ValueError("icp_dense: the maps' h and w must be in [1, %d]" % RAYCAST_MAX_SIDE)
    if J > 65535 or H > 16384 or W > 16384:
        raise ValueError("icp_dense: at most 65535 jobs a call and frames of at most 16384 pixels a side")
    R_out, t_out, s_out = torch.empty_like(R), torch.empty_like(t), torch.empty_like(s)
    info = torch.empty(J, 4, device=dev, dtype=torch.int32)
    rmse = torch.empty(J, device=dev, dtype=torch.float32)
    corr = torch.empty(J, corr_cap, device=dev, dtype=torch.int32) if corr_cap else None
    if J > 0:
        a = _lib.IcpDenseArgs(depth=_p(depth), camk=_p(camk), S=S, H=H, W=W, mask=_p(mask), job_mask_val=_p(job_mask_val), vertex=_p(vertex),
                              normal=_p(normal), z=_p(z), h=h, w=w, job_window=_p(window), job_ref=_p(ref_pose), job_img=_p(job_img),
                              job_rect=_p(rect), J=J, stride=stride, R=_p(R), t=_p(t), s=_p(s), max_dist=_p(max_dist), iters=iters,
                              tol_rot=float(tol_rot), tol_trans=float(tol_trans), min_inliers=min_inliers, R_out=_p(R_out), t_out=_p(t_out),
                              s_out=_p(s_out), info=_p(info), rmse=_p(rmse), corr=_p(corr), corr_cap=corr_cap)
        check(_lib.lib().tgp_icp_dense(ctypes.byref(a), _stream(job_img)), "tgp_icp_dense")
    out = (R_out, t_out, s_out, info, rmse)
    return out + (corr,) if corr_cap else out


# ------------------------------------------------------------------------------------------------------------ maps of posed meshes
MESH_MAPS_MAX_JOBS = _lib.MAPS_MAX_JOBS


def _mesh_map_jobs(meshset, camk, job_img, job_mesh, job_pose, who):
    if not isinstance(meshset, MeshSet):
        raise TypeError("%s: meshset must be an ops.MeshSet" % who)
    dev = meshset.verts.device
    _gpu_args(who, dev, [(camk, "camk", torch.float32), (job_img, "job_img", torch.int32), (job_mesh, "job_mesh", torch.int32),
                         (job_pose, "job_pose", torch.float32)])
    J = job_img.numel()
    if camk.dim() != 2 or camk.shape[1] != 4 or camk.shape[0] < 1 or job_img.dim() != 1 or job_mesh.shape != (J,) or job_pose.shape != (J, 3, 4):
        raise ValueError("%s: camk (S,4), job_img (J), job_mesh (J), job_pose (J,3,4) are expected" % who)
    if J > MESH_MAPS_MAX_JOBS:
        raise ValueError("%s: at most %d jobs" % (who, MESH_MAPS_MAX_JOBS))
    return dev, J


def mesh_maps(meshset, camk, job_img, job_mesh, job_pose, window, h, w, *, near=0.01, normals="face", return_face=False):
    """The surface of posed meshes as cameras see it, as tsdf_raycast's maps (tgp_mesh_maps, csrc/meshmaps.hip; DESIGN.md section 3
    "Mesh maps and dense model-based tracking").  Job j rasterises mesh job_mesh[j] of the set at job_pose[j] (3,4) [s R | t] (model ->
    camera, metres) under the intrinsics camk[job_img[j]] into an h x w grid whose cell (r, c) is the pixel coordinate (u0 + c du, v0 +
    r dv) of window[j] = (u0, v0, du, dv): render_depth's surface, sampled by the window.  All tensors on the mesh set's GPU: camk (S,4)
    float32, job_img, job_mesh (J) int32, job_pose (J,3,4), window (J,4) float32.  normals: 'face' (the winning triangle's normal,
    turned towards the camera) or 'vertex' (meshset.vert_normals interpolated over the triangle and renormalised; not turned).
    -> dict: z (J,h,w) float32 camera depth in metres (0: a miss), depth (J,h,w) int16-viewed uint16 millimetres, vertex, normal
    (J,h,w,3) float32 in the MODEL frame (zeros on a miss), count (J) int32 hits, dropped (J) int32 triangles dropped by the near rule
    and the guard band, status (J) int32: 1 for a job whose frame or mesh index is out of range (all its cells miss); with
    return_face face (J,h,w) int32 within the mesh, -1 on a miss.  icp_dense(rc=...) and IcpModels.from_raycast take the dict as it
    stands.  Nothing is read back."""
    dev, J = _mesh_map_jobs(meshset, camk, job_img, job_mesh, job_pose, "mesh_maps")
    if not (torch.is_tensor(window) and window.is_cuda and window.dtype == torch.float32 and window.is_contiguous() and window.device == dev
            and window.shape == (J, 4)):
        raise ValueError("mesh_maps: window must be a contiguous (J,4) float32 tensor on the mesh set's device")
    if not (isinstance(h, int) and isinstance(w, int) and 1 <= h <= RAYCAST_MAX_SIDE and 1 <= w <= RAYCAST_MAX_SIDE):
        raise ValueError("mesh_maps: h and w must be ints in [1, %d]" % RAYCAST_MAX_SIDE)
    if not (0.0 < float(near) < math.inf):
        raise ValueError("mesh_maps: near must be positive and finite")
    if normals not in ("face", "vertex"):
        raise ValueError("mesh_maps: normals must be 'face' or 'vertex'")
    vn = None
    if normals == "vertex":
        vn = meshset.vert_normals
        if vn is None:
            raise ValueError("mesh_maps: normals='vertex' needs meshset.vert_normals (ops.mesh_vertex_normals makes them)")
        _gpu_args("mesh_maps", dev, [(vn, "meshset.vert_normals", torch.float32)])
        if vn.shape != meshset.verts.shape:
            raise ValueError("mesh_maps: meshset.vert_normals must be (sum V,3), one row per vertex")
    out = {"z": torch.empty(J, h, w, device=dev, dtype=torch.float32), "depth": torch.empty(J, h, w, device=dev, dtype=torch.int16),
           "vertex": torch.empty(J, h, w, 3, device=dev, dtype=torch.float32), "normal": torch.empty(J, h, w, 3, device=dev, dtype=torch.float32),
           "count": torch.empty(J, device=dev, dtype=torch.int32), "dropped": torch.empty(J, device=dev, dtype=torch.int32),
           "status": torch.empty(J, device=dev, dtype=torch.int32)}
    if return_face:
        out["face"] = torch.empty(J, h, w, device=dev, dtype=torch.int32)
    if J == 0:
        return out
    mesh = meshset.fields(maxima=True)
    ws = _workspace(dev, _lib.lib().tgp_mesh_maps_workspace_bytes(J, mesh["max_verts"], mesh["max_faces"]), "tgp_mesh_maps_workspace_bytes")
    a = _lib.MeshMapsArgs(camk=_p(camk), vnormals=_p(vn), job_img=_p(job_img), job_mesh=_p(job_mesh), job_pose=_p(job_pose),
                          job_window=_p(window), S=camk.shape[0], J=J, h=h, w=w, near=float(near), z=_p(out["z"]), depth=_p(out["depth"]),
                          vertex=_p(out["vertex"]), normal=_p(out["normal"]), face=_p(out.get("face")), count=_p(out["count"]),
                          dropped=_p(out["dropped"]), status=_p(out["status"]), workspace=_p(ws), workspace_bytes=ws.numel(), **mesh)
    check(_lib.lib().tgp_mesh_maps(ctypes.byref(a), _stream(job_pose)), "tgp_mesh_maps")
    return out


def mesh_windows(meshset, camk, job_img, job_mesh, job_pose, h, w, H, W, pad=1.0):
    """The map windows that frame each job's mesh: tsdf_windows' rule on the eight corners of the mesh's axis-aligned bounding box
    (MeshSet.bounds, made once on the device) instead of a cube's: (J,4) float32 (u0, v0, du, dv) on the device, an h x w grid that spans
    the box of the projected corners grown by ``pad`` pixels and clamped to the frame [0, W-1] x [0, H-1] (du = (u1 - u0) / (w - 1); 1
    for a single column).  A box with a corner at or behind the camera (z <= 1e-6), or whose projection is not finite, gets four NaN:
    every cell of it misses.  Indices out of range are clamped here (mesh_maps refuses the job).  Made of torch operations, float32 one
    operation at a time (tests/meshmaps_ref.py windows); nothing is read back."""
    dev, J = _mesh_map_jobs(meshset, camk, job_img, job_mesh, job_pose, "mesh_windows")
    if not all(isinstance(v, int) and v >= 1 for v in (h, w, H, W)):
        raise ValueError("mesh_windows: h, w, H, W must be ints >= 1")
    bounds = meshset.bounds()[job_mesh.long().clamp(0, len(meshset) - 1)]            # (J,2,3): the least and the greatest coordinates
    K = camk[job_img.long().clamp(0, camk.shape[0] - 1)]
    k = torch.arange(8, device=dev)
    high = torch.stack([k // 4 % 2, k // 2 % 2, k % 2], 1).bool()                            # (8,3), made on the device
    p = torch.where(high[None], bounds[:, None, 1], bounds[:, None, 0])                     # (J,8,3)
    T = job_pose
    c = [((T[:, None, r, 0] * p[:, :, 0] + T[:, None, r, 1] * p[:, :, 1]) + T[:, None, r, 2] * p[:, :, 2]) + T[:, None, r, 3] for r in range(3)]
    us = K[:, None, 0] * (c[0] / c[2]) + K[:, None, 2]
    vs = K[:, None, 1] * (c[1] / c[2]) + K[:, None, 3]
    good = (c[2] > 1e-6).all(1) & torch.isfinite(us).all(1) & torch.isfinite(vs).all(1)
    u0 = (us.min(1).values - float(pad)).clamp(0.0, float(W - 1))
    u1 = (us.max(1).values + float(pad)).clamp(0.0, float(W - 1))
    v0 = (vs.min(1).values - float(pad)).clamp(0.0, float(H - 1))
    v1 = (vs.max(1).values + float(pad)).clamp(0.0, float(H - 1))
    # a tensor divided by a tensor is a correctly rounded division; by a Python number it may become a product with the reciprocal
    du = (u1 - u0) / torch.full_like(u0, float(w - 1)) if w > 1 else torch.ones_like(u0)
    dv = (v1 - v0) / torch.full_like(v0, float(h - 1)) if h > 1 else torch.ones_like(v0)
    win = torch.stack([u0, v0, du, dv], 1)
    return torch.where(good[:, None], win, torch.full_like(win, float("nan"))).contiguous()


# ------------------------------------------------------------------------------------------------------------ the supporting plane
PLANE_STATUS = {1: "no hypothesis reached min_inliers", 2: "a refit was not finite (the plane of before it is returned)"}


def _plane_frames(depth, camk, who):
    """depth (S,H,W) 16-bit and camk (S,4) float32, contiguous on one GPU -> (S, H, W); ValueError otherwise"""
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype in (torch.int16, torch.uint16) and depth.dim() == 3
            and depth.is_contiguous() and depth.numel() > 0):
        raise ValueError("%s: depth must be a contiguous (S,H,W) 16-bit GPU tensor" % who)
    S, H, W = depth.shape
    if not (torch.is_tensor(camk) and camk.device == depth.device and camk.dtype == torch.float32 and camk.shape == (S, 4)
            and camk.is_contiguous()):
        raise ValueError("%s: camk must be a contiguous (S,4) float32 tensor on the depth's device" % who)
    if S > 65535 or H >= 32768 or W >= 32768 or H * W >= 2 ** 24:
        raise ValueError("%s: at most 65535 frames of fewer than 2^24 pixels, sides below 32768" % who)
    return S, H, W


def plane_fit(depth, camk, *, tol=0.004, hypotheses=256, seed=0, keys=None, refine_iters=2, min_inliers=100, return_counts=False):
    """tgp_plane_fit (csrc/plane.hip; DESIGN.md section 3 "The supporting plane"): the dominant plane of each of the S frames of depth
    (S,H,W) (int16-viewed uint16 millimetres, 0 invalid) with intrinsics camk (S,4) fx, fy, cx, cy, in one call.  ``hypotheses``
    three-pixel planes per frame are drawn from the Philox words of (seed, keys[s]) (keys: (S) ints or an int64 tensor; default the
    frame's index), scored by their count of pixels within ``tol`` metres, and the best is refitted ``refine_iters`` times by total
    least squares over its inliers.  -> (plane (S,4) float32: unit normal and offset, n.p + d = 0, d >= 0; info (S,4) int32: status
    (PLANE_STATUS), the best hypothesis's count, the final inliers, the valid pixels[; counts (S, hypotheses) int32]).  Nothing is
    read back (plane_check_status does)."""
    S, H, W = _plane_frames(depth, camk, "plane_fit")
    if not (isinstance(hypotheses, int) and 1 <= hypotheses <= _lib.PLANE_MAX_HYPOTHESES):
        raise ValueError("plane_fit: hypotheses must be an int in [1, %d]" % _lib.PLANE_MAX_HYPOTHESES)
    if not (isinstance(refine_iters, int) and 0 <= refine_iters <= _lib.PLANE_MAX_REFITS):
        raise ValueError("plane_fit: refine_iters must be an int in [0, %d]" % _lib.PLANE_MAX_REFITS)
    if not (isinstance(min_inliers, int) and min_inliers >= 0):
        raise ValueError("plane_fit: min_inliers must be an int >= 0")
    if not (0.0 <= float(tol) < math.inf):
        raise ValueError("plane_fit: tol must be a finite number >= 0")
    dev = depth.device
    if keys is None:
        keys = torch.arange(S, dtype=torch.int64, device=dev)
    elif not torch.is_tensor(keys):
        import numpy as np
        keys = torch.from_numpy(np.asarray([int(k) & (2 ** 64 - 1) for k in keys], dtype=np.uint64).view(np.int64)).to(dev)
    if not (keys.dtype == torch.int64 and keys.device == dev and keys.shape == (S,) and keys.is_contiguous()):
        raise ValueError("plane_fit: keys must be (S) = (%d) 64-bit integers on the depth's device" % S)
    plane = torch.empty(S, 4, device=dev, dtype=torch.float32)
    info = torch.empty(S, 4, device=dev, dtype=torch.int32)
    counts = torch.empty(S, hypotheses, device=dev, dtype=torch.int32)
    a = _lib.PlaneFitArgs(depth=_p(depth), camk=_p(camk), keys=_p(keys), seed=int(seed) & (2 ** 64 - 1), S=S, H=H, W=W,
                          hypotheses=hypotheses, tol=float(tol), refine_iters=refine_iters, min_inliers=min_inliers, plane=_p(plane),
                          info=_p(info), counts=_p(counts))
    check(_lib.lib().tgp_plane_fit(ctypes.byref(a), _stream(depth)), "tgp_plane_fit")
    return (plane, info, counts) if return_counts else (plane, info)


def plane_cut(depth, plane, info, camk, margin=0.006, return_side=False):
    """tgp_plane_cut: the frames of depth (S,H,W) without their plane: a pixel keeps its depth when its signed distance to plane[s]
    is above ``margin`` metres (on the camera's side), else it becomes 0; a frame whose info[s, 0] is not 0 is copied through.  plane
    (S,4) and info (S,4) are plane_fit's, read on the device.  -> out (S,H,W), the depth's dtype[, side (S,H,W) uint8: 0 invalid,
    1 within the margin, 2 above, 3 below]."""
    S, H, W = _plane_frames(depth, camk, "plane_cut")
    dev = depth.device
    if not (torch.is_tensor(plane) and plane.device == dev and plane.dtype == torch.float32 and plane.shape == (S, 4) and plane.is_contiguous()):
        raise ValueError("plane_cut: plane must be a contiguous (S,4) float32 tensor on the depth's device")
    if not (torch.is_tensor(info) and info.device == dev and info.dtype == torch.int32 and info.shape == (S, 4) and info.is_contiguous()):
        raise ValueError("plane_cut: info must be a contiguous (S,4) int32 tensor on the depth's device")
    if not (0.0 <= float(margin) < math.inf):
        raise ValueError("plane_cut: margin must be a finite number >= 0")
    out = torch.empty_like(depth)
    side = torch.empty(S, H, W, device=dev, dtype=torch.uint8) if return_side else None
    check(_lib.lib().tgp_plane_cut(_p(depth), _p(plane), _p(info), _p(camk), S, H, W, float(margin), _p(out), _p(side), _stream(depth)),
          "tgp_plane_cut")
    return (out, side) if return_side else out


def plane_check_status(info, what="plane_fit"):
    """one read of the (S,4) info words; raises TgpError naming the first frame without a plane"""
    st = info[:, 0].cpu().tolist()
    bad = [(j, s) for j, s in enumerate(st) if s != 0]
    if bad:
        raise _lib.TgpError("%s: frame %d: %s (%d of %d frames)" % (what, bad[0][0], PLANE_STATUS.get(bad[0][1], bad[0][1]), len(bad), len(st)))


def plane_lsq(pc, w, eps=0.0):
    """tgp_plane_lsq: the weighted regression z = a x + b y + c of the B clouds pc (B,n,3) with weights w (B,n), float32 on the GPU,
    one launch.  -> (X (B,3) = a, b, c; normal (B,3); dn (B,3); p2plane (B)) float32, tools/plane_utils.py's formulas with its
    ``eps`` added to the divisor of dn.  A singular system (n < 3, collinear points) gives NaN rows."""
    if not (torch.is_tensor(pc) and pc.is_cuda and pc.dtype == torch.float32 and pc.dim() == 3 and pc.shape[2] == 3 and pc.is_contiguous()
            and pc.shape[0] >= 1 and pc.shape[1] >= 1):
        raise ValueError("plane_lsq: pc must be a contiguous (B,n,3) float32 GPU tensor, B, n >= 1")
    B, n = pc.shape[:2]
    if not (torch.is_tensor(w) and w.device == pc.device and w.dtype == torch.float32 and w.shape == (B, n) and w.is_contiguous()):
        raise ValueError("plane_lsq: w must be a contiguous (B,n) float32 tensor on pc's device")
    if not (0.0 <= float(eps) < math.inf):
        raise ValueError("plane_lsq: eps must be a finite number >= 0")
    X, normal, dn = (torch.empty(B, 3, device=pc.device, dtype=torch.float32) for _ in range(3))
    p2 = torch.empty(B, device=pc.device, dtype=torch.float32)
    check(_lib.lib().tgp_plane_lsq(_p(pc), _p(w), B, n, float(eps), _p(X), _p(normal), _p(dn), _p(p2), _stream(pc)), "tgp_plane_lsq")
    return X, normal, dn, p2


# --------------------------------------------------------------------------------------------------------- segments of depth frames
SEG_MAX_SEGMENTS, SEG_STAT_COLS = _lib.SEG_MAX_SEGMENTS, _lib.SEG_STAT_COLS
SEG_STATUS = {1: "more components qualified than max_segments (the first max_segments in root order are kept)"}


class Segments(object):
    """What segment_depth returns, all on the depth's device: ``labels`` (S,H,W) uint8 (0: no segment, l: segment l), ``info`` (S,4)
    int32 (status, segments kept, components that qualified, valid pixels), ``stats`` (S, max_segments, 12) int64 (row l - 1 for label
    l: pixels, y1, x1, y2, x2 with exclusive ends, root, sum x, sum y, sum z, sum x z, sum y z, min z; rows past the kept count zero),
    ``centers`` (S, max_segments, 3) float32 metres or None (rows past the kept count NaN), and the parameters of the call."""

    def __init__(self, labels, info, stats, centers, max_step, connectivity, min_pixels, max_segments):
        self.labels, self.info, self.stats, self.centers = labels, info, stats, centers
        self.max_step, self.connectivity, self.min_pixels, self.max_segments = max_step, connectivity, min_pixels, max_segments

    def by_size(self):
        """(S, max_segments) int64: per frame the rows of ``stats`` by descending pixel count, equal counts (the empty rows among
        them) by ascending label -- a stable sort on the device, nothing is read back"""
        return torch.sort(self.stats[:, :, 0], dim=1, descending=True, stable=True).indices


def segment_depth(depth, *, max_step=10, connectivity=4, min_pixels=50, max_segments=32, camk=None):
    """tgp_segment_depth (csrc/segment.hip; DESIGN.md section 3 "Segments of a depth frame"): the connected components of each of the
    S frames of depth (S,H,W) (int16-viewed uint16 millimetres, 0 invalid), in one call.  Neighbouring valid pixels (``connectivity``
    4 or 8) are joined when their depths differ by at most ``max_step`` millimetres; components of at least ``min_pixels`` pixels are
    numbered 1, 2, ... by their smallest flat index, ``max_segments`` (at most SEG_MAX_SEGMENTS) of them at most.  camk (S,4) fx,
    fy, cx, cy: the segments' centroids are returned too.  -> Segments.  Nothing is read back (seg_check_status does)."""
    if not (isinstance(max_step, int) and 0 <= max_step <= 65535):
        raise ValueError("segment_depth: max_step must be an int in [0, 65535]")
    if connectivity not in (4, 8):
        raise ValueError("segment_depth: connectivity must be 4 or 8")
    if not (isinstance(min_pixels, int) and min_pixels >= 1):
        raise ValueError("segment_depth: min_pixels must be an int >= 1")
    if not (isinstance(max_segments, int) and 1 <= max_segments <= SEG_MAX_SEGMENTS):
        raise ValueError("segment_depth: max_segments must be an int in [1, %d]" % SEG_MAX_SEGMENTS)
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype in (torch.int16, torch.uint16) and depth.dim() == 3
            and depth.is_contiguous() and depth.numel() > 0):
        raise ValueError("segment_depth: depth must be a contiguous (S,H,W) 16-bit GPU tensor")
    S, H, W = depth.shape
    if S > 65535 or H >= 32768 or W >= 32768 or H * W >= 2 ** 24:
        raise ValueError("segment_depth: at most 65535 frames of fewer than 2^24 pixels, sides below 32768")
    if camk is not None and not (torch.is_tensor(camk) and camk.device == depth.device and camk.dtype == torch.float32
                                 and camk.shape == (S, 4) and camk.is_contiguous()):
        raise ValueError("segment_depth: camk must be a contiguous (S,4) float32 tensor on the depth's device")
    dev = depth.device
    work = _workspace(dev, _lib.lib().tgp_segment_workspace_bytes(S, H, W), "tgp_segment_workspace_bytes", torch.int32)
    labels = torch.empty(S, H, W, device=dev, dtype=torch.uint8)
    info = torch.empty(S, 4, device=dev, dtype=torch.int32)
    stats = torch.empty(S, max_segments, SEG_STAT_COLS, device=dev, dtype=torch.int64)
    centers = torch.empty(S, max_segments, 3, device=dev, dtype=torch.float32) if camk is not None else None
    a = _lib.SegmentArgs(depth=_p(depth), camk=_p(camk), S=S, H=H, W=W, max_step=max_step, connectivity=int(connectivity),
                         min_pixels=min(min_pixels, 2 ** 31 - 1), max_segments=max_segments, labels=_p(labels), info=_p(info),
                         stats=_p(stats), centers=_p(centers), workspace=_p(work), workspace_bytes=work.numel() * 4)
    check(_lib.lib().tgp_segment_depth(ctypes.byref(a), _stream(depth)), "tgp_segment_depth")
    return Segments(labels, info, stats, centers, max_step, int(connectivity), min_pixels, max_segments)


def seg_check_status(info, what="segment_depth"):
    """one read of the (S,4) info words; raises TgpError naming the first frame whose segments were cut off at max_segments"""
    st = info[:, 0].cpu().tolist()
    bad = [(j, s) for j, s in enumerate(st) if s != 0]
    if bad:
        raise _lib.TgpError("%s: frame %d: %s (%d of %d frames)" % (what, bad[0][0], SEG_STATUS.get(bad[0][1], bad[0][1]), len(bad), len(st)))


# ---------------------------------------------------------------------------------------------------------- the optimizer step
def ranger_plan(table):
    """Check a host descriptor table (a ctypes array of _lib.RangerTensor) and fill its unit0 fields (tgp_ranger_plan, host only:
    nothing is launched); returns the launch's number of work units."""
    units = ctypes.c_int64(0)
    check(_lib.lib().tgp_ranger_plan(table, len(table), ctypes.byref(units)), "tgp_ranger_plan")
    return units.value


def ranger_step(table_dev, n, units):
    """One Ranger step (tgp_ranger_step) over the n descriptors of table_dev: a uint8 device tensor holding the bytes of the table
    ranger_plan filled, on the current stream of its device."""
    a = _lib.RangerArgs()
    a.tensors, a.n, a.units = _p(table_dev), int(n), int(units)
    check(_lib.lib().tgp_ranger_step(ctypes.byref(a), _stream(table_dev)), "tgp_ranger_step")


# ------------------------------------------------------------------------------------------------ the training augmentation
def _aug_arg(t, name, shape, dtype=torch.float32):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError("augment: %s must be a contiguous %s GPU tensor" % (name, dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("augment: %s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def augment(pc, base=None, view=None, pc_out=None, ld_out=3):
    """The training item's cloud augmentation (tgp_augment, include/tgpose.h), one launch for the batch.

    pc (B,N,3).  base: dict draws (B,6), R (B,3,3), t, s, mean_shape, aug_bb, aug_rt_t (B,3), sym (B,4), aug_rt_R (B,3,3), cat_id,
    nocs_scale (B), model_point (B,n_model,3), defor (B,N,3), pro = (bb, rt, bc, pc) and pc_r floats.  view: dict op (B) int32,
    noise (B,N,3) float32, drop_ratio (B), drop_u (B,N) and boxes (B,AUGMENT_MAX_TRY,6) float64, crop_max_try, cutout_max_try,
    crop_min_points, cutout_min_points.  pc_out: the base-augmented cloud's buffer (may be pc; new when None).
    -> dict: with base, pc / R / t / s / flags (B,4) int32; with view, view (B,N,3) and counts (B,2) int32 = (M, attempt)."""
    if base is None and view is None:
        raise ValueError("augment: nothing to do")
    B, N = pc.shape[0], pc.shape[1]
    _aug_arg(pc, "pc", (B, N, 3))
    dev = pc.device
    if ld_out not in (3, 4):
        raise ValueError("augment: ld_out must be 3 or 4")
    a = _lib.AugmentArgs()
    a.B, a.N, a.pc, a.ld_out = B, N, _p(pc), ld_out
    out = {}
    if base is not None:
        nm = base["model_point"].shape[1] if base["model_point"].dim() == 3 else -1
        for k, shp in (("draws", (B, 6)), ("R", (B, 3, 3)), ("t", (B, 3)), ("s", (B, 3)), ("mean_shape", (B, 3)), ("sym", (B, 4)),
                       ("aug_bb", (B, 3)), ("aug_rt_t", (B, 3)), ("aug_rt_R", (B, 3, 3)), ("cat_id", (B,)), ("nocs_scale", (B,)),
                       ("model_point", (B, nm, 3)), ("defor", (B, N, 3))):
            setattr(a, k, _p(_aug_arg(base[k], k, shp)))
        a.n_model = nm
        a.pro_bb, a.pro_rt, a.pro_bc, a.pro_pc = (float(v) for v in base["pro"])
        a.pc_r = float(base["pc_r"])
        pc_out = torch.empty(B, N, ld_out, device=dev) if pc_out is None else _aug_arg(pc_out, "pc_out", (B, N, ld_out))
        out.update(pc=pc_out, R=torch.empty(B, 3, 3, device=dev), t=torch.empty(B, 3, device=dev), s=torch.empty(B, 3, device=dev),
                   flags=torch.empty(B, 4, device=dev, dtype=torch.int32))
        a.pc_out, a.R_out, a.t_out, a.s_out, a.flags_out = (_p(out[k]) for k in ("pc", "R", "t", "s", "flags"))
    if view is not None:
        _aug_arg(view["op"], "op", (B,), torch.int32)
        _aug_arg(view["noise"], "noise", (B, N, 3))
        _aug_arg(view["drop_ratio"], "drop_ratio", (B,), torch.float64)
        _aug_arg(view["drop_u"], "drop_u", (B, N), torch.float64)
        _aug_arg(view["boxes"], "boxes", (B, _lib.AUGMENT_MAX_TRY, 6), torch.float64)
        a.op, a.noise, a.drop_ratio, a.drop_u, a.boxes = (_p(view[k]) for k in ("op", "noise", "drop_ratio", "drop_u", "boxes"))
        for k in ("crop_max_try", "cutout_max_try", "crop_min_points", "cutout_min_points"):
            setattr(a, k, int(view[k]))
        out.update(view=torch.empty(B, N, ld_out, device=dev), counts=torch.empty(B, 2, device=dev, dtype=torch.int32))
        a.view_out, a.count_out = _p(out["view"]), _p(out["counts"])
    check(_lib.lib().tgp_augment(ctypes.byref(a), _stream(pc)), "tgp_augment")
    return out


def _pd_launch(pcl, images, tets=False, tet_cap=0):
    if not isinstance(pcl, torch.Tensor) or pcl.dim() != 3 or pcl.shape[2] != 3:
        raise ValueError("persistence: pcl must be a (B, N, 3) tensor")
    if pcl.dtype != torch.float32 or pcl.device.type != "cuda":
        raise ValueError("persistence: pcl must be float32 on the device")
    B, N = pcl.shape[0], pcl.shape[1]
    if B == 0 or N == 0 or N > _lib.PD_MAX_POINTS:
        raise ValueError("persistence: 1 <= N <= %d points per cloud, B >= 1" % _lib.PD_MAX_POINTS)
    pcl = pcl.contiguous()
    dev = pcl.device
    lib = _lib.lib()
    ws = torch.empty(B * int(lib.tgp_pd_workspace_bytes()), dtype=torch.uint8, device=dev)
    out = dict(h1=torch.empty(B, _lib.PD_MAX_PAIRS, 2, dtype=torch.float64, device=dev),
               h2=torch.empty(B, _lib.PD_MAX_PAIRS, 2, dtype=torch.float64, device=dev),
               counts=torch.empty(B, 2, dtype=torch.int32, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev))
    a = _lib.PdArgs()
    a.B, a.N, a.pcl, a.workspace, a.tet_cap = B, N, _p(pcl), _p(ws), int(tet_cap)
    a.h1, a.h2, a.counts, a.status = (_p(out[k]) for k in ("h1", "h2", "counts", "status"))
    if tets:
        out.update(tets=torch.empty(B, _lib.PD_MAX_TETS, 4, dtype=torch.int32, device=dev), ntet=torch.empty(B, dtype=torch.int32, device=dev))
        a.tets, a.ntet = _p(out["tets"]), _p(out["ntet"])
    if images:
        out.update(pdh1=torch.empty(B, _lib.PD_PIXELS, device=dev), pdh2=torch.empty(B, _lib.PD_PIXELS, device=dev))
        a.pdh1, a.pdh2 = _p(out["pdh1"]), _p(out["pdh2"])
    check(lib.tgp_persistence(ctypes.byref(a), _stream(pcl)), "tgp_persistence")
    out["_ws"] = ws           # kept alive until the launches have run
    return out


def pd_check_status(status):
    """raise TgpError naming the clouds whose status word is not 0 (synchronises)"""
    st = status.cpu().numpy()
    bad = [(i, int(s)) for i, s in enumerate(st) if s != 0]
    if bad:
        raise _lib.TgpError("tgp_persistence failed for %d cloud(s): %s" % (len(bad), ", ".join(
            "cloud %d: %s" % (i, _lib.PD_STATUS.get(s, "status %d" % s)) for i, s in bad[:8])))


def persistence_images(pcl, check_status=True):
    """The reference's compute_pd images for a batch of clouds (tgp_persistence, include/tgpose.h): two launches, no host sync.

    pcl (B, N, 3) float32 on the device, N <= 1024.  -> (pdh1, pdh2), each (B, 2500) float32.  check_status=True synchronises
    once and raises TgpError if a cloud failed (capacity, degenerate cloud); False returns (pdh1, pdh2, status) without a sync,
    for graph capture (a failed cloud's images are zeros and its status word names the reason)."""
    out = _pd_launch(pcl, images=True)
    if check_status:
        pd_check_status(out["status"])
        return out["pdh1"], out["pdh2"]
    return out["pdh1"], out["pdh2"], out["status"]


def alpha_persistence(pcl, tet_cap=0):
    """Diagnosis and tests: the padded pairs and the triangulation of each cloud, without images and without a sync.

    -> dict h1 / h2 (B, 4096, 2) float64 (birth, death) rows [0, counts), counts (B, 2) int32 {H1, H2}, status (B) int32,
    tets (B, 8192, 4) int32 rows [0, ntet) the finite Delaunay tetrahedra as row indices of pcl, ntet (B) int32.
    tet_cap < 8192 caps the triangulation's storage (status TGP_PD_ETETS when it is exceeded)."""
    out = _pd_launch(pcl, images=False, tets=True, tet_cap=tet_cap)
    return out


# ------------------------------------------------------------------------------------------------- gradients to the points
@_timed("graph")
def gconv_dirgrad(xyz, idx, sdn, dg, S, C, proj=None, slots=None):
    """d(unit neighbour direction) (B, n, k, 3) of HSlayer_surface.graph_conv (proj None) or HS_layer.graph_conv (proj (B, n, 8C) rows;
    slots: gconv_hs_slots' record, read before gconv_hs_bwd_gather consumes it, or None: the winners are recomputed) from dg (B, n, C)"""
    _f32(xyz, "xyz", 3), _i32(idx, "idx"), _f32(sdn, "sdn", 2)
    if not xyz.is_contiguous() or not sdn.is_contiguous():
        raise ValueError("gconv_dirgrad: xyz and sdn must be contiguous")
    dg, ldg = _rows(dg, "dg")
    B, n, k = idx.shape
    ldp = 0
    if proj is not None:
        proj, ldp = _rows(proj, "proj")
    if slots is not None and (slots.dtype != torch.uint8 or slots.numel() != B * n * S * C or not slots.is_contiguous()):
        raise ValueError("gconv_dirgrad: slots must be a contiguous uint8 tensor of B*n*S*C entries")
    ddir = torch.empty(B, n, k, 3, device=xyz.device, dtype=torch.float32)
    check(_lib.lib().tgp_gconv_dirgrad(_p(xyz), _p(idx), _p(proj), ldp, _p(sdn), _p(dg), ldg, _p(slots), B, n, k, S, C, _p(ddir),
                                       _stream(xyz)), "tgp_gconv_dirgrad")
    return ddir


@_timed("graph")
def neighbor_dirs(xyz, idx, unnormed=False):
    """xyz (B, n, 3), idx (B, n, k) int32 -> unit directions (B, n, k, 3) [, the unnormalised differences]"""
    _f32(xyz, "xyz", 3), _i32(idx, "idx")
    B, n, k = idx.shape
    if not xyz.is_contiguous() or tuple(xyz.shape) != (B, n, 3):
        raise ValueError("neighbor_dirs: xyz must be contiguous (B, n, 3) with idx's B and n")
    unit = torch.empty(B, n, k, 3, device=xyz.device, dtype=torch.float32)
    raw = torch.empty_like(unit) if unnormed else None
    check(_lib.lib().tgp_neighbor_dirs(_p(xyz), _p(idx), B, n, k, _p(unit), _p(raw), _stream(xyz)), "tgp_neighbor_dirs")
    return (unit, raw) if unnormed else unit


def xyz_reverse_lists(idx, n_src):
    """reverse lists of a (B, n, k) xyz / feature graph for dirs_to_xyz: (rptr, rent, rev_global) -- tgp_reverse_graph's where it sorts
    the shape, else tgp_child_lists' over the flattened entries"""
    rev = reverse_graph(idx, n_src)
    if rev is not None:
        return rev[0], rev[1], 0
    B, n, k = idx.shape
    ptr, ent = child_lists(idx.contiguous().view(B, n * k), n_src)
    return ptr, ent, 1


@_timed("graph")
def dirs_to_xyz(xyz, idx, ddir, rev=None, dun=None, out=None, accumulate=False):
    """backward of get_neighbor_direction_norm: ddir (B, n, k, 3) d unit direction, dun (same) d unnormalised difference or None ->
    dxyz (B, n, 3); rev = xyz_reverse_lists(idx, n) or reverse_graph's pair (computed when None); accumulate: added to out"""
    _f32(xyz, "xyz", 3), _i32(idx, "idx"), _f32(ddir, "ddir", 4)
    B, n, k = idx.shape
    if not xyz.is_contiguous() or tuple(xyz.shape) != (B, n, 3):
        raise ValueError("dirs_to_xyz: xyz must be contiguous (B, n, 3) with idx's B and n")
    if tuple(ddir.shape) != (B, n, k, 3) or not ddir.is_contiguous():
        raise ValueError("dirs_to_xyz: ddir must be contiguous (B, n, k, 3)")
    if dun is not None:
        _f32(dun, "dun", 4)
        if tuple(dun.shape) != (B, n, k, 3) or not dun.is_contiguous():
            raise ValueError("dirs_to_xyz: dun must be contiguous (B, n, k, 3)")
    if rev is None:
        rev = xyz_reverse_lists(idx, n)
    elif len(rev) == 2:
        rev = (rev[0], rev[1], 0)
    if out is None:
        if accumulate:
            raise ValueError("dirs_to_xyz: accumulate needs out")
        out = torch.empty(B, n, 3, device=xyz.device, dtype=torch.float32)
    elif not (out.is_contiguous() and tuple(out.shape) == (B, n, 3) and out.dtype == torch.float32):
        raise ValueError("dirs_to_xyz: out must be contiguous float32 (B, n, 3)")
    check(_lib.lib().tgp_dirs_to_xyz(_p(xyz), _p(idx), _p(rev[0]), _p(rev[1]), int(rev[2]), _p(ddir), _p(dun), B, n, k, _p(out),
                                     int(accumulate), _stream(xyz)), "tgp_dirs_to_xyz")
    return out


def center_bwd(dxyz, dmean=None):
    """backward of center(): dxyz (B, n, 3), dmean (B, 3) or None -> d points (B, n, 3)"""
    _f32(dxyz, "dxyz", 3)
    dxyz = dxyz.contiguous()
    B, n, _ = dxyz.shape
    if dmean is not None:
        dmean = _f32(dmean, "dmean").reshape(B, 3).contiguous()
    out = torch.empty_like(dxyz)
    check(_lib.lib().tgp_center_bwd(_p(dxyz), _p(dmean), B, n, _p(out), _stream(dxyz)), "tgp_center_bwd")
    return out


def bn_apply(x, mean, var, gamma, beta, eps=1e-5, act=0, slope=0.0):
    """act((x - mean) / sqrt(var + eps) * gamma + beta) over rows with fixed statistics (eval-mode BatchNorm on the running ones)"""
    x, ld = _rows(x, "x")
    C = x.shape[-1]
    rows = math.prod(x.shape[:-1])
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    check(_lib.lib().tgp_bn_apply(_p(x), ld, rows, C, _p(mean), _p(var), _p(gamma), _p(beta), float(eps), act, float(slope), None,
                                  _p(out), C, None, 0, 0, 0, _stream(x)), "tgp_bn_apply")
    return out


def bn_eval_bwd(dy, x, mean, var, gamma, beta, eps=1e-5, act=0, slope=0.0):
    """backward of bn_apply: -> (dx, dgamma, dbeta)"""
    dy, lddy = _rows(dy, "dy")
    x, ld = _rows(x, "x")
    rows, C = math.prod(x.shape[:-1]), x.shape[-1]
    dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws = _ws(_lib.lib().tgp_bn_eval_workspace_floats(C), x.device)
    check(_lib.lib().tgp_bn_eval_bwd(_p(dy), lddy, _p(x), ld, rows, C, _p(mean), _p(var), float(eps), _p(gamma), _p(beta), act, float(slope),
                                     _p(dx), C, _p(dg), _p(db), _p(ws), _stream(x)), "tgp_bn_eval_bwd")
    return dx, dg, db


def bn_eval_bwd_pooled(dpool, argrow, x, rows_per_obj, mean, var, gamma, beta, eps=1e-5, act=0, slope=0.0):
    """backward of colmax_arg(x, bn=(running mean, running var, gamma, beta)): -> (dense dx (objects * n, C), dgamma, dbeta)"""
    x, ld = _rows(x, "x")
    objects, C = dpool.shape
    dpool = dpool.contiguous()
    dx = torch.empty(objects * rows_per_obj, C, device=x.device, dtype=torch.float32)
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws = _ws(objects * C, x.device)
    check(_lib.lib().tgp_bn_eval_bwd_pooled(_p(dpool), dpool.stride(0), _p(argrow), argrow.stride(0), _p(x), ld, objects, rows_per_obj, C,
                                            _p(mean), _p(var), float(eps), _p(gamma), _p(beta), act, float(slope), _p(dx), C, _p(dg), _p(db),
                                            _p(ws), _stream(x)), "tgp_bn_eval_bwd_pooled")
    return dx, dg, db


# ------------------------------------------------------------------------------------- the training batch's draws on the device
def _keys(keys, name="keys"):
    """item keys: a contiguous (D,) int64 GPU tensor holding the 64-bit keys' bit patterns"""
    if not (torch.is_tensor(keys) and keys.is_cuda and keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()):
        raise TypeError("%s must be a contiguous (D,) int64 GPU tensor" % name)
    return keys


def _u64(seed):
    return int(seed) & (2 ** 64 - 1)


def draw_words(keys, seed, site, n_counters):
    """tgp_draw_words: the generator's words, (D, n_counters, 4) int32-viewed uint32"""
    D = _keys(keys).numel()
    out = torch.empty(D, int(n_counters), 4, device=keys.device, dtype=torch.int32)
    check(_lib.lib().tgp_draw_words(_p(keys), D, _u64(seed), int(site), int(n_counters), _p(out), _stream(keys)), "tgp_draw_words")
    return out


def draw_band_subset(band_counts, u, pro, keys, seed, validity=True, drop_words=2048):
    """tgp_draw_band_subset: defor_2D's draws from roi_band's (D,3) counts without reading them back; u (D,) float64 GPU
    -> (defor_on (D,) int32, drop_bits (D, drop_words) int32)"""
    _i32(band_counts, "band_counts")
    D = _keys(keys).numel()
    if band_counts.shape != (D, 3) or not (u.is_cuda and u.dtype == torch.float64 and u.shape == (D,) and u.is_contiguous()):
        raise ValueError("draw_band_subset: band_counts must be (D,3) int32 and u (D,) float64")
    on = torch.empty(D, device=keys.device, dtype=torch.int32)
    bits = torch.empty(D, int(drop_words), device=keys.device, dtype=torch.int32)
    check(_lib.lib().tgp_draw_band_subset(_p(band_counts), _p(u), float(pro), _p(keys), _u64(seed), D, 1 if validity else 0, _p(on), _p(bits),
                                          int(drop_words), _stream(keys)), "tgp_draw_band_subset")
    return on, bits


def draw_alive(counts, B, min_points, forced=None):
    """tgp_draw_alive: counts (D,3) int32 -> (status (D,), slot_item (B,), n_alive (1,)) int32, nothing read back"""
    _i32(counts, "counts")
    D = counts.shape[0]
    if counts.dim() != 2 or counts.shape[1] != 3 or (forced is not None and _i32(forced, "forced").shape != (D,)):
        raise ValueError("draw_alive: counts must be (D,3) and forced (D,)")
    dev = counts.device
    status, slot, n = (torch.empty(k, device=dev, dtype=torch.int32) for k in (D, int(B), 1))
    check(_lib.lib().tgp_draw_alive(_p(counts), _p(forced), D, int(B), int(min_points), _p(status), _p(slot), _p(n), _stream(counts)),
          "tgp_draw_alive")
    return status, slot, n


def draw_selection(totals, keys, seed, site, n_out, shuffle_always=False):
    """tgp_draw_selection -> (D, n_out) int32.  totals: an int (every item's total) or an int32 GPU tensor view whose element
    [d] (any constant stride along its one dimension, e.g. counts[:, 2]) is item d's total, read on the device"""
    D = _keys(keys).numel()
    sel = torch.empty(D, int(n_out), device=keys.device, dtype=torch.int32)
    if torch.is_tensor(totals):
        if not (totals.is_cuda and totals.dtype == torch.int32 and totals.dim() == 1 and totals.numel() == D):
            raise ValueError("draw_selection: totals must be a (D,) int32 GPU view")
        ptr, ld, const = _p(totals), max(int(totals.stride(0)), 1), 0
    else:
        ptr, ld, const = None, 0, int(totals)
    check(_lib.lib().tgp_draw_selection(ptr, ld, const, _p(keys), _u64(seed), int(site), D, int(n_out), 1 if shuffle_always else 0, _p(sel),
                                        _stream(keys)), "tgp_draw_selection")
    return sel


def draw_fill(keys, seed, N, defor=False, noise=None, drop_u=False):
    """tgp_draw_fill: the per-point draws.  defor: (D,N,3) float32 uniforms; noise = (std, clip): (D,N,3) float32 clamped normals;
    drop_u: (D,N) float64 uniforms -> dict of the buffers asked for"""
    D = _keys(keys).numel()
    dev = keys.device
    out = {}
    if defor:
        out["defor"] = torch.empty(D, N, 3, device=dev)
    if noise is not None:
        out["noise"] = torch.empty(D, N, 3, device=dev)
    if drop_u:
        out["drop_u"] = torch.empty(D, N, device=dev, dtype=torch.float64)
    std, clip = (float(v) for v in noise) if noise is not None else (0.0, 0.0)
    check(_lib.lib().tgp_draw_fill(_p(keys), _u64(seed), D, int(N), _p(out.get("defor")), _p(out.get("noise")), std, clip, _p(out.get("drop_u")),
                                   _stream(keys)), "tgp_draw_fill")
    return out


def gather_slots(slot_item, tensors):
    """tgp_gather_slots: for each contiguous GPU tensor (D, ...) of a 4- or 8-byte type, the (B, ...) tensor of its rows slot_item[s]
    (zeros where slot_item is -1); one launch per _lib.GATHER_SLOTS_MAX tensors"""
    _i32(slot_item, "slot_item")
    B = slot_item.numel()
    tensors = list(tensors)
    D = tensors[0].shape[0]
    outs = []
    for t in tensors:
        if not (t.is_cuda and t.is_contiguous() and t.shape[0] == D and t.element_size() in (4, 8) and t.numel() > 0):
            raise ValueError("gather_slots: contiguous (D, ...) GPU tensors of 4- or 8-byte elements")
        outs.append(torch.empty((B,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype))
    for i0 in range(0, len(tensors), _lib.GATHER_SLOTS_MAX):
        a = _lib.GatherSlotsArgs()
        part = list(zip(tensors, outs))[i0:i0 + _lib.GATHER_SLOTS_MAX]
        a.slot_item, a.B, a.D, a.n = _p(slot_item).value, B, D, len(part)
        for k, (t, o) in enumerate(part):
            a.src[k], a.dst[k], a.row_words[k] = t.data_ptr(), o.data_ptr(), t[0].numel() * t.element_size() // 4
        check(_lib.lib().tgp_gather_slots(ctypes.byref(a), _stream(slot_item)), "tgp_gather_slots")
    return outs
