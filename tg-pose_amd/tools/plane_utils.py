"""The reference's ``tools/plane_utils.py`` on the device: the weighted regression z = a x + b y + c of point clouds and the three
quantities it derives, with the reference's function names, signatures and return tuples.

The reference builds an n x n ``diag(W)`` per cloud and multiplies through it; here one launch (ops.plane_lsq, csrc/plane.hip) takes
the nine weighted sums of every cloud in float64 and solves the 3 x 3 system in float64.  Inputs are brought to float32 on their
(GPU) device; outputs are float32 cast back to the input's dtype.  A singular system (fewer than three points, collinear points)
gives NaN where the reference's ``torch.inverse`` raises on the CPU or returns meaningless numbers; nothing is raised here.
"""
import torch

from .. import ops


def _run(pc, pc_w, eps):
    lead = pc.shape[:-2]
    n = pc.shape[-2]
    if pc.shape[-1] != 3 or tuple(pc_w.shape) != tuple(lead) + (n,):
        raise ValueError("plane_utils: pc (..., n, 3) and pc_w (..., n) are needed")
    p = pc.reshape(-1, n, 3).float().contiguous()
    w = pc_w.reshape(-1, n).float().contiguous()
    return [x.to(pc.dtype) for x in ops.plane_lsq(p, w, eps)], lead


def get_plane(pc, pc_w):
    """pc (n,3), pc_w (n,) -> (normal_n (3,), dn (3,), for_p2plane (1,))"""
    (X, normal, dn, p2), _ = _run(pc, pc_w, 0.0)
    return normal[0], dn[0], p2


def get_plane_in_batch(pc, pc_w):
    """pc (..., n, 3), pc_w (..., n) -> (normal_n (..., 3), dn (..., 3), for_p2plane (..., 1)); dn divides by dn_norm + 1e-8"""
    (X, normal, dn, p2), lead = _run(pc, pc_w, 1e-8)
    return normal.reshape(lead + (3,)), dn.reshape(lead + (3,)), p2.reshape(lead + (1,))


def get_plane_parameter(pc, pc_w):
    """pc (n,3), pc_w (n,) -> X (3,1): a, b, c"""
    (X, normal, dn, p2), _ = _run(pc, pc_w, 0.0)
    return X[0].reshape(3, 1)
