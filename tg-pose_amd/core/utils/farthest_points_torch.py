"""Drop-in for ``core/utils/farthest_points_torch.py``: farthest point sampling of one cloud, on the device.

``farthest_points(data, n_clusters, ...)`` and ``get_fps_and_center_torch(points, num_fps, ...)`` keep the reference's signatures and
return order (``clusters, centers[, distances]``).  All ``n_clusters`` steps run inside ONE launch (``csrc/fps.hip``, ``tgp_fps``: the
cloud and its running distances stay in registers) with the reference's arithmetic bit for bit (DESIGN.md section 3 "Farthest point
sampling"): ``F.pairwise_distance``'s ``||c - p + 1e-6||``, the lowest index among equal maxima, ``clusters[distances == new] = i``.

What is accepted: ``data`` a float32 GPU tensor (M, 3), M <= ``ops.fps_max_points()``, and the default ``dist_func``
(``F.pairwise_distance``); anything else raises ValueError -- there is no slow path.  Differences from the reference, both stated
here: with ``init_center=True`` the virtual first centre is the kernel's centroid (a pairwise-tree fp32 sum, bit-repeatable) rather
than ``torch.mean``'s unspecified summation order -- on every cloud compared the centres are the same (tests/golden/fps_ref.npz);
and the results live on ``data``'s device (the reference builds them on the CPU whatever the input's device)."""
import torch
from torch.nn import functional as F

from ... import ops


def _check(data, dist_func):
    if dist_func is not F.pairwise_distance:
        raise ValueError("farthest_points: only dist_func=F.pairwise_distance is implemented on the device")
    if not (torch.is_tensor(data) and data.is_cuda and data.dtype == torch.float32 and data.dim() == 2 and data.shape[1] == 3):
        raise ValueError("farthest_points: data must be a float32 GPU tensor of shape (M, 3)")


def farthest_points(data, n_clusters: int, dist_func=F.pairwise_distance, return_center_indexes=True, return_distances=False,
                    verbose=False, init_center=True):
    """Returns clusters, [centers, distances] as the reference: clusters (M,) long, the last step at which a new centre came at
    least as close to the point as every centre before (-1: none); centers (n_clusters,) long in selection order; distances (M,)
    float32 to the nearest centre (the virtual first centre included)."""
    _check(data, dist_func)
    if verbose:
        raise ValueError("farthest_points: verbose=True (a print per step) has no device counterpart")
    M, dev = data.shape[0], data.device
    if n_clusters >= M:
        if return_center_indexes:
            return torch.arange(M, dtype=torch.long, device=dev), torch.arange(M, dtype=torch.long, device=dev)
        return torch.arange(M, dtype=torch.long, device=dev)
    if n_clusters < 1:
        raise ValueError("farthest_points: n_clusters must be at least 1")
    if M > ops.fps_max_points():
        raise ValueError("farthest_points: %d points are above the kernel's cap of %d; thin the cloud first" % (M, ops.fps_max_points()))
    idx, dist, clusters = ops.farthest_points(data.contiguous()[None], n_clusters, init_center=bool(init_center), return_distances=True,
                                              return_clusters=True)
    clusters, centers = clusters[0].long(), idx[0].long()
    if return_center_indexes:
        if return_distances:
            return clusters, centers, dist[0]
        return clusters, centers
    return clusters


def get_fps_and_center_torch(points, num_fps: int, init_center=True, dist_func=F.pairwise_distance):
    """-> (num_fps + 1, 3): the sampled points in selection order, then torch.mean(points, 0)"""
    _check(points, dist_func)
    center = torch.mean(points, 0, keepdim=True)
    _, fps_inds = farthest_points(points, n_clusters=num_fps, dist_func=dist_func, return_center_indexes=True, init_center=init_center)
    return torch.cat([points[fps_inds], center], dim=0)
