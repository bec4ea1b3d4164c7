"""numpy restatement of the EMD contract (DESIGN.md "EMD"; the auction of losses/metrics/EMD/emd_cuda.cu:95-226) in fp32 with
its one double step: the oracle the HIP kernel is compared with bit for bit.

Nothing of the reference's EMD can run here -- it is a CUDA extension, and its own shape rule (n % 1024 == 0) refuses most of the
shapes tested -- so this file is a restatement, not a recording.  It is in turn pinned to ground truth by what the auction
algorithm guarantees (tests/test_emd_cpu.py: against exact matching).

``winner="highest"`` replaces the contract's lowest-bidder rule by the other extreme of the reference's write race
(tests/test_emd_cpu.py shows that the two pick among equivalent outcomes)."""
import numpy as np

NONE = np.float32(-1e9)


def _bids(x1, x2, price, eps, block):
    """best object (first k at the maximum), increment (best - better) + eps for every row of x1"""
    n = len(x2)
    bid, inc = np.empty(len(x1), np.int64), np.empty(len(x1), np.float32)
    for o in range(0, len(x1), block):
        q = x1[o:o + block]
        dx, dy, dz = (x2[None, :, c] - q[:, None, c] for c in range(3))
        s = (dx * dx + dy * dy) + dz * dz                                          # fp32, each operation rounded
        d = (3.0 - np.sqrt(s).astype(np.float64) - price.astype(np.float64)[None, :]).astype(np.float32)
        k = np.argmax(d, axis=1)                                                   # first occurrence of the maximum
        rows = np.arange(len(q))
        best = d[rows, k]
        if n > 1:
            d[rows, k] = -np.inf
            better = d.max(axis=1)                                                 # second largest, duplicates counted
        else:
            better = np.full(len(q), NONE)
        bid[o:o + block], inc[o:o + block] = k, (best - better).astype(np.float32) + np.float32(eps)
    return bid, inc


def emd_pair(x1, x2, eps, iters, winner="lowest", block=512):
    """x1, x2 (n,3) float32 -> dist (n,) float32, assignment (n,) int32, info {'converged_at': first iteration that found nothing
    unassigned, or None}"""
    x1, x2 = np.ascontiguousarray(x1, np.float32), np.ascontiguousarray(x2, np.float32)
    n = len(x1)
    assert x2.shape == x1.shape == (n, 3) and iters >= 1
    assign, ainv = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    price, maxinc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    converged = None
    for it in range(iters):
        un = np.flatnonzero(assign == -1)                                          # ascending j
        if len(un) == 0:
            converged = it
            break
        bid, inc = _bids(x1[un], x2, price, eps, block)
        np.maximum.at(maxinc, bid, inc)
        if it == iters - 1:
            assign[un] = bid
            break
        m, i64 = maxinc[bid].astype(np.float64), inc.astype(np.float64)
        ok = (i64 - 1e-6 <= m) & (m <= i64 + 1e-6)
        cand_j, cand_k, cand_inc = un[ok], bid[ok], inc[ok]
        if winner == "highest":
            cand_j, cand_k, cand_inc = cand_j[::-1], cand_k[::-1], cand_inc[::-1]
        ks, first = np.unique(cand_k, return_index=True)                           # first = the lowest (highest) j per object
        js, incs = cand_j[first], cand_inc[first]
        old = ainv[ks]
        assign[old[old != -1]] = -1
        ainv[ks], assign[js] = js, ks
        price[ks] = price[ks] + incs
        maxinc[ks] = NONE
    a = assign
    d = x1 - x2[a]
    dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return dist.astype(np.float32), a.astype(np.int32), {"converged_at": converged}


def emd(xyz1, xyz2, eps, iters, **kw):
    """(B,n,3) batches -> dist (B,n) float32, assignment (B,n) int32"""
    out = [emd_pair(a, b, eps, iters, **kw)[:2] for a, b in zip(np.asarray(xyz1), np.asarray(xyz2))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def emd_grad(xyz1, xyz2, grad_dist, assignment):
    """the backward's closed form in fp32: (grad_dist * 2) * (xyz1 - xyz2[assignment])"""
    xyz1, xyz2 = np.asarray(xyz1, np.float32), np.asarray(xyz2, np.float32)
    g = (np.asarray(grad_dist, np.float32) * np.float32(2))[..., None]
    return g * (xyz1 - np.take_along_axis(xyz2, np.asarray(assignment, np.int64)[..., None], axis=1))


def lattice(shift=0.25):
    """Two copies of a 4^3 grid against two copies of the grid shifted by `shift` cells: n = 128, every distance occurs many times
    (exact ties in d and in the increments; all coordinates are multiples of 1/16, exact in fp32)."""
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) / 4
    a = np.concatenate([g, g])
    b = np.concatenate([g, g]) + np.float32(shift / 4)
    return a, b.astype(np.float32)
