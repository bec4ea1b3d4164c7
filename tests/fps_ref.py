"""numpy restatement of the farthest point sampling contract (DESIGN.md section 3 "Farthest point sampling"; the reference's
core/utils/farthest_points_torch.py:6-62 with dist_func = F.pairwise_distance) in fp32, the fused multiply-adds computed through
float64 and rounded once.

    e = fl(fl(c - p) + 1e-6f),  d = sqrt_rn(fma(e.z, e.z, fma(e.y, e.y, fl(e.x * e.x))))
    step i: centre = lowest index of max(running); new = d(centre, .); where new <= running: running = new, cluster = i

tests/golden/fps_ref.npz holds what the reference itself returned (tests/golden/make_fps_golden.py); tests/test_fps_cpu.py compares."""
import numpy as np

F32 = np.float32
EPS = F32(1e-6)


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding: the product of two fp32 is exact in float64; the float64 sum is brought to round-to-odd
    (TwoSum gives its error), after which rounding 53 -> 24 bits is the correct rounding of the exact value"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)
    even = (t.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(t)
    toward = np.where(err > 0, np.inf, -np.inf)
    t = np.where(fix, np.nextafter(t, toward), t)
    return t.astype(F32)


def dist(c, pts):
    """F.pairwise_distance(c broadcast, pts): (M,) float32"""
    pts = np.asarray(pts, dtype=F32)
    e = (np.asarray(c, dtype=F32)[None, :] - pts) + EPS
    s = e[:, 0] * e[:, 0]
    s = fma32(e[:, 1], e[:, 1], s)
    s = fma32(e[:, 2], e[:, 2], s)
    return np.sqrt(s)


def centroid(pts):
    """the kernel's centroid: pairwise-tree fp32 sum over the row index (zeros beyond the count), divided by (float)count"""
    pts = np.asarray(pts, dtype=F32)
    cnt = len(pts)
    size = 1
    while size < cnt:
        size *= 2
    a = np.zeros((size, 3), F32)
    a[:cnt] = pts
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0] / F32(cnt)


def fps(pts, n, start=None, init_center=True):
    """one cloud (its live rows) -> idx (n,) int32, running distances (M,) float32, clusters (M,) int32.  len(pts) <= n: the
    tiling rule, no step runs (the initial distances, clusters -1)."""
    pts = np.ascontiguousarray(pts, dtype=F32)[:, :3]
    M = len(pts)
    if init_center:
        d = dist(centroid(pts) if start is None else start, pts)
    else:
        d = np.full(M, 1e7, F32)
    clusters = np.full(M, -1, np.int32)
    if M <= n:
        return (np.arange(n) % M).astype(np.int32), d, clusters
    idx = np.zeros(n, np.int32)
    for i in range(n):
        c = int(np.argmax(d))                    # the first of the maxima
        idx[i] = c
        new = dist(pts[c], pts)
        upd = new <= d
        d = np.where(upd, new, d)
        clusters[upd] = i
    return idx, d, clusters


def fps_batch(xyz, n, counts=None, start=None, init_center=True):
    """xyz (B,M,>=3) -> idx (B,n) int32, dist (B,M) float32 (NaN at and beyond the count), clusters (B,M) int32 (-1 there)"""
    xyz = np.asarray(xyz, dtype=F32)
    B, M = xyz.shape[:2]
    idx = np.zeros((B, n), np.int32)
    d = np.full((B, M), np.nan, F32)
    cl = np.full((B, M), -1, np.int32)
    for b in range(B):
        c = M if counts is None else int(counts[b])
        idx[b], d[b, :c], cl[b, :c] = fps(xyz[b, :c], n, None if start is None else start[b], init_center)
    return idx, d, cl


def thin_indices(total, pool):
    """clouds_from_frames(sampler='fps') candidates: the whole cloud up to ``pool`` records, else the evenly spaced
    floor(i * total / pool), i < pool"""
    if total <= pool:
        return np.arange(total, dtype=np.int64)
    return (np.arange(pool, dtype=np.int64) * int(total)) // int(pool)


def coverage_radius(pts, sel):
    """max over the cloud of the distance to the nearest selected point (float64)"""
    pts = np.asarray(pts, dtype=np.float64)
    s = pts[np.asarray(sel)]
    best = np.full(len(pts), np.inf)
    for lo in range(0, len(s), 256):
        best = np.minimum(best, np.sqrt(((pts[:, None] - s[None, lo:lo + 256]) ** 2).sum(-1)).min(1))
    return float(best.max())
