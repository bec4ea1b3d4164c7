"""NumPy restatement of tgp_segment_depth (include/tgpose.h, DESIGN.md section 3 "Segments of a depth frame"): a flood fill in scan
order -- the first pixel of a component the scan meets is its smallest flat index, its root -- then the ranking, the integer moments
(Python ints, no rounding anywhere) and the centroids in float64 rounded once."""
import numpy as np

MAX_SEGMENTS, STAT_COLS = 255, 12
N4 = ((0, 1), (1, 0), (0, -1), (-1, 0))
N8 = N4 + ((1, 1), (1, -1), (-1, 1), (-1, -1))


def components(depth, max_step, connectivity):
    """-> (H,W) int64: the root (smallest flat index) of every valid pixel's component, -1 for an invalid pixel"""
    assert connectivity in (4, 8) and 0 <= max_step <= 65535
    H, W = depth.shape
    z = depth.astype(np.int64)
    root = np.full((H, W), -1, np.int64)
    offs = N8 if connectivity == 8 else N4
    for p in np.nonzero(z.reshape(-1) > 0)[0].tolist():
        y0, x0 = divmod(p, W)
        if root[y0, x0] >= 0:
            continue
        root[y0, x0] = p
        stack = [(y0, x0)]
        while stack:
            y, x = stack.pop()
            zp = z[y, x]
            for dy, dx in offs:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and root[v, u] < 0 and z[v, u] > 0 and abs(zp - z[v, u]) <= max_step:
                    root[v, u] = p
                    stack.append((v, u))
    return root


def segment(depth, max_step=10, connectivity=4, min_pixels=50, max_segments=32, camk=None, root=None):
    """depth (H,W) uint16 -> dict(labels (H,W) uint8, info (4,) int32, stats (max_segments,12) int64, centers (max_segments,3) float32
    or None); root: components(depth, max_step, connectivity) when the caller has it already"""
    assert min_pixels >= 1 and 1 <= max_segments <= MAX_SEGMENTS
    H, W = depth.shape
    root = components(depth, max_step, connectivity) if root is None else root
    flat = root.reshape(-1)
    roots, counts = np.unique(flat[flat >= 0], return_counts=True)                 # ascending roots
    qualified = roots[counts >= min_pixels]
    kept = qualified[:max_segments]
    labels = np.zeros(H * W, np.uint8)
    stats = np.zeros((max_segments, STAT_COLS), np.int64)
    centers = None if camk is None else np.full((max_segments, 3), np.nan, np.float32)
    zs = depth.reshape(-1)
    for r, rt in enumerate(kept.tolist()):
        pix = np.nonzero(flat == rt)[0]
        labels[pix] = r + 1
        ys, xs, z = [int(v) for v in pix // W], [int(v) for v in pix % W], [int(v) for v in zs[pix]]
        n, sx, sy, sz = len(pix), sum(xs), sum(ys), sum(z)
        sxz, syz = sum(a * b for a, b in zip(xs, z)), sum(a * b for a, b in zip(ys, z))
        stats[r] = [n, min(ys), min(xs), max(ys) + 1, max(xs) + 1, rt, sx, sy, sz, sxz, syz, min(z)]
        if camk is not None:
            fx, fy, cx, cy = (np.float64(np.float32(v)) for v in camk)
            n64, sz64 = np.float64(n), np.float64(sz)
            centers[r] = [np.float32((np.float64(sxz) - cx * sz64) / (fx * n64) / 1000.0),
                          np.float32((np.float64(syz) - cy * sz64) / (fy * n64) / 1000.0), np.float32(sz64 / n64 / 1000.0)]
    info = np.array([len(qualified) > max_segments, len(kept), len(qualified), int((zs > 0).sum())], np.int32)
    return dict(labels=labels.reshape(H, W), info=info, stats=stats, centers=centers)


def edges(depth, max_step, connectivity):
    """the joined pairs as flat indices (k,2), each once: the relation itself, for an independent labelling"""
    H, W = depth.shape
    z = depth.astype(np.int64)
    idx = np.arange(H * W).reshape(H, W)
    out = []
    for dy, dx in ((0, 1), (1, 0)) + (((1, 1), (1, -1)) if connectivity == 8 else ()):
        a = (slice(0, H - dy), slice(max(0, -dx), W - max(0, dx)))
        b = (slice(dy, H), slice(max(0, dx), W + min(0, dx)))
        ok = (z[a] > 0) & (z[b] > 0) & (np.abs(z[a] - z[b]) <= max_step)
        out.append(np.stack([idx[a][ok], idx[b][ok]], 1))
    return np.concatenate(out)


def by_size(stats):
    """rows by descending pixel count, equal counts by ascending row"""
    return np.argsort(-stats[:, 0], kind="stable")
