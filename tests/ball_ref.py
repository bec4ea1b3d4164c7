"""The ball crop's contract (include/tgpose.h "Ball crop", DESIGN.md section 3 "Ball crop and tracking") restated in NumPy.  The
kernels of csrc/ballcrop.hip must agree with these functions bit for bit; tests/test_ball_crop_cpu.py checks the functions
themselves against what the reference's crop_ball_from_pts / crop_ball_from_depth_image returned (tests/golden/ball_crop_ref.npz).

Everything is float32, every operation rounded on its own; NumPy's float32 division and square root are correctly rounded."""
import numpy as np

LEVELS, THREADS = 10, 1024
F = np.float32


def pixel_points(xs, ys, dep, camk):
    """the point of source pixel (xs, ys) with depth dep (millimetres): _depth_to_pcl then / 1000, as the ROI path computes it"""
    fx, fy, cx, cy = (F(v) for v in camk)
    dep = np.asarray(dep).astype(F)
    px = ((np.asarray(xs).astype(F) - cx) * dep / fx) / F(1000.0)
    py = ((np.asarray(ys).astype(F) - cy) * dep / fy) / F(1000.0)
    return np.stack([px, py, dep / F(1000.0)], -1).astype(F)


def distances(pts, center):
    """sqrt((dx^2 + dy^2) + dz^2): the order of torch's CPU sum(-1) over three elements"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(pts, F) - np.asarray(center, F)[None, :]
        sq = d * d
        return np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])


def ladder_of(radius):
    """ops.ball_ladder's rule for one radius given as a float32"""
    r = F(radius)
    if r < F(0.05):
        out, s = [], 0.05
        for _ in range(LEVELS):
            out.append(F(s))
            s *= 1.10
        return np.asarray(out, F)
    out = []
    for _ in range(LEVELS):
        out.append(r)
        r = F(r * F(1.10))
    return np.asarray(out, F)


def crop_levels(d, ladder, n_valid):
    """d: the distances of the valid elements in row-major order -> (kept positions, counts[1:4] = count, L, status)"""
    with np.errstate(invalid="ignore"):
        lad = np.fmax.accumulate(np.asarray(ladder, F))         # d <= lad[i]  <=>  the smallest i with d <= ladder[i] is <= i
        cum = [int((d <= lad[i]).sum()) for i in range(LEVELS)]
        L = next((i for i in range(LEVELS) if cum[i] >= 10), LEVELS - 1)
        keep = np.nonzero(d <= lad[L])[0]
    assert len(keep) == cum[L]
    return keep, (cum[L], L, 2 if n_valid == 0 else 1 if cum[L] == 0 else 0)


def valid_pixels(depth, mask=None, mask_val=0):
    """row-major indices of the pixels with depth > 0 that the mask (H,W) admits: any non-zero byte, or the byte mask_val > 0"""
    ok = depth.reshape(-1) > 0
    if mask is not None:
        m = np.asarray(mask).reshape(-1).astype(np.int64)
        ok &= (m == mask_val) if mask_val else (m != 0)
    return np.nonzero(ok)[0]


def ball_cloud(depth, camk, center, ladder, mask=None, mask_val=0, cap=None):
    """one job on one frame depth (H,W) uint16 -> (recs: the first min(count, cap) pixel indices, counts (4,) int32)"""
    H, W = depth.shape
    cap = H * W if cap is None else cap
    pix = valid_pixels(depth, mask, mask_val)
    pts = pixel_points(pix % W, pix // W, depth.reshape(-1)[pix], camk)
    keep, (count, L, status) = crop_levels(distances(pts, center), ladder, len(pix))
    return pix[keep][:cap].astype(np.uint32), np.asarray([len(pix), count, L, status], np.int32)


def ball_cloud_pts(pts, center, ladder, cap=None):
    """one job on a point list (N,3) float32: every point is valid, a record is the point's index"""
    cap = len(pts) if cap is None else cap
    keep, (count, L, status) = crop_levels(distances(pts, center), ladder, len(pts))
    return keep[:cap].astype(np.uint32), np.asarray([len(pts), count, L, status], np.int32)


def doubled_len(n, n_pts):
    """the length of the reference's index list after `while len(idx) < num_points: idx = cat([idx, idx])`"""
    while n < n_pts:
        n *= 2
    return n


def ball_select(recs, count, cap, sel, points_of):
    """sel indexes the doubled list of the first n = min(count, cap) records; points_of(pixel indices) -> (k,3) float32.
    -> (out (n_pts,3) float32, pix (n_pts,) int32); an index outside the list: NaN, -1"""
    n, n_pts = min(int(count), cap), len(sel)
    out, pix = np.full((n_pts, 3), np.nan, F), np.full(n_pts, -1, np.int32)
    if n > 0:
        sel = np.asarray(sel, np.int64)
        ok = (sel >= 0) & (sel < doubled_len(n, n_pts))
        src = recs[sel[ok] % n].astype(np.int64)
        out[ok], pix[ok] = points_of(src), src
    return out, pix


def depth_points_of(depth, camk):
    W = depth.shape[1]
    return lambda p: pixel_points(p % W, p // W, depth.reshape(-1)[p], camk)


def _mix32(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _feistel(v, half_bits, key):
    mask = (1 << half_bits) - 1
    l, r = v >> half_bits, v & mask
    for rnd in range(4):
        f = _mix32(r ^ ((key + 0x9e3779b9 * (rnd + 1)) & 0xffffffff)) & mask
        l, r = r, l ^ f
    return (l << half_bits) | r


def sample_selection(n, n_pts, seed, j):
    """tgp_ball_sample's draw for job j: the first n_pts elements of the keyed permutation of the doubled list's length"""
    dlen = doubled_len(n, n_pts)
    half_bits = 1
    while (1 << (2 * half_bits)) < dlen:
        half_bits += 1
    key = _mix32((seed & 0xffffffff) ^ _mix32(((seed >> 32) + 0x632be5ab * (j + 1)) & 0xffffffff))
    out = []
    for i in range(n_pts):
        e = _feistel(i, half_bits, key)
        while e >= dlen:
            e = _feistel(e, half_bits, key)
        out.append(e)
    return np.asarray(out, np.int32)


def rect(center, radius, camk, H, W):
    """the pixel rectangle (x0, x1, y0, y1), half open, inside which the kernel evaluates distances for a ball of the given last
    radius; the whole frame when the formula cannot bound it (csrc/ballcrop.hip ball_rect, in double as there; before the columns
    are widened to whole 16-byte load groups)"""
    fx, fy, pcx, pcy = (float(F(v)) for v in camk)
    c0, c1, c2 = (float(F(v)) for v in center)
    R = float(F(radius))
    Rm = R * 1.001 + 1e-5
    z0, z1 = c2 - Rm, c2 + Rm
    if not (R >= 0 and np.isfinite([Rm, c0, c1, c2, fx, fy, pcx, pcy]).all() and z0 > 1e-6):
        return 0, W, 0, H

    def span(c, f, pc, n):
        a, b = c - Rm, c + Rm
        q = [a / z0, a / z1, b / z0, b / z1]
        u0, u1 = pc + f * min(q), pc + f * max(q)
        ulo, uhi = np.floor(min(u0, u1) - 1.0), np.ceil(max(u0, u1) + 1.0)
        lo = int(min(max(ulo, 0.0), float(n)))
        hi = int(min(max(uhi + 1.0, 0.0), float(n)))
        return lo, max(hi, lo)
    return span(c0, fx, pcx, W) + span(c1, fy, pcy, H)
