"""NumPy restatement of dense projective ICP (include/tgpose.h tgp_icp_dense; DESIGN.md section 3 "Dense projective registration"),
written from that text.  One job per call.  float32 exactly where the contract says float32 -- the source point, the model-frame
point q, the projection into the map's window, the gate -- float64 everywhere else.  The sums over the inliers and the solve are
NumPy's (pairwise sums, LAPACK's triangular solves): the kernel's summation order differs, which is what the tests' 1e-6 allows for.
to_model_frame, solve_plane and rodrigues are tests/icp_ref.py's, the maps tests/raycast_ref.py's; nothing of them is restated here.

    refine(depth (H,W) uint16, camk (4,), maps = dict z (h,w), vertex, normal (h,w,3), window (4,), ref (3,4), rect (4,), R, t, s,
           max_dist, stride=1, mask=None, mask_val=None, iters=30, tol_rot=1e-5, tol_trans=1e-6, min_inliers=6)
        -> dict R, t, s float32 (the float64 state rounded once), R64 / t64, status, inliers, iters, candidates, rmse, corr (npix,)
    rects(window (J,4), h, w, H, W) -> (J,4) int32: ops.dense_rects
"""
import numpy as np

from tests import ball_ref, icp_ref

f32 = np.float32


def grid(rect, stride, H, W):
    """the job's source pixels: (x0 + i stride, y0 + k stride), i, k >= 0, inside the rectangle clipped to the frame -> (xs, ys),
    row-major, flat"""
    x0, y0, x1, y1 = (int(v) for v in rect)
    cols = [x for x in range(x0 + (max(-x0, 0) + stride - 1) // stride * stride, min(x1, W - 1) + 1, stride)]
    rows = [y for y in range(y0 + (max(-y0, 0) + stride - 1) // stride * stride, min(y1, H - 1) + 1, stride)]
    if not cols or not rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    yy, xx = np.meshgrid(np.array(rows, np.int64), np.array(cols, np.int64), indexing="ij")
    return xx.ravel(), yy.ravel()


def associate(p, live, camk, maps, window, ref, R, t, s, gate):
    """one association pass at the pose (R, t, s): -> (q (n,3) float32, cell (n,) int64 (-1 unless associated), inlier (n,) bool)"""
    h, w = maps["z"].shape
    K, T, win = np.asarray(camk, f32), np.asarray(ref, f32).reshape(3, 4), np.asarray(window, f32)
    with np.errstate(all="ignore"):
        q = icp_ref.to_model_frame(p, R, t, s)
        c = [((T[r, 0] * q[:, 0] + T[r, 1] * q[:, 1]) + T[r, 2] * q[:, 2]) + T[r, 3] for r in range(3)]
        front = c[2] > f32(1e-6)
        u = K[0] * (c[0] / c[2]) + K[2]
        v = K[1] * (c[1] / c[2]) + K[3]
        col, row = np.rint((u - win[0]) / win[2]), np.rint((v - win[1]) / win[3])
        inside = live & front & (col >= 0) & (col <= f32(w - 1)) & (row >= 0) & (row <= f32(h - 1))
        cell = np.where(inside, row.astype(np.float64) * w + col.astype(np.float64), 0).astype(np.int64)
        assoc = inside & (maps["z"].reshape(-1)[cell] > 0)
        y = maps["vertex"].reshape(-1, 3)[cell].astype(f32)
        e = q - y
        dist = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        g = np.float64(gate) / np.float64(s)                       # icp_ref.refine's threshold; NumPy's float64 so that s = 0 divides
        thr = f32(g * g)
        inlier = assoc & (dist <= thr)
    return q, np.where(assoc, cell, -1), inlier


def refine(depth, camk, maps, window, ref, rect, R, t, s, max_dist, stride=1, mask=None, mask_val=None, iters=30, tol_rot=1e-5,
           tol_trans=1e-6, min_inliers=6):
    depth = np.asarray(depth, dtype=np.uint16)
    H, W = depth.shape
    assert stride >= 1 and iters >= 1
    xs, ys = grid(rect, stride, H, W)
    d = depth[ys, xs]
    live = d != 0
    if mask is not None:
        live &= np.asarray(mask)[ys, xs] == mask_val
    p = ball_ref.pixel_points(xs, ys, d, camk)
    y64 = maps["vertex"].reshape(-1, 3).astype(np.float64)
    n64 = maps["normal"].reshape(-1, 3).astype(np.float64)
    R0 = np.asarray(R, dtype=f32).astype(np.float64).reshape(3, 3)
    t0 = np.asarray(t, dtype=f32).astype(np.float64).reshape(3)
    R, t = R0, t0
    s = float(f32(s))
    gate = float(f32(max_dist))
    tol_rot, tol_trans = float(f32(tol_rot)), float(f32(tol_trans))
    min_inliers = max(int(min_inliers), 6)
    never_stop = not (tol_rot > 0) and not (tol_trans > 0)
    status, done, candidates = 0, 0, None
    for it in range(iters):
        q, cell, inl = associate(p, live, camk, maps, window, ref, R, t, s, gate)
        if candidates is None:
            candidates = int((cell >= 0).sum())
        if inl.sum() < min_inliers:
            status = 1
            break
        with np.errstate(all="ignore"):                            # an infinite row makes NaN sums: status 2, by the rule
            st, Rn, tn, ang, tr = icp_ref.solve_plane(q[inl].astype(np.float64), y64[cell[inl]], n64[cell[inl]], R, t, s)
        if st:
            status = st
            break
        R, t = Rn, tn
        done = it + 1
        if not never_stop and ang <= tol_rot and tr <= tol_trans:
            break
    if status:
        R, t = R0, t0                                              # a failed job goes back to the pose it came with
    q, cell, inl = associate(p, live, camk, maps, window, ref, R, t, s, gate)
    k = int(inl.sum())
    e = q[inl].astype(np.float64) - y64[cell[inl]]
    with np.errstate(all="ignore"):
        rmse = f32(s * np.sqrt(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).sum() / k)) if k else f32(np.nan)
    return dict(R=R.astype(f32), t=t.astype(f32), s=f32(s), R64=R, t64=t, status=status, inliers=k, iters=done, candidates=candidates,
                rmse=rmse, corr=np.where(inl, cell, -1).astype(np.int32))


def rects(window, h, w, H, W):
    """ops.dense_rects: the pixels a window's h x w ray grid covers, (x0, y0, x1, y1) inclusive int32: floor of the smaller and ceil
    of the larger of each axis' two ends (u0 and u0 + (float)(w - 1) du in float32), clamped to the frame; a window with a NaN in an
    end gives the empty rectangle (0, 0, -1, -1)"""
    win = np.asarray(window, dtype=f32).reshape(-1, 4)
    out = np.zeros((len(win), 4), np.int32)
    with np.errstate(all="ignore"):
        ua, va = win[:, 0], win[:, 1]
        ub, vb = ua + f32(w - 1) * win[:, 2], va + f32(h - 1) * win[:, 3]
        bad = np.isnan(ua) | np.isnan(ub) | np.isnan(va) | np.isnan(vb)
        lo = lambda a, b, top: np.clip(np.floor(np.fmin(a, b)), f32(0), f32(top))
        hi = lambda a, b, top: np.clip(np.ceil(np.fmax(a, b)), f32(0), f32(top))
        box = np.stack([lo(ua, ub, W - 1), lo(va, vb, H - 1), hi(ua, ub, W - 1), hi(va, vb, H - 1)], 1)
    out[:] = np.where(bad[:, None], f32(0), box).astype(np.int32)
    out[bad] = (0, 0, -1, -1)
    return out
