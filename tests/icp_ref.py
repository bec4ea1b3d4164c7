"""numpy restatement of the ICP contract (include/tgpose.h tgp_icp_refine; DESIGN.md section 3 "ICP refinement and model-based
tracking"), written from that text.  One job per call.  float32 exactly where the contract says float32 -- the model-frame point q
and the nearest-point search, tgp_nn1's arithmetic with the two fmaf steps computed exactly in float64 and rounded once -- float64
everywhere else.  The sums over the inliers are numpy's (pairwise) sums, the eigenvectors numpy's: the kernel's summation order and
its Jacobi rotations differ, which is what the tests' 1e-6 allows for.

    refine(model (m,6), src (n,3), R, t, s, max_dist, mode=1, with_scale=False, iters=30, tol_rot=1e-5, tol_trans=1e-6, min_inliers=6)
        -> dict R (3,3) / t (3,) / s float32 (the float64 state rounded once), R64 / t64 / s64, status, inliers, iters, rmse,
           corr (n,) int32, first_corr / first_q (the pre-update correspondences and points of iteration 0)
"""
import numpy as np

MAX_POINTS = 2048
f32 = np.float32


def fma32(a, b, c):
    """float32 fmaf(a, b, c): the product of two float32 is exact in float64; the sum's double rounding (to float64, then to float32)
    differs from the single one only when the float64 sum lies within 2^-29 relative of a float32 tie -- not on the tests' data,
    which compare the result with ops.nn1's"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def to_model_frame(src, R, t, s):
    """q = float32(R^T (p - t) / s): float64 on the float32 points, every product and sum rounded on its own, in the kernel's order"""
    d = np.asarray(src, dtype=f32).astype(np.float64) - t[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        q = [((R[0, a] * d[:, 0] + R[1, a] * d[:, 1]) + R[2, a] * d[:, 2]) / s for a in range(3)]
        return np.stack(q, 1).astype(f32)


def nearest(q, y):
    """tgp_nn1's float32 search of q (n,3) in y (m,3) -> (index (n,), value (n,)); first index on ties; a NaN row gives index 0"""
    q, y = np.asarray(q, dtype=f32), np.asarray(y, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        qq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        yy = (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
        best = np.zeros(len(q), dtype=f32)
        besti = np.zeros(len(q), dtype=np.int64)
        for lo in range(0, len(q), 256):                           # rows in blocks: the (block, m) tables stay small
            qb = q[lo:lo + 256]
            inner = qb[:, 0:1] * y[None, :, 0]
            inner = fma32(np.broadcast_to(qb[:, 1:2], inner.shape), np.broadcast_to(y[None, :, 1], inner.shape), inner)
            inner = fma32(np.broadcast_to(qb[:, 2:3], inner.shape), np.broadcast_to(y[None, :, 2], inner.shape), inner)
            dv = (yy[None, :] + qq[lo:lo + 256, None]) - f32(2.0) * inner
            # the scan: index 0 first, then every strictly smaller value; a NaN at index 0 is never beaten
            nan0 = np.isnan(dv[:, 0])
            i = np.argmin(np.where(np.isnan(dv), f32(np.inf), dv), axis=1)
            i = np.where(nan0, 0, i)
            besti[lo:lo + 256] = i
            best[lo:lo + 256] = dv[np.arange(len(qb)), i]
    return besti, best


def rotation_angle(Ra, Rb):
    D = Ra.T @ Rb
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0)))


def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-4:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def solve_point(y, p, s, with_scale):
    """the least-squares similarity p = s R y + t of the pairs, R proper (Horn's quaternion) -> (status, R, t, s)"""
    ybar, pbar = y.mean(0), p.mean(0)
    yc, pc = y - ybar, p - pbar
    S = yc.T @ pc                                                  # S[a][b] = sum yc_a pc_b
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])
    if not np.isfinite(N).all():
        return 2, None, None, None
    w, x, yq, z = np.linalg.eigh(N)[1][:, -1]
    R = np.array([[1 - 2 * (yq * yq + z * z), 2 * (x * yq - w * z), 2 * (x * z + w * yq)],
                  [2 * (x * yq + w * z), 1 - 2 * (x * x + z * z), 2 * (yq * z - w * x)],
                  [2 * (x * z - w * yq), 2 * (yq * z + w * x), 1 - 2 * (x * x + yq * yq)]])
    if with_scale:
        with np.errstate(invalid="ignore", divide="ignore"):
            s = float((R * S.T).sum() / (yc * yc).sum())
        if not (s > 0 and np.isfinite(s)):
            return 2, None, None, None
    return 0, R, pbar - s * (R @ ybar), s


def solve_plane(q, y, nrm, R, t, s):
    """one damped Gauss-Newton step in the model frame -> (status, R, t, angle, translation)"""
    rows = np.concatenate([np.cross(q, nrm), nrm], 1)              # (k, 6)
    r = ((q - y) * nrm).sum(1)
    A, b = rows.T @ rows, rows.T @ r
    A = A + np.eye(6) * (1e-9 * np.trace(A) / 6.0)
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        if not d > 0:
            return 2, None, None, None, None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    with np.errstate(all="ignore"):
        x = np.linalg.solve(L.T, np.linalg.solve(L, -b))
    if not np.isfinite(x).all():
        return 2, None, None, None, None
    Rn = R @ rodrigues(x[:3]).T
    tn = t - s * (Rn @ x[3:])
    if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
        return 2, None, None, None, None
    return 0, Rn, tn, float(np.linalg.norm(x[:3])), float(s * np.linalg.norm(x[3:]))


def refine(model, src, R, t, s, max_dist, mode=1, with_scale=False, iters=30, tol_rot=1e-5, tol_trans=1e-6, min_inliers=6):
    model = np.asarray(model, dtype=f32)
    src = np.asarray(src, dtype=f32).reshape(-1, 3)
    assert 1 <= len(model) <= MAX_POINTS and len(src) <= MAX_POINTS and iters >= 1 and not (mode == 1 and with_scale)
    y32 = model[:, :3]
    y64, n64 = y32.astype(np.float64), model[:, 3:6].astype(np.float64)
    p64 = src.astype(np.float64)
    R = np.asarray(R, dtype=f32).astype(np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=f32).astype(np.float64).reshape(3)
    s = float(f32(s))
    gate = float(f32(max_dist))
    tol_rot, tol_trans = float(f32(tol_rot)), float(f32(tol_trans))
    min_inliers = max(int(min_inliers), 6)
    finite = np.isfinite(src).all(1)
    never_stop = not (tol_rot > 0) and not (tol_trans > 0)

    def correspond():
        q = to_model_frame(src, R, t, s)
        if len(src) == 0:
            return q, np.zeros(0, np.int64), np.zeros(0, bool)
        idx, val = nearest(q, y32)
        thr = f32((gate / s) * (gate / s))
        with np.errstate(invalid="ignore"):
            return q, idx, (val <= thr) & finite

    status, done, first = 0, 0, None
    for it in range(iters):
        q, idx, inl = correspond()
        if first is None:
            first = (q.copy(), np.where(inl, idx, -1).astype(np.int32))
        if inl.sum() < min_inliers:
            status = 1
            break
        if mode == 0:
            st, Rn, tn, sn = solve_point(y64[idx[inl]], p64[inl], s, with_scale)
            if st:
                status = st
                break
            ang, tr = rotation_angle(R, Rn), float(np.linalg.norm(tn - t))
            R, t, s = Rn, tn, sn
        else:
            st, Rn, tn, ang, tr = solve_plane(q[inl].astype(np.float64), y64[idx[inl]], n64[idx[inl]], R, t, s)
            if st:
                status = st
                break
            R, t = Rn, tn
        done = it + 1
        if not never_stop and ang <= tol_rot and tr <= tol_trans:
            break
    q, idx, inl = correspond()
    k = int(inl.sum())
    d = q[inl].astype(np.float64) - y64[idx[inl]]
    rmse = f32(s * np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum() / k)) if k else f32(np.nan)
    return dict(R=R.astype(f32), t=t.astype(f32), s=f32(s), R64=R, t64=t, s64=s, status=status, inliers=k, iters=done, rmse=rmse,
                corr=np.where(inl, idx, -1).astype(np.int32), first_q=first[0], first_corr=first[1])


def rot(axis, deg):
    """rotation matrix (float64) about ``axis`` by ``deg`` degrees"""
    a = np.asarray(axis, dtype=np.float64)
    return rodrigues(a / np.linalg.norm(a) * np.deg2rad(deg))


def pose_error(R, t, Rg, tg):
    """(degrees, millimetres) between two poses"""
    return np.rad2deg(rotation_angle(np.asarray(Rg, np.float64), np.asarray(R, np.float64))), 1000.0 * float(np.linalg.norm(np.asarray(t, np.float64) - np.asarray(tg, np.float64)))


def two_boxes():
    """the tests' model: two boxes of unequal edges joined off-centre (no symmetry) -> (verts, faces), model units about 1 across"""
    from tgpose_amd.datasets import shapes
    v1, f1 = shapes.box((0.9, 0.5, 0.6))
    v2, f2 = shapes.box((0.4, 0.35, 0.3))
    v2 = v2 + np.array([0.2, 0.425, 0.1], dtype=np.float32)      # on top of the first, towards +x and +z
    return np.concatenate([v1, v2]).astype(f32), np.concatenate([f1, f2 + len(v1)]).astype(np.int32)


# ---- the rendered scenes of the GPU tests (tests/test_icp_gpu.py, tests/test_track_icp_gpu.py): two_boxes instances standing on a table
TABLE_TILT = -150.0          # degrees about the camera's x axis: the models' +y (up) points towards the camera's -y, tilted to the camera
OBJECTS = [dict(s=0.16, x=0.0, z=0.0, yaw=35.0, inst_id=11), dict(s=0.14, x=-0.27, z=0.03, yaw=-50.0, inst_id=12),
           dict(s=0.13, x=0.26, z=-0.02, yaw=120.0, inst_id=13)]


def table_scene(k=0, objects=(0, 1, 2), gap=0.0):
    """frame k of the sequence: the chosen objects (mesh 0, two_boxes) moved 4 mm along and 2 degrees about the table's normal per
    frame, and the table (mesh 1, a plane in z = 0) under their bottom faces -> list of instance dicts for synthetic.render_scenes"""
    base = rot([1, 0, 0], TABLE_TILT)
    centre = np.array([0.02, 0.0, 0.8])
    sc = []
    for o in objects:
        ob = OBJECTS[o]
        sign = 1.0 if o % 2 == 0 else -1.0
        on_table = np.array([ob["x"] + sign * 0.004 * k, 0.25 * ob["s"], ob["z"] - 0.003 * k])      # the bottom face is y = -0.25 s
        sc.append(dict(mesh=0, inst_id=ob["inst_id"], R=base @ rot([0, 1, 0], ob["yaw"] + sign * 2.0 * k), t=centre + base @ on_table, s=ob["s"]))
    sc.append(dict(mesh=1, inst_id=200, R=base @ rot([1, 0, 0], -90.0), t=centre - base @ np.array([0.0, gap, 0.0]), s=1.0))   # the plane's +z is the objects' +y
    return sc
