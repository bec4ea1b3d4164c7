"""numpy restatement of the distance-field pose search (include/tgpose.h tgp_field_build / tgp_pose_search; DESIGN.md section 3
"Model-based acquisition"), written from that text.  Everything after the floor is an integer, so the kernels must equal this file
bit for bit; the operation order of the float32 part is written down HERE, once:

    field     c_a = ctr_a + ((i_a - G/2) + 0.5) voxel         float32, product and sum rounded on their own
              dv  = (|y|^2 + |c|^2) - 2 fmaf(c_z, y_z, fmaf(c_y, y_y, c_x y_x))       tgp_nn1's value (icp_ref.fma32), the least over y
              byte = #{l in 1..cap : dv >= T_l},  T_l = float32((l voxel / 4)^2) from float64
    search    inv = float32(1 / (float64(s) float64(voxel)))
              e   = p - anchor                                float32
              u_a = (R[0][a] e_0 + R[1][a] e_1) + R[2][a] e_2    float32, NO fused product
              w_a = u_a inv + G/2                             float32, product and sum rounded on their own
              b_a = floor(min(max(w_a, -512), 511)),  a NaN w_a -> -512
    cost(r,d) = sum over the live, finite points of field[b + d], cap where b + d leaves the grid          int32
    pose      t_i = anchor_i - s ((R_i0 m_0 + R_i1 m_1) + R_i2 m_2),  m_a = ctr_a + d_a voxel               float64, rounded once

    field_meta(points, G, cap) -> (meta (4,) f32, thresholds (cap,) f32)
    build_field(points, G, cap) -> (field (G,G,G) uint8, meta, thresholds)
    bases(cloud, count, anchor, scale, voxel, G, rotations) -> (b (R,n,3) int64, live (n,) bool)
    search(field, meta, cap, cloud, count, anchor, scale, rotations, K, stride, top) -> dict table (R,2), cost, rot, shift (top,)
        int32, poses (top,3,4) float32
    brute(points, meta, cap, G, cloud, count, anchor, scale, rotations, K, stride) -> (R, D) float64-derived costs (the CPU test)
    acquire_chain(...) -> the whole chain of pose.ModelSearch for one cloud: search, icp_ref.refine of every candidate,
        verify_ref.verify_job of every refined candidate, the best score (ties: the lower rank)
"""
import numpy as np

from tests.icp_ref import fma32

f32 = np.float32
REFUSED = 2 ** 31 - 1


def field_meta(points, G, cap):
    pts = np.asarray(points, dtype=f32).reshape(-1, 3)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    ctr = ((lo + hi) * 0.5).astype(f32)
    half = f32(0.575 * (hi - lo).max())
    voxel = f32(2.0 * np.float64(half) / G)
    edge = np.arange(1, cap + 1, dtype=np.float64) * np.float64(voxel) / 4.0
    return np.array([ctr[0], ctr[1], ctr[2], voxel], dtype=f32), (edge * edge).astype(f32)


def shifts(K, stride):
    """(D,3) int64 in shift-index order"""
    r = np.arange(-K, K + 1, dtype=np.int64) * stride
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def build_field(points, G, cap):
    y = np.asarray(points, dtype=f32).reshape(-1, 3)
    meta, thr = field_meta(y, G, cap)
    voxel = meta[3]
    k = ((np.arange(G, dtype=f32) - f32(G // 2)) + f32(0.5)) * voxel
    c = [meta[a] + k for a in range(3)]                            # float32 throughout
    cx, cy, cz = [g.reshape(-1) for g in np.meshgrid(c[0], c[1], c[2], indexing="ij")]
    qq = (cx * cx + cy * cy) + cz * cz
    yy = (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
    best = np.full(cx.shape, np.inf, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, len(y), 64):                            # model points in blocks: the (voxels, block) tables stay small
            yb, shape = y[lo:lo + 64], (len(cx), len(y[lo:lo + 64]))
            inner = cx[:, None] * yb[None, :, 0]
            inner = fma32(np.broadcast_to(cy[:, None], shape), np.broadcast_to(yb[None, :, 1], shape), inner)
            inner = fma32(np.broadcast_to(cz[:, None], shape), np.broadcast_to(yb[None, :, 2], shape), inner)
            dv = (yy[None, lo:lo + 64] + qq[:, None]) - f32(2.0) * inner
            best = np.minimum(best, np.where(np.isnan(dv), f32(np.inf), dv).min(1))
    field = (best[:, None] >= thr[None, :]).sum(1).astype(np.uint8)
    return field.reshape(G, G, G), meta, thr


def bases(cloud, count, anchor, scale, voxel, G, rotations):
    p = np.asarray(cloud, dtype=f32).reshape(-1, 3)
    n = len(p) if count is None else int(count)
    p = p[:n]
    live = np.isfinite(p).all(1)
    Rs = np.asarray(rotations, dtype=f32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        inv = f32(1.0 / (np.float64(f32(scale)) * np.float64(f32(voxel))))
        e = p - np.asarray(anchor, dtype=f32)[None, :]
        out = np.empty((len(Rs), n, 3), dtype=np.int64)
        for a in range(3):
            u = (Rs[:, None, 0, a] * e[None, :, 0] + Rs[:, None, 1, a] * e[None, :, 1]) + Rs[:, None, 2, a] * e[None, :, 2]
            w = u * inv + f32(G // 2)
            assert w.dtype == f32
            out[:, :, a] = np.floor(np.fmin(np.fmax(w, f32(-512.0)), f32(511.0))).astype(np.int64)
    return out, live


def rotation_costs(field, cap, b, live, K, stride):
    """the (D,) int64 costs of one rotation's bases b (n,3)"""
    G, reach = field.shape[0], K * stride
    pad = 2 * reach + 1
    big = np.full((G + 2 * pad,) * 3, cap, dtype=np.int64)
    big[pad:pad + G, pad:pad + G, pad:pad + G] = field
    bb = np.clip(b[live], -reach - 1, G + reach) + pad             # a base this far out is out for every shift, as it was
    d = np.arange(-K, K + 1, dtype=np.int64) * stride
    X, Y, Z = [bb[:, a:a + 1] + d[None, :] for a in range(3)]
    return big[X[:, :, None, None], Y[:, None, :, None], Z[:, None, None, :]].sum(0).reshape(-1)


def poses_of(meta, anchor, scale, rotations, rot, shift, K, stride):
    out = np.full((len(rot), 3, 4), np.nan, dtype=f32)
    sh = shifts(K, stride)
    ctr, voxel, s = meta[:3].astype(np.float64), np.float64(meta[3]), np.float64(f32(scale))
    for t, (r, sx) in enumerate(zip(rot, shift)):
        if r < 0:
            continue
        R = np.asarray(rotations[r], dtype=f32).astype(np.float64)
        m = ctr + sh[sx].astype(np.float64) * voxel
        Rm = (R[:, 0] * m[0] + R[:, 1] * m[1]) + R[:, 2] * m[2]
        out[t, :, :3] = rotations[r]
        out[t, :, 3] = (np.asarray(anchor, dtype=f32).astype(np.float64) - s * Rm).astype(f32)
    return out


def select(table, top):
    R = len(table)
    order = np.lexsort((np.arange(R), table[:, 0]))[:top]
    cost = np.full(top, REFUSED, dtype=np.int32)
    rot = np.full(top, -1, dtype=np.int32)
    shift = np.full(top, -1, dtype=np.int32)
    ok = table[order, 0] != REFUSED
    k = int(ok.sum())
    cost[:k], rot[:k], shift[:k] = table[order[:k], 0], order[:k], table[order[:k], 1]
    return cost, rot, shift


def search(field, meta, cap, cloud, count, anchor, scale, rotations, K, stride, top, n_models=1, job_model=0):
    rotations = np.asarray(rotations, dtype=f32).reshape(-1, 3, 3)
    R, n_cap = len(rotations), len(np.asarray(cloud).reshape(-1, 3))
    table = np.empty((R, 2), dtype=np.int32)
    if not (0 <= job_model < n_models) or (count is not None and not 0 <= count <= n_cap):
        table[:, 0], table[:, 1] = REFUSED, -1
    else:
        b, live = bases(cloud, count, anchor, scale, meta[3], field.shape[0], rotations)
        for r in range(R):
            c = rotation_costs(field, cap, b[r], live, K, stride)
            table[r] = c.min(), c.argmin()                         # argmin: the first, i.e. the smaller shift index
    cost, rot, shift = select(table, top)
    return dict(table=table, cost=cost, rot=rot, shift=shift, poses=poses_of(meta, anchor, scale, rotations, rot, shift, K, stride))


def brute(points, meta, cap, G, cloud, count, anchor, scale, rotations, K, stride):
    """The statement without a grid's quantisation, in float64: a point's cost at (r, d) is the number of quarter voxels its distance
    to the nearest model point holds (at most cap), cap outside the cube -> (R, D) int64.  A voxel's centre is at most sqrt(3)/2
    voxel = 3.47 quarter voxels from any point inside it and the distance to a set is 1-Lipschitz, so the restatement's cost of a
    point differs by at most 4."""
    y = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)[:count]
    p = p[np.isfinite(p).all(1)]
    ctr, voxel, s = meta[:3].astype(np.float64), float(meta[3]), float(scale)
    sh = shifts(K, stride).astype(np.float64)
    out = np.zeros((len(rotations), len(sh)), dtype=np.int64)
    for r, R in enumerate(np.asarray(rotations, dtype=np.float64)):
        q = (p - np.asarray(anchor, dtype=np.float64)) @ R / (s * voxel)              # rows R^T e
        for k, d in enumerate(sh):
            w = q + d + G / 2
            inside = ((w >= 0) & (w < G)).all(1)
            pos = ctr + (w - G / 2) * voxel
            dist = np.sqrt(((pos[:, None, :] - y[None, :, :]) ** 2).sum(2)).min(1)
            out[r, k] = np.where(inside, np.minimum(np.floor(4.0 * dist / voxel), cap), cap).sum()
    return out


def acquire_chain(field, meta, cap, model, mesh, cloud, scale, rotations, K, stride, top, gate, depth, camk, tau, mask=None, mask_val=0):
    """pose.ModelSearch with refine (point-to-plane, gate metres) and verify (tau millimetres) for ONE cloud, restated: the anchor is the
    cloud's float64 mean rounded once; every candidate of the top list goes through icp_ref.refine (a failed one keeps its start) and
    verify_ref.verify_job against ``depth`` (H,W) uint16; the highest score wins, ties to the lower rank.
    -> dict rank, R (3,3) / t (3,) float32, score, inliers, status, found (search's dict)"""
    from tests import icp_ref, verify_ref
    cloud = np.asarray(cloud, dtype=f32)
    scale = f32(scale)
    anchor = cloud[np.isfinite(cloud).all(1)].astype(np.float64).mean(0).astype(f32)
    found = search(field, meta, cap, cloud, None, anchor, scale, rotations, K, stride, top)
    best = None
    for rank in range(top):
        if found["rot"][rank] < 0:
            continue
        P = found["poses"][rank]
        r = icp_ref.refine(model, cloud, P[:, :3], P[:, 3], scale, gate, mode=1)
        R, t = (r["R"], r["t"]) if r["status"] == 0 else (P[:, :3], P[:, 3])
        pose = np.concatenate([R * scale, t[:, None]], 1).astype(f32)
        _, score = verify_ref.verify_job(mesh, pose, np.asarray(camk, dtype=f32), depth, tau, mask=mask, mask_val=mask_val)
        if best is None or score > best["score"]:
            best = dict(rank=rank, R=R, t=t, score=score, inliers=r["inliers"], status=r["status"])
    return dict(best, found=found)
