"""NumPy restatement of the TSDF ray caster (DESIGN.md section 3 "Ray casting and frame-to-model tracking"; the kernel is
csrc/raycast.hip), of ops.tsdf_windows and of ops.IcpModels.from_raycast's packing.  Written from the contract's text, not from the
kernel: float32 products, sums, quotients and square roots that each round on their own; all rays of a job at once."""
import math

import numpy as np

F = np.float32


def inverse_pose(job_pose):
    """(J,3,4) [s R | t] -> (J,3,4) float32: the inverse map, by cofactors in float64 in a fixed order of operations (ops.pose_inverse
    does the same operations in torch), rounded once"""
    T = np.asarray(job_pose, dtype=F).astype(np.float64).reshape(-1, 3, 4)
    a, b, c = T[:, 0, 0], T[:, 0, 1], T[:, 0, 2]
    d, e, f = T[:, 1, 0], T[:, 1, 1], T[:, 1, 2]
    g, h, i = T[:, 2, 0], T[:, 2, 1], T[:, 2, 2]
    with np.errstate(all="ignore"):
        c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
        c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
        c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
        det = (a * c00 + b * c10) + c * c20
        A = np.stack([np.stack([c00, c01, c02], 1), np.stack([c10, c11, c12], 1), np.stack([c20, c21, c22], 1)], 1) / det[:, None, None]
        t = T[:, :, 3]
        back = -((A[:, :, 0] * t[:, None, 0] + A[:, :, 1] * t[:, None, 1]) + A[:, :, 2] * t[:, None, 2])
    return np.concatenate([A, back[:, :, None]], 2).astype(F)


def max_samples(G, step):
    return int(math.ceil(1.7320508075688772 * float(G - 1) / float(F(step)))) + 2


def _cell(vsum, weight, G, min_weight, g):
    """g: 3 arrays (n,) float32 -> (known (n,), f (8, n) float32, t: 3 arrays)"""
    hi = F(G)
    with np.errstate(all="ignore"):
        inside = np.ones(g[0].shape, dtype=bool)
        for q in range(3):
            inside &= (g[q] >= F(-1)) & (g[q] <= hi)
        idx, t = [], []
        for q in range(3):
            i = np.clip(np.floor(np.where(inside, g[q], F(0))).astype(np.int64), 0, G - 2)
            idx.append(i)
            t.append((g[q] - i.astype(F)).astype(F))
        known = inside.copy()
        f = np.zeros((8,) + g[0].shape, dtype=F)
        for k in range(8):
            q = (idx[0] + (k >> 2), idx[1] + ((k >> 1) & 1), idx[2] + (k & 1))
            w, s = weight[q], vsum[q]
            known &= w >= min_weight
            f[k] = s.astype(F) / w.astype(F)
    return known, f, t


def _lerp(a, b, t):
    return a + t * (b - a)


def _trilinear(f, t):
    c00, c01, c10, c11 = _lerp(f[0], f[1], t[2]), _lerp(f[2], f[3], t[2]), _lerp(f[4], f[5], t[2]), _lerp(f[6], f[7], t[2])
    c0, c1 = _lerp(c00, c01, t[1]), _lerp(c10, c11, t[1])
    return _lerp(c0, c1, t[0]), (c00, c01, c10, c11, c0, c1)


def raycast(vsum, weight, meta, camk, job_img, job_model, job_inv, window, h, w, min_weight=1, step=1.0, near=0.01):
    """tgp_tsdf_raycast: vsum, weight (M,G,G,G) int32, meta (M,4), camk (S,4), job_inv (J,3,4), window (J,4) float32 -> dict z (J,h,w)
    float32, depth (J,h,w) uint16, vertex, normal (J,h,w,3) float32, count, status (J) int32"""
    M, G = vsum.shape[0], vsum.shape[1]
    S = len(camk)
    J = len(job_img)
    step, near = F(step), F(near)
    cap = max_samples(G, step)
    out = dict(z=np.zeros((J, h, w), F), depth=np.zeros((J, h, w), np.uint16), vertex=np.zeros((J, h, w, 3), F),
               normal=np.zeros((J, h, w, 3), F), count=np.zeros(J, np.int32), status=np.zeros(J, np.int32))
    inf = F(np.inf)
    for j in range(J):
        m, s = int(job_model[j]), int(job_img[j])
        if not (0 <= m < M and 0 <= s < S):
            out["status"][j] = 1
            continue
        K = np.asarray(camk[s], dtype=F)
        I = np.asarray(job_inv[j], dtype=F).reshape(3, 4)
        win = np.asarray(window[j], dtype=F)
        mt = np.asarray(meta[m], dtype=F)
        voxel, half, last = mt[3], F(G // 2) - F(0.5), F(G - 1)
        rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        rr, cc = rr.ravel(), cc.ravel()
        n = h * w
        with np.errstate(all="ignore"):
            u = win[0] + cc.astype(F) * win[2]
            v = win[1] + rr.astype(F) * win[3]
            dx, dy = (u - K[2]) / K[0], (v - K[3]) / K[1]
            e = [(((I[q, 0] * dx + I[q, 1] * dy) + I[q, 2]) / voxel).astype(F) for q in range(3)]
            o = [np.full(n, (I[q, 3] - mt[q]) / voxel + half, dtype=F) for q in range(3)]
            zin, zout = np.full(n, near, dtype=F), np.full(n, inf, dtype=F)
            ok = np.ones(n, dtype=bool)
            for q in range(3):
                moving = e[q] != 0
                t0, t1 = (F(0) - o[q]) / e[q], (last - o[q]) / e[q]
                zin = np.where(moving, np.fmax(zin, np.fmin(t0, t1)), zin)
                zout = np.where(moving, np.fmin(zout, np.fmax(t0, t1)), zout)
                ok &= np.where(moving, (t0 == t0) & (t1 == t1), (o[q] >= 0) & (o[q] <= last))
            length = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            dz = (step / length).astype(F)
            ok &= (length > 0) & (length < inf) & (dz > 0) & (dz < inf) & (zin <= zout) & (zin < inf) & (zout < inf)
            alive = ok.copy()
            have = np.zeros(n, dtype=bool)
            fprev = np.zeros(n, dtype=F)
            hit = np.zeros(n, dtype=bool)
            zs = np.zeros(n, dtype=F)
            for k in range(cap):
                if not alive.any():
                    break
                zk = zin + F(k) * dz
                alive &= zk <= zout
                g = [o[q] + zk * e[q] for q in range(3)]
                known, f8, t = _cell(vsum[m], weight[m], G, min_weight, g)
                f, _ = _trilinear(f8, t)
                unknown = alive & ~known
                have[unknown] = False
                pos = alive & known & (f > 0)
                have[pos] = True
                fprev[pos] = f[pos]
                end = alive & known & ~(f > 0)
                now = end & have
                zstar = (zin + F(k - 1) * dz) + dz * (fprev / (fprev - f))
                zs[now] = zstar[now]
                hit |= now
                alive &= ~end
            g = [o[q] + zs * e[q] for q in range(3)]
            known, f8, t = _cell(vsum[m], weight[m], G, min_weight, g)
            hit &= known
            _, (c00, c01, c10, c11, c0, c1) = _trilinear(f8, t)
            nx = c1 - c0
            ny = _lerp(c01 - c00, c11 - c10, t[0])
            nz = _lerp(_lerp(f8[1] - f8[0], f8[3] - f8[2], t[1]), _lerp(f8[5] - f8[4], f8[7] - f8[6], t[1]), t[0])
            size = np.sqrt((nx * nx + ny * ny) + nz * nz)
            hit &= (size > 0) & (size < inf)
            normal = np.stack([nx / size, ny / size, nz / size], 1)
            mid = F(G // 2)
            vertex = np.stack([mt[q] + ((g[q] + F(0.5)) - mid) * voxel for q in range(3)], 1)
            zs = np.where(hit, zs, F(0)).astype(F)
            mm = np.rint(zs * F(1000))
            depth = np.where(hit & (mm <= F(65535)), mm, 0).astype(np.uint16)
        out["z"][j] = zs.reshape(h, w)
        out["depth"][j] = depth.reshape(h, w)
        out["vertex"][j] = np.where(hit[:, None], vertex, F(0)).astype(F).reshape(h, w, 3)
        out["normal"][j] = np.where(hit[:, None], normal, F(0)).astype(F).reshape(h, w, 3)
        out["count"][j] = int(hit.sum())
    return out


def windows(meta, G, camk, job_img, job_model, job_pose, h, w, H, W, pad=1.0):
    """ops.tsdf_windows: (J,4) float32 (u0, v0, du, dv): the box of the cube's eight projected corners, grown by ``pad`` pixels, clamped
    to the frame [0, W-1] x [0, H-1], as an h x w grid that spans it (du = (u1 - u0) / (w - 1), 1 when w == 1).  A corner at or behind
    z = 1e-6, or a projection that is not finite, empties the window: four NaN, so every ray misses by the rule.  Indices out of range
    are clamped (the ray cast refuses the job itself).  float32 elementwise; the min and max over the eight corners are exact in any
    order."""
    J = len(job_img)
    out = np.zeros((J, 4), F)
    for j in range(J):
        m = int(np.clip(job_model[j], 0, len(meta) - 1))
        s = int(np.clip(job_img[j], 0, len(camk) - 1))
        mt, K, T = np.asarray(meta[m], F), np.asarray(camk[s], F), np.asarray(job_pose[j], F).reshape(3, 4)
        halfe = F(G) * mt[3] * F(0.5)
        us, vs, zs = [], [], []
        with np.errstate(all="ignore"):
            for k in range(8):
                p = [mt[q] + (halfe if k >> (2 - q) & 1 else -halfe) for q in range(3)]
                c = [((T[r, 0] * p[0] + T[r, 1] * p[1]) + T[r, 2] * p[2]) + T[r, 3] for r in range(3)]
                us.append(K[0] * (c[0] / c[2]) + K[2])
                vs.append(K[1] * (c[1] / c[2]) + K[3])
                zs.append(c[2])
            us, vs, zs = np.array(us, F), np.array(vs, F), np.array(zs, F)
            good = bool((zs > F(1e-6)).all()) and bool(np.isfinite(us).all()) and bool(np.isfinite(vs).all())
            u0 = np.clip(us.min() - F(pad), F(0), F(W - 1))
            u1 = np.clip(us.max() + F(pad), F(0), F(W - 1))
            v0 = np.clip(vs.min() - F(pad), F(0), F(H - 1))
            v1 = np.clip(vs.max() + F(pad), F(0), F(H - 1))
            du = (u1 - u0) / F(max(w - 1, 1)) if w > 1 else F(1)
            dv = (v1 - v0) / F(max(h - 1, 1)) if h > 1 else F(1)
        out[j] = (u0, v0, du, dv) if good else (F(np.nan),) * 4
    return out


def pack(rc):
    """ops.IcpModels.from_raycast's packing: (points (J, h w, 6) float32, counts (J) int32): each job's hits first, in ray order,
    [vertex, normal]; rows past the count are zero"""
    J, h, w = rc["z"].shape
    pts = np.zeros((J, h * w, 6), F)
    for j in range(J):
        hit = rc["z"][j].ravel() > 0
        rows = np.concatenate([rc["vertex"][j].reshape(-1, 3), rc["normal"][j].reshape(-1, 3)], 1)[hit]
        pts[j, :len(rows)] = rows
    return pts, rc["count"].astype(np.int32)
