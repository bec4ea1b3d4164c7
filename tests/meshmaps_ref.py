"""NumPy restatement of the mesh maps (include/tgpose.h tgp_mesh_maps; DESIGN.md section 3 "Mesh maps and dense model-based
tracking"), written from that text on tests/render_ref.py: the window becomes the camera K', render_ref rasterises the job as a w x h
frame under it (its z and face are the maps' winners), and what is restated here is what is done with a winner -- the surface point,
the normal, the miss of a triangle without a model-frame normal -- and ops.mesh_windows.  float32 products, sums and quotients that
each round on their own; int64 edge functions.

    camera(K (4,), window (4,)) -> K' (4,) float32
    maps(meshes, camk (S,4), job_img, job_mesh, job_pose (J,3,4), window (J,4), h, w, near=0.01, vnormals=None)
        -> dict z (J,h,w), depth uint16, vertex, normal (J,h,w,3), face int32, count, dropped, status (J) int32
    windows(meshes, camk, job_img, job_mesh, job_pose, h, w, H, W, pad=1.0) -> (J,4) float32
"""
import numpy as np

from tests import render_ref

F = np.float32


def camera(K, window):
    """the window (u0, v0, du, dv) as a camera: K' = (fx / du, fy / dv, (cx - u0) / du, (cy - v0) / dv)"""
    K, win = np.asarray(K, F), np.asarray(window, F)
    with np.errstate(all="ignore"):
        return np.array([K[0] / win[2], K[1] / win[3], (K[2] - win[0]) / win[2], (K[3] - win[1]) / win[3]], F)


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def resolve(verts, faces, pose, Kp, near, z, face, vnormals=None):
    """the winners (z (h,w) with +inf empty, face (h,w) with -1 empty, as render_ref.render_scene gives them) of one job -> z, vertex,
    normal, face with the maps' misses: 0, zeros, -1"""
    h, w = z.shape
    verts, faces = np.asarray(verts, F), np.asarray(faces, np.int64).reshape(-1, 3)
    T = np.asarray(pose, F).reshape(3, 4)
    out_z, out_f = np.zeros((h, w), F), np.full((h, w), -1, np.int32)
    out_v, out_n = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
    rr, cc = np.nonzero(face >= 0)
    if not len(rr):
        return out_z, out_v, out_n, out_f
    X, Y, iz, _ = render_ref.project(verts, pose, Kp, near)
    idx = faces[face[rr, cc]]                                                      # (n,3)
    area = _orient(X[idx[:, 0]], Y[idx[:, 0]], X[idx[:, 1]], Y[idx[:, 1]], X[idx[:, 2]], Y[idx[:, 2]])
    idx = np.where((area < 0)[:, None], idx[:, [0, 2, 1]], idx)                    # corners 1 and 2 change places
    x, y = X[idx], Y[idx]
    sx, sy = cc.astype(np.int64) * 256, rr.astype(np.int64) * 256
    e = [_orient(x[:, (k + 1) % 3], y[:, (k + 1) % 3], x[:, (k + 2) % 3], y[:, (k + 2) % 3], sx, sy) for k in range(3)]
    fa = np.abs(area).astype(F)
    zz = z[rr, cc].astype(F)
    with np.errstate(all="ignore"):
        b = [((e[k].astype(F) / fa) * iz[idx[:, k]]) * zz for k in range(3)]
        p = [verts[idx[:, k]] for k in range(3)]                                   # (n,3) each
        vert = np.stack([(b[0] * p[0][:, a] + b[1] * p[1][:, a]) + b[2] * p[2][:, a] for a in range(3)], 1)
        if vnormals is None:
            u, v = p[1] - p[0], p[2] - p[0]
            n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        else:
            vn = np.asarray(vnormals, F)
            q = [vn[idx[:, k]] for k in range(3)]
            n = np.stack([(b[0] * q[0][:, a] + b[1] * q[1][:, a]) + b[2] * q[2][:, a] for a in range(3)], 1)
        n = n.astype(F)
        s = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        hit = (s > 0) & (s < F(np.inf))                                            # False for a NaN
        n = n / np.where(hit, s, F(1))[:, None]
        if vnormals is None:
            m = [(T[r, 0] * n[:, 0] + T[r, 1] * n[:, 1]) + T[r, 2] * n[:, 2] for r in range(3)]
            rx, ry = (cc.astype(F) - Kp[2]) / Kp[0], (rr.astype(F) - Kp[3]) / Kp[1]
            away = (m[0] * rx + m[1] * ry) + m[2] > 0
            n = np.where(away[:, None], -n, n)
    rr, cc = rr[hit], cc[hit]
    out_z[rr, cc] = zz[hit]
    out_v[rr, cc] = vert[hit].astype(F)
    out_n[rr, cc] = n[hit].astype(F)
    out_f[rr, cc] = face[face >= 0][hit]
    return out_z, out_v, out_n, out_f


def maps(meshes, camk, job_img, job_mesh, job_pose, window, h, w, near=0.01, vnormals=None):
    """meshes: list of (verts (V,3), faces (F,3)); vnormals: None (face normals) or one (V,3) array per mesh"""
    J, S, M = len(job_img), len(camk), len(meshes)
    out = dict(z=np.zeros((J, h, w), F), depth=np.zeros((J, h, w), np.uint16), vertex=np.zeros((J, h, w, 3), F),
               normal=np.zeros((J, h, w, 3), F), face=np.full((J, h, w), -1, np.int32), count=np.zeros(J, np.int32),
               dropped=np.zeros(J, np.int32), status=np.zeros(J, np.int32))
    for j in range(J):
        img, mi = int(job_img[j]), int(job_mesh[j])
        if not (0 <= img < S and 0 <= mi < M):
            out["status"][j] = 1
            continue
        Kp = camera(camk[img], window[j])
        r = render_ref.render_scene(meshes, [(mi, 1, job_pose[j])], Kp, h, w, near)
        z, v, n, f = resolve(meshes[mi][0], meshes[mi][1], job_pose[j], Kp, near, r["z"], r["face"], None if vnormals is None else vnormals[mi])
        with np.errstate(all="ignore"):
            mm = np.rint(z * F(1000))
        out["z"][j], out["vertex"][j], out["normal"][j], out["face"][j] = z, v, n, f
        out["depth"][j] = np.where(mm <= 65535, mm, 0).astype(np.uint16)
        out["count"][j] = int((f >= 0).sum())
        out["dropped"][j] = int(r["dropped"].sum())
    return out


def windows(meshes, camk, job_img, job_mesh, job_pose, h, w, H, W, pad=1.0):
    """ops.mesh_windows: tests/raycast_ref.py windows' rule on the eight corners of the mesh's bounding box (corner k takes the greatest
    coordinate on axis q where bit 2 - q of k is set, else the least)"""
    J = len(job_img)
    out = np.zeros((J, 4), F)
    for j in range(J):
        m = int(np.clip(job_mesh[j], 0, len(meshes) - 1))
        s = int(np.clip(job_img[j], 0, len(camk) - 1))
        v = np.asarray(meshes[m][0], F)
        lo, hi = v.min(0), v.max(0)
        K, T = np.asarray(camk[s], F), np.asarray(job_pose[j], F).reshape(3, 4)
        us, vs, zs = [], [], []
        with np.errstate(all="ignore"):
            for k in range(8):
                p = [hi[q] if k >> (2 - q) & 1 else lo[q] for q in range(3)]
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
            du = (u1 - u0) / F(w - 1) if w > 1 else F(1)
            dv = (v1 - v0) / F(h - 1) if h > 1 else F(1)
        out[j] = (u0, v0, du, dv) if good else (F(np.nan),) * 4
    return out
