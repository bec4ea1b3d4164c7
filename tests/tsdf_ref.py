"""NumPy restatement of TSDF fusion and marching-tetrahedra meshing (DESIGN.md section 3 "Models from depth sequences"; the kernels
are csrc/tsdf.hip).  Written from the contract's text, not from the kernels: float32 products, sums and quotients that each round on
their own, np.rint's ties to even, integer sums.  The winding table the kernel carries is DERIVED here (derive_flip) from the
geometry of the six Kuhn tetrahedra; tests/test_tsdf_cpu.py holds the kernel's copy against it."""
import itertools

import numpy as np

F = np.float32

PERMS = list(itertools.permutations(range(3)))


def _paths():
    out = np.zeros((6, 4, 3), dtype=np.int64)
    for k, perm in enumerate(PERMS):
        for c, axis in enumerate(perm):
            out[k, c + 1] = out[k, c]
            out[k, c + 1, axis] += 1
    return out


PATHS = _paths()                        # (tetrahedron, path corner, axis): the corner's offset in the cube


def case_triangles(case):
    """the triangles of a tetrahedron whose path corner c is inside iff bit c of ``case`` is set, before any flip: a list of
    triangles, each three edges (a, b) of path corners with a < b"""
    ins = [c for c in range(4) if case >> c & 1]
    outs = [c for c in range(4) if not case >> c & 1]
    edge = lambda i, o: (min(i, o), max(i, o))
    if len(ins) == 1:
        return [[edge(ins[0], o) for o in outs]]
    if len(ins) == 3:
        return [[edge(i, outs[0]) for i in ins]]
    if len(ins) == 2:
        quad = [edge(ins[0], outs[0]), edge(ins[0], outs[1]), edge(ins[1], outs[1]), edge(ins[1], outs[0])]
        return [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return []


def derive_flip():
    """(6,) ints: bit ``case`` of word k is set iff the triangles of tetrahedron k in that case must swap their second and third
    vertex for the normal (b - a) x (c - a) to point from the inside corners to the outside ones.  Checked here for cut points
    anywhere on the edges, not only their middles: the sign cannot depend on them, and does not."""
    rng = np.random.RandomState(0)
    words = []
    for k in range(6):
        word = 0
        corners = PATHS[k].astype(np.float64)
        for case in range(1, 15):
            ins = [c for c in range(4) if case >> c & 1]
            outs = [c for c in range(4) if not case >> c & 1]
            toward = corners[outs].mean(0) - corners[ins].mean(0)
            signs = set()
            for trial in range(8):
                t = {e: (0.5 if trial == 0 else rng.uniform(0.02, 0.98)) for e in itertools.combinations(range(4), 2)}
                for tri in case_triangles(case):
                    p = [corners[a] + t[(a, b)] * (corners[b] - corners[a]) for a, b in tri]
                    signs.add(np.sign(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), toward)))
            assert len(signs) == 1 and 0.0 not in signs, (k, case, signs)
            if signs.pop() < 0:
                word |= 1 << case
        words.append(word)
    return tuple(words)


FLIP = derive_flip()


def centres(meta, G):
    """(3, G) float32: the voxel centres along x, y, z: c + (((float)i + 0.5f) - G/2) * voxel, float32 at every step"""
    meta = np.asarray(meta, dtype=F)
    i = (np.arange(G).astype(F) + F(0.5)) - F(G // 2)
    return np.stack([meta[a] + i * meta[3] for a in range(3)]).astype(F)


def tsdf_meta(center, extent, G):
    """ops.TsdfVolumes' cube rule (ops.field_meta's): half = 0.575 x the largest extent, voxel = 2 half / G; float64 on the float32
    inputs, each rounded to float32 once"""
    ctr = np.asarray(center, dtype=F)
    half = F(0.575 * float(np.asarray(extent, dtype=F).astype(np.float64).max()))
    return np.concatenate([ctr, [F(2.0 * float(half) / G)]]).astype(F)


def integrate(vsum, weight, meta, depth, camk, job_img, job_model, job_pose, trunc, near=0.01, mask=None, job_mask_val=None):
    """tgp_tsdf_integrate on vsum, weight (M,G,G,G) int32 IN PLACE; -> status (J) int32"""
    M, G = vsum.shape[0], vsum.shape[1]
    S, H, W = depth.shape
    trunc = F(trunc)
    inv = F(1024.0 / float(trunc))
    near = F(near)
    J = len(job_img)
    status = np.zeros(J, dtype=np.int32)
    for j in range(J):
        s, m = int(job_img[j]), int(job_model[j])
        if not (0 <= s < S and 0 <= m < M):
            status[j] = 1
            continue
        T = np.asarray(job_pose[j], dtype=F).reshape(3, 4)
        K = np.asarray(camk[s], dtype=F)
        c = centres(meta[m], G)
        x, y, z = c[0][:, None, None], c[1][None, :, None], c[2][None, None, :]
        with np.errstate(all="ignore"):
            p = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
            ok = p[2] > near
            u = K[0] * (p[0] / p[2]) + K[2]
            v = K[1] * (p[1] / p[2]) + K[3]
            ru, rv = np.rint(u), np.rint(v)
            ok = ok & (ru >= 0) & (ru <= F(W - 1)) & (rv >= 0) & (rv <= F(H - 1))
            xi = np.where(ok, ru, 0).astype(np.int64)
            yi = np.where(ok, rv, 0).astype(np.int64)
            d = depth[s][yi, xi]
            ok = ok & (d != 0)
            if mask is not None:
                ok = ok & (mask[s][yi, xi] == job_mask_val[j])
            sdf = d.astype(F) - p[2] * F(1000)
            ok = ok & ~(sdf < -trunc)
            q = np.rint(np.minimum(sdf, trunc) * inv)
        vsum[m] += np.where(ok, q, 0).astype(np.int32)
        weight[m] += ok.astype(np.int32)
    return status


def edge_vertex(sa, wa, sb, wb, pa, pb):
    """the cut point of an edge from its end a (earlier in the path: the smaller flat index) to b; pa, pb (n,3) float32"""
    fa = sa.astype(F) / wa.astype(F)
    fb = sb.astype(F) / wb.astype(F)
    t = fa / (fa - fb)
    return pa + t[:, None] * (pb - pa)


def mesh(vsum, weight, meta, min_weight=1, face_cap=None, return_tags=False):
    """tgp_tsdf_mesh_count / emit on one volume: vsum, weight (G,G,G) int32, meta (4,) -> (verts (3 F,3) float32, total, status);
    F = min(total, face_cap).  return_tags adds (F,3) int64 rows (cube flat index, tetrahedron, triangle)."""
    G = vsum.shape[0]
    c = centres(meta, G)
    n = G - 1
    ix, iy, iz = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    corner = lambda a, d: a[d[0]:d[0] + n, d[1]:d[1] + n, d[2]:d[2] + n]
    offs = list(itertools.product((0, 1), repeat=3))
    valid = np.ones((n, n, n), dtype=bool)
    for d in offs:
        valid &= corner(weight, d) >= min_weight
    keys, tris = [], []
    for k in range(6):
        case = np.zeros((n, n, n), dtype=np.int64)
        for cidx in range(4):
            case |= (corner(vsum, PATHS[k, cidx]) < 0).astype(np.int64) << cidx
        for cs in range(1, 15):
            sel = valid & (case == cs)
            if not sel.any():
                continue
            bx, by, bz = ix[sel], iy[sel], iz[sel]
            flat = (bx * G + by) * G + bz
            for ti, tri in enumerate(case_triangles(cs)):
                if FLIP[k] >> cs & 1:
                    tri = [tri[0], tri[2], tri[1]]
                pts = []
                for a, b in tri:
                    qa = (bx + PATHS[k, a, 0], by + PATHS[k, a, 1], bz + PATHS[k, a, 2])
                    qb = (bx + PATHS[k, b, 0], by + PATHS[k, b, 1], bz + PATHS[k, b, 2])
                    pa = np.stack([c[0][qa[0]], c[1][qa[1]], c[2][qa[2]]], 1)
                    pb = np.stack([c[0][qb[0]], c[1][qb[1]], c[2][qb[2]]], 1)
                    pts.append(edge_vertex(vsum[qa], weight[qa], vsum[qb], weight[qb], pa, pb))
                keys.append((flat * 6 + k) * 2 + ti)
                tris.append(np.stack(pts, 1))                                       # (n, 3 vertices, 3)
    if keys:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        order = np.argsort(keys, kind="stable")
        keys, tris = keys[order], tris[order]
    else:
        keys, tris = np.zeros(0, dtype=np.int64), np.zeros((0, 3, 3), dtype=F)
    total = len(keys)
    kept = total if face_cap is None else min(total, int(face_cap))
    verts = tris[:kept].reshape(-1, 3).astype(F)
    status = int(total > kept)
    if return_tags:
        tags = np.stack([keys[:kept] // 12, keys[:kept] // 2 % 6, keys[:kept] % 2], 1)
        return verts, total, status, tags
    return verts, total, status
