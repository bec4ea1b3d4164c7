"""NumPy restatement of the welded marching-tetrahedra mesh and of the vertex normals (DESIGN.md section 3 "Indexed meshes from
volumes"; the kernels are csrc/weld.hip).  Written from the contract's text in include/tgpose.h, not from the kernels: a vertex is
named by the voxel edge it cuts, vertices are ranked by name, faces name vertices; the positions are tests/tsdf_ref.py's
edge_vertex, the triangles and their order tests/tsdf_ref.py's mesh.  Nothing here looks at a float to decide that two vertices are
one."""
import itertools

import numpy as np

from tests import tsdf_ref as tr

F = np.float32
CORNERS = list(itertools.product((0, 1), repeat=3))


def valid_cubes(weight, min_weight):
    """(G,G,G) bool: the cube whose origin is the voxel meshes (all eight corners seen min_weight times); False in the last rows"""
    G = weight.shape[0]
    n = G - 1
    seen = weight >= min_weight
    inner = np.ones((n, n, n), dtype=bool)
    for d in CORNERS:
        inner &= seen[d[0]:d[0] + n, d[1]:d[1] + n, d[2]:d[2] + n]
    out = np.zeros((G, G, G), dtype=bool)
    out[:n, :n, :n] = inner
    return out


def _at(a, step):
    """b[A] = a[A + step] per axis (step in {-1, 0, 1}^3), False where A + step is outside"""
    G = a.shape[0]
    out = np.zeros_like(a)
    dst = tuple(slice(max(0, -s), G - max(0, s)) for s in step)
    src = tuple(slice(max(0, s), G - max(0, -s)) for s in step)
    out[dst] = a[src]
    return out


def mark(vsum, weight, min_weight=1):
    """(G,G,G) uint8: bit d = dx << 2 | dy << 1 | dz of mask[A] is set iff the vertex (A, d) exists: the edge from A to A + d changes
    sign and at least one cube that holds both ends meshes"""
    inside = vsum < 0
    valid = valid_cubes(weight, min_weight)
    mask = np.zeros(vsum.shape, dtype=np.uint8)
    for d in range(1, 8):
        step = (d >> 2, d >> 1 & 1, d & 1)
        held = np.zeros(vsum.shape, dtype=bool)
        for o in CORNERS:                                   # the cube's origin is A - o: A where d steps, A or A - 1 elsewhere
            if not any(o[i] and step[i] for i in range(3)):
                held |= _at(valid, tuple(-x for x in o))
        exists = held & (inside != _at(inside, step))      # held is False where A + d is outside
        mask |= (exists.astype(np.uint8) << d).astype(np.uint8)
    return mask


def weld(vsum, weight, meta, min_weight=1, face_cap=None, vert_cap=None, cluster=1):
    """tgp_tsdf_weld_* on one volume: vsum, weight (G,G,G) int32, meta (4,) -> dict: verts (n_verts,3) float32, faces (n_faces,3)
    int32, n_verts, n_faces, status, mask (G^3) uint8, keys (n_verts) int64 (the vertices' names; with cluster > 1 the flat indices
    of the occupied cells)"""
    if cluster != 1:
        return decimate(weld(vsum, weight, meta, min_weight, face_cap, vert_cap), meta, vsum.shape[0], cluster)
    G = vsum.shape[0]
    c = tr.centres(meta, G)
    mask = mark(vsum, weight, min_weight)
    keys = np.nonzero(((mask.reshape(-1, 1) >> np.arange(8)) & 1).reshape(-1))[0].astype(np.int64)      # ascending flat(A) 8 + d
    flat, d = keys // 8, keys % 8
    A = (flat // (G * G), flat // G % G, flat % G)
    B = (A[0] + (d >> 2), A[1] + (d >> 1 & 1), A[2] + (d & 1))
    pa = np.stack([c[0][A[0]], c[1][A[1]], c[2][A[2]]], 1)
    pb = np.stack([c[0][B[0]], c[1][B[1]], c[2][B[2]]], 1)
    with np.errstate(all="ignore"):
        verts = tr.edge_vertex(vsum[A], weight[A], vsum[B], weight[B], pa, pb).astype(F).reshape(-1, 3)
    V = len(keys)

    n = G - 1
    ix, iy, iz = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    corner = lambda a, o: a[o[0]:o[0] + n, o[1]:o[1] + n, o[2]:o[2] + n]
    valid = valid_cubes(weight, min_weight)[:n, :n, :n]
    order, names = [], []
    for k in range(6):
        case = np.zeros((n, n, n), dtype=np.int64)
        for p in range(4):
            case |= (corner(vsum, tr.PATHS[k, p]) < 0).astype(np.int64) << p
        for cs in range(1, 15):
            sel = valid & (case == cs)
            if not sel.any():
                continue
            origin = np.stack([ix[sel], iy[sel], iz[sel]], 1)
            cube = (origin[:, 0] * G + origin[:, 1]) * G + origin[:, 2]
            for ti, tri in enumerate(tr.case_triangles(cs)):
                if tr.FLIP[k] >> cs & 1:
                    tri = [tri[0], tri[2], tri[1]]
                row = []
                for a, b in tri:                                                    # path corners, a earlier than b
                    qa = origin + tr.PATHS[k, a]
                    st = tr.PATHS[k, b] - tr.PATHS[k, a]
                    row.append(((qa[:, 0] * G + qa[:, 1]) * G + qa[:, 2]) * 8 + (st[0] << 2 | st[1] << 1 | st[2]))
                order.append((cube * 6 + k) * 2 + ti)
                names.append(np.stack(row, 1))
    if order:
        order, names = np.concatenate(order), np.concatenate(names)
        names = names[np.argsort(order, kind="stable")]
        faces = np.searchsorted(keys, names)
        assert (keys[np.minimum(faces, V - 1)] == names).all()                    # every face names a vertex that exists
    else:
        faces = np.zeros((0, 3), dtype=np.int64)
    vcap = V if vert_cap is None else int(vert_cap)
    faces = faces[(faces < vcap).all(1)]                                         # a face that names a vertex beyond the cap is dropped
    total = len(faces)
    kept = total if face_cap is None else min(total, int(face_cap))
    nv = min(V, vcap)
    return dict(verts=verts[:nv], faces=faces[:kept].astype(np.int32), n_verts=nv, n_faces=kept, status=int(total > kept) | 2 * int(V > vcap),
                mask=mask.reshape(-1), keys=keys[:nv])


def decimate(out, meta, G, c):
    """voxel clusters on weld's result: a vertex (A, d) belongs to cell A // c of a grid of side ceil(G / c); the occupied cells are
    numbered in ascending flat index; a cell's representative is the mean of its members in 2^-16 voxel fixed point; faces are
    renamed, those with two equal names dropped, the rest rotated to start at their smallest name, duplicates removed, sorted"""
    assert c in (2, 4, 8)
    side = -(-G // c)
    flat = out["keys"] // 8
    cell = ((flat // (G * G) // c) * side + flat // G % G // c) * side + flat % G // c
    occupied = np.unique(cell)
    number = np.searchsorted(occupied, cell)
    first = tr.centres(meta, G)[:, 0].astype(np.float64)                          # voxel 0's centre (float32) on each axis
    voxel = float(F(np.asarray(meta, dtype=F)[3]))
    offs = np.rint((out["verts"].astype(np.float64) - first) * (65536.0 / voxel)).astype(np.int64)
    sums = np.zeros((len(occupied), 3), dtype=np.int64)
    np.add.at(sums, number, offs)
    count = np.bincount(number, minlength=len(occupied)).astype(np.int64)
    rep = (first + ((sums.astype(np.float64) / count.astype(np.float64)[:, None]) * voxel) / 65536.0).astype(F).reshape(-1, 3)
    names = number[out["faces"].astype(np.int64)].reshape(-1, 3)
    names = names[(names[:, 0] != names[:, 1]) & (names[:, 1] != names[:, 2]) & (names[:, 2] != names[:, 0])]
    renamed = len(names)
    turn = (names.argmin(1)[:, None] + np.arange(3)[None]) % 3
    faces = np.unique(np.take_along_axis(names, turn, 1), axis=0) if renamed else names
    return dict(verts=rep, faces=faces.astype(np.int32), n_verts=len(occupied), n_faces=len(faces), status=out["status"], mask=out["mask"],
                keys=occupied, renamed=renamed, cell_lo=np.stack([occupied // (side * side), occupied // side % side, occupied % side], 1) * c)


def volume_scale(voxel):
    """the quantisation of a volume mesh's normals: 2^30 / voxel^2 in float64 on the float32 voxel edge"""
    v = float(F(voxel))
    return 2.0 ** 30 / (v * v)


def extent_scale(verts):
    """the quantisation of any other mesh's normals: 2^40 / (largest extent)^2 in float64 on the float32 extent"""
    e = float((verts.max(0) - verts.min(0)).astype(F).max())
    return 2.0 ** 40 / (e * e)


def vertex_normals(verts, faces, vptr, fptr, scale, return_sums=False):
    """tgp_mesh_vertex_normals on a packed set: verts (V,3) float32, faces (sum F,3) local to their mesh, vptr / fptr (M+1), scale (M)
    float64 -> (V,3) float32"""
    verts = np.ascontiguousarray(verts, dtype=F)
    sums = np.zeros((len(verts), 3), dtype=np.int64)
    for m in range(len(vptr) - 1):
        v = verts[vptr[m]:vptr[m + 1]]
        f = np.asarray(faces[fptr[m]:fptr[m + 1]], dtype=np.int64)
        f = f[((f >= 0) & (f < len(v))).all(1)]
        p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        with np.errstate(all="ignore"):
            u, w = p1 - p0, p2 - p0
            cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                              u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1).astype(F)
            q = cross.astype(np.float64) * np.float64(scale[m])
            q = np.rint(np.where(np.abs(q) < 4.0e15, q, 0.0)).astype(np.int64)
        part = sums[vptr[m]:vptr[m + 1]]
        for j in range(3):
            np.add.at(part, f[:, j], q)
    s = sums.astype(np.float64)
    zero = (sums == 0).all(1)
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    out = np.where(zero[:, None], 0.0, s / np.where(zero, 1.0, length)[:, None]).astype(F)
    return (out, sums) if return_sums else out


def edges(faces):
    """(directed (3 F,2), undirected sorted unique (E,2), each undirected edge's face count (E))"""
    f = np.asarray(faces, dtype=np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, count = np.unique(np.sort(directed, 1), axis=0, return_counts=True)
    return directed, und, count
