"""The NumPy restatement of TSDF fusion and marching tetrahedra (tests/tsdf_ref.py) against what the contract promises (DESIGN.md
section 3 "Models from depth sequences"): a closed, outward, well-placed surface for the analytic sphere, every tetrahedron case by
hand, the cube and cap rules, each rule of the fusion on exact voxel centres, and the fusion's quality on rendered frames, measured.
No GPU; tests/test_tsdf_gpu.py holds the kernels against the same restatement, byte for byte."""
import os
import re

import numpy as np
import pytest

from tests import tsdf_cases as tc
from tests import tsdf_ref as tr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def triangles(verts):
    return verts.astype(np.float64).reshape(-1, 3, 3)


def normals(tri):
    return np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])


# ------------------------------------------------------------------------------------------------------------------ the sphere
@pytest.mark.parametrize("G,faces", [(16, 3480), (24, 7752)])
def test_analytic_sphere(G, faces):
    vsum, weight, meta = tc.sphere(G)
    verts, total, status = tr.mesh(vsum, weight, meta)
    assert total == faces and status == 0 and verts.shape == (3 * faces, 3) and verts.dtype == F
    tri = triangles(verts)
    nrm = normals(tri)
    assert (np.linalg.norm(nrm, axis=1) > 0).all()                                   # no degenerate triangle
    # welded by bit pattern: every directed edge once, and its reverse once -- a closed, consistently wound surface
    _, ids = np.unique(verts.view(np.uint32), axis=0, return_inverse=True)
    f = ids.reshape(-1, 3)
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    keys, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 1).all()
    assert {tuple(e) for e in keys.tolist()} == {tuple(e) for e in keys[:, ::-1].tolist()}
    off = np.abs(np.linalg.norm(verts.astype(np.float64), axis=1) - 0.4) / float(meta[3])
    print("G = %d: the worst vertex is %.4f voxel off the sphere" % (G, off.max()))
    assert off.max() < 0.1
    assert ((nrm * tri.mean(1)).sum(1) > 0).all()                                    # every normal points away from the centre


# ------------------------------------------------------------------------------------------------------------------ the cases
def test_flip_table_is_the_kernels():
    """the kernel carries the winding table and the tetrahedron paths as literals: they are the derived ones"""
    src = open(os.path.join(ROOT, "tg-pose_amd", "csrc", "tsdf.hip")).read()
    flip = re.search(r"tsdf_flip\[6\]\s*=\s*\{([^}]*)\}", src).group(1)
    assert tuple(int(w, 16) for w in flip.split(",")) == tr.FLIP
    path = re.search(r"tsdf_path\[6\]\[4\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    codes = np.array([int(x) for x in re.findall(r"\d+", path)]).reshape(6, 4)
    assert np.array_equal(codes, tr.PATHS[:, :, 0] * 4 + tr.PATHS[:, :, 1] * 2 + tr.PATHS[:, :, 2])
    assert [tuple(np.argmax(np.diff(tr.PATHS[k], axis=0), axis=1)) for k in range(6)] == tr.PERMS


def by_hand_vertex(vsum, weight, meta, qa, qb):
    """the contract's vertex on the edge of voxels qa, qb, scalar by scalar, from the end with the smaller flat index"""
    G = vsum.shape[0]
    flat = lambda q: (q[0] * G + q[1]) * G + q[2]
    a, b = (qa, qb) if flat(qa) < flat(qb) else (qb, qa)
    centre = lambda q: [F(meta[k]) + ((F(q[k]) + F(0.5)) - F(G // 2)) * F(meta[3]) for k in range(3)]
    fa, fb = F(vsum[a]) / F(weight[a]), F(vsum[b]) / F(weight[b])
    t = fa / (fa - fb)
    return np.array([pa + t * (pb - pa) for pa, pb in zip(centre(a), centre(b))], dtype=F)


@pytest.mark.parametrize("k", range(6))
def test_every_tetrahedron_case(k):
    differs = 0
    for case in range(1, 15):
        vsum, weight, meta = tc.one_tetrahedron(k, case)
        verts, total, status, tags = tr.mesh(vsum, weight, meta, return_tags=True)
        G = vsum.shape[0]
        assert (tags[:, 0] == (tc.CUBE_AT[0] * G + tc.CUBE_AT[1]) * G + tc.CUBE_AT[2]).all() and status == 0
        assert np.array_equal(tags, tags[np.lexsort((tags[:, 2], tags[:, 1], tags[:, 0]))])     # cube, tetrahedron, triangle
        mine = tags[:, 1] == k
        n_in = bin(case).count("1")
        assert mine.sum() == (2 if n_in == 2 else 1), (k, case)
        corner = lambda c: tuple(np.add(tc.CUBE_AT, tr.PATHS[k, c]))
        ins = [corner(c) for c in range(4) if case >> c & 1]
        outs = [corner(c) for c in range(4) if not case >> c & 1]
        pos = lambda q: np.array([tr.centres(meta, G)[a][q[a]] for a in range(3)], dtype=np.float64)
        toward = np.mean([pos(q) for q in outs], 0) - np.mean([pos(q) for q in ins], 0)
        tri = triangles(verts)[mine]
        assert ((normals(tri) * toward).sum(1) > 0).all(), (k, case)
        # each vertex is the by-hand vertex of one inside-outside edge, bit for bit; from the other end it would often differ
        hand = {(i, o): by_hand_vertex(vsum, weight, meta, i, o) for i in ins for o in outs}
        for v in verts.reshape(-1, 3, 3)[mine].reshape(-1, 3):
            assert any(v.tobytes() == h.tobytes() for h in hand.values()), (k, case)
        used = {next(e for e, h in hand.items() if h.tobytes() == v.tobytes()) for v in verts.reshape(-1, 3, 3)[mine].reshape(-1, 3)}
        assert len(used) == (4 if n_in == 2 else 3)
        flat = lambda q: (q[0] * G + q[1]) * G + q[2]
        c = tr.centres(meta, G)
        for (i, o) in hand:
            a, b = (i, o) if flat(i) > flat(o) else (o, i)                          # the WRONG end first
            fa, fb = F(vsum[a]) / F(weight[a]), F(vsum[b]) / F(weight[b])
            t = fa / (fa - fb)
            wrong = np.array([c[x][a[x]] + t * (c[x][b[x]] - c[x][a[x]]) for x in range(3)], dtype=F)
            differs += wrong.tobytes() != hand[(i, o)].tobytes()
    assert differs > 0            # the rule is not idle: the other end gives other bits somewhere


def test_all_corner_patterns_are_closed_between_tetrahedra():
    """all 256 corner patterns: inside a cube the six tetrahedra's pieces fit -- every edge that is not on the cube's faces is
    shared by two triangles of opposite direction (the split and the winding table agree with each other)"""
    vsum, weight, meta = tc.all_patterns()
    verts, total, status, tags = tr.mesh(vsum, weight, meta, return_tags=True)
    assert total == len(tags) > 0 and status == 0
    assert len(np.unique(tags[:, 0])) == 254                                      # all but the all-inside and all-outside cubes
    c = tr.centres(meta, vsum.shape[0]).astype(np.float64)
    G = vsum.shape[0]
    for cube in np.unique(tags[:, 0])[::7]:
        ix, iy, iz = cube // (G * G), cube // G % G, cube % G
        v = verts[np.repeat(tags[:, 0] == cube, 3)]
        _, ids = np.unique(v.view(np.uint32), axis=0, return_inverse=True)
        f = ids.reshape(-1, 3)
        edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        uniq = {tuple(e) for e in edges.tolist()}
        assert len(uniq) == len(edges)                                            # no directed edge twice
        lo, hi = np.array([c[0][ix], c[1][iy], c[2][iz]]), np.array([c[0][ix + 1], c[1][iy + 1], c[2][iz + 1]])
        pts = np.zeros((ids.max() + 1, 3))
        pts[ids.reshape(-1)] = v.astype(np.float64)
        for a, b in uniq:
            on_face = (np.isclose(pts[a], lo) & np.isclose(pts[b], lo)).any() or (np.isclose(pts[a], hi) & np.isclose(pts[b], hi)).any()
            assert on_face or (b, a) in uniq, (cube, a, b)


# ------------------------------------------------------------------------------------------------------------------ cubes and caps
def test_cube_validity_and_caps():
    vsum, weight, meta, q = tc.weak_corner()
    full, total, status, tags = tr.mesh(vsum, weight, meta, min_weight=1, return_tags=True)
    assert total == 3480
    G = vsum.shape[0]
    around = [((q[0] - a) * G + q[1] - b) * G + q[2] - c for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    lost = np.isin(tags[:, 0], around)
    assert lost.sum() > 0
    verts3, total3, status3 = tr.mesh(vsum, weight, meta, min_weight=3)
    assert total3 == total - lost.sum() and status3 == 0
    assert verts3.tobytes() == full.reshape(-1, 3, 3)[~lost].tobytes()               # the other cubes' triangles, unchanged
    one = np.zeros((16, 16, 16), np.int32)
    one[:2, :2, :2] = -5
    one[0, 0, 0] = 5
    w = np.ones_like(one)
    assert tr.mesh(one, w, meta)[1] > 0
    w[1, 1, 1] = 0
    w2 = np.where(np.arange(16)[:, None, None] < 2, w, 0) * (np.arange(16)[None, :, None] < 2) * (np.arange(16)[None, None, :] < 2)
    assert tr.mesh(one, w2.astype(np.int32), meta)[1] == 0                           # a corner below min_weight: nothing
    empty = np.zeros((16, 16, 16), np.int32)
    verts0, total0, status0 = tr.mesh(empty, empty, meta)
    assert total0 == 0 and status0 == 0 and verts0.shape == (0, 3)
    capped, totalc, statusc = tr.mesh(vsum, weight, meta, face_cap=total - 1)
    assert totalc == total and statusc == 1 and capped.tobytes() == full[:-3].tobytes()
    exact, _, statuse = tr.mesh(vsum, weight, meta, face_cap=total)
    assert statuse == 0 and exact.tobytes() == full.tobytes()
    tail = tc.tail_volume()
    _, totalt, _, tagst = tr.mesh(*tail, return_tags=True)
    assert totalt > 0 and (tagst[:, 0] // (16 * 16) == 14).all()


# ------------------------------------------------------------------------------------------------------------------ the fusion's rules
def test_integrate_rules():
    case = tc.rules()
    vsum, weight, status = tc.fused("rules")
    name = {n: k for k, n in enumerate(tc.RULE_JOBS)}
    vol = lambda n: case["job_model"][name[n]]
    assert status.tolist() == [0] * 11 + [1] * 4
    inv = F(1024.0 / float(F(case["trunc"])))
    # base: p_z = 1 + k/128 with k = 2 iz - 15; sdf = -7.8125 k
    s, w = vsum[vol("base")], weight[vol("base")]
    assert (w[:, :, :10] == 1).all() and (w[:, :, 10:] == 0).all()                   # k = 3 (iz 9) is exactly -trunc: kept; k = 5: skipped
    assert (s[:, :, 9] == int(np.rint(-F(case["trunc"]) * inv))).all() and (s[:, :, 9] < -1000).all()
    assert (s[:, :, :7] == 1024).all() and (s[:, :, 7] == int(np.rint(F(7.8125) * inv))).all()   # sdf >= trunc from k = -3 down
    # near: p_z = k/128: the layers k <= 1 are skipped, k = 3 is kept wherever its pixel is in the frame
    w = weight[vol("near")]
    assert (w[:, :, :9] == 0).all() and w[:, :, 9].sum() > 0 and w[:, :, 9].sum() < 256
    # the four sides: the cube straddles the edge: some voxels of every z layer in front are kept, not all
    for side in ("left", "right", "top", "bottom"):
        w = weight[vol(side)][:, :, :10]
        assert 0 < w.sum() < w.size, side
    assert weight[vol("left")][:8].sum() == 0 or weight[vol("left")][8:].sum() > weight[vol("left")][:8].sum()
    # zero depth and the mask: both on frame 1, together they miss what each misses
    wz, wm = weight[vol("zero")], weight[vol("mask")]
    unmasked = tc.fused("rules", False)[1]
    assert np.array_equal(unmasked[vol("zero")], unmasked[vol("mask")]) and wz.sum() > 0 and wm.sum() > 0
    assert np.array_equal(wz + wm, unmasked[vol("zero")])                            # every kept pixel carries one of the two bytes
    assert unmasked[vol("zero")][7, 7].sum() == 0 and weight[vol("base")][7, 7, 0] == 1   # pixel (32, 24) is in the zero block
    # half: the voxels with p_x = p_y = 0 (ix = iy = 7) read pixel (32, 24), not (33, 23) or (32, 23)
    d = case["depth"][2]
    assert d[24, 32] != d[23, 33] and d[24, 32] != d[23, 32] and d[24, 32] != d[24, 33]
    iz = 3
    pz = F(1) + F((2 * iz - 15) / 128.0)
    want = int(np.rint(np.minimum(F(d[24, 32]) - pz * F(1000), F(case["trunc"])) * inv))
    assert weight[vol("half")][7, 7, iz] == 1 and vsum[vol("half")][7, 7, iz] == want
    # a NaN pose adds nothing; the ignored jobs added nothing to volume 0 beyond the base job
    assert weight[vol("nan_x")].sum() == 0 and vsum[vol("nan_x")].any() == 0
    alone = tc.fuse(case, [name["base"]])
    assert np.array_equal(alone[0][0], vsum[0]) and np.array_equal(alone[1][0], weight[0])


def test_integrate_adds_and_ignores_order():
    case = tc.several(16)
    vsum, weight, status = tc.fused("several16")
    assert status.tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert all(weight[m].max() >= 1 for m in range(3)) and weight[0].max() == 2       # two jobs on volume 0
    a, b = tc.fuse(case, [0]), tc.fuse(case, [1])
    assert np.array_equal(a[0][0] + b[0][0], vsum[0]) and np.array_equal(a[1][0] + b[1][0], weight[0])
    back = tc.fuse(case, list(range(7))[::-1])
    assert np.array_equal(back[0], vsum) and np.array_equal(back[1], weight)
    two = tc.fuse(case, [0, 2, 4, 6])
    tc.fuse(case, [1, 3, 5], volumes=two[:2])
    assert np.array_equal(two[0], vsum) and np.array_equal(two[1], weight)
    plain = tc.fused("several16", False)
    assert plain[1].sum() > weight.sum()                                              # the mask took pixels away


# ------------------------------------------------------------------------------------------------------------------ the quality
QUALITY_G, QUALITY_H, QUALITY_W = 32, 120, 160


def fuse_turntable():
    from tests import render_ref as rr
    v, f = tc.turntable_mesh()
    camk = np.array([140, 140, 79.5, 59.5], dtype=F)
    poses = [rr.pose34(*tc.turntable_pose(k), s=tc.TURN_SCALE) for k in range(tc.TURN_FRAMES)]
    depth = np.stack([rr.render_scene([(v, f)], [(0, 1, p)], camk, QUALITY_H, QUALITY_W)["depth"] for p in poses])
    meta = tr.tsdf_meta((v.max(0).astype(np.float64) + v.min(0)) / 2, v.max(0) - v.min(0), QUALITY_G)
    vsum, weight = np.zeros((1,) + (QUALITY_G,) * 3, np.int32), np.zeros((1,) + (QUALITY_G,) * 3, np.int32)
    trunc = 2000.0 * float(meta[3]) * tc.TURN_SCALE
    tr.integrate(vsum, weight, meta[None], depth, np.tile(camk, (len(poses), 1)), np.arange(len(poses)), np.zeros(len(poses), np.int64),
                 np.stack(poses), trunc)
    verts, total, _ = tr.mesh(vsum[0], weight[0], meta)
    return v, f, meta, verts, total


def test_fusion_quality_measured():
    """a bottle rendered by tests/render_ref.py at 160 x 120 from 12 turntable poses, fused at G = 32 with the true poses and
    meshed (truncation: two voxels): the largest distance of a mesh vertex from the true surface, in voxels.  Measured with this
    restatement: 0.590 voxel; the bound is that x 1.5, and a restatement above one voxel would mean the case or the rule is wrong.
    (A truncation of three voxels measures 1.94: the bottle's neck is 3.3 voxels thick, and behind a part thinner than the
    truncation the far side's free space is taken for inside.  That is the rule's known limit, and why scan's default is two.)"""
    v, f, meta, verts, total = fuse_turntable()
    assert total > 1000
    worst = tc.surface_distance(verts, v, f).max() / float(meta[3])
    print("fusion quality: %d triangles, the worst vertex %.4f voxel from the true surface" % (total, worst))
    assert worst < 1.0
    assert worst <= QUALITY_BOUND


QUALITY_BOUND = 1.5 * 0.590
