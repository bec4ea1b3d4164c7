"""The restatement of the welded mesh and the vertex normals (tests/weld_ref.py) against the soup's restatement (tests/tsdf_ref.py
mesh) and against the properties a welded surface has: DESIGN.md section 3 "Indexed meshes from volumes".  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

from tests import tsdf_cases as tc
from tests import tsdf_ref as tr
from tests import weld_ref as wr


def test_the_tables_are_the_soup_kernels():
    """weld.hip carries the tetrahedron paths and the winding table as literals, as tsdf.hip does (tests/test_tsdf_cpu.py holds that
    copy against the derived tables): the two texts are equal"""
    from tests.util import ROOT
    found = []
    for name in ("tsdf.hip", "weld.hip"):
        src = open(os.path.join(ROOT, "tg-pose_amd", "csrc", name)).read()
        found.append((re.search(r"tsdf_flip\[6\]\s*=\s*\{([^}]*)\}", src).group(1), re.search(r"tsdf_path\[6\]\[4\]\s*=\s*\{(.*?)\};", src, re.S).group(1)))
    assert found[0] == found[1]
    assert tuple(int(w, 16) for w in found[1][0].split(",")) == tr.FLIP


def zero_pole():
    """sphere(16) with the sum of the voxel on its +x pole set to 0: outside, t = 0 on each of its cut edges"""
    vsum, weight, meta, q = tc.weak_corner(16)
    vsum = vsum.copy()
    vsum[q] = 0
    return vsum, tc.sphere(16)[1], meta


@functools.lru_cache(maxsize=None)
def welded(name):
    """the restatement's mesh of a named case, computed once and shared (do not write to it)"""
    vol = {"sphere16": lambda: tc.sphere(16), "sphere24": lambda: tc.sphere(24), "all_patterns": tc.all_patterns,
           "tail": tc.tail_volume, "zero_pole": zero_pole}[name]()
    return vol, wr.weld(*vol)


def same_soup(vol, out, **kw):
    soup, total, status = tr.mesh(*vol, **kw)
    assert out["verts"][out["faces"]].reshape(-1, 3).tobytes() == soup.tobytes()
    assert out["n_faces"] == len(soup) // 3 and (out["status"] & 1) == status
    return soup


@pytest.mark.parametrize("name", ["sphere16", "sphere24", "all_patterns", "tail"])
def test_soup_identity(name):
    vol, out = welded(name)
    soup = same_soup(vol, out)
    assert len(soup) > 0 and out["status"] == 0
    assert out["verts"].dtype == np.float32 and out["faces"].dtype == np.int32 and out["mask"].dtype == np.uint8
    assert (np.diff(out["keys"]) > 0).all()                                            # vertices ascend by name
    assert sorted(set(out["faces"].reshape(-1).tolist())) == list(range(out["n_verts"]))   # every vertex is used
    if name == "tail":                                                                   # all vertices at the end of the prefix sum
        assert out["keys"].min() // 8 >= 14 * 16 * 16


def test_soup_identity_weak_corner():
    vsum, weight, meta, q = tc.weak_corner()
    out = wr.weld(vsum, weight, meta, min_weight=3)
    same_soup((vsum, weight, meta), out, min_weight=3)
    assert out["n_faces"] < welded("sphere16")[1]["n_faces"] and out["n_verts"] < 1742
    _, _, count = wr.edges(out["faces"])
    assert count.min() == 1                                                              # the dropped cubes leave a hole


@pytest.mark.parametrize("k", range(6))
def test_soup_identity_one_tetrahedron(k):
    for case in range(16):
        vol = tc.one_tetrahedron(k, case)
        out = wr.weld(*vol)
        same_soup(vol, out)


def topology(faces, V):
    directed, und, count = wr.edges(faces)
    assert len(np.unique(directed, axis=0)) == len(directed)                             # every directed edge once
    return len(und), (count == 2).all(), V - len(und) + len(faces)


@pytest.mark.parametrize("name, V, Fc, E", [("sphere16", 1742, 3480, 5220), ("sphere24", 3878, 7752, 11628)])
def test_topology(name, V, Fc, E):
    _, out = welded(name)
    assert (out["n_verts"], out["n_faces"]) == (V, Fc)
    assert topology(out["faces"], V) == (E, True, 2)


def test_vertex_counts_and_position_uniqueness():
    assert welded("all_patterns")[1]["n_verts"] == 2432
    for name in ("sphere16", "sphere24", "all_patterns"):
        (vsum, weight, _), out = welded(name)
        assert not ((vsum == 0) & (weight > 0)).any()
        assert len(np.unique(out["verts"], axis=0)) == out["n_verts"], name
    vol, out = welded("zero_pole")
    same_soup(vol, out)
    assert out["n_verts"] == 1742 and len(np.unique(out["verts"], axis=0)) == 1739      # equal positions, different names


def sphere_normals(name):
    (_, _, meta), out = welded(name)
    ptr = lambda n: np.array([0, n])
    return out, wr.vertex_normals(out["verts"], out["faces"], ptr(out["n_verts"]), ptr(out["n_faces"]), [wr.volume_scale(meta[3])],
                                  return_sums=True)


@pytest.mark.parametrize("name, bound", [("sphere16", 0.98), ("sphere24", 0.99)])
def test_normals_on_the_sphere(name, bound):
    out, (normals, sums) = sphere_normals(name)
    v = out["verts"].astype(np.float64)
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert (np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1) < 1e-6).all()          # none is zero
    assert ((normals * radial).sum(1)).min() > bound
    assert 2.0 ** 30 < np.abs(sums).max() < 2.0 ** 34                                   # a face's cross product is about a voxel^2
    # the area-weighted normal in float64 without quantisation
    f = out["faces"].astype(np.int64)
    cross = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    acc = np.zeros_like(v)
    for j in range(3):
        np.add.at(acc, f[:, j], cross)
    acc /= np.linalg.norm(acc, axis=1, keepdims=True)
    assert np.abs(acc - normals).max() < 1e-5


def test_normals_of_an_unused_vertex_and_of_two_meshes():
    _, out = welded("sphere16")
    meta = tc.sphere(16)[2]
    verts = np.concatenate([out["verts"], [[9, 9, 9]], out["verts"][:3]]).astype(np.float32)
    faces = np.concatenate([out["faces"], [[0, 1, 2], [0, 1, 7]]]).astype(np.int32)      # the last one lies outside its mesh
    V, Fc = out["n_verts"], out["n_faces"]
    s = wr.volume_scale(meta[3])
    got = wr.vertex_normals(verts, faces, [0, V + 1, V + 4], [0, Fc, Fc + 2], [s, wr.extent_scale(verts[V + 1:])])
    alone = wr.vertex_normals(out["verts"], out["faces"], [0, V], [0, Fc], [s])
    assert got[:V].tobytes() == alone.tobytes() and got[V].tolist() == [0, 0, 0]
    assert got[V + 1].tobytes() == got[V + 2].tobytes() == got[V + 3].tobytes() and abs(np.linalg.norm(got[V + 1]) - 1) < 1e-6


def test_caps():
    vol, full = welded("sphere16")
    out = wr.weld(*vol, face_cap=1000)
    assert out["status"] == 1 and out["n_faces"] == 1000 and out["n_verts"] == 1742
    assert out["faces"].tobytes() == full["faces"][:1000].tobytes()
    same_soup(vol, out, face_cap=1000)
    out = wr.weld(*vol, vert_cap=1500)
    keep = (full["faces"] < 1500).all(1)
    assert out["status"] == 2 and out["n_verts"] == 1500 and 0 < keep.sum() < len(keep)
    assert out["faces"].tobytes() == full["faces"][keep].tobytes() and out["verts"].tobytes() == full["verts"][:1500].tobytes()
    out = wr.weld(*vol, vert_cap=1500, face_cap=2000)
    assert out["status"] == 3 and out["faces"].tobytes() == full["faces"][keep][:2000].tobytes()
    out = wr.weld(*vol, vert_cap=1742, face_cap=3480)
    assert out["status"] == 0 and out["faces"].tobytes() == full["faces"].tobytes()
    out = wr.weld(*vol, vert_cap=0, face_cap=0)
    assert out["status"] == 2 and out["n_verts"] == out["n_faces"] == 0               # every face names a vertex beyond the cap


@pytest.mark.parametrize("name, c, V, Fc, E", [("sphere16", 2, 146, 288, 432), ("sphere16", 4, 38, 72, 108), ("sphere24", 2, 326, 648, 972),
                                               ("sphere24", 4, 80, 156, 234)])
def test_clusters_on_the_sphere(name, c, V, Fc, E):
    vol, _ = welded(name)
    out = wr.weld(*vol, cluster=c)
    assert (out["n_verts"], out["n_faces"]) == (V, Fc)
    assert topology(out["faces"], V) == (E, True, 2)                                     # closed, every directed edge once, Euler 2
    assert (out["faces"][:, 0] < out["faces"][:, 1]).all() and (out["faces"][:, 0] < out["faces"][:, 2]).all()
    packed = (out["faces"].astype(np.int64) * [1 << 42, 1 << 21, 1]).sum(1)
    assert (np.diff(packed) > 0).all()                                                   # sorted by the rotated triple, no duplicate
    # the winding survives: the decimated normals still point outward
    normals = wr.vertex_normals(out["verts"], out["faces"], [0, V], [0, Fc], [wr.volume_scale(vol[2][3])])
    v = out["verts"].astype(np.float64)
    assert ((normals * v).sum(1) / np.linalg.norm(v, axis=1)).min() > 0.9


@pytest.mark.parametrize("name, c", [("sphere16", 2), ("sphere16", 4), ("sphere24", 2), ("sphere24", 8), ("all_patterns", 4), ("tail", 2)])
def test_cluster_representatives_lie_in_their_cells(name, c):
    (vsum, weight, meta), _ = welded(name)
    out = wr.weld(vsum, weight, meta, cluster=c)
    G = vsum.shape[0]
    voxel = float(meta[3])
    first = tr.centres(meta, G)[:, 0].astype(np.float64)
    lo = first + out["cell_lo"] * voxel
    slack = 2.0 ** -16 * voxel + np.spacing(np.abs(out["verts"]).astype(np.float32)).astype(np.float64)
    v = out["verts"].astype(np.float64)
    assert (v >= lo - slack).all() and (v <= lo + c * voxel + slack).all()


def test_cluster_duplicate_rule():
    vol, _ = welded("all_patterns")
    out = wr.weld(*vol, cluster=4)
    assert out["renamed"] == 64 and out["n_faces"] == 44
    # a pair of faces with opposite winding is kept: (a, b, c) and (a, c, b) are different rotated triples
    fake = dict(welded("sphere16")[1])
    fake["faces"] = np.concatenate([fake["faces"], fake["faces"][:, [0, 2, 1]]]).astype(np.int32)
    both = wr.decimate(fake, tc.sphere(16)[2], 16, 2)
    assert both["n_faces"] == 2 * 288 and both["renamed"] == 2 * wr.weld(*tc.sphere(16), cluster=2)["renamed"]
