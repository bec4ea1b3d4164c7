"""The contract of the mesh maps (include/tgpose.h tgp_mesh_maps; DESIGN.md section 3 "Mesh maps and dense model-based tracking") on
its NumPy restatement tests/meshmaps_ref.py alone: what the rules give on the cases of tests/meshmaps_cases.py, what the maps are
geometrically, and how well dense projective ICP registers a frame against the map of a true mesh.  tests/test_meshmaps_gpu.py holds
the kernel to the same cases, byte for byte."""
import numpy as np
import pytest

from tests import icp_dense_cases as dc
from tests import icp_dense_ref as dr
from tests import icp_ref
from tests import meshmaps_cases as mc
from tests import meshmaps_ref as mr
from tests import raycast_ref as rr
from tests import render_ref
from tests.render_ref import pose34

F = np.float32
NAMES = sorted(mc.calls())


@pytest.mark.parametrize("name", ["one_cell", "partial_tiles", "cap_sweep", "coincident", "near_guard"])
def test_full_frame_window_is_the_renderer(name):
    """window (0, 0, 1, 1) with (h, w) = (H, W): K' is K in every bit, and z and face are render_ref's of the one-instance scene"""
    c, e = mc.calls()[name], mc.expected(name)
    assert c["window"].tolist() == [list(mc.FULL)] and mr.camera(c["camk"][0], c["window"][0]).tobytes() == c["camk"][0].tobytes()
    r = render_ref.render_scene(c["meshes"], [(0, 1, c["job_pose"][0])], c["camk"][0], c["h"], c["w"], c["near"])
    hit = r["face"] >= 0
    assert np.array_equal(e["face"][0], r["face"]) and e["count"][0] == hit.sum() > 0
    assert np.array_equal(e["z"][0][hit].view(np.int32), r["z"][hit].view(np.int32)) and (e["z"][0][~hit] == 0).all() and np.isinf(r["z"][~hit]).all()
    assert np.array_equal(e["depth"][0], r["depth"]) and e["dropped"][0] == r["dropped"].sum()


@pytest.mark.parametrize("name", NAMES)
def test_maps_are_the_surface(name):
    """every hit: pose @ vertex (float64) reprojects under K' to within 1/128 cell of its cell -- the vertex is the perspective-correct
    combination of the TRUE corners by the weights of the SNAPPED ones, and a corner snaps by at most 1/512 px, so 1/128 leaves the
    float32 arithmetic three quarters of the bound -- its camera z is within 1e-5 relative of the cell's z; normals are unit to 1e-6
    and, in face mode, look at the camera: cos(normal, ray to the vertex) <= the angle a 1/256 px step of the ray subtends + 1e-5 (the
    rule tests the ray through the cell, the check the ray to the vertex).  A miss is zeros; nothing is a NaN."""
    c, e = mc.calls()[name], mc.expected(name)
    for k in ("z", "vertex", "normal"):
        assert np.isfinite(e[k]).all(), k
    for j in range(len(c["job_img"])):
        hit = e["z"][j] > 0
        assert np.array_equal(hit, e["face"][j] >= 0) and hit.sum() == e["count"][j]
        assert not e["vertex"][j][~hit].any() and not e["normal"][j][~hit].any() and not e["depth"][j][~hit].any()
        if e["status"][j]:
            assert not hit.any()
        if not hit.any():
            continue
        Kp = mr.camera(c["camk"][c["job_img"][j]], c["window"][j]).astype(np.float64)
        T = c["job_pose"][j].astype(np.float64)
        rr_, cc = np.nonzero(hit)
        x = e["vertex"][j][hit].astype(np.float64) @ T[:, :3].T + T[:, 3]
        u, v = Kp[0] * x[:, 0] / x[:, 2] + Kp[2], Kp[1] * x[:, 1] / x[:, 2] + Kp[3]
        assert np.abs(u - cc).max() <= 1 / 128 and np.abs(v - rr_).max() <= 1 / 128, (name, j, np.abs(u - cc).max(), np.abs(v - rr_).max())
        z = e["z"][j][hit].astype(np.float64)
        assert (np.abs(x[:, 2] - z) <= 1e-5 * z).all(), (name, j)
        assert np.array_equal(e["depth"][j][hit], np.where(np.rint(e["z"][j][hit] * F(1000)) <= 65535, np.rint(e["z"][j][hit] * F(1000)), 0).astype(np.uint16))
        n = e["normal"][j][hit].astype(np.float64)
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-6
        if c["vnormals"] is None:
            m = n @ T[:, :3].T
            cos = (m * x).sum(1) / (np.linalg.norm(m, axis=1) * np.linalg.norm(x, axis=1))
            assert cos.max() <= 1 / (256 * min(abs(Kp[0]), abs(Kp[1]))) + 1e-5, (name, j, cos.max())


def test_rules_by_hand():
    e = {n: mc.expected(n) for n in NAMES}
    assert e["one_cell"]["count"].tolist() == [1] and e["one_cell"]["face"].tolist() == [[[0]]]
    assert e["no_sample"]["count"].tolist() == [0] and e["no_sample"]["dropped"].tolist() == [0] and (e["no_sample"]["face"] == -1).all()
    assert e["cap_sweep"]["count"].tolist() == [256] and len(np.unique(e["cap_sweep"]["face"])) > 1         # the front changes over the frame
    cs = mc.calls()["cap_sweep"]
    X, Y, _, flag = render_ref.project(cs["meshes"][0][0], cs["job_pose"][0], cs["camk"][0], cs["near"])
    x, y = X[cs["meshes"][0][1]], Y[cs["meshes"][0][1]]
    meets = (-((-x.min(1)) // 256) <= np.minimum(x.max(1) // 256, 15)) & (x.max(1) >= 0) & (-((-y.min(1)) // 256) <= np.minimum(y.max(1) // 256, 15)) & (y.max(1) >= 0)
    assert len(x) == 700 and not flag.any() and meets.sum() > 512                       # a sweep in mid-walk; 700 is no multiple of 256
    hit = e["coincident"]["face"][0] >= 0
    assert hit.sum() > 20 and (e["coincident"]["face"][0][hit] == 0).all()                                    # the lower index of the three
    for k in ("z", "vertex", "normal", "face", "depth"):
        assert e["windings"][k][0].tobytes() == e["windings"][k][1].tobytes(), k                             # the winding changes nothing
    assert e["windings"]["count"][0] > 20 and (e["windings"]["normal"][0][..., 2][e["windings"]["z"][0] > 0] < 0).all()
    assert e["near_guard"]["dropped"].tolist() == [2] and e["near_guard"]["count"][0] == e["coincident"]["count"][0]
    assert e["windows"]["count"][:2].min() > 1000 and e["windows"]["count"].tolist()[2:4] == [0, 0] and e["windows"]["count"][5] == 0
    assert e["windows"]["dropped"].tolist() == [0, 0, 80, 80, 0, 0] and e["windows"]["status"].tolist() == [0] * 6
    assert e["bad_index"]["status"].tolist() == [1, 1, 1, 1, 0] and e["bad_index"]["count"][:4].tolist() == [0] * 4 and e["bad_index"]["count"][4] > 100
    assert (e["three_jobs"]["count"] > 50).all() and e["three_jobs"]["status"].tolist() == [0, 0, 0]
    assert e["vertex_normals"]["count"][0] > 1000


def test_negative_step_mirrors_the_map():
    """window (44, 0, -1, 1) is the columns 44, 43, ...: the map of window (u0 - 47, 0, 1, 1) read from the right, in its hits"""
    c = mc.calls()["windows"]
    e = mc.expected("windows")
    flip = dict(c, window=np.array([[44.0 - 47.0, 0, 1, 1]], F), job_img=c["job_img"][:1], job_mesh=c["job_mesh"][:1], job_pose=c["job_pose"][:1])
    m = mc.run(flip)
    assert np.array_equal(e["face"][1] >= 0, m["face"][0][:, ::-1] >= 0)
    both = e["face"][1] >= 0
    assert np.abs(e["z"][1][both] - m["z"][0][:, ::-1][both]).max() <= 1e-6


def test_degenerate_sliver_is_a_miss_not_a_nan():
    """the rasteriser has a winner on the model-degenerate face 0 (its snapped area is not zero); the maps have a miss there, and the
    honest triangle behind it does not show through: the winner is resolved, not re-rendered"""
    c, e = mc.calls()["sliver"], mc.expected("sliver")
    v, f = c["meshes"][0]
    assert not np.cross(v[f[0, 1]] - v[f[0, 0]], v[f[0, 2]] - v[f[0, 0]]).any()                              # an exact zero in float32
    r = render_ref.render_scene(c["meshes"], [(0, 1, c["job_pose"][0])], c["camk"][0], c["h"], c["w"], c["near"])
    won = r["face"] == 0
    assert won.sum() == 1 and (r["face"] >= 0).all()
    assert (e["face"][0][won] == -1).all() and (e["z"][0][won] == 0).all() and e["count"][0] == c["h"] * c["w"] - 1
    assert (e["face"][0][~won] == 1).all()


def test_windows_follow_the_cube_rule():
    """a mesh whose bounding box IS a volume's cube gets the cube's window, bit for bit; a box behind the camera gets the NaN window"""
    meta = np.array([0.01, -0.02, 0.005, 0.004], F)
    G = 32
    halfe = F(G) * meta[3] * F(0.5)
    v = np.array([[meta[q] + (halfe if k >> (2 - q) & 1 else -halfe) for q in range(3)] for k in range(8)], F)
    meshes = [(v, np.array([[0, 1, 2]], np.int32))]
    K = np.array([[288.8, 288.8, 159.5, 119.5]], F)
    poses = np.stack([pose34(icp_ref.rot([1, 2, 3], 20.0), [0.02, 0.01, 0.5]), pose34(np.eye(3), [0, 0, 0.05]), pose34(np.eye(3), [0.3, 0, 0.4], 1.5)])
    got = mr.windows(meshes, K, [0, 0, 0], [0, 0, 5], poses, 96, 128, 240, 320)
    want = rr.windows(meta[None], G, K, [0, 0, 0], [0, 0, 0], poses, 96, 128, 240, 320)
    assert got.tobytes() == want.tobytes() and np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()
    assert mr.windows(meshes, K, [0], [0], poses[:1], 1, 1, 240, 320)[0, 2:].tolist() == [1.0, 1.0]


# measured on the restatement (this test's printed line): see the docstring
def test_object_accuracy_against_the_true_mesh():
    """tests/test_icp_dense_cpu.py's accuracy case -- the frame the fused two boxes show from a held-out pose, the start 5 degrees and
    10 mm off it, 60 x 80 maps, gate 20 mm -- with the maps made from the TRUE icp_ref.two_boxes mesh instead of the fused volume.
    The conditions are asserted; the error is recorded, not bounded (the frame is the VOLUME's surface, so the true mesh is registered
    to a surface that is not quite its own)."""
    c, truth, _ = dc.object_case()
    v, f = icp_ref.two_boxes()
    K, P = c["camk"], c["ref"]
    H, W = c["depth"].shape[1:]
    win = mr.windows([(v, f)], K, [0], [0], P, dc.OBJ_MAP_H, dc.OBJ_MAP_W, H, W)
    maps = mr.maps([(v, f)], K, [0], [0], P, win, dc.OBJ_MAP_H, dc.OBJ_MAP_W)
    rect = dr.rects(win, dc.OBJ_MAP_H, dc.OBJ_MAP_W, H, W)[0]
    r = dr.refine(c["depth"][0], K[0], dict(z=maps["z"][0], vertex=maps["vertex"][0], normal=maps["normal"][0]), win[0], P[0], rect, c["R"][0],
                  c["t"][0], c["s"][0], c["max_dist"][0], iters=50)
    err = icp_ref.pose_error(r["R64"], r["t64"], *truth)
    start = icp_ref.pose_error(c["R"][0], c["t"][0], *truth)
    print("true mesh: %d map hits, %d candidates, %d inliers, %d iterations; start %.3f deg %.3f mm; dense against the mesh %.4f deg %.4f mm"
          % (maps["count"][0], r["candidates"], r["inliers"], r["iters"], *start, *err))
    assert r["status"] == 0 and r["candidates"] >= 300 and 2 * r["inliers"] >= r["candidates"]
    assert abs(start[0] - 5.0) < 1e-3 and abs(start[1] - 10.0) < 1e-3
