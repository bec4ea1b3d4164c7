"""The distance-field pose search without a GPU: the NumPy restatement (tests/search_ref.py) against a float64 statement with no grid,
the view sampler against what the reference returns (tests/golden/view_sampler_ref.npz), the pose formula, and the wrappers'
refusals that need no device."""
import os

import numpy as np
import pytest

from tests import search_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32


def view_sampler():
    from tgpose_amd.tools.lynne_lib import view_sampler as vs
    return vs


def lattice_model(G, seed, n=60):
    """a model whose points sit on voxel centres of its own cube: two corner points fix the bounding box (so centre and voxel),
    the rest are centres ctr + (i - G/2 + 0.5) voxel of random voxels i -> (points (n+2,3) float32, i (n,3), meta)"""
    r = np.random.RandomState(seed)
    corners = np.array([[-0.45, -0.3, -0.35], [0.4, 0.35, 0.3]], dtype=f32)
    meta, _ = sr.field_meta(corners, G, 32)
    i = r.randint(3, G - 3, (n, 3))
    pts = (meta[:3].astype(np.float64) + (i - G / 2 + 0.5) * np.float64(meta[3])).astype(f32)
    pts = pts[(np.abs(pts - meta[:3]) < 0.29).all(1)]              # inside the corners' box: the box, so the cube, stays
    i = i[:0] if len(pts) == 0 else np.floor((pts.astype(np.float64) - meta[:3]) / np.float64(meta[3]) + G / 2).astype(np.int64)
    return np.concatenate([corners, pts]), i, meta


def test_restatement_against_the_float64_statement():
    """tiny case: G = 16, 30 points, 6 rotations, K = 1 with stride 4 (27 shifts).  Per point the two statements differ by at most 4
    levels (search_ref.brute's docstring) wherever both see the point inside the cube or both outside; a point within 1e-4 voxel of
    a cube face may be seen differently by float32 and float64, none is here (asserted).  So |cost - brute| <= 4 n everywhere, and
    where the float64 winner of a rotation leads by more than 8 n, the restatement's winner is the same shift."""
    vs = view_sampler()
    G, cap, K, stride = 16, 32, 1, 4
    r = np.random.RandomState(3)
    y = (r.uniform(-0.5, 0.5, (30, 3)) * [1.0, 0.7, 0.8]).astype(f32)
    field, meta, thr = sr.build_field(y, G, cap)
    Rs = vs.rotation_grid(12, 2)[[0, 5, 9, 13, 18, 23]]
    s, t = 0.12, np.array([0.05, -0.1, 0.7])
    cloud = (s * y.astype(np.float64) @ Rs[2].astype(np.float64).T + t).astype(f32)
    anchor = (s * Rs[2].astype(np.float64) @ (meta[:3] + np.array([4, 0, -4]) * np.float64(meta[3])) + t).astype(f32)
    n = len(cloud)
    want = sr.brute(y, meta, cap, G, cloud, n, anchor, s, Rs, K, stride)
    b, live = sr.bases(cloud, n, anchor, s, meta[3], G, Rs)
    assert live.all()
    q = np.stack([(cloud.astype(np.float64) - anchor) @ R.astype(np.float64) / (s * np.float64(meta[3])) + G / 2 for R in Rs])
    assert (np.abs(q - np.round(q)) > 1e-4).all() and np.array_equal(b, np.floor(q).astype(np.int64))
    got = np.stack([sr.rotation_costs(field, cap, b[k], live, K, stride) for k in range(len(Rs))])
    print("largest |restatement - float64| cost %d of the allowed %d; costs %d..%d" % (np.abs(got - want).max(), 4 * n, got.min(), got.max()))
    assert (np.abs(got - want) <= 4 * n).all()
    decided = 0
    for k in range(len(Rs)):
        order = np.sort(want[k])
        if order[1] - order[0] > 8 * n:
            decided += 1
            assert got[k].argmin() == want[k].argmin(), k
    assert decided >= 1 and want[2].argmin() == got[2].argmin()
    # the true rotation at the true shift (index of d = (4, 0, -4) = stride (1, 0, -1)) is the overall winner of both
    true_shift = ((1 + K) * 3 + (0 + K)) * 3 + (-1 + K)
    assert np.unravel_index(got.argmin(), got.shape) == (2, true_shift) == np.unravel_index(want.argmin(), want.shape)


def test_field_levels():
    """the byte is the number of thresholds reached: 0 at a voxel whose centre is a model point, rising by about 4 a voxel, cap far away"""
    pts, i, meta = lattice_model(16, 0)
    field, meta2, thr = sr.build_field(pts, 16, 32)
    assert np.array_equal(meta, meta2) and (np.diff(thr) > 0).all() and thr[0] == f32((np.float64(meta[3]) / 4.0) ** 2)
    assert len(i) >= 20 and (field[i[:, 0], i[:, 1], i[:, 2]] == 0).all()
    c = meta[:3].astype(np.float64) + (np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1) - 8 + 0.5) * np.float64(meta[3])
    dist = np.sqrt(((c[..., None, :] - pts.astype(np.float64)) ** 2).sum(-1)).min(-1)
    quarters = 4.0 * dist / np.float64(meta[3])
    exact = np.minimum(np.floor(quarters), 32)
    # lattice points lie whole voxels apart, so many distances sit ON a threshold: there float32 may fall on either side
    on_edge = np.abs(quarters - np.round(quarters)) < 1e-4
    assert np.array_equal(field[~on_edge], exact[~on_edge]) and np.abs(field.astype(np.int64) - exact).max() <= 1 and (~on_edge).mean() > 0.5
    few, _, _ = sr.build_field(pts, 16, 8)
    assert np.array_equal(few, np.minimum(field, 8))


@pytest.mark.parametrize("G,K,stride,d", [(16, 2, 1, (2, -1, 1)), (32, 1, 3, (-3, 3, 0)), (48, 0, 1, (0, 0, 0))])
def test_an_exact_image_costs_nothing_and_its_pose_comes_back(G, K, stride, d):
    vs = view_sampler()
    pts, i, meta = lattice_model(G, G)
    field, _, _ = sr.build_field(pts, G, 32)
    Rs = vs.rotation_grid(12, 3)
    r, s, t = 17, 0.2, np.array([-0.1, 0.05, 0.9])
    R = Rs[r].astype(np.float64)
    y = pts[2:].astype(np.float64)
    cloud = np.full((len(y) + 3, 3), np.nan, dtype=f32)           # two NaN rows inside, a row of rubbish behind the count
    cloud[[0, 5]] = np.nan
    rows = [k for k in range(len(y) + 2) if k not in (0, 5)]
    cloud[rows] = (s * y @ R.T + t).astype(f32)
    cloud[-1] = 3.0
    anchor = (s * R @ (meta[:3].astype(np.float64) + np.array(d) * np.float64(meta[3])) + t).astype(f32)
    out = sr.search(field, meta, 32, cloud, len(y) + 2, anchor, s, Rs, K, stride, 5)
    side = 2 * K + 1
    shift = ((d[0] // stride + K) * side + (d[1] // stride + K)) * side + (d[2] // stride + K)
    assert out["table"][r].tolist() == [0, shift]
    assert out["cost"][0] == 0 and out["rot"][0] == r and out["shift"][0] == shift and (out["cost"][1:] >= 0).all()
    assert np.array_equal(sr.shifts(K, stride)[shift], d)
    P = out["poses"][0].astype(np.float64)
    assert np.array_equal(out["poses"][0][:, :3], Rs[r])
    moved = s * y @ P[:, :3].T + P[:, 3]
    assert np.abs(moved - cloud[rows].astype(np.float64)).max() < s * np.float64(meta[3])        # within one voxel (in fact ~1e-7)
    assert np.abs(P[:, 3] - t).max() < 1e-6
    # selection: least (cost, r), refused rows behind R
    few = sr.search(field, meta, 32, cloud, len(y) + 2, anchor, s, Rs[:3], K, stride, 5)
    assert (few["cost"][3:] == sr.REFUSED).all() and (few["rot"][3:] == -1).all() and np.isnan(few["poses"][3:]).all()
    assert sorted(few["rot"][:3].tolist()) == [0, 1, 2] and (np.diff(few["cost"][:3]) >= 0).all()
    bad = sr.search(field, meta, 32, cloud, len(cloud) + 1, anchor, s, Rs[:3], K, stride, 2)
    assert (bad["table"][:, 0] == sr.REFUSED).all() and (bad["cost"] == sr.REFUSED).all()


def test_view_sampler_against_the_golden():
    vs = view_sampler()
    g = np.load(os.path.join(HERE, "golden", "view_sampler_ref.npz"))
    for n in (12, 42, 162):
        pts, level = vs.hinter_sampling(n)
        assert isinstance(pts, np.ndarray) and pts.dtype == np.float64 and isinstance(level, list)
        assert pts.shape == (n, 3) and np.abs(pts - g["pts.%d" % n]).max() <= 1e-12 and level == g["level.%d" % n].tolist()
        assert np.abs(np.linalg.norm(pts, axis=1) - 1.0).max() < 1e-12
        views, level2 = vs.sample_views(n)
        assert isinstance(views, list) and len(views) == n and level2 == level and set(views[0]) == {"R", "t"}
        R, t = np.stack([v["R"] for v in views]), np.stack([v["t"] for v in views])
        assert t.shape == (n, 3, 1) and np.abs(R - g["R.%d" % n]).max() <= 1e-12 and np.abs(t - g["t.%d" % n]).max() <= 1e-12
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1.0).max() < 1e-12
    assert len(vs.hinter_sampling(13)[0]) == 42 and np.abs(np.linalg.norm(vs.hinter_sampling(12, radius=2.5)[0], axis=1) - 2.5).max() < 1e-12
    upper, _ = vs.sample_views(42, elev_range=(0, 0.5 * np.pi))
    assert 0 < len(upper) < 42 and all(-v["R"].T.dot(v["t"])[2, 0] >= -1e-12 for v in upper)      # the camera centres lie above z = 0


def test_rotation_grid():
    vs = view_sampler()
    views, _ = vs.sample_views(42)
    Rs = vs.rotation_grid(42, 12)
    assert Rs.shape == (504, 3, 3) and Rs.dtype == np.float32
    R64 = Rs.astype(np.float64)
    assert np.abs(R64 @ R64.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(R64) - 1.0).max() < 1e-6
    for v in (0, 7, 41):                                           # views outer: v * 12 + k = Rz(30 k degrees) R_v
        assert np.array_equal(Rs[v * 12], views[v]["R"].astype(f32))
        for k in (1, 5, 11):
            a = 2.0 * np.pi * k / 12
            Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            assert np.abs(R64[v * 12 + k] - Rz @ views[v]["R"]).max() < 1e-6
    assert vs.rotation_grid(12, 1).shape == (12, 3, 3)
    d = np.abs(R64[:, None] - R64[None]).max((2, 3)) + np.eye(504)
    assert d.min() > 1e-3                                          # no rotation twice
    with pytest.raises(ValueError):
        vs.rotation_grid(12, 0)


def test_host_meta_is_the_restatement_s():
    from tgpose_amd import ops
    r = np.random.RandomState(5)
    for G in (16, 32, 48):
        pts = (r.randn(77, 3) * [0.3, 0.1, 0.2] + [0.5, -1.0, 2.0]).astype(f32)
        a, b = ops.field_meta(pts, G, 32), sr.field_meta(pts, G, 32)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == f32 and a[1].dtype == f32
        lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
        assert np.allclose(a[0][:3], (lo + hi) / 2, atol=1e-6) and np.isclose(a[0][3] * G / 2, 0.575 * (hi - lo).max(), rtol=1e-6)
    assert np.array_equal(ops.search_shifts(2, 3).numpy(), sr.shifts(2, 3))


def test_wrapper_refusals_without_a_device():
    from tgpose_amd import ops, pose
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    with pytest.raises(TypeError, match="IcpModels"):
        ops.DistanceFields(np.zeros((1, 8, 6), f32))
    with pytest.raises(TypeError, match="DistanceFields"):
        ops.pose_search(None, None, None, None, None, None, None)
    with pytest.raises(TypeError, match="DistanceFields"):
        pose.ModelSearch(None, None, np.eye(3, dtype=f32)[None])
    assert ops.SEARCH_MAX_POINTS == 1024 and ops.SEARCH_MAX_TOP == 64 and ops.SEARCH_GRIDS == (16, 32, 48) and ops.SEARCH_REFUSED == sr.REFUSED
    assert callable(myEvaluater.acquire_models)


def test_the_restated_chain_finds_the_hardest_object():
    """search_ref + icp_ref + verify_ref on the recorded plane-cut, segmented 128-point cloud of the second object of
    icp_ref.table_scene frame 0 (tests/golden/acquire_models_ref.npz; scripts/search_chain_check.py runs all six): the chain of
    tests/test_acquire_models_gpu.py with its parameters ends within 2 degrees / 2 mm, from a candidate that is not rank 0"""
    from tests import icp_ref, plane_cases as pc
    vs = view_sampler()
    d = np.load(os.path.join(HERE, "golden", "acquire_models_ref.npz"))
    slot = d["obj.0"].tolist().index(1)
    assert np.array_equal(d["meta"], sr.field_meta(d["model"][:, :3], 32, 32)[0])
    best = sr.acquire_chain(d["field"], d["meta"], 32, d["model"], pc.meshes()[0], d["clouds.0"][slot], icp_ref.OBJECTS[1]["s"], vs.rotation_grid(42, 12),
                            5, 2, 16, 0.01, d["cut.0"], pc.CAMK, 5, mask=d["labels.0"], mask_val=slot + 1)
    Rg, tg, _ = pc.gt_pose(0, 1)
    deg, mm = icp_ref.pose_error(best["R"], best["t"], Rg, tg)
    print("rank %d, score %.4f, %d inliers: %.3f deg %.3f mm" % (best["rank"], best["score"], best["inliers"], deg, mm))
    assert best["status"] == 0 and best["rank"] > 0 and deg < 2.0 and mm < 2.0
