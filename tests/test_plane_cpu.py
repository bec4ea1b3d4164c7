"""The supporting plane without a GPU: the ABI's three new entry points, the wrappers' argument checks, and the NumPy restatement of
the contract (tests/plane_ref.py) against what it must find -- the table of the rendered tracking scene, the tracking simulation
tests/test_track_plane_gpu.py relies on, and the reference's tools/plane_utils.py (tests/golden/plane_utils_ref.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import plane_cases as pc
from tests import plane_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_utils_ref.npz")
NAMES = ("tgp_plane_fit", "tgp_plane_cut", "tgp_plane_lsq")


def test_header_declares_and_library_exports_the_entry_points():
    from tgpose_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(handle, name) is not None
    assert _lib.ABI_VERSION == 9
    assert "tgp_plane_fit_args" in _lib.STRUCTS
    fields = [f[0] for f in _lib.PlaneFitArgs._fields_]
    assert fields == ["depth", "camk", "keys", "seed", "S", "H", "W", "hypotheses", "tol", "refine_iters", "min_inliers", "plane", "info", "counts"]
    assert _lib.SIGNATURES["tgp_plane_lsq"][1][4] is ctypes.c_double


def test_the_draw_site_follows_the_mesh_sampler():
    from tgpose_amd import _lib
    assert _lib.PLANE_SITE == _lib.MESH_SITE + 1 == plane_ref.SITE
    assert _lib.PLANE_MAX_HYPOTHESES == plane_ref.MAX_HYPOTHESES and _lib.PLANE_MAX_REFITS == plane_ref.MAX_REFITS


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from tgpose_amd import ops, pose
    depth = torch.zeros(2, 8, 8, dtype=torch.int16)
    camk = torch.ones(2, 4)
    plane, info = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.plane_fit(depth, camk)
    with pytest.raises(ValueError):
        ops.plane_cut(depth, plane, info, camk)
    with pytest.raises(ValueError):
        ops.plane_lsq(torch.zeros(1, 4, 3), torch.ones(1, 4))
    with pytest.raises(ValueError):
        ops.plane_fit(np.zeros((2, 8, 8), np.uint16), camk)
    with pytest.raises(ValueError):
        pose.SupportPlane(tol=-1.0)
    s = pose.SupportPlane()
    assert (s.tol, s.margin, s.hypotheses, s.refine_iters) == (0.004, 0.006, 256, 2)


def test_track_takes_a_support_argument():
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    import inspect
    assert inspect.signature(myEvaluater.track).parameters["support"].default is None


def test_plane_utils_keeps_the_reference_names():
    from tgpose_amd.tools import plane_utils
    import inspect
    for name in ("get_plane", "get_plane_in_batch", "get_plane_parameter"):
        assert list(inspect.signature(getattr(plane_utils, name)).parameters) == ["pc", "pc_w"]


def test_restatement_finds_the_table():
    """Measured: the normal within 0.0013 degrees and d within 0.032 mm of the scene's table in all six frames (about 64 500 inliers
    of 71 360 valid pixels, depth quantised to 1 mm); the best hypothesis alone is within 0.11 degrees / 1.7 mm."""
    for k in range(pc.FRAMES):
        ft = pc.fitted(k)
        ang, off = pc.plane_error(ft["plane"], k)
        print("frame %d: status %d, best hypothesis %d with %d inliers, final %d of %d valid; normal %.5f deg, d %.4f mm off the table"
              % (k, ft["info"][0], ft["best"], ft["info"][1], ft["info"][2], ft["info"][3], ang, off))
        assert ft["info"][0] == 0 and ft["info"][2] > 60000
        assert ang < 0.1 and off < 1.0
        assert ft["plane"][3] >= 0 and abs(float(np.linalg.norm(ft["plane"][:3].astype(np.float64))) - 1.0) < 1e-6
        out, side = plane_ref.cut(pc.rendered(k), ft["plane"], 0, pc.CAMK, pc.MARGIN)
        assert (side == 3).sum() == 0                                              # nothing is below the table
        assert 5000 < (out > 0).sum() < 8000                                      # the objects are left


def test_cut_copies_a_frame_without_a_plane_through():
    depth = pc.rendered(0)
    out, side = plane_ref.cut(depth, np.zeros(4, np.float32), 1, pc.CAMK, pc.MARGIN)
    assert np.array_equal(out, depth) and set(np.unique(side)) == {0, 1}
    ft = plane_ref.fit(np.zeros((8, 9), np.uint16), pc.CAMK, hypotheses_n=5)
    assert ft["info"].tolist() == [1, 0, 0, 0] and not ft["plane"].any()


def test_two_planes_tie_and_the_first_hypothesis_wins():
    fr = pc.small_frames()[3]
    ft = plane_ref.fit(fr, pc.SMALL_CAMK, key=pc.SMALL_KEYS[3], seed=0, hypotheses_n=pc.SMALL_HYPOTHESES, refine_iters=0)
    top = np.nonzero(ft["counts"] == 962)[0]
    assert ft["counts"].max() == 962 and ft["best"] == top[0]
    assert {float(d) for d in ft["hyp"][top, 3]} == {float(np.float32(0.8)), 1.0}  # both planes are hit, with equal counts
    assert ft["plane"][3] == ft["hyp"][top[0], 3]


def test_tracking_simulation_with_and_without_the_cut():
    """Measured (the device's keyed draw restated, seed 5): with the cut the worst frame is 0.79 degrees / 0.40 mm with at least
    501 of 512 inliers; without it 1.82 degrees / 1.58 mm and at least 367 inliers."""
    with_cut, without = pc.simulate(True), pc.simulate(False)
    for name, sim in (("cut", with_cut), ("uncut", without)):
        for k, row in enumerate(sim):
            print("%s frame %d: %s" % (name, k, "  ".join("%.3f deg %.3f mm %d inliers" % e[:3] for e in row)))
    for row in with_cut:
        for rot, trans, inliers, status in row:
            assert status == 0 and rot < 1.0 and trans < 1.5 and inliers >= 400
    assert pc.worst(without)[0] > pc.worst(with_cut)[0]


def _golden_margin(g, key):
    """the reference's own float32-vs-float64 deviation on this output, or 1e-6 when that is smaller"""
    return max(float(np.abs(g["f32." + key].astype(np.float64) - g["f64." + key]).max()), 1e-6)


def test_restated_regression_against_the_reference():
    g = np.load(GOLDEN)
    pc_, w = g["pc"], g["pc_w"]
    for i in range(2):
        for j in range(3):
            for eps, group in ((0.0, "single"), (1e-8, "batch")):
                X, normal, dn, p2 = plane_ref.lsq(pc_[i, j], w[i, j], eps)
                got = dict(normal=normal, dn=dn, p2plane=np.array([p2]))
                if group == "single":
                    got["X"] = X.reshape(3, 1)
                for name, val in got.items():
                    key = "%s.%s" % (group, name)
                    err = float(np.abs(val.astype(np.float64) - g["f64." + key][i, j]).max())
                    assert err <= _golden_margin(g, key), (key, i, j, err)
    # singular systems: one point, two points, collinear points
    for n in (1, 2):
        assert all(np.isnan(np.asarray(x)).all() for x in plane_ref.lsq(pc_[0, 0, :n], w[0, 0, :n]))
    line = np.stack([np.linspace(-0.1, 0.1, 9), np.linspace(-0.1, 0.1, 9) * 0.5, np.linspace(0, 1, 9)], 1)
    assert all(np.isnan(np.asarray(x)).all() for x in plane_ref.lsq(line, np.ones(9)))
