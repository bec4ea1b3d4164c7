"""The contract of dense projective ICP (include/tgpose.h tgp_icp_dense; DESIGN.md section 3 "Dense projective registration") on its
NumPy restatement tests/icp_dense_ref.py alone: what each rule of the contract gives on the cases of tests/icp_dense_cases.py, and
how well the rule registers a fused object.  tests/test_icp_dense_gpu.py holds the kernel to the same cases."""
import numpy as np
import pytest

from tests import icp_dense_cases as dc
from tests import icp_dense_ref as dr
from tests import icp_ref


def unchanged(c, j, r):
    return r["R"].tobytes() == c["R"][j].tobytes() and r["t"].tobytes() == c["t"][j].tobytes() and r["s"].tobytes() == c["s"][j].tobytes()


def test_exact_case_meets_its_own_cells():
    """start = truth on the plane: iteration 0 associates every hit pixel of the frame with its own cell, the update is below the
    tolerances and the loop stops after one iteration"""
    c, (r,) = dc.rule_calls()["exact"], dc.expected("exact")
    hits = np.flatnonzero(c["depth"][0].ravel() > 0)
    assert r["status"] == 0 and r["iters"] == 1 and r["candidates"] == r["inliers"] == len(hits) > 800
    assert np.array_equal(np.flatnonzero(r["corr"] >= 0), hits) and np.array_equal(r["corr"][hits], hits)    # the map is the frame's grid
    assert icp_ref.rotation_angle(c["R"][0].astype(np.float64), r["R64"]) <= 1e-5 and np.linalg.norm(r["t64"] - c["t"][0]) <= 1e-6
    assert float(r["rmse"]) <= 1e-6


# measured on the restatement (this test's printed line): dense 0.0397 degrees / 0.1205 mm, the sparse path's restatement on the
# same frame and volume 0.2017 degrees / 0.1145 mm; the bounds are the dense figures x 1.5, this project's factor
OBJECT_BOUND_DEG, OBJECT_BOUND_MM = 1.5 * 0.0397, 1.5 * 0.1205


def test_object_accuracy():
    """icp_ref.two_boxes fused at G = 32 from 12 rendered views, the frame the volume ray-cast at a held-out pose, the start 5
    degrees and 10 mm off it, 60 x 80 maps, gate 20 mm.  Measured: 1536 frame pixels, 1417 candidates, 1469 final inliers, 6
    iterations, 0.0397 degrees / 0.1205 mm from the truth.  The sparse path's restatement on the same data (icp_ref.refine on the 40 x
    48 hits, 520 of them, and a 1024-point sample of the frame): 0.2017 degrees / 0.1145 mm -- recorded, no order between the two is
    asserted."""
    c, truth, sp = dc.object_case()
    (r,) = dc.expected("object")
    err = icp_ref.pose_error(r["R64"], r["t64"], *truth)
    start = icp_ref.pose_error(c["R"][0], c["t"][0], *truth)
    s = icp_ref.refine(sp["model"], sp["cloud"], sp["R"], sp["t"], sp["s"], dc.OBJ_GATE, mode=1, iters=50)
    sparse = icp_ref.pose_error(s["R64"], s["t64"], *truth)
    print("object: %d frame pixels, %d source pixels, %d candidates, %d inliers, %d iterations; start %.3f deg %.3f mm; dense %.4f deg %.4f mm; "
          "sparse (%d hits, %d inliers, %d iterations) %.4f deg %.4f mm"
          % ((c["depth"] > 0).sum(), dc.pixels(c, 0), r["candidates"], r["inliers"], r["iters"], *start, *err, sp["hits"], s["inliers"], s["iters"], *sparse))
    # the conditions, so that no later test hides behind them
    assert r["status"] == 0 and r["candidates"] >= 300 and 2 * r["inliers"] >= r["candidates"]
    assert s["status"] == 0 and abs(start[0] - 5.0) < 1e-3 and abs(start[1] - 10.0) < 1e-3
    assert err[0] <= OBJECT_BOUND_DEG and err[1] <= OBJECT_BOUND_MM


# name -> per job (status, inliers, iterations, candidates); None: not fixed by hand (checked for consistency below)
RULES = {
    "rect_outside": [(1, 0, 0, 0)] * 3,
    "rect_empty": [(1, 0, 0, 0)] * 2,
    "zero_frame": [(1, 0, 0, 0)],
    "nan_window": [(1, 0, 0, 0)] * 3,
    "bad_img": [(3, 0, 0, 0), (3, 0, 0, 0), (0, 841, 1, 841)],
    "map_1x1": [(1, 1, 0, 1)],                                     # the one pixel on the axis ray
    "behind_ref": [(1, 0, 0, 0)],
    "five_pixels": [(1, 5, 0, 5)],                                 # min_inliers = 0: the floor of 6 holds
}


@pytest.mark.parametrize("name", sorted(RULES))
def test_rule_refuses(name):
    c, got = dc.rule_calls()[name], dc.expected(name)
    assert len(got) == len(RULES[name])
    for j, (r, want) in enumerate(zip(got, RULES[name])):
        assert (r["status"], r["inliers"], r["iters"], r["candidates"]) == want, (name, j)
        if r["status"]:
            assert unchanged(c, j, r), (name, j)
            assert np.isnan(r["rmse"]) == (r["inliers"] == 0)


def test_rule_bad_pose_is_never_a_success():
    """a NaN or an infinity in the start pose, or a scale of 0: status 1 or 2, the pose returned as it came, never a NaN as success"""
    c, got = dc.rule_calls()["bad_pose"], dc.expected("bad_pose")
    assert len(got) == 8
    for j, r in enumerate(got):
        assert r["status"] in (1, 2) and r["iters"] == 0 and unchanged(c, j, r), j
    assert [r["status"] for r in got] == [1, 1, 1, 1, 1, 1, 2, 1]       # s = inf puts every pixel on the axis cell: a step that is not finite


@pytest.mark.parametrize("name,stride,source", [("shifted", 1, 3072), ("rect_partly_outside", 1, 41 * 31), ("stride2", 2, 30 * 23), ("stride3", 3, 21 * 16),
                                                ("mask_half", 1, 3072), ("six_by_eight", 1, 56)])
def test_rule_converges(name, stride, source):
    """a start 0.4 degrees and 3 mm off the plane, in the directions a plane holds: the tilt and the depth come back; the source pixels
    are the rectangle's grid cut to the frame, the candidates the frame's hits among them"""
    c, (r,) = dc.rule_calls()[name], dc.expected(name)
    xs, ys = dr.grid(c["rect"][0], c["stride"], dc.RULE_H, dc.RULE_W)
    assert c["stride"] == stride and len(xs) == source == len(r["corr"])
    assert (xs >= 0).all() and (xs < dc.RULE_W).all() and (ys >= 0).all() and (ys < dc.RULE_H).all()
    assert ((xs - int(c["rect"][0][0])) % stride == 0).all() and ((ys - int(c["rect"][0][1])) % stride == 0).all()
    live = c["depth"][0][ys, xs] > 0
    if c["mask"] is not None:
        live &= c["mask"][0][ys, xs] == c["job_mask_val"][0]
        assert 0.4 * (c["depth"][0][ys, xs] > 0).sum() < live.sum() < 0.6 * (c["depth"][0][ys, xs] > 0).sum()
    assert r["status"] == 0 and r["candidates"] == live.sum() == r["inliers"] and 1 <= r["iters"] <= 5
    assert np.array_equal(r["corr"] >= 0, live)
    n = r["R64"] @ np.array([0.0, 0.0, 1.0])                        # the plane's normal and depth as the camera sees them
    assert np.rad2deg(np.arccos(min(1.0, n[2]))) < 0.01 and abs(r["t64"][2] - 1.0) < 2e-5


def test_rule_one_iteration():
    """iters = 1 with both tolerances 0: exactly one iteration, the pose moved"""
    c, (r,) = dc.rule_calls()["one_iteration"], dc.expected("one_iteration")
    assert r["status"] == 0 and r["iters"] == 1 and not unchanged(c, 0, r)
    more = dc.expected("shifted")[0]
    assert more["iters"] == 2                                       # with the default tolerances the same start goes on


def test_three_jobs_are_three_answers():
    got = dc.expected("three_jobs")
    assert [r["status"] for r in got] == [0, 0, 0] and all(r["candidates"] >= 300 and 2 * r["inliers"] >= r["candidates"] for r in got)
    c = dc.rule_calls()["three_jobs"]
    assert len({c["rect"][j].tobytes() for j in range(3)}) == 3 and c["job_img"].tolist() == [0, 1, 0]


def test_rects_by_hand():
    win = np.array([[10.2, 5.7, 0.5, 0.25], [30, 10, -1, 1], [np.nan, 5, 1, 1], [5, 5, 1, np.nan], [np.inf, 5, 1, 1]], np.float32)
    assert dr.rects(win, 9, 21, 48, 64).tolist() == [[10, 5, 21, 8], [10, 10, 30, 18], [0, 0, -1, -1], [0, 0, -1, -1], [63, 5, 63, 13]]
    assert dr.rects(np.array([[-3.5, 40.0, 2.0, 1.0]], np.float32), 20, 40, 48, 64).tolist() == [[0, 40, 63, 47]]      # clamped to the frame
    assert dr.rects(np.array([[32.5, 24.5, 1, 1], [32, 24, 7, 7]], np.float32), 1, 1, 48, 64).tolist() == [[32, 24, 33, 25], [32, 24, 32, 24]]
    assert dr.rects(np.array([[0, 0, 1, 1]], np.float32), 48, 64, 48, 64).tolist() == [[0, 0, 63, 47]]
    assert dr.rects(np.zeros((0, 4), np.float32), 4, 4, 48, 64).shape == (0, 4)
