"""The ray caster's rule (DESIGN.md section 3 "Ray casting and frame-to-model tracking") on the NumPy restatement tests/raycast_ref.py
alone: its accuracy on the analytic sphere and on a fused object, each rule on a hand-built volume with the outputs written down here,
and the packing rule of ops.IcpModels.from_raycast.  tests/test_raycast_gpu.py holds the kernel to the same restatement bit for bit."""
import numpy as np
import pytest

from tests import raycast_cases as rc
from tests import raycast_ref as rr
from tests import tsdf_cases as tc
from tests.render_ref import pose34

F = np.float32

# measured with this restatement (worst over the three poses), and the bounds: x 1.5 for other poses and compilers
SPHERE_MEASURED = {16: (0.1016, 6.953), 24: (0.0798, 4.579)}          # |z - z_analytic| in voxels, normal against radial in degrees


@pytest.mark.parametrize("G", [16, 24])
def test_analytic_sphere(G):
    """tsdf_cases.sphere(G) from three poses on a 33 x 65 grid: every ray whose line passes the centre at least one voxel inside the
    silhouette hits, every ray that passes more than one voxel outside misses; over the former, the depth error in voxels (|z -
    z_analytic| over the voxel edge in metres) and the angle between the normal and the radial direction.  Measured: 0.1016 voxel
    and 6.953 degrees at G = 16, 0.0798 voxel and 4.579 degrees at G = 24 (the mesh's worst vertex on these volumes is 0.065 /
    0.045 voxel); the bounds are those x 1.5."""
    c = rc.sphere_call(G)
    out = rc.expected("sphere%d" % G)
    z, gap, normal = rc.sphere_analytic(c)
    hit = out["z"] > 0
    inside, outside = gap <= -1, gap >= 1
    assert inside.sum() > 1000 and outside.sum() > 1000
    assert hit[inside].all() and not hit[outside].any()
    assert out["count"].tolist() == hit.reshape(3, -1).sum(1).tolist() and out["status"].tolist() == [0, 0, 0]
    voxel_m = np.array([p[3] for p in rc.SPHERE_POSES])[:, None, None] * float(c["meta"][0, 3])
    err = (np.abs(out["z"] - z) / voxel_m)[inside].max()
    cos = (out["normal"].astype(np.float64) * normal).sum(-1)[inside]
    angle = np.rad2deg(np.arccos(np.clip(cos, -1, 1))).max()
    print("sphere G=%d: worst depth error %.4f voxel, worst normal angle %.3f degrees over %d rays" % (G, err, angle, inside.sum()))
    assert abs(np.linalg.norm(out["normal"][hit], axis=1) - 1).max() < 1e-6
    assert err <= 1.5 * SPHERE_MEASURED[G][0] and angle <= 1.5 * SPHERE_MEASURED[G][1]
    # the vertex is the hit in the model frame: the inverse pose of the camera-frame point
    j = 1
    T = c["job_pose"][j].astype(np.float64)
    cam = out["vertex"][j][hit[j]].astype(np.float64) @ T[:, :3].T + T[:, 3]
    assert np.abs(cam[:, 2] - out["z"][j][hit[j]]).max() < 1e-5
    assert not out["vertex"][~hit].any() and not out["normal"][~hit].any() and not out["depth"][~hit].any()


BOTTLE_MEASURED = (0.0662, 0.2413, 0.0434)                           # median and 95th percentile |depth difference| in voxels, missed share


def test_fused_object_against_the_true_mesh():
    """tests/test_tsdf_cpu.py's bottle (12 frames of tests/render_ref.py at 160 x 120, fused by tests/tsdf_ref.py at G = 32, truncation
    two voxels), ray-cast over the full frame at a held-out pose (half a step between two of the turntable's) and compared with
    render_ref's depth of the true mesh there.  Measured: over the pixels both call surface the median |depth difference| is 0.0662
    voxel and the 95th percentile 0.2413 voxel; 4.34 % of the true surface's pixels are missed (rays along the silhouette, whose
    cells hold a voxel no frame saw).  Bounds: x 1.5, and the share + 0.02; a share of 0.25 would mean the rule is wrong."""
    from tests import render_ref
    v, f, meta, vsum, weight = rc.fused_bottle()
    p = pose34(*tc.turntable_pose(2, offset=0.5), s=tc.TURN_SCALE)
    true = render_ref.render_scene([(v, f)], [(0, 1, p)], rc.QUALITY_K, rc.QUALITY_H, rc.QUALITY_W)
    out = rc.run(rc.call(vsum, weight, meta[None], rc.QUALITY_K, [0], [0], [p], [(0, 0, 1, 1)], rc.QUALITY_H, rc.QUALITY_W))
    surf, hit = true["depth"] > 0, out["z"][0] > 0
    both = surf & hit
    voxel_m = float(meta[3]) * tc.TURN_SCALE
    d = np.abs(out["z"][0][both].astype(np.float64) - true["z"][both]) / voxel_m
    median, p95, missed = float(np.median(d)), float(np.percentile(d, 95)), float((surf & ~hit).sum()) / float(surf.sum())
    print("fused bottle: %d true pixels, %d hits; median %.4f voxel, 95th percentile %.4f voxel, missed share %.4f" % (surf.sum(), hit.sum(), median, p95, missed))
    assert surf.sum() > 400 and int(out["count"][0]) == hit.sum()
    assert missed < 0.25
    assert median <= 1.5 * BOTTLE_MEASURED[0] and p95 <= 1.5 * BOTTLE_MEASURED[1] and missed <= BOTTLE_MEASURED[2] + 0.02
    assert np.array_equal(out["depth"][0], np.where(hit, np.rint(out["z"][0] * F(1000)), 0).astype(np.uint16))


def one(name):
    """the single ray of a 1 x 1 rule call: (z, depth, vertex, normal, count, status)"""
    o = rc.expected(name)
    return float(o["z"][0, 0, 0]), int(o["depth"][0, 0, 0]), o["vertex"][0, 0, 0].tolist(), o["normal"][0, 0, 0].tolist(), int(o["count"][0]), int(o["status"][0])


MISS = (0.0, 0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0, 0)


def test_rule_cases():
    # the axis ray meets the plane at voxel coordinate 7.5 = the model's z = 0, one metre from the camera: exact in float32
    assert one("plane") == (1.0, 1000, [0.0, 0.0, 0.0], [0.0, 0.0, -1.0], 1, 0)
    # f = 0 at the sample itself: the hit is that sample, on the face between two cells
    assert one("boundary") == (1.0078125, 1008, [0.0, 0.0, 0.0078125], [0.0, 0.0, -1.0], 1, 0)
    assert one("misses_cube") == MISS
    assert one("inside") == MISS                                           # the first known sample is negative
    assert one("unknown_layer") == MISS                                    # the unknown layer forgot the positive sample
    assert one("unknown_layer_low") == (1.0, 1000, [0.0, 0.0, 0.0], [0.0, 0.0, -1.0], 1, 0)
    assert one("from_behind") == MISS
    assert one("exit") == MISS                                             # unknown, negative, positive: the - -> + change is no hit
    z, depth, vertex, normal, count, status = one("near_cuts")             # the march starts at g_z = 4.3 and still finds z = 1
    assert abs(z - 1.0) < 1e-6 and depth == 1000 and np.abs(vertex).max() < 1e-6 and normal == [0.0, 0.0, -1.0] and count == 1
    assert one("near_beyond") == MISS
    z, depth, vertex, normal, count, status = one("far")
    assert abs(z - 70.0) < 1e-4 and depth == 0 and count == 1 and normal == [0.0, 0.0, -1.0]      # beyond 65.535 m: z is kept
    for name, J in (("bad_pose", 5), ("bad_window", 6)):
        o = rc.expected(name)
        assert o["status"].tolist() == [0] * J and o["count"].tolist() == [0] * J
        assert not o["z"].any() and not o["depth"].any() and not o["vertex"].any() and not o["normal"].any()
    o = rc.expected("bad_index")
    assert o["status"].tolist() == [1, 1, 1, 1, 0] and o["count"].tolist() == [0, 0, 0, 0, 1] and not o["z"][:4].any() and o["z"][4, 0, 0] == 1.0


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 65)])
def test_rule_grids_over_two_volumes(h, w):
    """J = 3 over two volumes of different meta: job 0 the plane at 7.5 of the 1/64 cube from the front, job 1 the plane at 8 of the
    1/32 cube (centre off the origin) from 1.5 m, job 2 the first again from a pose turned by 20 degrees.  Every hit of job 0 has
    z = 1 (the plane is the camera's z = 1) and the model's z = 0; the rays outside the cube's image miss."""
    c = rc.rule_calls()["grid_%dx%d" % (h, w)]
    o = rc.expected("grid_%dx%d" % (h, w))
    hit = o["z"] > 0
    assert o["z"].shape == (3, h, w) and o["status"].tolist() == [0, 0, 0] and o["count"].tolist() == hit.reshape(3, -1).sum(1).tolist()
    assert hit[:, h // 2, w // 2].all()
    if h > 1:
        assert not hit[0].all() and hit[0].sum() > h * w // 4
    assert np.abs(o["z"][0][hit[0]] - 1.0).max() < 1e-6 and np.abs(o["vertex"][0][hit[0]][:, 2]).max() < 1e-6
    assert (o["normal"][0][hit[0]] == np.array([0, 0, -1], F)).all() and (o["normal"][1][hit[1]] == np.array([0, 0, -1], F)).all()
    # job 1: the plane at voxel coordinate 8 of the second cube is the model's z = 0.03 + 0.5 / 32, seen from t_z = 1.5
    assert np.abs(o["z"][1][hit[1]] - (1.5 + 0.03 + 0.5 / 32)).max() < 1e-5
    # job 2: a turned camera still reports points of the model's plane z = 0, and its depths differ from ray to ray
    assert np.abs(o["vertex"][2][hit[2]][:, 2]).max() < 1e-5
    if h > 1:
        assert np.ptp(o["z"][2][hit[2]]) > 0.01
    T = c["job_pose"][2].astype(np.float64)
    cam = o["vertex"][2][hit[2]].astype(np.float64) @ T[:, :3].T + T[:, 3]
    assert np.abs(cam[:, 2] - o["z"][2][hit[2]]).max() < 1e-5


def test_inverse_pose_and_windows():
    c = rc.sphere_call(16)
    inv = rr.inverse_pose(c["job_pose"])
    for T, I in zip(c["job_pose"].astype(np.float64), inv.astype(np.float64)):
        assert np.abs(I[:, :3] @ T[:, :3] - np.eye(3)).max() < 1e-6 and np.abs(I[:, :3] @ T[:, 3] + I[:, 3]).max() < 1e-6
    win = rr.windows(c["meta"], 16, c["camk"], c["job_img"], c["job_model"], c["job_pose"], 40, 48, 240, 320)
    z, gap, _ = rc.sphere_analytic(c)
    for j in range(3):                                                      # the window holds the sphere's image
        w0 = c["window"][j].astype(np.float64)
        rows, cols = np.nonzero(gap[j] < 0)
        u, v = w0[0] + cols * w0[2], w0[1] + rows * w0[3]
        u1, v1 = win[j, 0] + 47 * win[j, 2], win[j, 1] + 39 * win[j, 3]
        assert win[j, 0] <= u.min() and u.max() <= u1 and win[j, 1] <= v.min() and v.max() <= v1
        assert 0 <= win[j, 0] and u1 <= 319.001 and 0 <= win[j, 1] and v1 <= 239.001
    behind = c["job_pose"].copy()
    behind[0, 2, 3] = -0.5
    behind[1, 0, 0] = np.nan
    win = rr.windows(c["meta"], 16, c["camk"], c["job_img"], c["job_model"], behind, 40, 48, 240, 320)
    assert np.isnan(win[0]).all() and np.isnan(win[1]).all() and np.isfinite(win[2]).all()
    win = rr.windows(c["meta"], 16, c["camk"], c["job_img"], c["job_model"], behind, 5, 7, 240, 320)
    empty = rr.raycast(c["vsum"], c["weight"], c["meta"], c["camk"], c["job_img"], c["job_model"], rr.inverse_pose(behind), win, 5, 7)
    assert empty["count"].tolist()[:2] == [0, 0] and empty["count"][2] > 0
    one = rr.windows(c["meta"], 16, c["camk"], c["job_img"], c["job_model"], c["job_pose"], 1, 1, 240, 320)
    assert (one[:, 2:] == 1).all()


def test_packing_rule():
    """ops.IcpModels.from_raycast: the hits first, in ray order, [vertex, normal]; the count is the number of hits"""
    o = rc.expected("grid_5x7")
    pts, counts = rr.pack(o)
    assert pts.shape == (3, 35, 6) and counts.tolist() == o["count"].tolist()
    for j in range(3):
        order = [i for i in range(35) if o["z"][j].ravel()[i] > 0]
        assert len(order) == counts[j]
        assert np.array_equal(pts[j, :len(order), :3], o["vertex"][j].reshape(-1, 3)[order])
        assert np.array_equal(pts[j, :len(order), 3:], o["normal"][j].reshape(-1, 3)[order])
        assert not pts[j, len(order):].any()
    assert 0 < counts[0] < 35
