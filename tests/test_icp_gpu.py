"""ops.icp_refine (csrc/icp.hip) against the NumPy restatement of its contract (tests/icp_ref.py) and against ground truth.

The model is icp_ref.two_boxes: two boxes of unequal edges joined off-centre, no symmetry.  Tolerances: the sums and the solve are
float64 on both sides, so poses differ by the one float32 rounding of the result (6e-8 relative) and by the order of summation through
the solve; 1e-6 leaves a factor of 16.  Correspondences and inlier counts are compared exactly.

Measured on the MI355X (this file's printed output):
  noise-free convergence (test 2), error against the truth, kernel / restatement, degrees and millimetres: see DESIGN.md section 3
  "ICP refinement and model-based tracking", which records them together with the rendered object's (test 5)."""
import numpy as np
import pytest
import torch

from tests import icp_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_S = {}
POSES = []                                                   # every pose tests 1 and 2 produced (test 3 checks them)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def up(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dtype)).to(DEV)


def truth():
    return icp_ref.rot([0.3, -0.5, 0.8], 140.0), np.array([0.05, -0.03, 0.8]), 0.16


def off_by(Rg, tg, deg, mm):
    return Rg @ icp_ref.rot([1.0, 2.0, -1.0], deg), tg + mm * 1e-3 * np.array([2.0, -1.0, 2.0]) / 3.0


def setup():
    """the mesh set (two_boxes, a plane), 2048 samples with normals of each (once), and test 1's five jobs"""
    if _S:
        return _S
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes
    ms = ops.MeshSet([icp_ref.two_boxes(), shapes.plane(1.0, 0.8, 2, 2)], device=DEV)
    dense = ops.mesh_sample(ms, [0, 0, 1, 0], 2048, keys=[0, 1, 2, 3], seed=3, normals=True, check_status=True)["points"]
    pn = dense[:2].clone()
    pn[0, 100:] = 1e3                                        # rows beyond a model's count are never read
    Rg, tg, sg = truth()
    other = dense[3, :, :3].cpu().numpy().astype(np.float64)           # samples that are NOT the models'
    img = (sg * other @ Rg.T + tg).astype(np.float32)
    counts = [1, 63, 257, 700, 2048]
    src = np.full((5, 2048, 3), 7.0, np.float32)             # rows beyond a job's count are never read
    for j, c in enumerate(counts):
        src[j, :c] = img[j * 5:j * 5 + c] if j < 4 else img
    src[3, 5:16] = np.nan                                    # the job with NaN rows
    src[3, 20, 1] = np.inf
    R0, t0 = off_by(Rg, tg, 2.0, 3.0)
    _S.update(ms=ms, dense=dense, models=ops.IcpModels(pn, counts=[100, 2048]), model_np=pn.cpu().numpy(), model_count=[100, 2048],
              job_model=[0, 1, 1, 0, 1], counts=counts, src=src, R0=np.tile(R0.astype(np.float32), (5, 1, 1)),
              t0=np.tile(t0.astype(np.float32), (5, 1)), gate=0.02, refs={})
    return _S


def call(s, mode, with_scale, jobs=range(5), **kw):
    from tgpose_amd import ops
    jobs = list(jobs)
    s0 = np.full(5, 0.16 * (1.01 if with_scale else 1.0), np.float32)
    return ops.icp_refine(s["models"], up(np.asarray(s["job_model"])[jobs], np.int32), up(s["src"][jobs]), up(s["R0"][jobs]), up(s["t0"][jobs]),
                          up(s0[jobs]), up(np.full(len(jobs), s["gate"], np.float32)), src_count=up(np.asarray(s["counts"])[jobs], np.int32),
                          mode=mode, with_scale=with_scale, return_corr=True, **kw)


def reference(s, mode, with_scale):
    """icp_ref on test 1's jobs, one iteration (computed once per mode)"""
    key = (mode, with_scale)
    if key not in s["refs"]:
        out = []
        for j in range(5):
            m = s["job_model"][j]
            out.append(icp_ref.refine(s["model_np"][m][:s["model_count"][m]], s["src"][j][:s["counts"][j]], s["R0"][j], s["t0"][j],
                                      np.float32(0.16 * (1.01 if with_scale else 1.0)), s["gate"], mode=1 if mode == "plane" else 0,
                                      with_scale=with_scale, iters=1, tol_rot=0.0, tol_trans=0.0))
        s["refs"][key] = out
    return s["refs"][key]


def check_proper(R, what):
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    for k, r in enumerate(R):
        assert np.abs(r.T @ r - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(r) - 1.0) <= 1e-6, (what, k)


@pytest.mark.parametrize("mode,with_scale", [("plane", False), ("point", False), ("point", True)])
def test_one_iteration_equals_the_contract(mode, with_scale):
    from tgpose_amd import ops
    s = setup()
    ref = reference(s, mode, with_scale)
    R, t, sc, info, rmse, corr = (x.cpu().numpy() for x in call(s, mode, with_scale, iters=1, tol_rot=0.0, tol_trans=0.0))
    POSES.append(R.copy())
    for j, r in enumerate(ref):
        n = s["counts"][j]
        print("%s scale %d job %d: status %d inliers %d iters %d rmse %.6e | ref %d %d %d %.6e | max |dR| %.2e |dt| %.2e ds %.2e" %
              (mode, with_scale, j, info[j, 0], info[j, 1], info[j, 2], rmse[j], r["status"], r["inliers"], r["iters"], r["rmse"],
               np.abs(R[j] - r["R64"]).max(), np.abs(t[j] - r["t64"]).max(), abs(sc[j] - r["s64"])))
        assert info[j].tolist() == [r["status"], r["inliers"], r["iters"], 0]
        assert np.array_equal(corr[j, :n], r["corr"]) and (corr[j, n:] == -1).all()
        assert np.abs(R[j].astype(np.float64) - r["R64"]).max() <= 1e-6
        assert np.abs(t[j].astype(np.float64) - r["t64"]).max() <= 1e-6 * max(1.0, np.linalg.norm(r["t64"]))
        assert abs(float(sc[j]) - r["s64"]) <= 1e-6 * r["s64"]
        if r["inliers"]:
            assert abs(float(rmse[j]) - float(r["rmse"])) <= 1e-6 * float(r["rmse"])
        else:
            assert np.isnan(rmse[j])
    assert info[0, 0] == 1 and (info[1:, 0] == 0).all()      # one source point is too few; the other jobs ran their iteration
    assert (corr[3, 5:16] == -1).all() and corr[3, 20] == -1 # the NaN / inf rows

    # the pre-update correspondences: a job that is refused for too few inliers keeps its start pose, so its final pass IS the
    # first pass.  They equal the restatement's and, for every inlier, ops.nn1 of the restatement's model-frame points.
    R1, t1, s1, info1, _, corr1 = (x.cpu().numpy() for x in call(s, mode, with_scale, iters=1, tol_rot=0.0, tol_trans=0.0, min_inliers=4096))
    assert (info1[:, 0] == 1).all() and (info1[:, 2] == 0).all()
    assert np.array_equal(R1, s["R0"]) and np.array_equal(t1, s["t0"])
    for j, r in enumerate(ref):
        n, m = s["counts"][j], s["job_model"][j]
        assert np.array_equal(corr1[j, :n], r["first_corr"]) and info1[j, 1] == (r["first_corr"] >= 0).sum()
        q = np.nan_to_num(r["first_q"], nan=0.0, posinf=0.0, neginf=0.0)
        nn = ops.nn1(up(q[None]), up(s["model_np"][m][None, :s["model_count"][m], :3])).cpu().numpy()[0]
        live = r["first_corr"] >= 0
        assert live.sum() >= min(n, 6) // 2 and np.array_equal(nn[live], corr1[j, :n][live])


@pytest.mark.parametrize("mode", ["plane", "point"])
def test_convergence_on_noise_free_data(mode):
    from tgpose_amd import ops
    s = setup()
    Rg, tg, sg = truth()
    pn = s["dense"][1:2, :1024].contiguous()
    model_np = pn[0].cpu().numpy()
    src = (sg * model_np[::2, :3].astype(np.float64) @ Rg.T + tg).astype(np.float32)           # exact images of half the samples
    starts = [off_by(Rg, tg, 5.0, 10.0), off_by(Rg, tg, 15.0, 30.0)]
    R0 = np.stack([a.astype(np.float32) for a, _ in starts])
    t0 = np.stack([b.astype(np.float32) for _, b in starts])
    R, t, sc, info, rmse = (x.cpu().numpy() for x in ops.icp_refine(ops.IcpModels(pn), up([0, 0], np.int32), up(np.stack([src, src])), up(R0), up(t0),
                                                                    up([sg, sg]), 0.05, mode=mode, iters=60))
    POSES.append(R.copy())
    for j in range(2):
        ref = icp_ref.refine(model_np, src, R0[j], t0[j], np.float32(sg), 0.05, mode=1 if mode == "plane" else 0, iters=60)
        e0 = icp_ref.pose_error(R0[j], t0[j], Rg, tg)
        ek = icp_ref.pose_error(R[j], t[j], Rg, tg)
        er = icp_ref.pose_error(ref["R"], ref["t"], Rg, tg)
        print("%s start %.2f deg %.2f mm: kernel %.3e deg %.3e mm in %d iterations (rmse %.3e) | restatement %.3e deg %.3e mm in %d" %
              (mode, e0[0], e0[1], ek[0], ek[1], info[j, 2], rmse[j], er[0], er[1], ref["iters"]))
        assert ref["status"] == 0 and ref["iters"] < 60
        assert info[j, 0] == 0 and info[j, 2] < 60 and info[j, 1] == len(src)
        assert ek[0] <= max(10.0 * er[0], 1e-4) and ek[1] <= max(10.0 * er[1], 1e-4)


@pytest.mark.parametrize("with_scale", [False, True])
def test_rotations_are_proper_on_a_flat_model(with_scale):
    from tgpose_amd import ops
    s = setup()
    Rg, tg, sg = truth()
    flat = s["dense"][2:3, :512].contiguous()                                                   # shapes.plane: every point in z = 0
    assert float(flat[0, :, 2].abs().max()) == 0.0
    other = s["dense"][2, 512:1024, :3].cpu().numpy().astype(np.float64)
    src = (sg * other @ Rg.T + tg).astype(np.float32)
    R0, t0 = off_by(Rg, tg, 3.0, 5.0)
    R, t, sc, info, rmse = (x.cpu().numpy() for x in ops.icp_refine(ops.IcpModels(flat), up([0], np.int32), up(src[None]), up(R0[None]), up(t0[None]),
                                                                    up([sg * (1.01 if with_scale else 1.0)]), 0.05, mode="point",
                                                                    with_scale=with_scale, iters=20))
    print("flat model, scale %d: status %d inliers %d iterations %d det %.9f s %.6f" % (with_scale, info[0, 0], info[0, 1], info[0, 2],
                                                                                       np.linalg.det(R[0].astype(np.float64)), sc[0]))
    assert info[0, 0] == 0 and info[0, 1] >= 256 and np.isfinite(R).all() and np.isfinite(t).all() and sc[0] > 0
    check_proper(R, "flat")
    # the plane's normal is found (in-plane sliding is free on a flat model): R z agrees with the truth's
    assert np.rad2deg(np.arccos(min(1.0, abs(float(R[0].astype(np.float64)[:, 2] @ Rg[:, 2]))))) <= 0.5


def test_every_pose_of_the_other_tests_is_proper():
    s = setup()
    if not POSES:                                            # run alone: produce them
        for mode, ws in (("plane", False), ("point", False), ("point", True)):
            POSES.append(call(s, mode, ws, iters=1, tol_rot=0.0, tol_trans=0.0)[0].cpu().numpy())
    for k, R in enumerate(POSES):
        check_proper(R, k)


def test_statuses_and_repeatability():
    from tgpose_amd import ops
    s = setup()
    args = lambda jobs: (up(np.asarray(s["job_model"])[jobs], np.int32), up(s["src"][jobs]), up(s["R0"][jobs]), up(s["t0"][jobs]),
                         up(np.full(len(jobs), 0.16, np.float32)))
    every = list(range(5))
    # an empty gate: status 1 and the start pose bit for bit
    jm, src, R0, t0, s0 = args(every)
    R, t, sc, info, rmse, corr = ops.icp_refine(s["models"], jm, src, R0, t0, s0, 1e-6, src_count=up(s["counts"], np.int32), return_corr=True)
    assert (info[:, 0] == 1).all() and (info[:, 1] < 6).all() and (info[:, 2] == 0).all()
    assert torch.equal(R, R0) and torch.equal(t, t0) and torch.equal(sc, s0)
    with pytest.raises(ops._lib.TgpError):
        ops.icp_check_status(info)
    # job_model = M: status 3, nothing read, the pose copied through
    bad = jm.clone()
    bad[2] = 2
    R, t, sc, info, rmse, corr = ops.icp_refine(s["models"], bad, src, R0, t0, s0, 0.02, src_count=up(s["counts"], np.int32), return_corr=True)
    assert info[:, 0].tolist() == [1, 0, 3, 0, 0] and info[2].tolist() == [3, 0, 0, 0]
    assert torch.equal(R[2], R0[2]) and torch.equal(t[2], t0[2]) and torch.equal(sc[2], s0[2])
    assert bool(torch.isnan(rmse[2])) and bool((corr[2] == -1).all())
    # a source count outside [0, n_cap] likewise
    cnt = up(s["counts"], np.int32)
    cnt[1] = 2049
    assert ops.icp_refine(s["models"], jm, src, R0, t0, s0, 0.02, src_count=cnt)[3][:, 0].tolist() == [1, 3, 0, 0, 0]
    # point-to-plane against one repeated point and normal: singular, or a finite pose -- never a non-finite output
    one = torch.tensor([0.1, 0.2, 0.3, 0.0, 0.0, 1.0], device=DEV).repeat(1, 64, 1).contiguous()
    R, t, sc, info, rmse = ops.icp_refine(ops.IcpModels(one), up([0] * 5, np.int32), src, R0, t0, s0, 10.0, src_count=up(s["counts"], np.int32),
                                          mode="plane", iters=4)
    print("one repeated point: status", info[:, 0].tolist(), "iterations", info[:, 2].tolist())
    assert set(info[1:, 0].tolist()) <= {0, 2} and info[0, 0] == 1
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all()) and bool(torch.isfinite(sc).all())
    # a job alone, as one of five, and run again: the same bits
    for mode in ("plane", "point"):
        five = call(s, mode, False, iters=5, tol_rot=0.0, tol_trans=0.0)
        again = call(s, mode, False, iters=5, tol_rot=0.0, tol_trans=0.0)
        alone = call(s, mode, False, jobs=[4], iters=5, tol_rot=0.0, tol_trans=0.0)
        bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x                 # job 0's rmse is NaN: compare the bits
        for a, b, c in zip(five, again, alone):
            assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a[4:5]), bits(c))
        assert five[3][4].tolist()[0] == 0 and five[3][4].tolist()[2] == 5


def test_a_rendered_object_end_to_end():
    """depth frame -> masked ball crop -> refine_poses, against the scene's ground truth; the restatement on the same cloud is the
    yardstick (its errors are recorded in DESIGN.md)"""
    from tgpose_amd import ops, pose
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluation import load_data_eval as lde
    H, W = 240, 320
    K = np.array([[288.8, 0, 159.5], [0, 288.8, 119.5], [0, 0, 1]], np.float32)
    ms = ops.MeshSet([icp_ref.two_boxes(), shapes.plane(3.0, 3.0, 4, 4)], device=DEV)
    scenes = [icp_ref.table_scene(0, objects=(0,))]          # the object stands on the table
    rendered = synthetic.render_scenes(ms, scenes, K, H, W)
    visible = int((rendered["mask"][0] == 11).sum())
    assert visible >= 600, visible
    gt = synthetic.scene_frame(ms, scenes, rendered, 0)
    RTg = gt["gt_RTs"][0]
    sg = np.cbrt(np.linalg.det(RTg[:3, :3]))
    Rg, tg = RTg[:3, :3] / sg, RTg[:3, 3]
    R0, t0 = off_by(Rg, tg, 5.0, 10.0)
    RT0 = np.eye(4, dtype=np.float32)
    RT0[:3, :3], RT0[:3, 3] = (sg * R0).astype(np.float32), t0.astype(np.float32)
    frame = dict(depth=rendered["depth"][0], inst_mask=rendered["mask"][0])
    clouds, ok, _ = lde.clouds_from_poses([frame], [0], up(RT0[None]), up(gt["gt_scales"][:1]), 0.6, K, n_pts=512, sampler="device", masks=[11],
                                          seed=0, device=DEV)
    assert bool(ok.all()) and bool(torch.isfinite(clouds).all())
    models = ops.IcpModels.from_meshset(ms, [0], 1024)
    jm = up([0], np.int32)
    RT, info, rmse = pose.refine_poses(models, jm, clouds, up(RT0[None]), 0.01, mode="plane")
    Rs, ts, ss = (x.cpu().numpy() for x in pose.split_RT(up(RT0[None])))                        # the start exactly as the kernel got it
    ref = icp_ref.refine(models.points_normals[0].cpu().numpy(), clouds[0].cpu().numpy(), Rs[0], ts[0], ss[0], 0.01, mode=1)
    Rk, tk, sk = (x.cpu().numpy()[0] for x in pose.split_RT(RT))
    e0, ek, er = icp_ref.pose_error(R0, t0, Rg, tg), icp_ref.pose_error(Rk, tk, Rg, tg), icp_ref.pose_error(ref["R"], ref["t"], Rg, tg)
    info = info.cpu().numpy()
    print("rendered object: %d pixels; start %.3f deg %.3f mm; restatement %.3f deg %.3f mm (%d inliers, %d iterations, rmse %.3e m); "
          "kernel %.3f deg %.3f mm (%d inliers, %d iterations, rmse %.3e m)" % (visible, e0[0], e0[1], er[0], er[1], ref["inliers"], ref["iters"],
                                                                                ref["rmse"], ek[0], ek[1], info[0, 1], info[0, 2], float(rmse[0])))
    assert ref["status"] == 0 and ref["inliers"] >= 0.9 * 512                                    # the condition on the view
    assert info[0, 0] == 0
    assert ek[0] <= 1.5 * er[0] + 0.05 and ek[1] <= 1.5 * er[1] + 0.05
    assert ek[0] < 1.0 and ek[1] < 1.5
    assert abs(float(sk) / sg - 1.0) <= 5e-6            # point-to-plane leaves the scale alone (float32 roundings of the 4x4 round trip)
