"""bop.score_track on the six-frame sequence of tests/plane_cases.py (three icp_ref.two_boxes standing on the table), tracked as
tests/test_track_verify_gpu.py tracks it: the model-based tracker (init_from='previous', point-to-plane ICP with a 1 cm gate) with
the plane cut out.  The score equals both ops calls applied afterwards to the returned poses, equals the restatement
(tests/bop_ref.py) within the tolerances of tests/test_bop_gpu.py, and every ground-truth pose scored against itself gives zeros
and AR = 1.  No accuracy threshold on the tracker is asserted; the measured errors are printed (DESIGN.md quotes them)."""
import numpy as np
import pytest
import torch

from tests import bop_cases as bc
from tests import bop_ref as br
from tests import icp_ref
from tests import plane_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N_PTS, RATIO, GATE, K, FRAMES = pc.H, pc.W, pc.N_PTS, pc.RATIO, pc.GATE, pc.K, pc.FRAMES
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def half_turn_y():
    """icp_ref.two_boxes is not symmetric; the second group (identity, half a turn about y) only exercises a group of two"""
    return np.stack([bc.turn_z(0, 1), np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0]], np.float64)]).astype(np.float32)


def setup():
    if _S:
        return _S
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    ms = ops.MeshSet(pc.meshes(), device=DEV)
    scenes = [icp_ref.table_scene(k) for k in range(FRAMES)]
    rendered = synthetic.render_scenes(ms, scenes, K, H, W)
    frames = [dict(depth=rendered["depth"][i], inst_mask=rendered["mask"][i]) for i in range(FRAMES)]
    gt0 = synthetic.scene_frame(ms, scenes, rendered, 0)
    net = PoseNet9D().to(DEV).eval()
    net.load_state_dict(seeded_state_dict(0))
    ev = myEvaluater(net, sampler="device", seed=pc.SEED)
    init = dict(class_ids=[3, 3, 3], RTs=gt0["gt_RTs"][:3].astype(np.float32), scales=gt0["gt_scales"][:3].astype(np.float32))
    refine = pose.IcpRefine(ops.IcpModels.from_meshset(ms, [0], 1024), [0, 0, 0], GATE, mode="plane")
    results = ev.track(frames, init, K, RATIO, n_pts=N_PTS, use_mask=False, refine=refine, init_from="previous", support=pose.SupportPlane())
    groups = [ops.SymmetrySet.identity(), half_turn_y()]
    _S.update(ms=ms, frames=frames, results=results, groups=groups, symset=ops.SymmetrySet(groups, device=DEV), gts=bc.track_gts(), job_sym=[0, 1, 0])
    return _S


def test_score_track_equals_the_ops_calls_and_the_restatement():
    from tgpose_amd import ops
    from tgpose_amd.evaluation import bop
    s = setup()
    sc = bop.score_track(s["results"], s["gts"], s["ms"], [0, 0, 0], s["frames"], K, s["symset"], s["job_sym"])
    n = 3
    J = FRAMES * n
    est = np.stack([r["pred_RTs"] for r in s["results"]]).astype(np.float32).reshape(J, 4, 4)[:, :3, :4]
    gt = s["gts"].reshape(J, 4, 4)[:, :3, :4]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    camk1 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
    jm, js = np.zeros(J, np.int32), np.tile(np.asarray(s["job_sym"], np.int32), FRAMES)
    job_img = np.repeat(np.arange(FRAMES, dtype=np.int32), n)
    depth = np.stack([f["depth"] for f in s["frames"]]).astype(np.uint16)
    assert sc["err"].shape == (J, 4) and sc["vsd_err"].shape == (J, 10) and sc["job_tau"].shape == (J, 10) and sc["diameter"].shape == (J,)
    # 1. both ops calls applied afterwards
    e = ops.pose_errors(s["ms"], up(jm), up(est), up(gt), s["symset"], up(js), up(np.tile(camk1, (J, 1))))
    v = ops.pose_vsd(s["ms"], up(depth.view(np.int16)), up(np.tile(camk1, (FRAMES, 1))), up(job_img), up(jm), up(est), up(gt), sc["job_tau"])
    for k, t in (("err", e["err"]), ("sym_best", e["sym_best"]), ("status", e["status"]), ("vsd_counts", v["counts"]), ("vsd_within", v["within"]),
                 ("vsd_err", v["err"])):
        assert torch.equal(sc[k], t), k
    # the thresholds: ceil(float64(tau) * float64(diameter in millimetres)), the diameter the mesh's times the ground truth's scale
    verts = pc.meshes()[0][0].astype(np.float64)
    d_model = max(np.linalg.norm(verts - p, axis=1).max() for p in verts)
    d_m = d_model * np.cbrt(np.abs(np.linalg.det(gt[:, :, :3].astype(np.float64))))
    assert np.allclose(sc["diameter"].cpu().numpy(), d_m, rtol=1e-12, atol=0)
    taus = sc["job_tau"].cpu().numpy()
    assert np.array_equal(taus, np.ceil(bop.TAUS[None] * (sc["diameter"].cpu().numpy() * 1000.0)[:, None]).astype(np.int32)) and taus.min() >= 1
    # 2. the restatement
    case = dict(meshes=pc.meshes(), groups=s["groups"], job_mesh=jm, job_sym=js, pose_est=est, pose_gt=gt, camk=np.tile(camk1, (J, 1)))
    ref = br.pose_errors(near=0.01, **case)
    tol = bc.tolerances(case, br.scale_L(**case))
    got = sc["err"].cpu().numpy()
    assert (ref["status"] == 0).all() and (sc["status"] == 0).all()
    assert (np.abs(got - ref["err"]) <= tol).all(), (np.abs(got - ref["err"]).max(0), tol.max(0))
    best = sc["sym_best"].cpu().numpy()
    for j in range(J):
        for col in (0, 1):
            per = ref["per_sym"][j][:, col]
            assert per[best[j, col]] - per.min() <= tol[j, 2 + col]
    vref = br.pose_vsd(pc.meshes(), depth, np.tile(camk1, (FRAMES, 1)), job_img, jm, est, gt, taus, delta=15)
    for k, r in (("vsd_counts", vref["counts"]), ("vsd_within", vref["within"])):
        assert np.array_equal(sc[k].cpu().numpy(), r), k
    assert np.array_equal(sc["vsd_err"].cpu().numpy().view(np.int32), vref["err"].view(np.int32))
    # AR from the errors, restated
    th = np.arange(0.05, 0.51, 0.05)
    ar_mssd = (got[:, 2, None] < th[None] * sc["diameter"].cpu().numpy()[:, None]).mean()
    ar_mspd = (got[:, 3, None] < (np.arange(5, 51, 5) * (W / 640.0))[None]).mean()
    ar_vsd = (vref["err"].astype(np.float64)[:, :, None] < th[None, None]).mean()
    assert float(sc["AR_MSSD"]) == ar_mssd and float(sc["AR_MSPD"]) == ar_mspd and float(sc["AR_VSD"]) == ar_vsd
    assert abs(float(sc["AR"]) - (ar_mssd + ar_mspd + ar_vsd) / 3) < 1e-15
    print("tracked sequence, %d (frame, object) pairs: ADD mean %.3f max %.3f mm; ADD-S mean %.3f mm; MSSD mean %.3f max %.3f mm; MSPD mean %.3f "
          "max %.3f px; VSD err mean %.4f; AR_MSSD %.4f AR_MSPD %.4f AR_VSD %.4f AR %.4f; diameter %.1f mm"
          % (J, 1e3 * got[:, 0].mean(), 1e3 * got[:, 0].max(), 1e3 * got[:, 1].mean(), 1e3 * got[:, 2].mean(), 1e3 * got[:, 2].max(), got[:, 3].mean(),
             got[:, 3].max(), float(vref["err"].mean()), ar_mssd, ar_mspd, ar_vsd, float(sc["AR"]), 1e3 * d_m[0]))


def test_ground_truth_scored_against_itself_is_perfect():
    from tgpose_amd.evaluation import bop
    s = setup()
    perfect = [dict(pred_RTs=s["gts"][k]) for k in range(FRAMES)]
    sc = bop.score_track(perfect, s["gts"], s["ms"], [0, 0, 0], s["frames"], K, s["symset"], s["job_sym"])
    assert (sc["err"] == 0).all() and (sc["sym_best"] == 0).all() and (sc["status"] == 0).all()
    assert (sc["vsd_err"] == 0).all() and (sc["vsd_counts"][:, 5] > 0).all() and torch.equal(sc["vsd_counts"][:, 4], sc["vsd_counts"][:, 5])
    assert torch.equal(sc["vsd_within"], sc["vsd_counts"][:, 4:5].expand(-1, 10))
    for k in ("AR_MSSD", "AR_MSPD", "AR_VSD", "AR"):
        assert float(sc[k]) == 1.0, k
