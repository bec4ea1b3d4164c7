"""The EMD kernel (csrc/emd.hip) against the numpy restatement of its contract (tests/emd_ref.py): assignment equal, dist bit
for bit; the Python surface above it (emdFunction, calc_emd, calc_cd with the F-score, the evaluater's recon_stats and
compute_degree_cm_mAP(eval_recon=True))."""
import numpy as np
import pytest
import torch

from tests import emd_ref
from tests.test_emd_cpu import SYNSET, check_recon_stats, recon_results

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def clouds(B, n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((B, n, 3), dtype=np.float32), rng.random((B, n, 3), dtype=np.float32)


def run(a, b, eps, iters):
    from tgpose_amd import ops
    dist, asg = ops.emd_fwd(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), eps, iters)
    assert dist.dtype == torch.float32 and asg.dtype == torch.int32 and dist.shape == asg.shape == a.shape[:2]
    return dist.cpu().numpy(), asg.cpu().numpy()


def check(a, b, eps, iters, **kw):
    dist, asg = run(a, b, eps, iters)
    want_d, want_a = emd_ref.emd(a, b, eps, iters, **kw)
    assert np.array_equal(asg, want_a), "assignment differs at %d of %d points" % ((asg != want_a).sum(), asg.size)
    assert np.array_equal(dist.view(np.int32), want_d.view(np.int32))
    return dist, asg


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_points(n):
    """no second best (n = 1: better = -1e9) and a second best that is the only other object"""
    check(*clouds(1, n, 10 + n), 0.005, 50)


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_and_workgroup_tails(n):
    check(*clouds(3, n, n), 0.01, 30)


def test_project_cloud_size_defaults():
    """n = 1028, the project's own N, which the reference's n % 1024 rule refuses; calc_emd's defaults"""
    _, asg = check(*clouds(2, 1028, 1028), 0.005, 50)
    assert (asg >= 0).all() and (asg < 1028).all()


def test_2048_points():
    check(*clouds(2, 2048, 2048), 0.005, 10)


def test_cap():
    """n = tgp_emd_max_points(), two iterations: one auction round, then everyone takes its bid (not a bijection);
    one point more is refused"""
    from tgpose_amd import ops, _lib
    cap = ops.emd_max_points()
    a, b = clouds(1, cap, 5)
    _, asg = check(a, b, 0.005, 2, block=256)
    assert len(np.unique(asg)) < cap
    a1, b1 = clouds(1, cap + 1, 6)
    with pytest.raises(_lib.TgpError, match="TGP_EUNSUPPORTED"):
        run(a1, b1, 0.005, 2)
    with pytest.raises(_lib.TgpError, match="TGP_EINVAL"):
        run(a, b, 0.005, 0)


def test_coincident_lattice():
    """exact ties in d (which k is `best`) and in the increments (which bidder wins): lowest k, lowest j"""
    a, b = emd_ref.lattice()
    _, asg = check(a[None], b[None], 0.01, 200)
    assert np.array_equal(np.sort(asg[0]), np.arange(128))


def test_cloud_against_itself():
    a, _ = clouds(2, 300, 77)
    dist, asg = check(a, a.copy(), 0.005, 50)
    assert not dist.any() and np.array_equal(asg, np.tile(np.arange(300, dtype=np.int32), (2, 1)))


def test_pairs_that_converge_at_different_iterations():
    """one near-identical pair among random ones: once nothing is unassigned the remaining iterations must do nothing"""
    n, eps, iters = 64, 0.01, 200
    a, b = clouds(3, n, 7)
    rng = np.random.default_rng(8)
    b[1] = (a[1][rng.permutation(n)] + rng.uniform(-1e-4, 1e-4, (n, 3))).astype(np.float32)
    at = [emd_ref.emd_pair(a[i], b[i], eps, iters)[2]["converged_at"] for i in range(3)]
    assert None not in at and at[1] < min(at[0], at[2]) and len(set(at)) == 3, at            # precondition
    _, asg = check(a, b, eps, iters)
    assert all(np.array_equal(np.sort(r), np.arange(n)) for r in asg)


def test_batch_independence_and_repeatability():
    a, b = clouds(5, 200, 21)
    d5, a5 = run(a, b, 0.005, 50)
    for i in (0, 3, 4):
        d1, a1 = run(a[i:i + 1], b[i:i + 1], 0.005, 50)
        assert np.array_equal(a1[0], a5[i]) and np.array_equal(d1[0].view(np.int32), d5[i].view(np.int32))
    from tgpose_amd import ops
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    r1, r2 = ops.emd_fwd(ta, tb, 0.005, 50), ops.emd_fwd(ta, tb, 0.005, 50)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


def test_backward_closed_form():
    """grad xyz1 = (grad_dist * 2) * (xyz1 - xyz2[assignment]) bit for bit, grad xyz2 = 0 (the assignment is piecewise constant:
    no gradcheck)"""
    from tgpose_amd.losses.metrics.EMD.emd_module import emdFunction, emdModule
    a, b = clouds(3, 130, 31)
    ta, tb = torch.from_numpy(a).to(DEV).requires_grad_(), torch.from_numpy(b).to(DEV).requires_grad_()
    dist, asg = emdModule()(ta, tb, 0.005, 50)
    assert not asg.requires_grad and dist.requires_grad
    w = torch.from_numpy(np.random.default_rng(32).standard_normal((3, 130)).astype(np.float32)).to(DEV)
    (dist * w).sum().backward()
    want = emd_ref.emd_grad(a, b, w.cpu().numpy(), asg.cpu().numpy())
    assert np.array_equal(ta.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    assert tb.grad is not None and not tb.grad.any()
    d2, a2 = emdFunction.apply(ta.detach(), tb.detach(), 0.005, 50)
    assert torch.equal(d2, dist.detach()) and torch.equal(a2, asg)


def test_calc_emd():
    """sqrt(dist).mean(1) of the kernel's own dist: within n * 2^-24 relative of the float64 mean, the worst case of an fp32
    sum of n terms"""
    from tgpose_amd import ops
    from tgpose_amd.losses.utils_v2.model_utils import calc_emd
    n = 1028
    a, b = clouds(3, n, 41)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = calc_emd(ta, tb)
    dist, _ = ops.emd_fwd(ta, tb, 0.005, 50)
    want = np.sqrt(dist.cpu().numpy().astype(np.float64)).mean(1)
    rel = np.abs(got.cpu().numpy().astype(np.float64) - want) / want
    print("calc_emd relative error", rel, "bound", n * 2.0 ** -24)
    assert got.shape == (3,) and (rel <= n * 2.0 ** -24).all()
    got2 = calc_emd(ta[:, :257], tb[:, :257], eps=0.01, iterations=30)                      # non-contiguous views, other arguments
    d2, _ = ops.emd_fwd(ta[:, :257].contiguous(), tb[:, :257].contiguous(), 0.01, 30)
    assert torch.equal(got2, torch.sqrt(d2).mean(1))


def test_calc_cd_with_fscore():
    from tgpose_amd.losses.chamfer3D.dist_chamfer_3D import chamfer_3DDist
    from tgpose_amd.losses.metrics import fscore
    from tgpose_amd.losses.utils_v2.model_utils import calc_cd
    rng = np.random.default_rng(51)
    gt = torch.from_numpy(rng.random((4, 300, 3), dtype=np.float32)).to(DEV)
    out = (gt[:, :200] + torch.from_numpy(rng.normal(0, 0.006, (4, 200, 3)).astype(np.float32)).to(DEV)).contiguous()
    out[3] += 0.5                                                                         # a pair with F-score 0
    cd_p, cd_t, f1, d1, d2, i1, i2 = calc_cd(out, gt, calc_f1=True, return_raw=True)
    assert d1.shape == (4, 300) and d2.shape == (4, 200)                                  # the kernel is called with (gt, output)
    w1, w2, j1, j2 = chamfer_3DDist()(gt, out)
    assert torch.equal(d1, w1) and torch.equal(d2, w2) and torch.equal(i1, j1) and torch.equal(i2, j2)
    f_want, p1, p2 = fscore(d1, d2)
    assert torch.equal(f1, f_want) and 0 < f1[0] < 1 and f1[3] == 0 and not torch.isnan(f1).any()
    # the precisions are counts / n: the counts exactly, the quotient and the four operations of the harmonic mean each within one
    # fp32 rounding (2^-24 relative) of the CPU's, whose mean may divide where the device multiplies: 2^-21 covers the chain
    assert torch.equal(torch.round(p1 * 300).long(), (d1 < 0.0001).sum(1)) and torch.equal(torch.round(p2 * 200).long(), (d2 < 0.0001).sum(1))
    cpu = fscore(d1.cpu(), d2.cpu())
    for x, y in zip((f_want, p1, p2), cpu):
        np.testing.assert_allclose(x.cpu().numpy(), y.numpy(), rtol=2.0 ** -21, atol=0)
    assert torch.equal(cd_p, (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2) and torch.equal(cd_t, d1.mean(1) + d2.mean(1))
    assert len(calc_cd(out, gt)) == 2 and calc_cd(out, gt, separate=True)[0].shape == (2, 4)


def _records(seeds, dets=3):
    from tests.util import synth_depth_scene
    recs = []
    for s in seeds:
        fr = synth_depth_scene(s, dets)
        rng = np.random.RandomState(s)
        RT = np.tile(np.eye(4), (dets, 1, 1))
        RT[:, :3, 3] = rng.uniform(-0.2, 0.2, (dets, 3)) + np.array([0, 0, 0.8])
        fr.update(gt_class_ids=fr["pred_class_ids"].copy(), gt_RTs=RT, gt_scales=rng.uniform(0.1, 0.3, (dets, 3)),
                  gt_handle_visibility=np.ones(dets, dtype=np.int32))
        recs.append(dict(frame=fr))
    return recs


def test_evaluater_recon_stats(monkeypatch):
    from tgpose_amd import PoseNet9D, seeded_state_dict
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation.load_data_eval import clouds_from_frames
    from tgpose_amd.losses.utils_v2.model_utils import calc_cd, calc_emd
    net = PoseNet9D().to(DEV).eval()
    net.load_state_dict(seeded_state_dict(0))
    recs = _records([501, 502, 503])
    bare = _records([504])[0]["frame"]                          # an image without detections
    bare.update(pred_masks=bare["pred_masks"][:, :, :0], pred_bboxes=bare["pred_bboxes"][:0], pred_class_ids=bare["pred_class_ids"][:0],
                pred_scores=bare["pred_scores"][:0])
    recs.insert(1, dict(frame=bare))
    with pytest.raises(ValueError):
        myEvaluater(net, graph=True, recon_stats=True)

    def seeds():
        np.random.seed(8)
        torch.manual_seed(8)
    seeds()
    got = myEvaluater(net, frames_per_batch=4, recon_stats=True).run(recs)
    assert len(got) == 4
    # the stages one after the other, with the same draws: clouds, one full forward that hands over the reconstruction
    seeds()
    cl = clouds_from_frames([r["frame"] for r in recs], device=DEV)
    pts = torch.cat([c for c in cl if c is not None and c.shape[0]])
    ids = np.concatenate([r["frame"]["pred_class_ids"] for r in recs]).astype(np.float32)
    probe = {}
    with torch.no_grad():
        net(pts, torch.from_numpy(ids - 1).reshape(-1, 1).to(DEV), probe=probe)
    recon, pos = probe["recon"], 0
    for r in got:
        n = len(r["pred_class_ids"])
        cmf, emd = r["chamfer_dis_cass"], r["emd_dis_cass"]
        assert cmf.shape == emd.shape == (n,) and np.isfinite(cmf).all() and np.isfinite(emd).all()
        if n:
            want_c = calc_cd(recon[pos:pos + n], pts[pos:pos + n])[0].cpu().numpy()
            want_e = calc_emd(recon[pos:pos + n], pts[pos:pos + n]).cpu().numpy()
            # the per-detection distances are batch independent; the row means are torch's, whose summation order may follow
            # the batch's shape: a few ulp of an fp32 mean
            np.testing.assert_allclose(cmf, want_c, rtol=1e-6, atol=0)
            np.testing.assert_allclose(emd, want_e, rtol=1e-6, atol=0)
            assert (emd > 0).all() and (cmf > 0).all()
        pos += n
    assert pos == pts.shape[0] and got[1]["pred_RTs"].shape == (0, 4, 4)
    # the poses are those of the full forward without the statistics
    monkeypatch.setenv("TGP_EVAL_FULL_FORWARD", "1")
    seeds()
    plain = myEvaluater(net, frames_per_batch=4).run(recs)
    assert not plain[0].keys() & {"chamfer_dis_cass", "emd_dis_cass"}
    for a, b in zip(got, plain):
        assert np.array_equal(a["pred_RTs"], b["pred_RTs"]) and np.array_equal(a["pred_scales"], b["pred_scales"])


def test_map_with_eval_recon(tmp_path):
    from tgpose_amd.evaluation.metrics import compute_degree_cm_mAP
    res, g = recon_results()
    deg, shift, iou = list(range(0, 61, 5)), [i / 2 for i in range(0, 21, 2)], [i / 100 for i in range(0, 101, 5)]
    kw = dict(iou_pose_thres=0.1, use_matches_for_pose=True, device=DEV)
    base = compute_degree_cm_mAP(res, SYNSET, str(tmp_path), deg, shift, iou, **kw)
    d = {}
    with_recon = compute_degree_cm_mAP(res, SYNSET, str(tmp_path), deg, shift, iou, eval_recon=True, recon_out=d, **kw)
    assert len(with_recon) == 2 and all(np.array_equal(x, y) for x, y in zip(base, with_recon))
    check_recon_stats(d, g)
    compute_degree_cm_mAP(res, SYNSET, None, deg, shift, iou, eval_recon=True, **kw)        # recon_out is optional
