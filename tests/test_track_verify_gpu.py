"""myEvaluater.track(verify=pose.Verify(...)) and acquire_verified on the vanished-object sequence of tests/verify_cases.py: the set-up
of tests/test_track_plane_gpu.py -- three icp_ref.two_boxes standing on the table, six frames, the model-based tracker
(init_from='previous', point-to-plane ICP with a 1 cm gate) with the plane cut out -- but object 2 is absent from frame 3 on.

Verification reports and does not gate: every other result is byte-equal to the same call without ``verify``; verify_counts equal
ops.pose_verify applied afterwards to the returned poses and the frames; 'verified' is True for the two objects that stay, in every
frame, and False for the one that leaves from the frame it leaves.  min_score is not fixed here: it is the midpoint of
tests/test_verify_cpu.py's separation (the least score of a present object at its ground-truth pose, the greatest of an absent one)."""
import numpy as np
import pytest
import torch

from tests import icp_ref
from tests import plane_cases as pc
from tests import verify_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N_PTS, RATIO, GATE, K, FRAMES = pc.H, pc.W, pc.N_PTS, pc.RATIO, pc.GATE, pc.K, pc.FRAMES
VERIFY_KEYS = {"verify_counts", "verify_score", "verified"}
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def setup():
    if _S:
        return _S
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    ms = ops.MeshSet([icp_ref.two_boxes(), shapes.plane(3.0, 3.0, 4, 4)], device=DEV)
    scenes = [icp_ref.table_scene(k, objects=tuple(o for o in range(3) if vc.present(k, o))) for k in range(FRAMES)]
    rendered = synthetic.render_scenes(ms, scenes, K, H, W)
    frames = [dict(depth=rendered["depth"][i], inst_mask=rendered["mask"][i]) for i in range(FRAMES)]
    print("the CPU's frames are the device's: %s" % all(np.array_equal(frames[k]["depth"], vc.vanished_rendered(k)[0]) for k in range(FRAMES)))
    gt0 = synthetic.scene_frame(ms, scenes, rendered, 0)
    models = ops.IcpModels.from_meshset(ms, [0], 1024)
    net = PoseNet9D().to(DEV).eval()
    net.load_state_dict(seeded_state_dict(0))
    lo, hi, mid = vc.separation()
    assert lo > hi
    _S.update(ms=ms, frames=frames, net=net, refine=pose.IcpRefine(models, [0, 0, 0], GATE, mode="plane"), support=pose.SupportPlane(),
              verify=pose.Verify(ms, [0, 0, 0], tau=vc.TAU, min_score=mid), min_score=mid, ev=myEvaluater(net, sampler="device", seed=pc.SEED),
              init=dict(class_ids=[3, 3, 3], RTs=gt0["gt_RTs"][:3].astype(np.float32), scales=gt0["gt_scales"][:3].astype(np.float32)),
              inst_ids=[i["inst_id"] for i in scenes[0][:3]])
    return _S


def camk_dev():
    return torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32, device=DEV)


def cut_frame(s, k):
    """frame k with the plane cut out as track(support=...) cuts it (tests/test_track_plane_gpu.py by_hand)"""
    from tgpose_amd import ops
    sup, camk = s["support"], camk_dev()
    depth = torch.from_numpy(s["frames"][k]["depth"][None].view(np.int16)).to(DEV)
    plane, pinfo = ops.plane_fit(depth, camk, tol=sup.tol, hypotheses=sup.hypotheses, seed=s["ev"].seed, keys=[k], refine_iters=sup.refine_iters,
                                 min_inliers=sup.min_inliers)
    return ops.plane_cut(depth, plane, pinfo, camk, sup.margin)


def afterwards(s, g, depth, mask=None, ids=None):
    """ops.pose_verify applied to a frame's returned poses"""
    from tgpose_amd import ops
    n = len(g["pred_RTs"])
    pose34 = torch.from_numpy(np.ascontiguousarray(g["pred_RTs"][:, :3, :4])).to(DEV)
    z = torch.zeros(n, dtype=torch.int32, device=DEV)
    return ops.pose_verify(s["ms"], depth, camk_dev(), z, z.clone(), pose34, tau=vc.TAU, mask=mask,
                           job_mask_val=None if ids is None else torch.tensor(ids, dtype=torch.uint8, device=DEV))


def check_against_plain(got, plain):
    assert len(got) == len(plain)
    for k, (g, p) in enumerate(zip(got, plain)):
        assert set(g) == set(p) | VERIFY_KEYS, k
        for key in p:
            assert g[key].dtype == p[key].dtype and g[key].tobytes() == p[key].tobytes(), (k, key)
        n = len(g["pred_RTs"])
        assert g["verify_counts"].shape == (n, 8) and g["verify_counts"].dtype == np.int32
        assert g["verify_score"].shape == (n,) and g["verify_score"].dtype == np.float32
        assert g["verified"].shape == (n,) and g["verified"].dtype == np.bool_


def test_the_model_based_tracker_flags_the_object_that_left():
    s = setup()
    kw = dict(n_pts=N_PTS, use_mask=False, refine=s["refine"], init_from="previous", support=s["support"])
    got = s["ev"].track(s["frames"], s["init"], K, RATIO, verify=s["verify"], **kw)
    plain = s["ev"].track(s["frames"], s["init"], K, RATIO, **kw)
    check_against_plain(got, plain)
    for k, g in enumerate(got):
        print("frame %d: status %s icp %s scores %s (min_score %.4f)\n%s" % (k, g["status"].tolist(), g["icp_status"].tolist(), g["verify_score"].tolist(),
                                                                            s["min_score"], g["verify_counts"]))
    for k, g in enumerate(got):
        after = afterwards(s, g, cut_frame(s, k))
        assert np.array_equal(g["verify_counts"], after["counts"].cpu().numpy()), k
        assert np.array_equal(g["verify_score"].view(np.int32), after["score"].cpu().numpy().view(np.int32)), k
        assert np.array_equal(g["verified"], g["verify_score"] >= np.float32(s["min_score"])), k
        assert g["verified"].tolist() == [True, True, vc.present(k, vc.VANISHED)], (k, g["verify_score"].tolist(), s["min_score"])
    again = type(s["ev"])(s["net"], sampler="device", seed=pc.SEED, overlap=False).track(s["frames"], s["init"], K, RATIO, verify=s["verify"], **kw)
    for g, a in zip(got, again):
        for key in g:
            assert g[key].tobytes() == a[key].tobytes(), key


def test_network_tracking_with_instance_masks():
    """init_from='net' with inst_ids and the frames' inst_mask, no plane cut: the byte-equality against the call without verify,
    with torch seeded as the tracking tests seed it, and the mask column"""
    s = setup()
    init = dict(s["init"], inst_ids=s["inst_ids"])
    frames = s["frames"][:3]
    torch.manual_seed(8)
    got = s["ev"].track(frames, init, K, RATIO, n_pts=N_PTS, refine=s["refine"], init_from="net", verify=s["verify"])
    torch.manual_seed(8)
    plain = s["ev"].track(frames, init, K, RATIO, n_pts=N_PTS, refine=s["refine"], init_from="net")
    check_against_plain(got, plain)
    for k, g in enumerate(got):
        depth = torch.from_numpy(frames[k]["depth"][None].view(np.int16)).to(DEV)
        mask = torch.from_numpy(frames[k]["inst_mask"][None]).to(DEV)
        after = afterwards(s, g, depth, mask, s["inst_ids"])
        assert np.array_equal(g["verify_counts"], after["counts"].cpu().numpy()), k
        bare = afterwards(s, g, depth)
        assert np.array_equal(np.delete(g["verify_counts"], 5, axis=1), np.delete(bare["counts"].cpu().numpy(), 5, axis=1)), k
    with pytest.raises(TypeError):
        s["ev"].track(frames[:1], init, K, RATIO, verify=dict(tau=5))
    with pytest.raises(ValueError, match="mesh indices"):
        from tgpose_amd import pose
        s["ev"].track(frames[:1], init, K, RATIO, n_pts=N_PTS, verify=pose.Verify(s["ms"], [0, 0]))


def test_acquire_verified():
    """the three keys with n rows, equal to ops.pose_verify applied afterwards against the cut frame and the label image; every
    other key as acquire returns it; no row for a frame without a segment"""
    from tgpose_amd import ops, pose
    s = setup()
    ev = s["ev"]
    one = pose.Verify(s["ms"], [0], tau=vc.TAU, min_score=s["min_score"])
    torch.manual_seed(3)
    got = ev.acquire_verified(s["frames"][0], 3, one, K, support=s["support"], n_pts=N_PTS)
    torch.manual_seed(3)
    plain = ev.acquire(s["frames"][0], 3, K, support=s["support"], n_pts=N_PTS)
    assert set(got) == set(plain) | VERIFY_KEYS and len(plain["RTs"]) == 3
    for key in plain:
        assert got[key].tobytes() == plain[key].tobytes(), key
    assert got["verify_counts"].shape == (3, 8) and got["verify_score"].shape == (3,) and got["verified"].shape == (3,)
    labels = torch.from_numpy(got["inst_mask"][None]).to(DEV)
    after = afterwards(s, dict(pred_RTs=got["RTs"]), cut_frame(s, 0), labels, [1, 2, 3])
    print("acquire: scores %s\n%s" % (got["verify_score"].tolist(), got["verify_counts"]))
    assert np.array_equal(got["verify_counts"], after["counts"].cpu().numpy())
    assert np.array_equal(got["verified"], got["verify_score"] >= np.float32(s["min_score"]))
    torch.manual_seed(3)
    each = ev.acquire_verified(s["frames"][0], 3, pose.Verify(s["ms"], [0, 0, 0], tau=vc.TAU, min_score=s["min_score"]), K, support=s["support"], n_pts=N_PTS)
    assert np.array_equal(each["verify_counts"], got["verify_counts"])
    with pytest.raises(ValueError, match="mesh indices"):
        ev.acquire_verified(s["frames"][0], 3, pose.Verify(s["ms"], [0, 0]), K, support=s["support"], n_pts=N_PTS)
    with pytest.raises(TypeError):
        ev.acquire_verified(s["frames"][0], 3, None, K)
    none = ev.acquire_verified(dict(depth=np.zeros((H, W), np.uint16)), 3, one, K, n_pts=N_PTS)
    assert none["RTs"].shape == (0, 4, 4) and none["verify_counts"].shape == (0, 8) and none["verify_counts"].dtype == np.int32
    assert none["verify_score"].shape == (0,) and none["verified"].shape == (0,) and none["verified"].dtype == np.bool_
