"""myEvaluater.track with the supporting plane cut out (support=pose.SupportPlane): the set-up of tests/test_track_icp_gpu.py -- three
instances of icp_ref.two_boxes, six frames of 5 mm and 2 degrees a frame, init_from='previous', point-to-plane ICP with a 1 cm gate,
crops NOT masked -- but with the objects standing ON the table (gap = 0), the case that test stages around.

With the cut, track must equal, bit for bit, a loop written here from ops.plane_fit, ops.plane_cut, clouds_from_poses and
refine_poses; every frame has a plane (within 0.2 degrees / 2 mm of the scene's table; the restatement is within 0.0013 degrees /
0.032 mm, tests/test_plane_cpu.py) and ICP status 0 with at least 400 of 512 inliers; and each object's error against the frame's
ground truth is at most 1.5 x the error of icp_ref.refine on the same cloud and start + 0.05 degrees / 0.05 mm, and below 1 degree /
1.5 mm outright, in every frame.  Simulated on the CPU with the same keyed draws (tests/plane_cases.py simulate): 0.79 degrees /
0.40 mm at worst with the cut, 1.82 degrees / 1.58 mm without.

Without the cut the errors are printed; that the uncut tracker is the worse one is asserted on the restatement alone."""
import numpy as np
import pytest
import torch

from tests import icp_ref
from tests import plane_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N_PTS, RATIO, GATE, K, FRAMES = pc.H, pc.W, pc.N_PTS, pc.RATIO, pc.GATE, pc.K, pc.FRAMES
CLASS_IDS = [3, 3, 3]
PLAIN_KEYS = {"pred_RTs", "pred_scales", "status", "tracked", "icp_status", "icp_inliers", "icp_rmse"}
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
    scenes = [icp_ref.table_scene(k, gap=0.0) for k in range(FRAMES)]
    rendered = synthetic.render_scenes(ms, scenes, K, H, W)
    frames = [dict(depth=rendered["depth"][i], inst_mask=rendered["mask"][i]) for i in range(FRAMES)]
    for k, fr in enumerate(frames):
        assert (fr["inst_mask"] == 200).sum() > 10000        # the table is there
    gts = [synthetic.scene_frame(ms, scenes, rendered, k) for k in range(FRAMES)]
    models = ops.IcpModels.from_meshset(ms, [0], 1024)
    net = PoseNet9D().to(DEV).eval()
    net.load_state_dict(seeded_state_dict(0))
    _S.update(frames=frames, gt=[g["gt_RTs"][:3] for g in gts], models=models, net=net,
              refine=pose.IcpRefine(models, [0, 0, 0], GATE, mode="plane"), support=pose.SupportPlane(),
              init=dict(class_ids=CLASS_IDS, RTs=gts[0]["gt_RTs"][:3].astype(np.float32), scales=gts[0]["gt_scales"][:3].astype(np.float32)))
    ev = myEvaluater(net, sampler="device", seed=pc.SEED)
    kw = dict(n_pts=N_PTS, use_mask=False, refine=_S["refine"], init_from="previous")
    _S.update(ev=ev, cut=ev.track(frames, _S["init"], K, RATIO, support=_S["support"], **kw), uncut=ev.track(frames, _S["init"], K, RATIO, **kw))
    return _S


def by_hand(s):
    """the loop track(support=SupportPlane()) must equal, from the public pieces; poses visit the host between frames.  Also returns,
    per frame, what the refinement was given: (clouds, start poses) as host arrays."""
    from tgpose_amd import ops
    from tgpose_amd.evaluation import load_data_eval as lde
    from tgpose_amd.pose import refine_poses
    ev, init, ref, sup = s["ev"], s["init"], s["refine"], s["support"]
    camk = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32, device=DEV)
    rts, scales = torch.from_numpy(init["RTs"]).clone(), torch.from_numpy(init["scales"]).clone()
    out, given = [], []
    for k, fr in enumerate(s["frames"]):
        with torch.no_grad():
            depth = torch.from_numpy(fr["depth"][None].view(np.int16)).to(DEV)
            plane, pinfo = ops.plane_fit(depth, camk, tol=sup.tol, hypotheses=sup.hypotheses, seed=ev.seed, keys=[k], refine_iters=sup.refine_iters,
                                         min_inliers=100)
            cut = ops.plane_cut(depth, plane, pinfo, camk, sup.margin)
            clouds, ok, pix, counts = lde.clouds_from_poses(dict(depth=cut), [0] * 3, rts.to(DEV), scales.to(DEV), RATIO, K, n_pts=N_PTS,
                                                            sampler="device", masks=None, seed=ev.seed + k, fps_pool=ev.fps_pool, device=DEV,
                                                            return_counts=True)
            start = rts.to(DEV)
            new_rts, info, rmse = refine_poses(ref.models, ref.job_model, clouds, start, ref.max_dist, **ref.kw)
        good = ok.cpu() & (info[:, 0].cpu() == 0)
        rts = torch.where(good[:, None, None], new_rts.cpu(), rts)
        out.append(dict(pred_RTs=rts.clone().numpy(), pred_scales=scales.clone().numpy(), status=counts[:, 3].cpu().numpy(),
                        icp_status=info[:, 0].cpu().numpy(), icp_inliers=info[:, 1].cpu().numpy(), icp_rmse=rmse.cpu().numpy(),
                        plane=plane[0].cpu().numpy(), plane_status=pinfo[0, 0].cpu().numpy(), plane_inliers=pinfo[0, 2].cpu().numpy()))
        given.append((clouds.cpu().numpy(), start.cpu().numpy(), (cut[0] != 0).sum().item(), (depth[0] != 0).sum().item()))
    return out, given


def split(RT):
    s = np.cbrt(np.linalg.det(RT[:3, :3].astype(np.float64)))
    return RT[:3, :3].astype(np.float64) / s, RT[:3, 3].astype(np.float64), s


def errors(results, s):
    return [[icp_ref.pose_error(*split(g["pred_RTs"][o])[:2], *split(s["gt"][k][o])[:2]) for o in range(3)] for k, g in enumerate(results)]


def test_tracking_on_the_table_with_the_plane_cut_out():
    from tgpose_amd import pose
    s = setup()
    got = s["cut"]
    want, given = by_hand(s)
    assert len(got) == len(want) == FRAMES
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) | {"tracked"}, k
        for key in w:
            assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape and np.array_equal(g[key], w[key], equal_nan=True), (k, key)
    model = s["models"].points_normals[0].cpu().numpy()
    print("the CPU simulation has the same model: %s, the same frame 0: %s" % (np.array_equal(model, pc.model()),
                                                                                 np.array_equal(s["frames"][0]["depth"], pc.rendered(0))))
    for k, g in enumerate(got):
        ang, off = pc.plane_error(g["plane"], k)
        print("frame %d: plane %s, %d inliers, %.4f deg %.4f mm off the table; %d of %d valid pixels left" % (k, g["plane"], g["plane_inliers"], ang,
                                                                                                          off, given[k][2], given[k][3]))
        assert g["plane"].shape == (4,) and g["plane_status"] == 0 and g["plane_inliers"] > 60000
        assert ang < 0.2 and off < 2.0, k
        assert g["status"].tolist() == [0, 0, 0] and g["icp_status"].tolist() == [0, 0, 0], k
        assert (g["icp_inliers"] >= 400).all(), (k, g["icp_inliers"])
        Rs, ts, ss = (x.cpu().numpy() for x in pose.split_RT(torch.from_numpy(given[k][1]).to(DEV)))
        for o in range(3):
            Rg, tg, _ = split(s["gt"][k][o])
            ref = icp_ref.refine(model, given[k][0][o], Rs[o], ts[o], ss[o], GATE, mode=1)
            Rk, tk, _ = split(g["pred_RTs"][o])
            ek, er = icp_ref.pose_error(Rk, tk, Rg, tg), icp_ref.pose_error(ref["R"], ref["t"], Rg, tg)
            print("frame %d object %d: restatement %.3f deg %.3f mm, %d inliers | kernel %.3f deg %.3f mm, %d inliers, rmse %.3e m"
                  % (k, o, er[0], er[1], ref["inliers"], ek[0], ek[1], g["icp_inliers"][o], g["icp_rmse"][o]))
            assert ref["status"] == 0
            assert ek[0] <= 1.5 * er[0] + 0.05 and ek[1] <= 1.5 * er[1] + 0.05, (k, o)
            assert ek[0] < 1.0 and ek[1] < 1.5, (k, o)


def test_the_uncut_tracker_is_the_worse_one():
    s = setup()
    cut, uncut = errors(s["cut"], s), errors(s["uncut"], s)
    for k in range(FRAMES):
        print("frame %d: cut %s | uncut %s, inliers %s" % (k, " ".join("%.3f deg %.3f mm" % e for e in cut[k]), " ".join("%.3f deg %.3f mm" % e for e in uncut[k]),
                                                         s["uncut"][k]["icp_inliers"].tolist()))
    wc, wu = max(e[0] for r in cut for e in r), max(e[0] for r in uncut for e in r)
    print("worst rotation error: %.3f deg with the cut, %.3f deg without (x %.2f)" % (wc, wu, wu / wc))
    assert pc.worst(pc.simulate(False))[0] > pc.worst(pc.simulate(True))[0]       # on the restatement alone


def test_result_keys():
    s = setup()
    for g in s["uncut"]:
        assert set(g) == PLAIN_KEYS                                                # support=None: the keys of before
    for g in s["cut"]:
        assert set(g) == PLAIN_KEYS | {"plane", "plane_status", "plane_inliers"}
    with pytest.raises(TypeError):
        s["ev"].track(s["frames"][:1], s["init"], K, RATIO, refine=s["refine"], init_from="previous", support=dict(tol=0.004))
