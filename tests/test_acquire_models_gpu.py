"""From a depth frame and a mesh to poses with no network, no detector and no ground truth: pose.ModelSearch and
myEvaluater.acquire_models on the tracker tests' scene (icp_ref.table_scene(k, gap=0.0): three icp_ref.two_boxes standing on the table;
pose.SupportPlane() and pose.Segmenter() find them).

rotation_grid(42, 12) = 504 rotations, G = 32, cap 32, K = 5, stride 2 (1331 shifts), top 16, 128 points per segment, point-to-plane ICP
with a 1 cm gate, render-and-compare with tau 5.
(a) the search of frame 0's clouds, read back: for the second object -- seen from its far side, the one whose anchor lies furthest from
    the cube's centre -- the kernel's whole top list equals tests/search_ref.py's on the same cloud (the field's bytes are the device's:
    tests/test_search_gpu.py holds them against the restatement at sizes where that takes seconds, not a minute).
(b) every object of frames 0 and 3 ends within 2 degrees / 2 mm of the scene's ground truth, and bop.errors gives an MSSD under 2 mm.
    The bound is a condition, not a measurement: the ICP tests end under 1 degree / 1 mm on this scene and a wrong basin is more than
    80 degrees off.
(c) track(init_from='previous') started from acquire_models' result stays within tests/test_track_plane_gpu.py's bounds (1 degree /
    1.5 mm, status 0, at least 400 of 512 inliers) in all six frames."""
import numpy as np
import pytest
import torch

from tests import icp_ref
from tests import plane_cases as pc
from tests import search_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, RATIO, GATE, K, FRAMES = pc.H, pc.W, pc.RATIO, pc.GATE, pc.K, pc.FRAMES
N_SEARCH, G, CAP, SK, STRIDE, TOP, TAU = 128, 32, 32, 5, 2, 16, 5
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def camk_dev():
    return torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32, device=DEV)


def split(RT):
    s = np.cbrt(np.linalg.det(RT[:3, :3].astype(np.float64)))
    return RT[:3, :3].astype(np.float64) / s, RT[:3, 3].astype(np.float64), s


def segments_by_hand(s, k):
    """frame k cut and segmented as acquire_models does it -> (cut depth (1,H,W), ops.Segments, n, the object of each segment)"""
    ev, sup, sg = s["ev"], s["support"], s["segmenter"]
    depth = torch.from_numpy(s["frames"][k]["depth"][None].view(np.int16)).to(DEV)
    cut = sup(depth, camk_dev(), [0], ev.seed)[0]
    seg = sg(cut, camk_dev())
    n = int(seg.info[0, 1])
    centers = seg.centers[0, :n].cpu().numpy().astype(np.float64)
    obj = [int(np.argmin([np.linalg.norm(c - split(g)[1]) for g in s["gt"][k]])) for c in centers]
    return cut, seg, n, obj


def setup():
    if _S:
        return _S
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.tools.lynne_lib import view_sampler
    ms = ops.MeshSet(pc.meshes(), device=DEV)
    scenes = [icp_ref.table_scene(k, gap=0.0) for k in range(FRAMES)]
    rendered = synthetic.render_scenes(ms, scenes, K, H, W)
    frames = [dict(depth=rendered["depth"][i]) for i in range(FRAMES)]
    gts = [synthetic.scene_frame(ms, scenes, rendered, k)["gt_RTs"][:3] for k in range(FRAMES)]
    models = ops.IcpModels.from_meshset(ms, [0], 2048)
    fields = ops.DistanceFields(models, G=G, cap=CAP)
    Rs = view_sampler.rotation_grid(42, 12)
    assert Rs.shape == (504, 3, 3)
    refine = pose.IcpRefine(models, [0], GATE, mode="plane")
    verify = pose.Verify(ms, [0], tau=TAU)
    net = PoseNet9D().to(DEV).eval()                               # the constructor wants one; acquire_models never touches it
    net.load_state_dict(seeded_state_dict(0))
    _S.update(ms=ms, frames=frames, gt=gts, models=models, fields=fields, Rs=Rs, refine=refine, verify=verify,
              search=pose.ModelSearch(fields, models, Rs, K=SK, stride=STRIDE, top=TOP, refine=refine, verify=verify),
              ev=myEvaluater(net, sampler="device", seed=pc.SEED), support=pose.SupportPlane(), segmenter=pose.Segmenter(), init={})
    return _S


def acquired(k):
    s = setup()
    if k not in s["init"]:
        _, _, n, obj = segments_by_hand(s, k)
        assert n == 3 and sorted(obj) == [0, 1, 2]
        scale = [icp_ref.OBJECTS[o]["s"] for o in obj]
        s["init"][k] = (s["ev"].acquire_models(s["frames"][k], s["search"], 0, scale, K, support=s["support"], segmenter=s["segmenter"],
                                               n_pts=N_SEARCH), obj)
    return s["init"][k]


def test_the_search_of_the_hardest_object_equals_the_restatement():
    from tgpose_amd import pose
    from tgpose_amd.evaluation import load_data_eval as lde
    s = setup()
    cut, seg, n, obj = segments_by_hand(s, 0)
    clouds, ok = lde.clouds_from_segments(cut, seg, camk_dev(), n_pts=N_SEARCH, sampler="device", seed=s["ev"].seed)
    M = s["segmenter"].max_segments
    scales = torch.full((M,), icp_ref.OBJECTS[0]["s"], device=DEV)
    for slot, o in enumerate(obj):
        scales[slot] = icp_ref.OBJECTS[o]["s"]
    found = pose.search_poses(s["fields"], torch.zeros(M, dtype=torch.int32, device=DEV), clouds.contiguous(), scales, torch.from_numpy(s["Rs"]).to(DEV),
                              K=SK, stride=STRIDE, top=TOP, return_table=True)
    torch.cuda.synchronize()
    slot = obj.index(1)
    cloud, anchor = clouds[slot].cpu().numpy(), found["anchors"][slot].cpu().numpy()
    fin = np.isfinite(cloud).all(1)
    assert fin.all() and np.abs(cloud.astype(np.float64).mean(0) - anchor).max() < 1e-6
    field = s["fields"].field[0].cpu().numpy()
    want = sr.search(field, s["fields"].meta_host[0], CAP, cloud, None, anchor, float(scales[slot]), s["Rs"], SK, STRIDE, TOP)
    got = {k: found[k][slot].cpu().numpy() for k in ("table", "cost", "rot", "shift", "poses")}
    print("object 1 (slot %d): cost %s rot %s shift %s" % (slot, got["cost"].tolist(), got["rot"].tolist(), got["shift"].tolist()))
    for k in ("table", "cost", "rot", "shift"):
        assert np.array_equal(got[k], want[k]), k
    assert np.allclose(got["poses"], want["poses"], rtol=0, atol=1e-6)
    Rg = split(s["gt"][0][1])[0]
    near = [r for r in got["rot"] if icp_ref.rotation_angle(Rg, s["Rs"][r].astype(np.float64)) < np.deg2rad(20.0)]
    print("rotations of the top list within 20 degrees of the truth: %s" % near)


@pytest.mark.parametrize("k", [0, 3])
def test_every_object_is_found(k):
    from tgpose_amd import ops
    from tgpose_amd.evaluation import bop
    s = setup()
    init, obj = acquired(k)
    assert set(init) >= {"class_ids", "RTs", "scales", "inst_ids", "inst_mask", "boxes", "pixels", "centers", "ok", "info", "search_cost",
                         "search_rank", "icp_status", "icp_inliers", "icp_rmse", "verify_score", "verify_counts"}
    assert init["RTs"].shape == (3, 4, 4) and init["RTs"].dtype == np.float32 and init["ok"].all()
    assert init["search_rank"].dtype == np.int32 and ((0 <= init["search_rank"]) & (init["search_rank"] < TOP)).all()
    gt = np.stack([s["gt"][k][o] for o in obj]).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    e = bop.errors(s["ms"], [0, 0, 0], up(init["RTs"]), up(gt), ops.SymmetrySet([ops.SymmetrySet.identity()], device=DEV), [0, 0, 0],
                   torch.tensor([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], device=DEV))
    err = e["err"].cpu().numpy()
    worst = []
    for slot, o in enumerate(obj):
        Rk, tk, sk = split(init["RTs"][slot])
        Rg, tg, sg = split(gt[slot])
        deg, mm = icp_ref.pose_error(Rk, tk, Rg, tg)
        worst.append((deg, mm, 1e3 * err[slot, 2]))
        print("frame %d object %d (label %d): rank %d cost %d, icp status %d inliers %d, score %.4f: %.3f deg %.3f mm, MSSD %.3f mm"
              % (k, o, slot + 1, init["search_rank"][slot], init["search_cost"][slot], init["icp_status"][slot], init["icp_inliers"][slot],
                 init["verify_score"][slot], deg, mm, 1e3 * err[slot, 2]))
        assert abs(sk - sg) < 1e-6
    assert (e["status"] == 0).all()
    for deg, mm, mssd in worst:
        assert deg < 2.0 and mm < 2.0 and mssd < 2.0, worst


def test_tracking_from_the_acquired_poses():
    from tgpose_amd import ops, pose
    s = setup()
    init, obj = acquired(0)
    models = ops.IcpModels.from_meshset(s["ms"], [0], 1024)
    refine = pose.IcpRefine(models, [0, 0, 0], GATE, mode="plane")
    got = s["ev"].track(s["frames"], init, K, RATIO, n_pts=pc.N_PTS, use_mask=False, refine=refine, init_from="previous", support=s["support"])
    assert len(got) == FRAMES
    for k, g in enumerate(got):
        assert g["status"].tolist() == [0, 0, 0] and g["icp_status"].tolist() == [0, 0, 0], k
        assert (g["icp_inliers"] >= 400).all(), (k, g["icp_inliers"])
        for slot, o in enumerate(obj):
            Rk, tk, _ = split(g["pred_RTs"][slot])
            Rg, tg, _ = split(s["gt"][k][o])
            deg, mm = icp_ref.pose_error(Rk, tk, Rg, tg)
            print("frame %d object %d: %.3f deg %.3f mm, %d inliers" % (k, o, deg, mm, g["icp_inliers"][slot]))
            assert deg < 1.0 and mm < 1.5, (k, o)


def test_refusals():
    from tgpose_amd import ops, pose
    s = setup()
    with pytest.raises(TypeError):
        s["ev"].acquire_models(s["frames"][0], dict(top=4), 0, 0.15, K)
    with pytest.raises(ValueError, match="job_model"):
        s["ev"].acquire_models(s["frames"][0], s["search"], 1, 0.15, K)
    with pytest.raises(ValueError, match="segments"):
        s["ev"].acquire_models(s["frames"][0], s["search"], [0, 0], 0.15, K, support=s["support"], n_pts=N_SEARCH)
    with pytest.raises(ValueError, match="built from"):
        pose.ModelSearch(s["fields"], ops.IcpModels.from_meshset(s["ms"], [0], 64), s["Rs"])
    none = s["ev"].acquire_models(dict(depth=np.zeros((H, W), np.uint16)), s["search"], 0, 0.15, K, n_pts=N_SEARCH)
    assert none["RTs"].shape == (0, 4, 4) and none["search_rank"].shape == (0,) and none["verify_counts"].shape == (0, 8)
