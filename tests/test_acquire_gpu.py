"""From a depth frame and a category to tracked poses with no detector result and no ground truth: load_data_eval.clouds_from_segments
and myEvaluater.acquire on the scene of tests/test_track_plane_gpu.py (three icp_ref.two_boxes standing on the table, seeded weights).

clouds_from_segments must equal, bit for bit, clouds_from_frames fed host masks and boxes made from the restatement's labels (one
mask channel per slot, so that detection d is slot d on both paths and the keyed draw has the same key), for 'device' and 'fps'.
acquire must equal a loop written here from the public pieces, its inst_mask the restatement's labelling of the cut frame, its
centroids within 5 mm of the centroids of the instances' visible points, and track must run from its result."""
import numpy as np
import pytest
import torch

from tests import icp_ref
from tests import plane_cases as pc
from tests import segment_cases as sc
from tests import segment_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N_PTS, RATIO, GATE, K, FRAMES = pc.H, pc.W, pc.N_PTS, pc.RATIO, pc.GATE, pc.K, pc.FRAMES
SLOTS = 4                    # mask channels per frame in the clouds test: three objects and an empty slot
PLAIN_KEYS = {"pred_RTs", "pred_scales", "status", "tracked", "icp_status", "icp_inliers", "icp_rmse"}      # tests/test_track_plane_gpu.py test_result_keys
INIT_KEYS = {"class_ids", "RTs", "scales", "inst_ids", "inst_mask", "boxes", "pixels", "centers", "ok", "info"}
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
    frames = [dict(depth=rendered["depth"][i]) for i in range(FRAMES)]
    models = ops.IcpModels.from_meshset(ms, [0], 1024)
    net = PoseNet9D().to(DEV).eval()
    net.load_state_dict(seeded_state_dict(0))
    ev = myEvaluater(net, sampler="device", seed=pc.SEED)
    _S.update(frames=frames, masks=[rendered["mask"][i] for i in range(FRAMES)], inst_ids=[i["inst_id"] for i in scenes[0][:3]], ev=ev, net=net,
              refine=pose.IcpRefine(models, [0, 0, 0], GATE, mode="plane"), support=pose.SupportPlane(), segmenter=pose.Segmenter())
    torch.manual_seed(3)
    _S["init"] = ev.acquire(frames[0], 3, K, support=_S["support"], segmenter=_S["segmenter"], n_pts=N_PTS)
    return _S


@pytest.mark.parametrize("sampler", ["device", "fps"])
def test_clouds_from_segments_equal_clouds_from_frames(sampler):
    from tgpose_amd import ops
    from tgpose_amd.evaluation import load_data_eval as lde
    cut = np.stack([sc.cut_frame(k) for k in range(FRAMES)])
    depth = torch.from_numpy(cut.view(np.int16)).to(DEV)
    seg = ops.segment_depth(depth, max_step=sc.STEP, connectivity=4, min_pixels=sc.MIN_PIXELS, max_segments=SLOTS)
    got, ok = lde.clouds_from_segments(depth, seg, K, n_pts=N_PTS, sampler=sampler, seed=17)
    assert got.shape == (FRAMES * SLOTS, N_PTS, 3) and ok.shape == (FRAMES * SLOTS,) and ok.dtype == torch.bool
    frames = []
    for k in range(FRAMES):
        ref = sr.segment(cut[k], sc.STEP, 4, sc.MIN_PIXELS, SLOTS)
        assert ref["info"].tolist()[:3] == [0, 3, 3] and np.array_equal(seg.labels[k].cpu().numpy(), ref["labels"])
        masks = np.stack([ref["labels"] == m + 1 for m in range(SLOTS)], axis=2)
        frames.append(dict(depth=cut[k], pred_masks=masks, pred_bboxes=ref["stats"][:, 1:5].copy()))
    want, want_ok = lde.clouds_from_frames(frames, K, n_pts=N_PTS, sampler=sampler, seed=17, device=DEV)
    want, want_ok = torch.cat(want).cpu().numpy(), torch.cat(want_ok).cpu().numpy()
    got, ok = got.cpu().numpy(), ok.cpu().numpy()
    assert np.array_equal(ok, want_ok) and ok.reshape(FRAMES, SLOTS).tolist() == [[True] * 3 + [False]] * FRAMES
    assert np.array_equal(got, want, equal_nan=True)
    g = got.reshape(FRAMES, SLOTS, N_PTS, 3)
    assert np.isnan(g[:, 3]).all() and np.isfinite(g[:, :3]).all()                  # an empty slot: NaN rows, ok False


def by_hand(s):
    """acquire from the public pieces, with the same seeds"""
    from tgpose_amd import ops
    from tgpose_amd.evaluation import load_data_eval as lde
    from tgpose_amd.evaluater.RT_TDA_Evaluater import MEAN_SHAPE_MM, SYM_INFO
    from tgpose_amd.pose import infer_device
    ev, sup, sg = s["ev"], s["support"], s["segmenter"]
    M = sg.max_segments
    camk = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32, device=DEV)
    with torch.no_grad():
        depth = torch.from_numpy(s["frames"][0]["depth"][None].view(np.int16)).to(DEV)
        plane, pinfo = ops.plane_fit(depth, camk, tol=sup.tol, hypotheses=sup.hypotheses, seed=ev.seed, keys=[0], refine_iters=sup.refine_iters,
                                     min_inliers=sup.min_inliers)
        cut = ops.plane_cut(depth, plane, pinfo, camk, sup.margin)
        seg = ops.segment_depth(cut, max_step=sg.max_step, connectivity=sg.connectivity, min_pixels=sg.min_pixels, max_segments=M, camk=camk)
        pts, ok = lde.clouds_from_segments(cut, seg, K, n_pts=N_PTS, sampler="device", seed=ev.seed)
        cat = torch.full((M, 1), 2.0, device=DEV)
        mean = torch.tensor([MEAN_SHAPE_MM[3]] * M, dtype=torch.float32, device=DEV) / 1000.0
        sym = torch.tensor([SYM_INFO[3]] * M, dtype=torch.float32, device=DEV)
        rts, scales = infer_device(s["net"], torch.nan_to_num(pts, nan=0.0), cat, mean, sym, ev.max_batch, eval_outputs_only=ev.eval_outputs_only)
    n = int(seg.info[0, 1])
    return dict(RTs=rts[:n].cpu().numpy(), scales=scales[:n].cpu().numpy(), cut=cut[0].cpu().numpy().view(np.uint16), seg=seg, n=n)


def test_acquire_equals_the_public_pieces_and_the_restatement():
    s = setup()
    init = s["init"]
    assert set(init) == INIT_KEYS
    torch.manual_seed(3)
    hand = by_hand(s)
    n = hand["n"]
    assert n == 3 and init["info"].tolist()[:3] == [0, 3, 3]
    assert init["RTs"].shape == (3, 4, 4) and init["scales"].shape == (3, 3) and init["RTs"].dtype == np.float32
    assert np.array_equal(init["RTs"], hand["RTs"]) and np.array_equal(init["scales"], hand["scales"]) and np.isfinite(init["RTs"]).all()
    assert init["class_ids"].tolist() == [3, 3, 3] and init["inst_ids"].tolist() == [1, 2, 3] and init["ok"].tolist() == [True] * 3
    print("the device's cut frame equals the restatement's: %s" % np.array_equal(hand["cut"], sc.cut_frame(0)))
    ref = sr.segment(hand["cut"], 10, 4, 50, 32, camk=pc.CAMK)
    assert init["inst_mask"].dtype == np.uint8 and np.array_equal(init["inst_mask"], ref["labels"])
    assert np.array_equal(init["boxes"], ref["stats"][:3, 1:5]) and np.array_equal(init["pixels"], ref["stats"][:3, 0])
    assert np.array_equal(init["centers"], ref["centers"][:3]) and np.array_equal(init["info"], ref["info"])
    # the centroid of each instance's visible points, from the rendered instance mask
    depth, mask = s["frames"][0]["depth"], s["masks"][0]
    seen = set()
    for r in range(3):
        ids, votes = np.unique(mask[init["inst_mask"] == r + 1], return_counts=True)
        inst = int(ids[np.argmax(votes)])
        assert inst in s["inst_ids"] and inst not in seen
        seen.add(inst)
        ys, xs = np.nonzero(mask == inst)
        z = depth[ys, xs].astype(np.float64) / 1000.0
        centroid = np.array([((xs - K[0, 2]) * z / K[0, 0]).mean(), ((ys - K[1, 2]) * z / K[1, 1]).mean(), z.mean()])
        dist = 1000.0 * np.linalg.norm(init["centers"][r].astype(np.float64) - centroid)
        print("segment %d: instance %d, %d of its %d pixels, centroid %.2f mm from the instance's" % (r + 1, inst, init["pixels"][r], len(ys), dist))
        assert dist < 5.0, (r, dist)


def test_class_ids_per_segment_and_a_frame_without_segments():
    s = setup()
    ev = s["ev"]
    torch.manual_seed(3)
    again = ev.acquire(s["frames"][0], [3, 3, 3], K, support=s["support"], segmenter=s["segmenter"], n_pts=N_PTS)
    for key in INIT_KEYS:
        assert np.array_equal(again[key], s["init"][key]), key
    with pytest.raises(ValueError):
        ev.acquire(s["frames"][0], [3, 3], K, support=s["support"], n_pts=N_PTS)
    with pytest.raises(ValueError):
        ev.acquire(s["frames"][0], 9, K)
    with pytest.raises(TypeError):
        ev.acquire(s["frames"][0], 3, K, segmenter=dict(max_step=10))
    none = ev.acquire(dict(depth=np.zeros((H, W), np.uint16)), 3, K, n_pts=N_PTS)
    assert set(none) == INIT_KEYS and none["RTs"].shape == (0, 4, 4) and none["scales"].shape == (0, 3) and none["centers"].shape == (0, 3)
    assert none["info"].tolist() == [0, 0, 0, 0] and not none["inst_mask"].any() and none["boxes"].shape == (0, 4) and len(none["class_ids"]) == 0


def test_track_runs_from_what_acquire_returns():
    s = setup()
    torch.manual_seed(4)
    out = s["ev"].track(s["frames"], s["init"], K, RATIO, n_pts=N_PTS, refine=s["refine"], init_from="net")
    assert len(out) == FRAMES
    for g in out:
        assert set(g) == PLAIN_KEYS
        assert g["pred_RTs"].shape == (3, 4, 4) and g["pred_scales"].shape == (3, 3) and np.isfinite(g["pred_RTs"]).all()
