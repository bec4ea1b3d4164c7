"""myEvaluater.track on rendered sequences: it must equal, frame by frame and bit for bit, a loop written here from the public pieces
(load_data_eval.clouds_from_poses, pose.infer_device, a copy to the host between frames), with the keyed draw and with farthest point
sampling, with and without the instance mask; and an object moved out of reach keeps its pose, is flagged, and leaves the others as
they were.  Every forward draws its pooling samples from torch's global CPU generator (gcn3d.py's torch.randperm), one forward per
frame in both loops, so each side starts from the same torch.manual_seed -- as the evaluater's own test seeds run() and the stages.
The network is randomly initialised (no trained weights exist here): nothing below is a claim about accuracy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, N_PTS, RATIO = 120, 160, 256, 0.3
K = np.array([[144.4, 0, 79.5], [0, 144.4, 59.5], [0, 0, 1]], np.float32)
CLASS_IDS, INST_IDS = [1, 2, 6], [11, 12, 13]               # bottle, bowl, mug
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def _rot_x(deg):
    a = np.deg2rad(deg)
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def setup():
    """the rendered sequences (once): 'base' -- three objects on a table, moved a few millimetres per frame; 'away' -- the same with
    object 1 moved 0.25 m up in frame 2 only, beyond its ball's last radius"""
    if _S:
        return _S
    from tgpose_amd import PoseNet9D, ops, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    ms = ops.MeshSet([shapes.lathe(shapes.PROFILES["bottle"], 16), shapes.lathe(shapes.PROFILES["bowl"], 16),
                      shapes.lathe(shapes.PROFILES["mug"], 16), shapes.plane(3.0, 3.0, 4, 4)], device=DEV)
    R = _rot_x(-160.0)                                      # the models' y axis points up, towards the camera's -y, tilted to the camera
    start = [np.array([-0.2, 0.0, 0.8]), np.array([0.0, 0.02, 0.75]), np.array([0.2, 0.0, 0.8])]
    size = [0.16, 0.14, 0.1]

    def scene(k, away):
        sc = []
        for o in range(3):
            t = start[o] + k * np.array([0.003, 0.002, -0.002])
            if away and o == 1 and k == 2:
                t = t + np.array([0.0, -0.25, 0.0])
            sc.append(dict(mesh=o, inst_id=INST_IDS[o], R=R, t=t, s=size[o]))
        sc.append(dict(mesh=3, inst_id=200, R=_rot_x(-70.0), t=np.array([0.0, 0.12, 0.9]), s=1.0))          # the table
        return sc
    scenes = [scene(k, False) for k in range(4)] + [scene(k, True) for k in range(4)]
    rendered = synthetic.render_scenes(ms, scenes, K, H, W)
    frames = [dict(depth=rendered["depth"][i], inst_mask=rendered["mask"][i]) for i in range(8)]
    for fr in frames:
        for i in INST_IDS:
            assert (fr["inst_mask"] == i).sum() > 60        # every object is seen in every frame
    first = synthetic.scene_frame(ms, scenes, rendered, 0)
    net = PoseNet9D().to(DEV).eval()
    net.load_state_dict(seeded_state_dict(0))
    _S.update(net=net, base=frames[:4], away=frames[4:],
              init=dict(class_ids=CLASS_IDS, RTs=first["gt_RTs"][:3].astype(np.float32), scales=first["gt_scales"][:3].astype(np.float32),
                        inst_ids=INST_IDS))
    return _S


def by_hand(ev, frames, init, sampler, use_mask):
    """the loop track must equal, from the public pieces; poses visit the host between frames"""
    from tgpose_amd.evaluater import RT_TDA_Evaluater as E
    from tgpose_amd.evaluation import load_data_eval as lde
    from tgpose_amd.pose import infer_device
    ids = np.asarray(init["class_ids"])
    f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV)
    cat = f32(ids - 1).reshape(-1, 1)
    mean = f32([E.MEAN_SHAPE_MM[int(c)] for c in ids]) / 1000.0
    sym = f32([E.SYM_INFO[int(c)] for c in ids])
    rts, scales = torch.from_numpy(init["RTs"]).clone(), torch.from_numpy(init["scales"]).clone()
    out = []
    for k, fr in enumerate(frames):
        with torch.no_grad():
            clouds, ok, pix, counts = lde.clouds_from_poses([fr], [0] * len(ids), rts.to(DEV), scales.to(DEV), RATIO, K, n_pts=N_PTS,
                                                            sampler=sampler, masks=init["inst_ids"] if use_mask else None,
                                                            seed=ev.seed + k, fps_pool=ev.fps_pool, device=DEV, return_counts=True)
            new_rts, new_scales = infer_device(ev.net1, torch.nan_to_num(clouds, nan=0.0), cat, mean, sym, ev.max_batch,
                                               eval_outputs_only=ev.eval_outputs_only)
        ok = ok.cpu()
        assert torch.equal(ok, counts[:, 3].cpu() == 0)
        rts = torch.where(ok[:, None, None], new_rts.cpu(), rts)
        scales = torch.where(ok[:, None], new_scales.cpu(), scales)
        out.append((rts.clone(), scales.clone(), counts[:, 3].cpu().clone()))
    return out


@pytest.mark.parametrize("use_mask", [True, False])
@pytest.mark.parametrize("sampler", ["device", "fps"])
def test_track_equals_the_loop_from_public_pieces(sampler, use_mask):
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    s = setup()
    ev = myEvaluater(s["net"], sampler=sampler, seed=5)
    torch.manual_seed(8)
    got = ev.track(s["base"], s["init"], K, RATIO, n_pts=N_PTS, use_mask=use_mask)
    torch.manual_seed(8)
    want = by_hand(ev, s["base"], s["init"], sampler, use_mask)
    assert len(got) == len(want) == 4
    for k, (g, (rts, scales, status)) in enumerate(zip(got, want)):
        print("frame %d status %s" % (k, g["status"].tolist()))
        assert g["pred_RTs"].shape == (3, 4, 4) and g["pred_scales"].shape == (3, 3) and g["status"].dtype == np.int32
        assert torch.equal(torch.from_numpy(g["pred_RTs"]), rts), k
        assert torch.equal(torch.from_numpy(g["pred_scales"]), scales), k
        assert torch.equal(torch.from_numpy(g["status"]), status) and np.array_equal(g["tracked"], g["status"] == 0), k
    assert got[0]["status"].tolist() == [0, 0, 0]           # frame 0 is cropped round the ground truth: every object is found
    assert np.isfinite(got[0]["pred_RTs"]).all() and not np.array_equal(got[0]["pred_RTs"], s["init"]["RTs"])
    # no overlap of fetch and launch: the same results
    torch.manual_seed(8)
    again = myEvaluater(s["net"], sampler=sampler, seed=5, overlap=False).track(s["base"], s["init"], K, RATIO, n_pts=N_PTS, use_mask=use_mask)
    for g, a in zip(got, again):
        assert all(np.array_equal(g[key], a[key]) for key in g)


def test_object_out_of_reach_keeps_its_pose():
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    s = setup()
    ev = myEvaluater(s["net"], sampler="device", seed=5)
    # every frame is cropped round the ground truth of frame 0 here (the objects move by millimetres): what a frame's crop finds
    # does not hang on a random network's previous answer
    def one(fr):
        torch.manual_seed(8)                                # the forward's pooling draws: the same for every call compared below
        return ev.track([fr], s["init"], K, RATIO, n_pts=N_PTS)[0]
    base, away = [one(fr) for fr in s["base"]], [one(fr) for fr in s["away"]]
    for k in range(4):
        assert base[k]["status"].tolist() == [0, 0, 0]
        assert away[k]["status"].tolist() == ([0, 1, 0] if k == 2 else [0, 0, 0]), k
    g = away[2]
    assert g["tracked"].tolist() == [True, False, True]
    assert np.array_equal(g["pred_RTs"][1], s["init"]["RTs"][1]) and np.array_equal(g["pred_scales"][1], s["init"]["scales"][1])
    for o in (0, 2):                                        # the others are unaffected
        assert np.array_equal(g["pred_RTs"][o], base[2]["pred_RTs"][o]) and np.array_equal(g["pred_scales"][o], base[2]["pred_scales"][o])
    # through a sequence: the flagged object's pose is carried into the next frame
    seq = ev.track(s["away"][2:], s["init"], K, RATIO, n_pts=N_PTS)
    assert seq[0]["status"].tolist() == [0, 1, 0] and np.array_equal(seq[0]["pred_RTs"][1], s["init"]["RTs"][1])
    assert seq[1]["status"][1] == 0                         # back within reach of the pose that was kept
    with pytest.raises(ValueError):
        ev.track(s["base"], s["init"], K)
    with pytest.raises(ValueError):
        ev.track(s["base"], s["init"], K, RATIO, sampler="numpy")
