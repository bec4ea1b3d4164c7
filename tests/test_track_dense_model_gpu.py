"""myEvaluater.track with dense model-based registration (refine=pose.DenseModelRefine) on tests/test_track_icp_gpu.py's rendered
sequence, with its constants: three instances of icp_ref.two_boxes over a table, six frames of 5 mm and 2 degrees a frame, NOT masked
-- the table's pixels are in every rectangle -- and a gate of 1 cm.  (On the CPU the restatement alone -- meshmaps_ref maps,
icp_dense_ref.refine, the frames rendered by render_ref -- meets every condition below on this scene without a mask: at most 0.062
degrees / 0.052 mm, at least 1793 inliers of 1874 candidates; DESIGN.md section 3 "Mesh maps and dense model-based tracking".)

init_from='previous' is the dense model-based tracker: no crop and no forward, the frame itself is registered to the objects'
rasterised meshes.  track must equal, bit for bit, a loop written here from the public pieces with a visit to the host between
frames; every frame must have status 0 with at least half of the candidates inliers, for the NumPy restatement as well; and the error
against each frame's ground truth is bounded by 1.5 x the restatement's on the same frame and start + 0.05 degrees / 0.05 mm, and by
the sparse tracker's outright bound of 1 degree / 1.5 mm, in every frame."""
import numpy as np
import pytest
import torch

from tests import icp_dense_ref as dr
from tests import icp_ref
from tests import meshmaps_ref as mr
from tests import test_track_icp_gpu as ti

pytestmark = pytest.mark.gpu
DEV, H, W, K, GATE, FRAMES = ti.DEV, ti.H, ti.W, ti.K, ti.GATE, ti.FRAMES
MAP_H, MAP_W = 96, 128
DENSE_KEYS = {"pred_RTs", "pred_scales", "status", "icp_status", "icp_inliers", "icp_rmse", "icp_candidates", "ray_hits"}
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def setup():
    if _S:
        return _S
    from tgpose_amd import ops, pose
    from tgpose_amd.datasets import shapes
    s = ti.setup()
    meshes = [icp_ref.two_boxes(), shapes.plane(3.0, 3.0, 4, 4)]
    ms = ops.MeshSet(meshes, device=DEV)
    _S.update(s, meshes=meshes, meshset=ms, dense=pose.DenseModelRefine(ms, [0, 0, 0], GATE, h=MAP_H, w=MAP_W))
    return _S


def by_hand(s, frames):
    """the loop track must equal, from the public pieces; poses visit the host between frames.  Also returns each frame's start poses."""
    init, ref = s["init"], s["dense"]
    rts = torch.from_numpy(init["RTs"]).clone()
    camk = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32).to(DEV)
    job_img = torch.zeros(3, dtype=torch.int32, device=DEV)
    out, given = [], []
    for fr in frames:
        depth = torch.from_numpy(fr["depth"].view(np.int16)[None]).to(DEV)
        start = rts.to(DEV)
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")                      # nothing is read back
        try:
            with torch.no_grad():
                new, info, rmse, hits = ref(depth, start, camk, job_img)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        given.append(rts.clone().numpy())
        rts = new.cpu()
        out.append(dict(pred_RTs=rts.clone().numpy(), pred_scales=init["scales"].copy(), status=np.zeros(3, np.int32),
                        icp_status=info[:, 0].cpu().numpy(), icp_inliers=info[:, 1].cpu().numpy(), icp_rmse=rmse.cpu().numpy(),
                        icp_candidates=info[:, 3].cpu().numpy(), ray_hits=hits.cpu().numpy()))
    return out, given


def same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == DENSE_KEYS | {"tracked"} == set(w) | {"tracked"}, k
        for key in w:
            assert g[key].dtype == w[key].dtype and np.array_equal(g[key], w[key], equal_nan=True), (k, key)
        assert np.array_equal(g["tracked"], g["status"] == 0)


def test_dense_model_tracking_follows_the_objects():
    from tgpose_amd import pose
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    s = setup()
    got = myEvaluater(s["net"], sampler="device", seed=5).track(s["frames"], s["init"], K, use_mask=False, refine=s["dense"], init_from="previous")
    want, given = by_hand(s, s["frames"])
    same(got, want)
    again = myEvaluater(s["net"], sampler="device", seed=5, overlap=False).track(s["frames"], s["init"], K, None, use_mask=False, refine=s["dense"],
                                                                                 init_from="previous")
    same(again, want)
    camk = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], np.float32)
    zero = np.zeros(1, np.int32)
    for k in range(FRAMES):
        g = got[k]
        assert g["status"].tolist() == [0, 0, 0] and g["icp_status"].tolist() == [0, 0, 0], k
        assert (2 * g["icp_inliers"] >= g["icp_candidates"]).all() and (g["icp_candidates"] >= 300).all(), (k, g["icp_inliers"], g["icp_candidates"])
        assert np.array_equal(g["pred_scales"], s["init"]["scales"])                             # carried through
        start = torch.from_numpy(given[k]).to(DEV)
        Rs, ts, ss = (x.cpu().numpy() for x in pose.split_RT(start))                             # the start as the kernel got it
        P = pose.verify_job_pose(start).cpu().numpy()
        for o in range(3):
            Rg, tg, _ = ti.split(s["gt"][k][o])
            win = mr.windows(s["meshes"], camk, zero, zero, P[o:o + 1], MAP_H, MAP_W, H, W)
            maps = mr.maps(s["meshes"], camk, zero, zero, P[o:o + 1], win, MAP_H, MAP_W)
            ref = dr.refine(s["frames"][k]["depth"], camk[0], dict(z=maps["z"][0], vertex=maps["vertex"][0], normal=maps["normal"][0]), win[0], P[o],
                            dr.rects(win, MAP_H, MAP_W, H, W)[0], Rs[o], ts[o], ss[o], GATE)
            Rk, tk, _ = ti.split(g["pred_RTs"][o])
            e0, ek, er = icp_ref.pose_error(Rs[o], ts[o], Rg, tg), icp_ref.pose_error(Rk, tk, Rg, tg), icp_ref.pose_error(ref["R64"], ref["t64"], Rg, tg)
            print("frame %d object %d: start %.3f deg %.3f mm | restatement %.3f deg %.3f mm, %d inliers of %d, %d iterations | kernel %.3f deg %.3f mm, "
                  "%d inliers of %d, %d hits, rmse %.3e m" % (k, o, e0[0], e0[1], er[0], er[1], ref["inliers"], ref["candidates"], ref["iters"], ek[0], ek[1],
                                                            g["icp_inliers"][o], g["icp_candidates"][o], g["ray_hits"][o], g["icp_rmse"][o]))
            assert ref["status"] == 0 and 2 * ref["inliers"] >= ref["candidates"] >= 300, (k, o)
            assert (g["icp_candidates"][o], g["ray_hits"][o]) == (ref["candidates"], maps["count"][0]), (k, o)   # the same maps, the same start
            assert ek[0] <= 1.5 * er[0] + 0.05 and ek[1] <= 1.5 * er[1] + 0.05, (k, o)
            assert ek[0] < 1.0 and ek[1] < 1.5, (k, o)


def test_an_empty_frame_moves_nothing_and_tracking_goes_on():
    """an all-zero frame between frames 2 and 3: no candidate, ICP status 1, the poses of frame 2 stay; frames 3.. are tracked again"""
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    s = setup()
    blank = dict(depth=np.zeros((H, W), np.uint16))
    frames = s["frames"][:3] + [blank] + s["frames"][3:]
    got = myEvaluater(s["net"], sampler="device", seed=5).track(frames, s["init"], K, use_mask=False, refine=s["dense"], init_from="previous")
    same(got, by_hand(s, frames)[0])
    assert len(got) == FRAMES + 1
    assert got[3]["icp_status"].tolist() == [1, 1, 1] and got[3]["icp_candidates"].tolist() == [0, 0, 0] and got[3]["status"].tolist() == [0, 0, 0]
    assert (got[3]["ray_hits"] > 1000).all()                                                    # the maps were there: the frame was not
    assert got[3]["pred_RTs"].tobytes() == got[2]["pred_RTs"].tobytes()
    full = myEvaluater(s["net"], sampler="device", seed=5).track(s["frames"], s["init"], K, use_mask=False, refine=s["dense"], init_from="previous")
    for k in range(4, FRAMES + 1):
        assert got[k]["icp_status"].tolist() == [0, 0, 0], k
        for key in DENSE_KEYS:                                                                   # as if the empty frame had not been
            assert np.array_equal(got[k][key], full[k - 1][key], equal_nan=True), (k, key)


def test_gate_and_few_hits_keep_the_pose():
    """a gate no solve can pass (more inliers than candidates x 1 and an rmse of 0) gives DENSE_GATED, more hits than the map has cells
    gives RAYCAST_FEW_HITS; either way the pose comes back in its own bits"""
    from tgpose_amd import pose
    s = setup()
    camk = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32).to(DEV)
    job_img = torch.zeros(3, dtype=torch.int32, device=DEV)
    depth = torch.from_numpy(s["frames"][1]["depth"].view(np.int16)[None]).to(DEV)
    start = torch.from_numpy(s["init"]["RTs"]).to(DEV)
    gated = pose.DenseModelRefine(s["meshset"], [0, 0, 0], GATE, h=MAP_H, w=MAP_W, max_rmse=0.0)(depth, start, camk, job_img)
    few = pose.DenseModelRefine(s["meshset"], [0, 0, 0], GATE, h=MAP_H, w=MAP_W, min_hits=MAP_H * MAP_W + 1)(depth, start, camk, job_img)
    plain = s["dense"](depth, start, camk, job_img)
    assert plain[1][:, 0].tolist() == [0, 0, 0] and not torch.equal(plain[0], start)
    assert gated[1][:, 0].tolist() == [pose.DENSE_GATED] * 3 and torch.equal(gated[0], start) and torch.equal(gated[1][:, 1:], plain[1][:, 1:])
    assert few[1][:, 0].tolist() == [pose.RAYCAST_FEW_HITS] * 3 and torch.equal(few[0], start) and torch.equal(few[3], plain[3])
    with pytest.raises(ValueError):
        pose.DenseModelRefine(s["meshset"], [0, 0, 0], GATE, normals="vertex")                  # the set has no vertex normals
    with pytest.raises(ValueError):
        pose.DenseModelRefine(s["meshset"], [0, 5, 0], GATE)                                    # no such mesh
    with pytest.raises(ValueError):
        pose.DenseModelRefine(s["meshset"], [0, 0], GATE)(depth, start, camk, job_img)          # two meshes for three poses


def test_masked_and_network_starts_and_todays_keys():
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    s = setup()
    ev = myEvaluater(s["net"], sampler="device", seed=5)
    init = dict(s["init"], inst_ids=[ob["inst_id"] for ob in icp_ref.OBJECTS])
    masked = ev.track(s["frames"][:2], init, K, refine=s["dense"], init_from="previous")
    open_ = ev.track(s["frames"][:2], s["init"], K, use_mask=False, refine=s["dense"], init_from="previous")
    for g, o in zip(masked, open_):
        assert set(g) == DENSE_KEYS | {"tracked"} and g["icp_status"].tolist() == [0, 0, 0]
        assert (g["icp_candidates"] < o["icp_candidates"]).all() and (g["icp_candidates"] >= 300).all()   # the table's pixels are out
    torch.manual_seed(8)
    net = ev.track(s["frames"][:1], s["init"], K, ti.RATIO, n_pts=ti.N_PTS, use_mask=False, refine=s["dense"], init_from="net")
    assert set(net[0]) == DENSE_KEYS | {"tracked"} and np.isfinite(net[0]["pred_RTs"]).all()
    with pytest.raises(ValueError):
        ev.track(s["frames"][:1], s["init"], K, use_mask=False, refine=s["dense"], init_from="net")       # the crop needs its ratio
    sparse = ev.track(s["frames"][:1], s["init"], K, ti.RATIO, n_pts=ti.N_PTS, use_mask=False, refine=s["refine"], init_from="previous")
    assert set(sparse[0]) == {"pred_RTs", "pred_scales", "status", "tracked", "icp_status", "icp_inliers", "icp_rmse"}    # an IcpRefine: today's keys only
