"""TSDF fusion and marching tetrahedra on the device (csrc/tsdf.hip: ops.TsdfVolumes, ops.tsdf_integrate, ops.tsdf_mesh,
ops.tsdf_meshset, pose.scan_models, myEvaluater.scan) against the NumPy restatement tests/tsdf_ref.py on the cases of
tests/tsdf_cases.py: the volumes' and the vertices' BYTES are equal, and a model scanned from rendered frames goes through ICP,
render-and-compare and the distance field as a CAD model does (DESIGN.md section 3 "Models from depth sequences")."""
import numpy as np
import pytest
import torch

from tests import tsdf_cases as tc
from tests import tsdf_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def device_fuse(case, jobs=None, masked=True, volumes=None):
    """ops.tsdf_integrate on a case's jobs -> (volumes, status)"""
    from tgpose_amd import ops
    jobs = np.arange(len(case["job_img"])) if jobs is None else np.asarray(jobs, dtype=np.int64)
    vol = volumes if volumes is not None else ops.TsdfVolumes.from_meta(case["meta"], case["G"], DEV)
    status = ops.tsdf_integrate(vol, up(case["depth"]), up(case["camk"]), up(case["job_img"][jobs]), up(case["job_model"][jobs]),
                                up(case["job_pose"][jobs]), case["trunc"], near=case["near"], mask=up(case["mask"]) if masked else None,
                                job_mask_val=up(case["job_mask_val"][jobs]) if masked else None)
    return vol, status


def same(vol, want, what):
    got_s, got_w = vol.sum.cpu().numpy(), vol.weight.cpu().numpy()
    assert got_w.tobytes() == want[1].tobytes(), (what, "weight", int((got_w != want[1]).sum()))
    assert got_s.tobytes() == want[0].tobytes(), (what, "sum", int((got_s != want[0]).sum()))


# ------------------------------------------------------------------------------------------------------------------ the fusion
@pytest.mark.parametrize("masked", [True, False])
def test_integrate_rules(masked):
    want = tc.fused("rules", masked)
    vol, status = device_fuse(tc.rules(), masked=masked)
    assert status.cpu().numpy().tolist() == want[2].tolist()
    assert want[1].sum() > 0
    same(vol, want, "rules")


@pytest.mark.parametrize("G", [16, 24])
@pytest.mark.parametrize("masked", [True, False])
def test_integrate_several_volumes(G, masked):
    case = tc.several(G)
    want = tc.fused("several%d" % G, masked)
    vol, status = device_fuse(case, masked=masked)
    assert status.cpu().numpy().tolist() == want[2].tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert all(want[1][m].sum() > 0 for m in range(3))
    same(vol, want, "several")
    if masked:
        again, _ = device_fuse(case)                                             # two calls give identical bytes
        assert torch.equal(again.sum, vol.sum) and torch.equal(again.weight, vol.weight)
        split, _ = device_fuse(case, [0, 2, 4, 6])                               # integrating in two calls equals one call
        device_fuse(case, [1, 3, 5], volumes=split)
        assert torch.equal(split.sum, vol.sum) and torch.equal(split.weight, vol.weight)
        assert split.zero_() is split and int(split.sum.abs().sum()) == 0 and int(split.weight.sum()) == 0


def test_integrate_volume_over_the_frames_edge():
    case = tc.straddle()
    want = tc.fused("straddle")
    c = tr.centres(case["meta"][0], case["G"]).astype(np.float64)
    T, K = case["job_pose"][0].astype(np.float64), case["camk"][0].astype(np.float64)
    p = [T[r, 0] * c[0][:, None, None] + T[r, 1] * c[1][None, :, None] + T[r, 2] * c[2][None, None, :] + T[r, 3] for r in range(3)]
    u = K[0] * p[0] / p[2] + K[2]
    assert (u < -1).sum() > 1000 and (u > 1).sum() > 1000 and 0 < want[1].sum() < (u > 1).sum()      # the cube hangs over the left edge
    vol, status = device_fuse(case)
    assert status.cpu().numpy().tolist() == [0]
    same(vol, want, "straddle")


def test_integrate_refusals():
    from tgpose_amd import ops
    case = tc.rules()
    with pytest.raises(ValueError):
        ops.TsdfVolumes(np.zeros((1, 3)), np.ones((1, 3)), G=20, device=DEV)
    with pytest.raises(ValueError):
        ops.TsdfVolumes(np.zeros((1, 3)), np.zeros((1, 3)), G=16, device=DEV)
    vol = ops.TsdfVolumes(np.zeros((2, 3)), [[1, 2, 3], [0.5, 0.1, 0.2]], G=16, device=DEV)
    assert np.array_equal(vol.meta_host, np.stack([tr.tsdf_meta([0, 0, 0], [1, 2, 3], 16), tr.tsdf_meta([0, 0, 0], [0.5, 0.1, 0.2], 16)]))
    assert np.array_equal(vol.meta.cpu().numpy(), vol.meta_host) and len(vol) == 2 and vol.sum.shape == (2, 16, 16, 16)
    assert np.array_equal(vol.meta_host[0], ops.field_meta(np.array([[-0.5, -1, -1.5], [0.5, 1, 1.5]], np.float32), 16, 4)[0])   # field_meta's cube
    args = [up(case[k]) for k in ("depth", "camk", "job_img", "job_model", "job_pose")]
    with pytest.raises(TypeError):
        ops.tsdf_integrate(vol, args[0], args[1], args[2].long(), args[3], args[4], 20.0)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol, args[0], args[1], args[2], args[3], args[4], 0.0)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol, args[0], args[1], args[2], args[3], args[4], 20.0, mask=up(case["mask"]))
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol, args[0], args[1], args[2], args[3][:3], args[4], 20.0)
    with pytest.raises(TypeError):
        ops.tsdf_integrate(None, *args, 20.0)


# ------------------------------------------------------------------------------------------------------------------ the mesher
def device_mesh(vsum, weight, meta, **kw):
    """the volume as model 1 of two (model 0 holds other numbers) -> ops.tsdf_mesh's dict"""
    from tgpose_amd import ops
    G = vsum.shape[0]
    vol = ops.TsdfVolumes.from_meta(np.stack([meta, meta]), G, DEV)
    vol.sum[0].fill_(-7), vol.weight[0].fill_(1)
    vol.sum[1].copy_(up(vsum)), vol.weight[1].copy_(up(weight))
    return ops.tsdf_mesh(vol, 1, **kw)


def same_mesh(out, want, what):
    verts, total, status = want
    n = len(verts) // 3
    assert int(out["n_faces"]) == n and int(out["status"]) == status, what
    assert int(out["counts"].sum()) == total, what
    got = out["verts"].cpu().numpy()
    assert got[:3 * n].tobytes() == verts.tobytes(), (what, int((got[:3 * n].view(np.uint32) != verts.view(np.uint32)).sum()))
    assert not got[3 * n:].any() and out["faces"].cpu().numpy().tolist() == np.arange(len(got)).reshape(-1, 3).tolist()


@pytest.mark.parametrize("G,faces", [(16, 3480), (24, 7752)])
def test_mesh_sphere(G, faces):
    vsum, weight, meta = tc.sphere(G)
    want = tr.mesh(vsum, weight, meta)
    assert want[1] == faces
    out = device_mesh(vsum, weight, meta)
    assert out["verts"].shape == (3 * faces, 3)
    same_mesh(out, want, "sphere")
    again = device_mesh(vsum, weight, meta)
    assert torch.equal(again["verts"], out["verts"])


def test_mesh_every_tetrahedron_case():
    vsum, weight, meta = tc.all_patterns()
    same_mesh(device_mesh(vsum, weight, meta), tr.mesh(vsum, weight, meta), "all patterns")
    for k, case in ((0, 1), (1, 6), (2, 9), (3, 14), (4, 5), (5, 10)):
        one = tc.one_tetrahedron(k, case)
        same_mesh(device_mesh(*one), tr.mesh(*one), (k, case))


def test_mesh_min_weight_and_caps():
    vsum, weight, meta, _ = tc.weak_corner()
    full = tr.mesh(vsum, weight, meta)
    weak = tr.mesh(vsum, weight, meta, min_weight=3)
    assert weak[1] < full[1] == 3480
    same_mesh(device_mesh(vsum, weight, meta, min_weight=3), weak, "min_weight")
    same_mesh(device_mesh(vsum, weight, meta, face_cap=full[1] - 1), tr.mesh(vsum, weight, meta, face_cap=full[1] - 1), "one short")
    assert tr.mesh(vsum, weight, meta, face_cap=full[1] - 1)[2] == 1
    roomy = device_mesh(vsum, weight, meta, face_cap=full[1] + 5)
    assert roomy["verts"].shape == (3 * (full[1] + 5), 3)
    same_mesh(roomy, tr.mesh(vsum, weight, meta, face_cap=full[1] + 5), "roomy")
    same_mesh(device_mesh(vsum, weight, meta, face_cap=0), tr.mesh(vsum, weight, meta, face_cap=0), "cap 0")
    empty = np.zeros_like(vsum)
    out = device_mesh(empty, empty, meta)
    assert out["verts"].shape == (0, 3) and int(out["n_faces"]) == 0 and int(out["status"]) == 0
    with pytest.raises(ValueError):
        device_mesh(vsum, weight, meta, min_weight=0)
    with pytest.raises(ValueError):
        device_mesh(vsum, weight, meta, face_cap=-1)


def test_mesh_surface_in_the_last_cube_row():
    tail = tc.tail_volume()
    want = tr.mesh(*tail)
    assert want[1] > 0
    same_mesh(device_mesh(*tail), want, "tail")


def test_meshset_refuses_an_empty_volume_by_name():
    from tgpose_amd import ops
    vsum, weight, meta = tc.sphere(16)
    vol = ops.TsdfVolumes.from_meta(np.stack([meta, meta]), 16, DEV)
    vol.sum[0].copy_(up(vsum)), vol.weight[0].copy_(up(weight))
    with pytest.raises(ValueError, match="volume 1 has no face"):
        ops.tsdf_meshset(vol)
    vol.sum[1].copy_(up(vsum)), vol.weight[1].copy_(up(weight))
    ms = ops.tsdf_meshset(vol)
    assert isinstance(ms, ops.MeshSet) and ms.n_faces == [3480, 3480] and ms.verts.cpu().numpy()[:3 * 3480].tobytes() == tr.mesh(vsum, weight, meta)[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ the loop
def test_scanned_model_serves_as_a_model():
    """12 rendered turntable frames -> myEvaluater.scan with the true poses -> a MeshSet; on a held-out view ICP from 5 degrees and
    10 mm off ends, with the scanned model, within the true mesh's own translation error plus one voxel edge, and within the angle
    one voxel subtends at the object's radius; render-and-compare scores the scanned mesh within 0.05 of the true mesh; a distance
    field builds from it.  The margin is the volume's resolution: what the scanned model cannot know."""
    got = tc.scan_loop(DEV)
    print(got)
    true, scanned = got["true"], got["scanned"]
    assert got["faces"] > 1000 and got["field_bytes"] == 32 ** 3
    assert true["icp_status"] == 0 and scanned["icp_status"] == 0
    assert scanned["trans_mm"] <= true["trans_mm"] + got["voxel_mm"], (scanned, true, got["voxel_mm"])
    assert scanned["rot_deg"] <= got["voxel_angle_deg"], (scanned, got["voxel_angle_deg"])
    assert abs(scanned["verify_score"] - true["verify_score"]) <= 0.05, (scanned, true)
    assert true["verify_score"] > 0.9


def test_scan_takes_what_track_returned():
    """myEvaluater.scan on records shaped like track's (pred_RTs, pred_scales, tracked) with instance masks: the volumes it makes
    and fills are those of ops.TsdfVolumes + ONE ops.tsdf_integrate call over the tracked (frame, object) pairs, byte for byte; an
    object that is not tracked in a frame is left out of it; the MeshSet is ops.tsdf_meshset's of those volumes"""
    from tgpose_amd import PoseNet9D, ops
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    case = tc.several(16)
    centres = [(0.0, 0.0, 0.6), (0.03, -0.02, 0.62)]
    rts = np.stack([np.stack([tc.pose44(tc.rodrigues((0, 1, 0), 20 + 30 * o + 10 * t), centres[t], 1.0 - 0.2 * o) for o in range(2)]) for t in range(2)])
    scales = np.array([[0.25, 0.2, 0.22], [0.3, 0.3, 0.25]], np.float32)
    tracked = [dict(pred_RTs=rts[0], pred_scales=scales, tracked=np.array([True, True])),
               dict(pred_RTs=rts[1], pred_scales=scales, tracked=np.array([True, False]))]
    frames = [dict(depth=case["depth"][t], inst_mask=case["mask"][t]) for t in range(2)]
    camK = np.stack([np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]]) for k in case["camk"]])
    ev = myEvaluater(PoseNet9D().to(DEV).eval(), sampler="device")
    vol, ms = ev.scan(frames, tracked, camK, G=16, inst_ids=[1, 1])
    want = ops.TsdfVolumes(np.zeros((2, 3), np.float32), scales, 16, device=DEV)
    assert np.array_equal(vol.meta_host, want.meta_host)
    s0 = np.cbrt(np.abs(np.linalg.det(rts[0, :, :3, :3].astype(np.float64))))      # the poses' scales: 1 and 0.8, as float32 holds them
    trunc = 2000.0 * float((want.meta_host[:, 3].astype(np.float64) * s0).max())          # two voxel edges of the coarsest volume
    pairs = [(0, 0), (0, 1), (1, 0)]
    status = ops.tsdf_integrate(want, up(case["depth"]), up(case["camk"]), up(np.array([t for t, _ in pairs], np.int32)),
                                up(np.array([o for _, o in pairs], np.int32)), up(np.stack([rts[t, o, :3] for t, o in pairs])), trunc,
                                mask=up(case["mask"]), job_mask_val=up(np.ones(3, np.uint8)))
    assert status.cpu().numpy().tolist() == [0, 0, 0] and int(want.weight[1].max()) == 1 and int(want.weight[0].max()) == 2
    assert torch.equal(vol.sum, want.sum) and torch.equal(vol.weight, want.weight)
    both = ops.tsdf_meshset(want)
    assert ms.n_faces == both.n_faces and min(ms.n_faces) > 0 and torch.equal(ms.verts, both.verts)
    more, _ = ev.scan(frames[:1], tracked[:1], camK[:1], volumes=vol, inst_ids=[1, 1], trunc_mm=trunc)     # a scan can be continued
    assert more is vol and int(vol.weight[0].max()) == 3
    with pytest.raises(ValueError):
        ev.scan(frames, tracked[:1], camK)
    with pytest.raises(ValueError):
        ev.scan(frames, [rts[0], rts[1]], camK)                                  # no volumes and no pred_scales to size them by


def test_scanned_model_through_search_and_bop():
    """the same scan at G = 32: pose.ModelSearch finds the held-out view's pose from its cloud alone with the scanned model -- search,
    ICP of 16 candidates, render-and-compare -- within what it finds with the true mesh plus one voxel edge, and within the angle one
    voxel subtends at the object's radius; evaluation.bop.score_track scores it on the scanned mesh, MSSD within the true mesh's plus
    one voxel edge"""
    got = tc.scan_downstream(DEV)
    print(got)
    true, scanned = got["true"], got["scanned"]
    assert got["faces"] > 1000
    assert scanned["trans_mm"] <= true["trans_mm"] + got["voxel_mm"], (scanned, true)
    assert scanned["rot_deg"] <= got["voxel_angle_deg"], (scanned, got["voxel_angle_deg"])
    assert scanned["mssd_mm"] <= true["mssd_mm"] + got["voxel_mm"], (scanned, true)
    assert abs(scanned["verify_score"] - true["verify_score"]) <= 0.05 and 0.0 <= scanned["AR"] <= 1.0
