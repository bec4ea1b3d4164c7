"""Pose verification without a GPU: the ABI's two new entry points and the argument checks of the C entry, the wrappers, and the
NumPy restatement of the contract (tests/verify_ref.py) against closed forms -- a rectangle against its own rendered depth and
against that depth shifted to each side of tau -- and against what it is for: a ground-truth pose scores above a displaced one, and
an object that is there scores above one that has left."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import plane_cases as pc
from tests import render_cases as rc
from tests import verify_cases as vc
from tests import verify_ref as vr

NAMES = ("tgp_pose_verify", "tgp_verify_workspace_bytes")
FIELDS = ["depth", "camk", "verts", "faces", "vptr", "fptr", "M", "n_verts", "n_faces", "max_verts", "max_faces", "job_img", "job_mesh",
          "job_pose", "mask", "job_mask_val", "S", "H", "W", "J", "tau", "near", "counts", "score", "workspace", "workspace_bytes"]
C = vr.COL


def test_header_declares_and_library_exports_the_entry_points():
    from tgpose_amd import _lib, ops
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(handle, name) is not None
    assert _lib.ABI_VERSION == 9
    assert "tgp_verify_args" in _lib.STRUCTS
    assert [f[0] for f in _lib.VerifyArgs._fields_] == FIELDS
    assert _lib.SIGNATURES["tgp_verify_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    assert _lib.VERIFY_COLS == len(vr.COUNTS) == 8 and _lib.VERIFY_MAX_JOBS == vr.MAX_JOBS == 65535 and _lib.VERIFY_MAX_TAU == vr.MAX_TAU == 1000
    assert ops.VERIFY_COUNTS == vr.COUNTS


def test_the_c_entry_refuses_bad_arguments_before_any_launch():
    """nothing is launched for a refused call, so this runs without a GPU; the pointers are never followed"""
    from tgpose_amd import _lib
    lib = _lib.lib()
    assert lib.tgp_verify_workspace_bytes(6, 100, 200) >= 6 * (100 * 16 + 200 * 8 + 16)
    assert lib.tgp_verify_workspace_bytes(0, 100, 200) >= 0
    for J, nv, nf in ((-1, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.tgp_verify_workspace_bytes(J, nv, nf) == _lib.EINVAL, (J, nv, nf)
    assert lib.tgp_verify_workspace_bytes(65536, 4, 4) == _lib.EUNSUPPORTED
    assert lib.tgp_verify_workspace_bytes(1, 4, lib.tgp_render_max_faces()) == _lib.EUNSUPPORTED
    fake = ctypes.c_void_p(4096)
    good = dict(depth=fake, camk=fake, verts=fake, faces=fake, vptr=fake, fptr=fake, M=1, n_verts=4, n_faces=2, max_verts=4, max_faces=2,
                job_img=fake, job_mesh=fake, job_pose=fake, mask=fake, job_mask_val=fake, S=1, H=8, W=8, J=1, tau=5, near=0.01, counts=fake,
                score=fake, workspace=fake, workspace_bytes=1 << 40)
    invalid = [dict(J=-1), dict(tau=-1), dict(near=0.0), dict(near=-1.0), dict(near=float("inf")), dict(near=float("nan")),
               dict(job_mask_val=None), dict(depth=None), dict(camk=None), dict(verts=None), dict(faces=None), dict(vptr=None),
               dict(fptr=None), dict(job_img=None), dict(job_mesh=None), dict(job_pose=None), dict(counts=None), dict(score=None),
               dict(workspace=None), dict(S=0), dict(H=0), dict(W=0), dict(M=0), dict(max_verts=0), dict(max_faces=0), dict(workspace_bytes=64)]
    for change in invalid:
        a = _lib.VerifyArgs(**dict(good, **change))
        assert lib.tgp_pose_verify(ctypes.byref(a), None) == _lib.EINVAL, change
    unsupported = [dict(J=65536), dict(tau=1001), dict(H=4096, W=4096), dict(H=1024, W=16385), dict(max_faces=lib.tgp_render_max_faces())]
    for change in unsupported:
        a = _lib.VerifyArgs(**dict(good, **change))
        assert lib.tgp_pose_verify(ctypes.byref(a), None) == _lib.EUNSUPPORTED, change
    assert lib.tgp_pose_verify(None, None) == _lib.EINVAL
    # no job: nothing to launch, nothing to refuse -- neither the job arrays nor a workspace are needed
    a = _lib.VerifyArgs(**dict(good, J=0, job_img=None, job_mesh=None, job_pose=None, counts=None, score=None, workspace=None, workspace_bytes=0))
    assert lib.tgp_pose_verify(ctypes.byref(a), None) == 0
    # a mask is optional, and its bytes are not asked for without it
    assert lib.tgp_pose_verify(ctypes.byref(_lib.VerifyArgs(**dict(good, mask=None, job_mask_val=None, J=-1))), None) == _lib.EINVAL


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from tgpose_amd import ops, pose
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    p = inspect.signature(ops.pose_verify).parameters
    assert [(k, v.default) for k, v in p.items()] == [
        ("meshset", inspect.Parameter.empty), ("depth", inspect.Parameter.empty), ("camk", inspect.Parameter.empty),
        ("job_img", inspect.Parameter.empty), ("job_mesh", inspect.Parameter.empty), ("job_pose", inspect.Parameter.empty), ("tau", 5),
        ("near", 0.01), ("mask", None), ("job_mask_val", None)]
    with pytest.raises(TypeError, match="MeshSet"):
        ops.pose_verify(None, None, None, None, None, None)
    ms = ops.MeshSet(pc.meshes(), device="cpu")
    depth = torch.zeros(1, 8, 8, dtype=torch.int16)
    with pytest.raises(TypeError, match="GPU tensor"):
        ops.pose_verify(ms, depth, torch.ones(1, 4), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, 4))
    for kw, word in ((dict(tau=-1), "tau"), (dict(tau=1001), "tau"), (dict(tau=2.5), "tau"), (dict(min_score=float("nan")), "min_score"),
                     (dict(near=0.0), "near")):
        with pytest.raises(ValueError, match=word):
            pose.Verify(ms, [0, 0], **kw)
    with pytest.raises(TypeError, match="MeshSet"):
        pose.Verify(pc.meshes(), [0])
    with pytest.raises(ValueError, match="outside the set"):
        pose.Verify(ms, [0, 2])
    v = pose.Verify(ms, [0, 0, 0])
    assert (v.tau, v.min_score, v.near, v.normalised) == (5, 0.5, 0.01, False) and v.job_mesh.dtype == torch.int32
    p = inspect.signature(pose.verify_poses).parameters
    assert list(p)[:5] == ["meshset", "job_mesh", "depth", "camk", "RTs"] and p["tau"].default == 5 and p["scales"].default is None
    assert inspect.signature(myEvaluater.track).parameters["verify"].default is None
    assert inspect.signature(myEvaluater.acquire_verified).parameters["verify"].default is inspect.Parameter.empty
    # the job pose of the 4x4 form, on whatever device the poses are: [s R | t] as it stands, or its columns times the scales
    RTs = torch.arange(32, dtype=torch.float32).reshape(2, 4, 4)
    assert torch.equal(pose.verify_job_pose(RTs), RTs[:, :3, :4]) and pose.verify_job_pose(RTs).is_contiguous()
    sc = torch.tensor([[1.0, 2.0, 3.0], [0.5, 0.25, 2.0]])
    want = RTs[:, :3, :4].clone()
    want[:, :, :3] *= sc[:, None, :]
    assert torch.equal(pose.verify_job_pose(RTs, sc), want)


@pytest.mark.parametrize("split", sorted(rc.RECT_SPLITS))
def test_the_restatement_on_a_rectangle_against_its_own_depth(split):
    """closed forms, no measured number: the rectangle covers the samples x = 10 .. 40, y = 5 .. 19 (render_cases.rectangle: 465
    pixels at 1000 mm); against its own depth every pixel matches at distance 0, at +tau still with abs_sum = tau * rendered, at
    +tau+1 every pixel is a violation, at -tau-1 every pixel is occluded and nothing is left to score, on a zeroed frame nothing
    is known"""
    c, ref = vc.reference("rectangle", split)
    n, tau = 31 * 15, vc.TAU
    want = {"own": dict(match=n, abs_sum=0), "plus_tau": dict(match=n, abs_sum=tau * n), "plus_tau_1": dict(violation=n),
            "minus_tau_1": dict(occluded=n), "zeroed": dict(nodata=n)}
    score = {"own": 1.0, "plus_tau": 1.0, "plus_tau_1": 0.0, "minus_tau_1": 0.0, "zeroed": 0.0}
    assert (c["depth"][0] > 0).sum() == n and set(np.unique(c["depth"][0])) == {0, 1000}
    for j, name in enumerate(vc.RECT_FRAMES):
        row = dict(rendered=n, match=0, violation=0, occluded=0, nodata=0, in_mask=15 * 15, abs_sum=0, dropped=0)
        row.update(want[name])
        assert dict(zip(vr.COUNTS, ref["counts"][j].tolist())) == row, name
        assert ref["score"][j] == np.float32(score[name]) and ref["score"].dtype == np.float32, name
    bare = vr.verify(**vc.without_mask(c))
    assert (bare["counts"][:, C["in_mask"]] == 0).all()
    keep = [i for i in range(8) if i != C["in_mask"]]
    assert np.array_equal(bare["counts"][:, keep], ref["counts"][:, keep]) and np.array_equal(bare["score"], ref["score"])


def test_the_invariant_and_the_score_on_every_case():
    for name in ("rectangle", "rules", "seven_jobs"):
        c, ref = vc.reference(name)
        n = ref["counts"].astype(np.int64)
        assert np.array_equal(n[:, C["rendered"]], n[:, [C["match"], C["violation"], C["occluded"], C["nodata"]]].sum(1)), name
        assert (n[:, C["abs_sum"]] <= c["tau"] * n[:, C["match"]]).all() and (n[:, C["in_mask"]] <= n[:, C["rendered"]]).all(), name
        den = n[:, C["rendered"]] - n[:, C["occluded"]]
        want = np.where(den > 0, n[:, C["match"]].astype(np.float32) / np.maximum(den, 1).astype(np.float32), np.float32(0))
        assert np.array_equal(ref["score"], want.astype(np.float32)), name
    _, ref = vc.reference("rules")
    rows = [dict(zip(vr.COUNTS, r)) for r in ref["counts"].tolist()]
    assert not any(rows[0].values())                                                   # wholly off-screen
    assert rows[1]["rendered"] == 0 and rows[1]["dropped"] == 1 and rows[2]["rendered"] == 0 and rows[2]["dropped"] == 1
    assert rows[3]["violation"] == rows[3]["rendered"] > 100                           # 0.5 m in front of a frame at 1 m
    assert rows[4]["nodata"] == rows[4]["rendered"] > 100 and ref["score"][4] == 0     # 70 m: over the range of uint16 millimetres
    c, ref = vc.reference("seven_jobs")
    rows = [dict(zip(vr.COUNTS, r)) for r in ref["counts"].tolist()]
    assert c["job_img"].tolist() == [2, 2, 2, 2, 1, 0, 3] and not any(rows[6].values())   # job_img out of range
    assert rows[5]["nodata"] == rows[5]["rendered"] > 0                                 # against the empty frame
    assert rows[4]["match"] == rows[4]["rendered"] == rows[4]["in_mask"] > 0 and ref["score"][4] == 1   # alone in its frame, as rendered
    assert all(r["in_mask"] == r["match"] for r in rows[:3]) and all(r["violation"] == 0 for r in rows[:3])
    assert rows[3]["violation"] > 0 and ref["score"][3] < ref["score"][:3].min()


def test_the_ground_truth_pose_scores_above_a_displaced_one():
    """plane_cases' frames: every object at its ground-truth pose against the pose moved 15 mm towards the camera and 15 mm sideways"""
    for k in (0, pc.FRAMES - 1):
        depth = pc.rendered(k)[None]
        moves = ((0.0, 0.0, 0.0), (0.0, 0.0, -0.015), (0.015, 0.0, 0.0))
        jobs = [(0, 0, vc.gt_pose34(k, o, mv), 0) for o in range(3) for mv in moves]
        score = vr.verify(**vc.case(pc.meshes(), depth, pc.CAMK, jobs))["score"].reshape(3, 3)
        print("frame %d: scores (ground truth, 15 mm nearer, 15 mm sideways) per object: %s" % (k, score.tolist()))
        assert (score[:, 0] > score[:, 1]).all() and (score[:, 0] > score[:, 2]).all(), (k, score)


def test_a_vanished_object_scores_below_every_present_one():
    """six frames, object 2 absent from frame 3 on, every object verified at its ground-truth pose in every frame: the least score
    over the present pairs is above the greatest over the absent ones; their midpoint is tests/test_track_verify_gpu.py's min_score"""
    lo, hi, mid = vc.separation()
    s = vc.vanished_scores()
    assert s.shape == (pc.FRAMES, 3) and sum(not vc.present(k, o) for k in range(pc.FRAMES) for o in range(3)) == pc.FRAMES - vc.GONE_FROM
    for k in range(vc.GONE_FROM):
        assert np.array_equal(vc.vanished_rendered(k)[0], pc.rendered(k))               # the same frames while it is there
    assert lo > hi, "present pairs score at least %.4f, absent pairs at most %.4f (midpoint %.4f)" % (lo, hi, mid)
    print("present pairs score at least %.4f, absent pairs at most %.4f: min_score = %.4f" % (lo, hi, mid))
