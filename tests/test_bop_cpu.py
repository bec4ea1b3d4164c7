"""The BOP pose errors without a GPU: the ABI's new entry points and the argument checks of both C entries and of the wrappers, the
helpers of tgpose_amd/evaluation/bop.py, and the NumPy restatement of the two contracts (tests/bop_ref.py) pinned by closed forms,
not by measured numbers."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from tests import bop_cases as bc
from tests import bop_ref as br
from tests import render_cases as rc

V = br.VCOL


def test_header_declares_and_library_exports_the_entry_points():
    from tgpose_amd import _lib, ops
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tgp_pose_errors", "tgp_pose_errors_workspace_bytes", "tgp_pose_vsd", "tgp_vsd_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        assert getattr(handle, name) is not None
    assert _lib.ABI_VERSION == 9 and "tgp_poseerr_args" in _lib.STRUCTS and "tgp_vsd_args" in _lib.STRUCTS
    assert [f[0] for f in _lib.PoseerrArgs._fields_] == [
        "verts", "vptr", "M", "n_verts", "sym", "sptr", "G", "n_syms", "max_syms", "job_mesh", "job_sym", "pose_est", "pose_gt", "camk", "J",
        "near", "err", "sym_best", "status", "workspace", "workspace_bytes"]
    assert [f[0] for f in _lib.VsdArgs._fields_] == [
        "depth", "camk", "verts", "faces", "vptr", "fptr", "M", "n_verts", "n_faces", "max_verts", "max_faces", "job_img", "job_mesh",
        "pose_est", "pose_gt", "job_tau", "S", "H", "W", "J", "n_tau", "delta", "near", "counts", "within", "err", "workspace", "workspace_bytes"]
    assert _lib.SIGNATURES["tgp_pose_errors_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int])
    assert _lib.SIGNATURES["tgp_vsd_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    assert _lib.POSEERR_MAX_JOBS == br.MAX_JOBS == 65535 and _lib.POSEERR_MAX_SYMS == br.MAX_SYMS == 1024 and _lib.POSEERR_COLS == 4
    assert _lib.VSD_COLS == len(br.VSD_COUNTS) == 8 and _lib.VSD_MAX_TAUS == br.MAX_TAUS == 16
    assert ops.POSE_ERRORS == br.ERRORS and ops.VSD_COUNTS == br.VSD_COUNTS
    assert _lib.POSEERR_TILE < max(bc.SIZES) and 315 > 4 * _lib.POSEERR_SPLIT and 315 % (4 * _lib.POSEERR_SPLIT)   # what the GPU cases rely on
    assert -(-max(bc.SIZES) // _lib.POSEERR_SPLIT) > 256


def test_pose_errors_c_entry_refuses_bad_arguments_before_any_launch():
    """nothing is launched for a refused call, so this runs without a GPU; the pointers are never followed"""
    from tgpose_amd import _lib
    lib = _lib.lib()
    assert lib.tgp_pose_errors_workspace_bytes(7) >= 7 * _lib.POSEERR_SPLIT * 48 and lib.tgp_pose_errors_workspace_bytes(0) >= 0
    assert lib.tgp_pose_errors_workspace_bytes(-1) == _lib.EINVAL and lib.tgp_pose_errors_workspace_bytes(65536) == _lib.EUNSUPPORTED
    fake = ctypes.c_void_p(4096)
    good = dict(verts=fake, vptr=fake, M=1, n_verts=4, sym=fake, sptr=fake, G=1, n_syms=1, max_syms=1, job_mesh=fake, job_sym=fake,
                pose_est=fake, pose_gt=fake, camk=fake, J=1, near=0.01, err=fake, sym_best=fake, status=fake, workspace=fake,
                workspace_bytes=1 << 40)
    invalid = [dict(J=-1), dict(near=0.0), dict(near=-1.0), dict(near=float("inf")), dict(near=float("nan")), dict(M=0), dict(n_verts=0),
               dict(G=0), dict(n_syms=0), dict(max_syms=0), dict(workspace_bytes=64)]
    invalid += [{k: None} for k in ("verts", "vptr", "sym", "sptr", "job_mesh", "job_sym", "pose_est", "pose_gt", "camk", "err", "sym_best",
                                    "status", "workspace")]
    for change in invalid:
        assert lib.tgp_pose_errors(ctypes.byref(_lib.PoseerrArgs(**dict(good, **change))), None) == _lib.EINVAL, change
    for change in (dict(J=65536), dict(max_syms=1025)):
        assert lib.tgp_pose_errors(ctypes.byref(_lib.PoseerrArgs(**dict(good, **change))), None) == _lib.EUNSUPPORTED, change
    assert lib.tgp_pose_errors(None, None) == _lib.EINVAL
    none = dict(good, J=0, job_mesh=None, job_sym=None, pose_est=None, pose_gt=None, camk=None, err=None, sym_best=None, status=None,
                workspace=None, workspace_bytes=0)
    assert lib.tgp_pose_errors(ctypes.byref(_lib.PoseerrArgs(**none)), None) == 0


def test_pose_vsd_c_entry_refuses_bad_arguments_before_any_launch():
    from tgpose_amd import _lib
    lib = _lib.lib()
    assert lib.tgp_vsd_workspace_bytes(6, 100, 200) >= 2 * 6 * (100 * 16 + 200 * 8 + 16) and lib.tgp_vsd_workspace_bytes(0, 100, 200) >= 0
    for J, nv, nf in ((-1, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.tgp_vsd_workspace_bytes(J, nv, nf) == _lib.EINVAL, (J, nv, nf)
    assert lib.tgp_vsd_workspace_bytes(65536, 4, 4) == _lib.EUNSUPPORTED
    assert lib.tgp_vsd_workspace_bytes(1, 4, lib.tgp_render_max_faces()) == _lib.EUNSUPPORTED
    fake = ctypes.c_void_p(4096)
    good = dict(depth=fake, camk=fake, verts=fake, faces=fake, vptr=fake, fptr=fake, M=1, n_verts=4, n_faces=2, max_verts=4, max_faces=2,
                job_img=fake, job_mesh=fake, pose_est=fake, pose_gt=fake, job_tau=fake, S=1, H=8, W=8, J=1, n_tau=10, delta=15, near=0.01,
                counts=fake, within=fake, err=fake, workspace=fake, workspace_bytes=1 << 40)
    invalid = [dict(J=-1), dict(delta=-1), dict(n_tau=0), dict(near=0.0), dict(near=-1.0), dict(near=float("inf")), dict(near=float("nan")),
               dict(S=0), dict(H=0), dict(W=0), dict(M=0), dict(n_verts=0), dict(n_faces=0), dict(max_verts=0), dict(max_faces=0),
               dict(workspace_bytes=64)]
    invalid += [{k: None} for k in ("depth", "camk", "verts", "faces", "vptr", "fptr", "job_img", "job_mesh", "pose_est", "pose_gt", "job_tau",
                                    "counts", "within", "err", "workspace")]
    for change in invalid:
        assert lib.tgp_pose_vsd(ctypes.byref(_lib.VsdArgs(**dict(good, **change))), None) == _lib.EINVAL, change
    unsupported = [dict(J=65536), dict(n_tau=17), dict(delta=65536), dict(H=4096, W=4096), dict(H=1024, W=16385),
                   dict(max_faces=lib.tgp_render_max_faces())]
    for change in unsupported:
        assert lib.tgp_pose_vsd(ctypes.byref(_lib.VsdArgs(**dict(good, **change))), None) == _lib.EUNSUPPORTED, change
    assert lib.tgp_pose_vsd(None, None) == _lib.EINVAL
    none = dict(good, J=0, job_img=None, job_mesh=None, pose_est=None, pose_gt=None, job_tau=None, counts=None, within=None, err=None,
                workspace=None, workspace_bytes=0)
    assert lib.tgp_pose_vsd(ctypes.byref(_lib.VsdArgs(**none)), None) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from tgpose_amd import ops
    from tgpose_amd.evaluation import bop
    E = inspect.Parameter.empty
    assert [(k, v.default) for k, v in inspect.signature(ops.pose_errors).parameters.items()] == [
        ("meshset", E), ("job_mesh", E), ("pose_est", E), ("pose_gt", E), ("symset", E), ("job_sym", E), ("camk", E), ("near", 0.01)]
    assert [(k, v.default) for k, v in inspect.signature(ops.pose_vsd).parameters.items()] == [
        ("meshset", E), ("depth", E), ("camk", E), ("job_img", E), ("job_mesh", E), ("pose_est", E), ("pose_gt", E), ("job_tau", E),
        ("delta", 15), ("near", 0.01)]
    assert list(inspect.signature(bop.errors).parameters)[:8] == ["meshset", "job_mesh", "RTs_est", "RTs_gt", "symset", "job_sym", "camk", "scales"]
    assert list(inspect.signature(bop.score_track).parameters)[:8] == ["results", "gts", "meshset", "job_mesh", "sequence", "camK", "symset", "job_sym"]
    ms = ops.MeshSet(bc.meshes(), device="cpu")
    ss = ops.SymmetrySet(bc.groups(), device="cpu")
    assert len(ss) == 6 and ss.sizes == [1, 2, 4, 315, 8, 6] and ss.sptr.tolist() == [0, 1, 3, 7, 322, 330, 336] and ss.sym.shape == (336, 3, 4)
    assert ss.sym.dtype == torch.float32 and ss.sptr.dtype == torch.int32
    assert np.array_equal(ops.SymmetrySet.identity(), bc.group_z(1))
    for bad in ([], [np.zeros((0, 3, 4))], [np.zeros((2, 4, 4))], [np.zeros((1025, 3, 4))]):
        with pytest.raises(ValueError, match="SymmetrySet"):
            ops.SymmetrySet(bad, device="cpu")
    z, p, k = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, 4), torch.ones(1, 4)
    with pytest.raises(TypeError, match="MeshSet"):
        ops.pose_errors(None, z, p, p, ss, z, k)
    with pytest.raises(TypeError, match="SymmetrySet"):
        ops.pose_errors(ms, z, p, p, None, z, k)
    with pytest.raises(TypeError, match="GPU tensor"):
        ops.pose_errors(ms, z, p, p, ss, z, k)
    with pytest.raises(TypeError, match="MeshSet"):
        ops.pose_vsd(None, None, k, z, z, p, p, torch.ones(1, 10, dtype=torch.int32))
    with pytest.raises(TypeError, match="GPU tensor"):
        ops.pose_vsd(ms, torch.zeros(1, 8, 8, dtype=torch.int16), k, z, z, p, p, torch.ones(1, 10, dtype=torch.int32))


def test_symmetry_transformations_diameter_taus_and_recall():
    from tgpose_amd import ops
    from tgpose_amd.evaluation import bop
    half_turn = [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0.5, 0, 0, 0, 1]
    for info, step in ((dict(), 0.01), (dict(symmetries_discrete=[half_turn]), 0.01),
                       (dict(symmetries_continuous=[dict(axis=[0, 0, 1], offset=[0.1, 0, 0])]), 0.01),
                       (dict(symmetries_discrete=[half_turn, half_turn], symmetries_continuous=[dict(axis=[0, 1, 0], offset=[0, 0, 0])]), 0.07)):
        T = bop.symmetry_transformations(info, step)
        disc, cont = len(info.get("symmetries_discrete", ())), len(info.get("symmetries_continuous", ()))
        assert T.shape == ((math.ceil(math.pi / step) if cont else 1) * (1 + disc), 3, 4) and T.dtype == np.float64
        assert np.abs(T[:, :, :3] @ T[:, :, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-14 and np.allclose(np.linalg.det(T[:, :, :3]), 1)
        assert np.array_equal(T[0], np.concatenate([np.eye(3), np.zeros((3, 1))], 1))               # the identity is kept
    T = bop.symmetry_transformations(dict(symmetries_continuous=[dict(axis=[0, 0, 1], offset=[0.1, 0, 0])]), 0.01)
    assert len(T) == 315 and np.abs(T[:, :, :3] @ np.array([0.1, 0, 0]) + T[:, :, 3] - np.array([0.1, 0, 0])).max() < 1e-15   # the axis stays
    assert np.allclose(T[1, :2, :2], [[math.cos(2 * math.pi / 315), -math.sin(2 * math.pi / 315)], [math.sin(2 * math.pi / 315), math.cos(2 * math.pi / 315)]])
    T = bop.symmetry_transformations(dict(symmetries_discrete=[half_turn]))
    assert np.array_equal(T[1], np.asarray(half_turn, np.float64).reshape(4, 4)[:3])
    from tgpose_amd.datasets import shapes
    ms = ops.MeshSet([shapes.box((0.3, 0.4, 1.2)), shapes.box(1.0), bc.meshes()[bc.TWO]], device="cpu")
    d = bop.diameter(ms, chunk=3)
    assert d.dtype == torch.float64 and np.allclose(d.numpy(), [1.3, math.sqrt(3.0), 0.5], rtol=0, atol=1e-7) and bop.diameter(ms) is d
    tau = bop.vsd_taus(torch.tensor([100.0, 101.0]))
    assert tau.dtype == torch.int32 and tau.shape == (2, 10)
    assert np.array_equal(tau.numpy(), np.ceil(np.arange(0.05, 0.51, 0.05)[None] * np.array([[100.0], [101.0]])).astype(np.int32))
    err = torch.tensor([[0.0, 0.0, 0.001, 4.0], [0.2, 0.1, 0.06, 30.0]], dtype=torch.float64)
    assert float(bop.recall(err[:, 2], [0.02, 0.07])) == 0.75 and float(bop.recall(err[:, 2], torch.tensor([[0.02], [0.05]]))) == 0.5
    ar = bop.average_recall(err, torch.tensor([[0.0] * 10, [1.0] * 10]), torch.tensor([0.1, 0.1]), 640)
    assert float(ar["AR_MSSD"]) == 0.5 and float(ar["AR_MSPD"]) == (10 + 4) / 20 and float(ar["AR_VSD"]) == 0.5
    assert abs(float(ar["AR"]) - (0.5 + 0.7 + 0.5) / 3) < 1e-15
    assert bop.add_s(err, [True, False]).tolist() == [0.0, 0.2]


def test_the_point_restatement_is_pinned_by_closed_forms():
    c, ref, scale = bc.point_reference("mixed")
    assert ref["status"].tolist() == [0, 0, 1, 0, 1, 2, 0]
    assert np.isnan(ref["err"][[2, 4]]).all() and (ref["sym_best"][[2, 4]] == -1).all()
    assert np.isinf(ref["err"][5, 3]) and np.isfinite(ref["err"][5, :3]).all() and ref["sym_best"][5].tolist()[1] == -1     # bit 2
    assert (ref["err"][6] == 0).all() and ref["sym_best"][6].tolist() == [0, 0]                    # est = gt: four zeros
    assert (ref["err"][[0, 1, 3], 1] <= ref["err"][[0, 1, 3], 0]).all() and (ref["err"][[0, 1, 3]] > 0).all()
    # R = I, 2^-6 m along x: add = mssd = 2^-6 exactly, adi <= add, the identity the best symmetry by far more than the tolerance
    c, ref, scale = bc.point_reference("translated")
    tol = bc.tolerances(c, scale)
    assert ref["err"][0, 0] == ref["err"][0, 2] == bc.STEP and ref["err"][0, 1] <= bc.STEP and ref["sym_best"][0].tolist() == [0, 0]
    for col in (0, 1):
        ranked = np.sort(ref["per_sym"][0][:, col])
        assert ranked[1] - ranked[0] > 1e6 * tol[0, 2 + col] > 0
    # a planar model at constant z: mspd = fx 2^-6 / z
    c, ref, scale = bc.point_reference("planar")
    tol = bc.tolerances(c, scale)
    assert abs(ref["err"][0, 3] - float(bc.CAMK[0]) * bc.STEP / 2.0) <= tol[0, 3] and ref["err"][0, 2] == bc.STEP
    assert 0 < tol[0, 3] < 1e-8 and 0 < tol[0, 0] < 1e-11
    # the cube a quarter turn about z: an error with the identity group, none with the 4-fold group, found at the quarter turn
    c, ref, scale = bc.point_reference("cube")
    tol = bc.tolerances(c, scale)
    assert ref["err"][0, 2] > 0.1 and ref["err"][1, 2] <= tol[1, 2] and ref["sym_best"][1].tolist() == [1, 1] and ref["err"][1, 3] <= tol[1, 3]
    assert ref["err"][0, 0] == ref["err"][1, 0] > 0 and ref["err"][0, 1] <= tol[0, 1]               # add is blind to the group, adi sees the cube
    for col in (0, 1):
        ranked = np.sort(ref["per_sym"][1][:, col])
        assert ranked[1] - ranked[0] > 1e6 * tol[1, 2 + col]
    # two points, swapped
    c, ref, scale = bc.point_reference("swapped")
    assert ref["err"][0, 1] == 0 and abs(ref["err"][0, 0] - 0.25) < 1e-7 and ref["err"][0, 2] > 0.2


def test_the_cases_that_reach_every_round_and_every_slot_of_the_symmetry_loop():
    """what tests/test_bop_gpu.py relies on, asserted on the restatement: the best of the 315 symmetries sits in the second round
    (200: workgroup 18; 130: workgroup 0) and in the tail of the third (314), with the runner-up far beyond twice the tolerance;
    bit 2 comes from one transform that workgroup 1 alone sees; equal values sit in two workgroups; a value that is not finite gives
    status 4 and a row of NaN, never an error of 0"""
    from tgpose_amd import _lib
    waves = 4 * _lib.POSEERR_SPLIT
    assert waves == 128 and [(q // waves, (q % waves) // 4) for q in bc.HIGH] == [(1, 18), (2, 14), (1, 0)] and bc.HIGH[1] == 315 - 1
    c, ref, scale = bc.point_reference("high_sym")
    tol = bc.tolerances(c, scale)
    assert ref["status"].tolist() == [0, 0, 0] and ref["sym_best"].tolist() == [[q, q] for q in bc.HIGH]
    for j in range(3):
        assert abs(ref["err"][j, 2] - bc.OFFSET) < 1e-7                      # the float32 rounding of G S_q is all that is left beside the offset
        for col in (0, 1):
            ranked = np.sort(ref["per_sym"][j][:, col])
            assert ranked[1] - ranked[0] > 1e6 * tol[j, 2 + col] > 0, (j, col)
    c, ref, scale = bc.point_reference("pushed")
    group, p = c["groups"][4], c["meshes"][3][0].astype(np.float64)
    assert (bc.PUSH % waves) // 4 == 1 and ref["status"].tolist() == [2] and np.isinf(ref["err"][0, 3]) and ref["sym_best"][0].tolist() == [0, -1]
    assert ref["err"][0, 0] == ref["err"][0, 2] == bc.STEP
    for q, S in enumerate(group):
        z = br.apply(c["pose_gt"][0], br.apply(S, p))[:, 2]
        assert (z.min() <= c["near"]) == (q == bc.PUSH), q
    assert (br.apply(c["pose_est"][0], p)[:, 2] > c["near"]).all()
    c, ref, scale = bc.point_reference("tied")
    per = ref["per_sym"][0]
    assert (per[[1, 3, 5]] == 0).all() and (per[[0, 2, 4]] > 0.1).all() and ref["sym_best"][0].tolist() == [1, 1] and 5 // 4 == 1
    c, ref, scale = bc.point_reference("nonfinite")
    assert ref["status"].tolist() == [4, 4, 4, 0] and np.isnan(ref["err"][:3]).all() and (ref["sym_best"][:3] == -1).all()
    assert np.isfinite(ref["err"][3]).all()
    from tgpose_amd.evaluation import bop
    assert float(bop.recall(torch.from_numpy(ref["err"][:3, 2]), [0.05, 0.5])) == 0.0          # NaN is below no threshold


def _rows(ref):
    return [dict(zip(br.VSD_COUNTS, r)) for r in ref["counts"].tolist()]


@pytest.mark.parametrize("n_tau", sorted(bc.TAUS))
def test_the_vsd_restatement_on_a_rectangle_against_its_own_depth(n_tau):
    """closed forms: the rectangle covers x = 10 .. 40, y = 5 .. 19 (465 pixels at 1000 mm)"""
    c, ref = bc.vsd_reference("rectangle", n_tau)
    n, taus = bc.RECT_N, np.asarray(bc.TAUS[n_tau])
    rows = dict(zip(bc.RECT_JOBS, _rows(ref)))
    err = dict(zip(bc.RECT_JOBS, ref["err"]))
    within = dict(zip(bc.RECT_JOBS, ref["within"]))
    assert ref["err"].dtype == np.float32 and ref["err"].shape == (7, n_tau) and (c["depth"][0] > 0).sum() == n
    full = dict(rendered_gt=n, rendered_est=n, visib_gt=n, visib_est=n, inter=n, union=n, dropped_gt=0, dropped_est=0)
    assert rows["same"] == full and np.array_equal(err["same"], np.where(taus >= 1, 0, 1).astype(np.float32))   # est = gt: 0 for every tau >= 1
    assert rows["plus_7"] == full and np.array_equal(err["plus_7"], np.where(taus <= 7, 1, 0).astype(np.float32))
    # 20 mm behind the frame is beyond delta, but stays visible through visib_gt; at z = 1.02 the far corner projects to 40.5 / 1.02
    # = 39.7 px: one column less, 30 x 15 pixels
    far = dict(full, rendered_est=30 * 15, visib_est=30 * 15, inter=30 * 15)
    assert rows["plus_20"] == far
    assert np.array_equal(err["plus_20"], np.where(taus <= 20, np.float32(1), np.float32(15) / np.float32(n)).astype(np.float32))
    k = bc.RECT_SHIFT
    assert rows["right_3px"] == dict(full, inter=(31 - k) * 15, union=(31 + k) * 15)
    assert np.array_equal(within["right_3px"], np.where(taus >= 1, (31 - k) * 15, 0))
    assert np.array_equal(err["right_3px"], np.where(taus >= 1, np.float32(2 * k * 15) / np.float32((31 + k) * 15), np.float32(1)).astype(np.float32))
    if n_tau == 3:                                                   # thresholds outside [1, 65535] are compared as the ints they are
        assert taus.tolist() == [-5, 0, 70000] and within["same"].tolist() == [0, 0, n] and within["plus_20"].tolist() == [0, 0, 30 * 15]
    assert rows["est_off"] == dict(full, rendered_est=0, visib_est=0, inter=0) and (err["est_off"] == 1).all()
    assert not any(rows["both_off"].values()) and (err["both_off"] == 1).all()
    assert rows["zeroed_plus_20"] == far and np.array_equal(err["zeroed_plus_20"], err["plus_20"])   # a zeroed frame: all visible


def test_the_vsd_invariants_on_every_case():
    for name in ("rectangle", "tails", "rules", "tiny_triangles", "seven_jobs"):
        c, ref = bc.vsd_reference(name)
        n, w = ref["counts"].astype(np.int64), ref["within"].astype(np.int64)
        assert (n[:, V["inter"]] <= n[:, V["visib_gt"]]).all() and (n[:, V["visib_est"]] <= n[:, V["union"]]).all(), name
        assert (w <= n[:, [V["inter"]]]).all() and (n[:, V["visib_gt"]] <= n[:, V["rendered_gt"]]).all(), name
        assert np.array_equal(n[:, V["union"]], n[:, V["visib_gt"]] + n[:, V["visib_est"]] - n[:, V["inter"]]), name
        assert ((ref["err"] >= 0) & (ref["err"] <= 1)).all() and (np.diff(w, axis=1) >= 0).all(), name      # the taus ascend
    c, ref = bc.vsd_reference("tails")
    rows = _rows(ref)
    assert rows[0]["visib_gt"] < rows[0]["rendered_gt"] and rows[0]["rendered_gt"] > 0.9 * 123 * 157   # the table behind the objects
    assert (ref["err"][:3] == 0).all() and ref["err"][3, 0] > 0.9 and ref["err"][3, -1] < 0.2 and rows[4]["visib_est"] > 0
    c, ref = bc.vsd_reference("rules")
    rows = _rows(ref)
    assert rows[0]["rendered_est"] == 0 and rows[0]["rendered_gt"] > 100 and (ref["err"][0] == 1).all()
    assert rows[1]["dropped_gt"] == rows[1]["dropped_est"] == 1 and rows[2]["dropped_gt"] == rows[2]["dropped_est"] == 1
    assert rows[1]["union"] == rows[2]["union"] == 0 and rows[3]["union"] == rows[3]["rendered_gt"] > 100 and (ref["err"][3] == 0).all()
    assert rows[4]["rendered_gt"] == rows[4]["rendered_est"] == 0 and (ref["err"][4] == 1).all()      # 70 m: never rendered
    c, ref = bc.vsd_reference("tiny_triangles")
    assert 100 <= ref["counts"][0, V["inter"]] <= 160 and (ref["err"][0] < 0.05).all() and len(c["meshes"][0][1]) == 20480
    c, ref = bc.vsd_reference("seven_jobs")
    rows = _rows(ref)
    assert c["job_img"].tolist() == [2, 2, 2, 2, 1, 0, 3] and not any(rows[6].values()) and (ref["err"][6] == 1).all()
    assert rows[5]["visib_gt"] == rows[5]["rendered_gt"] > 0 and (ref["err"][[0, 1, 2, 4, 5]] == 0).all() and ref["err"][3, 0] > 0
