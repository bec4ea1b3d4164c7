"""ICP without a GPU: the NumPy restatement (tests/icp_ref.py) recovers a known similarity on noise-free data in both modes; the
header declares the entry points and the built library exports them; ops.icp_refine refuses CPU tensors and bad arguments.

Bounds of the recovery test.  The source points are float32 images of model samples at about 0.8 m, so each coordinate carries a
rounding error of at most 2^-25 * 0.8 m = 2.4e-5 mm; a least-squares pose over 256 of them cannot be off by more than that in
translation, nor by more than that over the model's half extent (0.16 * 0.5 = 80 mm) in rotation: 3e-7 rad = 1.7e-5 degrees.  The
test asks for 1e-4 mm and 1e-4 degrees, the floor of the GPU test of the same set-up."""
import ctypes

import numpy as np
import pytest
import torch

from tests import icp_ref, mesh_sample_ref


def noise_free(n_model=512, n_src=256, seed=0):
    v, f = icp_ref.two_boxes()
    rng = np.random.default_rng(seed)
    model = mesh_sample_ref.sample(v, f, rng.random((n_model, 3)))[0].astype(np.float32)
    Rg, tg, sg = icp_ref.rot([0.3, -0.5, 0.8], 140.0), np.array([0.05, -0.03, 0.8]), 0.16
    pick = rng.permutation(n_model)[:n_src]
    src = (sg * model[pick, :3].astype(np.float64) @ Rg.T + tg).astype(np.float32)
    return model, src, pick, Rg, tg, sg


@pytest.mark.parametrize("mode,with_scale", [(1, False), (0, False), (0, True)])
def test_reference_recovers_a_known_similarity(mode, with_scale):
    model, src, pick, Rg, tg, sg = noise_free()
    R0 = Rg @ icp_ref.rot([1.0, 2.0, -1.0], 5.0)
    t0 = tg + 0.010 * np.array([2.0, -1.0, 2.0]) / 3.0
    s0 = sg * (1.02 if with_scale else 1.0)
    e0 = icp_ref.pose_error(R0, t0, Rg, tg)
    out = icp_ref.refine(model, src, R0, t0, s0, 0.05, mode=mode, with_scale=with_scale, iters=60)
    er, et = icp_ref.pose_error(out["R64"], out["t64"], Rg, tg)
    print("mode %d scale %d: start %.3f deg %.3f mm -> %.2e deg %.2e mm, s %.9f, %d iterations, rmse %.3e" %
          (mode, with_scale, e0[0], e0[1], er, et, out["s64"], out["iters"], out["rmse"]))
    assert abs(e0[0] - 5.0) < 1e-6 and abs(e0[1] - 10.0) < 1e-6
    assert out["status"] == 0 and out["iters"] < 60 and out["inliers"] == len(src)
    assert np.array_equal(out["corr"], pick.astype(np.int32))       # every source point found the sample it is the image of
    assert er <= 1e-4 and et <= 1e-4
    assert abs(out["s64"] / sg - 1.0) <= 1e-6
    # mode 1 multiplies the float32 start rotation by exact rotations: it stays as orthonormal as float32 made it
    assert abs(np.linalg.det(out["R64"]) - 1.0) <= 1e-6 and np.abs(out["R64"].T @ out["R64"] - np.eye(3)).max() <= 1e-6


def test_reference_statuses_and_fixed_iterations():
    model, src, pick, Rg, tg, sg = noise_free()
    off = tg + np.array([0.0, 0.01, 0.0])
    out = icp_ref.refine(model, src, Rg, off, sg, 1e-6, mode=1)                 # an empty gate: every point is 10 mm from its sample
    assert out["status"] == 1 and out["iters"] == 0 and out["inliers"] < 6 and np.array_equal(out["R"], Rg.astype(np.float32))
    assert np.array_equal(out["t"], off.astype(np.float32))
    out = icp_ref.refine(model, src, Rg, tg, sg, 0.05, mode=0, iters=3, tol_rot=0.0, tol_trans=0.0)
    assert out["status"] == 0 and out["iters"] == 3
    bad = src.copy()
    bad[:10] = np.nan
    out = icp_ref.refine(model, bad, Rg, tg, sg, 0.05, mode=1, iters=2, tol_rot=0.0, tol_trans=0.0)
    assert out["inliers"] == len(src) - 10 and (out["corr"][:10] == -1).all()
    flat = np.tile(np.array([[0.1, 0.2, 0.3, 0.0, 0.0, 1.0]], np.float32), (8, 1))
    out = icp_ref.refine(flat, src, Rg, tg, sg, 10.0, mode=1, iters=2)          # one repeated point and normal
    assert out["status"] in (0, 2) and np.isfinite(out["R"]).all() and np.isfinite(out["t"]).all()


def test_header_and_library_declare_icp():
    from tgpose_amd import _lib
    assert _lib.CONSTANTS["ICP_MAX_POINTS"] == icp_ref.MAX_POINTS == 2048
    assert "tgp_icp_refine" in _lib.SIGNATURES and "tgp_icp_max_points" in _lib.SIGNATURES
    assert _lib.SIGNATURES["tgp_icp_refine"][1][0]._type_ is _lib.STRUCTS["tgp_icp_args"] is _lib.IcpArgs
    names = [n for n, _ in _lib.IcpArgs._fields_]
    for field in ("models", "model_count", "src", "src_count", "job_model", "R", "t", "s", "max_dist", "mode", "with_scale", "iters",
                  "tol_rot", "tol_trans", "min_inliers", "R_out", "t_out", "s_out", "info", "rmse", "corr"):
        assert field in names
    handle = ctypes.CDLL(_lib.LIB_PATH)                                          # the built library exports them (host calls only)
    assert hasattr(handle, "tgp_icp_refine")
    assert _lib.lib().tgp_icp_max_points() == 2048
    assert _lib.ABI_VERSION == 9
    # argument errors are answered before anything touches a device
    a = _lib.IcpArgs()
    assert _lib.lib().tgp_icp_refine(ctypes.byref(a), None) == _lib.EINVAL
    assert _lib.lib().tgp_icp_refine(None, None) == _lib.EINVAL
    one = ctypes.c_void_p(16)                                                    # never dereferenced: the sizes are refused first
    full = dict(models=one, job_model=one, src=one, R=one, t=one, s=one, max_dist=one, R_out=one, t_out=one, s_out=one, info=one,
                rmse=one, M=1, m_cap=8, J=1, n_cap=8, iters=1)
    for change, want in ((dict(iters=0), _lib.EINVAL), (dict(J=0), _lib.EINVAL), (dict(mode=1, with_scale=1), _lib.EINVAL),
                         (dict(mode=2), _lib.EINVAL), (dict(rmse=None), _lib.EINVAL), (dict(m_cap=2049), _lib.EUNSUPPORTED),
                         (dict(n_cap=2049), _lib.EUNSUPPORTED), (dict(J=65536), _lib.EUNSUPPORTED)):
        a = _lib.IcpArgs(**dict(full, **change))
        assert _lib.lib().tgp_icp_refine(ctypes.byref(a), None) == want, change


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from tgpose_amd import ops, pose
    J, n = 2, 16
    src, R, t, s = torch.zeros(J, n, 3), torch.eye(3).repeat(J, 1, 1), torch.zeros(J, 3), torch.ones(J)
    jm = torch.zeros(J, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.IcpModels(torch.zeros(1, 8, 6))                                      # a CPU tensor
    with pytest.raises(TypeError):
        ops.icp_refine(None, jm, src, R, t, s, 0.01)                             # CPU tensors
    with pytest.raises(TypeError):
        pose.refine_poses(None, jm, src, torch.eye(4).repeat(J, 1, 1), 0.01)
    with pytest.raises(ValueError):
        ops.icp_refine(None, jm, src, R, t, s, 0.01, mode="surface")
    with pytest.raises(ValueError):
        ops.icp_refine(None, jm, src, R, t, s, 0.01, mode="plane", with_scale=True)
    with pytest.raises(ValueError):
        ops.icp_refine(None, jm, src, R, t, s, 0.01, iters=0)
    with pytest.raises(ValueError):
        ops.icp_refine(None, jm, src, R, t, s, 0.01, tol_rot=-1.0)
    with pytest.raises(TypeError):
        pose.IcpRefine(None, [0, 0], 0.01)
    assert ops.ICP_MAX_POINTS == 2048 and set(ops.ICP_STATUS) == {1, 2, 3}
