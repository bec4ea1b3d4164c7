"""EMD / F-score without a GPU: the numpy restatement of the EMD contract (tests/emd_ref.py) against exact matching, the
tie rule, fscore and the eval_recon aggregation against the reference's recorded numbers (tests/golden/emd.npz), the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

from tests import emd_ref
from tests.util import golden, synth_eval_results

SYNSET = ['BG', 'bottle', 'bowl', 'camera', 'can', 'laptop', 'mug']


def _optimum(a, b):
    from scipy.optimize import linear_sum_assignment
    C = np.sqrt(((a[:, None].astype(np.float64) - b[None].astype(np.float64)) ** 2).sum(-1))
    r, c = linear_sum_assignment(C)
    return C[r, c].sum()


def test_restatement_within_auction_bound_of_exact_matching():
    """Where the auction has converged (nothing unassigned before the last iteration) the assignment is a permutation and its
    cost is within n*eps (epsilon-complementary slackness) + n*1e-4 (fp32 price rounding and the 1e-6 winner window: far above
    both, far below n*eps) of the optimum of scipy's exact solver on float64 distances."""
    rng = np.random.default_rng(7)
    for n, eps, iters in [(64, 0.01, 400), (96, 0.01, 600), (257, 0.005, 3000)]:
        a, b = rng.random((n, 3), dtype=np.float32), rng.random((n, 3), dtype=np.float32)
        dist, asg, info = emd_ref.emd_pair(a, b, eps, iters)
        assert info["converged_at"] is not None and info["converged_at"] < iters - 1, (n, info)      # precondition, not a skip
        assert np.array_equal(np.sort(asg), np.arange(n))
        d64 = a.astype(np.float64) - b[asg].astype(np.float64)
        assert np.allclose(dist, (d64 ** 2).sum(-1), rtol=1e-6, atol=1e-12)
        cost, opt = np.sqrt(dist.astype(np.float64)).sum(), _optimum(a, b)
        print("n=%d converged at %d: cost - optimum = %.4f, bound %.4f" % (n, info["converged_at"], cost - opt, n * eps + n * 1e-4))
        assert opt - n * 1e-4 <= cost <= opt + n * eps + n * 1e-4


def test_lowest_and_highest_winner_rules_reach_the_same_cost_on_the_lattice():
    """Coincident distances (two copies of a 4^3 grid against shifted copies): equal increments compete for every object, the
    reference's write race may let any of them win; the lowest and the highest bidder both lead to a complete matching of the
    same total cost, the optimum."""
    a, b = emd_ref.lattice()
    out = {}
    for rule in ("lowest", "highest"):
        dist, asg, info = emd_ref.emd_pair(a, b, 0.01, 200, winner=rule)
        assert info["converged_at"] is not None
        assert np.array_equal(np.sort(asg), np.arange(len(a)))
        out[rule] = (np.sqrt(dist.astype(np.float64)).sum(), asg)
    assert out["lowest"][0] == out["highest"][0]
    assert not np.array_equal(out["lowest"][1], out["highest"][1])           # the rule did decide something
    assert abs(out["lowest"][0] - _optimum(a, b)) < 1e-9 * len(a)


def test_restatement_edge_cases():
    """n = 1 (no second best: the increment is best + 1e9 + eps), a cloud against itself (zero distances), one iteration (everyone
    takes its bid: not a bijection)."""
    a, b = np.float32([[0.2, 0.3, 0.4]]), np.float32([[0.6, 0.3, 0.1]])
    dist, asg, _ = emd_ref.emd_pair(a, b, 0.005, 50)
    d = (a - b)[0]
    assert asg.tolist() == [0] and dist[0] == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] and dist.dtype == np.float32
    rng = np.random.default_rng(1)
    c = rng.random((100, 3), dtype=np.float32)
    dist, asg, info = emd_ref.emd_pair(c, c, 0.005, 50)
    assert info["converged_at"] == 1 and np.array_equal(asg, np.arange(100)) and not dist.any()
    d = rng.random((100, 3), dtype=np.float32)
    dist, asg, info = emd_ref.emd_pair(c, d, 0.005, 1)
    nearest = ((c[:, None] - d[None]) ** 2).sum(-1).argmin(1)
    assert np.array_equal(asg, nearest) and len(set(asg.tolist())) < 100


def test_fscore_equals_reference():
    from tgpose_amd.losses.metrics import fscore as via_package
    from tgpose_amd.losses.metrics.CD.fscore import fscore
    assert via_package is fscore
    g = golden("emd.npz")
    d1, d2 = torch.from_numpy(g["fs_dist1"]), torch.from_numpy(g["fs_dist2"])
    got = torch.stack(fscore(d1, d2)).numpy()
    assert np.array_equal(got, g["fs_out0"])
    assert got[0, 2] == 0 and got[0, 3] == 0 and not np.isnan(got).any()     # 0 / 0 and one empty direction
    got = torch.stack(fscore(d1, d2, float(g["fs_thresholds"][1]))).numpy()
    assert np.array_equal(got, g["fs_out1"])
    assert not d1.isnan().any() and np.array_equal(d1.numpy(), g["fs_dist1"])    # inputs untouched


def recon_results():
    """the result list tests/golden/make_emd_golden.py gave the reference"""
    g = golden("emd.npz")
    res = synth_eval_results(int(g["recon_seed"]), int(g["recon_images"]))
    pos = 0
    for r in res:
        P = len(r["pred_class_ids"])
        r["chamfer_dis_cass"], r["emd_dis_cass"] = g["recon_cmf"][pos:pos + P], g["recon_emd"][pos:pos + P]
        pos += P
    assert pos == len(g["recon_cmf"])
    return res, g


def check_recon_stats(stats, g):
    for key in ("emd", "cmf"):
        want = g["recon_%s_class" % key]
        names = [c for c, w in zip(SYNSET, want) if not np.isnan(w)]
        assert sorted(stats[key]) == sorted(names + ["mean"])
        for c in names:
            assert stats[key][c] == want[SYNSET.index(c)]
        assert stats[key]["mean"] == float(g["recon_%s_mean" % key])


def test_recon_statistics_equal_reference():
    from tgpose_amd.evaluation.metrics import recon_statistics
    res, g = recon_results()
    check_recon_stats(recon_statistics(res, SYNSET), g)
    # an image without detections is passed over; a class without detections has no entry
    only = [r for r in res if len(r["pred_class_ids"])][:1] + [r for r in res if not len(r["pred_class_ids"])][:1]
    stats = recon_statistics(only, SYNSET)
    assert set(stats["emd"]) == {SYNSET[c] for c in only[0]["pred_class_ids"]} | {"mean"}


def test_emd_abi():
    """the caps, and argument errors launch nothing (no GPU is touched); tests/test_abi_cpu.py holds the symbols against the header"""
    from tgpose_amd import _lib
    lib = _lib.lib()
    assert lib.tgp_version() == 9 and _lib.ABI_VERSION == 9
    cap = lib.tgp_emd_max_points()
    assert cap >= 2048
    assert lib.tgp_emd_workspace_bytes(32, cap) >= 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tgp_emd_fwd(None, p, 1, 4, 0.005, 50, p, p, None, None) == -1
    assert lib.tgp_emd_fwd(p, p, 1, 4, 0.005, 50, None, p, None, None) == -1
    assert lib.tgp_emd_fwd(p, p, 1, 4, 0.005, 0, p, p, None, None) == -1          # iters < 1
    assert lib.tgp_emd_fwd(p, p, 1, 0, 0.005, 50, p, p, None, None) == -1         # n < 1
    assert lib.tgp_emd_fwd(p, p, 0, 4, 0.005, 50, p, p, None, None) == -1
    assert lib.tgp_emd_fwd(p, p, 1, cap + 1, 0.005, 50, p, p, None, None) == -2   # above the cap
    assert lib.tgp_emd_bwd(p, p, p, None, 1, 4, p, None) == -1
    assert lib.tgp_emd_bwd(p, p, p, p, 1, 0, p, None) == -1


def test_python_surface_mirrors_reference_names():
    from tgpose_amd.losses.metrics import cd, emd
    from tgpose_amd.losses.metrics.EMD.emd_module import emdFunction, emdModule
    from tgpose_amd.losses.utils_v2 import model_utils
    from tgpose_amd.losses.chamfer3D.dist_chamfer_3D import chamfer_3DDist
    import inspect
    assert emd is emdModule and cd is chamfer_3DDist and issubclass(emdFunction, torch.autograd.Function)
    sig = inspect.signature(model_utils.calc_emd)
    assert list(sig.parameters) == ["output", "gt", "eps", "iterations"]
    assert sig.parameters["eps"].default == 0.005 and sig.parameters["iterations"].default == 50
    assert list(inspect.signature(model_utils.calc_cd).parameters)[:4] == ["output", "gt", "calc_f1", "return_raw"]
    from tgpose_amd.evaluation.metrics import compute_degree_cm_mAP
    assert inspect.signature(compute_degree_cm_mAP).parameters["recon_out"].default is None
    with pytest.raises(NotImplementedError):
        compute_degree_cm_mAP([], SYNSET, plot_figure=True)
