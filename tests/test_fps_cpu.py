"""Farthest point sampling without a GPU: the numpy restatement (tests/fps_ref.py) against what the reference's own
farthest_points returned (tests/golden/fps_ref.npz, recorded by tests/golden/make_fps_golden.py), the even-thinning rule, the C ABI."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import fps_ref
from tests.util import golden

NAMES = ("grid", "dups", "rand", "depth0", "depth1")


def test_fixture_lists_the_clouds():
    g = golden("fps_ref.npz")
    assert tuple(g["names"].tolist()) == NAMES
    assert dict(zip(NAMES, g["n"].tolist())) == dict(grid=256, dups=200, rand=64, depth0=1024, depth1=1024)
    assert len(g["grid_xyz"]) == 1600 and len(g["dups_xyz"]) == 400 and len(g["rand_xyz"]) == 300
    assert 3000 < len(g["depth0_xyz"]) < 3600 and 6500 < len(g["depth1_xyz"]) < 7300
    assert g["time_M"].tolist() == [2048, 4096, 8192] and (g["time_seconds"] > 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference(name):
    """with the reference's torch.mean row as the start: centres, clusters and every distance bit; with the restatement's own
    centroid (the kernel's pairwise tree): the centres"""
    g = golden("fps_ref.npz")
    xyz, n = g[name + "_xyz"], int(g["n"][NAMES.index(name)])
    idx, d, cl = fps_ref.fps(xyz, n, start=g[name + "_mean"])
    assert np.array_equal(idx, g[name + "_centers"])
    assert np.array_equal(cl, g[name + "_clusters"])
    assert np.array_equal(d.view(np.int32), g[name + "_dist"].view(np.int32))
    assert np.array_equal(fps_ref.fps(xyz, n)[0], g[name + "_centers"])
    if name == "dups":                          # 50 distinct points, 200 centres: once every point has a centre at distance
        assert len(set(idx[:50].tolist())) == 50 and not idx[50:].any()        # sqrt(3) * 1e-6 all maxima are equal: row 0 from then on


def test_restatement_rules():
    """init_center=False starts at row 0; the tiling rule at and below n; fma32 rounds once (a double-rounding case)"""
    rng = np.random.default_rng(3)
    p = rng.random((50, 3), dtype=np.float32)
    idx, d, cl = fps_ref.fps(p, 7, init_center=False)
    assert idx[0] == 0 and len(set(idx.tolist())) == 7 and cl[idx[-1]] == 6 and (d[idx] == np.sqrt(np.float32(3e-12))).all()
    for n in (50, 51, 120):
        idx, d, cl = fps_ref.fps(p, n)
        assert np.array_equal(idx, np.arange(n) % 50) and (cl == -1).all()
        assert np.array_equal(d, fps_ref.dist(fps_ref.centroid(p), p))
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 exactly, an fp32 midpoint; +-2^-60 decides it, but float64 drops that term before the
    # second rounding: a sum through float64 alone returns the tie's even neighbour both times
    a = np.float32([1.0 + 2.0 ** -12])
    lo, hi = np.float32(1.0 + 2.0 ** -11), np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert fps_ref.fma32(a, a, np.float32([2.0 ** -60]))[0] == hi
    assert fps_ref.fma32(a, a, np.float32([-2.0 ** -60]))[0] == lo
    assert fps_ref.fma32(a, a, np.float32([0.0]))[0] == lo
    assert np.array_equal(fps_ref.centroid(p[:1]), p[0])
    t = p[:5].copy()
    want = (((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + 0) + 0)) / np.float32(5)
    assert np.array_equal(fps_ref.centroid(t), want)


@pytest.mark.parametrize("pool", [512, 4096])
def test_even_thinning_indices(pool):
    for total in (pool - 1, pool, pool + 1, 3 * pool + 7):
        got = fps_ref.thin_indices(total, pool)
        want = [i for i in range(total)] if total <= pool else [(i * total) // pool for i in range(pool)]
        assert got.tolist() == want
        assert len(set(want)) == len(want) and want[-1] < total and want[0] == 0


def test_fps_abi():
    """the cap, and argument errors launch nothing (no GPU is touched); tests/test_abi_cpu.py holds the symbols against the header"""
    from tgpose_amd import _lib, ops
    lib = _lib.lib()
    assert lib.tgp_version() == 9 and _lib.ABI_VERSION == 9
    cap = lib.tgp_fps_max_points()
    assert cap >= 8192 and ops.fps_max_points() == cap
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(xyz=p, ld=3, counts=None, B=1, M=4, n=2, start=None, init_center=1, idx=p, dist=None, clusters=None, stream=None)
    call = lambda **kw: lib.tgp_fps(*{**ok, **kw}.values())
    assert call(xyz=None) == -1 and call(idx=None) == -1
    assert call(B=0) == -1 and call(M=0) == -1 and call(n=0) == -1
    assert call(ld=2) == -1 and call(ld=5) == -1
    assert call(M=cap + 1) == -2                                   # above the cap
    assert call(M=cap + 1, ld=2) == -1


def test_python_surface():
    from tgpose_amd import ops
    from tgpose_amd.core.utils import farthest_points_torch as fpt
    from tgpose_amd.datasets import load_data as ld
    from tgpose_amd.evaluation import load_data_eval as lde
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    import torch
    from torch.nn import functional as F
    sig = inspect.signature(fpt.farthest_points)
    assert list(sig.parameters) == ["data", "n_clusters", "dist_func", "return_center_indexes", "return_distances", "verbose", "init_center"]
    assert sig.parameters["dist_func"].default is F.pairwise_distance and sig.parameters["init_center"].default is True
    assert list(inspect.signature(fpt.get_fps_and_center_torch).parameters) == ["points", "num_fps", "init_center", "dist_func"]
    assert list(inspect.signature(ld.farthest_point_sample).parameters) == ["xyz", "npoint"]
    assert list(inspect.signature(ops.farthest_points).parameters) == ["xyz", "n", "counts", "start", "init_center", "return_distances",
                                                                       "return_clusters"]
    assert inspect.signature(lde.clouds_from_frames).parameters["fps_pool"].default == 4096
    assert inspect.signature(ld.train_batch).parameters["pcl_select"].default == "random"
    assert inspect.signature(ld.TrainBatches.__init__).parameters["pcl_select"].default == "random"
    with pytest.raises(ValueError, match="float32 GPU tensor"):
        fpt.farthest_points(torch.zeros(10, 3), 4)                 # a CPU tensor
    with pytest.raises(ValueError, match="dist_func"):
        fpt.farthest_points(torch.zeros(10, 3), 4, dist_func=lambda a, b: (a - b).abs().sum(-1))
    with pytest.raises(ValueError, match="'numpy', 'device' or 'fps'"):
        myEvaluater(torch.nn.Linear(1, 1), sampler="farthest")
    with pytest.raises(ValueError, match="pcl_select"):
        ld.train_batch([{}], pcl_select="farthest", device="cpu")
