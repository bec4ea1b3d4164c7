"""CPU tests of the persistence-image contract ("Ground-truth persistence images"): the float64 restatement
tests/pd_ref.py checks its own bookkeeping, persim's legacy PersImage semantics against hand values, and tgp_persistence's
refusals without a launch.  gudhi and persim are not installed: their rules are restated from their documented behaviour, unpinned."""
import ctypes
import itertools

import numpy as np
import pytest
from scipy.stats import norm

from tests import pd_ref



def _euler(tets):
    faces = set()
    for t in map(tuple, np.sort(tets, axis=1)):
        for k in range(1, 5):
            faces.update(itertools.combinations(t, k))
    return sum((-1) ** (len(f) - 1) for f in faces), faces


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_bookkeeping(seed):
    """Euler characteristic 1, empty circumspheres, and pair counts equal to the Betti bookkeeping of the whole complex"""
    P = np.random.RandomState(seed).normal(size=(120, 3)).astype(np.float32)
    U, _ = pd_ref.unique_points(P)
    T = pd_ref.delaunay_tets(U)
    chi, faces = _euler(T)
    assert chi == 1
    for t in T:
        c, r2 = pd_ref._sphere(U, t)
        d = ((U - c) ** 2).sum(1)
        assert (d >= r2 * (1 - 1e-9)).all()
    val = pd_ref.alpha_filtration(U, T)
    assert len(val) == len(faces)
    for s, v in val.items():                          # faces no later than cofaces
        for k in range(len(s)):
            if len(s) > 1:
                assert val[s[:k] + s[k + 1:]] <= v
    # pairs of every persistence: #edges = (V - 1) + (H1 births); #triangles = H1 deaths + H2 births; #tets = H2 deaths
    order = sorted(val, key=lambda s: (val[s], len(s), s))
    n = {d: sum(1 for s in val if len(s) == d + 1) for d in range(4)}
    index = {s: i for i, s in enumerate(order)}
    pivot, npairs = {}, {0: 0, 1: 0, 2: 0}
    for s in order:
        if len(s) == 1:
            continue
        col = {index[s[:k] + s[k + 1:]] for k in range(len(s))}
        while col and max(col) in pivot:
            col ^= pivot[max(col)]
        if col:
            pivot[max(col)] = col
            npairs[len(s) - 2] += 1
    assert npairs[0] == n[0] - 1
    assert npairs[1] + npairs[2] == n[2] and npairs[2] == n[3]
    assert n[1] - npairs[0] == npairs[1]
    h1, h2 = pd_ref.diagrams(P)
    assert (h1[:, 1] > h1[:, 0]).all() and (h2[:, 1] > h2[:, 0]).all()


def test_single_pair_image_is_closed_form():
    b, d = 0.02, 0.05
    im = pd_ref.PersImage().transform(np.array([[b, d]]))
    maxBD = max(b, d - b)
    dx = maxBD / 50
    lo = np.linspace(0, maxBD, 50)
    xs = norm.cdf(lo + dx, b, 0.01) - norm.cdf(lo, b, 0.01)
    ys = norm.cdf(lo + dx, d - b, 0.01) - norm.cdf(lo, d - b, 0.01)
    want = np.outer(xs, ys).T[::-1]                 # weight (1 / max p) * p = 1
    assert np.allclose(im, want, rtol=0, atol=1e-15)
    assert im.shape == (50, 50)


def test_h2_takes_h1_range_and_empty_dimension_is_zero():
    h1 = np.array([[0.0, 0.04], [0.01, 0.02]])
    h2 = np.array([[0.03, 0.09]])
    i1, i2 = pd_ref.images(h1, h2)
    pim = pd_ref.PersImage()
    pim.transform(h1)
    assert pim.specs["maxBD"] == 0.04
    own = pd_ref.PersImage().transform(h2)
    shared = pim.transform(h2)
    assert not np.allclose(own, shared)
    s = shared.astype(np.float32)
    assert np.array_equal(i2, (s / (s.max() + np.float32(1e-20))).reshape(-1))
    z1, z2 = pd_ref.images(np.zeros((0, 2)), h2)
    assert not z1.any() and z2.max() == np.float32(1.0)          # H2 alone: its own range
    assert i1.max() == np.float32(1.0) and i1.dtype == np.float32 and i1.shape == (2500,)


def test_pd_abi_refuses_bad_arguments_without_launching():
    from tgpose_amd import _lib
    lib = _lib.lib()
    assert lib.tgp_version() == 9 and lib.tgp_pd_max_points() == 1024 and lib.tgp_pd_workspace_bytes() > 0
    fake = 1 << 20

    def args(**kw):
        a = _lib.PdArgs()
        a.B, a.N = 2, 1024
        for k in ("pcl", "workspace", "h1", "h2", "counts", "status"):
            setattr(a, k, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.tgp_persistence(None, None) == -1
    for kw in (dict(B=0), dict(N=0), dict(N=1025), dict(pcl=None), dict(workspace=None), dict(workspace=fake + 4), dict(status=None),
               dict(tets=fake), dict(pdh1=fake), dict(tet_cap=-1)):
        assert lib.tgp_persistence(ctypes.byref(args(**kw)), None) == -1, kw


def test_ops_refuse_cpu_tensors():
    import torch
    from tgpose_amd import ops
    with pytest.raises(ValueError):
        ops.persistence_images(torch.zeros(1, 8, 3))
    with pytest.raises(ValueError):
        ops.alpha_persistence(torch.zeros(8, 3))
