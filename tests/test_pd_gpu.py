"""GPU tests of the ground-truth persistence images (csrc/persistence.hip, tgp_persistence; ops.persistence_images,
ops.alpha_persistence, datasets.compute_pd, load_data.train_batch(persistence=True)) against tests/golden/pd.npz, written by
tests/golden/make_pd_golden.py from the float64 restatement tests/pd_ref.py.  Parity with gudhi / persim themselves is unverified
(neither is installed); the contract is DESIGN.md section 3."""
import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

from tests import pd_ref
from tests.pd_ref import IMG_ATOL, PAIR_RTOL          # 1e-9 relative on a pair, 1e-6 absolute on an image
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# pairs whose persistence is at the rounding level of the squared radii (~1e-3) are not compared: two float64 evaluations of the
# same sphere may differ in the last bit and so create or remove a zero-length pair
PERS_MIN = 1e-12


@pytest.fixture(scope="module")
def fx():
    return golden("pd.npz")


@pytest.fixture(scope="module")
def run(fx):
    """every fixture cloud alone: (alpha_persistence result as numpy, pdh1, pdh2)"""
    from tgpose_amd import ops
    out = {}
    for name in fx["names"]:
        pc = torch.from_numpy(fx["cloud." + name]).to(DEV)[None]
        a = {k: v.cpu().numpy() for k, v in ops.alpha_persistence(pc).items() if not k.startswith("_")}
        h1, h2, st = ops.persistence_images(pc, check_status=False)
        assert int(st[0]) == 0, name
        out[str(name)] = (a, h1[0].cpu().numpy(), h2[0].cpu().numpy())
    return out


def _pairs(a, dim):
    k = int(a["counts"][0, dim])
    p = a["h%d" % (dim + 1)][0, :k]
    p = p[(p[:, 1] - p[:, 0]) > PERS_MIN]
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def _close(got, want):
    want = want[(want[:, 1] - want[:, 0]) > PERS_MIN]
    assert got.shape == want.shape, (got.shape, want.shape)
    if len(want):
        assert (np.abs(got - want) <= PAIR_RTOL * np.abs(want)).all(), np.max(np.abs(got - want) / np.abs(want))


def test_triangulation_is_delaunay(fx, run):
    """no point strictly inside any circumsphere (float64), Euler characteristic 1, volume = the convex hull's; status 0"""
    from tests.test_pd_cpu import _euler
    for name in fx["names"]:
        a = run[str(name)][0]
        assert int(a["status"][0]) == 0, name
        T = a["tets"][0, : int(a["ntet"][0])]
        P = fx["cloud." + name].astype(np.float64)
        U = np.unique(T)
        assert len(U) == len(np.unique(P, axis=0)), name
        assert _euler(T)[0] == 1, name
        A, B, C, D = (P[T[:, k]] for k in range(4))
        vol = np.einsum("ij,ij->i", B - A, np.cross(C - A, D - A))
        assert (vol > 0).all(), name
        assert abs(vol.sum() / 6 - ConvexHull(P[U]).volume) <= 1e-9 * ConvexHull(P[U]).volume, name
        for t in T:
            c, r2 = pd_ref._sphere(P, t)
            assert (((P[U] - c) ** 2).sum(1) >= r2 * (1 - 1e-9)).all(), name


def test_diagrams_match_restatement(fx, run):
    for name in fx["names"]:
        a = run[str(name)][0]
        if "h1." + name in fx:
            want = (fx["h1." + name], fx["h2." + name])
        else:       # the depth patch: the restatement's filtration and reduction on the kernel's own triangulation
            P = fx["cloud." + name].astype(np.float64)
            T = a["tets"][0, : int(a["ntet"][0])]
            dg = pd_ref.persistence(pd_ref.alpha_filtration(P, np.sort(T, axis=1)))
            want = tuple(d[np.lexsort((d[:, 1], d[:, 0]))] for d in (dg[1], dg[2]))
        _close(_pairs(a, 0), want[0])
        _close(_pairs(a, 1), want[1])


def test_images_match_restatement(fx, run):
    for name in fx["names"]:
        _, h1, h2 = run[str(name)]
        if "pdh1." + name in fx:
            w1, w2 = fx["pdh1." + name], fx["pdh2." + name]
        else:       # the depth patch: the image stage on the kernel's own pairs, all of them (rounding-level ones included)
            a = run[str(name)][0]
            w1, w2 = pd_ref.images(*(a["h%d" % (d + 1)][0, : int(a["counts"][0, d])] for d in (0, 1)))
        assert np.abs(h1 - w1).max() <= IMG_ATOL, name
        assert np.abs(h2 - w2).max() <= IMG_ATOL, name
        for im in (h1, h2):
            assert im.max() in (0.0, 1.0)
    assert run["sphere"][2].max() == 1.0 and run["torus"][1].max() == 1.0


def test_long_lived_features(run):
    s = _pairs(run["sphere"][0], 1)
    assert np.sort(s[:, 1] - s[:, 0])[-1] > 0.5 * 0.1 ** 2
    t = _pairs(run["torus"][0], 0)
    assert (np.sort(t[:, 1] - t[:, 0])[-2:] > 0.5 * 0.03 ** 2).all()


def test_bits_repeat_and_batch_independent(fx):
    """two runs give identical bits; a cloud alone equals the same cloud inside a B = 256 batch"""
    from tgpose_amd import ops
    names = list(fx["names"])
    clouds = [fx["cloud." + n] for n in names if len(fx["cloud." + n]) == 1024]
    rng = np.random.RandomState(0)
    batch = np.stack([clouds[i % len(clouds)] for i in range(256)])
    batch[5] = rng.normal(size=(1024, 3)).astype(np.float32) * 0.05
    pc = torch.from_numpy(batch).to(DEV)
    a1, a2 = ops.persistence_images(pc), ops.persistence_images(pc)
    for x, y in zip(a1, a2):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for i in (0, 5, 255):
        s1, s2 = ops.persistence_images(pc[i:i + 1])
        assert torch.equal(s1[0].view(torch.int32), a1[0][i].view(torch.int32))
        assert torch.equal(s2[0].view(torch.int32), a1[1][i].view(torch.int32))


def test_overflow_and_degenerate_report_status():
    """a capped triangulation and a flat cloud set their status words and raise through persistence_images, without a fault"""
    from tgpose_amd import _lib, ops
    pc = torch.from_numpy(np.random.RandomState(1).normal(size=(2, 1024, 3)).astype(np.float32)).to(DEV)
    a = ops.alpha_persistence(pc, tet_cap=512)
    assert a["status"].cpu().tolist() == [1, 1] and a["counts"].cpu().abs().sum() == 0
    flat = pc.clone()
    flat[1, :, 2] = 0.5
    st = ops.alpha_persistence(flat)["status"].cpu().tolist()
    assert st == [0, 7]
    with pytest.raises(_lib.TgpError, match="TGP_PD_EFLAT"):
        ops.persistence_images(flat)
    h1, h2, st = ops.persistence_images(flat, check_status=False)
    assert not h1[1].any() and not h2[1].any() and int(st[1]) == 7


def test_compute_pd_matches_fixture(fx):
    from tgpose_amd.datasets.compute_pd import compute_pd
    for k in range(7):
        name = "ref%d" % k
        p1, p2 = compute_pd(fx["cloud." + name])
        assert p1.device.type == "cpu" and p1.shape == (2500,) and p1.dtype == torch.float32
        assert np.abs(p1.numpy() - fx["pdh1." + name]).max() <= IMG_ATOL
        assert np.abs(p2.numpy() - fx["pdh2." + name]).max() <= IMG_ATOL


def test_train_batch_persistence():
    """persistence=True: every other output bit-identical to persistence=False under the same RNG state; pdh1 / pdh2 equal
    ops.persistence_images(pcl_in); items carrying pdh1 are refused; RL_TDA_train_step accepts the batch"""
    from tests.test_gpu_parity import _step_db, _trainer
    from tests.util import synth_depth_scene
    from tgpose_amd import ops
    from tgpose_amd.datasets.load_data import REAL_INTRINSICS, train_batch
    B = 8
    cats = [i % 6 for i in range(B)]
    syn = _step_db(cats, 16, 11)
    items = []
    for i in range(B):
        fr = synth_depth_scene(60 + i // 4, 4)
        mask = np.zeros(fr["depth"].shape, np.uint8)
        for q in range(4):
            mask[fr["pred_masks"][:, :, q]] = q + 1
        it = dict(depth=fr["depth"], mask=mask, inst_id=i % 4 + 1, camK=REAL_INTRINSICS, bbox=fr["pred_bboxes"][i % 4])
        it.update(rotation=syn["rotation"][i].numpy(), translation=syn["translation"][i].numpy(), fsnet_scale=syn["fsnet_scale"][i].numpy(),
                  mean_shape=np.array([0.1, 0.1, 0.1], np.float32), sym_info=syn["sym_info"][i].numpy(),
                  model_point=np.random.RandomState(i).rand(64, 3).astype(np.float32) - 0.5, nocs_scale=0.3, cat_id=float(cats[i]))
        for k in ("pdh1_category", "pdh2_category", "points_category"):
            it[k] = syn[k][i].numpy()
        items.append(it)
    run = lambda p: train_batch(items, rng=np.random.RandomState(4), gen=torch.Generator().manual_seed(4), device=DEV, persistence=p)
    a, b = run(False), run(True)
    assert set(b) == set(a) | {"pdh1", "pdh2"}
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), k
        else:
            assert v == b[k]
    w1, w2 = ops.persistence_images(a["pcl_in"])
    assert torch.equal(b["pdh1"], w1) and torch.equal(b["pdh2"], w2)
    assert b["pdh1"].shape == (b["pcl_in"].shape[0], 2500) and b["pdh1"].max() == 1.0
    bad = [dict(items[0], pdh1=np.zeros(2500, np.float32))] + items[1:]
    with pytest.raises(ValueError):
        train_batch(bad, rng=np.random.RandomState(4), device=DEV, persistence=True)
    tr = _trainer(3)
    _, ld = tr.RL_TDA_train_step(b)
    torch.cuda.synchronize()
    assert ld and all(torch.isfinite(torch.as_tensor(v)).all() for d in ld.values() for v in (d.values() if isinstance(d, dict) else [d]))
