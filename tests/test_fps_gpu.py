"""Farthest point sampling on the GPU (csrc/fps.hip, ops.farthest_points) against the numpy restatement of its contract
(tests/fps_ref.py: idx equal, distances bit for bit, clusters equal) and against what the reference's own farthest_points returned
(tests/golden/fps_ref.npz); the surfaces above it: core.utils.farthest_points_torch, clouds_from_frames(sampler='fps'), myEvaluater,
train_batch(pcl_select='fps')."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fps_ref
from tests.test_fps_cpu import NAMES
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the kernel's variants (threads x points per thread) change at these M; every boundary - 1 / 0 / + 1, and the small and odd sizes
BOUNDARIES = (64, 256, 512, 1024, 2048, 4096)
SIZES = sorted({1, 2, 63, 64, 65, 300, 1023, 1025, 2048} | {b + d for b in BOUNDARIES for d in (-1, 0, 1)})
STEPS = (1, 7, 64, 1024)
MODES = ("start", "centroid", "row0")             # start given / start NULL with init_center / init_center off


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def _cloud(M, seed, B=1):
    rng = np.random.default_rng(seed)
    return (rng.random((B, M, 3), dtype=np.float32) * np.float32(0.3) + np.float32([0.1, -0.2, 0.8])).astype(np.float32)


def _device_rows(xyz, ld):
    """the cloud on the device with rows ld floats apart; the fourth column is poison (it must not be read)"""
    t = torch.from_numpy(np.ascontiguousarray(xyz)).to(DEV)
    return t if ld == 3 else torch.cat([t, torch.full_like(t[..., :1], float("nan"))], dim=-1)


def _run(xyz, n, ld=3, counts=None, start=None, init_center=True):
    from tgpose_amd import ops
    c = None if counts is None else torch.as_tensor(np.asarray(counts, dtype=np.int32)).to(DEV)
    s = None if start is None else torch.from_numpy(np.ascontiguousarray(start, dtype=np.float32)).to(DEV)
    idx, d, cl = ops.farthest_points(_device_rows(xyz, ld), n, counts=c, start=s, init_center=init_center, return_distances=True,
                                     return_clusters=True)
    assert idx.dtype == torch.int32 and cl.dtype == torch.int32 and d.dtype == torch.float32
    return idx.cpu().numpy(), d.cpu().numpy(), cl.cpu().numpy()


def _equal(got, want, counts=None, what=""):
    (gi, gd, gc), (wi, wd, wc) = got, want
    assert np.array_equal(gi, wi), (what, "idx", int((gi != wi).sum()), np.argwhere(gi != wi)[:4].tolist())
    B, M = gd.shape
    for b in range(B):
        c = M if counts is None else int(counts[b])
        assert np.array_equal(gd[b, :c].view(np.int32), wd[b, :c].view(np.int32)), (what, b, "distance bits")
        assert np.array_equal(gc[b], wc[b]), (what, b, "clusters")
        assert np.isnan(gd[b, c:]).all() and (gc[b, c:] == -1).all()


def _mode_args(mode, xyz):
    if mode == "start":
        return dict(start=xyz.mean(axis=1, dtype=np.float64).astype(np.float32) + np.float32(0.01))
    return dict(init_center=mode == "centroid")


@pytest.mark.parametrize("M", SIZES)
def test_kernel_equals_restatement(M):
    """every n of STEPS below M, the three start modes, rows 3 and 4 floats apart: idx, distance bits, clusters"""
    xyz = _cloud(M, 100 + M)
    ran = 0
    for n in [n for n in STEPS if n < M]:
        for mode in MODES:
            kw = _mode_args(mode, xyz)
            want = fps_ref.fps_batch(xyz, n, **kw)
            for ld in (3, 4):
                _equal(_run(xyz, n, ld=ld, **kw), want, what=(M, n, mode, ld))
                ran += 1
    if M == 1:                                    # no n < M: the tiling rule is all there is
        for mode in MODES:
            kw = _mode_args(mode, xyz)
            _equal(_run(xyz, 3, **kw), fps_ref.fps_batch(xyz, 3, **kw), what=(M, 3, mode))
            ran += 1
    assert ran >= 3


def test_kernel_at_the_cap():
    from tgpose_amd import ops
    cap = ops.fps_max_points()
    xyz = _cloud(cap, 5)
    for mode in MODES:
        kw = _mode_args(mode, xyz)
        want = fps_ref.fps_batch(xyz, 64, **kw)
        for ld in (3, 4):
            _equal(_run(xyz, 64, ld=ld, **kw), want, what=("cap", mode, ld))
    with pytest.raises(ValueError, match="cap"):
        ops.farthest_points(torch.zeros(1, cap + 1, 3, device=DEV), 64)


@pytest.mark.parametrize("M,n", [(300, 64), (2500, 256)])
def test_mixed_counts_in_one_batch(M, n):
    """five clouds with counts 1, n - 1, n, n + 1 and M: the tiling rows, the shortest sampled cloud, a full one; rows at and
    beyond a count keep the sentinel that was there before the launch (the C entry point on caller-filled buffers)"""
    from tgpose_amd import _lib, ops
    counts = [1, n - 1, n, n + 1, M]
    xyz = _cloud(M, 77, B=5)
    want = fps_ref.fps_batch(xyz, n, counts=counts)
    for b, c in enumerate(counts[:3]):
        assert np.array_equal(want[0][b], np.arange(n) % c)
    for ld in (3, 4):
        _equal(_run(xyz, n, ld=ld, counts=counts), want, counts=counts, what=("mixed", ld))
    t = _device_rows(xyz, 4)
    c = torch.tensor(counts, dtype=torch.int32, device=DEV)
    idx = torch.full((5, n), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((5, M), -123.0, device=DEV)
    cl = torch.full((5, M), -99, dtype=torch.int32, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = _lib.lib().tgp_fps(p(t), 4, p(c), 5, M, n, None, 1, p(idx), p(dist), p(cl),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), want[0])
    for b, k in enumerate(counts):
        assert np.array_equal(dist[b, :k].cpu().numpy().view(np.int32), want[1][b, :k].view(np.int32))
        assert np.array_equal(cl[b, :k].cpu().numpy(), want[2][b, :k])
        assert (dist[b, k:] == -123.0).all() and (cl[b, k:] == -99).all()
    # the same clouds without the optional outputs
    assert np.array_equal(ops.farthest_points(t, n, counts=c).cpu().numpy(), want[0])


def test_ties():
    """the planar grid (equal maxima at every step), 50 points 8 times each (once the distinct points are used up every running
    distance is sqrt(3) * 1e-6: row 0 is chosen again and again, as the reference does) and a cloud of identical points (row 0 only)"""
    g = golden("fps_ref.npz")
    for name, n in (("grid", 256), ("dups", 200)):
        xyz = g[name + "_xyz"][None]
        for mode in MODES:
            kw = _mode_args(mode, xyz)
            _equal(_run(xyz, n, **kw), fps_ref.fps_batch(xyz, n, **kw), what=(name, mode))
    same = np.tile(np.float32([[0.25, -0.5, 1.0]]), (700, 1))[None]
    for mode in MODES:
        kw = _mode_args(mode, same)
        got = _run(same, 300, ld=4, **kw)
        _equal(got, fps_ref.fps_batch(same, 300, **kw), what=("identical", mode))
        assert not got[0].any()


@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_reference_fixture(name):
    """what the reference's farthest_points returned on its CPU: with its torch.mean row as the start, centres, clusters and every
    distance bit; with the kernel's own centroid (start=None), the centres"""
    g = golden("fps_ref.npz")
    xyz, n = g[name + "_xyz"][None], int(g["n"][NAMES.index(name)])
    idx, d, cl = _run(xyz, n, start=g[name + "_mean"][None])
    assert np.array_equal(idx[0], g[name + "_centers"])
    assert np.array_equal(cl[0], g[name + "_clusters"])
    assert np.array_equal(d[0].view(np.int32), g[name + "_dist"].view(np.int32))
    assert np.array_equal(_run(xyz, n, ld=4)[0][0], g[name + "_centers"])


def test_batch_independence_and_repeatability():
    """a cloud alone (M = its count) and as the live prefix of a longer row inside a batch of other counts: the same centres and
    the same distance bits (the centroid's summation tree does not depend on M); two runs are identical"""
    n = 64
    own = _cloud(700, 9)[0]
    alone = _run(own[None], n)
    big = _cloud(3000, 10, B=4)
    big[2, :700] = own
    counts = [3000, 65, 700, 1500]
    a, b = _run(big, n, counts=counts, ld=4), _run(big, n, counts=counts, ld=4)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert np.array_equal(a[0][2], alone[0][0])
    assert np.array_equal(a[1][2, :700].view(np.int32), alone[1][0].view(np.int32)) and np.array_equal(a[2][2, :700], alone[2][0])
    _equal(a, fps_ref.fps_batch(big, n, counts=counts), counts=counts, what="batch")


def test_reference_named_module():
    from torch.nn import functional as F
    from tgpose_amd.core.utils.farthest_points_torch import farthest_points, get_fps_and_center_torch
    from tgpose_amd.datasets.load_data import farthest_point_sample
    xyz = _cloud(500, 21)[0]
    t = torch.from_numpy(xyz).to(DEV)
    want = fps_ref.fps(xyz, 100)
    clusters, centers, distances = farthest_points(t, 100, return_distances=True)
    assert clusters.dtype == centers.dtype == torch.long and clusters.shape == (500,) and centers.shape == (100,)
    assert np.array_equal(centers.cpu().numpy(), want[0]) and np.array_equal(clusters.cpu().numpy(), want[2])
    assert np.array_equal(distances.cpu().numpy().view(np.int32), want[1].view(np.int32))
    two = farthest_points(t, 100, dist_func=F.pairwise_distance)
    assert len(two) == 2 and torch.equal(two[0], clusters) and torch.equal(two[1], centers)
    assert torch.equal(farthest_points(t, 100, return_center_indexes=False), clusters)
    row0 = farthest_points(t, 100, init_center=False)[1]
    assert np.array_equal(row0.cpu().numpy(), fps_ref.fps(xyz, 100, init_center=False)[0]) and int(row0[0]) == 0
    for n in (500, 501):                                                   # n_clusters >= M: arange, no sampling
        c, k = farthest_points(t, n)
        assert torch.equal(c.cpu(), torch.arange(500)) and torch.equal(k.cpu(), torch.arange(500)) and c.dtype == torch.long
        assert torch.equal(farthest_points(t, n, return_center_indexes=False).cpu(), torch.arange(500))
    assert torch.equal(farthest_point_sample(t, 100), centers)
    got = get_fps_and_center_torch(t, 100)
    assert got.shape == (101, 3) and torch.equal(got[:100], t[centers]) and torch.equal(got[100], torch.mean(t, 0))
    with pytest.raises(ValueError, match="float32 GPU tensor"):
        farthest_points(t.cpu(), 100)
    with pytest.raises(ValueError, match="float32 GPU tensor"):
        farthest_points(t.double(), 100)
    with pytest.raises(ValueError, match="dist_func"):
        farthest_points(t, 100, dist_func=lambda a, b: (a - b).abs().sum(-1))
    with pytest.raises(ValueError, match="dist_func"):
        get_fps_and_center_torch(t, 100, dist_func=torch.cdist)


# ------------------------------------------------------------------------------------------------- clouds_from_frames(sampler='fps')
K_REAL = np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]], dtype=np.float32)
N_PTS, POOL, IMG = 128, 512, 64
# (cy, cx, ry, rx) of elliptical masks; at img_size 64 the cut clouds hold about 1677, 265, 70, (fewer than 26: invalid) and 663, 183
SHAPES = ([(120, 150, 50, 50), (300, 400, 8, 30), (200, 500, 3, 30), (400, 100, 1, 1)], [(240, 320, 20, 20), (100, 500, 6, 34)])


def _frame(seed, shapes):
    rng = np.random.RandomState(seed)
    H, W = 480, 640
    yy, xx = np.mgrid[0:H, 0:W]
    depth = 800.0 + 0.3 * xx + 0.2 * yy + 25.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.randn(H, W) * 1.5
    n = len(shapes)
    masks, boxes = np.zeros((H, W, n), bool), np.zeros((n, 4), np.int32)
    for j, (cy, cx, ry, rx) in enumerate(shapes):
        m = ((yy - cy) / float(ry)) ** 2 + ((xx - cx) / float(rx)) ** 2 <= 1.0
        masks[:, :, j] = m
        ys, xs = np.where(m)
        boxes[j] = [ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]
    return dict(depth=np.clip(depth, 0, 65535).astype(np.uint16), pred_masks=masks, pred_bboxes=boxes,
                pred_class_ids=(np.arange(n) % 6 + 1).astype(np.int32), pred_scores=np.full(n, 0.9))


def test_clouds_from_frames_fps():
    from tgpose_amd import ops
    from tgpose_amd.evaluation import load_data_eval as lde
    frames = [_frame(40 + s, sh) for s, sh in enumerate(SHAPES)]
    kw = dict(img_size=IMG, n_pts=N_PTS, sampler="fps", fps_pool=POOL, device=DEV)
    state = np.random.get_state()
    out, ok = lde.clouds_from_frames(frames, K_REAL, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:], state[1:]))     # the global stream is not consumed
    out2, ok2 = lde.clouds_from_frames(frames, K_REAL, seed=99, rng=np.random.RandomState(5), **kw)
    rc = lde.build(frames, K_REAL, IMG, DEV)
    counts = rc.counts.cpu().numpy()
    total = counts[:, 2]
    valid = (total > 0) & (counts[:, 0] > 1) & (counts[:, 1] > 1)
    print("totals:", total.tolist(), "valid:", valid.tolist())
    assert [o.shape for o in out] == [(4, N_PTS, 3), (2, N_PTS, 3)]
    got, got_ok = torch.cat(out).cpu().numpy(), torch.cat(ok).cpu().numpy()
    assert np.array_equal(got.view(np.int32), torch.cat(out2).cpu().numpy().view(np.int32)) and torch.equal(torch.cat(ok), torch.cat(ok2))
    assert np.array_equal(got_ok, valid) and valid.tolist() == [True, True, True, False, True, True]
    # both candidate branches, a short cloud and an invalid one occur
    assert (total[valid] > POOL).sum() >= 2 and ((total > N_PTS) & (total <= POOL)).sum() >= 2 and ((total > 0) & (total < N_PTS)).any()
    full = rc.points(IMG * IMG).cpu().numpy()
    for d in range(len(total)):
        if not valid[d]:
            assert np.isnan(got[d]).all()
            continue
        cloud = full[d, :total[d]]
        cand = cloud[fps_ref.thin_indices(int(total[d]), POOL)]
        want = cand[fps_ref.fps(cand, N_PTS)[0]]
        assert np.array_equal(got[d].view(np.int32), want.view(np.int32)), d
        rows = {r.tobytes() for r in cloud}
        assert all(r.tobytes() in rows for r in got[d])                     # every row is a row of the detection's cloud
        if total[d] >= N_PTS:
            assert len({r.tobytes() for r in got[d]}) == N_PTS              # and no row twice (the synthetic clouds have no duplicates)
    # 'device' marks the same detections invalid
    _, ok_dev = lde.clouds_from_frames(frames, K_REAL, img_size=IMG, n_pts=N_PTS, sampler="device", seed=1, device=DEV)
    assert torch.equal(torch.cat(ok_dev), torch.cat(ok))
    with pytest.raises(ValueError, match="fps_pool"):
        lde.clouds_from_frames(frames, K_REAL, img_size=IMG, n_pts=N_PTS, sampler="fps", fps_pool=ops.fps_max_points() + 1, device=DEV)
    with pytest.raises(ValueError, match="'numpy', 'device' or 'fps'"):
        lde.clouds_from_frames(frames, K_REAL, img_size=IMG, n_pts=N_PTS, sampler="farthest", device=DEV)


def test_evaluater_fps_is_repeatable():
    """myEvaluater(sampler='fps'): two runs with different sampler seeds and NumPy states give the same poses bit for bit (torch's
    global generator, from which the network draws its pooling subsets as the reference's does, is set alike: that draw is not the
    input side's)"""
    from tests.util import synth_depth_scene
    from tgpose_amd import FLAGS, PoseNet9D, seeded_state_dict
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    net = PoseNet9D()
    net.load_state_dict(seeded_state_dict(0), strict=True)
    net = net.to(DEV).eval()
    FLAGS.train = 0
    recs = [dict(frame=synth_depth_scene(900 + i, 3)) for i in range(2)]
    np.random.seed(1)
    torch.manual_seed(8)
    a = myEvaluater(net, frames_per_batch=2, sampler="fps", seed=3).run(recs)
    np.random.seed(2)
    torch.manual_seed(8)
    b = myEvaluater(net, frames_per_batch=2, sampler="fps", seed=4).run(recs)
    assert len(a) == len(b) >= 1 and sum(len(r["pred_RTs"]) for r in a) >= 3
    for ra, rb in zip(a, b):
        for k in ("pred_RTs", "pred_scales"):
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
        assert np.isfinite(np.asarray(ra["pred_RTs"])).all()


# ------------------------------------------------------------------------------------------------------ train_batch(pcl_select='fps')
def _train_items():
    """three items, all alive: two of the synthetic scenes and one short cloud (a 30 x 30 pixel mask: fewer than 2048 points)"""
    from tests.test_device_draws_gpu import _blob_item
    from tests.test_train_loop_gpu import _items
    good = _items(3)
    items = [good[0], _blob_item(good[0], 30), good[2]]
    return [{k: v for k, v in it.items() if k not in ("pdh1", "pdh2")} for it in items]


def _same(a, b, key):
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().reshape(-1).view(torch.uint8), b.cpu().reshape(-1).view(torch.uint8)), key
    else:
        assert a == b, key


@pytest.mark.parametrize("draws", ["host", "device"])
def test_train_batch_fps(draws, monkeypatch):
    from tgpose_amd.datasets import load_data as ld
    items = _train_items()
    _, counts = ld._roi_records(items, 256, torch.device(DEV))
    assert 50 <= counts[1][2] < 2048 < min(counts[0][2], counts[2][2]), counts       # one short item, none abandoned

    def batch(**kw):
        if draws == "host":
            return ld.train_batch(items, rng=np.random.RandomState(5), gen=torch.Generator().manual_seed(5), device=DEV, persistence=True, **kw)
        return ld.train_batch(items, draws="device", seed=13, device=DEV, persistence=True, **kw)

    fps = batch(pcl_select="fps")
    default = batch()
    # the 'random' batch of the same draws: on the host path the second _sample_points permutation comes from a stream of its own, so
    # the draws around it are the ones the fps batch made (which does not draw it); on the device path its site is simply unused
    side = np.random.RandomState(77)
    plain = ld._selection
    monkeypatch.setattr(ld, "_selection", lambda total, n_pts, rng: plain(total, n_pts, side if n_pts == 1024 else rng))
    rnd = batch(pcl_select="random")
    monkeypatch.undo()

    B = 3
    assert set(fps) == set(rnd) | {"PC", "pcl_index"} and "PC" not in rnd and "pcl_index" not in rnd
    assert fps["PC"].shape == (B, 2048, 3) and fps["pcl_index"].shape == (B, 1024) and fps["pcl_index"].dtype == torch.int32
    PC = fps["PC"].cpu().numpy()
    want = fps_ref.fps_batch(PC, 1024)[0]
    assert np.array_equal(fps["pcl_index"].cpu().numpy(), want)
    picked = np.take_along_axis(PC, want[:, :, None].astype(np.int64), axis=1)
    assert np.array_equal(fps["pcl_in"].cpu().numpy().view(np.int32), picked.view(np.int32))
    differing = {"pcl_in", "pdh1", "pdh2", "pd_status"}
    for k in rnd:
        if k not in differing:
            _same(fps[k], rnd[k], k)
    assert not torch.equal(fps["pcl_in"], rnd["pcl_in"]) and fps["pdh1"].shape == rnd["pdh1"].shape == (B, 2500)
    assert torch.isfinite(fps["pdh1"]).all() and torch.isfinite(fps["pdh2"]).all()
    # the default is 'random', with the streams it always had: equal to an explicit 'random' call from the same state
    explicit = ld.train_batch(items, rng=np.random.RandomState(5), gen=torch.Generator().manual_seed(5), device=DEV, persistence=True,
                              pcl_select="random") if draws == "host" else batch(pcl_select="random")
    assert set(default) == set(explicit) and "PC" not in default and "pcl_index" not in default
    for k in default:
        _same(default[k], explicit[k], k)


def test_train_batches_pass_the_option_on():
    from tgpose_amd.datasets.load_data import TrainBatches
    items = _train_items()
    src = TrainBatches(items, 3, rng=np.random.RandomState(2), gen=torch.Generator().manual_seed(2), device=DEV, prefetch=False,
                       shuffle=False, pcl_select="fps")
    db = next(iter(src))
    want = fps_ref.fps_batch(db["PC"].cpu().numpy(), 1024)[0]
    assert np.array_equal(db["pcl_index"].cpu().numpy(), want)
    with pytest.raises(ValueError, match="pcl_select"):
        TrainBatches(items, 3, pcl_select="farthest", device=DEV)
