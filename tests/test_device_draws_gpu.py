"""GPU tests of the training loader's draws='device' mode: train_batch / train_clouds / TrainBatches / defor_2D with every draw a
function of (seed, key, site, counter) and no host read between the items and the step (datasets/load_data.py, csrc/draws.hip).

The mode is tied to the kernels the existing tests pin to the reference by REPLAY (the device-made draw buffers, read back and fed
to the host path's launches, give the same batch bit for bit); what is left, the draws themselves, is judged by distribution
(Kolmogorov-Smirnov at alpha = 1e-6 with a fixed seed), by the permutation properties of the selections, and by key discipline."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 8                    # with keys 0..9 and dzi=True: operators [Jitter, skipped, Dropout, Dropout, Cutout, Jitter, Crop, Jitter, Crop, Cutout]
ROW_KEYS = ("pcl_in", "aug_pcl_in", "rotation", "translation", "fsnet_scale", "aug_flags", "aug_counts")


@pytest.fixture(scope="module")
def fx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    return golden("train_loop.npz")


def _items(n=10):
    from tests.test_train_loop_gpu import _items as make
    return make(n)


def _k64(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64)).to(DEV)


def _host(dr):
    return {k: v.cpu().numpy() for k, v in dr.items()}


def _blob_item(base, side, depth_zero=False, inst=1):
    """an item on a 480 x 640 frame of plain depth whose instance mask is one side x side square inside a 440-pixel window (1.72
    source pixels per ROI pixel): side 9 .. 12 gives 26 .. 49 ROI points (abandoned after the cut: fewer than 50), side 4 .. 6 gives
    2 .. 25 (the cloud below 26 points)"""
    H, W = 480, 640
    yy, xx = np.mgrid[0:H, 0:W]
    it = dict(base)
    it["depth"] = np.zeros((H, W), np.uint16) if depth_zero else (900 + (xx + 2 * yy) % 40).astype(np.uint16)
    mask = np.zeros((H, W), np.uint8)
    mask[240:240 + side, 320:320 + side] = inst
    it.update(mask=mask, inst_id=1, bbox=np.array([20, 100, 460, 540], np.int32))
    return it


# ------------------------------------------------------------------------------------------------------------------ 1. replay
def test_replay_of_the_device_draws_equals_the_host_path(fx):
    """the draw buffers a draws='device' batch made, read back and fed to the host path's launches (_train_batch_from_draws), give
    the same rows bit for bit: dzi, roi_mask_pro 0.5, an abandoned item, accepted crops and cutouts.  _train_batch_from_draws
    launches through load_data._records and load_data._augment_rows, the functions train_batch(draws='host') itself calls (and
    draws='device' too): the comparison is with the host path's code, not with a copy of it"""
    from tgpose_amd import _lib
    from tgpose_amd.datasets.load_data import train_batch, _train_batch_from_draws, DRAW_KEYS
    items = _items(10)
    db = train_batch(items, draws="device", seed=SEED, dzi=True, roi_mask_pro=0.5, device=DEV, keep_draws=True)
    dr = _host(db["_draws"])
    assert sorted(dr) == sorted(DRAW_KEYS)
    want, keep = _train_batch_from_draws(items, dr, device=DEV)
    status, slot = db["status"].cpu().numpy(), db["item_index"].cpu().numpy()
    print("status:", status.tolist(), "counts:", db["aug_counts"].cpu().tolist())
    assert keep == [d for d in range(10) if status[d] == 0] and 4 <= len(keep) < 10
    assert status[1] == _lib.ITEM_NO_MASK and int(db["n_alive"]) == len(keep)
    assert slot.tolist() == [keep[s % len(keep)] for s in range(10)]             # fewer alive items than slots: the tail repeats them
    rows = torch.as_tensor([keep.index(i) for i in slot.tolist()], device=DEV)
    for k in ROW_KEYS:
        assert db[k].shape == want[k][rows].shape and db[k].dtype == want[k].dtype, k
        assert torch.equal(db[k], want[k][rows]), k
    op, counts = dr["op"][slot], db["aug_counts"].cpu().numpy()
    assert ((op == _lib.AUG_CROP) & (counts[:, 1] >= 0)).any() and ((op == _lib.AUG_CUTOUT) & (counts[:, 1] >= 0)).any(), (op, counts)
    assert db["aug_op"].cpu().tolist() == [[0, 0, 3, 3, 1, 0, 2, 0, 2, 1][i] for i in slot.tolist()]
    assert bool(db["aug_flags"].any()) and dr["defor_on"].any() and not dr["defor_on"].all()
    # the labels travel by slot; nothing else is on the host
    want_cat = torch.tensor([items[i]["cat_id"] for i in slot.tolist()])
    assert torch.equal(db["cat_id"].cpu(), want_cat) and all(v.is_cuda for k, v in db.items() if k != "_draws")
    assert "aug_name" not in db and db["n_alive"].dtype == torch.int32 and db["item_index"].dtype == torch.int64
    # train_clouds makes the same first draws
    cl = train_batch(items, draws="device", seed=SEED, dzi=True, roi_mask_pro=0.5, device=DEV)
    from tgpose_amd.datasets.load_data import train_clouds
    tc = train_clouds(items, draws="device", seed=SEED, dzi=True, roi_mask_pro=0.5, device=DEV)
    assert tc["PC"].shape == (10, 2048, 3) and tc["pcl_in"].shape == (10, 1024, 3) and torch.equal(tc["item_index"], cl["item_index"])
    assert torch.isfinite(tc["pcl_in"]).all()


# ------------------------------------------------------------------------------------------------------------ 2. distributions
N_DRAWS = 64 * 2048                                           # draws per site and seed
KS_BOUND = math.sqrt(math.log(2 / 1e-6) / (2 * N_DRAWS))      # one-sample critical value at alpha = 1e-6: 0.00744 for n = 131072
CORR_BOUND = 6 / math.sqrt(N_DRAWS)                           # six standard errors of a correlation of n independent pairs


def _ks(x, cdf):
    x = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    n = x.size
    f = cdf(x)
    return max(np.abs(f - np.arange(n) / n).max(), np.abs(f - np.arange(1, n + 1) / n).max())


def _corr(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("seed", [20240229, 7])
def test_draws_have_the_reference_distributions(fx, seed):
    """per draw site, n = 131072 draws (64 consecutive keys x 2048 counters) from a fixed seed: range, endpoints, KS distance to the
    site's law below sqrt(ln(2 / 1e-6) / (2 n)) = 0.00744, neighbouring counters and neighbouring keys uncorrelated within 6 / sqrt(n)
    = 0.0166"""
    from tgpose_amd import ops
    from tgpose_amd.datasets import device_draws as dd
    assert N_DRAWS >= 10 ** 5 and abs(KS_BOUND - 0.00744) < 1e-5
    keys = _k64(np.arange(64) + 1000)
    std, clip = 0.005, 0.05
    fill = {k: v.cpu().numpy() for k, v in ops.draw_fill(keys, seed, 2048, defor=True, noise=(std, clip), drop_u=True).items()}
    uni = lambda lo, hi: (lambda x: np.clip((x - lo) / (hi - lo), 0, 1))
    erf = np.vectorize(math.erf)
    normal = lambda x: 0.5 * (1 + erf(x / (std * math.sqrt(2))))        # the clamp at 10 deviations moves the law by < 1e-22
    sites = {"defor.%d" % j: (fill["defor"][..., j], uni(0, 1), 0.0, 1.0) for j in range(3)}
    sites.update({"noise.%d" % j: (fill["noise"][..., j], normal, -clip, clip) for j in range(3)})
    sites["drop_u"] = (fill["drop_u"], uni(0, 1), 0.0, 1.0)
    # the host's scalar draws are transforms of the site-0 words: the device's words, the host's transforms
    w = ops.draw_words(keys, seed, 0, 2048).cpu().numpy().view(np.uint32)
    assert np.array_equal(w, dd.philox_words(seed, np.arange(64) + 1000, 0, np.arange(2048)))
    sites["host.f64"] = (dd.uniform_f64(w[..., 0], w[..., 1]), uni(0, 1), 0.0, 1.0)
    sites["host.f32"] = (dd.uniform_f32(w[..., 2]), uni(0, 1), 0.0, 1.0)
    sites["host.dropout_ratio"] = (dd.uniform_f64(w[..., 2], w[..., 3]) * 0.5, uni(0, 0.5), 0.0, 0.5)     # max_dropout_ratio 0.5
    sites["host.aug_bb"] = (dd.uniform_f64(w[..., 1], w[..., 2]) * 0.4 + 0.8, uni(0.8, 1.2), 0.8, 1.2)
    for name, (x, cdf, lo, hi) in sites.items():
        assert x.size == N_DRAWS and x.shape == (64, 2048), name
        ks = _ks(x, cdf)
        c_ctr, c_key = _corr(x[:, :-1], x[:, 1:]), _corr(x[:-1], x[1:])
        print("seed %d site %-18s min %.6g max %.6g KS %.5f (bound %.5f) corr counters %+.5f keys %+.5f (bound %.5f)"
              % (seed, name, x.min(), x.max(), ks, KS_BOUND, c_ctr, c_key, CORR_BOUND))
        assert np.isfinite(x).all() and x.min() >= lo and (x.max() <= hi if name.startswith("noise") else x.max() < hi), name
        assert ks < KS_BOUND, (name, ks)
        assert abs(c_ctr) <= CORR_BOUND and abs(c_key) <= CORR_BOUND, (name, c_ctr, c_key)
    assert _ks(fill["noise"], normal) < KS_BOUND and abs(_corr(fill["noise"][..., 0], fill["noise"][..., 1])) <= CORR_BOUND
    # the operator index: two bits of a word, each value a quarter within six binomial deviations
    k = np.bincount((w[..., 0] & 3).reshape(-1), minlength=4)
    assert (np.abs(k - N_DRAWS / 4) <= 6 * math.sqrt(N_DRAWS * 0.25 * 0.75)).all(), k
    # bit-repeatable
    again = ops.draw_fill(keys, seed, 2048, defor=True, noise=(std, clip), drop_u=True)
    assert all(np.array_equal(again[k].cpu().numpy(), fill[k]) for k in fill)


# --------------------------------------------------------------------------------------------------------------- 3. selections
TOTALS = (1, 49, 1023, 1024, 1025, 2047, 2048, 2049, 5000, 65536)


def test_selections_are_prefixes_of_permutations(fx):
    from tgpose_amd import ops, _lib
    from tgpose_amd.datasets import device_draws as dd
    D = len(TOTALS)
    counts = torch.zeros(D, 3, dtype=torch.int32)
    counts[:, 2] = torch.tensor(TOTALS, dtype=torch.int32)
    counts = counts.to(DEV)
    keys = _k64(np.arange(D) + 50)
    for n, site, always in ((2048, _lib.SITE_SEL2K, False), (1024, _lib.SITE_SEL1K, False), (1024, _lib.SITE_SHUFFLE, True)):
        sel = ops.draw_selection(counts[:, 2], keys, 5, site, n, shuffle_always=always).cpu().numpy()
        for d, total in enumerate(TOTALS):
            s = sel[d]
            assert s.min() >= 0 and s.max() < total, (n, total)
            if total >= n:
                assert np.unique(s).size == n, (n, total)
            if not always and total < n:
                assert np.array_equal(s, np.arange(n) % total), (n, total)
            if not always and total == n:
                assert np.array_equal(s, np.arange(n))
            if always:                                         # pc_sampler: always shuffled; short clouds repeat the shuffled rows
                m = min(total, n)
                assert np.unique(s[:m]).size == m
                if total < n:
                    assert np.array_equal(s, s[:total][np.arange(n) % total])
                if total >= 49:
                    assert not np.array_equal(s[:m], np.arange(m))
            if total > n or (always and total > 1):            # the NumPy walk under the site's key, element for element
                key = dd.feistel_key(5, d + 50, site)
                assert np.array_equal(s, dd.perm_at(np.arange(n) % total, total, key)), (n, total)
    # the 1024 are a subset of the 2048: a prefix of a permutation of the 2048 slots
    p1k = ops.draw_selection(2048, keys, 5, _lib.SITE_SEL1K, 1024).cpu().numpy()
    sel2k = ops.draw_selection(counts[:, 2], keys, 5, _lib.SITE_SEL2K, 2048).cpu().numpy()
    for d, total in enumerate(TOTALS):
        assert p1k[d].min() >= 0 and p1k[d].max() < 2048 and np.unique(p1k[d]).size == 1024
        assert set(sel2k[d][p1k[d]].tolist()) <= set(sel2k[d].tolist())
        if total >= 2048:
            assert np.unique(sel2k[d][p1k[d]]).size == 1024
    # 2000 keys at total = 5000: every source index is included n / total of the time, and slot 0 is uniform over the cloud
    K, total, n = 2000, 5000, 2048
    sel = ops.draw_selection(5000, _k64(np.arange(K)), 5, _lib.SITE_SEL2K, n).cpu().numpy()
    inc = np.zeros(total)
    for row in sel:
        inc[row] += 1
    p = n / total
    bound = 6 * math.sqrt(K * p * (1 - p))                       # six binomial deviations: 131.9 around 819.2
    print("inclusion counts: min %d max %d (expected %.1f +- %.1f)" % (inc.min(), inc.max(), K * p, bound))
    assert (np.abs(inc - K * p) <= bound).all()
    bins = np.bincount(sel[:, 0] // (total // 50), minlength=50)
    bound0 = 6 * math.sqrt(K * 0.02 * 0.98)                      # 37.6 around 40
    print("slot 0 in 50 bins: min %d max %d (expected 40 +- %.1f)" % (bins.min(), bins.max(), bound0))
    assert bins.size == 50 and (np.abs(bins - K / 50) <= bound0).all()
    assert (np.diff(sel[:, :64].astype(np.int64), axis=1) < 0).any(axis=1).all()          # random order, not sorted
    # different seeds and different keys: different selections
    other = ops.draw_selection(5000, _k64(np.arange(K)), 6, _lib.SITE_SEL2K, n).cpu().numpy()
    assert not (sel == other).all(axis=1).any() and np.unique(sel[:, :8], axis=0).shape[0] == K


def test_band_subset_has_exactly_half_of_the_band(fx):
    from tgpose_amd import ops
    sizes = (0, 1, 2, 3, 1000, 65535)
    bc = torch.tensor([[2, 2, l] for l in sizes], dtype=torch.int32).to(DEV)
    u = torch.zeros(len(sizes), dtype=torch.float64, device=DEV)
    on, bits = ops.draw_band_subset(bc, u, 0.5, _k64(np.arange(len(sizes)) + 9), 3)
    flags = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    assert flags.shape == (len(sizes), 65536) and on.cpu().tolist() == [0, 1, 1, 1, 1, 1]
    for d, l in enumerate(sizes):
        assert flags[d, :l].sum() == l // 2 and flags[d, l:].sum() == 0, l
    # the reference's conditions: no deformation for an abandoned item, nor when rand() > pro
    bc2 = torch.tensor([[1, 9, 100], [9, 1, 100], [9, 9, 100], [9, 9, 100]], dtype=torch.int32).to(DEV)
    u2 = torch.tensor([0.1, 0.1, 0.6, 0.5], dtype=torch.float64, device=DEV)
    on2, bits2 = ops.draw_band_subset(bc2, u2, 0.5, _k64([1, 2, 3, 4]), 3, drop_words=8)
    assert on2.cpu().tolist() == [0, 0, 0, 1] and int((bits2[:3] != 0).sum()) == 0
    assert ops.draw_band_subset(bc2, u2, 0.5, _k64([1, 2, 3, 4]), 3, validity=False, drop_words=8)[0].cpu().tolist() == [1, 1, 0, 1]
    # per-rank frequency over 2000 keys at l = 1000: each rank is dropped half of the time, within six binomial deviations
    K, l = 2000, 1000
    bc3 = torch.tensor([[2, 2, l]] * K, dtype=torch.int32).to(DEV)
    _, b3 = ops.draw_band_subset(bc3, torch.zeros(K, dtype=torch.float64, device=DEV), 1.0, _k64(np.arange(K)), 3, drop_words=32)
    f3 = np.unpackbits(b3.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    assert (f3[:, :l].sum(axis=1) == l // 2).all() and f3[:, l:].sum() == 0
    freq, bound = f3[:, :l].sum(axis=0), 6 * math.sqrt(K * 0.25)                        # 134.2 around 1000
    print("band rank drop counts: min %d max %d (expected %d +- %.1f)" % (freq.min(), freq.max(), K // 2, bound))
    assert (np.abs(freq - K / 2) <= bound).all()


def test_defor_2d_on_the_device_draws(fx):
    """a bare mask: the deformed mask differs from the mask only on the band, by exactly l // 2 dropped band pixels"""
    from tests.morph_ref import band as band_of
    from tgpose_amd.datasets.data_augmentation import defor_2D
    m = np.zeros((128, 128), np.float32)
    m[30:90, 40:100] = 1
    m[50:60, 60:70] = 0
    band = band_of(m).astype(bool)
    hit = 0
    for key in range(8):
        out = defor_2D(torch.from_numpy(m).to(DEV), rand_pro=0.5, draws="device", seed=11, key=key).cpu().numpy()
        if np.array_equal(out, m):
            continue
        hit += 1
        assert np.array_equal(out[~band], m[~band]) and int((out[band] == 0).sum()) == int(band.sum()) // 2
    assert 0 < hit < 8


# ------------------------------------------------------------------------------------------------------------ 4. key discipline
def _by_item(seq):
    """{item: its rows} over a sequence of batches; an item met twice (a spare, a cyclic repeat) must have the same rows"""
    out = {}
    for db in seq:
        idx = db["item_index"].cpu().tolist()
        for s, i in enumerate(idx):
            row = {k: db[k][s].cpu() for k in ROW_KEYS + ("aug_op", "cat_id")}
            if i in out:
                for k in row:
                    assert torch.equal(out[i][k], row[k]), (i, k)
            out[i] = row
    return out


def _source(items, **kw):
    from tgpose_amd.datasets.load_data import TrainBatches
    gc = golden("category_clouds.npz")
    args = dict(device=DEV, dzi=True, roi_mask_pro=0.5, draws="device", spares=2, seed=3,
                category_tables=(gc["points_category"], gc["pdh1_category"], gc["pdh2_category"]))
    args.update(kw)
    return TrainBatches(items, args.pop("batch_size", 4), **args)


def _epoch(src):
    it = iter(src)
    seq = []
    for db in it:
        seq.append(db)
        it.prefetch()
    return seq


def test_key_discipline(fx):
    from tgpose_amd.datasets.load_data import train_batch
    items = _items(10)
    kw = dict(draws="device", dzi=True, roi_mask_pro=0.5, device=DEV, keep_draws=True)
    alone = train_batch([items[3]], seed=SEED, keys=[77], **kw)
    big_items = [items[(5 * j) % 10] for j in range(32)]
    big_keys = [1000 + j for j in range(32)]
    for slot in (0, 17, 31):
        its, ks = list(big_items), list(big_keys)
        its[slot], ks[slot] = items[3], 77
        big = train_batch(its, seed=SEED, keys=ks, **kw)
        s = big["item_index"].cpu().tolist().index(slot)
        for k in ROW_KEYS + ("aug_op",):
            assert torch.equal(big[k][s], alone[k][0]), (slot, k)
    # different seeds and different keys give different selections
    sel = alone["_draws"]["sel2k"][0]
    assert not torch.equal(train_batch([items[3]], seed=SEED + 1, keys=[77], **kw)["_draws"]["sel2k"][0], sel)
    assert not torch.equal(train_batch([items[3]], seed=SEED, keys=[78], **kw)["_draws"]["sel2k"][0], sel)
    assert torch.equal(train_batch([items[3]], seed=SEED, keys=[77], **kw)["_draws"]["sel2k"][0], sel)
    # TrainBatches: prefetch on = off, batch by batch; rank 0 / 1 = the union of ranks 0 / 2 and 1 / 2, item by item; the batch size
    # does not matter; a resumed epoch reproduces its items
    a, b = _epoch(_source(items, prefetch=True)), _epoch(_source(items, prefetch=False))
    assert len(a) == len(b) == 3 and [x["pcl_in"].shape[0] for x in a] == [4, 4, 2]
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k, v in x.items():
            assert torch.equal(v, y[k]), k
    one = _by_item(a)
    assert 1 not in one and len(one) >= 6                                                 # item 1 is abandoned, nothing is refilled
    two = _by_item(_epoch(_source(items, rank=0, world_size=2)) + _epoch(_source(items, rank=1, world_size=2)))
    other_b = _by_item(_epoch(_source(items, batch_size=5, spares=1)))
    assert sorted(two) == sorted(one) == sorted(other_b)
    for i in one:
        for k in one[i]:
            assert torch.equal(one[i][k], two[i][k]) and torch.equal(one[i][k], other_b[i][k]), (i, k)
    src = _source(items)
    e0 = _by_item(_epoch(src))
    e1 = _by_item(_epoch(src))
    assert any(not torch.equal(e0[i]["pcl_in"], e1[i]["pcl_in"]) for i in e0)              # a new epoch, new keys
    src2 = _source(items)
    src2.set_epoch(1)
    r1 = _by_item(_epoch(src2))
    for i in e1:
        for k in e1[i]:
            assert torch.equal(e1[i][k], r1[i][k]), (i, k)
    for i in one:
        for k in one[i]:
            assert torch.equal(one[i][k], e0[i][k]), (i, k)


# --------------------------------------------------------------------------------------------------------------- 5. abandonment
def _mixed_items():
    good = _items(4)                     # item 1 of these names an instance its frame lacks: n_valid = 0
    base = good[0]
    out = [good[0], good[1], good[2], _blob_item(base, 10, depth_zero=True)]
    out += [_blob_item(base, s) for s in (9, 10, 11, 12)] + [_blob_item(base, s) for s in (4, 5, 6)] + [good[3]]
    return out


def test_abandonment_without_a_read_back(fx, tmp_path):
    from tgpose_amd import _lib
    from tgpose_amd.datasets.load_data import train_batch, _train_batch_from_draws
    items = _mixed_items()
    D = len(items)
    kw = dict(draws="device", seed=21, roi_mask_pro=0.5, device=DEV)
    db = train_batch(items, batch_size=3, keep_draws=True, **kw)
    status = db["status"].cpu().tolist()
    print("status:", status)
    assert status[0] == status[2] == status[D - 1] == _lib.ITEM_ALIVE
    assert status[1] == _lib.ITEM_NO_MASK and status[3] == _lib.ITEM_NO_DEPTH
    assert _lib.ITEM_FEW_POINTS in status[4:8] and set(status[8:11]) == {_lib.ITEM_BELOW_26}
    alive = [d for d in range(D) if status[d] == _lib.ITEM_ALIVE]
    # the host path's keep on the same items and the same deformation bits
    want, keep = _train_batch_from_draws(items, _host(db["_draws"]), device=DEV)
    assert keep == alive
    assert db["item_index"].cpu().tolist() == alive[:3] and int(db["n_alive"]) == 3
    for k in ROW_KEYS:
        assert torch.equal(db[k], want[k][:3]), k
    # more dead items than spares: the tail repeats the alive ones cyclically, and n_alive says so
    B = len(alive) + 3
    db2 = train_batch(items, batch_size=B, **kw)
    assert int(db2["n_alive"]) == len(alive) and db2["item_index"].cpu().tolist() == [alive[s % len(alive)] for s in range(B)]
    rows = torch.as_tensor([s % len(alive) for s in range(B)], device=DEV)
    for k in ROW_KEYS:
        assert torch.equal(db2[k], want[k][rows]), k
    assert torch.equal(db2["status"], db["status"])
    # all dead: zero rows, n_alive 0
    dead = [items[d] for d in range(D) if status[d] != _lib.ITEM_ALIVE]
    db3 = train_batch(dead, batch_size=4, **kw)
    assert int(db3["n_alive"]) == 0 and db3["item_index"].cpu().tolist() == [-1] * 4
    for k, v in db3.items():
        if k not in ("status", "item_index", "n_alive"):
            assert v.shape[0] == 4 and bool((v == 0).all()), k
    # a window source_tables refuses counts as abandoned (status), it does not end the batch
    from tgpose_amd.datasets import load_data as ld
    real = ld.source_tables
    calls = []

    def refusing(center, scale, img_size=256):
        calls.append(1)
        if len(calls) == 1:
            raise ValueError("source_tables: the walk is not separable for this window (rot = 0 expected)")
        return real(center, scale, img_size)
    ld.source_tables = refusing
    try:
        db4 = train_batch(items, batch_size=3, **kw)
    finally:
        ld.source_tables = real
    rest = alive[1:]
    assert db4["status"].cpu().tolist()[0] == _lib.ITEM_WINDOW and db4["item_index"].cpu().tolist() == [rest[s % len(rest)] for s in range(3)]


def test_a_batch_without_an_alive_item_is_a_skipped_step(fx, tmp_path):
    """RL_TDA_train over [an alive batch, an all-dead batch] leaves the parameters, Ranger's state and the scheduler's count where
    the alive batch alone left them (as a NaN step does; the BatchNorm buffers see the forward, as they do in a NaN step)"""
    from tests.test_train_loop_gpu import _trainer, _Flags, _state, FLAGS_train_reset
    good = _items(4)
    good[1] = good[2]
    dead = []
    for i in range(4):
        it = dict(good[i])
        it["inst_id"] = 9
        dead.append(it)
    flags = json.loads(str(fx["flags"]))
    got = {}
    with _Flags(model_save=str(tmp_path), **flags):
        for name, items in (("alive", good), ("both", good + dead)):
            for graph in (True, False):
                tr = _trainer(71)
                lines = []
                tr.logger = type("L", (), {"info": staticmethod(lambda m: lines.append(str(m)))})()
                torch.manual_seed(13)
                src = _source(items, shuffle=False, spares=0)
                tr.RL_TDA_train(src, 1, graph=graph)
                st = _state(tr)
                got[name, graph] = {k: v for k, v in st.items() if not k.startswith("net2.") and "running_" not in k and "num_batches" not in k}
                assert tr.scheduler.last_epoch == 1
                assert any("0 batches trained with fewer alive items than slots" in l for l in lines), lines
                del tr
    FLAGS_train_reset()
    from tests.test_train_loop_gpu import _same
    for graph in (True, False):
        _same(got["alive", graph], got["both", graph])


# ---------------------------------------------------------------------------------------------------------------- 6. no host read
class _CpuCalls(object):
    """counts the device-to-host copies made through Tensor.cpu (the read-back probe of scripts/augment_time.py)"""

    def __enter__(self):
        self.n, self.cpu = 0, torch.Tensor.cpu
        me = self

        def counted(t, *a, **kw):
            me.n += bool(t.is_cuda)
            return me.cpu(t, *a, **kw)
        torch.Tensor.cpu = counted
        return self

    def __exit__(self, *a):
        torch.Tensor.cpu = self.cpu


def test_no_host_read_between_the_items_and_the_batch(fx):
    from tgpose_amd.datasets.load_data import train_batch
    from tgpose_amd.datasets.data_augmentation import OPERATOR_NAMES
    items = _items(10)
    kw = dict(dzi=True, roi_mask_pro=0.5, device=DEV)
    train_batch(items, draws="device", seed=SEED, **kw)                 # (first calls: allocator, pinned pool)
    torch.cuda.synchronize()
    # the watch is shown to work on the host mode: the band sizes, the counts and -- with an applied crop or cutout -- M
    seen = set()
    for s in range(12):
        with _CpuCalls() as c:
            db = train_batch(items[2:4], rng=np.random.RandomState(s), gen=torch.Generator().manual_seed(s), **kw)
        deferred = any(n in ("RandomCrop", "RandomCutout") and int(a) >= 0 for n, a in zip(db["aug_name"], db["aug_counts"][:, 1].cpu()))
        has_op = any(n in ("RandomCrop", "RandomCutout") for n in db["aug_name"])
        assert c.n in (2, 3) and (c.n == 3 or not deferred) and (c.n == 2 or has_op), (s, c.n, db["aug_name"])
        seen.add(c.n)
    assert seen == {2, 3}, seen
    src = _source(items, prefetch=False)                                # (its category tables are uploaded here, once)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            train_batch(items, rng=np.random.RandomState(0), gen=torch.Generator().manual_seed(0), **kw)      # the host mode synchronises
        with _CpuCalls() as c:
            db = train_batch(items, draws="device", seed=SEED, **kw)
            tb = next(iter(src))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert c.n == 0 and db["pcl_in"].shape == (10, 1024, 3) and tb["pcl_in"].shape == (4, 1024, 3)
    torch.cuda.synchronize()
    assert torch.isfinite(db["pcl_in"]).all() and 4 <= int(db["n_alive"]) < 10


# --------------------------------------------------------------------------------------------------------------- 7. the loop trains
def test_the_loop_trains_on_device_draws(fx, tmp_path):
    """RL_TDA_train over TrainBatches(draws='device'), two epochs of the ten items: graphed = eager bit for bit, a run resumed from
    the first epoch's checkpoint = the uninterrupted one, finite losses, the checkpoint's five keys"""
    from tests.test_train_loop_gpu import _trainer, _Flags, _state, _same, FLAGS_train_reset
    from tgpose_amd.trainer.RL_TDA import CHECKPOINT_KEYS
    items = _items(10)
    flags = json.loads(str(fx["flags"]))
    got, totals = {}, []

    def watched(tr):
        real = tr.loss_is_nan

        def loss_is_nan(total, n_alive=None):
            totals.append((float(total.detach()), None if n_alive is None else int(n_alive)))
            return real(total, n_alive)
        tr.loss_is_nan = loss_is_nan
        return tr

    with _Flags(model_save=str(tmp_path), **flags):
        for graph in (True, False):
            tr = watched(_trainer(81))
            torch.manual_seed(17)
            tr.RL_TDA_train(_source(items), 2, graph=graph)
            got[graph] = _state(tr)
            assert tr.scheduler.last_epoch == 6                      # 2 epochs x (4, 4, 2 items)
            del tr
        assert len(totals) == 12 and all(math.isfinite(t) and 1 <= n <= 4 for t, n in totals), totals
        _same(got[True], got[False])
        # resume: one epoch, its checkpoint, a fresh trainer and a fresh source at epoch 1
        for f in os.listdir(str(tmp_path)):
            os.remove(os.path.join(str(tmp_path), f))
        tr = _trainer(81)
        torch.manual_seed(17)
        tr.RL_TDA_train(_source(items), 1)
        rng = torch.get_rng_state()
        path = os.path.join(str(tmp_path), "rl_tda_model_00.pth")
        assert os.path.exists(path) and tuple(torch.load(path)) == CHECKPOINT_KEYS
        del tr
        tr2 = _trainer(5)
        assert tr2.load_old_model_params(path, "RL_TDA") == 0
        src = _source(items)
        src.set_epoch(1)
        torch.set_rng_state(rng)
        tr2.RL_TDA_train(src, 1)
        resumed = _state(tr2)
    FLAGS_train_reset()
    _same(resumed, got[True])
