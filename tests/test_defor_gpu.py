"""The training loader's mask deformation (defor_2D) on the device: tgp_roi_band + tgp_roi_cloud_defor against the reference's own
defor_2D and training __getitem__ (tests/golden/defor.npz, tests/golden/make_defor_golden.py)."""
import numpy as np
import pytest
import torch

from tests import morph_ref
from tests.test_augment_cpu import np_rng
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 256
PC_TOL, LABEL_TOL = 2e-6, 1e-6          # the bars of tests/test_augment_gpu.py
LABELS = ("rotation", "translation", "fsnet_scale", "mean_shape", "sym_info", "model_point", "nocs_scale", "cat_id")


@pytest.fixture(scope="module")
def fx():
    return golden("defor.npz")


def same_records(ra, ca, rb, cb, d=None):
    """the records a launch defines (the first counts[d][2] of each item; the rest of the scratch is undefined) and the counts agree"""
    rows = range(len(ca)) if d is None else [d]
    for i in rows:
        n = max(int(ca[i][2]), 0)
        if not (np.array_equal(ca[i], cb[i]) and torch.equal(ra.recs[i, :n], rb.recs[i, :n])):
            return False
    return True


def same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def fixture_items(fx):
    """-> list of (item with the recorded window, fixture index); the frames as make_defor_golden.item_mask builds them"""
    from tests.util import synth_depth_scene
    from tgpose_amd.datasets.load_data import REAL_INTRINSICS
    out = []
    for n in range(int(fx["gi.n_items"])):
        p = "gi.%d." % n
        fr = synth_depth_scene(int(fx[p + "scene"]), 4)
        mask = np.zeros(fr["depth"].shape, np.uint8)
        for q in range(4):
            mask[fr["pred_masks"][:, :, q]] = q + 1
        j, w, variant = int(fx[p + "det"]), fx[p + "window"], str(fx[p + "variant"])
        if variant.startswith("tiny:"):
            ys, xs = np.nonzero(mask == j + 1)
            mask[mask == j + 1] = 0
            mask[ys[:int(variant[5:])], xs[:int(variant[5:])]] = j + 1
        out.append((dict(depth=fr["depth"], mask=mask, inst_id=int(fx[p + "inst"]), camK=REAL_INTRINSICS, bbox_center=w[:2].copy(),
                         scale=float(w[2]), bbox=fr["pred_bboxes"][j]), n))
    return out


def roi_restated(item):
    """the warped ROI mask and depth (numpy; nearest-neighbour warp through the same source tables)"""
    from tgpose_amd.datasets.load_data import source_tables
    sx, sy = source_tables(item["bbox_center"], item["scale"], S)
    H, W = item["depth"].shape
    inb = (sy[:, None] >= 0) & (sy[:, None] < H) & (sx[None, :] >= 0) & (sx[None, :] < W)
    cy, cx = np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)
    M = inb & (item["mask"][cy][:, cx] == item["inst_id"])
    d = np.where(inb, item["depth"][cy][:, cx], 0)
    return M.astype(np.float32), d


def test_band_counts_vs_restatement(fx):
    from tgpose_amd import ops
    from tgpose_amd.datasets.load_data import source_tables
    for item, n in fixture_items(fx):
        M, d = roi_restated(item)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        tabs = up(source_tables(item["bbox_center"], item["scale"], S)[None])
        H, W = item["depth"].shape
        got = ops.roi_band(up(item["depth"][None].view(np.int16)), up(item["mask"].reshape(-1)), up(np.zeros(1, np.int64)),
                           up(np.ones(1, np.int32)), up(np.zeros(1, np.int32)), None, roi_size=S, tables=tabs,
                           mask_val=up(np.array([item["inst_id"]], np.int32))).cpu().numpy()[0]
        want = [int((d > 0).sum()), int(((d > 0) & (M > 0)).sum()), int(morph_ref.band(M).sum())]
        assert list(got) == want, n
        assert int(fx["gi.%d.n_mask" % n]) in (-1, int(M.sum()))


def test_device_defor_2D_vs_reference(fx):
    from tgpose_amd.datasets.data_augmentation import defor_2D
    for i in range(len(fx["m.names"])):
        p = "m.%d." % i
        m = np.unpackbits(fx[p + "mask"])[:S * S].reshape(S, S).astype(np.float32)
        rng = np.random.RandomState(int(fx[p + "seed"]))
        got = defor_2D(torch.from_numpy(m)[None].to(DEV), rand_r=3, rand_pro=float(fx[p + "pro"]), rng=rng)
        want = np.unpackbits(fx[p + "out"])[:S * S].reshape(S, S).astype(np.float32)
        assert got.shape == (S, S) and np.array_equal(got.cpu().numpy(), want), fx["m.names"][i]
        assert same_state(rng, np_rng(fx, p + "after")), fx["m.names"][i]


def test_deformed_cut_cloud_vs_reference_getitem(fx):
    """from NumPy's state after aug_bbox_DZI: the deformation draws + the deformed compaction give the reference's cut cloud bit for
    bit and leave the generator where the reference's generate_aug_parameters finds it; abandoned items match its outcome"""
    from tgpose_amd import ops
    from tgpose_amd.datasets.load_data import _item_total, _roi_records
    seen = set()
    for item, n in fixture_items(fx):
        p = "gi.%d." % n
        rng = np_rng(fx, p + "np_dzi")
        it = {k: v for k, v in item.items() if k != "bbox"}
        outcome = int(fx[p + "outcome"])
        seen.add(outcome)
        rr, counts = _roi_records([it], S, torch.device(DEV), rng, float(fx[p + "pro"]))
        if outcome in (2, 4):
            with pytest.raises(IndexError if outcome == 2 else ValueError):
                _item_total(counts[0], 50, deformed=True)
            continue
        total = _item_total(counts[0], 50, deformed=True)
        if outcome in (1, 3):
            assert total is None, n
            continue
        cut = fx[p + "cut"]
        assert total == cut.shape[0], n
        got = ops.cloud_select(rr, torch.arange(total, dtype=torch.int32, device=DEV)[None].contiguous())[0].cpu().numpy()
        assert np.array_equal(got.view(np.int32), cut.view(np.int32)), n
        assert same_state(rng, np_rng(fx, p + "np_gap")), n
    assert {0, 1, 2, 3} <= seen


def _batch_items(fx, n_items):
    items = [it for it, _ in fixture_items(fx)]
    return [{k: v for k, v in items[i % len(items)].items() if k != "bbox"} for i in range(n_items)]


def test_none_is_todays_path_and_unapplied_is_bit_identical(fx):
    from tgpose_amd.datasets.load_data import _roi_records, train_clouds
    items = _batch_items(fx, 6)
    dev = torch.device(DEV)
    r0, c0 = _roi_records(items, S, dev)
    r1, c1 = _roi_records(items, S, dev, np.random.RandomState(1), None)
    assert same_records(r0, c0, r1, c1)
    a = train_clouds(items, rng=np.random.RandomState(5), device=DEV)
    b = train_clouds(items, rng=np.random.RandomState(5), device=DEV, roi_mask_pro=None)
    for x, y in zip(a, b):
        assert (x is None) == (y is None) and (x is None or (torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])))

    class Above(np.random.RandomState):            # every rand() above pro: nothing applied, only extra draws
        def rand(self, *a):
            super().rand(*a)
            return 0.99
    r2, c2 = _roi_records(items, S, dev, Above(1), 0.5)
    for d in range(len(items)):
        n = int(c0[d][2]) if c0[d][2] > 0 else 0
        assert np.array_equal(c0[d], c2[d]) and torch.equal(r0.recs[d, :n], r2.recs[d, :n]), d


def test_pro_zero_draws_one_rand_per_valid_item(fx):
    from tgpose_amd.datasets.load_data import _roi_records
    items = _batch_items(fx, 5) + [dict(_batch_items(fx, 1)[0], inst_id=9)]       # the last: no pixel of its instance
    dev = torch.device(DEV)
    rng, ref = np.random.RandomState(7), np.random.RandomState(7)
    r0, c0 = _roi_records(items, S, dev)
    r1, c1 = _roi_records(items, S, dev, rng, 0.0)
    for _ in range(5):
        ref.rand()
    assert same_state(rng, ref)
    assert np.array_equal(c0, c1)
    for d in range(len(items)):
        n = max(int(c0[d][2]), 0)
        assert torch.equal(r0.recs[d, :n], r1.recs[d, :n])


def test_item_in_batch_of_32_equals_item_alone(fx):
    from tgpose_amd import ops
    from tgpose_amd.datasets.load_data import _roi_records, defor_draws, source_tables
    items = _batch_items(fx, 32)
    dev = torch.device(DEV)
    full, cf = _roi_records(items, S, dev, np.random.RandomState(11), 1.0)
    full2, cf2 = _roi_records(items, S, dev, np.random.RandomState(11), 1.0)
    assert same_records(full, cf, full2, cf2)
    # item by item, replaying the batch's drop sets
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    H, W = items[0]["depth"].shape
    band = np.stack([[int(v) for v in ops.roi_band(up(it["depth"][None].view(np.int16)), up(it["mask"].reshape(-1)),
                                                   up(np.zeros(1, np.int64)), up(np.ones(1, np.int32)), up(np.zeros(1, np.int32)), None,
                                                   roi_size=S, tables=up(source_tables(it["bbox_center"], it["scale"], S)[None]),
                                                   mask_val=up(np.array([it["inst_id"]], np.int32))).cpu().numpy()[0]] for it in items])
    on, bits = defor_draws(band, 1.0, np.random.RandomState(11))
    for d in range(0, 32, 5):
        it = items[d]
        rr = ops.roi_cloud(up(it["depth"][None].view(np.int16)), up(it["mask"].reshape(-1)), up(np.zeros(1, np.int64)),
                           up(np.ones(1, np.int32)), up(np.zeros(1, np.int32)), None,
                           up(np.array([[it["camK"][0, 0], it["camK"][1, 1], it["camK"][0, 2], it["camK"][1, 2]]], np.float32)),
                           roi_size=S, tables=up(source_tables(it["bbox_center"], it["scale"], S)[None]),
                           mask_val=up(np.array([it["inst_id"]], np.int32)), cut_frac=0.15, defor=(up(on[d:d + 1]), up(bits[d:d + 1])))
        c = rr.counts.cpu().numpy()[0]
        assert np.array_equal(c, cf[d]), d
        n = max(int(c[2]), 0)
        assert torch.equal(rr.recs[0, :n], full.recs[d, :n]), d


def test_argument_errors_raise_before_launch(fx):
    from tgpose_amd import ops
    from tgpose_amd.datasets.data_augmentation import defor_2D
    from tgpose_amd.datasets.load_data import train_clouds
    items = _batch_items(fx, 2)
    with pytest.raises(ValueError):
        train_clouds(items, device=DEV, roi_mask_pro=1.5)
    with pytest.raises(ValueError):
        train_clouds(items, device=DEV, roi_mask_pro=0.5, dzi=True)            # dzi needs 'bbox'
    with pytest.raises(ValueError):
        defor_2D(torch.full((S, S), 0.5, device=DEV), rand_pro=1.0)
    with pytest.raises(ValueError):
        defor_2D(torch.zeros(100, 100, device=DEV), rand_pro=1.0)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
    depth, masks = z(1, S, S, dt=torch.int16), z(S * S, dt=torch.uint8)
    args = (depth, masks, z(1, dt=torch.int64), z(1) + 1, z(1), None, torch.ones(1, 4, device=DEV))
    tabs = torch.arange(S, dtype=torch.int32, device=DEV).repeat(1, 2, 1).contiguous()
    with pytest.raises(ValueError):
        ops.roi_cloud(*args, roi_size=S, tables=tabs, defor=(z(2), z(1, 4)))                 # defor_on of the wrong length
    with pytest.raises(ValueError):
        ops.roi_cloud(*args, roi_size=S, tables=tabs, defor=(z(1), z(1, 4096)))              # bitmap too long
    with pytest.raises(TypeError):
        ops.roi_cloud(*args, roi_size=S, tables=tabs, defor=(z(1, dt=torch.int64), z(1, 4)))
    with pytest.raises(ValueError):
        ops.roi_cloud(*args, roi_size=S, tables=tabs, cut_frac=-0.5, defor=(z(1), z(1, 4)))


def test_train_batch_end_to_end_vs_reference_getitem(fx):
    """train_batch([item], roi_mask_pro=pro, dzi=True) from the reference's entry seed (NumPy and torch) = the reference's training
    __getitem__ from aug_bbox_DZI through pc_sampler: the operator equal; pcl_in, rotation, translation, fsnet_scale within the bars
    of tests/test_augment_gpu.py; aug_pcl_in within them where the operator is not an applied crop / cutout, and M equal where the
    recorder found the chosen box clear of the points"""
    from tgpose_amd.config import FLAGS
    from tgpose_amd.datasets.data_augmentation import OPERATOR_NAMES
    from tgpose_amd.datasets.load_data import train_batch
    kept = 0
    old = FLAGS.DZI_TYPE
    try:
        for item, n in fixture_items(fx):
            p = "gi.%d." % n
            if int(fx[p + "outcome"]) != 0:
                continue
            kept += 1
            it = {k: v for k, v in item.items() if k not in ("bbox_center", "scale")}
            it.update({k: fx[p + "in." + k] for k in LABELS})
            FLAGS.DZI_TYPE = str(fx[p + "dzi"])
            db = train_batch([it], rng=np.random.RandomState(int(fx[p + "seed"])),
                             gen=torch.Generator().manual_seed(int(fx[p + "torch_base.seed"])), device=DEV,
                             roi_mask_pro=float(fx[p + "pro"]), dzi=True)
            assert db["aug_name"] == [OPERATOR_NAMES[int(fx[p + "op"])]], n
            for k, tol in (("pcl_in", PC_TOL), ("rotation", LABEL_TOL), ("translation", LABEL_TOL), ("fsnet_scale", LABEL_TOL)):
                assert np.abs(db[k][0].cpu().numpy() - fx[p + "out." + k]).max() <= tol, (n, k)
            if p + "out.aug_pcl_in" in fx:
                assert np.abs(db["aug_pcl_in"][0].cpu().numpy() - fx[p + "out.aug_pcl_in"]).max() <= PC_TOL, n
            if int(fx[p + "M_pinned"]):
                assert int(db["aug_counts"][0, 0]) == int(fx[p + "M"]), n
    finally:
        FLAGS.DZI_TYPE = old
    assert kept >= 8
