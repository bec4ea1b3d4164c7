"""The mask deformation's host half (defor_2D's draws) and its test oracle, without a GPU: tests/morph_ref.py's restatement of
OpenCV's erode / dilate against scipy.ndimage, and load_data.defor_draws replaying the reference's defor_2D draws on the
fixture's masks (tests/golden/defor.npz, recorded from the reference's own code by tests/golden/make_defor_golden.py)."""
import numpy as np
import pytest
import scipy.ndimage as ndi

from tests import morph_ref
from tests.test_augment_cpu import np_rng
from tests.util import golden

S = 256


@pytest.fixture(scope="module")
def fx():
    return golden("defor.npz")


def unpack(a):
    return np.unpackbits(a)[:S * S].reshape(S, S)


def test_morph_ref_vs_scipy():
    """erode / dilate of the 2x2 ellipse = grey_erosion / grey_dilation with footprint [[0,1,0],[1,1,0],[0,0,0]] (reflected for
    dilation) and mode='nearest' (a replicated neighbour equals the pixel itself: the same as ignoring it)"""
    k = morph_ref.getStructuringElement(morph_ref.MORPH_ELLIPSE, (2, 2))
    assert np.array_equal(k, [[0, 1], [1, 1]])
    fp = np.array([[0, 1, 0], [1, 1, 0], [0, 0, 0]], bool)
    r = np.random.RandomState(0)
    for t in range(40):
        h, w = r.randint(1, 70, 2)
        m = (r.rand(h, w) < r.rand()).astype(np.float32)
        assert np.array_equal(morph_ref.erode(m, k, 3), ndi.grey_erosion(m, footprint=fp, mode="nearest"))
        assert np.array_equal(morph_ref.dilate(m, k, 3), ndi.grey_dilation(m, footprint=fp[::-1, ::-1], mode="nearest"))


def band_counts(m):
    """the band launch's counts as data_augmentation.defor_2D passes them on: a mask has no validity test (n_depth = n_valid = 2)"""
    return np.array([[2, 2, int(morph_ref.band(m).sum())]], np.int32)


def test_defor_draws_replay_reference(fx):
    """defor_draws + the restated deformation = the reference's defor_2D, output and generator state, on every fixture mask"""
    from tgpose_amd.datasets.load_data import defor_draws
    n = len(fx["m.names"])
    assert n >= 36
    for i in range(n):
        p = "m.%d." % i
        m = unpack(fx[p + "mask"]).astype(np.float32)
        rng = np.random.RandomState(int(fx[p + "seed"]))
        on, bits = defor_draws(band_counts(m), float(fx[p + "pro"]), rng)
        drop = np.unpackbits(bits.view(np.uint8), bitorder="little")
        got = morph_ref.defor_mask(m, np.nonzero(drop)[0]) if on[0] else m
        assert np.array_equal(got > 0, unpack(fx[p + "out"]) > 0), fx["m.names"][i]
        want = np_rng(fx, p + "after").get_state()
        st = rng.get_state()
        assert np.array_equal(st[1], want[1]) and st[2:] == want[2:], fx["m.names"][i]


def test_fixture_covers_the_cases(fx):
    """items kept, abandoned by the validity tests, raising IndexError and abandoned under 50 points after the deformation; one
    whose deformed mask grew; both DZI kinds"""
    outs = [int(fx["gi.%d.outcome" % n]) for n in range(int(fx["gi.n_items"]))]
    assert {0, 1, 2, 3} <= set(outs)
    assert any(int(fx["gi.%d.n_def" % n]) > int(fx["gi.%d.n_mask" % n]) for n in range(len(outs)))
    assert {str(fx["gi.%d.dzi" % n]) for n in range(len(outs))} == {"uniform", "none"}


def _state_equal(rng, fx, prefix):
    want, st = np_rng(fx, prefix).get_state(), rng.get_state()
    return np.array_equal(st[1], want[1]) and st[2:] == want[2:]


def test_aug_bbox_dzi_vs_reference(fx):
    """load_data.aug_bbox_dzi = the reference's aug_bbox_DZI (uniform, roi10d, none) bit for bit, window and generator state; and
    the windows of the fixture's __getitem__ items from their entry seeds"""
    from tests.util import synth_depth_scene
    from tgpose_amd.config import FLAGS
    from tgpose_amd.datasets.load_data import aug_bbox_dzi
    assert fx["dzi.flags"].tolist() == [FLAGS.DZI_PAD_SCALE, FLAGS.DZI_SCALE_RATIO, FLAGS.DZI_SHIFT_RATIO]
    kinds = set()
    for n in range(int(fx["dzi.n"])):
        p = "dzi.%d." % n
        fr = synth_depth_scene(int(fx[p + "scene"]), 4)
        H, W = fr["depth"].shape
        rng = np.random.RandomState(int(fx[p + "seed"]))
        c, sc = aug_bbox_dzi(fr["pred_bboxes"][int(fx[p + "det"])], H, W, rng, dzi_type=str(fx[p + "kind"]))
        assert np.array_equal(np.array([c[0], c[1], sc], np.float64).view(np.int64), fx[p + "window"].view(np.int64)), n
        assert _state_equal(rng, fx, p + "after"), n
        kinds.add(str(fx[p + "kind"]))
    assert kinds == {"uniform", "roi10d", "none"}
    for n in range(int(fx["gi.n_items"])):
        p = "gi.%d." % n
        fr = synth_depth_scene(int(fx[p + "scene"]), 4)
        H, W = fr["depth"].shape
        rng = np.random.RandomState(int(fx[p + "seed"]))
        c, sc = aug_bbox_dzi(fr["pred_bboxes"][int(fx[p + "det"])], H, W, rng, dzi_type=str(fx[p + "dzi"]))
        assert np.array_equal(np.array([c[0], c[1], sc], np.float64).view(np.int64), fx[p + "window"].view(np.int64)), n
        assert _state_equal(rng, fx, p + "np_dzi"), n
    with pytest.raises(NotImplementedError):
        aug_bbox_dzi(fr["pred_bboxes"][0], H, W, np.random.RandomState(0), dzi_type="truncnorm")


def test_item_total_mirrors_the_reference_exceptions():
    """tgp_roi_cloud_defor writes -(1 + deformed count) below 26 points: 0 points -> np.min's ValueError, else IndexError with the
    deformed size; the undeformed kernel's -1 reports n_valid"""
    from tgpose_amd.datasets.load_data import _item_total
    with pytest.raises(ValueError):
        _item_total(np.array([9, 4, -1]), 50, deformed=True)
    with pytest.raises(IndexError, match="size 3"):
        _item_total(np.array([9, 4, -4]), 50, deformed=True)
    with pytest.raises(IndexError, match="size 4"):
        _item_total(np.array([9, 4, -1]), 50)
    assert _item_total(np.array([9, 1, -1]), 50, deformed=True) is None
    assert _item_total(np.array([90, 60, 49]), 50, deformed=True) is None
    assert _item_total(np.array([90, 60, 50]), 50, deformed=True) == 50


def test_refused_batch_leaves_rng_untouched():
    """every item is checked before the first DZI draw"""
    from tgpose_amd.datasets.load_data import _roi_records
    from tests.util import synth_depth_scene
    fr = synth_depth_scene(41, 4)
    mask = np.zeros(fr["depth"].shape, np.uint8)
    good = dict(depth=fr["depth"], mask=mask, inst_id=1, camK=np.eye(3, dtype=np.float32), bbox=fr["pred_bboxes"][0])
    rng, ref = np.random.RandomState(3), np.random.RandomState(3)
    with pytest.raises(ValueError):
        _roi_records([good, dict(good, inst_id=0)], 256, "cpu", rng, 0.5, dzi=True)
    st, want = rng.get_state(), ref.get_state()
    assert np.array_equal(st[1], want[1]) and st[2:] == want[2:]
