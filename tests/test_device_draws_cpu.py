"""CPU tests of the training loader's draws='device' mode (datasets/load_data.py, datasets/device_draws.py, csrc/draws.hip): the
constants of the new entry points, their argument errors (which return before any launch), the NumPy restatement of the generator against
words recorded on the device, and the permutation walk restated in NumPy."""
import ctypes
import os

import numpy as np
import pytest

from tests.util import ROOT

TOTALS = (1, 49, 1023, 1024, 1025, 2047, 2048, 2049, 5000, 65536)


def test_new_symbols_are_declared_bound_and_exported():
    """the ABI number and the counts of the draw constants; tests/test_abi_cpu.py holds every symbol, type and value against the header"""
    from tgpose_amd import _lib
    assert _lib.lib().tgp_version() == _lib.ABI_VERSION == 9          # additive: the ABI number stays
    consts = [k for k in _lib.CONSTANTS if k.split("_")[0] in ("SITE", "ITEM", "DRAW", "GATHER")]
    assert len(consts) == 8 + 6 + 2 + 1
    assert sorted(_lib.CONSTANTS[k] for k in consts if k.startswith("SITE_")) == list(range(8))
    assert sorted(_lib.CONSTANTS[k] for k in consts if k.startswith("ITEM_")) == list(range(6))


def test_argument_errors_return_before_any_launch():
    from tgpose_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(8)                        # a non-null pointer that is never followed: every call below is refused
    assert h.tgp_draw_words(None, 1, 0, 0, 1, one, None) == -1 and h.tgp_draw_words(one, 0, 0, 0, 1, one, None) == -1
    assert h.tgp_draw_band_subset(one, one, 0.5, one, 0, 1, 1, one, None, 2048, None) == -1
    assert h.tgp_draw_band_subset(one, one, 0.5, one, 0, 1, 1, one, one, 2049, None) == -1          # more than 65536 ranks
    assert h.tgp_draw_band_subset(one, one, 0.5, one, 0, 1, 1, one, one, 12, None) == -1            # not whole 256-rank blocks
    assert h.tgp_draw_band_subset(one, one, 1.5, one, 0, 1, 1, one, one, 2048, None) == -1
    assert h.tgp_draw_alive(one, None, 4, 5, 50, one, one, one, None) == -1                          # B > D
    assert h.tgp_draw_alive(one, None, _lib.DRAW_MAX_ITEMS + 1, 4, 50, one, one, one, None) == -1
    assert h.tgp_draw_alive(None, None, 4, 4, 50, one, one, one, None) == -1
    assert h.tgp_draw_selection(None, 0, -1, one, 0, 2, 1, 2048, 0, one, None) == -1
    assert h.tgp_draw_selection(one, 0, 0, one, 0, 2, 1, 2048, 0, one, None) == -1                   # a totals pointer without a stride
    assert h.tgp_draw_selection(None, 0, 5, one, 0, 2, 1, 0, 0, one, None) == -1
    assert h.tgp_draw_fill(one, 0, 1, 2048, None, None, 0.0, 0.0, None, None) == -1                  # nothing to fill
    assert h.tgp_draw_fill(one, 0, 1, 2048, None, one, -1.0, 0.05, None, None) == -1
    a = _lib.GatherSlotsArgs()
    assert h.tgp_gather_slots(a, None) == -1
    a.slot_item, a.B, a.D, a.n = 8, 1, 1, _lib.GATHER_SLOTS_MAX + 1
    assert h.tgp_gather_slots(a, None) == -1
    a.n = 1
    a.src[0], a.dst[0], a.row_words[0] = 8, 8, 4                                                     # in place
    assert h.tgp_gather_slots(a, None) == -1


def test_python_argument_errors():
    from tgpose_amd.datasets import load_data as ld, data_augmentation as da
    with pytest.raises(ValueError, match="draws must be"):
        ld.train_batch([{}], draws="gpu")
    with pytest.raises(ValueError, match="draws must be"):
        ld.train_clouds([{}], draws="gpu")
    with pytest.raises(ValueError, match="draws must be"):
        ld.TrainBatches([{}], 1, draws="gpu", seed=0, device="cpu")
    with pytest.raises(ValueError, match="spares"):
        ld.TrainBatches([{}], 1, draws="device", spares=-1, seed=0, device="cpu")
    with pytest.raises(ValueError, match="needs a seed"):
        ld.train_batch([{}], draws="device", device="cpu")
    with pytest.raises(ValueError, match="batch_size"):
        ld.train_batch([{}], draws="device", seed=1, batch_size=2, device="cpu")
    with pytest.raises(ValueError, match="draws must be"):
        da.defor_2D(None, draws="gpu")
    with pytest.raises(ValueError, match="needs a seed"):
        da.defor_2D(None, draws="device")


def test_numpy_philox_known_answers():
    """Philox-4x32-10 of Random123's known-answer file (kat_vectors): counter and key all zero, all ones, and the digits of pi"""
    from tgpose_amd.datasets import device_draws as dd
    # philox_words(seed, key, site, counter): Philox key = (seed lo, seed hi), counter = (counter, site, key lo, key hi)
    w = dd.philox_words(0, [0], 0, [0])[0, 0]
    assert [int(x) for x in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    w = dd.philox_words(2 ** 64 - 1, [2 ** 64 - 1], 0xffffffff, [0xffffffff])[0, 0]
    assert [int(x) for x in w] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    w = dd.philox_words((0x299f31d0 << 32) | 0xa4093822, [(0x03707344 << 32) | 0x13198a2e], 0x85a308d3, [0x243f6a88])[0, 0]
    assert [int(x) for x in w] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_numpy_generator_equals_the_device_words():
    """the host's scalar draws come from the same words as the device's: device_draws.philox_words against tgp_draw_words' output
    recorded on the GPU (tests/golden/make_device_draws_golden.py); a missing file fails"""
    from tgpose_amd.datasets import device_draws as dd
    path = os.path.join(ROOT, "tests", "golden", "device_draws.npz")
    assert os.path.exists(path), "tests/golden/device_draws.npz is missing: run tests/golden/make_device_draws_golden.py on a GPU"
    fx = np.load(path)
    n = 0
    for j in range(int(fx["n_cases"])):
        seed, site = int(fx["seed.%d" % j]), int(fx["site.%d" % j])
        keys, words = fx["keys.%d" % j], fx["words.%d" % j]
        got = dd.philox_words(seed, keys, site, np.arange(words.shape[1]))
        assert got.dtype == np.uint32 and np.array_equal(got, words), (j, seed, site)
        n += words.size
    assert n >= 3000
    # the transforms of the recorded device buffers: float32 / float64 uniforms from the same words, bit for bit
    seed, keys = int(fx["fill.seed"]), fx["fill.keys"]
    N = fx["fill.defor"].shape[1]
    w = dd.philox_words(seed, keys, 4, np.arange(N))
    assert np.array_equal(dd.uniform_f32(w[..., :3]), fx["fill.defor"])
    w = dd.philox_words(seed, keys, 6, np.arange(N))
    assert np.array_equal(dd.uniform_f64(w[..., 0], w[..., 1]), fx["fill.drop_u"])
    # and a permutation's prefix: the device's selection is the NumPy walk under the site's key
    total = int(fx["sel.total"])
    for d, key in enumerate(keys):
        want = dd.perm_at(np.arange(fx["sel.sel"].shape[1]), total, dd.feistel_key(seed, int(key), 2))
        assert np.array_equal(want, fx["sel.sel"][d])


@pytest.mark.parametrize("total", TOTALS)
def test_permutation_walk_is_a_bijection(total):
    from tgpose_amd.datasets import device_draws as dd
    for key in (0, 1, 0x9e3779b9, 0xffffffff):
        p = dd.perm_at(np.arange(total), total, key)
        assert p.min() >= 0 and p.max() < total and np.unique(p).size == total
        assert np.array_equal(dd.perm_pos(p, total, key), np.arange(total))
    h = dd.half_bits_of(total)
    assert (1 << (2 * h)) >= total and (h == 1 or (1 << (2 * (h - 1))) < total)       # the domain is below 4 x total: the walk ends


def test_item_stream_draws_are_keyed():
    """the per-item scalars: a function of (seed, key) alone, in [0, 1) with both 53-bit and 24-bit laws, regions independent of how
    much an earlier region consumed"""
    from tgpose_amd.datasets import device_draws as dd
    a, b = dd.item_streams(7, [11, 12]), dd.item_streams(7, [12, 11, 5])
    assert np.array_equal(a[0].w, b[1].w) and np.array_equal(a[1].w, b[0].w)
    assert not np.array_equal(a[0].w, a[1].w) and not np.array_equal(a[0].w, dd.item_streams(8, [11])[0].w)
    st = a[0]
    x = st.seek(st.PARAMS).rand(3)
    st.seek(st.DZI).rand(5)
    assert np.array_equal(st.seek(st.PARAMS).rand(3), x)
    u = st.seek(0).random_sample((100,))
    assert u.dtype == np.float64 and (0 <= u).all() and (u < 1).all()
    f = st.seek(0).floats32(200)
    assert f.dtype == np.float32 and (0 <= f).all() and (f < 1).all()
    assert dd.uniform_f32(np.uint32(0xffffffff)) == np.float32(1 - 2.0 ** -24) and dd.uniform_f64(0xffffffff, 0xffffffff) == 1 - 2.0 ** -53
    with pytest.raises(ValueError):
        st.seek(250).rand(4)
    lo = st.seek(st.OPERATOR).uniform(0, 1 - np.array([0.3, 0.4, 0.5]))
    assert lo.shape == (3,) and (lo >= 0).all() and (lo < np.array([0.7, 0.6, 0.5])).all()
    assert st.uniform(0.3, 0.6, 3).shape == (3,) and 0 <= st.seek(st.OP_INDEX).randint4() < 4


def test_separable_walk_decides_as_the_full_map_does():
    """source_tables' separability test walks only the distinct row offsets; the decision and the tables are those of the full
    256 x 256 map, on separable walks and on walks that the offsets' noise makes inseparable"""
    from tgpose_amd.datasets.load_data import _separable_walk, AB_BITS
    rng = np.random.RandomState(0)
    seen = {True: 0, False: 0}
    for trial in range(400):
        n = 64
        adelta = np.rint(np.arange(n) * rng.uniform(300, 3000)).astype(np.int64)
        bdelta = rng.randint(-1, 2, n).astype(np.int64) * (trial % 4 == 0)
        X0 = rng.randint(0, 10 ** 6) + rng.randint(-1, 2, n).astype(np.int64) * (trial % 3 == 0) * rng.randint(1, 600)
        Y0 = np.rint(np.arange(n) * rng.uniform(300, 3000)).astype(np.int64) + rng.randint(0, 10 ** 6)
        sx2, sy2 = (X0[:, None] + adelta[None, :]) >> AB_BITS, (Y0[:, None] + bdelta[None, :]) >> AB_BITS
        full = bool((sx2 == sx2[0][None, :]).all() and (sy2 == sy2[:, 0][:, None]).all())
        got = _separable_walk(X0, adelta, Y0, bdelta)
        assert (got is not None) == full, trial
        if full:
            assert np.array_equal(got[0], sx2[0]) and np.array_equal(got[1], sy2[:, 0])
        seen[full] += 1
    assert seen[True] > 50 and seen[False] > 50, seen
