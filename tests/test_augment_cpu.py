"""CPU tests of the training augmentation's host side (tgpose_amd.datasets.data_augmentation): the FLAGS defaults, the draw schedule
replayed from the generator states the reference left in tests/golden/augment.npz (tests/golden/make_augment_golden.py), pc_sampler's
rows, and tgp_augment's refusals without a launch."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "augment.npz"))


def np_rng(fx, prefix, cls=np.random.RandomState):
    r = cls()
    pos = fx[prefix + ".pos"]
    r.set_state(("MT19937", fx[prefix + ".keys"], int(pos[0]), int(pos[1]), float(fx[prefix + ".gauss"])))
    return r


def seeded_np(fx, prefix, cls=np.random.RandomState):
    """a state the recorder stored as its seed (it checked that the state was the one seeding leaves)"""
    return cls(int(fx[prefix + ".seed"]))


def seeded_torch(fx, prefix):
    return torch.Generator().manual_seed(int(fx[prefix + ".seed"]))


def view_in(fx, k):
    return fx["view.clouds"][int(fx["view.%d.cloud" % k])]


def view_out(fx, k):
    """the operator's output: stored in full, or as row numbers of its input"""
    key = "view.%d.out" % k
    return fx[key] if key in fx.files else view_in(fx, k)[fx["view.%d.out_rows" % k].astype(np.int64)]


def view_sampled(fx, k):
    """pc_sampler's output, stored as row numbers of the operator's output"""
    return view_out(fx, k)[fx["view.%d.sampled_rows" % k].astype(np.int64)]


class LoggingRandomState(np.random.RandomState):
    """a RandomState that logs what each draw returned (as the recorder's spy does: up to 8 values, else the size)"""

    def __init__(self, *a):
        super().__init__(*a)
        self.log = []

    def _rec(self, v):
        v = np.asarray(v, dtype=np.float64).ravel()
        self.log.append(v.copy() if v.size <= 8 else np.array([v.size], np.float64))

    def uniform(self, *a, **kw):
        r = super().uniform(*a, **kw)
        self._rec(r)
        return r

    def random_sample(self, *a, **kw):
        r = super().random_sample(*a, **kw)
        self._rec(r)
        return r

    def rand(self, *a):
        r = super().rand(*a)
        self._rec(r)
        return r

    def randint(self, *a, **kw):
        r = super().randint(*a, **kw)
        self._rec(r)
        return r

    def flat(self):
        return np.concatenate(self.log) if self.log else np.zeros(0)


def make_operator(name, kw):
    from tgpose_amd.datasets import data_augmentation as da
    return getattr(da, name)(**kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_aug_flags_default_to_reference_config():
    """config/config.py:28-32"""
    from tgpose_amd.config.flags import _DEFAULTS
    want = dict(aug_pc_pro=0.2, aug_pc_r=0.2, aug_rt_pro=0.3, aug_bb_pro=0.3, aug_bc_pro=0.3)
    assert {k: _DEFAULTS[k] for k in want} == want


def test_generate_aug_parameters_replays_reference(fx):
    """load_data.py:440-451 from NumPy's state at the call: aug_bb, aug_rt_t and aug_rt_R bit for bit"""
    from tgpose_amd.datasets.data_augmentation import generate_aug_parameters
    for n in range(int(fx["gi.n_items"])):
        got = generate_aug_parameters(np_rng(fx, "gi.%d.np_gap" % n))
        flat = np.concatenate([np.asarray(v, np.float32).ravel() for v in got])
        assert np.array_equal(bits(flat), bits(fx["gi.%d.gap" % n]))
        assert got[2].dtype == np.float32 and got[2].shape == (3, 3)


def test_get_rotation_is_float64_then_float32():
    from tgpose_amd.datasets.data_augmentation import get_rotation
    R = get_rotation(10.0, -20.0, 30.0)
    assert R.dtype == np.float32
    x, y, z = np.deg2rad([10.0, -20.0, 30.0])
    rx = np.array([[1, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1]])
    assert np.abs(R - (rz @ ry @ rx)).max() < 1e-7


def test_base_draws_replay_reference(fx):
    """PC_BasicAugment's six scalar draws (prob_bb, prob_rt, prob_bc, ey_up, ey_down, prob_pc) from torch's state at the call,
    for the direct cases and the __getitem__ items"""
    from tgpose_amd.datasets.data_augmentation import base_draws
    for k in range(len(fx["base.names"])):
        g = seeded_torch(fx, "base.%d.torch" % k)
        d, defor = base_draws(1, fx["base.%d.in.pcl_in" % k].shape[0], "cpu", gen=g, defor_gen=g)
        assert np.array_equal(bits(d.numpy().ravel()), bits(fx["base.%d.draws" % k]))
        assert defor.shape == (1, fx["base.%d.in.pcl_in" % k].shape[0], 3)
    for n in range(int(fx["gi.n_items"])):
        g = seeded_torch(fx, "gi.%d.torch_base" % n)
        d, _ = base_draws(1, 100, "cpu", gen=g, defor_gen=g)
        assert np.array_equal(bits(d.numpy().ravel()), bits(fx["gi.%d.base_draws" % n]))


def _check_op_draws(op, rng, ref, n_calls):
    """the operator's draws replay the reference's; crop / cutout draw every attempt up front, of which the reference consumed the
    first ones"""
    op.draw(2048, rng, torch.Generator().manual_seed(0))
    got = rng.flat()
    from tgpose_amd.datasets.data_augmentation import PcRandomCrop, PcRandomCutout
    if isinstance(op, (PcRandomCrop, PcRandomCutout)) and len(rng.log) > 1:
        assert len(rng.log) == 1 + (op.max_try_num + 1) * (3 if isinstance(op, PcRandomCrop) else 2)
        assert len(rng.log) >= n_calls
    else:
        assert len(rng.log) == n_calls
    assert np.array_equal(got[:ref.size], ref)


def test_operator_draws_replay_reference(fx):
    """the four operators' NumPy draws, direct cases (skipped by p, applied, crop / cutout accepted at the first and a later attempt,
    exhausted, a degenerate cloud), from NumPy's state at the call"""
    names = [str(v) for v in fx["view.names"]]
    for k, name in enumerate(names):
        op = make_operator(str(fx["view.%d.op" % k]), json.loads(str(fx["view.%d.kw" % k])))
        _check_op_draws(op, seeded_np(fx, "view.%d.np" % k, LoggingRandomState), fx["view.%d.draws" % k], int(fx["view.%d.n_draw_calls" % k]))
    assert {"crop_later", "cutout_later", "crop_exhausted", "cutout_exhausted", "crop_degenerate", "jitter_skipped"} <= set(names)


def test_getitem_operator_draws_replay_reference(fx):
    """the __getitem__ items: the operator's draws from NumPy's state after randint(0, 4) picked it"""
    from tgpose_amd.datasets.data_augmentation import default_operators
    for n in range(int(fx["gi.n_items"])):
        op = default_operators()[int(fx["gi.%d.op" % n])]
        _check_op_draws(op, np_rng(fx, "gi.%d.np_op" % n, LoggingRandomState), fx["gi.%d.op_draws" % n],
                        int(fx["gi.%d.op_draw_calls" % n]))


def test_pc_sampler_rows_replay_reference(fx):
    """pc_sampler (:12-16) on the operators' outputs from NumPy's state at the call (host indexing of an array)"""
    from tgpose_amd.datasets.data_augmentation import pc_sampler
    for k in range(len(fx["view.names"])):
        got = pc_sampler(view_out(fx, k), 1024, np_rng(fx, "view.%d.np_sampler" % k))
        assert np.array_equal(bits(got), bits(view_sampled(fx, k)))


def test_augment_abi_refuses_bad_arguments_without_launching():
    """host-side checks only: every call below returns TGP_EINVAL before anything reaches a device (none is needed here)"""
    from tgpose_amd import _lib
    lib = _lib.lib()
    assert lib.tgp_version() == 9 == _lib.ABI_VERSION
    assert lib.tgp_augment_max_points() == 2048
    fake = 1 << 20                      # never dereferenced: each call fails a host check

    def args(base=True, view=True, **kw):
        a = _lib.AugmentArgs()
        a.B, a.N, a.pc = 2, 2048, fake
        if base:
            for k in ("draws", "R", "t", "s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_R", "cat_id", "nocs_scale", "model_point",
                      "defor", "pc_out", "R_out", "t_out", "s_out"):
                setattr(a, k, fake)
            a.n_model = 64
        if view:
            for k in ("op", "noise", "drop_ratio", "drop_u", "boxes", "view_out", "count_out"):
                setattr(a, k, fake + 4096)
            a.crop_max_try = a.cutout_max_try = 10
            a.crop_min_points = a.cutout_min_points = 1024
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.tgp_augment(None, None) == -1
    assert lib.tgp_augment(ctypes.byref(args(base=False, view=False)), None) == -1          # nothing to do
    bad = [dict(B=0), dict(N=0), dict(pc=None), dict(N=2049), dict(crop_max_try=16), dict(cutout_max_try=-1),
           dict(crop_min_points=-1), dict(n_model=0), dict(view_out=fake), dict(boxes=None), dict(count_out=None), dict(drop_u=None),
           dict(model_point=None), dict(defor=None), dict(R=None), dict(cat_id=None)]
    for kw in bad:
        assert lib.tgp_augment(ctypes.byref(args(**kw)), None) == -1, kw
    assert lib.tgp_augment(ctypes.byref(args(view=False, pc_out=None)), None) == -1          # base alone needs its output


def test_ops_augment_refuses_cpu_and_misshaped_tensors():
    from tgpose_amd import ops
    with pytest.raises(ValueError):
        ops.augment(torch.zeros(1, 8, 3))
    with pytest.raises(TypeError):
        ops.augment(torch.zeros(1, 8, 3), view=dict())
