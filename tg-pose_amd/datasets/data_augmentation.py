"""The training loader's point-cloud augmentation (datasets/data_augmentation.py of the reference) on the device.

``PC_BasicAugment`` (:19-63) and the four second-view operators (:66-207) are one kernel here (csrc/augment.hip, ``tgp_augment``):
a workgroup per item, the base augmentation per point in the reference's fp32 rounding, the operator on the item's cloud in LDS.
The kernel draws nothing.  Every random number is drawn on the host, from the generators the reference uses and in its order:
torch for the base augmentation's probabilities, ``ey_up`` / ``ey_down`` and the per-point ``defor`` (and for the jitter's
``normal_``), NumPy for ``generate_aug_parameters``, the operator choice and the operators' own draws, and ``pc_sampler``'s shuffle.

One deviation from the reference: ``PcRandomCrop`` and ``PcRandomCutout`` draw all ``max_try_num + 1`` attempts up front (the
kernel then takes the first valid one), where the reference stops drawing at the first valid attempt.  An item whose crop or
cutout is accepted at attempt k therefore consumed ``max_try_num - k`` attempts more of NumPy's stream than the reference does;
the attempts it used are the first ones drawn, so its own result is the reference's.  Items of the other operators draw exactly
the reference's stream.
"""
import math

import numpy as np
import torch

from .. import _lib, ops
from ..config import FLAGS

OPERATOR_NAMES = ['Jitter', 'RandomCutout', 'RandomCrop', 'RandomDropout']       # load_data.py:158


def pc_sampler(points, num, rng=np.random):
    """:12-16: the first ``num`` rows of one shuffle of the row numbers (NumPy's stream).  A GPU cloud is gathered by tgp_gather_rows;
    a CPU tensor or an array is indexed on the host, as the reference does."""
    idx = sampler_perm(points.shape[0], num, rng)
    if torch.is_tensor(points) and points.is_cuda:
        C = points.shape[1]
        src = torch.nn.functional.pad(points, (0, -C % 4)).view(1, points.shape[0], -1)     # rows of a multiple of 4 floats
        dst = torch.empty(1, idx.shape[0], src.shape[2], device=points.device, dtype=points.dtype)
        return ops.gather_rows(src, torch.from_numpy(idx).to(points.device).view(1, -1), dst)[0, :, :C]
    return points[idx] if not torch.is_tensor(points) else points[torch.from_numpy(idx.astype(np.int64))]


def sampler_perm(n, num, rng=np.random):
    """pc_sampler's rows: np.arange(n) shuffled, the first num (int32)"""
    idx = np.arange(0, n)
    rng.shuffle(idx)
    return idx[:num].astype(np.int32)


def get_rotation(x_, y_, z_):
    """:319-336: R_z R_y R_x of three angles in degrees, in float64, returned as float32"""
    x, y, z = (float(v / 180) * math.pi for v in (x_, y_, z_))
    cx, sx, cy, sy, cz, sz = math.cos(x), math.sin(x), math.cos(y), math.sin(y), math.cos(z), math.sin(z)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.dot(rz, np.dot(ry, rx)).astype(np.float32)


def generate_aug_parameters(rng=np.random, s_x=(0.8, 1.2), s_y=(0.8, 1.2), s_z=(0.8, 1.2), ax=50, ay=50, az=50, a=15):
    """load_data.py:440-451: the box scaling factors, the translation (m) and the rotation of the rt augmentation, from ``rng``
    -> (aug_bb (3,) float32, aug_rt_t (3,) float32, aug_rt_R (3,3) float32)"""
    ex, ey, ez = rng.rand(3)
    ex = ex * (s_x[1] - s_x[0]) + s_x[0]
    ey = ey * (s_y[1] - s_y[0]) + s_y[0]
    ez = ez * (s_z[1] - s_z[0]) + s_z[0]
    ang = [rng.uniform(-a, a) for _ in range(3)]
    Rm = get_rotation(*ang)
    d = [rng.rand() * 2 * lim - lim for lim in (ax, ay, az)]
    return np.array([ex, ey, ez], dtype=np.float32), np.array(d, dtype=np.float32) / 1000.0, Rm


def base_draws(bs, n, device, gen=None, defor_gen=None):
    """PC_BasicAugment's draws in its order: prob_bb, prob_rt, prob_bc (:42-55), ey_up, ey_down (defor_3D_bc_in_batch, drawn whether
    or not bc applies), prob_pc (:58) on ``device`` from ``gen``; then defor_3D_pc's torch.rand(pc.shape), which the reference draws
    on the CPU (``defor_gen``; None: torch's default CPU generator) whether or not pc applies.
    -> (draws (bs, 6) on device, defor (bs, n, 3) CPU float32 uniforms)"""
    r = [torch.rand((bs, 1), device=device, generator=gen) for _ in range(6)]
    defor = torch.rand((bs, n, 3), generator=defor_gen)
    return torch.cat(r, dim=1), defor


def _base_inputs(draws, R, t, s, mean_shape, sym, aug_bb, aug_rt_t, aug_rt_R, cat_id, nocs_scale, model_point, defor):
    f = lambda v: v.float().contiguous()
    return dict(draws=f(draws), R=f(R), t=f(t), s=f(s), mean_shape=f(mean_shape), sym=f(sym), aug_bb=f(aug_bb), aug_rt_t=f(aug_rt_t),
                aug_rt_R=f(aug_rt_R), cat_id=f(cat_id.reshape(-1)), nocs_scale=f(nocs_scale.reshape(-1)), model_point=f(model_point),
                defor=f(defor), pro=(FLAGS.aug_bb_pro, FLAGS.aug_rt_pro, FLAGS.aug_bc_pro, FLAGS.aug_pc_pro), pc_r=FLAGS.aug_pc_r)


class PC_BasicAugment(object):
    """:19-63 on device tensors: one item's db (unbatched tensors, as the reference's __getitem__ passes it), a batch of one.
    The draws are the reference's calls on PC.device (defor on the CPU, as the reference draws it), so after the same seeding this
    is the reference class run on that device.  -> (PC (1,N,3), R (1,3,3), t (1,3), s (1,3))"""

    def __init__(self):
        self.mode = 'train'
        self.last_flags = None        # (1, 4) int32 {bb, rt, bc, pc} of the last call (device)

    def __call__(self, db):
        PC = db['pcl_in'].unsqueeze(0)
        dev = PC.device
        draws, defor = base_draws(1, PC.shape[1], dev)
        u = lambda k: db[k].unsqueeze(0).to(dev)
        base = _base_inputs(draws, u('rotation'), u('translation'), u('fsnet_scale'), u('mean_shape'), u('sym_info'), u('aug_bb'),
                            u('aug_rt_t'), u('aug_rt_R'), u('cat_id'), u('nocs_scale'), u('model_point'), defor.to(dev))
        out = ops.augment(PC.float().contiguous(), base=base)
        self.last_flags = out['flags']
        return out['pc'], out['R'], out['t'], out['s']


class _Operator(object):
    """A second-view operator: ``draw`` takes the reference's draws for one cloud of n points; ``__call__`` applies the operator to
    one GPU cloud (N <= 2048) through the kernel."""
    name = None

    def _skip(self, rng):
        return rng.uniform(0, 1) > self.p

    def draw(self, n, rng=np.random, gen=None):
        raise NotImplementedError

    def __call__(self, points, rng=np.random, gen=None):
        rec = self.draw(points.shape[0], rng, gen)
        pts = points.float().contiguous().view(1, -1, 3)
        out = ops.augment(pts, view=view_inputs([rec], pts.shape[1], points.device, [self]))
        m = int(out['counts'][0, 0].item())
        return out['view'][0, :m]


def _record(kind, n, **kw):
    rec = dict(op=kind, noise=None, drop_ratio=0.0, drop_u=None, boxes=None, n_try=0)
    rec.update(kw)
    return rec


class PcJitter(_Operator):
    """:66-79: out = points + clamp(normal(0, std), -clip, clip); the normal_ draw from torch (``gen``; None: the default CPU one)"""
    name = 'Jitter'

    def __init__(self, std=0.01, clip=0.05, p=1):
        self.std, self.clip, self.p = std, clip, p

    def draw(self, n, rng=np.random, gen=None):
        if rng.uniform() > self.p:
            return _record(_lib.AUG_NONE, n)
        noise = torch.empty(n, 3).normal_(mean=0, std=self.std, generator=gen).clamp_(-self.clip, self.clip)
        return _record(_lib.AUG_JITTER, n, noise=noise)


class PcRandomDropout(_Operator):
    """:82-98: rows whose uniform is <= ratio (= uniform * max_dropout_ratio) become row 0"""
    name = 'RandomDropout'

    def __init__(self, max_dropout_ratio=0.875, p=1):
        assert max_dropout_ratio >= 0 and max_dropout_ratio < 1
        self.max_dropout_ratio, self.p = max_dropout_ratio, p

    def draw(self, n, rng=np.random, gen=None):
        if self._skip(rng):
            return _record(_lib.AUG_NONE, n)
        ratio = rng.random_sample() * self.max_dropout_ratio
        return _record(_lib.AUG_DROPOUT, n, drop_ratio=ratio, drop_u=rng.random_sample((n,)))


class PcRandomCrop(_Operator):
    """:101-160: the points strictly inside the first box whose count c has min_num_points <= c < N (attempts 1..max_try_num; the
    reference draws an 11th and discards it).  All max_try_num + 1 attempts are drawn here up front (module docstring)."""
    name = 'RandomCrop'

    def __init__(self, x_min=0.6, x_max=1.1, ar_min=0.75, ar_max=1.33, p=1, min_num_points=4096, max_try_num=10):
        self.x_min, self.x_max, self.ar_min, self.ar_max = x_min, x_max, ar_min, ar_max
        self.p, self.max_try_num, self.min_num_points = p, max_try_num, min_num_points

    def draw(self, n, rng=np.random, gen=None):
        if self._skip(rng):
            return _record(_lib.AUG_NONE, n)
        boxes = np.zeros((_lib.AUGMENT_MAX_TRY, 6))
        for t in range(self.max_try_num + 1):
            rg = np.zeros(3)
            rg[0] = rng.uniform(self.x_min, self.x_max)
            ar = rng.uniform(self.ar_min, self.ar_max)
            rg[1] = rg[0] * ar
            rg[2] = rg[0] / ar
            lo = rng.uniform(0, 1 - rg)
            boxes[t, :3], boxes[t, 3:] = lo, lo + rg
        return _record(_lib.AUG_CROP, n, boxes=boxes, n_try=self.max_try_num + 1)


class PcRandomCutout(_Operator):
    """:163-207: the points outside the first box that cuts c > 0 points and leaves N - c >= min_num_points (attempts
    1..max_try_num; the reference returns the cloud on drawing an 11th).  All attempts are drawn up front (module docstring)."""
    name = 'RandomCutout'

    def __init__(self, ratio_min=0.3, ratio_max=0.6, p=1, min_num_points=4096, max_try_num=10):
        self.ratio_min, self.ratio_max, self.p = ratio_min, ratio_max, p
        self.min_num_points, self.max_try_num = min_num_points, max_try_num

    def draw(self, n, rng=np.random, gen=None):
        if self._skip(rng):
            return _record(_lib.AUG_NONE, n)
        boxes = np.zeros((_lib.AUGMENT_MAX_TRY, 6))
        for t in range(self.max_try_num + 1):
            cut = rng.uniform(self.ratio_min, self.ratio_max, 3)
            lo = rng.uniform(0, 1 - cut)
            boxes[t, :3], boxes[t, 3:] = lo, lo + cut
        return _record(_lib.AUG_CUTOUT, n, boxes=boxes, n_try=self.max_try_num + 1)


def default_operators():
    """the training dataset's operators (load_data.py:160-163), in OPERATOR_NAMES order"""
    return [PcJitter(std=0.005, clip=0.05, p=0.6), PcRandomCutout(p=0.9, min_num_points=1024), PcRandomCrop(p=0.9, min_num_points=1024),
            PcRandomDropout(p=0.9, max_dropout_ratio=0.5)]


def view_limits(operators):
    """the crop / cutout limits of the kernel's second view, from the operators of those kinds in ``operators`` (the defaults of
    PcRandomCrop / PcRandomCutout without one); refuses a max_try_num the kernel's attempt table cannot hold"""
    for o in operators:
        if isinstance(o, (PcRandomCrop, PcRandomCutout)) and not 0 <= o.max_try_num < _lib.AUGMENT_MAX_TRY:
            raise ValueError("max_try_num must be in [0, %d)" % _lib.AUGMENT_MAX_TRY)
    crop = next((o for o in operators if isinstance(o, PcRandomCrop)), PcRandomCrop())
    cut = next((o for o in operators if isinstance(o, PcRandomCutout)), PcRandomCutout())
    return dict(crop_max_try=crop.max_try_num, cutout_max_try=cut.max_try_num, crop_min_points=crop.min_num_points,
                cutout_min_points=cut.min_num_points)


def view_arrays(records, n):
    """a batch of draw records (one per item, clouds of n points) as the host arrays of the kernel's second-view inputs: op int32,
    noise float32, drop_ratio, drop_u and boxes float64"""
    B = len(records)
    out = dict(op=np.array([r['op'] for r in records], dtype=np.int32), noise=np.zeros((B, n, 3), np.float32),
               drop_ratio=np.array([r['drop_ratio'] for r in records], dtype=np.float64), drop_u=np.zeros((B, n)),
               boxes=np.zeros((B, _lib.AUGMENT_MAX_TRY, 6)))
    for i, r in enumerate(records):
        for k in ('noise', 'drop_u', 'boxes'):
            if r[k] is not None:
                out[k][i] = r[k].numpy() if torch.is_tensor(r[k]) else r[k]
    return out


def view_inputs(records, n, device, operators):
    """The kernel's second-view inputs for a batch of draw records (one per item, clouds of n points).  The crop / cutout limits
    come from the operators of those kinds in ``operators``."""
    limits = view_limits(operators)
    return dict({k: torch.from_numpy(v).to(device) for k, v in view_arrays(records, n).items()}, **limits)


def defor_2D(roi_mask, rand_r=2, rand_pro=0.3, rng=np.random, draws="host", seed=None, key=0):
    """The reference's mask deformation (data_augmentation.py:319-342) on a GPU (S,S) or (1,S,S) 0/1 float32 mask, S in {64, 128,
    256} -> the deformed (S,S) mask (a new tensor).  Draws as the reference: rng.rand(), then, when it is not > rand_pro and the
    band is not empty, rng.choice(l, l // 2, replace=False).  rand_r is inert, as in the reference (it reaches cv2.erode / dilate
    as their dst: one iteration).  Runs the training loader's kernels with the mask as a frame, identity source tables and unit
    depth (tgp_roi_band, tgp_roi_cloud_defor without the cut) and scatters the records back; one read-back (the band size).
    draws='device': rand() from (seed, key)'s host stream and the choice drawn on the device from the band size it never reads back
    (tgp_draw_band_subset; the reference's distributions, not its stream; rng is not consumed); no read-back at all -- the mask's
    values are then not checked to be 0 / 1 (a value other than 1 counts as 0)."""
    from .load_data import defor_draws
    if draws not in ("host", "device"):
        raise ValueError("draws must be 'host' or 'device'")
    if draws == "device" and seed is None:
        raise ValueError("draws='device' needs a seed")
    if not (torch.is_tensor(roi_mask) and roi_mask.is_cuda and roi_mask.dtype == torch.float32):
        raise TypeError("defor_2D: roi_mask must be a float32 GPU tensor")
    S = roi_mask.shape[-1]
    if not (roi_mask.dim() in (2, 3) and roi_mask.shape[-2] == S and roi_mask.numel() == S * S and S in (64, 128, 256)):
        raise ValueError("defor_2D: roi_mask must be (S,S) or (1,S,S) with S in {64, 128, 256}")
    m = roi_mask.reshape(S, S)
    if draws == "host" and not bool(((m == 0) | (m == 1)).all()):
        raise ValueError("defor_2D: roi_mask must hold only 0 and 1")
    dev = m.device
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32, device=dev)
    mask8 = m.to(torch.uint8).contiguous().reshape(-1)
    depth = torch.ones(1, S, S, dtype=torch.int16, device=dev)
    tabs = torch.arange(S, dtype=torch.int32, device=dev).repeat(1, 2, 1).contiguous()
    args = (depth, mask8, torch.zeros(1, dtype=torch.int64, device=dev), i32([1]), i32([0]), None)
    cap = S * S
    if draws == "device":
        from . import device_draws as dd
        st = dd.item_streams(seed, [int(key) & (2 ** 64 - 1)])[0]
        if st.seek(st.DEFOR).rand() > rand_pro:              # the host's scalar decides alone; an empty band changes nothing
            return m.clone()
        keys = torch.tensor([int(key) & (2 ** 64 - 1)], dtype=torch.uint64).view(torch.int64).to(dev)
        band = ops.roi_band(*args, roi_size=S, tables=tabs, mask_val=i32([1]))
        on, bits = ops.draw_band_subset(band, torch.zeros(1, dtype=torch.float64, device=dev), 1.0, keys, seed, validity=False,
                                        drop_words=cap // 32)
        rr = ops.roi_cloud(*args, torch.tensor([[1.0, 1.0, 0.0, 0.0]], device=dev), roi_size=S, tables=tabs, mask_val=i32([1]),
                           cut_frac=-1.0, defor=(on, bits))
        pix = (rr.recs[0] >> 16) & 0xffff
        live = torch.arange(cap, device=dev) < rr.counts[0, 2]
        out = torch.zeros(cap + 1, dtype=torch.float32, device=dev)
        out.scatter_(0, torch.where(live, pix, cap).long(), 1.0)
        return out[:cap].reshape(S, S)
    band = ops.roi_band(*args, roi_size=S, tables=tabs, mask_val=i32([1])).cpu().numpy()
    band[0, :2] = 2                   # the draws of a mask, not of an item: no validity test
    on, bits = defor_draws(band, float(rand_pro), rng)
    if not on[0]:
        return m.clone()
    rr = ops.roi_cloud(*args, torch.tensor([[1.0, 1.0, 0.0, 0.0]], device=dev), roi_size=S, tables=tabs, mask_val=i32([1]),
                       cut_frac=-1.0, defor=(i32(on), i32(bits)))
    cap = S * S
    pix = (rr.recs[0] >> 16) & 0xffff
    live = torch.arange(cap, device=dev) < rr.counts[0, 2]
    out = torch.zeros(cap + 1, dtype=torch.float32, device=dev)
    out.scatter_(0, torch.where(live, pix, cap).long(), 1.0)
    return out[:cap].reshape(S, S)
