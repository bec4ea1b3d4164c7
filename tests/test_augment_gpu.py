"""GPU tests of the training augmentation (csrc/augment.hip, tgp_augment; tgpose_amd.datasets.data_augmentation and
load_data.train_batch) against the reference's own PC_BasicAugment, operators, pc_sampler and training __getitem__
(tests/golden/augment.npz, recorded by tests/golden/make_augment_golden.py), each stage fed the reference's inputs; against an fp64
restatement; and the batch's properties (determinism, independence of the items, the trainer's step on its result)."""
import json

import numpy as np
import pytest
import torch

from tests.test_augment_cpu import bits, make_operator, np_rng, seeded_np, seeded_torch, view_in, view_out, view_sampled
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PC_TOL, LABEL_TOL = 2e-6, 1e-6


@pytest.fixture(scope="module")
def fx():
    return golden("augment.npz")


def base_fp64(inp, draws, defor, pro, pc_r):
    """PC_BasicAugment restated in float64 (data_augmentation.py:19-63 and the *_in_batch functions): one item"""
    d = lambda k: np.asarray(inp[k], dtype=np.float64)
    pc, R, t, s, ms = d("pcl_in"), d("rotation"), d("translation"), d("fsnet_scale"), d("mean_shape")
    mp, e = d("model_point"), d("aug_bb")
    u = np.asarray(draws, dtype=np.float32)
    f32 = lambda v: np.float32(v)
    bb, rt = u[0] < f32(pro[0]), u[1] < f32(pro[1])
    cat = float(inp["cat_id"])
    bc, pcf = u[2] < f32(pro[2]) and cat in (1.0, 5.0), u[5] < f32(pro[3])
    eu = float(u[3]) * float(np.float32(1.2 - 0.8)) + 0.8
    ed = float(u[4]) * float(np.float32(1.2 - 0.8)) + 0.8
    nb = (e + e[[2, 1, 0]]) / 2.0 if float(inp["sym_info"][0]) == 1.0 else e
    if bb:
        pc = ((pc - t) @ R * nb) @ R.T + t
        s = (s + ms) * nb - ms
        mp = mp * nb
    if rt:
        Ra, at = d("aug_rt_R"), d("aug_rt_t")
        pc = (pc + at) @ Ra.T
        R, t = Ra @ R, Ra @ (t + at)
    if bc:
        sy = (s + ms)[1]
        r = (pc - t) @ R
        k = (r[:, 1] + sy / 2) / sy * (eu - ed) + ed
        r[:, 0] *= k
        r[:, 2] *= k
        pc = r @ R.T + t
        m = mp.copy()
        km = (m[:, 1] + sy / 2) / sy * (eu - ed) + ed
        m[:, 0] *= km
        m[:, 2] *= km
        s = (m.max(0) - m.min(0)) * float(inp["nocs_scale"]) - ms
    if pcf:
        pc = pc + np.asarray(defor, np.float64) * float(np.float32(pc_r)) * (pc - t)
    return pc, R, t, s, [bb, rt, bc, pcf]


def _dev_base(inp, draws, defor, pro, pc_r):
    from tgpose_amd.datasets import data_augmentation as da
    g = lambda k: torch.as_tensor(np.asarray(inp[k], dtype=np.float32)).unsqueeze(0).to(DEV)
    base = da._base_inputs(torch.as_tensor(np.asarray(draws, np.float32)).view(1, 6).to(DEV), g("rotation"), g("translation"),
                           g("fsnet_scale"), g("mean_shape"), g("sym_info"), g("aug_bb"), g("aug_rt_t"), g("aug_rt_R"), g("cat_id"),
                           g("nocs_scale"), g("model_point"), defor.reshape(1, -1, 3).to(DEV))
    base["pro"], base["pc_r"] = tuple(pro[:4]), pc_r
    return base


def test_base_augmentation_vs_reference(fx):
    """PC_BasicAugment teacher-forced: every flag on and off, sym[0] 0 and 1, bc on a bowl, on a mug and skipped on a camera; the
    cloud within 2e-6 m and R, t, s within 1e-6 of the reference and of the fp64 restatement; every flag off: the input's bits"""
    from tgpose_amd import ops
    from tgpose_amd.datasets.data_augmentation import base_draws
    names = [str(v) for v in fx["base.names"]]
    seen = set()
    for k, name in enumerate(names):
        inp = {kk[len("base.%d.in." % k):]: fx[kk] for kk in fx.files if kk.startswith("base.%d.in." % k)}
        pro = fx["base.%d.pro" % k]
        g = seeded_torch(fx, "base.%d.torch" % k)
        draws, defor = base_draws(1, inp["pcl_in"].shape[0], "cpu", gen=g, defor_gen=g)
        base = _dev_base(inp, fx["base.%d.draws" % k], defor, pro, float(pro[4]))
        pc = torch.as_tensor(inp["pcl_in"]).unsqueeze(0).to(DEV).contiguous()
        out = ops.augment(pc, base=base)
        got = {kk: out[kk][0].cpu().numpy() for kk in ("pc", "R", "t", "s", "flags")}
        assert got["flags"].tolist() == fx["base.%d.flags" % k].tolist(), name
        for kk, tol in (("pc", PC_TOL), ("R", LABEL_TOL), ("t", LABEL_TOL), ("s", LABEL_TOL)):
            assert np.abs(got[kk] - fx["base.%d.out.%s" % (k, kk)]).max() <= tol, (name, kk)
        w = base_fp64(inp, fx["base.%d.draws" % k], defor[0].numpy(), pro, float(pro[4]))
        for kk, want, tol in (("pc", w[0], PC_TOL), ("R", w[1], LABEL_TOL), ("t", w[2], LABEL_TOL), ("s", w[3], LABEL_TOL)):
            assert np.abs(got[kk] - want).max() <= tol, (name, kk, "fp64")
        assert w[4] == [bool(v) for v in got["flags"]]
        if not any(got["flags"]):
            assert np.array_equal(bits(got["pc"]), bits(inp["pcl_in"]))
            assert np.array_equal(bits(got["R"]), bits(inp["rotation"])) and np.array_equal(bits(got["s"]), bits(inp["fsnet_scale"]))
        seen.update((i, bool(v)) for i, v in enumerate(got["flags"]))
    assert seen == {(i, v) for i in range(4) for v in (False, True)}


def test_second_view_bit_identical_to_reference(fx):
    """the four operators teacher-forced on the reference's input clouds: applied and skipped by p, crop / cutout accepted at the
    first and a later attempt, exhausted, a degenerate cloud; aug cloud and M bit for bit, then pc_sampler's rows (tgp_gather_rows)"""
    from tgpose_amd import ops
    from tgpose_amd.datasets import data_augmentation as da
    for k, name in enumerate(str(v) for v in fx["view.names"]):
        op = make_operator(str(fx["view.%d.op" % k]), json.loads(str(fx["view.%d.kw" % k])))
        gen = seeded_torch(fx, "view.%d.torch" % k) if ("view.%d.torch.seed" % k) in fx.files else None
        rec = op.draw(2048, seeded_np(fx, "view.%d.np" % k), gen)
        pts = torch.as_tensor(view_in(fx, k)).view(1, -1, 3).to(DEV)
        out = ops.augment(pts, view=da.view_inputs([rec], 2048, DEV, [op]))
        M, att = (int(v) for v in out["counts"][0].cpu())
        ref = view_out(fx, k)
        assert M == ref.shape[0], name
        got = out["view"][0, :M].cpu().numpy()
        assert np.array_equal(bits(got), bits(ref)), name
        assert not out["view"][0, M:].any()
        if name.endswith("later"):
            assert att >= 1
        if "exhausted" in name or "degenerate" in name:
            assert att == -1 and M == 2048
        got_s = da.pc_sampler(out["view"][0, :M].contiguous(), 1024, np_rng(fx, "view.%d.np_sampler" % k))
        assert np.array_equal(bits(got_s.cpu().numpy()), bits(view_sampled(fx, k))), name


def getitem_items(fx):
    """-> list of (train_batch item, np RandomState at generate_aug_parameters, torch Generator at base_aug, index) of the fixture's
    __getitem__ items"""
    from tests.util import synth_depth_scene
    from tgpose_amd.datasets.load_data import REAL_INTRINSICS
    out = []
    for n in range(int(fx["gi.n_items"])):
        p = "gi.%d." % n
        fr = synth_depth_scene(int(fx[p + "scene"]), int(fx["gi.scene_dets"]))
        mask = np.zeros(fr["depth"].shape, np.uint8)
        for q in range(int(fx["gi.scene_dets"])):
            mask[fr["pred_masks"][:, :, q]] = q + 1
        j = int(fx[p + "det"])
        w = fx[p + "window"]
        item = dict(depth=fr["depth"], mask=mask, inst_id=j + 1, camK=REAL_INTRINSICS, bbox_center=w[:2].copy(), scale=float(w[2]))
        for k in ("rotation", "translation", "fsnet_scale", "mean_shape", "sym_info", "model_point", "nocs_scale", "cat_id"):
            item[k] = fx[p + "in." + k]
        out.append((item, np_rng(fx, p + "np_gap"), seeded_torch(fx, p + "torch_base"), n))
    return out


def test_train_batch_end_to_end_vs_reference_getitem(fx):
    """train_batch on the fixture's frames, one item at a time from the reference's generator states: the operator and every flag
    equal; pcl_in, rotation, translation, fsnet_scale within the bars; aug_pcl_in within the bars where the operator is not an
    applied crop / cutout (whose shuffle is drawn after the up-front attempts); for those, M equal"""
    from tgpose_amd.datasets.load_data import train_batch
    from tgpose_amd.datasets.data_augmentation import OPERATOR_NAMES
    kinds = set()
    for item, rng, gen, n in getitem_items(fx):
        p = "gi.%d." % n
        db = train_batch([item], rng=rng, gen=gen, device=DEV)
        assert db["aug_name"] == [OPERATOR_NAMES[int(fx[p + "op"])]]
        assert db["aug_flags"][0].cpu().tolist() == fx[p + "flags"].tolist()
        for k, tol in (("pcl_in", PC_TOL), ("rotation", LABEL_TOL), ("translation", LABEL_TOL), ("fsnet_scale", LABEL_TOL)):
            assert np.abs(db[k][0].cpu().numpy() - fx[p + "out." + k]).max() <= tol, (n, k)
        crop_cut = db["aug_name"][0] in ("RandomCrop", "RandomCutout") and bool(fx[p + "op_applied"])
        assert int(db["aug_counts"][0, 0]) == int(fx[p + "M"])
        if not crop_cut:
            assert np.abs(db["aug_pcl_in"][0].cpu().numpy() - fx[p + "out.aug_pcl_in"]).max() <= PC_TOL, n
        kinds.add((db["aug_name"][0], crop_cut))
        assert db["model_point"].shape == (1,) + fx[p + "in.model_point"].shape
    assert len(kinds) >= 4


def _batch(fx, n_items, seed):
    from tgpose_amd.datasets.load_data import train_batch
    items = [it for it, _, _, _ in getitem_items(fx)]
    items = [items[i % len(items)] for i in range(n_items)]
    return train_batch(items, rng=np.random.RandomState(seed), gen=torch.Generator().manual_seed(seed), device=DEV)


def test_train_batch_is_deterministic(fx):
    a, b = _batch(fx, 12, 5), _batch(fx, 12, 5)
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), k
        else:
            assert v == b[k]


def test_item_in_batch_of_32_equals_item_alone():
    """the kernel's result for an item does not depend on the other items of the launch"""
    from tgpose_amd import ops
    from tgpose_amd.datasets import data_augmentation as da
    B, N, rng = 32, 2048, np.random.RandomState(3)
    g = torch.Generator().manual_seed(3)
    ops_ = da.default_operators()
    ops_[1].min_num_points = ops_[2].min_num_points = 600
    pc = (torch.rand(B, N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 0.8])).to(DEV)
    R = torch.stack([torch.as_tensor(da.get_rotation(*rng.uniform(-90, 90, 3))) for _ in range(B)])
    params = [da.generate_aug_parameters(rng) for _ in range(B)]
    draws, defor = torch.rand(B, 6, generator=g) * 0.5, torch.rand(B, N, 3, generator=g)
    base = da._base_inputs(draws.to(DEV), R.to(DEV), torch.tensor([0.0, 0.0, 0.8]).repeat(B, 1).to(DEV),
                           (torch.rand(B, 3, generator=g) * 0.01).to(DEV), torch.full((B, 3), 0.1).to(DEV),
                           torch.tensor([[float(i % 2), 1, 0, 1] for i in range(B)]).to(DEV),
                           torch.as_tensor(np.stack([p[0] for p in params])).to(DEV), torch.as_tensor(np.stack([p[1] for p in params])).to(DEV),
                           torch.as_tensor(np.stack([p[2] for p in params])).to(DEV), torch.tensor([float(i % 6) for i in range(B)]).to(DEV),
                           torch.full((B,), 0.3).to(DEV), (torch.rand(B, 64, 3, generator=g) - 0.5).to(DEV), defor.to(DEV))
    recs = [ops_[i % 4].draw(N, rng, g) for i in range(B)]
    view = da.view_inputs(recs, N, DEV, ops_)
    full = ops.augment(pc, base=base, view=view)
    assert {r["op"] for r in recs} >= {0, 1, 2, 3}
    for i in range(B):
        one = lambda d: {k: (v[i:i + 1].contiguous() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B else v) for k, v in d.items()}
        alone = ops.augment(pc[i:i + 1].contiguous(), base=one(base), view=one(view))
        for k in ("pc", "R", "t", "s", "flags", "view", "counts"):
            assert torch.equal(alone[k][0], full[k][i]), (i, k)


def test_class_level_basic_augment_matches_fp64(fx):
    """PC_BasicAugment()(db) on device tensors after torch.manual_seed: the same device draws (and defor from torch's CPU
    generator, as the reference draws it) give the fp64 restatement within the bars"""
    from tgpose_amd import FLAGS
    from tgpose_amd.datasets.data_augmentation import PC_BasicAugment, base_draws
    old = {k: getattr(FLAGS, k) for k in ("aug_bb_pro", "aug_rt_pro", "aug_bc_pro", "aug_pc_pro")}
    try:
        for k in range(len(fx["base.names"])):
            inp = {kk[len("base.%d.in." % k):]: fx[kk] for kk in fx.files if kk.startswith("base.%d.in." % k)}
            pro = fx["base.%d.pro" % k]
            FLAGS.aug_bb_pro, FLAGS.aug_rt_pro, FLAGS.aug_bc_pro, FLAGS.aug_pc_pro = (float(v) for v in pro[:4])
            db = {kk: torch.as_tensor(np.asarray(v, np.float32)).to(DEV) for kk, v in inp.items()}
            torch.manual_seed(40 + k)
            PC, R, t, s = PC_BasicAugment()(db)
            torch.manual_seed(40 + k)
            draws, defor = base_draws(1, inp["pcl_in"].shape[0], DEV)
            w = base_fp64(inp, draws[0].cpu().numpy(), defor[0].numpy(), pro, float(FLAGS.aug_pc_r))
            for got, want, tol in ((PC[0], w[0], PC_TOL), (R[0], w[1], LABEL_TOL), (t[0], w[2], LABEL_TOL), (s[0], w[3], LABEL_TOL)):
                assert np.abs(got.cpu().numpy() - want).max() <= tol, k
            assert PC.shape == (1, inp["pcl_in"].shape[0], 3) and R.shape == (1, 3, 3)
    finally:
        for kk, v in old.items():
            setattr(FLAGS, kk, v)


def test_trainer_step_on_train_batch():
    """RT_TDA_Trainer.RL_TDA_train_step on a train_batch result at B = 32, N = 1024: finite losses"""
    from tests.test_gpu_parity import _step_db, _trainer
    from tests.util import synth_depth_scene
    from tgpose_amd.datasets.load_data import REAL_INTRINSICS, train_batch
    B = 32
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
        for k in ("pdh1", "pdh2", "pdh1_category", "pdh2_category", "points_category"):
            it[k] = syn[k][i].numpy()
        items.append(it)
    db = train_batch(items, rng=np.random.RandomState(1), gen=torch.Generator().manual_seed(1), device=DEV)
    assert db["pcl_in"].shape[1] == 1024 and db["aug_pcl_in"].shape[1] == 1024
    tr = _trainer(3)
    _, ld = tr.RL_TDA_train_step(db)
    torch.cuda.synchronize()
    assert ld and all(torch.isfinite(torch.as_tensor(v)).all() for d in ld.values() for v in (d.values() if isinstance(d, dict) else [d]))
