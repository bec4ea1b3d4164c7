"""GPU tests of the training loop: RT_TDA_Trainer.RL_TDA_train / load_old_model_params / init_RL_TDA_model
(trainer/RL_TDA.py) and the loop's batch source datasets.load_data.TrainBatches.

The loop against the reference's own RL_TDA_train (tests/golden/train_loop.npz, tests/golden/make_train_loop_golden.py: one epoch of
four B = 4, N = 256 batches, batch 3 with a NaN translation target, Ranger + flat_and_anneal, the same subsample draws).  Bars: loss
terms 2e-4 relative (test_gpu_parity.py::test_train_step_vs_reference_trainer); parameters 5e-2 of the largest change of that
parameter's samples since the start plus 4 ulp for steps 1-3 (step 4's update, made on weights the LR-5e-4 update left 1.6 % apart
in loss, within 25 % relative L2 over all samples) -- the gradients agree to 3 % relative L2 (GRAD_TOL
there) and Ranger's first steps move each parameter by a multiple of its centralised gradient, so the bar of test_ranger_gpu.py (set
on the update) is applied with the gradients' 3 % and a margin; loss terms after the first full-LR update 3e-2 (two fp32
trajectories from there on); the LR sequence and the skip exactly.  Because the comparison with the reference's own run loosens
after the full-LR update, every update the loop makes is also held, at the Ranger tests' bar, to the fp64 restatement of the
reference's Ranger (tests/test_ranger_gpu.py::Ref64) applied to the device's own pre-step weights, clipped gradients and state."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    return golden("train_loop.npz")


class _Flags(object):
    """sets FLAGS for one test and puts them back"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from tgpose_amd import FLAGS
        self.old = {k: getattr(FLAGS, k) for k in list(self.kw) + ["train"]}
        for k, v in self.kw.items():
            setattr(FLAGS, k, v)

    def __exit__(self, *a):
        from tgpose_amd import FLAGS
        for k, v in self.old.items():
            setattr(FLAGS, k, v)


def _trainer(wseed):
    from tests.test_gpu_parity import _trainer as make
    tr = make(wseed)
    tr.set_optimizer_scheduler()
    return tr


def _fixture_batches(fx, dev=DEV):
    from tests.test_gpu_parity import _step_db
    N = int(fx["n_points"])
    out = []
    for c, s in zip(fx["cat_ids"], fx["data_seeds"]):
        out.append({k: torch.as_tensor(v).to(dev) for k, v in _step_db([int(x) for x in c], N, int(s)).items()})
    out[int(fx["nan_batch"]) - 1]["translation"][1, 0] = float("nan")
    return out


def _logger():
    lines = []
    return types.SimpleNamespace(info=lambda m: lines.append(str(m)), lines=lines)


def _state(tr):
    """every value a continuing run depends on: both nets' state, Ranger's state, the scheduler's counter"""
    out = {"net1." + k: v.detach().clone() for k, v in tr.net1.state_dict().items()}
    out.update({"net2." + k: v.detach().clone() for k, v in tr.net2.state_dict().items()})
    for i, p in enumerate(tr.net1.parameters()):
        for f, v in tr.optimizer.state.get(p, {}).items():
            out["opt.%d.%s" % (i, f)] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    out["sched"] = torch.tensor(tr.scheduler.last_epoch)
    return out


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint8) if t.dtype.is_floating_point else t


def _same(a, b):
    """bit for bit (a NaN equals the same NaN)"""
    assert sorted(a) == sorted(b)
    bad = [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]
    assert not bad, bad[:8]


def _stats(net):
    out = {}
    for k, p in net.named_parameters():
        f = p.detach().reshape(-1)
        pick = torch.linspace(0, f.numel() - 1, 16).long().to(f.device)
        out[k] = torch.cat([f.double().sum().float().view(1), f.double().norm().float().view(1), f[pick]]).cpu().numpy()
    return out


def _pre_step(tr):
    """what finish_step's clip and Ranger start from: the parameters, the gradients, Ranger's state"""
    named = [(n, p) for n, p in tr.net1.named_parameters()]
    return dict(named=named, p=[p.detach().clone() for _, p in named],
                g=[None if p.grad is None else p.grad.detach().clone() for _, p in named],
                st=[{k: (v.clone() if torch.is_tensor(v) else v) for k, v in tr.optimizer.state.get(p, {}).items()} for _, p in named])


def _update_error(tr, pre, lr):
    """the step's update against tests/test_ranger_gpu.py's fp64 restatement of the reference's Ranger, from the device's own
    pre-step parameters, gradients (clipped to norm 5 here, as clip_grad_norm_ does) and state; -> the worst error / bar over
    every parameter, with the bar of test_trainer_graphed_overlap_step_with_ranger (1e-4 + 1e-5 of the update, 4 ulp)"""
    from tests.test_ranger_gpu import Ref64
    grads = [g for g in pre["g"] if g is not None]
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    coef = torch.clamp(5.0 / (norm + 1e-6), max=1.0)
    ref = Ref64(pre["p"], lr)
    for i, st in enumerate(pre["st"]):
        if st:
            ref.st[i] = dict(step=st["step"], m=st["exp_avg"].double(), v=st["exp_avg_sq"].double(), slow=st["slow_buffer"].double())
    ref.step([None if g is None else g * coef for g in pre["g"]])
    worst = 0.0
    for i, (n_, p) in enumerate(pre["named"]):
        if pre["g"][i] is None:
            continue
        d_ref = (ref.p[i] - pre["p"][i].double()).abs().max().item()
        bar = 1.1e-4 * d_ref + 4 * torch.from_numpy(_ulp(ref.p[i].cpu().numpy())).to(p.device)
        worst = max(worst, ((p.detach().double() - ref.p[i]).abs() / bar).max().item())
    return worst


def _run_recorded(tr, batches, epochs=1, graph=True, check=None):
    """RL_TDA_train with every finish / iteration recorded: (lr the step saw, stepped, loss terms, net1 stats after it); with a
    list ``check``, every optimizer step's update is also checked against the fp64 Ranger (_update_error) and its error appended"""
    rec, inside = [], []
    fin, it = tr.finish_step, tr.train_iteration

    def terms(ld):
        t = {k: float(v.detach().reshape(-1)[0]) for k, v in ld.items() if k != "TDA_loss"}
        t.update({"TDA." + k: float(v.detach().reshape(-1)[0]) for k, v in ld["TDA_loss"].items()})
        return t

    def finish_step(total=None):
        lr = tr.optimizer.param_groups[0]["lr"]
        pre = _pre_step(tr) if check is not None else None
        ok = fin(total=total)
        if pre is not None and ok:
            check.append(_update_error(tr, pre, lr))
        if not inside:                      # (train_iteration's own finish_step is recorded there)
            rec.append((lr, ok, terms(tr._loop[1].loss_dict), _stats(tr.net1)))
        return ok

    def train_iteration(db):
        lr = tr.optimizer.param_groups[0]["lr"]
        inside.append(1)
        try:
            total, ld = it(db)
        finally:
            inside.pop()
        rec.append((lr, not tr._skipped, terms(ld), _stats(tr.net1)))
        return total, ld

    tr.finish_step, tr.train_iteration = finish_step, train_iteration
    try:
        tr.RL_TDA_train(batches, epochs, graph=graph)
    finally:
        del tr.finish_step, tr.train_iteration
    return rec


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("graph", [True, False])
def test_loop_matches_reference_loop(fx, tmp_path, graph):
    """RL_TDA_train over the fixture's four batches = the reference's RL_TDA_train step by step: loss terms, parameters, the NaN
    batch skipped (weights, Ranger state and scheduler count unchanged across it), the LR sequence exact, the log line's labels
    and order, the checkpoint's keys"""
    flags = json.loads(str(fx["flags"]))
    with _Flags(model_save=str(tmp_path), **flags):
        tr = _trainer(int(fx["weight_seed"]))
        tr.logger = log = _logger()
        init = _stats(tr.net1)
        batches = _fixture_batches(fx)
        torch.manual_seed(int(fx["forward_seed"]))
        upd = []
        rec = _run_recorded(tr, batches, graph=graph, check=upd)
    assert len(rec) == 4
    # every update the loop made (clip, Ranger at the LR the schedule gave) is the reference's Ranger applied to the device's own
    # pre-step state, at every LR including the full one -- the comparison below with the reference's own run drifts after the
    # LR-5e-4 update, this one does not
    print("updates vs the fp64 Ranger from the device's own state (error / bar):", upd)
    assert len(upd) == 3 and max(upd) <= 1.0, upd
    assert [r[0] for r in rec] == fx["lr"].tolist()                                  # the LR sequence, exactly
    assert [r[1] for r in rec] == fx["stepped"].tolist() == [True, True, False, True]
    names = json.loads(str(fx["loss.names"]))
    # R_DCD weighs every point by how many points chose it as their nearest (calc_dcd): a near-tie decided the other way moves
    # the term by a step of about 1/N -- without the reference's neighbour graphs injected, it gets 1e-2 (the rest 2e-4).  Steps 0
    # and 1 see weights moved by at most the LR of 1e-6; steps 2 and 3 see the update at LR 5e-4, made from gradients that agree
    # to 3 %: two fp32 trajectories from there on, held to 3e-2 (measured: 1.5e-2 at most, on Rot_r_a)
    tol0 = np.array([1e-2 if n == "TDA.R_DCD_cate_pred" else 2e-4 for n in names])
    for s, r in enumerate(rec):
        tol = tol0 if s < 2 else np.maximum(tol0, 3e-2)
        got, want = np.array([r[2][k] for k in names], dtype=np.float64), fx["loss"][s].astype(np.float64)
        rel = np.abs(got - want) / (np.abs(want) + 1e-2)
        print("step %d: worst relative loss-term error %s" % (s, sorted(zip(np.nan_to_num(rel).round(7).tolist(), names))[-3:]))
        ok = np.isnan(want) | (np.abs(got - want) <= tol * np.abs(want) + 2e-6)
        assert ok.all() and (np.isnan(got) == np.isnan(want)).all(), (s, [(n, g_, w_) for n, o, g_, w_ in zip(names, ok, got, want) if not o])
    pnames = json.loads(str(fx["param.names"]))
    assert sorted(pnames) == sorted(init)
    worst, fails, dg, dw = [0.0], [], [], []
    for j, k in enumerate(pnames):
        want = fx["param.%d" % j].astype(np.float64)                                  # (5, 18): start, after every step
        assert np.array_equal(init[k][2:], want[0, 2:]), k                              # the same starting weights
        assert np.allclose(init[k][:2], want[0, :2], rtol=1e-6, atol=1e-6), k          # (sum and norm: float64 on host and device)
        numel = dict(tr.net1.named_parameters())[k].numel()
        # step 3's update is made at weights the LR-5e-4 update left apart (the loss terms differ by up to 1.6 % there): it is held
        # in aggregate below, the steps before it parameter by parameter
        dg.append(rec[3][3][k][2:].astype(np.float64) - rec[2][3][k][2:])
        dw.append(want[4, 2:] - want[3, 2:])
        for s in range(3):
            got = rec[s][3][k].astype(np.float64)
            d = np.abs(want[s + 1, 2:] - want[0, 2:]).max()
            f = 5e-2
            worst[0] = max(worst[0], np.abs(got[2:] - want[s + 1, 2:]).max() / max(d, 1e-30))
            bar = f * d + 4 * _ulp(want[s + 1])
            u = _ulp(np.abs(want[s + 1, 2:]).max())                    # an update below the weights' rounding rounds either way
            bar[0] = f * d * numel + numel * u + 1e-6 * abs(want[s + 1, 0])        # the sum
            bar[1] = f * d * np.sqrt(numel) + np.sqrt(numel) * u + 1e-6 * want[s + 1, 1]     # the norm
            r = np.abs(got - want[s + 1]) / bar
            fails.append((float(r.max()), s, k, int(r.argmax())))
    print("worst parameter sample error / change of that parameter: %.4f" % worst[0])
    fails.sort(reverse=True)
    print("worst (error / bar, step, parameter, statistic):", fails[:6])
    assert fails[0][0] <= 1.0, fails[:6]
    dg, dw = np.concatenate(dg), np.concatenate(dw)
    rel3 = np.linalg.norm(dg - dw) / np.linalg.norm(dw)
    print("step 3: relative L2 of the update over every parameter's samples: %.4f" % rel3)
    assert rel3 <= 0.25, rel3
    for k in pnames:                                                                  # the skipped batch moved nothing
        assert np.array_equal(rec[2][3][k], rec[1][3][k]), k
    assert tr.scheduler.last_epoch == 3
    assert len(tr.optimizer.state) > 100 and all(st["step"] == 3 for st in tr.optimizer.state.values())
    ref_log = json.loads(str(fx["log"]))
    pat = lambda s: re.sub(r"-?\d+\.\d+|nan", "#", s)
    ours = [l for l in log.lines if l.startswith("Stage")]
    assert [pat(l) for l in ours] == [pat(l) for l in ref_log if l.startswith("Stage")]
    keys = json.loads(str(fx["checkpoint"]))
    assert sorted(os.listdir(tmp_path)) == keys["files"]
    ck = torch.load(os.path.join(tmp_path, keys["files"][0]), map_location="cpu")
    assert list(ck) == keys["top"] and ck["epoch"] == keys["epoch"]
    assert list(ck["net1_state_dict"]) == keys["net1"] and list(ck["net2_state_dict"]) == keys["net2"]
    assert list(ck["optimizer_state_dict"]) == keys["optimizer"]
    assert sorted(set(k for st in ck["optimizer_state_dict"]["state"].values() for k in st)) == keys["optimizer.state"]
    assert sorted(ck["scheduler_state_dict"]) == keys["scheduler"]
    FLAGS_train_reset()


def FLAGS_train_reset():
    from tgpose_amd import FLAGS
    FLAGS.train = 0


def _sized_batches(fx, sizes):
    from tests.test_gpu_parity import _step_db
    out = []
    for j, B in enumerate(sizes):
        out.append({k: torch.as_tensor(v).to(DEV) for k, v in _step_db([(j + i) % 6 for i in range(B)], 256, 90 + j).items()})
    return out


def test_graphed_loop_equals_eager_loop_bit_for_bit(fx, tmp_path):
    """graph=True (one capture, replays; the smaller last batch runs eagerly) and graph=False over the same batches and draws:
    both nets, Ranger's state and the scheduler bit-identical"""
    flags = json.loads(str(fx["flags"]))
    batches = _sized_batches(fx, [4, 4, 4, 3])
    got = {}
    with _Flags(model_save=str(tmp_path), **flags):
        for graph in (True, False):
            tr = _trainer(31)
            torch.manual_seed(5)
            tr.RL_TDA_train(batches, 1, graph=graph)
            got[graph] = _state(tr)
            assert tr.scheduler.last_epoch == 4
            del tr
    FLAGS_train_reset()
    _same(got[True], got[False])


@pytest.mark.parametrize("captured", [False, True])
def test_resume_is_exact(fx, tmp_path, captured):
    """2 batches, checkpoint, a fresh trainer loads it (load_old_model_params) and runs 2 more: bit-identical to 4 uninterrupted
    batches.  captured=True: the fresh trainer has already trained a batch of its own before the load -- a captured step, Ranger's
    flat state buffer and descriptor table, a stepped scheduler are all in place and must be replaced by the file's"""
    flags = json.loads(str(fx["flags"]))
    batches = _sized_batches(fx, [4, 4, 4, 4])
    with _Flags(model_save=str(tmp_path), **flags):
        tr = _trainer(41)
        torch.manual_seed(6)
        tr.RL_TDA_train(batches, 1)
        want = _state(tr)
        del tr
        tr = _trainer(41)
        torch.manual_seed(6)
        tr.RL_TDA_train(batches[:2], 1)
        rng = torch.get_rng_state()
        path = os.path.join(str(tmp_path), "rl_tda_model_00.pth")
        assert os.path.exists(path)
        del tr
        tr2 = _trainer(7)                                   # other weights: everything must come from the file
        if captured:
            from tgpose_amd import FLAGS
            FLAGS.model_save = str(tmp_path / "other")          # (its own checkpoint must not replace the one loaded below)
            torch.manual_seed(99)
            tr2.RL_TDA_train(batches[3:], 1)
            FLAGS.model_save = str(tmp_path)
            assert tr2._loop is not None and tr2.optimizer._flat is not None and tr2.scheduler.last_epoch == 1
        assert tr2.load_old_model_params(path, "RL_TDA") == 0
        torch.set_rng_state(rng)
        tr2.RL_TDA_train(batches[2:], 1)
        got = _state(tr2)
    FLAGS_train_reset()
    _same(got, want)


def test_checkpoint_format_and_loading(fx, tmp_path):
    """the file has the reference's keys and only CPU tensors; plain torch.load reads it in a fresh process that never imports
    this package; a checkpoint saved from device tensors loads through load_old_model_params; init_RL_TDA_model renames"""
    from tgpose_amd.trainer.RL_TDA import CHECKPOINT_KEYS
    flags = json.loads(str(fx["flags"]))
    batches = _sized_batches(fx, [4])
    with _Flags(model_save=str(tmp_path), **flags):
        tr = _trainer(51)
        torch.manual_seed(8)
        tr.RL_TDA_train(batches, 1)
        path = os.path.join(str(tmp_path), "rl_tda_model_00.pth")
        ck = torch.load(path)
        assert tuple(ck) == CHECKPOINT_KEYS

        def walk(o):
            if torch.is_tensor(o):
                yield o
            elif isinstance(o, dict):
                for v in o.values():
                    yield from walk(v)
            elif isinstance(o, (list, tuple)):
                for v in o:
                    yield from walk(v)
        ts = list(walk(ck))
        assert ts and all(t.device.type == "cpu" for t in ts)
        assert len(ck["optimizer_state_dict"]["state"]) == len(tr.optimizer.state) > 100
        code = ("import sys, torch; ck = torch.load(sys.argv[1]); assert 'tgpose_amd' not in sys.modules; "
                "print(sorted(ck), len(ck['net1_state_dict']))")
        r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        assert r.returncode == 0, r.stderr[-2000:]
        assert str(sorted(CHECKPOINT_KEYS)) in r.stdout
        # a checkpoint whose tensors were saved on the device (as the reference's are)
        dev_ck = {"epoch": 3, "net1_state_dict": tr.net1.state_dict(), "net2_state_dict": tr.net2.state_dict(),
                  "optimizer_state_dict": tr.optimizer.state_dict(), "scheduler_state_dict": tr.scheduler.state_dict()}
        assert next(iter(dev_ck["net1_state_dict"].values())).is_cuda
        dpath = os.path.join(str(tmp_path), "device.pth")
        torch.save(dev_ck, dpath)
        want = _state(tr)
        tr2 = _trainer(52)
        assert tr2.load_old_model_params(dpath, "RL_TDA") == 3
        _same(_state(tr2), want)
        # init_RL_TDA_model: an RL-stage net1 names its encoder face_enc
        own = tr2.net1.state_dict()
        rl = {k.replace("face_all", "face_enc"): v + 1 for k, v in own.items() if "face_all" in k and v.dtype.is_floating_point}
        assert rl
        rl["face_enc.ph_pred.weight"] = torch.zeros(3)
        rpath = os.path.join(str(tmp_path), "rl.pth")
        torch.save({"net1_state_dict": rl}, rpath)
        before = {k: v.clone() for k, v in own.items()}
        done = tr2.init_RL_TDA_model(rpath)
        after = tr2.net1.state_dict()
        assert sorted(done) == sorted(k.replace("face_enc", "face_all") for k in rl if "ph_pred" not in k)
        for k, v in after.items():
            if k in done:
                assert torch.equal(v, before[k] + 1), k
            else:
                assert torch.equal(v, before[k]), k
    FLAGS_train_reset()


# ------------------------------------------------------------------------------------------------------------ TrainBatches
def _items(n=10):
    """train_batch items from synthetic depth frames (as tests/test_augment_gpu.py builds them); item 1 names an instance its frame
    does not have, so the reference's __getitem__ abandons it"""
    from tests.test_gpu_parity import _step_db
    from tests.util import synth_depth_scene
    from tgpose_amd.datasets.load_data import REAL_INTRINSICS
    cats = [i % 6 for i in range(n)]
    syn = _step_db(cats, 16, 12)
    items = []
    for i in range(n):
        fr = synth_depth_scene(70 + i // 4, 4)
        mask = np.zeros(fr["depth"].shape, np.uint8)
        for q in range(4):
            mask[fr["pred_masks"][:, :, q]] = q + 1
        it = dict(depth=fr["depth"], mask=mask, inst_id=(9 if i == 1 else i % 4 + 1), camK=REAL_INTRINSICS, bbox=fr["pred_bboxes"][i % 4])
        it.update(rotation=syn["rotation"][i].numpy(), translation=syn["translation"][i].numpy(), fsnet_scale=syn["fsnet_scale"][i].numpy(),
                  mean_shape=np.array([0.1, 0.1, 0.1], np.float32), sym_info=syn["sym_info"][i].numpy(),
                  model_point=np.random.RandomState(i).rand(64, 3).astype(np.float32) - 0.5, nocs_scale=0.3, cat_id=float(cats[i]),
                  pdh1=syn["pdh1"][i].numpy(), pdh2=syn["pdh2"][i].numpy())
        items.append(it)
    return items


def _source(prefetch, items):
    from tgpose_amd.datasets.load_data import TrainBatches
    gc = golden("category_clouds.npz")
    return TrainBatches(items, 4, rng=np.random.RandomState(3), gen=torch.Generator().manual_seed(3), device=DEV, prefetch=prefetch,
                        dzi=True, roi_mask_pro=0.5, category_tables=(gc["points_category"], gc["pdh1_category"], gc["pdh2_category"]))


def test_prefetch_is_transparent(fx, tmp_path):
    """TrainBatches with prefetch = without it, bit for bit: every tensor of every batch (with DZI, roi_mask_pro 0.5, crop or
    cutout items, an abandoned item refilled from the next index) and the weights after a short graphed loop over them"""
    items = _items()
    got = {}
    for prefetch in (True, False):
        src = _source(prefetch, items)
        it = iter(src)
        seq = []
        for db in it:
            seq.append(db)
            it.prefetch()
        got[prefetch] = seq
    a, b = got[True], got[False]
    assert [len(x["item_index"]) for x in a] == [4, 4, 2] and len(a) == len(b) == len(_source(False, items))
    names = [n for x in a for n in x["aug_name"]]
    assert {"RandomCrop", "RandomCutout"} & set(names), names
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y) and x["aug_name"] == y["aug_name"]
        for k, v in x.items():
            if torch.is_tensor(v):
                assert torch.equal(v, y[k]), k
    # the abandoned item (index 1) is replaced by item 2, so its batch keeps four rows
    idx = [x["item_index"].tolist() for x in a]
    order = [i for x in idx for i in x]
    assert 1 not in order
    gc = golden("category_clouds.npz")
    for x in a:
        cid = x["cat_id"].reshape(-1).long().cpu()
        assert torch.equal(x["points_category"].cpu(), torch.from_numpy(gc["points_category"])[cid])
    # the loop over both sources
    flags = json.loads(str(fx["flags"]))
    st = {}
    with _Flags(model_save=str(tmp_path), **flags):
        for prefetch in (False, True):
            tr = _trainer(61)
            torch.manual_seed(9)
            tr.RL_TDA_train(_source(prefetch, items), 2)
            st[prefetch] = _state(tr)
            del tr
    FLAGS_train_reset()
    _same(st[True], st[False])


def test_abandoned_item_is_refilled_from_the_next_index(fx):
    """a batch whose item 1 is abandoned gets item 2 in its place: four rows, item_index [0, 2, 2, 3]"""
    from tgpose_amd.datasets.load_data import TrainBatches
    items = _items(4)
    src = TrainBatches(items, 4, rng=np.random.RandomState(4), gen=torch.Generator().manual_seed(4), device=DEV, prefetch=False,
                       shuffle=False)
    db = next(iter(src))
    assert db["item_index"].tolist() == [0, 2, 2, 3]
    assert db["pcl_in"].shape == (4, 1024, 3) and len(db["aug_name"]) == 4
    assert torch.equal(db["cat_id"].cpu(), torch.tensor([0.0, 2.0, 2.0, 3.0]))


def test_persistence_images_match_category_priors(fx):
    """ops.persistence_images of the reference's six obj_model clouds = its stored pdh1 / pdh2 priors (which are compute_pd's
    output, i.e. gudhi's alpha complex and persim's images) within 1e-6"""
    from tgpose_amd import ops
    gc = golden("category_clouds.npz")
    h1, h2 = ops.persistence_images(torch.from_numpy(gc["points_category"]).to(DEV))
    assert np.abs(h1.cpu().numpy() - gc["pdh1_category"]).max() <= 1e-6
    assert np.abs(h2.cpu().numpy() - gc["pdh2_category"]).max() <= 1e-6
