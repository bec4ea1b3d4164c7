"""Times the training loop (RT_TDA_Trainer.RL_TDA_train over datasets.load_data.TrainBatches) at B = 32 on synthetic frames.

Four runs: prefetch on / off, each with the persistence images off (the items carry pdh1 / pdh2) and on (tgp_persistence computes
them per batch).  A run first trains --warmup batches (the step is captured there), then --steps (--pd-steps with persistence)
batches, timed.  Every step's device time on the trainer's stream is cut by HIP events recorded where the work is enqueued:

    end of step i-1 | idle_before | step call: input copies, subsample draws + upload, gradient zeroing (inputs) | replay |
    idle_after | clip_grad_norm_ (clip) | Ranger (optimizer) | end of step i

  * idle_before: from the end of step i-1's Ranger to the first work step i enqueues (the static-input copies).  Nothing of the
    loop's is enqueued on the stream in between (with prefetch only a wait on the side stream's event): device idle, waiting for
    the host or for the side stream;
  * inputs: the step's static-input copies, the subsample upload and the gradient zeroing, with the host's subsample draws between
    them: small kernels plus the device waiting on the host;
  * idle_after: from the replay's end to the clip's first kernel.  The clip is enqueued only after finish_step has read the step's
    NaN flag, and that read follows prefetch(): device idle while the host prepares the next batch or reads the flag;
  * clip, optimizer: the clip's launches and Ranger's.
Reported per run: batches per second and ms per step (device time from the second timed step's first work to the last one's
end), the median of every part above, and the host time of prefetch() and of the whole loop.
Writes profiles/train_loop_time.json.

    python scripts/train_loop_time.py [--steps 200] [--pd-steps 30] [--warmup 3] [--out profiles/train_loop_time.json]
    python scripts/train_loop_time.py --device-draws [--steps 200]      # draws host / device at B = 32 and 256 (HostSplit, main_draws)
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B = 32


def item_pool(n=64):
    from tests.util import synth_depth_scene
    from tgpose_amd.datasets.load_data import REAL_INTRINSICS
    gc = np.load(os.path.join(ROOT, "tests", "golden", "category_clouds.npz"))
    rng = np.random.RandomState(0)
    out, scene = [], 0
    while len(out) < n:
        fr = synth_depth_scene(300 + scene, 4)
        scene += 1
        mask = np.zeros(fr["depth"].shape, np.uint8)
        for q in range(4):
            mask[fr["pred_masks"][:, :, q]] = q + 1
        for j in range(4):
            c = len(out) % 6
            out.append(dict(depth=fr["depth"], mask=mask, inst_id=j + 1, camK=REAL_INTRINSICS, bbox=fr["pred_bboxes"][j],
                            rotation=np.eye(3, dtype=np.float32), translation=np.array([0, 0, 0.8], np.float32),
                            fsnet_scale=np.zeros(3, np.float32), mean_shape=np.full(3, 0.1, np.float32),
                            sym_info=np.asarray(gc["sym"][c], np.float32), model_point=(rng.rand(64, 3) - 0.5).astype(np.float32),
                            nocs_scale=0.3, cat_id=float(c), pdh1=gc["pdh1_category"][c], pdh2=gc["pdh2_category"][c]))
    return out[:n], (gc["points_category"], gc["pdh1_category"], gc["pdh2_category"])


class Marks(object):
    """HIP events recorded on the current stream at the cut points of every step, and host times"""

    def __init__(self):
        self.ev = {k: [] for k in ("step", "replay", "replay_end", "clip", "optimizer", "end")}
        self.host_prefetch = []

    def mark(self, key):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev[key].append(e)

    def parts(self, steps):
        ev = self.ev
        assert all(len(v) == steps for v in ev.values()), {k: len(v) for k, v in ev.items()}
        med = lambda xs: float(np.median(xs))
        out = dict(idle_before_ms=med([ev["end"][i - 1].elapsed_time(ev["step"][i]) for i in range(1, steps)]))
        for name, a, b in (("inputs_ms", "step", "replay"), ("replay_ms", "replay", "replay_end"), ("idle_after_ms", "replay_end", "clip"),
                           ("clip_ms", "clip", "optimizer"), ("optimizer_ms", "optimizer", "end")):
            out[name] = med([ev[a][i].elapsed_time(ev[b][i]) for i in range(1, steps)])
        span = ev["step"][1].elapsed_time(ev["end"][-1]) / 1e3
        out.update(batches_per_s=(steps - 1) / span, ms_per_step=1e3 * span / (steps - 1),
                   host_prefetch_ms=med(self.host_prefetch) if self.host_prefetch else 0.0)
        return out


class Timed(object):
    """an iterable over a TrainBatches whose iterator times prefetch() on the host"""

    def __init__(self, src, marks):
        self.src, self.marks = src, marks

    def __iter__(self):
        it, marks = iter(self.src), self.marks

        class _It(object):
            def __iter__(self):
                return self

            def __next__(self):
                return next(it)

            def prefetch(self):
                t = time.perf_counter()
                it.prefetch()
                marks.host_prefetch.append(1e3 * (time.perf_counter() - t))
        return _It()


class _Replay(object):
    """stands for the captured graph inside the GraphedStep: events around its replay"""

    def __init__(self, graph, marks):
        self.graph, self.marks = graph, marks

    def replay(self):
        self.marks.mark("replay")
        self.graph.replay()
        self.marks.mark("replay_end")


def instrument(tr, marks):
    """events at the cut points of the loop's captured step, its clip and its Ranger step (the trainer's own objects wrapped)"""
    sig, step = tr._loop
    g = step.graph
    assert g.graph2 is None
    g.graph = _Replay(g.graph, marks)

    def timed_step(db=None, sample_idx=None):
        marks.mark("step")
        return step(db, sample_idx)
    timed_step.graph, timed_step.loss_dict = g, step.loss_dict
    tr._loop = (sig, timed_step)
    opt_step = tr.optimizer.step

    def optimizer_step(*a, **k):
        marks.mark("optimizer")
        return opt_step(*a, **k)
    tr.optimizer.step = optimizer_step
    fin = tr.finish_step

    def finish_step(total=None, **kw):
        ok = fin(total=total, **kw)
        marks.mark("end")
        return ok
    tr.finish_step = finish_step


def run(pool, tables, persistence, prefetch, steps, warmup, model_save):
    from tgpose_amd import FLAGS, seeded_state_dict
    from tgpose_amd.datasets.load_data import TrainBatches
    from tgpose_amd.trainer.RL_TDA import RT_TDA_Trainer
    items = pool if not persistence else [{k: v for k, v in it.items() if k not in ("pdh1", "pdh2")} for it in pool]
    tr = RT_TDA_Trainer(device="cuda:0")
    tr.init_network("RL_TDA")
    tr.init_loss()
    tr.net1.load_state_dict(seeded_state_dict(3), strict=True)
    tr.net2.load_state_dict(seeded_state_dict(4, only_encoder=True), strict=True)
    for net in (tr.net1, tr.net2):
        net.train()
    tr.set_optimizer_scheduler()
    FLAGS.log_every, FLAGS.model_save = 10 ** 9, model_save
    mk = lambda n, seed: TrainBatches([items[i % len(items)] for i in range(n * B)], B, rng=np.random.RandomState(seed),
                                      gen=torch.Generator().manual_seed(seed), prefetch=prefetch, persistence=persistence,
                                      roi_mask_pro=0.5, category_tables=tables, drop_last=True)
    torch.manual_seed(0)
    tr.RL_TDA_train(mk(warmup, 1), 1)
    marks = Marks()
    instrument(tr, marks)
    clip = torch.nn.utils.clip_grad_norm_

    def timed_clip(*a, **k):
        marks.mark("clip")
        return clip(*a, **k)
    torch.nn.utils.clip_grad_norm_ = timed_clip
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.RL_TDA_train(Timed(mk(steps, 2), marks), 1)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        torch.nn.utils.clip_grad_norm_ = clip
    FLAGS.train = 0
    out = dict(persistence=persistence, prefetch=prefetch, B=B, steps=steps)
    out.update(marks.parts(steps))
    out.update(host_ms_per_step=1e3 * wall / steps, wall_s=wall)
    return out


class HostSplit(object):
    """splits the host time of prefetch(): wraps the loader's functions that upload (and, in the host mode, read back) and the ones
    that draw; times the new device launches with HIP events"""
    UPLOAD = {"host": ("_roi_records",), "device": ("_upload_frames", "_stack_labels")}
    DRAWS = {"host": ("defor_draws", "_selection"), "device": ("_item_scalars",)}

    def __init__(self, draws):
        from tgpose_amd import ops
        from tgpose_amd.datasets import data_augmentation as da, load_data as ld
        self.t = dict(upload=0.0, draws=0.0)
        self.rows, self.events, self.kernel_us, self._undo = [], [], [], []
        for name in self.UPLOAD[draws]:
            self._host(ld, name, "upload")
        for name in self.DRAWS[draws]:
            self._host(ld, name, "draws", inside="upload" if name == "defor_draws" else None)
        if draws == "host":
            for n in ("generate_aug_parameters", "base_draws", "sampler_perm"):
                self._host(da, n, "draws")
            for cls in (da.PcJitter, da.PcRandomCutout, da.PcRandomCrop, da.PcRandomDropout):
                self._host(cls, "draw", "draws")
        for n in ("draw_band_subset", "draw_alive", "draw_selection", "draw_fill", "gather_slots"):
            self._dev(ops, n)

    def _host(self, mod, name, bucket, inside=None):
        fn = getattr(mod, name)

        def w(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                dt = time.perf_counter() - t0
                self.t[bucket] += dt
                if inside is not None:                 # called from within another bucket's function: not counted twice
                    self.t[inside] -= dt
        setattr(mod, name, w)
        self._undo.append((mod, name, fn))

    def _dev(self, mod, name):
        fn = getattr(mod, name)

        def w(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            self.events.append((e0, e1))
            return r
        setattr(mod, name, w)
        self._undo.append((mod, name, fn))

    def batch_done(self, prefetch_ms):
        self.rows.append((1e3 * self.t["upload"], 1e3 * self.t["draws"], prefetch_ms))
        self.t = dict(upload=0.0, draws=0.0)
        self.kernel_us.append(self.events)
        self.events = []

    def close(self):
        for mod, name, fn in reversed(self._undo):
            setattr(mod, name, fn)

    def summary(self):
        r = np.asarray(self.rows[1:])
        med = lambda x: float(np.median(x))
        out = dict(host_upload_ms=med(r[:, 0]), host_draws_ms=med(r[:, 1]), host_other_ms=med(r[:, 2] - r[:, 0] - r[:, 1]))
        if any(self.kernel_us):
            out["draw_kernels_us"] = med([1e3 * sum(a.elapsed_time(b) for a, b in ev) for ev in self.kernel_us[1:] if ev])
        return out


def run_draws(pool, tables, draws, batch, steps, warmup, model_save):
    """one run of the device-draws comparison: prefetch on, persistence off, ``draws`` 'host' or 'device' at batch size ``batch``"""
    global B
    from tgpose_amd.datasets import load_data as ld
    keep, B = B, batch
    real = ld.TrainBatches

    def batches(items, batch_size, **kw):
        if draws == "device":
            kw.update(draws="device", spares=2, seed=5)
        return real(items, batch_size, **kw)
    ld.TrainBatches = batches
    split = HostSplit(draws)
    timed_it = Timed.__iter__

    def it_with_split(self):
        it = timed_it(self)
        pre = it.prefetch

        def prefetch():
            n = len(self.marks.host_prefetch)
            pre()
            if len(self.marks.host_prefetch) > n:
                split.batch_done(self.marks.host_prefetch[-1])
        it.prefetch = prefetch
        return it
    Timed.__iter__ = it_with_split
    try:
        out = run(pool, tables, False, True, steps, warmup, model_save)
    finally:
        ld.TrainBatches, Timed.__iter__, B = real, timed_it, keep
        split.close()
    out.update(draws=draws, **split.summary())
    return out


def main_draws(a):
    """profiles/train_loop_device_draws.json: B = 32 and 256, draws host / device alternating (twice each), prefetch on, persistence
    off; the host mode here is the code path the draws='device' mode leaves untouched"""
    pool, tables = item_pool()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for batch, steps in ((32, a.steps), (256, a.steps)):
            for rep in range(2):
                for draws in ("host", "device"):
                    r = run_draws(pool, tables, draws, batch, steps, a.warmup, tmp)
                    r["rep"] = rep
                    print(json.dumps(r), flush=True)
                    rows.append(r)
    out = dict(device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName, runs=rows,
               note="RL_TDA_train over TrainBatches (roi_mask_pro 0.5, category tables, prefetch on, persistence off), graphed step, Ranger; "
                    "host_prefetch_ms = host_upload_ms (host mode: _roi_records, i.e. uploads, source tables, both read-backs and the ROI "
                    "launches; device mode: the frame and label uploads) + host_draws_ms + host_other_ms; draw_kernels_us: device time of "
                    "the tgp_draw_* and tgp_gather_slots launches per batch; runs alternate host / device in one process")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pd-steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loop_time.json"))
    ap.add_argument("--device-draws", action="store_true", help="the host / device draws comparison (train_loop_device_draws.json)")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    if a.device_draws:
        if a.out.endswith("train_loop_time.json"):
            a.out = os.path.join(os.path.dirname(a.out), "train_loop_device_draws.json")
        return main_draws(a)
    pool, tables = item_pool()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for persistence in (False, True):
            for prefetch in (True, False):
                r = run(pool, tables, persistence, prefetch, a.pd_steps if persistence else a.steps, a.warmup, tmp)
                print(json.dumps(r), flush=True)
                rows.append(r)
    out = dict(device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName, B=B, runs=rows,
               note="RL_TDA_train over TrainBatches (roi_mask_pro 0.5, each item's own window, category tables), graphed step, Ranger; synthetic "
                    "depth frames (tests/util.synth_depth_scene)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
