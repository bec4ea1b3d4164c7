"""Times the training augmentation (load_data.train_batch) at B = 32 and B = 256 on synthetic frames.

Recorded per batch size (median over --reps calls after --warmup):
  * device time of the augmentation's launches (tgp_augment and the two tgp_gather_rows of pcl_in / aug_pcl_in), by HIP events
    around each launch on its stream;
  * host draw time: the time spent in the draws (generate_aug_parameters, the torch draws of the base augmentation, the two
    permutations, the operators' draws, pc_sampler's shuffles);
  * the number of device-to-host read-backs per call (the ROI counts, plus M when an item's operator is an applied crop / cutout);
  * the wall time of the whole train_batch call (ROI clouds included).
Writes profiles/augment_time.json.  A figure not taken on an MI355X is marked as not measured there.

    python scripts/augment_time.py [--reps 10] [--warmup 2] [--out profiles/augment_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def items_for(B):
    from tests.util import synth_depth_scene
    from tgpose_amd.datasets.load_data import REAL_INTRINSICS
    out, scene = [], 0
    while len(out) < B:
        fr = synth_depth_scene(200 + scene, 4)
        mask = np.zeros(fr["depth"].shape, np.uint8)
        for q in range(4):
            mask[fr["pred_masks"][:, :, q]] = q + 1
        for j in range(4):
            c = len(out) % 6
            out.append(dict(depth=fr["depth"], mask=mask, inst_id=j + 1, camK=REAL_INTRINSICS, bbox=fr["pred_bboxes"][j],
                            rotation=np.eye(3, dtype=np.float32), translation=np.array([0, 0, 0.8], np.float32),
                            fsnet_scale=np.zeros(3, np.float32), mean_shape=np.full(3, 0.1, np.float32),
                            sym_info=np.array([c in (0, 1, 3), 1, 0, 1], np.float32),
                            model_point=np.random.RandomState(c).rand(1024, 3).astype(np.float32) - 0.5, nocs_scale=0.3, cat_id=float(c)))
        scene += 1
    return out[:B]


class Probe(object):
    """wraps the draw functions and the launches train_batch makes; counts read-backs"""

    def __init__(self):
        from tgpose_amd import ops
        from tgpose_amd.datasets import data_augmentation as da, load_data as ld
        self.host, self.events, self.readbacks = 0.0, [], 0
        self._undo = []

        def timed_host(mod, name):
            fn = getattr(mod, name)

            def w(*a, **kw):
                t0 = time.perf_counter()
                try:
                    return fn(*a, **kw)
                finally:
                    self.host += time.perf_counter() - t0
            setattr(mod, name, w)
            self._undo.append((mod, name, fn))

        def timed_dev(mod, name):
            fn = getattr(mod, name)

            def w(*a, **kw):
                st = torch.cuda.current_stream()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                r = fn(*a, **kw)
                e1.record(st)
                self.events.append((e0, e1))
                return r
            setattr(mod, name, w)
            self._undo.append((mod, name, fn))

        for n in ("generate_aug_parameters", "base_draws", "sampler_perm"):
            timed_host(da, n)
        timed_host(ld, "_selection")
        for cls in (da.PcJitter, da.PcRandomCutout, da.PcRandomCrop, da.PcRandomDropout):
            timed_host(cls, "draw")
        timed_dev(ops, "augment")
        timed_dev(ops, "gather_rows")
        cpu = torch.Tensor.cpu

        def counted(t, *a, **kw):
            if t.is_cuda:
                self.readbacks += 1
            return cpu(t, *a, **kw)
        torch.Tensor.cpu = counted
        self._undo.append((torch.Tensor, "cpu", cpu))

    def close(self):
        for mod, name, fn in reversed(self._undo):
            setattr(mod, name, fn)

    def reset(self):
        self.host, self.events, self.readbacks = 0.0, [], 0


def run(B, reps, warmup):
    from tgpose_amd.datasets.load_data import train_batch
    items = items_for(B)
    rng, gen = np.random.RandomState(0), torch.Generator().manual_seed(0)
    for _ in range(warmup):
        train_batch(items, rng=rng, gen=gen)
    torch.cuda.synchronize()
    probe = Probe()
    rows = []
    try:
        for _ in range(reps):
            probe.reset()
            t0 = time.perf_counter()
            db = train_batch(items, rng=rng, gen=gen)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            dev = sum(e0.elapsed_time(e1) for e0, e1 in probe.events) * 1e3
            rows.append(dict(device_us=dev, host_draw_ms=probe.host * 1e3, readbacks=probe.readbacks, wall_ms=wall * 1e3,
                             launches=len(probe.events), items=int(db["pcl_in"].shape[0]),
                             crop_cutout=sum(int(c[1]) >= 0 for c in db["aug_counts"].cpu().tolist())))
    finally:
        probe.close()
    med = lambda k: float(np.median([r[k] for r in rows]))
    return dict(B=B, items_kept=rows[-1]["items"], launches=rows[-1]["launches"], augment_device_us=med("device_us"),
                host_draw_ms=med("host_draw_ms"), readbacks_per_call=sorted({r["readbacks"] for r in rows}),
                train_batch_wall_ms=med("wall_ms"), accepted_crop_cutout_items=[r["crop_cutout"] for r in rows], reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_time.json"))
    a = ap.parse_args()
    name = torch.cuda.get_device_name(0)
    arch = torch.cuda.get_device_properties(0).gcnArchName
    res = dict(device=name, arch=arch, measured_on_mi355x=arch.startswith("gfx950"), runs=[run(B, a.reps, a.warmup) for B in (32, 256)])
    if not res["measured_on_mi355x"]:
        res["note"] = "not measured on the MI355X"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
