"""Records tests/golden/train_batch_host.npz on a GPU: digests of what the training loader's HOST draw mode returns, for
tests/test_train_batch_host_gpu.py (which recomputes the cases with ``cases`` below and compares for equality).  Recorded once, at
the commit before the loader's three modes were given one launch path, so the fixture pins the host mode to that commit: every
returned tensor bit for bit, and how far ``rng`` and ``gen`` were consumed.

The items are tests/test_train_loop_gpu._items(10) (ten 480 x 640 synthetic frames, item 1 abandoned).  Per case and returned tensor:
the SHA-256 of its bytes, its shape and dtype; aug_name; a digest of rng.get_state() and of gen.get_state() after the call.
  a  train_batch, defaults                         b  train_batch, dzi=True, roi_mask_pro=0.5
  c  train_batch, pcl_select='fps'                 d  train_clouds with a's and with b's options
  e  TrainBatches(items, 4, dzi=True, roi_mask_pro=0.5, category_tables=..., prefetch=False): every batch of one epoch (the refill)
with rng = RandomState(s), gen = manual_seed(s) for the first s = 0, 1, 2, ... at which case a keeps an item with an accepted crop
or cutout (the deferred shuffle and the read-back of M) and one with jitter or dropout, and case b deforms some masks and not others.

    python tests/golden/make_train_batch_host_golden.py [output path]
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _tensor(t):
    a = t.detach().cpu().contiguous().numpy()
    return [_sha(a.tobytes()), list(a.shape), str(a.dtype)]


def _generators(rng, gen):
    st = rng.get_state()
    return dict(rng=_sha(st[1].tobytes() + repr(st[2:]).encode()), gen=_sha(gen.get_state().numpy().tobytes()))


def _batch(db):
    out = {k: _tensor(v) for k, v in sorted(db.items()) if torch.is_tensor(v)}
    out["aug_name"] = list(db["aug_name"])
    return out


def cases(s, items=None):
    """-> {case: record} for seed s, records made of lists, dicts, strings and ints only (they go through JSON)"""
    from tests.test_train_loop_gpu import _items
    from tests.util import golden
    from tgpose_amd.datasets.load_data import TrainBatches, train_batch, train_clouds
    items = _items(10) if items is None else items
    fresh = lambda: (np.random.RandomState(s), torch.Generator().manual_seed(s))
    out = {}
    for name, kw in (("a", {}), ("b", dict(dzi=True, roi_mask_pro=0.5)), ("c", dict(pcl_select="fps"))):
        rng, gen = fresh()
        out[name] = _batch(train_batch(items, rng=rng, gen=gen, device=DEV, **kw))
        out[name].update(_generators(rng, gen))
    for name, kw in (("d.a", {}), ("d.b", dict(dzi=True, roi_mask_pro=0.5))):
        rng, gen = fresh()
        got = train_clouds(items, rng=rng, device=DEV, **kw)
        out[name] = dict(clouds=[None if c is None else [_tensor(c[0]), _tensor(c[1])] for c in got], **_generators(rng, gen))
    gc = golden("category_clouds.npz")
    rng, gen = fresh()
    src = TrainBatches(items, 4, rng=rng, gen=gen, device=DEV, prefetch=False, dzi=True, roi_mask_pro=0.5,
                       category_tables=(gc["points_category"], gc["pdh1_category"], gc["pdh2_category"]))
    out["e"] = dict(batches=[_batch(db) for db in src], **_generators(rng, gen))
    return out


def _suits(s, items):
    """the conditions on the seed: what case a and case b must exercise"""
    from tgpose_amd.datasets import load_data as ld
    rng, gen = np.random.RandomState(s), torch.Generator().manual_seed(s)
    db = ld.train_batch(items, rng=rng, gen=gen, device=DEV)
    accepted = (db["aug_counts"][:, 1] >= 0).cpu().tolist()
    deferred = any(n in ("RandomCrop", "RandomCutout") and ok for n, ok in zip(db["aug_name"], accepted))
    plain = any(n in ("Jitter", "RandomDropout") for n in db["aug_name"])
    seen, real = [], ld.defor_draws

    def recorded(*a, **kw):
        on, bits = real(*a, **kw)
        seen.append(on)
        return on, bits
    ld.defor_draws = recorded
    try:
        ld.train_batch(items, rng=np.random.RandomState(s), gen=torch.Generator().manual_seed(s), device=DEV, dzi=True, roi_mask_pro=0.5)
    finally:
        ld.defor_draws = real
    on = np.concatenate(seen)
    return deferred and plain and len(db["item_index"]) < len(items) and 0 < on.sum() < on.size, list(db["aug_name"])


def main(path):
    from tests.test_train_loop_gpu import _items
    items = _items(10)
    for s in range(64):
        ok, names = _suits(s, items)
        if ok:
            break
    else:
        raise SystemExit("no seed below 64 meets the conditions")
    first, second = cases(s, items), cases(s)
    assert first == second, "two runs disagree: " + str([k for k in first if first[k] != second[k]])
    np.savez_compressed(path, seed=np.int32(s), digests=np.array(json.dumps(first, sort_keys=True)))
    print("wrote", path, "seed", s, "case a operators", names, "batches in e", len(first["e"]["batches"]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "train_batch_host.npz"))
