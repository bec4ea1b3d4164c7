"""GPU test that pins the training loader's host draw mode (train_batch, train_clouds, TrainBatches with draws='host') to the commit
before its three modes were given one launch path: tests/golden/train_batch_host.npz holds, per case, the SHA-256, shape and dtype of
every returned tensor, aug_name, and digests of rng's and gen's state after the call, recorded by
tests/golden/make_train_batch_host_golden.py at that commit.  The cases are recomputed with the maker's own ``cases`` and compared for
equality."""
import importlib.util
import json
import os

import pytest
import torch

from tests.util import GOLDEN, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    spec = importlib.util.spec_from_file_location("make_train_batch_host_golden", os.path.join(GOLDEN, "make_train_batch_host_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    fx = golden("train_batch_host.npz")
    return json.loads(json.dumps(maker.cases(int(fx["seed"])))), json.loads(str(fx["digests"]))


@pytest.mark.parametrize("case", ["a", "b", "c", "d.a", "d.b", "e"])
def test_host_path_equals_the_recorded_commit(both, case):
    """every tensor's bytes, shape and dtype, aug_name, and the states rng and gen are left in: equal to the recording.  Item 1 of
    the ten is abandoned (the launches run on a row subset); the recording's seed gives case a accepted crops and cutouts (the
    deferred shuffle after the read-back of M) next to jitter and dropout, case b deformed and undeformed masks, case e a refill"""
    got, want = both
    assert sorted(got) == sorted(want) == ["a", "b", "c", "d.a", "d.b", "e"]
    g, w = got[case], want[case]
    if case == "e":
        assert len(g["batches"]) == len(w["batches"]) == 3
        g, w = dict(g, **{"batch%d" % j: b for j, b in enumerate(g["batches"])}), dict(w, **{"batch%d" % j: b for j, b in enumerate(w["batches"])})
        del g["batches"], w["batches"]
    flat = lambda r: {(k, k2): v2 for k, v in r.items() for k2, v2 in (v.items() if isinstance(v, dict) else [("", v)])}
    g, w = flat(g), flat(w)
    assert sorted(g) == sorted(w)
    bad = [k for k in w if g[k] != w[k]]
    assert not bad, [(k, g[k], w[k]) for k in bad[:6]]
