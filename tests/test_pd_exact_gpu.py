"""csrc/persistence.hip on the device, against exact arithmetic: the clouds of tests/pd_cases.py through ops.alpha_persistence and
ops.persistence_images, refereed by tests/pd_exact.py exactly as tests/test_pd_exact_cpu.py referees the host build, and compared
bit for bit with that host build.  Every status case is a documented error path that returns before the triangulation or stops at
a bounded capacity."""
import numpy as np
import pytest
import torch

from tests import pd_cases, pd_ref
from tests.pd_ref import IMG_ATOL
from tests.test_pd_exact_cpu import ORDER, check_exact_case, check_status_case, plain_results

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ran = {}


def run(name):
    """one cloud alone, once per session: dict status, tets, h1, h2 (rows in use), counts, images (pdh1, pdh2), image status"""
    if name not in _ran:
        from tgpose_amd import ops
        pc = torch.from_numpy(pd_cases.cloud(name).copy()).to(DEV)[None]
        a = {k: v.cpu().numpy() for k, v in ops.alpha_persistence(pc).items() if not k.startswith("_")}
        p1, p2, st = ops.persistence_images(pc, check_status=False)
        c1, c2 = (int(x) for x in a["counts"][0])
        _ran[name] = dict(status=int(a["status"][0]), tets=a["tets"][0, : int(a["ntet"][0])], h1=a["h1"][0, :c1], h2=a["h2"][0, :c2],
                          counts=(c1, c2), images=(p1[0].cpu().numpy(), p2[0].cpu().numpy()), image_status=int(st[0]))
    return _ran[name]


def check_images(r, name):
    """the image launch on the device's own pairs, all of them: the restatement's images of those pairs"""
    assert r["image_status"] == r["status"], name
    w1, w2 = pd_ref.images(r["h1"], r["h2"]) if r["status"] == 0 else (np.zeros(2500, np.float32),) * 2
    for got, want in zip(r["images"], (w1, w2)):
        assert got.shape == (2500,) and np.abs(got - want).max() <= IMG_ATOL, name
        if r["status"]:
            assert not got.any(), name


@pytest.mark.parametrize("name", list(pd_cases.EXACT))
def test_kernel_matches_exact(name):
    r = run(name)
    check_exact_case(name, r["status"], r["tets"], r["h1"], r["h2"])
    check_images(r, name)


@pytest.mark.parametrize("name", list(pd_cases.STATUS))
def test_kernel_status(name):
    r = run(name)
    check_status_case(name, r["status"], len(r["tets"]), r["counts"])
    check_images(r, name)


def test_kernel_equals_host_build(tmp_path_factory):
    """pd_run with 256 lanes on the device and with one lane on the host (the plain build; the sanitizer build belongs to the CPU
    tests alone): the same status, tetrahedra, counts and pair bits"""
    host = plain_results(tmp_path_factory)[0]
    for name in list(pd_cases.EXACT) + list(pd_cases.STATUS):
        r, h = run(name), host[ORDER.index(name)]
        assert (r["status"], r["counts"]) == (h["status"], h["counts"]), name
        for key in ("tets", "h1", "h2"):
            assert r[key].tobytes() == h[key].tobytes(), (name, key)


def test_mixed_batch_is_independent():
    """failing and passing clouds in one batch: each failing cloud has its status, zero counts and zero images, each passing one the
    bits of its stand-alone run"""
    from tgpose_amd import ops
    names = [n for n, _ in pd_cases.MIXED]
    pc = torch.from_numpy(np.stack([pd_cases.cloud(n) for n in names])).to(DEV)
    a = {k: v.cpu().numpy() for k, v in ops.alpha_persistence(pc).items() if not k.startswith("_")}
    p1, p2, st = (x.cpu().numpy() for x in ops.persistence_images(pc, check_status=False))
    assert a["status"].tolist() == [s for _, s in pd_cases.MIXED] and st.tolist() == a["status"].tolist()
    for i, (name, status) in enumerate(pd_cases.MIXED):
        if status:
            assert not a["counts"][i].any() and not p1[i].any() and not p2[i].any(), name
            continue
        r = run(name)
        c1, c2 = (int(x) for x in a["counts"][i])
        assert (c1, c2) == r["counts"] and c1 + c2 > 0, name
        assert a["tets"][i, : int(a["ntet"][i])].tobytes() == r["tets"].tobytes(), name
        assert a["h1"][i, :c1].tobytes() == r["h1"].tobytes() and a["h2"][i, :c2].tobytes() == r["h2"].tobytes(), name
        assert p1[i].tobytes() == r["images"][0].tobytes() and p2[i].tobytes() == r["images"][1].tobytes(), name
