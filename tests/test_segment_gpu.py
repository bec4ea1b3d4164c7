"""tgp_segment_depth (csrc/segment.hip) against its NumPy restatement tests/segment_ref.py on the frames of tests/segment_cases.py.
Every output is integer work or a float64 expression of integers rounded once, so everything is compared with np.array_equal
(NaN-equal for the centroids): labels, info, stats and centers, for both connectivities, min_pixels 1 and 50, max_segments 1, 32 and
255; the small frames in one call against each alone; two calls against each other; max_step 0 and 65535; by_size against argsort."""
import functools

import numpy as np
import pytest
import torch

from tests import plane_cases as pc
from tests import segment_cases as sc
from tests import segment_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAMK = pc.SMALL_CAMK


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


@functools.lru_cache(maxsize=None)
def roots(i, connectivity, max_step=None):
    _, depth, step = sc.cases()[i]
    return sr.components(depth, step if max_step is None else max_step, connectivity)


def dev_frames(depth):
    return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(DEV)


def run(depth, camk=CAMK, **kw):
    """ops.segment_depth of (S,H,W) uint16 host frames -> host arrays"""
    from tgpose_amd import ops
    ck = torch.tensor([camk] * depth.shape[0], dtype=torch.float32, device=DEV)
    seg = ops.segment_depth(dev_frames(depth), camk=ck, **kw)
    assert seg.labels.dtype == torch.uint8 and seg.info.dtype == torch.int32 and seg.stats.dtype == torch.int64 and seg.centers.dtype == torch.float32
    return dict(labels=seg.labels.cpu().numpy(), info=seg.info.cpu().numpy(), stats=seg.stats.cpu().numpy(), centers=seg.centers.cpu().numpy()), seg


def same(got, s, want, what):
    for key in ("info", "stats", "labels"):
        assert got[key][s].shape == want[key].shape and np.array_equal(got[key][s], want[key]), (what, key, got["info"][s], want["info"])
    assert np.array_equal(got["centers"][s], want["centers"], equal_nan=True), (what, "centers")


@pytest.mark.parametrize("max_segments", [1, 32, 255])
@pytest.mark.parametrize("min_pixels", [1, 50])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_every_case_equals_the_restatement(connectivity, min_pixels, max_segments):
    cut_off = 0
    for i, (name, depth, step) in enumerate(sc.cases()):
        want = sr.segment(depth, step, connectivity, min_pixels, max_segments, camk=CAMK, root=roots(i, connectivity))
        got, _ = run(depth[None], max_step=step, connectivity=connectivity, min_pixels=min_pixels, max_segments=max_segments)
        same(got, 0, want, name)
        cut_off += int(want["info"][0])
    assert cut_off > 0 or max_segments > 1                                          # status 1 is among the cases


def test_the_checkerboard_is_cut_off_at_max_segments():
    (name, depth, step), = [c for c in sc.cases() if c[0] == "checkerboard"]
    got, _ = run(depth[None], max_step=step, connectivity=4, min_pixels=1, max_segments=255)
    assert got["info"][0].tolist() == [1, 255, 981, 981]
    assert np.array_equal(got["stats"][0][:, 5], np.arange(255) * 2)                # the first 255 roots in flat order
    got, _ = run(depth[None], max_step=step, connectivity=8, min_pixels=1, max_segments=255)
    assert got["info"][0].tolist() == [0, 1, 1, 981]


def test_the_small_frames_in_one_call_equal_each_alone_and_a_second_call():
    small = sc.small_cases()
    depth = np.stack([d for _, d, _ in small])
    for connectivity in (4, 8):
        kw = dict(max_step=sc.STEP, connectivity=connectivity, min_pixels=1, max_segments=32)
        both, _ = run(depth, **kw)
        again, _ = run(depth, **kw)
        back, _ = run(depth[::-1], **kw)
        for s, (name, d, _) in enumerate(small):
            alone, _ = run(d[None], **kw)
            for key in ("labels", "info", "stats", "centers"):
                assert np.array_equal(both[key][s], alone[key][0], equal_nan=True), (name, key)
                assert np.array_equal(both[key][s], again[key][s], equal_nan=True), (name, key)
                assert np.array_equal(both[key][s], back[key][len(small) - 1 - s], equal_nan=True), (name, key)


@pytest.mark.parametrize("max_step", [0, 65535])
def test_the_ends_of_max_step(max_step):
    names = ("step_columns", "blobs", "many_tiles", "cut2")
    for i, (name, depth, _) in enumerate(sc.cases()):
        if name not in names:
            continue
        for connectivity in (4, 8):
            want = sr.segment(depth, max_step, connectivity, 1, 255, camk=CAMK, root=roots(i, connectivity, max_step))
            got, _ = run(depth[None], max_step=max_step, connectivity=connectivity, min_pixels=1, max_segments=255)
            same(got, 0, want, (name, connectivity))
            if name == "step_columns":          # 0: every column its own; 65535: 1 and 65535 join at last, one component
                assert want["info"][2] == (sc.SW if max_step == 0 else 1)


def test_by_size():
    i = [c[0] for c in sc.cases()].index("blobs")
    small = sc.small_cases()
    depth = np.stack([d for _, d, _ in small])
    got, seg = run(depth, max_step=sc.STEP, connectivity=4, min_pixels=1, max_segments=32)
    order = seg.by_size()
    assert order.device.type == "cuda" and order.shape == (len(small), 32)
    order = order.cpu().numpy()
    for s in range(len(small)):
        assert np.array_equal(order[s], sr.by_size(got["stats"][s])), small[s][0]
    sizes = got["stats"][i][order[i], 0]
    assert (np.diff(sizes) <= 0).all() and (sizes == 0).sum() > 1                   # the empty rows tie, and stay in label order
