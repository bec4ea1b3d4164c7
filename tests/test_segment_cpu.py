"""Depth segmentation without a GPU: the ABI's two new entry points, the argument checks of the C entry, the wrappers and
pose.Segmenter, and the NumPy restatement of the contract (tests/segment_ref.py) against an independent labelling
(scipy.sparse.csgraph.connected_components on the same edge list) and against what it must find in the tracking tests' frames: after
the plane cut exactly the three rendered objects, each segment on one instance and covering most of it."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import icp_ref
from tests import plane_cases as pc
from tests import render_ref
from tests import segment_cases as sc
from tests import segment_ref as sr

NAMES = ("tgp_segment_depth", "tgp_segment_workspace_bytes")
FIELDS = ["depth", "camk", "S", "H", "W", "max_step", "connectivity", "min_pixels", "max_segments", "labels", "info", "stats", "centers",
          "workspace", "workspace_bytes"]


def test_header_declares_and_library_exports_the_entry_points():
    from tgpose_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(handle, name) is not None
    assert _lib.ABI_VERSION == 9
    assert "tgp_segment_args" in _lib.STRUCTS
    assert [f[0] for f in _lib.SegmentArgs._fields_] == FIELDS
    assert _lib.SIGNATURES["tgp_segment_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    assert _lib.SEG_MAX_SEGMENTS == sr.MAX_SEGMENTS == 255 and _lib.SEG_STAT_COLS == sr.STAT_COLS == 12
    assert sorted(n for n in _lib.CONSTANTS if n.startswith("SEG_")) == ["SEG_MAX_SEGMENTS", "SEG_STAT_COLS"]      # and no draw site


def test_the_c_entry_refuses_bad_arguments_before_any_launch():
    """nothing is launched for a refused call, so this runs without a GPU; the pointers are never followed"""
    from tgpose_amd import _lib
    lib = _lib.lib()
    assert lib.tgp_segment_workspace_bytes(1, 480, 640) >= 2 * 4 * 480 * 640 and lib.tgp_segment_workspace_bytes(1, 480, 640) % 16 == 0
    assert lib.tgp_segment_workspace_bytes(65536, 4, 4) == _lib.EUNSUPPORTED
    for S, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 32768), (1, 4096, 4096)):
        assert lib.tgp_segment_workspace_bytes(S, H, W) == _lib.EINVAL, (S, H, W)
    fake = ctypes.c_void_p(4096)
    good = dict(depth=fake, camk=fake, S=1, H=8, W=8, max_step=10, connectivity=4, min_pixels=50, max_segments=32, labels=fake, info=fake,
                stats=fake, centers=fake, workspace=fake, workspace_bytes=1 << 20)
    bad = [dict(depth=None), dict(labels=None), dict(info=None), dict(stats=None), dict(workspace=None), dict(camk=None), dict(S=0), dict(H=0),
           dict(W=32768), dict(H=4096, W=4096), dict(max_step=-1), dict(max_step=65536), dict(connectivity=6), dict(min_pixels=0),
           dict(max_segments=0), dict(max_segments=256), dict(workspace_bytes=8 * 64)]
    for change in bad:
        a = _lib.SegmentArgs(**dict(good, **change))
        assert lib.tgp_segment_depth(ctypes.byref(a), None) == _lib.EINVAL, change
    a = _lib.SegmentArgs(**dict(good, S=65536, workspace_bytes=1 << 40))
    assert lib.tgp_segment_depth(ctypes.byref(a), None) == _lib.EUNSUPPORTED
    assert lib.tgp_segment_depth(None, None) == _lib.EINVAL


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from tgpose_amd import ops, pose
    from tgpose_amd.evaluation import load_data_eval as lde
    depth = torch.zeros(2, 8, 8, dtype=torch.int16)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.segment_depth(depth)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.segment_depth(np.zeros((2, 8, 8), np.uint16))
    for kw, word in ((dict(max_step=-1), "max_step"), (dict(max_step=65536), "max_step"), (dict(max_step=2.5), "max_step"),
                     (dict(connectivity=6), "connectivity"), (dict(min_pixels=0), "min_pixels"), (dict(max_segments=0), "max_segments"),
                     (dict(max_segments=256), "max_segments")):
        with pytest.raises(ValueError, match=word):
            ops.segment_depth(depth, **kw)
        with pytest.raises(ValueError, match=word):
            pose.Segmenter(**kw)
    s = pose.Segmenter()
    assert (s.max_step, s.connectivity, s.min_pixels, s.max_segments) == (10, 4, 50, 32)
    with pytest.raises(ValueError, match="GPU tensor"):
        s(depth, torch.ones(2, 4))
    p = inspect.signature(ops.segment_depth).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("max_step", 10), ("connectivity", 4), ("min_pixels", 50), ("max_segments", 32), ("camk", None)]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k != "depth")
    assert ops.SEG_STATUS[1] and callable(ops.seg_check_status) and callable(ops.Segments.by_size)
    with pytest.raises(TypeError):
        lde.clouds_from_segments(depth, dict(labels=depth))
    with pytest.raises(ValueError, match="sampler"):
        lde.clouds_from_segments(depth, None, sampler="numpy")
    p = inspect.signature(lde.clouds_from_segments).parameters
    assert [(k, v.default) for k, v in p.items()][3:] == [("img_size", 256), ("n_pts", 1024), ("sampler", "device"), ("seed", 0), ("fps_pool", 4096)]


def test_the_device_windows_are_get_bbox():
    """load_data_eval._segment_windows (torch integer ops, run on the CPU here) against get_bbox / _windows for boxes all over and
    beyond a 480 x 640 frame, the empty slot's (0,0,0,0) among them"""
    from tgpose_amd.evaluation import load_data_eval as lde
    r = np.random.RandomState(2)
    y1, x1 = r.randint(0, 480, 400), r.randint(0, 640, 400)
    boxes = np.stack([y1, x1, np.minimum(y1 + r.randint(1, 480, 400), 480), np.minimum(x1 + r.randint(1, 640, 400), 640)], 1)
    boxes = np.concatenate([boxes, [[0, 0, 0, 0], [0, 0, 480, 640], [479, 639, 480, 640], [0, 0, 1, 1], [100, 5, 140, 45]]]).astype(np.int64)
    for H, W in ((480, 640), (240, 320)):
        want = []
        for b in boxes:
            rmin, rmax, cmin, cmax = lde.get_bbox(b)
            want.append((cmin + cmax, rmin + rmax, min(max(rmax - rmin, cmax - cmin), max(H, W))))
        got = lde._segment_windows(torch.from_numpy(boxes), H, W)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), np.asarray(want))


def test_acquire_has_the_stated_signature():
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    p = inspect.signature(myEvaluater.acquire).parameters
    assert list(p) == ["self", "frame", "class_ids", "camK", "support", "segmenter", "n_pts", "sampler"]
    assert p["support"].default is None and p["segmenter"].default is None and p["n_pts"].default == 1024 and p["sampler"].default is None


def partition(root):
    """a labelling as a set of frozensets of flat indices"""
    flat = root.reshape(-1)
    order = np.argsort(flat, kind="stable")
    order = order[flat[order] >= 0]
    cuts = np.nonzero(np.diff(flat[order]))[0] + 1
    return {frozenset(g.tolist()) for g in np.split(order, cuts)} if len(order) else set()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_restatement_against_an_independent_labelling(connectivity):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    for name, depth, step in sc.cases():
        for max_step in {step, 0, 65535}:
            root = sr.components(depth, max_step, connectivity)
            H, W = depth.shape
            e = sr.edges(depth, max_step, connectivity)
            g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(H * W, H * W))
            _, comp = connected_components(g, directed=False)
            valid = depth.reshape(-1) > 0
            assert np.array_equal(root.reshape(-1) >= 0, valid), name
            assert partition(root) == partition(np.where(valid, comp, -1)), (name, max_step)
            flat = root.reshape(-1)
            for rt in np.unique(flat[valid]):
                assert rt == np.nonzero(flat == rt)[0].min(), (name, rt)           # the root is the component's smallest flat index


def test_the_restatement_on_the_shapes_it_was_built_for():
    by_name = {name: (depth, step) for name, depth, step in sc.cases()}
    d, step = by_name["serpentine"]
    for connectivity in (4, 8):
        out = sr.segment(d, step, connectivity, 1, 32)
        assert out["info"].tolist() == [0, 1, 1, int((d > 0).sum())] and out["stats"][0, 5] == 0
        assert out["stats"][0, 1:5].tolist() == [0, 0, sc.SH, sc.SW] and d[sc.SH - 1, sc.SW - 1] > 0 and d[0, 0] > 0
    d, step = by_name["checkerboard"]
    assert sr.segment(d, step, 4, 1, 32)["info"].tolist() == [1, 32, 981, 981]
    assert sr.segment(d, step, 8, 1, 32)["info"].tolist() == [0, 1, 1, 981]
    d, step = by_name["step_columns"]
    root = sr.components(d, step, 4)
    assert root[0, 0] == root[0, 1] == root[0, 2] != root[0, 3]                     # steps of 10, 10, then 11
    assert len({int(root[0, x]) for x in range(sc.SW - 4, sc.SW)}) == 3            # 1 | 65535 ~ 65525 | 65504
    assert d[0, sc.SW - 4] == 1 and d[0, sc.SW - 3] == 65535 and root[0, sc.SW - 4] != root[0, sc.SW - 3]
    d, step = by_name["combs"]
    assert sr.segment(d, step, 4, 1, 32)["info"][2] == 7                           # the comb and six U shapes
    assert sr.segment(d[:-1], step, 4, 1, 32)["info"][2] == 11 + 2 + 5             # without the last row: eleven teeth, two arms, five U shapes
    d, _ = by_name["many_tiles"]
    assert d.shape[0] > 2 * sc.TILE_H and d.shape[1] > 2 * sc.TILE_W and d.shape[0] % sc.TILE_H and d.shape[1] % sc.TILE_W
    assert sr.segment(by_name["invalid"][0], 10, 4, 1, 32)["info"].tolist() == [0, 0, 0, 0]


def test_the_restatement_finds_the_objects_on_the_table():
    shares = []
    for k in range(pc.FRAMES):
        cut = sc.cut_frame(k)
        scene = icp_ref.table_scene(k, gap=0.0)
        inst = [(i["mesh"], i["inst_id"], render_ref.pose34(i["R"], i["t"], i["s"])) for i in scene]
        ren = render_ref.render_scene(pc.meshes(), inst, pc.CAMK, pc.H, pc.W)
        assert np.array_equal(ren["depth"], pc.rendered(k))
        assert 6391 <= (cut > 0).sum() <= 6833
        for connectivity in (4, 8):
            out = sr.segment(cut, sc.STEP, connectivity, sc.MIN_PIXELS, 32, camk=pc.CAMK)
            assert out["info"][:3].tolist() == [0, 3, 3], (k, connectivity, out["info"])
            seen = set()
            for r in range(3):
                on = ren["mask"][out["labels"] == r + 1]
                ids = np.unique(on)
                assert len(ids) == 1 and ids[0] != 0, (k, r, ids)                 # every pixel of the segment on one instance
                slot = [i[1] for i in inst].index(int(ids[0]))
                assert slot < 3 and slot not in seen                               # an object, not the table, and each one once
                seen.add(slot)
                share = len(on) / float((ren["mask"] == ids[0]).sum())
                y1, x1, y2, x2 = out["stats"][r, 1:5]
                by1, bx1, by2, bx2 = ren["bbox"][slot]
                assert by1 <= y1 and bx1 <= x1 and y2 <= by2 and x2 <= bx2, (k, r)
                assert share >= 0.90, (k, r, share)
                if connectivity == 4:
                    shares.append(share)
        small = sr.segment(cut, 4, 4, 1, 255)
        print("frame %d: %d valid pixels, shares %s; with a 4 mm step %d components" % (
            k, (cut > 0).sum(), " ".join("%.1f %%" % (100 * s) for s in shares[-3:]), small["info"][2]))
        assert small["info"][2] > 30, k
    print("a segment covers %.1f to %.1f %% of its instance's pixels" % (100 * min(shares), 100 * max(shares)))
