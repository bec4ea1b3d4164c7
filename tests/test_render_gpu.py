"""The depth renderer on the GPU (csrc/render.hip, ops.render_depth) against the numpy restatement of its contract
(tests/render_ref.py): z bits, face, mask, depth, visible, bbox and dropped are equal, every pixel compared; then the surfaces above
it -- datasets.synthetic into both loaders, tools.render.renderer."""
import numpy as np
import pytest
import torch

from tests import render_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("z", "face", "mask", "depth", "visible", "bbox", "dropped")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


_MESHSETS = {}


def _args(c):
    from tgpose_amd import ops
    key = id(c["meshes"])
    if key not in _MESHSETS:
        _MESHSETS[key] = (c["meshes"], ops.MeshSet(c["meshes"], device=DEV))
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to(DEV)
    return (_MESHSETS[key][1],) + tuple(up(c[k]) for k in ("scene_ptr", "inst_mesh", "inst_id", "inst_pose", "camk")) + (c["H"], c["W"])


def _render(c, **kw):
    from tgpose_amd import ops
    kw = {"return_z": True, "return_face": True, **kw}
    return ops.render_depth(*_args(c), near=c["near"], **kw)


def _assert_equal(out, ref):
    for k in KEYS:
        got, want = out[k].cpu().numpy(), ref[k]
        assert got.shape == want.shape and got.dtype == want.dtype, k
        if k == "z":
            got, want = got.view(np.int32), want.view(np.int32)
        bad = got != want
        assert not bad.any(), "%s: %d of %d differ, first at %s: %r != %r" % (k, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


CASES = [("rectangle", s) for s in sorted(rc.RECT_SPLITS)] + [("slanted_plane", 1), ("slanted_plane", 24), ("rules", None), ("cube", None),
                                                              ("tails", None), ("tiny_triangles", None), ("three_scenes", None),
                                                              ("slot_carry", None)]


@pytest.mark.parametrize("name,arg", CASES, ids=["%s-%s" % c if c[1] is not None else c[0] for c in CASES])
def test_kernel_equals_restatement(name, arg):
    """the CPU file's closed-form cases; tile tails and triangles longer than the image at 123 x 157; 20 480 sub-pixel triangles
    in one tile; three scenes of 0, 1 and 7 instances with a camk each and ids out of slot order; two instances whose records share
    the tile's list when it crosses the sweep threshold"""
    c, ref = rc.reference(name, arg)
    out = _render(c)
    _assert_equal(out, ref)
    if name == "tails":
        assert (ref["mask"][0] > 0).mean() > 0.9 and set(np.unique(ref["mask"][0])) >= {3, 17, 200} and (ref["visible"] > 0).all()
    if name == "tiny_triangles":
        assert 100 <= ref["visible"][0] <= 160 and len(np.unique(ref["face"][0])) > 100
        bb = ref["bbox"][0]
        assert bb[2] - bb[0] <= 14 and bb[3] - bb[1] <= 14
    if name == "three_scenes":
        assert c["scene_ptr"].tolist() == [0, 0, 1, 8] and (ref["mask"][0] == 0).all() and np.isinf(ref["z"][0]).all() and (ref["face"][0] == -1).all()
        assert (ref["visible"] > 0).sum() >= 6 and len(np.unique(ref["mask"][2])) >= 6


def test_optional_outputs_and_repeatability():
    """the same call twice gives torch.equal on every output; without z / face the others do not change"""
    c, ref = rc.reference("tails")
    a, b = _render(c), _render(c)
    assert set(a) == set(KEYS)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    lean = _render(c, return_z=False, return_face=False)
    assert set(lean) == {"depth", "mask", "visible", "bbox", "dropped"}
    for k in lean:
        assert torch.equal(lean[k], a[k]), k


def test_graph_capture():
    """captured in a torch.cuda.graph and replayed: the same bytes as the eager call"""
    c, ref = rc.reference("three_scenes")
    eager = _render(c)
    args = _args(c)
    from tgpose_amd import ops
    ops.render_depth(*args, near=c["near"], return_z=True, return_face=True)       # warm the allocator outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.render_depth(*args, near=c["near"], return_z=True, return_face=True)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], eager[k]), k
    _assert_equal(out, ref)


# The loaders are written for the 480 x 640 sensor (get_bbox's window arithmetic), so the two tests through them render at that
# size with the camera's intrinsics; the closure bound is test_render_cpu.test_closure's: 0.5 mm of quantisation along the ray
# plus 0.1 mm for the float error.
def _cube_scene():
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluation.load_data_eval import CAMERA_INTRINSICS
    from tgpose_amd import ops
    ms = ops.MeshSet([shapes.box(1.0), shapes.icosphere(0.5, 2)], device=DEV)
    lab = dict(cat_id=2, fsnet_scale=np.zeros(3, np.float32), mean_shape=np.full(3, 0.2, np.float32), sym_info=np.zeros(4, np.float32),
               model_point=np.zeros((8, 3), np.float32))
    scenes = [[dict(mesh=0, inst_id=7, R=rc.CUBE_R, t=rc.CUBE_T, s=rc.CUBE_S, labels=lab),
               dict(mesh=1, inst_id=3, R=np.eye(3), t=(0.0, 0.0, -1.0), s=0.1, labels=lab)]]               # behind the camera: invisible
    rendered = synthetic.render_scenes(ms, scenes, CAMERA_INTRINSICS, 480, 640)
    return ms, scenes, rendered


def _on_cube(points):
    plane, excess = rc.closure_error(points, rc.CUBE_R, rc.CUBE_T, rc.CUBE_S)
    print("closure: %d points, %.4f mm from a face plane, %.4f mm beyond the half-extent" % (len(points), plane * 1e3, excess * 1e3))
    assert plane <= 0.6e-3 and excess <= 0.6e-3


def test_scene_items_through_train_clouds():
    """the pixel convention against the input-side kernels: every PC point train_clouds returns lies on the posed cube"""
    from tgpose_amd.datasets import load_data as ld, synthetic
    ms, scenes, rendered = _cube_scene()
    assert rendered["visible"].tolist()[1] == 0 and rendered["visible"][0] > 20000 and rendered["dropped"].tolist() == [[320, 0]]
    items = synthetic.scene_items(scenes, rendered)
    assert len(items) == 1
    it = items[0]
    assert it["depth"].dtype == np.uint16 and it["mask"].dtype == np.uint8 and it["inst_id"] == 7 and it["camK"].shape == (3, 3)
    ys, xs = np.nonzero(it["mask"] == 7)
    assert it["bbox"].tolist() == [ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]
    assert np.array_equal(it["rotation"], rc.CUBE_R.astype(np.float32)) and np.allclose(it["translation"], rc.CUBE_T) and it["cat_id"] == 2
    assert np.isclose(it["nocs_scale"], rc.CUBE_S)
    (pc, pcl_in), = ld.train_clouds(items, rng=np.random.RandomState(0), device=DEV)
    assert pc.shape == (2048, 3) and pcl_in.shape == (1024, 3)
    _on_cube(pc.cpu().numpy())
    _on_cube(pcl_in.cpu().numpy())


def test_scene_frame_through_clouds_from_frames():
    """one cloud per visible instance, on the cube"""
    from tgpose_amd.datasets import synthetic
    from tgpose_amd.evaluation import load_data_eval as lde
    ms, scenes, rendered = _cube_scene()
    fr = synthetic.scene_frame(ms, scenes, rendered, 0)
    assert fr["pred_masks"].shape == (480, 640, 1) and fr["pred_masks"].dtype == bool and fr["pred_bboxes"].shape == (1, 4)
    assert fr["pred_class_ids"].tolist() == [3] and fr["pred_scores"].tolist() == [1.0] and fr["pred_inst"].tolist() == [0]
    assert fr["gt_RTs"].shape == (2, 4, 4) and np.allclose(fr["gt_RTs"][0, :3, :3], rc.CUBE_R * rc.CUBE_S) and np.allclose(fr["gt_RTs"][0, :3, 3], rc.CUBE_T)
    assert np.allclose(fr["gt_scales"], 1.0) and fr["gt_class_ids"].tolist() == [3, 3]
    clouds = lde.clouds_from_frames([fr], camK=lde.CAMERA_INTRINSICS, rng=np.random.RandomState(0), device=DEV)
    assert len(clouds) == 1 and clouds[0].shape == (1, 1024, 3)
    _on_cube(clouds[0][0].cpu().numpy())


def test_create_renderer_render_object():
    """the reference's interface: render_object equals ops.render_depth for the same single-instance scene, in the model's units"""
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes
    from tgpose_amd.tools.render import renderer
    ren = renderer.create_renderer(rc.W, rc.H, renderer_type="hip", mode="depth", device=DEV)
    v, f = shapes.lathe(shapes.PROFILES["bowl"], 20)
    ren.add_object(5, {"pts": v * 100.0, "faces": f}, scale=0.001)                 # a model in millimetres, 100 mm across
    R, t = rc.rot("x", 200) @ rot_y(25), np.array([15.0, -10.0, 420.0])
    got = ren.render_object(5, R, t, *rc.CAMK)["depth"]
    assert got.shape == (rc.H, rc.W) and got.dtype == np.float32
    ms = ops.MeshSet([(v * 100.0, f)], device=DEV)
    out = ops.render_depth(ms, *ren.scene(5, R, t, *rc.CAMK), rc.H, rc.W, return_z=True)
    z = out["z"][0].cpu().numpy()
    want = np.where(np.isfinite(z), z / np.float32(0.001), np.float32(0)).astype(np.float32)
    assert np.array_equal(got, want) and (got > 0).sum() == out["visible"][0].item() > 500
    assert 350.0 < got[got > 0].min() and got.max() < 490.0                        # millimetres
    with pytest.raises(ValueError, match="already loaded"):
        ren.add_object(5, (v, f))
    ren.remove_object(5)
    with pytest.raises(KeyError):
        ren.render_object(5, R, t, *rc.CAMK)


def rot_y(deg):
    return rc.rot("y", deg)
