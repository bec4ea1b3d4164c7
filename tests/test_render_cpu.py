"""The depth renderer without a GPU: the numpy restatement of its contract (tests/render_ref.py) against closed forms -- there is no
golden fixture, the reference's renderer needs an OpenGL context -- the C ABI's argument checks, and the Python surface."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import render_cases as rc


@pytest.mark.parametrize("split", sorted(rc.RECT_SPLITS))
def test_rectangle_rule(split):
    """corners at pixel (10, 5) - (40.5, 20): exactly columns 10..40 and rows 5..19 whichever diagonal and winding"""
    _, ref = rc.reference("rectangle", split)
    want = np.zeros((rc.H, rc.W), dtype=bool)
    want[5:20, 10:41] = True
    assert want.sum() == 465
    assert np.array_equal(ref["mask"][0] == 1, want)
    z = ref["z"][0]
    assert np.isinf(z[~want]).all() and (ref["face"][0][~want] == -1).all() and (ref["depth"][0][~want] == 0).all()
    assert np.abs(z[want].view(np.int32) - np.float32(1).view(np.int32)).max() <= 4           # within 4 ulp of 1
    assert (ref["depth"][0][want] == 1000).all()
    assert ref["visible"].tolist() == [465] and ref["bbox"].tolist() == [[5, 10, 20, 41]] and ref["dropped"].tolist() == [[0, 0]]


@pytest.mark.parametrize("n", [1, 24])
def test_slanted_plane(n):
    """z against the analytic ray-plane depth: 0.1 mm in float (the interpolation's error; 0.029 mm was measured over the covered
    pixels of a prototype), and the quantised values differ by at most 1 (0.5 mm of rounding on each side of a boundary)"""
    _, ref = rc.reference("slanted_plane", n)
    hit = ref["mask"][0] > 0
    assert 5000 < hit.sum() < 9000 and ref["dropped"].tolist() == [[0, 0]]
    true = rc.plane_depth_analytic()
    err = np.abs(ref["z"][0].astype(np.float64) - true)[hit]
    print("slanted plane n=%d: %d pixels, worst |z - analytic| = %.4f mm" % (n, hit.sum(), err.max() * 1e3))
    assert err.max() <= 1e-4
    q = np.rint(true * 1000.0)
    assert np.abs(ref["depth"][0].astype(np.int64) - q)[hit].max() <= 1


def _shift_or(m):
    out = m.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            s = np.zeros_like(m)
            s[max(dy, 0):m.shape[0] + min(dy, 0), max(dx, 0):m.shape[1] + min(dx, 0)] = \
                m[max(-dy, 0):m.shape[0] + min(-dy, 0), max(-dx, 0):m.shape[1] + min(-dx, 0)]
            out |= s
    return out


def test_no_cracks():
    """the 24 x 24 x 2 tessellation covers what the two triangles cover, up to one pixel at the outline, with no hole inside"""
    coarse = rc.reference("slanted_plane", 1)[1]["mask"][0] > 0
    fine = rc.reference("slanted_plane", 24)[1]["mask"][0] > 0
    eroded, dilated = ~_shift_or(~coarse), _shift_or(coarse)
    assert eroded.sum() > 4000
    assert fine[eroded].all()
    assert not fine[~dilated].any()


def test_closure():
    """render -> the loaders' back-projection -> the inverse pose lands on the cube: 0.5 mm of quantisation along the ray plus
    0.1 mm for the float error of test_slanted_plane"""
    c, ref = rc.reference("cube")
    assert ref["visible"][0] > 1500 and (ref["mask"][0][ref["depth"][0] > 0] == 7).all()
    pts = rc.backproject(ref["depth"][0], rc.CAMK)
    assert len(pts) == ref["visible"][0]
    plane, excess = rc.closure_error(pts, rc.CUBE_R, rc.CUBE_T, rc.CUBE_S)
    print("cube closure: %d points, %.4f mm from a face plane, %.4f mm beyond the half-extent" % (len(pts), plane * 1e3, excess * 1e3))
    assert plane <= 0.6e-3 and excess <= 0.6e-3


def test_rules():
    c, ref = rc.reference("rules")
    empty = lambda s: (ref["mask"][s] == 0).all() and (ref["depth"][s] == 0).all() and np.isinf(ref["z"][s]).all() and (ref["face"][s] == -1).all()
    assert ref["dropped"].tolist() == [[1, 0], [0, 1], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert empty(0) and empty(1) and empty(2)                                 # dropped whole, dropped whole, zero area
    hit = ref["mask"][3] > 0                                                  # coplanar duplicates: the earlier instance, id 9
    assert hit.sum() > 1000 and (ref["mask"][3][hit] == 9).all()
    assert ref["visible"].tolist()[3:5] == [int(hit.sum()), 0] and ref["bbox"][4].tolist() == [0, 0, 0, 0]
    hit = ref["mask"][4] > 0                                                  # duplicate faces: the lowest index
    assert hit.sum() > 1000 and (ref["face"][4][hit] == 0).all()
    assert np.array_equal(hit, ref["mask"][3] > 0)
    hit = ref["mask"][5] > 0                                                  # 70 m: a surface, no uint16 millimetres
    assert hit.sum() > 1000 and (ref["depth"][5] == 0).all() and np.allclose(ref["z"][5][hit], 70.0, rtol=1e-5)


def test_slot_carry():
    """the case whose record list crosses the sweep threshold with both slots' records in it (the builder asserts the counts): the
    restatement gives the closed form -- the 14 x 14 block at (1, 1) at 1000 mm, its columns alternating between the two instances"""
    c, ref = rc.reference("slot_carry")
    want = np.zeros((32, 32), dtype=np.uint8)
    want[1:15, 1:15] = np.where(np.arange(14) % 2 == 0, rc.CARRY_IDS[0], rc.CARRY_IDS[1])[None, :]
    assert np.array_equal(ref["mask"][0], want) and np.array_equal(ref["depth"][0], np.where(want > 0, 1000, 0))
    k = (np.arange(32)[:, None] - 1) * 14 + (np.arange(32)[None, :] - 1)                      # the face at a pixel of the block: 0 .. 195
    assert np.array_equal(ref["face"][0], np.where(want > 0, k, -1))
    assert ref["visible"].tolist() == [98, 98] and ref["bbox"].tolist() == [[1, 1, 15, 14], [1, 2, 15, 15]] and ref["dropped"].tolist() == [[0, 0]]
    assert int((ref["mask"][0] > 0).sum()) == int(ref["visible"].sum())


def test_render_abi():
    """the caps, and argument errors launch nothing (no GPU is touched); tests/test_abi_cpu.py holds the symbols and tgp_render_args
    against the header"""
    from tgpose_amd import _lib, ops
    lib = _lib.lib()
    assert lib.tgp_version() == 9 and _lib.ABI_VERSION == 9
    assert lib.tgp_render_max_faces() == 1 << 24 and lib.tgp_render_max_instances() == 255
    assert ops.render_max_faces() == 1 << 24 and ops.render_max_instances() == 255
    assert lib.tgp_render_workspace_bytes(3, 100, 200) >= 3 * (100 * 16 + 200 * 8 + 16)
    assert lib.tgp_render_workspace_bytes(0, 1, 1) > 0 and lib.tgp_render_workspace_bytes(-1, 1, 1) == -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(verts=p, faces=p, vptr=p, fptr=p, M=1, n_verts=3, n_faces=1, max_verts=3, max_faces=1, scene_ptr=p, inst_mesh=p, inst_id=p,
              inst_pose=p, camk=p, S=1, I=1, max_scene_inst=1, H=4, W=4, near=0.01, workspace=p, depth=p, mask=p, z=None, face=None,
              visible=p, bbox=p, dropped=p)
    assert set(ok) == {f[0] for f in _lib.RenderArgs._fields_}
    call = lambda **kw: lib.tgp_render_depth(ctypes.byref(_lib.RenderArgs(**{**ok, **kw})), None)
    assert lib.tgp_render_depth(None, None) == -1
    for k in ("verts", "faces", "vptr", "fptr", "scene_ptr", "inst_mesh", "inst_id", "inst_pose", "camk", "workspace", "depth", "mask",
              "visible", "bbox", "dropped"):
        assert call(**{k: None}) == -1, k
    for k in ("M", "n_verts", "n_faces", "max_verts", "max_faces", "S", "H", "W"):
        assert call(**{k: 0}) == -1 and call(**{k: -3}) == -1, k
    assert call(I=-1) == -1 and call(near=0.0) == -1 and call(near=-1.0) == -1 and call(near=float("nan")) == -1
    assert call(max_faces=1 << 24) == -2 and call(max_scene_inst=256) == -2 and call(H=16385) == -2 and call(W=16385) == -2
    assert call(max_faces=1 << 24, H=0) == -1                                  # a bad argument comes first


def test_python_surface():
    import torch
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.tools.render import renderer
    assert list(inspect.signature(ops.render_depth).parameters) == ["meshset", "scene_ptr", "inst_mesh", "inst_id", "inst_pose", "camk", "H",
                                                                   "W", "near", "return_z", "return_face"]
    sig = inspect.signature(ops.render_depth).parameters
    assert sig["near"].default == 0.01 and sig["return_z"].default is False and sig["return_face"].default is False
    sig = inspect.signature(renderer.create_renderer).parameters
    assert list(sig)[:4] == ["width", "height", "renderer_type", "mode"] and sig["renderer_type"].default == "hip" and sig["mode"].default == "depth"
    assert list(inspect.signature(renderer.RendererHip.add_object).parameters) == ["self", "obj_id", "model", "scale"]
    assert list(inspect.signature(renderer.RendererHip.remove_object).parameters) == ["self", "obj_id"]
    assert list(inspect.signature(renderer.RendererHip.render_object).parameters) == ["self", "obj_id", "R", "t", "fx", "fy", "cx", "cy"]
    assert list(inspect.signature(synthetic.render_scenes).parameters)[:5] == ["meshset", "scenes", "camK", "H", "W"]
    # the refusals
    with pytest.raises(NotImplementedError, match="depth"):
        renderer.create_renderer(160, 120, mode="rgb+depth")
    with pytest.raises(NotImplementedError, match="RGB"):
        renderer.create_renderer(160, 120, mode="rgb")
    with pytest.raises(ValueError, match="Unknown renderer type"):
        renderer.create_renderer(160, 120, renderer_type="python")
    ms = ops.MeshSet([shapes.box(1.0), shapes.icosphere(1.0, 1)], device="cpu")          # packing alone needs no GPU
    assert len(ms) == 2 and ms.n_faces == [12, 80] and ms.vptr.tolist() == [0, 8, 50] and ms.fptr.tolist() == [0, 12, 92]
    assert np.allclose(ms.extent[0], 1.0)
    c = rc.cube()
    cpu = [torch.from_numpy(c[k]) for k in ("scene_ptr", "inst_mesh", "inst_id", "inst_pose", "camk")]
    with pytest.raises(TypeError, match="GPU tensor"):
        ops.render_depth(ms, *cpu, rc.H, rc.W)
    with pytest.raises(TypeError, match="MeshSet"):
        ops.render_depth([shapes.box(1.0)], *cpu, rc.H, rc.W)
    with pytest.raises(ValueError, match="face index"):
        ops.MeshSet([(np.zeros((3, 3)), np.array([[0, 1, 3]]))], device="cpu")
    inst = lambda i, m=0: dict(mesh=m, inst_id=i, R=np.eye(3), t=(0, 0, 1.0), s=1.0)
    with pytest.raises(ValueError, match="duplicate inst_id 4"):
        synthetic.pack_scenes([[inst(1)], [inst(4), inst(2), inst(4)]])
    with pytest.raises(ValueError, match="outside 1..255"):
        synthetic.pack_scenes([[inst(0)]])
    with pytest.raises(ValueError, match="mesh index"):
        synthetic.pack_scenes([[inst(1, 2)]], n_meshes=2)
    ptr, mesh, ids, pose = synthetic.pack_scenes([[], [inst(3), inst(1)]], n_meshes=1)
    assert ptr.tolist() == [0, 0, 2] and ids.tolist() == [3, 1] and ids.dtype == np.uint8 and pose.shape == (2, 3, 4) and pose.dtype == np.float32


def test_shapes_are_closed():
    from tgpose_amd.datasets import shapes
    solids = dict(box=shapes.box((0.1, 0.2, 0.3)), cylinder=shapes.cylinder(0.3, 1.0, 12), ico0=shapes.icosphere(1.0, 0),
                  ico3=shapes.icosphere(0.5, 3), **{k: shapes.lathe(p, 16) for k, p in shapes.PROFILES.items()})
    assert set(shapes.PROFILES) == {"bottle", "bowl", "can", "mug"}
    for name, (v, f) in solids.items():
        assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape[1] == 3 and f.shape[1] == 3, name
        assert f.min() == 0 and f.max() == len(v) - 1, name
        assert set(shapes.edge_counts(f).values()) == {2}, name                       # every edge is shared by exactly two faces
        a, b, c = v[f[:, 0]].astype(np.float64), v[f[:, 1]].astype(np.float64), v[f[:, 2]].astype(np.float64)
        vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0                    # positive: wound counter-clockwise from outside
        assert vol > 0, name
    assert len(solids["ico3"][1]) == 1280 and len(shapes.icosphere(1.0, 5)[1]) == 20480
    assert np.allclose(np.linalg.norm(solids["ico3"][0], axis=1), 0.5, atol=1e-6)
    assert np.isclose(np.einsum("ij,ij->i", *(lambda v, f: (v[f[:, 0]].astype(np.float64), np.cross(v[f[:, 1]], v[f[:, 2]])))(*solids["box"])).sum() / 6, 0.006)
    v, f = shapes.plane(0.6, 0.4, 3, 2)
    assert v.shape == (12, 3) and f.shape == (12, 3) and (v[:, 2] == 0).all() and np.allclose(v.max(0) - v.min(0), [0.6, 0.4, 0])
    assert sorted(set(shapes.edge_counts(f).values())) == [1, 2]                       # an open mesh: boundary edges once
    with pytest.raises(ValueError, match="lathe"):
        shapes.lathe([(0.1, 0), (0.2, 1), (0, 2)], 8)
