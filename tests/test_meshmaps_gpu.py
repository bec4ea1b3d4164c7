"""The mesh maps on the device (csrc/meshmaps.hip: ops.mesh_maps, ops.mesh_windows) against the NumPy restatement
tests/meshmaps_ref.py on the cases of tests/meshmaps_cases.py, byte for byte in every output; against ops.render_depth; and as the
maps of ops.icp_dense (DESIGN.md section 3 "Mesh maps and dense model-based tracking").

Tolerances: the maps are compared EXACTLY.  The registration on them is compared as tests/test_icp_dense_gpu.py compares it: counts
and correspondences exactly, poses to 1e-6 relative (float64 sums in another order, one float32 rounding of the result)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import icp_dense_ref as dr
from tests import icp_ref
from tests import meshmaps_cases as mc
from tests import meshmaps_ref as mr
from tests import render_ref
from tests.render_ref import pose34

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("z", "depth", "vertex", "normal", "face", "count", "dropped", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def up(a):
    a = np.array(a, order="C")                                        # a copy: the shared cases are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def meshset(c):
    from tgpose_amd import ops
    ms = ops.MeshSet(c["meshes"], device=DEV)
    if c["vnormals"] is not None:
        ms.vert_normals = up(np.concatenate(c["vnormals"]))
    return ms


def device_call(c, ms=None):
    from tgpose_amd import ops
    ms = ms or meshset(c)
    out = ops.mesh_maps(ms, up(c["camk"]), up(c["job_img"]), up(c["job_mesh"]), up(c["job_pose"]), up(c["window"]), c["h"], c["w"], near=c["near"],
                        normals="face" if c["vnormals"] is None else "vertex", return_face=True)
    assert set(out) == set(KEYS)
    return {k: (v.view(torch.uint16) if k == "depth" else v).cpu().numpy() for k, v in out.items()}


def same_bytes(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k].view(np.int32 if got[k].itemsize == 4 else np.uint16) != want[k].view(np.int32 if got[k].itemsize == 4 else np.uint16))
            raise AssertionError("%s: %s differs in %d words, first at %s: %r != %r" % (what, k, len(bad), bad[0].tolist(), got[k][tuple(bad[0])],
                                                                                       want[k][tuple(bad[0])]))


@pytest.mark.parametrize("name", sorted(mc.calls()))
def test_kernel_equals_the_restatement(name):
    c = mc.calls()[name]
    got = device_call(c)
    print("%s: %d jobs of %d x %d, hits %s dropped %s status %s" % (name, len(c["job_img"]), c["h"], c["w"], got["count"].tolist(), got["dropped"].tolist(),
                                                                   got["status"].tolist()))
    same_bytes(got, mc.expected(name), name)


@pytest.mark.parametrize("name", ["partial_tiles", "cap_sweep", "vertex_normals"])
def test_full_frame_window_equals_render_depth(name):
    """window (0, 0, 1, 1) and (h, w) = (H, W): z and face are ops.render_depth's of the one-instance scene, byte for byte (a miss is 0
    here and +inf there); a 37 x 53 frame for the sphere of vertex_normals, whose own window is not the full frame"""
    from tgpose_amd import ops
    c = mc.calls()[name]
    if name == "vertex_normals":
        c = dict(c, window=np.array([mc.FULL], np.float32), h=37, w=53)
    ms = meshset(c)
    got = device_call(c, ms)
    r = ops.render_depth(ms, up(np.array([0, 1], np.int32)), up(c["job_mesh"]), up(np.array([1], np.uint8)), up(c["job_pose"]), up(c["camk"]), c["h"],
                         c["w"], near=c["near"], return_z=True, return_face=True)
    z, face = r["z"][0].cpu().numpy(), r["face"][0].cpu().numpy()
    hit = face >= 0
    assert hit.sum() > 100 and got["face"][0].tobytes() == face.tobytes()
    assert got["z"][0][hit].tobytes() == z[hit].tobytes() and np.isinf(z[~hit]).all() and not got["z"][0][~hit].any()
    assert got["depth"][0].tobytes() == r["depth"][0].view(torch.uint16).cpu().numpy().tobytes()
    assert got["dropped"][0] == int(r["dropped"].sum())


def test_two_calls_give_identical_bytes():
    for name in ("three_jobs", "cap_sweep", "windows"):
        c = mc.calls()[name]
        ms = meshset(c)
        a, b = device_call(c, ms), device_call(c, ms)
        same_bytes(a, b, name)


@pytest.mark.parametrize("name", ["three_jobs", "windows", "bad_index"])
def test_a_job_does_not_depend_on_its_neighbours(name):
    """each job alone gives the bytes it gives among the others"""
    c = mc.calls()[name]
    ms = meshset(c)
    together = device_call(c, ms)
    for j in range(len(c["job_img"])):
        alone = device_call(mc.job_alone(c, j), ms)
        for k in KEYS:
            assert alone[k][0].tobytes() == together[k][j].tobytes(), (name, j, k)


def test_without_face_and_without_jobs():
    from tgpose_amd import ops
    c = mc.calls()["three_jobs"]
    ms = meshset(c)
    args = (ms, up(c["camk"]), up(c["job_img"]), up(c["job_mesh"]), up(c["job_pose"]), up(c["window"]), c["h"], c["w"])
    out = ops.mesh_maps(*args)
    assert set(out) == set(KEYS) - {"face"}
    want = mc.expected("three_jobs")
    for k in out:
        assert (out[k].view(torch.uint16) if k == "depth" else out[k]).cpu().numpy().tobytes() == want[k].tobytes(), k
    none = ops.mesh_maps(ms, args[1], args[2][:0].contiguous(), args[3][:0].contiguous(), args[4][:0].contiguous(), args[5][:0].contiguous(), 4, 5)
    assert none["z"].shape == (0, 4, 5) and none["vertex"].shape == (0, 4, 5, 3) and none["count"].shape == (0,)
    models = ops.IcpModels.from_raycast(out)                          # the dict serves where a ray cast's does
    assert len(models) == 3
    with pytest.raises(ValueError):
        ops.mesh_maps(*args, normals="vertex")                        # the set has no vertex normals
    with pytest.raises(ValueError):
        ops.mesh_maps(*args, normals="smooth")
    with pytest.raises(ValueError):
        ops.mesh_maps(*args[:6], 0, 5)
    with pytest.raises(ValueError):
        ops.mesh_maps(*args, near=0.0)
    with pytest.raises(ValueError):
        ops.mesh_maps(*args[:5], args[5][:2].contiguous(), c["h"], c["w"])
    with pytest.raises(TypeError):
        ops.mesh_maps(*args[:3], args[3].long(), *args[4:])
    with pytest.raises(TypeError):
        ops.mesh_maps(None, *args[1:])


def test_refusals_leave_the_outputs_untouched():
    from tgpose_amd import _lib
    c = mc.calls()["three_jobs"]
    ms = meshset(c)
    J, h, w = 3, c["h"], c["w"]
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    ins = dict(camk=up(c["camk"]), job_img=up(c["job_img"]), job_mesh=up(c["job_mesh"]), job_pose=up(c["job_pose"]), job_window=up(c["window"]))
    out = {k: torch.full(sh, 7, device=DEV, dtype=d) for k, sh, d in (("z", (J, h, w), torch.float32), ("depth", (J, h, w), torch.int16),
                                                                    ("vertex", (J, h, w, 3), torch.float32), ("normal", (J, h, w, 3), torch.float32),
                                                                    ("face", (J, h, w), torch.int32), ("count", (J,), torch.int32),
                                                                    ("dropped", (J,), torch.int32), ("status", (J,), torch.int32))}
    mesh = dict(ms.fields(maxima=True))
    need = _lib.lib().tgp_mesh_maps_workspace_bytes(J, mesh["max_verts"], mesh["max_faces"])
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def c_call(**change):
        a = dict(mesh, vnormals=None, S=3, J=J, h=h, w=w, near=0.01, workspace=p(ws), workspace_bytes=need, **{k: p(v) for k, v in ins.items()},
                 **{k: p(v) for k, v in out.items()})
        a.update(change)
        return _lib.lib().tgp_mesh_maps(ctypes.byref(_lib.MeshMapsArgs(**a)), None)
    for change in ([{k: None} for k in ("camk", "verts", "faces", "vptr", "fptr", "job_img", "job_mesh", "job_pose", "job_window", "z", "depth", "vertex",
                                        "normal", "count", "dropped", "status", "workspace")] +
                   [dict(S=0), dict(M=0), dict(h=0), dict(w=0), dict(n_verts=0), dict(n_faces=0), dict(max_verts=0), dict(max_faces=0), dict(J=-1),
                    dict(near=0.0), dict(near=-1.0), dict(near=float("inf")), dict(near=float("nan")), dict(workspace_bytes=need - 1)]):
        assert c_call(**change) == _lib.EINVAL, change
    for change in (dict(J=65536), dict(h=_lib.RAYCAST_MAX_SIDE + 1), dict(w=_lib.RAYCAST_MAX_SIDE + 1), dict(max_faces=_lib.lib().tgp_render_max_faces())):
        assert c_call(**change) == _lib.EUNSUPPORTED, change
    assert c_call(J=0) == 0
    wsb = _lib.lib().tgp_mesh_maps_workspace_bytes
    assert wsb(-1, 8, 8) == _lib.EINVAL and wsb(1, 0, 8) == _lib.EINVAL and wsb(1, 8, 0) == _lib.EINVAL
    assert wsb(65536, 8, 8) == _lib.EUNSUPPORTED and wsb(1, 8, _lib.lib().tgp_render_max_faces()) == _lib.EUNSUPPORTED and wsb(0, 8, 8) >= 0
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())
    assert c_call() == 0 and c_call(face=None) == 0
    torch.cuda.synchronize()
    want = mc.expected("three_jobs")
    for k, v in out.items():
        assert (v.view(torch.uint16) if k == "depth" else v).cpu().numpy().tobytes() == want[k].tobytes(), k


def test_mesh_windows_equal_the_restatement():
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes
    meshes = [icp_ref.two_boxes(), shapes.icosphere(0.1, 1), shapes.box((0.3, 0.2, 0.1))]
    ms = ops.MeshSet(meshes, device=DEV)
    K = np.array([[288.8, 288.8, 159.5, 119.5], [150.0, 140.0, 80.0, 60.0]], np.float32)
    poses = np.stack([pose34(icp_ref.rot([1, 2, 3], 20.0), [0.02, 0.01, 0.5], 0.16), pose34(np.eye(3), [0, 0, 0.05]), pose34(np.eye(3), [0.3, 0, 0.4], 1.5),
                      pose34(icp_ref.rot([0, 1, 0], 80.0), [-0.3, 0.1, 0.9]), pose34(np.eye(3), [0, 0, np.nan]), pose34(np.eye(3), [5.0, 0, 0.3])])
    job_img, job_mesh = np.array([0, 1, 1, 0, 0, 7], np.int32), np.array([0, 1, 2, -3, 0, 2], np.int32)
    for h, w, H, W in ((96, 128, 240, 320), (1, 1, 240, 320), (40, 48, 120, 160)):
        got = ops.mesh_windows(ms, up(K), up(job_img), up(job_mesh), up(poses), h, w, H, W)
        want = mr.windows(meshes, K, job_img, job_mesh, poses, h, w, H, W)
        assert got.dtype == torch.float32 and got.is_contiguous() and got.cpu().numpy().tobytes() == want.tobytes(), (h, w, got.cpu().numpy(), want)
    assert np.isnan(want[1]).all() and np.isnan(want[4]).all() and np.isfinite(want[[0, 2, 3, 5]]).all()
    assert ms.bounds() is ms.bounds() and ms.bounds().shape == (3, 2, 3)                      # made once


def test_icp_dense_on_mesh_maps_equals_the_restatement():
    """two jobs on one rendered frame of icp_ref.two_boxes, from 3 degrees / 6 mm and 1 degree / 2 mm off: ops.mesh_windows, ops.mesh_maps,
    ops.dense_rects and ops.icp_dense equal meshmaps_ref + icp_dense_ref.refine: the maps in every byte, counts and correspondences
    exactly, the poses to 1e-6"""
    from tgpose_amd import ops
    v, f = icp_ref.two_boxes()
    H, W, h, w, s, gate = 120, 160, 60, 80, 0.16, 0.02
    K = np.array([[300.0, 300.0, 79.5, 59.5]], np.float32)
    R_true, t_true = icp_ref.rot([1, 0, 0], -150.0) @ icp_ref.rot([0, 1, 0], 35.0), np.array([0.01, 0.0, 0.6])
    frame = render_ref.render_scene([(v, f)], [(0, 1, pose34(R_true, t_true, s))], K[0], H, W)["depth"]
    starts = [(icp_ref.rot([1, 2, -1], 3.0) @ R_true, t_true + 0.006 * np.array([2.0, -1.0, 2.0]) / 3.0),
              (icp_ref.rot([-1, 1, 1], 1.0) @ R_true, t_true + 0.002 * np.array([1.0, 2.0, -2.0]) / 3.0)]
    P = np.stack([pose34(R, t, s) for R, t in starts])
    R0, t0, s0 = np.stack([R for R, _ in starts]).astype(np.float32), np.stack([t for _, t in starts]).astype(np.float32), np.full(2, s, np.float32)
    zero = np.zeros(2, np.int32)
    win = mr.windows([(v, f)], K, zero, zero, P, h, w, H, W)
    maps = mr.maps([(v, f)], K, zero, zero, P, win, h, w)
    rect = dr.rects(win, h, w, H, W)
    ms = ops.MeshSet([(v, f)], device=DEV)
    dwin = ops.mesh_windows(ms, up(K), up(zero), up(zero), up(P), h, w, H, W)
    dmaps = ops.mesh_maps(ms, up(K), up(zero), up(zero), up(P), dwin, h, w)
    drect = ops.dense_rects(dwin, h, w, H, W)
    assert dwin.cpu().numpy().tobytes() == win.tobytes() and drect.cpu().numpy().tobytes() == rect.tobytes()
    for k in ("z", "vertex", "normal", "count"):
        assert dmaps[k].cpu().numpy().tobytes() == maps[k].tobytes(), k
    cap = (int(rect[:, 2].max() - rect[:, 0].min()) + 1) * (int(rect[:, 3].max() - rect[:, 1].min()) + 1) + 3
    R, t, sc, info, rmse, corr = (x.cpu().numpy() for x in ops.icp_dense(up(frame[None]), up(K), up(zero), drect, dmaps, dwin, up(P), up(R0), up(t0), up(s0),
                                                                         gate, iters=50, corr_cap=cap))
    for j in range(2):
        r = dr.refine(frame, K[0], dict(z=maps["z"][j], vertex=maps["vertex"][j], normal=maps["normal"][j]), win[j], P[j], rect[j], R0[j], t0[j], s0[j],
                      gate, iters=50)
        err = icp_ref.pose_error(R[j], t[j], R_true, t_true)
        print("job %d: %d hits, status %d inliers %d iters %d candidates %d | ref %d %d %d %d | %.4f deg %.4f mm from the truth"
              % (j, maps["count"][j], *info[j], r["status"], r["inliers"], r["iters"], r["candidates"], *err))
        n = len(r["corr"])
        assert r["status"] == 0 and r["candidates"] >= 300 and 2 * r["inliers"] >= r["candidates"]
        assert info[j].tolist() == [r["status"], r["inliers"], r["iters"], r["candidates"]], j
        assert n <= cap and np.array_equal(corr[j, :n], r["corr"]) and (corr[j, n:] == -1).all(), j
        assert np.abs(R[j].astype(np.float64) - r["R64"]).max() <= 1e-6 and np.abs(t[j].astype(np.float64) - r["t64"]).max() <= 1e-6, j
        assert abs(float(rmse[j]) - float(r["rmse"])) <= 1e-6 * abs(float(r["rmse"])) + 1e-12
