"""The TSDF ray caster on the device (csrc/raycast.hip: ops.tsdf_raycast, ops.tsdf_windows, ops.pose_inverse,
ops.IcpModels.from_raycast, pose.RaycastRefine, myEvaluater.scan_track) against the NumPy restatement tests/raycast_ref.py on the cases
of tests/raycast_cases.py: every output's BYTES are equal; a ray-cast model serves ICP as a mesh model does; and an object without a
model is tracked while it is scanned (DESIGN.md section 3 "Ray casting and frame-to-model tracking")."""
import ctypes

import numpy as np
import pytest
import torch

from tests import icp_ref
from tests import raycast_cases as rc
from tests import raycast_ref as rr
from tests import tsdf_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("z", "depth", "vertex", "normal", "count", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def up(a):
    a = np.array(a, order="C")                                        # a copy: the shared cases are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def volumes_of(c):
    from tgpose_amd import ops
    vol = ops.TsdfVolumes.from_meta(np.array(c["meta"]), c["vsum"].shape[1], DEV)
    vol.sum.copy_(up(c["vsum"])), vol.weight.copy_(up(c["weight"]))
    return vol


def device_cast(c, vol=None, raw=False):
    """ops.tsdf_raycast on a call of tests/raycast_cases.py, with the restatement's inverse poses -> host arrays"""
    from tgpose_amd import ops
    vol = vol if vol is not None else volumes_of(c)
    out = ops.tsdf_raycast(vol, up(c["camk"]), up(c["job_img"]), up(c["job_model"]), up(c["job_pose"]), up(c["window"]), c["h"], c["w"],
                           job_inv=up(c["job_inv"]), **c["kw"])
    if raw:
        return out
    got = {k: out[k].cpu().numpy() for k in KEYS}
    got["depth"] = got["depth"].view(np.uint16)
    return got


def same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, int((got[k] != want[k]).sum()), got[k].ravel()[:6], want[k].ravel()[:6])


# ------------------------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("name", sorted(rc.rule_calls()))
def test_rule_cases_bit_for_bit(name):
    same(device_cast(rc.rule_calls()[name]), rc.expected(name), name)


def test_sphere_bit_for_bit_and_twice():
    c = rc.sphere_call(16)
    vol = volumes_of(c)
    got = device_cast(c, vol)
    assert got["count"].min() > 500
    same(got, rc.expected("sphere16"), "sphere16")
    again = device_cast(c, vol)
    for k in KEYS:
        assert again[k].tobytes() == got[k].tobytes(), k
    # the default inverse (ops.pose_inverse: float64 cofactors on the device) is the restatement's, bit for bit
    from tgpose_amd import ops
    assert ops.pose_inverse(up(c["job_pose"])).cpu().numpy().tobytes() == c["job_inv"].tobytes()
    plain = ops.tsdf_raycast(vol, up(c["camk"]), up(c["job_img"]), up(c["job_model"]), up(c["job_pose"]), up(c["window"]), c["h"], c["w"])
    assert plain["z"].cpu().numpy().tobytes() == got["z"].tobytes()


def test_step_and_min_weight_bit_for_bit():
    """half a voxel a step, and min_weight = 3 on the sphere with one corner seen twice (tsdf_cases.weak_corner)"""
    c = dict(rc.sphere_call(16))
    vsum, weight, meta, _ = tc.weak_corner()
    c.update(vsum=vsum[None], weight=weight[None], kw=dict(step=0.5, min_weight=3))
    want = rc.run(c)
    full = rc.expected("sphere16")
    assert 0 < want["count"].sum() < full["count"].sum()
    same(device_cast(c), want, "weak corner")


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_launch():
    from tgpose_amd import _lib, ops
    c = rc.sphere_call(16)
    vol = volumes_of(c)
    args = [up(c[k]) for k in ("camk", "job_img", "job_model", "job_pose", "window")]
    call = lambda *a, **kw: ops.tsdf_raycast(vol, *a, **kw)
    with pytest.raises(TypeError):
        ops.tsdf_raycast(None, *args, 5, 7)
    with pytest.raises(TypeError):
        call(args[0], args[1].long(), *args[2:], 5, 7)
    for bad in (dict(min_weight=0), dict(step=0.0), dict(step=float("nan")), dict(step=0.01), dict(near=0.0), dict(near=float("inf"))):
        with pytest.raises(ValueError):
            call(*args, 5, 7, **bad)
    for h, w in ((0, 7), (5, 0), (5, ops.RAYCAST_MAX_SIDE + 1)):
        with pytest.raises(ValueError):
            call(*args, h, w)
    with pytest.raises(ValueError):
        call(*args[:4], args[4][:2], 5, 7)
    empty = call(args[0], args[1][:0], args[2][:0], args[3][:0], args[4][:0], 5, 7)                 # J == 0: nothing to do
    assert empty["z"].shape == (0, 5, 7) and empty["count"].shape == (0,)
    with pytest.raises(ValueError):
        ops.IcpModels.from_raycast(device_cast(c, vol, raw=True))                                       # 33 x 65 rays > ICP_MAX_POINTS
    # the C entry point itself: each refusal comes back before any launch, and the outputs keep their bytes
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {k: torch.full(s, 7, device=DEV, dtype=d) for k, s, d in (("z", (3, 5, 7), torch.float32), ("depth", (3, 5, 7), torch.int16),
                                                                   ("vertex", (3, 5, 7, 3), torch.float32), ("normal", (3, 5, 7, 3), torch.float32),
                                                                   ("count", (3,), torch.int32), ("status", (3,), torch.int32))}
    inv = up(c["job_inv"])

    def c_call(**change):
        kw = dict(sum=p(vol.sum), weight=p(vol.weight), meta=p(vol.meta), M=1, G=16, camk=p(args[0]), S=1, job_img=p(args[1]), job_model=p(args[2]),
                  job_inv=p(inv), job_window=p(args[4]), J=3, h=5, w=7, min_weight=1, step=1.0, near=0.01, **{k: p(v) for k, v in out.items()})
        kw.update(change)
        return _lib.lib().tgp_tsdf_raycast(ctypes.byref(_lib.TsdfRaycastArgs(**kw)), None)
    for change in (dict(sum=None), dict(job_inv=None), dict(count=None), dict(M=0), dict(S=0), dict(J=-1), dict(h=0), dict(w=0), dict(min_weight=0),
                   dict(step=0.0), dict(step=float("inf")), dict(near=-1.0), dict(near=float("nan"))):
        assert c_call(**change) == _lib.EINVAL, change
    for change in (dict(G=12), dict(G=8), dict(G=264), dict(J=65536), dict(h=_lib.RAYCAST_MAX_SIDE + 1), dict(step=0.03)):
        assert c_call(**change) == _lib.EUNSUPPORTED, change
    assert c_call(J=0) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())
    assert c_call() == 0
    torch.cuda.synchronize()
    assert out["count"].cpu().tolist() == [int((out["z"][j] > 0).sum()) for j in range(3)]


# ------------------------------------------------------------------------------------------------------------------ packing and windows
def test_packing_and_windows():
    from tgpose_amd import ops
    c = rc.rule_calls()["grid_5x7"]
    raw = device_cast(c, raw=True)
    models = ops.IcpModels.from_raycast(raw)
    pts, counts = rr.pack(rc.expected("grid_5x7"))
    assert models.points_normals.cpu().numpy().tobytes() == pts.tobytes() and models.counts.cpu().numpy().tolist() == counts.tolist()
    assert models.counts.dtype == torch.int32 and len(models) == 3 and models.m_cap == 35
    # windows: float32 elementwise operations in the restatement's order, and min / max, which are exact in any order: equal bytes, no
    # ulp of slack is needed anywhere
    s = rc.sphere_call(16)
    vol = volumes_of(s)
    poses = s["job_pose"].copy()
    poses = np.concatenate([poses, poses[:2]])
    poses[3, 2, 3] = -0.5                                                          # the cube behind the camera
    poses[4, 0, 0] = np.nan
    img, mdl = np.zeros(5, np.int32), np.array([0, 0, 0, 0, 0], np.int32)
    for h, w, H, W in ((40, 48, 240, 320), (1, 1, 240, 320), (5, 7, 100, 170)):      # the last frame clamps the boxes
        got = ops.tsdf_windows(vol, up(s["camk"]), up(img), up(mdl), up(poses), h, w, H, W).cpu().numpy()
        want = rr.windows(s["meta"], 16, s["camk"], img, mdl, poses, h, w, H, W)
        assert got.tobytes() == want.tobytes(), (h, w, got, want)
        assert np.isnan(got[3:]).all() and np.isfinite(got[:3]).all()
    win = ops.tsdf_windows(vol, up(s["camk"]), up(img), up(mdl), up(poses), 5, 7, 240, 320)
    out = ops.tsdf_raycast(vol, up(s["camk"]), up(img), up(mdl), up(poses), win, 5, 7)
    assert out["count"].cpu().tolist()[3:] == [0, 0] and min(out["count"].cpu().tolist()[:3]) > 0


# ------------------------------------------------------------------------------------------------------------------ the round trip
def _pose_error(rt, truth):
    rt = np.asarray(rt, dtype=np.float64)
    s = np.cbrt(np.linalg.det(rt[:3, :3]))
    return icp_ref.pose_error(rt[:3, :3] / s, rt[:3, 3], *truth)


def test_raycast_model_serves_icp():
    """tsdf_cases.scanned_two_boxes at G = 64: the volumes ray-cast at the held-out pose (40 x 48 rays over the cube's image) make an
    IcpModels; pose.refine_poses from scan_loop's start (5 degrees and 10 mm off) ends within the true mesh model's own translation
    error plus one voxel edge, and within the angle one voxel subtends at the object's radius -- tests/test_tsdf_gpu.py's bounds for
    the meshed model, restated"""
    from tgpose_amd import ops, pose
    c = tc.scanned_two_boxes(DEV, 64)
    R_true, t_true = c["held_pose"]
    start = tc.pose44(icp_ref.rot([1, 2, -1], 5.0) @ R_true, t_true + 0.010 * np.array([2.0, -1.0, 2.0]) / 3.0, tc.TURN_SCALE)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    P = up(c["held_rt"][None, :3, :4])
    win = ops.tsdf_windows(c["volumes"], c["held_camk"], zero, zero, P, 40, 48, tc.LOOP_H, tc.LOOP_W)
    cast = ops.tsdf_raycast(c["volumes"], c["held_camk"], zero, zero, P, win, 40, 48)
    hits = int(cast["count"][0])
    assert hits > 300 and int(cast["status"][0]) == 0
    err = {}
    for name, models in (("true", ops.IcpModels.from_meshset(c["true"], [0], 1024)), ("raycast", ops.IcpModels.from_raycast(cast))):
        got, info, rmse = pose.refine_poses(models, zero, up(c["cloud"][None]), up(start[None]), 0.02, mode="plane", iters=50)
        assert int(info[0, 0]) == 0, name
        err[name] = _pose_error(got[0].cpu().numpy(), c["held_pose"])
    voxel_mm, angle = 1000 * c["voxel_m"], float(np.rad2deg(np.arctan(c["voxel_m"] / c["radius_m"])))
    print("round trip: %d hits; true mesh model %.3f deg %.3f mm, ray-cast model %.3f deg %.3f mm; voxel %.3f mm = %.3f deg"
          % (hits, err["true"][0], err["true"][1], err["raycast"][0], err["raycast"][1], voxel_mm, angle))
    assert err["raycast"][1] <= err["true"][1] + voxel_mm and err["raycast"][0] <= angle
    # the full-frame depth map of the volume against the rendered frame of the true mesh: the same surface
    full = ops.tsdf_raycast(c["volumes"], c["held_camk"], zero, zero, P, up(np.array([[0, 0, 1, 1]], np.float32)), tc.LOOP_H, tc.LOOP_W)
    mine, true = full["depth"][0].cpu().numpy().view(np.uint16).astype(np.int64), c["held_depth_host"].astype(np.int64)
    both = (mine > 0) & (true > 0)
    print("full frame: %d true pixels, %d of them hit, median |difference| %.1f mm" % ((true > 0).sum(), both.sum(), np.median(np.abs(mine[both] - true[both]))))
    assert both.sum() > 0.75 * (true > 0).sum() and np.median(np.abs(mine[both] - true[both])) <= voxel_mm      # the CPU test's cap on the missed share


def test_raycast_refine_reads_nothing_back():
    """what scan_track adds to a frame -- pose.RaycastRefine (windows, ray cast, packing, ICP), the gate's arithmetic and
    ops.tsdf_integrate with the gated volume indices -- runs under torch's synchronisation debug mode 'error': no step reads a device
    value on the host.  A job whose volume holds nothing has fewer than min_hits hits: it keeps its pose and has status 4."""
    from tgpose_amd import ops, pose
    c = tc.scanned_two_boxes(DEV, 64)
    vol = ops.TsdfVolumes.from_meta(np.tile(c["volumes"].meta_host, (2, 1)), 64, DEV)
    vol.sum[0].copy_(c["volumes"].sum[0]), vol.weight[0].copy_(c["volumes"].weight[0])              # volume 1 stays empty
    R_true, t_true = c["held_pose"]
    start = up(np.stack([tc.pose44(icp_ref.rot([1, 2, -1], 2.0) @ R_true, t_true + 0.003, tc.TURN_SCALE)] * 2))
    clouds, img = up(np.stack([c["cloud"]] * 2)), torch.zeros(2, dtype=torch.int32, device=DEV)
    refine = pose.RaycastRefine(vol, 0.01, mode="plane")
    every = torch.arange(2, dtype=torch.int32, device=DEV)

    def frame():
        rts, info, rmse, hits = refine(clouds, start, c["held_camk"], img, tc.LOOP_H, tc.LOOP_W)
        ok = (info[:, 0] == 0) & (info[:, 1].float() >= 0.5 * torch.isfinite(clouds).all(-1).sum(1).float())
        job_model = torch.where(ok, every, torch.full_like(every, -1))
        status = ops.tsdf_integrate(vol, c["held_depth"], c["held_camk"], img, job_model, pose.verify_job_pose(rts), 6.0)
        return rts, info, hits, status
    frame()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rts, info, hits, status = frame()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert info[:, 0].cpu().tolist() == [0, pose.RAYCAST_FEW_HITS] and hits.cpu().tolist()[1] == 0 and int(hits[0]) > 300
    assert torch.equal(rts[1], start[1]) and not torch.equal(rts[0], start[0]) and status.cpu().tolist() == [0, 1]
    assert _pose_error(rts[0].cpu().numpy(), c["held_pose"])[1] < 1000 * c["voxel_m"] and int(vol.weight[1].sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ scan_track
RATIO, GATE, N_PTS = 0.6, 0.01, 1024
_S = {}


def sequence():
    """the smooth sequence of raycast_cases (24 frames of icp_ref.two_boxes at 240 x 320, 4 degrees a frame) rendered by
    ops.render_depth, the evaluater, init = the true pose of frame 0, and both trackers' results"""
    if _S:
        return _S
    from tgpose_amd import PoseNet9D, ops, pose
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    mesh = icp_ref.two_boxes()
    true = ops.MeshSet([mesh], device=DEV)
    n = rc.SEQ_FRAMES
    rts = rc.smooth_rts(n)
    camk = up(np.tile(np.array([tc.LOOP_K[0, 0], tc.LOOP_K[1, 1], tc.LOOP_K[0, 2], tc.LOOP_K[1, 2]], dtype=np.float32), (n, 1)))
    ren = ops.render_depth(true, torch.arange(n + 1, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
                           torch.ones(n, dtype=torch.uint8, device=DEV), up(rts[:, :3, :4]), camk, tc.LOOP_H, tc.LOOP_W)
    depth = ren["depth"].cpu().numpy().view(np.uint16)
    frames = [dict(depth=depth[k]) for k in range(n)]
    assert all((fr["depth"] > 0).sum() > 2000 for fr in frames)
    extent = (mesh[0].max(0) - mesh[0].min(0)).astype(np.float32)
    init = dict(class_ids=[3], RTs=rts[:1].astype(np.float32), scales=extent[None])
    ev = myEvaluater(PoseNet9D().to(DEV).eval(), sampler="device")
    cubes = lambda: ops.TsdfVolumes.from_meshset(true, 64)
    refine = pose.IcpRefine(ops.IcpModels.from_meshset(true, [0], 1024), [0], GATE, mode="plane")
    with_model = ev.track(frames, init, tc.LOOP_K, RATIO, n_pts=N_PTS, use_mask=False, refine=refine, init_from="previous")
    results, volumes = ev.scan_track(frames, init, tc.LOOP_K, RATIO, volumes=cubes(), n_pts=N_PTS, use_mask=False)
    voxel = float(volumes.meta_host[0, 3])
    centre = (mesh[0].max(0).astype(np.float64) + mesh[0].min(0)) / 2
    radius = float(np.linalg.norm(mesh[0].astype(np.float64) - centre, axis=1).max())
    _S.update(mesh=mesh, true=true, rts=rts, frames=frames, init=init, ev=ev, cubes=cubes, with_model=with_model, results=results, volumes=volumes,
              voxel=voxel, voxel_mm=1000 * voxel * tc.TURN_SCALE, voxel_deg=float(np.rad2deg(np.arctan(voxel / radius))))
    return _S


def truth(s, k):
    rt = s["rts"][k].astype(np.float64)
    return rt[:3, :3] / tc.TURN_SCALE, rt[:3, 3]


def test_scan_track_follows_an_object_without_a_model():
    """every frame is tracked and fused, and in every frame the pose error against the truth is at most that of the model-based
    tracker (track(init_from='previous', refine=IcpRefine(the true mesh's model))) on the same frames plus one voxel edge in
    translation and the angle a voxel subtends at the object's radius in rotation: the resolution of the model being built.
    Measured on one MI355X: worst over the 24 frames 1.21 degrees / 2.48 mm, the true-model tracker 0.56 degrees / 2.73 mm; the
    voxel is 3.23 mm = 1.35 degrees.  Nothing between frames synchronises with the host: scan_track is launches and torch operations
    on device tensors, the gate included, and its results are fetched one frame late on the fetch stream
    (test_raycast_refine_reads_nothing_back holds the new steps to it; the loop round them is read from its code)."""
    s = sequence()
    got, ref = s["results"], s["with_model"]
    assert len(got) == len(ref) == rc.SEQ_FRAMES
    keys = {"pred_RTs", "pred_scales", "status", "tracked", "icp_status", "icp_inliers", "icp_rmse", "ray_hits", "fused"}
    worst = dict(scan=[0.0, 0.0], model=[0.0, 0.0])
    for k, (g, r) in enumerate(zip(got, ref)):
        assert set(g) == keys and g["fused"].dtype == np.bool_ and g["ray_hits"].dtype == np.int32 and g["pred_RTs"].shape == (1, 4, 4)
        a, b = _pose_error(g["pred_RTs"][0], truth(s, k)), _pose_error(r["pred_RTs"][0], truth(s, k))
        print("frame %2d: scan_track %.3f deg %.3f mm (hits %d, inliers %d, rmse %.5f) | with the true model %.3f deg %.3f mm"
              % (k, a[0], a[1], g["ray_hits"][0], g["icp_inliers"][0], g["icp_rmse"][0], b[0], b[1]))
        worst["scan"] = [max(worst["scan"][0], a[0]), max(worst["scan"][1], a[1])]
        worst["model"] = [max(worst["model"][0], b[0]), max(worst["model"][1], b[1])]
    print("worst: scan_track %.3f deg %.3f mm, with the true model %.3f deg %.3f mm; voxel %.3f mm = %.3f deg"
          % (*worst["scan"], *worst["model"], s["voxel_mm"], s["voxel_deg"]))
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g["tracked"].all() and g["fused"].all() and g["status"].tolist() == [0] and g["icp_status"].tolist() == [0], k
        assert r["tracked"].all() and r["icp_status"].tolist() == [0], k
        a, b = _pose_error(g["pred_RTs"][0], truth(s, k)), _pose_error(r["pred_RTs"][0], truth(s, k))
        assert a[1] <= b[1] + s["voxel_mm"] and a[0] <= b[0] + s["voxel_deg"], (k, a, b)
        if k:
            assert g["ray_hits"][0] >= 64


def test_scan_track_builds_the_model():
    """the mesh of the volumes scan_track returns lies as close to the true surface as the mesh ``scan`` makes of the same frames with
    the TRUE poses, plus one voxel: the worst vertex-to-surface distance of both, in model units"""
    from tgpose_amd import ops
    s = sequence()
    tracked = ops.tsdf_meshset(s["volumes"])
    _, posed = s["ev"].scan(s["frames"], [s["rts"][k][None] for k in range(rc.SEQ_FRAMES)], tc.LOOP_K, volumes=s["cubes"]())
    worst = {}
    for name, ms in (("scan_track", tracked), ("scan", posed)):
        assert ms.n_faces[0] > 1000
        worst[name] = float(tc.surface_distance(ms.verts.cpu().numpy()[:3 * ms.n_faces[0]], *s["mesh"]).max())
    print("worst vertex from the true surface: scan_track %.4f voxel, scan with the true poses %.4f voxel"
          % (worst["scan_track"] / s["voxel"], worst["scan"] / s["voxel"]))
    assert worst["scan_track"] <= worst["scan"] + s["voxel"]


def test_scan_track_skips_an_empty_frame():
    """a frame whose depth is all zero, after frame 11: the poses and the volumes' bytes stay what they were, ``fused`` is False, and
    the frame after it is tracked again"""
    s = sequence()
    fr = s["frames"]
    blank = dict(depth=np.zeros_like(fr[0]["depth"]))
    head, vol_head = s["ev"].scan_track(fr[:12], s["init"], tc.LOOP_K, RATIO, volumes=s["cubes"](), n_pts=N_PTS, use_mask=False)
    got, vol = s["ev"].scan_track(fr[:12] + [blank], s["init"], tc.LOOP_K, RATIO, volumes=s["cubes"](), n_pts=N_PTS, use_mask=False)
    assert torch.equal(vol.sum, vol_head.sum) and torch.equal(vol.weight, vol_head.weight) and int(vol.weight.sum()) > 0
    for k in range(12):
        assert got[k]["pred_RTs"].tobytes() == head[k]["pred_RTs"].tobytes() == s["results"][k]["pred_RTs"].tobytes(), k
    assert got[12]["fused"].tolist() == [False] and got[12]["tracked"].tolist() == [False] and got[12]["status"].tolist() != [0]
    assert got[12]["pred_RTs"].tobytes() == got[11]["pred_RTs"].tobytes()
    more, _ = s["ev"].scan_track(fr[:12] + [blank] + fr[12:14], s["init"], tc.LOOP_K, RATIO, volumes=s["cubes"](), n_pts=N_PTS, use_mask=False)
    for k, t in ((13, 12), (14, 13)):
        assert more[k]["fused"].tolist() == [True] and more[k]["tracked"].tolist() == [True]
        a, b = _pose_error(more[k]["pred_RTs"][0], truth(s, t)), _pose_error(s["with_model"][t]["pred_RTs"][0], truth(s, t))
        assert a[1] <= b[1] + s["voxel_mm"] and a[0] <= b[0] + s["voxel_deg"], (k, a, b)
