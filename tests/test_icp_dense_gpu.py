"""Dense projective ICP on the device (csrc/icp_dense.hip: ops.icp_dense, ops.dense_rects, pose.DenseRefine,
myEvaluater.scan_track(register='dense')) against the NumPy restatement tests/icp_dense_ref.py on the cases of
tests/icp_dense_cases.py, and against ground truth (DESIGN.md section 3 "Dense projective registration").

Tolerances: correspondences, inliers, candidates, iterations and status are compared EXACTLY.  The sums and the solve are float64 on
both sides, so poses differ by the one float32 rounding of the result and by the order of summation through the solve: 1e-6 relative,
tests/test_icp_gpu.py's tolerance for the same reason.  s is not touched: its bits are the input's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import icp_dense_cases as dc
from tests import icp_dense_ref as dr
from tests import icp_ref
from tests import raycast_cases as rc
from tests import tsdf_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def up(a):
    a = np.array(a, order="C")                                        # a copy: the shared cases are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def device_args(c):
    rcd = dict(z=up(c["z"]), vertex=up(c["vertex"]), normal=up(c["normal"]))
    pos = (up(c["depth"]), up(c["camk"]), up(c["job_img"]), up(c["rect"]), rcd, up(c["window"]), up(c["ref"]), up(c["R"]), up(c["t"]), up(c["s"]),
           up(c["max_dist"]))
    kw = dict(stride=c["stride"], mask=None if c["mask"] is None else up(c["mask"]),
              job_mask_val=None if c["mask"] is None else up(c["job_mask_val"]), **c["kw"])
    return pos, kw


def device_call(c, corr_cap):
    from tgpose_amd import ops
    pos, kw = device_args(c)
    return [x.cpu().numpy() for x in ops.icp_dense(*pos, corr_cap=corr_cap, **kw)]


def compare(name, c, got, want, corr_cap):
    R, t, s, info, rmse, corr = got
    assert s.tobytes() == c["s"].tobytes(), name
    for j, r in enumerate(want):
        n = dc.pixels(c, j) if r["status"] != 3 else 0
        print("%s job %d: %d pixels, status %d inliers %d iters %d candidates %d rmse %.6e | ref %d %d %d %d %.6e | max |dR| %.2e |dt| %.2e"
              % (name, j, n, *info[j], rmse[j], r["status"], r["inliers"], r["iters"], r["candidates"], r["rmse"],
                 np.abs(R[j] - r["R64"]).max(), np.abs(t[j] - r["t64"]).max()))
        assert info[j].tolist() == [r["status"], r["inliers"], r["iters"], r["candidates"]], (name, j)
        assert n <= corr_cap and np.array_equal(corr[j, :n], r["corr"][:n]) and (corr[j, n:] == -1).all(), (name, j)
        if r["status"]:
            assert R[j].tobytes() == c["R"][j].tobytes() and t[j].tobytes() == c["t"][j].tobytes(), (name, j)
        else:
            assert np.abs(R[j].astype(np.float64) - r["R64"]).max() <= 1e-6, (name, j)
            assert np.abs(t[j].astype(np.float64) - r["t64"]).max() <= 1e-6 * max(1.0, np.linalg.norm(r["t64"])), (name, j)
        if r["inliers"] and np.isfinite(r["rmse"]):
            assert abs(float(rmse[j]) - float(r["rmse"])) <= 1e-6 * abs(float(r["rmse"])) + 1e-12, (name, j)   # 1e-12: an exact fit's zero
        else:
            assert np.isnan(rmse[j]) == bool(np.isnan(r["rmse"])), (name, j)


# what the shapes cover beyond the rules: a single partial wave (six_by_eight, 56 pixels; five_pixels), pixel counts that are no
# multiple of 512 (rect_partly_outside 1271, stride2 690, stride3 336), more than 512 x 8 pixels (object, 5772: several per lane), and
# three jobs with their own rectangles, volumes and intrinsics in one call (three_jobs)
@pytest.mark.parametrize("name", sorted(dc.rule_calls()) + ["object"])
def test_kernel_equals_the_restatement(name):
    c = dc.object_case()[0] if name == "object" else dc.rule_calls()[name]
    J = len(c["job_img"])
    cap = max(max(dc.pixels(c, j) for j in range(J)) + 3, 8)          # a few words past the longest job: they must read -1
    got = device_call(c, cap)
    compare(name, c, got, dc.expected(name), cap)
    if name == "object":
        assert dc.pixels(c, 0) > 512 * 8
    if name == "six_by_eight":
        assert dc.pixels(c, 0) < 64
    # a shorter corr than the job: only its first words are written, and without one the results are the same
    from tgpose_amd import ops
    pos, kw = device_args(c)
    short = ops.icp_dense(*pos, corr_cap=5, **kw)
    none = ops.icp_dense(*pos, **kw)
    assert len(none) == 5 and np.array_equal(short[5].cpu().numpy(), got[5][:, :5])
    for a, b, d in zip(none, short, got):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == d.tobytes()


def test_two_calls_give_identical_bytes():
    for c in (dc.object_case()[0], dc.rule_calls()["three_jobs"]):
        a, b = device_call(c, 6000), device_call(c, 6000)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_job_does_not_depend_on_its_neighbours():
    """the jobs of three_jobs one at a time give the bytes they give together"""
    from tgpose_amd import ops
    c = dc.rule_calls()["three_jobs"]
    pos, kw = device_args(c)
    together = ops.icp_dense(*pos, **kw)
    for j in range(3):
        alone = ops.icp_dense(*[x[j:j + 1].contiguous() if torch.is_tensor(x) and i >= 2 else
                                ({k: v[j:j + 1].contiguous() for k, v in x.items()} if isinstance(x, dict) else x) for i, x in enumerate(pos)], **kw)
        for a, b in zip(alone, together):
            assert torch.equal(a[0], b[j]), j


def test_refusals_leave_the_outputs_untouched():
    from tgpose_amd import _lib, ops
    c = dc.rule_calls()["three_jobs"]
    pos, kw = device_args(c)
    depth, camk, job_img, rect, rcd, window, ref, R, t, s, gate = pos
    with pytest.raises(ValueError):
        ops.icp_dense(*pos, stride=0)
    with pytest.raises(ValueError):
        ops.icp_dense(*pos, iters=0)
    with pytest.raises(ValueError):
        ops.icp_dense(*pos, tol_rot=-1.0)
    with pytest.raises(ValueError):
        ops.icp_dense(*pos, mask=torch.zeros_like(depth, dtype=torch.uint8))                              # a mask without values
    with pytest.raises(ValueError):
        ops.icp_dense(depth, camk, job_img, rect[:2].contiguous(), rcd, window, ref, R, t, s, gate)
    with pytest.raises(TypeError):
        ops.icp_dense(depth, camk, job_img, rect.float(), rcd, window, ref, R, t, s, gate)
    with pytest.raises(TypeError):
        ops.icp_dense(depth, camk, job_img, rect, dict(z=rcd["z"]), window, ref, R, t, s, gate)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    empty = ops.icp_dense(depth, camk, none, rect[:0].contiguous(), {k: v[:0].contiguous() for k, v in rcd.items()}, window[:0].contiguous(),
                          ref[:0].contiguous(), R[:0].contiguous(), t[:0].contiguous(), s[:0].contiguous(), gate[:0].contiguous())
    assert empty[0].shape == (0, 3, 3) and empty[3].shape == (0, 4)
    # the C entry point itself: each refusal comes back before any launch, and the outputs keep their bytes
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    out = {k: torch.full(sh, 7, device=DEV, dtype=d) for k, sh, d in (("R_out", (3, 3, 3), torch.float32), ("t_out", (3, 3), torch.float32),
                                                                    ("s_out", (3,), torch.float32), ("info", (3, 4), torch.int32),
                                                                    ("rmse", (3,), torch.float32), ("corr", (3, 16), torch.int32))}
    mask, vals = torch.zeros(depth.shape, dtype=torch.uint8, device=DEV), torch.zeros(3, dtype=torch.uint8, device=DEV)
    h, w = rcd["z"].shape[1:]

    def c_call(**change):
        a = dict(depth=p(depth), camk=p(camk), S=2, H=dc.RULE_H, W=dc.RULE_W, mask=None, job_mask_val=None, vertex=p(rcd["vertex"]),
                 normal=p(rcd["normal"]), z=p(rcd["z"]), h=h, w=w, job_window=p(window), job_ref=p(ref), job_img=p(job_img), job_rect=p(rect), J=3,
                 stride=1, R=p(R), t=p(t), s=p(s), max_dist=p(gate), iters=20, tol_rot=1e-5, tol_trans=1e-6, min_inliers=6, corr_cap=16,
                 **{k: p(v) for k, v in out.items()})
        a.update(change)
        return _lib.lib().tgp_icp_dense(ctypes.byref(_lib.IcpDenseArgs(**a)), None)
    for change in (dict(depth=None), dict(camk=None), dict(vertex=None), dict(normal=None), dict(z=None), dict(job_window=None), dict(job_ref=None),
                   dict(job_img=None), dict(job_rect=None), dict(R=None), dict(t=None), dict(s=None), dict(max_dist=None), dict(R_out=None),
                   dict(t_out=None), dict(s_out=None), dict(info=None), dict(rmse=None), dict(corr=None), dict(mask=p(mask)), dict(S=0), dict(H=0),
                   dict(W=0), dict(J=-1), dict(h=0), dict(w=0), dict(stride=0), dict(iters=0), dict(tol_rot=-1e-9), dict(tol_trans=-1.0),
                   dict(tol_rot=float("nan")), dict(min_inliers=-1), dict(corr_cap=-1)):
        assert c_call(**change) == _lib.EINVAL, change
    for change in (dict(J=65536), dict(h=_lib.RAYCAST_MAX_SIDE + 1), dict(w=_lib.RAYCAST_MAX_SIDE + 1), dict(H=16385), dict(W=16385)):
        assert c_call(**change) == _lib.EUNSUPPORTED, change
    assert c_call(J=0) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())
    assert c_call() == 0 and c_call(mask=p(mask), job_mask_val=p(vals)) == 0 and c_call(corr=None, corr_cap=0) == 0
    torch.cuda.synchronize()
    assert out["info"][:, 0].cpu().tolist() == [0, 0, 0]


def test_dense_rects_equal_the_restatement():
    from tgpose_amd import ops
    nan, inf = np.nan, np.inf
    win = np.array([[10.2, 5.7, 0.5, 0.25], [30, 10, -1, 1], [nan, 5, 1, 1], [5, 5, 1, nan], [inf, 5, 1, 1], [-3.5, 40.0, 2.0, 1.0], [5, -inf, 1, 1],
                    [0, 0, 1, 1], [63.4, 47.2, 0.1, 0.1], [5, 5, inf, 1], [nan, nan, nan, nan]], np.float32)
    c, _, _ = dc.object_case()
    win = np.concatenate([win, c["window"], dc.rule_calls()["three_jobs"]["window"]])
    for h, w, H, W in ((9, 21, 48, 64), (1, 1, 48, 64), (96, 128, 240, 320), (60, 80, 120, 160)):
        got = ops.dense_rects(up(win), h, w, H, W)
        assert got.dtype == torch.int32 and got.is_contiguous()
        assert got.cpu().numpy().tobytes() == dr.rects(win, h, w, H, W).tobytes(), (h, w, got.cpu().numpy(), dr.rects(win, h, w, H, W))
    assert ops.dense_rects(up(win[2:4]), 4, 4, 48, 64).cpu().tolist() == [[0, 0, -1, -1]] * 2


# ------------------------------------------------------------------------------------------------------------------ the round trip
def _pose_error(rt, truth):
    rt = np.asarray(rt, dtype=np.float64)
    s = np.cbrt(np.linalg.det(rt[:3, :3]))
    return icp_ref.pose_error(rt[:3, :3] / s, rt[:3, 3], *truth)


def held_start(c, deg=5.0, mm=10.0):
    R_true, t_true = c["held_pose"]
    return tc.pose44(icp_ref.rot([1, 2, -1], deg) @ R_true, t_true + 0.001 * mm * np.array([2.0, -1.0, 2.0]) / 3.0, tc.TURN_SCALE)


def test_dense_refine_round_trip():
    """tsdf_cases.scanned_two_boxes at G = 64: pose.DenseRefine on the held-out frame from 5 degrees and 10 mm off ends within the
    bounds tests/test_raycast_gpu.py test_raycast_model_serves_icp holds the ray-cast model to: the true mesh model's own translation
    error (pose.refine_poses on the frame's 1024-point cloud) plus one voxel edge, and the angle one voxel subtends at the object's
    radius.  Measured on one MI355X: 3347 hits of the 96 x 128 map, 5466 candidates, 5712 final inliers, 7 iterations; 0.072 degrees /
    0.150 mm against 0.427 degrees / 0.116 mm with the true mesh's model (the sparse path's ray-cast model: 0.240 / 0.462); the voxel
    is 3.234 mm = 1.347 degrees."""
    from tgpose_amd import ops, pose
    c = tc.scanned_two_boxes(DEV, 64)
    start = up(held_start(c)[None])
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    got, info, rmse = pose.refine_poses(ops.IcpModels.from_meshset(c["true"], [0], 1024), zero, up(c["cloud"][None]), start, 0.02, mode="plane", iters=50)
    assert int(info[0, 0]) == 0
    true = _pose_error(got[0].cpu().numpy(), c["held_pose"])
    rts, info, rmse, hits = pose.DenseRefine(c["volumes"], 0.02, iters=50)(c["held_depth"], start, c["held_camk"], zero)
    info = info.cpu().numpy()
    dense = _pose_error(rts[0].cpu().numpy(), c["held_pose"])
    voxel_mm, angle = 1000 * c["voxel_m"], float(np.rad2deg(np.arctan(c["voxel_m"] / c["radius_m"])))
    print("round trip: %d hits, %d candidates, %d inliers, %d iterations, rmse %.5f; dense %.3f deg %.3f mm, true mesh model %.3f deg %.3f mm; "
          "voxel %.3f mm = %.3f deg" % (int(hits[0]), info[0, 3], info[0, 1], info[0, 2], float(rmse[0]), *dense, *true, voxel_mm, angle))
    assert info[0, 0] == 0 and info[0, 3] >= 300 and 2 * info[0, 1] >= info[0, 3] and int(hits[0]) > 300
    assert dense[1] <= true[1] + voxel_mm and dense[0] <= angle


def test_dense_refine_reads_nothing_back():
    """what scan_track(register='dense') adds to a frame -- pose.DenseRefine (windows, ray cast, rectangles, dense ICP), the gate's
    arithmetic and ops.tsdf_integrate with the gated volume indices -- runs under torch's synchronisation debug mode 'error', as
    tests/test_raycast_gpu.py test_raycast_refine_reads_nothing_back holds its sibling.  A job whose volume holds nothing has fewer
    than min_hits hits: it keeps its pose and has status 4."""
    from tgpose_amd import ops, pose
    c = tc.scanned_two_boxes(DEV, 64)
    vol = ops.TsdfVolumes.from_meta(np.tile(c["volumes"].meta_host, (2, 1)), 64, DEV)
    vol.sum[0].copy_(c["volumes"].sum[0]), vol.weight[0].copy_(c["volumes"].weight[0])              # volume 1 stays empty
    start = up(np.stack([held_start(c, 2.0, 3.0)] * 2))
    img = torch.zeros(2, dtype=torch.int32, device=DEV)
    refine = pose.DenseRefine(vol, 0.01)
    every = torch.arange(2, dtype=torch.int32, device=DEV)

    def frame():
        rts, info, rmse, hits = refine(c["held_depth"], start, c["held_camk"], img)
        ok = (info[:, 0] == 0) & (info[:, 1].float() >= 0.5 * info[:, 3].float())
        job_model = torch.where(ok, every, torch.full_like(every, -1))
        status = ops.tsdf_integrate(vol, c["held_depth"], c["held_camk"], img, job_model, pose.verify_job_pose(torch.where(ok[:, None, None], rts, start)), 6.0)
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
_D = {}


def dense_sequence():
    """tests/test_raycast_gpu.py's sequence (24 frames of icp_ref.two_boxes at 240 x 320, 4 degrees a frame; both of its trackers'
    results) and scan_track(register='dense') on it"""
    if not _D:
        from tests import test_raycast_gpu as sparse
        s = sparse.sequence()
        results, volumes = s["ev"].scan_track(s["frames"], s["init"], tc.LOOP_K, volumes=s["cubes"](), use_mask=False, register="dense")
        _D.update(s=s, results=results, volumes=volumes, truth=sparse.truth)
    return _D


def test_scan_track_dense_follows_an_object_without_a_model():
    """every frame is tracked and fused, and in every frame the pose error against the truth is within the bound
    tests/test_raycast_gpu.py holds the sparse path to: that of the model-based tracker on the same frames plus one voxel edge in
    translation and the angle a voxel subtends at the object's radius in rotation.  Measured on one MI355X, worst over the 24 frames:
    dense 0.213 degrees / 1.988 mm, the sparse path 1.214 degrees / 2.481 mm (recorded there as 1.21 / 2.48), the true-model tracker
    0.560 degrees / 2.734 mm; 4670 to 6064 inliers a frame against the sparse path's 813 to 977; the voxel is 3.234 mm = 1.347
    degrees.  The table is printed."""
    d = dense_sequence()
    s, got = d["s"], d["results"]
    ref, sparse = s["with_model"], s["results"]
    assert len(got) == len(ref) == rc.SEQ_FRAMES
    keys = {"pred_RTs", "pred_scales", "status", "tracked", "icp_status", "icp_inliers", "icp_rmse", "ray_hits", "fused"}
    worst = dict(dense=[0.0, 0.0], sparse=[0.0, 0.0], model=[0.0, 0.0])
    rows = []
    for k, (g, p, r) in enumerate(zip(got, sparse, ref)):
        assert set(g) == keys and g["fused"].dtype == np.bool_ and g["ray_hits"].dtype == np.int32 and g["pred_RTs"].shape == (1, 4, 4)
        a, b, m = (_pose_error(x["pred_RTs"][0], d["truth"](s, k)) for x in (g, p, r))
        rows.append((a, m))
        print("frame %2d: dense %.3f deg %.3f mm (hits %d, inliers %d, rmse %.5f) | sparse %.3f deg %.3f mm (inliers %d) | with the true model %.3f deg %.3f mm"
              % (k, a[0], a[1], g["ray_hits"][0], g["icp_inliers"][0], g["icp_rmse"][0], b[0], b[1], p["icp_inliers"][0], m[0], m[1]))
        for name, e in (("dense", a), ("sparse", b), ("model", m)):
            worst[name] = [max(worst[name][0], e[0]), max(worst[name][1], e[1])]
    print("worst: dense %.3f deg %.3f mm, sparse %.3f deg %.3f mm (recorded: 1.21 deg 2.48 mm), with the true model %.3f deg %.3f mm; voxel %.3f mm = %.3f deg"
          % (*worst["dense"], *worst["sparse"], *worst["model"], s["voxel_mm"], s["voxel_deg"]))
    for k, (g, (a, m)) in enumerate(zip(got, rows)):
        assert g["tracked"].all() and g["fused"].all() and g["status"].tolist() == [0] and g["icp_status"].tolist() == [0], k
        assert a[1] <= m[1] + s["voxel_mm"] and a[0] <= m[0] + s["voxel_deg"], (k, a, m)
        if k:
            assert g["ray_hits"][0] >= 64 and g["icp_inliers"][0] >= 300


def test_scan_track_dense_skips_an_empty_frame():
    """a frame whose depth is all zero, after frame 11: the poses and the volumes' bytes stay what they were, ``fused`` is False, and
    the frame after it is tracked again"""
    d = dense_sequence()
    s = d["s"]
    fr = s["frames"]
    blank = dict(depth=np.zeros_like(fr[0]["depth"]))
    run = lambda frames: s["ev"].scan_track(frames, s["init"], tc.LOOP_K, volumes=s["cubes"](), use_mask=False, register="dense")
    head, vol_head = run(fr[:12])
    got, vol = run(fr[:12] + [blank])
    assert torch.equal(vol.sum, vol_head.sum) and torch.equal(vol.weight, vol_head.weight) and int(vol.weight.sum()) > 0
    for k in range(12):
        assert got[k]["pred_RTs"].tobytes() == head[k]["pred_RTs"].tobytes() == d["results"][k]["pred_RTs"].tobytes(), k
    assert got[12]["fused"].tolist() == [False] and got[12]["status"].tolist() == [0] and got[12]["icp_status"].tolist() == [1]
    assert got[12]["pred_RTs"].tobytes() == got[11]["pred_RTs"].tobytes()
    more, _ = run(fr[:12] + [blank] + fr[12:14])
    for k, t in ((13, 12), (14, 13)):
        assert more[k]["fused"].tolist() == [True] and more[k]["icp_status"].tolist() == [0]
        a, b = _pose_error(more[k]["pred_RTs"][0], d["truth"](s, t)), _pose_error(s["with_model"][t]["pred_RTs"][0], d["truth"](s, t))
        assert a[1] <= b[1] + s["voxel_mm"] and a[0] <= b[0] + s["voxel_deg"], (k, a, b)


def test_scan_track_sparse_is_the_default():
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    import inspect
    assert inspect.signature(myEvaluater.scan_track).parameters["register"].default == "sparse"
    d = dense_sequence()
    with pytest.raises(ValueError):
        d["s"]["ev"].scan_track(d["s"]["frames"][:1], d["s"]["init"], tc.LOOP_K, 0.6, use_mask=False, register="projective")
