"""Times the mesh maps (ops.mesh_maps: csrc/meshmaps.hip), pose.DenseModelRefine and myEvaluater.track(refine=DenseModelRefine)
beside what they stand next to, on the six-object rendered 480 x 640 scene of scripts/icp_time.py.  Writes profiles/meshmaps_time.json:

  * mesh_maps: device time of ONE call of 6 and of 192 jobs (the six objects in one and in 32 frames) at 40 x 48 and 96 x 128, windows
    by ops.mesh_windows at each object's ground-truth pose turned 2 degrees and moved 3 mm; beside the same maps COMPOSED from
    ops.render_depth (one scene per job under the window's camera, return_z and return_face) and torch gathers and elementwise
    float32 operations in the kernel's order (composed below); `equal_bytes` says whether z, vertex and normal came out the same.
  * refine: pose.DenseModelRefine (windows, maps, rectangles, dense ICP) against today's model-based step on the same jobs:
    load_data_eval.clouds_from_poses (the ball crop and its 1024-point sample) + pose.IcpRefine; device time of the whole chain and
    the inliers per object of both.
  * track: host-clock milliseconds per frame of myEvaluater.track(init_from='previous') with a DenseModelRefine and with today's
    IcpRefine, under the instance masks, with the worst error against the ground truth over the sequence: translation in millimetres
    and the tilt of the model's y axis in degrees (three of the four shapes are solids of revolution about y: the angle about it is
    free).
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/meshmaps_time.py [--reps 10] [--warmup 3] [--out profiles/meshmaps_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from raycast_time import _median_ms  # noqa: E402


def composed(ms, camk, job_img, job_mesh, P, win, h, w, near=0.01):
    """ops.mesh_maps(normals='face') from ops.render_depth and torch: the winners of one scene per job under the window's camera, then
    the kernel's float32 arithmetic, one torch operation per rounding -> z, vertex, normal"""
    from tgpose_amd import ops
    J, dev = job_img.numel(), P.device
    K = camk[job_img.long()]
    Kp = torch.stack([K[:, 0] / win[:, 2], K[:, 1] / win[:, 3], (K[:, 2] - win[:, 0]) / win[:, 2], (K[:, 3] - win[:, 1]) / win[:, 3]], 1).contiguous()
    r = ops.render_depth(ms, torch.arange(J + 1, dtype=torch.int32, device=dev), job_mesh, torch.ones(J, dtype=torch.uint8, device=dev), P, Kp, h, w,
                         near=near, return_z=True, return_face=True)
    hit = r["face"] >= 0
    f = r["face"].clamp(min=0).long() + ms.fptr[job_mesh.long()].long()[:, None, None]
    idx = ms.faces[f].long() + ms.vptr[job_mesh.long()].long()[:, None, None, None]                 # (J,h,w,3)
    p = ms.verts[idx]                                                                               # (J,h,w,3 corners,3)
    T = P[:, None, None, None]                                                                      # (J,1,1,1,3,4)
    c = [((T[..., q, 0] * p[..., 0] + T[..., q, 1] * p[..., 1]) + T[..., q, 2] * p[..., 2]) + T[..., q, 3] for q in range(3)]
    kp = Kp[:, None, None, None]
    X = torch.round((kp[..., 0] * (c[0] / c[2]) + kp[..., 2]) * 256.0).long()
    Y = torch.round((kp[..., 1] * (c[1] / c[2]) + kp[..., 3]) * 256.0).long()
    iz = 1.0 / c[2]
    orient = lambda ax, ay, bx, by, cx, cy: (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    area = orient(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], X[..., 2], Y[..., 2])
    order = torch.where((area < 0)[..., None], torch.tensor([0, 2, 1], device=dev), torch.tensor([0, 1, 2], device=dev))
    X, Y, iz = X.gather(-1, order), Y.gather(-1, order), iz.gather(-1, order)
    p = p.gather(-2, order[..., None].expand(-1, -1, -1, -1, 3))
    sy, sx = torch.meshgrid(torch.arange(h, device=dev) * 256, torch.arange(w, device=dev) * 256, indexing="ij")
    fa = area.abs().float()
    z = torch.where(hit, r["z"], torch.zeros_like(r["z"]))
    b = [((orient(X[..., (k + 1) % 3], Y[..., (k + 1) % 3], X[..., (k + 2) % 3], Y[..., (k + 2) % 3], sx, sy).float() / fa) * iz[..., k]) * z for k in range(3)]
    vert = torch.stack([(b[0] * p[..., 0, a] + b[1] * p[..., 1, a]) + b[2] * p[..., 2, a] for a in range(3)], -1)
    u, v = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :]
    n = torch.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)
    s = torch.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    hit = hit & (s > 0) & (s < float("inf"))
    n = n / s[..., None]
    Tj = P[:, None, None]
    m = [(Tj[..., q, 0] * n[..., 0] + Tj[..., q, 1] * n[..., 1]) + Tj[..., q, 2] * n[..., 2] for q in range(3)]
    kj = Kp[:, None, None]
    rx, ry = ((sx // 256).float() - kj[..., 2]) / kj[..., 0], ((sy // 256).float() - kj[..., 3]) / kj[..., 1]
    n = torch.where((((m[0] * rx + m[1] * ry) + m[2]) > 0)[..., None], -n, n)
    zero = torch.zeros((), device=dev)
    return dict(z=torch.where(hit, z, zero), vertex=torch.where(hit[..., None], vert, zero), normal=torch.where(hit[..., None], n, zero))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshmaps_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("meshmaps_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tests import icp_ref
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": bct.H, "W": bct.W, "gate_m": 0.01,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so"}
    K = lde.CAMERA_INTRINSICS
    ms = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    res["mesh_faces"] = ms.n_faces[:4]
    sc = bct.scenes(a.frames)
    rendered = synthetic.render_scenes(ms, sc, K, bct.H, bct.W)
    frames = [synthetic.scene_frame(ms, sc, rendered, i) for i in range(a.frames)]
    seq = [dict(depth=fr["depth"], inst_mask=rendered["mask"][i]) for i, fr in enumerate(frames)]
    RTs = np.stack([fr["gt_RTs"][:6] for fr in frames]).astype(np.float32)
    scales = np.stack([fr["gt_scales"][:6] for fr in frames]).astype(np.float32)
    depth_all, inst_all, camk_all = lde._depth_frames(seq, K, dev)
    inst_all = inst_all.view(torch.uint8)
    start = RTs.astype(np.float64).copy()
    start[:, :, :3, :3] = icp_ref.rot([1, 2, -1], 2.0) @ start[:, :, :3, :3]
    start[:, :, :3, 3] += 0.003 * np.array([2.0, -1.0, 2.0]) / 3.0
    models = ops.IcpModels.from_meshset(ms, [0, 1, 2, 3], 1024)
    res["mesh_maps"], res["refine"] = [], []
    for S in (1, a.frames):
        J = 6 * S
        job_img = torch.from_numpy(np.repeat(np.arange(S), 6).astype(np.int32)).to(dev)
        job_mesh = torch.from_numpy(np.tile(np.arange(6) % 4, S).astype(np.int32)).to(dev)
        vals = torch.from_numpy(np.tile(np.arange(1, 7), S).astype(np.uint8)).to(dev)
        rts = torch.from_numpy(start[:S].reshape(J, 4, 4).astype(np.float32)).to(dev)
        scl = torch.from_numpy(scales[:S].reshape(J, 3)).to(dev)
        depth, inst, camk = depth_all[:S].contiguous(), inst_all[:S].contiguous(), camk_all[:S].contiguous()
        P = pose.verify_job_pose(rts)
        for h, w in ((40, 48), (96, 128)):
            win = ops.mesh_windows(ms, camk, job_img, job_mesh, P, h, w, bct.H, bct.W)
            run = lambda: ops.mesh_maps(ms, camk, job_img, job_mesh, P, win, h, w)
            comp = lambda: composed(ms, camk, job_img, job_mesh, P, win, h, w)
            got, want = run(), comp()
            equal = all(bool(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))) for k in ("z", "vertex", "normal"))
            row = dict(jobs=J, h=h, w=w, launches=3, mean_hits=float(got["count"].float().mean()), equal_bytes=equal,
                       **_median_ms(run, a.warmup, a.reps, 20 if S == 1 else 5))
            crow = _median_ms(comp, a.warmup, a.reps, 5 if S == 1 else 2)
            row.update(composed_median_ms=crow["median_ms"], composed_min_ms=crow["min_ms"], composed_max_ms=crow["max_ms"],
                       composed_over_kernel=crow["median_ms"] / row["median_ms"])
            res["mesh_maps"].append(row)
            print(json.dumps(row), flush=True)
        dense = pose.DenseModelRefine(ms, job_mesh, 0.01)
        sparse = pose.IcpRefine(models, job_mesh, 0.01, mode="plane")
        crop = dict(depth=depth, inst_mask=inst)
        ids = vals.cpu().tolist()

        def today():
            pts = lde.clouds_from_poses(crop, job_img, rts, scl, bct.RATIO, K, n_pts=bct.N_PTS, sampler="device", masks=ids, seed=1, device=dev)[0]
            return sparse(pts, rts)
        for name, fn in (("DenseModelRefine", lambda: dense(depth, rts, camk, job_img, mask=inst, job_mask_val=vals)),
                         ("clouds_from_poses + IcpRefine", today)):
            out = fn()
            info = out[1].cpu().numpy()
            row = dict(path=name, jobs=J, ok=int((info[:, 0] == 0).sum()), mean_inliers=float(info[:, 1].mean()), inliers_first_frame=info[:6, 1].tolist(),
                       **_median_ms(fn, a.warmup, a.reps, 10 if S == 1 else 3))
            res["refine"].append(row)
            print(json.dumps(row), flush=True)
    init = dict(class_ids=frames[0]["gt_class_ids"][:6], RTs=frames[0]["gt_RTs"][:6], scales=frames[0]["gt_scales"][:6], inst_ids=[1, 2, 3, 4, 5, 6])
    net = PoseNet9D().to(dev).eval()
    net.load_state_dict(seeded_state_dict(0))
    ev = myEvaluater(net, sampler="device", seed=1)
    six = [o % 4 for o in range(6)]
    res["track"] = []
    for name, ratio, refine in (("previous + DenseModelRefine", None, pose.DenseModelRefine(ms, six, 0.01)),
                                ("previous + IcpRefine (today)", bct.RATIO, pose.IcpRefine(models, six, 0.01, mode="plane"))):
        go = lambda frames_: ev.track(frames_, init, K, ratio, refine=refine, init_from="previous")
        go(seq[:4])
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            out = go(seq)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t_0) * 1e3 / len(seq))
        got = np.stack([o["pred_RTs"] for o in out]).astype(np.float64)
        mm = 1000.0 * np.linalg.norm(got[:, :, :3, 3] - RTs[:, :, :3, 3], axis=-1)
        ya, yb = got[:, :, :3, 1], RTs[:, :, :3, 1].astype(np.float64)
        tilt = np.rad2deg(np.arccos(np.clip((ya * yb).sum(-1) / (np.linalg.norm(ya, axis=-1) * np.linalg.norm(yb, axis=-1)), -1.0, 1.0)))
        row = dict(path=name, frames=len(seq), objects=6, host_clock=True, ms_per_frame=statistics.median(t), min_ms=min(t), max_ms=max(t),
                   icp_ok_share=float(np.mean([(o["icp_status"] == 0).mean() for o in out])), mean_inliers=float(np.mean([o["icp_inliers"].mean() for o in out])),
                   worst_translation_mm=float(mm.max()), worst_y_tilt_deg=float(tilt.max()), worst_translation_mm_per_object=mm.max(0).tolist(),
                   worst_y_tilt_deg_per_object=tilt.max(0).tolist())
        res["track"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, default=float)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
