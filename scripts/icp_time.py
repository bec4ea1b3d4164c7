"""Times ICP refinement (ops.icp_refine: csrc/icp.hip, ONE launch for all jobs and all iterations).  Writes profiles/icp_time.json:

  * icp_refine: device time of one call for J = 6 and 192 jobs, n = 512 and 1024 source points, m = 1024 and 2048 model points, in
    both modes, with a fixed number of iterations (--iters, tolerances 0, so the work is known: iters + 1 correspondence passes of
    n x m pairs and iters solves per job), inputs on the device.  The model is two boxes joined off-centre, the sources are images
    of other samples of it under a pose 2 degrees / 3 mm from the start, the gate is 2 cm.
  * torch_composition: the same iterations composed from torch operations on the same device -- torch_icp below: cdist, argmin,
    gathers, masked sums, and torch.linalg.svd (point) or torch.linalg.solve (plane) in float64 -- batched over the jobs; its poses
    are compared with the kernel's (max_pose_diff; float32 search in another arithmetic: agreement, not equality).
  * track_previous: milliseconds per frame, host clock, of myEvaluater.track(refine=..., init_from='previous') on the six-object
    rendered scene of scripts/ball_crop_time.py (no forward runs), beside track with the network and no refinement.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/icp_time.py [--reps 5] [--warmup 2] [--iters 10] [--out profiles/icp_time.json]
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


def _median_ms(fn, warmup, reps, calls):
    times = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(s.elapsed_time(e) / calls)
    return dict(calls_per_window=calls, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a) * np.deg2rad(deg)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = np.linalg.norm(a)
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)


def two_boxes():
    from tgpose_amd.datasets import shapes
    v1, f1 = shapes.box((0.9, 0.5, 0.6))
    v2, f2 = shapes.box((0.4, 0.35, 0.3))
    v2 = v2 + np.array([0.2, 0.425, 0.1], dtype=np.float32)
    return np.concatenate([v1, v2]).astype(np.float32), np.concatenate([f1, f2 + len(v1)]).astype(np.int32)


def torch_icp(model, src, R, t, s, gate, mode, iters):
    """`iters` ICP iterations of J jobs against ONE model (m,6), composed from torch operations: what ops.icp_refine replaces.
    src (J,n,3), R (J,3,3), t (J,3), s (J,) float32 on the device -> (R, t) float64.  The search is float32 (cdist), sums and
    solves float64, as in the kernel; there is no inlier floor, no status and no early stop."""
    y, nrm = model[:, :3], model[:, 3:6].double()
    R, t, s64 = R.double(), t.double(), s.double()
    p = src.double()
    J = src.shape[0]
    for _ in range(iters):
        q = (torch.einsum("jba,jnb->jna", R, p - t[:, None, :]) / s64[:, None, None]).float()
        d = torch.cdist(q, y[None].expand(J, -1, -1))
        dist, idx = d.min(2)
        w = (dist <= (gate / s)[:, None]).double()
        yj = y[idx].double()
        cnt = w.sum(1)
        if mode == "point":
            pbar, ybar = (w[:, :, None] * p).sum(1) / cnt[:, None], (w[:, :, None] * yj).sum(1) / cnt[:, None]
            S = torch.einsum("jn,jna,jnb->jab", w, p - pbar[:, None], yj - ybar[:, None])
            U, _, Vh = torch.linalg.svd(S)
            D = torch.ones(J, 3, dtype=torch.float64, device=src.device)
            D[:, 2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vh))
            R = U @ torch.diag_embed(D) @ Vh
            t = pbar - s64[:, None] * torch.einsum("jab,jb->ja", R, ybar)
        else:
            nj = nrm[idx]
            q64 = q.double()
            rows = torch.cat([torch.linalg.cross(q64, nj), nj], 2)
            r = ((q64 - yj) * nj).sum(2)
            A = torch.einsum("jn,jna,jnb->jab", w, rows, rows)
            b = torch.einsum("jn,jna,jn->ja", w, rows, r)
            A = A + torch.eye(6, dtype=torch.float64, device=src.device) * (1e-9 * torch.diagonal(A, dim1=1, dim2=2).sum(1) / 6.0)[:, None, None]
            x = torch.linalg.solve(A, -b)
            E = torch.linalg.matrix_exp(torch.linalg.cross(x[:, None, :3].expand(-1, 3, -1), -torch.eye(3, dtype=torch.float64, device=src.device)[None]))
            R = R @ E.transpose(1, 2)
            t = t - s64[:, None] * torch.einsum("jab,jb->ja", R, x[:, 3:])
    return R, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("icp_time.py measures on a GPU; none is visible")
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "iters": a.iters,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so.  One icp_refine call = `iters` iterations + the final pass for every job"}
    ms = ops.MeshSet([two_boxes()], device=dev)
    dense = ops.mesh_sample(ms, [0, 0], 2048, keys=[0, 1], seed=3, normals=True, check_status=True)["points"]
    Rg, tg, sg = _rot([0.3, -0.5, 0.8], 140.0), np.array([0.05, -0.03, 0.8]), 0.16
    img = (sg * dense[1, :, :3].double().cpu().numpy() @ Rg.T + tg).astype(np.float32)
    R0 = (Rg @ _rot([1.0, 2.0, -1.0], 2.0)).astype(np.float32)
    t0 = (tg + 0.003 * np.array([2.0, -1.0, 2.0]) / 3.0).astype(np.float32)
    res["icp_refine"], res["torch_composition"] = [], []
    for J in (6, 192):
        for n in (512, 1024):
            for m in (1024, 2048):
                models = ops.IcpModels(dense[:1, :m].contiguous())
                src = torch.from_numpy(np.stack([np.roll(img, -7 * j, 0)[:n] for j in range(J)])).to(dev)
                R = torch.from_numpy(R0).to(dev).repeat(J, 1, 1)
                t = torch.from_numpy(t0).to(dev).repeat(J, 1)
                s = torch.full((J,), sg, device=dev)
                gate = torch.full((J,), 0.02, device=dev)
                jm = torch.zeros(J, dtype=torch.int32, device=dev)
                for mode in ("plane", "point"):
                    def run():
                        return ops.icp_refine(models, jm, src, R, t, s, gate, mode=mode, iters=a.iters, tol_rot=0.0, tol_trans=0.0)
                    Rk, tk, _, info, rmse = run()
                    info = info.cpu().numpy()
                    assert (info[:, 0] == 0).all() and (info[:, 2] == a.iters).all()
                    row = dict(jobs=J, n=n, m=m, mode=mode, launches=1, iters=a.iters, mean_inliers=float(info[:, 1].mean()),
                               pairs_per_call=int(J) * n * m * (a.iters + 1), **_median_ms(run, a.warmup, a.reps, 20 if J <= 6 else 5))
                    row["us_per_iteration"] = row["median_ms"] * 1e3 / (a.iters + 1)
                    res["icp_refine"].append(row)
                    print(json.dumps(row), flush=True)

                    def comp():
                        return torch_icp(models.points_normals[0], src, R, t, s, gate, mode, a.iters)
                    Rt, tt = comp()
                    crow = dict(jobs=J, n=n, m=m, mode=mode, iters=a.iters,
                                max_pose_diff=float(max((Rt - Rk.double()).abs().max(), (tt - tk.double()).abs().max())),
                                **_median_ms(comp, a.warmup, a.reps, 2))
                    crow["ratio_to_kernel"] = crow["median_ms"] / row["median_ms"]
                    res["torch_composition"].append(crow)
                    print(json.dumps(crow), flush=True)
    # the model-based tracker on ball_crop_time's six-object frames
    import ball_crop_time as bct
    K = lde.CAMERA_INTRINSICS
    ms6 = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    sc = bct.scenes(a.frames)
    rendered = synthetic.render_scenes(ms6, sc, K, bct.H, bct.W)
    frames = [synthetic.scene_frame(ms6, sc, rendered, i) for i in range(a.frames)]
    seq = [dict(depth=fr["depth"], inst_mask=rendered["mask"][i]) for i, fr in enumerate(frames)]
    init = dict(class_ids=frames[0]["gt_class_ids"][:6], RTs=frames[0]["gt_RTs"][:6], scales=frames[0]["gt_scales"][:6], inst_ids=[1, 2, 3, 4, 5, 6])
    net = PoseNet9D().to(dev).eval()
    net.load_state_dict(seeded_state_dict(0))
    refine = pose.IcpRefine(ops.IcpModels.from_meshset(ms6, [0, 1, 2, 3], 1024), [o % 4 for o in range(6)], 0.01, mode="plane")
    ev = myEvaluater(net, sampler="device", seed=1)
    res["track_previous"] = []
    for name, kw in (("previous+icp", dict(refine=refine, init_from="previous")), ("net", {}), ("net+icp", dict(refine=refine))):
        ev.track(seq[:4], init, K, bct.RATIO, **kw)
        torch.cuda.synchronize()
        t_0 = time.perf_counter()
        out = ev.track(seq, init, K, bct.RATIO, **kw)
        torch.cuda.synchronize()
        row = dict(path=name, frames=len(seq), objects=6, n_pts=bct.N_PTS, host_clock=True, ms_per_frame=(time.perf_counter() - t_0) * 1e3 / len(seq))
        if "icp_status" in out[0]:
            row.update(icp_ok_share=float(np.mean([(o["icp_status"] == 0).mean() for o in out])),
                       mean_inliers=float(np.mean([o["icp_inliers"].mean() for o in out])))
        res["track_previous"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
