"""Times the BOP pose errors (ops.pose_errors: csrc/poseerr.hip, two launches; ops.pose_vsd: csrc/vsd.hip, four launches, no frame
written).  Writes profiles/bop_time.json:

  * pose_errors / pose_vsd: device time of one call at 480 x 640 on the scenes of scripts/verify_time.py (the six-object rendered
    scene of scripts/ball_crop_time.py): every object's ground-truth pose against an estimate 3 mm and half a degree off, J = 6 jobs
    on one frame and 32 x 6 = 192 jobs over 32 frames; the point errors with symmetry groups of 1 and of 315 transforms (BOP's
    step 0.01 about the lathe axis), VSD with BOP's ten taus.
  * composed: the only routes to the same numbers without the kernels, in the same run -- float64 torch.cdist and broadcasting for
    the point errors (`torch_point_errors`, jobs batched per mesh once, outside the timed calls; its largest difference from the kernel is recorded: the orders
    of the sums differ, and torch.cdist in its default mode takes the distances from a matrix product), ops.render_depth with one
    scene per pose (2 J full frames written) and torch operations for VSD (`torch_vsd`; counts, within and err are compared for
    equality).
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/bop_time.py [--reps 10] [--warmup 3] [--out profiles/bop_time.json]
"""
import argparse
import json
import os
import statistics
import sys

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


def point_batches(ms, groups, job_mesh, job_sym, device):
    """The jobs of host lists job_mesh / job_sym batched per (mesh, group): a list of (job indices on the device, the mesh's vertices
    and the group's transforms as float64).  Host work and uploads, done once, outside what is timed."""
    start = np.concatenate([[0], np.cumsum(ms.n_verts)])
    out = []
    for m, g in sorted(set(zip(job_mesh, job_sym))):
        idx = torch.tensor([j for j in range(len(job_mesh)) if (job_mesh[j], job_sym[j]) == (m, g)], device=device)
        out.append((idx, ms.verts[start[m]:start[m + 1]].double(), groups[g].double()))
    return out


def torch_point_errors(batches, pose_est, pose_gt, camk):
    """ops.pose_errors' err (J,4) with float64 torch operations over point_batches' batches: torch.cdist for adi, a
    (jobs, Q, P, 3) broadcast for mssd and mspd.  Device work only: nothing here visits the host."""
    J = pose_est.shape[0]
    out = torch.empty(J, 4, dtype=torch.float64, device=pose_est.device)
    E, G, K = pose_est.double(), pose_gt.double(), camk.double()
    apply = lambda T, p: p @ T[..., :3].transpose(-1, -2) + T[..., None, :, 3]
    proj = lambda x, k: torch.stack([k[..., 0] * (x[..., 0] / x[..., 2]) + k[..., 2], k[..., 1] * (x[..., 1] / x[..., 2]) + k[..., 3]], -1)
    for idx, p, group in batches:
        e, gt = apply(E[idx], p), apply(G[idx], p)                                           # (n, P, 3)
        out[idx, 0] = (e - gt).norm(dim=2).mean(1)
        out[idx, 1] = torch.cdist(e, gt).min(2).values.mean(1)
        sp = apply(group, p)                                                                 # (Q, P, 3)
        gs = apply(G[idx][:, None], sp[None])                                                # (n, Q, P, 3)
        out[idx, 2] = (e[:, None] - gs).norm(dim=3).max(2).values.min(1).values
        k = K[idx]
        out[idx, 3] = (proj(e, k[:, None])[:, None] - proj(gs, k[:, None, None])).norm(dim=3).max(2).values.min(1).values
    return out


def torch_vsd(ops, ms, depth, camk, job_img, job_mesh, pose_est, pose_gt, job_tau, delta, H, W):
    """ops.pose_vsd's outputs from ops.render_depth run with one scene per pose (2 J frames), with torch operations"""
    J = job_img.numel()
    wide = lambda t: t.view(torch.int16).to(torch.int32) & 0xffff
    idx = job_img.long()
    ren = ops.render_depth(ms, torch.arange(2 * J + 1, device=depth.device, dtype=torch.int32), torch.cat([job_mesh, job_mesh]),
                           torch.ones(2 * J, device=depth.device, dtype=torch.uint8), torch.cat([pose_est, pose_gt]),
                           torch.cat([camk[idx], camk[idx]]), H, W)
    d = wide(ren["depth"])
    d_e, d_g, d_o = d[:J], d[J:], wide(depth)[idx]
    vis = lambda x: (x > 0) & ((d_o == 0) | (x - d_o <= delta))
    vg = vis(d_g)
    ve = vis(d_e) | (vg & (d_e > 0))
    inter, union = vg & ve, vg | ve
    dropped = ren["dropped"].sum(1)
    counts = torch.stack([x.sum((1, 2)) for x in (d_g > 0, d_e > 0, vg, ve, inter, union)] + [dropped[J:], dropped[:J]], 1).to(torch.int32)
    diff = (d_g - d_e).abs()
    within = torch.stack([(inter & (diff < job_tau[:, k, None, None])).sum((1, 2)) for k in range(job_tau.shape[1])], 1).to(torch.int32)
    un = counts[:, 5:6]
    err = torch.where(un > 0, (un - within).float() / un.clamp(min=1).float(), torch.ones((), device=depth.device))
    return counts, within, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bop_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bop_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluation import bop
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": bct.H, "W": bct.W, "delta": 15,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after `warmup`"}
    K = lde.CAMERA_INTRINSICS
    ms = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    res["mesh_vertices"] = ms.n_verts[:4]
    sc = bct.scenes(a.frames)
    rendered = synthetic.render_scenes(ms, sc, K, bct.H, bct.W)
    frames = [synthetic.scene_frame(ms, sc, rendered, i) for i in range(a.frames)]
    depth_all = torch.from_numpy(np.stack([fr["depth"] for fr in frames]).view(np.int16)).to(dev)
    camk_all = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]] * a.frames, dtype=torch.float32, device=dev)
    RTs = torch.from_numpy(np.stack([fr["gt_RTs"][:6] for fr in frames]).astype(np.float32)).to(dev)           # (frames, 6, 4, 4)
    half = np.deg2rad(0.5)
    off = torch.tensor([[np.cos(half), -np.sin(half), 0, 0.003], [np.sin(half), np.cos(half), 0, -0.002], [0, 0, 1, 0.004], [0, 0, 0, 1]],
                       dtype=torch.float32, device=dev)
    lathe = bop.symmetry_transformations(dict(symmetries_continuous=[dict(axis=[0, 1, 0], offset=[0, 0, 0])]), 0.01)
    groups = [ops.SymmetrySet.identity(), lathe.astype(np.float32)]
    symset = ops.SymmetrySet(groups, device=dev)
    groups_dev = [torch.from_numpy(g).to(dev) for g in groups]
    diam = bop.diameter(ms)
    res["pose_errors"], res["pose_errors_composed"], res["pose_vsd"], res["pose_vsd_composed"] = [], [], [], []
    for S in (1, a.frames):
        J = 6 * S
        depth, camk = depth_all[:S].contiguous(), camk_all[:S].contiguous()
        job_img = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(6).contiguous()
        mesh_list = [o % 4 for o in range(6)] * S
        job_mesh = torch.tensor(mesh_list, dtype=torch.int32, device=dev)
        gt44 = RTs[:S].reshape(J, 4, 4)
        est44 = off[None] @ gt44                                                              # moved in the camera's frame
        pose_gt, pose_est = gt44[:, :3, :4].contiguous(), est44[:, :3, :4].contiguous()
        camk_job = camk[job_img.long()].contiguous()
        for g in (0, 1):
            sym_list = [g] * J
            job_sym = torch.tensor(sym_list, dtype=torch.int32, device=dev)

            batches = point_batches(ms, groups_dev, mesh_list, sym_list, dev)

            def run():
                return ops.pose_errors(ms, job_mesh, pose_est, pose_gt, symset, job_sym, camk_job)

            def comp():
                return torch_point_errors(batches, pose_est, pose_gt, camk_job)
            out, want = run(), comp()
            row = dict(jobs=J, frames=S, symmetries=len(groups[g]), launches=2, status_all_zero=bool((out["status"] == 0).all()),
                       mean_err=dict(zip(ops.POSE_ERRORS, out["err"].mean(0).tolist())), **_median_ms(run, a.warmup, a.reps, 20 if S == 1 else 5))
            res["pose_errors"].append(row)
            print(json.dumps(row), flush=True)
            crow = dict(jobs=J, frames=S, symmetries=len(groups[g]), max_abs_difference=float((out["err"] - want).abs().max()),
                        **_median_ms(comp, a.warmup, a.reps, 5 if S == 1 else 2))
            crow["equal_within_1e-9"] = crow["max_abs_difference"] <= 1e-9
            crow["ratio_to_kernel"] = crow["median_ms"] / row["median_ms"]
            res["pose_errors_composed"].append(crow)
            print(json.dumps(crow), flush=True)
        scale = torch.linalg.det(gt44[:, :3, :3].double()).abs().pow(1.0 / 3.0)
        job_tau = bop.vsd_taus(diam[job_mesh.long()] * scale * 1000.0)

        def run_v():
            return ops.pose_vsd(ms, depth, camk, job_img, job_mesh, pose_est, pose_gt, job_tau)

        def comp_v():
            return torch_vsd(ops, ms, depth, camk, job_img, job_mesh, pose_est, pose_gt, job_tau, 15, bct.H, bct.W)
        out, (wc, ww, we) = run_v(), comp_v()
        counts = out["counts"].cpu().numpy()
        row = dict(jobs=J, frames=S, taus=10, launches=4, rendered_pixels=int(counts[:, :2].sum()), frame_pixels=2 * J * bct.H * bct.W,
                   mean_err=float(out["err"].mean()), **_median_ms(run_v, a.warmup, a.reps, 20 if S == 1 else 5))
        res["pose_vsd"].append(row)
        print(json.dumps(row), flush=True)
        crow = dict(jobs=J, frames=S, counts_equal=bool(torch.equal(out["counts"], wc)), within_equal=bool(torch.equal(out["within"], ww)),
                    err_equal=bool(torch.equal(out["err"], we)), **_median_ms(comp_v, a.warmup, a.reps, 5 if S == 1 else 2))
        crow["ratio_to_kernel"] = crow["median_ms"] / row["median_ms"]
        res["pose_vsd_composed"].append(crow)
        print(json.dumps(crow), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
