"""Times the distance-field pose search (ops.pose_search: csrc/search.hip, two launches).  Writes profiles/search_time.json:

  * pose_search: device time of one call on clouds drawn from the model (icp_ref.two_boxes, 2048 samples) under random rotations:
    6 and 192 jobs, n = 128 / 512 points, R = 504 / 1944 rotations (42 / 162 views x 12 in-plane), K = 5 / 8 at stride 2 (1331 / 4913
    shifts), G = 32 / 48 -- the base case and one change at a time, then the large job counts.  `lookups` = jobs x R x shifts x n.
  * composed: the same search from torch operations on the same device -- the rotation as broadcast products in the kernel's
    operation order (a batched matmul rounds differently and would miss the integers at voxel faces), floor, one gather on the padded
    field tensor per block of rotations, sum, min on a (cost, shift) key, topk on a (cost, rotation) key.  Its cost, rot and shift
    are compared with the kernel's (integers_equal) in the same run.
  * field_build: device time of ops.DistanceFields' launch, per G.
  * chain: pose.ModelSearch on the three segments of icp_ref.table_scene frame 0 at 240 x 320 (32 segmenter slots, 16 candidates
    each): search alone, search + ICP, search + ICP + verify, and myEvaluater.acquire_models end to end on the host's clock.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/search_time.py [--reps 10] [--warmup 3] [--out profiles/search_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def torch_search(fields, job_model, clouds, anchors, scales, Rs, K, stride, top, block=32):
    """ops.pose_search's cost, rot and shift (J, top) from torch operations; finite clouds, every row live"""
    G, cap, dev = fields.G, fields.cap, clouds.device
    reach = K * stride
    pad = 2 * reach + 1
    S = G + 2 * pad
    big = torch.nn.functional.pad(fields.field.to(torch.int32), (pad,) * 6, value=cap).reshape(len(fields), -1)
    d = torch.arange(-K, K + 1, device=dev) * stride
    lin_d = ((d[:, None, None] * S + d[None, :, None]) * S + d[None, None, :]).reshape(-1)          # (D,) in shift-index order
    D, R = lin_d.numel(), Rs.shape[0]
    cost, rot, shift = [], [], []
    for j in range(clouds.shape[0]):
        m = int(job_model[j])
        voxel = fields.meta[m, 3]
        inv = (1.0 / (scales[j].double() * voxel.double())).float()
        e = clouds[j] - anchors[j][None, :]
        keys = []
        for lo in range(0, R, block):
            Rb = Rs[lo:lo + block]
            u = (Rb[:, None, 0, :] * e[None, :, 0, None] + Rb[:, None, 1, :] * e[None, :, 1, None]) + Rb[:, None, 2, :] * e[None, :, 2, None]
            b = torch.floor(torch.clamp(u * inv + float(G // 2), -512.0, 511.0)).long().clamp(-reach - 1, G + reach) + pad
            lin = (b[:, :, 0] * S + b[:, :, 1]) * S + b[:, :, 2]                                    # (Rb, n)
            c = big[m][lin[:, :, None] + lin_d[None, None, :]].sum(1)                               # (Rb, D)
            keys.append((c.long() * D + torch.arange(D, device=dev)[None, :]).min(1).values)
        key = torch.cat(keys)
        c, sx = key // D, key % D
        best = torch.topk(c * R + torch.arange(R, device=dev), top, largest=False).values
        cost.append(best // R), rot.append(best % R), shift.append(sx[best % R])
    return torch.stack(cost).int(), torch.stack(rot).int(), torch.stack(shift).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("search_time.py measures on a GPU; none is visible")
    from tests import icp_ref, plane_cases as pc
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.tools.lynne_lib import view_sampler
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so"}
    ms = ops.MeshSet(pc.meshes(), device=dev)
    models = ops.IcpModels.from_meshset(ms, [0], 2048)
    grids = {42: torch.from_numpy(view_sampler.rotation_grid(42, 12)).to(dev), 162: torch.from_numpy(view_sampler.rotation_grid(162, 12)).to(dev)}
    fields, res["field_build"] = {}, []
    for G in (32, 48):
        fields[G] = ops.DistanceFields(models, G=G, cap=32)
        f = fields[G]
        args = ops._lib.FieldArgs(models=ops._p(models.points_normals), model_count=None, M=1, m_cap=models.m_cap, meta=ops._p(f.meta),
                                  thresholds=ops._p(f.thresholds), G=G, cap=32, field=ops._p(f.field))
        build = lambda: ops.check(ops._lib.lib().tgp_field_build(ops.ctypes.byref(args), ops._stream(f.field)), "tgp_field_build")
        row = dict(G=G, model_points=models.m_cap, **_median_ms(build, a.warmup, a.reps, 20))
        res["field_build"].append(row)
        print(json.dumps(row), flush=True)

    r = np.random.RandomState(2)
    y = models.points_normals[0, :, :3].cpu().numpy().astype(np.float64)

    def jobs(J, n):
        clouds = np.empty((J, n, 3), np.float32)
        for j in range(J):
            R = icp_ref.rot(r.randn(3), r.uniform(0, 180))
            clouds[j] = 0.15 * (y[r.randint(0, len(y), n)] + r.randn(n, 3) * 0.003) @ R.T + [0.0, 0.0, 0.8] + r.randn(3) * 0.05
        c = torch.from_numpy(clouds).to(dev)
        return c, pose.cloud_anchors(c), torch.full((J,), 0.15, device=dev), torch.zeros(J, dtype=torch.int32, device=dev)

    base = dict(jobs=6, n=128, views=42, K=5, G=32)
    cases = [base] + [dict(base, **ch) for ch in (dict(n=512), dict(views=162), dict(K=8), dict(G=48))]
    cases += [dict(base, jobs=192), dict(base, jobs=192, n=512), dict(base, jobs=192, G=48), dict(base, jobs=192, views=162, K=8, n=512, G=48)]
    res["pose_search"], res["composed"] = [], []
    for c in cases:
        clouds, anchors, scales, jm = jobs(c["jobs"], c["n"])
        Rs, f = grids[c["views"]], fields[c["G"]]
        run = lambda: ops.pose_search(f, jm, clouds, None, anchors, scales, Rs, K=c["K"], stride=2, top=16)
        out = run()
        lookups = c["jobs"] * Rs.shape[0] * (2 * c["K"] + 1) ** 3 * c["n"]
        heavy, huge = lookups > 1e10, lookups > 2e11
        row = dict(c, R=Rs.shape[0], shifts=(2 * c["K"] + 1) ** 3, launches=2, lookups=lookups,
                   **_median_ms(run, 1 if huge else a.warmup, 3 if huge else a.reps, 1 if huge else 2 if heavy else 10))
        row["lookups_per_ns"] = lookups / (row["median_ms"] * 1e6)
        res["pose_search"].append(row)
        print(json.dumps(row), flush=True)
        if huge:                                   # the composition would take minutes: the kernel's row stands alone
            continue
        comp = lambda: torch_search(f, jm, clouds, anchors, scales, Rs, c["K"], 2, 16)
        want = comp()
        crow = dict(c, integers_equal=bool(all(torch.equal(out[k], w) for k, w in zip(("cost", "rot", "shift"), want))),
                    **_median_ms(comp, 1, 3 if heavy else a.reps, 1))
        crow["ratio_to_kernel"] = crow["median_ms"] / row["median_ms"]
        res["composed"].append(crow)
        print(json.dumps(crow), flush=True)

    # the chain on the table scene
    K = pc.K
    scenes = [icp_ref.table_scene(0, gap=0.0)]
    rendered = synthetic.render_scenes(ms, scenes, K, pc.H, pc.W)
    frame = dict(depth=rendered["depth"][0])
    refine = pose.IcpRefine(models, [0], 0.01, mode="plane")
    verify = pose.Verify(ms, [0], tau=5)
    net = PoseNet9D().to(dev).eval()
    net.load_state_dict(seeded_state_dict(0))
    ev = myEvaluater(net, sampler="device", seed=pc.SEED)
    sup, sg = pose.SupportPlane(), pose.Segmenter()
    from tgpose_amd.evaluation import load_data_eval as lde
    depth, _, camk = lde._depth_frames([frame], K, dev)
    cut = sup(depth, camk, [0], ev.seed)[0]
    seg = sg(cut, camk)
    pts, _ = lde.clouds_from_segments(cut, seg, camk, n_pts=128, sampler="device", seed=ev.seed)
    M = sg.max_segments
    sc = torch.full((M,), 0.15, device=dev)
    jm = torch.zeros(M, dtype=torch.int32, device=dev)
    vals = torch.arange(1, M + 1, device=dev).to(torch.uint8)
    res["chain"] = []
    stages = (("search", None, None), ("search+icp", refine, None), ("search+icp+verify", refine, verify))
    for name, rf, vf in stages:
        search = pose.ModelSearch(fields[32], models, grids[42], K=5, stride=2, top=16, refine=rf, verify=vf)
        run = lambda: search(pts, jm, sc, depth=cut, camk=camk, mask=seg.labels, job_mask_val=vals)
        row = dict(stage=name, slots=M, segments=int(seg.info[0, 1]), candidates=16, n_pts=128, **_median_ms(run, a.warmup, a.reps, 5))
        res["chain"].append(row)
        print(json.dumps(row), flush=True)
    t = []
    for k in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t_0 = time.perf_counter()
        ev.acquire_models(frame, search, 0, 0.15, K, support=sup, segmenter=sg, n_pts=128)
        torch.cuda.synchronize()
        if k >= a.warmup:
            t.append((time.perf_counter() - t_0) * 1e3)
    row = dict(stage="acquire_models", host_clock=True, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
    res["chain"].append(row)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
