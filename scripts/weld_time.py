"""Times the indexed meshes from volumes (ops.tsdf_mesh_indexed, ops.mesh_vertex_normals, ops.tsdf_meshset(indexed=True): csrc/weld.hip)
on scripts/tsdf_time.py's scene -- 32 frames of 480 x 640 of six objects fused into six volumes of G = 64 -- and what the welded
and the decimated model cost and give downstream.  Writes profiles/weld_time.json:

  * mesh: device time of tsdf_mesh_indexed on one volume with both caps given (mark, prefix sum, count, prefix sum, vertices, faces;
    nothing read back) against tsdf_mesh with a face_cap on the same volume; of the same with cluster=2 (it reads the cell count
    back and torch.unique sizes its result, so its windows include those waits); and of mesh_vertex_normals on the welded mesh.
  * meshset: host-clock time of tsdf_meshset over the six volumes: soup, indexed, indexed with cluster=2, in the same session.
  * scan: host-clock time of the whole of myEvaluater.scan with and without indexed.
  * counts: vertices and faces of the soup, welded and cluster=2 sets.
  * downstream, on those three sets: device time of ops.pose_errors (192 jobs; median of 3 single calls after 1), of
    evaluation.bop.diameter (computed afresh, one call) and of ops.pose_verify (192 jobs), and the mean verification score at the
    true poses.
  * two_boxes: tests/tsdf_cases.scan_downstream's setting (the model scanned at G = 32, the held-out view's pose found by
    pose.ModelSearch on the soup set): that pose's ADD / MSSD and the verification score at the true pose on the three sets, and ICP
    against IcpModels.from_vertices of the welded and the decimated set from 5 degrees / 10 mm off.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition.

    python scripts/weld_time.py [--reps 10] [--warmup 3] [--out profiles/weld_time.json]
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

from tsdf_time import _median_ms  # noqa: E402


def _host_ms(fn, warmup, reps):
    t = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t_0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r >= warmup:
            t.append((time.perf_counter() - t_0) * 1e3)
    return out, dict(host_clock=True, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weld_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("weld_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tests import icp_ref
    from tests import tsdf_cases as tc
    from tgpose_amd import PoseNet9D, ops, pose
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import bop
    from tgpose_amd.evaluation import load_data_eval as lde
    from tgpose_amd.tools.lynne_lib import view_sampler
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": bct.H, "W": bct.W, "G": a.G,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so"}
    # scripts/tsdf_time.py's scene
    K = lde.CAMERA_INTRINSICS
    shapes_ms = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    objects = ops.MeshSet([shapes.lathe(shapes.PROFILES[bct.NAMES[o % 4]], 24) for o in range(6)], device=dev)
    sc = bct.scenes(a.frames)
    rendered = synthetic.render_scenes(shapes_ms, sc, K, bct.H, bct.W)
    frames = [synthetic.scene_frame(shapes_ms, sc, rendered, i) for i in range(a.frames)]
    S, J = a.frames, 6 * a.frames
    depth = torch.from_numpy(np.stack([fr["depth"] for fr in frames]).view(np.int16)).to(dev)
    mask = torch.from_numpy(np.stack([rendered["mask"][i] for i in range(S)])).to(dev)
    camk = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]] * S, dtype=torch.float32, device=dev)
    RTs = np.stack([fr["gt_RTs"][:6] for fr in frames]).astype(np.float32)
    volumes = ops.TsdfVolumes.from_meshset(objects, a.G)
    trunc = 2000.0 * float(volumes.meta_host[:, 3].max()) * 0.14
    job_img = torch.from_numpy(np.repeat(np.arange(S), 6).astype(np.int32)).to(dev)
    job_model = torch.from_numpy(np.tile(np.arange(6), S).astype(np.int32)).to(dev)
    job_val = torch.from_numpy(np.tile(np.arange(1, 7), S).astype(np.uint8)).to(dev)
    job_pose = pose.verify_job_pose(torch.from_numpy(RTs.reshape(J, 4, 4)).to(dev))
    ops.tsdf_integrate(volumes, depth, camk, job_img, job_model, job_pose, trunc, mask=mask, job_mask_val=job_val)

    # one volume
    full = ops.tsdf_mesh_indexed(volumes, 0)
    nv, nf = int(full["n_verts"]), int(full["n_faces"])
    soup = ops.tsdf_mesh(volumes, 0, face_cap=nf)
    assert torch.equal(full["verts"][full["faces"].long()].reshape(-1, 3), soup["verts"])
    res["mesh"] = [dict(what="tsdf_mesh", faces=nf, read_back=False, **_median_ms(lambda: ops.tsdf_mesh(volumes, 0, face_cap=nf), a.warmup, a.reps, 10)),
                   dict(what="tsdf_mesh_indexed", verts=nv, faces=nf, read_back=False,
                        **_median_ms(lambda: ops.tsdf_mesh_indexed(volumes, 0, vert_cap=nv, face_cap=nf), a.warmup, a.reps, 10)),
                   dict(what="tsdf_mesh_indexed cluster=2", read_back=True,
                        **_median_ms(lambda: ops.tsdf_mesh_indexed(volumes, 0, vert_cap=nv, face_cap=nf, cluster=2), a.warmup, a.reps, 10)),
                   dict(what="mesh_vertex_normals", verts=nv, faces=nf, **_median_ms(lambda: ops.mesh_vertex_normals(full), a.warmup, a.reps, 10))]
    for row in res["mesh"]:
        print(json.dumps(row), flush=True)

    # the six volumes
    sets, res["meshset"], res["counts"] = {}, [], {}
    for name, kw in (("soup", {}), ("welded", dict(indexed=True)), ("cluster2", dict(indexed=True, cluster=2))):
        sets[name], row = _host_ms(lambda: ops.tsdf_meshset(volumes, **kw), a.warmup, a.reps)
        res["meshset"].append(dict(what=name, volumes=6, **row))
        res["counts"][name] = dict(verts=sets[name].n_verts, faces=sets[name].n_faces)
        print(json.dumps(res["meshset"][-1]), json.dumps(res["counts"][name]), flush=True)
    seq = [dict(depth=fr["depth"], inst_mask=rendered["mask"][i]) for i, fr in enumerate(frames)]
    ev = myEvaluater(PoseNet9D().to(dev).eval(), sampler="device")
    res["scan"] = []
    for indexed in (False, True):
        _, row = _host_ms(lambda: ev.scan(seq, list(RTs), K, volumes=ops.TsdfVolumes.from_meshset(objects, a.G), trunc_mm=trunc,
                                          inst_ids=[1, 2, 3, 4, 5, 6], indexed=indexed), a.warmup, a.reps)
        res["scan"].append(dict(frames=S, objects=6, indexed=indexed, **row))
        print(json.dumps(res["scan"][-1]), flush=True)

    # downstream on the three sets
    sym = ops.SymmetrySet([ops.SymmetrySet.identity()], device=dev)
    job_sym = torch.zeros(J, dtype=torch.int32, device=dev)
    est = job_pose.clone()
    est[:, :, 3] += 0.002
    job_camk = camk[job_img.long()].contiguous()
    res["downstream"] = []
    for name, ms in sets.items():
        row = dict(what=name, verts=sum(ms.n_verts), faces=sum(ms.n_faces))
        row["pose_errors_192"] = _median_ms(lambda: ops.pose_errors(ms, job_model, est, job_pose, sym, job_sym, job_camk), 1, 3, 1)

        def diam():
            ms._diameter = None
            return bop.diameter(ms)
        row["diameter"] = _median_ms(diam, 0, 1, 1)                        # one call: the soup's takes seconds
        row["diameter_model_units"] = [float(x) for x in bop.diameter(ms).cpu()]
        row["pose_verify_192"] = _median_ms(lambda: ops.pose_verify(ms, depth, camk, job_img, job_model, job_pose, tau=5, mask=mask, job_mask_val=job_val),
                                            a.warmup, a.reps, 5)
        score = ops.pose_verify(ms, depth, camk, job_img, job_model, job_pose, tau=5, mask=mask, job_mask_val=job_val)["score"]
        row["verify_score_true_pose_mean"] = float(score.mean())
        res["downstream"].append(row)
        print(json.dumps(row), flush=True)

    # the two boxes at G = 32: tests/tsdf_cases.scan_downstream's search on the soup set, scored on the three sets
    c = tc.scanned_two_boxes(dev, 32)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    models = ops.IcpModels.from_meshset(c["scanned"], [0], 1024)
    search = pose.ModelSearch(ops.DistanceFields(models, G=32), models, view_sampler.rotation_grid(42, 12), K=5, stride=2, top=16,
                              refine=pose.IcpRefine(models, [0], 0.01, mode="plane"), verify=pose.Verify(c["scanned"], [0], tau=tc.LOOP_TAU))
    found = search(up(c["cloud"][None, ::2]), torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1,), tc.TURN_SCALE, device=dev),
                   depth=c["held_depth"], camk=c["held_camk"])
    rt = found["RTs"].cpu().numpy()
    R_true, t_true = c["held_pose"]
    start = tc.pose44(icp_ref.rot([1, 2, -1], 5.0) @ R_true, t_true + 0.010 * np.array([2.0, -1.0, 2.0]) / 3.0, tc.TURN_SCALE)
    res["two_boxes"] = dict(G=32, voxel_mm=1000 * c["voxel_m"], radius_mm=1000 * c["radius_m"], sets=[])
    for name, kw in (("soup", {}), ("welded", dict(indexed=True, normals=True)), ("cluster2", dict(indexed=True, cluster=2, normals=True))):
        ms = ops.tsdf_meshset(c["volumes"], **kw)
        score = bop.score_track([dict(pred_RTs=rt)], c["held_rt"][None, None], ms, [0], [dict(depth=c["held_depth_host"])], tc.LOOP_K, sym, [0])
        err = score["err"][0].cpu().numpy()
        row = dict(what=name, verts=ms.n_verts[0], faces=ms.n_faces[0], add_mm=1000 * float(err[0]), adi_mm=1000 * float(err[1]),
                   mssd_mm=1000 * float(err[2]), diameter_mm=1000 * tc.TURN_SCALE * float(bop.diameter(ms)[0]),
                   verify_score_true_pose=float(pose.Verify(ms, [0], tau=tc.LOOP_TAU)(c["held_depth"], c["held_camk"], up(c["held_rt"][None]))["score"][0]))
        if ms.vert_normals is not None:
            n = min(1024, ms.n_verts[0] // 512 * 512)
            got, info, rmse = pose.refine_poses(ops.IcpModels.from_vertices(ms, [0], n), torch.zeros(1, dtype=torch.int32, device=dev),
                                                up(c["cloud"][None]), up(start[None]), 0.02, mode="plane", iters=50)
            deg, mm = tc._pose_error(got[0].cpu().numpy(), c["held_pose"])
            row["icp_from_vertices"] = dict(n=n, rot_deg=float(deg), trans_mm=float(mm), status=int(info[0, 0]), inliers=int(info[0, 1]))
        res["two_boxes"]["sets"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
