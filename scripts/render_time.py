"""Times the depth renderer (ops.render_depth: csrc/render.hip) on the workload it was built for and writes profiles/render_time.json:

  * kernel: S = 32 scenes of 640 x 480, six objects of about 5 k faces each (icosphere level 4, lathe bottle / bowl / can / mug with
    the steps that give 5 k faces) standing on a two-triangle table, and the same scenes with the table cut into 64 x 64 x 2 triangles; device time per call
    by HIP events around the call (output and workspace allocation and the ctypes call included), median of --reps calls after
    --warmup; the bytes the call writes; the triangles per scene;
  * restatement_cpu: tests/render_ref.py on one of those frames on a CPU (one run, one thread), as the comparison;
  * the first frame of each workload is checked against the restatement bit for bit (depth and mask) before anything is recorded.

    python scripts/render_time.py [--reps 10] [--warmup 3] [--scenes 32] [--out profiles/render_time.json]
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

H, W = 480, 640


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])}[axis]


def table_scenes(S, table_mesh, object_meshes, seed=0):
    """S scenes: the table (a 2.0 x 1.4 m rectangle tilted 55 degrees, 1.2 m away) and six objects standing on it, their up axis
    (model y) along the table's normal, a random yaw, size and place in a 3 x 2 grid"""
    rng = np.random.RandomState(seed)
    Rt, tt = rot("x", 55), np.array([0.0, 0.05, 1.2])
    up = Rt @ rot("x", -90)                                            # model y -> the table's normal towards the camera
    scenes = []
    for _ in range(S):
        sc = [dict(mesh=table_mesh, inst_id=1, R=Rt, t=tt, s=1.0)]
        for k in range(6):
            s = rng.uniform(0.18, 0.3)
            place = np.array([(k % 3 - 1) * 0.42 + rng.uniform(-0.06, 0.06), (k // 3 - 0.5) * 0.5 + rng.uniform(-0.06, 0.06), -0.5 * s])
            sc.append(dict(mesh=object_meshes[rng.randint(len(object_meshes))], inst_id=2 + k, R=up @ rot("y", rng.uniform(0, 360)),
                           t=Rt @ place + tt, s=s))
        scenes.append(sc)
    return scenes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.json"))
    a = ap.parse_args()
    from tests import render_ref
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluation.load_data_eval import CAMERA_INTRINSICS as K
    dev = "cuda:0"
    meshes = [shapes.plane(2.0, 1.4, 1, 1), shapes.plane(2.0, 1.4, 64, 64), shapes.icosphere(0.5, 4)] + \
             [shapes.lathe(p, int(round(5000.0 / (2 * (len(p) - 2))))) for p in (shapes.PROFILES[n] for n in ("bottle", "bowl", "can", "mug"))]
    ms = ops.MeshSet(meshes, device=dev)
    camk = np.tile(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dtype=np.float32), (a.scenes, 1))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "H": H, "W": W, "scenes": a.scenes,
           "mesh_faces": ms.n_faces, "kernel": [], "restatement_cpu": [],
           "note": "kernel: HIP events around ops.render_depth (depth, mask, visible, bbox, dropped; no z / face), median of `reps` calls "
                   "after `warmup`; restatement_cpu: tests/render_ref.py, one frame, one run"}
    for table, name in ((0, "table of 2 triangles"), (1, "table of 64 x 64 x 2 triangles")):
        scenes = table_scenes(a.scenes, table, list(range(2, len(meshes))))
        ptr, mesh, ids, pose = synthetic.pack_scenes(scenes, len(ms))
        args = (ms, up(ptr), up(mesh), up(ids), up(pose), up(camk), H, W)
        out = ops.render_depth(*args)
        t0 = time.perf_counter()
        ref = render_ref.render(meshes, ptr[:2], mesh, ids, pose, camk[:1], H, W)
        cpu_s = time.perf_counter() - t0
        assert np.array_equal(out["depth"][0].cpu().numpy(), ref["depth"][0]) and np.array_equal(out["mask"][0].cpu().numpy(), ref["mask"][0])
        times = []
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = ops.render_depth(*args)
            e.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times.append(s.elapsed_time(e))
        tri = int(sum(ms.n_faces[m] for m in mesh) / a.scenes)
        I = len(mesh)
        run = dict(workload=name, scenes=a.scenes, instances=I, triangles_per_scene=tri, launches=4, median_ms=statistics.median(times),
                   min_ms=min(times), max_ms=max(times), ms_per_frame=statistics.median(times) / a.scenes,
                   bytes_written=a.scenes * H * W * 3 + I * 20 + a.scenes * 8, covered_fraction=float((out["mask"] > 0).float().mean().item()),
                   visible_instances=int((out["visible"] > 0).sum().item()), dropped=out["dropped"].sum(0).tolist())
        res["kernel"].append(run)
        print(json.dumps(run), flush=True)
        cpu = dict(workload=name, frames=1, triangles=tri, seconds=cpu_s, equal_to_kernel=True)
        res["restatement_cpu"].append(cpu)
        print(json.dumps(cpu), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
