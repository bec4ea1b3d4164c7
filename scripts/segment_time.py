"""Times the depth segmentation (ops.segment_depth: csrc/segment.hip) and myEvaluater.acquire.  Writes profiles/segment_time.json:

  * segment: device time of one segment_depth call (step 10 mm, 4-neighbours, min_pixels 50, 32 segments, with centroids) for S = 1, 6
    and 32 frames of 480 x 640 -- the six-object table scenes of scripts/ball_crop_time.py rendered on the device -- after the plane
    cut ("cut": what the tracker segments) and as rendered ("uncut": the table is one huge component), and for one 480 x 640
    serpentine (a one-pixel-wide path of about 154 000 pixels through the whole frame: the longest chains the merge can meet).
  * torch_composition: the same labelling composed from torch operations on the same device -- torch_label below: every valid pixel
    starts with its flat index and takes the minimum over its joined neighbours until nothing changes (one host read per sweep to
    learn that).  Labels are compared with the kernel's (equal: true).  The serpentine needs as many sweeps as its path is long; there
    a fixed number of sweeps is timed and the total extrapolated (extrapolated: true).
  * scipy: the same labelling on one CPU core, host clock, median of three runs: the joined pairs as a NumPy edge list and
    scipy.sparse.csgraph.connected_components (scipy.ndimage.label knows no depth step).
  * acquire: milliseconds per call, host clock (it ends with a read-back), of myEvaluater.acquire(support=SupportPlane()) on frame 0.
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  A call includes the wrapper's allocations.  No time is a pass or fail condition.

    python scripts/segment_time.py [--reps 5] [--warmup 2] [--out profiles/segment_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from icp_time import _median_ms  # noqa: E402

STEP, CONNECTIVITY, MIN_PIXELS, MAX_SEGMENTS = 10, 4, 50, 32
BIG = 2 ** 30


def torch_neighbours(depth, step):
    """depth (S,H,W) int16-viewed uint16 -> (start labels (S,H,W) int32: the flat index, BIG where invalid; the joined masks of the pairs (x, x + 1) and (y, y + 1))"""
    S, H, W = depth.shape
    z = depth.int() & 0xffff
    valid = z > 0
    flat = torch.arange(H * W, device=depth.device, dtype=torch.int32).reshape(1, H, W).expand(S, H, W)
    lab = torch.where(valid, flat, torch.full_like(flat, BIG)).contiguous()
    right = valid[:, :, :-1] & valid[:, :, 1:] & ((z[:, :, :-1] - z[:, :, 1:]).abs() <= step)        # (x, x + 1)
    down = valid[:, :-1] & valid[:, 1:] & ((z[:, :-1] - z[:, 1:]).abs() <= step)                       # (y, y + 1)
    return lab, right, down


def torch_sweep(lab, right, down):
    new = lab.clone()
    new[:, :, :-1] = torch.minimum(new[:, :, :-1], torch.where(right, lab[:, :, 1:], BIG))
    new[:, :, 1:] = torch.minimum(new[:, :, 1:], torch.where(right, lab[:, :, :-1], BIG))
    new[:, :-1] = torch.minimum(new[:, :-1], torch.where(down, lab[:, 1:], BIG))
    new[:, 1:] = torch.minimum(new[:, 1:], torch.where(down, lab[:, :-1], BIG))
    return new


def torch_label(depth, step, max_sweeps=None):
    """-> (root image (S,H,W) int32, BIG where invalid; sweeps made)"""
    lab, right, down = torch_neighbours(depth, step)
    sweeps = 0
    while max_sweeps is None or sweeps < max_sweeps:
        new = torch_sweep(lab, right, down)
        sweeps += 1
        if max_sweeps is None and torch.equal(new, lab):
            break
        lab = new
    return lab, sweeps


def scipy_label(depth, step):
    """depth (H,W) uint16 on the host -> number of components among the valid pixels"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    H, W = depth.shape
    z = depth.astype(np.int32)
    idx = np.arange(H * W, dtype=np.int32).reshape(H, W)
    pairs = []
    for a, b in (((slice(None), slice(0, W - 1)), (slice(None), slice(1, W))), ((slice(0, H - 1), slice(None)), (slice(1, H), slice(None)))):
        ok = (z[a] > 0) & (z[b] > 0) & (np.abs(z[a] - z[b]) <= step)
        pairs.append(np.stack([idx[a][ok], idx[b][ok]], 1))
    e = np.concatenate(pairs)
    g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(H * W, H * W))
    comp = connected_components(g, directed=False)[1]
    return len(np.unique(comp[depth.reshape(-1) > 0]))


def serpentine(H, W, z=800):
    d = np.zeros((H, W), np.uint16)
    d[0::2] = z
    for k, y in enumerate(range(1, H - 1, 2)):
        d[y, W - 1 if k % 2 == 0 else 0] = z
    if H % 2 == 0:
        d[H - 1] = 0
    return d


def roots_of(seg):
    """the kernel's labelling as a root image like torch_label's: BIG where the pixel has no segment"""
    S, M = seg.stats.shape[:2]
    table = torch.cat([torch.full((S, 1), BIG, device=seg.stats.device, dtype=torch.int64), seg.stats[:, :, 5]], 1)
    return torch.gather(table, 1, seg.labels.reshape(S, -1).long()).reshape(seg.labels.shape).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_time.json"))
    ap.add_argument("--kernel-only", type=int, default=0, metavar="S",
                    help="only 50 segment_depth calls on S cut frames, nothing written: the run a kernel trace is taken of")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segment_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "max_step": STEP, "connectivity": CONNECTIVITY,
           "min_pixels": MIN_PIXELS, "max_segments": MAX_SEGMENTS, "H": bct.H, "W": bct.W,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so.  One call = two memsets and seven launches for all frames, and the wrapper's "
                   "five allocations"}
    K = lde.CAMERA_INTRINSICS
    ms6 = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    sc = bct.scenes(32)
    rendered = synthetic.render_scenes(ms6, sc, K, bct.H, bct.W)
    uncut_all = torch.from_numpy(rendered["depth"].view(np.int16)).to(dev)
    camk_all = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32, device=dev).repeat(32, 1)
    support = pose.SupportPlane()
    cut_all, _, pinfo = support(uncut_all, camk_all, torch.arange(32, dtype=torch.int64, device=dev), 1)
    assert (pinfo[:, 0] == 0).all()
    serp = torch.from_numpy(serpentine(bct.H, bct.W)[None].view(np.int16)).to(dev)
    if a.kernel_only:
        depth, camk = cut_all[:a.kernel_only].contiguous(), camk_all[:a.kernel_only].contiguous()
        for _ in range(50):
            ops.segment_depth(depth, max_step=STEP, connectivity=CONNECTIVITY, min_pixels=MIN_PIXELS, max_segments=MAX_SEGMENTS, camk=camk)
        torch.cuda.synchronize()
        return
    scipy_label(np.ones((4, 4), np.uint16), STEP)                      # the import is not part of the first timing
    res["segment"], res["torch_composition"], res["scipy"] = [], [], []
    work = [("cut", cut_all, S) for S in (1, 6, 32)] + [("uncut", uncut_all, S) for S in (1, 6, 32)] + [("serpentine", serp, 1)]
    for name, frames, S in work:
        depth, camk = frames[:S].contiguous(), camk_all[:S].contiguous()

        def seg():
            return ops.segment_depth(depth, max_step=STEP, connectivity=CONNECTIVITY, min_pixels=MIN_PIXELS, max_segments=MAX_SEGMENTS, camk=camk)
        out = seg()
        info = out.info.cpu().numpy()
        row = dict(frames_of=name, frames=S, mean_valid=float(info[:, 3].mean()), mean_qualified=float(info[:, 2].mean()),
                   mean_kept=float(info[:, 1].mean()), cut_off_frames=int((info[:, 0] != 0).sum()),
                   **_median_ms(seg, a.warmup, a.reps, 20 if S <= 6 else 5))
        row["us_per_frame"] = row["median_ms"] * 1e3 / S
        res["segment"].append(row)
        print(json.dumps(row), flush=True)

        if name == "serpentine":
            sweeps = 200
            t = _median_ms(lambda: torch_label(depth, STEP, max_sweeps=sweeps), 1, 3, 1)
            needed = int(info[0, 3])                                   # the minimum travels one pixel of the path per sweep
            crow = dict(frames_of=name, frames=S, sweeps_timed=sweeps, ms_per_sweep=t["median_ms"] / sweeps, sweeps_needed=needed,
                        extrapolated=True, median_ms=t["median_ms"] / sweeps * needed)
        else:
            lab, sweeps = torch_label(depth, STEP)
            mine = roots_of(out)
            small = torch.zeros_like(lab, dtype=torch.bool)            # components the kernel drops (under min_pixels) are not compared
            small[mine == BIG] = True
            crow = dict(frames_of=name, frames=S, sweeps=sweeps, equal=bool(torch.equal(torch.where(small, BIG, lab), mine)),
                        **_median_ms(lambda: torch_label(depth, STEP), 1, 3, 1))
        crow["ratio_to_kernels"] = crow["median_ms"] / row["median_ms"]
        res["torch_composition"].append(crow)
        print(json.dumps(crow), flush=True)

        host = depth.cpu().numpy().view(np.uint16)
        runs = []
        for _ in range(3):
            t_0 = time.perf_counter()
            comps = [scipy_label(host[s], STEP) for s in range(S)]
            runs.append((time.perf_counter() - t_0) * 1e3)
        ms = sorted(runs)[1]
        srow = dict(frames_of=name, frames=S, host_clock=True, cores=1, runs=3, mean_components=float(np.mean(comps)), median_ms=ms,
                    ratio_to_kernels=ms / row["median_ms"])
        res["scipy"].append(srow)
        print(json.dumps(srow), flush=True)
        torch.cuda.empty_cache()
    # from a frame and a category to the tracker's init
    net = PoseNet9D().to(dev).eval()
    net.load_state_dict(seeded_state_dict(0))
    ev = myEvaluater(net, sampler="device", seed=1)
    frame = dict(depth=rendered["depth"][0])
    init = ev.acquire(frame, 1, K, support=support, segmenter=pose.Segmenter())
    times = []
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t_0 = time.perf_counter()
        ev.acquire(frame, 1, K, support=support, segmenter=pose.Segmenter())
        times.append((time.perf_counter() - t_0) * 1e3)
    times = sorted(times[a.warmup:])
    res["acquire"] = dict(objects_in_scene=6, segments_found=int(init["info"][1]), slots_forwarded=MAX_SEGMENTS, n_pts=1024, host_clock=True,
                          median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1], pixels=[int(p) for p in init["pixels"]])
    print(json.dumps(res["acquire"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
