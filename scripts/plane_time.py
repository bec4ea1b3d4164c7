"""Times the supporting plane (ops.plane_fit + ops.plane_cut: csrc/plane.hip).  Writes profiles/plane_time.json:

  * fit_cut: device time of one plane_fit (256 hypotheses, 2 refits) and of fit + cut for S = 1, 6 and 32 frames of 480 x 640 -- the
    six-object table scenes of scripts/ball_crop_time.py, rendered on the device; frames stay on the device.
  * torch_composition: the same work composed from torch operations on the same device -- torch_fit_cut below: three random pixels
    per hypothesis and their float64 cross product, a batched (S, hypotheses, H*W) distance test (in chunks of frames that fit in
    memory), argmax, per refit masked float64 moments and torch.linalg.eigh, and the cut as torch.where.  Its hypotheses are
    torch.randint's, not the kernel's: the refitted planes are compared (max_plane_diff; agreement, not equality).
  * track: milliseconds per frame, host clock, of myEvaluater.track(refine=..., init_from='previous') on those scenes with and
    without support=pose.SupportPlane().
Device times are per call: a window is `calls` back-to-back calls between two HIP events, divided by the number of calls; median of
--reps windows after --warmup.  No time is a pass or fail condition; the capability is new, so there is no earlier figure.

    python scripts/plane_time.py [--reps 5] [--warmup 2] [--out profiles/plane_time.json]
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

HYPOTHESES, TOL, MARGIN, REFITS = 256, 0.004, 0.006, 2


def torch_fit_cut(depth, camk, hypotheses, tol, margin, refits, chunk=2):
    """depth (S,H,W) int16-viewed uint16, camk (S,4) -> (plane (S,4) float32, cut depth): what plane_fit + plane_cut replace"""
    S, H, W = depth.shape
    HW = H * W
    dev = depth.device
    dep = (depth.reshape(S, HW).int() & 0xffff).float()
    valid = dep > 0
    xs = torch.arange(W, device=dev, dtype=torch.float32).repeat(H)[None]
    ys = torch.arange(H, device=dev, dtype=torch.float32).repeat_interleave(W)[None]
    z = dep / 1000.0
    pts = torch.stack([(xs - camk[:, 2:3]) * dep / camk[:, 0:1] / 1000.0, (ys - camk[:, 3:4]) * dep / camk[:, 1:2] / 1000.0, z], 2)      # (S,HW,3)
    idx = torch.randint(HW, (S, hypotheses * 3), device=dev)
    tri = torch.gather(pts, 1, idx[:, :, None].expand(-1, -1, 3)).double().reshape(S, hypotheses, 3, 3)
    ok = torch.gather(valid, 1, idx).reshape(S, hypotheses, 3).all(2)
    n = torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
    nn = (n * n).sum(2, keepdim=True)
    ok = ok & (nn[:, :, 0] > 1e-18)
    n = n / nn.sqrt()
    d = -(n * tri[:, :, 0]).sum(2, keepdim=True)
    planes = (torch.cat([n, d], 2) * torch.where(d < 0, -1.0, 1.0)).float()
    planes = torch.where(ok[:, :, None], planes, torch.full_like(planes, float("nan")))
    counts = torch.empty(S, hypotheses, dtype=torch.int64, device=dev)
    for lo in range(0, S, chunk):
        dist = torch.baddbmm(planes[lo:lo + chunk, :, 3:4], planes[lo:lo + chunk, :, :3], pts[lo:lo + chunk].transpose(1, 2))     # (c,Hn,HW)
        counts[lo:lo + chunk] = ((dist.abs() <= tol) & valid[lo:lo + chunk, None, :]).sum(2)
    best = counts.argmax(1)
    plane = planes[torch.arange(S, device=dev), best]
    p64 = pts.double()
    for _ in range(refits):
        dist = (pts * plane[:, None, :3]).sum(2) + plane[:, None, 3]
        w = ((dist.abs() <= tol) & valid).double()
        N = w.sum(1)
        mean = (w[:, :, None] * p64).sum(1) / N[:, None]
        c = p64 - mean[:, None]
        C = torch.einsum("sp,spa,spb->sab", w, c, c)
        q = torch.linalg.eigh(C)[1][:, :, 0]
        d = -(q * mean).sum(1, keepdim=True)
        plane = (torch.cat([q, d], 1) * torch.where(d < 0, -1.0, 1.0)).float()
    dist = (pts * plane[:, None, :3]).sum(2) + plane[:, None, 3]
    cut = torch.where((dist > margin).reshape(S, H, W), depth, torch.zeros_like(depth))
    return plane, cut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plane_time.py measures on a GPU; none is visible")
    import ball_crop_time as bct
    from tgpose_amd import PoseNet9D, ops, pose, seeded_state_dict
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "hypotheses": HYPOTHESES, "tol": TOL, "margin": MARGIN,
           "refine_iters": REFITS, "H": bct.H, "W": bct.W,
           "note": "per call: windows of `calls_per_window` back-to-back calls between two HIP events; median of `reps` windows after "
                   "`warmup`; host-clock entries say so.  One fit = a memset, the scoring launch and the finish launch for all frames"}
    K = lde.CAMERA_INTRINSICS
    ms6 = ops.MeshSet([shapes.lathe(shapes.PROFILES[nm], 24) for nm in bct.NAMES] + [shapes.plane(4.0, 4.0, 4, 4)], device=dev)
    sc = bct.scenes(32)
    rendered = synthetic.render_scenes(ms6, sc, K, bct.H, bct.W)
    depth_all = torch.from_numpy(rendered["depth"].view(np.int16)).to(dev)
    camk_all = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32, device=dev).repeat(32, 1)
    res["fit_cut"], res["torch_composition"] = [], []
    for S in (1, 6, 32):
        depth, camk = depth_all[:S].contiguous(), camk_all[:S].contiguous()
        keys = torch.arange(S, dtype=torch.int64, device=dev)

        def fit():
            return ops.plane_fit(depth, camk, tol=TOL, hypotheses=HYPOTHESES, seed=1, keys=keys, refine_iters=REFITS)

        def fit_cut():
            plane, info = fit()
            return plane, info, ops.plane_cut(depth, plane, info, camk, MARGIN)
        plane, info, cut = fit_cut()
        info_h = info.cpu().numpy()
        assert (info_h[:, 0] == 0).all()
        calls = 20 if S <= 6 else 5
        t_fit, t_both = _median_ms(fit, a.warmup, a.reps, calls), _median_ms(fit_cut, a.warmup, a.reps, calls)
        row = dict(frames=S, launches_fit=2, launches_cut=1, tests_per_call=int(S) * HYPOTHESES * bct.H * bct.W,
                   mean_valid=float(info_h[:, 3].mean()), mean_plane_inliers=float(info_h[:, 2].mean()),
                   mean_left_after_cut=float((cut != 0).sum().item()) / S, fit=t_fit, fit_cut=t_both)
        row["us_per_frame_fit_cut"] = t_both["median_ms"] * 1e3 / S
        res["fit_cut"].append(row)
        print(json.dumps(row), flush=True)

        def comp():
            return torch_fit_cut(depth, camk, HYPOTHESES, TOL, MARGIN, REFITS)
        torch.manual_seed(0)
        tp, tcut = comp()
        flip = torch.where((tp[:, :3] * plane[:, :3]).sum(1, keepdim=True) < 0, -1.0, 1.0)
        crow = dict(frames=S, max_plane_diff=float((tp * flip - plane).abs().max()), **_median_ms(comp, a.warmup, a.reps, 2 if S <= 6 else 1))
        crow["ratio_to_kernels"] = crow["median_ms"] / t_both["median_ms"]
        res["torch_composition"].append(crow)
        print(json.dumps(crow), flush=True)
        del tp, tcut
        torch.cuda.empty_cache()
    # the model-based tracker on the same scenes, with and without the cut
    frames = [synthetic.scene_frame(ms6, sc, rendered, i) for i in range(a.frames)]
    seq = [dict(depth=fr["depth"], inst_mask=rendered["mask"][i]) for i, fr in enumerate(frames)]
    init = dict(class_ids=frames[0]["gt_class_ids"][:6], RTs=frames[0]["gt_RTs"][:6], scales=frames[0]["gt_scales"][:6], inst_ids=[1, 2, 3, 4, 5, 6])
    net = PoseNet9D().to(dev).eval()
    net.load_state_dict(seeded_state_dict(0))
    refine = pose.IcpRefine(ops.IcpModels.from_meshset(ms6, [0, 1, 2, 3], 1024), [o % 4 for o in range(6)], 0.01, mode="plane")
    ev = myEvaluater(net, sampler="device", seed=1)
    res["track"] = []
    for name, kw in (("previous+icp", {}), ("previous+icp+support", dict(support=pose.SupportPlane(TOL, MARGIN, HYPOTHESES, REFITS)))):
        kw = dict(refine=refine, init_from="previous", use_mask=False, **kw)
        ev.track(seq[:4], init, K, bct.RATIO, **kw)
        torch.cuda.synchronize()
        t_0 = time.perf_counter()
        out = ev.track(seq, init, K, bct.RATIO, **kw)
        torch.cuda.synchronize()
        row = dict(path=name, frames=len(seq), objects=6, n_pts=1024, host_clock=True, ms_per_frame=(time.perf_counter() - t_0) * 1e3 / len(seq),
                   icp_ok_share=float(np.mean([(o["icp_status"] == 0).mean() for o in out])),
                   mean_inliers=float(np.mean([o["icp_inliers"].mean() for o in out])))
        if "plane_status" in out[0]:
            row.update(plane_ok_share=float(np.mean([o["plane_status"] == 0 for o in out])),
                       mean_plane_inliers=float(np.mean([o["plane_inliers"] for o in out])))
        res["track"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
