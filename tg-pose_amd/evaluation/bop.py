"""The BOP pose errors and scores on the device: symmetry groups, diameters, the 4x4 forms of ops.pose_errors (ADD, ADD-S, MSSD,
MSPD) and ops.pose_vsd (VSD), recall and average recall, and the scoring of a tracked sequence (DESIGN.md section 3 "BOP pose
errors").  The kernels are csrc/poseerr.hip and csrc/vsd.hip; what is here is plumbing and a few reductions in plain torch.

The reference vendors lib/pysixd for this (get_symmetry_transformations, calc_pts_diameter, the VSD / ADD / ADI error signatures)
without a path that runs it; the definitions are those of the BOP toolkit (Hodan et al., "BOP Challenge 2020 on 6D Object
Localization"), with one stated deviation for VSD: depth along the optical axis, not distance from the camera centre."""
import math

import numpy as np
import torch

from .. import ops, pose

TAUS = np.arange(0.05, 0.51, 0.05)              # VSD's misalignment tolerances, fractions of the diameter
THETAS = np.arange(0.05, 0.51, 0.05)            # the correctness thresholds of VSD, and of MSSD as fractions of the diameter
MSPD_PX = np.arange(5, 51, 5)                   # the correctness thresholds of MSPD in pixels at a width of 640


def rodrigues(axis, angle):
    """the rotation by ``angle`` radians about ``axis`` (3,), float64: I + sin a K + (1 - cos a) K^2 with K the unit axis' cross matrix"""
    k = np.asarray(axis, dtype=np.float64).reshape(3)
    n = np.linalg.norm(k)
    if not n > 0:
        raise ValueError("rodrigues: the axis must not be zero")
    k = k / n
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=np.float64)
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """The symmetry group of a BOP models_info entry as (Q,3,4) float64 [R | t], in the entry's units: the identity and each of
    'symmetries_discrete' (16 numbers, a row-major 4x4), each composed with every step of each of 'symmetries_continuous' ({'axis',
    'offset'}): ceil(pi / max_sym_disc_step) steps of 2 pi / steps radians, R_c = rotation about the axis, t_c = offset - R_c offset;
    composition R = R_c R_d, t = R_c t_d + t_c, discrete outer, continuous inner -- the reference's get_symmetry_transformations
    (lib/pysixd/misc.py).  One deviation: the steps run from 0, so the identity step is included, as in the BOP toolkit; the
    reference's loop starts at 1 and loses the identity whenever a continuous symmetry exists.  Q = steps * (1 + discrete) with a
    continuous symmetry, 1 + discrete without."""
    disc = [(np.eye(3), np.zeros(3))]
    for s in model_info.get("symmetries_discrete", ()):
        m = np.asarray(s, dtype=np.float64).reshape(4, 4)
        disc.append((m[:3, :3], m[:3, 3]))
    cont = []
    for s in model_info.get("symmetries_continuous", ()):
        offset = np.asarray(s["offset"], dtype=np.float64).reshape(3)
        steps = int(math.ceil(math.pi / max_sym_disc_step))
        step = 2.0 * math.pi / steps
        for i in range(steps):
            R = rodrigues(s["axis"], i * step)
            cont.append((R, offset - R @ offset))
    out = []
    for Rd, td in disc:
        if cont:
            out += [np.concatenate([Rc @ Rd, (Rc @ td + tc)[:, None]], 1) for Rc, tc in cont]
        else:
            out.append(np.concatenate([Rd, td[:, None]], 1))
    return np.stack(out)


def diameter(meshset, chunk=None):
    """(M) float64 on the mesh set's device: the largest vertex-to-vertex distance of each mesh, in model units (the reference's
    calc_pts_diameter), by chunked float64 differences: ``chunk`` rows against all vertices at a time, by default about 2^20
    pairs (some 50 MB of temporaries whatever the mesh).  Computed once per mesh set and kept on it (MeshSet._diameter): the value
    does not depend on ``chunk``, so a later call returns it whatever its ``chunk``."""
    if not isinstance(meshset, ops.MeshSet):
        raise TypeError("diameter: meshset must be an ops.MeshSet")
    if meshset._diameter is None:
        out, start = [], 0
        for n in meshset.n_verts:
            v = meshset.verts[start:start + n].double()
            best = torch.zeros((), dtype=torch.float64, device=v.device)
            rows = chunk or max(1, (1 << 20) // n)
            for i in range(0, n, rows):
                best = torch.maximum(best, (v[i:i + rows, None, :] - v[None, :, :]).square().sum(2).max().sqrt())
            out.append(best)
            start += n
        meshset._diameter = torch.stack(out)
    return meshset._diameter


def _i32(x, dev):
    return x.to(device=dev, dtype=torch.int32).contiguous() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.int32, device=dev)


def _job_camk(camk, J):
    camk = camk.float()
    if camk.dim() == 1:
        camk = camk[None].expand(J, 4)
    if camk.shape != (J, 4):
        raise ValueError("bop.errors: camk must be (4) or (J,4) = fx, fy, cx, cy")
    return camk.contiguous()


def errors(meshset, job_mesh, RTs_est, RTs_gt, symset, job_sym, camk, scales=None, near=0.01):
    """ops.pose_errors on the project's 4x4 poses [s R | t] (J,4,4) on the mesh set's device: job poses by pose.verify_job_pose
    (with ``scales`` (J,3) the meshes are normalised and both poses' linear parts are multiplied by diag(scales)).  camk (4) or
    (J,4).  -> ops.pose_errors' dict."""
    dev = meshset.verts.device
    J = RTs_est.shape[0]
    return ops.pose_errors(meshset, _i32(job_mesh, dev), pose.verify_job_pose(RTs_est, scales), pose.verify_job_pose(RTs_gt, scales), symset,
                           _i32(job_sym, dev), _job_camk(camk, J), near=near)


def vsd_taus(diameter_mm, taus=TAUS):
    """job_tau (J, n_tau) int32 = ceil(float64(tau) * float64(diameter in millimetres)): |d_g - d_e| < tau * diameter on integer
    millimetres is |d_g - d_e| < ceil(tau * diameter)"""
    d = diameter_mm.double().reshape(-1, 1)
    t = torch.as_tensor(np.asarray(taus, dtype=np.float64), device=d.device).reshape(1, -1)
    return torch.ceil(t * d).to(torch.int32).contiguous()


def vsd(meshset, depth, camk, job_img, job_mesh, RTs_est, RTs_gt, diameter_mm, scales=None, taus=TAUS, delta=15, near=0.01):
    """ops.pose_vsd on 4x4 poses: depth (S,H,W) millimetres, camk (S,4), diameter_mm (J) each job's object diameter in millimetres
    (the model's diameter times the pose's scale times 1000); job_tau by vsd_taus.  -> ops.pose_vsd's dict plus 'job_tau'."""
    dev = meshset.verts.device
    job_tau = vsd_taus(diameter_mm.to(dev), taus)
    out = ops.pose_vsd(meshset, depth, camk, _i32(job_img, dev), _i32(job_mesh, dev), pose.verify_job_pose(RTs_est, scales),
                       pose.verify_job_pose(RTs_gt, scales), job_tau, delta=delta, near=near)
    out["job_tau"] = job_tau
    return out


def recall(err, thresholds):
    """The fraction of (job, threshold) pairs with err < threshold, a 0-dim float64 tensor on err's device.  err (J) with thresholds
    (T) or (J,T); or err (J,K) -- VSD's, one column per tau -- with thresholds (T): every column against every threshold."""
    if not torch.is_tensor(thresholds):
        thresholds = torch.as_tensor(np.asarray(thresholds, dtype=np.float64), device=err.device)
    e, t = err.double(), thresholds.double()
    if e.numel() == 0:
        return torch.zeros((), dtype=torch.float64, device=err.device)
    if e.dim() == 2:
        return (e[:, :, None] < t.reshape(1, 1, -1)).double().mean()
    return (e[:, None] < (t if t.dim() == 2 else t[None])).double().mean()


def average_recall(err, vsd_err, diameter_m, width):
    """BOP's average recall of J jobs: err (J,4) ops.pose_errors' (metres, pixels), vsd_err (J,10) over TAUS, diameter_m (J)
    the objects' diameters in metres, width the image width in pixels.  AR_MSSD: thresholds 0.05 .. 0.5 of the diameter; AR_MSPD:
    5 .. 50 px times width / 640; AR_VSD: 0.05 .. 0.5 over the taus; AR their mean.  -> dict of 0-dim float64 tensors."""
    dev = err.device
    th = torch.as_tensor(THETAS, device=dev)
    ar_mssd = recall(err[:, 2], diameter_m.double().reshape(-1, 1) * th[None])
    ar_mspd = recall(err[:, 3], torch.as_tensor(MSPD_PX.astype(np.float64), device=dev) * (float(width) / 640.0))
    ar_vsd = recall(vsd_err, th)
    return dict(AR_MSSD=ar_mssd, AR_MSPD=ar_mspd, AR_VSD=ar_vsd, AR=(ar_mssd + ar_mspd + ar_vsd) / 3.0)


def add_s(err, symmetric):
    """ADD(-S) per job: adi where ``symmetric`` (J) bool, add elsewhere"""
    sym = torch.as_tensor(symmetric, dtype=torch.bool, device=err.device)
    return torch.where(sym, err[:, 1], err[:, 0])


def score_track(results, gts, meshset, job_mesh, sequence, camK, symset, job_sym, taus=TAUS, delta=15, near=0.01):
    """Scores what myEvaluater.track returns for a sequence against ground truth, in one call of each kernel over all (frame, object)
    pairs.  results: the list over frames of {'pred_RTs' (n,4,4), ...}; gts: (frames, n, 4, 4) ground-truth poses [s R | t];
    job_mesh, job_sym (n): each object's mesh (in the model's units, as pose.Verify takes it) and symmetry group; sequence: the
    frames ({'depth' (H,W) uint16 millimetres}); camK the 3x3 intrinsics.  Job f * n + o is object o in frame f; an object's
    diameter is its mesh's times the cube root of the ground-truth pose's determinant.
    -> dict of device tensors: err (F n,4), sym_best, status, vsd_counts, vsd_within, vsd_err (F n, len(taus)), job_tau,
    diameter (F n) metres, and AR_MSSD, AR_MSPD, AR_VSD, AR."""
    dev = meshset.verts.device
    F = len(results)
    est = np.stack([np.asarray(r["pred_RTs"], dtype=np.float32) for r in results])
    gt = np.asarray(gts, dtype=np.float32)
    if est.ndim != 4 or est.shape != gt.shape or est.shape[2:] != (4, 4) or len(sequence) != F:
        raise ValueError("score_track: results and gts must both be (frames, n, 4, 4), one frame of the sequence each")
    n = est.shape[1]
    est, gt = torch.from_numpy(est.reshape(F * n, 4, 4)).to(dev), torch.from_numpy(gt.reshape(F * n, 4, 4)).to(dev)
    jm, js = _i32(job_mesh, dev).repeat(F), _i32(job_sym, dev).repeat(F)
    K = np.asarray(camK, dtype=np.float32)
    camk = torch.tensor([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dtype=torch.float32, device=dev)
    depth = torch.from_numpy(np.stack([np.asarray(f["depth"]).astype(np.uint16) for f in sequence]).view(np.int16)).to(dev)
    job_img = torch.arange(F, dtype=torch.int32, device=dev).repeat_interleave(n)
    diam = diameter(meshset)[jm.long()] * torch.linalg.det(gt[:, :3, :3].double()).abs().pow(1.0 / 3.0)
    e = errors(meshset, jm, est, gt, symset, js, camk, near=near)
    v = vsd(meshset, depth, camk[None].expand(F, 4).contiguous(), job_img, jm, est, gt, diam * 1000.0, taus=taus, delta=delta, near=near)
    out = dict(err=e["err"], sym_best=e["sym_best"], status=e["status"], vsd_counts=v["counts"], vsd_within=v["within"], vsd_err=v["err"],
               job_tau=v["job_tau"], diameter=diam)
    out.update(average_recall(e["err"], v["err"], diam, depth.shape[2]))
    return out
