"""NumPy restatement of the BOP pose errors' contracts (DESIGN.md section 3 "BOP pose errors"; the kernels are csrc/poseerr.hip and
csrc/vsd.hip).  Written from the contracts' text.  The point-based errors are float64 on the widened float32 inputs; the order of
the sums is NumPy's, not the kernel's, which is what the tolerance of tests/test_bop_gpu.py is for.  VSD renders each pose as a
scene of its one instance with tests/render_ref.py -- the depth renderer's restatement -- and is all-integer up to one fp32 division."""
import numpy as np

from tests import render_ref

ERRORS = ("add", "adi", "mssd", "mspd")
VSD_COUNTS = ("rendered_gt", "rendered_est", "visib_gt", "visib_est", "inter", "union", "dropped_gt", "dropped_est")
VCOL = {name: i for i, name in enumerate(VSD_COUNTS)}
MAX_JOBS, MAX_SYMS, MAX_TAUS = 65535, 1024, 16


def apply(T, p):
    """T (3,4) and points p (n,3), float64: ((T0 x + T1 y) + T2 z) + T3 per row"""
    T, p = np.asarray(T, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def project(x, camk):
    fx, fy, cx, cy = (float(k) for k in camk)
    return np.stack([fx * (x[:, 0] / x[:, 2]) + cx, fy * (x[:, 1] / x[:, 2]) + cy], 1)


def norms(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) if d.shape[1] == 3 else np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def job_errors(verts, E, G, group, camk, near=0.01, chunk=512):
    """one job: verts (P,3) float32, E, G (3,4) float32, group (Q,3,4) float32, camk (4,) float32
    -> dict err (4,) float64, sym_best (2,) int32, status int (0; 2: a projected point without z > near, mspd +inf; 4: a transformed
    point or an intrinsic is not finite, NaN and -1), and per_sym (Q,2) float64: max_i of the two distances for every S"""
    p = np.asarray(verts, dtype=np.float32).astype(np.float64)
    E, G = np.asarray(E, np.float32).astype(np.float64), np.asarray(G, np.float32).astype(np.float64)
    camk = np.asarray(camk, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e, g = apply(E, p), apply(G, p)
        gss = [apply(G, apply(S, p)) for S in np.asarray(group, np.float32).astype(np.float64)]
    if not (np.isfinite(e).all() and np.isfinite(g).all() and all(np.isfinite(x).all() for x in gss) and np.isfinite(camk).all()):
        # status 4, alone: something is not finite, and no threshold may count the job as correct
        return dict(err=np.full(4, np.nan), sym_best=np.full(2, -1, np.int32), status=4, per_sym=None)
    add = norms(e - g).mean()
    nearest = np.empty(len(p))
    for i in range(0, len(p), chunk):                                        # no P x P matrix here either
        d = e[i:i + chunk, None, :] - g[None, :, :]
        nearest[i:i + chunk] = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(1))
    adi = nearest.mean()
    behind = not (e[:, 2] > near).all()
    per_sym = np.empty((len(group), 2))
    with np.errstate(all="ignore"):
        pe = project(e, camk)
        for q, gs in enumerate(gss):
            behind = behind or not (gs[:, 2] > near).all()
            per_sym[q] = norms(e - gs).max(), norms(pe - project(gs, camk)).max()
    best = per_sym.argmin(0)                                                 # the first index among equal values
    err = np.array([add, adi, per_sym[best[0], 0], per_sym[best[1], 1]])
    sym_best = best.astype(np.int32)
    if behind:
        err[3], sym_best[1] = np.inf, -1
    return dict(err=err, sym_best=sym_best, status=2 if behind else 0, per_sym=per_sym)


def pose_errors(meshes, groups, job_mesh, job_sym, pose_est, pose_gt, camk, near=0.01):
    """the kernel's call: meshes list of (verts, faces), groups list of (Q,3,4), camk (J,4)
    -> dict err (J,4) float64, sym_best (J,2) int32, status (J,) int32, per_sym list of (Q,2) or None"""
    J = len(job_mesh)
    err, sym_best, status, per_sym = np.full((J, 4), np.nan), np.full((J, 2), -1, np.int32), np.zeros(J, np.int32), []
    for j in range(J):
        mi, gi = int(job_mesh[j]), int(job_sym[j])
        if not (0 <= mi < len(meshes) and 0 <= gi < len(groups)):
            status[j] = 1
            per_sym.append(None)
            continue
        r = job_errors(meshes[mi][0], pose_est[j], pose_gt[j], groups[gi], camk[j], near)
        err[j], sym_best[j], status[j] = r["err"], r["sym_best"], r["status"]
        per_sym.append(r["per_sym"])
    return dict(err=err, sym_best=sym_best, status=status, per_sym=per_sym)


def scale_L(meshes, groups, job_mesh, job_sym, pose_est, pose_gt, camk):
    """per job: L = 1 + the largest absolute coordinate of any transformed point (E p, G p, S p, G S p, and p itself), and z_min =
    the least z of any projected point; NaN for a job out of range"""
    out = np.full((len(job_mesh), 2), np.nan)
    for j in range(len(job_mesh)):
        mi, gi = int(job_mesh[j]), int(job_sym[j])
        if not (0 <= mi < len(meshes) and 0 <= gi < len(groups)) or not (np.isfinite(pose_est[j]).all() and np.isfinite(pose_gt[j]).all()):
            continue
        p = np.asarray(meshes[mi][0], np.float32).astype(np.float64)
        e = apply(pose_est[j], p)
        big, zmin = max(np.abs(p).max(), np.abs(e).max()), e[:, 2].min()
        for S in np.asarray(groups[gi], np.float32):
            sp = apply(S, p)
            gs = apply(pose_gt[j], sp)
            big, zmin = max(big, np.abs(sp).max(), np.abs(gs).max()), min(zmin, gs[:, 2].min())
        out[j] = 1.0 + big, zmin
    return out


def vsd_job(mesh, pose_est, pose_gt, camk, depth, taus, delta, near=0.01):
    """one job -> (counts (8,) int32, within (n_tau,) int32, err (n_tau,) float32)"""
    H, W = depth.shape
    re = render_ref.render_scene([mesh], [(0, 1, pose_est)], camk, H, W, near)
    rg = render_ref.render_scene([mesh], [(0, 1, pose_gt)], camk, H, W, near)
    d_e, d_g, d_o = re["depth"].astype(np.int64), rg["depth"].astype(np.int64), depth.astype(np.int64)
    vis = lambda d: (d > 0) & ((d_o == 0) | (d - d_o <= delta))
    visib_gt = vis(d_g)
    visib_est = vis(d_e) | (visib_gt & (d_e > 0))
    inter, union = visib_gt & visib_est, visib_gt | visib_est
    counts = np.array([(d_g > 0).sum(), (d_e > 0).sum(), visib_gt.sum(), visib_est.sum(), inter.sum(), union.sum(), rg["dropped"].sum(),
                       re["dropped"].sum()], dtype=np.int32)
    within = np.array([(inter & (np.abs(d_g - d_e) < int(t))).sum() for t in taus], dtype=np.int32)
    un = counts[VCOL["union"]]
    err = (un - within).astype(np.float32) / np.float32(un) if un > 0 else np.ones(len(taus), np.float32)   # exact conversions, one division
    return counts, within, err.astype(np.float32)


def pose_vsd(meshes, depth, camk, job_img, job_mesh, pose_est, pose_gt, job_tau, delta=15, near=0.01):
    """the kernel's call: depth (S,H,W) uint16, camk (S,4), job_tau (J,n_tau) int -> dict counts (J,8) int32, within (J,n_tau)
    int32, err (J,n_tau) float32.  A job whose frame or mesh index is out of range is zeros with err 1.  A threshold is compared as
    the int it is: the kernel reads them on the device and refuses none, so one below 1 counts nothing and one above 65535 counts
    every inter pixel."""
    depth = np.asarray(depth)
    job_tau = np.asarray(job_tau)
    assert depth.dtype == np.uint16 and depth.ndim == 3 and isinstance(delta, int) and 0 <= delta <= 65535
    assert job_tau.ndim == 2 and 1 <= job_tau.shape[1] <= MAX_TAUS
    S, J, n_tau = depth.shape[0], len(job_img), job_tau.shape[1]
    counts, within, err = np.zeros((J, 8), np.int32), np.zeros((J, n_tau), np.int32), np.ones((J, n_tau), np.float32)
    for j in range(J):
        img, mi = int(job_img[j]), int(job_mesh[j])
        if 0 <= img < S and 0 <= mi < len(meshes):
            counts[j], within[j], err[j] = vsd_job(meshes[mi], pose_est[j], pose_gt[j], camk[img], depth[img], job_tau[j], delta, near)
    return dict(counts=counts, within=within, err=err)
