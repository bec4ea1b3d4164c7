"""NumPy restatement of pose verification's contract (DESIGN.md section 3 "Pose verification"; the kernel is csrc/verify.hip).
Written from the contract's text: each job is rendered as a scene of its one instance by tests/render_ref.py -- the depth renderer's
restatement, so the rendered surface is the renderer's by construction -- and every covered pixel is classified against the frame
with integer arithmetic.  The score is one fp32 division of two exactly converted integers."""
import numpy as np

from tests import render_ref

COUNTS = ("rendered", "match", "violation", "occluded", "nodata", "in_mask", "abs_sum", "dropped")
COL = {name: i for i, name in enumerate(COUNTS)}
MAX_JOBS, MAX_TAU = 65535, 1000


def classify(d_r, covered, d_o, tau):
    """d_r (H,W) rendered millimetres, covered (H,W) bool, d_o (H,W) the frame's millimetres -> bool images nodata, occluded, match,
    violation: a partition of ``covered``, decided in this order"""
    d_r, d_o = d_r.astype(np.int64), d_o.astype(np.int64)
    nodata = covered & ((d_o == 0) | (d_r == 0))
    rest = covered & ~nodata
    occluded = rest & (d_o + tau < d_r)
    match = rest & (np.abs(d_o - d_r) <= tau)
    violation = rest & (d_o > d_r + tau)
    return nodata, occluded, match, violation


def verify_job(mesh, pose, camk, depth, tau, near=0.01, mask=None, mask_val=0):
    """one job: mesh (verts, faces), pose (3,4), camk (4,), depth (H,W) uint16 -> (counts (8,) int32, score float32)"""
    H, W = depth.shape
    r = render_ref.render_scene([mesh], [(0, 1, pose)], camk, H, W, near)
    covered = r["slot"] >= 0
    nodata, occluded, match, violation = classify(r["depth"], covered, depth, tau)
    diff = np.abs(depth.astype(np.int64) - r["depth"].astype(np.int64))
    in_mask = int((covered & (mask == mask_val)).sum()) if mask is not None else 0
    counts = np.array([covered.sum(), match.sum(), violation.sum(), occluded.sum(), nodata.sum(), in_mask, diff[match].sum(),
                       r["dropped"].sum()], dtype=np.int64)
    assert counts.max() < 2 ** 31
    den = counts[0] - counts[3]
    score = np.float32(counts[1]) / np.float32(den) if den > 0 else np.float32(0)
    return counts.astype(np.int32), np.float32(score)


def verify(meshes, depth, camk, job_img, job_mesh, job_pose, tau=5, near=0.01, mask=None, job_mask_val=None):
    """the kernel's call: depth (S,H,W) uint16, camk (S,4), J jobs -> dict counts (J,8) int32, score (J,) float32.  A job whose frame
    or mesh index is out of range is a row of zeros."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim == 3 and isinstance(tau, int) and 0 <= tau <= MAX_TAU
    assert (mask is None) == (job_mask_val is None)
    S, J = depth.shape[0], len(job_img)
    counts, score = np.zeros((J, len(COUNTS)), np.int32), np.zeros(J, np.float32)
    for j in range(J):
        img, mi = int(job_img[j]), int(job_mesh[j])
        if not (0 <= img < S and 0 <= mi < len(meshes)):
            continue
        counts[j], score[j] = verify_job(meshes[mi], job_pose[j], camk[img], depth[img], tau, near, None if mask is None else mask[img],
                                         None if mask is None else int(job_mask_val[j]))
    return dict(counts=counts, score=score)
