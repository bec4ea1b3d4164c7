"""Pose assembly for the evaluation driver.

``generate_RT`` stands where ``tools.geom_utils.generate_RT`` stands in the reference
(``evaluater/RT_TDA_Evaluater.py:7,94``); the reference ships that module only as py3.8 bytecode, its semantics
are recorded in SURVEY.md section 8c.  ``batched_inference`` is the cross-image batching the reference lacks: it
runs one forward over the detections of many images and returns per-image ``pred_RTs`` / ``pred_scales`` with a
single device-to-host copy at the end (the reference synchronises per image, RT_TDA_Evaluater.py:97-98).
"""
import torch

from . import ops


def generate_RT(R, f, T, mode="vec", sym=None):
    """R = [p_green (B,3), p_red (B,3)], f = [f_green (B,), f_red (B,)], T (B,3), sym (B,4) -> (B,4,4)"""
    if mode != "vec":
        raise NotImplementedError("only mode='vec' is used by the reference's evaluater")
    return ops.generate_rt(R[0], R[1], f[0], f[1], T, sym)


def infer_device(net, pts, cat, ms, sym, max_batch=256, eval_outputs_only=None, recon_out=None):
    """One or more forwards over (n,N,3) clouds already on the device -> (pred_RTs (n,4,4), pred_scales (n,3)) device tensors;
    nothing synchronises (the caller decides when to copy back).  eval_outputs_only: handed to each forward (None = the net's /
    the process's setting): the six pose outputs are all this function reads.  recon_out (a list): the forwards run full and
    each one's reconstruction (b,N,3) is appended."""
    rts, scales = [], []
    kw = {} if eval_outputs_only is None else dict(eval_outputs_only=bool(eval_outputs_only))
    for lo in range(0, pts.shape[0], max_batch):
        if recon_out is not None:
            kw["probe"] = {}
        out = net(pts[lo:lo + max_batch], cat[lo:lo + max_batch], **kw)
        if recon_out is not None:
            recon_out.append(kw["probe"]["recon"])
        rts.append(generate_RT([out["p_green_R"], out["p_red_R"]], [out["f_green_R"], out["f_red_R"]], out["Pred_T"],
                               mode="vec", sym=sym[lo:lo + max_batch]))
        scales.append(out["Pred_s"] + ms[lo:lo + max_batch])
    return torch.cat(rts), torch.cat(scales)


def split_RT(RTs):
    """(J,4,4) [s R | t] -> (R (J,3,3), t (J,3), s (J,)) with s = cbrt(det), elementwise torch ops on RTs' device (no read-back)"""
    A = RTs[:, :3, :3]
    det = (A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1]) - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0])
           + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]))
    s = torch.sign(det) * det.abs().pow(1.0 / 3.0)
    return (A / s[:, None, None]).contiguous(), RTs[:, :3, 3].contiguous(), s.contiguous()


def join_RT(R, t, s):
    """the inverse of split_RT"""
    RTs = torch.zeros(R.shape[0], 4, 4, device=R.device, dtype=R.dtype)
    RTs[:, :3, :3] = R * s[:, None, None]
    RTs[:, :3, 3] = t
    RTs[:, 3, 3] = 1.0
    return RTs


def refine_poses(models, job_model, clouds, RTs, max_dist, **kw):
    """ICP refinement (ops.icp_refine) of the project's 4x4 poses [s R | t] against clouds (J,n,3) in camera-frame metres, as
    load_data_eval.clouds_from_poses cuts them (NaN rows of failed crops are never inliers).  models: ops.IcpModels; job_model (J)
    int32; max_dist: the gate in metres, (J,) or one number; kw: icp_refine's keywords.  The poses are taken apart and put together on
    the device.  -> (RTs (J,4,4), info (J,4) int32, rmse (J,)); a job whose status info[:, 0] is not 0 returns the pose of its last
    good iteration, put together again (equal to the pose it came with to rounding when that is the start)."""
    if kw.get("return_corr"):
        raise ValueError("refine_poses: return_corr is ops.icp_refine's")
    R, t, s = split_RT(RTs)
    R, t, s, info, rmse = ops.icp_refine(models, job_model, clouds, R, t, s, max_dist, **kw)
    return join_RT(R, t, s), info, rmse


class IcpRefine(object):
    """What myEvaluater.track(refine=...) needs to refine its objects' poses: ``models`` (ops.IcpModels), ``job_model`` (one model
    index per tracked object; kept as an int32 tensor on the models' device), ``max_dist`` (the gate in metres, one number or one
    per object) and ops.icp_refine's keywords (mode, iters, tol_rot, ...)."""

    def __init__(self, models, job_model, max_dist, **kw):
        if not isinstance(models, ops.IcpModels):
            raise TypeError("IcpRefine: models must be an ops.IcpModels")
        dev = models.points_normals.device
        self.models = models
        self.job_model = torch.as_tensor(job_model, dtype=torch.int32).to(dev).contiguous()
        self.max_dist = max_dist.to(dev).float().contiguous() if torch.is_tensor(max_dist) else float(max_dist)
        self.kw = dict(kw)

    def __call__(self, clouds, RTs):
        return refine_poses(self.models, self.job_model, clouds, RTs, self.max_dist, **self.kw)


class SupportPlane(object):
    """What myEvaluater.track(support=...) needs to take the supporting plane out of each frame before the crop: ops.plane_fit's
    ``tol`` (the inlier band, metres), ``hypotheses`` and ``refine_iters``, and ops.plane_cut's ``margin`` (metres above the plane
    below which a pixel goes).  __call__(depth (S,H,W), camk (S,4), keys, seed) -> (cut depth, plane (S,4), info (S,4)), device
    tensors, nothing read back; a frame without a plane (info[:, 0] != 0) comes back uncut."""

    def __init__(self, tol=0.004, margin=0.006, hypotheses=256, refine_iters=2, min_inliers=100):
        if not (tol >= 0 and margin >= 0):
            raise ValueError("SupportPlane: tol and margin must not be negative")
        self.tol, self.margin, self.hypotheses, self.refine_iters, self.min_inliers = float(tol), float(margin), int(hypotheses), int(refine_iters), int(min_inliers)

    def __call__(self, depth, camk, keys, seed):
        plane, info = ops.plane_fit(depth, camk, tol=self.tol, hypotheses=self.hypotheses, seed=seed, keys=keys, refine_iters=self.refine_iters,
                                    min_inliers=self.min_inliers)
        return ops.plane_cut(depth, plane, info, camk, self.margin), plane, info


class Segmenter(object):
    """What myEvaluater.acquire(segmenter=...) needs to split a (cut) depth frame into objects: ops.segment_depth's ``max_step``
    (millimetres between joined neighbours), ``connectivity`` (4 or 8), ``min_pixels`` (smaller components are dropped) and
    ``max_segments``.  __call__(depth (S,H,W), camk (S,4)) -> ops.Segments with centroids, device tensors, nothing read back."""

    def __init__(self, max_step=10, connectivity=4, min_pixels=50, max_segments=32):
        if not (isinstance(max_step, int) and 0 <= max_step <= 65535):
            raise ValueError("Segmenter: max_step must be an int in [0, 65535]")
        if connectivity not in (4, 8):
            raise ValueError("Segmenter: connectivity must be 4 or 8")
        if not (isinstance(min_pixels, int) and min_pixels >= 1):
            raise ValueError("Segmenter: min_pixels must be an int >= 1")
        if not (isinstance(max_segments, int) and 1 <= max_segments <= ops.SEG_MAX_SEGMENTS):
            raise ValueError("Segmenter: max_segments must be an int in [1, %d]" % ops.SEG_MAX_SEGMENTS)
        self.max_step, self.connectivity, self.min_pixels, self.max_segments = max_step, int(connectivity), min_pixels, max_segments

    def __call__(self, depth, camk):
        return ops.segment_depth(depth, max_step=self.max_step, connectivity=self.connectivity, min_pixels=self.min_pixels,
                                 max_segments=self.max_segments, camk=camk)


def verify_job_pose(RTs, scales=None):
    """The (J,3,4) float32 pose ops.pose_verify renders a mesh at, from the project's 4x4 poses, on their device.  scales None: the
    mesh is in the model's units and RTs = [s R | t] takes it to the camera in metres as it stands -- the convention of
    IcpRefine's models (refine_poses applies s R m + t to the model's points).  scales (J,3): the mesh is NORMALISED, each axis
    spanning one unit about the origin, and the object's size along its axes is carried by ``scales`` as in pose_balls: the
    linear part becomes RTs[:3,:3] @ diag(scales)."""
    P = RTs[:, :3, :4].float()
    if scales is not None:
        P = torch.cat([P[:, :, :3] * scales.float()[:, None, :], P[:, :, 3:]], dim=2)
    return P.contiguous()


def verify_poses(meshset, job_mesh, depth, camk, RTs, job_img=None, scales=None, tau=5, near=0.01, mask=None, job_mask_val=None):
    """Render-and-compare (ops.pose_verify) of the project's 4x4 poses [s R | t] against depth frames (S,H,W) in millimetres with
    intrinsics camk (S,4), as refine_poses is ops.icp_refine's 4x4 form.  job_mesh (J) int32: each pose's mesh in ``meshset``;
    job_img (J) int32: its frame (default: frame 0 for every job); scales: see verify_job_pose.  The job poses are built on the
    device; nothing is read back.  -> {'counts' (J,8) int32 in ops.VERIFY_COUNTS' order, 'score' (J,) float32}."""
    if job_img is None:
        job_img = torch.zeros(RTs.shape[0], dtype=torch.int32, device=RTs.device)
    return ops.pose_verify(meshset, depth, camk, job_img, job_mesh, verify_job_pose(RTs, scales), tau=tau, near=near, mask=mask,
                           job_mask_val=job_mask_val)


class Verify(object):
    """What myEvaluater.track(verify=...) and acquire_verified need to check their poses against the frame they came from:
    ``meshset`` (ops.MeshSet), ``job_mesh`` (one mesh index per object; kept as an int32 tensor on the set's device; a single
    index serves every object), ops.pose_verify's ``tau`` (millimetres) and ``near``, and ``min_score``: an object is 'verified'
    when its score reaches it.  The meshes are in the model's units and are posed by RTs = [s R | t] as they stand -- the models of
    IcpRefine built from the same set (ops.IcpModels.from_meshset) follow the same convention; with ``normalised`` the meshes span
    one unit per axis and the poses' linear part is RTs[:3,:3] @ diag(scales) (verify_job_pose).
    __call__(depth (S,H,W), camk (S,4), RTs (J,4,4), scales (J,3), job_img, mask, job_mask_val) -> {'counts', 'score', 'verified'
    (J,) bool}, device tensors, nothing read back.  Verification reports; it changes no pose."""

    def __init__(self, meshset, job_mesh, tau=5, min_score=0.5, near=0.01, normalised=False):
        self.job_mesh = ops._mesh_jobs(meshset, job_mesh, "Verify")
        if not (isinstance(tau, int) and 0 <= tau <= ops.VERIFY_MAX_TAU):
            raise ValueError("Verify: tau must be an int in [0, %d] (millimetres)" % ops.VERIFY_MAX_TAU)
        if not 0.0 <= float(min_score) <= 1.0:
            raise ValueError("Verify: min_score must be in [0, 1]")
        if not float(near) > 0.0:
            raise ValueError("Verify: near must be positive")
        self.meshset, self.tau, self.min_score, self.near, self.normalised = meshset, tau, float(min_score), float(near), bool(normalised)

    def on(self, job_mesh):
        """the same check for other objects"""
        return Verify(self.meshset, job_mesh, self.tau, self.min_score, self.near, self.normalised)

    def jobs(self, n):
        """job_mesh for n objects: as given, or the single index n times"""
        if self.job_mesh.numel() == 1 and n != 1:
            return self.job_mesh.expand(n).contiguous()
        if self.job_mesh.numel() != n:
            raise ValueError("Verify: %d mesh indices for %d objects" % (self.job_mesh.numel(), n))
        return self.job_mesh

    def __call__(self, depth, camk, RTs, scales=None, job_img=None, mask=None, job_mask_val=None):
        out = verify_poses(self.meshset, self.jobs(RTs.shape[0]), depth, camk, RTs, job_img, scales if self.normalised else None, self.tau,
                           self.near, mask, job_mask_val)
        out["verified"] = out["score"] >= self.min_score
        return out


def batched_inference(net, clouds, cat_ids, mean_shapes, syms, max_batch=256):
    """clouds: list over images of (n_det_i, N, 3) tensors (same N); cat_ids / mean_shapes / syms likewise.
    Returns a list over images of dicts {'pred_RTs': (n_det_i,4,4) ndarray, 'pred_scales': (n_det_i,3) ndarray}."""
    counts = [c.shape[0] for c in clouds]
    keep = [i for i, n in enumerate(counts) if n > 0]
    results = [dict(pred_RTs=torch.zeros(0, 4, 4).numpy(), pred_scales=torch.zeros(0, 4, 4).numpy()) for _ in counts]
    if not keep:
        return results
    dev = next(net.parameters()).device
    pts = torch.cat([clouds[i] for i in keep]).to(dev).float()
    cat = torch.cat([cat_ids[i].reshape(-1, 1) for i in keep]).to(dev).float()
    ms = torch.cat([mean_shapes[i] for i in keep]).to(dev).float()
    sym = torch.cat([syms[i] for i in keep]).to(dev).float()
    rts, scales = infer_device(net, pts, cat, ms, sym, max_batch)
    rts, scales = rts.cpu().numpy(), scales.cpu().numpy()                           # the only device-to-host copies
    pos = 0
    for i in keep:
        results[i] = dict(pred_RTs=rts[pos:pos + counts[i]], pred_scales=scales[pos:pos + counts[i]])
        pos += counts[i]
    return results
