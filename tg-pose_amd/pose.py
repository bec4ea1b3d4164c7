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


def scan_models(volumes, depth, camk, RTs, scales=None, job_img=None, job_model=None, trunc_mm=None, near=0.01, mask=None,
                job_mask_val=None):
    """TSDF fusion (ops.tsdf_integrate) of depth frames (S,H,W) into ``volumes`` (ops.TsdfVolumes) at the project's 4x4 poses
    [s R | t], as verify_poses is ops.pose_verify's 4x4 form: job j fuses frame job_img[j] (default: frame 0) into volume
    job_model[j] (default: volume j) at RTs[j]; scales: see verify_job_pose (the volume is then in the normalised model's units).
    trunc_mm: the truncation in millimetres (default: two voxel edges of the coarsest volume, at the first pose's scale -- one
    read of RTs[0]; pass a number to read nothing back).  The job poses are built on the device.  -> status (J,) int32."""
    J, dev = RTs.shape[0], RTs.device
    if job_img is None:
        job_img = torch.zeros(J, dtype=torch.int32, device=dev)
    if job_model is None:
        job_model = torch.arange(J, dtype=torch.int32, device=dev)
    P = verify_job_pose(RTs, scales)
    if trunc_mm is None:
        trunc_mm = 2000.0 * float(volumes.meta_host[:, 3].max()) * float(P[0, :, :3].double().det().abs().pow(1.0 / 3.0))
    return ops.tsdf_integrate(volumes, depth, camk, job_img, job_model, P, trunc_mm, near=near, mask=mask, job_mask_val=job_mask_val)


RAYCAST_FEW_HITS = 4           # RaycastRefine's status beside ops.ICP_STATUS' 1..3: fewer than min_hits rays met the surface


class RaycastRefine(object):
    """Frame-to-model registration against TSDF volumes as they stand (DESIGN.md section 3 "Ray casting and frame-to-model
    tracking"): the surface each volume shows from its object's current pose is ray-cast (ops.tsdf_windows, ops.tsdf_raycast: h x w
    rays over the cube's image, h w <= ops.ICP_MAX_POINTS) into an ops.IcpModels (from_raycast), and the pose is registered to the
    frame's cloud by ONE ops.icp_refine call.  volumes: ops.TsdfVolumes; job_model: one volume index per object (default: object j
    is volume j); max_dist: the gate in metres; min_weight, step, near: the ray cast's; icp_kw: ops.icp_refine's keywords.
    __call__(clouds (J,n,3) camera metres, RTs (J,4,4) [s R | t], camk (S,4), job_img (J) int32, H, W: the frame's size)
    -> (RTs (J,4,4), info (J,4) int32, rmse (J,), hits (J,) int32).  A job with fewer than ``min_hits`` hits keeps the pose it
    came with and has status RAYCAST_FEW_HITS in info[:, 0].  Three launches and torch's glue; nothing is read back."""

    def __init__(self, volumes, max_dist, h=40, w=48, min_weight=1, step=1.0, near=0.01, min_hits=64, job_model=None, **icp_kw):
        if not isinstance(volumes, ops.TsdfVolumes):
            raise TypeError("RaycastRefine: volumes must be an ops.TsdfVolumes")
        if not (isinstance(h, int) and isinstance(w, int) and h >= 1 and w >= 1 and h * w <= ops.ICP_MAX_POINTS):
            raise ValueError("RaycastRefine: h x w rays must be at least 1 and at most %d" % ops.ICP_MAX_POINTS)
        if not (isinstance(min_hits, int) and min_hits >= 0):
            raise ValueError("RaycastRefine: min_hits must be an int >= 0")
        if icp_kw.get("return_corr"):
            raise ValueError("RaycastRefine: return_corr is ops.icp_refine's")
        dev = volumes.sum.device
        self.volumes, self.h, self.w, self.min_weight, self.step, self.near, self.min_hits = volumes, h, w, min_weight, step, near, min_hits
        self.job_model = None if job_model is None else torch.as_tensor(job_model, dtype=torch.int32).to(dev).contiguous()
        self.max_dist = max_dist.to(dev).float().contiguous() if torch.is_tensor(max_dist) else float(max_dist)
        self.kw = dict(icp_kw)

    def __call__(self, clouds, RTs, camk, job_img, H, W):
        J, dev = RTs.shape[0], RTs.device
        job_model = self.job_model if self.job_model is not None else torch.arange(J, dtype=torch.int32, device=dev)
        P = verify_job_pose(RTs)
        win = ops.tsdf_windows(self.volumes, camk, job_img, job_model, P, self.h, self.w, H, W)
        rc = ops.tsdf_raycast(self.volumes, camk, job_img, job_model, P, win, self.h, self.w, min_weight=self.min_weight, step=self.step,
                              near=self.near)
        models = ops.IcpModels.from_raycast(rc)
        new, info, rmse = refine_poses(models, torch.arange(J, dtype=torch.int32, device=dev), clouds, RTs, self.max_dist, **self.kw)
        few = rc["count"] < self.min_hits
        info = torch.cat([torch.where(few, torch.full_like(info[:, 0], RAYCAST_FEW_HITS), info[:, 0])[:, None], info[:, 1:]], 1)
        return torch.where(few[:, None, None], RTs, new), info, rmse, rc["count"]


class DenseRefine(object):
    """Frame-to-model registration against TSDF volumes by dense projective ICP (DESIGN.md section 3 "Dense projective
    registration"): the surface each volume shows from its object's current pose is ray-cast into h x w vertex and normal maps
    (ops.tsdf_windows, ops.tsdf_raycast), and the frame's depth pixels under each map (ops.dense_rects, every ``stride``-th a side)
    are registered to it by ONE ops.icp_dense call -- no crop, no sampler, no sort and no nearest-neighbour search between the ray
    cast and the solve.  volumes: ops.TsdfVolumes; job_model: one volume index per object (default: object j is volume j);
    max_dist: the gate in metres; min_weight, step, near: the ray cast's; kw: ops.icp_dense's keywords (iters, tol_rot, ...).
    __call__(depth (S,H,W) 16-bit millimetres, RTs (J,4,4) [s R | t], camk (S,4), job_img (J) int32, mask (S,H,W) uint8 with
    job_mask_val (J) uint8 or neither) -> (RTs (J,4,4), info (J,4) int32 = status, inliers, iterations, candidates, rmse (J,), hits
    (J,) int32).  A job with fewer than ``min_hits`` hits keeps the pose it came with and has status RAYCAST_FEW_HITS in info[:, 0].
    Two launches and torch's glue; nothing is read back."""

    def __init__(self, volumes, max_dist, h=96, w=128, stride=1, min_weight=1, step=1.0, near=0.01, min_hits=64, job_model=None, **kw):
        if not isinstance(volumes, ops.TsdfVolumes):
            raise TypeError("DenseRefine: volumes must be an ops.TsdfVolumes")
        if not (isinstance(h, int) and isinstance(w, int) and 1 <= h <= ops.RAYCAST_MAX_SIDE and 1 <= w <= ops.RAYCAST_MAX_SIDE):
            raise ValueError("DenseRefine: h and w must be ints in [1, %d]" % ops.RAYCAST_MAX_SIDE)
        if not (isinstance(stride, int) and stride >= 1):
            raise ValueError("DenseRefine: stride must be an int >= 1")
        if not (isinstance(min_hits, int) and min_hits >= 0):
            raise ValueError("DenseRefine: min_hits must be an int >= 0")
        if kw.get("corr_cap"):
            raise ValueError("DenseRefine: corr_cap is ops.icp_dense's")
        dev = volumes.sum.device
        self.volumes, self.h, self.w, self.stride, self.min_weight, self.step, self.near, self.min_hits = volumes, h, w, stride, min_weight, step, near, min_hits
        self.job_model = None if job_model is None else torch.as_tensor(job_model, dtype=torch.int32).to(dev).contiguous()
        self.max_dist = max_dist.to(dev).float().contiguous() if torch.is_tensor(max_dist) else float(max_dist)
        self.kw = dict(kw)

    def __call__(self, depth, RTs, camk, job_img, mask=None, job_mask_val=None):
        J, dev = RTs.shape[0], RTs.device
        H, W = depth.shape[1:]
        job_model = self.job_model if self.job_model is not None else torch.arange(J, dtype=torch.int32, device=dev)
        P = verify_job_pose(RTs)
        win = ops.tsdf_windows(self.volumes, camk, job_img, job_model, P, self.h, self.w, H, W)
        rc = ops.tsdf_raycast(self.volumes, camk, job_img, job_model, P, win, self.h, self.w, min_weight=self.min_weight, step=self.step,
                              near=self.near)
        rect = ops.dense_rects(win, self.h, self.w, H, W)
        R, t, s = split_RT(RTs)
        R, t, s, info, rmse = ops.icp_dense(depth, camk, job_img, rect, rc, win, P, R, t, s, self.max_dist, stride=self.stride, mask=mask,
                                            job_mask_val=job_mask_val, **self.kw)
        few = rc["count"] < self.min_hits
        info = torch.cat([torch.where(few, torch.full_like(info[:, 0], RAYCAST_FEW_HITS), info[:, 0])[:, None], info[:, 1:]], 1)
        return torch.where(few[:, None, None], RTs, join_RT(R, t, s)), info, rmse, rc["count"]


DENSE_GATED = 5                # DenseModelRefine's status beside 1..4: the solve succeeded and failed the inlier / rmse gate


class DenseModelRefine(object):
    """Frame-to-model registration against MESH models by dense projective ICP (DESIGN.md section 3 "Mesh maps and dense model-based
    tracking"): each object's mesh is rasterised at its current pose into h x w vertex and normal maps (ops.mesh_windows,
    ops.mesh_maps), and the frame's depth pixels under each map (ops.dense_rects, every ``stride``-th a side) are registered to it by
    ONE ops.icp_dense call -- DenseRefine with a mesh where it has a volume: no crop, no sampler, no nearest-neighbour search, and
    every depth pixel of the object takes part.  meshset: ops.MeshSet in the model's units, posed by RTs = [s R | t] as they stand
    (pose.Verify's and IcpRefine's convention); job_mesh: one mesh index per object; max_dist: the gate in metres; near, normals:
    ops.mesh_maps'; kw: ops.icp_dense's keywords (iters, tol_rot, ...).
    __call__(depth (S,H,W) 16-bit millimetres, RTs (J,4,4) [s R | t], camk (S,4), job_img (J) int32, mask (S,H,W) uint8 with
    job_mask_val (J) uint8 or neither) -> (RTs (J,4,4), info (J,4) int32 = status, inliers, iterations, candidates, rmse (J,), hits
    (J,) int32).  A job keeps the pose it came with unless its status is 0: RAYCAST_FEW_HITS for fewer than ``min_hits`` map hits;
    ops.ICP_STATUS' 1..3 from the solve; DENSE_GATED for a solve that succeeded with fewer inliers than ``min_inlier_frac`` x its
    candidates (the pixels its map associated at the start pose) or, with ``max_rmse`` (metres), a larger rmse.  Three launches and
    torch's glue; nothing is read back (it runs under torch.cuda.set_sync_debug_mode("error"))."""

    def __init__(self, meshset, job_mesh, max_dist, h=96, w=128, stride=1, near=0.01, min_hits=64, normals="face", min_inlier_frac=0.5,
                 max_rmse=None, **kw):
        self.job_mesh = ops._mesh_jobs(meshset, job_mesh, "DenseModelRefine")
        if not (isinstance(h, int) and isinstance(w, int) and 1 <= h <= ops.RAYCAST_MAX_SIDE and 1 <= w <= ops.RAYCAST_MAX_SIDE):
            raise ValueError("DenseModelRefine: h and w must be ints in [1, %d]" % ops.RAYCAST_MAX_SIDE)
        if not (isinstance(stride, int) and stride >= 1):
            raise ValueError("DenseModelRefine: stride must be an int >= 1")
        if not (isinstance(min_hits, int) and min_hits >= 0):
            raise ValueError("DenseModelRefine: min_hits must be an int >= 0")
        if normals not in ("face", "vertex") or (normals == "vertex" and meshset.vert_normals is None):
            raise ValueError("DenseModelRefine: normals must be 'face' or 'vertex', and 'vertex' needs meshset.vert_normals")
        if not 0.0 <= float(min_inlier_frac) <= 1.0:
            raise ValueError("DenseModelRefine: min_inlier_frac must be in [0, 1]")
        if not float(near) > 0.0:
            raise ValueError("DenseModelRefine: near must be positive")
        if kw.get("corr_cap"):
            raise ValueError("DenseModelRefine: corr_cap is ops.icp_dense's")
        dev = meshset.verts.device
        self.meshset, self.h, self.w, self.stride, self.near, self.min_hits, self.normals = meshset, h, w, stride, float(near), min_hits, normals
        self.min_inlier_frac, self.max_rmse = float(min_inlier_frac), None if max_rmse is None else float(max_rmse)
        self.max_dist = max_dist.to(dev).float().contiguous() if torch.is_tensor(max_dist) else float(max_dist)
        self.kw = dict(kw)

    def __call__(self, depth, RTs, camk, job_img, mask=None, job_mask_val=None):
        J = RTs.shape[0]
        if self.job_mesh.numel() != J:
            raise ValueError("DenseModelRefine: %d mesh indices for %d poses" % (self.job_mesh.numel(), J))
        H, W = depth.shape[1:]
        P = verify_job_pose(RTs)
        win = ops.mesh_windows(self.meshset, camk, job_img, self.job_mesh, P, self.h, self.w, H, W)
        maps = ops.mesh_maps(self.meshset, camk, job_img, self.job_mesh, P, win, self.h, self.w, near=self.near, normals=self.normals)
        rect = ops.dense_rects(win, self.h, self.w, H, W)
        R, t, s = split_RT(RTs)
        R, t, s, info, rmse = ops.icp_dense(depth, camk, job_img, rect, maps, win, P, R, t, s, self.max_dist, stride=self.stride, mask=mask,
                                            job_mask_val=job_mask_val, **self.kw)
        solved = info[:, 0] == 0
        passed = info[:, 1].float() >= self.min_inlier_frac * info[:, 3].float()
        if self.max_rmse is not None:
            passed = passed & (rmse <= self.max_rmse)
        few = maps["count"] < self.min_hits
        status = torch.where(solved & ~passed, torch.full_like(info[:, 0], DENSE_GATED), info[:, 0])
        status = torch.where(few, torch.full_like(status, RAYCAST_FEW_HITS), status)
        info = torch.cat([status[:, None], info[:, 1:]], 1)
        return torch.where((status == 0)[:, None, None], join_RT(R, t, s), RTs), info, rmse, maps["count"]


def cloud_anchors(clouds, counts=None):
    """The mean of each cloud's finite rows (of the first counts[j] rows): float64 sums on the device, rounded once -> (J,3) float32;
    a cloud without a finite row gives 0."""
    fin = torch.isfinite(clouds).all(-1)
    if counts is not None:
        fin = fin & (torch.arange(clouds.shape[1], device=clouds.device)[None, :] < counts[:, None])
    total = torch.where(fin[:, :, None], clouds.double(), torch.zeros((), dtype=torch.float64, device=clouds.device)).sum(1)
    return (total / fin.sum(1).clamp(min=1)[:, None]).float().contiguous()


def search_poses(fields, job_model, clouds, scales, rotations, counts=None, **kw):
    """ops.pose_search with each cloud's mean (cloud_anchors) as its anchor: the point tried at the centre of the model's cube and,
    through K and stride, around it.  fields: ops.DistanceFields; job_model (J) int32; clouds (J,n,3) float32 camera-frame metres
    (NaN rows count for nothing); scales (J) float32 metres per model unit; rotations (R,3,3) float32; kw: K, stride, top,
    return_table.  -> ops.pose_search's dict plus 'anchors' (J,3).  Nothing is read back."""
    anchors = cloud_anchors(clouds, counts)
    out = ops.pose_search(fields, job_model, clouds, counts, anchors, scales, rotations, **kw)
    out["anchors"] = anchors
    return out


def _first_where(mask):
    """(J, top) bool -> (J,) the first True column (top where none)"""
    top = mask.shape[1]
    cols = torch.arange(top, device=mask.device)[None, :].expand_as(mask)
    return torch.where(mask, cols, torch.full_like(cols, top)).min(1).values


class ModelSearch(object):
    """Poses from mesh models alone (DESIGN.md section 3 "Model-based acquisition"): for each cloud the ``top`` rotations of least
    distance-field cost with their translations (search_poses), all J * top candidates refined in ONE ops.icp_refine call, all
    checked against the frame in ONE ops.pose_verify call, one candidate kept per job.

    fields: ops.DistanceFields built from ``models`` (ops.IcpModels); rotations (R,3,3) float32 (a tensor on the models' device, or
    an array: tools.lynne_lib.view_sampler.rotation_grid); K, stride, top: ops.pose_search's.  refine (a pose.IcpRefine; its models,
    gate and keywords are used, its job_model is not: the candidates' models are the call's) or None; verify (a pose.Verify; its
    meshes are in the models' units; its job_mesh holds one mesh index per job, or one for all) or None.
    Kept per job: with verify the candidate of the highest score, ties to the lower search rank; without it the one with the most
    ICP inliers, then the least rmse, then the lower rank; without refine rank 0.

    __call__(clouds (J,n,3), job_model (J) int32, scales (J) float32, depth, camk, job_img, mask, job_mask_val, counts) -> dict of
    device tensors: RTs (J,4,4) [s R | t], search_cost, search_rank (J) int32, candidates (J,top,4,4) (after ICP where it ran) and
    cand_cost (J,top); with refine icp_status, icp_inliers (J) int32, icp_rmse (J); with verify verify_score (J) and verify_counts
    (J,8).  A job without a candidate (ops.SEARCH_REFUSED) has search_rank 0 and a NaN pose.  Nothing is read back."""

    def __init__(self, fields, models, rotations, K=5, stride=2, top=16, refine=None, verify=None):
        if not isinstance(fields, ops.DistanceFields):
            raise TypeError("ModelSearch: fields must be an ops.DistanceFields")
        if not isinstance(models, ops.IcpModels) or fields.models is not models:
            raise ValueError("ModelSearch: models must be the ops.IcpModels the fields were built from")
        if refine is not None and not isinstance(refine, IcpRefine):
            raise TypeError("ModelSearch: refine must be a pose.IcpRefine")
        if verify is not None and not isinstance(verify, Verify):
            raise TypeError("ModelSearch: verify must be a pose.Verify")
        if verify is not None and verify.normalised:
            raise ValueError("ModelSearch: verify's meshes must be in the models' units (normalised=False)")
        dev = models.points_normals.device
        rotations = torch.as_tensor(rotations, dtype=torch.float32).to(dev).contiguous()
        if rotations.dim() != 3 or rotations.shape[1:] != (3, 3) or not 1 <= rotations.shape[0] <= ops.SEARCH_MAX_ROTATIONS:
            raise ValueError("ModelSearch: rotations must be (R,3,3) with 1 <= R <= %d" % ops.SEARCH_MAX_ROTATIONS)
        if not (isinstance(K, int) and 0 <= K <= ops.SEARCH_MAX_K and isinstance(stride, int) and stride >= 1 and K * stride <= ops.SEARCH_MAX_REACH):
            raise ValueError("ModelSearch: K must be an int in [0, %d], stride an int >= 1 and K * stride <= %d" % (ops.SEARCH_MAX_K, ops.SEARCH_MAX_REACH))
        if not (isinstance(top, int) and 1 <= top <= ops.SEARCH_MAX_TOP):
            raise ValueError("ModelSearch: top must be an int in [1, %d]" % ops.SEARCH_MAX_TOP)
        self.fields, self.models, self.rotations, self.K, self.stride, self.top = fields, models, rotations, K, stride, top
        self.refine, self.verify = refine, verify

    def __call__(self, clouds, job_model, scales, depth=None, camk=None, job_img=None, mask=None, job_mask_val=None, counts=None):
        J, top, dev = clouds.shape[0], self.top, clouds.device
        if self.verify is not None and (depth is None or camk is None):
            raise ValueError("ModelSearch: verify needs the depth frames and their intrinsics")
        found = search_poses(self.fields, job_model, clouds, scales, self.rotations, counts, K=self.K, stride=self.stride, top=top)
        valid = found["rot"] >= 0                                                     # (J, top)
        R = found["poses"][:, :, :, :3].reshape(J * top, 3, 3).contiguous()
        t = found["poses"][:, :, :, 3].reshape(J * top, 3).contiguous()
        s = scales.repeat_interleave(top).contiguous()
        out = {}
        if self.refine is not None:
            ref = self.refine
            gate = ref.max_dist.repeat_interleave(top).contiguous() if torch.is_tensor(ref.max_dist) else ref.max_dist
            Rn, tn, sn, info, rmse = ops.icp_refine(ref.models, job_model.repeat_interleave(top).contiguous(),
                                                    clouds.repeat_interleave(top, dim=0).contiguous(), R, t, s, gate,
                                                    src_count=None if counts is None else counts.repeat_interleave(top).contiguous(), **ref.kw)
            good = (info[:, 0] == 0) & valid.reshape(-1)
            R, t, s = torch.where(good[:, None, None], Rn, R), torch.where(good[:, None], tn, t), torch.where(good, sn, s)
            info, rmse = info.reshape(J, top, 4), rmse.reshape(J, top)
        cand = join_RT(R, t, s)
        if self.verify is not None:
            vmesh = self.verify.jobs(J)
            rep = lambda x: None if x is None else x.repeat_interleave(top).contiguous()
            img = torch.zeros(J, dtype=torch.int32, device=dev) if job_img is None else job_img
            vf = self.verify.on(rep(vmesh))(depth, camk, torch.nan_to_num(cand, nan=0.0), None, job_img=rep(img), mask=mask,
                                            job_mask_val=rep(job_mask_val))
            score = torch.where(valid, vf["score"].reshape(J, top), torch.full((), -1.0, device=dev))
            rank = _first_where(score == score.max(1, keepdim=True).values)
        elif self.refine is not None:
            inl = torch.where(valid & (info[:, :, 0] == 0), info[:, :, 1], torch.full((), -1, dtype=torch.int32, device=dev))
            most = inl == inl.max(1, keepdim=True).values
            err = torch.where(most, torch.nan_to_num(rmse, nan=float("inf")), torch.full((), float("inf"), device=dev))
            rank = _first_where(most & (err == err.min(1, keepdim=True).values))
        else:
            rank = torch.zeros(J, dtype=torch.int64, device=dev)
        rank = rank.clamp(max=top - 1)
        pick = lambda x: x[torch.arange(J, device=dev), rank].contiguous()           # x is (J, top, ...)
        cand = cand.reshape(J, top, 4, 4)
        out.update(RTs=pick(cand), search_cost=pick(found["cost"]), search_rank=rank.to(torch.int32), candidates=cand,
                   cand_cost=found["cost"], anchors=found["anchors"])
        if self.refine is not None:
            chosen = pick(info)
            out.update(icp_status=chosen[:, 0].contiguous(), icp_inliers=chosen[:, 1].contiguous(), icp_rmse=pick(rmse))
        if self.verify is not None:
            out.update(verify_score=pick(vf["score"].reshape(J, top)), verify_counts=pick(vf["counts"].reshape(J, top, -1)))
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
