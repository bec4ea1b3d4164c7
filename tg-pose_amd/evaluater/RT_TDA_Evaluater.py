"""The evaluation driver (``evaluater/RT_TDA_Evaluater.py``: ``myEvaluater.run`` :55-109, ``calc_pose_metric`` :111-175) over the
device pipeline: frames -> clouds (``evaluation.load_data_eval``) -> ``PoseNet9D.forward`` -> pose assembly
(``pose``, f-1) -> NOCS mAP (``evaluation.metrics``, f-2).

The reference walks the dataset one image at a time: ``__getitem__`` builds the clouds on the CPU, ``run`` uploads them, runs a
forward of a handful of objects, assembles the poses and copies them back -- two synchronisations and a dozen tiny launches per
image.  ``run`` here takes the same per-image records minus the CPU cloud building (depth image + detection pickle + ground
truth) in chunks of ``frames_per_batch`` images: one ``tgp_roi_cloud`` launch, forwards of up to ``max_batch`` objects, one
device-to-host copy of the (n,4,4) / (n,3) results per chunk.  It returns the list the reference pickles
(``evaluation/evaluate.py:53-67``): the detection dict without ``pred_masks`` plus ``pred_RTs`` / ``pred_scales``, merged
with the ground-truth record.

The per-category tables are the reference's data (``evaluation/load_data_eval.py:477-545`` mean shapes in millimetres,
``:547-566`` symmetry flags); file reading stays with the caller.
"""
import os

import numpy as np
import torch

from .. import ops
from ..evaluation import load_data_eval as lde
from ..evaluation.metrics import compute_degree_cm_mAP
from ..losses.utils_v2.model_utils import calc_cd, calc_emd
from ..pose import DenseModelRefine, IcpRefine, ModelSearch, Segmenter, SupportPlane, Verify, infer_device, scan_models

SYNSET_NAMES = ['BG', 'bottle', 'bowl', 'camera', 'can', 'laptop', 'mug']                                   # :115
MEAN_SHAPE_MM = {1: (87, 220, 89), 2: (165, 80, 165), 3: (88, 128, 156), 4: (68, 146, 72), 5: (346, 200, 335), 6: (146, 83, 114)}
SYM_INFO = {1: (1, 1, 0, 1), 2: (1, 1, 0, 1), 3: (0, 0, 0, 0), 4: (1, 1, 1, 1), 5: (0, 1, 0, 0), 6: (0, 1, 0, 0)}


class myEvaluater:
    """``sampler='numpy'``: the reference's draws (one small read-back per chunk for the point counts).  ``sampler='device'``:
    nothing is read back until a chunk's poses are; with ``overlap`` (default) chunk c's results are fetched after chunk c+1
    has been enqueued, so packing / uploading the next frames runs beside the GPU's work on the current ones.
    ``sampler='fps'``: as 'device', with farthest point sampling of each detection's cloud (``fps_pool`` candidates at most,
    load_data_eval.clouds_from_frames) in place of the keyed draw: no random number enters, two runs give the same poses.

    ``recon_stats=True`` (what ``compute_degree_cm_mAP(eval_recon=True)`` reads, eval_utils_v1.py:1517-1518): the forwards run
    full -- the decoder is needed -- and each detection dict gains ``chamfer_dis_cass`` (``calc_cd``'s cd_p of the reconstruction
    against the input cloud, the ``Recon`` target of the training loss, trainer/RL_TDA.py:166) and ``emd_dis_cass`` (``calc_emd``
    with its defaults), one value per detection.  Not available together with ``graph``."""

    def __init__(self, net, frames_per_batch=32, max_batch=256, sampler="numpy", seed=0, overlap=True, graph=False,
                 recon_stats=False, fps_pool=4096):
        if sampler not in ("numpy", "device", "fps"):
            raise ValueError("sampler must be 'numpy', 'device' or 'fps'")
        self.fps_pool = int(fps_pool)
        if recon_stats and graph:
            raise ValueError("recon_stats is not available on the captured path: pass graph=False")
        self.recon_stats = bool(recon_stats)
        self.net1 = net.eval()
        # The driver reads the six pose outputs only (:143-150): PH predictor and decoder are dead code here, as in the reference's
        # eval dict, so its forwards run lean BY DEFAULT (TGP_EVAL_FULL_FORWARD=1 or eval_outputs_only=False: the full forward).
        # The setting is this evaluater's and travels with each call; the caller's module is not touched.
        self.eval_outputs_only = not os.environ.get("TGP_EVAL_FULL_FORWARD")
        self.device = next(net.parameters()).device
        self.frames_per_batch, self.max_batch, self.sampler, self.seed, self.overlap = frames_per_batch, max_batch, sampler, seed, overlap
        self.graph = graph                                   # replay the forward as a captured hipGraph (PoseNet9D.graph_replay)
        self._fetch = torch.cuda.Stream(device=self.device)  # results come back on their own stream (see _finish)

    def _launch(self, records, camK):
        """Enqueue everything for a chunk of frames; returns what _finish needs.  No synchronisation on the device-sampler path."""
        frames = [r["frame"] for r in records]
        per = [fr["pred_masks"].shape[2] for fr in frames]
        if self.sampler == "numpy":
            clouds = lde.clouds_from_frames(frames, camK, device=self.device)
            alive, ok = [c is not None for c in clouds], None
        else:
            clouds, ok = lde.clouds_from_frames(frames, camK, sampler=self.sampler, seed=self.seed, device=self.device,
                                                fps_pool=self.fps_pool)
            alive = [True] * len(frames)                     # decided in _finish from `ok`
            # an invalid detection's rows are NaN: zero them for the forward (objects are independent in eval mode) and drop
            # the frame afterwards, as the reference drops it (load_data_eval.py:332-337)
        kept = [i for i, a in enumerate(alive) if a and per[i] > 0]
        if not kept:
            return records, alive, ok, kept, None, None, None, None
        ids = [np.asarray(frames[i]["pred_class_ids"]).astype(np.int64) for i in kept]
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(self.device, non_blocking=True)
        flat = np.concatenate(ids)
        cat = t(flat - 1).reshape(-1, 1)                                                                   # cat_id_0base (:368)
        mean = t([MEAN_SHAPE_MM[int(c)] for c in flat]).reshape(-1, 3) / 1000.0                            # :362
        sym = t([SYM_INFO[int(c)] for c in flat]).reshape(-1, 4)
        pts = torch.cat([clouds[i] for i in kept])
        if ok is not None:
            pts = torch.nan_to_num(pts, nan=0.0)
        stats = None
        with torch.no_grad():
            if self.recon_stats:
                recon = []
                rts, scales = infer_device(self.net1, pts, cat, mean, sym, self.max_batch, eval_outputs_only=False, recon_out=recon)
                # scored in the forwards' own batches: a pair's EMD does not depend on the batch around it, nor does its Chamfer
                cmf = [calc_cd(r, pts[lo:lo + r.shape[0]])[0] for r, lo in zip(recon, range(0, pts.shape[0], self.max_batch))]
                emd = [calc_emd(r, pts[lo:lo + r.shape[0]]) for r, lo in zip(recon, range(0, pts.shape[0], self.max_batch))]
                stats = torch.stack([torch.cat(cmf), torch.cat(emd)])
            else:
                rts, scales = infer_device(self.net1, pts, cat, mean, sym, self.max_batch, eval_outputs_only=self.eval_outputs_only)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        return records, alive, ok, kept, rts, scales, done, stats

    def _finish(self, launched):
        records, alive, ok, kept, rts, scales, done, stats = launched
        # The copies back are stream-ordered: on the compute stream they would queue behind the NEXT chunk's forward, which
        # has already been enqueued, and the overlap would be lost.  They run on a fetch stream that waits only for this
        # chunk's event.
        with torch.cuda.stream(self._fetch):
            if done is not None:
                self._fetch.wait_event(done)
            if ok is not None and len(ok):
                flags = torch.stack([o.all() if o.numel() else torch.ones((), dtype=torch.bool, device=self.device) for o in ok])
                flags.record_stream(self._fetch)
                okc = flags.cpu().tolist()                   # first read-back of the chunk (device sampler)
                alive = [a and bool(b) for a, b in zip(alive, okc)]
            if rts is not None:
                rts.record_stream(self._fetch), scales.record_stream(self._fetch)
                rts, scales = rts.cpu().numpy(), scales.cpu().numpy()
            if stats is not None:
                stats.record_stream(self._fetch)
                stats = stats.cpu().numpy()
        out = []
        pos = 0
        empty = dict(pred_RTs=np.zeros((0, 4, 4)), pred_scales=np.zeros((0, 4, 4)))                       # RT_TDA_Evaluater.py:70-71
        if self.recon_stats:
            empty.update(chamfer_dis_cass=np.zeros(0, np.float32), emd_dis_cass=np.zeros(0, np.float32))
        for i, rec in enumerate(records):
            fr = rec["frame"]
            n = fr["pred_masks"].shape[2]
            pose = empty
            if i in kept:
                pose = dict(pred_RTs=rts[pos:pos + n], pred_scales=scales[pos:pos + n])
                if stats is not None:
                    pose.update(chamfer_dis_cass=stats[0, pos:pos + n], emd_dis_cass=stats[1, pos:pos + n])
                pos += n
            if not alive[i]:
                continue
            det = {k: v for k, v in fr.items() if k not in ("pred_masks", "depth")}
            det.update(pose)
            det.update(rec.get("gts", {}))
            out.append(det)
        return out

    def run(self, dataset, camK=lde.REAL_INTRINSICS):
        """dataset: iterable of {'frame': {'depth','pred_masks','pred_bboxes','pred_class_ids','pred_scores'}, 'gts': {...}}
        (None entries are skipped, as the reference skips them :66-67) -> pred_results list."""
        results, chunk, pending = [], [], None
        was = getattr(self.net1, "graph_replay", False)
        self.net1.graph_replay = bool(self.graph) or was

        def flush():
            nonlocal pending, chunk
            launched = self._launch(chunk, camK)
            chunk = []
            if pending is not None:
                results.extend(self._finish(pending))
            pending = launched
            if not self.overlap:
                results.extend(self._finish(pending))
                pending = None
        for rec in dataset:
            if rec is None:
                continue
            chunk.append(rec)
            if len(chunk) == self.frames_per_batch:
                flush()
        if chunk:
            flush()
        if pending is not None:
            results.extend(self._finish(pending))
        self.net1.graph_replay = was
        return results

    def acquire(self, frame, class_ids, camK=lde.REAL_INTRINSICS, support=None, segmenter=None, n_pts=1024, sampler=None):
        """The ``init`` that ``track`` takes, from one depth frame and a category: no detector result, no ground truth.

        frame: {'depth' (H,W) uint16}.  class_ids: one 1-based category id for every segment, or a sequence with one id per kept
        segment, in label order.  support (a pose.SupportPlane): the supporting plane is cut out first, with key 0 and seed =
        self.seed as ``track`` cuts frame 0.  segmenter (a pose.Segmenter; default Segmenter()): the frame's connected components
        (ops.segment_depth) are the objects.  sampler: 'device' (keyed draw, seed = self.seed) or 'fps'; default as in ``track``.

        Everything is enqueued without a read-back: the cut, the segmentation, load_data_eval.clouds_from_segments over the
        segmenter's max_segments slots, and ONE pose.infer_device forward over all of these slots (an empty slot's NaN cloud is zeroed;
        objects are independent in eval mode) -- how many segments were kept is only known on the device.  Then everything is read
        back once and cut down to the n kept segments.
        -> {'class_ids' (n,), 'RTs' (n,4,4), 'scales' (n,3), 'inst_ids' (n,) = the labels 1..n, 'inst_mask' (H,W) uint8 = the label
        image, 'boxes' (n,4) y1, x1, y2, x2 (ends exclusive), 'pixels' (n,), 'centers' (n,3) metres, 'ok' (n,) bool (False: the ROI
        path found the segment's cloud invalid, its pose is meaningless), 'info' (4,) int32 = ops.segment_depth's}; n = 0 for a
        frame without a segment."""
        return self._acquire(frame, class_ids, camK, support, segmenter, n_pts, sampler, None)

    def acquire_verified(self, frame, class_ids, verify, camK=lde.REAL_INTRINSICS, support=None, segmenter=None, n_pts=1024, sampler=None):
        """``acquire`` with its poses checked against the frame they came from.  verify (a pose.Verify; its job_mesh holds one mesh
        index for every segment, or one per kept segment in label order): the poses of all the segmenter's slots are verified in the
        same enqueue, before the one read-back -- against the cut depth when ``support`` is given, with the label image as the mask
        and each segment's label as its mask byte -- and the result gains 'verify_counts' (n,8) int32 (ops.VERIFY_COUNTS),
        'verify_score' (n,) float32 and 'verified' (n,) bool = score >= verify.min_score; n = 0 gives them with no row.
        (A method of its own: ``acquire``'s parameter list is part of what its callers and tests rely on.)"""
        if not isinstance(verify, Verify):
            raise TypeError("acquire_verified: verify must be a pose.Verify")
        return self._acquire(frame, class_ids, camK, support, segmenter, n_pts, sampler, verify)

    def acquire_models(self, frame, search, job_model, job_scale, camK=lde.REAL_INTRINSICS, support=None, segmenter=None, n_pts=128,
                       sampler=None):
        """The ``init`` that ``track`` takes, from one depth frame and mesh models alone: no network forward, no detector result, no
        ground truth (DESIGN.md section 3 "Model-based acquisition").  The constructor still wants a network (it reads the device
        from it); this method never touches it.

        frame, camK, support, segmenter, sampler: as ``acquire``.  search (a pose.ModelSearch: the distance fields, the rotation
        table, and optionally ICP and the render-and-compare check).  job_model: one model index for every segment, or a sequence
        with one per kept segment in label order; job_scale: metres per model unit, likewise.  n_pts (at most
        ops.SEARCH_MAX_POINTS): the points drawn per segment for the search and ICP.

        Everything is enqueued without a read-back, over the segmenter's max_segments slots: the cut, the segmentation,
        load_data_eval.clouds_from_segments, the search, ONE ICP call and ONE verify call over all slots x top candidates (against
        the cut depth when ``support`` is given, with the label image as the mask).  Then everything is read back once and cut down
        to the n kept segments.
        -> ``acquire``'s dict -- 'RTs' (n,4,4) = [s R | t] with s = job_scale, 'scales' (n,3) = the model's extent in model units
        (its points' bounding box; what ``track`` sizes its crop balls with), 'class_ids' (n,) all 1 (``track`` reads them for the
        network alone; init_from='previous' never does) -- plus 'search_cost' and 'search_rank' (n,) int32 (which candidate won),
        with ICP 'icp_status', 'icp_inliers' (n,) int32 and 'icp_rmse' (n,), with verify 'verify_score' (n,) and 'verify_counts'
        (n,8).  'ok' is False for a segment whose cloud the ROI path found invalid or that got no candidate."""
        if not isinstance(search, ModelSearch):
            raise TypeError("acquire_models: search must be a pose.ModelSearch")
        if support is not None and not isinstance(support, SupportPlane):
            raise TypeError("acquire_models: support must be a pose.SupportPlane")
        segmenter = Segmenter() if segmenter is None else segmenter
        if not isinstance(segmenter, Segmenter):
            raise TypeError("acquire_models: segmenter must be a pose.Segmenter")
        sampler = sampler or (self.sampler if self.sampler in ("device", "fps") else "device")
        if sampler not in ("device", "fps"):
            raise ValueError("acquire_models: sampler must be 'device' or 'fps' (nothing is read back before the search)")
        if not 1 <= int(n_pts) <= ops.SEARCH_MAX_POINTS:
            raise ValueError("acquire_models: n_pts must be in [1, %d]" % ops.SEARCH_MAX_POINTS)
        dev, M = self.device, segmenter.max_segments
        one_m, one_s = np.ndim(job_model) == 0, np.ndim(job_scale) == 0
        jm, js = np.asarray(job_model).astype(np.int64).reshape(-1), np.asarray(job_scale).astype(np.float32).reshape(-1)
        if len(jm) == 0 or len(js) == 0 or not all(0 <= int(m) < len(search.models) for m in jm) or not (js > 0).all():
            raise ValueError("acquire_models: job_model must index the search's %d models and job_scale be positive" % len(search.models))
        if max(len(jm), len(js)) > M:
            raise ValueError("acquire_models: more models or scales than the segmenter's %d slots" % M)
        slot_m, slot_s = np.full(M, jm[0], dtype=np.int32), np.full(M, js[0], dtype=np.float32)
        if not one_m:
            slot_m[:len(jm)] = jm
        if not one_s:
            slot_s[:len(js)] = js
        with torch.no_grad():
            depth, _, camk = lde._depth_frames([frame], camK, dev)
            if support is not None:
                depth = support(depth, camk, [0], self.seed)[0]
            seg = segmenter(depth, camk)
            pts, ok = lde.clouds_from_segments(depth, seg, camk, n_pts=n_pts, sampler=sampler, seed=self.seed, fps_pool=self.fps_pool)
            model_t = torch.from_numpy(slot_m).to(dev)
            found = search(pts.contiguous(), model_t, torch.from_numpy(slot_s).to(dev), depth=depth, camk=camk, mask=seg.labels,
                           job_mask_val=torch.arange(1, M + 1, device=dev).to(torch.uint8))
            ok = ok & (found["search_cost"] != 2 ** 31 - 1)
            meta = search.models.points_normals[:, :, :3]
            if search.models.counts is None:
                extent = meta.amax(1) - meta.amin(1)
            else:
                live = torch.arange(meta.shape[1], device=dev)[None, :, None] < search.models.counts[:, None, None]
                extent = torch.where(live, meta, -torch.inf).amax(1) - torch.where(live, meta, torch.inf).amin(1)
            scales = extent[model_t.long()]
        info = seg.info[0].cpu().numpy()                                                     # the read-back
        n = int(info[1])
        for what, given, one in (("job_model", jm, one_m), ("job_scale", js, one_s)):
            if not one and len(given) != n:
                raise ValueError("acquire_models: %d entries of %s for %d segments" % (len(given), what, n))
        stats = seg.stats[0, :n].cpu().numpy()
        out = {k: found[k][:n].cpu().numpy() for k in ("search_cost", "search_rank", "icp_status", "icp_inliers", "icp_rmse", "verify_score",
                                                       "verify_counts") if k in found}
        return dict(out, class_ids=np.ones(n, dtype=np.int64), RTs=found["RTs"][:n].cpu().numpy(), scales=scales[:n].cpu().numpy(),
                    inst_ids=np.arange(1, n + 1, dtype=np.int32), inst_mask=seg.labels[0].cpu().numpy(), boxes=stats[:, 1:5].copy(),
                    pixels=stats[:, 0].copy(), centers=seg.centers[0, :n].cpu().numpy(), ok=ok[:n].cpu().numpy(), info=info)

    def _acquire(self, frame, class_ids, camK, support, segmenter, n_pts, sampler, verify):
        if support is not None and not isinstance(support, SupportPlane):
            raise TypeError("acquire: support must be a pose.SupportPlane")
        segmenter = Segmenter() if segmenter is None else segmenter
        if not isinstance(segmenter, Segmenter):
            raise TypeError("acquire: segmenter must be a pose.Segmenter")
        sampler = sampler or (self.sampler if self.sampler in ("device", "fps") else "device")
        if sampler not in ("device", "fps"):
            raise ValueError("acquire: sampler must be 'device' or 'fps' (nothing is read back before the forward)")
        one = np.ndim(class_ids) == 0
        ids = np.asarray(class_ids).astype(np.int64).reshape(-1)
        if not all(int(c) in MEAN_SHAPE_MM for c in ids):
            raise ValueError("acquire: class_ids must be 1-based category ids in [1, %d]" % len(MEAN_SHAPE_MM))
        dev, M = self.device, segmenter.max_segments
        if not one and len(ids) > M:
            raise ValueError("acquire: %d class_ids for at most %d segments" % (len(ids), M))
        slot_ids = np.full(M, ids[0] if len(ids) else 1, dtype=np.int64)
        if not one:
            slot_ids[:len(ids)] = ids
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev)
        cat = t(slot_ids - 1).reshape(-1, 1)
        mean = t([MEAN_SHAPE_MM[int(c)] for c in slot_ids]).reshape(-1, 3) / 1000.0
        sym = t([SYM_INFO[int(c)] for c in slot_ids]).reshape(-1, 4)
        with torch.no_grad():
            depth, _, camk = lde._depth_frames([frame], camK, dev)
            if support is not None:
                depth = support(depth, camk, [0], self.seed)[0]
            seg = segmenter(depth, camk)
            pts, ok = lde.clouds_from_segments(depth, seg, camk, n_pts=n_pts, sampler=sampler, seed=self.seed, fps_pool=self.fps_pool)
            rts, scales = infer_device(self.net1, torch.nan_to_num(pts, nan=0.0), cat, mean, sym, self.max_batch,
                                       eval_outputs_only=self.eval_outputs_only)
            vf = None
            if verify is not None:
                # every slot is a job (how many are kept is only known on the device); an empty slot's row is cut off below
                vmesh = verify.job_mesh
                if vmesh.numel() != 1:                       # one per kept segment: the slots behind them take the first
                    vmesh = torch.cat([vmesh, vmesh[:1].expand(max(M - vmesh.numel(), 0))])[:M].contiguous()
                vf = verify.on(vmesh)(depth, camk, rts, scales, mask=seg.labels,
                                      job_mask_val=torch.arange(1, M + 1, device=dev).to(torch.uint8))
        info = seg.info[0].cpu().numpy()                                                     # the read-back
        n = int(info[1])
        if not one and len(ids) != n:
            raise ValueError("acquire: %d class_ids for %d segments" % (len(ids), n))
        if vf is not None and verify.job_mesh.numel() not in (1, n):
            raise ValueError("acquire_verified: %d mesh indices for %d segments" % (verify.job_mesh.numel(), n))
        stats = seg.stats[0, :n].cpu().numpy()
        out = {} if vf is None else dict(verify_counts=vf["counts"][:n].cpu().numpy(), verify_score=vf["score"][:n].cpu().numpy(),
                                         verified=vf["verified"][:n].cpu().numpy())
        return dict(out, class_ids=slot_ids[:n].copy(), RTs=rts[:n].cpu().numpy(), scales=scales[:n].cpu().numpy(),
                    inst_ids=np.arange(1, n + 1, dtype=np.int32), inst_mask=seg.labels[0].cpu().numpy(), boxes=stats[:, 1:5].copy(),
                    pixels=stats[:, 0].copy(), centers=seg.centers[0, :n].cpu().numpy(), ok=ok[:n].cpu().numpy(), info=info)

    def track(self, sequence, init, camK=lde.REAL_INTRINSICS, ratio=None, n_pts=1024, sampler=None, use_mask=True, refine=None,
              init_from="net", support=None, verify=None):
        """Follow objects through a depth sequence from their previous poses: no detector result after frame 0.

        sequence: iterable of frames {'depth' (H,W) uint16[, 'inst_mask' (H,W) uint8]}.  init: {'class_ids' (n,) 1-based category
        ids, 'RTs' (n,4,4), 'scales' (n,3)[, 'inst_ids' (n,)]} -- ground truth, or what ``run`` returned for frame 0; with inst_ids
        (and use_mask, and an 'inst_mask' in the frame) object k only sees the pixels whose mask byte is inst_ids[k].  ratio: the
        crop ball's radius over |RT[:3,:3] @ scale| (load_data_eval.pose_balls); required.  sampler: 'device' (keyed draw, seed =
        self.seed + frame number) or 'fps'; default: this evaluater's when it is one of the two, else 'device'.

        Per frame: one ball launch for all objects (load_data_eval.clouds_from_poses), the sampling, one forward
        (pose.infer_device).  Frame t's centres and radii are frame t-1's device outputs; nothing is read back between frames, and
        the results are fetched on the fetch stream, frame t-1's after frame t has been enqueued (``overlap``).  An object whose
        crop status is not 0 (1: nothing within the last radius; 2: no valid pixel) keeps its previous pose and is flagged.
        Each forward draws its pooling samples from torch's global CPU generator, as every forward of the network does: seed it for
        repeatable poses.

        refine (a pose.IcpRefine: models, job_model, max_dist and ops.icp_refine's keywords): the frame's poses are registered to
        the same cropped cloud by ICP (pose.refine_poses, one launch for all objects) before they become frame t+1's centres.
        init_from='net': the poses refined are the network's.  init_from='previous' (needs refine): no forward runs at all, the
        previous pose is refined against the new crop -- the model-based tracker; pred_scales are carried through.  An object whose
        ICP status is not 0 (ops.ICP_STATUS) keeps its previous pose and scales; the results gain 'icp_status', 'icp_inliers'
        (int32) and 'icp_rmse' (float32), (n,) each.  Still nothing is read back between frames.

        support (a pose.SupportPlane): the frame's dominant plane -- the table the objects stand on -- is found and cut out of the
        depth on the device before the crop (ops.plane_fit with key = the frame's number and seed = self.seed, ops.plane_cut), so
        that its pixels are in no crop; a frame without a plane (ops.PLANE_STATUS) is tracked uncut.  The results gain 'plane' (4,)
        float32, 'plane_status' and 'plane_inliers' (int32 scalars).  Nothing is read back for it either.

        verify (a pose.Verify: a mesh set, one mesh index per object, tau, min_score): once the frame's poses are final -- after
        ``refine`` when given -- each is rendered and compared with that frame's depth (ops.pose_verify, one call for all objects on
        the same stream; the cut depth when ``support`` is given; the frame's 'inst_mask' with inst_ids as the mask when both are
        there).  The results gain 'verify_counts' (n,8) int32 (ops.VERIFY_COUNTS), 'verify_score' (n,) float32 and 'verified' (n,)
        bool = score >= verify.min_score, fetched with the others.  Verification reports and does not gate: the poses carried to
        the next frame, and every other result, are those of the same call without ``verify``.

        refine may also be a pose.DenseModelRefine (DESIGN.md section 3 "Mesh maps and dense model-based tracking"): the frame
        itself -- uploaded once, after the optional plane cut, with its 'inst_mask' and inst_ids as the mask when use_mask and both
        are there -- is registered to the objects' rasterised meshes by dense projective ICP.  With init_from='previous' there is no
        crop and no forward: ratio may be None, n_pts and sampler are not used, and 'status' is 0 for every object.  With
        init_from='net' the crop and the forward run as above and the registration starts from the network's poses.  An object
        whose ICP status is not 0 (ops.ICP_STATUS, pose.RAYCAST_FEW_HITS, pose.DENSE_GATED) keeps its previous pose; the results
        gain 'icp_status', 'icp_inliers', 'icp_candidates', 'ray_hits' (int32) and 'icp_rmse' (float32), (n,) each.
        -> list over frames of {'pred_RTs' (n,4,4), 'pred_scales' (n,3), 'status' (n,) int32, 'tracked' (n,) bool} ndarrays."""
        if init_from not in ("net", "previous"):
            raise ValueError("track: init_from must be 'net' or 'previous'")
        dense = isinstance(refine, DenseModelRefine)
        if ratio is None and not (dense and init_from == "previous"):
            raise ValueError("track: ratio is required (the reference fixes none)")
        if refine is not None and not isinstance(refine, (IcpRefine, DenseModelRefine)):
            raise TypeError("track: refine must be a pose.IcpRefine or a pose.DenseModelRefine")
        if support is not None and not isinstance(support, SupportPlane):
            raise TypeError("track: support must be a pose.SupportPlane")
        if verify is not None and not isinstance(verify, Verify):
            raise TypeError("track: verify must be a pose.Verify")
        if init_from == "previous" and refine is None:
            raise ValueError("track: init_from='previous' needs refine (without it nothing would move the poses)")
        sampler = sampler or (self.sampler if self.sampler in ("device", "fps") else "device")
        if sampler not in ("device", "fps"):
            raise ValueError("track: sampler must be 'device' or 'fps' (nothing is read back between frames)")
        dev = self.device
        ids = np.asarray(init["class_ids"]).astype(np.int64)
        n = len(ids)
        if verify is not None:
            verify.jobs(n)                                   # one mesh index per object, or one for all: refused here, before any launch
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev)
        cat = t(ids - 1).reshape(-1, 1)
        mean = t([MEAN_SHAPE_MM[int(c)] for c in ids]).reshape(-1, 3) / 1000.0
        sym = t([SYM_INFO[int(c)] for c in ids]).reshape(-1, 4)
        rts, scales = t(init["RTs"]).reshape(n, 4, 4), t(init["scales"]).reshape(n, 3)
        inst_ids = init.get("inst_ids") if use_mask else None
        job_img = torch.zeros(n, dtype=torch.int32, device=dev)
        mask_val = torch.as_tensor(np.asarray(inst_ids), dtype=torch.uint8).to(dev) if dense and inst_ids is not None else None
        results, pending = [], None

        def fetch(item):
            r, s, st, done, icp, pl, vf = item
            with torch.cuda.stream(self._fetch):
                self._fetch.wait_event(done)
                for x in (r, s, st) + icp + pl + vf:
                    x.record_stream(self._fetch)
                r, s, st = r.cpu().numpy(), s.cpu().numpy(), st.cpu().numpy()
                icp = [x.cpu().numpy() for x in icp]
                pl = [x.cpu().numpy() for x in pl]
                vf = [x.cpu().numpy() for x in vf]
            results.append(dict(pred_RTs=r, pred_scales=s, status=st, tracked=st == 0))
            if icp:
                results[-1].update(icp_status=icp[0][:, 0].copy(), icp_inliers=icp[0][:, 1].copy(), icp_rmse=icp[1])
            if len(icp) == 3:                                # a DenseModelRefine's
                results[-1].update(icp_candidates=icp[0][:, 3].copy(), ray_hits=icp[2])
            if pl:
                results[-1].update(plane=pl[0][0].copy(), plane_status=pl[1][0, 0].copy(), plane_inliers=pl[1][0, 2].copy())
            if vf:
                results[-1].update(verify_counts=vf[0], verify_score=vf[1], verified=vf[2])
        for k, frame in enumerate(sequence):
            masks = inst_ids if inst_ids is not None and "inst_mask" in frame else None
            with torch.no_grad():
                pl = ()
                on_device = support is not None or verify is not None or dense
                if on_device:                                # the frame is uploaded here, once: the crop reads the same tensors
                    depth, inst, camk = lde._depth_frames([frame], camK, dev)
                    if support is not None:
                        depth, plane, pinfo = support(depth, camk, [k], self.seed)
                        pl = (plane, pinfo)
                    frame = dict(depth=depth) if inst is None else dict(depth=depth, inst_mask=inst)
                frames = frame if on_device else [frame]
                if dense and init_from == "previous":        # no crop: the frame itself is registered
                    ok = torch.ones(n, dtype=torch.bool, device=dev)
                    status = torch.zeros(n, dtype=torch.int32, device=dev)
                else:
                    pts, ok, _, counts = lde.clouds_from_poses(frames, job_img, rts, scales, ratio, camK, n_pts=n_pts, sampler=sampler,
                                                               masks=masks, seed=self.seed + k, fps_pool=self.fps_pool, device=dev,
                                                               return_counts=True)
                    status = counts[:, 3].contiguous()
                if init_from == "net":
                    new_rts, new_scales = infer_device(self.net1, torch.nan_to_num(pts, nan=0.0), cat, mean, sym, self.max_batch,
                                                       eval_outputs_only=self.eval_outputs_only)
                else:
                    new_rts, new_scales = rts, scales
                icp = ()
                if dense:
                    new_rts, info, rmse, hits = refine(depth, new_rts, camk, job_img, mask=inst.view(torch.uint8) if masks is not None else None,
                                                       job_mask_val=mask_val if masks is not None else None)
                    ok = ok & (info[:, 0] == 0)
                    icp = (info, rmse, hits)
                elif refine is not None:
                    new_rts, info, rmse = refine(pts, new_rts)      # a failed crop's NaN rows are never inliers: status 1
                    ok = ok & (info[:, 0] == 0)
                    icp = (info, rmse)
                rts = torch.where(ok[:, None, None], new_rts, rts)
                scales = torch.where(ok[:, None], new_scales, scales)
                vf = ()
                if verify is not None:
                    vmask = inst.view(torch.uint8) if masks is not None else None
                    vids = torch.as_tensor(np.asarray(masks), dtype=torch.uint8).to(dev) if masks is not None else None
                    v = verify(depth, camk, rts, scales, job_img=job_img, mask=vmask, job_mask_val=vids)
                    vf = (v["counts"], v["score"], v["verified"])
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
            item = (rts, scales, status, done, icp, pl, vf)
            if pending is not None:
                fetch(pending)
            pending = item
            if not self.overlap:
                fetch(pending)
                pending = None
        if pending is not None:
            fetch(pending)
        return results

    def scan(self, sequence, tracked, camK=lde.REAL_INTRINSICS, volumes=None, G=64, trunc_mm=None, support=None, use_mask=True,
             inst_ids=None, min_weight=1, near=0.01, indexed=False, cluster=1):
        """Build a mesh model of every tracked object from the depth sequence it was tracked through (DESIGN.md section 3 "Models
        from depth sequences"): TSDF fusion of all frames x objects in ONE ops.tsdf_integrate call, then marching tetrahedra.

        sequence: the frames ``track`` took, {'depth' (H,W) uint16[, 'inst_mask' (H,W) uint8]}.  tracked: what ``track`` returned
        for them (a list over frames of {'pred_RTs' (n,4,4)[, 'pred_scales' (n,3), 'tracked' (n,) bool]}; an object that is not
        'tracked' in a frame is left out of that frame), or poses from anywhere else, ground truth included: a list over frames
        of (n,4,4) arrays.  The poses are [s R | t], model units to camera metres, as pose.Verify and pose.IcpRefine read them; the
        model comes out in those units.  volumes (an ops.TsdfVolumes with one cube per object; it is added to, so a scan can be
        continued) or None: cubes of G^3 voxels about the model origin, sized by frame 0's 'pred_scales' (the object's extent in
        model units).  trunc_mm: the truncation (default: two voxel edges of the coarsest volume at frame 0's scale: thin parts
        need a truncation below their thickness).  support (a
        pose.SupportPlane): each frame's supporting plane is cut out first, keyed by the frame's number as ``track`` does.
        use_mask with inst_ids (n,) and an 'inst_mask' in every frame: object k only fuses the pixels whose byte is inst_ids[k].
        The frames are uploaded once; nothing is read back before the meshing, which reads each volume's triangle count and soup.
        indexed, cluster: ops.tsdf_meshset's -- indexed=True welds each model into an indexed mesh on the device (the same triangles
        over shared vertices; only counts are read back), cluster in (2, 4, 8) then decimates it by voxel clusters (DESIGN.md section
        3 "Indexed meshes from volumes").
        -> (volumes, ops.MeshSet of the n scanned models); a volume without a face raises ValueError."""
        if support is not None and not isinstance(support, SupportPlane):
            raise TypeError("scan: support must be a pose.SupportPlane")
        if cluster not in ops.WELD_CLUSTERS or (cluster != 1 and not indexed):
            raise ValueError("scan: cluster must be 1, 2, 4 or 8, and needs indexed=True")
        frames = list(sequence)
        if not frames or len(tracked) != len(frames):
            raise ValueError("scan: one entry of tracked per frame of a sequence that is not empty")
        is_rec = isinstance(tracked[0], dict)
        rts = np.stack([np.asarray(t["pred_RTs"] if is_rec else t, dtype=np.float32) for t in tracked])          # (T, n, 4, 4)
        if rts.ndim != 4 or rts.shape[2:] != (4, 4) or rts.shape[1] < 1:
            raise ValueError("scan: every frame needs (n,4,4) poses of the same n >= 1 objects")
        T, n = rts.shape[:2]
        live = np.stack([np.asarray(t["tracked"], dtype=bool) if is_rec and "tracked" in t else np.ones(n, dtype=bool) for t in tracked])
        dev = self.device
        if volumes is None:
            if not (is_rec and "pred_scales" in tracked[0]):
                raise ValueError("scan: without volumes, tracked[0]['pred_scales'] must give the objects' extents in model units")
            volumes = ops.TsdfVolumes(np.zeros((n, 3), dtype=np.float32), np.asarray(tracked[0]["pred_scales"], dtype=np.float32).reshape(n, 3),
                                      G, device=dev)
        if not isinstance(volumes, ops.TsdfVolumes) or len(volumes) != n:
            raise ValueError("scan: volumes must be an ops.TsdfVolumes with one cube for each of the %d objects" % n)
        if trunc_mm is None:
            s0 = np.cbrt(np.abs(np.linalg.det(rts[0, :, :3, :3].astype(np.float64))))
            trunc_mm = 2000.0 * float((volumes.meta_host[:, 3].astype(np.float64) * s0).max())
        masked = use_mask and inst_ids is not None and all("inst_mask" in fr for fr in frames)
        job_model = np.where(live, np.arange(n, dtype=np.int32)[None, :], -1).astype(np.int32).reshape(-1)    # -1: the job is ignored
        with torch.no_grad():
            depth, inst, camk = lde._depth_frames(frames, camK, dev)
            if support is not None:
                depth = support(depth, camk, list(range(T)), self.seed)[0]
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            scan_models(volumes, depth, camk, up(rts.reshape(T * n, 4, 4)), job_img=up(np.repeat(np.arange(T, dtype=np.int32), n)),
                        job_model=up(job_model), trunc_mm=trunc_mm, near=near, mask=inst.view(torch.uint8) if masked else None,
                        job_mask_val=up(np.tile(np.asarray(inst_ids).astype(np.uint8), T)) if masked else None)
            return volumes, ops.tsdf_meshset(volumes, min_weight, indexed=indexed, cluster=cluster)

    def scan_track(self, sequence, init, camK=lde.REAL_INTRINSICS, ratio=None, volumes=None, G=64, trunc_mm=None, refine_kw=None,
                   n_pts=1024, sampler=None, use_mask=True, support=None, min_inlier_frac=0.5, max_rmse=None, near=0.01, register="sparse"):
        """Track objects that have no model while scanning them (DESIGN.md section 3 "Ray casting and frame-to-model tracking"): each
        frame is registered to the TSDF volumes as they stand and is then fused into them.  One pose per object in frame 0 is all it
        needs.

        sequence, init, camK, ratio, n_pts, sampler, use_mask, support: as ``track`` takes them (init['RTs'] are [s R | t], model
        units to camera metres, and init['scales'] the objects' extents in model units, as ``scan`` reads them; class_ids are not
        used).  volumes: an ops.TsdfVolumes with one cube per object (it is added to), default ``scan``'s cubes of G^3 voxels from
        init['scales']; trunc_mm: default ``scan``'s two voxel edges.  refine_kw: pose.RaycastRefine's keywords (default: max_dist
        = three voxel edges of the coarsest volume at frame 0's scale, mode 'plane').
        Frame 0 is fused at init's poses.  Frame k >= 1: the optional plane cut, the ball crop round the previous poses
        (load_data_eval.clouds_from_poses, as ``track`` crops), pose.RaycastRefine from the previous poses, and ONE
        ops.tsdf_integrate call.  An object is registered when its crop and its ICP succeeded, its inliers reach min_inlier_frac x
        its cloud's finite rows and (with max_rmse, metres) its rmse stays within it; one that is not keeps its previous pose, and
        its job's volume index becomes -1 on the device, so that the frame adds nothing to its volume.  Nothing is read back between
        frames; the results are fetched on the fetch stream as ``track`` fetches them.
        -> (results, volumes): per frame ``track``'s {'pred_RTs', 'pred_scales', 'status', 'tracked'} plus 'icp_status',
        'icp_inliers' (int32), 'icp_rmse' (float32), 'ray_hits' (int32) and 'fused' (bool: registered, and so fused), (n,) each
        (frame 0: status 0, no ICP, fused).  Mesh the volumes with ops.tsdf_meshset (indexed=True, cluster=c for a welded or a
        decimated model, as ``scan`` takes them).
        register='dense' (DESIGN.md section 3 "Dense projective registration"): frame k >= 1 is not cropped; after the optional
        plane cut the frame itself, with its instance mask when it has one, is registered by pose.DenseRefine (refine_kw: its
        keywords; ratio, n_pts and sampler are not used).  An object is registered when its status is 0 and its inliers reach
        min_inlier_frac x its candidates (the pixels its map associated at the previous pose), plus max_rmse; 'status' is 0 for
        every object.  The result keys are the same."""
        from ..pose import DenseRefine, RaycastRefine, verify_job_pose
        if register not in ("sparse", "dense"):
            raise ValueError("scan_track: register must be 'sparse' or 'dense'")
        if ratio is None and register == "sparse":
            raise ValueError("scan_track: ratio is required (the reference fixes none)")
        if support is not None and not isinstance(support, SupportPlane):
            raise TypeError("scan_track: support must be a pose.SupportPlane")
        sampler = sampler or (self.sampler if self.sampler in ("device", "fps") else "device")
        if sampler not in ("device", "fps"):
            raise ValueError("scan_track: sampler must be 'device' or 'fps' (nothing is read back between frames)")
        if not 0.0 <= float(min_inlier_frac) <= 1.0:
            raise ValueError("scan_track: min_inlier_frac must be in [0, 1]")
        dev = self.device
        rts0 = np.asarray(init["RTs"], dtype=np.float32).reshape(-1, 4, 4)
        n = len(rts0)
        scales0 = np.asarray(init["scales"], dtype=np.float32).reshape(n, 3)
        if volumes is None:
            volumes = ops.TsdfVolumes(np.zeros((n, 3), dtype=np.float32), scales0, G, device=dev)
        if not isinstance(volumes, ops.TsdfVolumes) or len(volumes) != n:
            raise ValueError("scan_track: volumes must be an ops.TsdfVolumes with one cube for each of the %d objects" % n)
        s0 = np.cbrt(np.abs(np.linalg.det(rts0[:, :3, :3].astype(np.float64))))
        voxel_m = float((volumes.meta_host[:, 3].astype(np.float64) * s0).max())
        if trunc_mm is None:
            trunc_mm = 2000.0 * voxel_m
        kw = dict(refine_kw or {})
        kw.setdefault("max_dist", 3.0 * voxel_m)
        kw.setdefault("near", near)
        refine = (DenseRefine if register == "dense" else RaycastRefine)(volumes, kw.pop("max_dist"), **kw)
        rts, scales = torch.from_numpy(rts0).to(dev), torch.from_numpy(scales0).to(dev)
        inst_ids = init.get("inst_ids") if use_mask else None
        mask_val = torch.as_tensor(np.asarray(inst_ids), dtype=torch.uint8).to(dev) if inst_ids is not None else None
        job_img = torch.zeros(n, dtype=torch.int32, device=dev)
        every = torch.arange(n, dtype=torch.int32, device=dev)
        results, pending = [], None

        def fetch(item):
            done, tensors = item
            with torch.cuda.stream(self._fetch):
                self._fetch.wait_event(done)
                for x in tensors:
                    x.record_stream(self._fetch)
                r, s, st, info, rmse, hits, fused = (x.cpu().numpy() for x in tensors)
            results.append(dict(pred_RTs=r, pred_scales=s, status=st, tracked=st == 0, icp_status=info[:, 0].copy(),
                                icp_inliers=info[:, 1].copy(), icp_rmse=rmse, ray_hits=hits, fused=fused))
        for k, frame in enumerate(sequence):
            masks = inst_ids if inst_ids is not None and "inst_mask" in frame else None
            with torch.no_grad():
                depth, inst, camk = lde._depth_frames([frame], camK, dev)
                H, W = depth.shape[1:]
                if support is not None:
                    depth = support(depth, camk, [k], self.seed)[0]
                if k == 0:
                    status = torch.zeros(n, dtype=torch.int32, device=dev)
                    info = torch.zeros(n, 4, dtype=torch.int32, device=dev)
                    rmse = torch.zeros(n, dtype=torch.float32, device=dev)
                    hits = torch.zeros(n, dtype=torch.int32, device=dev)
                    ok = torch.ones(n, dtype=torch.bool, device=dev)
                elif register == "dense":
                    new_rts, info, rmse, hits = refine(depth, rts, camk, job_img, mask=inst.view(torch.uint8) if masks is not None else None,
                                                       job_mask_val=mask_val if masks is not None else None)
                    ok = (info[:, 0] == 0) & (info[:, 1].float() >= float(min_inlier_frac) * info[:, 3].float())
                    if max_rmse is not None:
                        ok = ok & (rmse <= float(max_rmse))
                    rts = torch.where(ok[:, None, None], new_rts, rts)
                    status = torch.zeros(n, dtype=torch.int32, device=dev)
                else:
                    crop = dict(depth=depth) if inst is None else dict(depth=depth, inst_mask=inst)
                    pts, ok, _, counts = lde.clouds_from_poses(crop, job_img, rts, scales, ratio, camK, n_pts=n_pts, sampler=sampler, masks=masks,
                                                               seed=self.seed + k, fps_pool=self.fps_pool, device=dev, return_counts=True)
                    new_rts, info, rmse, hits = refine(pts, rts, camk, job_img, H, W)   # a failed crop's NaN rows are never inliers
                    rows = torch.isfinite(pts).all(-1).sum(1)
                    ok = ok & (info[:, 0] == 0) & (info[:, 1].float() >= float(min_inlier_frac) * rows.float())
                    if max_rmse is not None:
                        ok = ok & (rmse <= float(max_rmse))
                    rts = torch.where(ok[:, None, None], new_rts, rts)
                    status = counts[:, 3].contiguous()
                job_model = torch.where(ok, every, torch.full_like(every, -1))           # -1: the job adds nothing
                ops.tsdf_integrate(volumes, depth, camk, job_img, job_model, verify_job_pose(rts), trunc_mm, near=near,
                                   mask=inst.view(torch.uint8) if masks is not None else None, job_mask_val=mask_val if masks is not None else None)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
            item = (done, (rts, scales, status, info, rmse, hits, ok))
            if pending is not None:
                fetch(pending)
            pending = item
            if not self.overlap:
                fetch(pending)
                pending = None
        if pending is not None:
            fetch(pending)
        return results, volumes


def calc_pose_metric(pred_results, output_path, per_obj=""):
    """:111-175 -- the mAP tables and the lines the reference logs (degree 0..60, shift 0..10 cm by 0.5, IoU 0..1 by 0.01)."""
    degree, shift, iou = list(range(0, 61, 1)), [i / 2 for i in range(21)], [i / 100 for i in range(101)]
    idx = SYNSET_NAMES.index(per_obj) if per_obj in SYNSET_NAMES else -1
    iou_aps, pose_aps = compute_degree_cm_mAP(pred_results, SYNSET_NAMES, output_path, degree, shift, iou, iou_pose_thres=0.1,
                                              use_matches_for_pose=True)[:2]
    i25, i50, i75 = iou.index(0.25), iou.index(0.5), iou.index(0.75)
    d5, d10, s2, s5, s10 = degree.index(5), degree.index(10), shift.index(2), shift.index(5), shift.index(10)
    messages = ['mAP:' if idx != -1 else 'average mAP:',
                '3D IoU at 25: {:.1f}'.format(iou_aps[idx, i25] * 100), '3D IoU at 50: {:.1f}'.format(iou_aps[idx, i50] * 100),
                '3D IoU at 75: {:.1f}'.format(iou_aps[idx, i75] * 100),
                '5 degree, 2cm: {:.1f}'.format(pose_aps[idx, d5, s2] * 100), '5 degree, 5cm: {:.1f}'.format(pose_aps[idx, d5, s5] * 100),
                '10 degree, 2cm: {:.1f}'.format(pose_aps[idx, d10, s2] * 100), '10 degree, 5cm: {:.1f}'.format(pose_aps[idx, d10, s5] * 100),
                '10 degree, 10cm: {:.1f}'.format(pose_aps[idx, d10, s10] * 100),
                '5 degree: {:.1f}'.format(pose_aps[idx, d5, -1] * 100), '10 degree: {:.1f}'.format(pose_aps[idx, d10, -1] * 100),
                '2cm: {:.1f}'.format(pose_aps[idx, -1, s2] * 100), '5cm: {:.1f}'.format(pose_aps[idx, -1, s5] * 100),
                '10cm: {:.1f}'.format(pose_aps[idx, -1, s10] * 100)]
    return iou_aps, pose_aps, messages
