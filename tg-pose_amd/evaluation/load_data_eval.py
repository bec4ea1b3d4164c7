"""Input side of the evaluation loader on the device.

Stands where the per-detection loop of ``PoseDataset.__getitem__`` stands in the reference
(``evaluation/load_data_eval.py:294-357``): for every Mask-RCNN detection of a frame it crops a square window round the
box, resamples depth / mask / pixel grid to ``FLAGS.img_size`` squared with nearest-neighbour ``cv2.warpAffine``,
back-projects the valid pixels (``_depth_to_pcl`` :451-462), cuts the points near point number 25 (:341-355) and
resamples to ``FLAGS.random_points`` (``_sample_points`` :404-417) -- about ten numpy / OpenCV passes over 65536 pixels per
detection on a DataLoader worker.  Here the frames' depth images and masks are uploaded once and ONE launch
(``tgp_roi_cloud``, a workgroup per detection) leaves every detection's cloud in HBM, in the reference's point order, as
4-byte records (ROI pixel, depth); the resampling is a gather that materialises only the 1024 selected points.  The clouds never visit the host: they are the ``pcl_in`` that ``PoseNet9D.forward`` consumes
(``pose.batched_inference``).

``sampler='numpy'`` reproduces the reference bit for bit, including its use of the global ``np.random`` stream: the
per-detection point counts (12 bytes each) are read back once per call, the permutations are drawn on the host in the
reference's order (frame by frame, detection by detection; a frame the reference abandons with ``return None`` has consumed
the draws of its earlier detections, as there), and their prefixes are uploaded for the gather.
``sampler='device'`` draws a keyed pseudo-random permutation on the device instead (``tgp_cloud_sample``): nothing is
read back, frames cannot be dropped on the host, so invalid detections come back as NaN rows with ``valid`` False.
``sampler='fps'`` draws nothing at all: farthest point sampling (``tgp_fps``, csrc/fps.hip -- what the reference's ``_sample_points``
docstring announces) of each detection's cloud, thinned evenly to ``fps_pool`` candidates first when it is longer.  Like
``'device'`` it reads nothing back and returns ``(clouds, valid)``; the result is a pure function of the frames.

What stays on the host, as integer arithmetic on four numbers per detection: ``get_bbox`` (the window rule of
``tools.eval_utils``, source twin ``network/point_sample/pc_sample_sphere.py:456-484``).  File reading / unpickling
(:239-284) and the category bookkeeping (:359-400) are not part of this module.
"""
import numpy as np
import torch

from .. import ops

REAL_INTRINSICS = np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]], dtype=np.float32)   # :160
CAMERA_INTRINSICS = np.array([[577.5, 0, 319.5], [0, 577.5, 239.5], [0, 0, 1]], dtype=np.float32)              # :158


def get_bbox(bbox):
    """Square crop window of a detection box (y1, x1, y2, x2) -> rmin, rmax, cmin, cmax (pc_sample_sphere.py:456-484)."""
    y1, x1, y2, x2 = (int(v) for v in bbox)
    img_width, img_length = 480, 640
    window_size = min((max(y2 - y1, x2 - x1) // 40 + 1) * 40, 440)
    half = int(window_size / 2)
    cy, cx = (y1 + y2) // 2, (x1 + x2) // 2
    rmin, rmax, cmin, cmax = cy - half, cy + half, cx - half, cx + half
    if rmin < 0:
        rmin, rmax = 0, rmax - rmin
    if cmin < 0:
        cmin, cmax = 0, cmax - cmin
    if rmax > img_width:
        rmin, rmax = rmin - (rmax - img_width), img_width
    if cmax > img_length:
        cmin, cmax = cmin - (cmax - img_length), img_length
    return rmin, rmax, cmin, cmax


def _windows(frames):
    """Host packing: per detection {cmin+cmax, rmin+rmax, s} (:305-316), its frame, its mask channel's offset and stride."""
    win, det_img, off, stride = [], [], [], []
    pos = 0
    for i, fr in enumerate(frames):
        H, W, n = fr["pred_masks"].shape
        if n >= 128:
            raise ValueError("frame %d: %d mask channels; tgp_roi_cloud addresses masks with 31-bit offsets (n < 128)" % (i, n))
        if len(fr["pred_bboxes"]) != n:
            raise ValueError("frame %d: %d boxes for %d mask channels" % (i, len(fr["pred_bboxes"]), n))
        for j in range(n):
            rmin, rmax, cmin, cmax = get_bbox(fr["pred_bboxes"][j])
            s = min(max(rmax - rmin, cmax - cmin), max(H, W))
            win.append((cmin + cmax, rmin + rmax, s))
            det_img.append(i), off.append(pos + j), stride.append(n)
        pos += H * W * n
    return win, det_img, off, stride


class RoiClouds:
    """Device-side result of ``build``: ``records`` (ops.RoiRecords: 4-byte records + counts (D,3) + descriptors), detections per
    frame.  ``points(n)`` materialises the first n points of every cloud (rows beyond a cloud's count are meaningless)."""

    def __init__(self, records, per_frame):
        self.records, self.per_frame = records, per_frame
        self.counts = None if records is None else records.counts

    def points(self, n):
        D = self.records.recs.shape[0]
        sel = torch.arange(n, dtype=torch.int32, device=self.records.recs.device).repeat(D, 1)
        return ops.cloud_select(self.records, sel)


def upload(frames, camK=REAL_INTRINSICS, device="cuda"):
    """Pack and upload what tgp_roi_cloud reads: (depth, masks, mask_off, mask_stride, det_img, window, camk) on the device."""
    dev = torch.device(device)
    H, W = frames[0]["depth"].shape
    for fr in frames:
        if fr["depth"].shape != (H, W) or fr["pred_masks"].shape[:2] != (H, W) or fr["depth"].dtype != np.uint16:
            raise ValueError("every frame needs a uint16 depth image and masks of one common (H,W)")
    win, det_img, off, stride = _windows(frames)
    camK = np.asarray(camK, dtype=np.float32)
    camK = np.broadcast_to(camK, (len(frames), 3, 3)) if camK.ndim == 2 else camK
    camk = np.stack([camK[:, 0, 0], camK[:, 1, 1], camK[:, 0, 2], camK[:, 1, 2]], axis=1).astype(np.float32)
    # The copies go out on their own stream: a host-to-device copy from pageable memory holds the host until it has run, and on
    # the compute stream it would queue behind the previous chunk's forward -- the host would pack chunk c+1 only after chunk c
    # had finished.  The compute stream waits for the copies' event; record_stream keeps the allocator from recycling the
    # buffers before the compute stream is done with them.
    cur = torch.cuda.current_stream(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(device=dev)
    cs = _COPY_STREAMS[key]
    host = [np.stack([fr["depth"] for fr in frames]).view(np.int16),
            np.concatenate([np.ascontiguousarray(fr["pred_masks"]).view(np.uint8).reshape(-1) for fr in frames if fr["pred_masks"].size]),
            np.asarray(off, dtype=np.int64), np.asarray(stride, dtype=np.int32), np.asarray(det_img, dtype=np.int32),
            np.asarray(win, dtype=np.int32).reshape(-1, 3), camk]
    with torch.cuda.stream(cs):
        out = [torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True) for a in host]
    done = torch.cuda.Event()
    done.record(cs)
    cur.wait_event(done)
    for t in out:
        t.record_stream(cur)
    return tuple(out)


_COPY_STREAMS = {}


def build(frames, camK=REAL_INTRINSICS, img_size=256, device="cuda"):
    """Upload the frames and run the per-detection kernel.  frames: list of dicts with 'depth' (H,W) uint16,
    'pred_masks' (H,W,n) bool / uint8, 'pred_bboxes' (n,4) (the detection pickle's layout, :271-303); camK one (3,3)
    matrix or one per frame.  All frames must share (H,W).  Nothing synchronises."""
    dev = torch.device(device)
    per_frame = [fr["pred_masks"].shape[2] for fr in frames]
    if sum(per_frame) == 0:
        return RoiClouds(None, per_frame)
    return RoiClouds(ops.roi_cloud(*upload(frames, camK, dev), roi_size=img_size), per_frame)


def _fps_clouds(rc, n_pts, fps_pool):
    """sampler='fps': per detection the candidates are the whole cloud (total <= fps_pool) or the evenly spaced records
    floor(i * total / fps_pool), i < fps_pool -- integer arithmetic on the device -- gathered by tgp_cloud_select; tgp_fps on the
    candidates with per-detection counts (a cloud of at most n_pts points is tiled there, as _sample_points tiles it); one row
    gather.  An invalid detection selects record -1 throughout, whose point is NaN."""
    recs = rc.records.recs
    dev = recs.device
    m = min(int(fps_pool), recs.shape[1])
    total = rc.counts[:, 2].long().clamp(min=0, max=recs.shape[1])
    ok = (rc.counts[:, 2] > 0) & (rc.counts[:, 0] > 1) & (rc.counts[:, 1] > 1)
    cand = torch.where(ok, total.clamp(max=m), torch.zeros_like(total))
    i = torch.arange(m, device=dev, dtype=torch.int64)[None, :]
    sel = torch.where((total > m)[:, None], (i * total[:, None]) // m, i)
    sel = torch.where(i < cand[:, None], sel, torch.full_like(sel, -1)).int()
    pts = ops.cloud_select(rc.records, sel)
    idx = ops.farthest_points(pts, n_pts, counts=cand.clamp(min=1).int())
    out = torch.gather(pts, 1, idx.long()[:, :, None].expand(-1, -1, 3))
    return out, ok


def clouds_from_frames(frames, camK=REAL_INTRINSICS, img_size=256, n_pts=1024, sampler="numpy", rng=np.random, seed=0, device="cuda",
                       fps_pool=4096):
    """-> list over frames of ``pcl_in`` (n_det, n_pts, 3) float32 GPU tensors; ``None`` for a frame the reference's
    ``__getitem__`` drops (:332-337).  Raises IndexError / ZeroDivisionError where the reference does (fewer than 26 valid
    points :350, an empty cloud after the cut :411).  With sampler='device' or 'fps' returns (list of tensors, list of bool masks).
    sampler='fps' consumes neither ``rng`` nor ``seed``; ``fps_pool`` (at most ops.fps_max_points()) is the number of candidates a
    longer cloud is thinned to before the sampling."""
    if sampler == "fps" and not 1 <= int(fps_pool) <= ops.fps_max_points():
        raise ValueError("fps_pool must be in [1, %d] (ops.fps_max_points())" % ops.fps_max_points())
    rc = build(frames, camK, img_size, device)
    D = sum(rc.per_frame)
    dev = torch.device(device)
    empty = torch.zeros(0, n_pts, 3, device=dev)
    if sampler == "fps":
        if D == 0:
            return [empty for _ in rc.per_frame], [torch.zeros(0, dtype=torch.bool, device=dev) for _ in rc.per_frame]
        out, ok = _fps_clouds(rc, n_pts, fps_pool)
        return list(out.split(rc.per_frame)), list(ok.split(rc.per_frame))
    if sampler == "device":
        if D == 0:
            return [empty for _ in rc.per_frame], [torch.zeros(0, dtype=torch.bool, device=dev) for _ in rc.per_frame]
        out = ops.cloud_sample(rc.records, n_pts, seed)
        ok = (rc.counts[:, 2] > 0) & (rc.counts[:, 0] > 1) & (rc.counts[:, 1] > 1)
        return list(out.split(rc.per_frame)), list(ok.split(rc.per_frame))
    if sampler != "numpy":
        raise ValueError("sampler must be 'numpy', 'device' or 'fps'")
    if D == 0:
        return [empty for _ in rc.per_frame]
    counts = rc.counts.cpu().numpy()                         # the one read-back: 12 bytes per detection
    sel = np.zeros((D, n_pts), dtype=np.int32)
    keep_frame, d = [], 0
    for n in rc.per_frame:
        alive = True
        for j in range(n):
            n_depth, n_valid, total = (int(v) for v in counts[d + j])
            if n_depth <= 1 or n_valid <= 1:                 # :332-337 -> return None (earlier detections already drew)
                alive = False
                break
            if total < 0:
                raise IndexError("index 25 is out of bounds for axis 0 with size %d" % n_valid)     # :350
            if total < n_pts:
                sel[d + j] = np.arange(n_pts) % total        # ZeroDivisionError for total == 0, as n_pts // 0 at :411
            elif total > n_pts:
                sel[d + j] = rng.permutation(total)[:n_pts]
            else:
                sel[d + j] = np.arange(n_pts)
        keep_frame.append(alive)
        d += n
    out = ops.cloud_select(rc.records, torch.from_numpy(sel).to(dev))
    return [c if alive else None for c, alive in zip(out.split(rc.per_frame), keep_frame)]


# ------------------------------------------------------------------------------------------- clouds from segments (no detector)
def _segment_windows(boxes, H, W):
    """get_bbox and _windows for (..., 4) int64 boxes (y1, x1, y2, x2) on the device -> (..., 3) int32 {cmin+cmax, rmin+rmax, s}:
    the same integers, step by step (every quantity is non-negative where Python's and torch's integer division could differ)"""
    y1, x1, y2, x2 = boxes.unbind(-1)
    size = (((torch.maximum(y2 - y1, x2 - x1) // 40) + 1) * 40).clamp(max=440)
    half = size // 2
    cy, cx = (y1 + y2) // 2, (x1 + x2) // 2
    rmin, rmax, cmin, cmax = cy - half, cy + half, cx - half, cx + half
    zero = torch.zeros_like(rmin)
    rmax, rmin = torch.where(rmin < 0, rmax - rmin, rmax), torch.where(rmin < 0, zero, rmin)
    cmax, cmin = torch.where(cmin < 0, cmax - cmin, cmax), torch.where(cmin < 0, zero, cmin)
    rmin, rmax = torch.where(rmax > 480, rmin - (rmax - 480), rmin), rmax.clamp(max=480)
    cmin, cmax = torch.where(cmax > 640, cmin - (cmax - 640), cmin), cmax.clamp(max=640)
    s = torch.maximum(rmax - rmin, cmax - cmin).clamp(max=max(H, W))
    return torch.stack([cmin + cmax, rmin + rmax, s], dim=-1).int()


def clouds_from_segments(depth, segments, camK=REAL_INTRINSICS, img_size=256, n_pts=1024, sampler="device", seed=0, fps_pool=4096):
    """The ROI path of clouds_from_frames fed from a label image instead of a detector's masks and boxes: slot m of frame s
    (``segments`` = ops.segment_depth's result for ``depth`` (S,H,W), M = segments.max_segments slots per frame) is detection
    s * M + m, its mask the pixels labelled m + 1, its box the segment's (stats columns 1..4), its window get_bbox's of that box --
    all of it device arithmetic, nothing is read back.  camK: one (3,3) matrix, one per frame, or the (S,4) fx, fy, cx, cy tensor
    on the device.  sampler 'device' (the keyed draw of tgp_cloud_sample under ``seed``) or 'fps'.
    -> (clouds (S*M, n_pts, 3), ok (S*M,) bool).  An empty slot (and a segment the ROI path finds invalid) has NaN rows and ok
    False.  The clouds equal clouds_from_frames' for M mask channels per frame holding the same masks and boxes, bit for bit."""
    if sampler not in ("device", "fps"):
        raise ValueError("sampler must be 'device' or 'fps'")
    if sampler == "fps" and not 1 <= int(fps_pool) <= ops.fps_max_points():
        raise ValueError("fps_pool must be in [1, %d] (ops.fps_max_points())" % ops.fps_max_points())
    if not isinstance(segments, ops.Segments):
        raise TypeError("clouds_from_segments: segments must be an ops.Segments")
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.dim() == 3 and depth.shape == segments.labels.shape
            and depth.device == segments.labels.device):
        raise ValueError("clouds_from_segments: depth must be the (S,H,W) GPU tensor the segments were made from")
    dev = depth.device
    S, H, W = depth.shape
    M = segments.max_segments
    if torch.is_tensor(camK) and camK.is_cuda:
        camk = camK
    else:
        camK = np.asarray(camK, dtype=np.float32)
        camK = np.broadcast_to(camK, (S, 3, 3)) if camK.ndim == 2 else camK
        camk = np.stack([camK[:, 0, 0], camK[:, 1, 1], camK[:, 0, 2], camK[:, 1, 2]], axis=1).astype(np.float32)
        camk = torch.from_numpy(np.ascontiguousarray(camk)).to(dev, non_blocking=True)
    det_img = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(M)
    mask_val = torch.arange(1, M + 1, device=dev, dtype=torch.int32).repeat(S)
    window = _segment_windows(segments.stats[:, :, 1:5], H, W).reshape(S * M, 3).contiguous()     # an empty slot: the box (0,0,0,0)'s
    rr = ops.roi_cloud(depth, segments.labels.reshape(-1), det_img.long() * (H * W), torch.ones_like(det_img), det_img, window, camk,
                       roi_size=img_size, mask_val=mask_val)
    if sampler == "fps":
        return _fps_clouds(RoiClouds(rr, [M] * S), n_pts, fps_pool)
    out = ops.cloud_sample(rr, n_pts, seed)
    ok = (rr.counts[:, 2] > 0) & (rr.counts[:, 0] > 1) & (rr.counts[:, 1] > 1)
    return out, ok


# ------------------------------------------------------------------------------------------------ clouds from poses (the ball crop)
def pose_balls(RTs, scales, ratio):
    """The balls crop_ball_from_depth_image (network/point_sample/pc_sample_sphere.py:350-357) crops round poses: centres = the
    translations, radius = ratio * |RT[:3, :3] @ scale|, and the ten radii its loop tests (ops.ball_ladder).  RTs (J,4,4) or
    (J,3,4), scales (J,3) device tensors -> (centers (J,3), ladder (J,10)); device ops only, nothing is read back."""
    RTs, scales = RTs.float(), scales.float()
    radius = torch.linalg.vector_norm(torch.bmm(RTs[:, :3, :3], scales[:, :, None])[:, :, 0], dim=1) * float(ratio)
    return RTs[:, :3, 3].contiguous(), ops.ball_ladder(radius)


def _depth_frames(frames, camK, dev):
    """frames: a list of {'depth' (H,W) uint16[, 'inst_mask' (H,W) uint8]} host records, or one dict of device tensors {'depth'
    (I,H,W) 16-bit[, 'inst_mask' (I,H,W) uint8]} -> (depth (I,H,W), inst (I,H,W) uint8 or None, camk (I,4)) on the device"""
    if isinstance(frames, dict):
        depth, inst = frames["depth"], frames.get("inst_mask")
    else:
        H, W = frames[0]["depth"].shape
        for fr in frames:
            if fr["depth"].shape != (H, W) or fr["depth"].dtype != np.uint16:
                raise ValueError("every frame needs a uint16 depth image of one common (H,W)")
        depth = torch.from_numpy(np.stack([fr["depth"] for fr in frames]).view(np.int16)).to(dev, non_blocking=True)
        inst = None
        if all("inst_mask" in fr for fr in frames):
            inst = torch.from_numpy(np.stack([np.ascontiguousarray(fr["inst_mask"]).view(np.uint8) for fr in frames])).to(dev, non_blocking=True)
    I = depth.shape[0]
    if inst is not None and (inst.shape != depth.shape or inst.dtype not in (torch.uint8, torch.bool)):
        raise ValueError("inst_mask must be a byte image per frame, of the depth's (H,W)")
    camK = np.asarray(camK, dtype=np.float32)
    camK = np.broadcast_to(camK, (I, 3, 3)) if camK.ndim == 2 else camK
    camk = np.stack([camK[:, 0, 0], camK[:, 1, 1], camK[:, 0, 2], camK[:, 1, 2]], axis=1).astype(np.float32)
    return depth, inst, torch.from_numpy(np.ascontiguousarray(camk)).to(dev, non_blocking=True)


def _ball_fps(br, n_pts, fps_pool):
    """sampler='fps' on ball crops, as _fps_clouds on ROI crops: the candidates are the crop's doubled list (the crop itself when it
    holds n_pts), thinned evenly to fps_pool entries when longer, gathered by tgp_ball_select; tgp_fps with per-job counts.  On a
    doubled list that returns the distinct points once and then the list's row 0, as the reference's farthest_points does."""
    dev = br.recs.device
    m = int(fps_pool)
    n = br.counts[:, 1].long().clamp(min=0, max=br.cap)
    ok = (br.counts[:, 3] == 0) & (n > 0)
    total = n.clamp(min=1)
    for _ in range(max(0, int(n_pts - 1).bit_length())):            # count * 2^m, the first >= n_pts: at most log2(n_pts) doublings
        total = torch.where(total < n_pts, total * 2, total)
    cand = torch.where(ok, total.clamp(max=m), torch.zeros_like(total))
    i = torch.arange(m, device=dev, dtype=torch.int64)[None, :]
    sel = torch.where((total > m)[:, None], (i * total[:, None]) // m, i)
    sel = torch.where(i < cand[:, None], sel, torch.full_like(sel, -1)).int()
    pts, pix = ops.ball_select(br, sel)        # a list doubled up to fps_pool entries holds the one doubled up to n_pts
    idx = ops.farthest_points(pts, n_pts, counts=cand.clamp(min=1).int()).long()
    return torch.gather(pts, 1, idx[:, :, None].expand(-1, -1, 3)), torch.gather(pix, 1, idx), ok


def clouds_from_poses(frames, job_img, RTs, scales, ratio, camK=REAL_INTRINSICS, n_pts=1024, sampler="device", masks=None, seed=0,
                      fps_pool=4096, device="cuda", cap=None, full_scan=False, return_counts=False):
    """The other way into the network: job j's cloud is cut out of depth frame job_img[j] by a ball round pose (RTs[j], scales[j]) --
    crop_ball_from_depth_image (pc_sample_sphere.py:350-371) for all jobs in one launch (ops.ball_cloud), with no detector result.
    frames as _depth_frames takes them; RTs (J,4,4) / scales (J,3) tensors or arrays (device tensors stay there: in tracking they
    are the previous forward's outputs); ratio: the ball's radius over |RT[:3,:3] @ scale| (the reference fixes none).
    masks: None, or per job the instance id whose pixels of the frame's 'inst_mask' are admitted (0: any non-zero byte).
    sampler: 'device' the keyed draw of tgp_ball_sample (seed); 'fps' farthest point sampling (fps_pool candidates at most);
    'torch' the reference's torch.randperm draws from torch's CPU generator, job by job -- the only one that reads the counts back.
    -> (clouds (J,n_pts,3), ok (J,) bool, pix (J,n_pts) int32 source pixels: gather image / coord rows with them)[, counts (J,4)].
    A job whose status (counts[:, 3]) is not 0 -- nothing within the last radius, no valid pixel -- has NaN rows, pix -1, ok False;
    the reference's fall-back to every valid point is crop_ball_from_pts' business, not this function's."""
    if sampler not in ("device", "fps", "torch"):
        raise ValueError("sampler must be 'device', 'fps' or 'torch'")
    if sampler == "fps" and not n_pts <= int(fps_pool) <= ops.fps_max_points():
        raise ValueError("fps_pool must be in [n_pts, %d] (ops.fps_max_points())" % ops.fps_max_points())
    dev = torch.device(device)
    depth, inst, camk = _depth_frames(frames, camK, dev)
    I, H, W = depth.shape
    job_img = torch.as_tensor(job_img, dtype=torch.int32).to(dev).contiguous()
    J = job_img.numel()
    RTs = torch.as_tensor(RTs).to(dev)
    scales = torch.as_tensor(scales).to(dev)
    if RTs.shape[0] != J or scales.shape != (J, 3):
        raise ValueError("clouds_from_poses: RTs (J,4,4) and scales (J,3) are needed for the J jobs")
    centers, ladder = pose_balls(RTs, scales, ratio)
    kw = {}
    if masks is not None:
        if inst is None:
            raise ValueError("clouds_from_poses: masks need an 'inst_mask' in every frame")
        kw = dict(masks=inst.reshape(-1), mask_off=job_img.long() * (H * W), mask_stride=torch.ones_like(job_img),
                  mask_val=torch.as_tensor(masks, dtype=torch.int32).to(dev).contiguous())
    br = ops.ball_cloud(depth, job_img, centers, ladder, camk, cap=cap, full_scan=full_scan, **kw)
    if sampler == "device":
        out, pix = ops.ball_sample(br, n_pts, seed)
        ok = br.counts[:, 3] == 0
    elif sampler == "fps":
        out, pix, ok = _ball_fps(br, n_pts, fps_pool)
    else:
        counts = br.counts.cpu().numpy()                     # the one read-back: 16 bytes per job
        sel = np.full((J, n_pts), -1, dtype=np.int32)
        for j in range(J):
            n = min(int(counts[j, 1]), br.cap)
            if counts[j, 3] == 0 and n > 0:
                total = n
                while total < n_pts:
                    total *= 2
                sel[j] = torch.randperm(total)[:n_pts].numpy()
        out, pix = ops.ball_select(br, torch.from_numpy(sel).to(dev))
        ok = br.counts[:, 3] == 0
    return (out, ok, pix, br.counts) if return_counts else (out, ok, pix)
