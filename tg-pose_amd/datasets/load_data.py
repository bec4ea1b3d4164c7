"""Device half of the TRAINING loader (the part round 2 left open).

Stands where ``PoseDataset.__getitem__`` of ``datasets/load_data.py`` does its per-item image work (:232-290, 335-336): the ROI
resampling of pixel grid / ground-truth instance mask / depth with nearest-neighbour ``cv2.warpAffine``
(``crop_resize_by_warp_affine``, tools/dataset_utils.py:80-136), the validity tests (:260-265), ``_depth_to_pcl`` (:395-407) / 1000,
the cut of the points within 0.15 x the extent's diagonal of point number 25 (:276-286), the ``len(pcl_in) < 50`` test (:288) and the
double subsample ``_sample_points(PC, 2048)`` then ``_sample_points(PC, 1024)`` (:335-336, 366-380).  A batch of items is ONE launch
of the evaluation loader's kernel (``tgp_roi_cloud_ex``: a workgroup per item, clouds kept as 4-byte records in the reference's
point order) plus one gather of the 2048 selected points (``tgp_cloud_select_ex``) and a row gather of the 1024 selected among them.

What differs from the evaluation loader, and how the kernel takes it:
  * the mask is the frame's instance-id image and the item is ``mask == inst_id`` (:245-247) -> ``mask_val``;
  * the window comes from ``aug_bbox_DZI`` (tools/dataset_utils.py:24-61), i.e. from the caller's augmentation draw: a real-valued
    centre and scale for which OpenCV's 10-bit fixed-point walk has no integer closed form -> ``source_tables`` evaluates that
    walk once per item on the host, in double as OpenCV does, and the kernel looks source pixels up;
  * the cut keeps the points farther than 0.15 (not 0.25) of the diagonal -> ``cut_frac``.

``train_clouds`` returns the clouds with the cloud augmentation off: with it off the result is the reference's ``pcl_in`` bit for bit
given the same ``np.random`` state (tests/test_gpu_parity.py::test_train_loader_vs_reference_getitem).  ``train_batch`` adds the
reference's two cloud augmentations (:333-350): ``PC_BasicAugment`` and the second view ``aug_pcl_in``, one ``tgp_augment`` launch for
the batch (datasets/data_augmentation.py of this package), with the draws made on the host in the reference's order.

``roi_mask_pro`` adds the reference's mask deformation ``defor_2D`` (:280, datasets/data_augmentation.py:319-342): a band launch
(``tgp_roi_band``: per item n_depth, the undeformed n_valid, the band size l), ONE read-back, the host's draws, then the deformed
compaction (``tgp_roi_cloud_defor``) in place of ``tgp_roi_cloud_ex``.  ``dzi=True`` draws ``aug_bbox_DZI``
(tools/dataset_utils.py:24-61) from the same ``rng`` (``aug_bbox_dzi``).  Out of scope, as in DESIGN.md section 8: reading
files.

``draws='device'`` (train_batch, train_clouds, TrainBatches; opt-in) makes every draw a function of (seed, item key, site, counter)
instead of a position in ``rng`` / ``gen``, the per-point ones and the permutations on the device (csrc/draws.hip), and reads nothing
back: the reference's distributions, not its stream ("Draws on the device")."""
import numpy as np
import torch

from .. import ops
from . import data_augmentation as da
from ..evaluation.load_data_eval import CAMERA_INTRINSICS, REAL_INTRINSICS, get_bbox  # noqa: F401  (re-exported)

AB_BITS = 10          # OpenCV's warpAffine works in 10-bit fixed point (AB_SCALE = 1024)


def _category_id(c):
    from ..evaluater.RT_TDA_Evaluater import SYNSET_NAMES
    return SYNSET_NAMES.index(c) if isinstance(c, str) and c in SYNSET_NAMES[1:] else None


def get_fs_net_scale(c, model, nocs_scale):
    """PoseDataset.get_fs_net_scale (datasets/load_data.py:453-519): category name c, model (P,3) in NOCS units, nocs_scale ->
    (the size residual, the category's mean size), both (3,) in millimetres.  The mean sizes are the evaluater's MEAN_SHAPE_MM;
    a name outside the six categories raises NotImplementedError (the ShapeNet synset ids the reference also lists are not kept)."""
    from ..evaluater.RT_TDA_Evaluater import MEAN_SHAPE_MM
    k = _category_id(c)
    if k is None:
        raise NotImplementedError("get_fs_net_scale: category %r is not one of the six" % (c,))
    model = np.asarray(model)
    size = (model.max(0) - model.min(0)) * nocs_scale * 1000                 # the model's extent in millimetres
    mean = np.array(MEAN_SHAPE_MM[k])
    return size - mean.astype(size.dtype), mean


def get_sym_info(c, mug_handle=1):
    """PoseDataset.get_sym_info (datasets/load_data.py:521-543) -> (4,) int32 from the evaluater's SYM_INFO; a mug without a visible
    handle is (1, 0, 0, 0); any other name is zeros, as in the reference"""
    from ..evaluater.RT_TDA_Evaluater import SYM_INFO
    k = _category_id(c)
    if k is None:
        return np.array([0, 0, 0, 0], dtype=np.int32)
    if c == "mug" and mug_handle == 0:
        return np.array([1, 0, 0, 0], dtype=np.int32)
    if c == "mug" and mug_handle != 1:
        return np.array([0, 0, 0, 0], dtype=np.int32)
    return np.array(SYM_INFO[k], dtype=np.int32)


def window_without_dzi(bbox, im_H, im_W):
    """load_data.py:233-238 when FLAGS.DZI_TYPE names none of the augmenting kinds (tools/dataset_utils.py:57-61): get_bbox's window
    -> (bbox_center (cx, cy) float64, scale)."""
    rmin, rmax, cmin, cmax = get_bbox(bbox)
    return np.array([0.5 * (cmin + cmax), 0.5 * (rmin + rmax)]), min(max(rmax - rmin, cmax - cmin), max(im_H, im_W)) * 1.0


def source_tables(bbox_center, scale, img_size=256):
    """Source pixel of every ROI column and row: cv2.warpAffine(img, get_affine_transform(center, scale, 0, img_size), INTER_NEAREST).

    tools/dataset_utils.py:95-136 builds three float32 point pairs for rot = 0 -- (centre, centre - (0, scale / 2), and their
    perpendicular third) onto (size / 2, size / 2), ... -- and cv2.getAffineTransform solves for the 2 x 3 matrix in double; with
    rot = 0 that matrix is diag(size / scale) plus a shift, written down here from the same float32 points.  cv2.warpAffine inverts
    it in double and walks X = (round((M01 y + M02) 1024) + 512 + round(M00 x 1024)) >> 10 (likewise Y) with round-half-even.
    -> (2, img_size) int32: [0] source column per ROI column, [1] source row per ROI row."""
    c = np.asarray(bbox_center, dtype=np.float64)
    # the three point pairs, in the arithmetic types the reference's set-up uses (float32 arrays filled from float64 sums, the
    # perpendicular third point in float32): the matrix must agree with OpenCV's to the last bit of those points
    src, dst = np.zeros((3, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32)
    src[0] = c
    src[1] = c + np.array([0.0, scale * -0.5])
    dst[0] = [img_size * 0.5, img_size * 0.5]
    dst[1] = np.array([img_size * 0.5, img_size * 0.5], np.float32) + np.array([0, img_size * -0.5], np.float32)
    perp = lambda a, b: b + np.array([-(a - b)[1], (a - b)[0]], dtype=np.float32)
    src[2], dst[2] = perp(src[0], src[1]), perp(dst[0], dst[1])
    pairs = [(src[i].astype(np.float64), dst[i].astype(np.float64)) for i in range(3)]
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for i, (s, d) in enumerate(pairs):
        A[2 * i, 0:2], A[2 * i, 2] = s, 1.0
        A[2 * i + 1, 3:5], A[2 * i + 1, 5] = s, 1.0
        b[2 * i], b[2 * i + 1] = d
    M = np.linalg.solve(A, b).reshape(2, 3)
    # cv2.warpAffine without WARP_INVERSE_MAP: invert in double
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    i00, i01, i10, i11 = A11, M[0, 1] * -D, M[1, 0] * -D, A22
    b1 = -i00 * M[0, 2] - i01 * M[1, 2]
    b2 = -i10 * M[0, 2] - i11 * M[1, 2]
    scale_ab = float(1 << AB_BITS)
    x = np.arange(img_size, dtype=np.float64)
    rnd = lambda v: np.rint(v).astype(np.int64)
    half = 1 << (AB_BITS - 1)
    adelta, bdelta = rnd(i00 * x * scale_ab), rnd(i10 * x * scale_ab)               # per ROI column
    X0, Y0 = rnd((i01 * x + b1) * scale_ab) + half, rnd((i11 * x + b2) * scale_ab) + half      # per ROI row
    # rot = 0: the cross terms i01, i10 are the solver's rounding noise (~1e-17), so X0 does not depend on the row nor bdelta on the
    # column and the map is separable; a window for which that noise moves a rounding tie is refused rather than approximated
    # OpenCV's map of pixel (r, c) is ((X0[r] + adelta[c]) >> 10, (Y0[r] + bdelta[c]) >> 10): whether the first depends on r (the second
    # on c) is decided by the DISTINCT values of X0 (bdelta) -- a handful, the noise's -- so only those rows (columns) are walked
    tabs = _separable_walk(X0, adelta, Y0, bdelta)
    if tabs is None:
        raise ValueError("source_tables: the walk is not separable for this window (rot = 0 expected)")
    sx, sy = tabs
    return np.clip(np.stack([sx, sy]), -32768, 32767).astype(np.int32)       # (OpenCV stores the map as shorts)


def _separable_walk(X0, adelta, Y0, bdelta):
    """(source column per ROI column, source row per ROI row) of the map (r, c) -> ((X0[r] + adelta[c]) >> 10, (Y0[r] + bdelta[c]) >> 10),
    or None when the column depends on r or the row on c.  Only the rows of the distinct X0 (the columns of the distinct bdelta) are
    walked: which rows differ is decided by the values alone."""
    sx, sy = (X0[0] + adelta) >> AB_BITS, (Y0 + bdelta[0]) >> AB_BITS
    sx2, sy2 = (np.unique(X0)[:, None] + adelta[None, :]) >> AB_BITS, (Y0[:, None] + np.unique(bdelta)[None, :]) >> AB_BITS
    return (sx, sy) if (sx2 == sx[None, :]).all() and (sy2 == sy[:, None]).all() else None


def aug_bbox_dzi(bbox, im_H, im_W, rng=np.random, dzi_type=None, scale_ratio=None, shift_ratio=None, pad_scale=None):
    """aug_bbox_DZI (tools/dataset_utils.py:24-61) on get_bbox's window of bbox (y1, x1, y2, x2), as load_data.py:233-238 calls
    it, drawing from ``rng``; None takes FLAGS.DZI_*.  Every branch of the reference, its roi10d ``x2 = min(max(x1, 0), im_W)``
    included.  -> (bbox_center (cx, cy) float64, scale)"""
    from ..config import FLAGS
    dzi_type = FLAGS.DZI_TYPE if dzi_type is None else dzi_type
    scale_ratio = FLAGS.DZI_SCALE_RATIO if scale_ratio is None else scale_ratio
    shift_ratio = FLAGS.DZI_SHIFT_RATIO if shift_ratio is None else shift_ratio
    pad_scale = FLAGS.DZI_PAD_SCALE if pad_scale is None else pad_scale
    rmin, rmax, cmin, cmax = get_bbox(bbox)
    x1, y1, x2, y2 = np.array([cmin, rmin, cmax, rmax]).copy()
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    bh, bw = y2 - y1, x2 - x1
    kind = dzi_type.lower()
    if kind == "uniform":
        sr = 1 + scale_ratio * (2 * rng.random_sample() - 1)
        sh = shift_ratio * (2 * rng.random_sample(2) - 1)
        center = np.array([cx + bw * sh[0], cy + bh * sh[1]])
        scale = max(y2 - y1, x2 - x1) * sr * pad_scale
    elif kind == "roi10d":
        a, b = -0.15, 0.15
        x1 += bw * (rng.rand() * (b - a) + a)
        x2 += bw * (rng.rand() * (b - a) + a)
        y1 += bh * (rng.rand() * (b - a) + a)
        y2 += bh * (rng.rand() * (b - a) + a)
        x1 = min(max(x1, 0), im_W)
        x2 = min(max(x1, 0), im_W)               # sic: the reference clamps x1 into x2
        y1 = min(max(y1, 0), im_H)
        y2 = min(max(y2, 0), im_H)
        center = np.array([0.5 * (x1 + x2), 0.5 * (y1 + y2)])
        scale = max(y2 - y1, x2 - x1) * pad_scale
    elif kind == "truncnorm":
        raise NotImplementedError("DZI truncnorm not implemented yet.")
    else:
        center = np.array([cx, cy])
        scale = max(y2 - y1, x2 - x1)
    return center, min(scale, max(im_H, im_W)) * 1.0


def defor_draws(band_counts, roi_mask_pro, rng=np.random):
    """defor_2D's draws (data_augmentation.py:327-336) for a batch, from the band launch's (D,3) counts (n_depth, undeformed n_valid,
    band size l), item by item: none for an item the validity tests (:259-264) abandon; else rng.rand(), and when it is not
    > roi_mask_pro and l >= 1, rng.choice(l, l // 2, replace=False) (the band ranks set to 0).
    -> (defor_on (D,) int32, drop_bits (D, words) int32: bit r of row d = band rank r dropped)"""
    D = len(band_counts)
    on = np.zeros(D, np.int32)
    chosen = [None] * D
    for d in range(D):
        n_depth, n_valid, l = (int(v) for v in band_counts[d])
        if n_depth <= 1 or n_valid <= 1:
            continue
        if rng.rand() > roi_mask_pro:
            continue
        if l < 1:
            continue
        chosen[d] = np.asarray(rng.choice(l, l // 2, replace=False), dtype=np.int64)
        on[d] = 1
    words = max([(int(band_counts[d][2]) + 31) // 32 for d in range(D) if on[d]] or [0])
    flags = np.zeros((D, words * 32), np.uint8)
    for d in range(D):
        if on[d]:
            flags[d, chosen[d]] = 1
    bits = np.packbits(flags, axis=1, bitorder="little").reshape(D, words * 4).view("<u4").view(np.int32)
    return on, np.ascontiguousarray(bits)


def _selection(total, n_pts, rng):
    """_sample_points (:366-380) as indices: tile when short, the prefix of one permutation when long"""
    if total < n_pts:
        return np.arange(n_pts) % total
    if total > n_pts:
        return rng.permutation(total)[:n_pts]
    return np.arange(n_pts)


def farthest_point_sample(xyz, npoint):
    """PoseDataset.farthest_point_sample (load_data.py:382-393): the indices of ``npoint`` farthest points of xyz (M,3), a float32
    GPU tensor, in selection order (core/utils/farthest_points_torch.farthest_points with init_center=True)"""
    from ..core.utils.farthest_points_torch import farthest_points
    _, idx = farthest_points(xyz, n_clusters=npoint, return_center_indexes=True, init_center=True)
    return idx


def train_clouds(items, img_size=256, rng=np.random, device="cuda", min_points=50, roi_mask_pro=None, roi_mask_r=3, dzi=False,
                 draws="host", seed=None, keys=None, batch_size=None):
    """items: list of dicts -- 'depth' (H,W) uint16 (load_depth's output), 'mask' (H,W) uint8 instance-id image (the reference reads
    ``cv2.imread(mask_path)[:, :, 2]``), 'inst_id' int, 'camK' (3,3) float32, and the window: 'bbox_center' (cx, cy) + 'scale' (the
    caller's aug_bbox_DZI draw) or 'bbox' (y1, x1, y2, x2) for the un-augmented window.  All frames share (H, W).
    -> list over items of (PC (2048,3), pcl_in (1024,3)) float32 GPU tensors, or None for an item the reference's __getitem__
    abandons and retries (:262-265 too few valid pixels, :288 fewer than 50 points after the cut).  The two permutations per item
    are drawn from ``rng`` in the reference's order (item by item, 2048 first).  One 12-byte read-back per item (the counts).
    dzi=True: the window is drawn by aug_bbox_dzi from each item's 'bbox' (FLAGS.DZI_*), all items first.  roi_mask_pro (a float;
    None: no deformation, no draw): defor_2D on each item's mask after one more read-back (defor_draws, after the DZI draws);
    roi_mask_r is inert, as in the reference (it reaches cv2.erode / dilate as their dst).  For one item the stream is the
    reference's from aug_bbox_DZI on; for a batch, every item's DZI and deformation draws precede the first permutation.
    draws='device' (seed, keys, batch_size as train_batch's): the same draws as train_batch(draws='device') makes up to the second
    selection, nothing read back -> dict PC (B,2048,3), pcl_in (B,1024,3), n_alive, status, item_index."""
    dev = torch.device(device)
    if draws not in ("host", "device"):
        raise ValueError("draws must be 'host' or 'device'")
    if not items:
        return []
    if draws == "device":
        return _train_batch_device(items, seed, keys, batch_size, img_size, dev, min_points, da.default_operators(), False, roi_mask_pro,
                                   roi_mask_r, dzi, clouds_only=True)
    rr, counts = _roi_records(items, img_size, dev, rng, roi_mask_pro, roi_mask_r, dzi)
    D = len(items)
    sel2k, p1k = np.zeros((D, 2048), dtype=np.int32), np.zeros((D, 1024), dtype=np.int32)
    alive = []
    for d in range(D):
        total = _item_total(counts[d], min_points, roi_mask_pro is not None)
        alive.append(total is not None)
        if alive[d]:
            sel2k[d] = _selection(total, 2048, rng)                # PC = _sample_points(PC, 2048)
            p1k[d] = _selection(2048, 1024, rng)                   # pcl_in = _sample_points(PC, 1024): a selection of the selection
    up = _pageable(dev)
    pc2k, pc1k = _two_clouds(rr, up(sel2k), up(p1k))
    pc1k = pc1k[..., :3].contiguous()
    return [(pc2k[d], pc1k[d]) if alive[d] else None for d in range(D)]


def _two_clouds(rr, sel2k, p1k):
    """PC = the records' points sel2k (D,2048), pcl_in = PC's rows p1k (D,1024) -> (D,2048,3), (D,1024,4) padded to 4 columns"""
    pc2k = ops.cloud_select(rr, sel2k)
    return pc2k, ops.gather_rows(torch.nn.functional.pad(pc2k, (0, 1)), p1k, torch.empty(len(p1k), 1024, 4, device=pc2k.device))


def _pageable(dev):
    """host array -> device tensor by a blocking copy from pageable memory (the host modes; draws='device' has _uploader)"""
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _window(it, H, W, dzi_rng=None):
    """an item's window (bbox_center, scale): aug_bbox_dzi's draw from dzi_rng (load_data.py:238), else its own, else get_bbox's"""
    if dzi_rng is not None:
        return aug_bbox_dzi(it["bbox"], H, W, dzi_rng)
    if "bbox_center" in it:
        return it["bbox_center"], it["scale"]
    return window_without_dzi(it["bbox"], H, W)


def _records(items, tabs, up, H, W, img_size, defor=None):
    """the frame upload and the items' ROI clouds as records, ONE tgp_roi_cloud_ex launch -- or, with defor = (defor_on, drop_bits) or a
    function that makes that pair from the band launch's (D,3) device counts, tgp_roi_cloud_defor -> (RoiRecords, the pair or None)"""
    args, tabs, mval, camk = _upload_frames(items, tabs, up, H, W)
    if callable(defor):
        defor = defor(ops.roi_band(*args, roi_size=img_size, tables=tabs, mask_val=mval))
    return ops.roi_cloud(*args, camk, roi_size=img_size, tables=tabs, mask_val=mval, cut_frac=0.15, defor=defor), defor


def _roi_records(items, img_size, dev, rng=np.random, roi_mask_pro=None, roi_mask_r=3, dzi=False):
    """the items' ROI clouds as records (one tgp_roi_cloud_ex launch) and their counts (one 12-byte read-back per item); with
    roi_mask_pro, the band launch, its read-back, the deformation draws and one tgp_roi_cloud_defor launch instead"""
    H, W = _check_items(items, roi_mask_pro, roi_mask_r, dzi)
    tabs = [source_tables(*_window(it, H, W, rng if dzi else None), img_size) for it in items]
    up = _pageable(dev)
    defor = None
    if roi_mask_pro is not None:              # the extra read-back, then :280
        defor = lambda band: tuple(up(a) for a in defor_draws(band.cpu().numpy(), float(roi_mask_pro), rng))
    rr = _records(items, tabs, up, H, W, img_size, defor)[0]
    return rr, rr.counts.cpu().numpy()


def _check_items(items, roi_mask_pro, roi_mask_r, dzi):
    """the argument checks of a batch of items, before the first draw -> (H, W)"""
    if roi_mask_pro is not None and not (isinstance(roi_mask_pro, (float, int)) and 0.0 <= float(roi_mask_pro) <= 1.0):
        raise ValueError("roi_mask_pro must be None or a probability in [0, 1]")
    if not (isinstance(roi_mask_r, (int, np.integer)) and roi_mask_r >= 0):
        raise ValueError("roi_mask_r must be a non-negative int (it is inert, as in the reference)")
    if dzi and any("bbox" not in it for it in items):
        raise ValueError("dzi=True draws the window from each item's 'bbox'")
    H, W = items[0]["depth"].shape
    for it in items:            # every item is checked before the first draw: a refused batch leaves rng untouched
        if it["depth"].shape != (H, W) or it["mask"].shape != (H, W) or it["depth"].dtype != np.uint16 or it["mask"].dtype != np.uint8:
            raise ValueError("every item needs a uint16 depth image and a uint8 instance mask of one common (H,W)")
        if not 0 < int(it["inst_id"]) < 256:
            raise ValueError("inst_id must be a non-zero byte value")
    return H, W


def _item_total(counts, min_points, deformed=False):
    """the cut cloud's point count, or None for an item the reference abandons.  deformed: the counts of tgp_roi_cloud_defor, whose
    third entry is -(1 + the deformed point count) below 26 points (tgp_roi_cloud_ex writes -1 and the count is n_valid)"""
    n_depth, n_valid, total = (int(v) for v in counts)
    if n_depth <= 1 or n_valid <= 1:                           # :262-265
        return None
    if total < 0:
        n = -1 - total if deformed else n_valid
        if n == 0:                                             # :272, np.min over the empty deformed cloud
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        raise IndexError("index 25 is out of bounds for axis 0 with size %d" % n)                # :281
    if total < min_points:                                     # :288
        return None
    return total


_IMAGE_KEYS = ("depth", "mask", "inst_id", "camK", "bbox_center", "scale", "bbox")
_POSE_KEYS = ("rotation", "translation", "fsnet_scale")


def train_batch(items, rng=np.random, gen=None, img_size=256, device="cuda", min_points=50, operators=None, persistence=False,
                roi_mask_pro=None, roi_mask_r=3, dzi=False, draws="host", seed=None, keys=None, batch_size=None, keep_draws=False,
                pcl_select="random"):
    """``train_clouds`` plus the reference's two augmentations (load_data.py:333-350): the batch the trainer's step reads.

    items: ``train_clouds``' dicts, each also carrying its labels 'rotation' (3,3), 'translation' (3,), 'fsnet_scale' (3,) (the
    residual), 'mean_shape' (3,), 'sym_info' (4,), 'model_point' (n_model,3) (one n_model for the batch), 'nocs_scale' and 'cat_id'
    (0-based).  Any other key (e.g. 'pdh1', 'points_category') is stacked and passed through.
    Per item, in the reference's order: generate_aug_parameters (``rng``), PC_BasicAugment's torch draws (``gen``; None: torch's
    default CPU generator, as the reference draws on the CPU), the two _sample_points permutations, the operator's randint(0, 4) and
    its draws (``operators``: default_operators()), pc_sampler's shuffle.  One launch of tgp_augment for the batch (base augmentation
    on the 2048 selected points, then the second view in LDS) and two tgp_gather_rows (pcl_in, aug_pcl_in).

    Deviations from one reference __getitem__ after another: crop and cutout draw all their attempts up front;
    the shuffle of an item whose operator is crop or cutout needs its kept count M, so it is drawn after ONE read-back of the counts
    for the batch, after every other item's draws; dzi=True / roi_mask_pro (see train_clouds) draw aug_bbox_DZI and defor_2D for
    every item of the batch before the first item's generate_aug_parameters (without them those draws stay with the caller).  A
    batch of one item without an applied crop or cutout draws exactly the reference's stream from aug_bbox_DZI through pc_sampler.
    Items the reference abandons (train_clouds' None) are left out, without draws; 'item_index' lists the items kept.
    -> dict of device tensors: pcl_in (B,1024,3), aug_pcl_in (B,1024,3), rotation (B,3,3), translation (B,3), fsnet_scale (B,3),
    the labels passed through, aug_flags (B,4) int32 {bb, rt, bc, pc}, aug_counts (B,2) int32 (M, accepted attempt or -1),
    item_index (B,) int64; and aug_name, a list of the operators' names.
    persistence=True also computes the reference's compute_pd targets from pcl_in (load_data.py:343): pdh1 and pdh2 (B, 2500)
    float32, by ops.persistence_images (no random draws, so the draw order above is unchanged); items that carry 'pdh1' or 'pdh2'
    themselves are refused.

    draws='device' (opt-in; 'host' is everything above, unchanged): no host read between the items and the returned batch.  Every
    draw is a pure function of (seed, keys[d], draw site, counter) -- Philox-4x32-10, csrc/draws.hip and device_draws.py -- so an
    item's rows depend on neither its slot, its batch nor rng / gen (not consumed); the reference's distributions, not its
    stream.  ``keys``: 64 bits per item (default: its position).  ``batch_size`` = B <= len(items): the batch holds the first B
    items, in item order, that the reference would keep (the rest are spares); with fewer than B alive the alive ones repeat
    cyclically, with none the rows are zeros.  An item whose deformed cloud has fewer than 26 points (the host path raises there) or
    whose drawn window source_tables refuses counts as abandoned.  -> the dict above, all on the device, with aug_op (B,) int32
    (the OPERATOR_NAMES index) in place of aug_name, item_index (B,) int64 (the item in each slot, -1 without one), n_alive ()
    int32 = min(alive items, B) and status (len(items),) int32 (TGP_ITEM_* of include/tgpose.h).  keep_draws=True adds '_draws':
    the draw buffers (DRAW_KEYS, one row per item) that _train_batch_from_draws replays.

    pcl_select='fps' (opt-in; 'random' is everything above, unchanged, draw streams included): pcl_in is the farthest point sampling
    of the augmented 2048-point cloud -- what the reference's _sample_points docstring announces and its farthest_point_sample
    method computes, but its __getitem__ never calls (:366-393) -- by ops.farthest_points (csrc/fps.hip, one launch for the batch,
    reading the padded rows in place; centroid start, DESIGN.md section 3 "Farthest point sampling").  A deviation from the
    reference's stream: the second _sample_points permutation is NOT drawn, so with draws='host' every later
    draw from ``rng`` moves up by that permutation; with draws='device' its site is simply not used and every other draw is the
    same.  persistence=True then runs on the FPS pcl_in.  In this mode only, the batch also carries PC (B,2048,3), the augmented
    cloud, and pcl_index (B,1024) int32, its rows in selection order: pcl_in == PC[pcl_index]."""
    if draws not in ("host", "device"):
        raise ValueError("draws must be 'host' or 'device'")
    if pcl_select not in ("random", "fps"):
        raise ValueError("pcl_select must be 'random' or 'fps'")
    fps = pcl_select == "fps"
    if persistence and any("pdh1" in it or "pdh2" in it for it in items):
        raise ValueError("train_batch: persistence=True computes pdh1 / pdh2; the items must not carry them")
    dev = torch.device(device)
    ops_ = da.default_operators() if operators is None else list(operators)
    if len(ops_) != 4:
        raise ValueError("train_batch: the four operators of OPERATOR_NAMES are expected")
    if not items:
        raise ValueError("train_batch: no items")
    if draws == "device":
        return _train_batch_device(items, seed, keys, batch_size, img_size, dev, min_points, ops_, persistence, roi_mask_pro, roi_mask_r,
                                   dzi, keep_draws=keep_draws, fps=fps)
    rr, counts = _roi_records(items, img_size, dev, rng, roi_mask_pro, roi_mask_r, dzi)
    keep, names, recs, shuf, defer = [], [], [], [], []
    h = {k: [] for k in ("aug_bb", "aug_rt_t", "aug_rt_R", "base", "defor", "p1k")}        # DRAW_KEYS buffers, a row per kept item
    sel2k = np.zeros((len(items), 2048), dtype=np.int32)                                      # (a row per item: the records')
    for d in range(len(items)):
        total = _item_total(counts[d], min_points, roi_mask_pro is not None)
        if total is None:
            continue
        keep.append(d)
        for k, v in zip(("aug_bb", "aug_rt_t", "aug_rt_R"), da.generate_aug_parameters(rng)):     # :318
            h[k].append(v)
        base, defor = da.base_draws(1, total, "cpu", gen=gen, defor_gen=gen)      # :333 base_aug
        sel2k[d] = _selection(total, 2048, rng)                                   # :335
        h["base"].append(base[0].numpy())
        h["defor"].append(defor[0].numpy()[sel2k[d]])                             # the rows of the selected points only
        if not fps:
            h["p1k"].append(_selection(2048, 1024, rng).astype(np.int32))         # :336
        k = int(rng.randint(0, len(ops_)))                                        # :346
        recs.append(ops_[k].draw(2048, rng, gen))                                 # :347
        names.append(da.OPERATOR_NAMES[k])
        if recs[-1]["op"] in (da._lib.AUG_CROP, da._lib.AUG_CUTOUT):
            shuf.append(None)                                                     # M comes from the kernel
            defer.append(len(keep) - 1)
        else:
            shuf.append(da.sampler_perm(2048, 1024, rng))                         # :348 pc_sampler
    if not keep:
        raise ValueError("train_batch: every item was abandoned")
    up = _pageable(dev)

    def shuffle(counts):
        if defer:                                                                 # the batch's one read-back of M
            m = counts[:, 0].cpu().numpy()
            for i in defer:
                shuf[i] = da.sampler_perm(int(m[i]), 1024, rng)
        return up(np.stack(shuf))
    kept = up(np.asarray(keep, dtype=np.int64))
    lab = _stack_labels([items[d] for d in keep], up)
    dr = {k: up(np.stack(v)) for k, v in h.items() if v}
    dr.update({k: up(v) for k, v in da.view_arrays(recs, 2048).items()}, sel2k=up(sel2k))
    db = _augment_rows(rr, dr, lab, ops_, shuffle, fps, rows=kept if len(keep) != len(items) else None)
    del db["shuf"]
    db.update({k: v for k, v in lab.items() if k not in _POSE_KEYS}, item_index=kept, aug_name=names)
    _unpad(db)
    if persistence:
        db["pdh1"], db["pdh2"] = ops.persistence_images(db["pcl_in"])
    return db


# ---------------------------------------------------------------------------------------- draws='device': no read between the items
# and the step.  Every draw is a function of (seed, item key, site, counter) (device_draws.py, csrc/draws.hip): the per-item scalars are
# made on the host from site 0, everything whose size or existence depends on a device result -- or that scales with the point
# count -- on the device, into the buffers the host path uploads.  All D = batch_size + spares items run through every launch; the
# batch's slots are filled from the alive ones at the end (tgp_draw_alive, tgp_gather_slots).
_DROP_WORDS = 2048          # 65536 band ranks: every ROI size


def _uploader(dev):
    """host array -> device tensor without stalling the host on a CUDA device: through pinned memory, non-blocking"""
    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev)
    return up


def _upload_frames(items, tabs, up, H, W):
    """the frames and per-item descriptors of tgp_roi_band / tgp_roi_cloud_* -> (args, tables, mask_val, camk)"""
    D = len(items)
    camk = []
    for it in items:
        K = np.asarray(it["camK"], dtype=np.float32)
        camk.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    depth = up(np.stack([it["depth"] for it in items]).view(np.int16))
    masks = up(np.stack([it["mask"] for it in items]).reshape(-1))
    args = (depth, masks, up(np.arange(D, dtype=np.int64) * (H * W)), up(np.ones(D, dtype=np.int32)), up(np.arange(D, dtype=np.int32)), None)
    return args, up(np.asarray(tabs, dtype=np.int32)), up(np.asarray([int(it["inst_id"]) for it in items], dtype=np.int32)), \
        up(np.asarray(camk, dtype=np.float32))


def _stack_labels(items, up):
    lab = {k: [it[k] for it in items] for k in items[0] if k not in _IMAGE_KEYS}
    for k in _POSE_KEYS + ("mean_shape", "sym_info", "model_point", "nocs_scale", "cat_id"):
        if k not in lab:
            raise ValueError("train_batch: every item needs %r" % k)
    return {k: up(np.stack([np.asarray(v, dtype=np.float32) for v in lab[k]])) for k in lab}


def _keyed_record(op, st):
    """an operator's scalar draws from an item's stream; its per-point draws (noise, drop_u) are made on the device"""
    if isinstance(op, da.PcJitter):
        return da._record(da._lib.AUG_NONE if st.uniform() > op.p else da._lib.AUG_JITTER, 2048)
    if isinstance(op, da.PcRandomDropout):
        if op._skip(st):
            return da._record(da._lib.AUG_NONE, 2048)
        return da._record(da._lib.AUG_DROPOUT, 2048, drop_ratio=st.random_sample() * op.max_dropout_ratio)
    return op.draw(2048, st, None)


def _item_scalars(items, seed, keys, H, W, img_size, dzi, ops_):
    """the per-item scalars of draws='device', from each item's stream (device_draws.ItemStream) -> dict of host arrays, D rows:
    tabs, forced (TGP_ITEM_WINDOW where source_tables refused the window), u_defor, aug_bb, aug_rt_t, aug_rt_R, base (the six
    PC_BasicAugment draws), op_index, op, drop_ratio, boxes"""
    from . import device_draws as dd
    D = len(items)
    sc = dict(tabs=np.zeros((D, 2, img_size), np.int32), forced=np.zeros(D, np.int32), u_defor=np.zeros(D), aug_bb=np.zeros((D, 3), np.float32),
              aug_rt_t=np.zeros((D, 3), np.float32), aug_rt_R=np.zeros((D, 3, 3), np.float32), base=np.zeros((D, 6), np.float32),
              op_index=np.zeros(D, np.int32), op=np.zeros(D, np.int32), drop_ratio=np.zeros(D), boxes=np.zeros((D, da._lib.AUGMENT_MAX_TRY, 6)))
    for d, (it, st) in enumerate(zip(items, dd.item_streams(seed, keys))):
        try:
            sc["tabs"][d] = source_tables(*_window(it, H, W, st.seek(st.DZI) if dzi else None), img_size)
        except ValueError:                       # not separable: the item is abandoned (its table stays pixel (0, 0))
            sc["forced"][d] = da._lib.ITEM_WINDOW
        sc["u_defor"][d] = st.seek(st.DEFOR).rand()
        sc["aug_bb"][d], sc["aug_rt_t"][d], sc["aug_rt_R"][d] = da.generate_aug_parameters(st.seek(st.PARAMS))
        sc["base"][d] = st.seek(st.BASE).floats32(6)
        k = st.seek(st.OP_INDEX).randint4()
        rec = _keyed_record(ops_[k], st.seek(st.OPERATOR))
        sc["op_index"][d], sc["op"][d], sc["drop_ratio"][d] = k, rec["op"], rec["drop_ratio"]
        if rec["boxes"] is not None:
            sc["boxes"][d] = rec["boxes"]
    return sc


DRAW_KEYS = ("tabs", "defor_on", "drop_bits", "aug_bb", "aug_rt_t", "aug_rt_R", "base", "op", "drop_ratio", "boxes", "sel2k", "p1k", "defor",
             "noise", "drop_u", "shuf")


def _augment_rows(rr, dr, lab, ops_, shuffle=None, fps=False, rows=None):
    """the launches that follow the records, the same for every mode, from the draws ``dr`` (device tensors under DRAW_KEYS): the 2048
    selected points, tgp_augment, the two row gathers.  shuffle(counts) draws 'shuf' when dr has none (it needs the launch's M).
    fps: the rows of pcl_in are the farthest point sampling of the augmented cloud instead of dr['p1k'] (not read).
    rows (B,) int64: the items to go on with after the selection, which runs on every item of rr with dr['sel2k']; lab and the
    rest of dr then hold B rows, for those items (the host path's kept items: an abandoned item's points never reach tgp_augment).
    -> dict of (B, ...) tensors: pcl_in, aug_pcl_in (padded to 4 columns), rotation, translation, fsnet_scale, aug_flags, aug_counts,
    shuf; with fps also PC (the augmented cloud, padded to 4 columns) and pcl_index"""
    pc2k = ops.cloud_select(rr, dr["sel2k"])
    if rows is not None:
        pc2k = pc2k[rows].contiguous()
    B, dev = pc2k.shape[0], pc2k.device
    base = da._base_inputs(dr["base"], lab["rotation"], lab["translation"], lab["fsnet_scale"], lab["mean_shape"], lab["sym_info"],
                           dr["aug_bb"], dr["aug_rt_t"], dr["aug_rt_R"], lab["cat_id"], lab["nocs_scale"], lab["model_point"], dr["defor"])
    view = dict(op=dr["op"], noise=dr["noise"], drop_ratio=dr["drop_ratio"], drop_u=dr["drop_u"], boxes=dr["boxes"], **da.view_limits(ops_))
    # padded (B, 2048, 4) outputs: tgp_gather_rows moves rows of a multiple of 4 floats
    out = ops.augment(pc2k, base=base, view=view, ld_out=4)
    shuf = dr["shuf"] if "shuf" in dr else shuffle(out["counts"])
    p1k = ops.farthest_points(out["pc"], 1024) if fps else dr["p1k"]
    pcl = ops.gather_rows(out["pc"], p1k, torch.empty(B, 1024, 4, device=dev))
    aug = ops.gather_rows(out["view"], shuf, torch.empty(B, 1024, 4, device=dev))
    got = dict(pcl_in=pcl, aug_pcl_in=aug, rotation=out["R"], translation=out["t"], fsnet_scale=out["s"], aug_flags=out["flags"],
               aug_counts=out["counts"], shuf=shuf)
    if fps:
        got.update(PC=out["pc"], pcl_index=p1k)
    return got


def _unpad(db):
    """cut the clouds that _augment_rows pads to 4 columns back to 3, in place"""
    for k in ("pcl_in", "aug_pcl_in", "PC"):
        if k in db:
            db[k] = db[k][..., :3].contiguous()


def _train_batch_from_draws(items, dr, img_size=256, device="cuda", min_points=50, operators=None, pcl_select="random"):
    """The host path's launches (_records, _augment_rows: the functions train_batch(draws='host') calls) on GIVEN draws: ``dr``
    holds host arrays under DRAW_KEYS, one row per item ('defor_on' / 'drop_bits' absent: no mask deformation) -- e.g. the buffers a
    draws='device' batch made, read back.  The counts are read back and the reference's rules applied on the host (_item_total; an
    item for which the host path raises counts as abandoned here).
    -> (dict of train_batch's device tensors, one row per KEPT item, list of the kept items)"""
    dev = torch.device(device)
    ops_ = da.default_operators() if operators is None else list(operators)
    H, W = _check_items(items, None, 3, False)
    up = _pageable(dev)
    t = {k: up(np.asarray(v)) for k, v in dr.items() if k in DRAW_KEYS and k != "tabs"}
    rr, defor = _records(items, dr["tabs"], up, H, W, img_size, (t["defor_on"], t["drop_bits"]) if "defor_on" in t else None)
    counts = rr.counts.cpu().numpy()
    keep = []
    for d in range(len(items)):
        try:
            if _item_total(counts[d], min_points, defor is not None) is not None:
                keep.append(d)
        except (ValueError, IndexError):
            pass
    got = _augment_rows(rr, t, _stack_labels(items, up), ops_, fps=pcl_select == "fps")
    kt = up(np.asarray(keep, dtype=np.int64))
    out = {k: v[kt].contiguous() for k, v in got.items()}
    _unpad(out)
    return out, keep


def _train_batch_device(items, seed, keys, batch_size, img_size, dev, min_points, ops_, persistence, roi_mask_pro, roi_mask_r, dzi,
                        keep_draws=False, clouds_only=False, fps=False):
    lib = da._lib
    D = len(items)
    B = D if batch_size is None else int(batch_size)
    if seed is None:
        raise ValueError("draws='device' needs a seed")
    if not 1 <= B <= D <= lib.DRAW_MAX_ITEMS:
        raise ValueError("draws='device': 1 <= batch_size <= len(items) <= %d" % lib.DRAW_MAX_ITEMS)
    keys = np.arange(D, dtype=np.uint64) if keys is None else np.asarray([int(k) & (2 ** 64 - 1) for k in keys], dtype=np.uint64)
    if keys.shape != (D,):
        raise ValueError("draws='device': one key per item")
    if dev.type != "cuda":
        raise ValueError("draws='device' needs a CUDA device")
    H, W = _check_items(items, roi_mask_pro, roi_mask_r, dzi)
    sc = _item_scalars(items, seed, keys, H, W, img_size, dzi, ops_)
    up = _uploader(dev)
    keys_t = up(keys.view(np.int64))
    dr = {k: up(sc[k]) for k in ("aug_bb", "aug_rt_t", "aug_rt_R", "base", "op", "drop_ratio", "boxes")}
    defor = None
    if roi_mask_pro is not None:
        defor = lambda band: ops.draw_band_subset(band, up(sc["u_defor"]), float(roi_mask_pro), keys_t, seed, drop_words=_DROP_WORDS)
    rr, defor = _records(items, sc["tabs"], up, H, W, img_size, defor)
    dr["tabs"] = rr.tables
    if defor is not None:
        dr["defor_on"], dr["drop_bits"] = defor
    status, slot, n_alive = ops.draw_alive(rr.counts, B, min_points, up(sc["forced"]))
    dr["sel2k"] = ops.draw_selection(rr.counts[:, 2], keys_t, seed, lib.SITE_SEL2K, 2048)
    if not fps:
        dr["p1k"] = ops.draw_selection(2048, keys_t, seed, lib.SITE_SEL1K, 1024)
    if clouds_only:
        pc2k, pc1k = ops.gather_slots(slot, _two_clouds(rr, dr["sel2k"], dr["p1k"]))
        return dict(PC=pc2k, pcl_in=pc1k[..., :3].contiguous(), n_alive=n_alive.reshape(()), status=status, item_index=slot.long())
    jit = next((o for o in ops_ if isinstance(o, da.PcJitter)), None)
    dr.update(ops.draw_fill(keys_t, seed, 2048, defor=True, noise=(jit.std, jit.clip) if jit is not None else (0.0, 0.0), drop_u=True))
    lab = _stack_labels(items, up)
    rows = _augment_rows(rr, dr, lab, ops_,
                         shuffle=lambda counts: ops.draw_selection(counts[:, 0], keys_t, seed, lib.SITE_SHUFFLE, 1024, shuffle_always=True),
                         fps=fps)
    names = [k for k in rows if k != "shuf"] + [k for k in lab if k not in _POSE_KEYS]
    src = [rows[k] for k in rows if k != "shuf"] + [lab[k] for k in lab if k not in _POSE_KEYS] + [up(sc["op_index"])]
    got = ops.gather_slots(slot, src)
    db = dict(zip(names + ["aug_op"], got))
    _unpad(db)
    db.update(n_alive=n_alive.reshape(()), status=status, item_index=slot.long())
    if persistence:            # no read here either: a failed cloud's images are zeros and 'pd_status' names the reason
        db["pdh1"], db["pdh2"], db["pd_status"] = ops.persistence_images(db["pcl_in"], check_status=False)
    if keep_draws:
        dr["shuf"] = rows["shuf"]
        db["_draws"] = dr
    return db


# ------------------------------------------------------------------------------------------------- the training loop's batches
CATEGORY_KEYS = ("points_category", "pdh1_category", "pdh2_category")


def epoch_batches(n, batch_size, gen=None, shuffle=True, drop_last=False, rank=0, world_size=1):
    """One epoch's item indices in batches, as DataLoader(shuffle=True, generator=gen) orders them: the loader's iterator draws its
    base seed from ``gen`` (None: torch's default CPU generator), then RandomSampler permutes with ``gen`` -- or, without one, with a
    generator seeded by one more draw.  Data parallel, as DistributedSampler splits: the
    order is padded with its own head to a multiple of world_size and rank r takes every world_size-th index from r, so every rank
    has the same number of batches (the ranks' ``gen`` must be seeded alike)."""
    if n <= 0 or batch_size <= 0:
        raise ValueError("epoch_batches: no items or a batch size below 1")
    if shuffle:
        torch.empty((), dtype=torch.int64).random_(generator=gen)                # the iterator's base seed
        if gen is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            order = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
        else:
            order = torch.randperm(n, generator=gen).tolist()
    else:
        order = list(range(n))
    if world_size > 1:
        total = -(-n // world_size) * world_size
        order = (order + order[: total - n])[rank::world_size]
    out = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    if drop_last and out and len(out[-1]) < batch_size:
        out.pop()
    return out


def fill_batch(indices, n, build):
    """The reference's refill (load_data.py:262-265, 288): an item its __getitem__ abandons is replaced by the item at the next index,
    (index + 1) % n, and so on, so the batch keeps its size.  build(list of item indices) -> (kept positions within that list, part)
    or None when every item was abandoned.  Rounds: every position still open is built again at its next index, after the round
    before it.  -> (parts [(batch positions, part)], the item index each position ended with)"""
    at = list(indices)
    open_ = list(range(len(at)))
    parts, rounds = [], 0
    while open_:
        if rounds > n:
            raise ValueError("fill_batch: every item was abandoned")
        got = build([at[p] for p in open_])
        kept = [] if got is None else [int(k) for k in got[0]]
        if kept:
            parts.append(([open_[k] for k in kept], got[1]))
        keep = set(kept)
        open_ = [p for k, p in enumerate(open_) if k not in keep]
        for p in open_:
            at[p] = (at[p] + 1) % n
        rounds += 1
    return parts, at


def _merge(parts, B):
    """the parts of fill_batch as one batch in position order"""
    if len(parts) == 1:
        return parts[0][1]
    pos = [p for ps, _ in parts for p in ps]
    order = np.argsort(np.asarray(pos))
    dbs = [db for _, db in parts]
    out = {}
    for k, v in dbs[0].items():
        if torch.is_tensor(v):
            cat = torch.cat([db[k] for db in dbs])
            out[k] = cat[torch.from_numpy(order).to(cat.device)].contiguous()
        elif isinstance(v, list):
            cat = [x for db in dbs for x in db[k]]
            out[k] = [cat[j] for j in order]
        else:
            out[k] = v
    assert len(pos) == B
    return out


class TrainBatches(object):
    """The training loop's batch source (the reference's DataLoader over PoseDataset, shuffle=True): ``items`` are host item dicts in
    train_batch's format (reading the files stays with the caller); each epoch draws an order (epoch_batches) and yields
    train_batch's device batches of ``batch_size`` items.

    * An item train_batch abandons is replaced by the next index's item (fill_batch), so a batch keeps batch_size items; the
      replacements' draws follow the batch's other draws.  'item_index' lists the item each row came from.
    * category_tables = (points (6,P,3), pdh1 (6,2500), pdh2 (6,2500)) -- the reference's obj_model/*.npy -- adds the batch's
      points_category / pdh1_category / pdh2_category, gathered by cat_id on the device.
    * persistence=True computes pdh1 / pdh2 with ops.persistence_images: the loop is then bounded by that kernel (about 440 ms per
      32-item batch on an MI355X against a ~16 ms step).
    * prefetch=True (a CUDA device): the iterator's ``prefetch()`` -- RL_TDA_train calls it after enqueuing a step -- makes the next
      batch's draws on the host and enqueues its kernels on a side stream, so they overlap the step; the next ``next()`` orders the
      current stream after them.  The draws happen in the same order as without prefetch (every draw of batch i+1 after every draw
      of step i), so the two loops are bit-identical.

    * dzi=True passes on train_batch's refusals: source_tables raises ValueError for a drawn window whose warp is not separable
      (rare; the affine map's rounding noise moves a tie), which ends the loop.
    * The epoch order comes from a generator of its own, seeded with ``seed + epoch`` (as DistributedSampler does): no augmentation
      draw, refill or subsample draw can move it, so under data parallel every rank computes the same order in every epoch and
      rank / world_size (default: torch.distributed's) give each rank its own slice of it.  seed=None draws the seed once, at
      construction, from ``gen`` (before any augmentation draw; ranks with alike-seeded generators agree); pass one seed to all
      ranks otherwise.  The epoch counts up at every iteration; set_epoch(e) sets it (a resumed run).
    * draws='device' (train_batch's mode of that name, seeded with ``seed``): a batch is built without a host read.  An item's key
      is epoch * len(items) + its index, so its rows depend on neither its batch, its slot, the batch size, prefetch nor the rank
      that builds it, and set_epoch reproduces them.  There is no refill: a batch is handed its own items plus ``spares`` more --
      the indices that follow it in this rank's epoch order, wrapping (they still appear in their own batch) -- and holds the first
      batch_size alive ones ('n_alive', 'status', 'item_index' as train_batch documents; -1 marks a slot without an item).
    * pcl_select='fps' (train_batch's option of that name): pcl_in by farthest point sampling; the batches then also carry PC and
      pcl_index.
    rng (NumPy) and gen (torch CPU generator; None: torch's default) feed train_batch."""

    def __init__(self, items, batch_size, rng=np.random, gen=None, device="cuda", prefetch=True, shuffle=True, drop_last=False,
                 persistence=False, dzi=False, roi_mask_pro=None, roi_mask_r=3, category_tables=None, min_points=50, operators=None,
                 img_size=256, rank=None, world_size=None, seed=None, draws="host", spares=0, pcl_select="random"):
        import torch.distributed as dist
        if not items:
            raise ValueError("TrainBatches: no items")
        self.items, self.batch_size = list(items), int(batch_size)
        self.rng, self.gen, self.device = rng, gen, torch.device(device)
        self.prefetch = bool(prefetch) and self.device.type == "cuda"
        self.shuffle, self.drop_last = shuffle, drop_last
        self.kw = dict(img_size=img_size, device=self.device, min_points=min_points, operators=operators, persistence=persistence,
                       roi_mask_pro=roi_mask_pro, roi_mask_r=roi_mask_r, dzi=dzi, pcl_select=pcl_select)
        if pcl_select not in ("random", "fps"):
            raise ValueError("TrainBatches: pcl_select must be 'random' or 'fps'")
        on = dist.is_available() and dist.is_initialized()
        self.world_size = int(world_size if world_size is not None else (dist.get_world_size() if on else 1))
        self.rank = int(rank if rank is not None else (dist.get_rank() if on else 0))
        self.tables = None
        if category_tables is not None:
            tabs = [torch.as_tensor(np.asarray(t, dtype=np.float32)) for t in category_tables]
            if len(tabs) != 3 or any(t.shape[0] != tabs[0].shape[0] for t in tabs):
                raise ValueError("category_tables: (points, pdh1, pdh2), one row per category")
            self.tables = [t.to(self.device) for t in tabs]
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()     # the side stream reads them from now on
        self._side = None
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_(generator=gen).item())
        self.seed, self.epoch = int(seed), 0
        if draws not in ("host", "device") or int(spares) < 0:
            raise ValueError("TrainBatches: draws must be 'host' or 'device' and spares >= 0")
        self.draws, self.spares = draws, int(spares)

    def __len__(self):
        n = -(-len(self.items) // self.world_size)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def build(self, indices):
        """one batch of the items at ``indices``, refilled, on the current stream"""
        n = len(self.items)

        def one(idx):
            try:
                db = train_batch([self.items[i] for i in idx], rng=self.rng, gen=self.gen, **self.kw)
            except ValueError as e:
                if "every item was abandoned" in str(e):
                    return None
                raise
            return db["item_index"].cpu().numpy(), db

        parts, at = fill_batch(indices, n, one)
        db = _merge(parts, len(indices))
        db["item_index"] = torch.as_tensor(np.asarray(at, dtype=np.int64)).to(self.device)
        return self._with_category_tables(db)

    def build_device(self, indices, spare_indices, epoch):
        """one draws='device' batch: the items at ``indices`` and their spares, on the current stream, nothing read back"""
        idx = list(indices) + list(spare_indices)
        n = len(self.items)
        db = train_batch([self.items[i] for i in idx], draws="device", seed=self.seed, keys=[int(epoch) * n + i for i in idx],
                         batch_size=len(indices), **self.kw)
        pos = db["item_index"]
        idx_t = _uploader(self.device)(np.asarray(idx, dtype=np.int64))
        db["item_index"] = torch.where(pos >= 0, idx_t[pos.clamp(min=0)], pos)
        return self._with_category_tables(db)

    def _with_category_tables(self, db):
        """adds the batch's points_category / pdh1_category / pdh2_category: the tables' rows at cat_id, gathered on the device"""
        if self.tables is not None:
            cid = db["cat_id"].reshape(-1).long()
            for k, t in zip(CATEGORY_KEYS, self.tables):
                db[k] = t.index_select(0, cid)
        return db

    def side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def order(self, epoch):
        """epoch ``epoch``'s batches of item indices for this rank (no draw from rng or gen)"""
        g = torch.Generator().manual_seed(self.seed + int(epoch))
        return epoch_batches(len(self.items), self.batch_size, g, self.shuffle, self.drop_last, self.rank, self.world_size)

    def __iter__(self):
        batches = self.order(self.epoch)
        self.epoch += 1
        return _EpochBatches(self, batches, self.epoch - 1)


class _EpochBatches(object):
    def __init__(self, src, batches, epoch=0):
        self.src, self.batches, self.at, self.ready, self.epoch = src, batches, 0, None, epoch
        self.flat = [i for b in batches for i in b]
        self.start = np.cumsum([0] + [len(b) for b in batches])

    def _build(self, j):
        if self.src.draws != "device":
            return self.src.build(self.batches[j])
        end = int(self.start[j + 1])
        spare = [self.flat[(end + q) % len(self.flat)] for q in range(self.src.spares)]
        return self.src.build_device(self.batches[j], spare, self.epoch)

    def __iter__(self):
        return self

    def prefetch(self):
        """build the next batch on the side stream now (a no-op without prefetch, at the epoch's end, or when one is ready)"""
        if not self.src.prefetch or self.ready is not None or self.at >= len(self.batches):
            return
        side = self.src.side_stream()
        with torch.cuda.stream(side):
            db = self._build(self.at)
            done = torch.cuda.Event()
            done.record(side)
        self.at += 1
        self.ready = (db, done)

    def __next__(self):
        if self.ready is not None:
            db, done = self.ready
            self.ready = None
            cur = torch.cuda.current_stream(self.src.device)
            cur.wait_event(done)
            for v in db.values():
                if torch.is_tensor(v):
                    v.record_stream(cur)            # allocated on the side stream, used and freed on this one
            return db
        if self.at >= len(self.batches):
            raise StopIteration
        db = self._build(self.at)
        self.at += 1
        return db
