"""Regenerates tests/golden/emd.npz from the REFERENCE's own ``losses/metrics/CD/fscore.py`` and the reconstruction statistics of
``evaluation/eval_utils_v1.py`` (compute_degree_cm_mAP with eval_recon=True, :1508-1543), both loaded by file path, unmodified, on
the CPU.  (The reference's EMD itself is a CUDA extension and cannot run: tests/emd_ref.py restates it.)

The reference computes the statistics into a local dict (``kind_result``) that it drops; a profile hook reads that local when the
function returns.  Nothing is copied from the reference: the fixture holds arrays only.

Stored:
  * fscore: dist1 (B,n), dist2 (B,m), the thresholds, and the reference's (fscore, precision_1, precision_2) per threshold; one row
    has no point below the threshold in either direction (the 0 / 0 case);
  * recon: the seed and image count of tests/util.synth_eval_results, the per-detection chamfer_dis_cass / emd_dis_cass given to it
    (concatenated over the images), and the reference's per-class means (NaN where a class has no detection) and their mean.

Usage:  python tests/golden/make_emd_golden.py REFERENCE_ROOT   (from the repo root)
"""
import importlib.util
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

SYNSET = ['BG', 'bottle', 'bowl', 'camera', 'can', 'laptop', 'mug']
RECON_SEED, RECON_IMAGES = 6, 16
GRIDS = (list(range(0, 61, 5)), [i / 2 for i in range(0, 21, 2)], [i / 100 for i in range(0, 101, 5)])


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recon_results():
    """the synthetic result list with a seeded Chamfer / EMD value per detection (shared with the tests)"""
    from tests.util import synth_eval_results
    res = synth_eval_results(RECON_SEED, RECON_IMAGES)
    rng = np.random.RandomState(RECON_SEED + 100)
    for r in res:
        P = len(r['pred_class_ids'])
        r["chamfer_dis_cass"] = rng.uniform(0.002, 0.03, P).astype(np.float32)
        r["emd_dis_cass"] = rng.uniform(0.005, 0.08, P).astype(np.float32)
    return res


def main():
    ref = os.path.abspath(sys.argv[1])
    fs = _load_by_path("ref_fscore", os.path.join(ref, "losses/metrics/CD/fscore.py"))
    rng = np.random.RandomState(3)
    dist1 = (rng.rand(5, 37) ** 2 * 4e-4).astype(np.float32)
    dist2 = (rng.rand(5, 50) ** 2 * 4e-4).astype(np.float32)
    dist1[2], dist2[2] = dist1[2] + 1.0, dist2[2] + 1.0          # nothing below any threshold: 0 / 0
    dist1[3] = dist1[3] + 1.0                                    # one direction empty
    thresholds = np.array([1e-4, 2.5e-5])
    arrays = dict(fs_dist1=dist1, fs_dist2=dist2, fs_thresholds=thresholds)
    for i, th in enumerate(thresholds):
        out = fs.fscore(torch.from_numpy(dist1), torch.from_numpy(dist2), float(th)) if i else \
            fs.fscore(torch.from_numpy(dist1), torch.from_numpy(dist2))                      # the default threshold
        arrays["fs_out%d" % i] = np.stack([o.numpy() for o in out])

    for m in ("cv2", "skimage", "skimage.color", "scipy.misc"):   # imported at module level, unused by this path
        sys.modules.setdefault(m, types.ModuleType(m))
    ev = _load_by_path("ref_eval_utils", os.path.join(ref, "evaluation/eval_utils_v1.py"))
    res = recon_results()
    seen = {}

    def hook(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "compute_degree_cm_mAP":
            seen.update(frame.f_locals["kind_result"])
    with tempfile.TemporaryDirectory() as tmp:
        sys.setprofile(hook)
        try:
            ev.compute_degree_cm_mAP(res, SYNSET, tmp, *GRIDS, iou_pose_thres=0.1, use_matches_for_pose=True, eval_recon=True,
                                     plot_figure=False)
        finally:
            sys.setprofile(None)
    for key in ("emd", "cmf"):
        arrays["recon_%s_class" % key] = np.array([seen[key].get(c, np.nan) for c in SYNSET], dtype=np.float64)
        arrays["recon_%s_mean" % key] = np.float64(seen[key]["mean"])
    arrays.update(recon_seed=np.int64(RECON_SEED), recon_images=np.int64(RECON_IMAGES),
                  recon_cmf=np.concatenate([r["chamfer_dis_cass"] for r in res]),
                  recon_emd=np.concatenate([r["emd_dis_cass"] for r in res]))
    np.savez_compressed(os.path.join(HERE, "emd.npz"), **arrays)
    print("wrote emd.npz", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
