"""Regenerates tests/golden/defor.npz from the REFERENCE's own defor_2D (datasets/data_augmentation.py:319-342) and training
PoseDataset.__getitem__ (datasets/load_data.py), on the CPU.

OpenCV is not installed: the ``cv2`` stand-in of make_augment_golden.py is extended with tests/morph_ref.py's
getStructuringElement / erode / dilate (a restatement of OpenCV, pinned to scipy.ndimage by tests/test_defor_cpu.py).

Two parts:
  * masks: defor_2D on a dozen 256x256 masks at rand_pro 0, 0.5, 1, each from a seeded np.random; recorded: the mask, the
    output, the seed, NumPy's state afterwards;
  * getitem: __getitem__ with roi_mask_pro 1.0 / 0.5, augmentation on, DZI 'uniform' or off, over the synthetic frames of
    tests/util.py; recorded for the FIRST attempt of each item: the entry seed, the window and NumPy's state after aug_bbox_DZI, the
    attempt's outcome (0 kept, 1 abandoned by the validity tests, 2 IndexError, 3 fewer than 50 points, 4 ValueError), the undeformed
    and deformed masks' sizes, and for a kept item NumPy's state at generate_aug_parameters, the cut cloud base_aug receives, the
    labels base_aug receives, the operator (with the spies of make_augment_golden.py) and the outputs pcl_in, aug_pcl_in (not for an
    applied crop / cutout, whose shuffle this project draws later), rotation, translation, fsnet_scale.

Usage:  python tests/golden/make_defor_golden.py REFERENCE_ROOT   (from the repo root)
"""
import importlib.util
import os
import pickle
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mag = _load_by_path("make_augment_golden", os.path.join(HERE, "make_augment_golden.py"))      # checks argv, sets sys.path
REF = mag.REF
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import morph_ref  # noqa: E402


def masks():
    S = 256
    yy, xx = np.mgrid[0:S, 0:S]
    out = {}
    out["blob"] = ((yy - 120) ** 2 / 40.0 ** 2 + (xx - 131) ** 2 / 55.0 ** 2 <= 1)
    r2 = (yy - 128) ** 2 + (xx - 128) ** 2
    out["ring"] = (r2 <= 70 ** 2) & (r2 >= 45 ** 2)
    out["line"] = np.zeros((S, S), bool)
    out["line"][100, 20:230] = True
    out["diagonal"] = np.eye(S, dtype=bool) | np.eye(S, k=1, dtype=bool)
    out["checker"] = np.zeros((S, S), bool)
    out["checker"][60:92, 70:102] = ((yy[60:92, 70:102] + xx[60:92, 70:102]) % 2) == 0
    out["top_left"] = (yy < 40) & (xx < 60)
    out["bottom_right"] = (yy > 200) & (xx > 180)
    out["rows_0_255"] = (xx > 100) & (xx < 140)
    out["cols_0_255"] = (yy > 30) & (yy < 50) | (xx == 0) | (xx == 255)
    out["single"] = (yy == 77) & (xx == 190)
    out["empty"] = np.zeros((S, S), bool)
    out["full"] = np.ones((S, S), bool)
    return out


def record_masks(rda, arrays):
    names = []
    n = 0
    for name, m in masks().items():
        for pro in (0.0, 0.5, 1.0):
            seed = 1000 + n
            np.random.seed(seed)
            res = rda.defor_2D(m.astype(np.float32)[None], rand_r=3, rand_pro=pro)
            st = np.random.get_state()
            pre = "m.%d." % n
            arrays[pre + "mask"] = np.packbits(m)
            arrays[pre + "out"] = np.packbits(res > 0)
            assert set(np.unique(res)) <= {0.0, 1.0} and res.shape == m.shape
            arrays[pre + "pro"], arrays[pre + "seed"] = np.float64(pro), np.int64(seed)
            mag.np_state_arrays(pre + "after", st, arrays)
            names.append(name)
            n += 1
    arrays["m.names"] = np.array(names)


class _Retry(Exception):
    pass


# (scene seed, detection, class id 1..6, DZI type, roi_mask_pro, seed, variant): variant None = the frame as drawn; "absent" = the
# label names an instance id the mask does not hold (the validity tests abandon the item); "tiny:k" = only the instance's first k
# pixels in row-major order stay in the mask (a cloud under 26 points after the deformation)
ITEMS = [(41, 0, 2, "uniform", 1.0, 3, None), (41, 1, 6, "none", 1.0, 4, None), (42, 0, 1, "uniform", 0.5, 5, None),
         (42, 2, 3, "none", 0.5, 6, None), (43, 1, 4, "uniform", 1.0, 7, None), (45, 1, 1, "uniform", 0.5, 11, None),
         (45, 0, 3, "none", 1.0, 12, None), (46, 2, 2, "uniform", 1.0, 13, None), (44, 3, 5, "uniform", 1.0, 21, None),
         (47, 1, 1, "none", 1.0, 22, None), (43, 0, 2, "uniform", 1.0, 23, "absent"), (42, 1, 4, "none", 1.0, 24, "tiny:2")]
OUTCOMES = {0: "kept", 1: "validity tests", 2: "IndexError", 3: "fewer than 50 points", 4: "ValueError (no point left)"}


def item_mask(fr, j, variant):
    inst_mask = np.zeros(fr["depth"].shape, np.uint8)
    for q in range(4):
        inst_mask[fr["pred_masks"][:, :, q]] = q + 1
    if variant and variant.startswith("tiny:"):
        k = int(variant[5:])
        ys, xs = np.nonzero(inst_mask == j + 1)
        inst_mask[inst_mask == j + 1] = 0
        inst_mask[ys[:k], xs[:k]] = j + 1
    return inst_mask


def record_getitem(ld, F, arrays):
    from tests.util import synth_depth_scene
    F.train = 1
    F.aug_pc_pro, F.aug_pc_r, F.aug_rt_pro, F.aug_bb_pro, F.aug_bc_pro = 0.2, 0.2, 0.3, 0.3, 0.3
    cap = {}
    real_dzi, real_defor = ld.aug_bbox_DZI, ld.defor_2D

    def dzi_spy(flags_, bbox_xyxy, im_H, im_W):
        if "window" in cap:
            raise _Retry()                        # a second attempt: the first one was abandoned
        c, sc = real_dzi(flags_, bbox_xyxy, im_H, im_W)
        cap["window"] = np.array([c[0], c[1], sc], np.float64)
        cap["np_dzi"] = np.random.get_state()
        return c, sc

    def defor_spy(roi_mask, rand_r=2, rand_pro=0.3):
        r = real_defor(roi_mask, rand_r=rand_r, rand_pro=rand_pro)
        cap["n_mask"], cap["n_def"] = int((roi_mask > 0).sum()), int((r > 0).sum())
        return r
    ld.aug_bbox_DZI, ld.defor_2D = dzi_spy, defor_spy
    arrays["gi.n_items"] = np.int64(len(ITEMS))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Real", "train", "scene_1"))
        try:
            os.chdir(REF)
            for n, (sseed, j, cls, dzi, pro, seed, variant) in enumerate(ITEMS):
                fr = synth_depth_scene(sseed, 4)
                inst_mask = item_mask(fr, j, variant)
                stem = os.path.join("Real", "train", "scene_1", "%04d" % n)
                inst = 9 if variant == "absent" else j + 1
                with open(os.path.join(tmp, stem + "_label.pkl"), "wb") as f:
                    pickle.dump(dict(class_ids=[cls], instance_ids=[inst], bboxes=[fr["pred_bboxes"][j]], model_list=["m0"], scales=[0.3],
                                     rotations=[mag.rot(seed)], translations=[np.array([0.01, -0.02, 0.8], np.float32)]), f)
                np.save(os.path.join(tmp, stem + "_color.png.npy"), np.zeros(fr["depth"].shape + (3,), np.uint8))
                np.save(os.path.join(tmp, stem + "_depth.png.npy"), fr["depth"])
                open(os.path.join(tmp, stem + "_depth.png"), "wb").close()
                np.save(os.path.join(tmp, stem + "_mask.png.npy"), np.repeat(inst_mask[:, :, None], 3, axis=2))
                ds = ld.PoseDataset.__new__(ld.PoseDataset)
                ds.source, ds.mode, ds.data_dir, ds.per_obj, ds.per_obj_id = "Real", "train", tmp, "", None
                ds.img_list, ds.length, ds.invaild_list = [stem], 1, []
                ds.camera_intrinsics = np.array([[577.5, 0, 319.5], [0, 577.5, 239.5], [0, 0, 1]], dtype=np.float32)
                ds.real_intrinsics = np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]], dtype=np.float32)
                ds.cat_names = ['bottle', 'bowl', 'camera', 'can', 'laptop', 'mug']
                ds.id2cat_name = {'1': 'bottle', '2': 'bowl', '3': 'camera', '4': 'can', '5': 'laptop', '6': 'mug'}
                ds.models = {"m0": np.random.RandomState(1).rand(64, 3).astype(np.float32) - 0.5}
                ds.mug_sym = {"scene_1_res": {n: n % 2}}
                ds.base_aug = ld.PC_BasicAugment()
                ds.operator_name = ['Jitter', 'RandomCutout', 'RandomCrop', 'RandomDropout']
                ds.custom_aug_operator = [ld.PcJitter(std=0.005, clip=0.05, p=0.6), ld.PcRandomCutout(p=0.9, min_num_points=1024),
                                          ld.PcRandomCrop(p=0.9, min_num_points=1024), ld.PcRandomDropout(p=0.9, max_dropout_ratio=0.5)]
                F.DZI_TYPE, F.roi_mask_pro, F.roi_mask_r = dzi, pro, 3
                real_gap, real_base = ds.generate_aug_parameters, ds.base_aug

                def gap_spy(*a, _r=real_gap, **kw):
                    cap["np_gap"] = np.random.get_state()
                    return _r(*a, **kw)

                def base_spy(db, _r=real_base):
                    cap["torch_base"] = torch.get_rng_state().numpy()
                    cap["db"] = {k: v.clone() for k, v in db.items()}
                    return _r(db)
                ds.generate_aug_parameters, ds.base_aug = gap_spy, base_spy
                wrapped = []
                for q, o in enumerate(ds.custom_aug_operator):
                    def op_spy(pts, _o=o, _q=q):
                        cap["op"], cap["op_in"] = _q, pts.numpy().copy()
                        del mag.LOG[:]
                        r = _o(pts)
                        cap["op_log"], cap["op_out_n"] = list(mag.LOG), int(r.shape[0])
                        return r
                    wrapped.append(op_spy)
                ds.custom_aug_operator = wrapped
                cap.clear()
                np.random.seed(seed)
                torch.manual_seed(seed)
                import random as _random
                _random.seed(seed)
                outcome, data = 0, None
                try:
                    data = ds[0]
                except _Retry:
                    outcome = 3 if "n_def" in cap else 1
                except IndexError:
                    outcome = 2
                except ValueError:
                    outcome = 4
                pre = "gi.%d." % n
                arrays[pre + "scene"], arrays[pre + "det"], arrays[pre + "cls"] = np.int64(sseed), np.int64(j), np.int64(cls)
                arrays[pre + "inst"], arrays[pre + "variant"] = np.int64(inst), np.array(variant or "")
                arrays[pre + "dzi"], arrays[pre + "pro"], arrays[pre + "seed"] = np.array(dzi), np.float64(pro), np.int64(seed)
                arrays[pre + "window"] = cap["window"]
                mag.np_state_arrays(pre + "np_dzi", cap["np_dzi"], arrays)
                arrays[pre + "outcome"] = np.int64(outcome)
                arrays[pre + "n_mask"] = np.int64(cap.get("n_mask", -1))
                arrays[pre + "n_def"] = np.int64(cap.get("n_def", -1))
                if outcome == 0:
                    mag.np_state_arrays(pre + "np_gap", cap["np_gap"], arrays)
                    mag.seeded(pre + "torch_base", seed, torch_state=cap["torch_base"], out=arrays)   # no torch draw before base_aug
                    arrays[pre + "cut"] = cap["cut"] = cap["db"]["pcl_in"].numpy()
                    for k in ("rotation", "translation", "fsnet_scale", "mean_shape", "sym_info", "model_point", "nocs_scale", "cat_id"):
                        arrays[pre + "in." + k] = cap["db"][k].numpy()
                    op = ds.operator_name[cap["op"]]
                    applied = cap["op_log"][0][2][0] <= mag.ds_p(op)
                    arrays[pre + "op"], arrays[pre + "op_applied"], arrays[pre + "M"] = np.int64(cap["op"]), np.int64(applied), \
                        np.int64(cap["op_out_n"])
                    crop_cut = op in ("RandomCrop", "RandomCutout") and applied
                    # M is compared where the chosen box has no point within 1e-5 of a face (the kernel's fp32 box test)
                    arrays[pre + "M_pinned"] = np.int64(not crop_cut or cap["op_out_n"] == 2048
                                                        or mag.box_faces_clear(cap["op_in"], cap["op_log"], op))
                    for k in ("pcl_in", "aug_pcl_in", "rotation", "translation", "fsnet_scale"):
                        if k == "aug_pcl_in" and crop_cut:
                            continue          # shuffled after the up-front attempts here: compared through M only
                        arrays[pre + "out." + k] = data[k].numpy()
                print("item %2d dzi %-7s pro %.1f %-26s mask %5d -> %5d cut %s" % (n, dzi, pro, OUTCOMES[outcome], cap.get("n_mask", -1),
                                                                               cap.get("n_def", -1), cap["cut"].shape if outcome == 0 else "-"))
        finally:
            os.chdir(cwd)


def record_dzi(ld, F, arrays):
    """the reference's aug_bbox_DZI on its own, as load_data.py:233-238 calls it, for the three kinds it implements"""
    from tests.util import synth_depth_scene
    n = 0
    for kind in ("uniform", "roi10d", "none"):
        for sseed in (41, 44, 47):
            fr = synth_depth_scene(sseed, 4)
            H, W = fr["depth"].shape
            for j in range(4):
                F.DZI_TYPE = kind
                rmin, rmax, cmin, cmax = ld.get_bbox(fr["pred_bboxes"][j])
                np.random.seed(500 + n)
                c, sc = ld.aug_bbox_DZI(F, np.array([cmin, rmin, cmax, rmax]), H, W)
                pre = "dzi.%d." % n
                arrays[pre + "kind"], arrays[pre + "scene"], arrays[pre + "det"] = np.array(kind), np.int64(sseed), np.int64(j)
                arrays[pre + "seed"], arrays[pre + "window"] = np.int64(500 + n), np.array([c[0], c[1], sc], np.float64)
                mag.np_state_arrays(pre + "after", np.random.get_state(), arrays)
                n += 1
    arrays["dzi.n"] = np.int64(n)
    arrays["dzi.flags"] = np.array([F.DZI_PAD_SCALE, F.DZI_SCALE_RATIO, F.DZI_SHIFT_RATIO], np.float64)


def main():
    mag.stand_ins()
    cv2 = sys.modules["cv2"]
    cv2.MORPH_ELLIPSE = morph_ref.MORPH_ELLIPSE
    cv2.getStructuringElement, cv2.erode, cv2.dilate = morph_ref.getStructuringElement, morph_ref.erode, morph_ref.dilate
    importlib.import_module("config.config")
    import absl.flags as flags
    F = flags.FLAGS
    rda = _load_by_path("ref_data_augmentation", os.path.join(REF, "datasets/data_augmentation.py"))
    sys.modules["datasets.data_augmentation"] = rda
    ld = _load_by_path("ref_load_data_defor", os.path.join(REF, "datasets/load_data.py"))
    for m in (rda, ld):
        m.np = mag._NpSpy("np")                         # logs the operators' draws (make_augment_golden.py); values pass through
    rda.torch = mag._TorchSpy("torch")
    arrays = {}
    record_masks(rda, arrays)
    record_dzi(ld, F, arrays)
    record_getitem(ld, F, arrays)
    path = os.path.join(HERE, "defor.npz")
    np.savez_compressed(path, **arrays)
    print("wrote defor.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
