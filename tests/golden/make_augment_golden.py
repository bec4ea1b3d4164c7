"""Regenerates tests/golden/augment.npz from the REFERENCE's own training augmentation (datasets/data_augmentation.py and
datasets/load_data.py, loaded unmodified), on the CPU.

Two parts:
  * direct: PC_BasicAugment, PcJitter / PcRandomCutout / PcRandomCrop / PcRandomDropout and pc_sampler run on chosen clouds;
  * getitem: the reference's training PoseDataset.__getitem__ with augmentation on (FLAGS as config/config.py sets them, except
    roi_mask_pro = 0: defor_2D's erode / dilate needs OpenCV), over the synthetic frames of tests/util.py.
Stand-ins as for make_golden.gen_train_loader: ``cv2`` (imread from .npy twins; warpAffine / getAffineTransform from
oracle/input_ref.py), ``mmengine`` (load = pickle.load), ``tools.eval_utils`` (the source twin network/point_sample/
pc_sample_sphere.py), ``datasets.compute_pd`` (zeros).  The modules' ``np.random`` and ``torch.rand`` are wrapped by spies that log
what the reference consumed; nothing else is changed.

Stored per case: NumPy's and torch's generator states at the stage boundaries (the tests replay the large draws from them: defor,
the jitter's normal_, dropout's uniforms, the permutations) -- as the seed where the state is the one seeding leaves (checked here) --,
the scalar draws consumed, the inputs and outputs.  Outputs that are selections of their input's rows (crop, cutout, dropout,
pc_sampler) are stored as row numbers; the view cases share three input clouds.

Usage:  python tests/golden/make_augment_golden.py REFERENCE_ROOT   (from the repo root; or set $TGP_REFERENCE)
"""
import importlib.util
import json
import os
import pickle
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TGP_REFERENCE", ""))
if not os.path.isdir(os.path.join(REF, "datasets")):
    sys.exit("usage: make_augment_golden.py REFERENCE_ROOT")
sys.path[:0] = [os.path.join(HERE, "_absl_shim"), REF]
sys.path.append(ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stand_ins():
    from oracle import input_ref as ir
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.INTER_LINEAR = 0, 1
    cv2.getAffineTransform = lambda src, dst: ir.get_affine_transform_cv(src, dst)

    def warp_affine(img, M, dsize, flags=1):
        assert flags == cv2.INTER_NEAREST
        return ir.warp_affine_nearest(img, M, dsize)

    def imread(path, flag=1):
        return np.load(path + ".npy") if os.path.exists(path + ".npy") else None
    cv2.warpAffine, cv2.imread = warp_affine, imread
    sys.modules["cv2"] = cv2
    mm = types.ModuleType("mmengine")
    mm.load = lambda path: pickle.load(open(path, "rb"))
    sys.modules["mmengine"] = mm
    twin = _load_by_path("ref_pc_sample_sphere", os.path.join(REF, "network/point_sample/pc_sample_sphere.py"))
    eu = types.ModuleType("tools.eval_utils")
    eu.load_depth, eu.get_bbox = twin.load_depth, twin.get_bbox
    sys.modules["tools.eval_utils"] = eu
    import datasets as ref_datasets
    assert ref_datasets.__file__.startswith(REF), ref_datasets.__file__
    cpd = types.ModuleType("datasets.compute_pd")
    cpd.compute_pd = lambda pts: (torch.zeros(2500), torch.zeros(2500))
    sys.modules["datasets.compute_pd"] = cpd


LOG = []          # (source, name, values) of every draw the spied modules make


class _NpRandomSpy(object):
    def __getattr__(self, k):
        f = getattr(np.random, k)
        if not callable(f):
            return f

        def call(*a, **kw):
            r = f(*a, **kw)
            v = np.asarray(a[0] if k == "shuffle" else r, dtype=np.float64).ravel()
            LOG.append(("np", k, v.copy() if v.size <= 8 else np.array([v.size], np.float64)))
            return r
        return call


class _NpSpy(types.ModuleType):
    random = _NpRandomSpy()

    def __getattr__(self, k):
        return getattr(np, k)


class _TorchSpy(types.ModuleType):
    def rand(self, *a, **kw):
        r = torch.rand(*a, **kw)
        v = r.detach().cpu().double().reshape(-1)
        LOG.append(("torch", "rand", v.numpy().copy() if v.numel() <= 8 else np.array([v.numel()], np.float64)))
        return r

    def __getattr__(self, k):
        return getattr(torch, k)


def seeded(prefix, seed, np_state=None, torch_state=None, out=None):
    """A generator state that is the state right after seeding is stored as its seed: check that it is, record the seed."""
    if np_state is not None:
        ref = np.random.RandomState(seed).get_state()
        assert np.array_equal(ref[1], np_state[1]) and ref[2:] == np_state[2:], prefix
    if torch_state is not None:
        assert np.array_equal(torch.Generator().manual_seed(seed).get_state().numpy(), np.asarray(torch_state)), prefix
    out[prefix + ".seed"] = np.int64(seed)


def np_state_arrays(prefix, st, out):
    out[prefix + ".keys"] = np.asarray(st[1], dtype=np.uint32)
    out[prefix + ".pos"] = np.array([st[2], st[3]], dtype=np.int64)
    out[prefix + ".gauss"] = np.float64(st[4])


def log_values(entries):
    """the scalar draws of a log slice, flattened (shuffles and large arrays as their size)"""
    return np.concatenate([e[2] for e in entries]) if entries else np.zeros(0)


def rot(seed):
    q = np.random.RandomState(seed).randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------- direct
# (name, seed, cat_id (0-based), sym0, pros (bb, rt, bc, pc)): 1.0 forces a stage on, 0.0 off; None = the config's probabilities
BASE_CASES = [("all_off", 1, 1, 1, (0.0, 0.0, 0.0, 0.0)), ("all_on_bowl_sym", 2, 1, 1, (1.0, 1.0, 1.0, 1.0)),
              ("all_on_mug", 3, 5, 0, (1.0, 1.0, 1.0, 1.0)), ("all_on_camera_bc_skipped", 4, 2, 0, (1.0, 1.0, 1.0, 1.0)),
              ("bb_sym", 5, 0, 1, (1.0, 0.0, 0.0, 0.0)), ("bb_nosym", 6, 2, 0, (1.0, 0.0, 0.0, 0.0)), ("rt", 7, 3, 1, (0.0, 1.0, 0.0, 0.0)),
              ("bc_mug", 8, 5, 0, (0.0, 0.0, 1.0, 0.0)), ("bc_bowl", 9, 1, 1, (0.0, 0.0, 1.0, 0.0)), ("pc", 10, 4, 0, (0.0, 0.0, 0.0, 1.0)),
              ("bb_bc_bowl", 11, 1, 1, (1.0, 0.0, 1.0, 0.0)), ("config_a", 12, 5, 0, None), ("config_b", 13, 1, 1, None)]
CONFIG_PRO = (0.3, 0.3, 0.3, 0.2)


def base_inputs(seed, cat, sym0, N=256, Nm=128):
    r = np.random.RandomState(100 + seed)
    ms = np.array([0.165, 0.08, 0.165], np.float32) * (0.5 + r.rand(3)).astype(np.float32)
    s = (r.rand(3).astype(np.float32) - 0.5) * np.float32(0.02)
    R, t = rot(seed), np.array([0.05, -0.03, 0.8], np.float32) + (r.rand(3).astype(np.float32) - 0.5) * np.float32(0.1)
    mp = ((r.rand(Nm, 3) - 0.5) * (ms + s) / np.linalg.norm(ms + s)).astype(np.float32)
    pc = ((r.rand(N, 3) - 0.5) * (ms + s)) @ R.T + t
    rda_bb, rda_t, rda_R = (np.array([0.8, 0.8, 0.8]) + 0.4 * r.rand(3)).astype(np.float32), \
        ((r.rand(3) - 0.5) * 0.1).astype(np.float32), rot(1000 + seed)
    sym = np.array([sym0, 1, 0, 1], np.float32)
    return dict(pcl_in=pc.astype(np.float32), rotation=R, translation=t, fsnet_scale=s, mean_shape=ms, sym_info=sym, aug_bb=rda_bb,
                aug_rt_t=rda_t, aug_rt_R=rda_R, model_point=mp, nocs_scale=np.float32(0.2 + 0.2 * r.rand()), cat_id=np.float32(cat))


def record_base(rda, F, out):
    names = []
    for k, (name, seed, cat, sym0, pros) in enumerate(BASE_CASES):
        names.append(name)
        inp = base_inputs(seed, cat, sym0)
        pro = CONFIG_PRO if pros is None else pros
        F.aug_bb_pro, F.aug_rt_pro, F.aug_bc_pro, F.aug_pc_pro, F.aug_pc_r = pro[0], pro[1], pro[2], pro[3], 0.2
        torch.manual_seed(500 + seed)
        seeded("base.%d.torch" % k, 500 + seed, torch_state=torch.get_rng_state().numpy(), out=out)
        db = {kk: torch.as_tensor(v, dtype=torch.float32) for kk, v in inp.items()}
        del LOG[:]
        PC, R, t, s = rda.PC_BasicAugment()(db)
        draws = log_values([e for e in LOG if e[0] == "torch"][:6])
        assert draws.size == 6 and [e[2][0] for e in LOG if e[0] == "torch"][6] == inp["pcl_in"].size, LOG
        for kk, v in inp.items():
            out["base.%d.in.%s" % (k, kk)] = np.asarray(v)
        out["base.%d.pro" % k] = np.array(list(pro) + [0.2], np.float64)
        out["base.%d.draws" % k] = draws.astype(np.float32)
        out["base.%d.out.pc" % k] = PC[0].numpy()
        out["base.%d.out.R" % k], out["base.%d.out.t" % k], out["base.%d.out.s" % k] = R[0].numpy(), t[0].numpy(), s[0].numpy()
        lt = lambda u, p: bool((torch.tensor(u, dtype=torch.float32) < p).item())
        flags = [lt(draws[0], pro[0]), lt(draws[1], pro[1]), lt(draws[2], pro[2]) and cat in (1, 5), lt(draws[5], pro[3])]
        out["base.%d.flags" % k] = np.array(flags, np.int32)
        print("base %-26s flags %s" % (name, flags))
    out["base.names"] = np.array(names)


def object_cloud(seed, n=2048):
    """a 2048-point cloud shaped like a cut object view (a noisy half shell), on a 2^-16 m grid (the fixture compresses)"""
    r = np.random.RandomState(seed)
    th, ph = r.rand(n) * np.pi, r.rand(n) * np.pi
    xyz = np.stack([np.cos(th) * np.sin(ph), np.cos(ph), np.sin(th) * np.sin(ph)], 1) * np.array([0.08, 0.05, 0.07])
    xyz = xyz + r.randn(n, 3) * 0.003 + np.array([0.02, -0.05, 0.75])
    return (np.round(xyz * 65536.0) / 65536.0).astype(np.float32)


# the view cases' input clouds: two object views and a degenerate cloud (every point the same)
VIEW_CLOUDS = [object_cloud(21), object_cloud(22), np.tile(object_cloud(1)[:1], (2048, 1))]


def as_rows(src, dst):
    """dst as row numbers of src when every row of dst is, bit for bit, a row of src (int16), else None"""
    first = {}
    for i, row in enumerate(src):
        first.setdefault(row.tobytes(), i)
    rows = [first.get(row.tobytes()) for row in dst]
    if any(r is None for r in rows):
        return None
    rows = np.asarray(rows, dtype=np.int16)
    assert np.array_equal(src[rows].view(np.uint32), dst.view(np.uint32))
    return rows


# (name, operator, constructor kwargs, cloud: "degenerate" or an object view, want) -- want: what the case must show (checked below)
VIEW_CASES = [
    ("jitter_applied", "PcJitter", dict(std=0.005, clip=0.05, p=0.6), 21, "applied"),
    ("jitter_skipped", "PcJitter", dict(std=0.005, clip=0.05, p=0.6), 22, "skipped"),
    ("jitter_default", "PcJitter", dict(), 23, "applied"),
    ("dropout_applied", "PcRandomDropout", dict(p=0.9, max_dropout_ratio=0.5), 24, "applied"),
    ("dropout_skipped", "PcRandomDropout", dict(p=0.9, max_dropout_ratio=0.5), 25, "skipped"),
    ("crop_first", "PcRandomCrop", dict(p=0.9, min_num_points=1024), 26, "first"),
    ("crop_later", "PcRandomCrop", dict(p=0.9, min_num_points=1024), 27, "later"),
    ("crop_skipped", "PcRandomCrop", dict(p=0.9, min_num_points=1024), 28, "skipped"),
    ("crop_exhausted", "PcRandomCrop", dict(), 29, "exhausted"),
    ("crop_degenerate", "PcRandomCrop", dict(p=0.9, min_num_points=1024), "degenerate", "exhausted"),
    ("cutout_first", "PcRandomCutout", dict(p=0.9, min_num_points=1024), 30, "first"),
    ("cutout_later", "PcRandomCutout", dict(p=0.9, min_num_points=1500), 31, "later"),
    ("cutout_skipped", "PcRandomCutout", dict(p=0.9, min_num_points=1024), 32, "skipped"),
    ("cutout_exhausted", "PcRandomCutout", dict(), 33, "exhausted"),
    ("cutout_degenerate", "PcRandomCutout", dict(p=0.9, min_num_points=1024), "degenerate", "exhausted"),
]


def outcome(name, entries, n_in, n_out, p):
    """what the logged draws say the operator did"""
    if entries[0][2][0] > p:
        return "skipped"
    if name in ("PcJitter", "PcRandomDropout"):
        return "applied"
    per = 3 if name == "PcRandomCrop" else 2
    tries = (len(entries) - 1) // per
    if n_out == n_in:
        assert tries == 11
        return "exhausted"
    return "first" if tries == 1 else "later"


def record_view(rda, out):
    names = []
    for k, (name, op, kw, cloud, want) in enumerate(VIEW_CASES):
        names.append(name)
        cls = getattr(rda, op)
        inst = cls(**kw)
        ci = 2 if cloud == "degenerate" else k % 2
        pts = VIEW_CLOUDS[ci]
        got = None
        for seed in range(1000 + k * 10000, 1000 + k * 10000 + 5000):         # the first seed that shows the case
            np.random.seed(seed)
            torch.manual_seed(seed)
            st_np, st_t = np.random.get_state(), torch.get_rng_state().numpy()
            del LOG[:]
            res = inst(torch.from_numpy(pts.copy()))
            ent = list(LOG)
            st_s = np.random.get_state()
            del LOG[:]
            samp = rda.pc_sampler(res, 1024)
            if outcome(op, ent, 2048, res.shape[0], inst.p) == want:
                got = (seed, st_np, st_t, ent, res.numpy(), st_s, samp.numpy())
                break
        assert got is not None, name
        seed, st_np, st_t, ent, res, st_s, samp = got
        seeded("view.%d.np" % k, seed, np_state=st_np, out=out)
        np_state_arrays("view.%d.np_sampler" % k, st_s, out)
        if op == "PcJitter":
            seeded("view.%d.torch" % k, seed, torch_state=st_t, out=out)
        out["view.%d.op" % k] = np.array(op)
        out["view.%d.kw" % k] = np.array(json.dumps(kw))
        # the input as an index into view.clouds; the output as row numbers of the input where it is a selection of them (crop,
        # cutout, dropout, a skipped operator), else in full (jitter); pc_sampler's result as row numbers of the output
        out["view.%d.cloud" % k] = np.int64(ci)
        rows = as_rows(pts, res)
        if rows is None:
            out["view.%d.out" % k] = res
        else:
            out["view.%d.out_rows" % k] = rows
        out["view.%d.sampled_rows" % k] = as_rows(res, samp)
        out["view.%d.draws" % k] = log_values(ent)
        out["view.%d.n_draw_calls" % k] = np.int64(len(ent))
        print("view %-18s seed %5d  M %4d  draw calls %d" % (name, seed, res.shape[0], len(ent)))
    out["view.names"] = np.array(names)
    out["view.clouds"] = np.stack(VIEW_CLOUDS)


# ------------------------------------------------------------------------------------------------------------------ getitem
# (scene seed, detection, class id 1..6, DZI type, seed)
ITEMS = [(41, 0, 2, "uniform", 3), (41, 1, 6, "uniform", 4), (42, 0, 1, "none", 5), (42, 2, 3, "uniform", 6), (43, 1, 4, "uniform", 7),
         (45, 1, 1, "uniform", 11), (45, 0, 3, "uniform", 12), (46, 2, 2, "none", 13)]


def box_faces_clear(pts, entries, op):
    """the chosen crop / cutout box (replayed from the logged draws) has no point within 1e-5 of a face"""
    per = 3 if op == "RandomCrop" else 2
    vals = [e[2] for e in entries[1:]]
    tries = len(vals) // per
    cmin, cmax = pts.min(0), pts.max(0)
    diff = cmax - cmin
    t = tries - 1
    if op == "RandomCrop":
        r0, ar, lo = vals[3 * t][0], vals[3 * t + 1][0], vals[3 * t + 2]
        rg = np.array([r0, r0 * ar, r0 / ar])
    else:
        rg, lo = vals[2 * t], vals[2 * t + 1]
    faces = np.concatenate([cmin + diff * lo, cmin + diff * (lo + rg)])
    d = np.abs(pts.astype(np.float64)[:, [0, 1, 2, 0, 1, 2]] - faces[None, :]).min()
    return d > 1e-5


def record_getitem(ld, F, out):
    from tests.util import synth_depth_scene
    F.train, F.roi_mask_pro = 1, 0.0
    F.aug_pc_pro, F.aug_pc_r, F.aug_rt_pro, F.aug_bb_pro, F.aug_bc_pro = 0.2, 0.2, 0.3, 0.3, 0.3
    windows, cap = [], {}
    real_dzi = ld.aug_bbox_DZI

    def dzi_spy(flags_, bbox_xyxy, im_H, im_W):
        c, sc = real_dzi(flags_, bbox_xyxy, im_H, im_W)
        windows.append((np.asarray(c, dtype=np.float64).copy(), float(sc)))
        return c, sc
    ld.aug_bbox_DZI = dzi_spy
    out["gi.n_items"] = np.int64(len(ITEMS))
    out["gi.scene_dets"] = np.int64(4)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Real", "train", "scene_1"))
        try:
            os.chdir(REF)                                  # __getitem__ reads ./obj_model/points_{cat}.npy
            for n, (sseed, j, cls, dzi, seed) in enumerate(ITEMS):
                fr = synth_depth_scene(sseed, 4)
                inst_mask = np.zeros(fr["depth"].shape, np.uint8)
                for q in range(4):
                    inst_mask[fr["pred_masks"][:, :, q]] = q + 1
                stem = os.path.join("Real", "train", "scene_1", "%04d" % n)
                with open(os.path.join(tmp, stem + "_label.pkl"), "wb") as f:
                    pickle.dump(dict(class_ids=[cls], instance_ids=[j + 1], bboxes=[fr["pred_bboxes"][j]], model_list=["m0"], scales=[0.3],
                                     rotations=[rot(seed)], translations=[np.array([0.01, -0.02, 0.8], np.float32)]), f)
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
                F.DZI_TYPE = dzi
                cap.clear()
                real_gap, real_base = ds.generate_aug_parameters, ds.base_aug

                def gap_spy(*a, _r=real_gap, **kw):
                    cap["np_gap"] = np.random.get_state()
                    cap["gap"] = _r(*a, **kw)
                    return cap["gap"]

                def base_spy(db, _r=real_base):
                    cap["torch_base"] = torch.get_rng_state().numpy()
                    cap["db"] = {k: v.clone() for k, v in db.items()}
                    del LOG[:]
                    res = _r(db)
                    cap["base_log"] = list(LOG)
                    return res
                ds.generate_aug_parameters, ds.base_aug = gap_spy, base_spy
                wrapped = []
                for q, o in enumerate(ds.custom_aug_operator):
                    def op_spy(pts, _o=o, _q=q):
                        cap["op"] = _q
                        cap["op_in"] = pts.numpy().copy()
                        cap["np_op"] = np.random.get_state()
                        del LOG[:]
                        r = _o(pts)
                        cap["op_log"] = list(LOG)
                        cap["op_out_n"] = int(r.shape[0])
                        return r
                    wrapped.append(op_spy)
                ds.custom_aug_operator = wrapped
                import random as _random
                for s_ in range(seed, seed + 20000, 1000):      # the item's seed, or the next one whose chosen box has clear faces
                    del windows[:]
                    np.random.seed(s_)
                    torch.manual_seed(s_)
                    _random.seed(s_)
                    data = ds[0]
                    assert len(windows) == 1
                    op = ds.operator_name[cap["op"]]
                    if op not in ("RandomCrop", "RandomCutout") or cap["op_out_n"] == 2048 or box_faces_clear(cap["op_in"], cap["op_log"], op):
                        break
                assert op not in ("RandomCrop", "RandomCutout") or cap["op_out_n"] == 2048 or box_faces_clear(cap["op_in"], cap["op_log"], op)
                base_draws = log_values([e for e in cap["base_log"] if e[0] == "torch"][:6])
                pro = (0.3, 0.3, 0.3, 0.2)
                lt = lambda u, p: bool((torch.tensor(u, dtype=torch.float32) < p).item())
                cat0 = cls - 1
                flags = [lt(base_draws[0], pro[0]), lt(base_draws[1], pro[1]), lt(base_draws[2], pro[2]) and cat0 in (1, 5),
                         lt(base_draws[5], pro[3])]
                applied = cap["op_log"][0][2][0] <= ds_p(op)
                pre = "gi.%d." % n
                out[pre + "scene"], out[pre + "det"], out[pre + "cls"] = np.int64(sseed), np.int64(j), np.int64(cls)
                out[pre + "seed"] = np.int64(s_)
                out[pre + "window"] = np.array([windows[0][0][0], windows[0][0][1], windows[0][1]], dtype=np.float64)
                np_state_arrays(pre + "np_gap", cap["np_gap"], out)
                np_state_arrays(pre + "np_op", cap["np_op"], out)
                seeded(pre + "torch_base", s_, torch_state=cap["torch_base"], out=out)     # (no torch draw before base_aug)
                for k in ("rotation", "translation", "fsnet_scale", "mean_shape", "sym_info", "model_point", "nocs_scale", "cat_id"):
                    out[pre + "in." + k] = cap["db"][k].numpy()
                out[pre + "gap"] = np.concatenate([np.asarray(v, np.float32).ravel() for v in cap["gap"]])
                out[pre + "base_draws"] = base_draws.astype(np.float32)
                out[pre + "flags"] = np.array(flags, np.int32)
                out[pre + "op"] = np.int64(cap["op"])
                out[pre + "op_applied"] = np.int64(applied)
                out[pre + "op_draws"] = log_values(cap["op_log"])
                out[pre + "op_draw_calls"] = np.int64(len(cap["op_log"]))
                out[pre + "M"] = np.int64(cap["op_out_n"])
                for k in ("pcl_in", "aug_pcl_in", "rotation", "translation", "fsnet_scale"):
                    if k == "aug_pcl_in" and op in ("RandomCrop", "RandomCutout") and applied:
                        continue          # drawn after the up-front attempts here: compared through M only (tests/test_augment_gpu.py)
                    out[pre + "out." + k] = data[k].numpy()
                print("item %2d cls %d flags %s op %-13s applied %d M %d" % (n, cls, flags, op, applied, cap["op_out_n"]))
        finally:
            os.chdir(cwd)


def ds_p(op):
    return {"Jitter": 0.6, "RandomCutout": 0.9, "RandomCrop": 0.9, "RandomDropout": 0.9}[op]


def main():
    stand_ins()
    importlib.import_module("config.config")           # defines the flags on the shim's FLAGS
    import absl.flags as flags
    F = flags.FLAGS
    rda = _load_by_path("ref_data_augmentation", os.path.join(REF, "datasets/data_augmentation.py"))
    sys.modules["datasets.data_augmentation"] = rda
    ld = _load_by_path("ref_load_data_aug", os.path.join(REF, "datasets/load_data.py"))
    for m in (rda, ld):
        m.np = _NpSpy("np")
    rda.torch = _TorchSpy("torch")
    out = {}
    record_base(rda, F, out)
    record_view(rda, out)
    record_getitem(ld, F, out)
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print("wrote augment.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
