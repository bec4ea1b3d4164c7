"""Regenerates tests/golden/mesh_sample_ref.npz from the REFERENCE's own ``network/point_sample/pc_sample_sphere.py`` (uniform_sample,
farthest_point_sampling; loaded by path, unmodified, with stand-in ``cv2`` / ``tqdm`` modules it imports and never calls here) and
``datasets/load_data.py`` (PoseDataset.get_fs_net_scale / get_sym_info, called unbound with None as self), on the CPU.

Stored: the meshes (float32 vertices, int32 faces), per case the seed, the reference's (n, 6) output under np.random.seed(seed) and
the next np.random.random() after it; one farthest point sampling case (512 samples of icosphere(50, 3) -> 256 indices); the label
functions' values for the six categories.

The maker ASSERTS the two conditions under which the kernel reproduces the reference itself, and moves to the next seed when one
fails:
  1. no u * total lies within 1e-12 * total of a cumulative-area boundary, so a cumulative sum added in another order (the kernel's
     chunks) picks the same faces;
  2. in the farthest point sampling case the best running distance exceeds the runner-up by at least 1e-4 model units at every step:
     torch's 1e-6 offset (at most 1.8e-6) and the float32 rounding of coordinates near 50 (about 1e-5) cannot change the choice.

Usage:  python tests/golden/make_mesh_sample_golden.py REFERENCE_ROOT   (from the repo root; or set $TGP_REFERENCE)
"""
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_augment_golden as mag  # noqa: E402  (its stand-ins for the reference loader's imports; puts REF and the repo on sys.path)

import numpy as np  # noqa: E402

REF, ROOT = mag.REF, mag.ROOT
SIZES = (1, 100, 1000)
FIRST_SEED = 7
CATEGORIES = ("bottle", "bowl", "camera", "can", "laptop", "mug")


def meshes():
    from tgpose_amd.datasets import shapes
    tri = (np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.25, 1.0, 0.5]], np.float32), np.array([[0, 1, 2]], np.int32))
    return [("triangle", tri), ("box", shapes.box((0.3, 0.2, 0.1))), ("icosphere1", shapes.icosphere(0.5, 1)),
            ("icosphere3", shapes.icosphere(0.5, 3)), ("mug", shapes.lathe(shapes.PROFILES["mug"], 24))]


def load_reference_sampler():
    for name in ("cv2", "tqdm"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.tqdm = lambda it, *a, **k: it
            sys.modules[name] = m
    return mag._load_by_path("ref_pc_sample_sphere_mesh", os.path.join(REF, "network/point_sample/pc_sample_sphere.py"))


def boundary_gap(v, f, seed, n):
    """the smallest |u * total - cum[k]| / total over the n samples' face draws and all boundaries (serial cumulative sum)"""
    tri = v.astype(np.float64)[f]
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1))
    u = np.random.RandomState(seed).random_sample((n, 3))[:, 0]
    return np.abs(u[:, None] * cum[-1] - cum[None, :]).min() / cum[-1]


def fps_margin(points, n):
    """farthest_point_sampling's loop restated, returning the smallest (best - runner-up) running distance over its n argmax steps"""
    d = np.sqrt(((points[:, None, :] - points[None, :, :]) ** 2).sum(-1))
    run, idx, worst = d[:, 0].copy(), 0, np.inf
    for _ in range(n):
        run = np.minimum(run, d[:, idx])
        top = np.sort(run)[-2:]
        worst = min(worst, top[1] - top[0])
        idx = int(np.argmax(run))
    return worst


def main():
    ref = load_reference_sampler()
    out = {"sizes": np.asarray(SIZES, np.int64), "names": np.asarray([k for k, _ in meshes()])}
    worst_gap = np.inf
    for name, (v, f) in meshes():
        out["mesh.%s.verts" % name], out["mesh.%s.faces" % name] = v, f
        for n in SIZES:
            seed = FIRST_SEED
            while boundary_gap(v, f, seed, n) <= 1e-12:
                seed += 1
            gap = boundary_gap(v, f, seed, n)
            assert gap > 1e-12, (name, n, seed, gap)
            worst_gap = min(worst_gap, gap)
            np.random.seed(seed)
            got = ref.uniform_sample(v.astype(np.float64), f, n, with_normal=True)
            nxt = np.random.random()
            assert got.shape == (n, 6) and got.dtype == np.float64
            out["case.%s.%d.seed" % (name, n)] = np.int64(seed)
            out["case.%s.%d.out" % (name, n)] = got
            out["case.%s.%d.next" % (name, n)] = np.float64(nxt)
    print("smallest boundary gap: %.3g of the total area" % worst_gap)

    from tgpose_amd.datasets import shapes
    v, f = shapes.icosphere(50.0, 3)
    seed = 3
    while True:
        np.random.seed(seed)
        pts = ref.uniform_sample(v.astype(np.float64), f, 512, with_normal=False)
        margin = fps_margin(pts, 256)
        if margin >= 1e-4 and boundary_gap(v, f, seed, 512) > 1e-12:
            break
        seed += 1
    assert margin >= 1e-4, margin
    idx = ref.farthest_point_sampling(pts, 256)
    print("fps case: seed %d, smallest margin %.3g model units" % (seed, margin))
    out["fps.verts"], out["fps.faces"], out["fps.seed"] = v, f, np.int64(seed)
    out["fps.points"], out["fps.index"], out["fps.margin"] = pts, np.asarray(idx, np.int64), np.float64(margin)

    mag.stand_ins()
    importlib.import_module("config.config")
    sys.modules["datasets.data_augmentation"] = mag._load_by_path("ref_data_augmentation_m", os.path.join(REF, "datasets/data_augmentation.py"))
    ld = mag._load_by_path("ref_load_data_mesh", os.path.join(REF, "datasets/load_data.py"))
    model = np.random.RandomState(0).rand(64, 3).astype(np.float32) - np.float32(0.5)
    out["labels.model"], out["labels.nocs_scale"] = model, np.float64(0.37)
    out["labels.names"] = np.asarray(CATEGORIES)
    for c in CATEGORIES:
        res, mean = ld.PoseDataset.get_fs_net_scale(None, c, model, 0.37)
        out["labels.%s.fsnet_scale" % c], out["labels.%s.mean_shape" % c] = np.asarray(res), np.asarray(mean)
        out["labels.%s.sym" % c] = ld.PoseDataset.get_sym_info(None, c)
    out["labels.mug.sym_no_handle"] = ld.PoseDataset.get_sym_info(None, "mug", mug_handle=0)
    out["labels.unknown.sym"] = ld.PoseDataset.get_sym_info(None, "teapot")
    path = os.path.join(HERE, "mesh_sample_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote mesh_sample_ref.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
