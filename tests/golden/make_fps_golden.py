"""Regenerates tests/golden/fps_ref.npz from the REFERENCE's own ``core/utils/farthest_points_torch.py`` (farthest_points with its
default dist_func = F.pairwise_distance, init_center=True), loaded by file path, unmodified, on the CPU.  Nothing is copied from the
reference: the fixture holds arrays only.

Clouds (name: points -> centres):
  * grid:   a 40 x 40 planar grid -> 256 (exact ties at every step);
  * dups:   50 points, each 8 times -> 200 (duplicates must be chosen);
  * rand:   300 random points -> 64;
  * depth0, depth1: back-projected elliptical patches of a noisy sloped depth surface, in the cut cloud's row-major pixel order
    (about 3300 and 6900 points) -> 1024.
Stored per cloud: <name>_xyz (M,3) float32, <name>_mean (3,) the reference's torch.mean row, <name>_centers (n,) int32,
<name>_clusters (M,) int32, <name>_dist (M,) float32 and <name>_seconds, the reference's CPU time for the call (one run; indicative
only); ``names`` and ``n`` list them.  ``time_M`` / ``time_seconds``: the reference's CPU time for one uniform random cloud of
2048, 4096 and 8192 points -> 1024 (the sizes scripts/fps_time.py times on the device; one run each, one thread, indicative only).

Before writing, the recorder checks the condition the tests rely on: tests/fps_ref.py with the stored mean reproduces every stored
centre, cluster and distance bit.  A cloud that failed it would have to be replaced, never the comparison weakened.

Usage:  python tests/golden/make_fps_golden.py REFERENCE_ROOT   (from the repo root)
"""
import importlib.util
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import fps_ref  # noqa: E402


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def depth_cloud(seed, ry, rx):
    """an elliptical mask over a noisy sloped depth image, back-projected with the REAL intrinsics, pixels in row-major order"""
    rng = np.random.RandomState(seed)
    H = W = 128
    yy, xx = np.mgrid[0:H, 0:W]
    e = ((yy - 64) / float(ry)) ** 2 + ((xx - 64) / float(rx)) ** 2
    z = 700.0 - 90.0 * np.sqrt(np.clip(1.0 - e, 0, 1)) + 0.3 * xx + rng.randn(H, W) * 1.5
    keep = (e <= 1.0) & (rng.rand(H, W) >= 0.03)
    z = np.round(z[keep]).astype(np.float32) / np.float32(1000.0)
    u, v = (xx[keep] + 250).astype(np.float32), (yy[keep] + 180).astype(np.float32)
    x = (u - np.float32(322.525)) * z / np.float32(591.0125)
    y = (v - np.float32(244.11084)) * z / np.float32(590.16775)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def clouds():
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * np.float32(0.025)
    grid = np.concatenate([g, np.full((1600, 1), 0.5, np.float32)], axis=1)
    base = rng.random((50, 3), dtype=np.float32)
    dups = np.repeat(base, 8, axis=0)
    rand = rng.random((300, 3), dtype=np.float32)
    return [("grid", grid, 256), ("dups", dups, 200), ("rand", rand, 64), ("depth0", depth_cloud(3, 30, 36), 1024),
            ("depth1", depth_cloud(4, 44, 52), 1024)]


def main(ref_root):
    fp = _load_by_path("ref_farthest_points_torch", os.path.join(ref_root, "core", "utils", "farthest_points_torch.py"))
    torch.set_num_threads(1)
    out = {"names": np.array([c[0] for c in clouds()]), "n": np.array([c[2] for c in clouds()], np.int32)}
    for name, xyz, n in clouds():
        t = torch.from_numpy(xyz)
        t0 = time.perf_counter()
        clusters, centers, dist = fp.farthest_points(t, n, return_center_indexes=True, return_distances=True, init_center=True)
        sec = time.perf_counter() - t0
        mean = torch.mean(t, 0, keepdim=True)[0].numpy()
        centers, clusters, dist = centers.numpy().astype(np.int32), clusters.numpy().astype(np.int32), dist.numpy()
        idx, d, cl = fps_ref.fps(xyz, n, start=mean)
        assert np.array_equal(idx, centers), (name, "centres", int((idx != centers).sum()))
        assert np.array_equal(cl, clusters), (name, "clusters")
        assert np.array_equal(d.view(np.int32), dist.view(np.int32)), (name, "distance bits")
        own = fps_ref.fps(xyz, n)[0]
        assert np.array_equal(own, centers), (name, "centres with the restatement's own centroid")
        print("%-7s M=%5d n=%4d  reference %.3f s  restatement equal (stored mean: idx, clusters, distance bits; own centroid: idx)"
              % (name, len(xyz), n, sec))
        out.update({name + "_xyz": xyz, name + "_mean": mean.astype(np.float32), name + "_centers": centers, name + "_clusters": clusters,
                    name + "_dist": dist, name + "_seconds": np.float64(sec)})
    sizes, secs = [2048, 4096, 8192], []
    for M in sizes:
        t = torch.from_numpy(np.random.default_rng(M).random((M, 3), dtype=np.float32))
        t0 = time.perf_counter()
        fp.farthest_points(t, 1024)
        secs.append(time.perf_counter() - t0)
        print("reference, %d -> 1024: %.3f s" % (M, secs[-1]))
    out.update(time_M=np.array(sizes, np.int32), time_seconds=np.array(secs, np.float64))
    path = os.path.join(HERE, "fps_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
