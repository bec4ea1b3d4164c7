"""Writes tests/golden/pd.npz: the persistence diagrams and images of tests/pd_ref.py (the float64 restatement of the reference's
datasets/compute_pd.py) on the clouds of ``clouds()``.

    python tests/golden/make_pd_golden.py

The inputs are the reference's own seven training pcl_in clouds (gi.*.out.pcl_in of augment.npz) and six synthetic ones: a jittered
sphere shell (one long-lived H2 pair), a jittered torus (two long-lived H1 pairs), an exact 8 x 8 x 8 lattice and a flat depth-like
patch on an exact grid (degenerate: cospherical and coplanar ties everywhere), a tiled cloud with heavy duplication, and a 5-point
cloud.  Rows: cloud.<name> (n, 3) float32, h1.<name> / h2.<name> (k, 2) float64 sorted by (birth, death), pdh1.<name> /
pdh2.<name> (2500,) float32; names lists the clouds in order and degenerate the names whose triangulation is not unique.
The depth patch has its cloud only: scipy's Qhull triangulates its coplanar, cospherical facets with flat simplices, so the
restatement's reduction runs on the kernel's own triangulation in the GPU tests instead.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

DEGENERATE = ("lattice", "depth_patch")
CLOUD_ONLY = ("depth_patch",)


def clouds():
    """name -> (n, 3) float32"""
    out = {}
    aug = np.load(os.path.join(HERE, "augment.npz"))
    for k in range(7):
        out["ref%d" % k] = aug["gi.%d.out.pcl_in" % k].astype(np.float32)
    rng = np.random.RandomState(7)
    v = rng.normal(size=(1024, 3))
    out["sphere"] = (0.1 * v / np.linalg.norm(v, axis=1, keepdims=True) * (1 + 0.01 * rng.uniform(-1, 1, (1024, 1)))).astype(np.float32)
    u, w = rng.uniform(0, 2 * np.pi, (2, 1024))
    R, r = 0.1, 0.03
    tor = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=1)
    out["torus"] = (tor + 1e-3 * rng.normal(size=tor.shape)).astype(np.float32)
    g = np.arange(8, dtype=np.float32) * np.float32(0.015625)         # exact binary lattice spacing
    out["lattice"] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    gx = np.arange(32, dtype=np.float32) * np.float32(0.00390625)
    X, Y = np.meshgrid(gx, gx, indexing="ij")
    Z = np.round((0.5 + 0.02 * np.sin(X * 40) + 0.01 * np.cos(Y * 55)) * 1024) / 1024      # depth quantised to 1/1024 m
    out["depth_patch"] = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    base = (0.05 * rng.normal(size=(166, 3))).astype(np.float32)
    out["tiled"] = np.tile(base, (7, 1))[:1024][rng.permutation(1024)]
    out["five"] = np.array([[0, 0, 0], [0.1, 0.01, 0.02], [0.03, 0.12, -0.01], [0.02, 0.04, 0.09], [0.05, 0.05, 0.05]], np.float32)
    return out


def main():
    from tests import pd_ref
    rows = {}
    names = []
    for name, pc in clouds().items():
        names.append(name)
        rows["cloud." + name] = pc
        if name in CLOUD_ONLY:
            continue
        pdh1, pdh2, h1, h2 = pd_ref.compute_pd(pc)
        rows.update({"h1." + name: h1, "h2." + name: h2, "pdh1." + name: pdh1, "pdh2." + name: pdh2})
        print(name, len(np.unique(pc, axis=0)), "unique points,", len(h1), "H1 and", len(h2), "H2 pairs", flush=True)
    rows["names"] = np.array(names)
    rows["degenerate"] = np.array(DEGENERATE)
    np.savez_compressed(os.path.join(HERE, "pd.npz"), **rows)


if __name__ == "__main__":
    main()
