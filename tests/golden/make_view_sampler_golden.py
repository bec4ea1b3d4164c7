"""Regenerates tests/golden/view_sampler_ref.npz from the REFERENCE's own ``tools/lynne_lib/view_sampler.py`` (loaded by path,
unmodified).  That file imports ``tools.transform``, which the reference's tree does not hold; tests/golden/_transform_shim stands in
for it (one function, a rotation about an axis) while the file loads.

Stored for n = 12, 42 and 162 views: ``pts.<n>`` (n,3) float64 and ``level.<n>`` (n,) int64 from hinter_sampling(n), ``R.<n>``
(n,3,3) and ``t.<n>`` (n,3,1) float64 from sample_views(n).  Arrays only.

Usage:  python tests/golden/make_view_sampler_golden.py REFERENCE_ROOT   (from the repo root; or set $TGP_REFERENCE)
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402


def main():
    ref_root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TGP_REFERENCE", ""))
    path = os.path.join(ref_root, "tools", "lynne_lib", "view_sampler.py")
    if not os.path.isfile(path):
        sys.exit("usage: make_view_sampler_golden.py REFERENCE_ROOT")
    sys.path.insert(0, os.path.join(HERE, "_transform_shim"))
    spec = importlib.util.spec_from_file_location("ref_view_sampler", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for n in (12, 42, 162):
        pts, level = ref.hinter_sampling(n)
        views, level2 = ref.sample_views(n)
        assert list(level) == list(level2) and len(views) == len(pts) == n
        out["pts.%d" % n], out["level.%d" % n] = np.asarray(pts, dtype=np.float64), np.asarray(level, dtype=np.int64)
        out["R.%d" % n] = np.stack([v["R"] for v in views]).astype(np.float64)
        out["t.%d" % n] = np.stack([v["t"] for v in views]).astype(np.float64)
    dst = os.path.join(HERE, "view_sampler_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote view_sampler_ref.npz %.1f KB" % (os.path.getsize(dst) / 1024.0))
    for k, v in out.items():
        print("  %-10s %s %s" % (k, v.dtype, v.shape))


if __name__ == "__main__":
    main()
