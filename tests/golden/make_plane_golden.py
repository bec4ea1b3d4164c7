"""Regenerates tests/golden/plane_utils_ref.npz from the REFERENCE's own ``tools/plane_utils.py`` (loaded by path, unmodified), on the
CPU.

Stored: pc (2,3,64,3) float32 about the origin with an extent of about 0.2 and random positive weights pc_w (2,3,64), and what the
reference returned for them, in float32 (``f32.*``) and again on ``.double()`` inputs (``f64.*``):
  get_plane_in_batch  on the whole batch                      -> batch.normal (2,3,3), batch.dn (2,3,3), batch.p2plane (2,3,1)
  get_plane           on each of the six 2-D slices            -> single.normal (2,3,3), single.dn (2,3,3), single.p2plane (2,3,1)
  get_plane_parameter on each slice                            -> single.X (2,3,3,1)
Arrays only.

Usage:  python tests/golden/make_plane_golden.py REFERENCE_ROOT   (from the repo root; or set $TGP_REFERENCE)
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ref_root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TGP_REFERENCE", ""))
    path = os.path.join(ref_root, "tools", "plane_utils.py")
    if not os.path.isfile(path):
        sys.exit("usage: make_plane_golden.py REFERENCE_ROOT")
    spec = importlib.util.spec_from_file_location("ref_plane_utils", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    r = np.random.RandomState(3)
    # clouds near tilted planes: z = a x + b y + c plus noise, x and y within +-0.1
    xy = r.uniform(-0.1, 0.1, (2, 3, 64, 2))
    abc = r.uniform(-0.5, 0.5, (2, 3, 1, 3)) * np.array([1.0, 1.0, 0.1])
    z = abc[..., 0] * xy[..., 0] + abc[..., 1] * xy[..., 1] + abc[..., 2] + r.randn(2, 3, 64) * 0.003
    pc = np.concatenate([xy, z[..., None]], -1).astype(np.float32)
    pc_w = r.uniform(0.1, 1.0, (2, 3, 64)).astype(np.float32)
    out = {"pc": pc, "pc_w": pc_w}
    for tag, cast in (("f32", lambda t: t), ("f64", lambda t: t.double())):
        P, Wt = cast(torch.from_numpy(pc)), cast(torch.from_numpy(pc_w))
        n, dn, p2 = ref.get_plane_in_batch(P, Wt)
        out["%s.batch.normal" % tag], out["%s.batch.dn" % tag], out["%s.batch.p2plane" % tag] = n.numpy(), dn.numpy(), p2.numpy()
        single = [[ref.get_plane(P[i, j], Wt[i, j]) for j in range(3)] for i in range(2)]
        for k, name in enumerate(("normal", "dn", "p2plane")):
            out["%s.single.%s" % (tag, name)] = np.stack([np.stack([single[i][j][k].numpy() for j in range(3)]) for i in range(2)])
        out["%s.single.X" % tag] = np.stack([np.stack([ref.get_plane_parameter(P[i, j], Wt[i, j]).numpy() for j in range(3)]) for i in range(2)])
    dst = os.path.join(HERE, "plane_utils_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote plane_utils_ref.npz %.1f KB" % (os.path.getsize(dst) / 1024.0))
    for k, v in out.items():
        print("  %-22s %s %s" % (k, v.dtype, v.shape))


if __name__ == "__main__":
    main()
