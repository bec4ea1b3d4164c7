"""The model-based acquisition chain restated on the CPU (tests/search_ref.py, tests/icp_ref.py, tests/verify_ref.py) on the real
plane-cut, segmented 128-point clouds of icp_ref.table_scene frames 0 and 3, recorded once in tests/golden/acquire_models_ref.npz
(scripts/search_chain_record.py): does every object end within 2 degrees / 2 mm with rotation_grid(42, 12), G = 32, cap 32, K = 5,
stride 2, top 16, ICP gate 1 cm point-to-plane, verify tau 5?  Prints one line per object; exits 1 when one misses.  About a minute.

    python scripts/search_chain_check.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import icp_ref, plane_cases as pc, search_ref as sr  # noqa: E402
from tgpose_amd.tools.lynne_lib import view_sampler  # noqa: E402

G, CAP, K, STRIDE, TOP, GATE, TAU = 32, 32, 5, 2, 16, 0.01, 5


def main():
    d = np.load(os.path.join(ROOT, "tests", "golden", "acquire_models_ref.npz"))
    Rs = view_sampler.rotation_grid(42, 12)
    model, field, meta = d["model"], d["field"], d["meta"]
    assert np.array_equal(meta, sr.field_meta(model[:, :3], G, CAP)[0])
    mesh = pc.meshes()[0]
    bad = 0
    for k in (0, 3):
        cut, labels = d["cut.%d" % k], d["labels.%d" % k]
        for slot, o in enumerate(d["obj.%d" % k]):
            best = sr.acquire_chain(field, meta, CAP, model, mesh, d["clouds.%d" % k][slot], icp_ref.OBJECTS[o]["s"], Rs, K, STRIDE, TOP, GATE, cut,
                                    pc.CAMK, TAU, mask=labels, mask_val=slot + 1)
            Rg, tg, _ = pc.gt_pose(k, o)
            deg, mm = icp_ref.pose_error(best["R"], best["t"], Rg, tg)
            ok = deg < 2.0 and mm < 2.0
            bad += not ok
            print("frame %d object %d: rank %d of cost %s, %d inliers, score %.4f: %.3f deg %.3f mm %s"
                  % (k, o, best["rank"], best["found"]["cost"][best["rank"]], best["inliers"], best["score"], deg, mm,
                     "" if ok else "MISSES 2 deg / 2 mm"), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
