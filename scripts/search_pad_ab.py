"""A/B of the pose search's LDS image of the field: the product library (rows of G bytes) against the same library built with
-DTGP_SEARCH_PAD=4 (each z row 4 bytes longer, against bank conflicts between the runs of bytes a wave reads two rows apart).  Both
libraries are loaded into ONE process and called with the same argument struct in interleaved rounds (9 rounds, the first 2 dropped;
windows of 10 / 3 back-to-back calls between two HIP events); the integer outputs are compared.  Build the variant first:

    python -m tgpose_amd.build --searchpad && python scripts/search_pad_ab.py          -> profiles/search_pad_ab.json
"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tests import icp_ref, plane_cases as pc
from tgpose_amd import _lib, ops, pose
from tgpose_amd.tools.lynne_lib import view_sampler
dev = "cuda:0"
h4 = ctypes.CDLL(os.path.join(ROOT, "tg-pose_amd", "libtgpose_hip_searchpad.so"))
for name, (res, args) in _lib.SIGNATURES.items():
    fn = getattr(h4, name)
    fn.restype, fn.argtypes = res, args
libs = {"pad0": _lib.lib(), "pad4": h4}
ms = ops.MeshSet(pc.meshes(), device=dev)
models = ops.IcpModels.from_meshset(ms, [0], 2048)
Rs = torch.from_numpy(view_sampler.rotation_grid(42, 12)).to(dev)
fields = {G: ops.DistanceFields(models, G=G, cap=32) for G in (32, 48)}
r = np.random.RandomState(2)
y = models.points_normals[0, :, :3].cpu().numpy().astype(np.float64)
out = []
for J, n, G in ((6, 128, 32), (6, 128, 48), (192, 128, 32), (192, 128, 48), (192, 512, 32)):
    clouds = np.empty((J, n, 3), np.float32)
    for j in range(J):
        R = icp_ref.rot(r.randn(3), r.uniform(0, 180))
        clouds[j] = 0.15 * (y[r.randint(0, len(y), n)] + r.randn(n, 3) * 0.003) @ R.T + [0.0, 0.0, 0.8] + r.randn(3) * 0.05
    c = torch.from_numpy(clouds).to(dev)
    anchors, scales, jm = pose.cloud_anchors(c), torch.full((J,), 0.15, device=dev), torch.zeros(J, dtype=torch.int32, device=dev)
    f, top = fields[G], 16
    res = {}
    for name in libs:
        o = dict(cost=torch.empty(J, top, device=dev, dtype=torch.int32), rot=torch.empty(J, top, device=dev, dtype=torch.int32),
                 shift=torch.empty(J, top, device=dev, dtype=torch.int32), poses=torch.empty(J, top, 3, 4, device=dev), table=torch.empty(J, 504, 2, device=dev, dtype=torch.int32))
        a = _lib.PoseSearchArgs(field=ops._p(f.field), meta=ops._p(f.meta), M=1, G=G, cap=32, job_model=ops._p(jm), clouds=ops._p(c), counts=None,
                                anchors=ops._p(anchors), scales=ops._p(scales), J=J, n_cap=n, rotations=ops._p(Rs), R=504, K=5, stride=2, top=top,
                                cost=ops._p(o["cost"]), rot=ops._p(o["rot"]), shift=ops._p(o["shift"]), poses=ops._p(o["poses"]),
                                workspace=ops._p(o["table"]), workspace_bytes=J * 504 * 8)
        res[name] = (o, a)
    def run(name):
        rc = libs[name].tgp_pose_search(ctypes.byref(res[name][1]), ops._stream(c))
        assert rc == 0, rc
    for name in libs:
        run(name)
    torch.cuda.synchronize()
    same = all(torch.equal(res["pad0"][0][k], res["pad4"][0][k]) for k in ("cost", "rot", "shift", "table"))
    calls = 10 if J == 6 else 3
    times = {name: [] for name in libs}
    for rnd in range(9):
        for name in libs:
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(calls):
                run(name)
            e.record()
            torch.cuda.synchronize()
            if rnd >= 2:
                times[name].append(s.elapsed_time(e) / calls)
    row = dict(jobs=J, n=n, G=G, equal=same, **{name + "_median_ms": statistics.median(t) for name, t in times.items()},
               **{name + "_min_ms": min(t) for name, t in times.items()})
    out.append(row)
    print(json.dumps(row), flush=True)
with open(os.path.join(ROOT, "profiles", "search_pad_ab.json"), "w") as fh:
    json.dump(dict(device=torch.cuda.get_device_name(0), rotations=504, K=5, stride=2, top=16, rows=out), fh, indent=1)
    fh.write("\n")
