"""Records tests/golden/acquire_models_ref.npz on the GPU: for icp_ref.table_scene(k, gap=0.0), k = 0 and 3, at 240 x 320 the
plane-cut depth frame (pose.SupportPlane()), its label image (pose.Segmenter()), the 128-point cloud of each of the three segments
(load_data_eval.clouds_from_segments, keyed draw, the tracking tests' seed) and which object each segment is; and the 2048-sample model
(ops.IcpModels.from_meshset) with the bytes and meta of its G = 32, cap 32 distance field.  scripts/search_chain_check.py and
tests/test_search_cpu.py run the restated chain on it.

    python scripts/search_chain_record.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    if not torch.cuda.is_available():
        sys.exit("search_chain_record.py records on a GPU; none is visible")
    from tests import icp_ref, plane_cases as pc
    from tgpose_amd import ops, pose
    from tgpose_amd.datasets import synthetic
    from tgpose_amd.evaluation import load_data_eval as lde
    dev = "cuda:0"
    ms = ops.MeshSet(pc.meshes(), device=dev)
    models = ops.IcpModels.from_meshset(ms, [0], 2048)
    fields = ops.DistanceFields(models, G=32, cap=32)
    sup, sg = pose.SupportPlane(), pose.Segmenter()
    K = pc.K
    camk = torch.tensor([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=torch.float32, device=dev)
    out = dict(field=fields.field[0].cpu().numpy(), meta=fields.meta_host[0], model=models.points_normals[0].cpu().numpy())
    for k in (0, 3):
        scene = icp_ref.table_scene(k, gap=0.0)
        rendered = synthetic.render_scenes(ms, [scene], K, pc.H, pc.W)
        depth = torch.from_numpy(rendered["depth"][0][None].view(np.int16)).to(dev)
        cut = sup(depth, camk, [0], pc.SEED)[0]
        seg = sg(cut, camk)
        n = int(seg.info[0, 1])
        clouds, _ = lde.clouds_from_segments(cut, seg, camk, n_pts=128, sampler="device", seed=pc.SEED)
        centers = seg.centers[0, :n].cpu().numpy().astype(np.float64)
        out["obj.%d" % k] = np.asarray([int(np.argmin([np.linalg.norm(c - np.asarray(i["t"])) for i in scene[:3]])) for c in centers])
        out["clouds.%d" % k] = clouds[:n].cpu().numpy()
        out["cut.%d" % k] = cut[0].cpu().numpy().view(np.uint16)
        out["labels.%d" % k] = seg.labels[0].cpu().numpy()
    dst = os.path.join(ROOT, "tests", "golden", "acquire_models_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s %.1f KB" % (dst, os.path.getsize(dst) / 1024.0))


if __name__ == "__main__":
    main()
