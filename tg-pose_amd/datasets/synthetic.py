"""Rendered synthetic data: depth frames and instance masks of posed meshes (ops.render_depth, csrc/render.hip) in the formats the
two loaders read, with pose labels that are the numbers that produced the pixels.

A scene is a list of instances, each ``dict(mesh=index into the mesh set, inst_id=1..255, R=(3,3), t=(3,) metres, s=scale,
labels=dict)``: the model -> camera map is x_cam = s R x_model + t.  Frames come back to the host once, at generation."""
import numpy as np
import torch

from .. import ops


def _camk(camK, S):
    K = np.asarray(camK, dtype=np.float32)
    if K.shape == (3, 3):
        K = np.broadcast_to(K, (S, 3, 3))
    if K.shape != (S, 3, 3):
        raise ValueError("camK must be one (3,3) matrix or one per scene")
    return np.ascontiguousarray(K)


def pose_matrix(R, t, s=1.0):
    """[s R | t] as float32 (3,4): the pose tgp_render_depth reads"""
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(3, 3) * float(s), np.asarray(t, dtype=np.float64).reshape(3, 1)],
                          1).astype(np.float32)


def pack_scenes(scenes, n_meshes=None):
    """the host arrays of a scene list: scene_ptr (S+1) int32, inst_mesh (I) int32, inst_id (I) uint8, inst_pose (I,3,4) float32.
    Refuses an inst_id outside 1..255 or used twice in a scene, a mesh index outside the set, more than 255 instances in a scene."""
    ptr, mesh, ids, pose = [0], [], [], []
    for si, sc in enumerate(scenes):
        seen = set()
        if len(sc) > 255:
            raise ValueError("scene %d has %d instances; the cap is 255" % (si, len(sc)))
        for inst in sc:
            i = int(inst["inst_id"])
            if not 1 <= i <= 255:
                raise ValueError("scene %d: inst_id %d is outside 1..255" % (si, i))
            if i in seen:
                raise ValueError("scene %d: duplicate inst_id %d" % (si, i))
            seen.add(i)
            m = int(inst["mesh"])
            if m < 0 or (n_meshes is not None and m >= n_meshes):
                raise ValueError("scene %d: mesh index %d is outside the mesh set" % (si, m))
            mesh.append(m), ids.append(i), pose.append(pose_matrix(inst["R"], inst["t"], inst.get("s", 1.0)))
        ptr.append(len(mesh))
    return (np.asarray(ptr, dtype=np.int32), np.asarray(mesh, dtype=np.int32), np.asarray(ids, dtype=np.uint8),
            np.stack(pose).astype(np.float32) if pose else np.zeros((0, 3, 4), dtype=np.float32))


def render_scenes(meshset, scenes, camK, H, W, near=0.01):
    """Render every scene in one call and bring the frames to the host -> dict of numpy arrays: depth (S,H,W) uint16 millimetres,
    mask (S,H,W) uint8 instance ids, visible (I,) and bbox (I,4) per instance in scene order, dropped (S,2), scene_ptr (S+1),
    camK (S,3,3)."""
    if not scenes:
        raise ValueError("render_scenes: no scenes")
    ptr, mesh, ids, pose = pack_scenes(scenes, len(meshset))
    K = _camk(camK, len(scenes))
    camk = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(meshset.device)
    out = ops.render_depth(meshset, up(ptr), up(mesh), up(ids), up(pose), up(camk), H, W, near=near)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(scene_ptr=ptr, camK=K)
    return res


def scene_items(scenes, rendered):
    """One host item per visible instance, in train_batch's format (datasets/load_data.py): depth, mask, inst_id, camK, bbox (from
    the visible pixels), rotation = R, translation = t, nocs_scale = s, and the instance's ``labels`` (fsnet_scale, mean_shape,
    sym_info, model_point, cat_id, category tables ...) copied through.  Items of one scene share its depth and mask arrays."""
    items = []
    for si, sc in enumerate(scenes):
        for k, inst in enumerate(sc):
            i = int(rendered["scene_ptr"][si]) + k
            if rendered["visible"][i] <= 0:
                continue
            it = dict(inst.get("labels", {}))
            it.update(depth=rendered["depth"][si], mask=rendered["mask"][si], inst_id=int(inst["inst_id"]), camK=rendered["camK"][si].copy(),
                      bbox=rendered["bbox"][i].copy(), rotation=np.asarray(inst["R"], dtype=np.float32).reshape(3, 3),
                      translation=np.asarray(inst["t"], dtype=np.float32).reshape(3), nocs_scale=np.float32(inst.get("s", 1.0)))
            items.append(it)
    return items


def scene_frame(meshset, scenes, rendered, index):
    """Scene ``index`` as the evaluation loader's frame dict (evaluation/load_data_eval.py): depth, and per VISIBLE instance a
    channel of pred_masks (H,W,n) bool, pred_bboxes (n,4) int32, pred_class_ids (n,) (labels['cat_id'] + 1; 0 without one),
    pred_scores = 1 -- a perfect detector -- plus pred_inst (n,) the instances' positions in the scene; and for EVERY instance the
    ground truth final_results carries: gt_RTs (m,4,4) with [s R | t], gt_scales (m,3) (the mesh's extent in model units),
    gt_class_ids (m,), gt_handle_visibility (m,) = 1."""
    sc = scenes[index]
    i0 = int(rendered["scene_ptr"][index])
    depth, mask = rendered["depth"][index], rendered["mask"][index]
    cls = lambda inst: int(inst.get("labels", {}).get("cat_id", -1)) + 1
    vis = [k for k in range(len(sc)) if rendered["visible"][i0 + k] > 0]
    RTs = np.tile(np.eye(4), (len(sc), 1, 1))
    for k, inst in enumerate(sc):
        RTs[k, :3, :3] = np.asarray(inst["R"], dtype=np.float64).reshape(3, 3) * float(inst.get("s", 1.0))
        RTs[k, :3, 3] = np.asarray(inst["t"], dtype=np.float64).reshape(3)
    return dict(depth=depth,
                pred_masks=np.stack([mask == int(sc[k]["inst_id"]) for k in vis], 2) if vis else np.zeros(mask.shape + (0,), dtype=bool),
                pred_bboxes=rendered["bbox"][[i0 + k for k in vis]].astype(np.int32).reshape(-1, 4),
                pred_class_ids=np.asarray([cls(sc[k]) for k in vis], dtype=np.int32), pred_scores=np.ones(len(vis)),
                pred_inst=np.asarray(vis, dtype=np.int32), gt_RTs=RTs,
                gt_scales=np.asarray([meshset.extent[int(inst["mesh"])] for inst in sc], dtype=np.float64).reshape(-1, 3),
                gt_class_ids=np.asarray([cls(inst) for inst in sc], dtype=np.int32), gt_handle_visibility=np.ones(len(sc), dtype=np.int32))
