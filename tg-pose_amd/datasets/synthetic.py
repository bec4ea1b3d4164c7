"""Rendered synthetic data: depth frames and instance masks of posed meshes (ops.render_depth, csrc/render.hip) in the formats the
two loaders read, with pose labels that are the numbers that produced the pixels.

A scene is a list of instances, each ``dict(mesh=index into the mesh set, inst_id=1..255, R=(3,3), t=(3,) metres, s=scale,
labels=dict)``: the model -> camera map is x_cam = s R x_model + t.  Frames come back to the host once, at generation.

``mesh_labels`` makes an instance's ``labels`` from its mesh (ops.mesh_sample_fps, csrc/meshsample.hip) and ``category_tables`` the
category clouds and persistence images TrainBatches takes, so nothing about a rendered item is hand-written."""
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


def _surface_clouds(meshset, meshes, n, seed):
    """(len(meshes), n, 3) float32 on the device: 2 n surface samples of each mesh thinned to n by farthest point sampling, the
    draws keyed by (seed, mesh index) -- a mesh's cloud depends on neither the other jobs nor the order of the calls"""
    meshes = [int(m) for m in meshes]
    return ops.mesh_sample_fps(meshset, meshes, int(n), 2, keys=meshes, seed=seed)


def mesh_labels(meshset, mesh, category, s, n_model=1024, seed=0):
    """The ``labels`` dict of an instance of mesh ``mesh`` (category name ``category``, scale ``s``: model units -> metres), made
    from the mesh and nothing hand-written: model_point (n_model,3) float32 in the mesh's own units (ops.mesh_sample_fps, ratio 2,
    device draws keyed by (seed, mesh)); fsnet_scale and mean_shape (3,) in metres -- load_data.get_fs_net_scale with nocs_scale = s,
    divided by 1000 as the reference's loader does (:273-276); sym_info, cat_id (0-based), nocs_scale.
    The size handed to get_fs_net_scale is the mesh's own axis-aligned extent, not the extent of model_point: the samples stop
    short of the outermost vertices by a fraction of a facet (1.4e-4 to 1.7e-2 model units on the four lathe shapes, up to 1.7 mm
    at s = 0.1), and the label is the object's size; model_point's own extent differs from it by that much."""
    from . import load_data as ld
    from ..evaluater.RT_TDA_Evaluater import SYNSET_NAMES
    mesh = int(mesh)
    if not 0 <= mesh < len(meshset):
        raise ValueError("mesh_labels: mesh index %d is outside the set of %d meshes" % (mesh, len(meshset)))
    out = _surface_clouds(meshset, [mesh], n_model, seed)
    ops.mesh_check_status(out["status"], "mesh_labels")
    ext = np.asarray(meshset.extent[mesh], dtype=np.float32)
    fsnet_scale, mean_shape = ld.get_fs_net_scale(category, np.stack([np.zeros_like(ext), ext]), s)
    return dict(model_point=out["points"][0].cpu().numpy(), fsnet_scale=(fsnet_scale / 1000.0).astype(np.float32),
                mean_shape=(mean_shape / 1000.0).astype(np.float32), sym_info=ld.get_sym_info(category),
                cat_id=SYNSET_NAMES.index(category) - 1, nocs_scale=np.float32(s))


def category_tables(meshset, cat_mesh, n=1024, seed=0):
    """TrainBatches(category_tables=...)'s triple from each category's canonical mesh: cat_mesh (C) mesh indices, None or a negative
    index for a category without a mesh (its rows are zeros) -> points_category (C,n,3), pdh1_category (C,2500), pdh2_category
    (C,2500), float32 numpy.  The clouds are sampled as mesh_labels' model_point (same keys: a category's cloud is its mesh's
    model_point at the same n and seed); the images are ops.persistence_images of those clouds."""
    cat_mesh = [-1 if m is None else int(m) for m in cat_mesh]
    live = [c for c, m in enumerate(cat_mesh) if m >= 0]
    if not live:
        raise ValueError("category_tables: no category has a mesh")
    if any(cat_mesh[c] >= len(meshset) for c in live):
        raise ValueError("category_tables: a mesh index is outside the set of %d meshes" % len(meshset))
    out = _surface_clouds(meshset, [cat_mesh[c] for c in live], n, seed)
    ops.mesh_check_status(out["status"], "category_tables")
    h1, h2 = ops.persistence_images(out["points"].contiguous())
    C = len(cat_mesh)
    tabs = [np.zeros((C, int(n), 3), np.float32), np.zeros((C, h1.shape[1]), np.float32), np.zeros((C, h2.shape[1]), np.float32)]
    for t, src in zip(tabs, (out["points"], h1, h2)):
        t[live] = src.cpu().numpy()
    return tuple(tabs)
