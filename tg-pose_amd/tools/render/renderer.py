"""The reference's renderer interface (tools/render/renderer.py: create_renderer, add_object, remove_object, render_object) over the
HIP depth rasteriser (ops.render_depth, csrc/render.hip).  The reference's only back end opens an OpenGL window; this one runs on a
headless GPU.  Deviations (DESIGN.md section 3 "The depth renderer"): depth only (no colour, no shading, no light); the sample
point of pixel (row j, column i) is (i, j) in the intrinsics' coordinates, the loaders' back-projection convention, not OpenGL's
pixel centre (i + 0.5, j + 0.5); a triangle with a vertex nearer than the near distance is dropped whole, not clipped; models are
given as arrays, file reading stays with the caller."""
import numpy as np
import torch

from ... import ops


class Renderer(object):
    """Abstract class of a renderer (the reference's)."""

    def __init__(self, width, height):
        self.width = width
        self.height = height

    def add_object(self, obj_id, model, **kwargs):
        raise NotImplementedError

    def remove_object(self, obj_id):
        raise NotImplementedError

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        raise NotImplementedError


class RendererHip(Renderer):
    """Depth renderer on the GPU.  ``near`` is in metres."""

    def __init__(self, width, height, device="cuda", near=0.01):
        super(RendererHip, self).__init__(int(width), int(height))
        self.device, self.near = device, float(near)
        self.models = {}

    def add_object(self, obj_id, model, scale=1.0):
        """model: a dict with 'pts' (V,3) and 'faces' (F,3), as the reference's load_ply returns, or a (verts, faces) pair.
        scale: metres per model unit (0.001 for a model in millimetres); poses and the rendered depth are in the model's units."""
        if obj_id in self.models:
            raise ValueError("object %r is already loaded" % (obj_id,))
        verts, faces = (model["pts"], model["faces"]) if isinstance(model, dict) else model
        if not float(scale) > 0.0:
            raise ValueError("scale must be positive")
        self.models[obj_id] = (ops.MeshSet([(verts, faces)], device=self.device), float(scale))

    def remove_object(self, obj_id):
        del self.models[obj_id]

    def scene(self, obj_id, R, t, fx, fy, cx, cy):
        """the single-instance scene render_object renders, as ops.render_depth's arguments after the mesh set"""
        meshset, scale = self.models[obj_id]
        pose = np.concatenate([np.asarray(R, dtype=np.float64).reshape(3, 3) * scale, np.asarray(t, dtype=np.float64).reshape(3, 1) * scale],
                              1).astype(np.float32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(meshset.device)
        return (up(np.array([0, 1], dtype=np.int32)), up(np.zeros(1, dtype=np.int32)), up(np.ones(1, dtype=np.uint8)), up(pose[None]),
                up(np.array([[fx, fy, cx, cy]], dtype=np.float32)))

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        """-> {'depth': (height, width) float32 ndarray} in the model's units, 0 where no surface"""
        meshset, scale = self.models[obj_id]
        out = ops.render_depth(meshset, *self.scene(obj_id, R, t, fx, fy, cx, cy), self.height, self.width, near=self.near, return_z=True)
        z = out["z"][0].cpu().numpy()
        return {"depth": np.where(np.isfinite(z), z / np.float32(scale), np.float32(0)).astype(np.float32)}


def create_renderer(width, height, renderer_type="hip", mode="depth", device="cuda"):
    """A factory with the reference's name.  renderer_type: 'hip' only (the reference's 'python' and 'cpp' back ends need an OpenGL
    context and are not rebuilt); mode: 'depth' only."""
    if renderer_type != "hip":
        raise ValueError("Unknown renderer type %r: only 'hip' is built (the reference's 'python' / 'cpp' renderers need OpenGL)" % (renderer_type,))
    if mode != "depth":
        raise NotImplementedError("mode %r: only 'depth' is rendered; there is no RGB output" % (mode,))
    return RendererHip(width, height, device=device)
