"""Procedural triangle meshes as (float32 verts (V,3), int32 faces (F,3)): shapes whose surface is known in closed form, for the depth
renderer (ops.render_depth) and the synthetic datasets built on it.  Every mesh but ``plane`` is closed (each edge is shared by exactly
two faces) and wound counter-clockwise seen from outside; the axis of the solids of revolution is y, the NOCS up axis."""
import numpy as np


def _mesh(verts, faces):
    return np.ascontiguousarray(verts, dtype=np.float32), np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)


def box(size):
    """an axis-aligned box centred at the origin; size: one edge length or (sx, sy, sz).  8 vertices, 12 faces"""
    h = np.broadcast_to(np.asarray(size, dtype=np.float64), (3,)) / 2.0
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * h      # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]            # -x +x -y +y -z +z
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return _mesh(v, f)


def plane(w, h, nx=1, ny=1):
    """a w x h rectangle in the plane z = 0, centred, cut into nx x ny cells of two triangles (an open mesh)"""
    xs, ys = np.linspace(-w / 2.0, w / 2.0, nx + 1), np.linspace(-h / 2.0, h / 2.0, ny + 1)
    gx, gy = np.meshgrid(xs, ys)
    v = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1)
    f = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            b, c, d = a + 1, a + nx + 2, a + nx + 1
            f += [(a, b, c), (a, c, d)]
    return _mesh(v, f)


def icosphere(r, level):
    """a sphere of radius r: the icosahedron, each face split in four ``level`` times; 20 * 4^level faces"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(level)):
        mid, nf = {}, []

        def m(a, b):
            k = (a, b) if a < b else (b, a)
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return _mesh(np.stack(v) * float(r), f)


def lathe(profile, n):
    """the solid of revolution of ``profile`` about the y axis in n steps.  profile: (radius, y) points in order, the first and the
    last on the axis (radius 0), every other radius positive; a closed outline (for instance up the outside of a bowl, over its rim
    and down the inside) gives a closed mesh.  Listed from the bottom pole up the outside, the faces are wound counter-clockwise
    seen from outside."""
    prof = np.asarray(profile, dtype=np.float64).reshape(-1, 2)
    n = int(n)
    if len(prof) < 3 or n < 3 or prof[0, 0] != 0 or prof[-1, 0] != 0 or (prof[1:-1, 0] <= 0).any():
        raise ValueError("lathe: at least 3 profile points, n >= 3, the first and last radius 0, the others positive")
    ang = 2.0 * np.pi * np.arange(n) / n
    c, s = np.cos(ang), np.sin(ang)
    v = [[0.0, prof[0, 1], 0.0]]
    for rad, y in prof[1:-1]:
        v += [[rad * c[i], y, rad * s[i]] for i in range(n)]
    v.append([0.0, prof[-1, 1], 0.0])
    rings = len(prof) - 2
    ring = lambda k, i: 1 + k * n + (i % n)
    top = 1 + rings * n
    f = []
    for i in range(n):
        f.append((0, ring(0, i), ring(0, i + 1)))
        for k in range(rings - 1):
            a, b, cc, d = ring(k, i), ring(k + 1, i), ring(k + 1, i + 1), ring(k, i + 1)
            f += [(a, b, cc), (a, cc, d)]
        f.append((top, ring(rings - 1, i + 1), ring(rings - 1, i)))
    return _mesh(v, f)


def cylinder(r, h, n):
    """a capped cylinder of radius r and height h about the y axis, n steps around: 2 n + 2 vertices, 4 n faces"""
    return lathe([(0, -h / 2.0), (r, -h / 2.0), (r, h / 2.0), (0, h / 2.0)], n)


def _arc(r0, y0, r1, y1, steps, bulge=0.0):
    """steps points from (r0, y0) towards (r1, y1), the end left out; bulge pushes the middle outwards in radius"""
    t = np.arange(steps) / float(steps)
    return [(r0 + (r1 - r0) * u + bulge * np.sin(np.pi * u), y0 + (y1 - y0) * u) for u in t]


def _bottle():
    p = [(0.0, -0.5)] + _arc(0.17, -0.5, 0.17, 0.12, 8) + _arc(0.17, 0.12, 0.06, 0.3, 6, 0.02) + _arc(0.06, 0.3, 0.06, 0.5, 3)
    return p + [(0.06, 0.5), (0.0, 0.5)]


def _bowl():
    out = [(0.0, -0.22)] + _arc(0.2, -0.22, 0.5, 0.22, 10, 0.06)
    inner = _arc(0.47, 0.22, 0.17, -0.18, 10, 0.06)
    return out + [(0.5, 0.22)] + inner + [(0.17, -0.18), (0.0, -0.18)]


def _can():
    return [(0.0, -0.5), (0.26, -0.5), (0.28, -0.47)] + _arc(0.28, -0.47, 0.28, 0.47, 8)[1:] + [(0.28, 0.47), (0.26, 0.5), (0.0, 0.5)]


def _mug():
    out = [(0.0, -0.4)] + _arc(0.33, -0.4, 0.35, 0.4, 8)
    inner = _arc(0.31, 0.4, 0.29, -0.33, 8)
    return out + [(0.35, 0.4)] + inner + [(0.29, -0.33), (0.0, -0.33)]


# ready (radius, y) outlines for lathe(), each about one unit tall or wide: NOCS-like normalised models
PROFILES = {"bottle": _bottle(), "bowl": _bowl(), "can": _can(), "mug": _mug()}


def edge_counts(faces):
    """how many faces share each undirected edge -> dict (a, b) -> count; a closed mesh has 2 everywhere"""
    e = np.sort(np.asarray(faces).reshape(-1, 3)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    keys, counts = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(keys, counts)}
