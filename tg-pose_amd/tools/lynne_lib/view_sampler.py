"""View-sphere sampling under the reference's names (``tools/lynne_lib/view_sampler.py``: ``hinter_sampling``, ``sample_views``), and
``rotation_grid``, the rotation table ops.pose_search tries (DESIGN.md section 3 "Model-based acquisition").

The reference's module cannot be imported where it stands (it needs a ``tools.transform`` its tree does not hold); its one use of
that module, a half turn about x, is ``diag(1, -1, -1)`` here.  Same point order, same return types; tests/golden/view_sampler_ref.npz
holds what the reference returns for 12, 42 and 162 views (tests/golden/make_view_sampler_golden.py).  Host code, float64.
"""
import math

import numpy as np

_G = (1.0 + math.sqrt(5.0)) / 2.0
# the icosahedron: the three golden rectangles' corners, and its 20 faces
_ICO_POINTS = ((-1.0, _G, 0.0), (1.0, _G, 0.0), (-1.0, -_G, 0.0), (1.0, -_G, 0.0), (0.0, -1.0, _G), (0.0, 1.0, _G),
               (0.0, -1.0, -_G), (0.0, 1.0, -_G), (_G, 0.0, -1.0), (_G, 0.0, 1.0), (-_G, 0.0, -1.0), (-_G, 0.0, 1.0))
_ICO_FACES = ((0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
              (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1))
_FLIP_YZ = np.diag([1.0, -1.0, -1.0])           # OpenGL camera axes -> OpenCV camera axes: a half turn about x


def _split(points, faces, levels, level):
    """every triangle into four: a new point on the middle of each edge (shared by the two triangles of the edge)"""
    middle, out = {}, []
    for a, b, c in faces:
        mids = []
        for u, v in ((a, b), (b, c), (c, a)):
            key = (u, v) if u < v else (v, u)
            if key not in middle:
                middle[key] = len(points)
                points.append((0.5 * (np.array(points[key[0]]) + np.array(points[key[1]]))).tolist())
                levels.append(level)
            mids.append(middle[key])
        ab, bc, ca = mids
        out += [(a, ab, ca), (ab, b, bc), (ab, bc, ca), (ca, bc, c)]
    return out


def _azimuth(x, y):
    return (math.atan2(y, x) + 2.0 * math.pi) % (2.0 * math.pi)


def hinter_sampling(min_n_pts, radius=1):
    """Points on a sphere by refining an icosahedron until it has at least ``min_n_pts`` corners (Hinterstoisser et al., BMVC 2008):
    12, 42, 162, 642, ...  -> (pts (n,3) float64 on the sphere of ``radius``, pts_level: the refinement level that made each point,
    a list).  Order: from the top point (largest z) outwards, ring by ring of the mesh, each ring by azimuth."""
    points, levels, faces = [list(p) for p in _ICO_POINTS], [0] * len(_ICO_POINTS), list(_ICO_FACES)
    level = 0
    while len(points) < min_n_pts:
        level += 1
        faces = _split(points, faces, levels, level)
    pts = np.array(points)
    pts *= (radius / np.linalg.norm(pts, axis=1)).reshape(-1, 1)

    linked = {}
    for face in faces:
        for k in range(3):
            linked.setdefault(face[k], set()).add(face[(k + 1) % 3])
            linked[face[k]].add(face[(k + 2) % 3])
    order, seen = [], [False] * len(pts)
    ring = [int(np.argmax(pts[:, 2]))]
    while len(order) != len(pts):
        ring = sorted(ring, key=lambda i: _azimuth(pts[i][0], pts[i][1]))
        reached = []
        for i in ring:
            order.append(i)
            seen[i] = True
            reached += [j for j in linked[i]]
        ring = [j for j in set(reached) if not seen[j]]
    return pts[np.array(order), :], [levels[i] for i in order]


def sample_views(min_n_views, radius=1, azimuth_range=(0, 2 * math.pi), elev_range=(-0.5 * math.pi, 0.5 * math.pi)):
    """Cameras on the view sphere looking at the origin -> (views: a list of {'R' (3,3), 't' (3,1)} with x_cam = R x + t, OpenCV axes
    (z forward, y down), pts_level as hinter_sampling returns it, for ALL points).  A point outside the azimuth or elevation range
    gives no view."""
    pts, pts_level = hinter_sampling(min_n_views, radius=radius)
    views = []
    for pt in pts:
        azimuth = math.atan2(pt[1], pt[0])
        if azimuth < 0:
            azimuth += 2.0 * math.pi
        elev = math.acos(np.linalg.norm([pt[0], pt[1], 0]) / np.linalg.norm(pt))
        if pt[2] < 0:
            elev = -elev
        if not (azimuth_range[0] <= azimuth <= azimuth_range[1] and elev_range[0] <= elev <= elev_range[1]):
            continue
        forward = -np.array(pt)
        forward /= np.linalg.norm(forward)
        side = np.cross(forward, np.array([0.0, 0.0, 1.0]))
        if np.count_nonzero(side) == 0:          # looking along z: any side will do, x is taken
            side = np.array([1.0, 0.0, 0.0])
        side /= np.linalg.norm(side)
        up = np.cross(side, forward)
        R = _FLIP_YZ.dot(np.array([side, up, -forward]))
        views.append({'R': R, 't': -R.dot(np.array(pt).reshape((3, 1)))})
    return views, pts_level


def rotation_grid(min_n_views, n_inplane):
    """Every view rotation of sample_views(min_n_views) times ``n_inplane`` rotations about the optical axis, views outer:
    rotation v * n_inplane + k = Rz(2 pi k / n_inplane) R_v -> (R,3,3) float32 (products in float64, rounded once)."""
    if not (isinstance(n_inplane, int) and n_inplane >= 1):
        raise ValueError("rotation_grid: n_inplane must be an int >= 1")
    views, _ = sample_views(min_n_views)
    out = []
    for v in views:
        for k in range(n_inplane):
            a = 2.0 * math.pi * k / n_inplane
            c, s = math.cos(a), math.sin(a)
            out.append(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]).dot(v['R']))
    return np.stack(out).astype(np.float32)
