"""A float64 restatement of the reference's datasets/compute_pd.py, written independently of csrc/persistence.hip.

compute_pd builds a gudhi AlphaComplex of the cloud, takes its persistence diagram and turns H1 and H2 into 50 x 50 legacy
persim PersImage images.  Neither library is installed here, so this module restates their documented behaviour (DESIGN.md
section 3, "Ground-truth persistence images"); parity with gudhi and persim themselves is unverified.

- points: float32 promoted to float64, exact duplicates removed (the first occurrence stays), as CGAL's triangulation does;
- the alpha filtration on scipy's Delaunay triangulation: a simplex is Gabriel when no vertex of a Delaunay coface lies strictly
  inside its smallest circumsphere; a Gabriel simplex takes its squared smallest-circumsphere radius, any other simplex the minimum
  value over its cofaces, a vertex 0.  Every value is then also capped by its cofaces' values (a no-op in exact arithmetic; it keeps
  faces before cofaces when two rounded radii of the same sphere differ in the last bit).  Spheres are evaluated from the
  simplex's shortest edge (``_near_order``), so a value does not depend on the row order of the cloud; the arithmetic stays plain
  float64 (tests/pd_exact.py is the exact referee);
- persistence over Z/2 by a plain boundary-matrix reduction in (value, dimension, index) order, pairs with death > birth, no
  infinite deaths;
- the image as persim's legacy PersImage(spread=1e-2, pixels=[50, 50]) with one object for both dimensions.
"""
import numpy as np
from scipy.spatial import Delaunay
from scipy.stats import norm

PIXELS = 50
SPREAD = 1e-2
# the tests' tolerances on the kernel against this restatement: a pair's birth and death (relative), an image pixel (absolute)
PAIR_RTOL, IMG_ATOL = 1e-9, 1e-6


def unique_points(pcl):
    """(n, 3) float32 -> (U, 3) float64 of the first occurrences, and their row indices"""
    P = np.asarray(pcl, dtype=np.float32).astype(np.float64)
    _, first = np.unique(P, axis=0, return_index=True)
    first = np.sort(first)
    return P[first], first


def delaunay_tets(P):
    """scipy's Delaunay tetrahedra (index rows into P); zero-volume simplices of a degenerate input's triangulated facets dropped"""
    tri = Delaunay(P)
    T = np.sort(tri.simplices, axis=1)
    a, b, c, d = (P[T[:, k]] for k in range(4))
    vol = np.einsum("ij,ij->i", b - a, np.cross(c - a, d - a))
    return T[vol != 0]


def _near_order(A):
    """rows of A reordered: an endpoint of the shortest edge first (the base of the differences), the edge's other endpoint,
    then the rest by distance from the base.  Based at a far vertex the cross products of two nearly equal long differences
    cancel, and the centre of a simplex with two close vertices and a distant one loses the digits the Gabriel tests need."""
    n = len(A)
    d = ((A[:, None, :] - A[None, :, :]) ** 2).sum(-1)
    i, j = min(((i, j) for i in range(n) for j in range(i + 1, n)), key=lambda ij: d[ij])
    rest = sorted((k for k in range(n) if k not in (i, j)), key=lambda k: d[i, k])
    return A[[i, j] + rest]


def _sphere(P, s):
    """smallest circumsphere (centre, squared radius) of the simplex s (2, 3 or 4 vertex indices); the value does not depend on
    the order of s beyond rounding"""
    A = P[list(s)]
    if len(s) > 2:
        A = _near_order(A)
    if len(s) == 2:
        c = (A[0] + A[1]) * 0.5
        d = A[0] - A[1]
        return c, float(d @ d) * 0.25
    a = A[0]
    U = A[1:] - a
    if len(s) == 3:
        u, v = U
        w = np.cross(u, v)
        o = (np.dot(u, u) * np.cross(v, w) + np.dot(v, v) * np.cross(w, u)) / (2.0 * np.dot(w, w))
    else:
        u, v, w = U
        o = (np.dot(u, u) * np.cross(v, w) + np.dot(v, v) * np.cross(w, u) + np.dot(w, w) * np.cross(u, v)) / (2.0 * np.dot(u, np.cross(v, w)))
    return a + o, float(o @ o)


def alpha_filtration(P, tets):
    """-> dict simplex (sorted tuple) -> value, for every face of every tetrahedron (vertices 0)"""
    cof = {}                     # simplex -> its direct cofaces
    for t in map(tuple, tets):
        for k in range(4):
            f = t[:k] + t[k + 1:]
            cof.setdefault(f, []).append(t)
    for f in [f for f in cof if len(f) == 3]:
        for k in range(3):
            cof.setdefault(f[:k] + f[k + 1:], []).append(f)
    val = {tuple(t): _sphere(P, t)[1] for t in map(tuple, tets)}
    for dim in (2, 1):
        for s in [s for s in cof if len(s) == dim + 1]:
            c, r2 = _sphere(P, s)
            verts = {v for f in cof[s] for v in f} - set(s)
            gabriel = all(float((P[v] - c) @ (P[v] - c)) >= r2 for v in verts)
            m = min(val[f] for f in cof[s])
            val[s] = min(r2, m) if gabriel else m
    for v in {v for t in tets for v in t}:
        val[(int(v),)] = 0.0
    return val


def persistence(val):
    """plain Z/2 reduction of the whole boundary matrix -> {dim: (k, 2) float64 (birth, death) with death > birth}"""
    order = sorted(val, key=lambda s: (val[s], len(s), s))
    index = {s: i for i, s in enumerate(order)}
    pivot = {}
    pairs = {0: [], 1: [], 2: []}
    for j, s in enumerate(order):
        if len(s) == 1:
            continue
        col = {index[s[:k] + s[k + 1:]] for k in range(len(s))}
        while col:
            low = max(col)
            if low not in pivot:
                break
            col ^= pivot[low]
        if col:
            low = max(col)
            pivot[low] = col
            b, d = val[order[low]], val[s]
            if d > b:
                pairs[len(s) - 2].append((b, d))
    return {k: np.asarray(v, dtype=np.float64).reshape(-1, 2) for k, v in pairs.items()}


def diagrams(pcl):
    """the H1 and H2 diagrams of a cloud, each sorted by (birth, death)"""
    P, _ = unique_points(pcl)
    dg = persistence(alpha_filtration(P, delaunay_tets(P)))
    return [dg[k][np.lexsort((dg[k][:, 1], dg[k][:, 0]))] for k in (1, 2)]


class PersImage(object):
    """legacy persim PersImage(spread=1e-2, pixels=[50, 50]) with the default linear weighting; the ranges ("specs") are set by
    the first transform of a non-empty diagram and kept"""

    def __init__(self, spread=SPREAD, pixels=PIXELS):
        self.spread, self.n, self.specs = spread, pixels, None

    def transform(self, dgm):
        dgm = np.asarray(dgm, dtype=np.float64).reshape(-1, 2)
        if len(dgm) == 0:
            return np.zeros((self.n, self.n))
        land = np.stack([dgm[:, 0], dgm[:, 1] - dgm[:, 0]], axis=1)             # (birth, persistence)
        if self.specs is None:
            self.specs = {"maxBD": max(float(land.max()), 0.0), "minBD": min(float(land.min()), 0.0)}
        maxBD, minBD = self.specs["maxBD"], min(self.specs["minBD"], 0.0)
        dx = maxBD / self.n
        xl = np.linspace(minBD, maxBD, self.n)
        yl = np.linspace(0, maxBD, self.n)
        xu, yu = xl + dx, yl + dx
        maxy = land[:, 1].max()
        img = np.zeros((self.n, self.n))
        for b, p in land:
            xs = norm.cdf(xu, b, self.spread) - norm.cdf(xl, b, self.spread)
            ys = norm.cdf(yu, p, self.spread) - norm.cdf(yl, p, self.spread)
            img += np.outer(xs, ys) * ((1 / maxy) * p)
        return img.T[::-1]


def images(h1, h2):
    """compute_pd's two images (2500,) float32 from the two diagrams"""
    pim = PersImage()
    out = []
    for dgm in (h1, h2):
        if len(dgm):
            im = pim.transform(dgm).astype(np.float32)
            im = im / (im.max() + np.float32(1e-20))
        else:
            im = np.zeros((PIXELS, PIXELS), dtype=np.float32)
        out.append(np.ascontiguousarray(im, dtype=np.float32).reshape(-1))
    return out


def compute_pd(pcl):
    """-> (pdh1, pdh2, h1, h2)"""
    h1, h2 = diagrams(pcl)
    return (*images(h1, h2), h1, h2)
