"""The exact-arithmetic referee of csrc/persistence.hip: float32 coordinates are lifted without rounding, to Python integers on
a common power-of-two grid for the predicates and to ``fractions.Fraction`` for the filtration values, so a wrong tie-break on
cospherical, coplanar or collinear points, or a value that lost its digits, cannot hide behind a float64 tolerance.

- ``check_triangulation(pc, tets)``: the tetrahedra are a Delaunay triangulation of the distinct points, every test exact;
- ``exact_filtration(pc, tets)``: tests/pd_ref.py's ``alpha_filtration`` (direct cofaces, Gabriel test, min) in rationals; its
  values go to ``pd_ref.persistence`` as they are;
- ``match(got, want, scale)``: a multiset match of (birth, death) rows, no alignment by sorting.
"""
from fractions import Fraction

import numpy as np

from tests import pd_ref
from tests.pd_ref import PAIR_RTOL               # 1e-9, the project's tolerance on a pair; here relative to the diagram's scale

PERS_FLOOR = 1e-9         # pairs with persistence <= PERS_FLOOR * scale are rounding-level and not compared


def grid_ints(pc):
    """(n, 3) float32 -> ((n, 3) object array of Python ints, den): coordinate = int / den exactly, den a power of two"""
    fr = [[Fraction(float(x)) for x in row] for row in np.asarray(pc, dtype=np.float32)]
    den = max([f.denominator for row in fr for f in row] + [1])
    out = np.empty((len(fr), 3), dtype=object)
    for i, row in enumerate(fr):
        for k, f in enumerate(row):
            out[i, k] = int(f * den)
    return out, den


def _det3(a, b, c):
    """determinant of the rows a, b, c, each (..., 3) of Python ints"""
    return (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) - a[..., 1] * (b[..., 0] * c[..., 2] - b[..., 2] * c[..., 0])
            + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))


def _orient(I, T):
    """det[b - a, c - a, d - a] of every row (a, b, c, d) of T: the kernel's orientation"""
    a = I[T[:, 0]]
    return _det3(I[T[:, 1]] - a, I[T[:, 2]] - a, I[T[:, 3]] - a)


def _insphere(I, T):
    """(T, n) determinants of rows (q - a, |q|^2 - |a|^2), q = b, c, d, e, for every tetrahedron (a, b, c, d) and every point e:
    expanded along e's row, so each tetrahedron costs four minors and each (tetrahedron, point) four products"""
    L = (I * I).sum(axis=1)
    a, la = I[T[:, 0]], L[T[:, 0]]
    rows = [np.concatenate([I[T[:, k]] - a, (L[T[:, k]] - la)[:, None]], axis=1) for k in (1, 2, 3)]
    coef = []
    for j in range(4):
        keep = [k for k in range(4) if k != j]
        m = _det3(*(r[:, keep] for r in rows))
        coef.append(m if (3 + j) % 2 == 0 else -m)
    const = -(coef[0] * a[:, 0] + coef[1] * a[:, 1] + coef[2] * a[:, 2] + coef[3] * la)
    return (const[:, None] + np.multiply.outer(coef[0], I[:, 0]) + np.multiply.outer(coef[1], I[:, 1])
            + np.multiply.outer(coef[2], I[:, 2]) + np.multiply.outer(coef[3], L))


def _inside_sign():
    """the sign _insphere gives a point strictly inside the sphere of a positively oriented tetrahedron, from one known case"""
    I = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4], [1, 1, 1], [9, 9, 9]], dtype=object)
    T = np.array([[0, 1, 2, 3]])
    assert _orient(I, T)[0] > 0
    D = _insphere(I, T)[0]
    assert D[4] != 0 and (D[5] > 0) != (D[4] > 0) and not D[:4].any()
    return 1 if D[4] > 0 else -1


INSIDE = _inside_sign()


def check_triangulation(pc, tets):
    """assert, exactly, that tets (T, 4) row indices of pc (n, 3) float32 are a Delaunay triangulation of pc's distinct points;
    -> the number of hull faces"""
    pc = np.asarray(pc, dtype=np.float32)
    T = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    assert len(T) > 0 and T.min() >= 0 and T.max() < len(pc), "tetrahedron indices"
    I, _ = grid_ints(pc)
    used = np.unique(T)
    points = {tuple(r) for r in I.tolist()}
    assert {tuple(r) for r in I[used].tolist()} == points and len(used) == len(points), "the vertices are not the distinct points"
    assert (_orient(I, T) > 0).all(), "a tetrahedron is flat or negatively oriented"
    faces = {}
    for t in T.tolist():
        for k in range(4):
            faces.setdefault(tuple(sorted(t[:k] + t[k + 1:])), []).append(t[k])
    assert max(len(o) for o in faces.values()) <= 2, "a face has more than two tetrahedra"
    inner = [(f, o) for f, o in faces.items() if len(o) == 2]
    hull = [(f, o[0]) for f, o in faces.items() if len(o) == 1]
    if inner:
        F = np.array([f for f, _ in inner])
        s1 = _orient(I, np.column_stack([F, [o[0] for _, o in inner]]))
        s2 = _orient(I, np.column_stack([F, [o[1] for _, o in inner]]))
        assert ((s1 > 0) & (s2 < 0) | (s1 < 0) & (s2 > 0)).all(), "two tetrahedra lie on the same side of a shared face"
    assert hull, "no hull face"
    F = np.array([f for f, _ in hull])
    a = I[F[:, 0]]
    u, v = I[F[:, 1]] - a, I[F[:, 2]] - a
    nrm = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    side = I[used].dot(nrm.T) - (nrm * a).sum(axis=1)[None, :]                    # (points, hull faces)
    own = ((I[[o for _, o in hull]] - a) * nrm).sum(axis=1)
    assert (own != 0).all()
    flip = np.where(own > 0, 1, -1).astype(object)
    assert (side * flip[None, :] >= 0).all(), "a point lies outside a boundary face: the union is not the convex hull"
    D = _insphere(I, T)[:, used]
    assert (D * INSIDE <= 0).all(), "a point lies strictly inside a circumsphere"
    return len(hull)


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _sphere(P, s):
    """smallest circumsphere of the simplex s on integer points: (base a, N, den) with centre a + N / den, squared radius
    |N|^2 / den^2"""
    a = P[s[0]]
    U = [[P[i][k] - a[k] for k in range(3)] for i in s[1:]]
    if len(s) == 2:
        return a, U[0], 2
    if len(s) == 3:
        u, v = U
        w = _cross(u, v)
        x, y = _cross(v, w), _cross(w, u)
        uu, vv = _dot(u, u), _dot(v, v)
        return a, [uu * x[k] + vv * y[k] for k in range(3)], 2 * _dot(w, w)
    u, v, w = U
    x, y, z = _cross(v, w), _cross(w, u), _cross(u, v)
    uu, vv, ww = _dot(u, u), _dot(v, v), _dot(w, w)
    return a, [uu * x[k] + vv * y[k] + ww * z[k] for k in range(3)], 2 * _dot(u, x)


def exact_filtration(pc, tets):
    """pd_ref.alpha_filtration in exact arithmetic: dict simplex (sorted tuple of pc's row indices) -> Fraction"""
    I, gden = grid_ints(pc)
    P = I.tolist()
    tets = [tuple(sorted(t)) for t in np.asarray(tets).reshape(-1, 4).tolist()]
    cof = {}
    for t in tets:
        for k in range(4):
            cof.setdefault(t[:k] + t[k + 1:], []).append(t)
    for f in [f for f in cof if len(f) == 3]:
        for k in range(3):
            cof.setdefault(f[:k] + f[k + 1:], []).append(f)

    def r2_of(N, den):
        return Fraction(_dot(N, N), den * den * gden * gden)

    val = {}
    for t in tets:
        _, N, den = _sphere(P, t)
        val[t] = r2_of(N, den)
    for dim in (2, 1):
        for s in [s for s in cof if len(s) == dim + 1]:
            a, N, den = _sphere(P, s)
            gabriel = True
            for p in {v for f in cof[s] for v in f} - set(s):
                q = [P[p][k] - a[k] for k in range(3)]
                # |q - N / den|^2 >= |N / den|^2  <=>  (|q|^2 den - 2 q.N) den >= 0
                if (_dot(q, q) * den - 2 * _dot(q, N)) * den < 0:
                    gabriel = False
                    break
            m = min(val[f] for f in cof[s])
            val[s] = min(r2_of(N, den), m) if gabriel else m
    for v in {v for t in tets for v in t}:
        val[(v,)] = Fraction(0)
    return val


_diagram_cache = {}


def exact_diagram(pc, tets):
    """{1: H1, 2: H2} float64 (k, 2) pairs of the exact filtration on the given triangulation (kept per (cloud, triangulation):
    the CPU and the GPU tests of one session ask for the same ones)"""
    pc = np.ascontiguousarray(pc, dtype=np.float32)
    T = np.sort(np.asarray(tets, dtype=np.int64).reshape(-1, 4), axis=1)
    T = np.ascontiguousarray(T[np.lexsort(T.T[::-1])])
    key = (pc.tobytes(), T.tobytes())
    if key not in _diagram_cache:
        dg = pd_ref.persistence(exact_filtration(pc, T))
        _diagram_cache[key] = {1: dg[1], 2: dg[2]}
    return _diagram_cache[key]


def kept(pairs, scale):
    """the rows whose persistence exceeds the relative floor"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    return pairs[(pairs[:, 1] - pairs[:, 0]) > PERS_FLOOR * scale]


def match(got, want, scale):
    """multiset match of the kept rows of got against those of want, each within PAIR_RTOL * scale in birth and in death;
    -> (unmatched rows of got, unmatched rows of want), both empty when the diagrams agree"""
    g, w = kept(got, scale), kept(want, scale)
    free = np.ones(len(g), dtype=bool)
    lone = []
    for row in w:
        err = np.abs(g - row).max(axis=1) if len(g) else np.zeros(0)
        err[~free] = np.inf
        k = int(np.argmin(err)) if len(err) else -1
        if k >= 0 and err[k] <= PAIR_RTOL * scale:
            free[k] = False
        else:
            lone.append(row)
    return g[free], np.asarray(lone, dtype=np.float64).reshape(-1, 2)
