"""The adversarial clouds of the persistence tests, shared by tests/test_pd_exact_cpu.py (the stand-alone host build of
csrc/persistence.hip) and tests/test_pd_exact_gpu.py (the kernel).  Deterministic: fixed seeds, and every constructed coordinate
is a small integer times a power of two, so float32 holds it exactly.

EXACT    name -> (tetrahedra or None, kept H1 pairs, kept H2 pairs): the clouds (<= 200 points) whose triangulation and diagram
         are checked with tests/pd_exact.py.  The pair counts are what the exact diagram keeps above pd_exact's relative floor
         (they do not depend on how ties are triangulated); the kernel must keep as many.  A tetrahedron count is listed where
         the geometry fixes it.
STATUS   name -> (status, tetrahedra or None, (H1 pairs, H2 pairs)): status and counts only, every reported pair counted.  The
         predicates are exact and the symbolic perturbation depends on the rows alone, so the counts of a passing cloud are
         deterministic; those listed are also the numbers of pairs of non-zero length in the exact rational diagram on the same
         triangulation.
"""
import numpy as np

ETETS, ERANGE, EFLAT = 1, 6, 7
MAX_TETS = 8192

EXACT = {
    "cosphere": (None, 163, 1),
    "cosphere_centre": (None, 189, 95),
    "pyramid": (None, 124, 1),
    "pyramid_off": (None, 124, 1),
    "prism": (None, 65, 1),
    "skew24": (23 * 23, 3, 1),
    "collinear_first": (None, 1, 0),
    "moment40": (703, 0, 0),
    "four": (1, 0, 0),
    "offset_cluster": (None, 442, 194),
    "ulp_twins_centred": (None, 181, 69),
    "ulp_twins_at_1m": (None, 181, 69),
    "ulp_triplets_centred": (None, 181, 69),
    "ulp_triplets_at_1m": (None, 181, 69),
}
# two 4 x 4 x 4 lattices: 81 H1 and 27 H2 pairs each (the lattice's squares and cubes); at k >= 28 the small lattice's pairs,
# ~2^-2k, lie below the floor that the large one's scale (0.75 * 2^-24) sets
for _k, _h1, _h2 in ((16, 162, 54), (24, 162, 54), (28, 81, 27), (32, 81, 27)):
    EXACT["two_scales%d" % _k] = (None, _h1, _h2)
    EXACT["two_scales%d_rev" % _k] = (None, _h1, _h2)

STATUS = {
    "n1": (EFLAT, 0, (0, 0)),
    "n2": (EFLAT, 0, (0, 0)),
    "n3": (EFLAT, 0, (0, 0)),
    "skew89": (0, 88 * 88, (3, 1)),      # 7744 finite tetrahedra: with the hull's ghost slots the largest that fits
    "skew90": (ETETS, None, (0, 0)),
    "skew512": (ETETS, None, (0, 0)),
    "moment200": (ETETS, None, (0, 0)),
    "moment1024": (ETETS, None, (0, 0)),
    "nan": (ERANGE, 0, (0, 0)),
    "inf": (ERANGE, 0, (0, 0)),
    "denormal": (ERANGE, 0, (0, 0)),
    "off_grid": (ERANGE, 0, (0, 0)),
    "on_grid": (0, 309, (108, 44)),
    "circle_poles": (0, 1112, (656, 192)),
}


def _sphere_points():
    pts = [(x, y, z) for x in range(-65, 66) for y in range(-65, 66) for z in range(-65, 66) if x * x + y * y + z * z == 65 * 65]
    pts = np.array(pts, dtype=np.float64)
    np.random.RandomState(11).shuffle(pts)
    return pts


def _skew(a, b):
    """a points on the x axis and b on a skew line: every tetrahedron joins an edge of one line to an edge of the other"""
    l1 = np.stack([np.arange(a), np.zeros(a), np.zeros(a)], axis=1)
    l2 = np.stack([np.zeros(b) + 3.5, np.arange(b) - 7.25, np.zeros(b) + 5.0], axis=1)
    return np.concatenate([l1, l2]) / 64


def _moment(n):
    t = np.arange(1, n + 1, dtype=np.float64)
    return np.stack([t, t * t, t * t * t], axis=1) / 65536


def _lattice4():
    g = np.arange(4)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)


def _two_scales(k):
    lat = _lattice4()
    return np.concatenate([lat * 2.0 ** -k, lat * 2.0 ** -12 + 0.5])


def _ulp(kind, offset):
    rng = np.random.RandomState(5)
    base = (rng.uniform(-0.05, 0.05, (96, 3)).astype(np.float32) + np.asarray(offset, dtype=np.float32)).astype(np.float32)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    if kind == "twins":
        twin = base[:32].copy()
        ax = rng.randint(0, 3, 32)
        twin[np.arange(32), ax] = np.nextafter(twin[np.arange(32), ax], up)
        return np.concatenate([base, twin])
    return np.concatenate([base, np.nextafter(base[:32], up), np.nextafter(base[:32], down)])


def _base64():
    """64 points with the largest magnitude in [0.5, 1): frexp exponent 0, so the exact grid is 2^-60"""
    pc = np.random.RandomState(3).uniform(-0.45, 0.45, (64, 3)).astype(np.float32)
    pc[0] = (0.75, -0.25, 0.125)
    return pc


def _with(value):
    pc = _base64()
    pc[17, 1] = value
    return pc


def _circle_poles():
    th = np.arange(600) * (2 * np.pi / 600)
    ring = np.stack([np.round(np.cos(th) * 4000), np.round(np.sin(th) * 4000), 0 * th], axis=1)
    return np.concatenate([ring, [[0, 0, 3000], [0, 0, -3000]]]) / 65536


def _build(name):
    if name == "cosphere":
        return _sphere_points()[:160] / 1024
    if name == "cosphere_centre":
        return np.concatenate([_sphere_points()[:96], [[0, 0, 0]]]) / 1024
    if name in ("pyramid", "pyramid_off"):
        g = np.arange(12)
        X, Y = np.meshgrid(g, g, indexing="ij")
        pc = np.concatenate([np.stack([X, Y, 0 * X], -1).reshape(-1, 3), [[5.5, 5.5, 7]]]) / 256.0
        return pc + np.array([0.25, -0.5, 1.5]) if name == "pyramid_off" else pc
    if name == "prism":
        th = np.arange(64) * (2 * np.pi / 64)
        return np.concatenate([np.stack([np.round(np.cos(th) * 1000), np.round(np.sin(th) * 1000), z + 0 * th], axis=1) for z in (0, 300)]) / 8192
    if name.startswith("skew"):
        return _skew(int(name[4:]), int(name[4:]))
    if name == "collinear_first":
        d = np.arange(40)
        return np.concatenate([np.stack([d, d, d], axis=1), [[3, 1, 0], [7, 2, 30]]]) / 128.0
    if name.startswith("moment"):
        return _moment(int(name[6:]))
    if name == "four":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) / 8.0
    if name in ("n1", "n2", "n3"):
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]])[: int(name[1])] / 8.0
    if name == "offset_cluster":
        return np.array([0.3, -0.2, 1.5]) + 2e-5 * np.random.RandomState(13).normal(size=(200, 3))
    if name.startswith("ulp_"):
        _, kind, where = name.split("_", 2)
        return _ulp(kind, (0.0, 0.0, 0.0) if where == "centred" else (0.2, -0.1, 1.0))
    if name.startswith("two_scales"):
        pc = _two_scales(int(name[10:12]))
        return pc[::-1] if name.endswith("_rev") else pc
    if name == "base64":
        return _base64()
    if name == "nan":
        return _with(np.nan)
    if name == "inf":
        return _with(np.inf)
    if name == "denormal":
        return _with(2.0 ** -130)
    if name == "off_grid":
        return _with(1.5 * 2.0 ** -60)            # a multiple of 2^-61 only
    if name == "on_grid":
        return _with(2.0 ** -60)
    if name == "flat64":
        pc = _base64()
        pc[:, 2] = 0.25
        return pc
    if name == "circle_poles":
        return _circle_poles()
    raise KeyError(name)


_clouds = {}


def cloud(name):
    """(n, 3) float32, C-contiguous; the same array every time (treat it as read-only)"""
    if name not in _clouds:
        pc = np.ascontiguousarray(np.asarray(_build(name), dtype=np.float64).astype(np.float32))
        pc.setflags(write=False)
        _clouds[name] = pc
    return _clouds[name]


# one same-size batch that mixes failing and passing clouds: (name, status)
MIXED = (("base64", 0), ("nan", ERANGE), ("on_grid", 0), ("flat64", EFLAT), ("inf", ERANGE), ("base64", 0), ("off_grid", ERANGE),
         ("denormal", ERANGE))
