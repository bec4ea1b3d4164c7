"""numpy restatement of the mesh surface sampling contract (include/tgpose.h tgp_mesh_area_cdf / tgp_mesh_sample; DESIGN.md section 3
"Mesh surface sampling"; the reference's network/point_sample/pc_sample_sphere.py:125-169), float64 on float32 vertices, every
product and sum rounded on its own.

    cross = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x),  norm = sqrt((c_x c_x + c_y c_y) + c_z c_z),  area = norm / 2
    cdf: chunks of CHUNK faces; a serial sum inside a chunk, a serial sum of the chunk totals in front of it
    face = first f with cdf[f] >= u * cdf[F - 1], clamped to F - 1
    point = ((1 - s) v0 + (s (1 - r2)) v1) + (s r2) v2, s = sqrt(r1);  normal = cross / norm

tests/golden/mesh_sample_ref.npz holds what the reference itself returned (tests/golden/make_mesh_sample_golden.py)."""
import numpy as np

CHUNK = 64          # TGP_MESH_AREA_CHUNK
SITE = 8            # TGP_MESH_SITE


def corners(verts, faces):
    """(F, 3 corners, 3) float64 of the float32 vertices"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    return v[np.asarray(faces, dtype=np.int64)]


def cross_norm(tri):
    a, b = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return c, np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def area_cdf(verts, faces, chunk=CHUNK):
    """the cumulative area in the kernel's order (np.cumsum and np.add.accumulate add serially)"""
    area = 0.5 * cross_norm(corners(verts, faces))[1]
    F = len(area)
    C = -(-F // chunk)
    local = np.cumsum(np.concatenate([area, np.zeros(C * chunk - F)]).reshape(C, chunk), axis=1)
    tot = local[:, -1]                                      # the padding adds 0.0: the last chunk's total is its last live prefix
    off = np.concatenate([[0.0], np.cumsum(tot[:-1])]) if C > 1 else np.zeros(1)
    return (off[:, None] + local).reshape(-1)[:F]


def search(cdf, x):
    """the kernel's binary search, element-wise: the first f with cdf[f] >= x, clamped to F - 1 (a NaN x gives 0)"""
    F = len(cdf)
    lo, hi = np.zeros(len(x), dtype=np.int64), np.full(len(x), F, dtype=np.int64)
    while (lo < hi).any():
        live = lo < hi
        mid = lo + ((hi - lo) >> 1)
        less = cdf[np.minimum(mid, F - 1)] < x
        lo = np.where(live & less, mid + 1, lo)
        hi = np.where(live & ~less, mid, hi)
    return np.minimum(lo, F - 1)


def device_uniforms(seed, key, n):
    """(n, 3) float64: the draws tgp_mesh_sample makes for a job keyed ``key`` under ``seed``"""
    from tgpose_amd.datasets import device_draws as dd
    w = dd.philox_words(seed, [key], SITE, np.arange(2 * n))[0].reshape(n, 2, 4)
    return np.stack([dd.uniform_f64(w[:, 0, 0], w[:, 0, 1]), dd.uniform_f64(w[:, 0, 2], w[:, 0, 3]), dd.uniform_f64(w[:, 1, 0], w[:, 1, 1])], 1)


def sample(verts, faces, u, cdf=None):
    """u (n, 3) float64 -> points+normals (n, 6) float64, face (n,) int32, status (0, or 1 without a positive finite area)"""
    tri = corners(verts, faces)
    cdf = area_cdf(verts, faces) if cdf is None else cdf
    total = cdf[-1]
    status = 0 if (total > 0 and np.isfinite(total)) else 1
    u = np.asarray(u, dtype=np.float64).reshape(-1, 3)
    face = search(cdf, u[:, 0] * total)
    t = tri[face]
    s = np.sqrt(u[:, 1])
    w0, w1, w2 = (1 - s)[:, None], (s * (1 - u[:, 2]))[:, None], (s * u[:, 2])[:, None]
    pts = (w0 * t[:, 0] + w1 * t[:, 1]) + w2 * t[:, 2]
    c, nrm = cross_norm(t)
    with np.errstate(invalid="ignore", divide="ignore"):
        normal = c / nrm[:, None]
    return np.concatenate([pts, normal], 1), face.astype(np.int32), status


def barycentric(verts, faces, face, points):
    """the three weights of each sample, solved from its point and its face's corners (least squares in the face's plane)"""
    t = corners(verts, faces)[face]
    a, b, d = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], np.asarray(points, dtype=np.float64) - t[:, 0]
    aa, ab, bb, da, db = (a * a).sum(1), (a * b).sum(1), (b * b).sum(1), (d * a).sum(1), (d * b).sum(1)
    det = aa * bb - ab * ab
    w1, w2 = (da * bb - db * ab) / det, (db * aa - da * ab) / det
    return np.stack([1 - w1 - w2, w1, w2], 1)


# the distribution test of the device draws (tests/test_mesh_sample_gpu.py): the box, one job; the seed is committed after the
# restatement passed with it (tests/test_mesh_sample_cpu.py), and the kernel equals the restatement bit for bit
DIST_SEED, DIST_KEY, DIST_N = 2024, 0, 65536


def distribution_draws(v, f):
    """the restatement's (face, points) of the test's draws"""
    out, face, _ = sample(v, f, device_uniforms(DIST_SEED, DIST_KEY, DIST_N))
    return face, out[:, :3]


def distribution_statistics(v, f, face, points):
    """chi-square of the per-face counts against the areas (F - 1 degrees of freedom); within the largest face, |mean barycentric
    weight - 1/3| per corner and its bound 4 / sqrt(count)"""
    area = 0.5 * cross_norm(corners(v, f))[1]
    n = len(face)
    counts = np.bincount(face, minlength=len(f)).astype(np.float64)
    expect = n * area / area.sum()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    big = int(np.argmax(area))
    w = barycentric(v, f, face[face == big], points[face == big])
    return chi2, np.abs(w.mean(0) - 1.0 / 3.0), 4.0 / np.sqrt(len(w))
