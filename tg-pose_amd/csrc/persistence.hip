// Ground-truth persistence images of the training clouds (the reference's datasets/compute_pd.py): the alpha complex of each
// cloud, its H1 / H2 persistence pairs, and the legacy persim PersImage(spread=1e-2, pixels=[50, 50]) of each dimension.
// Two launches per batch, no host round trip:
//   pd_diagram_kernel  one workgroup per cloud: dedup + Morton order (all lanes), incremental Bowyer-Watson Delaunay with exact
//                      predicates (lane 0), simplices and alpha values (all lanes), sorts (all lanes), H0 / H2 union-find and H1
//                      column reduction (lane 0) -> padded pairs + counts + status
//   pd_image_kernel    one workgroup per (cloud, dimension): the 50 x 50 image from the pairs, normalised to max 1
//
// The per-cloud algorithm (pd_run) is written for `nt` cooperating lanes: strided loops, lane-0 sections, PD_SYNC() between
// them.  With nt = 1 on the host it is the same computation serially (PD_SYNC() is then nothing): tests/host/pd_host.cpp
// builds exactly that as a stand-alone program.  tests/test_pd_exact_cpu.py runs it, also under the address and undefined-
// behaviour sanitizers, and checks its triangulations and diagrams with exact integer and rational arithmetic;
// tests/test_pd_exact_gpu.py finds the kernel's status, tetrahedra and pair bits equal to that program's on every test cloud.
//
// Values.  A simplex's filtration value is the squared radius of its smallest circumsphere, evaluated in double-double
// arithmetic (~2^-100) from the simplex's shortest edge and rounded once to float64, and the Gabriel tests compare
// double-doubles.  The evaluation is accurate to ~2^-100, not exact: a value depends on the order of the simplex's vertices
// far below float64's rounding, and two simplices with the same sphere get the same float64 unless the true value lies that
// close to a rounding boundary.  So a pair of zero length in exact arithmetic is almost never reported (none is on the test
// clouds), but that is not guaranteed; nor is the direction in which a true length below half an ulp rounds.  Against the exact rational diagram the pairs agree within 1e-9 of the diagram's
// largest death, also for clusters 2^-32 wide beside coordinates of 0.5.
//
// Exactness.  Coordinates are float32; promoted to float64 they are integers on the grid 2^G, G = (top exponent of the cloud) - 60,
// unless a coordinate is below ~1e-11 of the cloud's extent (then the status is TGP_PD_ERANGE).  orient3d / insphere first run
// in float64 with Shewchuk's forward error bounds (o3derrboundA, isperrboundA); when the bound does not decide, the same
// polynomial is evaluated exactly on the grid integers in 384-bit two's complement (differences < 2^61, the insphere
// determinant < 2^313).  Exact ties (cospherical, coplanar-on-the-hull) are broken by the symbolic perturbation of Devillers and
// Teillaud (perturbations for Delaunay triangulations in 3D): points ranked lexicographically, the lifted coordinate perturbed by
// rank.  So every predicate answers consistently and every cloud with 4 affinely independent points gets a valid Delaunay
// triangulation.  Every data-dependent loop has a bound; running out of a capacity sets the cloud's status word and stops that
// cloud (its pairs count 0, its images zero).
#include "tgp_common.h"
#include <math.h>

#define PD_HD __host__ __device__
#ifdef __HIP_DEVICE_COMPILE__
#define PD_SYNC() __syncthreads()
#else
#define PD_SYNC() ((void)0)
#endif

namespace pd {

constexpr int NMAX = TGP_PD_MAX_POINTS;
constexpr int TCAP = TGP_PD_MAX_TETS;          // tetrahedron slots, finite + ghost (infinite vertex)
constexpr int FCAP = 2 * TCAP;                  // triangles
constexpr int ECAP = TCAP + NMAX;               // edges
constexpr int SCAP = 2 * TCAP;                  // sort buffer (power of two >= FCAP)
constexpr int CCAP = 2048;                      // cavity tetrahedra per insertion
constexpr int BCAP = 4096;                      // cavity boundary faces per insertion
constexpr int PAIRCAP = TGP_PD_MAX_PAIRS;
constexpr int POOLCAP = 1 << 17;                // stored reduced H1 columns (edge ranks)
constexpr int WCAP = 2048;                      // one column during its reduction
constexpr int RING_CAP = 4096;                  // tetrahedra around one edge
constexpr int WALK_CAP = 4 * TCAP;
constexpr int INF_V = NMAX;                     // the infinite vertex
constexpr int DEAD = -2;
constexpr int THREADS = 256;

static_assert((SCAP & (SCAP - 1)) == 0 && SCAP >= FCAP && SCAP >= ECAP, "sort buffer");

// ---- the per-cloud workspace: one fixed layout, all offsets in bytes --------------------------------------------------------
struct Layout {
    size_t P, I, vid, key, ord, tv, tn, mark, freel, cav, bnd, pend, tval, fin, tri_of, tri, tri_c, fval, edge, eval,
        skey, sidx, erank, eord, epos, tet_edge, uf, rep, fneg, pcol, pool, work, work2, total;
};
PD_HD inline Layout layout()
{
    Layout L;
    size_t o = 0;
    auto take = [&o](size_t bytes) { size_t r = o; o += (bytes + 255) & ~size_t(255); return r; };
    L.P = take(sizeof(double) * 3 * NMAX);
    L.I = take(sizeof(int64_t) * 3 * NMAX);
    L.vid = take(sizeof(int) * NMAX);
    L.key = take(sizeof(uint64_t) * NMAX);
    L.ord = take(sizeof(int) * NMAX);
    L.tv = take(sizeof(int) * 4 * TCAP);
    L.tn = take(sizeof(int) * 4 * TCAP);
    L.mark = take(sizeof(int) * TCAP);
    L.freel = take(sizeof(int) * TCAP);
    L.cav = take(sizeof(int) * CCAP);
    L.bnd = take(sizeof(int) * 8 * BCAP);        // per boundary face: new verts[4], face index, outside tet, back index, new id
    L.pend = take(sizeof(int) * 4 * 3 * BCAP);   // (edge key a, b, tet, face)
    L.tval = take(sizeof(double) * TCAP);
    L.fin = take(sizeof(int) * TCAP);            // slot -> compact finite index or -1
    L.tri_of = take(sizeof(int) * 4 * TCAP);
    L.tri = take(sizeof(int) * 3 * FCAP);
    L.tri_c = take(sizeof(int) * 2 * FCAP);      // cofaces: tet slots, -1 = outside
    L.fval = take(sizeof(double) * FCAP);
    L.edge = take(sizeof(int) * 2 * ECAP);
    L.eval = take(sizeof(double) * ECAP);
    L.skey = take(sizeof(uint64_t) * SCAP);
    L.sidx = take(sizeof(int) * SCAP);
    L.erank = take(sizeof(int) * ECAP);          // edge -> rank
    L.eord = take(sizeof(int) * ECAP);          // rank -> edge
    L.epos = take(sizeof(int) * ECAP);
    L.tet_edge = take(sizeof(int) * 6 * TCAP);   // (slot, local edge) -> edge id
    L.uf = take(sizeof(int) * (TCAP + 1));
    L.rep = take(sizeof(int) * (TCAP + 1));
    L.fneg = take(sizeof(int) * FCAP);
    L.pcol = take(sizeof(int) * 2 * ECAP);       // per edge rank: (pool offset, length) of the column whose low it is
    L.pool = take(sizeof(int) * POOLCAP);
    L.work = take(sizeof(int) * WCAP);
    L.work2 = take(sizeof(int) * WCAP);
    L.total = o;
    return L;
}

// ---- exact arithmetic: 384-bit two's complement ----------------------------------------------------------------------------
struct I384 {
    uint64_t w[6];
};
PD_HD inline uint64_t mulhi64(uint64_t a, uint64_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
PD_HD inline I384 ii(int64_t v)
{
    I384 r;
    const uint64_t s = v < 0 ? ~0ull : 0ull;
    r.w[0] = (uint64_t)v;
    for (int k = 1; k < 6; ++k) r.w[k] = s;
    return r;
}
PD_HD inline I384 iadd(const I384 &a, const I384 &b)
{
    I384 r;
    uint64_t c = 0;
    for (int k = 0; k < 6; ++k) {
        const uint64_t s = a.w[k] + c;
        const uint64_t c1 = s < c;
        const uint64_t t = s + b.w[k];
        r.w[k] = t;
        c = c1 + (t < s);
    }
    return r;
}
PD_HD inline bool ineg_p(const I384 &a) { return (a.w[5] >> 63) != 0; }
PD_HD inline I384 ineg(I384 a)
{
    for (int k = 0; k < 6; ++k) a.w[k] = ~a.w[k];
    return iadd(a, ii(1));
}
PD_HD inline I384 isub(const I384 &a, const I384 &b) { return iadd(a, ineg(b)); }
PD_HD inline int isign(const I384 &a)
{
    if (ineg_p(a)) return -1;
    for (int k = 0; k < 6; ++k)
        if (a.w[k]) return 1;
    return 0;
}
PD_HD inline I384 imul(I384 a, I384 b)      // the operands' magnitudes stay far below 2^383 here
{
    const bool na = ineg_p(a), nb = ineg_p(b);
    if (na) a = ineg(a);
    if (nb) b = ineg(b);
    I384 r = ii(0);
    for (int i = 0; i < 6; ++i) {
        if (!a.w[i]) continue;
        uint64_t carry = 0;
        for (int j = 0; i + j < 6; ++j) {
            const uint64_t lo = a.w[i] * b.w[j];
            uint64_t hi = mulhi64(a.w[i], b.w[j]);
            const uint64_t s = r.w[i + j] + lo;
            hi += s < lo;
            const uint64_t s2 = s + carry;
            hi += s2 < s;
            r.w[i + j] = s2;
            carry = hi;
        }
    }
    return na != nb ? ineg(r) : r;
}

// ---- predicates ------------------------------------------------------------------------------------------------------------
// orient(a, b, c, d) = sign det[b - a, c - a, d - a]  (> 0: d on the side of plane abc that a right-handed abc normal points to)
// insph(a, b, c, d, e) > 0: e strictly inside the circumsphere of the positively oriented (a, b, c, d)
constexpr double O3D_ERR = (7.0 + 56.0 * 1.1102230246251565e-16) * 1.1102230246251565e-16;
constexpr double ISP_ERR = (16.0 + 224.0 * 1.1102230246251565e-16) * 1.1102230246251565e-16;

struct Pts {
    const double *P;     // (n, 3)
    const int64_t *I;    // (n, 3) grid integers
};

PD_HD inline int orient_exact(const Pts &s, int a, int b, int c, int d)
{
    const int64_t *A = s.I + 3 * a, *B = s.I + 3 * b, *C = s.I + 3 * c, *D = s.I + 3 * d;
    const I384 bx = ii(B[0] - A[0]), by = ii(B[1] - A[1]), bz = ii(B[2] - A[2]);
    const I384 cx = ii(C[0] - A[0]), cy = ii(C[1] - A[1]), cz = ii(C[2] - A[2]);
    const I384 dx = ii(D[0] - A[0]), dy = ii(D[1] - A[1]), dz = ii(D[2] - A[2]);
    const I384 m0 = isub(imul(cy, dz), imul(cz, dy));
    const I384 m1 = isub(imul(cz, dx), imul(cx, dz));
    const I384 m2 = isub(imul(cx, dy), imul(cy, dx));
    return isign(iadd(iadd(imul(bx, m0), imul(by, m1)), imul(bz, m2)));
}

PD_HD inline int orient(const Pts &s, int a, int b, int c, int d)
{
    const double *A = s.P + 3 * a, *B = s.P + 3 * b, *C = s.P + 3 * c, *D = s.P + 3 * d;
    const double bx = B[0] - A[0], by = B[1] - A[1], bz = B[2] - A[2];
    const double cx = C[0] - A[0], cy = C[1] - A[1], cz = C[2] - A[2];
    const double dx = D[0] - A[0], dy = D[1] - A[1], dz = D[2] - A[2];
    const double cydz = cy * dz, czdy = cz * dy, czdx = cz * dx, cxdz = cx * dz, cxdy = cx * dy, cydx = cy * dx;
    const double det = bx * (cydz - czdy) + by * (czdx - cxdz) + bz * (cxdy - cydx);
    const double perm = fabs(bx) * (fabs(cydz) + fabs(czdy)) + fabs(by) * (fabs(czdx) + fabs(cxdz)) + fabs(bz) * (fabs(cxdy) + fabs(cydx));
    const double err = O3D_ERR * perm;
    if (det > err) return 1;
    if (-det > err) return -1;
    return orient_exact(s, a, b, c, d);
}

// Shewchuk's insphere polynomial (e as the origin); its sign is the opposite of insph for a positive `orient`
PD_HD inline int insph_exact(const Pts &s, int a, int b, int c, int d, int e)
{
    const int64_t *E = s.I + 3 * e;
    I384 x[4], y[4], z[4], l[4];
    const int v[4] = {a, b, c, d};
    for (int k = 0; k < 4; ++k) {
        const int64_t *Q = s.I + 3 * v[k];
        x[k] = ii(Q[0] - E[0]);
        y[k] = ii(Q[1] - E[1]);
        z[k] = ii(Q[2] - E[2]);
        l[k] = iadd(iadd(imul(x[k], x[k]), imul(y[k], y[k])), imul(z[k], z[k]));
    }
    const I384 ab = isub(imul(x[0], y[1]), imul(x[1], y[0])), bc = isub(imul(x[1], y[2]), imul(x[2], y[1]));
    const I384 cd = isub(imul(x[2], y[3]), imul(x[3], y[2])), da = isub(imul(x[3], y[0]), imul(x[0], y[3]));
    const I384 ac = isub(imul(x[0], y[2]), imul(x[2], y[0])), bd = isub(imul(x[1], y[3]), imul(x[3], y[1]));
    const I384 abc = iadd(isub(imul(z[0], bc), imul(z[1], ac)), imul(z[2], ab));
    const I384 bcd = iadd(isub(imul(z[1], cd), imul(z[2], bd)), imul(z[3], bc));
    const I384 cda = iadd(iadd(imul(z[2], da), imul(z[3], ac)), imul(z[0], cd));
    const I384 dab = iadd(iadd(imul(z[3], ab), imul(z[0], bd)), imul(z[1], da));
    const I384 det = iadd(isub(imul(l[3], abc), imul(l[2], dab)), isub(imul(l[1], cda), imul(l[0], bcd)));
    return -isign(det);
}

PD_HD inline int insph(const Pts &s, int a, int b, int c, int d, int e)
{
    const double *E = s.P + 3 * e;
    double x[4], y[4], z[4];
    const int v[4] = {a, b, c, d};
    for (int k = 0; k < 4; ++k) {
        const double *Q = s.P + 3 * v[k];
        x[k] = Q[0] - E[0];
        y[k] = Q[1] - E[1];
        z[k] = Q[2] - E[2];
    }
    const double aexbey = x[0] * y[1], bexaey = x[1] * y[0], ab = aexbey - bexaey;
    const double bexcey = x[1] * y[2], cexbey = x[2] * y[1], bc = bexcey - cexbey;
    const double cexdey = x[2] * y[3], dexcey = x[3] * y[2], cd = cexdey - dexcey;
    const double dexaey = x[3] * y[0], aexdey = x[0] * y[3], da = dexaey - aexdey;
    const double aexcey = x[0] * y[2], cexaey = x[2] * y[0], ac = aexcey - cexaey;
    const double bexdey = x[1] * y[3], dexbey = x[3] * y[1], bd = bexdey - dexbey;
    const double abc = z[0] * bc - z[1] * ac + z[2] * ab;
    const double bcd = z[1] * cd - z[2] * bd + z[3] * bc;
    const double cda = z[2] * da + z[3] * ac + z[0] * cd;
    const double dab = z[3] * ab + z[0] * bd + z[1] * da;
    const double la = x[0] * x[0] + y[0] * y[0] + z[0] * z[0], lb = x[1] * x[1] + y[1] * y[1] + z[1] * z[1];
    const double lc = x[2] * x[2] + y[2] * y[2] + z[2] * z[2], ld = x[3] * x[3] + y[3] * y[3] + z[3] * z[3];
    const double det = (ld * abc - lc * dab) + (lb * cda - la * bcd);
    const double za = fabs(z[0]), zb = fabs(z[1]), zc = fabs(z[2]), zd = fabs(z[3]);
    const double p_ab = fabs(aexbey) + fabs(bexaey), p_bc = fabs(bexcey) + fabs(cexbey), p_cd = fabs(cexdey) + fabs(dexcey);
    const double p_da = fabs(dexaey) + fabs(aexdey), p_ac = fabs(aexcey) + fabs(cexaey), p_bd = fabs(bexdey) + fabs(dexbey);
    const double perm = (p_cd * zb + p_bd * zc + p_bc * zd) * la + (p_da * zc + p_ac * zd + p_cd * za) * lb
                      + (p_ab * zd + p_bd * za + p_da * zb) * lc + (p_bc * za + p_ac * zb + p_ab * zc) * ld;
    const double err = ISP_ERR * perm;
    if (det > err) return -1;
    if (-det > err) return 1;
    return insph_exact(s, a, b, c, d, e);
}

// exact 2D orientation of a, b, c projected onto the coordinate plane that drops axis `ax`
PD_HD inline int orient2_exact(const Pts &s, int a, int b, int c, int ax)
{
    const int i = ax == 0 ? 1 : 0, j = ax == 2 ? 1 : 2;
    const int64_t *A = s.I + 3 * a, *B = s.I + 3 * b, *C = s.I + 3 * c;
    const I384 d = isub(imul(ii(B[i] - A[i]), ii(C[j] - A[j])), imul(ii(B[j] - A[j]), ii(C[i] - A[i])));
    return isign(d);
}

PD_HD inline bool lex_less(const Pts &s, int a, int b)
{
    const double *A = s.P + 3 * a, *B = s.P + 3 * b;
    if (A[0] != B[0]) return A[0] < B[0];
    if (A[1] != B[1]) return A[1] < B[1];
    return A[2] < B[2];
}

PD_HD inline void sort_lex(const Pts &s, int *v, int n)
{
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && lex_less(s, v[j], v[j - 1]); --j) {
            const int t = v[j];
            v[j] = v[j - 1];
            v[j - 1] = t;
        }
}

// perturbed insphere of the positive finite tetrahedron v against e: +1 conflict, -1 not (never 0)
PD_HD inline int insph_sos(const Pts &s, const int *v, int e)
{
    const int r = insph(s, v[0], v[1], v[2], v[3], e);
    if (r) return r;
    int q[5] = {v[0], v[1], v[2], v[3], e};
    sort_lex(s, q, 5);
    for (int i = 4; i > 1; --i) {
        if (q[i] == e) return -1;
        int w[4] = {v[0], v[1], v[2], v[3]};
        for (int k = 0; k < 4; ++k)
            if (w[k] == q[i]) w[k] = e;
        const int o = orient(s, w[0], w[1], w[2], w[3]);
        if (o) return o;
    }
    return -1;      // unreachable for a non-degenerate tetrahedron
}

// perturbed "e strictly inside the circumcircle of the coplanar triangle (a, b, c)", with d any point off its plane and
// (a, b, c, d) positive; +1 / -1
PD_HD inline int incircle_sos(const Pts &s, int a, int b, int c, int d, int e)
{
    const int r = insph(s, a, b, c, d, e);     // e lies in the plane: inside the sphere <=> inside the circle
    if (r) return r;
    int ax = 0, oref = 0;
    for (; ax < 3; ++ax)
        if ((oref = orient2_exact(s, a, b, c, ax)) != 0) break;
    int q[4] = {a, b, c, e};
    sort_lex(s, q, 4);
    for (int i = 3; i > 1; --i) {
        if (q[i] == e) return -1;
        int o = 0;
        if (q[i] == c) o = orient2_exact(s, a, b, e, ax);
        else if (q[i] == b) o = orient2_exact(s, a, e, c, ax);
        else o = orient2_exact(s, e, b, c, ax);
        if (o) return o == oref ? 1 : -1;
    }
    return -1;
}

// ---- the cloud ---------------------------------------------------------------------------------------------------------------
struct Cloud {
    // inputs
    const float *pc;
    int n, tet_cap;
    // workspace
    double *P;
    int64_t *I;
    int *vid;
    uint64_t *key;
    int *ord;
    int *tv, *tn, *mark, *freel, *cav, *bnd, *pend;
    double *tval;
    int *fin, *tri_of, *tri, *tri_c;
    double *fval;
    int *edge;
    double *eval;
    uint64_t *skey;
    int *sidx, *erank, *eord, *epos, *tet_edge, *uf, *rep, *fneg, *pcol, *pool, *work, *work2;
    // outputs
    double *h1, *h2;       // (PAIRCAP, 2)
    int *cnt;              // {h1, h2}
    int *status;
    int *tets_out;         // (TCAP, 4) original point indices, or NULL
    int *ntet_out;
    // shared scalars (lane 0 writes, everyone reads after a sync)
    int *sc;               // [0] unique points U, [1] slots used, [2] finite tets T, [3] triangles F, [4] edges E, [5] grid exponent
};

PD_HD inline void fail(Cloud &c, int code)
{
    if (*c.status == 0) *c.status = code;
}

PD_HD inline int pos_of(const int *v, int x)
{
    for (int k = 0; k < 4; ++k)
        if (v[k] == x) return k;
    return -1;
}

// conflict of tet slot t with vertex p: +1 / -1
PD_HD inline int conflict(const Cloud &c, const Pts &s, int t, int p)
{
    const int *v = c.tv + 4 * t;
    const int k = pos_of(v, INF_V);
    if (k < 0) return insph_sos(s, v, p);
    int w[4] = {v[0], v[1], v[2], v[3]};
    w[k] = p;
    const int o = orient(s, w[0], w[1], w[2], w[3]);
    if (o) return o;
    // p on the plane of the hull face: is it inside the face's circumcircle?  The finite tetrahedron across the face supplies
    // the sphere: its positive order with the off-plane vertex moved to the end by two transpositions
    const int *u = c.tv + 4 * c.tn[4 * t + k];
    int opp = 0;
    for (int m = 0; m < 4; ++m)
        if (pos_of(v, u[m]) < 0) opp = m;
    int q[4] = {u[0], u[1], u[2], u[3]};
    if (opp != 3) {
        const int t2 = q[opp];
        q[opp] = q[3];
        q[3] = t2;
        const int t3 = q[0];
        q[0] = q[1];
        q[1] = t3;
    }
    return incircle_sos(s, q[0], q[1], q[2], q[3], p);
}

PD_HD inline uint64_t spread3(uint32_t x)
{
    uint64_t v = x & 0x3ff;
    v = (v | (v << 16)) & 0x30000ff;
    v = (v | (v << 8)) & 0x300f00f;
    v = (v | (v << 4)) & 0x30c30c3;
    v = (v | (v << 2)) & 0x9249249;
    return v;
}

// link faces of two tetrahedra if they share three vertices (used for the first five)
PD_HD inline void link_pair(Cloud &c, int t, int u)
{
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j) {
            int hit = 0;
            for (int a = 0; a < 4; ++a) {
                if (a == i) continue;
                for (int b = 0; b < 4; ++b)
                    if (b != j && c.tv[4 * t + a] == c.tv[4 * u + b]) ++hit;
            }
            if (hit == 3) {
                c.tn[4 * t + i] = u;
                c.tn[4 * u + j] = t;
            }
        }
    }
}

// insert vertex p; returns a finite tetrahedron of the new star, or -1 on failure (status set)
PD_HD inline int insert(Cloud &c, const Pts &s, int p, int start, int stamp, int &nslots, int &nfree)
{
    // visibility walk (deterministic face rotation)
    int t = start;
    int step = 0;
    for (; step < WALK_CAP; ++step) {
        const int *v = c.tv + 4 * t;
        if (pos_of(v, INF_V) >= 0) break;
        int moved = -1;
        for (int r = 0; r < 4 && moved < 0; ++r) {
            const int i = (r + step) & 3;
            int w[4] = {v[0], v[1], v[2], v[3]};
            w[i] = p;
            if (orient(s, w[0], w[1], w[2], w[3]) < 0) moved = c.tn[4 * t + i];
        }
        if (moved < 0) break;
        t = moved;
    }
    if (step == WALK_CAP) { fail(c, TGP_PD_EWALK); return -1; }
    // cavity
    const int IN = 2 * stamp, OUT = 2 * stamp + 1;
    int ncav = 0, head = 0;
    c.mark[t] = IN;
    c.cav[ncav++] = t;
    while (head < ncav) {
        const int u = c.cav[head++];
        for (int i = 0; i < 4; ++i) {
            const int nb = c.tn[4 * u + i];
            if (c.mark[nb] == IN || c.mark[nb] == OUT) continue;
            if (conflict(c, s, nb, p) > 0) {
                if (ncav == CCAP) { fail(c, TGP_PD_ECAVITY); return -1; }
                c.mark[nb] = IN;
                c.cav[ncav++] = nb;
            } else {
                c.mark[nb] = OUT;
            }
        }
    }
    // boundary faces
    int nb_ = 0;
    for (int q = 0; q < ncav; ++q) {
        const int u = c.cav[q];
        for (int i = 0; i < 4; ++i) {
            const int o = c.tn[4 * u + i];
            if (c.mark[o] == IN) continue;
            if (nb_ == BCAP) { fail(c, TGP_PD_ECAVITY); return -1; }
            int *B = c.bnd + 8 * nb_++;
            for (int k = 0; k < 4; ++k) B[k] = c.tv[4 * u + k];
            B[i] = p;
            B[4] = i;
            B[5] = o;
            B[6] = -1;
            for (int k = 0; k < 4; ++k)
                if (c.tn[4 * o + k] == u) B[6] = k;
        }
    }
    // slots: the cavity's, then new ones
    for (int q = ncav - 1; q >= 0; --q) {
        c.freel[nfree++] = c.cav[q];
        c.tv[4 * c.cav[q]] = DEAD;
    }
    if (nb_ > nfree + (c.tet_cap - nslots)) { fail(c, TGP_PD_ETETS); return -1; }
    int first_fin = -1, npend = 0;
    for (int q = 0; q < nb_; ++q) {
        int *B = c.bnd + 8 * q;
        const int id = nfree ? c.freel[--nfree] : nslots++;
        B[7] = id;
        c.mark[id] = -1;
        for (int k = 0; k < 4; ++k) c.tv[4 * id + k] = B[k];
        const int i = B[4];
        c.tn[4 * id + i] = B[5];
        c.tn[4 * B[5] + B[6]] = id;
        if (first_fin < 0 && pos_of(B, INF_V) < 0) first_fin = id;
        for (int k = 0; k < 4; ++k) {
            if (k == i) continue;
            int e0 = -1, e1 = -1;
            for (int m = 0; m < 4; ++m) {
                if (m == i || m == k) continue;
                if (e0 < 0) e0 = B[m]; else e1 = B[m];
            }
            if (e0 > e1) { const int tt = e0; e0 = e1; e1 = tt; }
            int hit = -1;
            for (int r = 0; r < npend; ++r)
                if (c.pend[4 * r] == e0 && c.pend[4 * r + 1] == e1) { hit = r; break; }
            if (hit >= 0) {
                const int ot = c.pend[4 * hit + 2], of = c.pend[4 * hit + 3];
                c.tn[4 * id + k] = ot;
                c.tn[4 * ot + of] = id;
                --npend;
                for (int m = 0; m < 4; ++m) c.pend[4 * hit + m] = c.pend[4 * npend + m];
            } else {
                if (npend == 3 * BCAP) { fail(c, TGP_PD_ECAVITY); return -1; }
                int *Q = c.pend + 4 * npend++;
                Q[0] = e0; Q[1] = e1; Q[2] = id; Q[3] = k;
            }
        }
    }
    if (npend != 0 || first_fin < 0) { fail(c, TGP_PD_EINTERNAL); return -1; }
    return first_fin;
}

// The order in which tet_r2 / tri_r2 take a simplex's n = 3 or 4 vertices: an endpoint of the shortest edge is the base of the
// differences, the edge's other endpoint comes next, the rest follow by distance from the base.  With a far vertex as the base
// the products u x v of two nearly equal long differences cancel, and the circumcentre of a simplex with two close vertices
// and a distant one loses the digits that the Gabriel tests need; based at the short edge the short difference enters exactly.
PD_HD inline void near_order(const double *const *V, int n, int *o)
{
    double best = INFINITY;
    o[0] = 0;
    o[1] = 1;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double x = V[i][0] - V[j][0], y = V[i][1] - V[j][1], z = V[i][2] - V[j][2];
            const double d = x * x + y * y + z * z;
            if (d < best) {
                best = d;
                o[0] = i;
                o[1] = j;
            }
        }
    int m = 2;
    for (int k = 0; k < n; ++k)
        if (k != o[0] && k != o[1]) o[m++] = k;
    if (n == 4) {
        const double *A = V[o[0]], *P = V[o[2]], *Q = V[o[3]];
        const double px = P[0] - A[0], py = P[1] - A[1], pz = P[2] - A[2], qx = Q[0] - A[0], qy = Q[1] - A[1], qz = Q[2] - A[2];
        if (qx * qx + qy * qy + qz * qz < px * px + py * py + pz * pz) {
            const int t = o[2];
            o[2] = o[3];
            o[3] = t;
        }
    }
}

// Double-double arithmetic (an unevaluated sum h + l of two float64, ~106 bits) for the filtration values.  Many simplices
// share one sphere (a right triangle and its hypotenuse, the tetrahedra of a cospherical group), and a plain float64 evaluation
// from different vertices gives values an ulp or two apart: a pair of that length where there is none.  Evaluated to ~2^-100 and
// rounded once, two expressions of one number give the same float64 unless it lies that close to a rounding boundary.
// fma() is written out; the library is compiled with -ffp-contract=off, which the error-free sums need.
struct DD {
    double h, l;
};
PD_HD inline DD dd_fast(double a, double b)          // |a| >= |b| or a == 0
{
    const double s = a + b;
    return {s, b - (s - a)};
}
PD_HD inline DD dd_sum(double a, double b)           // exact a + b
{
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
PD_HD inline DD dd_prod(double a, double b)          // exact a * b
{
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
PD_HD inline DD dd_add(DD a, DD b)
{
    DD s = dd_sum(a.h, b.h);
    const DD t = dd_sum(a.l, b.l);
    s = dd_sum(s.h, s.l + t.h);              // after a cancellation the low parts may outweigh s.h
    return dd_fast(s.h, s.l + t.l);
}
PD_HD inline DD dd_sub(DD a, DD b) { return dd_add(a, DD{-b.h, -b.l}); }
PD_HD inline DD dd_mul(DD a, DD b)
{
    const DD p = dd_prod(a.h, b.h);
    return dd_fast(p.h, p.l + (a.h * b.l + a.l * b.h));
}
PD_HD inline DD dd_scale(DD a, double p2) { return {a.h * p2, a.l * p2}; }       // p2 a power of two
PD_HD inline DD dd_div(DD a, DD b)
{
    const double q1 = a.h / b.h;
    DD r = dd_sub(a, dd_mul(b, DD{q1, 0.0}));
    const double q2 = r.h / b.h;
    r = dd_sub(r, dd_mul(b, DD{q2, 0.0}));
    const double q3 = r.h / b.h;
    return dd_add(dd_fast(q1, q2), DD{q3, 0.0});
}
PD_HD inline bool dd_less(DD a, DD b) { return a.h < b.h || (a.h == b.h && a.l < b.l); }
PD_HD inline void dd_diff3(const double *B, const double *A, DD *u)
{
    for (int k = 0; k < 3; ++k) u[k] = dd_sum(B[k], -A[k]);
}
PD_HD inline void dd_cross(const DD *a, const DD *b, DD *c)
{
    c[0] = dd_sub(dd_mul(a[1], b[2]), dd_mul(a[2], b[1]));
    c[1] = dd_sub(dd_mul(a[2], b[0]), dd_mul(a[0], b[2]));
    c[2] = dd_sub(dd_mul(a[0], b[1]), dd_mul(a[1], b[0]));
}
PD_HD inline DD dd_dot(const DD *a, const DD *b)
{
    return dd_add(dd_add(dd_mul(a[0], b[0]), dd_mul(a[1], b[1])), dd_mul(a[2], b[2]));
}

// the squared circumradius and (ctr != NULL) the circumcentre from the offsets o = N / den of the base vertex A
PD_HD inline DD dd_centre(const double *A, const DD *N, DD den, DD *ctr)
{
    DD r2 = {0.0, 0.0};
    for (int k = 0; k < 3; ++k) {
        const DD o = dd_div(N[k], den);
        if (ctr) ctr[k] = dd_add(DD{A[k], 0.0}, o);
        r2 = dd_add(r2, dd_mul(o, o));
    }
    return r2;
}

// Smallest circumspheres.  The vertices are taken in near_order; the squared radius comes back as a double-double (its .h is
// the value, rounded once) and the centre as three, for the Gabriel tests.
PD_HD inline DD tet_r2(const double *A, const double *B, const double *C, const double *D, DD *ctr)
{
    const double *const V[4] = {A, B, C, D};
    int o[4];
    near_order(V, 4, o);
    DD u[3], v[3], w[3], vw[3], wu[3], uv[3], N[3];
    dd_diff3(V[o[1]], V[o[0]], u);
    dd_diff3(V[o[2]], V[o[0]], v);
    dd_diff3(V[o[3]], V[o[0]], w);
    dd_cross(v, w, vw);
    dd_cross(w, u, wu);
    dd_cross(u, v, uv);
    const DD uu = dd_dot(u, u), vv = dd_dot(v, v), ww = dd_dot(w, w);
    for (int k = 0; k < 3; ++k) N[k] = dd_add(dd_add(dd_mul(uu, vw[k]), dd_mul(vv, wu[k])), dd_mul(ww, uv[k]));
    return dd_centre(V[o[0]], N, dd_scale(dd_dot(u, vw), 2.0), ctr);
}

PD_HD inline DD tri_r2(const double *A, const double *B, const double *C, DD *ctr)
{
    const double *const V[3] = {A, B, C};
    int o[4];
    near_order(V, 3, o);
    DD u[3], v[3], w[3], vw[3], wu[3], N[3];
    dd_diff3(V[o[1]], V[o[0]], u);
    dd_diff3(V[o[2]], V[o[0]], v);
    dd_cross(u, v, w);
    dd_cross(v, w, vw);
    dd_cross(w, u, wu);
    const DD uu = dd_dot(u, u), vv = dd_dot(v, v);
    for (int k = 0; k < 3; ++k) N[k] = dd_add(dd_mul(uu, vw[k]), dd_mul(vv, wu[k]));
    return dd_centre(V[o[0]], N, dd_scale(dd_dot(w, w), 2.0), ctr);
}

PD_HD inline DD edge_r2(const double *A, const double *B, DD *ctr)
{
    DD d[3];
    dd_diff3(A, B, d);
    for (int k = 0; k < 3; ++k) ctr[k] = dd_scale(dd_sum(A[k], B[k]), 0.5);
    return dd_scale(dd_dot(d, d), 0.25);
}

PD_HD inline DD dist2(const double *A, const DD *ctr)
{
    DD d[3];
    for (int k = 0; k < 3; ++k) d[k] = dd_sub(DD{A[k], 0.0}, ctr[k]);
    return dd_dot(d, d);
}

PD_HD inline uint64_t dkey(double v)
{
    union {
        double d;
        uint64_t u;
    } x;
    x.d = v;
    return x.u;      // values are >= 0: the bit pattern orders them
}

// one bitonic pass over (skey, sidx), ascending by (key, idx)
PD_HD inline void bitonic_pass(Cloud &c, int n2, int k, int j, int tid, int nt)
{
    for (int i = tid; i < n2; i += nt) {
        const int l = i ^ j;
        if (l <= i) continue;
        const bool up = (i & k) == 0;
        const uint64_t ka = c.skey[i], kb = c.skey[l];
        const int ia = c.sidx[i], ib = c.sidx[l];
        const bool gt = ka > kb || (ka == kb && ia > ib);
        if (gt == up) {
            c.skey[i] = kb; c.skey[l] = ka;
            c.sidx[i] = ib; c.sidx[l] = ia;
        }
    }
}

PD_HD inline int pow2_at_least(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

PD_HD inline void sort_keys(Cloud &c, int n, int tid, int nt)
{
    const int n2 = pow2_at_least(n < 2 ? 2 : n);
    for (int i = n + tid; i < n2; i += nt) {
        c.skey[i] = ~0ull;
        c.sidx[i] = 0x7fffffff;
    }
    PD_SYNC();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            bitonic_pass(c, n2, k, j, tid, nt);
            PD_SYNC();
        }
}

PD_HD inline int uf_find(int *uf, int x)
{
    int r = x;
    for (int g = 0; g <= TCAP + 1 && uf[r] != r; ++g) r = uf[r];
    for (int g = 0; g <= TCAP + 1 && uf[x] != r; ++g) {
        const int nx = uf[x];
        uf[x] = r;
        x = nx;
    }
    return r;
}

PD_HD inline bool tet_older(const Cloud &c, int a, int b)    // (value, index) order of tet slots; slot TCAP = outside = +inf
{
    if (a == TCAP) return false;
    if (b == TCAP) return true;
    if (c.tval[a] != c.tval[b]) return c.tval[a] < c.tval[b];
    return a < b;
}

// the walk around edge (a, b) of tet slot t: calls f(cur, px, y) for each face crossed, the face of `cur` at position px,
// (a, b, y); returns false when the ring does not close within RING_CAP
template <class F>
PD_HD inline bool ring(const Cloud &c, int t, int a, int b, F f)
{
    const int *v = c.tv + 4 * t;
    int x = -1;
    for (int k = 0; k < 4 && x < 0; ++k)
        if (v[k] != a && v[k] != b) x = v[k];
    int cur = t;
    for (int g = 0; g < RING_CAP; ++g) {
        const int *cv = c.tv + 4 * cur;
        const int px = pos_of(cv, x);
        int y = -1;
        for (int k = 0; k < 4; ++k)
            if (cv[k] != a && cv[k] != b && cv[k] != x) y = cv[k];
        f(cur, px, y);
        cur = c.tn[4 * cur + px];      // across (a, b, y); there the next face to cross is the one opposite y
        x = y;
        if (cur == t) return true;
    }
    return false;
}

PD_HD inline int pair_slot(int i, int j)       // local edge number of positions i < j
{
    return i == 0 ? j - 1 : (i == 1 ? j + 1 : 5);
}

// the triangle id of face px of slot cur (a ghost slot's finite face: through the finite tetrahedron across it)
PD_HD inline int face_tri(const Cloud &c, int cur, int px)
{
    if (c.fin[cur] >= 0) return c.tri_of[4 * cur + px];
    const int o = c.tn[4 * cur + px];
    return c.tri_of[4 * o + pos_of(c.tn + 4 * o, cur)];
}

PD_HD inline void push_pair(Cloud &c, double *out, int which, double b, double d)
{
    if (!(d > b)) return;
    const int k = c.cnt[which];
    if (k == PAIRCAP) { fail(c, TGP_PD_EPAIRS); return; }
    out[2 * k] = b;
    out[2 * k + 1] = d;
    c.cnt[which] = k + 1;
}

// the whole cloud; every lane of the workgroup calls it
PD_HD inline void pd_run(Cloud &c, int tid, int nt)
{
    const Layout L = layout();
    (void)L;
    const int n = c.n;
    // ---- 0: status, bounds, the grid exponent -------------------------------------------------------------------------------
    if (tid == 0) {
        *c.status = 0;
        c.cnt[0] = c.cnt[1] = 0;
        if (c.ntet_out) *c.ntet_out = 0;
        float m = 0.f;
        bool finite = true;                            // fmaxf drops a NaN, so each coordinate is looked at on its own: a cloud
        for (int i = 0; i < 3 * n; ++i) {              // with one stops here, before any float -> int conversion sees it
            const float a = fabsf(c.pc[i]);
            finite = finite && a < INFINITY;
            m = fmaxf(m, a);
        }
        int e = 0;
        frexp((double)m, &e);
        c.sc[5] = e - 60;
        if (!finite) fail(c, TGP_PD_ERANGE);
    }
    PD_SYNC();
    if (*c.status) return;
    // ---- 1: Morton keys (10 bits per axis over the bounding box), rank sort, dedup -----------------------------------------
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], c.pc[3 * i + k]);
            hi[k] = fmaxf(hi[k], c.pc[3 * i + k]);
        }
    for (int i = tid; i < n; i += nt) {
        uint64_t code = 0;
        for (int k = 0; k < 3; ++k) {
            const float ext = hi[k] - lo[k];
            const float f = ext > 0.f ? (c.pc[3 * i + k] - lo[k]) / ext * 1023.f : 0.f;
            const int q = f >= 0.f ? (f < 1023.f ? (int)f : 1023) : 0;      // an extent beyond float32 gives inf / inf: cell 0
            code |= spread3((uint32_t)q) << k;
        }
        c.key[i] = (code << 32) | (uint64_t)i;
    }
    PD_SYNC();
    for (int i = tid; i < n; i += nt) {
        int r = 0;
        const uint64_t ki = c.key[i];
        for (int j = 0; j < n; ++j) r += c.key[j] < ki;
        c.ord[r] = i;
    }
    PD_SYNC();
    if (tid == 0) {
        int U = 0;
        const int G = c.sc[5];
        for (int r = 0; r < n; ++r) {
            const int i = c.ord[r];
            const float *p = c.pc + 3 * i;
            bool dup = false;
            // duplicates share the Morton cell: scan back over this cell's earlier points
            for (int q = r - 1; q >= 0 && (c.key[c.ord[q]] >> 32) == (c.key[i] >> 32) && !dup; --q) {
                const float *o = c.pc + 3 * c.ord[q];
                dup = o[0] == p[0] && o[1] == p[1] && o[2] == p[2];
            }
            if (dup) continue;
            for (int k = 0; k < 3; ++k) {
                const double x = (double)p[k];
                const double g = ldexp(x, -G);
                c.P[3 * U + k] = x;
                c.I[3 * U + k] = (int64_t)g;
                if ((double)(int64_t)g != g) fail(c, TGP_PD_ERANGE);
            }
            c.vid[U++] = i;
        }
        c.sc[0] = U;
    }
    PD_SYNC();
    if (*c.status) return;
    const int U = c.sc[0];
    const Pts s = {c.P, c.I};
    // ---- 2: Delaunay (lane 0) -----------------------------------------------------------------------------------------------
    if (tid == 0) {
        int i1 = 1, i2 = -1, i3 = -1;
        if (U >= 4) {
            for (int k = 2; k < U && i2 < 0; ++k)
                if (orient2_exact(s, 0, i1, k, 0) || orient2_exact(s, 0, i1, k, 1) || orient2_exact(s, 0, i1, k, 2)) i2 = k;
            for (int k = 2; i2 >= 0 && k < U && i3 < 0; ++k)
                if (k != i2 && orient(s, 0, i1, i2, k) != 0) i3 = k;
        }
        if (i3 < 0) {
            fail(c, TGP_PD_EFLAT);
        } else {
            int v0 = 0, v1 = i1;
            if (orient(s, v0, v1, i2, i3) < 0) { v0 = i1; v1 = 0; }
            const int base[4] = {v0, v1, i2, i3};
            for (int k = 0; k < 4; ++k) c.tv[k] = base[k];
            for (int g = 0; g < 4; ++g) {
                int *w = c.tv + 4 * (1 + g);
                for (int k = 0; k < 4; ++k) w[k] = base[k];
                w[g] = INF_V;
                const int a = (g + 1) & 3, b = (g + 2) & 3;
                const int t = w[a];
                w[a] = w[b];
                w[b] = t;
            }
            for (int t = 0; t < 5; ++t) c.mark[t] = -1;
            for (int t = 0; t < 5; ++t)
                for (int u = t + 1; u < 5; ++u) link_pair(c, t, u);
            int nslots = 5, nfree = 0, last = 0;
            for (int v = 1; v < U && *c.status == 0; ++v) {
                if (v == i1 || v == i2 || v == i3) continue;
                last = insert(c, s, v, last, v, nslots, nfree);
            }
            c.sc[1] = nslots;
        }
    }
    PD_SYNC();
    if (*c.status) return;
    const int nslots = c.sc[1];
    // ---- 3: finite tetrahedra: compact index, value; triangles (lane 0 numbers them) ---------------------------------------
    if (tid == 0) {
        int T = 0;
        for (int t = 0; t < nslots; ++t) {
            const int *v = c.tv + 4 * t;
            c.fin[t] = (v[0] == DEAD || pos_of(v, INF_V) >= 0) ? -1 : T++;
        }
        c.sc[2] = T;
        int F = 0;
        for (int t = 0; t < nslots && !*c.status; ++t) {
            if (c.fin[t] < 0) continue;
            for (int i = 0; i < 4; ++i) {
                const int o = c.tn[4 * t + i];
                if (c.fin[o] >= 0 && o < t) {                    // numbered from the other side already
                    c.tri_of[4 * t + i] = c.tri_of[4 * o + pos_of(c.tn + 4 * o, t)];
                    continue;
                }
                if (F == FCAP) { fail(c, TGP_PD_ETETS); break; }
                int k = 0;
                for (int m = 0; m < 4; ++m)
                    if (m != i) c.tri[3 * F + k++] = c.tv[4 * t + m];
                c.tri_c[2 * F] = t;
                c.tri_c[2 * F + 1] = c.fin[o] >= 0 ? o : -1;
                c.tri_of[4 * t + i] = F++;
            }
        }
        c.sc[3] = F;
        if (c.tets_out) {
            for (int t = 0; t < nslots; ++t)
                if (c.fin[t] >= 0)
                    for (int k = 0; k < 4; ++k) c.tets_out[4 * c.fin[t] + k] = c.vid[c.tv[4 * t + k]];
            *c.ntet_out = T;
        }
    }
    PD_SYNC();
    if (*c.status) return;
    const int F = c.sc[3];
    for (int t = tid; t < nslots; t += nt)
        if (c.fin[t] >= 0) {
            const int *v = c.tv + 4 * t;
            c.tval[t] = tet_r2(c.P + 3 * v[0], c.P + 3 * v[1], c.P + 3 * v[2], c.P + 3 * v[3], nullptr).h;
        }
    PD_SYNC();
    for (int f = tid; f < F; f += nt) {
        const int *v = c.tri + 3 * f;
        DD ctr[3];
        const DD r2 = tri_r2(c.P + 3 * v[0], c.P + 3 * v[1], c.P + 3 * v[2], ctr);
        double val = INFINITY;
        bool gab = true;
        for (int side = 0; side < 2; ++side) {
            const int t = c.tri_c[2 * f + side];
            if (t < 0) continue;
            const int *u = c.tv + 4 * t;
            for (int m = 0; m < 4; ++m)
                if (u[m] != v[0] && u[m] != v[1] && u[m] != v[2] && dd_less(dist2(c.P + 3 * u[m], ctr), r2)) gab = false;
            val = fmin(val, c.tval[t]);
        }
        c.fval[f] = gab ? fmin(r2.h, val) : val;
    }
    PD_SYNC();
    // ---- 4: edges, each numbered by the lowest finite tetrahedron around it (lane 0) ----------------------------------------
    if (tid == 0) {
        int E = 0;
        for (int t = 0; t < nslots && !*c.status; ++t) {
            if (c.fin[t] < 0) continue;
            const int *v = c.tv + 4 * t;
            for (int i = 0; i < 4; ++i)
                for (int j = i + 1; j < 4; ++j) {
                    const int a = v[i], b = v[j];
                    int lowest = t;
                    const bool ok = ring(c, t, a, b, [&](int cur, int, int) {
                        if (c.fin[cur] >= 0 && cur < lowest) lowest = cur;
                    });
                    if (!ok) { fail(c, TGP_PD_EINTERNAL); break; }
                    if (lowest != t) continue;
                    if (E == ECAP) { fail(c, TGP_PD_ETETS); break; }
                    c.edge[2 * E] = a;
                    c.edge[2 * E + 1] = b;
                    c.epos[E] = t;                               // the owner, for the walks below
                    ring(c, t, a, b, [&](int cur, int, int) {
                        const int *cv = c.tv + 4 * cur;
                        const int pa = pos_of(cv, a), pb = pos_of(cv, b);
                        c.tet_edge[6 * cur + pair_slot(pa < pb ? pa : pb, pa < pb ? pb : pa)] = E;
                    });
                    ++E;
                }
        }
        c.sc[4] = E;
    }
    PD_SYNC();
    if (*c.status) return;
    const int E = c.sc[4];
    for (int e = tid; e < E; e += nt) {
        const int a = c.edge[2 * e], b = c.edge[2 * e + 1];
        DD ctr[3];
        const DD r2 = edge_r2(c.P + 3 * a, c.P + 3 * b, ctr);
        double val = INFINITY;
        bool gab = true;
        ring(c, c.epos[e], a, b, [&](int cur, int px, int y) {
            if (y == INF_V) return;
            if (dd_less(dist2(c.P + 3 * y, ctr), r2)) gab = false;
            val = fmin(val, c.fval[face_tri(c, cur, px)]);
        });
        c.eval[e] = gab ? fmin(r2.h, val) : val;
    }
    PD_SYNC();
    // ---- 5: H0 (Kruskal over the edges in order; negative edges leave the H1 rows) ------------------------------------------
    for (int e = tid; e < E; e += nt) {
        c.skey[e] = dkey(c.eval[e]);
        c.sidx[e] = e;
    }
    sort_keys(c, E, tid, nt);
    for (int r = tid; r < E; r += nt) {
        c.erank[c.sidx[r]] = r;
        c.eord[r] = c.sidx[r];
    }
    PD_SYNC();
    if (tid == 0) {
        for (int v = 0; v < U; ++v) c.uf[v] = v;
        for (int r = 0; r < E; ++r) {
            const int e = c.eord[r];
            const int ra = uf_find(c.uf, c.edge[2 * e]), rb = uf_find(c.uf, c.edge[2 * e + 1]);
            c.epos[e] = ra == rb;                                 // positive: creates a cycle
            if (ra != rb) c.uf[ra < rb ? rb : ra] = ra < rb ? ra : rb;
        }
    }
    PD_SYNC();
    // ---- 6: H2 by union-find on the dual graph (tetrahedra + the outside), triangles in decreasing order ---------------------
    for (int f = tid; f < F; f += nt) {
        c.skey[f] = dkey(c.fval[f]);
        c.sidx[f] = f;
    }
    sort_keys(c, F, tid, nt);
    if (tid == 0) {
        for (int t = 0; t <= TCAP; ++t) {
            c.uf[t] = t;
            c.rep[t] = t;
        }
        for (int r = F - 1; r >= 0; --r) {
            const int f = c.sidx[r];
            const int t1 = c.tri_c[2 * f], t2 = c.tri_c[2 * f + 1] < 0 ? TCAP : c.tri_c[2 * f + 1];
            const int r1 = uf_find(c.uf, t1), r2 = uf_find(c.uf, t2);
            if (r1 == r2) { c.fneg[f] = 1; continue; }            // kills an H1 class
            c.fneg[f] = 0;                                        // creates a void, which the younger component's tet fills
            const int a = c.rep[r1], b = c.rep[r2];
            const bool a_young = tet_older(c, a, b);
            push_pair(c, c.h2, 1, c.fval[f], c.tval[a_young ? a : b]);
            c.uf[r1] = r2;
            c.rep[r2] = a_young ? b : a;
        }
    }
    PD_SYNC();
    if (*c.status) return;
    // ---- 7: H1 by column reduction of the negative triangles over the positive edges (lane 0) ----------------------------------
    if (tid == 0) {
        for (int r = 0; r < E; ++r) c.pcol[2 * r] = -1;
        int used = 0;
        for (int r = 0; r < F && !*c.status; ++r) {
            const int f = c.sidx[r];
            if (!c.fneg[f]) continue;
            const int t = c.tri_c[2 * f];
            int i = 0;
            while (i < 3 && c.tri_of[4 * t + i] != f) ++i;
            int *w = c.work, *w2 = c.work2;
            int m = 0;
            for (int p = 0; p < 4; ++p)
                for (int q = p + 1; q < 4; ++q) {
                    if (p == i || q == i) continue;
                    const int e = c.tet_edge[6 * t + pair_slot(p, q)];
                    if (c.epos[e]) w[m++] = c.erank[e];
                }
            for (int x = 1; x < m; ++x)                           // decreasing ranks
                for (int y = x; y > 0 && w[y] > w[y - 1]; --y) {
                    const int tt = w[y];
                    w[y] = w[y - 1];
                    w[y - 1] = tt;
                }
            int guard = 0;
            while (m > 0 && c.pcol[2 * w[0]] >= 0 && guard++ <= E) {
                const int *col = c.pool + c.pcol[2 * w[0]];
                const int cm = c.pcol[2 * w[0] + 1];
                int x = 0, y = 0, k = 0;                           // symmetric difference of two decreasing lists
                while ((x < m || y < cm) && k <= WCAP) {
                    if (y == cm || (x < m && w[x] > col[y])) { if (k < WCAP) w2[k] = w[x]; ++k; ++x; }
                    else if (x == m || col[y] > w[x]) { if (k < WCAP) w2[k] = col[y]; ++k; ++y; }
                    else { ++x; ++y; }
                }
                if (k > WCAP) { fail(c, TGP_PD_ECOLUMNS); break; }
                int *tt = w; w = w2; w2 = tt;
                m = k;
            }
            if (*c.status) break;
            if (m == 0 || guard > E) { fail(c, TGP_PD_EINTERNAL); break; }
            if (used + m > POOLCAP) { fail(c, TGP_PD_ECOLUMNS); break; }
            for (int x = 0; x < m; ++x) c.pool[used + x] = w[x];
            c.pcol[2 * w[0]] = used;
            c.pcol[2 * w[0] + 1] = m;
            used += m;
            push_pair(c, c.h1, 0, c.eval[c.eord[w[0]]], c.fval[f]);
        }
    }
    PD_SYNC();
    if (*c.status && tid == 0) c.cnt[0] = c.cnt[1] = 0;
}

PD_HD inline Cloud cloud_at(const tgp_pd_args &a, int b)
{
    const Layout L = layout();
    char *base = (char *)a.workspace + (size_t)b * L.total;
    Cloud c;
    c.pc = a.pcl + (size_t)b * a.N * 3;
    c.n = a.N;
    c.tet_cap = a.tet_cap > 0 && a.tet_cap < TCAP ? a.tet_cap : TCAP;
    c.P = (double *)(base + L.P);
    c.I = (int64_t *)(base + L.I);
    c.vid = (int *)(base + L.vid);
    c.key = (uint64_t *)(base + L.key);
    c.ord = (int *)(base + L.ord);
    c.tv = (int *)(base + L.tv);
    c.tn = (int *)(base + L.tn);
    c.mark = (int *)(base + L.mark);
    c.freel = (int *)(base + L.freel);
    c.cav = (int *)(base + L.cav);
    c.bnd = (int *)(base + L.bnd);
    c.pend = (int *)(base + L.pend);
    c.tval = (double *)(base + L.tval);
    c.fin = (int *)(base + L.fin);
    c.tri_of = (int *)(base + L.tri_of);
    c.tri = (int *)(base + L.tri);
    c.tri_c = (int *)(base + L.tri_c);
    c.fval = (double *)(base + L.fval);
    c.edge = (int *)(base + L.edge);
    c.eval = (double *)(base + L.eval);
    c.skey = (uint64_t *)(base + L.skey);
    c.sidx = (int *)(base + L.sidx);
    c.erank = (int *)(base + L.erank);
    c.eord = (int *)(base + L.eord);
    c.epos = (int *)(base + L.epos);
    c.tet_edge = (int *)(base + L.tet_edge);
    c.uf = (int *)(base + L.uf);
    c.rep = (int *)(base + L.rep);
    c.fneg = (int *)(base + L.fneg);
    c.pcol = (int *)(base + L.pcol);
    c.pool = (int *)(base + L.pool);
    c.work = (int *)(base + L.work);
    c.work2 = (int *)(base + L.work2);
    c.h1 = a.h1 + (size_t)b * PAIRCAP * 2;
    c.h2 = a.h2 + (size_t)b * PAIRCAP * 2;
    c.cnt = a.counts + 2 * b;
    c.status = a.status + b;
    c.tets_out = a.tets ? a.tets + (size_t)b * TCAP * 4 : nullptr;
    c.ntet_out = a.tets ? a.ntet + b : nullptr;
    return c;
}

// ---- the image (legacy persim PersImage, spread 1e-2, 50 x 50, linear weighting) ------------------------------------------
constexpr int PIX = 50;
constexpr int CHUNK = 32;

PD_HD inline double ndtr(double a)            // the standard normal CDF as scipy's ndtr evaluates it
{
    const double x = a * 0.70710678118654752440, z = fabs(x);
    if (z < 0.70710678118654752440) return 0.5 + 0.5 * erf(x);
    const double y = 0.5 * erfc(z);
    return x > 0 ? 1.0 - y : y;
}

}  // namespace pd

__global__ void __launch_bounds__(pd::THREADS) pd_diagram_kernel(tgp_pd_args a)
{
    __shared__ int sc[8];
    pd::Cloud c = pd::cloud_at(a, blockIdx.x);
    c.sc = sc;
    pd::pd_run(c, threadIdx.x, blockDim.x);
}

__global__ void __launch_bounds__(pd::THREADS) pd_image_kernel(tgp_pd_args a)
{
    using namespace pd;
    const int b = blockIdx.x, dim = blockIdx.y, tid = threadIdx.x;
    __shared__ double phx[CHUNK][PIX], phy[CHUNK][PIX], wt[CHUNK];
    __shared__ double red[THREADS];
    __shared__ float redf[THREADS];
    float *out = (dim == 0 ? a.pdh1 : a.pdh2) + (size_t)b * PIX * PIX;
    const int ok = a.status[b] == 0;
    const int n1 = ok ? a.counts[2 * b] : 0, n = ok ? a.counts[2 * b + dim] : 0;
    const double *own = (dim == 0 ? a.h1 : a.h2) + (size_t)b * PAIRCAP * 2;
    const double *spec = n1 > 0 ? a.h1 + (size_t)b * PAIRCAP * 2 : own;     // the first non-empty transform sets the ranges
    const int ns = n1 > 0 ? n1 : n;
    // maxBD over (birth, persistence) of the spec diagram, max persistence of this one (max is exact in any order)
    double mbd = 0.0, mp = 0.0;
    for (int k = tid; k < ns; k += THREADS) mbd = fmax(mbd, fmax(spec[2 * k], spec[2 * k + 1] - spec[2 * k]));
    red[tid] = mbd;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double maxbd = red[0];
    __syncthreads();
    for (int k = tid; k < n; k += THREADS) mp = fmax(mp, own[2 * k + 1] - own[2 * k]);
    red[tid] = mp;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double maxp = red[0];
    const double inv = 1.0 / maxp;
    const double dx = maxbd / PIX, step = maxbd / (PIX - 1);
    constexpr int PER = (PIX * PIX + THREADS - 1) / THREADS;
    double acc[PER];
    for (int q = 0; q < PER; ++q) acc[q] = 0.0;
    for (int k0 = 0; k0 < n; k0 += CHUNK) {
        __syncthreads();
        const int m = n - k0 < CHUNK ? n - k0 : CHUNK;
        for (int j = tid; j < m * PIX; j += THREADS) {
            const int k = j / PIX, i = j % PIX;
            const double bi = own[2 * (k0 + k)], p = own[2 * (k0 + k) + 1] - bi;
            const double lo = i == PIX - 1 ? maxbd : i * step, up = lo + dx;
            phx[k][i] = ndtr((up - bi) / 1e-2) - ndtr((lo - bi) / 1e-2);
            phy[k][i] = ndtr((up - p) / 1e-2) - ndtr((lo - p) / 1e-2);
            if (i == 0) wt[k] = inv * p;
        }
        __syncthreads();
        for (int q = 0; q < PER; ++q) {
            const int px = tid + q * THREADS;
            if (px >= PIX * PIX) break;
            const int r = px / PIX, col = px % PIX, yb = PIX - 1 - r;  // img.T[::-1]: row r = persistence bin 49 - r
            double s = acc[q];
            for (int k = 0; k < m; ++k) s += (phx[k][col] * phy[k][yb]) * wt[k];
            acc[q] = s;
        }
    }
    float mx = 0.f;
    for (int q = 0; q < PER; ++q)
        if (tid + q * THREADS < PIX * PIX) mx = fmaxf(mx, (float)acc[q]);
    redf[tid] = mx;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) redf[tid] = fmaxf(redf[tid], redf[tid + s]);
        __syncthreads();
    }
    const float den = redf[0] + 1e-20f;
    for (int q = 0; q < PER; ++q) {
        const int px = tid + q * THREADS;
        if (px < PIX * PIX) out[px] = n > 0 ? (float)acc[q] / den : 0.f;
    }
}

extern "C" int64_t tgp_pd_workspace_bytes(void) { return (int64_t)pd::layout().total; }
extern "C" int tgp_pd_max_points(void) { return TGP_PD_MAX_POINTS; }

extern "C" int tgp_persistence(const tgp_pd_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->B > 0 && a->N > 0 && a->N <= TGP_PD_MAX_POINTS);
    TGP_REQUIRE(a->pcl && a->workspace && a->h1 && a->h2 && a->counts && a->status);
    TGP_REQUIRE(((uintptr_t)a->workspace & 255) == 0);
    TGP_REQUIRE(!a->tets || a->ntet);
    TGP_REQUIRE((a->pdh1 == nullptr) == (a->pdh2 == nullptr));
    TGP_REQUIRE(a->tet_cap >= 0);
    hipLaunchKernelGGL(pd_diagram_kernel, dim3(a->B), dim3(pd::THREADS), 0, tgp_hs(stream), *a);
    int rc = TGP_LAUNCH_RESULT();
    if (rc) return rc;
    if (a->pdh1) {
        hipLaunchKernelGGL(pd_image_kernel, dim3(a->B, 2), dim3(pd::THREADS), 0, tgp_hs(stream), *a);
        rc = TGP_LAUNCH_RESULT();
    }
    return rc;
}
