// The Ranger optimizer step (tools/torch_utils/solver/ranger2020.py:43-246: RAdam + Lookahead + gradient centralisation) over every
// tensor of a step in ONE launch.  Memory bound: per element it reads p, g, m, v (+ slow on a lookahead step) and writes p, m, v
// (+ g where the gradient is centralised, + slow on a lookahead step).  The scalars of the step (step_size, the adaptive and the
// lookahead decisions) come from the host per tensor (include/tgpose.h, tgp_ranger_tensor).
//
// Work units, a function of (numel, row_len, flags) alone, so that a tensor's result never depends on the other tensors of the launch:
//   centralised, row_len <= RG_SHORT:  64 rows, one per lane (the rows are summed in element order by their lane);
//   centralised, longer rows:          one row per wave; up to RG_SPAN elements the row's gradient stays in registers between the sum
//                                      and the update, longer rows are read twice;
//   not centralised:                   RG_SPAN elements.
// A wave walks the units u = its global wave index, + the number of waves, ...  Within a span the layout is: h head elements (one per
// lane) up to the first 16-byte boundary of exp_avg (the optimizer's own buffer: its phase is a function of the shape), then float4
// quads (lane l takes quads l, l + 64, ...), then up to 3 tail elements.  Every other array uses 16-byte accesses when it is aligned at
// the same element as exp_avg, 4-byte accesses otherwise (gradients inside flat buckets sit at any 4-byte offset).
// The row sum: each lane adds its head element, its quads ((x + y) + (z + w), in quad order) and its tail element, then a butterfly over
// the 64 lanes (commutative pairwise adds: every lane ends with the same bits).  mean = sum / row_len, as torch's mean.
#include "tgp_common.h"

namespace {

constexpr int RG_WAVES = 4;                  // waves per workgroup
constexpr int RG_SHORT = 32;                 // centralised rows up to this length: one row per lane
constexpr int RG_NV = 16;                    // float4 registers per lane of a row kept in registers
constexpr int RG_SPAN = RG_NV * 4 * 64;      // 4096 elements: the register bound of a row, the size of a plain unit

struct Upd {
    float b1, omb1, b2, omb2, eps, wd, lr, alpha;
    bool adaptive, look;
};

struct Span {
    float *p, *g, *m, *v, *s;                // at the span's first element
    bool vp, vg, vv, vs;                     // 16-byte accesses (aligned at the head's end like m)
    int h, nq, r;                            // head elements, quads, tail elements
};

__device__ __forceinline__ bool al16(const float *a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

__device__ __forceinline__ Span make_span(float *p, float *g, float *m, float *v, float *s, int64_t n)
{
    Span sp;
    int h = (int)(((16 - (reinterpret_cast<uintptr_t>(m) & 15)) & 15) >> 2);
    if (h > n) h = (int)n;
    sp.p = p, sp.g = g, sp.m = m, sp.v = v, sp.s = s;
    sp.h = h;
    sp.nq = (int)((n - h) >> 2);
    sp.r = (int)((n - h) & 3);
    sp.vp = al16(p + h), sp.vg = al16(g + h), sp.vv = al16(v + h), sp.vs = al16(s + h);
    return sp;
}

__device__ __forceinline__ float4 ld4(const float *a, int64_t i, bool vec)
{
    if (vec) return *reinterpret_cast<const float4 *>(a + i);
    return make_float4(a[i], a[i + 1], a[i + 2], a[i + 3]);
}

__device__ __forceinline__ void st4(float *a, int64_t i, float4 x, bool vec)
{
    if (vec) {
        *reinterpret_cast<float4 *>(a + i) = x;
    } else {
        a[i] = x.x, a[i + 1] = x.y, a[i + 2] = x.z, a[i + 3] = x.w;
    }
}

// one element, in the reference's order: moments, update (G aliases exp_avg on the non-adaptive branch), lookahead
__device__ __forceinline__ void upd1(const Upd &u, float g, float &p, float &m, float &v, float &s)
{
    v = v * u.b2;
    v = v + (u.omb2 * g) * g;                       // addcmul_: self + value * t1 * t2
    m = fmaf(g, u.omb1, m * u.b1);                  // add_(grad, alpha): one rounding
    float G;
    if (u.adaptive) {
        G = m / (sqrtf(v) + u.eps);
        if (u.wd != 0.f) G = fmaf(p, u.wd, G);
    } else {
        if (u.wd != 0.f) m = fmaf(p, u.wd, m);      // G_grad.add_ on exp_avg itself: the change stays in the state
        G = m;
    }
    p = fmaf(G, u.lr, p);
    if (u.look) {
        s = fmaf(p - s, u.alpha, s);
        p = s;
    }
}

__device__ __forceinline__ void elem(const Upd &u, const Span &sp, int64_t i, float g, bool wg)
{
    float p = sp.p[i], m = sp.m[i], v = sp.v[i], s = u.look ? sp.s[i] : 0.f;
    upd1(u, g, p, m, v, s);
    if (wg) sp.g[i] = g;
    sp.p[i] = p, sp.m[i] = m, sp.v[i] = v;
    if (u.look) sp.s[i] = s;
}

__device__ __forceinline__ void quad(const Upd &u, const Span &sp, int64_t i, float4 g, bool wg)
{
    float4 p = ld4(sp.p, i, sp.vp), m = ld4(sp.m, i, true), v = ld4(sp.v, i, sp.vv);
    float4 s = u.look ? ld4(sp.s, i, sp.vs) : make_float4(0.f, 0.f, 0.f, 0.f);
    upd1(u, g.x, p.x, m.x, v.x, s.x);
    upd1(u, g.y, p.y, m.y, v.y, s.y);
    upd1(u, g.z, p.z, m.z, v.z, s.z);
    upd1(u, g.w, p.w, m.w, v.w, s.w);
    if (wg) st4(sp.g, i, g, sp.vg);
    st4(sp.p, i, p, sp.vp);
    st4(sp.m, i, m, true);
    st4(sp.v, i, v, sp.vv);
    if (u.look) st4(sp.s, i, s, sp.vs);
}

__device__ __forceinline__ float4 sub4(float4 a, float b) { return make_float4(a.x - b, a.y - b, a.z - b, a.w - b); }

__device__ __forceinline__ float wave_sum(float s)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// span without a register copy of g: the plain units (gc = false) and the second pass over a long row (gc = true, mean given)
__device__ void stream_span(const Upd &u, const Span &sp, int lane, bool gc, float mean)
{
    if (lane < sp.h) {
        float g = sp.g[lane];
        elem(u, sp, lane, gc ? g - mean : g, gc);
    }
    for (int q = lane; q < sp.nq; q += 64) {
        const int64_t i = sp.h + 4 * (int64_t)q;
        float4 g = ld4(sp.g, i, sp.vg);
        quad(u, sp, i, gc ? sub4(g, mean) : g, gc);
    }
    if (lane < sp.r) {
        const int64_t i = sp.h + 4 * (int64_t)sp.nq + lane;
        float g = sp.g[i];
        elem(u, sp, i, gc ? g - mean : g, gc);
    }
}

// a centralised row of more than RG_SHORT elements, one wave
__device__ void gc_row(const Upd &u, const Span &sp, int64_t L, int lane)
{
    float acc = 0.f;
    if (L <= RG_SPAN) {
        float4 gr[RG_NV];
        float gh = 0.f, gt = 0.f;
        if (lane < sp.h) gh = sp.g[lane];
        if (lane < sp.r) gt = sp.g[sp.h + 4 * (int64_t)sp.nq + lane];
#pragma unroll
        for (int k = 0; k < RG_NV; ++k) {
            const int q = lane + 64 * k;
            gr[k] = q < sp.nq ? ld4(sp.g, sp.h + 4 * (int64_t)q, sp.vg) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (lane < sp.h) acc = gh;
#pragma unroll
        for (int k = 0; k < RG_NV; ++k)
            if (lane + 64 * k < sp.nq) acc += (gr[k].x + gr[k].y) + (gr[k].z + gr[k].w);
        if (lane < sp.r) acc += gt;
        const float mean = wave_sum(acc) / (float)L;
        if (lane < sp.h) elem(u, sp, lane, gh - mean, true);
#pragma unroll
        for (int k = 0; k < RG_NV; ++k) {
            const int q = lane + 64 * k;
            if (q < sp.nq) quad(u, sp, sp.h + 4 * (int64_t)q, sub4(gr[k], mean), true);
        }
        if (lane < sp.r) elem(u, sp, sp.h + 4 * (int64_t)sp.nq + lane, gt - mean, true);
        return;
    }
    // longer rows: sum pass, then the update pass reads g again
    if (lane < sp.h) acc = sp.g[lane];
    for (int q = lane; q < sp.nq; q += 64) {
        const float4 g = ld4(sp.g, sp.h + 4 * (int64_t)q, sp.vg);
        acc += (g.x + g.y) + (g.z + g.w);
    }
    if (lane < sp.r) acc += sp.g[sp.h + 4 * (int64_t)sp.nq + lane];
    const float mean = wave_sum(acc) / (float)L;
    stream_span(u, sp, lane, true, mean);
}

__global__ void __launch_bounds__(64 * RG_WAVES) ranger_kernel(const tgp_ranger_tensor *__restrict__ T, int n, int64_t units)
{
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * RG_WAVES;
    int64_t u = (int64_t)blockIdx.x * RG_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (; u < units; u += nwaves) {
        // the last tensor whose first unit is <= u (tensors without units share their unit0 with the next one)
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (T[mid].unit0 <= u) lo = mid;
            else hi = mid - 1;
        }
        const tgp_ranger_tensor &d = T[lo];
        Upd up;
        up.b1 = d.beta1, up.omb1 = d.one_minus_beta1, up.b2 = d.beta2, up.omb2 = d.one_minus_beta2;
        up.eps = d.eps, up.wd = d.weight_decay, up.lr = d.neg_step_lr, up.alpha = d.alpha;
        up.adaptive = (d.flags & TGP_RANGER_ADAPTIVE) != 0;
        up.look = (d.flags & TGP_RANGER_LOOKAHEAD) != 0;
        const int64_t local = u - d.unit0, numel = d.numel;
        if (d.flags & TGP_RANGER_GC) {
            const int64_t L = d.row_len, rows = numel / L;
            if (L <= RG_SHORT) {
                const int64_t row = local * 64 + lane;
                if (row < rows) {
                    const int64_t o = row * L;
                    float acc = 0.f;
                    for (int j = 0; j < L; ++j) acc += d.g[o + j];
                    const float mean = acc / (float)L;
                    Span sp;
                    sp.p = d.p + o, sp.g = d.g + o, sp.m = d.m + o, sp.v = d.v + o, sp.s = d.slow + o;
                    for (int j = 0; j < L; ++j) elem(up, sp, j, sp.g[j] - mean, true);
                }
            } else {
                const int64_t o = local * L;
                gc_row(up, make_span(d.p + o, d.g + o, d.m + o, d.v + o, d.slow + o, L), L, lane);
            }
        } else {
            const int64_t o = local * RG_SPAN;
            const int64_t len = numel - o < RG_SPAN ? numel - o : RG_SPAN;
            stream_span(up, make_span(d.p + o, d.g + o, d.m + o, d.v + o, d.slow + o, len), lane, false, 0.f);
        }
    }
}

int64_t units_of(const tgp_ranger_tensor &t)
{
    if (t.numel == 0) return 0;
    if (t.flags & TGP_RANGER_GC) {
        const int64_t rows = t.numel / t.row_len;
        return t.row_len <= RG_SHORT ? (rows + 63) / 64 : rows;
    }
    return (t.numel + RG_SPAN - 1) / RG_SPAN;
}

}  // namespace

extern "C" int tgp_ranger_plan(tgp_ranger_tensor *t, int n, int64_t *units)
{
    TGP_REQUIRE(units && n >= 0 && (n == 0 || t));
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const tgp_ranger_tensor &d = t[i];
        TGP_REQUIRE(d.p && d.g && d.m && d.v && d.slow && d.numel >= 0);
        TGP_REQUIRE((d.flags & ~(TGP_RANGER_GC | TGP_RANGER_ADAPTIVE | TGP_RANGER_LOOKAHEAD)) == 0);
        if (d.flags & TGP_RANGER_GC) TGP_REQUIRE(d.row_len >= 1 && d.numel % d.row_len == 0);
        auto al4 = [](const float *q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; };
        TGP_REQUIRE(al4(d.p) && al4(d.g) && al4(d.m) && al4(d.v) && al4(d.slow));
    }
    for (int i = 0; i < n; ++i) {
        t[i].unit0 = total;
        total += units_of(t[i]);
    }
    *units = total;
    return 0;
}

extern "C" int tgp_ranger_step(const tgp_ranger_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->n >= 0 && a->units >= 0 && (a->n > 0 || a->units == 0) && (a->n == 0 || a->tensors));
    if (a->units == 0) return 0;
    // as many workgroups as fill every CU's wave slots (147 VGPRs: 3 waves per SIMD, 3 workgroups of 4 waves per CU; a wave then
    // walks its units); fewer when there is less work
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
    }
    const int64_t want = (a->units + RG_WAVES - 1) / RG_WAVES;
    const int blocks = (int)(want < (int64_t)cus * 3 ? want : (int64_t)cus * 3);
    hipLaunchKernelGGL(ranger_kernel, dim3(blocks), dim3(64 * RG_WAVES), 0, tgp_hs(stream), a->tensors, a->n, a->units);
    return TGP_LAUNCH_RESULT();
}
