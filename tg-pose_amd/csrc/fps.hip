// Farthest point sampling (core/utils/farthest_points_torch.py: farthest_points) on gfx950.
//
// The reference runs n dependent steps of (argmax, pairwise_distance, min, ==) over the whole cloud as CPU tensor operations.  Here
// ONE workgroup owns a cloud: every thread keeps P consecutive points and their running distances in registers for all n steps
// (thread t holds points t*P .. t*P + P - 1, so a lower lane, wave and register slot is a lower point index), and a step is
//   1. the thread's maximum at its first slot (strict >), fused with the previous step's update,
//   2. the wave's maximum (DPP row reduction, no LDS) and the first lane that holds it (ballot),
//   3. that lane's (value, index, x, y, z) into the wave's LDS slot, ONE barrier, every thread scans the <= 8 slots in wave
//      order (strict >) and so agrees on the centre without a second barrier: the slots are double buffered by step parity.
// No atomics, no workgroup waits on another, every loop is bounded by n and P.
//
// Arithmetic (DESIGN.md section 3 "Farthest point sampling" is the contract; the library is built with -ffp-contract=off):
//   e = fl(fl(c - p) + 1e-6f) per component, d = sqrt_rn(fma(e.z, e.z, fma(e.y, e.y, fl(e.x * e.x))))
// which is torch's CPU F.pairwise_distance bit for bit.  Step i: centre = the lowest index of the maximum running distance;
// new = d(centre, .); where new <= running: running = new, cluster = i.  The centroid (start == NULL, init_center != 0) is the
// pairwise-tree fp32 sum over the point index -- level k adds the neighbours 2j and 2j + 1 of level k - 1, rows at and beyond the
// count are zeros -- divided by (float)count: the thread's P points, the wave's lanes (xor 1, 2, .. 32) and the waves are exactly
// the levels of that tree, and adding the zero subtree beyond the count changes nothing, so the result does not depend on M, P or
// the threads per workgroup.
#include "tgp_common.h"

#define FPS_MAX_POINTS 8192
#define FPS_MAX_WAVES 8
#define FPS_DEAD (-1.0f) // running distance of rows at and beyond the count: below every distance, never updated

__device__ __forceinline__ float fps_dist(float cx, float cy, float cz, float px, float py, float pz)
{
    const float ex = (cx - px) + 1e-6f, ey = (cy - py) + 1e-6f, ez = (cz - pz) + 1e-6f;
    return sqrtf(__fmaf_rn(ez, ez, __fmaf_rn(ey, ey, ex * ex)));
}

template <int CTRL, int ROW_MASK> __device__ __forceinline__ float fps_dpp_max(float v)
{
    // lanes without a source (row_bcast into a masked row) keep v: max(v, v)
    const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
    return fmaxf(v, __int_as_float(o));
}

// the wave's maximum in every lane: butterflies inside a row of 16 (quad_perm [1,0,3,2], [2,3,0,1], row_ror 4, 8), lane 15 of a row
// into the next row (rows 1, 3), lane 31 into rows 2, 3; lane 63 then holds the maximum of all 64
__device__ __forceinline__ float fps_wave_max(float v)
{
    v = fps_dpp_max<0xb1, 0xf>(v);
    v = fps_dpp_max<0x4e, 0xf>(v);
    v = fps_dpp_max<0x124, 0xf>(v);
    v = fps_dpp_max<0x128, 0xf>(v);
    v = fps_dpp_max<0x142, 0xa>(v);
    v = fps_dpp_max<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

template <int T, int P, bool CL>
__global__ __launch_bounds__(T) void fps_kernel(const float *__restrict__ xyz, int ld, const int32_t *__restrict__ counts, int M, int n,
                                                const float *__restrict__ start, int init_center, int32_t *__restrict__ idx,
                                                float *__restrict__ dist_out, int32_t *__restrict__ clusters_out)
{
    constexpr int W = T / TGP_WAVE;
    __shared__ float s_val[2][FPS_MAX_WAVES];
    __shared__ float4 s_win[2][FPS_MAX_WAVES]; // {index bits, x, y, z} of the wave's winner
    __shared__ float s_sum[FPS_MAX_WAVES][4];

    const int tid = threadIdx.x, lane = tid & (TGP_WAVE - 1), wave = tid / TGP_WAVE;
    const size_t b = blockIdx.x;
    int cnt = counts ? counts[b] : M;
    cnt = min(max(cnt, 1), M);
    const float *src = xyz + b * (size_t)M * ld;
    int32_t *out_idx = idx + b * (size_t)n;

    if (cnt <= n) { // _sample_points' tiling rule; no sampling: the optional outputs hold the initial state
        for (int i = tid; i < n; i += T) out_idx[i] = i % cnt;
    }

    float px[P], py[P], pz[P], d[P];
    int cl[P];
    const int i0 = tid * P;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const bool live = i0 + j < cnt;
        px[j] = live ? src[(size_t)(i0 + j) * ld + 0] : 0.f;
        py[j] = live ? src[(size_t)(i0 + j) * ld + 1] : 0.f;
        pz[j] = live ? src[(size_t)(i0 + j) * ld + 2] : 0.f;
        cl[j] = -1;
    }

    if (init_center) {
        float cx, cy, cz;
        if (start) {
            cx = start[b * 3 + 0], cy = start[b * 3 + 1], cz = start[b * 3 + 2];
        } else {
            float tx[P], ty[P], tz[P];
#pragma unroll
            for (int j = 0; j < P; ++j) tx[j] = px[j], ty[j] = py[j], tz[j] = pz[j];
#pragma unroll
            for (int w = 1; w < P; w <<= 1)
#pragma unroll
                for (int j = 0; j < P; j += 2 * w) tx[j] += tx[j + w], ty[j] += ty[j + w], tz[j] += tz[j + w];
            float sx = tx[0], sy = ty[0], sz = tz[0];
            for (int m = 1; m < TGP_WAVE; m <<= 1) {
                sx += __shfl_xor(sx, m, TGP_WAVE);
                sy += __shfl_xor(sy, m, TGP_WAVE);
                sz += __shfl_xor(sz, m, TGP_WAVE);
            }
            if (lane == 0) s_sum[wave][0] = sx, s_sum[wave][1] = sy, s_sum[wave][2] = sz;
            __syncthreads();
            float t3[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float a[W];
#pragma unroll
                for (int w = 0; w < W; ++w) a[w] = s_sum[w][c];
#pragma unroll
                for (int w = 1; w < W; w <<= 1)
#pragma unroll
                    for (int j = 0; j < W; j += 2 * w) a[j] += a[j + w];
                t3[c] = a[0];
            }
            const float fc = (float)cnt;
            cx = t3[0] / fc, cy = t3[1] / fc, cz = t3[2] / fc;
        }
#pragma unroll
        for (int j = 0; j < P; ++j) d[j] = i0 + j < cnt ? fps_dist(cx, cy, cz, px[j], py[j], pz[j]) : FPS_DEAD;
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) d[j] = i0 + j < cnt ? 1e7f : FPS_DEAD;
    }

    if (cnt > n) {
        float best = d[0];
        int bj = 0;
#pragma unroll
        for (int j = 1; j < P; ++j)
            if (d[j] > best) best = d[j], bj = j;

        for (int i = 0; i < n; ++i) {
            const int buf = i & 1;
            const float wmax = fps_wave_max(best);
            const unsigned long long hit = __ballot(best == wmax);
            const int first = hit ? __ffsll((long long)hit) - 1 : 0; // no lane equals the maximum only with non-finite input
            if (lane == first) {
                float bx = px[0], by = py[0], bz = pz[0];
#pragma unroll
                for (int j = 1; j < P; ++j)
                    if (bj == j) bx = px[j], by = py[j], bz = pz[j];
                s_val[buf][wave] = best;
                s_win[buf][wave] = make_float4(__int_as_float(i0 + bj), bx, by, bz);
            }
            __syncthreads();
            int ww = 0;
            float wv = s_val[buf][0];
#pragma unroll
            for (int w = 1; w < W; ++w) {
                const float v = s_val[buf][w];
                if (v > wv) wv = v, ww = w;
            }
            const float4 c = s_win[buf][ww];
            if (tid == 0) out_idx[i] = min(__float_as_int(c.x), cnt - 1); // inside the cloud whatever the input holds
            best = FPS_DEAD - 1.f;
            bj = 0;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const float nd = fps_dist(c.y, c.z, c.w, px[j], py[j], pz[j]);
                if (nd <= d[j]) { // dead rows hold -1: never
                    d[j] = nd;
                    if (CL) cl[j] = i;
                }
                if (d[j] > best) best = d[j], bj = j;
            }
        }
    }

#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (i0 + j < cnt) {
            if (dist_out) dist_out[b * (size_t)M + i0 + j] = d[j];
            if (CL) clusters_out[b * (size_t)M + i0 + j] = cl[j];
        }
    }
}

template <int T, int P>
static int fps_launch(const float *xyz, int ld, const int32_t *counts, int B, int M, int n, const float *start, int init_center, int32_t *idx,
                      float *dist_out, int32_t *clusters_out, tgp_stream_t stream)
{
    static_assert(T * P <= FPS_MAX_POINTS && T / TGP_WAVE <= FPS_MAX_WAVES, "fps variant");
    if (clusters_out)
        hipLaunchKernelGGL((fps_kernel<T, P, true>), dim3(B), dim3(T), 0, tgp_hs(stream), xyz, ld, counts, M, n, start, init_center, idx,
                           dist_out, clusters_out);
    else
        hipLaunchKernelGGL((fps_kernel<T, P, false>), dim3(B), dim3(T), 0, tgp_hs(stream), xyz, ld, counts, M, n, start, init_center, idx,
                           dist_out, clusters_out);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_fps_max_points(void) { return FPS_MAX_POINTS; }

// Threads and points per thread from M: one wave up to 64 points, one wave per SIMD (256 threads) up to 1024, two waves per SIMD
// (512 threads, the full vector issue rate) above.
extern "C" int tgp_fps(const float *xyz, int ld, const int32_t *counts, int B, int M, int n, const float *start, int init_center,
                       int32_t *idx, float *dist_out, int32_t *clusters_out, tgp_stream_t stream)
{
    TGP_REQUIRE(xyz && idx && B > 0 && M > 0 && n > 0 && (ld == 3 || ld == 4));
    if (M > FPS_MAX_POINTS) return TGP_EUNSUPPORTED;
#define FPS_CASE(LIMIT, T, P) \
    if (M <= (LIMIT)) return fps_launch<T, P>(xyz, ld, counts, B, M, n, start, init_center, idx, dist_out, clusters_out, stream)
    FPS_CASE(64, 64, 1);
    FPS_CASE(256, 256, 1);
    FPS_CASE(512, 256, 2);
    FPS_CASE(1024, 256, 4);
    FPS_CASE(2048, 512, 4);
    FPS_CASE(4096, 512, 8);
    FPS_CASE(8192, 512, 16);
#undef FPS_CASE
    return TGP_EUNSUPPORTED;
}
