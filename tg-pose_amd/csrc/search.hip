// Distance-field pose search on gfx950 (DESIGN.md section 3 "Model-based acquisition" and include/tgpose.h are the contract;
// tests/search_ref.py restates it in NumPy, bit for bit).
//
// field_kernel: one thread per voxel, the model's points through LDS in tiles as float4 (x, y, z, |y|^2); the least of tgp_nn1's
// float32 values is counted against the host's threshold table.  No square root, no division.
//
// search_kernel: one workgroup of SR_GROUPS x 256 lanes per (job, block of TGP_SEARCH_ROT_BLOCK rotations).  The job's field -- G^3
// bytes -- is copied to LDS once; every lookup of the workgroup hits it, and the four groups, a rotation each at a time, share it
// (at G = 48 only one field fits a CU: the groups are what fills its SIMDs).  Each lane keeps its (at most four) points minus the
// anchor in registers; the points that contribute (live, finite) are numbered once, by ballots.  Per rotation a group writes their
// records to LDS: the base voxel packed 3 x 10 bits and its linear index (bit 30 marks the up to three records that pad to four); then a lane owns up to SR_SH shifts at a time and walks the points four at
// a time: two broadcast 16-byte LDS reads, and per (point, shift) one add and one masked compare for the range test of all three
// axes, one add for the address and a byte lookup -- sixteen independent lookups in flight.  The rotation arithmetic is paid once
// per (rotation, point) and nothing crosses lanes inside the walk.  A min-reduction on the key (cost << 32 | shift index) follows:
// wave shuffles, then LDS.
//
// finish_kernel: one workgroup per job takes `top` times the least key (cost << 32 | rotation) above the one before, and writes
// the rows and their poses (float64, rounded once).  No atomics anywhere: two calls give identical bytes.
#include "tgp_common.h"

namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_WAVES = SR_THREADS / TGP_WAVE;
constexpr int SR_PPL = TGP_SEARCH_MAX_POINTS / SR_THREADS;       // points per lane
constexpr int SR_SH = 4;                                         // shifts a lane walks side by side
constexpr int SR_BIAS = 256;
constexpr int SR_MAX_REACH = 200;                                // K * stride at most: 255 - 200 >= 48, the largest G
#ifndef TGP_SEARCH_PAD
#define TGP_SEARCH_PAD 0                                         // bytes behind each z row of the field's LDS image, a multiple of 4 (measured: DESIGN.md)
#endif
constexpr int SR_PAD = TGP_SEARCH_PAD;
constexpr int SR_GROUPS = 4;                                     // groups of SR_THREADS lanes in a workgroup, a rotation each at a time
constexpr int FB_THREADS = 256;
constexpr int FB_TILE = 1024;
constexpr int INT_MAX32 = 0x7fffffff;

__global__ void __launch_bounds__(FB_THREADS) field_kernel(tgp_field_args a)
{
    __shared__ float4 s_pts[FB_TILE];
    __shared__ float s_thr[256];
    const int m = blockIdx.y, tid = threadIdx.x, G = a.G;
    const int v = blockIdx.x * FB_THREADS + tid;                 // G^3 is a multiple of FB_THREADS for every G the entry admits
    int count = a.model_count ? a.model_count[m] : a.m_cap;
    count = min(max(count, 0), a.m_cap);
    for (int l = tid; l < a.cap; l += FB_THREADS) s_thr[l] = a.thresholds[(size_t)m * a.cap + l];
    const float *mt = a.meta + (size_t)m * 4;
    const float voxel = mt[3];
    const int ix = v / (G * G), iy = (v / G) % G, iz = v % G;
    const float half = (float)(G / 2);
    const float cx = mt[0] + (((float)ix - half) + 0.5f) * voxel;
    const float cy = mt[1] + (((float)iy - half) + 0.5f) * voxel;
    const float cz = mt[2] + (((float)iz - half) + 0.5f) * voxel;
    float qq = cx * cx;
    qq = qq + cy * cy;
    qq = qq + cz * cz;
    float best = __builtin_inff();
    const float *mp = a.models + (size_t)m * a.m_cap * 6;
    for (int lo = 0; lo < count; lo += FB_TILE) {
        const int nt = min(FB_TILE, count - lo);
        __syncthreads();
        for (int j = tid; j < nt; j += FB_THREADS) {
            const float *p = mp + (size_t)(lo + j) * 6;
            const float x = p[0], y = p[1], z = p[2];
            float q = x * x;
            q = q + y * y;
            q = q + z * z;
            s_pts[j] = make_float4(x, y, z, q);
        }
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const float4 y = s_pts[j];
            float inner = cx * y.x;
            inner = fmaf(cy, y.y, inner);
            inner = fmaf(cz, y.z, inner);
            const float sum = y.w + qq;
            const float dv = sum - 2.0f * inner;
            if (dv < best) best = dv;
        }
    }
    __syncthreads();                                             // s_thr, also when the model has no point
    int lv = 0;
    for (int l = 0; l < a.cap; ++l) lv += best >= s_thr[l] ? 1 : 0;
    a.field[(size_t)m * G * G * G + v] = (uint8_t)lv;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long x)
{
#pragma unroll
    for (int off = TGP_WAVE / 2; off >= 1; off >>= 1) {
        const unsigned long long y = __shfl_xor(x, off, TGP_WAVE);
        x = y < x ? y : x;
    }
    return x;
}

// In-range test of three axes at once.  A point's base voxel b (clamped to [-256, 255]) is stored as three 10-bit fields b + 256, a
// shift as three fields d + 256 (|d| <= SR_MAX_REACH keeps every sum inside its field: no carry crosses), so one integer add gives
// the three fields b + d + 512, and b + d is inside [0, G) exactly when each field is inside [512, 512 + G).
constexpr uint32_t SR_REP = 1u | (1u << 10) | (1u << 20);
template <int G>
__device__ __forceinline__ bool fields_in_grid(uint32_t f)
{
    if (G == 16) return (f & (0x3f0u * SR_REP)) == 0x200u * SR_REP;
    if (G == 32) return (f & (0x3e0u * SR_REP)) == 0x200u * SR_REP;
    // 48: inside [512, 576), and bits 4 and 5 not both set (that would be [560, 576))
    return (f & (0x3c0u * SR_REP)) == 0x200u * SR_REP && ((f & (f >> 1)) & (0x10u * SR_REP)) == 0;
}

// the costs of NK shifts per lane, sidx0 + k * SR_THREADS (k < NK), over the n4 (a multiple of 4) point records; a shift index >= D
// gives a key of ~0.  A record is (fields | dead << 30, linear voxel index of b); the field has two bytes behind it, cap and 0:
// what a live point off the grid, and a dead point, cost.
template <int G, int NK>
__device__ __forceinline__ unsigned long long walk(const uint8_t *s_field, const uint2 *s_base, int n4, int sidx0, int D, int K, int stride)
{
    constexpr int PZ = G + SR_PAD, F3 = G * G * PZ;
    const int side = 2 * K + 1;
    uint32_t sf[NK];
    int sl[NK], cost[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int sidx = sidx0 + k * SR_THREADS;
        const int dx = (sidx / (side * side) - K) * stride, dy = ((sidx / side) % side - K) * stride, dz = (sidx % side - K) * stride;
        sf[k] = (uint32_t)(dx + SR_BIAS) | ((uint32_t)(dy + SR_BIAS) << 10) | ((uint32_t)(dz + SR_BIAS) << 20);
        sl[k] = (dx * G + dy) * PZ + dz;
        cost[k] = 0;
    }
    for (int i = 0; i < n4; i += 4) {
        const uint4 r01 = *reinterpret_cast<const uint4 *>(s_base + i), r23 = *reinterpret_cast<const uint4 *>(s_base + i + 2);   // broadcasts
        const uint32_t pf[4] = {r01.x, r01.z, r23.x, r23.z};
        const int pl[4] = {(int)r01.y, (int)r01.w, (int)r23.y, (int)r23.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int off = F3 + (int)(pf[q] >> 30);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const bool in = fields_in_grid<G>(pf[q] + sf[k]);   // bit 30 (dead) is outside every mask
                cost[k] += s_field[in ? pl[q] + sl[k] : off];
            }
        }
    }
    unsigned long long best = ~0ull;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int sidx = sidx0 + k * SR_THREADS;
        const unsigned long long key = ((unsigned long long)(uint32_t)cost[k] << 32) | (uint32_t)sidx;
        if (sidx < D && key < best) best = key;
    }
    return best;
}

constexpr int search_lds(int G) { return G * G * (G + SR_PAD) + 16 + SR_GROUPS * (TGP_SEARCH_MAX_POINTS * 8 + SR_WAVES * 8 + SR_PPL * SR_WAVES * 4); }

template <int G>
__global__ void __launch_bounds__(SR_THREADS *SR_GROUPS) search_kernel(tgp_pose_search_args a)
{
    extern __shared__ __align__(16) unsigned char s_mem[];
    constexpr int G3 = G * G * G, PZ = G + SR_PAD, F3 = G * G * PZ;
    uint8_t *s_field = s_mem;
    const int grp = threadIdx.x / SR_THREADS, tid = threadIdx.x % SR_THREADS, lane = tid & (TGP_WAVE - 1), wave = tid / TGP_WAVE;
    uint2 *s_base = reinterpret_cast<uint2 *>(s_mem + F3 + 16) + grp * TGP_SEARCH_MAX_POINTS;
    unsigned long long *s_red = reinterpret_cast<unsigned long long *>(s_mem + F3 + 16 + SR_GROUPS * TGP_SEARCH_MAX_POINTS * 8) + grp * SR_WAVES;
    const int job = blockIdx.y;
    const int r0 = blockIdx.x * TGP_SEARCH_ROT_BLOCK, r1 = min(r0 + TGP_SEARCH_ROT_BLOCK, a.R);
    int32_t *table = static_cast<int32_t *>(a.workspace) + (size_t)job * a.R * 2;

    const int jm = a.job_model[job];
    const int n = a.counts ? a.counts[job] : a.n_cap;
    if (!(jm >= 0 && jm < a.M && n >= 0 && n <= a.n_cap)) {      // the same in every thread: nothing else is read
        if ((int)threadIdx.x < r1 - r0) table[(size_t)(r0 + threadIdx.x) * 2] = INT_MAX32, table[(size_t)(r0 + threadIdx.x) * 2 + 1] = -1;
        return;
    }
    {
        if (SR_PAD == 0) {
            const uint4 *src = reinterpret_cast<const uint4 *>(a.field + (size_t)jm * G3);
            uint4 *dst = reinterpret_cast<uint4 *>(s_field);
            for (int i = threadIdx.x; i < G3 / 16; i += SR_THREADS * SR_GROUPS) dst[i] = src[i];
        } else {                                                 // dword by dword, each z row PZ bytes apart
            const uint32_t *src = reinterpret_cast<const uint32_t *>(a.field + (size_t)jm * G3);
            for (int i = threadIdx.x; i < G3 / 4; i += SR_THREADS * SR_GROUPS)
                *reinterpret_cast<uint32_t *>(s_field + (i / (G / 4)) * PZ + (i % (G / 4)) * 4) = src[i];
        }
        if (threadIdx.x == 0) s_field[F3] = (uint8_t)a.cap, s_field[F3 + 1] = 0;
    }
    const float voxel = a.meta[(size_t)jm * 4 + 3];
    const float inv = (float)(1.0 / ((double)a.scales[job] * (double)voxel));
    const float ax = a.anchors[(size_t)job * 3], ay = a.anchors[(size_t)job * 3 + 1], az = a.anchors[(size_t)job * 3 + 2];
    float ex[SR_PPL], ey[SR_PPL], ez[SR_PPL];
    bool dead[SR_PPL];
    const float inf = __builtin_inff();
#pragma unroll
    for (int k = 0; k < SR_PPL; ++k) {
        const int i = tid + k * SR_THREADS;
        ex[k] = ey[k] = ez[k] = 0.f;
        dead[k] = true;
        if (i < n) {
            const float *p = a.clouds + ((size_t)job * a.n_cap + i) * 3;
            const float x = p[0], y = p[1], z = p[2];
            dead[k] = !(fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf);
            ex[k] = x - ax, ey[k] = y - ay, ez[k] = z - az;
        }
    }
    // The points that contribute get the records 0 .. live-1, in any order (the cost is an integer sum): a NaN row of a failed crop,
    // or a whole empty slot, then costs nothing to walk.  Each group does this for itself.
    int pos[SR_PPL], n_live = 0;
    {
        int *s_cnt = reinterpret_cast<int *>(s_mem + F3 + 16 + SR_GROUPS * (TGP_SEARCH_MAX_POINTS * 8 + SR_WAVES * 8)) + grp * SR_PPL * SR_WAVES;
        unsigned long long alive[SR_PPL];
#pragma unroll
        for (int k = 0; k < SR_PPL; ++k) {
            alive[k] = __ballot(!dead[k]);
            if (lane == 0) s_cnt[k * SR_WAVES + wave] = __popcll(alive[k]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SR_PPL; ++k) {
            int before = 0;
            for (int e = 0; e < k * SR_WAVES + wave; ++e) before += s_cnt[e];
            pos[k] = dead[k] ? -1 : before + __popcll(alive[k] & ((1ull << lane) - 1ull));
        }
        for (int e = 0; e < SR_PPL * SR_WAVES; ++e) n_live += s_cnt[e];
    }
    const int n4 = (n_live + 3) & ~3;                            // <= TGP_SEARCH_MAX_POINTS, a multiple of 4 itself
    if (tid < n4 - n_live) s_base[n_live + tid] = make_uint2(1u << 30, 0u);       // fields 0: off the grid under every shift; bit 30: costs 0
    const int side = 2 * a.K + 1, D = side * side * side;
    const float half = (float)(G / 2);

    // group grp takes the rotations r0 + grp, r0 + grp + SR_GROUPS, ...; every group makes every trip, for the barriers
    for (int rb = r0; rb < r1; rb += SR_GROUPS) {
        const int r = rb + grp;
        const bool mine = r < r1;
        if (mine) {
            const float *Rm = a.rotations + (size_t)r * 9;
            const float R0 = Rm[0], R1 = Rm[1], R2 = Rm[2], R3 = Rm[3], R4 = Rm[4], R5 = Rm[5], R6 = Rm[6], R7 = Rm[7], R8 = Rm[8];
#pragma unroll
            for (int k = 0; k < SR_PPL; ++k) {
                if (pos[k] >= 0) {
                    float wx = (R0 * ex[k] + R3 * ey[k]) + R6 * ez[k];
                    float wy = (R1 * ex[k] + R4 * ey[k]) + R7 * ez[k];
                    float wz = (R2 * ex[k] + R5 * ey[k]) + R8 * ez[k];
                    wx = wx * inv + half, wy = wy * inv + half, wz = wz * inv + half;
                    // the contract clamps to [-512, 511] (fmaxf / fminf return the other operand for a NaN: a NaN goes to -512); a
                    // base at or beyond [-256, 255] is off the grid under every shift either way (SR_MAX_REACH), so it may stand there
                    const int bx = min(max((int)floorf(fminf(fmaxf(wx, -512.f), 511.f)), -SR_BIAS), SR_BIAS - 1),
                              by = min(max((int)floorf(fminf(fmaxf(wy, -512.f), 511.f)), -SR_BIAS), SR_BIAS - 1),
                              bz = min(max((int)floorf(fminf(fmaxf(wz, -512.f), 511.f)), -SR_BIAS), SR_BIAS - 1);
                    uint2 rec;
                    rec.x = (uint32_t)(bx + SR_BIAS) | ((uint32_t)(by + SR_BIAS) << 10) | ((uint32_t)(bz + SR_BIAS) << 20);
                    rec.y = (uint32_t)((bx * G + by) * PZ + bz);
                    s_base[pos[k]] = rec;
                }
            }
        }
        __syncthreads();                                         // the records (and, the first time, the field) are in LDS
        unsigned long long best = ~0ull;
        if (mine)
            for (int s0 = 0; s0 < D; s0 += SR_THREADS * SR_SH) {
                const int nk = min(SR_SH, (D - s0 + SR_THREADS - 1) / SR_THREADS);   // uniform
                unsigned long long key;
                if (nk == 4) key = walk<G, 4>(s_field, s_base, n4, s0 + tid, D, a.K, a.stride);
                else if (nk == 3) key = walk<G, 3>(s_field, s_base, n4, s0 + tid, D, a.K, a.stride);
                else if (nk == 2) key = walk<G, 2>(s_field, s_base, n4, s0 + tid, D, a.K, a.stride);
                else key = walk<G, 1>(s_field, s_base, n4, s0 + tid, D, a.K, a.stride);
                best = key < best ? key : best;
            }
        best = wave_min_u64(best);
        if (lane == 0) s_red[wave] = best;
        __syncthreads();                                         // every walk over the records is done as well
        if (mine && tid == 0) {
#pragma unroll
            for (int w = 1; w < SR_WAVES; ++w) best = s_red[w] < best ? s_red[w] : best;
            table[(size_t)r * 2] = (int32_t)(best >> 32);
            table[(size_t)r * 2 + 1] = (int32_t)(best & 0xffffffffu);
        }
    }
}

__global__ void __launch_bounds__(SR_THREADS) finish_kernel(tgp_pose_search_args a)
{
    __shared__ unsigned long long s_key[TGP_SEARCH_MAX_ROTATIONS];
    __shared__ unsigned long long s_red[2][SR_WAVES];
    __shared__ unsigned long long s_sel[TGP_SEARCH_MAX_TOP];
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & (TGP_WAVE - 1), wave = tid / TGP_WAVE;
    const int32_t *table = static_cast<const int32_t *>(a.workspace) + (size_t)job * a.R * 2;
    for (int r = tid; r < a.R; r += SR_THREADS) s_key[r] = ((unsigned long long)(uint32_t)table[(size_t)r * 2] << 32) | (uint32_t)r;
    __syncthreads();
    unsigned long long prev = 0;
    for (int t = 0; t < a.top; ++t) {
        unsigned long long best = ~0ull;
        for (int r = tid; r < a.R; r += SR_THREADS) {
            const unsigned long long key = s_key[r];
            if ((t == 0 || key > prev) && key < best) best = key;
        }
        best = wave_min_u64(best);
        if (lane == 0) s_red[t & 1][wave] = best;
        __syncthreads();
        best = s_red[t & 1][0];
#pragma unroll
        for (int w = 1; w < SR_WAVES; ++w) best = s_red[t & 1][w] < best ? s_red[t & 1][w] : best;
        if (tid == 0) s_sel[t] = best;
        if (best == ~0ull) {                                     // the same in every thread: no rotation is left
            for (int u = t + 1 + tid; u < a.top; u += SR_THREADS) s_sel[u] = ~0ull;
            break;
        }
        prev = best;
    }
    __syncthreads();
    const int jm = a.job_model[job];
    const bool model_ok = jm >= 0 && jm < a.M;
    for (int e = tid; e < a.top * 3; e += SR_THREADS) {
        const int t = e / 3, i = e % 3;
        const unsigned long long key = s_sel[t];
        const int cost = (int)(key >> 32);
        const size_t row = (size_t)job * a.top + t;
        float *P = a.poses + row * 12 + i * 4;
        if (key == ~0ull || cost == INT_MAX32 || !model_ok) {
            if (i == 0) a.cost[row] = INT_MAX32, a.rot[row] = -1, a.shift[row] = -1;
            P[0] = P[1] = P[2] = P[3] = __builtin_nanf("");
            continue;
        }
        const int r = (int)(key & 0xffffffffu), sidx = table[(size_t)r * 2 + 1];
        if (i == 0) a.cost[row] = cost, a.rot[row] = r, a.shift[row] = sidx;
        const int side = 2 * a.K + 1;
        const int d[3] = {(sidx / (side * side) - a.K) * a.stride, ((sidx / side) % side - a.K) * a.stride, (sidx % side - a.K) * a.stride};
        const float *mt = a.meta + (size_t)jm * 4;
        const double voxel = (double)mt[3], s = (double)a.scales[job];
        const double m0 = (double)mt[0] + (double)d[0] * voxel, m1 = (double)mt[1] + (double)d[1] * voxel, m2 = (double)mt[2] + (double)d[2] * voxel;
        const float *Rm = a.rotations + (size_t)r * 9 + i * 3;
        const double Rm0 = (double)Rm[0], Rm1 = (double)Rm[1], Rm2 = (double)Rm[2];
        P[0] = Rm[0], P[1] = Rm[1], P[2] = Rm[2];
        P[3] = (float)((double)a.anchors[(size_t)job * 3 + i] - s * ((Rm0 * m0 + Rm1 * m1) + Rm2 * m2));
    }
}

template <int G>
int search_launch(const tgp_pose_search_args &a, hipStream_t st)
{
    static TgpLdsAttr attr;
    constexpr int lds = search_lds(G);
    static_assert(lds <= 160 * 1024 && SR_PAD % 4 == 0 && TGP_SEARCH_ROT_BLOCK % SR_GROUPS == 0, "one field, SR_GROUPS record tables");
    if (lds > 64 * 1024)
        if (const int e = tgp_lds_attr(attr, reinterpret_cast<const void *>(search_kernel<G>), lds)) return e;
    hipLaunchKernelGGL(search_kernel<G>, dim3(tgp_cdiv(a.R, TGP_SEARCH_ROT_BLOCK), a.J), dim3(SR_THREADS * SR_GROUPS), lds, st, a);
    if (const int e = TGP_LAUNCH_RESULT()) return e;
    hipLaunchKernelGGL(finish_kernel, dim3(a.J), dim3(SR_THREADS), 0, st, a);
    return TGP_LAUNCH_RESULT();
}

bool grid_ok(int G) { return G == 16 || G == 32 || G == 48; }

}  // namespace

extern "C" int tgp_field_build(const tgp_field_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->models && a->meta && a->thresholds && a->field);
    TGP_REQUIRE(a->M >= 1 && a->m_cap >= 1 && a->cap >= 1 && a->cap <= 255);
    if (!grid_ok(a->G) || a->m_cap > TGP_ICP_MAX_POINTS || a->M > 65535) return TGP_EUNSUPPORTED;
    static_assert((16 * 16 * 16) % FB_THREADS == 0 && (48 * 48 * 48) % FB_THREADS == 0, "a thread per voxel, no tail");
    hipLaunchKernelGGL(field_kernel, dim3(a->G * a->G * a->G / FB_THREADS, a->M), dim3(FB_THREADS), 0, tgp_hs(stream), *a);
    return TGP_LAUNCH_RESULT();
}

extern "C" int64_t tgp_pose_search_workspace_bytes(int J, int R)
{
    if (J < 1 || R < 1) return TGP_EINVAL;
    if (J > 65535 || R > TGP_SEARCH_MAX_ROTATIONS) return TGP_EUNSUPPORTED;
    return (int64_t)J * R * 2 * (int64_t)sizeof(int32_t);
}

extern "C" int tgp_pose_search(const tgp_pose_search_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->field && a->meta && a->job_model && a->clouds && a->anchors && a->scales && a->rotations);
    TGP_REQUIRE(a->cost && a->rot && a->shift && a->poses && a->workspace);
    TGP_REQUIRE(a->M >= 1 && a->J >= 1 && a->R >= 1 && a->n_cap >= 1 && a->top >= 1 && a->K >= 0 && a->stride >= 1 && a->cap >= 1 && a->cap <= 255);
    TGP_REQUIRE((reinterpret_cast<uintptr_t>(a->field) & 15) == 0 && (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0);
    if (!grid_ok(a->G) || a->n_cap > TGP_SEARCH_MAX_POINTS || a->R > TGP_SEARCH_MAX_ROTATIONS || a->top > TGP_SEARCH_MAX_TOP ||
        a->K > TGP_SEARCH_MAX_K || (int64_t)a->K * a->stride > TGP_SEARCH_MAX_REACH || a->J > 65535)
        return TGP_EUNSUPPORTED;
    TGP_REQUIRE(a->workspace_bytes >= tgp_pose_search_workspace_bytes(a->J, a->R));
    static_assert(SR_PPL * SR_THREADS == TGP_SEARCH_MAX_POINTS && SR_MAX_REACH == TGP_SEARCH_MAX_REACH, "every point has a lane");
    if (a->G == 16) return search_launch<16>(*a, tgp_hs(stream));
    if (a->G == 32) return search_launch<32>(*a, tgp_hs(stream));
    return search_launch<48>(*a, tgp_hs(stream));
}
