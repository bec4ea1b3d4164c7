// Earth mover's distance by auction matching (losses/metrics/EMD: emd_cuda.cu Bid / GetMax / Assign / CalcDist, the algorithm
// of Liu et al.) on gfx950.
//
// The reference runs 7 launches per iteration with global atomics, accepts only n % 1024 == 0 and B <= 512.  Here ONE workgroup of
// 1024 threads owns a cloud pair and keeps the pair's whole state in LDS -- the target cloud as float4, prices, the per-object maximum
// increment and winner, both assignment directions, bids, increments and the list of unassigned points: 48 bytes per point, 96 KB at
// the cap of 2048 points -- and runs every iteration and the final distance pass inside one launch, for any 1 <= n <= cap and any B.
// Nothing waits on another workgroup; every loop is bounded by iters and n.
//
// Arithmetic (DESIGN.md "EMD" is the contract): d = (float)(3.0 - (double)sqrtf((dx*dx + dy*dy) + dz*dz) - (double)price[k]) with
// every fp32 operation rounded on its own; `best` is the maximum at the lowest k that reaches it, `better` the second largest counting
// duplicates (-1e9f when there is none).  A bidder's k range is dealt to L lanes (L a power of two, as many as the unassigned count
// leaves room for); the partial (best, k, better) triples are merged by a rule that is symmetric and associative, so L changes
// neither value.  The reference resolves the winner of an object by a write race; here the lowest bidder inside its 1e-6 window wins
// (integer atomicMin in LDS).  The per-object maximum is an integer atomicMax on the order-preserving key of the float: there are no
// float atomics, and every result is independent of the order in which lanes arrive.
#include "tgp_common.h"

#include <limits.h>

#define EMD_THREADS 1024
#define EMD_MAX_POINTS 2048
#define EMD_BYTES_PER_POINT 48 // float4 target + 8 words of state
#define EMD_NONE (-1e9f)

__device__ __forceinline__ void emd_merge(float &best, int &bk, float &better, float ob, int ok, float ot)
{
    // (best, first k that reaches it, second largest with duplicates) of the union of two disjoint k sets
    const float lo = fminf(best, ob);
    if (ob > best || (ob == best && ok < bk)) best = ob, bk = ok;
    better = fmaxf(lo, fmaxf(better, ot));
}

__global__ __launch_bounds__(EMD_THREADS) void emd_fwd_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int n,
                                                              float eps, int iters, float *__restrict__ dist,
                                                              int32_t *__restrict__ assignment)
{
    extern __shared__ float4 emd_lds[];
    __shared__ int cnt[2];
    float4 *c2 = emd_lds;
    float *price = reinterpret_cast<float *>(c2 + n);
    uint32_t *maxkey = reinterpret_cast<uint32_t *>(price + n); // max_increments as tgp_float_key
    int *winner = reinterpret_cast<int *>(maxkey + n);
    int *assign = winner + n;
    int *ainv = assign + n;
    int *bid = ainv + n;
    float *inc = reinterpret_cast<float *>(bid + n);
    int *list = reinterpret_cast<int *>(inc + n);

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const float *p1 = xyz1 + b * n * 3;
    const float *p2 = xyz2 + b * n * 3;
    for (int k = tid; k < n; k += EMD_THREADS) {
        c2[k] = make_float4(p2[k * 3 + 0], p2[k * 3 + 1], p2[k * 3 + 2], 0.f);
        price[k] = 0.f;
        maxkey[k] = tgp_float_key(0.f);
        winner[k] = INT_MAX;
        assign[k] = -1;
        ainv[k] = -1;
    }
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();

    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        // the unassigned points (in arrival order: no result depends on the order of this list)
        if (tid == 0) cnt[(it + 1) & 1] = 0;
        for (int j = tid; j < n; j += EMD_THREADS)
            if (assign[j] == -1) list[atomicAdd(&cnt[it & 1], 1)] = j;
        __syncthreads();
        const int U = cnt[it & 1];
        if (U == 0) break; // a complete matching: the remaining iterations would change nothing

        // ---- Bid: L lanes per bidder, lane `sub` takes k = sub, sub + L, ...
        int lg = 0;
        while (lg < 6 && (U << (lg + 1)) <= EMD_THREADS) ++lg;
        const int L = 1 << lg, G = EMD_THREADS >> lg;
        const int sub = tid & (L - 1);
        for (int base = 0; base < U; base += G) {
            const int g = base + (tid >> lg);
            const bool active = g < U;
            const int j = active ? list[g] : 0;
            float best = EMD_NONE, better = EMD_NONE;
            int bk = INT_MAX;
            if (active) {
                const float x1 = p1[j * 3 + 0], y1 = p1[j * 3 + 1], z1 = p1[j * 3 + 2];
                for (int k = sub; k < n; k += L) {
                    const float4 c = c2[k];
                    const float dx = c.x - x1, dy = c.y - y1, dz = c.z - z1;
                    const float s = (dx * dx + dy * dy) + dz * dz;
                    const float d = (float)(3.0 - (double)sqrtf(s) - (double)price[k]);
                    if (d > best) {
                        better = best;
                        best = d;
                        bk = k;
                    } else if (d > better) {
                        better = d;
                    }
                }
            }
            for (int m = 1; m < L; m <<= 1) { // groups are L consecutive lanes of one wave
                const float ob = __shfl_xor(best, m, TGP_WAVE), ot = __shfl_xor(better, m, TGP_WAVE);
                const int ok = __shfl_xor(bk, m, TGP_WAVE);
                emd_merge(best, bk, better, ob, ok, ot);
            }
            if (active && sub == 0) {
                if (bk >= n) bk = 0; // no d compared above -1e9 (non-finite input): stay inside the arrays
                const float v = (best - better) + eps;
                bid[j] = bk;
                inc[j] = v;
                winner[bk] = INT_MAX;
                atomicMax(&maxkey[bk], tgp_float_key(v));
            }
        }
        __syncthreads();

        // ---- winner per object: the lowest bidder whose increment is within 1e-6 of the object's maximum
        for (int g = tid; g < U; g += EMD_THREADS) {
            const int j = list[g];
            const int k = bid[j];
            const double bi = (double)inc[j], mx = (double)tgp_key_float(maxkey[k]);
            if (bi - 1e-6 <= mx && mx <= bi + 1e-6) atomicMin(&winner[k], j);
        }
        __syncthreads();

        // ---- Assign
        for (int g = tid; g < U; g += EMD_THREADS) {
            const int j = list[g];
            const int k = bid[j];
            if (last) {
                assign[j] = k; // every bidder takes its object: the result need not be a bijection
            } else if (winner[k] == j) {
                const int old = ainv[k];
                if (old != -1) assign[old] = -1;
                ainv[k] = j;
                assign[j] = k;
                price[k] = price[k] + inc[j];
                maxkey[k] = tgp_float_key(EMD_NONE);
            }
        }
        __syncthreads();
    }

    for (int j = tid; j < n; j += EMD_THREADS) {
        const int a = assign[j];
        const float4 c = c2[a];
        const float dx = p1[j * 3 + 0] - c.x, dy = p1[j * 3 + 1] - c.y, dz = p1[j * 3 + 2] - c.z;
        dist[b * n + j] = (dx * dx + dy * dy) + dz * dz;
        assignment[b * n + j] = a;
    }
}

__global__ __launch_bounds__(256) void emd_bwd_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                      const float *__restrict__ grad_dist, const int32_t *__restrict__ assignment,
                                                      int64_t total, int n, float *__restrict__ grad_xyz1)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t i2 = (i / n) * n + assignment[i];
    const float g = grad_dist[i] * 2;
    grad_xyz1[i * 3 + 0] = g * (xyz1[i * 3 + 0] - xyz2[i2 * 3 + 0]);
    grad_xyz1[i * 3 + 1] = g * (xyz1[i * 3 + 1] - xyz2[i2 * 3 + 1]);
    grad_xyz1[i * 3 + 2] = g * (xyz1[i * 3 + 2] - xyz2[i2 * 3 + 2]);
}

extern "C" int tgp_emd_max_points(void) { return EMD_MAX_POINTS; }

// The pair's state lives in LDS: no global scratch is needed up to the cap.
extern "C" int64_t tgp_emd_workspace_bytes(int B, int n) { return 0; }

extern "C" int tgp_emd_fwd(const float *xyz1, const float *xyz2, int B, int n, float eps, int iters, float *dist,
                           int32_t *assignment, void *ws, tgp_stream_t stream)
{
    TGP_REQUIRE(xyz1 && xyz2 && dist && assignment && B > 0 && n > 0 && iters > 0);
    if (n > EMD_MAX_POINTS) return TGP_EUNSUPPORTED;
    static TgpLdsAttr attr;
    if (const int e = tgp_lds_attr(attr, reinterpret_cast<const void *>(emd_fwd_kernel), EMD_MAX_POINTS * EMD_BYTES_PER_POINT))
        return e;
    hipLaunchKernelGGL(emd_fwd_kernel, dim3(B), dim3(EMD_THREADS), (size_t)n * EMD_BYTES_PER_POINT, tgp_hs(stream), xyz1, xyz2, n,
                       eps, iters, dist, assignment);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_emd_bwd(const float *xyz1, const float *xyz2, const float *grad_dist, const int32_t *assignment, int B, int n,
                           float *grad_xyz1, tgp_stream_t stream)
{
    TGP_REQUIRE(xyz1 && xyz2 && grad_dist && assignment && grad_xyz1 && B > 0 && n > 0);
    const int64_t total = (int64_t)B * n;
    TGP_REQUIRE(total <= (int64_t)INT_MAX * 256);
    hipLaunchKernelGGL(emd_bwd_kernel, dim3(tgp_cdiv(total, 256)), dim3(256), 0, tgp_hs(stream), xyz1, xyz2, grad_dist, assignment,
                       total, n, grad_xyz1);
    return TGP_LAUNCH_RESULT();
}
