// The training batch's random draws on the device (datasets/load_data.py train_batch(draws='device')).
//
// Every draw is a pure function of (seed, item key, draw site, counter): Philox-4x32-10 (Salmon et al., "Parallel random numbers:
// as easy as 1, 2, 3", SC'11) with the 64-bit seed as its key and (counter, site, key low, key high) as its 128-bit counter.  No
// state, no stream: an item's draws do not depend on its slot, its batch or the rank that builds it.  Philox rather than the mix32
// hash of inputside.hip for the VALUES because its statistical quality is established (BigCrush) and its ten rounds are two
// 32 x 32 -> 64 multiplies each, which a few lines of NumPy restate bit for bit (datasets/device_draws.py); the hash stays what
// it was, the round function of the Feistel bijection that turns one Philox word into a permutation.
//
// The kernels FILL the buffers the host path uploads (drop_bits, selections, defor, noise, drop_u), so tgp_roi_cloud_defor,
// tgp_cloud_select_ex, tgp_augment and tgp_gather_rows run unchanged.  One launch per stage for the batch, no atomics, nothing
// allocated, results bit-repeatable.
#include "tgp_common.h"
#include "philox.h"

namespace {

// Box-Muller on 24-bit uniforms, u1 in (0, 1): |z| <= sqrt(-2 ln 2^-25) = 5.89 standard deviations
__device__ __forceinline__ void normal_pair(uint32_t a, uint32_t b, float &z0, float &z1)
{
    const float u1 = ((float)(a >> 8) + 0.5f) * 5.9604644775390625e-8f, u2 = uniform_f32(b);
    const float r = sqrtf(-2.0f * logf(u1)), t = 6.283185307179586f * u2;
    z0 = r * cosf(t), z1 = r * sinf(t);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
// the keyed bijection of [0, 2^(2 half_bits)) that cloud_sample_kernel walks (inputside.hip), and its inverse
__device__ __forceinline__ uint32_t feistel(uint32_t v, int half_bits, uint32_t key)
{
    const uint32_t mask = (1u << half_bits) - 1u;
    uint32_t l = v >> half_bits, r = v & mask;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
        const uint32_t f = mix32(r ^ (key + 0x9e3779b9u * (round + 1))) & mask;
        const uint32_t nl = r;
        r = l ^ f;
        l = nl;
    }
    return (l << half_bits) | r;
}
__device__ __forceinline__ uint32_t feistel_inv(uint32_t v, int half_bits, uint32_t key)
{
    const uint32_t mask = (1u << half_bits) - 1u;
    uint32_t l = v >> half_bits, r = v & mask;
#pragma unroll
    for (int round = 3; round >= 0; --round) {
        const uint32_t f = mix32(l ^ (key + 0x9e3779b9u * (round + 1))) & mask;
        const uint32_t nr = l;
        l = r ^ f;
        r = nr;
    }
    return (l << half_bits) | r;
}
__device__ __forceinline__ int half_bits_of(uint32_t total)
{
    int h = 1;
    while ((1u << (2 * h)) < total) ++h;
    return h;
}
// element i of the permutation of [0, total): cycle walking (the bijection's domain is below 4 x total, the walk ends)
__device__ __forceinline__ uint32_t perm_at(uint32_t i, uint32_t total, int h, uint32_t key)
{
    uint32_t k = feistel(i, h, key);
    while (k >= total) k = feistel(k, h, key);
    return k;
}
// the position of element v in that permutation
__device__ __forceinline__ uint32_t perm_pos(uint32_t v, uint32_t total, int h, uint32_t key)
{
    uint32_t k = feistel_inv(v, h, key);
    while (k >= total) k = feistel_inv(k, h, key);
    return k;
}

__global__ void words_kernel(const uint64_t *__restrict__ keys, uint64_t seed, uint32_t site, int n, int64_t total, uint32_t *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const Words w = philox(seed, keys[t / n], site, (uint32_t)(t % n));
    out[t * 4] = w.w[0], out[t * 4 + 1] = w.w[1], out[t * 4 + 2] = w.w[2], out[t * 4 + 3] = w.w[3];
}

// defor_2D's choice(l, l // 2, replace=False) as a bitmap over band ranks: rank r is dropped iff its position in the item's
// permutation of [0, l) is below l // 2 -- exactly l // 2 bits.  A wave's 64 ranks are two words of the ballot.
__global__ void __launch_bounds__(256) band_subset_kernel(const int *__restrict__ band_counts, const double *__restrict__ u, double pro,
                                                          const uint64_t *__restrict__ keys, uint64_t seed, int validity,
                                                          int *__restrict__ defor_on, uint32_t *__restrict__ drop_bits, int drop_words)
{
    const int d = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;            // < 32 * drop_words (the grid covers whole words)
    const int n_depth = band_counts[d * 3], n_valid = band_counts[d * 3 + 1];
    const int l = min(max(band_counts[d * 3 + 2], 0), 32 * drop_words);
    const bool on = (!validity || (n_depth > 1 && n_valid > 1)) && !(u[d] > pro) && l >= 1;
    if (r == 0) defor_on[d] = on;
    bool drop = false;
    if (on && r < l) {
        const uint32_t key = philox(seed, keys[d], TGP_SITE_BAND, 0).w[0];
        drop = perm_pos((uint32_t)r, (uint32_t)l, half_bits_of((uint32_t)l), key) < (uint32_t)(l >> 1);
    }
    const unsigned long long m = __ballot(drop);
    if ((threadIdx.x & 63) == 0) {
        uint32_t *o = drop_bits + (size_t)d * drop_words + (r >> 5);
        o[0] = (uint32_t)m, o[1] = (uint32_t)(m >> 32);
    }
}

// _item_total's rules on the device, the first B alive items in item order, cyclic repeats when fewer are alive
constexpr int ALIVE_THREADS = 1024;
__global__ void __launch_bounds__(ALIVE_THREADS) alive_kernel(const int *__restrict__ counts, const int *__restrict__ forced, int D, int B,
                                                              int min_points, int *__restrict__ status, int *__restrict__ slot_item,
                                                              int *__restrict__ n_alive)
{
    __shared__ int list[TGP_DRAW_MAX_ITEMS];
    __shared__ int wtot[ALIVE_THREADS / TGP_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int d0 = 0; d0 < D; d0 += ALIVE_THREADS) {
        const int d = d0 + tid;
        int st = -1;
        if (d < D) {
            const int n_depth = counts[d * 3], n_valid = counts[d * 3 + 1], total = counts[d * 3 + 2];
            st = TGP_ITEM_ALIVE;
            if (forced && forced[d] != 0) st = forced[d];
            else if (n_depth <= 1) st = TGP_ITEM_NO_DEPTH;
            else if (n_valid <= 1) st = TGP_ITEM_NO_MASK;
            else if (total < 0) st = TGP_ITEM_BELOW_26;
            else if (total < min_points) st = TGP_ITEM_FEW_POINTS;
            status[d] = st;
        }
        const unsigned long long m = __ballot(st == TGP_ITEM_ALIVE);
        __syncthreads();
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        int off = base, all = 0;
        for (int w = 0; w < ALIVE_THREADS / TGP_WAVE; ++w) {
            off += w < wave ? wtot[w] : 0;
            all += wtot[w];
        }
        if (st == TGP_ITEM_ALIVE) list[off + __popcll(m & ((1ull << lane) - 1ull))] = d;       // < D <= TGP_DRAW_MAX_ITEMS
        base += all;
    }
    __syncthreads();
    if (tid == 0) *n_alive = min(base, B);
    for (int s = tid; s < B; s += ALIVE_THREADS) slot_item[s] = base > 0 ? list[s < base ? s : s % base] : -1;
}

// _sample_points (shuffle_always 0: tile when short, identity at n_out, else a permutation's prefix) and pc_sampler
// (shuffle_always 1: always the permutation; slots past total walk it again, i % total)
__global__ void selection_kernel(const int *__restrict__ totals, int ld_total, int total_const, const uint64_t *__restrict__ keys,
                                 uint64_t seed, uint32_t site, int64_t count, int n_out, int shuffle_always, int *__restrict__ sel)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int d = (int)(t / n_out), i = (int)(t % n_out);
    const int total = min(totals ? totals[(size_t)d * ld_total] : total_const, TGP_DRAW_MAX_TOTAL);
    int k = 0;
    if (total > 0) {
        if (!shuffle_always && total <= n_out) {
            k = total == n_out ? i : i % total;
        } else {
            const uint32_t key = philox(seed, keys[d], site, 0).w[0];
            k = (int)perm_at((uint32_t)(i % total), (uint32_t)total, half_bits_of((uint32_t)total), key);
        }
    }
    sel[t] = k;
}

// per point i of item d (counter = i): defor_3D_pc's three uniforms, PcJitter's three clamped normals, PcRandomDropout's uniform
__global__ void fill_kernel(const uint64_t *__restrict__ keys, uint64_t seed, int64_t count, int N, float *__restrict__ defor,
                            float *__restrict__ noise, float std, float clip, double *__restrict__ drop_u)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint64_t key = keys[t / N];
    const uint32_t i = (uint32_t)(t % N);
    if (defor) {
        const Words w = philox(seed, key, TGP_SITE_DEFOR, i);
        defor[t * 3] = uniform_f32(w.w[0]), defor[t * 3 + 1] = uniform_f32(w.w[1]), defor[t * 3 + 2] = uniform_f32(w.w[2]);
    }
    if (noise) {
        const Words w = philox(seed, key, TGP_SITE_NOISE, i);
        float z0, z1, z2, z3;
        normal_pair(w.w[0], w.w[1], z0, z1);
        normal_pair(w.w[2], w.w[3], z2, z3);
        noise[t * 3] = fminf(fmaxf(z0 * std, -clip), clip);
        noise[t * 3 + 1] = fminf(fmaxf(z1 * std, -clip), clip);
        noise[t * 3 + 2] = fminf(fmaxf(z2 * std, -clip), clip);
    }
    if (drop_u) {
        const Words w = philox(seed, key, TGP_SITE_DROP, i);
        drop_u[t] = uniform_f64(w.w[0], w.w[1]);
    }
}

// out[s] = rows[slot_item[s]] for up to TGP_GATHER_SLOTS_MAX tensors of 32-bit words; a slot without an item (-1) gets zeros
__global__ void gather_slots_kernel(tgp_gather_slots_args a)
{
    const int s = blockIdx.x, k = blockIdx.y;
    const int item = a.slot_item[s];
    const int words = a.row_words[k];
    const uint32_t *src = (const uint32_t *)a.src[k] + (size_t)max(item, 0) * words;
    uint32_t *dst = (uint32_t *)a.dst[k] + (size_t)s * words;
    const bool live = item >= 0 && item < a.D;
    for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = live ? src[i] : 0u;
}

}  // namespace

extern "C" int tgp_draw_words(const uint64_t *keys, int D, uint64_t seed, uint32_t site, int n_counters, uint32_t *out, tgp_stream_t stream)
{
    TGP_REQUIRE(keys && out && D > 0 && n_counters > 0);
    const int64_t total = (int64_t)D * n_counters;
    hipLaunchKernelGGL(words_kernel, dim3(tgp_cdiv(total, 256)), dim3(256), 0, tgp_hs(stream), keys, seed, site, n_counters, total, out);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_draw_band_subset(const int *band_counts, const double *u, double pro, const uint64_t *keys, uint64_t seed, int D,
                                    int validity, int *defor_on, uint32_t *drop_bits, int drop_words, tgp_stream_t stream)
{
    TGP_REQUIRE(band_counts && u && keys && defor_on && drop_bits && D > 0 && D <= 65535);
    TGP_REQUIRE(drop_words >= 8 && drop_words <= 2048 && drop_words % 8 == 0 && pro >= 0.0 && pro <= 1.0);      // whole 256-rank blocks
    hipLaunchKernelGGL(band_subset_kernel, dim3(drop_words / 8, D), dim3(256), 0, tgp_hs(stream), band_counts, u, pro, keys, seed, validity,
                       defor_on, drop_bits, drop_words);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_draw_alive(const int *counts, const int *forced, int D, int B, int min_points, int *status, int *slot_item, int *n_alive,
                              tgp_stream_t stream)
{
    TGP_REQUIRE(counts && status && slot_item && n_alive && D > 0 && D <= TGP_DRAW_MAX_ITEMS && B > 0 && B <= D && min_points >= 0);
    hipLaunchKernelGGL(alive_kernel, dim3(1), dim3(ALIVE_THREADS), 0, tgp_hs(stream), counts, forced, D, B, min_points, status, slot_item,
                       n_alive);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_draw_selection(const int *totals, int ld_total, int total_const, const uint64_t *keys, uint64_t seed, uint32_t site, int D,
                                  int n_out, int shuffle_always, int32_t *sel, tgp_stream_t stream)
{
    TGP_REQUIRE(keys && sel && D > 0 && n_out > 0 && (totals ? ld_total >= 1 : total_const >= 0));
    const int64_t count = (int64_t)D * n_out;
    hipLaunchKernelGGL(selection_kernel, dim3(tgp_cdiv(count, 256)), dim3(256), 0, tgp_hs(stream), totals, ld_total, total_const, keys, seed,
                       site, count, n_out, shuffle_always, sel);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_draw_fill(const uint64_t *keys, uint64_t seed, int D, int N, float *defor, float *noise, float std, float clip,
                             double *drop_u, tgp_stream_t stream)
{
    TGP_REQUIRE(keys && D > 0 && N > 0 && (defor || noise || drop_u) && (!noise || (std >= 0.f && clip >= 0.f)));
    const int64_t count = (int64_t)D * N;
    hipLaunchKernelGGL(fill_kernel, dim3(tgp_cdiv(count, 256)), dim3(256), 0, tgp_hs(stream), keys, seed, count, N, defor, noise, std, clip,
                       drop_u);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_gather_slots(const tgp_gather_slots_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->slot_item && a->B > 0 && a->D > 0 && a->n >= 1 && a->n <= TGP_GATHER_SLOTS_MAX);
    for (int k = 0; k < a->n; ++k) TGP_REQUIRE(a->src[k] && a->dst[k] && a->row_words[k] > 0 && a->src[k] != a->dst[k]);
    hipLaunchKernelGGL(gather_slots_kernel, dim3(a->B, a->n), dim3(256), 0, tgp_hs(stream), *a);
    return TGP_LAUNCH_RESULT();
}
