// The arithmetic that turns a source pixel and its depth into a camera-frame point, and the keyed permutation of the device
// resampling: shared by the ROI crop (inputside.hip) and the ball crop (ballcrop.hip), so that the same pixel gives the same bits
// on both paths.
#pragma once
#include "tgp_common.h"

// x / b for a divisor that is uniform over the launch: the refined reciprocal of the compiler's IEEE division sequence
// (v_rcp_f32 + one Newton step) is computed once, and each quotient is that sequence's remaining five operations --
// q = a*r; q += fma(-b,q,a)*r; q += fma(-b,q,a)*r -- i.e. exactly what `a / b` compiles to when v_div_scale / v_div_fixup
// are no-ops (operands far from overflow / denormals: pixel coordinates x millimetres over focal lengths and 1000).
// Correctly rounded there; the parity tests compare bit patterns with numpy's division over ~10^6 quotients.
struct UniformDiv {
    float b, r;
    __device__ __forceinline__ explicit UniformDiv(float divisor) : b(divisor)
    {
        const float r0 = __builtin_amdgcn_rcpf(divisor);
        r = fmaf(fmaf(-divisor, r0, 1.0f), r0, r0);
    }
    __device__ __forceinline__ float operator()(float a) const
    {
        float q = a * r;
        q = fmaf(fmaf(-b, q, a), r, q);
        return fmaf(fmaf(-b, q, a), r, q);
    }
};

// _depth_to_pcl (load_data_eval.py:451-462) then /1000.0 (:338) for source pixel (sx, sy) with depth dep (millimetres as a float):
// float32 step by step, correctly rounded quotients.
__device__ __forceinline__ void tgp_pixel_point(int sx, int sy, float dep, float cx, float cy, const UniformDiv &div_fx,
                                                const UniformDiv &div_fy, const UniformDiv &div_k, float &px, float &py, float &pz)
{
    px = div_k(div_fx(((float)sx - cx) * dep));
    py = div_k(div_fy(((float)sy - cy) * dep));
    pz = div_k(dep);
}

// A keyed bijection of [0, 2^(2 half_bits)) (four Feistel rounds); cycle-walked into [0, total) it gives element i of a
// pseudo-random permutation statelessly (tgp_cloud_sample, tgp_ball_sample).
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
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

// the per-item key of that permutation
__device__ __forceinline__ uint32_t tgp_sample_key(uint64_t seed, int j)
{
    return mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + 0x632be5abu * (uint32_t)(j + 1)));
}
