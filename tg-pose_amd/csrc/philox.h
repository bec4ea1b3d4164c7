// The keyed generator every device draw comes from (draws.hip, meshsample.hip): Philox-4x32-10 (Salmon et al., "Parallel random
// numbers: as easy as 1, 2, 3", SC'11) with the 64-bit seed as its key and (counter, site, key low, key high) as its 128-bit counter,
// and the transforms of its words into uniforms.  datasets/device_draws.py restates them in NumPy bit for bit.
#pragma once
#include "tgp_common.h"

namespace {

struct Words {
    uint32_t w[4];
};

__device__ __forceinline__ Words philox(uint64_t seed, uint64_t key, uint32_t site, uint32_t counter)
{
    uint32_t c0 = counter, c1 = site, c2 = (uint32_t)key, c3 = (uint32_t)(key >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

// torch.rand's float32 law: 24 random bits, [0, 1)
__device__ __forceinline__ float uniform_f32(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }
// NumPy's random_sample law: 53 random bits, [0, 1)
__device__ __forceinline__ double uniform_f64(uint32_t a, uint32_t b)
{
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

}  // namespace
