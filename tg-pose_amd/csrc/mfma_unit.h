// What the hand-scheduled MFMA kernels (heads_fused.hip, dec_fused.hip, hs_chain.hip; gemm_pp.hip for the waits, the range rule and
// the LDS-DMA) share: the vector types, the fp16 hi / lo split by mixed-precision fma, the s_waitcnt encoder, the fp16 block range
// rule, the LDS-DMA piece and the staging-unit body.  Everything here is forced inline or a macro: a kernel's instruction stream is
// what the same text written out in its file gives.
#pragma once
#include "tgp_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));      // (gemm_epi.h declares the same four names for the tile kernels)
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define TGP_SB() __builtin_amdgcn_sched_barrier(0)

// ---- fp16 hi / lo split of an fp32 value: hi = fp16(v), lo = fp16(v - hi); the difference by one mixed-precision fma per element
// (hi -> fp32 is exact, one rounding: the value a convert-and-subtract gives).  hpair: two packed fp16 values.
__device__ __forceinline__ float tgp_mix_lo(uint32_t hpair, float v)     // v - (float)(low half of hpair), one rounding
{
    float d;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hpair), "v"(v));
    return d;
}
__device__ __forceinline__ float tgp_mix_hi(uint32_t hpair, float v)     // v - (float)(high half of hpair)
{
    float d;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hpair), "v"(v));
    return d;
}
__device__ __forceinline__ void tgp_split4(const float4 v, uint2 &hi, uint2 &lo)     // four values -> their packed hi and lo halves
{
    const f32x4 x = {v.x, v.y, v.z, v.w};
    hi = __builtin_bit_cast(uint2, __builtin_convertvector(x, f16x4));
    const f32x4 rest = {tgp_mix_lo(hi.x, v.x), tgp_mix_hi(hi.x, v.y), tgp_mix_lo(hi.y, v.z), tgp_mix_hi(hi.y, v.w)};
    lo = __builtin_bit_cast(uint2, __builtin_convertvector(rest, f16x4));
}

// ---- the SIMM16 of s_waitcnt in the gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt (bits 6:4) left at "don't wait", lgkmcnt in
// bits 11:8 (15: don't wait).  Loads and stores share the one in-order vmcnt counter: vmcnt(n) leaves the n youngest in flight.
__host__ __device__ constexpr int tgp_waitcnt(int vm, int lgkm = 15) { return 0x0070 | (vm & 15) | ((vm >> 4) << 14) | ((lgkm & 15) << 8); }

// ---- fp16 block range rule, over the magnitude word a producer recorded (bits of max |a| of a 32-row block; or the largest word of
// a tile's blocks).  The two-term fp16 split is faithful only inside fp16's range: a magnitude >= 65504 (0x477fe000; every NaN's bits
// lie above) splits into inf, and a block with nothing at or above 2^-4 (0x3d800000) -- and not all zero -- loses relative precision
// in every product (its lo halves are subnormal or flushed).  Such a block is computed in fp32 by the caller, or raises its flag.
// (A macro: as an inline function the same condition reaches the optimiser in another shape and moves the kernels' instruction streams.)
#define TGP_FP16_OUT_OF_RANGE(AM) ((AM) >= 0x477fe000u || ((AM) != 0u && (AM) < 0x3d800000u))

// ---- one LDS-DMA piece: 64 lanes x 16 bytes from global memory into 1 KB of LDS at `lds` (lane l lands at lds + 16 l).  Inline
// assembly: opaque to the compiler's counters, so no vmcnt(0) appears before the LDS reads that follow; the waits are written by hand
// (tgp_waitcnt) before the barrier that publishes the pieces.  The LDS base travels in m0 as a register-constrained input.  The
// kernels' lambdas keep their own addressing (buffer stride, short last round, ring slot) and name the LDS address before the call:
// the order in which the two addresses are computed is part of the schedule.
__device__ __forceinline__ void tgp_lds_dma(const uint32_t voff, const char *src, const uint32_t lds)     // lane's source: src (scalar) + voff
{
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(src), "{m0}"(lds) : "memory");
}
__device__ __forceinline__ void tgp_lds_dma(const char *lane_src, const uint32_t lds)                     // ... a full address per lane
{
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(lane_src), "{m0}"(lds) : "memory");
}
// A fragment-blocked image is staged in rounds of four pieces: piece j = 4 j0 + wave is 1 KB at offset 1024 j of the image and of its
// LDS buffer, so round j0 of a wave is { vector offset voff0 + 4096 j0, scalar source base, LDS address lds0 + 4096 j0 }.
__device__ __forceinline__ uint32_t tgp_dma_voff0(const int lane, const int wave) { return lane * 16 + wave * 1024; }
__device__ __forceinline__ uint32_t tgp_dma_lds0(const char *smem, const int wave)
{
    return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem) + wave * 1024;
}

// ---- the staging-unit body.  A staging unit is NQ (K-step s, output block j) pairs of weight fragments in LDS, pair q = s * NB + j as
// two 1 KB pieces in lane order (hi at WROW + 2048 q, lo 1 KB behind; WROW already holds the lane's 16 bytes), packed by
// tgp_pack_units.  With one wave per SIMD whatever follows a run of MFMAs into the same accumulators hides behind its last one only,
// so every non-matrix instruction sits BETWEEN the dependent MFMAs, fenced by sched_barriers so that the compiler keeps it there.  Per
// pair three MFMAs into ACC[j], smallest terms first as in the tile kernel (W lo x A hi, W hi x A lo, W hi x A hi; BH / BL: the points'
// hi / lo fragments, expressions of s), and in the gaps behind them
//   gap 1: the weight fragments of pair q + 2 (two ahead: nothing else hides the LDS latency), then FILL_A;
//   gap 2: STAGE -- a DMA piece of a later unit --, then FILL_B;
//   gap 3: GAP3 -- TGP_UNIT_GAP(filler), or nothing at all: a unit without a third gap has ONE barrier between a pair's last MFMA
//          and the next pair's first (two barriers with nothing between them pin the allocation differently from one).
// The fillers are statement fragments that may name q, s and j.  TAIL ends the unit: what remains of the staging, the counted wait for
// this wave's share of the next unit (TGP_UNIT_END) and the barrier after which everybody's has landed and this buffer is free.
#define TGP_UNIT_BODY(WROW, NQ, NB, ACC, BH, BL, STAGE, FILL_A, FILL_B, GAP3, TAIL)                                          \
    {                                                                                                                        \
        const char *wrow = (WROW);                                                                                           \
        auto wfrag = [&](int q, int plane) { return *reinterpret_cast<const uint4 *>(wrow + (q * 2 + plane) * 1024); };      \
        uint4 wh0 = wfrag(0, 0), wl0 = wfrag(0, 1), wh1 = wfrag((NQ) > 1 ? 1 : 0, 0), wl1 = wfrag((NQ) > 1 ? 1 : 0, 1);      \
        TGP_SB();                                                                                                            \
        _Pragma("unroll") for (int q = 0; q < (NQ); ++q) {                                                                   \
            const int s = q / (NB), j = q % (NB);                                                                            \
            uint4 wh2 = wh1, wl2 = wl1;                                                                                      \
            const f16x8 bh = BH, bl = BL;                                                                                    \
            ACC[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wl0), bh, ACC[j], 0, 0, 0);            \
            TGP_SB();                                                                                                        \
            if (q + 2 < (NQ)) wh2 = wfrag(q + 2, 0), wl2 = wfrag(q + 2, 1);                                                  \
            FILL_A;                                                                                                          \
            TGP_SB();                                                                                                        \
            ACC[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh0), bl, ACC[j], 0, 0, 0);            \
            TGP_SB();                                                                                                        \
            STAGE;                                                                                                           \
            FILL_B;                                                                                                          \
            TGP_SB();                                                                                                        \
            ACC[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh0), bh, ACC[j], 0, 0, 0);            \
            TGP_SB();                                                                                                        \
            GAP3                                                                                                             \
            wh0 = wh1, wl0 = wl1, wh1 = wh2, wl1 = wl2;                                                                      \
        }                                                                                                                    \
        TAIL                                                                                                                 \
    }
#define TGP_UNIT_GAP(FILL) \
    FILL;                  \
    TGP_SB();
#define TGP_UNIT_END(WAITCNT)                                                                                                \
    __builtin_amdgcn_s_waitcnt(WAITCNT);        /* this wave's share of the next unit has landed (what was issued after it may fly) */ \
    __syncthreads();                            /* ... everybody's has, and this buffer's readers are done */
#define TGP_ZERO4(ACC)                                                \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                     \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) ACC[j][e] = 0.f;

// ---- weights -> staging units (hs_chain.hip): W (N, K) fp32 row-major, leading dimension ld, into `units` units of 64 KB at out.
// Pair q of unit u is K-step (u % upg) * (32 / nb) + q / nb, output block (u / upg) * nb + q % nb: nb output blocks per K-step and unit,
// upg units per group of nb blocks (one group: upg = units).  permuted: the K order the previous layer's accumulators leave.
int tgp_pack_units(const float *W, int ld, int N, int K, int nb, int upg, int steps, int units, int permuted, uint16_t *out, hipStream_t stream);
