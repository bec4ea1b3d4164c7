// The training item's point-cloud augmentation (datasets/data_augmentation.py, datasets/load_data.py:333-350) in one launch: a
// workgroup per item.
//
// Base augmentation, PC_BasicAugment (:19-63), per point in the reference's order and fp32 rounding: box scaling (aug_bb_with_flag),
// rotation + translation (aug_rt_with_flag), box-cage resize (aug_3D_bc_with_flag, bowl and mug only) and per-point deformation
// (aug_pc_with_flag).  The 3 x 3 products are explicit 3-term sums ((a0 b0 + a1 b1) + a2 b2); the reference's CPU matmul has an
// order of its own, so the cloud agrees to a few ulp, not bit for bit.  The per-item labels (R, t, s) are computed by every thread
// of the workgroup from the same inputs (identical bits).  The box cage's new size needs the extents of the item's model points
// after the box scaling: a min / max over the workgroup (exact in any order).
//
// Second view (load_data.py:345-350), the cloud after the base augmentation held in LDS:
//   Jitter   out = pc + noise (the host's clamped normal_ draw)                                 (:66-79)
//   Dropout  rows whose float64 uniform is <= the ratio take the original row 0                 (:82-98)
//   Crop     keep the points strictly inside the first valid box                                (:101-160)
//   Cutout   drop the points strictly inside the first valid box                                (:163-207)
// Crop / cutout: the fp32 min / max of the cloud, each attempt's unit-cube bounds mapped to coordinates in float64 as NumPy promotes
// them (coord_min + coord_diff * u), strict float64 comparisons, in-box counts by ballot + popcount, the kept points compacted in
// their order by a ballot / mbcnt prefix.  Attempts 0 .. max_try - 1 can be accepted; the reference draws one more before it gives
// up (crop tests it and discards it, cutout returns before testing it), so that attempt is never accepted.  A degenerate cloud
// (coord_diff 0) has empty boxes: nothing is valid and the original comes back.
#include "tgp_common.h"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_WAVES = AG_THREADS / TGP_WAVE;
constexpr int AG_MAXN = TGP_AUGMENT_MAX_POINTS;
constexpr int AG_PER = AG_MAXN / AG_THREADS;     // points per thread in the view

struct V3 {
    float x, y, z;
};

__device__ __forceinline__ V3 mul_t(const float *M, V3 v)        // M^T v, M row-major 3 x 3
{
    return {(M[0] * v.x + M[3] * v.y) + M[6] * v.z, (M[1] * v.x + M[4] * v.y) + M[7] * v.z, (M[2] * v.x + M[5] * v.y) + M[8] * v.z};
}

__device__ __forceinline__ V3 mul(const float *M, V3 v)          // M v
{
    return {(M[0] * v.x + M[1] * v.y) + M[2] * v.z, (M[3] * v.x + M[4] * v.y) + M[5] * v.z, (M[6] * v.x + M[7] * v.y) + M[8] * v.z};
}

// the item's base augmentation state: flags and the labels before / after each stage
struct Item {
    bool bb, rt, bc, pc;
    float R0[9], t0[3];        // input pose (bb's frame)
    float nb[3];               // bb's factors (symmetric variant folded in)
    float R1[9], t1[3];        // pose after rt (bc's frame, pc's centre)
    float at[3], Ra[9];        // rt's translation and rotation
    float sy, eu, ed;          // bc: s_y of (s + mean_shape) after bb, ey_up, ey_down
    float defr;                // aug_pc_r
};

__device__ __forceinline__ V3 base_point(const Item &it, V3 p, const float *u)
{
    if (it.bb) {                                    // defor_3D_bb_in_batch
        V3 d = {p.x - it.t0[0], p.y - it.t0[1], p.z - it.t0[2]};
        V3 r = mul_t(it.R0, d);
        r = {r.x * it.nb[0], r.y * it.nb[1], r.z * it.nb[2]};
        V3 q = mul(it.R0, r);
        p = {q.x + it.t0[0], q.y + it.t0[1], q.z + it.t0[2]};
    }
    if (it.rt) {                                    // defor_3D_rt_in_batch
        V3 q = {p.x + it.at[0], p.y + it.at[1], p.z + it.at[2]};
        p = mul(it.Ra, q);
    }
    if (it.bc) {                                    // defor_3D_bc_in_batch
        V3 d = {p.x - it.t1[0], p.y - it.t1[1], p.z - it.t1[2]};
        V3 r = mul_t(it.R1, d);
        const float rs = (r.y + it.sy / 2.0f) / it.sy * (it.eu - it.ed) + it.ed;
        r.x = r.x * rs;
        r.z = r.z * rs;
        V3 q = mul(it.R1, r);
        p = {q.x + it.t1[0], q.y + it.t1[1], q.z + it.t1[2]};
    }
    if (it.pc) {                                    // defor_3D_pc: pc + (rand * r) * (pc - t)
        p = {p.x + (u[0] * it.defr) * (p.x - it.t1[0]), p.y + (u[1] * it.defr) * (p.y - it.t1[1]),
             p.z + (u[2] * it.defr) * (p.z - it.t1[2])};
    }
    return p;
}

__device__ float block_min_max(float v, bool is_max, float *red)
{
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o);
        v = is_max ? fmaxf(v, w) : fminf(v, w);
    }
    const int wave = threadIdx.x / TGP_WAVE;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < AG_WAVES; ++w) r = is_max ? fmaxf(r, red[w]) : fminf(r, red[w]);
    return r;
}

__device__ int block_sum(int v, int *red)
{
    const int wave = threadIdx.x / TGP_WAVE;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    int r = 0;
    for (int w = 0; w < AG_WAVES; ++w) r += red[w];
    return r;
}

__device__ __forceinline__ bool in_box(float x, float y, float z, const double *lo, const double *hi)
{
    return ((double)x > lo[0] && (double)x < hi[0]) && ((double)y > lo[1] && (double)y < hi[1]) && ((double)z > lo[2] && (double)z < hi[2]);
}

__global__ void __launch_bounds__(AG_THREADS) augment_kernel(tgp_augment_args a, int do_base, int do_view)
{
    __shared__ float sx[AG_MAXN], sy[AG_MAXN], sz[AG_MAXN];
    __shared__ float fred[AG_WAVES];
    __shared__ int ired[AG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, ldo = a.ld_out == 4 ? 4 : 3;
    const float *pc = a.pc + (int64_t)b * N * 3;

    Item it;
    it.bb = it.rt = it.bc = it.pc = false;
    if (do_base) {
        const float *dr = a.draws + b * 6;
        it.bb = dr[0] < a.pro_bb;
        it.rt = dr[1] < a.pro_rt;
        const float cat = a.cat_id[b];
        it.bc = dr[2] < a.pro_bc && (cat == 5.0f || cat == 1.0f);
        it.pc = dr[5] < a.pro_pc;
        const float span = (float)(1.2 - 0.8);
        it.eu = dr[3] * span + 0.8f;
        it.ed = dr[4] * span + 0.8f;
        it.defr = a.pc_r;
        float s[3], ms[3];
        #pragma unroll
        for (int j = 0; j < 3; ++j) {
            it.t0[j] = a.t[b * 3 + j];
            s[j] = a.s[b * 3 + j];
            ms[j] = a.mean_shape[b * 3 + j];
            it.at[j] = a.aug_rt_t[b * 3 + j];
        }
        #pragma unroll
        for (int j = 0; j < 9; ++j) it.R0[j] = a.R[b * 9 + j], it.Ra[j] = a.aug_rt_R[b * 9 + j];
        const float *e = a.aug_bb + b * 3;
        if (a.sym[b * 4] == 1.0f) {
            it.nb[0] = (e[0] + e[2]) / 2.0f;
            it.nb[1] = (e[1] + e[1]) / 2.0f;
            it.nb[2] = (e[2] + e[0]) / 2.0f;
        } else {
            it.nb[0] = e[0], it.nb[1] = e[1], it.nb[2] = e[2];
        }
        if (it.bb)
            #pragma unroll
            for (int j = 0; j < 3; ++j) s[j] = (s[j] + ms[j]) * it.nb[j] - ms[j];
        // rt: R1 = Ra R0, t1 = Ra (t0 + at)
        #pragma unroll
        for (int j = 0; j < 9; ++j) it.R1[j] = it.R0[j];
        #pragma unroll
        for (int j = 0; j < 3; ++j) it.t1[j] = it.t0[j];
        if (it.rt) {
            #pragma unroll
            for (int i = 0; i < 3; ++i)
                #pragma unroll
                for (int j = 0; j < 3; ++j)
                    it.R1[i * 3 + j] = (it.Ra[i * 3] * it.R0[j] + it.Ra[i * 3 + 1] * it.R0[3 + j]) + it.Ra[i * 3 + 2] * it.R0[6 + j];
            V3 tt = mul(it.Ra, V3{it.t0[0] + it.at[0], it.t0[1] + it.at[1], it.t0[2] + it.at[2]});
            it.t1[0] = tt.x, it.t1[1] = tt.y, it.t1[2] = tt.z;
        }
        it.sy = s[1] + ms[1];
        if (it.bc) {
            // the model points as bb left them, resized like the cloud; the new size is their extent times nocs_scale
            const float sy_ = it.sy;
            float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            const float *mp = a.model_point + (int64_t)b * a.n_model * 3;
            for (int i = tid; i < a.n_model; i += AG_THREADS) {
                float m[3] = {mp[i * 3], mp[i * 3 + 1], mp[i * 3 + 2]};
                if (it.bb)
                    #pragma unroll
                    for (int j = 0; j < 3; ++j) m[j] = m[j] * it.nb[j];
                const float rs = (m[1] + sy_ / 2.0f) / sy_ * (it.eu - it.ed) + it.ed;
                m[0] = m[0] * rs;
                m[2] = m[2] * rs;
                #pragma unroll
                for (int j = 0; j < 3; ++j) mn[j] = fminf(mn[j], m[j]), mx[j] = fmaxf(mx[j], m[j]);
            }
            const float ns = a.nocs_scale[b];
            #pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float hi = block_min_max(mx[j], true, fred);
                const float lo = block_min_max(mn[j], false, fred);
                s[j] = (hi - lo) * ns - ms[j];
            }
        }
        if (tid == 0) {                              // (constant indices: the arrays stay in registers)
#pragma unroll
            for (int j = 0; j < 9; ++j)
                if (a.R_out) a.R_out[b * 9 + j] = it.R1[j];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (a.t_out) a.t_out[b * 3 + j] = it.t1[j];
                if (a.s_out) a.s_out[b * 3 + j] = s[j];
            }
        }
        if (tid == 0 && a.flags_out) {
            a.flags_out[b * 4] = it.bb, a.flags_out[b * 4 + 1] = it.rt, a.flags_out[b * 4 + 2] = it.bc, a.flags_out[b * 4 + 3] = it.pc;
        }
    }

    // the points: base augmentation (or a copy), into pc_out and, for the view, into LDS
    for (int i = tid; i < N; i += AG_THREADS) {
        V3 p = {pc[i * 3], pc[i * 3 + 1], pc[i * 3 + 2]};
        if (do_base) {
            const float *u = a.defor + ((int64_t)b * N + i) * 3;
            float uu[3] = {0.f, 0.f, 0.f};
            if (it.pc) uu[0] = u[0], uu[1] = u[1], uu[2] = u[2];
            p = base_point(it, p, uu);
            if (a.pc_out) {
                float *o = a.pc_out + ((int64_t)b * N + i) * ldo;
                o[0] = p.x, o[1] = p.y, o[2] = p.z;
                if (ldo == 4) o[3] = 0.f;
            }
        }
        if (do_view) sx[i] = p.x, sy[i] = p.y, sz[i] = p.z;
    }
    if (!do_view) return;
    __syncthreads();

    const int op = a.op[b];
    float *out = a.view_out + (int64_t)b * N * ldo;
    auto put = [&](int d, float x, float y, float z) {
        float *o = out + (int64_t)d * ldo;
        o[0] = x, o[1] = y, o[2] = z;
        if (ldo == 4) o[3] = 0.f;
    };
    int M = N, att = -1;
    if (op == TGP_AUG_JITTER) {
        const float *nz = a.noise + (int64_t)b * N * 3;
        for (int i = tid; i < N; i += AG_THREADS) {
            put(i, sx[i] + nz[i * 3], sy[i] + nz[i * 3 + 1], sz[i] + nz[i * 3 + 2]);
        }
    } else if (op == TGP_AUG_DROPOUT) {
        const double ratio = a.drop_ratio[b];
        const double *du = a.drop_u + (int64_t)b * N;
        for (int i = tid; i < N; i += AG_THREADS) {
            const int k = du[i] <= ratio ? 0 : i;
            put(i, sx[k], sy[k], sz[k]);
        }
    } else if (op == TGP_AUG_CROP || op == TGP_AUG_CUTOUT) {
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = tid; i < N; i += AG_THREADS) {
            mn[0] = fminf(mn[0], sx[i]), mn[1] = fminf(mn[1], sy[i]), mn[2] = fminf(mn[2], sz[i]);
            mx[0] = fmaxf(mx[0], sx[i]), mx[1] = fmaxf(mx[1], sy[i]), mx[2] = fmaxf(mx[2], sz[i]);
        }
        double cmin[3], cdiff[3];
        #pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float hi = block_min_max(mx[j], true, fred);
            const float lo = block_min_max(mn[j], false, fred);
            cmin[j] = (double)lo;
            cdiff[j] = (double)(hi - lo);           // fp32 difference, promoted
        }
        const bool crop = op == TGP_AUG_CROP;
        const int min_pts = crop ? a.crop_min_points : a.cutout_min_points;
        const int max_try = crop ? a.crop_max_try : a.cutout_max_try;
        const int lane = tid & 63;
        double lo[3], hi[3];
        for (int t = 0; t < max_try && att < 0; ++t) {
            const double *u = a.boxes + ((int64_t)b * TGP_AUGMENT_MAX_TRY + t) * 6;
            #pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double pl = cdiff[j] * u[j], ph = cdiff[j] * u[3 + j];   // products round before the sums (no FMA)
                lo[j] = cmin[j] + pl;
                hi[j] = cmin[j] + ph;
            }
            int cnt = 0;
#pragma unroll
            for (int c = 0; c < AG_PER; ++c) {
                const int i = c * AG_THREADS + tid;
                const bool inb = i < N && in_box(sx[i], sy[i], sz[i], lo, hi);
                const uint64_t m = __ballot(inb);
                if (lane == 0) cnt += __popcll(m);
            }
            const int k = block_sum(cnt, ired);       // points inside the box
            const bool ok = crop ? (k >= min_pts && k < N) : (N - k >= min_pts && k > 0);
            if (ok) att = t, M = crop ? k : N - k;
        }
        if (att < 0) {
            for (int i = tid; i < N; i += AG_THREADS) put(i, sx[i], sy[i], sz[i]);
        } else {
            // order-preserving compaction: chunk by chunk, the kept points of a wave are placed by mbcnt, the waves by their counts
            int base = 0;
            const int wave = tid / TGP_WAVE;
#pragma unroll
            for (int c = 0; c < AG_PER; ++c) {
                const int i = c * AG_THREADS + tid;
                const bool keep = i < N && (in_box(sx[i], sy[i], sz[i], lo, hi) == crop);
                const uint64_t m = __ballot(keep);
                const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                __syncthreads();
                if (lane == 0) ired[wave] = __popcll(m);
                __syncthreads();
                int off = base;
                for (int w = 0; w < wave; ++w) off += ired[w];
                if (keep) {
                    put(off + below, sx[i], sy[i], sz[i]);
                }
                for (int w = 0; w < AG_WAVES; ++w) base += ired[w];
            }
            for (int i = M + tid; i < N; i += AG_THREADS) put(i, 0.f, 0.f, 0.f);
        }
    } else {                                         // TGP_AUG_NONE: the operator's p skipped it
        for (int i = tid; i < N; i += AG_THREADS) put(i, sx[i], sy[i], sz[i]);
    }
    if (tid == 0) a.count_out[b * 2] = M, a.count_out[b * 2 + 1] = att;
}

}  // namespace

extern "C" int tgp_augment_max_points(void) { return TGP_AUGMENT_MAX_POINTS; }

extern "C" int tgp_augment(const tgp_augment_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->B >= 1 && a->N >= 1 && a->pc && (a->ld_out == 0 || a->ld_out == 3 || a->ld_out == 4));
    const bool base = a->draws != nullptr, view = a->op != nullptr;
    TGP_REQUIRE(base || view);
    if (base) {
        TGP_REQUIRE(a->R && a->t && a->s && a->mean_shape && a->sym && a->aug_bb && a->aug_rt_t && a->aug_rt_R && a->cat_id &&
                    a->nocs_scale && a->model_point && a->n_model >= 1 && a->defor);
        TGP_REQUIRE(view || a->pc_out);
    }
    if (view) {
        TGP_REQUIRE(a->N <= TGP_AUGMENT_MAX_POINTS && a->noise && a->drop_ratio && a->drop_u && a->boxes && a->view_out && a->count_out);
        TGP_REQUIRE(a->crop_max_try >= 0 && a->crop_max_try < TGP_AUGMENT_MAX_TRY && a->cutout_max_try >= 0 &&
                    a->cutout_max_try < TGP_AUGMENT_MAX_TRY && a->crop_min_points >= 0 && a->cutout_min_points >= 0);
        // the view reads the cloud from LDS: its output may not alias the input it is still reading on another workgroup
        TGP_REQUIRE(a->view_out != a->pc);
    }
    hipLaunchKernelGGL(augment_kernel, dim3(a->B), dim3(AG_THREADS), 0, tgp_hs(stream), *a, base ? 1 : 0, view ? 1 : 0);
    return TGP_LAUNCH_RESULT();
}
