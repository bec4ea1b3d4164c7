// BOP pose errors, the point-based ones: ADD, ADD-S (ADI), MSSD and MSPD of J (estimate, ground truth) pairs per call
// (include/tgpose.h, DESIGN.md section 3 "BOP pose errors"; tests/bop_ref.py restates the contract in NumPy).  float32 inputs
// widened to float64, every operation float64 and rounded on its own (the library is built with -ffp-contract=off), as icp.hip.
//
//   poseerr_kernel          grid (J, TGP_POSEERR_SPLIT), 256 threads.  Workgroup (j, b):
//                           - points [b c, (b+1) c), c = ceil(P / SPLIT), one per thread and round: |E p - G p| for add, and for adi
//                             the nearest of ALL ground-truth points G p_k, which pass through LDS in tiles of TGP_POSEERR_TILE
//                             (each tile is posed by the workgroup as it is filled: no P x P matrix, no per-job buffer);
//                           - symmetries 4 b + w, + 4 SPLIT, ... on wave w: the lanes stride over the points, the maxima are joined
//                             by shuffles (max is exact in any order), the wave keeps its least (value, index).
//                           Its partial results -- two sums, two (value, index) pairs, one flag word -- go to slot (j, b) of the workspace.
//   poseerr_finish_kernel   one thread per job: the slots in index order -> err, sym_best, status.
//
// No atomics at all.  Sums: thread t adds its points in index order, the threads are joined by a tree in LDS, the workgroups by the
// finishing thread in index order: two calls give identical bytes, and a job's result depends on neither the other jobs nor J.
#include "tgp_common.h"

#define POSEERR_THREADS 256
#define POSEERR_WAVES (POSEERR_THREADS / TGP_WAVE)
#define POSEERR_SPLIT TGP_POSEERR_SPLIT
#define POSEERR_TILE TGP_POSEERR_TILE

struct PoseErrSlot {
    double add, adi, mssd, mspd;
    int mssd_i, mspd_i, behind, pad;
};
static_assert(sizeof(PoseErrSlot) == 48, "PoseErrSlot");

struct PoseErrJob {
    int vbase, nv, sbase, nq;
};

// the mesh and the symmetry group of a job, checked against the host's bounds before anything is addressed with them
__device__ __forceinline__ bool poseerr_job(const tgp_poseerr_args &a, int j, PoseErrJob &m)
{
    const int mesh = a.job_mesh[j], grp = a.job_sym[j];
    if (mesh < 0 || mesh >= a.M || grp < 0 || grp >= a.G) return false;
    m.vbase = a.vptr[mesh];
    m.sbase = a.sptr[grp];
    const long long nv = (long long)a.vptr[mesh + 1] - m.vbase, nq = (long long)a.sptr[grp + 1] - m.sbase;
    if (m.vbase < 0 || m.sbase < 0 || nv < 1 || nq < 1 || m.vbase + nv > a.n_verts || m.sbase + nq > a.n_syms || nq > a.max_syms) return false;
    m.nv = (int)nv;
    m.nq = (int)nq;
    return true;
}

struct D3 {
    double x, y, z;
};

// rows of a (3,4) float32 transform widened: ((T0 x + T1 y) + T2 z) + T3
__device__ __forceinline__ D3 poseerr_apply(const double *T, const D3 p)
{
    D3 r;
    r.x = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
    r.y = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
    r.z = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
    return r;
}

__device__ __forceinline__ double poseerr_dist2(const D3 a, const D3 b)
{
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ D3 poseerr_vertex(const float *v)
{
    D3 p;
    p.x = (double)v[0], p.y = (double)v[1], p.z = (double)v[2];
    return p;
}

// the larger of two squared distances; one that is not a number stays (fmax would drop it)
__device__ __forceinline__ double poseerr_max(double m, double v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ double poseerr_wave_max(double v)
{
#pragma unroll
    for (int o = TGP_WAVE / 2; o > 0; o >>= 1) v = poseerr_max(v, __shfl_xor(v, o, TGP_WAVE));
    return v;
}

__global__ __launch_bounds__(POSEERR_THREADS) void poseerr_kernel(const tgp_poseerr_args a)
{
    __shared__ double s_g[POSEERR_TILE * 3]; // a tile of posed ground-truth points; the sums' tree afterwards
    __shared__ double s_best[POSEERR_WAVES][2];
    __shared__ int s_besti[POSEERR_WAVES][3];

    const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;
    PoseErrJob m;
    if (!poseerr_job(a, j, m)) return; // the same for every lane; the finishing thread does not read this job's slots

    double E[12], G[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        E[k] = (double)a.pose_est[(size_t)j * 12 + k];
        G[k] = (double)a.pose_gt[(size_t)j * 12 + k];
    }
    const float *verts = a.verts + (size_t)m.vbase * 3;
    const double near = (double)a.near;

    // ---- add and adi over this workgroup's slice of the points
    const int chunk = (m.nv + POSEERR_SPLIT - 1) / POSEERR_SPLIT;
    const long long lo = (long long)b * chunk;
    const int p0 = (int)min(lo, (long long)m.nv), p1 = (int)min(lo + chunk, (long long)m.nv);
    double sum_add = 0.0, sum_adi = 0.0;
    for (int base = p0; base < p1; base += POSEERR_THREADS) { // the same trip count for every lane: the barriers below are met
        const int i = base + tid;
        const bool live = i < p1;
        D3 e = {0.0, 0.0, 0.0};
        if (live) {
            const D3 p = poseerr_vertex(verts + (size_t)i * 3);
            e = poseerr_apply(E, p);
            sum_add += sqrt(poseerr_dist2(e, poseerr_apply(G, p)));
        }
        double best = __builtin_inf();
        for (int t0 = 0; t0 < m.nv; t0 += POSEERR_TILE) {
            const int n = min(POSEERR_TILE, m.nv - t0);
            __syncthreads(); // the scan of the tile before this one is over
            for (int k = tid; k < n; k += POSEERR_THREADS) {
                const D3 g = poseerr_apply(G, poseerr_vertex(verts + (size_t)(t0 + k) * 3));
                s_g[k * 3 + 0] = g.x, s_g[k * 3 + 1] = g.y, s_g[k * 3 + 2] = g.z;
            }
            __syncthreads();
            if (live)
                for (int k = 0; k < n; ++k) { // every lane reads the same address: a broadcast
                    const D3 g = {s_g[k * 3 + 0], s_g[k * 3 + 1], s_g[k * 3 + 2]};
                    best = fmin(best, poseerr_dist2(e, g));
                }
        }
        if (live) sum_adi += sqrt(best);
    }

    // ---- mssd and mspd over this workgroup's symmetries, one per wave at a time
    const int lane = tid % TGP_WAVE, wave = tid / TGP_WAVE;
    const double fx = (double)a.camk[(size_t)j * 4 + 0], fy = (double)a.camk[(size_t)j * 4 + 1];
    const double cx = (double)a.camk[(size_t)j * 4 + 2], cy = (double)a.camk[(size_t)j * 4 + 3];
    double best_s = __builtin_inf(), best_p = __builtin_inf();
    int best_si = 0x7fffffff, best_pi = 0x7fffffff, behind = 0; // behind: bit 0 a point not in front of near, bit 1 a distance not finite
    for (int q = b * POSEERR_WAVES + wave; q < m.nq; q += POSEERR_SPLIT * POSEERR_WAVES) {
        double S[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) S[k] = (double)a.sym[(size_t)(m.sbase + q) * 12 + k];
        double ms = 0.0, mp = 0.0;
        for (int i = lane; i < m.nv; i += TGP_WAVE) {
            const D3 p = poseerr_vertex(verts + (size_t)i * 3);
            const D3 e = poseerr_apply(E, p), g = poseerr_apply(G, poseerr_apply(S, p));
            ms = poseerr_max(ms, poseerr_dist2(e, g));
            if (e.z > near && g.z > near) { // false for a NaN too
                const double du = (fx * (e.x / e.z) + cx) - (fx * (g.x / g.z) + cx);
                const double dv = (fy * (e.y / e.z) + cy) - (fy * (g.y / g.z) + cy);
                mp = poseerr_max(mp, du * du + dv * dv);
            } else {
                behind |= 1;
            }
        }
        ms = sqrt(poseerr_wave_max(ms));
        mp = sqrt(poseerr_wave_max(mp));
        if (!(ms < __builtin_inf())) behind |= 2; // a pose, a transform or a vertex that is not finite: status 4
        if (ms < best_s) best_s = ms, best_si = q; // q ascends: the first of equal values stays
        if (mp < best_p) best_p = mp, best_pi = q;
    }
    behind = (__any(behind & 1) ? 1 : 0) | (__any(behind & 2) ? 2 : 0);

    // ---- join the workgroup: the sums by a tree in fixed order, the waves' (value, index) pairs by the lowest index among equals
    __syncthreads(); // the last tile has been read
    s_g[tid] = sum_add;
    s_g[POSEERR_THREADS + tid] = sum_adi;
    if (lane == 0) {
        s_best[wave][0] = best_s, s_best[wave][1] = best_p;
        s_besti[wave][0] = best_si, s_besti[wave][1] = best_pi, s_besti[wave][2] = behind;
    }
    __syncthreads();
    for (int o = POSEERR_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            s_g[tid] += s_g[tid + o];
            s_g[POSEERR_THREADS + tid] += s_g[POSEERR_THREADS + tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        PoseErrSlot r;
        r.add = s_g[0], r.adi = s_g[POSEERR_THREADS];
        r.mssd = r.mspd = __builtin_inf();
        r.mssd_i = r.mspd_i = 0x7fffffff;
        r.behind = r.pad = 0;
        for (int w = 0; w < POSEERR_WAVES; ++w) {
            if (s_best[w][0] < r.mssd || (s_best[w][0] == r.mssd && s_besti[w][0] < r.mssd_i)) r.mssd = s_best[w][0], r.mssd_i = s_besti[w][0];
            if (s_best[w][1] < r.mspd || (s_best[w][1] == r.mspd && s_besti[w][1] < r.mspd_i)) r.mspd = s_best[w][1], r.mspd_i = s_besti[w][1];
            r.behind |= s_besti[w][2];
        }
        ((PoseErrSlot *)a.workspace)[(size_t)j * POSEERR_SPLIT + b] = r;
    }
}

__global__ __launch_bounds__(256) void poseerr_finish_kernel(const tgp_poseerr_args a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.J) return;
    double *err = a.err + (size_t)j * TGP_POSEERR_COLS;
    int32_t *sb = a.sym_best + (size_t)j * 2;
    PoseErrJob m;
    if (!poseerr_job(a, j, m)) {
        err[0] = err[1] = err[2] = err[3] = __builtin_nan("");
        sb[0] = sb[1] = -1;
        a.status[j] = 1;
        return;
    }
    const PoseErrSlot *slot = (const PoseErrSlot *)a.workspace + (size_t)j * POSEERR_SPLIT;
    PoseErrSlot r = slot[0];
#pragma unroll 2
    for (int b = 1; b < POSEERR_SPLIT; ++b) {
        const PoseErrSlot s = slot[b];
        r.add += s.add;
        r.adi += s.adi;
        if (s.mssd < r.mssd || (s.mssd == r.mssd && s.mssd_i < r.mssd_i)) r.mssd = s.mssd, r.mssd_i = s.mssd_i;
        if (s.mspd < r.mspd || (s.mspd == r.mspd && s.mspd_i < r.mspd_i)) r.mspd = s.mspd, r.mspd_i = s.mspd_i;
        r.behind |= s.behind;
    }
    err[0] = r.add / (double)m.nv;
    err[1] = r.adi / (double)m.nv;
    err[2] = r.mssd;
    bool finite = !(r.behind & 2) && err[0] < __builtin_inf() && err[1] < __builtin_inf();
#pragma unroll
    for (int k = 0; k < 4; ++k) finite = finite && fabsf(a.camk[(size_t)j * 4 + k]) < __builtin_inff();
    if (!finite) { // a pose, a transform, a vertex or an intrinsic that is not finite
        err[0] = err[1] = err[2] = err[3] = __builtin_nan("");
        sb[0] = sb[1] = -1;
        a.status[j] = 4;
        return;
    }
    sb[0] = r.mssd_i;
    if (r.behind) {
        err[3] = __builtin_inf();
        sb[1] = -1;
    } else {
        err[3] = r.mspd;
        sb[1] = r.mspd_i;
    }
    a.status[j] = r.behind ? 2 : 0;
}

extern "C" int64_t tgp_pose_errors_workspace_bytes(int J)
{
    if (J < 0) return TGP_EINVAL;
    if (J > TGP_POSEERR_MAX_JOBS) return TGP_EUNSUPPORTED;
    return (int64_t)J * POSEERR_SPLIT * (int64_t)sizeof(PoseErrSlot) + 16;
}

extern "C" int tgp_pose_errors(const tgp_poseerr_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_poseerr_args &a = *args;
    TGP_REQUIRE(a.verts && a.vptr && a.sym && a.sptr);
    TGP_REQUIRE(a.M > 0 && a.n_verts > 0 && a.G > 0 && a.n_syms > 0 && a.max_syms > 0 && a.J >= 0);
    TGP_REQUIRE(a.near > 0.f && a.near < __builtin_inff());
    if (a.J > 0) TGP_REQUIRE(a.job_mesh && a.job_sym && a.pose_est && a.pose_gt && a.camk && a.err && a.sym_best && a.status && a.workspace);
    if (a.J > TGP_POSEERR_MAX_JOBS || a.max_syms > TGP_POSEERR_MAX_SYMS) return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    TGP_REQUIRE(a.workspace_bytes >= tgp_pose_errors_workspace_bytes(a.J));
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(poseerr_kernel, dim3((unsigned)a.J, POSEERR_SPLIT), dim3(POSEERR_THREADS), 0, st, a);
    hipLaunchKernelGGL(poseerr_finish_kernel, dim3(tgp_cdiv(a.J, 256)), dim3(256), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
