// ICP pose refinement against point-and-normal models on gfx950: J jobs in ONE launch, one workgroup per job, every iteration of a
// job inside the kernel (DESIGN.md section 3 "ICP refinement and model-based tracking" and include/tgpose.h are the contract;
// tests/icp_ref.py restates it in NumPy).
//
// A job's model is staged once into LDS as float4 (x, y, z, |y|^2), the normals beside it in point-to-plane mode.  Each lane keeps
// its PPL source points in registers, so one broadcast LDS read of a model point serves all of them.  Per iteration: the source
// points go to the model frame (float64, rounded once to float32), the nearest model point is found with tgp_nn1's float32
// arithmetic, the sums over the inliers are float64 -- per lane in point order, across the wave by a shuffle tree, across the waves
// serially in LDS: a fixed order that depends on nothing but the job -- and lane 0 solves the 3x3 (Horn's quaternion, Jacobi
// eigenvectors of the 4x4 matrix) or 6x6 (Cholesky) problem in float64.  No atomics, nothing allocated, nothing read back.
#include "icp_solve.h"

namespace {

constexpr int ICP_MAX = TGP_ICP_MAX_POINTS;

template <int MODE, int PPL>
__global__ void __launch_bounds__(ICP_THREADS) icp_kernel(tgp_icp_args a)
{
    __shared__ float4 s_model[ICP_MAX];
    __shared__ float s_normal[MODE == 1 ? ICP_MAX * 3 : 1];
    __shared__ IcpShared sh;
    const int job = blockIdx.x, tid = threadIdx.x;

    const int jm = a.job_model[job];
    const int n = a.src_count ? a.src_count[job] : a.n_cap;
    int m = 0;
    bool good = jm >= 0 && jm < a.M && n >= 0 && n <= a.n_cap;
    if (good) {
        m = a.model_count ? a.model_count[jm] : a.m_cap;
        good = m >= 1 && m <= a.m_cap;
    }
    const float *Rin = a.R + (size_t)job * 9, *tin = a.t + (size_t)job * 3;
    if (!good) {                                                 // the same in every thread: nothing else is read
        if (tid < 9) a.R_out[(size_t)job * 9 + tid] = Rin[tid];
        if (tid < 3) a.t_out[(size_t)job * 3 + tid] = tin[tid];
        if (tid < 4) a.info[(size_t)job * 4 + tid] = tid == 0 ? 3 : 0;
        if (tid == 0) a.s_out[job] = a.s[job], a.rmse[job] = __builtin_nanf("");
        if (a.corr)
            for (int i = tid; i < a.n_cap; i += ICP_THREADS) a.corr[(size_t)job * a.n_cap + i] = -1;
        return;
    }

    const float *mp = a.models + (size_t)jm * a.m_cap * 6;
    for (int j = tid; j < m; j += ICP_THREADS) {
        const float *p = mp + (size_t)j * 6;
        const float x = p[0], y = p[1], z = p[2];
        float q = x * x;
        q = q + y * y;
        q = q + z * z;
        s_model[j] = make_float4(x, y, z, q);
        if (MODE == 1) s_normal[j * 3] = p[3], s_normal[j * 3 + 1] = p[4], s_normal[j * 3 + 2] = p[5];
    }
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) sh.R[k] = (double)Rin[k];
        for (int k = 0; k < 3; ++k) sh.t[k] = (double)tin[k];
        sh.s = (double)a.s[job];
        sh.stop = 0, sh.status = 0, sh.iters_done = 0;
    }
    float px[PPL], py[PPL], pz[PPL];
    bool live[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        const int i = tid + k * ICP_THREADS;
        live[k] = i < n;
        px[k] = py[k] = pz[k] = 0.f;
        if (live[k]) {
            const float *p = a.src + ((size_t)job * a.n_cap + i) * 3;
            px[k] = p[0], py[k] = p[1], pz[k] = p[2];
        }
    }
    const double gate = (double)a.max_dist[job];
    const int min_inliers = max(a.min_inliers, 6);
    const bool never_stop = !(a.tol_rot > 0.f) && !(a.tol_trans > 0.f);
    __syncthreads();

    // pass `iters` is the correspondence pass at the final pose
    for (int it = 0;; ++it) {
        const bool last = it >= a.iters || sh.stop;
        const double s = sh.s;
        const double R0 = sh.R[0], R1 = sh.R[1], R2 = sh.R[2], R3 = sh.R[3], R4 = sh.R[4], R5 = sh.R[5], R6 = sh.R[6], R7 = sh.R[7], R8 = sh.R[8];
        const double t0 = sh.t[0], t1 = sh.t[1], t2 = sh.t[2];
        const double g = gate / s;
        const float thr = (float)(g * g);
        float qx[PPL], qy[PPL], qz[PPL], qq[PPL], best[PPL];
        int bi[PPL];
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
            const double d0 = (double)px[k] - t0, d1 = (double)py[k] - t1, d2 = (double)pz[k] - t2;
            qx[k] = (float)(((R0 * d0 + R3 * d1) + R6 * d2) / s);
            qy[k] = (float)(((R1 * d0 + R4 * d1) + R7 * d2) / s);
            qz[k] = (float)(((R2 * d0 + R5 * d1) + R8 * d2) / s);
            float q = qx[k] * qx[k];
            q = q + qy[k] * qy[k];
            q = q + qz[k] * qz[k];
            qq[k] = q;
            bi[k] = 0;
        }
        {
            const float4 y = s_model[0];
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                float inner = qx[k] * y.x;
                inner = fmaf(qy[k], y.y, inner);
                inner = fmaf(qz[k], y.z, inner);
                const float sum = y.w + qq[k];
                best[k] = sum - 2.0f * inner;
            }
        }
        for (int j = 1; j < m; ++j) {
            const float4 y = s_model[j];
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                float inner = qx[k] * y.x;
                inner = fmaf(qy[k], y.y, inner);
                inner = fmaf(qz[k], y.z, inner);
                const float sum = y.w + qq[k];
                const float dv = sum - 2.0f * inner;
                if (dv < best[k]) best[k] = dv, bi[k] = j;
            }
        }
        bool in[PPL];
        const float inf = __builtin_inff();
#pragma unroll
        for (int k = 0; k < PPL; ++k)
            in[k] = live[k] && best[k] <= thr && fabsf(px[k]) < inf && fabsf(py[k]) < inf && fabsf(pz[k]) < inf;

        if (last) {
            double v[2] = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                if (in[k]) {
                    const float4 y = s_model[bi[k]];
                    const double dx = (double)qx[k] - (double)y.x, dy = (double)qy[k] - (double)y.y, dz = (double)qz[k] - (double)y.z;
                    v[0] = v[0] + 1.0;
                    v[1] = v[1] + ((dx * dx + dy * dy) + dz * dz);
                }
                const int i = tid + k * ICP_THREADS;
                if (a.corr && i < a.n_cap) a.corr[(size_t)job * a.n_cap + i] = in[k] ? bi[k] : -1;
            }
            block_sum<2>(v, sh);
            if (tid == 0) {
                const double cnt = sh.sum[0];
                a.info[(size_t)job * 4] = sh.status;
                a.info[(size_t)job * 4 + 1] = (int)cnt;
                a.info[(size_t)job * 4 + 2] = sh.iters_done;
                a.info[(size_t)job * 4 + 3] = 0;
                a.rmse[job] = cnt > 0.0 ? (float)(s * sqrt(sh.sum[1] / cnt)) : __builtin_nanf("");
                a.s_out[job] = (float)s;
            }
            if (tid < 9) a.R_out[(size_t)job * 9 + tid] = (float)sh.R[tid];
            if (tid < 3) a.t_out[(size_t)job * 3 + tid] = (float)sh.t[tid];
            return;
        }

        if (MODE == 0) {
            double v[10];
#pragma unroll
            for (int c = 0; c < 7; ++c) v[c] = 0.0;
#pragma unroll
            for (int k = 0; k < PPL; ++k)
                if (in[k]) {
                    const float4 y = s_model[bi[k]];
                    v[0] = v[0] + 1.0;
                    v[1] = v[1] + (double)px[k], v[2] = v[2] + (double)py[k], v[3] = v[3] + (double)pz[k];
                    v[4] = v[4] + (double)y.x, v[5] = v[5] + (double)y.y, v[6] = v[6] + (double)y.z;
                }
            block_sum<7>(v, sh);
            const double cnt = sh.sum[0];
            double pbar[3], ybar[3];
            if (cnt >= (double)min_inliers) {                    // the same in every thread
#pragma unroll
                for (int c = 0; c < 3; ++c) pbar[c] = sh.sum[1 + c] / cnt, ybar[c] = sh.sum[4 + c] / cnt;
                __syncthreads();                                 // sh.sum is rewritten below
#pragma unroll
                for (int c = 0; c < 10; ++c) v[c] = 0.0;
#pragma unroll
                for (int k = 0; k < PPL; ++k)
                    if (in[k]) {
                        const float4 y = s_model[bi[k]];
                        const double yc[3] = {(double)y.x - ybar[0], (double)y.y - ybar[1], (double)y.z - ybar[2]};
                        const double pc[3] = {(double)px[k] - pbar[0], (double)py[k] - pbar[1], (double)pz[k] - pbar[2]};
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int c = 0; c < 3; ++c) v[r * 3 + c] = v[r * 3 + c] + yc[r] * pc[c];
                        v[9] = v[9] + ((yc[0] * yc[0] + yc[1] * yc[1]) + yc[2] * yc[2]);
                    }
                block_sum<10>(v, sh);
            }
            if (tid == 0) {
                if (cnt < (double)min_inliers) sh.status = 1, sh.stop = 1;
                else {
                    double ang = 0.0, tr = 0.0;
                    const int st = solve_point(sh.sum, sh.sum[9], pbar, ybar, a.with_scale, sh, ang, tr);
                    if (st) sh.status = st, sh.stop = 1;
                    else {
                        sh.iters_done = it + 1;
                        if (!never_stop && ang <= (double)a.tol_rot && tr <= (double)a.tol_trans) sh.stop = 1;
                    }
                }
            }
        } else {
            double v[ICP_NV];
#pragma unroll
            for (int c = 0; c < ICP_NV; ++c) v[c] = 0.0;
#pragma unroll
            for (int k = 0; k < PPL; ++k)
                if (in[k]) {
                    const float4 y = s_model[bi[k]];
                    const double nx = (double)s_normal[bi[k] * 3], ny = (double)s_normal[bi[k] * 3 + 1], nz = (double)s_normal[bi[k] * 3 + 2];
                    const double x = (double)qx[k], yy = (double)qy[k], z = (double)qz[k];
                    const double row[6] = {yy * nz - z * ny, z * nx - x * nz, x * ny - yy * nx, nx, ny, nz};
                    const double r = (nx * (x - (double)y.x) + ny * (yy - (double)y.y)) + nz * (z - (double)y.z);
                    int e = 0;
#pragma unroll
                    for (int i = 0; i < 6; ++i)
#pragma unroll
                        for (int j = i; j < 6; ++j, ++e) v[e] = v[e] + row[i] * row[j];
#pragma unroll
                    for (int i = 0; i < 6; ++i) v[21 + i] = v[21 + i] + row[i] * r;
                    v[27] = v[27] + 1.0;
                }
            block_sum<ICP_NV>(v, sh);
            if (tid == 0) {
                if (sh.sum[27] < (double)min_inliers) sh.status = 1, sh.stop = 1;
                else {
                    double ang = 0.0, tr = 0.0;
                    const int st = solve_plane(sh.sum, sh, ang, tr);
                    if (st) sh.status = st, sh.stop = 1;
                    else {
                        sh.iters_done = it + 1;
                        if (!never_stop && ang <= (double)a.tol_rot && tr <= (double)a.tol_trans) sh.stop = 1;
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <int MODE>
int icp_launch(const tgp_icp_args &a, hipStream_t st)
{
    const dim3 grid(a.J), block(ICP_THREADS);
    if (a.n_cap <= ICP_THREADS) hipLaunchKernelGGL((icp_kernel<MODE, 1>), grid, block, 0, st, a);
    else if (a.n_cap <= 2 * ICP_THREADS) hipLaunchKernelGGL((icp_kernel<MODE, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((icp_kernel<MODE, 4>), grid, block, 0, st, a);
    return TGP_LAUNCH_RESULT();
}

}  // namespace

extern "C" int tgp_icp_max_points(void) { return ICP_MAX; }

extern "C" int tgp_icp_refine(const tgp_icp_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->models && a->job_model && a->src && a->R && a->t && a->s && a->max_dist);
    TGP_REQUIRE(a->R_out && a->t_out && a->s_out && a->info && a->rmse);
    TGP_REQUIRE(a->M >= 1 && a->m_cap >= 1 && a->J >= 1 && a->n_cap >= 1 && a->iters >= 1);
    TGP_REQUIRE((a->mode == 0 || a->mode == 1) && !(a->mode == 1 && a->with_scale));
    if (a->m_cap > ICP_MAX || a->n_cap > ICP_MAX || a->J > 65535) return TGP_EUNSUPPORTED;
    static_assert(ICP_MAX == 4 * ICP_THREADS, "the widest kernel holds four points per lane");
    return a->mode == 0 ? icp_launch<0>(*a, tgp_hs(stream)) : icp_launch<1>(*a, tgp_hs(stream));
}
