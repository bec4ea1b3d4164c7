// Dense projective ICP of depth frames against ray-cast vertex / normal maps on gfx950: J jobs in ONE launch, one workgroup per job,
// every iteration of a job inside the kernel (DESIGN.md section 3 "Dense projective registration" and include/tgpose.h are the
// contract; tests/icp_dense_ref.py restates it in NumPy).
//
// The map is indexed by pixel: a source pixel goes to the model frame (float64, rounded once, icp.hip's sequence), through the
// reference pose the maps were cast from and the job's intrinsics into the map's window, and reads ONE cell -- no search, no crop,
// no sampler, no cap on the number of source pixels.  A lane walks the job's pixels e = tid, tid + 512, ... and recomputes its point
// from the depth word each iteration: the frame sits in L2 and a pixel's state would cost registers for nothing.  The job's window,
// reference pose and intrinsics are indexed by blockIdx alone (scalar loads); neighbouring pixels project to neighbouring cells, so
// the map reads of a wave are coherent and go through the cache.  The sums, the reduction and the 6x6 solve are icp.hip's mode 1
// (icp_solve.h).  No atomics, nothing allocated, nothing read back.
#include "icp_solve.h"
#include "pixel_point.h"

namespace {

// The job's source pixels: the grid (x0 + i stride, y0 + k stride) cut to the frame.
struct DenseGrid {
    int xs, ys, nx, ny;               // the first column / row inside the frame and how many follow at the stride
};

__device__ __forceinline__ void dense_axis(int lo, int hi, int stride, int size, int &first, int &count)
{
    const long long l = lo, st = stride;
    const long long skip = l < 0 ? (-l + st - 1) / st : 0;       // steps until the grid is at or right of 0
    const long long f = l + skip * st;
    const long long last = hi < size - 1 ? hi : size - 1;
    first = 0, count = 0;
    if (f <= last) first = (int)f, count = (int)((last - f) / st) + 1;
}

struct DenseCell {
    bool assoc, inlier;
    int cell;
    float qx, qy, qz, yx, yy, yz, nx, ny, nz;
};

struct DenseJob {
    const uint16_t *frame;
    const uint8_t *mframe;
    int mval, W, stride;
    DenseGrid g;
    float cx, cy;
    float K0, K1, K2, K3;
    float T[12];
    float u0, v0, du, dv;
    float wlast, hlast;
    int w;
    const float *z, *vertex, *normal;
};

struct DensePose {
    double R0, R1, R2, R3, R4, R5, R6, R7, R8, t0, t1, t2, s;
    float thr;
};

// one source pixel at the current pose
__device__ __forceinline__ void dense_pixel(const DenseJob &jb, const UniformDiv &div_fx, const UniformDiv &div_fy, const UniformDiv &div_k,
                                            const DensePose &ps, int e, DenseCell &c)
{
    c.assoc = c.inlier = false;
    c.cell = -1;
    const int k = e / jb.g.nx, i = e - k * jb.g.nx;
    const int x = jb.g.xs + i * jb.stride, y = jb.g.ys + k * jb.stride;          // inside the frame by dense_axis
    const size_t o = (size_t)y * jb.W + x;
    const int d = jb.frame[o];
    if (d == 0) return;
    if (jb.mframe && jb.mframe[o] != jb.mval) return;
    float px, py, pz;
    tgp_pixel_point(x, y, (float)d, jb.cx, jb.cy, div_fx, div_fy, div_k, px, py, pz);
    const double d0 = (double)px - ps.t0, d1 = (double)py - ps.t1, d2 = (double)pz - ps.t2;
    const float qx = (float)(((ps.R0 * d0 + ps.R3 * d1) + ps.R6 * d2) / ps.s);
    const float qy = (float)(((ps.R1 * d0 + ps.R4 * d1) + ps.R7 * d2) / ps.s);
    const float qz = (float)(((ps.R2 * d0 + ps.R5 * d1) + ps.R8 * d2) / ps.s);
    const float *T = jb.T;
    const float cx = ((T[0] * qx + T[1] * qy) + T[2] * qz) + T[3];
    const float cy = ((T[4] * qx + T[5] * qy) + T[6] * qz) + T[7];
    const float cz = ((T[8] * qx + T[9] * qy) + T[10] * qz) + T[11];
    if (!(cz > 1e-6f)) return;                                                  // a NaN too
    const float u = jb.K0 * (cx / cz) + jb.K2, v = jb.K1 * (cy / cz) + jb.K3;
    const float col = rintf((u - jb.u0) / jb.du), row = rintf((v - jb.v0) / jb.dv);
    if (!(col >= 0.f && col <= jb.wlast && row >= 0.f && row <= jb.hlast)) return; // a NaN too
    const int cell = (int)row * jb.w + (int)col;                                // < h w: both are whole numbers in range
    if (!(jb.z[cell] > 0.f)) return;
    c.assoc = true;
    const float *yp = jb.vertex + (size_t)cell * 3, *np = jb.normal + (size_t)cell * 3;
    c.yx = yp[0], c.yy = yp[1], c.yz = yp[2];
    c.nx = np[0], c.ny = np[1], c.nz = np[2];
    c.qx = qx, c.qy = qy, c.qz = qz;
    const float ex = qx - c.yx, ey = qy - c.yy, ez = qz - c.yz;
    const float dist = (ex * ex + ey * ey) + ez * ez;
    c.inlier = dist <= ps.thr;                                                  // a NaN is not
    c.cell = cell;
}

__global__ void __launch_bounds__(ICP_THREADS) icp_dense_kernel(tgp_icp_dense_args a)
{
    __shared__ IcpShared sh;
    __shared__ int s_cand;
    const int job = blockIdx.x, tid = threadIdx.x;
    const int img = a.job_img[job];
    const float *Rin = a.R + (size_t)job * 9, *tin = a.t + (size_t)job * 3;
    if (!(img >= 0 && img < a.S)) {                              // the same in every thread: nothing else is read
        if (tid < 9) a.R_out[(size_t)job * 9 + tid] = Rin[tid];
        if (tid < 3) a.t_out[(size_t)job * 3 + tid] = tin[tid];
        if (tid < 4) a.info[(size_t)job * 4 + tid] = tid == 0 ? 3 : 0;
        if (tid == 0) a.s_out[job] = a.s[job], a.rmse[job] = __builtin_nanf("");
        for (int i = tid; i < a.corr_cap; i += ICP_THREADS) a.corr[(size_t)job * a.corr_cap + i] = -1;
        return;
    }

    DenseJob jb;
    const size_t plane = (size_t)a.H * a.W, cells = (size_t)a.h * a.w;
    jb.frame = a.depth + (size_t)img * plane;
    jb.mframe = a.mask ? a.mask + (size_t)img * plane : nullptr;
    jb.mval = a.mask ? a.job_mask_val[job] : 0;
    jb.W = a.W, jb.stride = a.stride, jb.w = a.w;
    const int32_t *rect = a.job_rect + (size_t)job * 4;
    dense_axis(rect[0], rect[2], a.stride, a.W, jb.g.xs, jb.g.nx);
    dense_axis(rect[1], rect[3], a.stride, a.H, jb.g.ys, jb.g.ny);
    const int npix = jb.g.nx * jb.g.ny;                          // at most H W <= 2^28
    const float *K = a.camk + (size_t)img * 4, *win = a.job_window + (size_t)job * 4, *ref = a.job_ref + (size_t)job * 12;
    jb.K0 = K[0], jb.K1 = K[1], jb.K2 = K[2], jb.K3 = K[3];
    jb.cx = K[2], jb.cy = K[3];
    const UniformDiv div_fx(K[0]), div_fy(K[1]), div_k(1000.0f);
#pragma unroll
    for (int k = 0; k < 12; ++k) jb.T[k] = ref[k];
    jb.u0 = win[0], jb.v0 = win[1], jb.du = win[2], jb.dv = win[3];
    jb.wlast = (float)(a.w - 1), jb.hlast = (float)(a.h - 1);
    jb.z = a.z + (size_t)job * cells;
    jb.vertex = a.vertex + (size_t)job * cells * 3;
    jb.normal = a.normal + (size_t)job * cells * 3;

    if (tid == 0) {
        for (int k = 0; k < 9; ++k) sh.R[k] = (double)Rin[k];
        for (int k = 0; k < 3; ++k) sh.t[k] = (double)tin[k];
        sh.s = (double)a.s[job];
        sh.stop = 0, sh.status = 0, sh.iters_done = 0;
        s_cand = 0;
    }
    const double gate = (double)a.max_dist[job];
    const int min_inliers = max(a.min_inliers, 6);
    const bool never_stop = !(a.tol_rot > 0.f) && !(a.tol_trans > 0.f);
    __syncthreads();

    // pass `iters` is the association pass at the final pose
    for (int it = 0;; ++it) {
        const bool last = it >= a.iters || sh.stop;
        DensePose ps;
        ps.s = sh.s;
        ps.R0 = sh.R[0], ps.R1 = sh.R[1], ps.R2 = sh.R[2], ps.R3 = sh.R[3], ps.R4 = sh.R[4], ps.R5 = sh.R[5], ps.R6 = sh.R[6], ps.R7 = sh.R[7],
        ps.R8 = sh.R[8];
        ps.t0 = sh.t[0], ps.t1 = sh.t[1], ps.t2 = sh.t[2];
        const double g = gate / ps.s;
        ps.thr = (float)(g * g);
        DenseCell c;

        if (last) {
            double v[2] = {0.0, 0.0};
            for (int e = tid; e < npix; e += ICP_THREADS) {
                dense_pixel(jb, div_fx, div_fy, div_k, ps, e, c);
                if (c.inlier) {
                    const double dx = (double)c.qx - (double)c.yx, dy = (double)c.qy - (double)c.yy, dz = (double)c.qz - (double)c.yz;
                    v[0] = v[0] + 1.0;
                    v[1] = v[1] + ((dx * dx + dy * dy) + dz * dz);
                }
                if (e < a.corr_cap) a.corr[(size_t)job * a.corr_cap + e] = c.inlier ? c.cell : -1;
            }
            for (int e = npix + tid; e < a.corr_cap; e += ICP_THREADS) a.corr[(size_t)job * a.corr_cap + e] = -1;
            block_sum<2>(v, sh);
            if (tid == 0) {
                const double cnt = sh.sum[0];
                a.info[(size_t)job * 4] = sh.status;
                a.info[(size_t)job * 4 + 1] = (int)cnt;
                a.info[(size_t)job * 4 + 2] = sh.iters_done;
                a.info[(size_t)job * 4 + 3] = s_cand;
                a.rmse[job] = cnt > 0.0 ? (float)(ps.s * sqrt(sh.sum[1] / cnt)) : __builtin_nanf("");
                a.s_out[job] = (float)ps.s;
            }
            if (tid < 9) a.R_out[(size_t)job * 9 + tid] = (float)sh.R[tid];
            if (tid < 3) a.t_out[(size_t)job * 3 + tid] = (float)sh.t[tid];
            return;
        }

        double v[ICP_NV];
#pragma unroll
        for (int k = 0; k < ICP_NV; ++k) v[k] = 0.0;
        double cand = 0.0;
        for (int e = tid; e < npix; e += ICP_THREADS) {
            dense_pixel(jb, div_fx, div_fy, div_k, ps, e, c);
            if (c.assoc) cand = cand + 1.0;
            if (c.inlier) {
                const double nx = (double)c.nx, ny = (double)c.ny, nz = (double)c.nz;
                const double x = (double)c.qx, yy = (double)c.qy, z = (double)c.qz;
                const double row[6] = {yy * nz - z * ny, z * nx - x * nz, x * ny - yy * nx, nx, ny, nz};
                const double r = (nx * (x - (double)c.yx) + ny * (yy - (double)c.yy)) + nz * (z - (double)c.yz);
                int q = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = i; j < 6; ++j, ++q) v[q] = v[q] + row[i] * row[j];
#pragma unroll
                for (int i = 0; i < 6; ++i) v[21 + i] = v[21 + i] + row[i] * r;
                v[27] = v[27] + 1.0;
            }
        }
        if (it == 0) {                                           // the same in every thread
            block_sum<1>(&cand, sh);
            if (tid == 0) s_cand = (int)sh.sum[0];
        }
        block_sum<ICP_NV>(v, sh);
        if (tid == 0) {
            int st = 0;
            if (sh.sum[27] < (double)min_inliers) st = 1;
            else {
                double ang = 0.0, tr = 0.0;
                st = solve_plane(sh.sum, sh, ang, tr);
                if (!st) {
                    sh.iters_done = it + 1;
                    if (!never_stop && ang <= (double)a.tol_rot && tr <= (double)a.tol_trans) sh.stop = 1;
                }
            }
            if (st) {                                            // a failed job goes back to the pose it came with
                sh.status = st, sh.stop = 1;
                for (int k = 0; k < 9; ++k) sh.R[k] = (double)Rin[k];
                for (int k = 0; k < 3; ++k) sh.t[k] = (double)tin[k];
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int tgp_icp_dense(const tgp_icp_dense_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a);
    TGP_REQUIRE(a->S >= 1 && a->H >= 1 && a->W >= 1 && a->J >= 0 && a->h >= 1 && a->w >= 1 && a->stride >= 1 && a->iters >= 1);
    TGP_REQUIRE(a->tol_rot >= 0.f && a->tol_trans >= 0.f && a->min_inliers >= 0 && a->corr_cap >= 0);     // a NaN tolerance too
    TGP_REQUIRE(a->depth && a->camk && a->vertex && a->normal && a->z);
    TGP_REQUIRE(!a->mask || a->job_mask_val);
    TGP_REQUIRE(a->corr_cap == 0 || a->corr);
    if (a->J > 0) {
        TGP_REQUIRE(a->job_window && a->job_ref && a->job_img && a->job_rect && a->R && a->t && a->s && a->max_dist);
        TGP_REQUIRE(a->R_out && a->t_out && a->s_out && a->info && a->rmse);
    }
    if (a->h > TGP_RAYCAST_MAX_SIDE || a->w > TGP_RAYCAST_MAX_SIDE || a->H > 16384 || a->W > 16384 || a->J > 65535) return TGP_EUNSUPPORTED;
    if (a->J == 0) return 0;
    tgp_icp_dense_args k = *a;
    if (!k.corr) k.corr_cap = 0;
    hipLaunchKernelGGL(icp_dense_kernel, dim3(a->J), dim3(ICP_THREADS), 0, tgp_hs(stream), k);
    return TGP_LAUNCH_RESULT();
}
