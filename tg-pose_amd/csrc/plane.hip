// The supporting plane of depth frames on gfx950 (DESIGN.md section 3 "The supporting plane" and include/tgpose.h are the contract;
// tests/plane_ref.py restates it in NumPy): tgp_plane_fit finds the dominant plane of S frames by RANSAC and refits it by total
// least squares, tgp_plane_cut removes it from the frames, tgp_plane_lsq is the reference's weighted regression z = a x + b y + c
// (tools/plane_utils.py) for B clouds in one launch.
//
// tgp_plane_fit is two launches behind a memset of the counts:
//   score   grid (pixel tiles, S), 256 threads.  Every workgroup derives the frame's hypotheses itself (Philox words -> three pixels
//           -> a float64 plane, one hypothesis per thread and round) into LDS as float4: no workspace and no launch before this one.
//           A thread keeps the points of 8 consecutive pixels in registers (one 16-byte depth load where the frame allows it);
//           per hypothesis one broadcast LDS read serves all of them, the comparison's lane mask is the ballot, its population
//           count one integer add per wave into an LDS count array, flushed once per workgroup with integer atomics.
//   finish  one workgroup per frame: the first largest count, then refine_iters + 1 passes over the frame -- the inliers' float64
//           moments in a fixed order (per thread in index order, shuffle tree, waves in order), thread 0 solves the 3x3
//           eigenproblem by cyclic Jacobi rotations -- the last pass only counts.
// No float atomics; integer sums do not depend on their order: every output is bit-repeatable and a frame's result is its own.
#include "pixel_point.h"
#include "philox.h"

#pragma clang fp contract(off)        // the float64 steps are rounded one by one, whatever the command line says

namespace {

constexpr int GROUP = 8;                                  // consecutive flat pixels a thread takes at a time
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_TILE = SCORE_THREADS * GROUP;
constexpr int FIT_THREADS = TGP_PLANE_FIT_THREADS;
constexpr int FIT_WAVES = FIT_THREADS / TGP_WAVE;
constexpr int FIT_NV = 9;                                 // sum p (3), sum p p^T (6)
constexpr int CUT_THREADS = 256;
constexpr int LSQ_THREADS = TGP_PLANE_LSQ_THREADS;
constexpr int LSQ_WAVES = LSQ_THREADS / TGP_WAVE;
constexpr int MAX_HYP = TGP_PLANE_MAX_HYPOTHESES;

struct Camera {
    float cx, cy;
    UniformDiv fx, fy, k;
    __device__ __forceinline__ explicit Camera(const float *camk) : cx(camk[2]), cy(camk[3]), fx(camk[0]), fy(camk[1]), k(1000.0f) {}
    __device__ __forceinline__ void point(int x, int y, int dep, float &px, float &py, float &pz) const
    {
        tgp_pixel_point(x, y, (float)dep, cx, cy, fx, fy, k, px, py, pz);
    }
};

// the depths of flat pixels [p0, p0 + 8) of a frame of HW pixels; 0 beyond the frame.  VEC: HW is a multiple of 8 and the frame's
// base is 16-byte aligned, so a group that starts inside the frame lies inside it and is one aligned load.
template <bool VEC>
__device__ __forceinline__ void load_group(const uint16_t *dimg, int p0, int HW, int (&dep)[GROUP])
{
    if constexpr (VEC) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p0 < HW) v = *reinterpret_cast<const uint4 *>(dimg + p0);
        dep[0] = v.x & 0xffff, dep[1] = v.x >> 16, dep[2] = v.y & 0xffff, dep[3] = v.y >> 16;
        dep[4] = v.z & 0xffff, dep[5] = v.z >> 16, dep[6] = v.w & 0xffff, dep[7] = v.w >> 16;
    } else {
#pragma unroll
        for (int i = 0; i < GROUP; ++i) dep[i] = p0 + i < HW ? (int)dimg[p0 + i] : 0;
    }
}

__device__ __forceinline__ float plane_dist(float n0, float n1, float n2, float d, float px, float py, float pz)
{
    float v = n0 * px;
    v = v + n1 * py;
    v = v + n2 * pz;
    return v + d;
}

__host__ __device__ __forceinline__ bool finite4(double a, double b, double c, double d)
{
    const double inf = __builtin_inf();
    return fabs(a) < inf && fabs(b) < inf && fabs(c) < inf && fabs(d) < inf;      // false for NaN
}

// hypothesis h of a frame -> (n, d) float32, or four NaNs for a void one (a NaN plane has no inlier)
__device__ float4 plane_hypothesis(uint64_t seed, uint64_t key, int h, const uint16_t *dimg, int HW, int W, const Camera &cam)
{
    const float nan = __builtin_nanf("");
    const Words w = philox(seed, key, TGP_PLANE_SITE, (uint32_t)h);
    float p[3][3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int idx = (int)(((uint64_t)w.w[k] * (uint64_t)HW) >> 32);       // < HW
        const int dep = dimg[idx], y = idx / W, x = idx - y * W;
        ok = ok && dep > 0;
        cam.point(x, y, dep, p[k][0], p[k][1], p[k][2]);
    }
    if (!ok) return make_float4(nan, nan, nan, nan);
    const double ax = p[0][0], ay = p[0][1], az = p[0][2];
    const double ex = (double)p[1][0] - ax, ey = (double)p[1][1] - ay, ez = (double)p[1][2] - az;
    const double fx = (double)p[2][0] - ax, fy = (double)p[2][1] - ay, fz = (double)p[2][2] - az;
    const double cx = ey * fz - ez * fy, cy = ez * fx - ex * fz, cz = ex * fy - ey * fx;
    const double nn = (cx * cx + cy * cy) + cz * cz;
    if (!(nn > 1e-18)) return make_float4(nan, nan, nan, nan);
    const double nrm = sqrt(nn);
    double nx = cx / nrm, ny = cy / nrm, nz = cz / nrm;
    double d = -((nx * ax + ny * ay) + nz * az);
    if (d < 0.0) nx = -nx, ny = -ny, nz = -nz, d = -d;
    return make_float4((float)nx, (float)ny, (float)nz, (float)d);
}

template <bool VEC>
__global__ void __launch_bounds__(SCORE_THREADS) plane_score_kernel(const tgp_plane_fit_args a)
{
    __shared__ float4 s_hyp[MAX_HYP];
    __shared__ int s_cnt[MAX_HYP];
    const int s = blockIdx.y, tid = threadIdx.x, lane = tid & (TGP_WAVE - 1);
    const int W = a.W, HW = a.H * a.W, Hn = a.hypotheses;
    const uint16_t *dimg = a.depth + (size_t)s * HW;
    const Camera cam(a.camk + s * 4);
    const uint64_t key = a.keys[s];
    for (int h = tid; h < Hn; h += SCORE_THREADS) {
        s_hyp[h] = plane_hypothesis(a.seed, key, h, dimg, HW, W, cam);
        s_cnt[h] = 0;
    }
    const int p0 = blockIdx.x * SCORE_TILE + tid * GROUP;
    int dep[GROUP];
    load_group<VEC>(dimg, p0, HW, dep);
    float px[GROUP], py[GROUP], pz[GROUP];
    {
        int y = p0 / W, x = p0 - y * W;
#pragma unroll
        for (int i = 0; i < GROUP; ++i) {
            px[i] = py[i] = pz[i] = __builtin_nanf("");      // an invalid pixel is inside no plane's band
            if (dep[i] > 0) cam.point(x, y, dep[i], px[i], py[i], pz[i]);
            if (++x == W) x = 0, ++y;
        }
    }
    const float tol = a.tol;
    __syncthreads();
    for (int h = 0; h < Hn; ++h) {
        const float4 pl = s_hyp[h];                          // one address for the wave: a broadcast read
        if (pl.x != pl.x) continue;                          // void: the same in every thread
        int c = 0;
#pragma unroll
        for (int i = 0; i < GROUP; ++i) c += __popcll(__ballot(fabsf(plane_dist(pl.x, pl.y, pl.z, pl.w, px[i], py[i], pz[i])) <= tol));
        if (lane == 0 && c) atomicAdd(&s_cnt[h], c);
    }
    __syncthreads();
    for (int h = tid; h < Hn; h += SCORE_THREADS)
        if (s_cnt[h]) atomicAdd(&a.counts[(size_t)s * Hn + h], s_cnt[h]);
}

struct FitShared {
    double red[FIT_WAVES][FIT_NV];
    double sum[FIT_NV];
    int ired[FIT_WAVES][2];
    int best_cnt[FIT_WAVES], best_idx[FIT_WAVES];
    float plane[4];
    int status;
};

// eigenvector of the smallest eigenvalue of the symmetric 3x3 matrix a (destroyed): cyclic Jacobi rotations (icp.hip has the 4x4 form)
__host__ __device__ void bottom_eigenvector3(double a[3][3], double q[3])
{
    double v[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = (fabs(a[0][1]) + fabs(a[0][2])) + fabs(a[1][2]);
        if (!(off > 0.0)) break;
        for (int p = 0; p < 2; ++p)
            for (int r = p + 1; r < 3; ++r) {
                const double apr = a[p][r];
                if (apr == 0.0) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * apr);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
                for (int k = 0; k < 3; ++k) {                    // A <- A G
                    const double akp = a[k][p], akr = a[k][r];
                    a[k][p] = c * akp - sn * akr;
                    a[k][r] = sn * akp + c * akr;
                }
                for (int k = 0; k < 3; ++k) {                    // A <- G^T A
                    const double apk = a[p][k], ark = a[r][k];
                    a[p][k] = c * apk - sn * ark;
                    a[r][k] = sn * apk + c * ark;
                }
                a[p][r] = a[r][p] = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = c * vkp - sn * vkr;
                    v[k][r] = sn * vkp + c * vkr;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 3; ++i)
        if (a[i][i] < a[best][best]) best = i;
    for (int k = 0; k < 3; ++k) q[k] = v[k][best];
}

// the total-least-squares plane of N points from sm = (sum p (3), sum p p^T upper triangle xx xy xz yy yz zz) -> false when not finite
__host__ __device__ bool refit_plane(const double *sm, double N, float *plane)
{
    const double mx = sm[0] / N, my = sm[1] / N, mz = sm[2] / N;
    double C[3][3];
    C[0][0] = sm[3] - sm[0] * sm[0] / N, C[0][1] = sm[4] - sm[0] * sm[1] / N, C[0][2] = sm[5] - sm[0] * sm[2] / N;
    C[1][1] = sm[6] - sm[1] * sm[1] / N, C[1][2] = sm[7] - sm[1] * sm[2] / N, C[2][2] = sm[8] - sm[2] * sm[2] / N;
    C[1][0] = C[0][1], C[2][0] = C[0][2], C[2][1] = C[1][2];
    for (int i = 0; i < 3; ++i)
        if (!finite4(C[i][0], C[i][1], C[i][2], 0.0)) return false;
    double q[3];
    bottom_eigenvector3(C, q);
    const double nq = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    double nx = q[0] / nq, ny = q[1] / nq, nz = q[2] / nq;
    double d = -((nx * mx + ny * my) + nz * mz);
    if (d < 0.0) nx = -nx, ny = -ny, nz = -nz, d = -d;
    if (!finite4(nx, ny, nz, d)) return false;
    plane[0] = (float)nx, plane[1] = (float)ny, plane[2] = (float)nz, plane[3] = (float)d;
    return true;
}

template <bool VEC>
__global__ void __launch_bounds__(FIT_THREADS) plane_finish_kernel(const tgp_plane_fit_args a)
{
    __shared__ FitShared sh;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (TGP_WAVE - 1), wave = tid / TGP_WAVE;
    const int W = a.W, HW = a.H * a.W, Hn = a.hypotheses;
    const uint16_t *dimg = a.depth + (size_t)s * HW;
    const Camera cam(a.camk + s * 4);

    // the largest count, the first index on ties
    int bc = -1, bi = 0x7fffffff;
    for (int h = tid; h < Hn; h += FIT_THREADS) {
        const int c = a.counts[(size_t)s * Hn + h];
        if (c > bc) bc = c, bi = h;
    }
#pragma unroll
    for (int o = TGP_WAVE / 2; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o), oi = __shfl_xor(bi, o);
        if (oc > bc || (oc == bc && oi < bi)) bc = oc, bi = oi;
    }
    if (lane == 0) sh.best_cnt[wave] = bc, sh.best_idx[wave] = bi;
    __syncthreads();
    bc = sh.best_cnt[0], bi = sh.best_idx[0];
    for (int w = 1; w < FIT_WAVES; ++w)
        if (sh.best_cnt[w] > bc || (sh.best_cnt[w] == bc && sh.best_idx[w] < bi)) bc = sh.best_cnt[w], bi = sh.best_idx[w];
    const int best_count = bc;
    if (tid == 0) {
        const float nan = __builtin_nanf("");
        float4 pl = make_float4(nan, nan, nan, nan);
        sh.status = best_count < max(a.min_inliers, 3) ? 1 : 0;
        if (!sh.status) pl = plane_hypothesis(a.seed, a.keys[s], bi, dimg, HW, W, cam);
        sh.plane[0] = pl.x, sh.plane[1] = pl.y, sh.plane[2] = pl.z, sh.plane[3] = pl.w;
    }
    __syncthreads();

    const float tol = a.tol;
    const int groups = (HW + GROUP - 1) / GROUP;
    for (int it = 0;; ++it) {
        const bool last = it >= a.refine_iters || sh.status != 0;      // the same in every thread
        const float n0 = sh.plane[0], n1 = sh.plane[1], n2 = sh.plane[2], d = sh.plane[3];
        int cnt = 0, nvalid = 0;
        double v[FIT_NV];
#pragma unroll
        for (int c = 0; c < FIT_NV; ++c) v[c] = 0.0;
        for (int g = tid; g < groups; g += FIT_THREADS) {
            const int p0 = g * GROUP;
            int dep[GROUP];
            load_group<VEC>(dimg, p0, HW, dep);
            int y = p0 / W, x = p0 - y * W;
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                if (dep[i] > 0) {
                    float px, py, pz;
                    cam.point(x, y, dep[i], px, py, pz);
                    ++nvalid;
                    if (fabsf(plane_dist(n0, n1, n2, d, px, py, pz)) <= tol) {
                        ++cnt;
                        if (!last) {
                            const double X = px, Y = py, Z = pz;
                            v[0] = v[0] + X, v[1] = v[1] + Y, v[2] = v[2] + Z;
                            v[3] = v[3] + X * X, v[4] = v[4] + X * Y, v[5] = v[5] + X * Z;
                            v[6] = v[6] + Y * Y, v[7] = v[7] + Y * Z, v[8] = v[8] + Z * Z;
                        }
                    }
                }
                if (++x == W) x = 0, ++y;
            }
        }
#pragma unroll
        for (int o = TGP_WAVE / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o), nvalid += __shfl_xor(nvalid, o);
        if (lane == 0) sh.ired[wave][0] = cnt, sh.ired[wave][1] = nvalid;
        if (!last) {
#pragma unroll
            for (int k = 0; k < FIT_NV; ++k) {
                double x = v[k];
#pragma unroll
                for (int off = TGP_WAVE / 2; off >= 1; off >>= 1) x = x + __shfl_down(x, off, TGP_WAVE);
                if (lane == 0) sh.red[wave][k] = x;
            }
        }
        __syncthreads();
        cnt = nvalid = 0;
        for (int w = 0; w < FIT_WAVES; ++w) cnt += sh.ired[w][0], nvalid += sh.ired[w][1];
        if (last) {
            if (tid == 0) {
                const bool none = sh.status == 1;
                for (int k = 0; k < 4; ++k) a.plane[(size_t)s * 4 + k] = none ? 0.f : sh.plane[k];
                a.info[(size_t)s * 4] = sh.status;
                a.info[(size_t)s * 4 + 1] = best_count;
                a.info[(size_t)s * 4 + 2] = none ? 0 : cnt;
                a.info[(size_t)s * 4 + 3] = nvalid;
            }
            return;
        }
        if (tid < FIT_NV) {
            double x = sh.red[0][tid];
            for (int w = 1; w < FIT_WAVES; ++w) x = x + sh.red[w][tid];
            sh.sum[tid] = x;
        }
        __syncthreads();
        if (tid == 0) {
            float pl[4];
            if (refit_plane(sh.sum, (double)cnt, pl)) sh.plane[0] = pl[0], sh.plane[1] = pl[1], sh.plane[2] = pl[2], sh.plane[3] = pl[3];
            else sh.status = 2;
        }
        __syncthreads();
    }
}

// one thread per group of 8 flat pixels.  VEC: depth and out are read / written 16 bytes, side 8 bytes at a time
template <bool VEC>
__global__ void __launch_bounds__(CUT_THREADS) plane_cut_kernel(const uint16_t *__restrict__ depth, const float *__restrict__ plane,
                                                               const int32_t *__restrict__ info, const float *__restrict__ camk, int H, int W,
                                                               float margin, uint16_t *out, uint8_t *side)
{
    const int s = blockIdx.y, HW = H * W;
    const int p0 = (blockIdx.x * CUT_THREADS + threadIdx.x) * GROUP;
    if (p0 >= HW) return;
    const uint16_t *dimg = depth + (size_t)s * HW;
    const Camera cam(camk + s * 4);
    const float n0 = plane[s * 4], n1 = plane[s * 4 + 1], n2 = plane[s * 4 + 2], d = plane[s * 4 + 3];
    const bool through = info[s * 4] != 0;
    int dep[GROUP];
    load_group<VEC>(dimg, p0, HW, dep);
    uint32_t o[GROUP], sd[GROUP];
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int i = 0; i < GROUP; ++i) {
        o[i] = 0, sd[i] = 0;
        if (dep[i] > 0) {
            float px, py, pz;
            cam.point(x, y, dep[i], px, py, pz);
            const float dist = plane_dist(n0, n1, n2, d, px, py, pz);
            sd[i] = dist > margin ? 2 : dist < -margin ? 3 : 1;
            o[i] = through || dist > margin ? (uint32_t)dep[i] : 0;
        }
        if (++x == W) x = 0, ++y;
    }
    uint16_t *oimg = out + (size_t)s * HW;
    uint8_t *simg = side ? side + (size_t)s * HW : nullptr;
    if constexpr (VEC) {
        *reinterpret_cast<uint4 *>(oimg + p0) = make_uint4(o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16);
        if (simg)
            *reinterpret_cast<uint2 *>(simg + p0) = make_uint2(sd[0] | sd[1] << 8 | sd[2] << 16 | sd[3] << 24, sd[4] | sd[5] << 8 | sd[6] << 16 | sd[7] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < GROUP; ++i)
            if (p0 + i < HW) {
                oimg[p0 + i] = (uint16_t)o[i];
                if (simg) simg[p0 + i] = (uint8_t)sd[i];
            }
    }
}

__global__ void __launch_bounds__(LSQ_THREADS) plane_lsq_kernel(const float *__restrict__ pc, const float *__restrict__ wt, int n, double eps,
                                                               float *__restrict__ Xo, float *__restrict__ normal, float *__restrict__ dn,
                                                               float *__restrict__ p2plane)
{
    __shared__ double red[LSQ_WAVES][9];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (TGP_WAVE - 1), wave = tid / TGP_WAVE;
    const float *p = pc + (size_t)b * n * 3, *w = wt + (size_t)b * n;
    double v[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = 0.0;
    for (int i = tid; i < n; i += LSQ_THREADS) {
        const double x = p[(size_t)i * 3], y = p[(size_t)i * 3 + 1], z = p[(size_t)i * 3 + 2], wi = w[i];
        const double wx = wi * x, wy = wi * y;                 // exact: two float32 factors
        v[0] = v[0] + wx * x, v[1] = v[1] + wx * y, v[2] = v[2] + wx;
        v[3] = v[3] + wy * y, v[4] = v[4] + wy, v[5] = v[5] + wi;
        v[6] = v[6] + wx * z, v[7] = v[7] + wy * z, v[8] = v[8] + wi * z;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        double x = v[k];
#pragma unroll
        for (int off = TGP_WAVE / 2; off >= 1; off >>= 1) x = x + __shfl_down(x, off, TGP_WAVE);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
    if (tid != 0) return;
    double m[9];
    for (int k = 0; k < 9; ++k) {
        double x = red[0][k];
        for (int wv = 1; wv < LSQ_WAVES; ++wv) x = x + red[wv][k];
        m[k] = x;
    }
    const double m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[3], m12 = m[4], m22 = m[5];
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    const double nan = __builtin_nan("");
    double A = nan, Bc = nan, C = nan;
    if (fabs(det) > 1e-12 * fabs(m00 * m11 * m22) && fabs(det) < __builtin_inf()) {
        A = ((c00 * m[6] + c01 * m[7]) + c02 * m[8]) / det;
        Bc = ((c01 * m[6] + c11 * m[7]) + c12 * m[8]) / det;
        C = ((c02 * m[6] + c12 * m[7]) + c22 * m[8]) / det;
    }
    const double q = (A * A + Bc * Bc) + 1.0;
    const double d0 = A * C / (q + eps), d1 = Bc * C / (q + eps), d2 = -C / (q + eps);
    const double len = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    Xo[b * 3] = (float)A, Xo[b * 3 + 1] = (float)Bc, Xo[b * 3 + 2] = (float)C;
    dn[b * 3] = (float)d0, dn[b * 3 + 1] = (float)d1, dn[b * 3 + 2] = (float)d2;
    normal[b * 3] = (float)(d0 / len), normal[b * 3 + 1] = (float)(d1 / len), normal[b * 3 + 2] = (float)(d2 / len);
    p2plane[b] = (float)(C / sqrt(q));
}

bool plane_aligned(const void *p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1u)) == 0; }

bool plane_frames_ok(int S, int H, int W) { return S >= 1 && H >= 1 && W >= 1 && H < 32768 && W < 32768 && (int64_t)H * W < (1ll << 24); }

}  // namespace

extern "C" int tgp_plane_fit(const tgp_plane_fit_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->depth && a->camk && a->keys && a->plane && a->info && a->counts);
    TGP_REQUIRE(plane_frames_ok(a->S, a->H, a->W));
    TGP_REQUIRE(a->hypotheses >= 1 && a->hypotheses <= MAX_HYP && a->refine_iters >= 0 && a->refine_iters <= TGP_PLANE_MAX_REFITS);
    TGP_REQUIRE(a->tol >= 0.f && a->tol < __builtin_inff() && a->min_inliers >= 0);
    if (a->S > 65535) return TGP_EUNSUPPORTED;
    const hipStream_t st = tgp_hs(stream);
    const int HW = a->H * a->W;
    const hipError_t e = hipMemsetAsync(a->counts, 0, (size_t)a->S * a->hypotheses * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const dim3 grid(tgp_cdiv(HW, SCORE_TILE), a->S);
    const bool vec = HW % GROUP == 0 && plane_aligned(a->depth, 16);
    if (vec) hipLaunchKernelGGL(plane_score_kernel<true>, grid, dim3(SCORE_THREADS), 0, st, *a);
    else hipLaunchKernelGGL(plane_score_kernel<false>, grid, dim3(SCORE_THREADS), 0, st, *a);
    const int rc = TGP_LAUNCH_RESULT();
    if (rc) return rc;
    if (vec) hipLaunchKernelGGL(plane_finish_kernel<true>, dim3(a->S), dim3(FIT_THREADS), 0, st, *a);
    else hipLaunchKernelGGL(plane_finish_kernel<false>, dim3(a->S), dim3(FIT_THREADS), 0, st, *a);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_plane_cut(const uint16_t *depth, const float *plane, const int32_t *info, const float *camk, int S, int H, int W,
                             float margin, uint16_t *out, uint8_t *side, tgp_stream_t stream)
{
    TGP_REQUIRE(depth && plane && info && camk && out);
    TGP_REQUIRE(plane_frames_ok(S, H, W) && margin >= 0.f && margin < __builtin_inff());
    if (S > 65535) return TGP_EUNSUPPORTED;
    const int HW = H * W;
    const dim3 grid(tgp_cdiv(tgp_cdiv(HW, GROUP), CUT_THREADS), S);
    if (HW % GROUP == 0 && plane_aligned(depth, 16) && plane_aligned(out, 16) && (!side || plane_aligned(side, 8)))
        hipLaunchKernelGGL(plane_cut_kernel<true>, grid, dim3(CUT_THREADS), 0, tgp_hs(stream), depth, plane, info, camk, H, W, margin, out, side);
    else
        hipLaunchKernelGGL(plane_cut_kernel<false>, grid, dim3(CUT_THREADS), 0, tgp_hs(stream), depth, plane, info, camk, H, W, margin, out, side);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_plane_lsq(const float *pc, const float *w, int B, int n, double eps, float *X, float *normal, float *dn, float *p2plane,
                             tgp_stream_t stream)
{
    TGP_REQUIRE(pc && w && X && normal && dn && p2plane && B >= 1 && n >= 1 && eps >= 0.0 && eps < __builtin_inf());
    hipLaunchKernelGGL(plane_lsq_kernel, dim3(B), dim3(LSQ_THREADS), 0, tgp_hs(stream), pc, w, n, eps, X, normal, dn, p2plane);
    return TGP_LAUNCH_RESULT();
}
