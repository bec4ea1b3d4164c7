// What the ICP kernels share (icp.hip: nearest-neighbour association against point models; icp_dense.hip: projective association
// against ray-cast maps): the workgroup's shape and shared state, the fixed-order float64 reduction, and the float64 solves that lane
// 0 runs.  One text, so that both kernels' updates are the same arithmetic.
#pragma once
#include "tgp_common.h"

namespace {

constexpr int ICP_THREADS = 512;
constexpr int ICP_WAVES = ICP_THREADS / TGP_WAVE;
constexpr int ICP_NV = 28;            // the widest reduction: 21 + 6 + 1 (point-to-plane)

struct IcpShared {
    double red[ICP_WAVES][ICP_NV];
    double sum[ICP_NV];
    double R[9], t[3], s;
    int stop;                          // 0 go on; 1 leave the loop
    int status, iters_done;
};

// sum of v[0..NV) over the workgroup -> sh.sum[0..NV), visible to every thread on return
template <int NV>
__device__ __forceinline__ void block_sum(double *v, IcpShared &sh)
{
    const int lane = threadIdx.x & (TGP_WAVE - 1), wave = threadIdx.x / TGP_WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double x = v[k];
#pragma unroll
        for (int off = TGP_WAVE / 2; off >= 1; off >>= 1) x = x + __shfl_down(x, off, TGP_WAVE);
        if (lane == 0) sh.red[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double x = sh.red[0][threadIdx.x];
        for (int w = 1; w < ICP_WAVES; ++w) x = x + sh.red[w][threadIdx.x];
        sh.sum[threadIdx.x] = x;
    }
    __syncthreads();
}

// The solves below are plain float64 C++ that lane 0 runs; they are __host__ too so that a stand-alone host program (with a host
// sanitizer) can call them.
__host__ __device__ __forceinline__ bool finite3(double a, double b, double c)
{
    const double inf = __builtin_inf();
    return fabs(a) < inf && fabs(b) < inf && fabs(c) < inf;      // false for NaN
}

// eigenvector of the largest eigenvalue of the symmetric 4x4 matrix a (destroyed): cyclic Jacobi rotations
__host__ __device__ void top_eigenvector4(double a[4][4], double q[4])
{
    double v[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) off += fabs(a[i][j]);
        if (!(off > 0.0)) break;
        for (int p = 0; p < 3; ++p)
            for (int r = p + 1; r < 4; ++r) {
                const double apr = a[p][r];
                if (apr == 0.0) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * apr);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
                for (int k = 0; k < 4; ++k) {                    // A <- A G
                    const double akp = a[k][p], akr = a[k][r];
                    a[k][p] = c * akp - sn * akr;
                    a[k][r] = sn * akp + c * akr;
                }
                for (int k = 0; k < 4; ++k) {                    // A <- G^T A
                    const double apk = a[p][k], ark = a[r][k];
                    a[p][k] = c * apk - sn * ark;
                    a[r][k] = sn * apk + c * ark;
                }
                a[p][r] = a[r][p] = 0.0;
                for (int k = 0; k < 4; ++k) {
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = c * vkp - sn * vkr;
                    v[k][r] = sn * vkp + c * vkr;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (a[i][i] > a[best][best]) best = i;
    for (int k = 0; k < 4; ++k) q[k] = v[k][best];
}

// rotation angle of Ra^T Rb (row-major 3x3)
__host__ __device__ double rotation_between(const double *Ra, const double *Rb)
{
    double D[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[i * 3 + j] = (Ra[0 + i] * Rb[0 + j] + Ra[3 + i] * Rb[3 + j]) + Ra[6 + i] * Rb[6 + j];
    const double vx = 0.5 * (D[7] - D[5]), vy = 0.5 * (D[2] - D[6]), vz = 0.5 * (D[3] - D[1]);
    const double sn = sqrt((vx * vx + vy * vy) + vz * vz), cs = 0.5 * (((D[0] + D[4]) + D[8]) - 1.0);
    return atan2(sn, cs);
}

// Mode 0 by lane 0: sums A = (n, sum p, sum y), B = (S[a][b] = sum yc_a pc_b, sum |yc|^2).  Returns the status (0 or 2) and leaves
// the update's rotation angle and translation in ang / tr.
__host__ __device__ int solve_point(const double *S9, double var_y, const double *pbar, const double *ybar, int with_scale, IcpShared &sh, double &ang,
                           double &tr)
{
    const double Sxx = S9[0], Sxy = S9[1], Sxz = S9[2], Syx = S9[3], Syy = S9[4], Syz = S9[5], Szx = S9[6], Szy = S9[7], Szz = S9[8];
    double N[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double q[4];
    top_eigenvector4(N, q);
    const double nq = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(nq > 0.0) || !(nq < __builtin_inf())) return 2;
    const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
    double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                   2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                   2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    double s = sh.s;
    if (with_scale) {
        double num = 0.0;                                        // sum_i pc_i . (R yc_i) = sum_ab R[a][b] S[b][a]
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) num = num + R[a * 3 + b] * S9[b * 3 + a];
        s = num / var_y;
        if (!(s > 0.0) || !(s < __builtin_inf())) return 2;
    }
    double t[3];
    for (int a = 0; a < 3; ++a) t[a] = pbar[a] - s * ((R[a * 3] * ybar[0] + R[a * 3 + 1] * ybar[1]) + R[a * 3 + 2] * ybar[2]);
    for (int k = 0; k < 9; ++k)
        if (!(fabs(R[k]) < __builtin_inf())) return 2;
    if (!finite3(t[0], t[1], t[2])) return 2;
    ang = rotation_between(sh.R, R);
    const double dx = t[0] - sh.t[0], dy = t[1] - sh.t[1], dz = t[2] - sh.t[2];
    tr = sqrt((dx * dx + dy * dy) + dz * dz);
    for (int k = 0; k < 9; ++k) sh.R[k] = R[k];
    for (int k = 0; k < 3; ++k) sh.t[k] = t[k];
    sh.s = s;
    return 0;
}

// Mode 1 by lane 0: sm = the 21 upper entries of A row by row, then b (6).  One damped Gauss-Newton step.
__host__ __device__ int solve_plane(const double *sm, IcpShared &sh, double &ang, double &tr)
{
    double A[6][6], b[6], L[6][6], x[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = sm[k++];
    for (int i = 0; i < 6; ++i) b[i] = sm[21 + i];
    double trace = 0.0;
    for (int i = 0; i < 6; ++i) trace = trace + A[i][i];
    const double lambda = 1e-9 * trace / 6.0;
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + lambda;
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int c = 0; c < j; ++c) d = d - L[j][c] * L[j][c];
        if (!(d > 0.0)) return 2;
        const double ljj = sqrt(d);
        L[j][j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int c = 0; c < j; ++c) v = v - L[i][c] * L[j][c];
            L[i][j] = v / ljj;
        }
    }
    for (int i = 0; i < 6; ++i) {                                // L z = -b
        double v = -b[i];
        for (int c = 0; c < i; ++c) v = v - L[i][c] * x[c];
        x[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {                               // L^T x = z
        double v = x[i];
        for (int c = i + 1; c < 6; ++c) v = v - L[c][i] * x[c];
        x[i] = v / L[i][i];
    }
    if (!finite3(x[0], x[1], x[2]) || !finite3(x[3], x[4], x[5])) return 2;
    const double wx = x[0], wy = x[1], wz = x[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
    double ca, cb;                                               // E = I + ca K + cb K^2
    if (th < 1e-4) ca = 1.0 - th2 / 6.0, cb = 0.5 - th2 / 24.0;
    else ca = sin(th) / th, cb = (1.0 - cos(th)) / th2;
    const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double E[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double k2 = (K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j]) + K[i * 3 + 2] * K[6 + j];
            E[i * 3 + j] = ((i == j ? 1.0 : 0.0) + ca * K[i * 3 + j]) + cb * k2;
        }
    double R[9];                                                 // R E^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = (sh.R[i * 3] * E[j * 3] + sh.R[i * 3 + 1] * E[j * 3 + 1]) + sh.R[i * 3 + 2] * E[j * 3 + 2];
    double t[3];
    for (int a = 0; a < 3; ++a) t[a] = sh.t[a] - sh.s * ((R[a * 3] * x[3] + R[a * 3 + 1] * x[4]) + R[a * 3 + 2] * x[5]);
    for (int q = 0; q < 9; ++q)
        if (!(fabs(R[q]) < __builtin_inf())) return 2;
    if (!finite3(t[0], t[1], t[2])) return 2;
    ang = th;
    tr = sh.s * sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    for (int q = 0; q < 9; ++q) sh.R[q] = R[q];
    for (int q = 0; q < 3; ++q) sh.t[q] = t[q];
    return 0;
}

}  // namespace
