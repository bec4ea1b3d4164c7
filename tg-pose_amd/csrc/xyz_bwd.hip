// Gradients with respect to the point coordinates (gcn3d.py:48-58 get_neighbor_direction_norm, the graph convolutions' theta,
// PoseNet9D.py:37,48 centring) and the eval-mode BatchNorm backward of the differentiable path.  No float atomics: every element
// of d xyz, d gamma and d beta is summed by one thread in a fixed order, so the results are bit-repeatable.
//
//   tgp_gconv_dirgrad    d(unit neighbour direction) (B, n, k, 3) of HSlayer_surface / HS_layer.graph_conv from d g (B, n, C)
//   tgp_neighbor_dirs    get_neighbor_direction_norm's forward: unit (and unnormalised) directions (B, n, k, 3) to the neighbours
//   tgp_dirs_to_xyz      F.normalize's backward + the difference's: d xyz[i] -= sum_j du_ij, d xyz[q] += du over q's reverse list
//   tgp_center_bwd       backward of (points - mean, mean): d points = d xyz + (d mean - sum_i d xyz_i) / n
//   tgp_bn_eval_bwd      backward of act((x - running_mean) / sqrt(running_var + eps) * gamma + beta) over rows: dx, d gamma, d beta
//   tgp_bn_eval_bwd_pooled  the same for the max over each object's points (the winners' rows only)
#include "tgp_common.h"

#define XB_S 7
#define XB_MAXK 64
#define XB_THREADS 256

// unit direction of neighbour row pn from centre pc, as every forward kernel computes it (gconv.hip / graph_bwd.hip)
__device__ __forceinline__ void xb_unit(const float *pn, const float *pc, float &ux, float &uy, float &uz)
{
    float dx = pn[0] - pc[0], dy = pn[1] - pc[1], dz = pn[2] - pc[2];
    const float nrm = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 1e-12f);
    ux = dx / nrm, uy = dy / nrm, uz = dz / nrm;
}

// theta of the forward kernels: the same fmaf chain
__device__ __forceinline__ float xb_theta(float ux, float uy, float uz, float s0, float s1, float s2)
{
    return fmaf(uz, s2, fmaf(uy, s1, ux * s0));
}

// One workgroup per point.  Phase 1: one thread per element e = s * C + c finds the winning neighbour of max_j over relu(theta_j)
// (surface) or relu(theta_j) * support_j (HS) -- strict '>' in slot order, the first maximum wins -- or takes it from the forward's
// slots, and the gradient that reaches theta at the winner: d g[c] / 7 (the mean over the supports), times the winner's support
// value (HS), where theta* > 0 (ReLU' (0) = 0).  Phase 2: d dir[j][comp] = sum over e whose winner is j of that gradient *
// sdn[comp][e], in e order: threads (group, j, comp) take contiguous shares of e, the shares are added in group order.
template <bool HS>
__global__ __launch_bounds__(XB_THREADS) void gconv_dirgrad_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ idx,
                                                                   const float *__restrict__ proj, int ldp, const float *__restrict__ sdn,
                                                                   const float *__restrict__ dg, int ldg, const uint8_t *__restrict__ slots,
                                                                   int n, int k, int C, float *__restrict__ ddir)
{
    extern __shared__ float xb_dyn[];
    __shared__ float s_u[XB_MAXK][3];
    __shared__ int s_nj[XB_MAXK];
    __shared__ float s_part[XB_THREADS];
    const int SC = XB_S * C;
    float *s_w = xb_dyn;                                            // (SC) gradient at theta*
    uint8_t *s_j = reinterpret_cast<uint8_t *>(xb_dyn + SC);       // (SC) winner
    const int64_t row = blockIdx.x;                                  // b * n + i
    const int64_t base = row - row % n;                              // b * n
    const int t = threadIdx.x;
    if (t < k) {
        const int nj = idx[row * k + t];
        float ux, uy, uz;
        xb_unit(xyz + (base + nj) * 3, xyz + row * 3, ux, uy, uz);
        s_u[t][0] = ux, s_u[t][1] = uy, s_u[t][2] = uz;
        s_nj[t] = nj;
    }
    __syncthreads();
    for (int e = t; e < SC; e += XB_THREADS) {
        const float s0 = sdn[e], s1 = sdn[SC + e], s2 = sdn[2 * SC + e];
        int js = 255;
        if (slots) {
            js = slots[row * SC + e];
        } else {
            float best = -INFINITY;
            for (int j = 0; j < k; ++j) {
                float v = fmaxf(xb_theta(s_u[j][0], s_u[j][1], s_u[j][2], s0, s1, s2), 0.f);
                if (HS) v = v * proj[(base + s_nj[j]) * ldp + C + e];
                if (v > best) best = v, js = j;
            }
        }
        float w = 0.f;
        if (js < k) {
            const float th = xb_theta(s_u[js][0], s_u[js][1], s_u[js][2], s0, s1, s2);
            if (th > 0.f) {
                w = dg[row * ldg + e % C] / 7.0f;
                if (HS) w = w * proj[(base + s_nj[js]) * ldp + C + e];
            }
        } else {
            js = 255;
        }
        s_w[e] = w;
        s_j[e] = (uint8_t)js;
    }
    __syncthreads();
    const int P = 3 * k;
    const int G = XB_THREADS / P;                                    // >= 1 for k <= 64 (P <= 192)
    const int grp = t / P, jc = t % P;
    float acc = 0.f;
    if (grp < G) {
        const int j = jc / 3;
        const float *sc = sdn + (jc % 3) * SC;
        const int per = (SC + G - 1) / G;
        const int e0 = grp * per, e1 = min(SC, e0 + per);
        for (int e = e0; e < e1; ++e)
            if (s_j[e] == j) acc = acc + s_w[e] * sc[e];
    }
    s_part[t] = acc;
    __syncthreads();
    if (t < P) {
        float s = s_part[t];
        for (int g = 1; g < G; ++g) s = s + s_part[g * P + t];
        ddir[row * P + t] = s;
    }
}

extern "C" int tgp_gconv_dirgrad(const float *xyz, const int32_t *idx, const float *proj, int ldp, const float *sdn, const float *dg, int ldg,
                                 const uint8_t *slots, int B, int n, int k, int S, int C, float *ddir, tgp_stream_t stream)
{
    TGP_REQUIRE(xyz && idx && sdn && dg && ddir && B > 0 && n > 0 && k > 0 && C > 0 && ldg >= C);
    TGP_REQUIRE(!proj || ldp >= 8 * C);
    TGP_REQUIRE(!slots || proj);                     // the slots are the HS layer's
    if (S != XB_S || k > XB_MAXK || (int64_t)B * n >= 0x7fffffff || (int64_t)B * n * XB_S * C >= ((int64_t)1 << 40)) return TGP_EUNSUPPORTED;
    const size_t lds = (size_t)XB_S * C * 5 + 16;
    if (lds > 60 * 1024) return TGP_EUNSUPPORTED;
    if (proj)
        hipLaunchKernelGGL(gconv_dirgrad_kernel<true>, dim3((unsigned)((int64_t)B * n)), dim3(XB_THREADS), lds, tgp_hs(stream), xyz, idx, proj,
                           ldp, sdn, dg, ldg, slots, n, k, C, ddir);
    else
        hipLaunchKernelGGL(gconv_dirgrad_kernel<false>, dim3((unsigned)((int64_t)B * n)), dim3(XB_THREADS), lds, tgp_hs(stream), xyz, idx,
                           nullptr, 0, sdn, dg, ldg, nullptr, n, k, C, ddir);
    return TGP_LAUNCH_RESULT();
}

// one thread per (point, neighbour): u = x[idx] - x, unit = u / max(|u|, 1e-12) (the forward kernels' expression)
__global__ __launch_bounds__(256) void neighbor_dirs_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ idx, int64_t rows, int n, int k,
                                                            float *__restrict__ unit, float *__restrict__ unnormed)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * k) return;
    const int64_t row = e / k;
    const int64_t base = row - row % n;
    const float *pn = xyz + (base + idx[e]) * 3, *pc = xyz + row * 3;
    float ux, uy, uz;
    xb_unit(pn, pc, ux, uy, uz);
    unit[e * 3] = ux, unit[e * 3 + 1] = uy, unit[e * 3 + 2] = uz;
    if (unnormed) unnormed[e * 3] = pn[0] - pc[0], unnormed[e * 3 + 1] = pn[1] - pc[1], unnormed[e * 3 + 2] = pn[2] - pc[2];
}

extern "C" int tgp_neighbor_dirs(const float *xyz, const int32_t *idx, int B, int n, int k, float *unit, float *unnormed, tgp_stream_t stream)
{
    TGP_REQUIRE(xyz && idx && unit && B > 0 && n > 0 && k > 0);
    const int64_t rows = (int64_t)B * n;
    hipLaunchKernelGGL(neighbor_dirs_kernel, dim3(tgp_cdiv(rows * k, 256)), dim3(256), 0, tgp_hs(stream), xyz, idx, rows, n, k, unit, unnormed);
    return TGP_LAUNCH_RESULT();
}

// d u of y = u / max(|u|, 1e-12) as torch differentiates F.normalize (norm -> clamp_min -> div): dy / den, minus u (dy . u) / den^2 / |u|
// where |u| >= eps (clamp_min passes its gradient there; the norm's own backward is 0 at |u| == 0)
__device__ __forceinline__ void xb_norm_bwd(float ux, float uy, float uz, const float *__restrict__ dy, const float *__restrict__ dun, float *du)
{
    const float r = sqrtf((ux * ux + uy * uy) + uz * uz);
    const float den = fmaxf(r, 1e-12f);
    const float gx = dy[0], gy = dy[1], gz = dy[2];
    du[0] = gx / den, du[1] = gy / den, du[2] = gz / den;
    if (r >= 1e-12f) {
        const float dr = -(((gx * ux + gy * uy) + gz * uz) / (den * den));
        const float f = dr / r;
        du[0] = du[0] + ux * f, du[1] = du[1] + uy * f, du[2] = du[2] + uz * f;
    }
    if (dun) du[0] = du[0] + dun[0], du[1] = du[1] + dun[1], du[2] = du[2] + dun[2];
}

// one thread per point q: -sum over its own k neighbours of du(q, j), then + du(i, j) for every (i, j) of its reverse list, in list order
__global__ __launch_bounds__(256) void dirs_to_xyz_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ idx,
                                                          const int32_t *__restrict__ rptr, const int32_t *__restrict__ rent, int rev_global,
                                                          const float *__restrict__ ddir, const float *__restrict__ dun, int B, int n, int k,
                                                          float *__restrict__ dxyz, int accumulate)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (int64_t)B * n) return;
    const int64_t base = row - row % n;
    const float px = xyz[row * 3], py = xyz[row * 3 + 1], pz = xyz[row * 3 + 2];
    float ax = 0.f, ay = 0.f, az = 0.f, du[3];
    for (int j = 0; j < k; ++j) {
        const int64_t r = base + idx[row * k + j];
        const int64_t e = (row * k + j) * 3;
        xb_norm_bwd(xyz[r * 3] - px, xyz[r * 3 + 1] - py, xyz[r * 3 + 2] - pz, ddir + e, dun ? dun + e : nullptr, du);
        ax = ax - du[0], ay = ay - du[1], az = az - du[2];
    }
    const int e0 = rptr[row], e1 = rptr[row + 1];
    for (int q = e0; q < e1; ++q) {
        const int ent = rent[q];
        int64_t src;
        int j;
        if (rev_global) src = ent / k, j = ent % k;                      // global entry (b * n + i) * k + j
        else src = base + (ent >> 6), j = ent & 63;                      // (i << 6) | j within the object
        const int64_t e = (src * k + j) * 3;
        xb_norm_bwd(px - xyz[src * 3], py - xyz[src * 3 + 1], pz - xyz[src * 3 + 2], ddir + e, dun ? dun + e : nullptr, du);
        ax = ax + du[0], ay = ay + du[1], az = az + du[2];
    }
    if (accumulate) ax = dxyz[row * 3] + ax, ay = dxyz[row * 3 + 1] + ay, az = dxyz[row * 3 + 2] + az;
    dxyz[row * 3] = ax, dxyz[row * 3 + 1] = ay, dxyz[row * 3 + 2] = az;
}

extern "C" int tgp_dirs_to_xyz(const float *xyz, const int32_t *idx, const int32_t *rptr, const int32_t *rent, int rev_global, const float *ddir,
                               const float *dun, int B, int n, int k, float *dxyz, int accumulate, tgp_stream_t stream)
{
    TGP_REQUIRE(xyz && idx && rptr && rent && ddir && dxyz && B > 0 && n > 0 && k > 0);
    if ((!rev_global && k > 64) || (int64_t)B * n * k >= 0x7fffffff) return TGP_EUNSUPPORTED;
    hipLaunchKernelGGL(dirs_to_xyz_kernel, dim3(tgp_cdiv((int64_t)B * n, 256)), dim3(256), 0, tgp_hs(stream), xyz, idx, rptr, rent, rev_global,
                       ddir, dun, B, n, k, dxyz, accumulate);
    return TGP_LAUNCH_RESULT();
}

// one workgroup per object: the sum over its points (strided per thread, then a fixed tree), then every point's row
__global__ __launch_bounds__(256) void center_bwd_kernel(const float *__restrict__ dxyz, const float *__restrict__ dmean, int n,
                                                         float *__restrict__ dpts)
{
    __shared__ float s_sum[3][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const float *d = dxyz + (int64_t)b * n * 3;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = t; i < n; i += 256) sx = sx + d[i * 3], sy = sy + d[i * 3 + 1], sz = sz + d[i * 3 + 2];
    s_sum[0][t] = sx, s_sum[1][t] = sy, s_sum[2][t] = sz;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w)
            for (int c = 0; c < 3; ++c) s_sum[c][t] = s_sum[c][t] + s_sum[c][t + w];
        __syncthreads();
    }
    float add[3];
    for (int c = 0; c < 3; ++c) add[c] = ((dmean ? dmean[b * 3 + c] : 0.f) - s_sum[c][0]) / (float)n;
    float *o = dpts + (int64_t)b * n * 3;
    for (int i = t; i < n; i += 256)
        for (int c = 0; c < 3; ++c) o[i * 3 + c] = d[i * 3 + c] + add[c];
}

extern "C" int tgp_center_bwd(const float *dxyz, const float *dmean, int B, int n, float *dpoints, tgp_stream_t stream)
{
    TGP_REQUIRE(dxyz && dpoints && B > 0 && n > 0);
    hipLaunchKernelGGL(center_bwd_kernel, dim3(B), dim3(256), 0, tgp_hs(stream), dxyz, dmean, n, dpoints);
    return TGP_LAUNCH_RESULT();
}

#define XB_BN_PARTS 64

__device__ __forceinline__ float xb_act_grad(float z, int act, float slope) { return act == 1 ? (z > 0.f ? 1.f : slope) : 1.f; }

// rows split into XB_BN_PARTS fixed shares (blockIdx.y), 64 columns x 4 row lanes per workgroup; each thread sums its rows in order,
// the four lanes are added in lane order, the shares in share order by bn_eval_finish_kernel
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const float *__restrict__ dy, int lddy, const float *__restrict__ x, int ld, int64_t rows,
                                                          int C, const float *__restrict__ mean, const float *__restrict__ var, float eps,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta, int act, float slope,
                                                          float *__restrict__ dx, int lddx, float *__restrict__ part)
{
    __shared__ float s_g[4][64], s_b[4][64];
    const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    float sg = 0.f, sb = 0.f;
    if (c < C) {
        const float mu = mean[c];
        const float inv = 1.0f / sqrtf(var[c] + eps);
        const float a = gamma[c] / sqrtf(var[c] + eps);
        const float bb = beta[c];
        const int64_t per = (rows + XB_BN_PARTS - 1) / XB_BN_PARTS;
        const int64_t r0 = blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
        for (int64_t r = r0 + lane; r < r1; r += 4) {
            const float xv = x[r * ld + c];
            const float z = (xv - mu) * a + bb;              // tgp_bn_apply's expression: the same activation branch
            const float d = dy[r * lddy + c] * xb_act_grad(z, act, slope);
            dx[r * lddx + c] = d * a;
            sg = sg + d * ((xv - mu) * inv);
            sb = sb + d;
        }
    }
    s_g[lane][cl] = sg, s_b[lane][cl] = sb;
    __syncthreads();
    if (lane == 0 && c < C) {
        part[((int64_t)blockIdx.y * 2) * C + c] = ((s_g[0][cl] + s_g[1][cl]) + s_g[2][cl]) + s_g[3][cl];
        part[((int64_t)blockIdx.y * 2 + 1) * C + c] = ((s_b[0][cl] + s_b[1][cl]) + s_b[2][cl]) + s_b[3][cl];
    }
}

__global__ void bn_eval_finish_kernel(const float *__restrict__ part, int parts, int C, float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float g = 0.f, b = 0.f;
    for (int p = 0; p < parts; ++p) g = g + part[(p * 2) * C + c], b = b + part[(p * 2 + 1) * C + c];
    dgamma[c] = g, dbeta[c] = b;
}

extern "C" int64_t tgp_bn_eval_workspace_floats(int C) { return (int64_t)XB_BN_PARTS * 2 * (C > 0 ? C : 0); }

extern "C" int tgp_bn_eval_bwd(const float *dy, int lddy, const float *x, int ld, int64_t rows, int C, const float *mean, const float *var,
                               float eps, const float *gamma, const float *beta, int act, float slope, float *dx, int lddx, float *dgamma,
                               float *dbeta, float *workspace, tgp_stream_t stream)
{
    TGP_REQUIRE(dy && x && mean && var && gamma && beta && dx && dgamma && dbeta && workspace && rows > 0 && C > 0);
    TGP_REQUIRE(lddy >= C && ld >= C && lddx >= C && (act == 0 || act == 1) && eps > 0.f);
    hipLaunchKernelGGL(bn_eval_bwd_kernel, dim3(tgp_cdiv(C, 64), XB_BN_PARTS), dim3(256), 0, tgp_hs(stream), dy, lddy, x, ld, rows, C, mean, var,
                       eps, gamma, beta, act, slope, dx, lddx, workspace);
    hipLaunchKernelGGL(bn_eval_finish_kernel, dim3(tgp_cdiv(C, 256)), dim3(256), 0, tgp_hs(stream), workspace, XB_BN_PARTS, C, dgamma, dbeta);
    return TGP_LAUNCH_RESULT();
}

// one thread per column: the objects in order; dxw (objects, C) = the winners' dx (tgp_colmax_bwd spreads it to the dense rows)
__global__ void bn_eval_bwd_pooled_kernel(const float *__restrict__ dpool, int ldp, const int32_t *__restrict__ arg, int lda,
                                          const float *__restrict__ x, int ld, int objects, int C, const float *__restrict__ mean,
                                          const float *__restrict__ var, float eps, const float *__restrict__ gamma, const float *__restrict__ beta,
                                          int act, float slope, float *__restrict__ dxw, float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float mu = mean[c];
    const float inv = 1.0f / sqrtf(var[c] + eps);
    const float a = gamma[c] / sqrtf(var[c] + eps);
    const float bb = beta[c];
    float sg = 0.f, sb = 0.f;
    for (int o = 0; o < objects; ++o) {
        const int64_t r = arg[(int64_t)o * lda + c];
        const float xv = x[r * ld + c];
        const float z = (xv - mu) * a + bb;
        const float d = dpool[(int64_t)o * ldp + c] * xb_act_grad(z, act, slope);
        dxw[(int64_t)o * C + c] = d * a;
        sg = sg + d * ((xv - mu) * inv);
        sb = sb + d;
    }
    dgamma[c] = sg, dbeta[c] = sb;
}

extern "C" int tgp_bn_eval_bwd_pooled(const float *dpool, int ldp, const int32_t *argrow, int lda, const float *x, int ld, int objects, int rows_per_obj,
                                      int C, const float *mean, const float *var, float eps, const float *gamma, const float *beta, int act, float slope,
                                      float *dx, int lddx, float *dgamma, float *dbeta, float *workspace, tgp_stream_t stream)
{
    TGP_REQUIRE(dpool && argrow && x && mean && var && gamma && beta && dx && dgamma && dbeta && workspace && objects > 0 && rows_per_obj > 0);
    TGP_REQUIRE(C > 0 && ldp >= C && lda >= C && ld >= C && lddx >= C && (act == 0 || act == 1) && eps > 0.f);
    hipLaunchKernelGGL(bn_eval_bwd_pooled_kernel, dim3(tgp_cdiv(C, 256)), dim3(256), 0, tgp_hs(stream), dpool, ldp, argrow, lda, x, ld, objects, C,
                       mean, var, eps, gamma, beta, act, slope, workspace, dgamma, dbeta);
    const int rc = TGP_LAUNCH_RESULT();
    if (rc) return rc;
    return tgp_colmax_bwd(workspace, C, argrow, lda, objects, rows_per_obj, C, dx, lddx, stream);
}
