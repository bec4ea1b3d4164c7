// Ball crop of a depth frame (or of a point list) around a pose: the reference's crop_ball_from_depth_image / crop_ball_from_pts
// (network/point_sample/pc_sample_sphere.py:258-280, 350-371) for J jobs in one launch, without the host in the loop.  The reference
// backprojects the whole frame, takes nonzero() of the valid pixels, and tests `distance <= radius` up to ten times with the
// radius growing by 1.10 until ten points are inside.  Here one 1024-thread workgroup per job makes two passes:
//
//   pass 1  the whole frame: the count of valid pixels (counts[0]; the reference's len(raw_pts), which the frame-wide states
//           "nothing within the last radius" and "no valid pixel" need), and for the pixels inside the job's rectangle the ten
//           cumulative counts #{d <= ladder[i]} at once -- the ten tests of the reference's loop in one read of the frame.
//           From them the level L (the first whose count reaches 10, else 9).
//   pass 2  the rectangle only: the pixels with d <= ladder[L], compacted in row-major order (the order of nonzero()) by a
//           wave prefix sum and a 16-entry LDS table per round, one barrier per round.
//
// The rectangle bounds the pixels whose point can lie within ladder[9] of the centre (ball_rect); outside it no distance is
// evaluated, and pass 2 does not read.  Depth is read 16 bytes (8 pixels) per lane where the rows are 16-byte aligned (W a multiple
// of 8 and an aligned base), else 2 bytes per lane; the rectangle's columns are widened to whole 16-byte groups, which cannot change
// the result.  What is written is the pixel index per kept pixel; tgp_ball_select / tgp_ball_sample re-read the depth of the
// few selected pixels and materialise only those points, with the arithmetic of the ROI path (pixel_point.h).
//
// No float atomics, no inter-workgroup traffic: a job's result depends on its own arguments alone and is bit-repeatable.
#include "pixel_point.h"

#define BALL_THREADS TGP_BALL_THREADS
#define BALL_WAVES (BALL_THREADS / TGP_WAVE)
#define BALL_LEVELS TGP_BALL_LEVELS

struct BallArgs {
    const uint16_t *depth;      // (I,H,W)                     | point list: NULL
    const float *pts;           // NULL                        | (I,W,3), H = 1
    const uint8_t *masks;       // or NULL: no mask
    const int64_t *mask_off;
    const int *mask_stride, *mask_val, *job_img;
    const float *centers, *ladder, *camk;
    int I, H, W, cap, full_scan;
    uint32_t *recs;
    int *counts;
};

struct BallRect {
    int x0, x1, y0, y1;
};

// The pixels whose point can be within R of the centre c: a point p of pixel (u, v) has u = cx + fx p_x / p_z, and over the box
// |p - c|_inf <= Rm with p_z > 0 the ratio p_x / p_z is monotone in each variable, so its extremes are at the corners.  Rm widens R
// by far more than the rounding of the float32 point and distance (relative 1e-6), and a pixel is added on each side.  Whatever the
// formula cannot bound -- a non-finite or negative argument, a ball that reaches z <= 0 -- scans the whole frame.
__device__ __forceinline__ BallRect ball_rect(float c0, float c1, float c2, float R, float fx, float fy, float pcx, float pcy, int H, int W,
                                              bool full)
{
    BallRect r = {0, W, 0, H};
    if (full) return r;
    const double Rm = (double)R * 1.001 + 1e-5, z0 = (double)c2 - Rm, z1 = (double)c2 + Rm;
    if (!(R >= 0.f) || !isfinite(Rm) || !isfinite(c0) || !isfinite(c1) || !isfinite(c2) || !(z0 > 1e-6)) return r;
    if (!isfinite(fx) || !isfinite(fy) || !isfinite(pcx) || !isfinite(pcy)) return r;
    auto span = [&](double c, double f, double pc, int n, int &lo, int &hi) {
        const double a = c - Rm, b = c + Rm;
        const double q0 = a / z0, q1 = a / z1, q2 = b / z0, q3 = b / z1;
        const double qmin = fmin(fmin(q0, q1), fmin(q2, q3)), qmax = fmax(fmax(q0, q1), fmax(q2, q3));
        const double u0 = pc + f * qmin, u1 = pc + f * qmax;
        const double ulo = floor(fmin(u0, u1) - 1.0), uhi = ceil(fmax(u0, u1) + 1.0);
        if (!isfinite(ulo) || !isfinite(uhi)) {
            lo = 0, hi = n;
            return;
        }
        lo = (int)fmin(fmax(ulo, 0.0), (double)n);
        hi = (int)fmin(fmax(uhi + 1.0, 0.0), (double)n);
        if (hi < lo) hi = lo;
    };
    span(c0, fx, pcx, W, r.x0, r.x1);
    span(c1, fy, pcy, H, r.y0, r.y1);
    return r;
}

// PTS: the elements are the points of list job_img[j] (H = 1, W = N, every point valid, no rectangle).  VEC: elements per lane and
// load (8: one 16-byte depth load; 1: plain loads).
template <bool PTS, int VEC>
__global__ __launch_bounds__(BALL_THREADS) void ball_cloud_kernel(const BallArgs a)
{
    __shared__ int red[BALL_LEVELS + 1][BALL_WAVES];
    __shared__ int tot[2][BALL_WAVES];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & (TGP_WAVE - 1), wave = tid / TGP_WAVE;
    const int H = a.H, W = a.W, cap = a.cap;
    int *cnt = a.counts + (size_t)j * 4;
    const int img = a.job_img[j];
    if (img < 0 || img >= a.I) {        // a job that names no frame: reported, nothing read
        if (tid == 0) cnt[0] = 0, cnt[1] = 0, cnt[2] = BALL_LEVELS - 1, cnt[3] = 3;
        return;
    }
    const float c0 = a.centers[j * 3], c1 = a.centers[j * 3 + 1], c2 = a.centers[j * 3 + 2];
    // lad[i] = max(ladder[0..i]): d <= lad[i]  <=>  the point's level (the smallest i with d <= ladder[i]) is <= i
    float lad[BALL_LEVELS];
#pragma unroll
    for (int i = 0; i < BALL_LEVELS; ++i) {
        const float v = a.ladder[j * BALL_LEVELS + i];
        lad[i] = i ? fmaxf(lad[i - 1], v) : v;
    }
    const float fx = PTS ? 1.f : a.camk[img * 4], fy = PTS ? 1.f : a.camk[img * 4 + 1];
    const float pcx = PTS ? 0.f : a.camk[img * 4 + 2], pcy = PTS ? 0.f : a.camk[img * 4 + 3];
    const UniformDiv div_fx(fx), div_fy(fy), div_k(1000.0f);
    const uint16_t *dimg = PTS ? nullptr : a.depth + (size_t)img * H * W;
    const float *plist = PTS ? a.pts + (size_t)img * W * 3 : nullptr;
    const bool masked = !PTS && a.masks != nullptr;
    const uint8_t *mimg = masked ? a.masks + a.mask_off[j] : nullptr;
    const int mstride = masked ? a.mask_stride[j] : 0;
    const int mval = masked && a.mask_val ? a.mask_val[j] : 0;     // 0: any non-zero byte; v > 0: the byte equals v
    BallRect rc = ball_rect(c0, c1, c2, lad[BALL_LEVELS - 1], fx, fy, pcx, pcy, H, W, PTS || a.full_scan != 0);
    if (VEC > 1) rc.x0 &= ~(VEC - 1), rc.x1 = min(W, (rc.x1 + VEC - 1) & ~(VEC - 1));       // whole load groups (W is a multiple of VEC)

    // the VEC elements that start at flat index p0 = y * W + x: dep[i] > 0 marks a valid one
    auto load = [&](int p0, int (&dep)[VEC]) {
        if constexpr (PTS) {
            dep[0] = 1;
        } else {
            if constexpr (VEC == 8) {
                const uint4 v = *reinterpret_cast<const uint4 *>(dimg + p0);
                dep[0] = v.x & 0xffff, dep[1] = v.x >> 16, dep[2] = v.y & 0xffff, dep[3] = v.y >> 16;
                dep[4] = v.z & 0xffff, dep[5] = v.z >> 16, dep[6] = v.w & 0xffff, dep[7] = v.w >> 16;
            } else {
                dep[0] = dimg[p0];
            }
            if (masked) {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (dep[i] > 0) {
                        const int m = mimg[(size_t)(p0 + i) * mstride];
                        if (!(mval ? m == mval : m != 0)) dep[i] = 0;
                    }
            }
        }
    };
    // d = sqrt((dx^2 + dy^2) + dz^2) of element (x, y) = flat index p, float32, every operation rounded on its own
    auto dist = [&](int x, int y, int p, int dep) {
        float px, py, pz;
        if constexpr (PTS) {
            px = plist[(size_t)p * 3], py = plist[(size_t)p * 3 + 1], pz = plist[(size_t)p * 3 + 2];
        } else {
            tgp_pixel_point(x, y, (float)dep, pcx, pcy, div_fx, div_fy, div_k, px, py, pz);
        }
        const float d0 = px - c0, d1 = py - c1, d2 = pz - c2;
        // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the latter is the bare 1-ulp v_sqrt_f32; sqrtf compiles to the
        // root plus its fused fix-up step, which is correctly rounded (no fast-math in this library)
        return sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    };

    // ---- pass 1: valid elements of the frame; cumulative level counts inside the rectangle
    int nvalid = 0, cum[BALL_LEVELS];
#pragma unroll
    for (int i = 0; i < BALL_LEVELS; ++i) cum[i] = 0;
    const int frame_groups = H * W / VEC;       // H * W < 2^24 (point list: < 2^30)
    for (int g = tid; g < frame_groups; g += BALL_THREADS) {
        const int p0 = g * VEC, y = PTS ? 0 : p0 / W, x = p0 - y * W;
        int dep[VEC];
        load(p0, dep);
        const bool rowin = y >= rc.y0 && y < rc.y1;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            nvalid += dep[i] > 0;
            if (dep[i] > 0 && rowin && x + i >= rc.x0 && x + i < rc.x1) {
                const float d = dist(x + i, y, p0 + i, dep[i]);
#pragma unroll
                for (int l = 0; l < BALL_LEVELS; ++l) cum[l] += d <= lad[l];
            }
        }
    }
#pragma unroll
    for (int o = TGP_WAVE / 2; o > 0; o >>= 1) {
        nvalid += __shfl_xor(nvalid, o);
#pragma unroll
        for (int l = 0; l < BALL_LEVELS; ++l) cum[l] += __shfl_xor(cum[l], o);
    }
    if (lane == 0) {
        red[BALL_LEVELS][wave] = nvalid;
#pragma unroll
        for (int l = 0; l < BALL_LEVELS; ++l) red[l][wave] = cum[l];
    }
    __syncthreads();
    nvalid = 0;
#pragma unroll
    for (int l = 0; l < BALL_LEVELS; ++l) cum[l] = 0;
    for (int w = 0; w < BALL_WAVES; ++w) {
        nvalid += red[BALL_LEVELS][w];
#pragma unroll
        for (int l = 0; l < BALL_LEVELS; ++l) cum[l] += red[l][w];
    }
    int L = BALL_LEVELS - 1;
    float rad = lad[BALL_LEVELS - 1];
    int count = cum[BALL_LEVELS - 1];
#pragma unroll
    for (int l = BALL_LEVELS - 2; l >= 0; --l)
        if (cum[l] >= 10) L = l, rad = lad[l], count = cum[l];
    if (tid == 0) cnt[0] = nvalid, cnt[1] = count, cnt[2] = L, cnt[3] = nvalid == 0 ? 2 : count == 0 ? 1 : 0;
    if (count == 0) return;

    // ---- pass 2: the elements of the rectangle with d <= ladder[L], in row-major order
    uint32_t *rec = a.recs + (size_t)j * cap;
    const int gpr = (rc.x1 - rc.x0) / VEC;              // load groups per rectangle row (> 0: count > 0)
    const int groups = gpr * (rc.y1 - rc.y0);
    int base = 0;
    for (int r = 0; r * BALL_THREADS < groups; ++r) {
        const int g = r * BALL_THREADS + tid;
        unsigned bits = 0;
        int p0 = 0;
        if (g < groups) {
            const int gy = g / gpr, y = rc.y0 + gy, x = rc.x0 + (g - gy * gpr) * VEC;
            p0 = y * W + x;
            int dep[VEC];
            load(p0, dep);
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (dep[i] > 0 && dist(x + i, y, p0 + i, dep[i]) <= rad) bits |= 1u << i;
        }
        const int n = __popc(bits);
        int incl = n;
#pragma unroll
        for (int o = 1; o < TGP_WAVE; o <<= 1) {
            const int up = __shfl_up(incl, o);
            incl += lane >= o ? up : 0;
        }
        if (lane == TGP_WAVE - 1) tot[r & 1][wave] = incl;
        __syncthreads();        // one per round: tot is double buffered by the round's parity
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BALL_WAVES; ++w) {
            const int t = tot[r & 1][w];
            before += w < wave ? t : 0;
            total += t;
        }
        int slot = base + before + incl - n;
        base += total;
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (bits >> i & 1u) {
                if (slot < cap) rec[slot] = (uint32_t)(p0 + i);
                ++slot;
            }
    }
}

static bool ball_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int tgp_ball_cloud(const uint16_t *depth, const uint8_t *masks, const int64_t *mask_off, const int *mask_stride,
                              const int *mask_val, const int *job_img, const float *centers, const float *ladder, const float *camk, int J,
                              int I, int H, int W, int cap, int full_scan, uint32_t *recs, int *counts, tgp_stream_t stream)
{
    TGP_REQUIRE(depth && job_img && centers && ladder && camk && recs && counts);
    TGP_REQUIRE(!masks || (mask_off && mask_stride));
    TGP_REQUIRE(J > 0 && I > 0 && H > 0 && W > 0 && H < 32768 && W < 32768 && (int64_t)H * W < (1ll << 24));
    TGP_REQUIRE(cap > 0 && (int64_t)J * cap < (1ll << 40));
    BallArgs a = {depth, nullptr, masks, mask_off, mask_stride, mask_val, job_img, centers, ladder, camk, I, H, W, cap, full_scan, recs, counts};
    if (W % 8 == 0 && ball_aligned16(depth))
        hipLaunchKernelGGL((ball_cloud_kernel<false, 8>), dim3(J), dim3(BALL_THREADS), 0, tgp_hs(stream), a);
    else
        hipLaunchKernelGGL((ball_cloud_kernel<false, 1>), dim3(J), dim3(BALL_THREADS), 0, tgp_hs(stream), a);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_ball_cloud_pts(const float *pts, const int *job_img, const float *centers, const float *ladder, int J, int I, int N,
                                  int cap, uint32_t *recs, int *counts, tgp_stream_t stream)
{
    TGP_REQUIRE(pts && job_img && centers && ladder && recs && counts);
    TGP_REQUIRE(J > 0 && I > 0 && N > 0 && N <= (1 << 30) - BALL_THREADS && cap > 0 && (int64_t)J * cap < (1ll << 40));
    BallArgs a = {nullptr, pts, nullptr, nullptr, nullptr, nullptr, job_img, centers, ladder, nullptr, I, 1, N, cap, 1, recs, counts};
    hipLaunchKernelGGL((ball_cloud_kernel<true, 1>), dim3(J), dim3(BALL_THREADS), 0, tgp_hs(stream), a);
    return TGP_LAUNCH_RESULT();
}

// out[j][i] = point(recs[j][e mod count_j]), pix[j][i] = that record, with e = sel[j][i] (SAMPLE: element i of the keyed permutation
// of the doubled list) and the doubled list's length = count_j * 2^m, the first such >= n_pts.
template <bool SAMPLE>
__global__ void ball_select_kernel(const uint32_t *__restrict__ recs, const int *__restrict__ counts, const int *__restrict__ sel,
                                   const int *__restrict__ job_img, const uint16_t *__restrict__ depth, const float *__restrict__ camk,
                                   const float *__restrict__ pts, int64_t total_out, int I, int H, int W, int cap, int n_pts, uint64_t seed,
                                   float *__restrict__ out, int *__restrict__ pix)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total_out) return;
    const int j = (int)(t / n_pts), i = (int)(t - (int64_t)j * n_pts);
    const int n = min(counts[j * 4 + 1], cap), img = job_img[j];
    float x = NAN, y = NAN, z = NAN;
    int src = -1;
    if (n > 0 && img >= 0 && img < I && (!SAMPLE || counts[j * 4 + 3] == 0)) {
        uint32_t dlen = (uint32_t)n;            // n, n_pts <= 2^29: dlen <= 2^30
        while (dlen < (uint32_t)n_pts) dlen <<= 1;
        uint32_t e;
        bool ok = true;
        if constexpr (SAMPLE) {
            int half_bits = 1;
            while ((1u << (2 * half_bits)) < dlen) ++half_bits;
            const uint32_t key = tgp_sample_key(seed, j);
            e = feistel((uint32_t)i, half_bits, key);
            while (e >= dlen) e = feistel(e, half_bits, key);       // a bijection of [0, 2^2h) >= [0, dlen): the walk returns
        } else {
            const int s = sel[t];
            ok = s >= 0 && (uint32_t)s < dlen;
            e = (uint32_t)s;
        }
        if (ok) {
            const uint32_t p = recs[(size_t)j * cap + e % (uint32_t)n];
            if (p < (uint32_t)(H * W)) {        // a record the crop did not write names no pixel
                src = (int)p;
                if (pts) {
                    const float *q = pts + ((size_t)img * W + p) * 3;
                    x = q[0], y = q[1], z = q[2];
                } else {
                    const int py = (int)p / W, px = (int)p - py * W;
                    const float dep = (float)depth[(size_t)img * H * W + p];
                    tgp_pixel_point(px, py, dep, camk[img * 4 + 2], camk[img * 4 + 3], UniformDiv(camk[img * 4]), UniformDiv(camk[img * 4 + 1]),
                                    UniformDiv(1000.0f), x, y, z);
                }
            }
        }
    }
    out[t * 3] = x, out[t * 3 + 1] = y, out[t * 3 + 2] = z;
    pix[t] = src;
}

static int ball_select_launch(bool sample, const uint32_t *recs, const int *counts, const int32_t *sel, const int *job_img,
                              const uint16_t *depth, const float *camk, const float *pts, int J, int I, int H, int W, int cap, int n_pts,
                              uint64_t seed, float *out, int32_t *pix, tgp_stream_t stream)
{
    TGP_REQUIRE(recs && counts && job_img && out && pix && (sample || sel));
    TGP_REQUIRE((pts != nullptr) != (depth != nullptr) && (pts || camk));
    TGP_REQUIRE(J > 0 && I > 0 && H > 0 && W > 0 && (int64_t)H * W <= (1ll << 30) && (pts ? H == 1 : (int64_t)H * W < (1ll << 24)));
    // the doubled list is shorter than 2 max(cap, n_pts) <= 2^30: the Feistel domain 4^h fits 32 bits and its shifts stay below 32
    TGP_REQUIRE(cap > 0 && cap <= (1 << 29) && n_pts > 0 && n_pts <= (1 << 29) && (int64_t)J * n_pts < (1ll << 40));
    const int64_t total = (int64_t)J * n_pts;
    if (sample)
        hipLaunchKernelGGL(ball_select_kernel<true>, dim3(tgp_cdiv(total, 256)), dim3(256), 0, tgp_hs(stream), recs, counts, sel, job_img, depth,
                           camk, pts, total, I, H, W, cap, n_pts, seed, out, pix);
    else
        hipLaunchKernelGGL(ball_select_kernel<false>, dim3(tgp_cdiv(total, 256)), dim3(256), 0, tgp_hs(stream), recs, counts, sel, job_img, depth,
                           camk, pts, total, I, H, W, cap, n_pts, seed, out, pix);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_ball_select(const uint32_t *recs, const int *counts, const int32_t *sel, const int *job_img, const uint16_t *depth,
                               const float *camk, const float *pts, int J, int I, int H, int W, int cap, int n_pts, float *out, int32_t *pix,
                               tgp_stream_t stream)
{
    return ball_select_launch(false, recs, counts, sel, job_img, depth, camk, pts, J, I, H, W, cap, n_pts, 0, out, pix, stream);
}

extern "C" int tgp_ball_sample(const uint32_t *recs, const int *counts, const int *job_img, const uint16_t *depth, const float *camk,
                               const float *pts, int J, int I, int H, int W, int cap, int n_pts, uint64_t seed, float *out, int32_t *pix,
                               tgp_stream_t stream)
{
    return ball_select_launch(true, recs, counts, nullptr, job_img, depth, camk, pts, J, I, H, W, cap, n_pts, seed, out, pix, stream);
}
