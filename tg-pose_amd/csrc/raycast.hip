// Ray casting of TSDF volumes (include/tgpose.h, DESIGN.md section 3 "Ray casting and frame-to-model tracking"; tests/raycast_ref.py
// restates the rule in NumPy, bit for bit).
//
//   tsdf_raycast_kernel   one wave per 8 x 8 patch of one job's rays, four patches a workgroup: neighbouring lanes walk neighbouring
//                         cells.  The job's inverse pose, intrinsics, window and volume meta are indexed by blockIdx.y alone, so
//                         they are scalar loads into SGPRs.  The march is a gather from a volume that sits in L2 (2 MiB of sums and
//                         weights at G = 64): the sixteen loads of a sample are issued together, before any of them is used.
//                         Every ray writes all its outputs; the job's hit count is a wave ballot and one integer atomic per wave.
//
// Nothing but integer atomics on a zeroed word, and fixed places: two calls give identical bytes.
#include "tgp_common.h"

#define RAYCAST_THREADS 256

struct RayCell {
    float f[8]; // corner (dx << 2 | dy << 1 | dz)
};

// the cell of the point g in voxel coordinates: false where the sample is unknown.  t: the fractions in the cell.
__device__ __forceinline__ bool raycast_cell(const int32_t *__restrict__ vsum, const int32_t *__restrict__ vweight, int G, int min_weight,
                                             float gx, float gy, float gz, RayCell &c, float &tx, float &ty, float &tz)
{
    const float hi = (float)G;
    if (!(gx >= -1.f && gx <= hi && gy >= -1.f && gy <= hi && gz >= -1.f && gz <= hi)) return false; // a NaN too
    int ix = (int)floorf(gx), iy = (int)floorf(gy), iz = (int)floorf(gz);
    ix = min(max(ix, 0), G - 2), iy = min(max(iy, 0), G - 2), iz = min(max(iz, 0), G - 2);
    tx = gx - (float)ix, ty = gy - (float)iy, tz = gz - (float)iz;
    const int base = (ix * G + iy) * G + iz; // < G^3 <= 2^24
    int s[8], w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int o = base + ((k >> 2) * G + ((k >> 1) & 1)) * G + (k & 1);
        w[k] = vweight[o];
        s[k] = vsum[o];
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ok = ok && w[k] >= min_weight;
        c.f[k] = (float)s[k] / (float)w[k]; // not used where a weight is 0
    }
    return ok;
}

__device__ __forceinline__ float raycast_lerp(float a, float b, float t) { return a + t * (b - a); }

__global__ __launch_bounds__(RAYCAST_THREADS) void tsdf_raycast_kernel(const tgp_tsdf_raycast_args a, int pw, int patches, int max_samples)
{
    const int j = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int patch = blockIdx.x * (RAYCAST_THREADS / 64) + wave;
    const int mdl = a.job_model[j], img = a.job_img[j];
    const bool job_ok = mdl >= 0 && mdl < a.M && img >= 0 && img < a.S;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[j] = job_ok ? 0 : 1;
    if (patch >= patches) return; // wave-uniform
    const int r = (patch / pw) * 8 + (lane >> 3), c = (patch % pw) * 8 + (lane & 7);
    const bool mine = r < a.h && c < a.w;

    float zs = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    bool hit = false;
    if (job_ok && mine) {
        const int G = a.G, min_weight = a.min_weight;
        const size_t cells = (size_t)G * G * G;
        const int32_t *vsum = a.sum + (size_t)mdl * cells, *vweight = a.weight + (size_t)mdl * cells;
        const float *meta = a.meta + (size_t)mdl * 4, *K = a.camk + (size_t)img * 4, *I = a.job_inv + (size_t)j * 12,
                    *win = a.job_window + (size_t)j * 4;
        const float voxel = meta[3], half = (float)(G / 2) - 0.5f, last = (float)(G - 1);
        const float u = win[0] + (float)c * win[2], v = win[1] + (float)r * win[3];
        const float dx = (u - K[2]) / K[0], dy = (v - K[3]) / K[1];
        float o[3], e[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            e[q] = ((I[q * 4] * dx + I[q * 4 + 1] * dy) + I[q * 4 + 2]) / voxel;
            o[q] = (I[q * 4 + 3] - meta[q]) / voxel + half;
        }
        const float inf = __builtin_inff();
        float zin = a.near, zout = inf;
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (e[q] != 0.f) { // a NaN too: it fails the test below
                const float t0 = (0.f - o[q]) / e[q], t1 = (last - o[q]) / e[q];
                zin = fmaxf(zin, fminf(t0, t1));
                zout = fminf(zout, fmaxf(t0, t1));
                ok = ok && t0 == t0 && t1 == t1; // fmaxf / fminf drop a NaN: name it
            } else
                ok = ok && o[q] >= 0.f && o[q] <= last;
        }
        const float len = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        const float dz = a.step / len;
        ok = ok && len > 0.f && len < inf && dz > 0.f && dz < inf && zin <= zout && zin < inf && zout < inf;
        if (ok) {
            bool have = false;
            float fprev = 0.f;
            RayCell cell;
            float tx, ty, tz;
            for (int k = 0; k < max_samples; ++k) {
                const float zk = zin + (float)k * dz;
                if (!(zk <= zout)) break;
                const float gx = o[0] + zk * e[0], gy = o[1] + zk * e[1], gz = o[2] + zk * e[2];
                if (!raycast_cell(vsum, vweight, G, min_weight, gx, gy, gz, cell, tx, ty, tz)) {
                    have = false;
                    continue;
                }
                const float c00 = raycast_lerp(cell.f[0], cell.f[1], tz), c01 = raycast_lerp(cell.f[2], cell.f[3], tz),
                            c10 = raycast_lerp(cell.f[4], cell.f[5], tz), c11 = raycast_lerp(cell.f[6], cell.f[7], tz);
                const float f = raycast_lerp(raycast_lerp(c00, c01, ty), raycast_lerp(c10, c11, ty), tx);
                if (f > 0.f) {
                    have = true, fprev = f;
                    continue;
                }
                if (have) {
                    hit = true;
                    zs = (zin + (float)(k - 1) * dz) + dz * (fprev / (fprev - f));
                }
                break; // a known f <= 0 ends the ray
            }
            if (hit) {
                const float gx = o[0] + zs * e[0], gy = o[1] + zs * e[1], gz = o[2] + zs * e[2];
                hit = raycast_cell(vsum, vweight, G, min_weight, gx, gy, gz, cell, tx, ty, tz);
                if (hit) {
                    const float c00 = raycast_lerp(cell.f[0], cell.f[1], tz), c01 = raycast_lerp(cell.f[2], cell.f[3], tz),
                                c10 = raycast_lerp(cell.f[4], cell.f[5], tz), c11 = raycast_lerp(cell.f[6], cell.f[7], tz);
                    const float c0 = raycast_lerp(c00, c01, ty), c1 = raycast_lerp(c10, c11, ty);
                    const float gnx = c1 - c0;
                    const float gny = raycast_lerp(c01 - c00, c11 - c10, tx);
                    const float r00 = cell.f[1] - cell.f[0], r01 = cell.f[3] - cell.f[2], r10 = cell.f[5] - cell.f[4], r11 = cell.f[7] - cell.f[6];
                    const float gnz = raycast_lerp(raycast_lerp(r00, r01, ty), raycast_lerp(r10, r11, ty), tx);
                    const float s = sqrtf((gnx * gnx + gny * gny) + gnz * gnz);
                    hit = s > 0.f && s < inf;
                    if (hit) {
                        nx = gnx / s, ny = gny / s, nz = gnz / s;
                        const float mid = (float)(G / 2);
                        vx = meta[0] + ((gx + 0.5f) - mid) * voxel;
                        vy = meta[1] + ((gy + 0.5f) - mid) * voxel;
                        vz = meta[2] + ((gz + 0.5f) - mid) * voxel;
                    }
                }
            }
        }
        if (!hit) zs = 0.f;
    }
    if (mine) {
        const size_t ray = ((size_t)j * a.h + r) * a.w + c;
        const float mm = rintf(zs * 1000.f);
        a.z[ray] = zs;
        a.depth[ray] = (uint16_t)(hit && mm <= 65535.f ? (int)mm : 0);
        a.vertex[ray * 3] = vx, a.vertex[ray * 3 + 1] = vy, a.vertex[ray * 3 + 2] = vz;
        a.normal[ray * 3] = nx, a.normal[ray * 3 + 1] = ny, a.normal[ray * 3 + 2] = nz;
    }
    const unsigned long long hits = __ballot(hit);
    if (lane == 0 && hits) atomicAdd(a.count + j, __popcll(hits));
}

extern "C" int tgp_tsdf_raycast(const tgp_tsdf_raycast_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_tsdf_raycast_args &a = *args;
    TGP_REQUIRE(a.sum && a.weight && a.meta && a.camk);
    TGP_REQUIRE(a.S > 0 && a.M > 0 && a.J >= 0 && a.h >= 1 && a.w >= 1 && a.min_weight >= 1);
    TGP_REQUIRE(a.step > 0.f && a.step < __builtin_inff() && a.near > 0.f && a.near < __builtin_inff());
    if (a.J > 0)
        TGP_REQUIRE(a.job_img && a.job_model && a.job_inv && a.job_window && a.z && a.depth && a.vertex && a.normal && a.count && a.status);
    if (a.G < TGP_TSDF_MIN_G || a.G > TGP_TSDF_MAX_G || a.G % 8 != 0 || a.J > TGP_TSDF_MAX_JOBS || a.h > TGP_RAYCAST_MAX_SIDE ||
        a.w > TGP_RAYCAST_MAX_SIDE || a.step < 0.0625f)
        return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    const int pw = tgp_cdiv(a.w, 8), ph = tgp_cdiv(a.h, 8); // at most 2048 each
    const int patches = pw * ph;
    const int max_samples = (int)ceil(1.7320508075688772 * (double)(a.G - 1) / (double)a.step) + 2;
    hipError_t e = hipMemsetAsync(a.count, 0, (size_t)a.J * sizeof(int32_t), tgp_hs(stream));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(tsdf_raycast_kernel, dim3((unsigned)tgp_cdiv(patches, RAYCAST_THREADS / 64), (unsigned)a.J), dim3(RAYCAST_THREADS), 0,
                       tgp_hs(stream), a, pw, patches, max_samples);
    return TGP_LAUNCH_RESULT();
}
