// Models from depth sequences: TSDF fusion of posed depth frames and marching-tetrahedra meshing (include/tgpose.h, DESIGN.md
// section 3 "Models from depth sequences"; tests/tsdf_ref.py restates both in NumPy, bit for bit).
//
//   tsdf_integrate_kernel   one workgroup per 8 x 8 x 8 brick of one volume, two voxels a lane (ix and ix + 4: a wave's lanes run
//                           along iz, then iy, so neighbouring lanes gather neighbouring pixels).  The workgroup walks all J jobs:
//                           the job's volume, frame, twelve pose floats and four intrinsics are wave-uniform loads, a job of
//                           another volume costs one compare, and a job whose projected brick (centre and radius, with slack)
//                           misses the frame is skipped whole.  The brick's sums and counts stay in registers and are added to
//                           memory once: no atomics, and a call touches the volume's memory once however many frames go in.
//   tsdf_count_kernel       one thread per voxel = per cube at that corner: the cube's triangle count
//   tsdf_emit_kernel        one thread per cube: its triangles at the cube's offset in the soup
//
// Integer sums and fixed places: two calls give identical bytes.
#include "tgp_common.h"

// the cube corner (dx << 2 | dy << 1 | dz) of path corner c of tetrahedron k: the axis steps of the k-th permutation of (0, 1, 2)
__device__ static const uint8_t tsdf_path[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
// bit `case` of word k: the triangles swap their second and third vertex (derived by tests/tsdf_ref.py derive_flip; the word of an
// odd permutation is the complement of an even one's over the cases 1..14)
__device__ static const uint16_t tsdf_flip[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
#include "tsdf_cells.h"

#define TSDF_THREADS 256

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(const tgp_tsdf_integrate_args a, int bricks)
{
    const int tid = threadIdx.x;
    if (blockIdx.x == 0)
        for (int j = tid; j < a.J; j += TSDF_THREADS) {
            const int img = a.job_img[j], mdl = a.job_model[j];
            a.status[j] = (img < 0 || img >= a.S || mdl < 0 || mdl >= a.M) ? 1 : 0;
        }
    const int G = a.G;
    const int per = bricks * bricks * bricks;
    const int m = blockIdx.x / per, b = blockIdx.x % per; // m < M: the grid is M * per
    const int bx = b / (bricks * bricks), by = (b / bricks) % bricks, bz = b % bricks;
    const float *meta = a.meta + (size_t)m * 4;
    const float cx = meta[0], cy = meta[1], cz = meta[2], voxel = meta[3];
    const int ix = bx * 8 + (tid >> 6), iy = by * 8 + ((tid >> 3) & 7), iz = bz * 8 + (tid & 7);
    const float x0 = tsdf_centre(cx, ix, G, voxel), x1 = tsdf_centre(cx, ix + 4, G, voxel);
    const float y = tsdf_centre(cy, iy, G, voxel), z = tsdf_centre(cz, iz, G, voxel);
    // the brick's centre and a radius that holds its voxel centres (3.5 sqrt(3) voxels) with room for every rounding below
    const float qx = cx + (float)(bx * 8 + 4 - G / 2) * voxel, qy = cy + (float)(by * 8 + 4 - G / 2) * voxel,
                qz = cz + (float)(bz * 8 + 4 - G / 2) * voxel;
    const float rad = 7.f * fabsf(voxel);
    const float near = a.near, trunc = a.trunc, inv = a.inv;
    const float wlast = (float)(a.W - 1), hlast = (float)(a.H - 1);
    const int W = a.W;
    const size_t plane = (size_t)a.H * a.W;

    int s0 = 0, s1 = 0, w0 = 0, w1 = 0;
    for (int j = 0; j < a.J; ++j) {
        if (a.job_model[j] != m) continue; // wave-uniform, as is every continue of this loop
        const int img = a.job_img[j];
        if (img < 0 || img >= a.S) continue;
        const float *T = a.job_pose + (size_t)j * 12;
        const float *K = a.camk + (size_t)img * 4;
        const float T0 = T[0], T1 = T[1], T2 = T[2], T3 = T[3], T4 = T[4], T5 = T[5], T6 = T[6], T7 = T[7], T8 = T[8], T9 = T[9],
                    T10 = T[10], T11 = T[11];
        const float K0 = K[0], K1 = K[1], K2 = K[2], K3 = K[3];
        {
            // every voxel centre of the brick lies within r of the posed brick centre (the Frobenius norm bounds the linear
            // part).  If the brick is wholly in front of near, its pixels lie between the bounds below: a miss by more than a pixel
            // skips the job.  A NaN anywhere makes a comparison false and the job is walked (its voxels then skip themselves).
            const float pcx = ((T0 * qx + T1 * qy) + T2 * qz) + T3, pcy = ((T4 * qx + T5 * qy) + T6 * qz) + T7,
                        pcz = ((T8 * qx + T9 * qy) + T10 * qz) + T11;
            const float r = rad * sqrtf(T0 * T0 + T1 * T1 + T2 * T2 + T4 * T4 + T5 * T5 + T6 * T6 + T8 * T8 + T9 * T9 + T10 * T10);
            const float zmin = pcz - r, zmax = pcz + r;
            if (zmin > near) {
                const float xh = pcx + r, xl = pcx - r, yh = pcy + r, yl = pcy - r;
                const float ua = K0 * (xl / (xl < 0.f ? zmin : zmax)) + K2, ub = K0 * (xh / (xh > 0.f ? zmin : zmax)) + K2;
                const float va = K1 * (yl / (yl < 0.f ? zmin : zmax)) + K3, vb = K1 * (yh / (yh > 0.f ? zmin : zmax)) + K3;
                const bool finite = fabsf(ua) < 1e30f && fabsf(ub) < 1e30f && fabsf(va) < 1e30f && fabsf(vb) < 1e30f; // false for a NaN
                if (finite && (fmaxf(ua, ub) < -2.f || fminf(ua, ub) > wlast + 2.f || fmaxf(va, vb) < -2.f || fminf(va, vb) > hlast + 2.f))
                    continue;
            }
        }
        const uint16_t *frame = a.depth + (size_t)img * plane;
        const uint8_t *mframe = a.mask ? a.mask + (size_t)img * plane : nullptr;
        const int mval = a.mask ? a.job_mask_val[j] : 0;
        auto visit = [&](float x, int &s, int &w) {
            const float px = ((T0 * x + T1 * y) + T2 * z) + T3;
            const float py = ((T4 * x + T5 * y) + T6 * z) + T7;
            const float pz = ((T8 * x + T9 * y) + T10 * z) + T11;
            if (!(pz > near)) return; // a NaN too
            const float u = K0 * (px / pz) + K2, v = K1 * (py / pz) + K3;
            const float ru = rintf(u), rv = rintf(v);
            if (!(ru >= 0.f && ru <= wlast && rv >= 0.f && rv <= hlast)) return; // a NaN too
            const size_t o = (size_t)(int)rv * W + (int)ru;
            const int d = frame[o];
            if (d == 0) return;
            if (mframe && mframe[o] != mval) return;
            const float sdf = (float)d - pz * 1000.f;
            if (sdf < -trunc) return;
            s += (int)rintf(fminf(sdf, trunc) * inv);
            w += 1;
        };
        visit(x0, s0, w0);
        visit(x1, s1, w1);
    }
    const size_t o0 = (((size_t)m * G + ix) * G + iy) * G + iz, o1 = o0 + (size_t)4 * G * G;
    if (w0) {
        a.sum[o0] += s0;
        a.weight[o0] += w0;
    }
    if (w1) {
        a.sum[o1] += s1;
        a.weight[o1] += w1;
    }
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------------------
// the cubes, the cases and the vertex arithmetic are tsdf_cells.h's, shared with weld.hip
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_count_kernel(const tgp_tsdf_mesh_args a)
{
    const int G = a.G;
    const size_t v = (size_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (v >= (size_t)G * G * G) return;
    const int iz = (int)(v % G), iy = (int)(v / G % G), ix = (int)(v / G / G);
    TsdfCube c;
    int n = 0;
    if (tsdf_cube(a, ix, iy, iz, c)) {
#pragma unroll
        for (int k = 0; k < 6; ++k) n += tsdf_case_faces(tsdf_case(c, k));
    }
    a.counts[v] = n;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_emit_kernel(const tgp_tsdf_mesh_args a)
{
    const int G = a.G;
    const size_t cells = (size_t)G * G * G;
    const size_t v = (size_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (v >= cells) return;
    if (v == cells - 1) {
        const long long total = a.offsets[v];
        a.info[0] = total < a.face_cap ? total : a.face_cap;
        a.info[1] = total > a.face_cap ? 1 : 0;
    }
    const int mine = a.counts[v];
    if (mine == 0) return;
    long long n = a.offsets[v] - mine; // the cube's first triangle in the soup
    if (n >= a.face_cap) return;
    const int iz = (int)(v % G), iy = (int)(v / G % G), ix = (int)(v / G / G);
    TsdfCube c;
    if (!tsdf_cube(a, ix, iy, iz, c)) return; // not with counts[v] > 0
    const float *meta = a.meta + (size_t)a.model * 4;
    for (int k = 0; k < 6; ++k) {
        const int cs = tsdf_case(c, k);
        const int faces = tsdf_case_faces(cs);
        if (faces == 0) continue;
        int ea[4], eb[4]; // the cut edges (path corners) in the order the contract lists them
        tsdf_case_edges(cs, ea, eb);
        const bool flip = tsdf_flip[k] >> cs & 1;
        for (int t = 0; t < faces; ++t, ++n) {
            if (n >= a.face_cap) return;
            float *dst = a.verts + (size_t)n * 9;
            for (int q = 0; q < 3; ++q) {
                const int e = tsdf_face_edge(t, q, flip);
                const int p0 = ea[e], p1 = eb[e];
                const int ka = tsdf_path[k][p0 < p1 ? p0 : p1], kb = tsdf_path[k][p0 < p1 ? p1 : p0]; // from the end earlier in the path
                tsdf_edge_vertex(meta, G, c.s[ka], c.w[ka], c.s[kb], c.w[kb], ix + (ka >> 2), iy + ((ka >> 1) & 1), iz + (ka & 1),
                                 ix + (kb >> 2), iy + ((kb >> 1) & 1), iz + (kb & 1), dst + q * 3);
            }
        }
    }
}

static bool tsdf_grid_ok(int G) { return G >= TGP_TSDF_MIN_G && G <= TGP_TSDF_MAX_G && G % 8 == 0; }

extern "C" int tgp_tsdf_integrate(const tgp_tsdf_integrate_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_tsdf_integrate_args &a = *args;
    TGP_REQUIRE(a.depth && a.camk && a.sum && a.weight && a.meta);
    TGP_REQUIRE(a.S > 0 && a.H > 0 && a.W > 0 && a.M > 0 && a.J >= 0);
    TGP_REQUIRE(a.trunc > 0.f && a.trunc < __builtin_inff() && a.inv > 0.f && a.inv < __builtin_inff());
    TGP_REQUIRE(a.near > 0.f && a.near < __builtin_inff());
    TGP_REQUIRE(!a.mask || a.job_mask_val);
    if (a.J > 0) TGP_REQUIRE(a.job_img && a.job_model && a.job_pose && a.status);
    if (!tsdf_grid_ok(a.G) || a.J > TGP_TSDF_MAX_JOBS || a.H > 16384 || a.W > 16384) return TGP_EUNSUPPORTED;
    const int bricks = a.G / 8;
    const int64_t grid = (int64_t)a.M * bricks * bricks * bricks;
    if (grid > 0x7fffffff) return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)grid), dim3(TSDF_THREADS), 0, tgp_hs(stream), a, bricks);
    return TGP_LAUNCH_RESULT();
}

static int tsdf_mesh_check(const tgp_tsdf_mesh_args *args, bool emit)
{
    TGP_REQUIRE(args);
    const tgp_tsdf_mesh_args &a = *args;
    TGP_REQUIRE(a.sum && a.weight && a.meta && a.counts);
    TGP_REQUIRE(a.M > 0 && a.model >= 0 && a.model < a.M && a.min_weight >= 1);
    if (emit) TGP_REQUIRE(a.offsets && a.info && a.face_cap >= 0 && (a.verts || a.face_cap == 0));
    if (!tsdf_grid_ok(a.G) || (emit && a.face_cap > TGP_TSDF_MAX_FACES)) return TGP_EUNSUPPORTED;
    return 0;
}

extern "C" int tgp_tsdf_mesh_count(const tgp_tsdf_mesh_args *args, tgp_stream_t stream)
{
    const int rc = tsdf_mesh_check(args, false);
    if (rc) return rc;
    const int64_t cells = (int64_t)args->G * args->G * args->G;
    hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)tgp_cdiv(cells, TSDF_THREADS)), dim3(TSDF_THREADS), 0, tgp_hs(stream), *args);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_tsdf_mesh_emit(const tgp_tsdf_mesh_args *args, tgp_stream_t stream)
{
    const int rc = tsdf_mesh_check(args, true);
    if (rc) return rc;
    const int64_t cells = (int64_t)args->G * args->G * args->G;
    hipLaunchKernelGGL(tsdf_emit_kernel, dim3((unsigned)tgp_cdiv(cells, TSDF_THREADS)), dim3(TSDF_THREADS), 0, tgp_hs(stream), *args);
    return TGP_LAUNCH_RESULT();
}
