// BOP pose errors, two-pose VSD: J jobs (frame, mesh, estimated pose, ground-truth pose) per call (include/tgpose.h, DESIGN.md
// section 3 "BOP pose errors"; tests/bop_ref.py restates the contract in NumPy on tests/render_ref.py).  Each of a job's two surfaces
// is the depth renderer's for a scene of that one instance: the vertex, box, coverage, z and winner arithmetic is raster.h's, as in
// csrc/verify.hip, whose launch shape this follows with 2 J pseudo-jobs q = 2 j + (0: estimate, 1: ground truth).  No frame is written.
//
//   vsd_vertex_kernel   one thread per (pseudo-job, vertex): pose, project, snap -> {X, Y, 1/z, flag}; zeroes counts and within
//   vsd_box_kernel      one thread per (pseudo-job, face): the drop rules and the pixel box; per workgroup one integer min / max into
//                       the pseudo-job's box and one add into the job's dropped_gt / dropped_est
//   vsd_tile_kernel     grid (J, T): workgroup (j, k) takes the 16 x 16 tiles k, k + T, ... of the UNION of job j's two boxes.  One
//                       pixel per lane; the estimate's triangle list and then the ground truth's are swept through the same LDS
//                       record array into two register keys; the pixel is classified against the frame in registers; the counts
//                       stay in registers over the workgroup's tiles, are summed in LDS and leave as at most 6 + n_tau integer adds
//   vsd_finish_kernel   one thread per (job, threshold): err = (union - within) / union
//
// Integer add / min / max are the only atomics: order-independent, so two calls give identical bytes.
#include "raster.h"

#define VSD_MAX_SIDE 16384
#define VSD_TILE RASTER_TILE
#define VSD_THREADS RASTER_THREADS
#define VSD_CAP RASTER_CAP
#define VSD_SUMS 6 // the columns the tile kernel adds to: all but the two dropped counts
#define VSD_MAX_T 1024

struct VsdJob {
    int img, vbase, nv, fbase, nf;
};

// the frame and mesh of a job, checked against the host's bounds and cut to the arrays; false: the job's rows stay zero
__device__ __forceinline__ bool vsd_job(const tgp_vsd_args &a, int j, VsdJob &m)
{
    m.img = a.job_img[j];
    const int mesh = a.job_mesh[j];
    if (m.img < 0 || m.img >= a.S || mesh < 0 || mesh >= a.M) return false;
    m.vbase = a.vptr[mesh];
    m.fbase = a.fptr[mesh];
    const long long nv = (long long)a.vptr[mesh + 1] - m.vbase, nf = (long long)a.fptr[mesh + 1] - m.fbase;
    if (m.vbase < 0 || m.fbase < 0 || nv < 1 || nf < 1 || m.vbase + nv > a.n_verts || m.fbase + nf > a.n_faces) return false;
    m.nv = (int)min(nv, (long long)a.max_verts);
    m.nf = (int)min(nf, (long long)a.max_faces);
    return true;
}

// the workspace, by pseudo-job: vertex records, triangle boxes, then first x, first y, last x, last y over the triangles' boxes
__device__ __forceinline__ int4 *vsd_vrec(const tgp_vsd_args &a) { return (int4 *)a.workspace; }
__device__ __forceinline__ short4 *vsd_boxes(const tgp_vsd_args &a)
{
    return (short4 *)((char *)a.workspace + (size_t)2 * a.J * a.max_verts * sizeof(int4));
}
__device__ __forceinline__ int *vsd_jobbox(const tgp_vsd_args &a)
{
    return (int *)((char *)a.workspace + (size_t)2 * a.J * a.max_verts * sizeof(int4) + (size_t)2 * a.J * a.max_faces * sizeof(short4));
}

__global__ __launch_bounds__(256) void vsd_vertex_kernel(const tgp_vsd_args a, int blocks_per_job)
{
    // the accumulators of this call: the first threads of the grid (it has at least 512 J threads, n_tau is at most 16)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < (size_t)a.J * TGP_VSD_COLS) a.counts[gid] = 0;
    if (gid < (size_t)a.J * a.n_tau) a.within[gid] = 0;
    if (gid < (size_t)2 * a.J) {
        int *jb = vsd_jobbox(a) + gid * 4;
        jb[0] = jb[1] = 0x7fffffff;
        jb[2] = jb[3] = -1;
    }
    const int q = blockIdx.x / blocks_per_job;
    const int v = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    const int j = q >> 1;
    VsdJob m;
    if (j >= a.J || !vsd_job(a, j, m) || v >= m.nv) return;
    const float *pose = ((q & 1) ? a.pose_gt : a.pose_est) + (size_t)j * 12;
    vsd_vrec(a)[(size_t)q * a.max_verts + v] = raster_vertex(a.verts + (size_t)(m.vbase + v) * 3, pose, a.camk + (size_t)m.img * 4, a.near);
}

__global__ __launch_bounds__(256) void vsd_box_kernel(const tgp_vsd_args a, int blocks_per_job)
{
    __shared__ int s_bb[4];
    __shared__ int s_drop;
    const int q = blockIdx.x / blocks_per_job;
    const int t = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    const int j = q >> 1;
    VsdJob m;
    if (j >= a.J || !vsd_job(a, j, m)) return; // the same for every lane
    if (threadIdx.x == 0) {
        s_bb[0] = s_bb[1] = 0x7fffffff;
        s_bb[2] = s_bb[3] = -1;
        s_drop = 0;
    }
    __syncthreads();
    if (t < m.nf) {
        const int32_t *f = a.faces + (size_t)(m.fbase + t) * 3;
        const int f0 = f[0], f1 = f[1], f2 = f[2];
        short4 box = make_short4(0x7fff, -1, 0x7fff, -1); // x first, x last, y first, y last: empty, it meets no tile
        if (f0 >= 0 && f0 < m.nv && f1 >= 0 && f1 < m.nv && f2 >= 0 && f2 < m.nv) {
            const int4 *vr = vsd_vrec(a) + (size_t)q * a.max_verts;
            if (raster_box(vr[f0], vr[f1], vr[f2], a.W, a.H, box)) { // the near rule or the guard band
                atomicAdd(&s_drop, 1);
            } else if (box.x <= box.y) {
                atomicMin(&s_bb[0], (int)box.x);
                atomicMin(&s_bb[1], (int)box.z);
                atomicMax(&s_bb[2], (int)box.y);
                atomicMax(&s_bb[3], (int)box.w);
            }
        }
        vsd_boxes(a)[(size_t)q * a.max_faces + t] = box;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_drop) atomicAdd(a.counts + (size_t)j * TGP_VSD_COLS + ((q & 1) ? 6 : 7), s_drop);
        if (s_bb[2] >= 0) {
            int *jb = vsd_jobbox(a) + (size_t)q * 4;
            atomicMin(jb + 0, s_bb[0]);
            atomicMin(jb + 1, s_bb[1]);
            atomicMax(jb + 2, s_bb[2]);
            atomicMax(jb + 3, s_bb[3]);
        }
    }
}

__global__ __launch_bounds__(VSD_THREADS) void vsd_tile_kernel(const tgp_vsd_args a)
{
    __shared__ RasterRec s_rec[VSD_CAP];
    __shared__ int s_n;
    __shared__ int s_sum[VSD_SUMS + TGP_VSD_MAX_TAUS];

    const int tid = threadIdx.x;
    const int j = blockIdx.x;
    VsdJob m;
    if (!vsd_job(a, j, m)) return; // the same for every lane, as is every return below
    const int *jb = vsd_jobbox(a) + (size_t)j * 8; // the estimate's box, then the ground truth's; an empty one is (max, max, -1, -1)
    const int bx0 = min(jb[0], jb[4]), by0 = min(jb[1], jb[5]), bx1 = max(jb[2], jb[6]), by1 = max(jb[3], jb[7]); // inside the frame
    if (bx1 < bx0 || by1 < by0) return;
    const int ntx = (bx1 - bx0) / VSD_TILE + 1, nty = (by1 - by0) / VSD_TILE + 1;
    const int ntiles = ntx * nty;
    if ((int)blockIdx.y >= ntiles) return;

    const int li = tid % VSD_TILE, lj = tid / VSD_TILE;
    const uint16_t *frame = a.depth + (size_t)m.img * a.H * a.W;
    const int delta = a.delta, n_tau = a.n_tau;
    const int32_t *tau = a.job_tau + (size_t)j * n_tau; // the same address for every lane

    int sums[VSD_SUMS]; // rendered_gt, rendered_est, visib_gt, visib_est, inter, union
    int within[TGP_VSD_MAX_TAUS];
#pragma unroll
    for (int c = 0; c < VSD_SUMS; ++c) sums[c] = 0;
#pragma unroll
    for (int c = 0; c < TGP_VSD_MAX_TAUS; ++c) within[c] = 0;
    if (tid < VSD_SUMS + TGP_VSD_MAX_TAUS) s_sum[tid] = 0;

    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int tx0 = bx0 + (tile % ntx) * VSD_TILE, ty0 = by0 + (tile / ntx) * VSD_TILE;
        const int tx1 = min(tx0 + VSD_TILE - 1, bx1), ty1 = min(ty0 + VSD_TILE - 1, by1);

        unsigned long long keys[2];
#pragma unroll
        for (int which = 0; which < 2; ++which) { // the estimate's surface, then the ground truth's, through the same records
            const int q = 2 * j + which;
            const short4 *boxes = vsd_boxes(a) + (size_t)q * a.max_faces;
            const int4 *vr = vsd_vrec(a) + (size_t)q * a.max_verts;
            unsigned long long key = ~0ull;
            __syncthreads(); // the sweep before this one has read s_n and s_rec
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int base = 0; base < m.nf; base += VSD_THREADS) {
                const int t = base + tid;
                if (t < m.nf) {
                    const short4 b = boxes[t];
                    if (b.x <= tx1 && b.y >= tx0 && b.z <= ty1 && b.w >= ty0) { // false for an empty box
                        const int32_t *f = a.faces + (size_t)(m.fbase + t) * 3;
                        // at most VSD_CAP - 256 records held + 256 of this chunk
                        raster_setup(s_rec[atomicAdd(&s_n, 1)], vr[f[0]], vr[f[1]], vr[f[2]], tx0, ty0, (uint32_t)t);
                    }
                }
                __syncthreads();
                const int n = s_n;
                __syncthreads(); // every lane has read s_n before a lane of the next chunk adds to it
                if (n > VSD_CAP - VSD_THREADS) {
                    raster_sweep(s_rec, n, li, lj, key);
                    __syncthreads();
                    if (tid == 0) s_n = 0;
                    __syncthreads();
                }
            }
            raster_sweep(s_rec, s_n, li, lj, key); // the last barrier above is behind every write of s_n and s_rec
            keys[which] = key;
        }

        const int px = tx0 + li, py = ty0 + lj;
        if (px <= bx1 && py <= by1) {
            const int d_e = keys[0] != ~0ull ? raster_depth_mm(__uint_as_float((uint32_t)(keys[0] >> 32))) : 0;
            const int d_g = keys[1] != ~0ull ? raster_depth_mm(__uint_as_float((uint32_t)(keys[1] >> 32))) : 0;
            if (d_e | d_g) {
                const int d_o = frame[(size_t)py * a.W + px];
                const bool vis_g = d_g > 0 && (d_o == 0 || d_g - d_o <= delta);
                const bool vis_e = (d_e > 0 && (d_o == 0 || d_e - d_o <= delta)) || (vis_g && d_e > 0);
                const bool inter = vis_g && vis_e;
                sums[0] += d_g > 0;
                sums[1] += d_e > 0;
                sums[2] += vis_g;
                sums[3] += vis_e;
                sums[4] += inter;
                sums[5] += vis_g || vis_e;
                if (inter) {
                    const int diff = abs(d_g - d_e);
#pragma unroll
                    for (int c = 0; c < TGP_VSD_MAX_TAUS; ++c)
                        if (c < n_tau) within[c] += diff < tau[c];
                }
            }
        }
    }

    // every lane is behind the first barrier of its first tile, so s_sum is zero
#pragma unroll
    for (int c = 0; c < VSD_SUMS; ++c)
        if (sums[c]) atomicAdd(&s_sum[c], sums[c]);
#pragma unroll
    for (int c = 0; c < TGP_VSD_MAX_TAUS; ++c)
        if (within[c]) atomicAdd(&s_sum[VSD_SUMS + c], within[c]); // zero from n_tau on
    __syncthreads();
    if (tid < VSD_SUMS && s_sum[tid]) atomicAdd(a.counts + (size_t)j * TGP_VSD_COLS + tid, s_sum[tid]);
    if (tid >= VSD_SUMS && tid < VSD_SUMS + n_tau && s_sum[tid]) atomicAdd(a.within + (size_t)j * n_tau + (tid - VSD_SUMS), s_sum[tid]);
}

__global__ __launch_bounds__(256) void vsd_finish_kernel(const tgp_vsd_args a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.J * a.n_tau) return;
    const int un = a.counts[(i / a.n_tau) * TGP_VSD_COLS + 5];
    a.err[i] = un > 0 ? (float)(un - a.within[i]) / (float)un : 1.f; // both below 2^24: the conversions are exact
}

extern "C" int64_t tgp_vsd_workspace_bytes(int J, int max_verts, int max_faces)
{
    if (J < 0 || max_verts < 1 || max_faces < 1) return TGP_EINVAL;
    if (J > TGP_VERIFY_MAX_JOBS || max_faces >= tgp_render_max_faces()) return TGP_EUNSUPPORTED;
    return 2 * ((int64_t)J * max_verts * (int64_t)sizeof(int4) + (int64_t)J * max_faces * (int64_t)sizeof(short4) + (int64_t)J * 16) + 16;
}

extern "C" int tgp_pose_vsd(const tgp_vsd_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_vsd_args &a = *args;
    TGP_REQUIRE(a.depth && a.camk && a.verts && a.faces && a.vptr && a.fptr);
    TGP_REQUIRE(a.M > 0 && a.n_verts > 0 && a.n_faces > 0 && a.max_verts > 0 && a.max_faces > 0);
    TGP_REQUIRE(a.S > 0 && a.H > 0 && a.W > 0 && a.J >= 0 && a.n_tau > 0 && a.delta >= 0);
    TGP_REQUIRE(a.near > 0.f && a.near < __builtin_inff());
    if (a.J > 0) TGP_REQUIRE(a.job_img && a.job_mesh && a.pose_est && a.pose_gt && a.job_tau && a.counts && a.within && a.err && a.workspace);
    if (a.J > TGP_VERIFY_MAX_JOBS || a.n_tau > TGP_VSD_MAX_TAUS || a.delta > 65535 || (int64_t)a.H * a.W >= (1 << 24) || a.H > VSD_MAX_SIDE ||
        a.W > VSD_MAX_SIDE || a.max_faces >= tgp_render_max_faces())
        return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    TGP_REQUIRE(a.workspace_bytes >= tgp_vsd_workspace_bytes(a.J, a.max_verts, a.max_faces));
    const int64_t vblocks = tgp_cdiv(a.max_verts, 256), fblocks = tgp_cdiv(a.max_faces, 256);
    const int64_t grid_v = 2 * a.J * vblocks, grid_f = 2 * a.J * fblocks;
    if (grid_v > 0x7fffffff || grid_f > 0x7fffffff) return TGP_EUNSUPPORTED;
    // T workgroups per job, as tgp_pose_verify chooses them
    const int64_t frame_tiles = (int64_t)tgp_cdiv(a.W, VSD_TILE) * tgp_cdiv(a.H, VSD_TILE);
    int64_t T = 4096 / a.J;
    T = T < 16 ? 16 : T > VSD_MAX_T ? VSD_MAX_T : T;
    T = T > frame_tiles ? frame_tiles : T;
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(vsd_vertex_kernel, dim3((unsigned)grid_v), dim3(256), 0, st, a, (int)vblocks);
    hipLaunchKernelGGL(vsd_box_kernel, dim3((unsigned)grid_f), dim3(256), 0, st, a, (int)fblocks);
    hipLaunchKernelGGL(vsd_tile_kernel, dim3((unsigned)a.J, (unsigned)T), dim3(VSD_THREADS), 0, st, a);
    hipLaunchKernelGGL(vsd_finish_kernel, dim3(tgp_cdiv((int64_t)a.J * a.n_tau, 256)), dim3(256), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
