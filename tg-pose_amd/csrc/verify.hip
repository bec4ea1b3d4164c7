// Pose verification, render-and-compare: J jobs (frame, mesh, pose) per call (include/tgpose.h, DESIGN.md section 3 "Pose
// verification").  A job's rendered surface is the depth renderer's for a scene of that one instance: the vertex, box, coverage, z
// and winner arithmetic is raster.h's, which csrc/render.hip runs too, with scene = job and the key's low word = the face.  No frame
// of it is written.
//
//   verify_vertex_kernel    one thread per (job, vertex): pose, project, snap to 1/256 px -> {X, Y, 1/z, flag}; zeroes the counts
//   verify_box_kernel       one thread per (job, face): the drop rules and the pixel box of the snapped triangle; per workgroup one
//                           integer min / max into the job's box and one add into its dropped count
//   verify_tile_kernel      grid (J, T): workgroup (j, k) takes the 16 x 16 tiles k, k + T, ... of job j's box -- no cap on a job's
//                           screen size, no workgroup over a tile outside every job.  One pixel per lane with its key {z bits, face}
//                           in a register and LDS triangle records swept as in render_tile_kernel; the winner is compared with the
//                           frame's pixel in registers, the class counts stay in registers over the workgroup's tiles, are summed in
//                           LDS and leave as one integer add per class
//   verify_score_kernel     one thread per job: score = match / (rendered - occluded)
//
// Integer add / min / max are the only atomics: order-independent, so two calls give identical bytes.
#include "raster.h"

#define VERIFY_MAX_SIDE 16384
#define VERIFY_TILE RASTER_TILE
#define VERIFY_THREADS RASTER_THREADS
#define VERIFY_CAP RASTER_CAP
#define VERIFY_SUMS 7 // the columns the tile kernel adds to: all but dropped
#define VERIFY_MAX_T 1024

struct VerifyJob {
    int img, vbase, nv, fbase, nf;
};

// the frame and mesh of a job, checked against the host's bounds and cut to the arrays; false: the job's row stays zero
__device__ __forceinline__ bool verify_job(const tgp_verify_args &a, int j, VerifyJob &m)
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

__device__ __forceinline__ int4 *verify_vrec(const tgp_verify_args &a) { return (int4 *)a.workspace; }
__device__ __forceinline__ short4 *verify_boxes(const tgp_verify_args &a)
{
    return (short4 *)((char *)a.workspace + (size_t)a.J * a.max_verts * sizeof(int4));
}
// per job: first x, first y, last x, last y over its triangles' boxes
__device__ __forceinline__ int *verify_jobbox(const tgp_verify_args &a)
{
    return (int *)((char *)a.workspace + (size_t)a.J * a.max_verts * sizeof(int4) + (size_t)a.J * a.max_faces * sizeof(short4));
}

__global__ __launch_bounds__(256) void verify_vertex_kernel(const tgp_verify_args a, int blocks_per_job)
{
    // the accumulators of this call: the first threads of the grid (it has at least 256 J threads)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < (size_t)a.J * TGP_VERIFY_COLS) a.counts[gid] = 0;
    if (gid < (size_t)a.J) {
        int *jb = verify_jobbox(a) + gid * 4;
        jb[0] = jb[1] = 0x7fffffff;
        jb[2] = jb[3] = -1;
    }
    const int j = blockIdx.x / blocks_per_job;
    const int v = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    VerifyJob m;
    if (j >= a.J || !verify_job(a, j, m) || v >= m.nv) return;
    verify_vrec(a)[(size_t)j * a.max_verts + v] = raster_vertex(a.verts + (size_t)(m.vbase + v) * 3, a.job_pose + (size_t)j * 12,
                                                                 a.camk + (size_t)m.img * 4, a.near);
}

__global__ __launch_bounds__(256) void verify_box_kernel(const tgp_verify_args a, int blocks_per_job)
{
    __shared__ int s_bb[4];
    __shared__ int s_drop;
    const int j = blockIdx.x / blocks_per_job;
    const int t = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    VerifyJob m;
    if (j >= a.J || !verify_job(a, j, m)) return; // the same for every lane
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
            const int4 *vr = verify_vrec(a) + (size_t)j * a.max_verts;
            if (raster_box(vr[f0], vr[f1], vr[f2], a.W, a.H, box)) { // the near rule or the guard band
                atomicAdd(&s_drop, 1);
            } else if (box.x <= box.y) {
                atomicMin(&s_bb[0], (int)box.x);
                atomicMin(&s_bb[1], (int)box.z);
                atomicMax(&s_bb[2], (int)box.y);
                atomicMax(&s_bb[3], (int)box.w);
            }
        }
        verify_boxes(a)[(size_t)j * a.max_faces + t] = box;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_drop) atomicAdd(a.counts + (size_t)j * TGP_VERIFY_COLS + 7, s_drop);
        if (s_bb[2] >= 0) {
            int *jb = verify_jobbox(a) + (size_t)j * 4;
            atomicMin(jb + 0, s_bb[0]);
            atomicMin(jb + 1, s_bb[1]);
            atomicMax(jb + 2, s_bb[2]);
            atomicMax(jb + 3, s_bb[3]);
        }
    }
}

__global__ __launch_bounds__(VERIFY_THREADS) void verify_tile_kernel(const tgp_verify_args a)
{
    __shared__ RasterRec s_rec[VERIFY_CAP];
    __shared__ int s_n;
    __shared__ int s_sum[VERIFY_SUMS];

    const int tid = threadIdx.x;
    const int j = blockIdx.x;
    VerifyJob m;
    if (!verify_job(a, j, m)) return; // the same for every lane, as is every return below
    const int *jb = verify_jobbox(a) + (size_t)j * 4;
    const int bx0 = jb[0], by0 = jb[1], bx1 = jb[2], by1 = jb[3]; // inside the frame: every triangle's box is
    if (bx1 < bx0 || by1 < by0) return;
    const int ntx = (bx1 - bx0) / VERIFY_TILE + 1, nty = (by1 - by0) / VERIFY_TILE + 1;
    const int ntiles = ntx * nty;
    if ((int)blockIdx.y >= ntiles) return;

    const int li = tid % VERIFY_TILE, lj = tid / VERIFY_TILE;
    const short4 *boxes = verify_boxes(a) + (size_t)j * a.max_faces;
    const int4 *vr = verify_vrec(a) + (size_t)j * a.max_verts;
    const uint16_t *frame = a.depth + (size_t)m.img * a.H * a.W;
    const uint8_t *mframe = a.mask ? a.mask + (size_t)m.img * a.H * a.W : nullptr;
    const int mask_val = a.mask ? a.job_mask_val[j] : 0;
    const int tau = a.tau;

    int sums[VERIFY_SUMS]; // the columns of counts: rendered, match, violation, occluded, nodata, in_mask, abs_sum
#pragma unroll
    for (int c = 0; c < VERIFY_SUMS; ++c) sums[c] = 0;
    if (tid < VERIFY_SUMS) s_sum[tid] = 0;

    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int tx0 = bx0 + (tile % ntx) * VERIFY_TILE, ty0 = by0 + (tile / ntx) * VERIFY_TILE;
        const int tx1 = min(tx0 + VERIFY_TILE - 1, bx1), ty1 = min(ty0 + VERIFY_TILE - 1, by1);
        __syncthreads(); // the sweep of the tile before this one has read s_n and s_rec
        if (tid == 0) s_n = 0;
        __syncthreads();

        unsigned long long key = ~0ull;

        auto sweep = [&](int n) { raster_sweep(s_rec, n, li, lj, key); };

        for (int base = 0; base < m.nf; base += VERIFY_THREADS) {
            const int t = base + tid;
            if (t < m.nf) {
                const short4 b = boxes[t];
                if (b.x <= tx1 && b.y >= tx0 && b.z <= ty1 && b.w >= ty0) { // false for an empty box
                    const int32_t *f = a.faces + (size_t)(m.fbase + t) * 3;
                    // at most VERIFY_CAP - 256 records held + 256 of this chunk
                    raster_setup(s_rec[atomicAdd(&s_n, 1)], vr[f[0]], vr[f[1]], vr[f[2]], tx0, ty0, (uint32_t)t);
                }
            }
            __syncthreads();
            const int n = s_n;
            __syncthreads(); // every lane has read s_n before a lane of the next chunk adds to it
            if (n > VERIFY_CAP - VERIFY_THREADS) {
                sweep(n);
                __syncthreads();
                if (tid == 0) s_n = 0;
                __syncthreads();
            }
        }
        sweep(s_n); // the last barrier above is behind every write of s_n and s_rec

        const int px = tx0 + li, py = ty0 + lj;
        if (px <= bx1 && py <= by1 && key != ~0ull) {
            const int d_r = raster_depth_mm(__uint_as_float((uint32_t)(key >> 32)));
            const size_t o = (size_t)py * a.W + px;
            const int d_o = frame[o];
            sums[0] += 1;
            if (d_o == 0 || d_r == 0) {
                sums[4] += 1;
            } else if (d_o + tau < d_r) {
                sums[3] += 1;
            } else if (d_o <= d_r + tau) {
                sums[1] += 1;
                sums[6] += abs(d_o - d_r);
            } else {
                sums[2] += 1;
            }
            if (mframe && mframe[o] == mask_val) sums[5] += 1;
        }
    }

    // every lane is behind the first barrier of its first tile, so s_sum is zero
#pragma unroll
    for (int c = 0; c < VERIFY_SUMS; ++c)
        if (sums[c]) atomicAdd(&s_sum[c], sums[c]);
    __syncthreads();
    if (tid < VERIFY_SUMS && s_sum[tid]) atomicAdd(a.counts + (size_t)j * TGP_VERIFY_COLS + tid, s_sum[tid]);
}

__global__ __launch_bounds__(256) void verify_score_kernel(const tgp_verify_args a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.J) return;
    const int32_t *row = a.counts + (size_t)j * TGP_VERIFY_COLS;
    const int den = row[0] - row[3];
    a.score[j] = den > 0 ? (float)row[1] / (float)den : 0.f; // both below 2^24: the conversions are exact
}

extern "C" int64_t tgp_verify_workspace_bytes(int J, int max_verts, int max_faces)
{
    if (J < 0 || max_verts < 1 || max_faces < 1) return TGP_EINVAL;
    if (J > TGP_VERIFY_MAX_JOBS || max_faces >= tgp_render_max_faces()) return TGP_EUNSUPPORTED;
    return (int64_t)J * max_verts * (int64_t)sizeof(int4) + (int64_t)J * max_faces * (int64_t)sizeof(short4) + (int64_t)J * 16 + 16;
}

extern "C" int tgp_pose_verify(const tgp_verify_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_verify_args &a = *args;
    TGP_REQUIRE(a.depth && a.camk && a.verts && a.faces && a.vptr && a.fptr);
    TGP_REQUIRE(a.M > 0 && a.n_verts > 0 && a.n_faces > 0 && a.max_verts > 0 && a.max_faces > 0);
    TGP_REQUIRE(a.S > 0 && a.H > 0 && a.W > 0 && a.J >= 0 && a.tau >= 0);
    TGP_REQUIRE(a.near > 0.f && a.near < __builtin_inff());
    TGP_REQUIRE(!a.mask || a.job_mask_val);
    if (a.J > 0) TGP_REQUIRE(a.job_img && a.job_mesh && a.job_pose && a.counts && a.score && a.workspace);
    if (a.J > TGP_VERIFY_MAX_JOBS || a.tau > TGP_VERIFY_MAX_TAU || (int64_t)a.H * a.W >= (1 << 24) || a.H > VERIFY_MAX_SIDE ||
        a.W > VERIFY_MAX_SIDE || a.max_faces >= tgp_render_max_faces())
        return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    TGP_REQUIRE(a.workspace_bytes >= tgp_verify_workspace_bytes(a.J, a.max_verts, a.max_faces));
    const int64_t vblocks = tgp_cdiv(a.max_verts, 256), fblocks = tgp_cdiv(a.max_faces, 256);
    const int64_t grid_v = a.J * vblocks, grid_f = a.J * fblocks;
    if (grid_v > 0x7fffffff || grid_f > 0x7fffffff) return TGP_EUNSUPPORTED;
    // T workgroups per job: enough that a few jobs fill the device, few enough that many jobs do not flood it with workgroups that
    // find no tile; never more than the frame has tiles
    const int64_t frame_tiles = (int64_t)tgp_cdiv(a.W, VERIFY_TILE) * tgp_cdiv(a.H, VERIFY_TILE);
    int64_t T = 4096 / a.J;
    T = T < 16 ? 16 : T > VERIFY_MAX_T ? VERIFY_MAX_T : T;
    T = T > frame_tiles ? frame_tiles : T;
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(verify_vertex_kernel, dim3((unsigned)grid_v), dim3(256), 0, st, a, (int)vblocks);
    hipLaunchKernelGGL(verify_box_kernel, dim3((unsigned)grid_f), dim3(256), 0, st, a, (int)fblocks);
    hipLaunchKernelGGL(verify_tile_kernel, dim3((unsigned)a.J, (unsigned)T), dim3(VERIFY_THREADS), 0, st, a);
    hipLaunchKernelGGL(verify_score_kernel, dim3(tgp_cdiv(a.J, 256)), dim3(256), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
