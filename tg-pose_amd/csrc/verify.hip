// Pose verification, render-and-compare: J jobs (frame, mesh, pose) per call (include/tgpose.h, DESIGN.md section 3 "Pose
// verification").  A job's rendered surface is the depth renderer's for a scene of that one instance: the vertex, box, coverage, z
// and winner arithmetic is raster.h's, which csrc/render.hip runs too, with scene = job and the key's low word = the face; so are the
// job's decode, the workspace (one unit per job), the box pass, the tile walk and the launch shape, which csrc/vsd.hip shares.  The
// classification of a pixel and the seven sums are this file's.  No frame of the surface is written.
//
//   verify_vertex_kernel    one thread per (job, vertex): pose, project, snap to 1/256 px -> {X, Y, 1/z, flag}; zeroes the counts
//   verify_box_kernel       one thread per (job, face): the drop rules and the pixel box of the snapped triangle; per workgroup one
//                           integer min / max into the job's box and one add into its dropped count
//   verify_tile_kernel      grid (J, T): workgroup (j, k) takes the 16 x 16 tiles k, k + T, ... of job j's box -- no cap on a job's
//                           screen size, no workgroup over a tile outside every job.  One pixel per lane with its key {z bits, face}
//                           in a register and raster.h's tile walk, reset before the tile and flushed after it; the winner is
//                           compared with the frame's pixel in registers, the class counts stay in registers over the workgroup's
//                           tiles, are summed in LDS and leave as one integer add per class
//   verify_score_kernel     one thread per job: score = match / (rendered - occluded)
//
// Integer add / min / max are the only atomics: order-independent, so two calls give identical bytes.
#include "raster.h"

#define VERIFY_SUMS 7 // the columns the tile kernel adds to: all but dropped

__global__ __launch_bounds__(256) void verify_vertex_kernel(const tgp_verify_args a, int blocks_per_job)
{
    // the accumulators of this call: the first threads of the grid (it has at least 256 J threads)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < (size_t)a.J * TGP_VERIFY_COLS) a.counts[gid] = 0;
    if (gid < (size_t)a.J) {
        int *jb = raster_workspace(a, a.J).unit_box(gid);
        jb[0] = jb[1] = 0x7fffffff;
        jb[2] = jb[3] = -1;
    }
    const int j = blockIdx.x / blocks_per_job;
    const int v = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    int img;
    RasterMesh m;
    if (j >= a.J || !raster_job(a, j, img, m) || v >= m.nv) return;
    raster_workspace(a, a.J).vrec(j)[v] = raster_vertex(a.verts + (size_t)(m.vbase + v) * 3, a.job_pose + (size_t)j * 12,
                                                        a.camk + (size_t)img * 4, a.near);
}

__global__ __launch_bounds__(256) void verify_box_kernel(const tgp_verify_args a, int blocks_per_job)
{
    const int j = blockIdx.x / blocks_per_job;
    const int t = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    int img;
    RasterMesh m;
    if (j >= a.J || !raster_job(a, j, img, m)) return; // the same for every lane
    const RasterWorkspace ws = raster_workspace(a, a.J);
    short4 box = make_short4(0x7fff, -1, 0x7fff, -1);
    const int rule = t < m.nf ? raster_face_box(a.faces, m, t, ws.vrec(j), a.W, a.H, ws.boxes(j), box) : 0;
    raster_box_reduce(rule, box, ws.unit_box(j), a.counts + (size_t)j * TGP_VERIFY_COLS + 7);
}

__global__ __launch_bounds__(RASTER_THREADS) void verify_tile_kernel(const tgp_verify_args a)
{
    __shared__ RasterRec s_rec[RASTER_CAP];
    __shared__ int s_n;
    __shared__ int s_sum[VERIFY_SUMS];

    const int tid = threadIdx.x;
    const int j = blockIdx.x;
    int img;
    RasterMesh m;
    if (!raster_job(a, j, img, m)) return; // the same for every lane, as is every return below
    const RasterWorkspace ws = raster_workspace(a, a.J);
    const int *jb = ws.unit_box(j);
    const int bx0 = jb[0], by0 = jb[1], bx1 = jb[2], by1 = jb[3]; // inside the frame: every triangle's box is
    if (bx1 < bx0 || by1 < by0) return;
    const int ntx = (bx1 - bx0) / RASTER_TILE + 1, nty = (by1 - by0) / RASTER_TILE + 1;
    const int ntiles = ntx * nty;
    if ((int)blockIdx.y >= ntiles) return;

    const int li = tid % RASTER_TILE, lj = tid / RASTER_TILE;
    const uint16_t *frame = a.depth + (size_t)img * a.H * a.W;
    const uint8_t *mframe = a.mask ? a.mask + (size_t)img * a.H * a.W : nullptr;
    const int mask_val = a.mask ? a.job_mask_val[j] : 0;
    const int tau = a.tau;

    int sums[VERIFY_SUMS]; // the columns of counts: rendered, match, violation, occluded, nodata, in_mask, abs_sum
#pragma unroll
    for (int c = 0; c < VERIFY_SUMS; ++c) sums[c] = 0;
    if (tid < VERIFY_SUMS) s_sum[tid] = 0;

    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int tx0 = bx0 + (tile % ntx) * RASTER_TILE, ty0 = by0 + (tile / ntx) * RASTER_TILE;
        const int tx1 = min(tx0 + RASTER_TILE - 1, bx1), ty1 = min(ty0 + RASTER_TILE - 1, by1);
        unsigned long long key = ~0ull;
        raster_reset(s_n);
        raster_bin(s_rec, s_n, ws.boxes(j), ws.vrec(j), a.faces, m.fbase, m.nf, tx0, ty0, tx1, ty1, 0u, li, lj, key);
        raster_flush(s_rec, s_n, li, lj, key);

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

    // every lane is behind the first reset's barriers, so s_sum is zero
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
    return raster_workspace_bytes(J, max_verts, max_faces);
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
    if (a.J > TGP_VERIFY_MAX_JOBS || a.tau > TGP_VERIFY_MAX_TAU || (int64_t)a.H * a.W >= (1 << 24) || !raster_side_ok(a.H, a.W) ||
        a.max_faces >= tgp_render_max_faces())
        return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    TGP_REQUIRE(a.workspace_bytes >= tgp_verify_workspace_bytes(a.J, a.max_verts, a.max_faces));
    RasterJobLaunch l;
    if (!raster_job_launch(a.J, a.J, a.H, a.W, a.max_verts, a.max_faces, l)) return TGP_EUNSUPPORTED;
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(verify_vertex_kernel, dim3(l.grid_v), dim3(256), 0, st, a, l.vblocks);
    hipLaunchKernelGGL(verify_box_kernel, dim3(l.grid_f), dim3(256), 0, st, a, l.fblocks);
    hipLaunchKernelGGL(verify_tile_kernel, dim3((unsigned)a.J, l.T), dim3(RASTER_THREADS), 0, st, a);
    hipLaunchKernelGGL(verify_score_kernel, dim3(tgp_cdiv(a.J, 256)), dim3(256), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
