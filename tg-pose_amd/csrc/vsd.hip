// BOP pose errors, two-pose VSD: J jobs (frame, mesh, estimated pose, ground-truth pose) per call (include/tgpose.h, DESIGN.md
// section 3 "BOP pose errors"; tests/bop_ref.py restates the contract in NumPy on tests/render_ref.py).  Each of a job's two surfaces
// is the depth renderer's for a scene of that one instance: the vertex, box, coverage, z and winner arithmetic is raster.h's, and so
// are the job's decode, the workspace, the box pass, the tile walk and the launch shape, as in csrc/verify.hip, here with 2 J units:
// the pseudo-jobs q = 2 j + (0: estimate, 1: ground truth).  The two keys, the union box and the within[] thresholds are this file's.
// No frame is written.
//
//   vsd_vertex_kernel   one thread per (pseudo-job, vertex): pose, project, snap -> {X, Y, 1/z, flag}; zeroes counts and within
//   vsd_box_kernel      one thread per (pseudo-job, face): the drop rules and the pixel box; per workgroup one integer min / max into
//                       the pseudo-job's box and one add into the job's dropped_gt / dropped_est
//   vsd_tile_kernel     grid (J, T): workgroup (j, k) takes the 16 x 16 tiles k, k + T, ... of the UNION of job j's two boxes.  One
//                       pixel per lane; the estimate's triangle list and then the ground truth's go through the same LDS record
//                       array (reset, bin, flush) into two register keys; the pixel is classified against the frame in registers;
//                       the counts stay in registers over the workgroup's tiles, are summed in LDS and leave as at most 6 + n_tau
//                       integer adds
//   vsd_finish_kernel   one thread per (job, threshold): err = (union - within) / union
//
// Integer add / min / max are the only atomics: order-independent, so two calls give identical bytes.
#include "raster.h"

#define VSD_SUMS 6 // the columns the tile kernel adds to: all but the two dropped counts

__global__ __launch_bounds__(256) void vsd_vertex_kernel(const tgp_vsd_args a, int blocks_per_job)
{
    // the accumulators of this call: the first threads of the grid (it has at least 512 J threads, n_tau is at most 16)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < (size_t)a.J * TGP_VSD_COLS) a.counts[gid] = 0;
    if (gid < (size_t)a.J * a.n_tau) a.within[gid] = 0;
    if (gid < (size_t)2 * a.J) {
        int *jb = raster_workspace(a, 2 * a.J).unit_box(gid);
        jb[0] = jb[1] = 0x7fffffff;
        jb[2] = jb[3] = -1;
    }
    const int q = blockIdx.x / blocks_per_job;
    const int v = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    const int j = q >> 1;
    int img;
    RasterMesh m;
    if (j >= a.J || !raster_job(a, j, img, m) || v >= m.nv) return;
    const float *pose = ((q & 1) ? a.pose_gt : a.pose_est) + (size_t)j * 12;
    raster_workspace(a, 2 * a.J).vrec(q)[v] = raster_vertex(a.verts + (size_t)(m.vbase + v) * 3, pose, a.camk + (size_t)img * 4, a.near);
}

__global__ __launch_bounds__(256) void vsd_box_kernel(const tgp_vsd_args a, int blocks_per_job)
{
    const int q = blockIdx.x / blocks_per_job;
    const int t = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    const int j = q >> 1;
    int img;
    RasterMesh m;
    if (j >= a.J || !raster_job(a, j, img, m)) return; // the same for every lane
    const RasterWorkspace ws = raster_workspace(a, 2 * a.J);
    short4 box = make_short4(0x7fff, -1, 0x7fff, -1);
    const int rule = t < m.nf ? raster_face_box(a.faces, m, t, ws.vrec(q), a.W, a.H, ws.boxes(q), box) : 0;
    raster_box_reduce(rule, box, ws.unit_box(q), a.counts + (size_t)j * TGP_VSD_COLS + ((q & 1) ? 6 : 7));
}

__global__ __launch_bounds__(RASTER_THREADS) void vsd_tile_kernel(const tgp_vsd_args a)
{
    __shared__ RasterRec s_rec[RASTER_CAP];
    __shared__ int s_n;
    __shared__ int s_sum[VSD_SUMS + TGP_VSD_MAX_TAUS];

    const int tid = threadIdx.x;
    const int j = blockIdx.x;
    int img;
    RasterMesh m;
    if (!raster_job(a, j, img, m)) return; // the same for every lane, as is every return below
    const RasterWorkspace ws = raster_workspace(a, 2 * a.J);
    const int *jb = ws.unit_box(2 * j); // the estimate's box, then the ground truth's; an empty one is (max, max, -1, -1)
    const int bx0 = min(jb[0], jb[4]), by0 = min(jb[1], jb[5]), bx1 = max(jb[2], jb[6]), by1 = max(jb[3], jb[7]); // inside the frame
    if (bx1 < bx0 || by1 < by0) return;
    const int ntx = (bx1 - bx0) / RASTER_TILE + 1, nty = (by1 - by0) / RASTER_TILE + 1;
    const int ntiles = ntx * nty;
    if ((int)blockIdx.y >= ntiles) return;

    const int li = tid % RASTER_TILE, lj = tid / RASTER_TILE;
    const uint16_t *frame = a.depth + (size_t)img * a.H * a.W;
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
        const int tx0 = bx0 + (tile % ntx) * RASTER_TILE, ty0 = by0 + (tile / ntx) * RASTER_TILE;
        const int tx1 = min(tx0 + RASTER_TILE - 1, bx1), ty1 = min(ty0 + RASTER_TILE - 1, by1);

        unsigned long long keys[2];
#pragma unroll
        for (int which = 0; which < 2; ++which) { // the estimate's surface, then the ground truth's, through the same records
            const int q = 2 * j + which;
            unsigned long long key = ~0ull;
            raster_reset(s_n);
            raster_bin(s_rec, s_n, ws.boxes(q), ws.vrec(q), a.faces, m.fbase, m.nf, tx0, ty0, tx1, ty1, 0u, li, lj, key);
            raster_flush(s_rec, s_n, li, lj, key);
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

    // every lane is behind the first reset's barriers, so s_sum is zero
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
    return raster_workspace_bytes(2 * (int64_t)J, max_verts, max_faces); // 2 x (J units) + 16
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
    if (a.J > TGP_VERIFY_MAX_JOBS || a.n_tau > TGP_VSD_MAX_TAUS || a.delta > 65535 || (int64_t)a.H * a.W >= (1 << 24) ||
        !raster_side_ok(a.H, a.W) || a.max_faces >= tgp_render_max_faces())
        return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    TGP_REQUIRE(a.workspace_bytes >= tgp_vsd_workspace_bytes(a.J, a.max_verts, a.max_faces));
    RasterJobLaunch l;
    if (!raster_job_launch(2 * (int64_t)a.J, a.J, a.H, a.W, a.max_verts, a.max_faces, l)) return TGP_EUNSUPPORTED;
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(vsd_vertex_kernel, dim3(l.grid_v), dim3(256), 0, st, a, l.vblocks);
    hipLaunchKernelGGL(vsd_box_kernel, dim3(l.grid_f), dim3(256), 0, st, a, l.fblocks);
    hipLaunchKernelGGL(vsd_tile_kernel, dim3((unsigned)a.J, l.T), dim3(RASTER_THREADS), 0, st, a);
    hipLaunchKernelGGL(vsd_finish_kernel, dim3(tgp_cdiv((int64_t)a.J * a.n_tau, 256)), dim3(256), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
