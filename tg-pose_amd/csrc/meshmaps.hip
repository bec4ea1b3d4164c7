// Vertex and normal maps of posed meshes: J (mesh, pose, window) jobs per call (include/tgpose.h tgp_mesh_maps, DESIGN.md section 3
// "Mesh maps and dense model-based tracking"; tests/meshmaps_ref.py restates every rule in NumPy on tests/render_ref.py).  The maps
// are tgp_tsdf_raycast's -- z, depth, vertex and normal in the MODEL frame, cell (r, c) at the pixel coordinates (u0 + c du, v0 + r
// dv) -- so tgp_icp_dense registers against a mesh as it registers against a volume.
//
// The window is a camera: K' = (fx / du, fy / dv, (cx - u0) / du, (cy - v0) / dv), and the job is a w x h frame under K' by raster.h's
// rules unchanged; the job's decode, the workspace (one unit per job), the box pass, the tile walk and the launch shape are raster.h's
// too, as csrc/verify.hip uses them.  What is done with a cell's winner is this file's (meshmaps_resolve).  In float32, every
// operation rounded on its own, no contraction, in the order written:
//   corners   (i0, i1, i2) the winner's face, records v_k, model corners p_k; where the snapped area is negative corners 1 and 2
//             change places, as raster_setup swaps them
//   e_k       the edge integers at the cell's sample (256 c, 256 r): e_0 = orient(v1, v2, s), e_1 = orient(v2, v0, s), e_2 =
//             orient(v0, v1, s) -- the sweep's q.e[k] + 256 (lj dx_k - li dy_k), which is the same integer
//   w_k       (float)e_k / (float)area;  z = the key's high word;  b_k = (w_k iz_k) z
//   vertex_a  (b_0 p0_a + b_1 p1_a) + b_2 p2_a
//   normal    face mode: u = p1 - p0, v = p2 - p0, n = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x);
//             vertex mode: n_a = (b_0 n0_a + b_1 n1_a) + b_2 n2_a over the corners' vertex normals;
//             s = sqrtf((n_x n_x + n_y n_y) + n_z n_z); the cell is a MISS unless 0 < s < inf; normal = n / s.
//             face mode only: m_r = (T_r0 n_x + T_r1 n_y) + T_r2 n_z on the unit normal, T = job_pose; ray = ((c - K'2) / K'0, (r - K'3)
//             / K'1, 1); the normal is negated iff (m_x ray_x + m_y ray_y) + m_z > 0 (it looks away from the camera)
//
//   meshmaps_vertex_kernel   one thread per (job, vertex): pose, project under K', snap -> {X, Y, 1/z, flag}; the first J threads write
//                            status and zero count, dropped and the job's box
//   meshmaps_box_kernel      one thread per (job, face): the drop rules and the cell box of the snapped triangle; per workgroup one
//                            integer min / max into the job's box and one add into dropped
//   meshmaps_tile_kernel     grid (J, T): workgroup (j, k) takes the 16 x 16 tiles k, k + T, ... of the WHOLE h x w grid, one cell per
//                            lane.  A tile that meets the job's box walks the triangle list through raster.h's records (40 968 bytes of
//                            LDS a workgroup: three workgroups a CU); any other tile bins nothing.  The winner is resolved once per lane,
//                            after the flush: three int4 records and three corners gathered through the cache.  Every cell of every
//                            job is written -- a tile row's 16 cells are 192 contiguous bytes of vertex -- and the hits are counted
//                            by wave ballots into one integer atomic per wave.  The job's pose, intrinsics and window are indexed by
//                            blockIdx.x alone and read before the first store: scalar loads.
//
// Integer add / min / max are the only atomics, on words the vertex pass zeroes: two calls give identical bytes, and a job's bytes do
// not depend on its neighbours.
#include "raster.h"

// the window's camera K' from the frame's K (fx, fy, cx, cy) and the window (u0, v0, du, dv)
__device__ __forceinline__ void meshmaps_camera(const float *K, const float *win, float *Kp)
{
    Kp[0] = K[0] / win[2];
    Kp[1] = K[1] / win[3];
    Kp[2] = (K[2] - win[0]) / win[2];
    Kp[3] = (K[3] - win[1]) / win[3];
}

__global__ __launch_bounds__(256) void meshmaps_vertex_kernel(const tgp_mesh_maps_args a, int blocks_per_job)
{
    // the accumulators of this call: the first threads of the grid (it has at least 256 J threads)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    int img;
    RasterMesh m;
    if (gid < (size_t)a.J) {
        a.status[gid] = raster_job(a, (int)gid, img, m) ? 0 : 1;
        a.count[gid] = 0;
        a.dropped[gid] = 0;
        int *jb = raster_workspace(a, a.J).unit_box(gid);
        jb[0] = jb[1] = 0x7fffffff;
        jb[2] = jb[3] = -1;
    }
    const int j = blockIdx.x / blocks_per_job;
    const int v = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    if (j >= a.J || !raster_job(a, j, img, m) || v >= m.nv) return;
    float Kp[4];
    meshmaps_camera(a.camk + (size_t)img * 4, a.job_window + (size_t)j * 4, Kp);
    raster_workspace(a, a.J).vrec(j)[v] = raster_vertex(a.verts + (size_t)(m.vbase + v) * 3, a.job_pose + (size_t)j * 12, Kp, a.near);
}

__global__ __launch_bounds__(256) void meshmaps_box_kernel(const tgp_mesh_maps_args a, int blocks_per_job)
{
    const int j = blockIdx.x / blocks_per_job;
    const int t = (blockIdx.x % blocks_per_job) * 256 + threadIdx.x;
    int img;
    RasterMesh m;
    if (j >= a.J || !raster_job(a, j, img, m)) return; // the same for every lane
    const RasterWorkspace ws = raster_workspace(a, a.J);
    short4 box = make_short4(0x7fff, -1, 0x7fff, -1);
    const int rule = t < m.nf ? raster_face_box(a.faces, m, t, ws.vrec(j), a.w, a.h, ws.boxes(j), box) : 0;
    raster_box_reduce(rule, box, ws.unit_box(j), a.dropped + j);
}

struct MeshMapsCell {
    float z, v[3], n[3];
    int face;
};

// the winner `key` of cell (r, c) = (py, px) of job j -> its surface point and normal; false: a miss (the model-frame normal has no
// length).  The arithmetic is stated at the head of this file.
__device__ __forceinline__ bool meshmaps_resolve(const tgp_mesh_maps_args &a, const RasterMesh &m, const int4 *vr, const float *T,
                                                 const float *Kp, unsigned long long key, int px, int py, MeshMapsCell &o)
{
    const int f = (int)(uint32_t)key;
    const int32_t *fp = a.faces + (size_t)(m.fbase + f) * 3;
    int i0 = fp[0], i1 = fp[1], i2 = fp[2]; // inside the mesh: raster_face_box gave any other face an empty box
    const int4 v0 = vr[i0];
    int4 v1 = vr[i1], v2 = vr[i2];
    long long area = raster_orient(v0.x, v0.y, v1.x, v1.y, v2.x, v2.y);
    if (area < 0) {
        const int4 tmp = v1;
        v1 = v2, v2 = tmp;
        const int ti = i1;
        i1 = i2, i2 = ti;
        area = -area;
    }
    const int sx = px * 256, sy = py * 256;
    const long long e0 = raster_orient(v1.x, v1.y, v2.x, v2.y, sx, sy);
    const long long e1 = raster_orient(v2.x, v2.y, v0.x, v0.y, sx, sy);
    const long long e2 = raster_orient(v0.x, v0.y, v1.x, v1.y, sx, sy);
    const float fa = (float)area;
    const float w0 = (float)e0 / fa, w1 = (float)e1 / fa, w2 = (float)e2 / fa;
    const float z = __uint_as_float((uint32_t)(key >> 32));
    const float b0 = (w0 * __int_as_float(v0.z)) * z, b1 = (w1 * __int_as_float(v1.z)) * z, b2 = (w2 * __int_as_float(v2.z)) * z;
    const float *p0 = a.verts + (size_t)(m.vbase + i0) * 3, *p1 = a.verts + (size_t)(m.vbase + i1) * 3,
                *p2 = a.verts + (size_t)(m.vbase + i2) * 3;
    const float p0x = p0[0], p0y = p0[1], p0z = p0[2], p1x = p1[0], p1y = p1[1], p1z = p1[2], p2x = p2[0], p2y = p2[1], p2z = p2[2];
    float nx, ny, nz;
    if (a.vnormals) {
        const float *n0 = a.vnormals + (size_t)(m.vbase + i0) * 3, *n1 = a.vnormals + (size_t)(m.vbase + i1) * 3,
                    *n2 = a.vnormals + (size_t)(m.vbase + i2) * 3;
        nx = (b0 * n0[0] + b1 * n1[0]) + b2 * n2[0];
        ny = (b0 * n0[1] + b1 * n1[1]) + b2 * n2[1];
        nz = (b0 * n0[2] + b1 * n1[2]) + b2 * n2[2];
    } else {
        const float ux = p1x - p0x, uy = p1y - p0y, uz = p1z - p0z, wx = p2x - p0x, wy = p2y - p0y, wz = p2z - p0z;
        nx = uy * wz - uz * wy;
        ny = uz * wx - ux * wz;
        nz = ux * wy - uy * wx;
    }
    const float s = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!(s > 0.f && s < __builtin_inff())) return false; // a NaN too
    nx = nx / s, ny = ny / s, nz = nz / s;
    if (!a.vnormals) {
        const float mx = (T[0] * nx + T[1] * ny) + T[2] * nz;
        const float my = (T[4] * nx + T[5] * ny) + T[6] * nz;
        const float mz = (T[8] * nx + T[9] * ny) + T[10] * nz;
        const float rx = ((float)px - Kp[2]) / Kp[0], ry = ((float)py - Kp[3]) / Kp[1];
        if ((mx * rx + my * ry) + mz > 0.f) nx = -nx, ny = -ny, nz = -nz;
    }
    o.z = z;
    o.v[0] = (b0 * p0x + b1 * p1x) + b2 * p2x;
    o.v[1] = (b0 * p0y + b1 * p1y) + b2 * p2y;
    o.v[2] = (b0 * p0z + b1 * p1z) + b2 * p2z;
    o.n[0] = nx, o.n[1] = ny, o.n[2] = nz;
    o.face = f;
    return true;
}

__global__ __launch_bounds__(RASTER_THREADS) void meshmaps_tile_kernel(const tgp_mesh_maps_args a)
{
    __shared__ RasterRec s_rec[RASTER_CAP];
    __shared__ int s_n;

    const int tid = threadIdx.x;
    const int j = blockIdx.x;
    int img;
    RasterMesh m;
    const bool job_ok = raster_job(a, j, img, m); // the same for every lane, as is every branch on it below
    const RasterWorkspace ws = raster_workspace(a, a.J);
    // the job's constants, indexed by blockIdx.x alone
    float T[12], Kp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = a.job_pose[(size_t)j * 12 + k];
    int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = -1, by1 = -1; // a job that renders nothing has the empty box
    if (job_ok) {
        meshmaps_camera(a.camk + (size_t)img * 4, a.job_window + (size_t)j * 4, Kp);
        const int *jb = ws.unit_box(j);
        bx0 = jb[0], by0 = jb[1], bx1 = jb[2], by1 = jb[3]; // inside the grid: every triangle's box is
    }
    const int ntx = (a.w + RASTER_TILE - 1) / RASTER_TILE, ntiles = ntx * ((a.h + RASTER_TILE - 1) / RASTER_TILE); // at most 2^20
    const int li = tid % RASTER_TILE, lj = tid / RASTER_TILE;
    const size_t cells = (size_t)a.h * a.w;
    float *zmap = a.z + (size_t)j * cells, *vmap = a.vertex + (size_t)j * cells * 3, *nmap = a.normal + (size_t)j * cells * 3;
    uint16_t *dmap = a.depth + (size_t)j * cells;
    int32_t *fmap = a.face ? a.face + (size_t)j * cells : nullptr;
    int hits = 0; // of this lane's wave: the same in each of its lanes

    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int tx0 = (tile % ntx) * RASTER_TILE, ty0 = (tile / ntx) * RASTER_TILE;
        const int tx1 = min(tx0 + RASTER_TILE - 1, a.w - 1), ty1 = min(ty0 + RASTER_TILE - 1, a.h - 1);
        unsigned long long key = ~0ull;
        if (bx0 <= tx1 && bx1 >= tx0 && by0 <= ty1 && by1 >= ty0) { // false for the empty box
            raster_reset(s_n);
            raster_bin(s_rec, s_n, ws.boxes(j), ws.vrec(j), a.faces, m.fbase, m.nf, tx0, ty0, tx1, ty1, 0u, li, lj, key);
            raster_flush(s_rec, s_n, li, lj, key);
        }
        const int px = tx0 + li, py = ty0 + lj;
        const bool mine = px < a.w && py < a.h;
        MeshMapsCell o;
        o.z = 0.f, o.v[0] = o.v[1] = o.v[2] = 0.f, o.n[0] = o.n[1] = o.n[2] = 0.f, o.face = -1;
        bool hit = false;
        if (mine && key != ~0ull) {
            MeshMapsCell got;
            hit = meshmaps_resolve(a, m, ws.vrec(j), T, Kp, key, px, py, got);
            if (hit) o = got;
        }
        if (mine) {
            const size_t cell = (size_t)py * a.w + px;
            zmap[cell] = o.z;
            dmap[cell] = (uint16_t)raster_depth_mm(o.z);
            vmap[cell * 3] = o.v[0], vmap[cell * 3 + 1] = o.v[1], vmap[cell * 3 + 2] = o.v[2];
            nmap[cell * 3] = o.n[0], nmap[cell * 3 + 1] = o.n[1], nmap[cell * 3 + 2] = o.n[2];
            if (fmap) fmap[cell] = o.face;
        }
        hits += __popcll(__ballot(hit));
    }
    if ((tid & (TGP_WAVE - 1)) == 0 && hits) atomicAdd(a.count + j, hits);
}

extern "C" int64_t tgp_mesh_maps_workspace_bytes(int J, int max_verts, int max_faces)
{
    if (J < 0 || max_verts < 1 || max_faces < 1) return TGP_EINVAL;
    if (J > TGP_MAPS_MAX_JOBS || max_faces >= tgp_render_max_faces()) return TGP_EUNSUPPORTED;
    return raster_workspace_bytes(J, max_verts, max_faces);
}

extern "C" int tgp_mesh_maps(const tgp_mesh_maps_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_mesh_maps_args &a = *args;
    TGP_REQUIRE(a.camk && a.verts && a.faces && a.vptr && a.fptr);
    TGP_REQUIRE(a.M > 0 && a.n_verts > 0 && a.n_faces > 0 && a.max_verts > 0 && a.max_faces > 0);
    TGP_REQUIRE(a.S > 0 && a.h > 0 && a.w > 0 && a.J >= 0);
    TGP_REQUIRE(a.near > 0.f && a.near < __builtin_inff());
    if (a.J > 0)
        TGP_REQUIRE(a.job_img && a.job_mesh && a.job_pose && a.job_window && a.z && a.depth && a.vertex && a.normal && a.count && a.dropped &&
                    a.status && a.workspace);
    if (a.J > TGP_MAPS_MAX_JOBS || a.h > TGP_RAYCAST_MAX_SIDE || a.w > TGP_RAYCAST_MAX_SIDE || !raster_side_ok(a.h, a.w) ||
        a.max_faces >= tgp_render_max_faces())
        return TGP_EUNSUPPORTED;
    if (a.J == 0) return 0;
    TGP_REQUIRE(a.workspace_bytes >= tgp_mesh_maps_workspace_bytes(a.J, a.max_verts, a.max_faces));
    RasterJobLaunch l;
    if (!raster_job_launch(a.J, a.J, a.h, a.w, a.max_verts, a.max_faces, l)) return TGP_EUNSUPPORTED;
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(meshmaps_vertex_kernel, dim3(l.grid_v), dim3(256), 0, st, a, l.vblocks);
    hipLaunchKernelGGL(meshmaps_box_kernel, dim3(l.grid_f), dim3(256), 0, st, a, l.fblocks);
    hipLaunchKernelGGL(meshmaps_tile_kernel, dim3((unsigned)a.J, l.T), dim3(RASTER_THREADS), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
