// Depth renderer: a z-buffer rasteriser of posed triangle meshes, S scenes per call (include/tgpose.h, DESIGN.md section 3 "The
// depth renderer").  Every rule below is the contract tests/render_ref.py restates in numpy; the two agree bit for bit.
//
//   render_vertex_kernel   one thread per (instance, vertex): pose, project, snap to 1/256 px -> {X, Y, 1/z, flag} (16 bytes)
//   render_box_kernel      one thread per (instance, face): the drop rules and the pixel box of the snapped triangle (8 bytes)
//   render_tile_kernel     one workgroup per 16 x 16 screen tile, one pixel per lane with its 64-bit key {z bits, slot, face} in a
//                          register.  The tile walks its scene's instance slots through raster.h's tile walk: one record list that
//                          carries over from slot to slot, swept when the next chunk of 256 boxes could overflow it and once after
//                          the last slot.  No list has a capacity a scene can exceed, no global atomic orders a pixel's winner,
//                          and the tile leaves once.
//   render_bbox_kernel     one thread per instance: the min / max accumulators -> (y1, x1, y2, x2)
//
// Integer add / min / max (visible, bbox, dropped) are the only atomics: order-independent, so two calls give identical bytes.
// The per-vertex, per-triangle and per-record arithmetic, the mesh decode, the workspace's layout (one unit per instance, the unit's
// four words being the bbox accumulators), a face's box and the tile walk are raster.h's, shared with verify.hip and vsd.hip; the
// scene lookup, the per-slot visibility and bbox, the per-scene dropped counts and the frame stores are this file's.
#include "raster.h"

#define RENDER_MAX_FACES (1 << 24)
#define RENDER_MAX_INSTANCES 255

// the scene whose instance range holds inst (the last s with scene_ptr[s] <= inst), inside [0, S)
__device__ __forceinline__ int render_scene_of(const tgp_render_args &a, int inst)
{
    int lo = 0, hi = a.S; // scene_ptr[lo] <= inst < scene_ptr[hi] where the table is monotone
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.scene_ptr[mid] <= inst) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void render_vertex_kernel(const tgp_render_args a, int blocks_per_inst)
{
    // the accumulators of this call: the first threads of the grid (it always has at least max(I, 2 S) threads)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < (size_t)a.I) {
        a.visible[gid] = 0;
        int *bb = raster_workspace(a, a.I).unit_box(gid);
        bb[0] = bb[1] = 0x7fffffff;
        bb[2] = bb[3] = -1;
    }
    if (gid < (size_t)a.S * 2) a.dropped[gid] = 0;
    if (a.I == 0) return;
    const int inst = blockIdx.x / blocks_per_inst;
    const int v = (blockIdx.x % blocks_per_inst) * 256 + threadIdx.x;
    if (inst >= a.I) return;
    RasterMesh m;
    if (!raster_mesh(a, a.inst_mesh[inst], m) || v >= m.nv) return;
    raster_workspace(a, a.I).vrec(inst)[v] = raster_vertex(a.verts + (size_t)(m.vbase + v) * 3, a.inst_pose + (size_t)inst * 12,
                                               a.camk + (size_t)render_scene_of(a, inst) * 4, a.near);
}

__global__ __launch_bounds__(256) void render_box_kernel(const tgp_render_args a, int blocks_per_inst)
{
    const int inst = blockIdx.x / blocks_per_inst;
    const int t = (blockIdx.x % blocks_per_inst) * 256 + threadIdx.x;
    RasterMesh m;
    if (inst >= a.I || !raster_mesh(a, a.inst_mesh[inst], m) || t >= m.nf) return;
    const RasterWorkspace ws = raster_workspace(a, a.I);
    short4 box;
    const int rule = raster_face_box(a.faces, m, t, ws.vrec(inst), a.W, a.H, ws.boxes(inst), box);
    if (rule) atomicAdd(a.dropped + (size_t)render_scene_of(a, inst) * 2 + (rule - 1), 1);
}

__global__ __launch_bounds__(RASTER_THREADS) void render_tile_kernel(const tgp_render_args a, int tiles_x, int tiles_y)
{
    __shared__ RasterRec s_rec[RASTER_CAP];
    __shared__ int s_n;
    __shared__ int s_vis[RENDER_MAX_INSTANCES + 1];
    __shared__ int s_bb[RENDER_MAX_INSTANCES + 1][4];

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int tx0 = (tile % tiles_x) * RASTER_TILE, ty0 = (tile / tiles_x) * RASTER_TILE;
    const int tx1 = min(tx0 + RASTER_TILE, a.W) - 1, ty1 = min(ty0 + RASTER_TILE, a.H) - 1;
    const int li = tid % RASTER_TILE, lj = tid / RASTER_TILE;

    const int s0 = min(max(a.scene_ptr[s], 0), a.I);
    const int s1 = min(max(a.scene_ptr[s + 1], s0), min(a.I, s0 + min(a.max_scene_inst, RENDER_MAX_INSTANCES)));
    const int ninst = s1 - s0;

    if (tid == 0) s_n = 0;
    for (int k = tid; k < ninst; k += RASTER_THREADS) {
        s_vis[k] = 0;
        s_bb[k][0] = s_bb[k][1] = 0x7fffffff;
        s_bb[k][2] = s_bb[k][3] = -1;
    }
    __syncthreads();

    const RasterWorkspace ws = raster_workspace(a, a.I);
    unsigned long long key = ~0ull;
    for (int slot = 0; slot < ninst; ++slot) { // one list over the slots: a slot's records wait for the next sweep, whichever slot's
        const int inst = s0 + slot;
        RasterMesh m;
        if (!raster_mesh(a, a.inst_mesh[inst], m)) continue; // the same for every lane
        raster_bin(s_rec, s_n, ws.boxes(inst), ws.vrec(inst), a.faces, m.fbase, m.nf, tx0, ty0, tx1, ty1, (uint32_t)slot << 24, li, lj, key);
    }
    raster_flush(s_rec, s_n, li, lj, key);

    const int px = tx0 + li, py = ty0 + lj;
    if (px < a.W && py < a.H) {
        const size_t o = ((size_t)s * a.H + py) * a.W + px;
        if (key == ~0ull) {
            a.depth[o] = 0;
            a.mask[o] = 0;
            if (a.z) a.z[o] = __uint_as_float(0x7f800000u);
            if (a.face) a.face[o] = -1;
        } else {
            const float z = __uint_as_float((uint32_t)(key >> 32));
            const int slot = (int)((uint32_t)key >> 24), face = (int)((uint32_t)key & 0xffffffu);
            a.depth[o] = (uint16_t)raster_depth_mm(z);
            a.mask[o] = a.inst_id[s0 + slot];
            if (a.z) a.z[o] = z;
            if (a.face) a.face[o] = face;
            atomicAdd(&s_vis[slot], 1);
            atomicMin(&s_bb[slot][0], py);
            atomicMin(&s_bb[slot][1], px);
            atomicMax(&s_bb[slot][2], py);
            atomicMax(&s_bb[slot][3], px);
        }
    }
    __syncthreads();
    for (int k = tid; k < ninst; k += RASTER_THREADS) {
        if (s_vis[k] > 0) {
            atomicAdd(a.visible + s0 + k, s_vis[k]);
            int *bb = ws.unit_box(s0 + k);
            atomicMin(bb + 0, s_bb[k][0]);
            atomicMin(bb + 1, s_bb[k][1]);
            atomicMax(bb + 2, s_bb[k][2]);
            atomicMax(bb + 3, s_bb[k][3]);
        }
    }
}

__global__ __launch_bounds__(256) void render_bbox_kernel(const tgp_render_args a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.I) return;
    const int *bb = raster_workspace(a, a.I).unit_box(i);
    const bool seen = a.visible[i] > 0;
    a.bbox[i * 4 + 0] = seen ? bb[0] : 0;
    a.bbox[i * 4 + 1] = seen ? bb[1] : 0;
    a.bbox[i * 4 + 2] = seen ? bb[2] + 1 : 0;
    a.bbox[i * 4 + 3] = seen ? bb[3] + 1 : 0;
}

extern "C" int tgp_render_max_faces(void) { return RENDER_MAX_FACES; }
extern "C" int tgp_render_max_instances(void) { return RENDER_MAX_INSTANCES; }

extern "C" int64_t tgp_render_workspace_bytes(int I, int max_verts, int max_faces)
{
    if (I < 0 || max_verts < 1 || max_faces < 1) return -1;
    return raster_workspace_bytes(I, max_verts, max_faces);
}

extern "C" int tgp_render_depth(const tgp_render_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_render_args &a = *args;
    TGP_REQUIRE(a.verts && a.faces && a.vptr && a.fptr && a.scene_ptr && a.camk && a.workspace);
    TGP_REQUIRE(a.depth && a.mask && a.dropped);
    TGP_REQUIRE(a.M > 0 && a.n_verts > 0 && a.n_faces > 0 && a.max_verts > 0 && a.max_faces > 0);
    TGP_REQUIRE(a.S > 0 && a.I >= 0 && a.max_scene_inst >= 0 && a.H > 0 && a.W > 0);
    TGP_REQUIRE(a.near > 0.f && a.near < __builtin_inff());
    if (a.I > 0) TGP_REQUIRE(a.inst_mesh && a.inst_id && a.inst_pose && a.visible && a.bbox);
    if (a.max_faces >= RENDER_MAX_FACES || a.max_scene_inst > RENDER_MAX_INSTANCES || !raster_side_ok(a.H, a.W))
        return TGP_EUNSUPPORTED;
    const int tiles_x = tgp_cdiv(a.W, RASTER_TILE), tiles_y = tgp_cdiv(a.H, RASTER_TILE);
    const int64_t vblocks = tgp_cdiv(a.max_verts, 256), fblocks = tgp_cdiv(a.max_faces, 256);
    const int64_t init_blocks = tgp_cdiv((int64_t)a.S * 2 > a.I ? (int64_t)a.S * 2 : a.I, 256);
    const int64_t grid_v = a.I * vblocks > init_blocks ? a.I * vblocks : init_blocks;
    const int64_t grid_f = a.I * fblocks, grid_t = (int64_t)tiles_x * tiles_y * a.S;
    if (grid_v > 0x7fffffff || grid_f > 0x7fffffff || grid_t > 0x7fffffff) return TGP_EUNSUPPORTED;
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)grid_v), dim3(256), 0, st, a, (int)vblocks);
    if (a.I > 0) hipLaunchKernelGGL(render_box_kernel, dim3((unsigned)grid_f), dim3(256), 0, st, a, (int)fblocks);
    hipLaunchKernelGGL(render_tile_kernel, dim3((unsigned)grid_t), dim3(RASTER_THREADS), 0, st, a, tiles_x, tiles_y);
    if (a.I > 0) hipLaunchKernelGGL(render_bbox_kernel, dim3(tgp_cdiv(a.I, 256)), dim3(256), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
