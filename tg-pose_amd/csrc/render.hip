// Depth renderer: a z-buffer rasteriser of posed triangle meshes, S scenes per call (include/tgpose.h, DESIGN.md section 3 "The
// depth renderer").  Every rule below is the contract tests/render_ref.py restates in numpy; the two agree bit for bit.
//
//   render_vertex_kernel   one thread per (instance, vertex): pose, project, snap to 1/256 px -> {X, Y, 1/z, flag} (16 bytes)
//   render_box_kernel      one thread per (instance, face): the drop rules and the pixel box of the snapped triangle (8 bytes)
//   render_tile_kernel     one workgroup per 16 x 16 screen tile, one pixel per lane with its 64-bit key {z bits, slot, face} in a
//                          register.  The tile walks its scene's boxes 256 at a time; a lane whose box meets the tile sets the
//                          triangle up into an LDS record; when the record list could overflow with the next chunk (and at the
//                          end) every lane runs the list against its pixel.  No list has a capacity a scene can exceed, no
//                          global atomic orders a pixel's winner, and the tile leaves once.
//   render_bbox_kernel     one thread per instance: the min / max accumulators -> (y1, x1, y2, x2)
//
// Integer add / min / max (visible, bbox, dropped) are the only atomics: order-independent, so two calls give identical bytes.
// The per-vertex, per-triangle and per-record arithmetic is raster.h's, shared with pose verification (verify.hip).
#include "raster.h"

#define RENDER_MAX_FACES (1 << 24)
#define RENDER_MAX_INSTANCES 255
#define RENDER_MAX_SIDE 16384
#define RENDER_TILE RASTER_TILE
#define RENDER_THREADS RASTER_THREADS
#define RENDER_CAP RASTER_CAP

struct RenderMesh {
    int vbase, nv, fbase, nf;
};

// the mesh of an instance, cut to the arrays and to the host's bounds; false: it renders nothing
__device__ __forceinline__ bool render_mesh(const tgp_render_args &a, int inst, RenderMesh &m)
{
    const int mesh = a.inst_mesh[inst];
    if (mesh < 0 || mesh >= a.M) return false;
    m.vbase = a.vptr[mesh];
    m.fbase = a.fptr[mesh];
    const long long nv = (long long)a.vptr[mesh + 1] - m.vbase, nf = (long long)a.fptr[mesh + 1] - m.fbase;
    if (m.vbase < 0 || m.fbase < 0 || nv < 1 || nf < 1 || m.vbase + nv > a.n_verts || m.fbase + nf > a.n_faces) return false;
    m.nv = (int)min(nv, (long long)a.max_verts);
    m.nf = (int)min(nf, (long long)a.max_faces);
    return true;
}

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

__device__ __forceinline__ int4 *render_vrec(const tgp_render_args &a) { return (int4 *)a.workspace; }
__device__ __forceinline__ short4 *render_boxes(const tgp_render_args &a)
{
    return (short4 *)((char *)a.workspace + (size_t)a.I * a.max_verts * sizeof(int4));
}
__device__ __forceinline__ int *render_bbacc(const tgp_render_args &a)
{
    return (int *)((char *)a.workspace + (size_t)a.I * a.max_verts * sizeof(int4) + (size_t)a.I * a.max_faces * sizeof(short4));
}

__global__ __launch_bounds__(256) void render_vertex_kernel(const tgp_render_args a, int blocks_per_inst)
{
    // the accumulators of this call: the first threads of the grid (it always has at least max(I, 2 S) threads)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < (size_t)a.I) {
        a.visible[gid] = 0;
        int *bb = render_bbacc(a) + gid * 4;
        bb[0] = bb[1] = 0x7fffffff;
        bb[2] = bb[3] = -1;
    }
    if (gid < (size_t)a.S * 2) a.dropped[gid] = 0;
    if (a.I == 0) return;
    const int inst = blockIdx.x / blocks_per_inst;
    const int v = (blockIdx.x % blocks_per_inst) * 256 + threadIdx.x;
    if (inst >= a.I) return;
    RenderMesh m;
    if (!render_mesh(a, inst, m) || v >= m.nv) return;
    render_vrec(a)[(size_t)inst * a.max_verts + v] = raster_vertex(a.verts + (size_t)(m.vbase + v) * 3, a.inst_pose + (size_t)inst * 12,
                                                                    a.camk + (size_t)render_scene_of(a, inst) * 4, a.near);
}

__global__ __launch_bounds__(256) void render_box_kernel(const tgp_render_args a, int blocks_per_inst)
{
    const int inst = blockIdx.x / blocks_per_inst;
    const int t = (blockIdx.x % blocks_per_inst) * 256 + threadIdx.x;
    RenderMesh m;
    if (inst >= a.I || !render_mesh(a, inst, m) || t >= m.nf) return;
    const int32_t *f = a.faces + (size_t)(m.fbase + t) * 3;
    const int f0 = f[0], f1 = f[1], f2 = f[2];
    short4 box = make_short4(0x7fff, -1, 0x7fff, -1); // x first, x last, y first, y last: empty, it meets no tile
    if (f0 >= 0 && f0 < m.nv && f1 >= 0 && f1 < m.nv && f2 >= 0 && f2 < m.nv) {
        const int4 *vr = render_vrec(a) + (size_t)inst * a.max_verts;
        const int rule = raster_box(vr[f0], vr[f1], vr[f2], a.W, a.H, box);
        if (rule) atomicAdd(a.dropped + (size_t)render_scene_of(a, inst) * 2 + (rule - 1), 1);
    }
    render_boxes(a)[(size_t)inst * a.max_faces + t] = box;
}

__global__ __launch_bounds__(RENDER_THREADS) void render_tile_kernel(const tgp_render_args a, int tiles_x, int tiles_y)
{
    __shared__ RasterRec s_rec[RENDER_CAP];
    __shared__ int s_n;
    __shared__ int s_vis[RENDER_MAX_INSTANCES + 1];
    __shared__ int s_bb[RENDER_MAX_INSTANCES + 1][4];

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int tx0 = (tile % tiles_x) * RENDER_TILE, ty0 = (tile / tiles_x) * RENDER_TILE;
    const int tx1 = min(tx0 + RENDER_TILE, a.W) - 1, ty1 = min(ty0 + RENDER_TILE, a.H) - 1;
    const int li = tid % RENDER_TILE, lj = tid / RENDER_TILE;

    const int s0 = min(max(a.scene_ptr[s], 0), a.I);
    const int s1 = min(max(a.scene_ptr[s + 1], s0), min(a.I, s0 + min(a.max_scene_inst, RENDER_MAX_INSTANCES)));
    const int ninst = s1 - s0;

    if (tid == 0) s_n = 0;
    for (int k = tid; k < ninst; k += RENDER_THREADS) {
        s_vis[k] = 0;
        s_bb[k][0] = s_bb[k][1] = 0x7fffffff;
        s_bb[k][2] = s_bb[k][3] = -1;
    }
    __syncthreads();

    unsigned long long key = ~0ull;

    auto sweep = [&](int n) { raster_sweep(s_rec, n, li, lj, key); };

    for (int slot = 0; slot < ninst; ++slot) {
        const int inst = s0 + slot;
        RenderMesh m;
        if (!render_mesh(a, inst, m)) continue; // the same for every lane
        const short4 *boxes = render_boxes(a) + (size_t)inst * a.max_faces;
        const int4 *vr = render_vrec(a) + (size_t)inst * a.max_verts;
        for (int base = 0; base < m.nf; base += RENDER_THREADS) {
            const int t = base + tid;
            if (t < m.nf) {
                const short4 b = boxes[t];
                if (b.x <= tx1 && b.y >= tx0 && b.z <= ty1 && b.w >= ty0) { // false for an empty box
                    const int32_t *f = a.faces + (size_t)(m.fbase + t) * 3;
                    // at most RENDER_CAP - 256 records held + 256 of this chunk
                    raster_setup(s_rec[atomicAdd(&s_n, 1)], vr[f[0]], vr[f[1]], vr[f[2]], tx0, ty0, ((uint32_t)slot << 24) | (uint32_t)t);
                }
            }
            __syncthreads();
            const int n = s_n;
            __syncthreads(); // every lane has read s_n before a lane of the next chunk adds to it
            if (n > RENDER_CAP - RENDER_THREADS) {
                sweep(n);
                __syncthreads();
                if (tid == 0) s_n = 0;
                __syncthreads();
            }
        }
    }
    sweep(s_n); // the last barrier above is behind every write of s_n and s_rec

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
    for (int k = tid; k < ninst; k += RENDER_THREADS) {
        if (s_vis[k] > 0) {
            atomicAdd(a.visible + s0 + k, s_vis[k]);
            int *bb = render_bbacc(a) + (size_t)(s0 + k) * 4;
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
    const int *bb = render_bbacc(a) + (size_t)i * 4;
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
    return (int64_t)I * max_verts * (int64_t)sizeof(int4) + (int64_t)I * max_faces * (int64_t)sizeof(short4) + (int64_t)I * 16 + 16;
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
    if (a.max_faces >= RENDER_MAX_FACES || a.max_scene_inst > RENDER_MAX_INSTANCES || a.H > RENDER_MAX_SIDE || a.W > RENDER_MAX_SIDE)
        return TGP_EUNSUPPORTED;
    const int tiles_x = tgp_cdiv(a.W, RENDER_TILE), tiles_y = tgp_cdiv(a.H, RENDER_TILE);
    const int64_t vblocks = tgp_cdiv(a.max_verts, 256), fblocks = tgp_cdiv(a.max_faces, 256);
    const int64_t init_blocks = tgp_cdiv((int64_t)a.S * 2 > a.I ? (int64_t)a.S * 2 : a.I, 256);
    const int64_t grid_v = a.I * vblocks > init_blocks ? a.I * vblocks : init_blocks;
    const int64_t grid_f = a.I * fblocks, grid_t = (int64_t)tiles_x * tiles_y * a.S;
    if (grid_v > 0x7fffffff || grid_f > 0x7fffffff || grid_t > 0x7fffffff) return TGP_EUNSUPPORTED;
    hipStream_t st = tgp_hs(stream);
    hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)grid_v), dim3(256), 0, st, a, (int)vblocks);
    if (a.I > 0) hipLaunchKernelGGL(render_box_kernel, dim3((unsigned)grid_f), dim3(256), 0, st, a, (int)fblocks);
    hipLaunchKernelGGL(render_tile_kernel, dim3((unsigned)grid_t), dim3(RENDER_THREADS), 0, st, a, tiles_x, tiles_y);
    if (a.I > 0) hipLaunchKernelGGL(render_bbox_kernel, dim3(tgp_cdiv(a.I, 256)), dim3(256), 0, st, a);
    return TGP_LAUNCH_RESULT();
}
