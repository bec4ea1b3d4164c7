// The rasteriser, shared by the depth renderer (render.hip), pose verification (verify.hip) and two-pose VSD (vsd.hip): DESIGN.md
// section 3 "The depth renderer" states every rule below and tests/render_ref.py restates them in numpy.  A vertex is posed,
// projected and snapped to 1/256 px; a triangle is dropped by the near rule or the guard band, or gets the pixel box of its snapped
// corners; a tile sets the triangles that meet it up into LDS records at its first sample point and every lane runs the records
// against its own pixel, keeping the smallest 64-bit key {z bits, lo}.  The loops around these steps are here too, once for the
// three files: the decode of a mesh of the set (raster_mesh, raster_job), the workspace's layout (RasterWorkspace), a face's box and
// a workgroup's reduction of its boxes (raster_face_box, raster_box_reduce), the walk of a triangle list through the tile's records
// (raster_reset, raster_bin, raster_flush) and the launch shape of the job kernels (raster_job_launch).  What a kernel does with a
// pixel's winner is its own.
//
// The tile walk's contract.  s_rec[RASTER_CAP] and s_n live in the kernel's LDS; every lane of the workgroup enters each of the
// three calls, in uniform control flow.
//   raster_reset   empties the list: a barrier (every lane is behind the sweep that last read s_n and s_rec), lane 0 writes
//                  s_n = 0, a barrier (no lane adds before the write).  The caller may write s_n = 0 itself where a barrier of
//                  its own follows, as the renderer does at its start.
//   raster_bin     walks one triangle list 256 boxes at a time.  It neither resets s_n nor sweeps on entry: it adds to the records
//                  it finds.  Per chunk: the lanes whose box meets the tile append a record; a barrier (every append is done); every
//                  lane reads n = s_n; a barrier (every lane has read s_n before a lane of the next chunk, or of the next call, adds to
//                  it).  Where n > RASTER_CAP - RASTER_THREADS -- the next chunk could overflow -- every lane sweeps the n records, a
//                  barrier (every lane is done with s_rec), lane 0 writes s_n = 0, a barrier.  So on return s_n <= RASTER_CAP -
//                  RASTER_THREADS, the last barrier is behind every write of s_n and s_rec, and the records not yet swept stay.
//   raster_flush   sweeps what is left; the barrier before it is raster_bin's last one (the reset's, where nothing was binned), and
//                  it leaves none behind it: the caller resets, or is done with the list.
// The renderer resets once, bins every instance slot of its scene -- records carry over from one slot to the next -- and flushes once
// after the last slot; its low word is slot << 24 | face.  Verification and VSD reset before each surface and flush after it; their
// low word is the face.
#ifndef TGP_RASTER_H
#define TGP_RASTER_H
#include "tgp_common.h"

#define RASTER_GUARD 4194304.f // 2^22 sub-pixel units
#define RASTER_TILE 16
#define RASTER_THREADS (RASTER_TILE * RASTER_TILE)
#define RASTER_CAP (2 * RASTER_THREADS) // records held before a raster sweep: one chunk always fits behind a sweep's threshold
#define RASTER_MAX_SIDE 16384           // a frame's side: at 256 units a pixel, the guard band
#define RASTER_MAX_T 1024               // workgroups per job of a job kernel's tile pass

struct RasterRec {
    long long e[3]; // edge functions at the tile's first sample point
    int dx[3], dy[3];
    float iz[3];
    float area;
    uint32_t lo;   // the key's low word: what breaks a tie in z (the renderer: slot << 24 | face)
    uint32_t open; // bit k: edge k is a top or left edge (E_k == 0 is inside)
    int pad[2];
};
static_assert(sizeof(RasterRec) == 80, "RasterRec");

// model vertex p under pose T (3,4) and intrinsics K (fx, fy, cx, cy) -> {X, Y in 1/256 px, bits of 1/z, flag}; flag 1: at or behind
// near, 2: beyond the guard band
__device__ __forceinline__ int4 raster_vertex(const float *p, const float *T, const float *K, float near)
{
    const float x = p[0], y = p[1], z = p[2];
    const float px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const float py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const float pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    int4 r = make_int4(0, 0, 0, 1);
    if (pz > near) { // false for a NaN too
        const float u = (K[0] * (px / pz) + K[2]) * 256.f;
        const float w = (K[1] * (py / pz) + K[3]) * 256.f;
        if (fabsf(u) <= RASTER_GUARD && fabsf(w) <= RASTER_GUARD) // false for a NaN too
            r = make_int4((int)rintf(u), (int)rintf(w), __float_as_int(1.f / pz), 0);
        else
            r.w = 2;
    }
    return r;
}

__device__ __forceinline__ long long raster_orient(int ax, int ay, int bx, int by, int cx, int cy)
{
    return (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
}

// the drop rules and the pixel box (x first, x last, y first, y last) of a snapped triangle in a W x H frame.  -> 1: dropped by the
// near rule, 2: by the guard band, 0 otherwise; the box is empty (it meets no tile) unless the triangle can cover a sample
__device__ __forceinline__ int raster_box(const int4 v0, const int4 v1, const int4 v2, int W, int H, short4 &box)
{
    box = make_short4(0x7fff, -1, 0x7fff, -1);
    if (v0.w == 1 || v1.w == 1 || v2.w == 1) return 1;
    if (v0.w | v1.w | v2.w) return 2;
    if (raster_orient(v0.x, v0.y, v1.x, v1.y, v2.x, v2.y) != 0) {
        // samples sit at multiples of 256: the first at or after the least coordinate, the last at or before the greatest
        const int x0 = max((min(min(v0.x, v1.x), v2.x) + 255) >> 8, 0), x1 = min(max(max(v0.x, v1.x), v2.x) >> 8, W - 1);
        const int y0 = max((min(min(v0.y, v1.y), v2.y) + 255) >> 8, 0), y1 = min(max(max(v0.y, v1.y), v2.y) >> 8, H - 1);
        if (x0 <= x1 && y0 <= y1) box = make_short4((short)x0, (short)x1, (short)y0, (short)y1);
    }
    return 0;
}

// the record of triangle (v0, v1, v2) for the tile whose first sample is pixel (tx0, ty0)
__device__ __forceinline__ void raster_setup(RasterRec &q, const int4 v0, int4 v1, int4 v2, int tx0, int ty0, uint32_t lo)
{
    long long area = raster_orient(v0.x, v0.y, v1.x, v1.y, v2.x, v2.y);
    if (area < 0) { // both windings render: the second and third vertex change places
        const int4 tmp = v1;
        v1 = v2, v2 = tmp;
        area = -area;
    }
    const int ox = tx0 * 256, oy = ty0 * 256;
    q.e[0] = raster_orient(v1.x, v1.y, v2.x, v2.y, ox, oy);
    q.e[1] = raster_orient(v2.x, v2.y, v0.x, v0.y, ox, oy);
    q.e[2] = raster_orient(v0.x, v0.y, v1.x, v1.y, ox, oy);
    q.dx[0] = v2.x - v1.x, q.dy[0] = v2.y - v1.y;
    q.dx[1] = v0.x - v2.x, q.dy[1] = v0.y - v2.y;
    q.dx[2] = v1.x - v0.x, q.dy[2] = v1.y - v0.y;
    uint32_t open = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (q.dy[k] < 0 || (q.dy[k] == 0 && q.dx[k] > 0)) open |= 1u << k;
    q.open = open;
    q.iz[0] = __int_as_float(v0.z), q.iz[1] = __int_as_float(v1.z), q.iz[2] = __int_as_float(v2.z);
    q.area = (float)area;
    q.lo = lo;
}

// n records against the pixel (li, lj) of their tile: key becomes the smallest {z bits, lo} of the triangles that cover its sample
__device__ __forceinline__ void raster_sweep(const RasterRec *rec, int n, int li, int lj, unsigned long long &key)
{
    for (int r = 0; r < n; ++r) {
        const RasterRec &q = rec[r];
        const long long e0 = q.e[0] + (long long)(lj * q.dx[0] - li * q.dy[0]) * 256;
        const long long e1 = q.e[1] + (long long)(lj * q.dx[1] - li * q.dy[1]) * 256;
        const long long e2 = q.e[2] + (long long)(lj * q.dx[2] - li * q.dy[2]) * 256;
        const uint32_t open = q.open;
        const bool in = (e0 > 0 || (e0 == 0 && (open & 1))) && (e1 > 0 || (e1 == 0 && (open & 2))) && (e2 > 0 || (e2 == 0 && (open & 4)));
        if (in) {
            const float w0 = (float)e0 / q.area, w1 = (float)e1 / q.area, w2 = (float)e2 / q.area;
            const float invz = (w0 * q.iz[0] + w1 * q.iz[1]) + w2 * q.iz[2];
            const float z = 1.f / invz;
            const unsigned long long k64 = ((unsigned long long)__float_as_uint(z) << 32) | q.lo;
            key = min(key, k64);
        }
    }
}

// metres -> the uint16 millimetres of a depth frame, 0 beyond its range
__device__ __forceinline__ int raster_depth_mm(float z)
{
    const float mm = rintf(z * 1000.f);
    return mm <= 65535.f ? (int)mm : 0;
}

struct RasterMesh {
    int vbase, nv, fbase, nf;
};

// mesh `mesh` of a's set, cut to the arrays and to the host's bounds; false: it renders nothing
template <class Args> __device__ __forceinline__ bool raster_mesh(const Args &a, int mesh, RasterMesh &m)
{
    if (mesh < 0 || mesh >= a.M) return false;
    m.vbase = a.vptr[mesh];
    m.fbase = a.fptr[mesh];
    const long long nv = (long long)a.vptr[mesh + 1] - m.vbase, nf = (long long)a.fptr[mesh + 1] - m.fbase;
    if (m.vbase < 0 || m.fbase < 0 || nv < 1 || nf < 1 || m.vbase + nv > a.n_verts || m.fbase + nf > a.n_faces) return false;
    m.nv = (int)min(nv, (long long)a.max_verts);
    m.nf = (int)min(nf, (long long)a.max_faces);
    return true;
}

// the frame and the mesh of job j, the frame checked against the host's S; false: the job's rows stay zero
template <class Args> __device__ __forceinline__ bool raster_job(const Args &a, int j, int &img, RasterMesh &m)
{
    img = a.job_img[j];
    const int mesh = a.job_mesh[j]; // read beside job_img, not behind its check: one load's latency less at the head of every kernel
    return img >= 0 && img < a.S && raster_mesh(a, mesh, m);
}

// the workspace of U units (instances, jobs or pseudo-jobs): U x max_verts vertex records, U x max_faces triangle boxes, then four
// words per unit (first x, first y, last x, last y over the unit's boxes for a job; the renderer's bbox accumulators)
__host__ __device__ inline int64_t raster_workspace_bytes(int64_t U, int max_verts, int max_faces)
{
    return U * max_verts * (int64_t)sizeof(int4) + U * max_faces * (int64_t)sizeof(short4) + U * 16 + 16;
}

struct RasterWorkspace {
    int4 *v;
    short4 *b;
    int *ub;
    int max_verts, max_faces;
    __device__ __forceinline__ RasterWorkspace(void *workspace, int64_t U, int max_verts, int max_faces)
        : v((int4 *)workspace), b((short4 *)(v + U * max_verts)), ub((int *)(b + U * max_faces)), max_verts(max_verts), max_faces(max_faces)
    {
    }
    __device__ __forceinline__ int4 *vrec(size_t u) const { return v + u * max_verts; }
    __device__ __forceinline__ short4 *boxes(size_t u) const { return b + u * max_faces; }
    __device__ __forceinline__ int *unit_box(size_t u) const { return ub + u * 4; }
};
template <class Args> __device__ __forceinline__ RasterWorkspace raster_workspace(const Args &a, int64_t U)
{
    return RasterWorkspace(a.workspace, U, a.max_verts, a.max_faces);
}

// face t of mesh m: its corners checked against the mesh, its box from the vertex records vr into boxes[t] (empty where a corner is
// outside the mesh or the triangle is dropped).  -> raster_box's rule
__device__ __forceinline__ int raster_face_box(const int32_t *faces, const RasterMesh &m, int t, const int4 *vr, int W, int H, short4 *boxes,
                                               short4 &box)
{
    const int32_t *f = faces + (size_t)(m.fbase + t) * 3;
    const int f0 = f[0], f1 = f[1], f2 = f[2];
    box = make_short4(0x7fff, -1, 0x7fff, -1); // x first, x last, y first, y last: empty, it meets no tile
    int rule = 0;
    if (f0 >= 0 && f0 < m.nv && f1 >= 0 && f1 < m.nv && f2 >= 0 && f2 < m.nv) rule = raster_box(vr[f0], vr[f1], vr[f2], W, H, box);
    boxes[t] = box;
    return rule;
}

// a workgroup's faces into their unit's box and dropped count: min / max / add in LDS, then one global atomic per class.  Entered by
// every lane with raster_face_box's rule and box, a lane without a face with rule 0 and an empty box
__device__ __forceinline__ void raster_box_reduce(int rule, const short4 box, int *unit_box, int32_t *dropped)
{
    __shared__ int s_bb[4];
    __shared__ int s_drop;
    if (threadIdx.x == 0) {
        s_bb[0] = s_bb[1] = 0x7fffffff;
        s_bb[2] = s_bb[3] = -1;
        s_drop = 0;
    }
    __syncthreads();
    if (rule) { // the near rule or the guard band
        atomicAdd(&s_drop, 1);
    } else if (box.x <= box.y) {
        atomicMin(&s_bb[0], (int)box.x);
        atomicMin(&s_bb[1], (int)box.z);
        atomicMax(&s_bb[2], (int)box.y);
        atomicMax(&s_bb[3], (int)box.w);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_drop) atomicAdd(dropped, s_drop);
        if (s_bb[2] >= 0) {
            atomicMin(unit_box + 0, s_bb[0]);
            atomicMin(unit_box + 1, s_bb[1]);
            atomicMax(unit_box + 2, s_bb[2]);
            atomicMax(unit_box + 3, s_bb[3]);
        }
    }
}

// the tile walk: the contract is at the head of this file
__device__ __forceinline__ void raster_reset(int &s_n)
{
    __syncthreads();
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
}

// the nf triangles faces[fbase ..] with their boxes and vertex records, against the tile of pixels [tx0, tx1] x [ty0, ty1] whose
// first sample is (tx0, ty0); a record's low word is lo_high | face; (li, lj) is the lane's pixel in the tile
__device__ __forceinline__ void raster_bin(RasterRec *s_rec, int &s_n, const short4 *boxes, const int4 *vr, const int32_t *faces, int fbase,
                                           int nf, int tx0, int ty0, int tx1, int ty1, uint32_t lo_high, int li, int lj,
                                           unsigned long long &key)
{
    for (int base = 0; base < nf; base += RASTER_THREADS) {
        const int t = base + threadIdx.x;
        if (t < nf) {
            const short4 b = boxes[t];
            if (b.x <= tx1 && b.y >= tx0 && b.z <= ty1 && b.w >= ty0) { // false for an empty box
                const int32_t *f = faces + (size_t)(fbase + t) * 3;
                // at most RASTER_CAP - 256 records held + 256 of this chunk
                raster_setup(s_rec[atomicAdd(&s_n, 1)], vr[f[0]], vr[f[1]], vr[f[2]], tx0, ty0, lo_high | (uint32_t)t);
            }
        }
        __syncthreads();
        const int n = s_n;
        __syncthreads();
        if (n > RASTER_CAP - RASTER_THREADS) {
            raster_sweep(s_rec, n, li, lj, key);
            __syncthreads();
            if (threadIdx.x == 0) s_n = 0;
            __syncthreads();
        }
    }
}

__device__ __forceinline__ void raster_flush(const RasterRec *s_rec, const int &s_n, int li, int lj, unsigned long long &key)
{
    raster_sweep(s_rec, s_n, li, lj, key);
}

// The launch shape of a job kernel (verification, VSD) over U units of J jobs: blocks of 256 per unit for the vertex and the box
// pass, and T workgroups per job for the tile pass -- enough that a few jobs fill the device, few enough that many jobs do not flood
// it with workgroups that find no tile; never more than the frame has tiles.  false: a grid would overflow
struct RasterJobLaunch {
    int vblocks, fblocks;
    unsigned grid_v, grid_f, T;
};
static inline bool raster_side_ok(int H, int W) { return H <= RASTER_MAX_SIDE && W <= RASTER_MAX_SIDE; }
static inline bool raster_job_launch(int64_t U, int J, int H, int W, int max_verts, int max_faces, RasterJobLaunch &l)
{
    l.vblocks = tgp_cdiv(max_verts, 256), l.fblocks = tgp_cdiv(max_faces, 256);
    const int64_t grid_v = U * l.vblocks, grid_f = U * l.fblocks;
    if (grid_v > 0x7fffffff || grid_f > 0x7fffffff) return false;
    const int64_t frame_tiles = (int64_t)tgp_cdiv(W, RASTER_TILE) * tgp_cdiv(H, RASTER_TILE);
    int64_t T = 4096 / J;
    T = T < 16 ? 16 : T > RASTER_MAX_T ? RASTER_MAX_T : T;
    l.grid_v = (unsigned)grid_v, l.grid_f = (unsigned)grid_f, l.T = (unsigned)(T > frame_tiles ? frame_tiles : T);
    return true;
}

#endif
