// Indexed meshes from volumes: the marching-tetrahedra surface of a TSDF volume welded into shared vertices, and area-weighted
// vertex normals of any packed mesh set (include/tgpose.h, DESIGN.md section 3 "Indexed meshes from volumes"; tests/weld_ref.py
// restates every kernel in NumPy, bit for bit).
//
// A vertex of the surface is a function of one voxel edge, and a voxel edge has an integer name: key = flat(A) * 8 + d, A the edge's
// componentwise smaller end and d = dx << 2 | dy << 1 | dz in 1..7 the step to the other end.  Welding is a bit mask per voxel, a
// prefix sum and a rank -- no float is hashed or sorted:
//   weld_mark_kernel     one thread per voxel A: bit d of mask[A] iff the edge (A, d) changes sign and lies in a cube that meshes
//   weld_count_kernel    one thread per cube: its triangles whose three vertices lie below vert_cap
//   weld_verts_kernel    one thread per voxel A: its vertices at their rank, with tsdf_emit_kernel's arithmetic (tsdf_cells.h)
//   weld_faces_kernel    one thread per cube: its triangles' vertex indices at the cube's offset, tsdf_emit_kernel's order
//   weld_cluster_kernel  one thread per voxel A: its vertices' cell, and their quantised offsets summed into the cell (int64 atomics)
//   normals_face_kernel  one thread per face: the float32 cross product, quantised, added to its three vertices (int64 atomics:
//                        integer sums are the same in any order)
//   normals_unit_kernel  one thread per vertex: the sum normalised in float64, rounded once
// Fixed places and integer sums: two calls give identical bytes.
#include "tgp_common.h"

// tsdf.hip's tables, literal here too (tests/test_weld_cpu.py holds the two copies equal)
// the cube corner (dx << 2 | dy << 1 | dz) of path corner c of tetrahedron k: the axis steps of the k-th permutation of (0, 1, 2)
__device__ static const uint8_t tsdf_path[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
// bit `case` of word k: the triangles swap their second and third vertex (derived by tests/tsdf_ref.py derive_flip; the word of an
// odd permutation is the complement of an even one's over the cases 1..14)
__device__ static const uint16_t tsdf_flip[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
#include "tsdf_cells.h"

#define WELD_THREADS 256

// ---- welding -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WELD_THREADS) void weld_mark_kernel(const tgp_tsdf_weld_args a)
{
    const int G = a.G;
    const size_t cells = (size_t)G * G * G;
    const size_t v = (size_t)blockIdx.x * WELD_THREADS + threadIdx.x;
    if (v >= cells) return;
    const int iz = (int)(v % G), iy = (int)(v / G % G), ix = (int)(v / G / G);
    const size_t base = (size_t)a.model * cells;
    // seen: bit (x * 3 + y) * 3 + z of the 3 x 3 x 3 voxels about A, A at (1, 1, 1), has weight >= min_weight (and exists)
    uint32_t seen = 0;
    for (int x = 0; x < 3; ++x)
        for (int y = 0; y < 3; ++y)
            for (int z = 0; z < 3; ++z) {
                const int jx = ix + x - 1, jy = iy + y - 1, jz = iz + z - 1;
                if (jx < 0 || jy < 0 || jz < 0 || jx >= G || jy >= G || jz >= G) continue;
                if (a.weight[base + ((size_t)jx * G + jy) * G + jz] >= a.min_weight) seen |= 1u << ((x * 3 + y) * 3 + z);
            }
    // cube: bit o = ox << 2 | oy << 1 | oz iff the cube whose origin is A - (ox, oy, oz) meshes: all eight corners seen (a corner
    // outside the volume is not, which rules out origins below 0 and at G - 1)
    uint32_t cube = 0;
    for (int o = 0; o < 8; ++o) {
        const int x0 = 1 - (o >> 2), y0 = 1 - ((o >> 1) & 1), z0 = 1 - (o & 1);
        uint32_t need = 0;
        for (int k = 0; k < 8; ++k) need |= 1u << (((x0 + (k >> 2)) * 3 + (y0 + ((k >> 1) & 1))) * 3 + (z0 + (k & 1)));
        if ((seen & need) == need) cube |= 1u << o;
    }
    uint32_t mask = 0;
    if (cube) {
        const bool in_a = a.sum[base + v] < 0;
        for (int d = 1; d < 8; ++d) {
            // the cubes that hold both ends: origin A on the axes where d steps, A or A - 1 on the others
            uint32_t holds = 0;
            for (int o = 0; o < 8; ++o)
                if ((o & d) == 0) holds |= 1u << o;
            if (!(cube & holds)) continue; // also: A + d lies in the volume, being a corner of a cube that meshes
            const size_t b = base + ((size_t)(ix + (d >> 2)) * G + (iy + ((d >> 1) & 1))) * G + (iz + (d & 1));
            if ((a.sum[b] < 0) != in_a) mask |= 1u << d;
        }
    }
    a.mask[v] = (uint8_t)mask;
    a.vcounts[v] = __popc(mask);
}

// the index of vertex (A, d): its rank among the volume's vertices in ascending key; only asked of a vertex that exists
__device__ __forceinline__ long long weld_index(const tgp_tsdf_weld_args &a, size_t flat, int d)
{
    const uint32_t m = a.mask[flat];
    return a.voffsets[flat] - __popc(m) + __popc(m & ((1u << d) - 1u));
}

// Walks the triangles of the cube at voxel (ix, iy, iz) in the soup's order -- tetrahedron, then triangle -- and hands each one whose
// three vertex indices lie below vert_cap to emit(index[3]); emit returns false to stop the walk.
template <class Emit>
__device__ __forceinline__ void weld_cube_faces(const tgp_tsdf_weld_args &a, int ix, int iy, int iz, const TsdfCube &c, Emit emit)
{
    const int G = a.G;
    for (int k = 0; k < 6; ++k) {
        const int cs = tsdf_case(c, k);
        const int faces = tsdf_case_faces(cs);
        if (faces == 0) continue;
        int ea[4], eb[4];
        tsdf_case_edges(cs, ea, eb);
        const bool flip = tsdf_flip[k] >> cs & 1;
        for (int t = 0; t < faces; ++t) {
            long long idx[3];
            bool below = true;
            for (int q = 0; q < 3; ++q) {
                const int e = tsdf_face_edge(t, q, flip);
                const int p0 = ea[e], p1 = eb[e];
                const int ka = tsdf_path[k][p0 < p1 ? p0 : p1], kb = tsdf_path[k][p0 < p1 ? p1 : p0]; // ka's bits are among kb's
                const size_t flat = ((size_t)(ix + (ka >> 2)) * G + (iy + ((ka >> 1) & 1))) * G + (iz + (ka & 1));
                idx[q] = weld_index(a, flat, kb ^ ka);
                below = below && idx[q] < a.vert_cap;
            }
            if (below && !emit(idx)) return;
        }
    }
}

__global__ __launch_bounds__(WELD_THREADS) void weld_count_kernel(const tgp_tsdf_weld_args a)
{
    const int G = a.G;
    const size_t v = (size_t)blockIdx.x * WELD_THREADS + threadIdx.x;
    if (v >= (size_t)G * G * G) return;
    const int iz = (int)(v % G), iy = (int)(v / G % G), ix = (int)(v / G / G);
    TsdfCube c;
    int n = 0;
    if (tsdf_cube(a, ix, iy, iz, c))
        weld_cube_faces(a, ix, iy, iz, c, [&](const long long *) {
            ++n;
            return true;
        });
    a.fcounts[v] = n;
}

__global__ __launch_bounds__(WELD_THREADS) void weld_verts_kernel(const tgp_tsdf_weld_args a)
{
    const int G = a.G;
    const size_t cells = (size_t)G * G * G;
    const size_t v = (size_t)blockIdx.x * WELD_THREADS + threadIdx.x;
    if (v >= cells) return;
    const uint32_t m = a.mask[v];
    if (m == 0) return;
    long long n = a.voffsets[v] - __popc(m); // the voxel's first vertex
    if (n >= a.vert_cap) return;
    const int iz = (int)(v % G), iy = (int)(v / G % G), ix = (int)(v / G / G);
    const size_t base = (size_t)a.model * cells;
    const float *meta = a.meta + (size_t)a.model * 4;
    const int sa = a.sum[base + v], wa = a.weight[base + v];
    for (int d = 1; d < 8; ++d) {
        if (!(m >> d & 1)) continue;
        if (n >= a.vert_cap) return;
        const int bx = ix + (d >> 2), by = iy + ((d >> 1) & 1), bz = iz + (d & 1);
        if (bx >= G || by >= G || bz >= G) return; // not with a mask that mark wrote
        const size_t b =base + ((size_t)bx * G + by) * G + bz;
        tsdf_edge_vertex(meta, G, sa, wa, a.sum[b], a.weight[b], ix, iy, iz, bx, by, bz, a.verts + (size_t)n * 3);
        ++n;
    }
}

__global__ __launch_bounds__(WELD_THREADS) void weld_faces_kernel(const tgp_tsdf_weld_args a)
{
    const int G = a.G;
    const size_t cells = (size_t)G * G * G;
    const size_t v = (size_t)blockIdx.x * WELD_THREADS + threadIdx.x;
    if (v >= cells) return;
    if (v == cells - 1) {
        const long long nv = a.voffsets[v], nf = a.foffsets[v];
        a.info[0] = nv < a.vert_cap ? nv : a.vert_cap;
        a.info[1] = nf < a.face_cap ? nf : a.face_cap;
        a.info[2] = (nf > a.face_cap ? 1 : 0) | (nv > a.vert_cap ? 2 : 0);
    }
    const int mine = a.fcounts[v];
    if (mine == 0) return;
    long long n = a.foffsets[v] - mine; // the cube's first triangle
    if (n >= a.face_cap) return;
    const int iz = (int)(v % G), iy = (int)(v / G % G), ix = (int)(v / G / G);
    TsdfCube c;
    if (!tsdf_cube(a, ix, iy, iz, c)) return; // not with fcounts[v] > 0
    weld_cube_faces(a, ix, iy, iz, c, [&](const long long *idx) {
        if (n >= a.face_cap) return false;
        int32_t *dst = a.faces + (size_t)n * 3;
        dst[0] = (int32_t)idx[0], dst[1] = (int32_t)idx[1], dst[2] = (int32_t)idx[2];
        ++n;
        return true;
    });
}

static int weld_check(const tgp_tsdf_weld_args *args, int stage)
{
    TGP_REQUIRE(args);
    const tgp_tsdf_weld_args &a = *args;
    TGP_REQUIRE(a.sum && a.weight && a.meta && a.mask);
    TGP_REQUIRE(a.M > 0 && a.model >= 0 && a.model < a.M && a.min_weight >= 1);
    if (stage == 0) TGP_REQUIRE(a.vcounts);
    if (stage >= 1) TGP_REQUIRE(a.voffsets && a.vert_cap >= 0);
    if (stage == 1 || stage == 3) TGP_REQUIRE(a.fcounts);
    if (stage == 2) TGP_REQUIRE(a.verts || a.vert_cap == 0);
    if (stage == 3) TGP_REQUIRE(a.foffsets && a.info && a.face_cap >= 0 && (a.faces || a.face_cap == 0));
    if (a.G < TGP_TSDF_MIN_G || a.G > TGP_TSDF_MAX_G || a.G % 8 != 0) return TGP_EUNSUPPORTED;
    if (stage >= 1 && a.vert_cap > TGP_WELD_MAX_VERTS) return TGP_EUNSUPPORTED;
    if (stage == 3 && a.face_cap > TGP_TSDF_MAX_FACES) return TGP_EUNSUPPORTED;
    return 0;
}

#define WELD_LAUNCH(kernel, stage)                                                                                                \
    const int rc = weld_check(args, stage);                                                                                      \
    if (rc) return rc;                                                                                                           \
    const int64_t cells = (int64_t)args->G * args->G * args->G;                                                                  \
    hipLaunchKernelGGL(kernel, dim3((unsigned)tgp_cdiv(cells, WELD_THREADS)), dim3(WELD_THREADS), 0, tgp_hs(stream), *args);       \
    return TGP_LAUNCH_RESULT();

extern "C" int tgp_tsdf_weld_mark(const tgp_tsdf_weld_args *args, tgp_stream_t stream) { WELD_LAUNCH(weld_mark_kernel, 0) }
extern "C" int tgp_tsdf_weld_count(const tgp_tsdf_weld_args *args, tgp_stream_t stream) { WELD_LAUNCH(weld_count_kernel, 1) }
extern "C" int tgp_tsdf_weld_verts(const tgp_tsdf_weld_args *args, tgp_stream_t stream) { WELD_LAUNCH(weld_verts_kernel, 2) }
extern "C" int tgp_tsdf_weld_faces(const tgp_tsdf_weld_args *args, tgp_stream_t stream) { WELD_LAUNCH(weld_faces_kernel, 3) }

// ---- voxel clusters -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WELD_THREADS) void weld_cluster_kernel(const tgp_weld_cluster_args a)
{
    const int G = a.G, c = a.cluster, side = (G + c - 1) / c;
    const size_t cells = (size_t)G * G * G;
    const size_t v = (size_t)blockIdx.x * WELD_THREADS + threadIdx.x;
    if (v >= cells) return;
    const uint32_t m = a.mask[v];
    if (m == 0) return;
    const int cnt = __popc(m);
    const long long first = a.voffsets[v] - cnt; // the voxel's first vertex
    if (first >= a.vert_cap) return;
    const int live = first + cnt <= a.vert_cap ? cnt : (int)(a.vert_cap - first);
    const int iz = (int)(v % G), iy = (int)(v / G % G), ix = (int)(v / G / G);
    const int cell = ((ix / c) * side + iy / c) * side + iz / c;
    const float *meta = a.meta + (size_t)a.model * 4;
    const float voxel = meta[3];
    const double to_grid = 65536.0 / (double)voxel;
    long long s[3] = {0, 0, 0};
    for (int n = 0; n < live; ++n) {
        a.vcell[first + n] = cell;
        for (int k = 0; k < 3; ++k) {
            const double o = ((double)a.verts[(size_t)(first + n) * 3 + k] - (double)tsdf_centre(meta[k], 0, G, voxel)) * to_grid;
            if (fabs(o) < 4.0e15) s[k] += llrint(o); // false for a NaN; a vertex lies within G voxels of the first centre
        }
    }
    for (int k = 0; k < 3; ++k) atomicAdd((unsigned long long *)(a.cell_sums + (size_t)cell * 3 + k), (unsigned long long)s[k]);
    atomicAdd(a.cell_counts + cell, live);
}

extern "C" int tgp_weld_cluster(const tgp_weld_cluster_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_weld_cluster_args &a = *args;
    TGP_REQUIRE(a.mask && a.voffsets && a.meta && a.cell_sums && a.cell_counts && a.M > 0 && a.model >= 0 && a.model < a.M);
    TGP_REQUIRE(a.vert_cap >= 0 && ((a.verts && a.vcell) || a.vert_cap == 0));
    if (a.G < TGP_TSDF_MIN_G || a.G > TGP_TSDF_MAX_G || a.G % 8 != 0 || a.vert_cap > TGP_WELD_MAX_VERTS) return TGP_EUNSUPPORTED;
    if (a.cluster != 2 && a.cluster != 4 && a.cluster != 8) return TGP_EUNSUPPORTED;
    const int64_t side = (a.G + a.cluster - 1) / a.cluster, grid = side * side * side;
    hipError_t e = hipMemsetAsync(a.cell_sums, 0, (size_t)grid * 3 * sizeof(int64_t), tgp_hs(stream));
    if (e == hipSuccess) e = hipMemsetAsync(a.cell_counts, 0, (size_t)grid * sizeof(int32_t), tgp_hs(stream));
    if (e != hipSuccess) return (int)e;
    const int64_t cells = (int64_t)a.G * a.G * a.G;
    hipLaunchKernelGGL(weld_cluster_kernel, dim3((unsigned)tgp_cdiv(cells, WELD_THREADS)), dim3(WELD_THREADS), 0, tgp_hs(stream), a);
    return TGP_LAUNCH_RESULT();
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WELD_THREADS) void normals_face_kernel(const tgp_mesh_normals_args a)
{
    const int f = blockIdx.x * WELD_THREADS + threadIdx.x;
    if (f >= a.F) return;
    // the face's mesh: the last m with fptr[m] <= f
    int lo = 0, hi = a.M;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.fptr[mid] <= f)
            lo = mid;
        else
            hi = mid;
    }
    const int m = lo;
    if (f < a.fptr[m] || f >= a.fptr[m + 1]) return; // fptr does not ascend
    const int v0 = a.vptr[m], nv = a.vptr[m + 1] - v0;
    if (v0 < 0 || nv <= 0 || (int64_t)v0 + nv > a.V) return;
    const int i0 = a.faces[(size_t)f * 3 + 0], i1 = a.faces[(size_t)f * 3 + 1], i2 = a.faces[(size_t)f * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return; // a face outside its mesh adds nothing
    const float *p0 = a.verts + (size_t)(v0 + i0) * 3, *p1 = a.verts + (size_t)(v0 + i1) * 3, *p2 = a.verts + (size_t)(v0 + i2) * 3;
    const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const float wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
    const float c[3] = {uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
    const double scale = a.scale[m];
    const int idx[3] = {i0, i1, i2};
    for (int k = 0; k < 3; ++k) {
        const double q = (double)c[k] * scale;
        if (!(fabs(q) < 4.0e15)) continue; // a NaN, or beyond what the int64 sums hold with room for every face of a mesh
        const long long n = llrint(q);
        if (n == 0) continue;
        for (int j = 0; j < 3; ++j)
            atomicAdd((unsigned long long *)(a.sums + (size_t)(v0 + idx[j]) * 3 + k), (unsigned long long)n);
    }
}

__global__ __launch_bounds__(WELD_THREADS) void normals_unit_kernel(const tgp_mesh_normals_args a)
{
    const int64_t v = (int64_t)blockIdx.x * WELD_THREADS + threadIdx.x;
    if (v >= a.V) return;
    const int64_t *s = a.sums + (size_t)v * 3;
    float *dst = a.normals + (size_t)v * 3;
    if (s[0] == 0 && s[1] == 0 && s[2] == 0) {
        dst[0] = dst[1] = dst[2] = 0.f;
        return;
    }
    const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
    const double len = __dsqrt_rn((x * x + y * y) + z * z);
    dst[0] = (float)__ddiv_rn(x, len), dst[1] = (float)__ddiv_rn(y, len), dst[2] = (float)__ddiv_rn(z, len);
}

extern "C" int tgp_mesh_vertex_normals(const tgp_mesh_normals_args *args, tgp_stream_t stream)
{
    TGP_REQUIRE(args);
    const tgp_mesh_normals_args &a = *args;
    TGP_REQUIRE(a.vptr && a.fptr && a.scale && a.M > 0 && a.V >= 0 && a.F >= 0);
    TGP_REQUIRE(a.V == 0 || (a.verts && a.sums && a.normals));
    TGP_REQUIRE(a.F == 0 || (a.faces && a.V > 0));
    if (a.V > TGP_WELD_MAX_VERTS || a.F > TGP_TSDF_MAX_FACES) return TGP_EUNSUPPORTED;
    if (a.V == 0) return 0;
    hipError_t e = hipMemsetAsync(a.sums, 0, (size_t)a.V * 3 * sizeof(int64_t), tgp_hs(stream));
    if (e != hipSuccess) return (int)e;
    if (a.F > 0) {
        hipLaunchKernelGGL(normals_face_kernel, dim3((unsigned)tgp_cdiv(a.F, WELD_THREADS)), dim3(WELD_THREADS), 0, tgp_hs(stream), a);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(normals_unit_kernel, dim3((unsigned)tgp_cdiv(a.V, WELD_THREADS)), dim3(WELD_THREADS), 0, tgp_hs(stream), a);
    return TGP_LAUNCH_RESULT();
}
