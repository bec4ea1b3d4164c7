// What the marching-tetrahedra kernels of tsdf.hip (the triangle soup) and weld.hip (the indexed mesh) share: the voxel centres, a
// cube's eight corners, the six Kuhn tetrahedra with their cases and windings, and the arithmetic of a cut edge's vertex.  One
// copy, so that the two files give the same bits (include/tgpose.h states the contract; tests/tsdf_ref.py restates it).
// The two tables it reads -- tsdf_path[6][4] and tsdf_flip[6] -- are literals of the including file, defined before this include:
// tests/test_tsdf_cpu.py and tests/test_weld_cpu.py hold each file's copy against the derived ones.
#pragma once
#include "tgp_common.h"

__device__ __forceinline__ float tsdf_centre(float c, int i, int G, float voxel)
{
    return c + (((float)i + 0.5f) - (float)(G / 2)) * voxel;
}

struct TsdfCube {
    int s[8], w[8];
};

// the cube at voxel v of the volume a.model: false where there is none (a last row, or a corner below min_weight).  A is an
// argument struct with sum, weight, G, model and min_weight.
template <class A>
__device__ __forceinline__ bool tsdf_cube(const A &a, int ix, int iy, int iz, TsdfCube &c)
{
    const int G = a.G;
    if (ix >= G - 1 || iy >= G - 1 || iz >= G - 1) return false;
    const size_t base = (size_t)a.model * G * G * G;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const size_t o = base + ((size_t)(ix + (k >> 2)) * G + (iy + ((k >> 1) & 1))) * G + (iz + (k & 1));
        c.w[k] = a.weight[o];
        c.s[k] = a.sum[o];
        ok = ok && c.w[k] >= a.min_weight;
    }
    return ok;
}

__device__ __forceinline__ int tsdf_case(const TsdfCube &c, int k)
{
    int cs = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) cs |= (c.s[tsdf_path[k][p]] < 0 ? 1 : 0) << p;
    return cs;
}

__device__ __forceinline__ int tsdf_case_faces(int cs)
{
    const int n = __popc(cs);
    return n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
}

// the cut edges (pairs of path corners) of a tetrahedron in case cs (1..14), in the order the contract lists them
__device__ __forceinline__ void tsdf_case_edges(int cs, int ea[4], int eb[4])
{
    // the path corners, inside ones first, each kind in path order
    int in[4], out[4], ni = 0, no = 0;
    for (int p = 0; p < 4; ++p) {
        if (cs >> p & 1)
            in[ni++] = p;
        else
            out[no++] = p;
    }
    if (ni == 1) {
        for (int e = 0; e < 3; ++e) ea[e] = in[0], eb[e] = out[e];
    } else if (ni == 3) {
        for (int e = 0; e < 3; ++e) ea[e] = in[e], eb[e] = out[0];
    } else {
        ea[0] = in[0], eb[0] = out[0];
        ea[1] = in[0], eb[1] = out[1];
        ea[2] = in[1], eb[2] = out[1];
        ea[3] = in[1], eb[3] = out[0];
    }
}

// corner q (0, 1, 2) of triangle t of a case: which of the case's cut edges it lies on; (0,1,2), then (0,2,3), the second and third
// swapped where the winding table says so
__device__ __forceinline__ int tsdf_face_edge(int t, int q, bool flip)
{
    if (q == 0) return 0;
    return ((q == 1) != flip) ? t + 1 : t + 2;
}

// the vertex on the edge from voxel (ax, ay, az) -- the end earlier in the path -- to voxel (bx, by, bz), whose sums and weights are
// (sa, wa) and (sb, wb): float32, every operation rounded on its own
__device__ __forceinline__ void tsdf_edge_vertex(const float *meta, int G, int sa, int wa, int sb, int wb, int ax, int ay, int az, int bx,
                                                 int by, int bz, float *dst)
{
    const float voxel = meta[3];
    const float fa = (float)sa / (float)wa, fb = (float)sb / (float)wb;
    const float tt = fa / (fa - fb);
    const float pax = tsdf_centre(meta[0], ax, G, voxel), pay = tsdf_centre(meta[1], ay, G, voxel), paz = tsdf_centre(meta[2], az, G, voxel);
    const float pbx = tsdf_centre(meta[0], bx, G, voxel), pby = tsdf_centre(meta[1], by, G, voxel), pbz = tsdf_centre(meta[2], bz, G, voxel);
    dst[0] = pax + tt * (pbx - pax);
    dst[1] = pay + tt * (pby - pay);
    dst[2] = paz + tt * (pbz - paz);
}
