// The rasteriser's arithmetic, shared by the depth renderer (render.hip) and pose verification (verify.hip): DESIGN.md section 3 "The
// depth renderer" states every rule below and tests/render_ref.py restates them in numpy.  A vertex is posed, projected and snapped to
// 1/256 px; a triangle is dropped by the near rule or the guard band, or gets the pixel box of its snapped corners; a tile sets the
// triangles that meet it up into LDS records at its first sample point and every lane runs the records against its own pixel, keeping
// the smallest 64-bit key {z bits, lo}.  The loops around these steps -- which boxes a tile walks, when the list is swept -- belong
// to the kernels.
#ifndef TGP_RASTER_H
#define TGP_RASTER_H
#include "tgp_common.h"

#define RASTER_GUARD 4194304.f // 2^22 sub-pixel units
#define RASTER_TILE 16
#define RASTER_THREADS (RASTER_TILE * RASTER_TILE)
#define RASTER_CAP (2 * RASTER_THREADS) // records held before a raster sweep: one chunk always fits behind a sweep's threshold

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

#endif
