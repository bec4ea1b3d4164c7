// Segments of depth frames on gfx950 (DESIGN.md section 3 "Segments of a depth frame" and include/tgpose.h are the contract;
// tests/segment_ref.py restates it in NumPy): tgp_segment_depth labels the connected components of S frames -- valid pixels joined to
// their 4- or 8-neighbours when their depths differ by at most max_step millimetres -- keeps those of at least min_pixels pixels,
// numbers them by their smallest flat index and returns the label image, the segments' integer moments and their centroids.
//
// A component is a tree of parent words (one int per pixel, parent <= the pixel's own flat index, a root is its own parent), and
// joining two pixels is a lock-free min-union: the larger of their two roots is pointed at the smaller with atomicMin.  Seven
// launches behind two memsets (the frame's valid-pixel counter, the stats):
//   tile     grid (W / 32, H / 16, S), 256 threads: the tile's components by the same min-union on LDS words, flattened; every pixel's
//            parent becomes its tile component's smallest flat index (-1 for an invalid pixel), its count word 0.
//   merge    a wave per tile, a lane per pixel of its top / left (8-neighbours: right too) edge: min-union in global memory with the
//            joined neighbours in the tiles before it.
//   count    a thread per four pixels: the root, written back as the pixel's parent; lanes of a wave that share a root are found
//            with ballots and add their number to the root's count word with ONE integer atomic.
//   chunk    per 4096 flat pixels the number of qualifying roots (a root whose count reaches min_pixels).
//   rank     per chunk: the qualifying roots before the chunk (a sum over the earlier chunks' numbers) plus an ordered prefix inside
//            it is a root's rank; its count word becomes its label (0 beyond max_segments), the stats row learns its root; the last
//            chunk writes info.
//   relabel  a thread per 16 consecutive pixels: label = the count word of the pixel's parent; runs of one label are summed in
//            registers, then in LDS (64-bit integer atomics), then in the stats (64-bit integer atomics; the minima as maxima of
//            complements, so that zero is every column's neutral element).
//   finish   a thread per stats row: the complements become minima, the centroid is computed in float64 and rounded once.
//
// TERMINATION.  No loop in this file waits for another thread, wave or workgroup: there is no flag, lock, ticket or spin.  The loops
// that are not counted are:
//   find_root   walks x <- parent[x].  It goes on only while 0 <= parent[x] < x, so x strictly decreases and it ends after at most x
//               steps WHATEVER the words hold, stale or torn values included; every index it touches lies in [0, start].
//   unite       each turn ends the loop or replaces (a, b) by two indices that are both smaller than max(a, b): with hi the larger
//               root and lo the smaller, old = atomicMin(&parent[hi], lo).  old == hi: hi was a root and hangs under lo now, done.
//               Else another thread had lowered parent[hi] to old < hi first; the word is min(old, lo) now, and what is left to join
//               are old and lo, both < hi.  The turn goes on only for 0 <= old < hi, so max(a, b) strictly decreases: at most
//               max(a, b) turns on any input, whatever the other workgroups do or do not do meanwhile.
//   the root-sharing loop of count clears at least the leader's bit of a wave-uniform mask each turn: at most 64 turns.
// CORRECTNESS of the concurrent unions: parent words only ever decrease and only ever point at a pixel of the same component (an
// edge, or an ancestor found by walking edges), so a stale read is an older ancestor, still valid.  A turn that finds old < hi has
// replaced the edge hi -> old by hi -> min(old, lo) and owes the union of old and lo, which it goes on to make; when the launch ends
// nothing is owed, every joined pair has one root, and since parents never exceed their pixel a root is its tree's smallest index.
#include "tgp_common.h"

#pragma clang fp contract(off)        // the centroid's float64 steps are rounded one by one

namespace {

constexpr int TW = 32, TH = 16, TILE = TW * TH;          // the LDS tile
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / TGP_WAVE;
constexpr int COUNT_PER = 4;                             // pixels of a thread in count, a workgroup's width apart
constexpr int PER = 16;                                  // consecutive flat pixels of a thread in chunk / rank / relabel
constexpr int CHUNK = THREADS * PER;
constexpr int COLS = TGP_SEG_STAT_COLS;
constexpr int MAXSEG = TGP_SEG_MAX_SEGMENTS;
constexpr int COORD_TOP = 32768, DEPTH_TOP = 65536;      // minima travel as maxima of (TOP - value) > 0

typedef unsigned long long u64;

struct LdsWords {                                        // parent words of a tile, indices local to it
    int *w;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int lower(int i, int v) const { return __hip_atomic_fetch_min(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct GlobalWords {                                     // parent words of a frame; the loads bypass the CU's L1
    int *w;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int lower(int i, int v) const { return __hip_atomic_fetch_min(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(int i, int v) const { __hip_atomic_store(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct SettledWords {                                    // parent words after the last union
    int *w;
    __device__ __forceinline__ int load(int i) const { return w[i]; }
    __device__ __forceinline__ void store(int i, int v) const { w[i] = v; }
};

template <class Words>
__device__ __forceinline__ int find_root(const Words &par, int x)
{
    for (;;) {
        const int p = par.load(x);
        if (p >= x || p < 0) return x;                   // a root (p == x); anything else that would not descend ends the walk too
        x = p;
    }
}

template <class Words>
__device__ __forceinline__ void unite(const Words &par, int a, int b)
{
    for (;;) {
        a = find_root(par, a), b = find_root(par, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = par.lower(hi, lo);
        if (old >= hi || old < 0) return;                // old == hi: hi was a root and hangs under lo now
        a = old, b = lo;                                 // both < hi
    }
}

__device__ __forceinline__ bool joined(int z, int zn, int max_step) { return zn > 0 && abs(z - zn) <= max_step; }

__global__ void __launch_bounds__(THREADS) seg_tile_kernel(const uint16_t *__restrict__ depth, int H, int W, int max_step, int conn8,
                                                          int *__restrict__ parent, int *__restrict__ count)
{
    __shared__ int s_z[TILE];
    __shared__ int s_par[TILE];
    const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const size_t base = (size_t)blockIdx.z * H * W;
    for (int i = tid; i < TILE; i += THREADS) {
        const int x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        s_z[i] = x < W && y < H ? (int)depth[base + y * W + x] : 0;
        s_par[i] = i;
    }
    __syncthreads();
    const LdsWords par{s_par};
    for (int i = tid; i < TILE; i += THREADS) {
        const int z = s_z[i], lx = i & (TW - 1), ly = i / TW;
        if (z == 0) continue;
        if (lx > 0 && joined(z, s_z[i - 1], max_step)) unite(par, i, i - 1);
        if (ly > 0) {
            if (joined(z, s_z[i - TW], max_step)) unite(par, i, i - TW);
            if (conn8) {
                if (lx > 0 && joined(z, s_z[i - TW - 1], max_step)) unite(par, i, i - TW - 1);
                if (lx < TW - 1 && joined(z, s_z[i - TW + 1], max_step)) unite(par, i, i - TW + 1);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < TILE; i += THREADS) {
        const int x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        if (x >= W || y >= H) continue;
        int g = -1;
        if (s_z[i] != 0) {
            const int r = find_root(par, i);             // local order is flat order: the tile component's smallest flat index
            g = (y0 + r / TW) * W + x0 + (r & (TW - 1));
        }
        parent[base + y * W + x] = g;
        count[base + y * W + x] = 0;
    }
}

// a wave per tile: lanes 0..31 its top row, 32..47 its left column, 48..63 its right column (8-neighbours only; the corners belong
// to the top row)
__global__ void __launch_bounds__(THREADS) seg_merge_kernel(const uint16_t *__restrict__ depth, int H, int W, int max_step, int conn8, int tiles_x,
                                                           int tiles, int *parent)
{
    const int gid = blockIdx.x * THREADS + threadIdx.x, tile = gid / TGP_WAVE, j = gid & (TGP_WAVE - 1);
    if (tile >= tiles) return;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    int lx, ly;
    if (j < TW) lx = j, ly = 0;
    else if (j < TW + TH) lx = 0, ly = j - TW;
    else lx = TW - 1, ly = j - TW - TH;
    if (j >= TW && (ly == 0 || (j >= TW + TH && !conn8))) return;
    const int x = tx * TW + lx, y = ty * TH + ly;
    if (x >= W || y >= H) return;
    const int p = y * W + x;
    const size_t base = (size_t)blockIdx.y * H * W;
    const uint16_t *dimg = depth + base;
    const int z = dimg[p];
    if (z == 0) return;
    const GlobalWords par{parent + base};
    auto join = [&](int q) {
        if (!joined(z, dimg[q], max_step)) return;
        const int before = par.load(p);
        unite(par, p, q);
        const int r = find_root(par, p);                 // shorten this pixel's path: an ancestor, never above the word's value
        if (r < before) par.lower(p, r);
    };
    if (x > 0 && lx == 0) join(p - 1);
    if (y > 0) {
        if (ly == 0) join(p - W);
        if (conn8) {
            if (x > 0 && (lx == 0 || ly == 0)) join(p - W - 1);
            if (x < W - 1 && (lx == TW - 1 || ly == 0)) join(p - W + 1);
        }
    }
}

// No union runs any more: a parent word holds what the merge left or, once this launch has flattened it, the root -- an ancestor
// either way, so plain (L1-cached) loads serve.  A thread takes COUNT_PER pixels a workgroup-width apart.
__global__ void __launch_bounds__(THREADS) seg_count_kernel(int HW, int *parent, int *count, int *nvalid)
{
    __shared__ int s_valid;
    const int tid = threadIdx.x, lane = tid & (TGP_WAVE - 1);
    const size_t base = (size_t)blockIdx.y * HW;
    const SettledWords par{parent + base};
    if (tid == 0) s_valid = 0;
    __syncthreads();
    int nv = 0;
#pragma unroll
    for (int k = 0; k < COUNT_PER; ++k) {
        const int p = (blockIdx.x * COUNT_PER + k) * THREADS + tid;
        int r = -1;
        if (p < HW) {
            const int p0 = par.load(p);
            if (p0 >= 0) {
                r = find_root(par, p);
                if (r != p0) par.store(p, r);            // a walk that passes here meanwhile still descends to r
            }
        }
        const bool valid = r >= 0;
        u64 todo = __ballot(valid);                      // the same in every lane; no lane has left the kernel
        nv += __popcll(todo);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int rl = __shfl(r, leader);
            const u64 same = __ballot(valid && r == rl); // holds the leader's bit
            if (lane == leader) atomicAdd(&count[base + rl], __popcll(same));
            todo &= ~same;
        }
    }
    if (lane == 0 && nv) atomicAdd(&s_valid, nv);
    __syncthreads();
    if (tid == 0 && s_valid) atomicAdd(&nvalid[blockIdx.y], s_valid);
}

// the sum of v over the workgroup, in every thread; s_w: WAVES ints
__device__ __forceinline__ int block_sum(int v, int *s_w)
{
#pragma unroll
    for (int o = TGP_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                     // s_w may still be read from an earlier call
    if ((threadIdx.x & (TGP_WAVE - 1)) == 0) s_w[threadIdx.x / TGP_WAVE] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += s_w[w];
    return t;
}

// bit i of the result: pixel p0 + i of the frame is a root whose count reaches min_pixels
__device__ __forceinline__ uint32_t qualifying(const int *__restrict__ parent, const int *__restrict__ count, int p0, int HW, int min_pixels)
{
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = p0 + i;
        if (p < HW && parent[p] == p && count[p] >= min_pixels) bits |= 1u << i;
    }
    return bits;
}

__global__ void __launch_bounds__(THREADS) seg_chunk_kernel(int HW, int min_pixels, const int *__restrict__ parent, const int *__restrict__ count,
                                                           int *__restrict__ chunk_count)
{
    __shared__ int s_w[WAVES];
    const size_t base = (size_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * CHUNK + threadIdx.x * PER;
    const int q = block_sum(__popc(qualifying(parent + base, count + base, p0, HW, min_pixels)), s_w);
    if (threadIdx.x == 0) chunk_count[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = q;
}

__global__ void __launch_bounds__(THREADS) seg_rank_kernel(int HW, int min_pixels, int max_segments, const int *__restrict__ parent, int *count,
                                                          const int *__restrict__ chunk_count, const int *__restrict__ nvalid,
                                                          int32_t *__restrict__ info, int64_t *__restrict__ stats)
{
    __shared__ int s_w[WAVES];
    const int s = blockIdx.y, c = blockIdx.x, nchunks = gridDim.x, tid = threadIdx.x, lane = tid & (TGP_WAVE - 1), wave = tid / TGP_WAVE;
    const size_t base = (size_t)s * HW;
    int before = 0;                                      // qualifying roots of the chunks before this one
    for (int k = tid; k < c; k += THREADS) before += chunk_count[(size_t)s * nchunks + k];
    before = block_sum(before, s_w);
    const int p0 = c * CHUNK + tid * PER;
    const uint32_t bits = qualifying(parent + base, count + base, p0, HW, min_pixels);
    const int q = __popc(bits);
    int incl = q;                                        // inclusive scan over the wave, then the waves in order
#pragma unroll
    for (int o = 1; o < TGP_WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == TGP_WAVE - 1) s_w[wave] = incl;
    __syncthreads();
    int rank = before + incl - q, total = before;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) rank += s_w[w];
        total += s_w[w];
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = p0 + i;
        if (p >= HW || parent[base + p] != p) continue;
        int label = 0;
        if (bits >> i & 1u) {
            label = rank < max_segments ? rank + 1 : 0;
            ++rank;
        }
        count[base + p] = label;                         // the root's count word is its component's label from here on
        if (label) stats[((size_t)s * max_segments + label - 1) * COLS + 5] = p;
    }
    if (c == nchunks - 1 && tid == 0) {
        info[s * 4] = total > max_segments ? 1 : 0;
        info[s * 4 + 1] = min(total, max_segments);
        info[s * 4 + 2] = total;
        info[s * 4 + 3] = nvalid[s];
    }
}

struct Run {                                             // the pixels of one label a thread has met in a row
    int n, ymin, ymax, xmin, xmax, zmin;
    u64 sx, sy, sz, sxz, syz;
    __device__ __forceinline__ void reset() { n = 0, ymin = xmin = COORD_TOP, ymax = xmax = -1, zmin = DEPTH_TOP, sx = sy = sz = sxz = syz = 0; }
    __device__ __forceinline__ void add(int x, int y, int z)
    {
        ++n, ymin = min(ymin, y), ymax = max(ymax, y), xmin = min(xmin, x), xmax = max(xmax, x), zmin = min(zmin, z);
        sx += (u64)x, sy += (u64)y, sz += (u64)z, sxz += (u64)x * (u64)z, syz += (u64)y * (u64)z;
    }
    __device__ __forceinline__ void flush(u64 *row) const
    {
        atomicAdd(row + 0, (u64)n);
        atomicMax(row + 1, (u64)(COORD_TOP - ymin)), atomicMax(row + 2, (u64)(COORD_TOP - xmin));
        atomicMax(row + 3, (u64)(ymax + 1)), atomicMax(row + 4, (u64)(xmax + 1));
        atomicAdd(row + 6, sx), atomicAdd(row + 7, sy), atomicAdd(row + 8, sz), atomicAdd(row + 9, sxz), atomicAdd(row + 10, syz);
        atomicMax(row + 11, (u64)(DEPTH_TOP - zmin));
    }
};

// VEC: H*W is a multiple of 16 and labels is 16-byte aligned, so a thread's 16 labels are one aligned store inside the frame
template <bool VEC>
__global__ void __launch_bounds__(THREADS) seg_relabel_kernel(const uint16_t *__restrict__ depth, int H, int W, int max_segments,
                                                             const int *__restrict__ parent, const int *__restrict__ count,
                                                             uint8_t *__restrict__ labels, u64 *stats)
{
    __shared__ u64 s_acc[MAXSEG * COLS];
    const int s = blockIdx.y, tid = threadIdx.x, HW = H * W, words = max_segments * COLS;
    const size_t base = (size_t)s * HW;
    for (int k = tid; k < words; k += THREADS) s_acc[k] = 0;
    __syncthreads();
    const int p0 = blockIdx.x * CHUNK + tid * PER;
    if (p0 < HW) {
        int y = p0 / W, x = p0 - y * W;
        int cur = 0, last_root = -1, last_label = 0;
        uint32_t packed[PER / 4] = {};
        Run run;
        run.reset();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int p = p0 + i;
            if (p < HW) {
                const int r = parent[base + p];
                int label = 0;
                if (r >= 0) {
                    if (r != last_root) last_root = r, last_label = count[base + r];
                    label = last_label;
                }
                if (label != cur) {
                    if (cur && run.n) run.flush(s_acc + (cur - 1) * COLS);
                    cur = label;
                    run.reset();
                }
                if (label) run.add(x, y, (int)depth[base + p]);
                if constexpr (VEC) packed[i / 4] |= (uint32_t)label << (8 * (i & 3));
                else labels[base + p] = (uint8_t)label;
                if (++x == W) x = 0, ++y;
            }
        }
        if (cur && run.n) run.flush(s_acc + (cur - 1) * COLS);
        if constexpr (VEC) *reinterpret_cast<uint4 *>(labels + base + p0) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
    }
    __syncthreads();
    u64 *rows = stats + (size_t)s * words;
    for (int k = tid; k < words; k += THREADS) {
        const u64 v = s_acc[k];
        if (v == 0) continue;                            // zero is neutral in every column
        const int col = k % COLS;
        if (col == 0 || (col >= 6 && col <= 10)) atomicAdd(rows + k, v);
        else atomicMax(rows + k, v);
    }
}

__global__ void __launch_bounds__(THREADS) seg_finish_kernel(const float *__restrict__ camk, int max_segments, const int32_t *__restrict__ info,
                                                            int64_t *__restrict__ stats, float *__restrict__ centers)
{
    const int s = blockIdx.x, r = threadIdx.x;
    if (r >= max_segments) return;
    const bool kept = r < info[s * 4 + 1];
    int64_t *row = stats + ((size_t)s * max_segments + r) * COLS;
    if (kept) row[1] = COORD_TOP - row[1], row[2] = COORD_TOP - row[2], row[11] = DEPTH_TOP - row[11];
    if (!centers) return;
    float *c = centers + ((size_t)s * max_segments + r) * 3;
    if (!kept) {
        c[0] = c[1] = c[2] = __builtin_nanf("");
        return;
    }
    const double n = (double)row[0], sz = (double)row[8], sxz = (double)row[9], syz = (double)row[10];
    const double fx = camk[s * 4], fy = camk[s * 4 + 1], cx = camk[s * 4 + 2], cy = camk[s * 4 + 3];
    c[0] = (float)((sxz - cx * sz) / (fx * n) / 1000.0);
    c[1] = (float)((syz - cy * sz) / (fy * n) / 1000.0);
    c[2] = (float)(sz / n / 1000.0);
}

int seg_frames_rc(int S, int H, int W)
{
    if (!(S >= 1 && H >= 1 && W >= 1 && H < 32768 && W < 32768 && (int64_t)H * W < (1ll << 24))) return TGP_EINVAL;
    return S > 65535 ? TGP_EUNSUPPORTED : 0;
}

// the workspace in ints: parent (S*HW), count (S*HW), nvalid (S), chunk_count (S * chunks)
int64_t seg_workspace_ints(int S, int H, int W)
{
    const int64_t HW = (int64_t)H * W;
    return 2 * S * HW + S + (int64_t)S * tgp_cdiv(HW, CHUNK);
}

}  // namespace

extern "C" int64_t tgp_segment_workspace_bytes(int S, int H, int W)
{
    const int rc = seg_frames_rc(S, H, W);
    if (rc) return rc;
    return (seg_workspace_ints(S, H, W) * (int64_t)sizeof(int) + 15) / 16 * 16;
}

extern "C" int tgp_segment_depth(const tgp_segment_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->depth && a->labels && a->info && a->stats && a->workspace && (a->camk || !a->centers));
    const int frames_rc = seg_frames_rc(a->S, a->H, a->W);
    if (frames_rc == TGP_EINVAL) return TGP_EINVAL;
    TGP_REQUIRE(a->max_step >= 0 && a->max_step <= 65535 && (a->connectivity == 4 || a->connectivity == 8) && a->min_pixels >= 1);
    TGP_REQUIRE(a->max_segments >= 1 && a->max_segments <= MAXSEG);
    if (frames_rc) return frames_rc;
    TGP_REQUIRE(a->workspace_bytes >= tgp_segment_workspace_bytes(a->S, a->H, a->W) && ((uintptr_t)a->workspace & 15u) == 0);
    const hipStream_t st = tgp_hs(stream);
    const int S = a->S, H = a->H, W = a->W, HW = H * W, conn8 = a->connectivity == 8, chunks = tgp_cdiv(HW, CHUNK);
    int *parent = (int *)a->workspace, *count = parent + (size_t)S * HW, *nvalid = count + (size_t)S * HW, *chunk_count = nvalid + S;
    hipError_t e = hipMemsetAsync(nvalid, 0, (size_t)S * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(a->stats, 0, (size_t)S * a->max_segments * COLS * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    const int tiles_x = tgp_cdiv(W, TW), tiles_y = tgp_cdiv(H, TH);
    const dim3 block(THREADS), chunked(chunks, S);
    hipLaunchKernelGGL(seg_tile_kernel, dim3(tiles_x, tiles_y, S), block, 0, st, a->depth, H, W, a->max_step, conn8, parent, count);
    int rc = TGP_LAUNCH_RESULT();
    if (rc) return rc;
    hipLaunchKernelGGL(seg_merge_kernel, dim3(tgp_cdiv((int64_t)tiles_x * tiles_y * TGP_WAVE, THREADS), S), block, 0, st, a->depth, H, W,
                       a->max_step, conn8, tiles_x, tiles_x * tiles_y, parent);
    if ((rc = TGP_LAUNCH_RESULT())) return rc;
    hipLaunchKernelGGL(seg_count_kernel, dim3(tgp_cdiv(HW, THREADS * COUNT_PER), S), block, 0, st, HW, parent, count, nvalid);
    if ((rc = TGP_LAUNCH_RESULT())) return rc;
    hipLaunchKernelGGL(seg_chunk_kernel, chunked, block, 0, st, HW, a->min_pixels, parent, count, chunk_count);
    if ((rc = TGP_LAUNCH_RESULT())) return rc;
    hipLaunchKernelGGL(seg_rank_kernel, chunked, block, 0, st, HW, a->min_pixels, a->max_segments, parent, count, chunk_count, nvalid, a->info, a->stats);
    if ((rc = TGP_LAUNCH_RESULT())) return rc;
    if (HW % PER == 0 && ((uintptr_t)a->labels & 15u) == 0)
        hipLaunchKernelGGL(seg_relabel_kernel<true>, chunked, block, 0, st, a->depth, H, W, a->max_segments, parent, count, a->labels, (u64 *)a->stats);
    else
        hipLaunchKernelGGL(seg_relabel_kernel<false>, chunked, block, 0, st, a->depth, H, W, a->max_segments, parent, count, a->labels, (u64 *)a->stats);
    if ((rc = TGP_LAUNCH_RESULT())) return rc;
    hipLaunchKernelGGL(seg_finish_kernel, dim3(S), block, 0, st, a->camk, a->max_segments, a->info, a->stats, a->centers);
    return TGP_LAUNCH_RESULT();
}
