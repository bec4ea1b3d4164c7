// Area-weighted surface sampling of triangle meshes (network/point_sample/pc_sample_sphere.py: uniform_sample) on gfx950.
//
// The reference draws one sample per Python iteration: a face by np.searchsorted on the cumulative triangle area, a point by the
// square-root barycentric map.  Here a mesh set's cumulative areas are built once (mesh_area_kernel, one workgroup per mesh) and a
// call is ONE launch for B jobs of n samples, one thread per sample: a binary search in the table (bounded by log2 F), the face's
// three vertices, eleven float64 products.  No atomics, nothing allocated, nothing read back, results bit-repeatable.
//
// Arithmetic (include/tgpose.h and DESIGN.md section 3 "Mesh surface sampling" are the contract; the library is built with
// -ffp-contract=off, so every product and sum below rounds on its own, as NumPy's do):
//   cross = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x), a = v1 - v0, b = v2 - v0 in float64 on the float32 vertices
//   norm = sqrt_rn((c_x c_x + c_y c_y) + c_z c_z), area = 0.5 norm
//   cdf: chunks of TGP_MESH_AREA_CHUNK faces, a serial prefix inside a chunk plus the serial prefix of the chunk totals
//   point = ((1 - s) v0 + (s (1 - r2)) v1) + (s r2) v2, s = sqrt_rn(r1); normal = cross / norm (div_rn)
#include "tgp_common.h"
#include "philox.h"

namespace {

constexpr int AREA_THREADS = 256;                    // one chunk per thread and pass: a pass covers AREA_THREADS * CHUNK faces
constexpr int CHUNK = TGP_MESH_AREA_CHUNK;
constexpr int SAMPLE_THREADS = 256;

struct MeshRange {
    int v0, V, f0, F;
    bool ok;
};

// the mesh's rows of the vertex and face arrays; ok only when both lie inside the arrays and are not empty
__device__ __forceinline__ MeshRange mesh_range(const int32_t *__restrict__ vptr, const int32_t *__restrict__ fptr, int m, int n_verts,
                                                int n_faces)
{
    MeshRange r;
    r.v0 = vptr[m], r.V = vptr[m + 1] - r.v0, r.f0 = fptr[m], r.F = fptr[m + 1] - r.f0;
    r.ok = r.v0 >= 0 && r.V >= 1 && r.V <= n_verts - r.v0 && r.f0 >= 0 && r.F >= 1 && r.F <= n_faces - r.f0;
    return r;
}

// face f (global row of `faces`) of a mesh whose vertices are rows [v0, v0 + V): its corners and cross vector in float64
__device__ __forceinline__ void face_cross(const float *__restrict__ verts, const int32_t *__restrict__ faces, int v0, int V, size_t f,
                                           double p[3][3], double c[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = min(max(faces[f * 3 + k], 0), V - 1);             // inside the mesh whatever the array holds
        const float *v = verts + (size_t)(v0 + i) * 3;
        p[k][0] = (double)v[0], p[k][1] = (double)v[1], p[k][2] = (double)v[2];
    }
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    c[0] = ay * bz - az * by;
    c[1] = az * bx - ax * bz;
    c[2] = ax * by - ay * bx;
}

__device__ __forceinline__ double cross_norm(const double c[3]) { return __dsqrt_rn((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]); }

// One workgroup per mesh.  Pass by pass over AREA_THREADS chunks: every thread sums its chunk serially into cdf (local[f]), thread 0
// extends the serial prefix of the chunk totals, every thread adds its chunk's offset.  The order of the additions is a function of
// F and CHUNK alone.
__global__ void __launch_bounds__(AREA_THREADS) mesh_area_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                 const int32_t *__restrict__ vptr, const int32_t *__restrict__ fptr,
                                                                 int n_verts, int n_faces, double *__restrict__ cdf)
{
    __shared__ double s_tot[AREA_THREADS], s_off[AREA_THREADS];
    const int tid = threadIdx.x;
    const MeshRange r = mesh_range(vptr, fptr, blockIdx.x, n_verts, n_faces);
    if (!r.ok) return;                                                  // the same in every thread
    double carry = 0.0;                                                 // thread 0: O of the pass's first chunk
    for (int64_t base = 0; base < r.F; base += AREA_THREADS * CHUNK) {
        const int64_t c0 = base + tid * CHUNK;
        const int len = c0 < r.F ? (int)min((int64_t)CHUNK, r.F - c0) : 0;
        double *o = cdf + (size_t)r.f0 + c0;
        double s = 0.0;
        for (int j = 0; j < len; ++j) {
            double p[3][3], c[3];
            face_cross(verts, faces, r.v0, r.V, (size_t)r.f0 + c0 + j, p, c);
            s = s + 0.5 * cross_norm(c);
            o[j] = s;
        }
        s_tot[tid] = s;
        __syncthreads();
        if (tid == 0) {
            const int live = (int)min((int64_t)AREA_THREADS, (r.F - base + CHUNK - 1) / CHUNK);
            for (int t = 0; t < live; ++t) {
                s_off[t] = carry;
                carry = carry + s_tot[t];
            }
        }
        __syncthreads();
        const double off = len ? s_off[tid] : 0.0;
        for (int j = 0; j < len; ++j) o[j] = off + o[j];
        __syncthreads();                                                // s_tot and s_off are rewritten by the next pass
    }
}

template <typename T>
__device__ __forceinline__ void store_row(T *__restrict__ o, const double *v, int cols)
{
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (k < cols) o[k] = (T)v[k];
}

__global__ void __launch_bounds__(SAMPLE_THREADS) mesh_sample_kernel(tgp_mesh_sample_args a)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * SAMPLE_THREADS + threadIdx.x;
    const int m = a.job_mesh[b];
    MeshRange r = {0, 0, 0, 0, false};
    if (m >= 0 && m < a.M) r = mesh_range(a.vptr, a.fptr, m, a.n_verts, a.n_faces);
    const double total = r.ok ? a.cdf[(size_t)r.f0 + r.F - 1] : 0.0;
    const bool good = total > 0.0 && total < __builtin_inf();           // false for NaN
    if (i == 0) a.status[b] = !r.ok ? 2 : good ? 0 : 1;
    if (i >= a.n) return;
    const size_t row = (size_t)b * a.n + i;
    const int cols = a.normals ? 6 : 3;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int face = -1;
    if (r.ok) {
        double u, r1, r2;
        if (a.u) {
            u = a.u[row * 3], r1 = a.u[row * 3 + 1], r2 = a.u[row * 3 + 2];
        } else {
            const uint64_t key = a.keys[b];
            const Words w0 = philox(a.seed, key, TGP_MESH_SITE, 2u * (uint32_t)i);
            const Words w1 = philox(a.seed, key, TGP_MESH_SITE, 2u * (uint32_t)i + 1u);
            u = uniform_f64(w0.w[0], w0.w[1]), r1 = uniform_f64(w0.w[2], w0.w[3]), r2 = uniform_f64(w1.w[0], w1.w[1]);
        }
        const double x = u * total;
        const double *cum = a.cdf + r.f0;
        int lo = 0, hi = r.F;                                           // the first f with cum[f] >= x
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cum[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        face = min(lo, r.F - 1);
        double p[3][3], c[3];
        face_cross(a.verts, a.faces, r.v0, r.V, (size_t)r.f0 + face, p, c);
        const double s = __dsqrt_rn(r1);
        const double w0 = 1.0 - s, w1 = s * (1.0 - r2), w2 = s * r2;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = (w0 * p[0][k] + w1 * p[1][k]) + w2 * p[2][k];
        if (a.normals) {
            const double nrm = cross_norm(c);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[3 + k] = __ddiv_rn(c[k], nrm);
        }
    }
    if (a.f32) store_row((float *)a.out + row * cols, v, cols);
    else store_row((double *)a.out + row * cols, v, cols);
    if (a.face) a.face[row] = face;
}

}  // namespace

extern "C" int tgp_mesh_area_cdf(const float *verts, const int32_t *faces, const int32_t *vptr, const int32_t *fptr, int M, int n_verts,
                                 int n_faces, double *cdf, tgp_stream_t stream)
{
    TGP_REQUIRE(verts && faces && vptr && fptr && cdf && M > 0 && n_verts > 0 && n_faces > 0);
    hipLaunchKernelGGL(mesh_area_kernel, dim3(M), dim3(AREA_THREADS), 0, tgp_hs(stream), verts, faces, vptr, fptr, n_verts, n_faces, cdf);
    return TGP_LAUNCH_RESULT();
}

extern "C" int tgp_mesh_sample(const tgp_mesh_sample_args *a, tgp_stream_t stream)
{
    TGP_REQUIRE(a && a->verts && a->faces && a->vptr && a->fptr && a->cdf && a->job_mesh && a->out && a->status);
    TGP_REQUIRE(a->M > 0 && a->n_verts > 0 && a->n_faces > 0 && a->B >= 1 && a->n >= 1 && (a->u != nullptr) != (a->keys != nullptr));
    if (a->B > 65535) return TGP_EUNSUPPORTED;
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(tgp_cdiv(a->n, SAMPLE_THREADS), a->B), dim3(SAMPLE_THREADS), 0, tgp_hs(stream), *a);
    return TGP_LAUNCH_RESULT();
}
