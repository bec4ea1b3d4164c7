/*
 * tgpose.h -- C ABI of libtgpose_hip.so: the MI355X (gfx950) kernels behind the TG-Pose
 * point-cloud forward path and its Chamfer distance.
 *
 * Conventions (all entry points):
 *   - plain pointers are DEVICE pointers (fp32 row-major, int32 indices) unless noted;
 *   - every buffer, including scratch, is owned and sized by the caller; nothing is allocated,
 *     nothing synchronises; work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - `ld*` arguments are row strides in ELEMENTS, so operators read/write column slices of
 *     wider buffers (the 1286-channel concat buffer) in place;
 *   - return value: 0 = enqueued; > 0 = hipError_t from the launch; < 0 = TGP_E* argument error
 *     (nothing was enqueued).
 *
 * Each declaration cites the reference interface it replaces (paths under the TG-Pose tree).
 * The reference has exactly one native binding on this path -- the pybind module `chamfer_3D`
 * (losses/chamfer3D/chamfer_cuda.cpp:30-33) -- and otherwise composes torch ops in
 * network/fs_net_repo/gcn3d.py; the operator-level entry points below are what a native binding
 * of those functions would export.  INTEGRATION.md shows the Python-side stubs.
 */
#ifndef TGPOSE_H
#define TGPOSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGP_ABI_VERSION 9
#define TGP_EINVAL (-1)       /* null pointer / non-positive size / misaligned stride */
#define TGP_EUNSUPPORTED (-2) /* shape outside what the kernels are built for */

typedef void *tgp_stream_t; /* hipStream_t */

int tgp_version(void);
/* Node census of a captured hipGraph (hipGraph_t): counts[0..3] = kernel, memcpy, memset, other nodes.  Host-only, nothing is
 * launched.  No reference counterpart (the reference never captures); the step capture of this repo refuses a graph that holds
 * a MEMSET node -- the mark of an ATen multi-block reduction inside the capture ("captured step"). */
int tgp_graph_node_counts(void *hip_graph, int *counts);
/* largest point count per object / neighbour count the kNN kernels accept */
int tgp_knn_max_points(void);
int tgp_knn_max_k(void);

/* ---- geometry ---------------------------------------------------------------------------- */

/* PoseNet9D.py:48  `points - points.mean(dim=1, keepdim=True)`.
 * points (B,n,3) -> xyz_c (B,n,3), mean (B,3).  The column sums follow ATen's cascade order so
 * that the centred cloud is bit-identical to the CPU path (the kNN order depends on it). */
int tgp_center(const float *points, int B, int n, float *xyz_c, float *mean, tgp_stream_t stream);
/* (ABI 6) tgp_center that also clears zero_words 32-bit words at `zero` (the forward's zero-initialised scratch: max keys, range
 * flags, magnitude words, tickets) in the same launch; every later launch of the forward is ordered behind it. */
int tgp_center_zero(const float *points, int B, int n, float *xyz_c, float *mean, void *zero, int64_t zero_words, tgp_stream_t stream);

/* ---- graph construction ------------------------------------------------------------------- */

/* gcn3d.py:14-23 get_neighbor_index for 3-d coordinates.  xyz (B,n,3) packed -> idx (B,n,k):
 * the k+1 nearest by fl(fl(-2<a,b> + |b|^2) + |a|^2) ordered by (distance, index), rank 0 dropped. */
int tgp_knn_xyz(const float *xyz, int B, int n, int k, int32_t *idx, tgp_stream_t stream);

/* Bytes of scratch tgp_knn_feat needs for (B,n,d). */
int64_t tgp_knn_feat_workspace_bytes(int B, int n, int d);

/* gcn3d.py:14-23 get_neighbor_index in feature space (mode 'RF-F', gcn3d.py:149,201-206).
 * feat (B,n,d) with row stride ld; d a multiple of 32, d <= 480.
 * (ABI 9) The variant of this call that took a kernel form from the caller is removed: the library has one kernel per shape. */
int tgp_knn_feat(const float *feat, int ld, int B, int n, int d, int k, int32_t *idx, void *workspace,
                 int64_t workspace_bytes, tgp_stream_t stream);
/* (ABI 6) tgp_knn_feat that also leaves, beside each list, the unit directions from the point to its selected neighbours in the
 * level's coordinates xyz (B, n, 3) (gcn3d.py:48-58 get_neighbor_direction_norm): dirs (B, n, k) float4 = (x, y, z, 0), 16-byte
 * aligned -- what tgp_gconv_hs_fwd_dirs takes, so the graph convolution that walks the list needs no direction launch.  The fused
 * kernel's shapes only (d = 128 / 256, n <= 1056): TGP_EUNSUPPORTED otherwise, nothing launched. */
int tgp_knn_feat_dirs(const float *feat, int ld, int B, int n, int d, int k, int32_t *idx, void *workspace,
                      int64_t workspace_bytes, const float *xyz, float *dirs, tgp_stream_t stream);

/* gcn3d.py:26-35 get_nearest_index: for each of n target points the nearest of m source points
 * by fl(fl(|s|^2 + |t|^2) - 2<t,s>), lowest index on ties.  idx (B,n). */
int tgp_nn1(const float *target, const float *source, int B, int n, int m, int32_t *idx, tgp_stream_t stream);
/* (ABI 6) tgp_nn1 of the same targets against two clouds in one launch: the two nearest-coarse-point look-ups of the up-sampling
 * (FaceRecon.py:71-77).  Same results as two tgp_nn1 calls. */
int tgp_nn1_pair(const float *target, const float *source1, const float *source2, int B, int n, int m1, int m2, int32_t *idx1,
                 int32_t *idx2, tgp_stream_t stream);
/* (ABI 6) tgp_nn1_pair whose launch also writes tgp_fill_tail's columns for the targets (target = the centred cloud xyz_c):
 * feat[b, i, col0 ...] = one-hot(obj_id[b]) | target[b, i] | 0 ... up to ld.  feat NULL = tgp_nn1_pair. */
int tgp_nn1_pair_tail(const float *target, const float *source1, const float *source2, int B, int n, int m1, int m2, int32_t *idx1,
                      int32_t *idx2, const float *obj_id, int n_cls, float *feat, int ld, int col0, tgp_stream_t stream);

/* ---- graph convolution --------------------------------------------------------------------- */

/* F.normalize(directions, dim=0) (gcn3d.py:100,165).  directions (3,SC) -> out (3,SC). */
int tgp_normalize_dirs(const float *directions, int SC, float *out, tgp_stream_t stream);
/* its backward (round 3): out (3, SC) = d loss / d directions from grad (3, SC) = d loss / d normalised directions */
int tgp_normalize_dirs_bwd(const float *directions, const float *grad, int SC, float *out, tgp_stream_t stream);

/* gcn3d.py:91-106 HSlayer_surface.graph_conv.  xyz (B,n,3), idx (B,n,k), sdn (3,S*C) unit support
 * directions -> out (B,n,C) row stride ldo:  mean_s max_j relu(<dir_j, sdn[:, s*C+c]>).
 * xyz_pad != 0 (ldo >= C + 4): the row's columns C..C+3 also receive the point (x, y, z, 0), so that the caller's next GEMM can
 * take HSlayer_surface's STE convolution of xyz (gcn3d.py:79,87) as four more K columns (ABI 4). */
int tgp_gconv_surface_fwd(const float *xyz, const int32_t *idx, const float *sdn, int B, int n, int k, int S,
                          int C, float *out, int ldo, int xyz_pad, tgp_stream_t stream);

/* gcn3d.py:157-180 HS_layer.graph_conv after the dense projection.  proj (B*n, (S+1)*C) row stride
 * ldp holds [centre | support] = feature_map @ weights + bias; idx is the feature-space graph.
 * out = centre + mean_s max_j relu(<dir_j, sdn>) * support[idx_j].
 * dirs_ws: scratch of B*n*k*4 floats (16-byte aligned) for the unit neighbour directions (gcn3d.py:48-58), or NULL;
 * with it, clouds whose support table fits LDS in channel slices take the LDS-staged kernel (same results). */
int tgp_gconv_hs_fwd(const float *xyz, const int32_t *idx, const float *proj, int ldp, const float *sdn, int B,
                     int n, int k, int S, int C, float *out, int ldo, float *dirs_ws, tgp_stream_t stream);
/* (ABI 6) tgp_gconv_hs_fwd with the unit neighbour directions supplied (tgp_knn_feat_dirs): the LDS-staged kernel alone.
 * TGP_EUNSUPPORTED (nothing launched) where that kernel does not serve the shape: the caller uses tgp_gconv_hs_fwd. */
int tgp_gconv_hs_fwd_dirs(const float *xyz, const int32_t *idx, const float *proj, int ldp, const float *sdn, int B,
                          int n, int k, int S, int C, float *out, int ldo, const float *dirs, tgp_stream_t stream);

/* gcn3d.py:210-217 get_ORL_global: g[b,c] = mean_i max_j feat[b, idx[b,i,j], c].
 * partial: scratch of tgp_orl_partial_floats(B,n,C) floats.  out (B,C). */
int64_t tgp_orl_partial_floats(int B, int n, int C);
int tgp_orl_global(const float *feat, int ldf, const int32_t *idx, int B, int n, int k, int C, float *partial,
                   float *out, tgp_stream_t stream);

/* get_ORL_global followed by the global half of ORL_forward's conv2 (gcn3d.py:108-112,182-186):
 * g as above (optionally stored to g_out, may be NULL), rb[b,:] = g[b,:] @ W2^T with w2t = W2 transposed (C,C). */
int tgp_orl_rowbias(const float *feat, int ldf, const int32_t *idx, int B, int n, int k, int C, float *partial,
                    const float *w2t, float *g_out, float *rb, tgp_stream_t stream);
/* (ABI 5) the same, and feat -- the A operand of the layer's last GEMM (gcn3d.py:108-112: conv2's feature half) -- also written as
 * blocked fp16 planes (tgp_gemm_args.A_planes: `kts` K-tiles per row block, K-tile c / 16 for channel c) with the per-row-block
 * magnitudes in amax (zero-filled by the caller; may be NULL).  xyz_tile (may be NULL; HSlayer_surface): points (B*n, 3) written as
 * K-tile C / 16 = (x, y, z, 0, ...), the STE convolution's extra K columns.  TGP_EUNSUPPORTED where the LDS-staged form does not
 * serve the shape (the caller falls back to tgp_orl_rowbias and an fp32 operand). */
int tgp_orl_rowbias_planes(const float *feat, int ldf, const int32_t *idx, int B, int n, int k, int C, float *partial,
                           const float *w2t, float *g_out, float *rb, void *planes, int kts, uint32_t *amax, const float *xyz_tile,
                           tgp_stream_t stream);
/* (ABI 6) tgp_orl_rowbias / tgp_orl_rowbias_planes (planes may be NULL) as ONE launch: the pooling kernel finishes the mean over
 * points and the projection itself -- each of an object's C / 16 workgroups adds its 16-channel slice of g @ W2^T to `contrib`
 * (B * (C / 16) * C floats of scratch) and the last one to arrive (tickets: B ints, zero on entry, zero again on return) sums the
 * slices in chunk order, so rb does not depend on the arrival order.  rb agrees with tgp_orl_rowbias to rounding (another summation
 * order), g_out bit for bit.  TGP_EUNSUPPORTED (nothing launched) where the LDS-staged form does not serve the shape. */
int tgp_orl_rowbias_fused(const float *feat, int ldf, const int32_t *idx, int B, int n, int k, int C, const float *w2t,
                          float *g_out, float *rb, void *planes, int kts, uint32_t *amax, const float *xyz_tile, float *contrib,
                          int32_t *tickets, tgp_stream_t stream);

/* gcn3d.py:219-245 Pool_layer.forward with the random subsample (randperm, :242) supplied by the
 * host: out_f[b,m,:] = max_{j<kpool} feat[b, idx[b, sample[m], j], :], out_xyz[b,m] = xyz[b, sample[m]].
 * idx has row stride ldi (>= kpool) so the k=4 list may be the prefix of a longer one. */
int tgp_pool_fwd(const float *xyz, const float *feat, int ldf, const int32_t *idx, int ldi, const int32_t *sample,
                 int B, int n, int n_out, int kpool, int C, float *out_xyz, float *out_f, int ldo,
                 tgp_stream_t stream);
/* (ABI 5) the same, the pooled features also written as blocked fp16 planes (tgp_gemm_args.A_planes; kts >= C / 16 K-tiles per row
 * block) with their per-row-block magnitude words (amax, zero-filled by the caller; may be NULL): they are the A operand of the next
 * layer's projection GEMM.  C / 4 a divisor of 64, else TGP_EUNSUPPORTED. */
int tgp_pool_fwd_planes(const float *xyz, const float *feat, int ldf, const int32_t *idx, int ldi, const int32_t *sample, int B, int n,
                        int n_out, int kpool, int C, float *out_xyz, float *out_f, int ldo, void *planes, int kts, uint32_t *amax,
                        tgp_stream_t stream);

/* gcn3d.py:38-46 indexing_neighbor_new with one neighbour (FaceRecon.py:69-73 nearest up-sampling):
 * dst[b,i,0:C] = src[b, idx[b,i], 0:C]. */
int tgp_gather_rows(const float *src, int lds, const int32_t *idx, int B, int n_src, int n_out, int C, float *dst,
                    int ldd, tgp_stream_t stream);

/* FaceRecon.py:49-54,75-77 and PoseNet9D.py:63: the tail columns of the concat buffer:
 * one_hot(obj_id) (n_cls columns at col0), then the centred xyz (3), then zero padding up to ld. */
int tgp_fill_tail(const float *obj_id, const float *xyz_c, int B, int n, int n_cls, float *feat, int ld, int col0,
                  tgp_stream_t stream);

/* ---- dense per-point layers ------------------------------------------------------------------ */

typedef struct tgp_gemm_args {
    /* C[m, n] = act( (sum_k A[m,k] * W[n,k] + bias[n] + rowbias[m / rows_per_obj, n]
     *                 + res1[m,n] + res2[m,n]) * scale[n] + shift[n] )
     * A (M,K) row stride lda; W (N,K) row stride ldw (Conv1d/Linear weight layout, FaceRecon.py:93-110,
     * PoseR.py:16-19); K, lda, ldw multiples of 4; every optional pointer may be NULL. */
    const float *A; int lda;
    const float *W; int ldw;
    float *C; int ldc;                 /* may be NULL when only colmax is wanted */
    int M, N, K;
    const float *bias;                 /* [N] */
    const float *rowbias; int ldrb;    /* [(M / rows_per_obj), N] */
    int rows_per_obj;
    const float *res1; int ldr1;
    const float *res2; int ldr2;
    const float *scale;                /* [N] eval-mode BatchNorm fold: gamma / sqrt(var + eps) */
    const float *shift;                /* [N] beta - mean * scale */
    int act;                           /* 0 none, 1 leaky-relu with `slope` (0 -> ReLU) */
    float slope;
    uint32_t *colmax_keys; int ldcm;   /* [(M / rows_per_obj), cm_cols] order-preserving keys, zero-filled by the
                                          caller; decoded by tgp_colmax_decode (torch.max(x, 2), PoseR.py:30) */
    /* Column ranges let ONE launch serve several layers that read the same rows (conv_5 and the three
     * head conv1 layers all read `feat`): per-column slope, colmax only for the first cm_cols columns,
     * C stored only for columns >= c_col0 (at C[m * ldc + n - c_col0]). */
    const float *slope_vec;            /* [N] per-column leaky slope, overrides `slope`; may be NULL */
    int cm_cols;                       /* 0 = all N columns */
    int c_col0;
    /* batch > 1: `batch` independent problems of the same shape in one launch; operand b starts at
     * A + b*batch_stride_a etc. (element strides; vec = bias/scale/shift/slope_vec). */
    int batch;
    int64_t batch_stride_a, batch_stride_w, batch_stride_c, batch_stride_vec, batch_stride_colmax;
    /* Optional: W pre-split into three bf16 terms by tgp_split_bf16 ([batch*N][ldws/16][3][16], ldws % 16 == 0).  When
     * given, launches that are large enough for the tile kernels run on the bf16 matrix cores with the
     * 3-term operand split (six MFMA terms, fp32 accumulate): fp32-level accuracy at 2.67x fewer MFMA cycles.
     * W itself is still required (small launches and the skinny kernel read it). */
    const uint16_t *W_split; int ldws;
    /* 0: W_split holds the three bf16 planes of tgp_split_bf16 (any fp32-range operands);
     * 1: the two fp16 planes of tgp_split_f16 ([batch*N][ldws/16][2][16]) -- three MFMA terms instead of six, products
     *    accurate to ~2^-22; requires |A|, |W| < 65504 (an out-of-range operand yields inf/NaN, never a wrong finite
     *    number) */
    int w_split_kind;
    /* Backward GEMMs on the fp16 split (w_split_kind 1 only; all three optional).  Gradients lie far below fp16's range, so
     * the caller picks a power of two s with max|A| * s < 65504 (tgp_absmax_scale): A is multiplied by *a_scale before it is
     * split, the accumulated sums by *c_scale (= 1 / s, or 1 when a later pass unscales) before the epilogue.  Both are
     * device pointers, so the scale of a step is chosen on the device and the step stays capturable in a graph.
     * ksplit_chunk > 0: split-K -- the `batch` problems are consecutive K-chunks of ONE problem: problem b reads
     * A[:, b*chunk : b*chunk + K], the W_split K-tiles from b*chunk on, and writes C + b*batch_stride_c (partial sums the
     * caller adds up, tgp_sum_slabs); chunk % 16 == 0, operands zero-padded so that every chunk holds K columns. */
    const float *a_scale, *c_scale;
    int ksplit_chunk;
    /* Gathered residuals (tile kernels only, M > 32): C[m, n] gains gres1[gidx1[m], n] + gres2[gidx2[m], n] before the
     * per-object bias and the BatchNorm fold.  This is how a layer over `feat` = [fine | up(coarse1) | up(coarse2)] (nearest
     * upsampling, FaceRecon.py:70-75) runs factored: W_coarse x coarse features is computed once per COARSE point (4x / 16x
     * fewer rows) and each point fetches the rows of its nearest coarse points, instead of multiplying upsampled copies.
     * gidx: int32 per output row, absolute row of gres; excludes res1 / res2; rows_per_obj >= 64 with rowbias / colmax. */
    const float *gres1; int ldg1; const int32_t *gidx1;
    const float *gres2; int ldg2; const int32_t *gidx2;
    /* 0: the library picks the epilogue form (LDS-staged 16-byte form when every operand is 16-byte addressable).
     * 1: the register-direct form (4-byte accesses; same arithmetic in the same order, bit-identical results; slower --
     *    a per-call A/B handle for tests, not a tuning knob; not available with gathered residuals). */
    int epilogue;
    /* Predicate (may be NULL): a device int; while it is 0 the launch does nothing (every workgroup returns at once).  For
     * repair launches whose condition is raised on the device -- tgp_heads_fused's overflow flag -- without a host read.
     */
    const int *pred;
    /* (ABI 4) The launch covers rows [row_base, row_base + M) of a batch whose objects are rows_per_obj rows each: the
     * per-object bias and the max over an object's points address object (row + row_base) / rows_per_obj.  A / C / residual /
     * gather-index pointers are those of the launch's first row, as always.  0 for whole-batch launches.  (The eval forward
     * hands the last rows of the heads' layers to the tile kernels beside the fused kernel: engine.wide_gemm_factored.) */
    int row_base;
    /* (ABI 5) Operands and results as BLOCKED fp16 planes.  A row-major fp32 matrix X (rows, K) in this form is
     * tgp_planes_bytes(rows, K) bytes: for each block of 32 rows and each 16-wide K-tile a 2 KB chunk
     *     [plane: hi | lo][h = (k % 16) / 8][r = row % 32][8 fp16],      x = hi + lo to ~2^-23 (the split of tgp_split_f16),
     * chunks ordered [row block][K-tile], `kt` K-tiles per row block (>= ceil(K / 16); rows and columns past the end are zero).
     * One plane of a chunk is 1 KB in the lane order of v_mfma_f32_32x32x16_f16's operand, so the kernels stage it by LDS-DMA and
     * never convert in their K loop.
     *   A_planes + W_planes (both or neither): the launch runs on the pre-split kernel (csrc/gemm_pp.hip); batch == 1, no
     *     a_scale / ksplit_chunk; every epilogue operand 16-byte addressable.  Results are bit-identical to the launch without
     *     them (same products, same order).  a_amax (may be NULL = unguarded): per 32-row block of A the bits of its largest
     *     magnitude, as tgp_planes_split / a producing launch's c_amax wrote them: a tile whose blocks hold a magnitude
     *     >= 65504 (or a NaN), or nothing >= 2^-4, is computed in exact fp32 from A / W, which are still required then.
     *   C_planes: the result (the columns >= c_col0) is ALSO written as planes, column c_col0 landing at plane column cp_col0
     *     (% 16 == 0), N - c_col0 a multiple of 16; c_amax (zero-filled by the caller once per tensor) receives the per-block
     *     magnitudes.  Tile kernels with the 16-byte epilogue only (the launch is refused otherwise).  C may be NULL.
     * pp_config: 0 = the library picks the tile shape; 1 .. 7 force one (tests, tuning scripts). */
    const void *A_planes; int a_kt; const uint32_t *a_amax;
    const void *W_planes; int w_kt;
    void *C_planes; int c_kt; int cp_col0; uint32_t *c_amax;
    int pp_config;
    /* (ABI 5) Planes-only tensors.  With C_planes, C and colmax_keys may both be NULL: the result exists as planes only.  A launch
     * whose A_planes come without the fp32 operand (A == NULL) cannot recompute a tile that its magnitude words put outside fp16's
     * comfortable range: it computes the tile on the split anyway and sets *range_flag = 1 (device int, zeroed by the caller;
     * required then) -- the caller follows the chain with its fp32 form predicated on that flag (`pred`), as tgp_heads_fused's
     * callers do.  A chain of layers whose activations feed only the next GEMM (the decoder, FaceRecon.py:112-117) then writes and
     * reads 4 bytes per element instead of 8 + 4. */
    int *range_flag;
    /* (ABI 6) The per-object vector layers (M <= 32, the weight-streaming kernel; refused elsewhere), FaceRecon.py:145-165:
     *   a_keys != 0: A holds the order-preserving max keys a colmax_keys launch left (uint32), decoded as they are loaded -- no
     *     decode launch; a_wrap > 0 (% 4 == 0): column k of the operand is key k % a_wrap, i.e. cat((max, max), 1)
     *     (FaceRecon.py:148) is never built.
     *   C_sigmoid != NULL: 1 / (1 + exp(-v)) of every stored value is also written there (row stride ldc): the PH predictor's
     *     nn.Sigmoid (FaceRecon.py:156,162) without a launch of its own. */
    int a_keys; int a_wrap;
    float *C_sigmoid;
} tgp_gemm_args;

/* W (rows, K) fp32, row stride ld -> out[rows][ldo/16][3][16] bf16: per 16-wide K-tile the hi, mid and lo terms
 * (x = hi+mid+lo to 2^-24) stored back to back; columns K..ldo-1 zero.  3*rows*ldo elements.  Done once per
 * weight version. */
int tgp_split_bf16(const float *W, int rows, int K, int ld, uint16_t *out, int ldo, tgp_stream_t stream);
/* Same for the two-term fp16 split: out[rows][ldo/16][2][16] (hi, lo), 2*rows*ldo elements. */
int tgp_split_f16(const float *W, int rows, int K, int ld, uint16_t *out, int ldo, tgp_stream_t stream);

/* (ABI 5) bytes of the blocked fp16 planes of a (rows, K) matrix (tgp_gemm_args.A_planes), and the split itself: X (rows, K) fp32
 * with row stride ld -> out (kts >= ceil(K / 16) K-tiles per row block; padding rows / columns zero); amax (may be NULL; ceil(rows /
 * 32) words, zero-filled by the caller) receives atomicMax of the bits of |x| per row block.  Weights at pack time; activations
 * whose producer does not write planes itself. */
int64_t tgp_planes_bytes(int64_t rows, int K);
int tgp_planes_split(const float *X, int rows, int K, int ld, void *out, int kts, uint32_t *amax, tgp_stream_t stream);
/* the same into a column range of a wider planes buffer: X's K columns land at plane columns col0 .. col0 + K - 1 (col0 % 16 == 0;
 * only those ceil(K / 16) K-tiles of each row block are written, the last one zero padded) */
int tgp_planes_split_cols(const float *X, int rows, int K, int ld, void *out, int kts, int col0, uint32_t *amax, tgp_stream_t stream);
/* tgp_gather_rows and tgp_planes_split in one pass: dst[b][p][0..C) = src[b][idx[b][p]][0..C) (dst may be NULL) and the planes of
 * the gathered rows' first K columns (columns K.. of the planes zero); kts * 16 >= C when dst is given. */
int tgp_planes_gather(const float *src, int lds, const int32_t *idx, int B, int n_src, int n_out, int K, int C, float *dst, int ldd,
                      void *out, int kts, uint32_t *amax, tgp_stream_t stream);

/* nn.Conv1d(kernel 1) / nn.Linear on channel-last rows with the fused epilogue above. */
int tgp_gemm_f32(const tgp_gemm_args *args, tgp_stream_t stream);

/* keys (rows, N) row stride ldk -> out[r, n] (row stride ldo) and, if out2 != NULL, a second copy
 * (FaceRecon.py:145-147 concatenates the pooled vector with itself). */
int tgp_colmax_decode(const uint32_t *keys, int ldk, int rows, int N, float *out, int ldo, float *out2,
                      tgp_stream_t stream);

/* PoseNet9D.py:50 feat_global.max(2): out[b,c] = max_i x[b,i,c], x (B,n,C) row stride ld. */
int tgp_colmax(const float *x, int ld, int B, int n, int C, float *out, tgp_stream_t stream);

/* FaceRecon.py:156,162 nn.Sigmoid on a contiguous vector. */
int tgp_sigmoid(const float *x, float *y, int64_t count, tgp_stream_t stream);

/* PoseNet9D.py:57-66: green/red (B,4) -> unit axes p_* (B,3) and confidences f_* (B); ts (B,6) + mean
 * -> Pred_T (B,3), Pred_s (B,3).  ldg / ldr / ldt: row strides of green / red / ts (ABI 4: the batched head tail writes the three
 * heads' outputs as rows of one (3, B, 8) buffer, read here in place). */
int tgp_head_post(const float *green, const float *red, const float *ts, int ldg, int ldr, int ldt, const float *mean, int B,
                  float *p_green, float *p_red, float *f_green, float *f_red, float *pred_T, float *pred_s, tgp_stream_t stream);

/* (ABI 6) The three pose heads after their max over points as ONE launch (PoseR.py:37-43, PoseTs.py:43-49 in eval mode, then
 * PoseNet9D.py:57-66): keys2 (3, B, 256) the order-preserving max keys of conv2's output (heads rot_green, rot_red, ts);
 * w3t (3, 256, 256) conv3's weights TRANSPOSED (input channel major); b3 / scale3 / shift3 (3, 256) bias and BatchNorm fold;
 * w4 (3, 8, 256) conv4 with its 4 / 4 / 6 rows zero-padded to 8, b4 (3, 8); outputs as tgp_head_post's; raw (may be NULL)
 * receives conv4's (3, B, 8) outputs. */
int tgp_pose_tail(const uint32_t *keys2, const float *w3t, const float *b3, const float *scale3, const float *shift3,
                  const float *w4, const float *b4, const float *mean, int B, float *p_green, float *p_red, float *f_green,
                  float *f_red, float *pred_T, float *pred_s, float *raw, tgp_stream_t stream);

/* (ABI 6) A per-point layer with n_out <= 4 outputs whose rows leave in another order -- the decoder's last conv
 * (FaceRecon.py:117) behind the row sort of the factored layers: out[obj, map[obj, i], j] = bias[j] + sum_k x[obj, i, k] W[j, k]
 * for the `rows` rows of x (row stride ld, K % 4 == 0), objects of rows_per_obj rows; map (int64, relative to the object; NULL =
 * identity); out (rows, n_out) contiguous.  TGP_EUNSUPPORTED for other n_out. */
int tgp_rows_out(const float *x, int ld, int64_t rows, int K, const float *W, int ldw, const float *bias, int n_out,
                 const int64_t *map, int rows_per_obj, float *out, tgp_stream_t stream);
/* (ABI 7) the same, predicated: the launch returns at once while *pred == 0 (pred may be NULL: always runs) -- the last step of a repair
 * chain (tgp_gemm_args.pred) whose result replaces tgp_dec_fused's rows */
int tgp_rows_out_pred(const float *x, int ld, int64_t rows, int K, const float *W, int ldw, const float *bias, int n_out,
                      const int64_t *map, int rows_per_obj, float *out, const int *pred, tgp_stream_t stream);

/* PoseNet9D.py:71 recon + mean, in place on recon (B,n,3). */
int tgp_add_mean(float *recon, const float *mean, int B, int n, tgp_stream_t stream);

/* ---- training-mode BatchNorm / dropout ------------------------------------------------------- */

/* nn.BatchNorm1d in train mode on channel-last rows x (rows, C) with row stride ld: per-channel batch mean and
 * BIASED variance (deterministic: one pass of shifted sums merged in chunk order when the rows are 16-byte addressable, two
 * passes otherwise).  workspace: tgp_bn_workspace_floats(rows, C) floats. */
int64_t tgp_bn_workspace_floats(int64_t rows, int C);
int tgp_bn_stats(const float *x, int ld, int64_t rows, int C, float *mean, float *var, float *workspace,
                 tgp_stream_t stream);
/* tgp_bn_stats that also moves nn.BatchNorm1d's buffers (ABI 4): run_mean / run_var (C) <- (1 - momentum) x running + momentum x
 * batch value, the variance with the unbiased factor rows / (rows - 1) (torch's `running.mul_(1 - m).add_(batch, alpha = m)`);
 * batches (one int64, may be NULL) += 1 (num_batches_tracked).  run_mean == run_var == NULL: statistics only. */
int tgp_bn_stats_running(const float *x, int ld, int64_t rows, int C, float *mean, float *var, float *workspace, float *run_mean,
                         float *run_var, float momentum, int64_t *batches, tgp_stream_t stream);

/* y = (x - mean) / sqrt(var + eps) * gamma + beta, then leaky-relu (act = 1; per-column slope_vec overrides slope);
 * out may alias x or be NULL; colmax_keys as in tgp_gemm_args (max over each object's rows_per_obj rows for the
 * first cm_cols columns). */
int tgp_bn_apply(const float *x, int ld, int64_t rows, int C, const float *mean, const float *var,
                 const float *gamma, const float *beta, float eps, int act, float slope, const float *slope_vec,
                 float *out, int ldo, uint32_t *colmax_keys, int ldcm, int cm_cols, int rows_per_obj,
                 tgp_stream_t stream);

/* nn.Dropout(p) in train mode with the keep mask (uint8 0/1) supplied by the host: y = keep ? x / (1 - p) : 0. */
int tgp_dropout_apply(const float *x, const uint8_t *keep, float p, int64_t count, float *y, tgp_stream_t stream);

/* ---- Chamfer distance ------------------------------------------------------------------------ */

/* chamfer_3D.forward (losses/chamfer3D/chamfer_cuda.cpp:17-19,31; kernels chamfer3D.cu:12-152).
 * xyz1 (B,n,3), xyz2 (B,m,3) -> dist1 (B,n), idx1 (B,n) nearest in xyz2; dist2 (B,m), idx2 (B,m)
 * nearest in xyz1.  Squared distance (dx*dx + dy*dy) + dz*dz in fp32, lowest index on ties. */
int tgp_chamfer_fwd(const float *xyz1, const float *xyz2, int B, int n, int m, float *dist1, float *dist2,
                    int32_t *idx1, int32_t *idx2, tgp_stream_t stream);

/* chamfer_3D.backward (chamfer_cuda.cpp:22-27,32; chamfer3D.cu:155-195): ACCUMULATES into
 * gradxyz1 (B,n,3) / gradxyz2 (B,m,3) (the caller zero-fills, dist_chamfer_3D.py:56-60).
 * Deterministic: contributions are summed in the serial order of the reference's CPU loop
 * (tools/pyTorchChamferDistance/chamfer_distance.cpp:140-175), no atomics. */
int tgp_chamfer_bwd(const float *xyz1, const float *xyz2, int B, int n, int m, const float *graddist1,
                    const float *graddist2, const int32_t *idx1, const int32_t *idx2, float *gradxyz1,
                    float *gradxyz2, tgp_stream_t stream);

/* ---- density-aware Chamfer loss (config 3: forward + Chamfer loss) ------------------------------ */

/* calc_dcd after the Chamfer search (losses/TDA_loss_sym_recon.py:427-445): per object
 * loss = mean_i(1 - exp(-alpha d1_i) w1_i) + 0.5 mean_j(1 - exp(-alpha d2_j) w2_j),
 * w1_i = frac_21 / (count1[idx1_i]^n_lambda + 1e-6) with count1 = bincount(idx1) (w2 likewise, frac_12).
 * loss (B); w1 (B,n), w2 (B,m) are optional outputs kept for the backward pass. n, m <= 4096. */
int tgp_dcd_fwd(const float *dist1, const float *dist2, const int32_t *idx1, const int32_t *idx2, int B, int n,
                int m, float alpha, float n_lambda, int non_reg, float *loss, float *w1, float *w2,
                tgp_stream_t stream);

/* Gradient of the above w.r.t. the distances (the weights are detached, :433,438): graddist1 (B,n), graddist2 (B,m)
 * from gloss (B); they feed tgp_chamfer_bwd. */
int tgp_dcd_bwd(const float *dist1, const float *dist2, const float *w1, const float *w2, const float *gloss,
                int B, int n, int m, float alpha, float *graddist1, float *graddist2, tgp_stream_t stream);

/* ---- earth mover's distance by auction matching (csrc/emd.hip; additive, ABI stays 8) ----------- */

/* emd.forward (losses/metrics/EMD/emd_module.py:41-80; kernels emd_cuda.cu:95-226), all `iters` auction iterations and the
 * distance pass in ONE launch, one workgroup per cloud pair with the pair's state in LDS.  xyz1, xyz2 (B,n,3) with coordinates
 * in [0,1] -> assignment (B,n) int32 (the point of xyz2 matched to each point of xyz1; a bijection once the auction has
 * converged, not necessarily before) and dist (B,n) the squared distances to it.  Any 1 <= n <= tgp_emd_max_points() (the
 * reference wants n % 1024 == 0) and any B >= 1; TGP_EINVAL for iters < 1, TGP_EUNSUPPORTED above the cap.  The arithmetic is
 * DESIGN.md "EMD": the reference's, with its one race (the winner among equal bidders) fixed to the lowest bidder.  Bit-repeatable
 * and independent of the batch around a pair; no float atomics.  ws: tgp_emd_workspace_bytes(B, n) bytes (0 up to the cap: may
 * be NULL). */
int tgp_emd_max_points(void);
int64_t tgp_emd_workspace_bytes(int B, int n);
int tgp_emd_fwd(const float *xyz1, const float *xyz2, int B, int n, float eps, int iters, float *dist, int32_t *assignment,
                void *ws, tgp_stream_t stream);
/* emd.backward (emd_cuda.cu:284-316): grad_xyz1 (B,n,3) = (grad_dist * 2) * (xyz1 - xyz2[assignment]), WRITTEN (not
 * accumulated); the gradient for xyz2 is zero, as the reference returns. */
int tgp_emd_bwd(const float *xyz1, const float *xyz2, const float *grad_dist, const int32_t *assignment, int B, int n,
                float *grad_xyz1, tgp_stream_t stream);

/* ---- farthest point sampling (csrc/fps.hip; additive, ABI stays 8) ------------------------------ */

/* farthest_points (core/utils/farthest_points_torch.py:6-62, dist_func = F.pairwise_distance), all n steps of every cloud in ONE
 * launch, one workgroup per cloud with the cloud and its running distances in registers.  xyz (B,M,ld) rows of ld = 3 or 4
 * floats (4: the padded rows tgp_augment writes; the fourth is not read); counts (B) int32, may be NULL (= M): cloud b is its
 * first counts[b] rows, 1 <= counts[b] <= M (values outside are clamped).  init_center != 0: the running distances start as the
 * distances to start (B,3), or with start NULL to the cloud's centroid, summed as the pairwise tree over the row index and divided
 * by (float)counts[b] (DESIGN.md section 3 "Farthest point sampling": it does not depend on M or on the batch); init_center == 0:
 * they start at 1e7f (the first centre is row 0) and start is not read.
 * -> idx (B,n) int32: for counts[b] > n the n centres in selection order (each the lowest row of the maximum running distance);
 * for counts[b] <= n no step runs and idx[i] = i % counts[b] (_sample_points' tiling).  dist_out (B,M) / clusters_out (B,M) int32,
 * each may be NULL: the final running distances and, per row, the last step whose centre came at least as close as every centre
 * before it (-1: none; the reference's `clusters`); with counts[b] <= n the initial distances and -1.  Rows at and beyond
 * counts[b] are not written.  The arithmetic is the reference's bit for bit; bit-repeatable, no atomics.
 * Any 1 <= M <= tgp_fps_max_points(), n >= 1, B >= 1; TGP_EUNSUPPORTED above the cap. */
int tgp_fps_max_points(void);
int tgp_fps(const float *xyz, int ld, const int32_t *counts, int B, int M, int n, const float *start, int init_center,
            int32_t *idx, float *dist_out, int32_t *clusters_out, tgp_stream_t stream);

/* ---- depth renderer (csrc/render.hip; additive, ABI stays 8) -------------------------------------- */

/* A z-buffer rasteriser of posed triangle meshes: S scenes in one call, every output a function of the inputs alone (DESIGN.md
 * section 3 "The depth renderer" states the arithmetic; tests/render_ref.py restates it in numpy and the two agree bit for bit).
 * Mesh set: verts (n_verts,3) fp32 model units; faces (n_faces,3) int32 LOCAL to their mesh; vptr, fptr (M+1) int32 prefix sums.
 * Scene set: scene_ptr (S+1) int32 into the instance arrays; inst_mesh (I) int32; inst_id (I) uint8 in 1..255; inst_pose (I,3,4)
 * fp32 [s R | t], model -> camera in metres; camk (S,4) fp32 = fx, fy, cx, cy.  Everything lives on the device; the host states only
 * sizes and bounds: max_verts / max_faces (the largest mesh; a longer mesh is cut to them) and max_scene_inst (the longest scene).
 * -> depth (S,H,W) uint16 millimetres, mask (S,H,W) uint8 instance id, both 0 where no surface; z (S,H,W) fp32 metres, +inf where
 * empty, and face (S,H,W) int32 (index within the mesh, -1 where empty), each may be NULL; visible (I) int32 pixels won; bbox (I,4)
 * int32 (y1,x1,y2,x2), y2/x2 exclusive, zeros when invisible; dropped (S,2) int32: triangles with a vertex at p_z <= near, triangles
 * with a snapped coordinate beyond 2^22 sub-pixel units.  A mesh index outside [0,M), a face index outside its mesh and rows of
 * vptr / fptr that leave the arrays render nothing.  workspace: tgp_render_workspace_bytes(I, max_verts, max_faces) bytes.
 * TGP_EINVAL: a NULL required pointer, S, M, H, W, max_verts or max_faces < 1, I < 0, near <= 0 or not finite.  TGP_EUNSUPPORTED:
 * max_faces >= tgp_render_max_faces() (2^24), max_scene_inst > tgp_render_max_instances() (255), H or W > 16384.  Nothing is
 * launched on an error.  Three kernels (vertices, triangle boxes, tiles) and one over the instances; graph-capturable. */
typedef struct {
    const float *verts;
    const int32_t *faces;
    const int32_t *vptr, *fptr;
    int M, n_verts, n_faces, max_verts, max_faces;
    const int32_t *scene_ptr;
    const int32_t *inst_mesh;
    const uint8_t *inst_id;
    const float *inst_pose;
    const float *camk;
    int S, I, max_scene_inst;
    int H, W;
    float near;
    void *workspace;
    uint16_t *depth;
    uint8_t *mask;
    float *z;          /* may be NULL */
    int32_t *face;     /* may be NULL */
    int32_t *visible;
    int32_t *bbox;
    int32_t *dropped;
} tgp_render_args;
int tgp_render_max_faces(void);
int tgp_render_max_instances(void);
int64_t tgp_render_workspace_bytes(int I, int max_verts, int max_faces);
int tgp_render_depth(const tgp_render_args *args, tgp_stream_t stream);

/* TDA_loss.R_DCD pose normalisation (:326-339): R from the predicted axes p_g, p_r (B,3) and confidences f_g, f_r
 * (B) -- for objects with sym[b*sym_ld] == 1 the green axis is paired with column 0 of the true rotation gR (B,3,3)
 * -- then out[b,i] = (R^T (points[b,i] - p_t[b])) * p_s[b].  R_out (B,3,3) optional. */
int tgp_canonicalize(const float *points, const float *gR, const float *p_g, const float *f_g, const float *p_r,
                     const float *f_r, const float *p_t, const float *p_s, const float *sym, int sym_ld, int B,
                     int n, float *out, float *R_out, tgp_stream_t stream);

/* Pose assembly of the evaluater: generate_RT([p_green, p_red], [f_green, f_red], T, mode='vec', sym)
 * (evaluater/RT_TDA_Evaluater.py:94; tools/rot_utils.py:95-98 to_R_matrices).  rt (B,4,4); sym may be NULL. */
int tgp_generate_rt(const float *p_green, const float *p_red, const float *f_green, const float *f_red,
                    const float *T, const float *sym, int sym_ld, int B, float *rt, tgp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Backward pass of the dense per-point layers (what torch autograd runs for nn.Conv1d(k=1) / nn.Linear /
 * nn.BatchNorm1d(train) / F.relu / F.leaky_relu / torch.max in loss.backward(), trainer/RL_TDA.py:205-224).
 * ------------------------------------------------------------------------------------------------------------------ */

/* C (N, K) (+)= A^T B over the rows: C[n][k] = sum_m A[m][n] * B[m][k]  (weight gradient dW = dx^T a).
 * workspace: tgp_gemm_tn_workspace_floats(rows, N, K) floats.  Row slices are summed in slice order (deterministic). */
int64_t tgp_gemm_tn_workspace_floats(int64_t rows, int N, int K);
int tgp_gemm_tn_f32(const float *A, int lda, const float *B, int ldb, int64_t rows, int N, int K, float *C, int ldc,
                    int accumulate, float *workspace, tgp_stream_t stream);

/* out[c] (+)= sum over rows of dy[r][c] (bias gradient).  workspace: tgp_bw_workspace_floats(rows, C). */
int64_t tgp_bw_workspace_floats(int64_t rows, int C);
int tgp_colsum(const float *dy, int lddy, int64_t rows, int C, float *out, int accumulate, float *workspace, tgp_stream_t stream);

/* y = act(BN_train(x)) backward: dz = dy * act'(z); dgamma = sum dz*xhat; dbeta = sum dz;
 * dx = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)).  x is the raw layer output the forward normalised, mean / var
 * its batch statistics (tgp_bn_stats).  dx may alias dy.  workspace: tgp_bw_workspace_floats(rows, C). */
int tgp_bn_bwd(const float *dy, int lddy, const float *x, int ld, int64_t rows, int C, const float *mean, const float *var,
               float eps, const float *gamma, const float *beta, int act, float slope, const float *slope_vec, float *dx,
               int lddx, float *dgamma, float *dbeta, float *workspace, uint32_t *absmax_bits, tgp_stream_t stream);
/* absmax_bits (round 3; NULL = not wanted): tgp_bn_bwd_absmax_words(rows, C) words, one per workgroup of the apply pass, that
 * receive the bit patterns of max |dx| -- the number the next layer's backward needs for its fp16 scale
 * (tgp_absmax_scale_from_bits over these words instead of tgp_absmax_scale's pass over dx).  Collected by the
 * 16-byte form only (C % 4 == 0, strides % 4 == 0, 16-byte aligned operands): TGP_EUNSUPPORTED otherwise. */
int64_t tgp_bn_bwd_absmax_words(int64_t rows, int C);
int tgp_absmax_scale_from_bits(const uint32_t *bits, int n, float target, float *out, tgp_stream_t stream);

/* The same for a layer followed by a max over each object's points: dpool (objects, C) is the gradient of the pooled
 * vector, argrow (objects, C) the winning global row from tgp_colmax_arg; dx (objects*rows_per_obj, C) is dense. */
int tgp_bn_bwd_pooled(const float *dpool, int ldp, const int *argrow, int lda, const float *x, int ld, int objects,
                      int rows_per_obj, int C, const float *mean, const float *var, float eps, const float *gamma,
                      const float *beta, int act, float slope, const float *slope_vec, float *dx, int lddx, float *dgamma,
                      float *dbeta, tgp_stream_t stream);

/* out[o][c] = max over the object's n rows of act(BN(x)) (mean == NULL: of x), argrow[o][c] = the winning global row
 * (first on ties, as torch.max). */
int tgp_colmax_arg(const float *x, int ld, int objects, int n, int C, const float *mean, const float *var, float eps,
                   const float *gamma, const float *beta, int act, float slope, const float *slope_vec, float *out, int ldo,
                   int *argrow, int lda, tgp_stream_t stream);

/* out[o][c] = sum over object o's n rows of dy (objects*n, C): gradient of a per-object bias broadcast over the object's points
 * (gcn3d.py:108-112 ORL_forward's global half; FaceRecon.py:165); fixed summation order. */
int tgp_colsum_objects(const float *dy, int ld, int objects, int n, int C, float *out, int ldo, tgp_stream_t stream);

/* Backward of tgp_colmax_arg without BatchNorm (PoseNet9D.py:50 feat_global = feat.max over points): dx (objects*rows_per_obj, C)
 * = dpool[o][c] on the recorded winning row, 0 elsewhere; written densely, deterministic. */
int tgp_colmax_bwd(const float *dpool, int ldp, const int *argrow, int lda, int objects, int rows_per_obj, int C, float *dx, int lddx,
                   tgp_stream_t stream);

/* dst (cols, rows) = src (rows, cols)^T. */
int tgp_transpose(const float *src, int ld_src, int rows, int cols, float *dst, int ld_dst, tgp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Backward pass of the graph layers (the `_bwd` entry points of SURVEY.md section 8b, seam #2).  Scatters use hardware
 * float atomics (as the reference's CUDA autograd does for index / max backward); d* outputs that are scattered into
 * must be zero-initialised (or hold a gradient to accumulate onto) by the caller.
 * ------------------------------------------------------------------------------------------------------------------ */

/* HSlayer_surface.graph_conv (gcn3d.py:91-106): dg (B,n,C) -> dsdn (3, S*C), the gradient w.r.t. the unit support
 * directions (F.normalize's own backward stays with the caller).  workspace: tgp_gconv_bwd_workspace_floats(B, n, C).
 * C >= 128 with 256 % C == 0 or C % 256 == 0, k <= 64 (the kernel stages two 16-point streams per workgroup): a narrower C is
 * TGP_EUNSUPPORTED, here and in tgp_gconv_hs_bwd, and nothing is launched. */
int64_t tgp_gconv_bwd_workspace_floats(int B, int n, int C);
int tgp_gconv_surface_bwd(const float *xyz, const int32_t *idx, const float *sdn, const float *dg, int ldg, int B, int n, int k,
                          int S, int C, float *dsdn, float *workspace, tgp_stream_t stream);

/* HS_layer.graph_conv (gcn3d.py:157-180): proj (B,n,>=8C) = [centre | 7 support blocks] as in tgp_gconv_hs_fwd;
 * dproj (same layout) += d centre, d support (scatter to the arg-max neighbour); dsdn (3, S*C) as above. */
int tgp_gconv_hs_bwd(const float *xyz, const int32_t *idx, const float *proj, int ldp, const float *sdn, const float *dg, int ldg,
                     int B, int n, int k, int S, int C, float *dproj, int lddp, float *dsdn, float *workspace, tgp_stream_t stream);

/* y[b][p][c] = max_j src[b][idx[b][p][j]][c], p < n_rows (get_ORL_global's and Pool_layer's neighbour max):
 * dsrc[b][arg][c] += dy.  per_object != 0: dy is (B, C) and every row receives dy[b][c] * scale (the mean over the
 * points that follows in get_ORL_global: scale = 1 / n); else dy is (B*n_rows, C). */
int tgp_nbrmax_bwd(const float *src, int ld_src, const int32_t *idx, int B, int n_src, int n_rows, int k, int C, const float *dy,
                   int lddy, int per_object, float scale, float *dsrc, int ld_dsrc, tgp_stream_t stream);

/* tgp_gather_rows backward: dsrc[b][idx[b][p]][:] += dy[b][p][:]. */
int tgp_gather_rows_bwd(const float *dy, int lddy, const int32_t *idx, int B, int n_src, int n_out, int C, float *dsrc,
                        int ld_dsrc, tgp_stream_t stream);

/* Differentiable half of TDA_loss.R_DCD's canonicalisation (losses/TDA_loss_sym_recon.py:334-337):
 * out[b][i] = (R[b]^T (points[b][i] - t[b])) * s[b]; R (B,3,3) row-major, t, s (B,3).  The backward returns dpoints (may be
 * NULL), dR, dt, ds (per-object sums over the n points, fixed order). */
int tgp_pose_transform_fwd(const float *points, const float *R, const float *t, const float *s, int B, int n, float *out,
                           tgp_stream_t stream);
int tgp_pose_transform_bwd(const float *points, const float *R, const float *t, const float *s, const float *dout, int B, int n,
                           float *dpoints, float *dR, float *dt, float *ds, tgp_stream_t stream);

/* ---- backward GEMMs on the fp16 operand split: scale selection, scaled transposes, K-split partial sums ----------------- */

/* out = {s, 1/s, max|x|} on the device: s = 2^k, the largest power of two with max|x| * s <= target (s = 1 for an all-zero
 * tensor).  x (rows, cols) row stride ld; workspace: 2048 uint32. */
int tgp_absmax_scale(const float *x, int ld, int64_t rows, int cols, float target, uint32_t *workspace, float *out,
                     tgp_stream_t stream);
/* dst (cols, rows_pad) = (src (rows, cols) * *scale)^T as fp32 (scale may be NULL), columns rows.. zero; rows_pad % 4 == 0,
 * dst 16-byte aligned */
int tgp_transpose_scaled(const float *src, int ld_src, int rows, int cols, const float *scale, float *dst, int rows_pad,
                         tgp_stream_t stream);
/* the same, written as the fp16 hi / lo planes of tgp_split_f16: dst [cols][rows_pad / 16][2][16]; rows_pad % 16 == 0 */
int tgp_transpose_split_f16(const float *src, int ld_src, int rows, int cols, const float *scale, uint16_t *dst, int rows_pad,
                            tgp_stream_t stream);
/* out[i] (+)= *scale * sum_z parts[z * n + i], z ascending (scale may be NULL) */
/* (round 3) W (rows, cols) -> dst_f32 (cols, rows_pad) = W^T zero padded and dst_split = its fp16 hi / lo planes
 * [cols][rows_pad / 16][2][16], rows_pad % 16 == 0: the weight operands of the backward's dx GEMM in one pass */
int tgp_transpose_both(const float *src, int ld_src, int rows, int cols, float *dst_f32, uint16_t *dst_split, int rows_pad,
                       tgp_stream_t stream);
int tgp_sum_slabs(const float *parts, int Z, int64_t n, const float *scale, float *out, int accumulate, tgp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The regression terms of the training loss either side of Chamfer (losses/TDA_loss_sym_recon.py, losses/consistency_loss.py).
 * The reference loops over the batch in Python with one host synchronisation per object and term (`if sym[i, 0] == 1`);
 * these entries make the symmetry tests on the device, one launch per bundle, so the loss is capturable in a HIP graph.
 * sym: (B, sym_ld) int32, column 0 = symmetric about y, column 1.. = reflection flags (datasets' sym_info).
 * ------------------------------------------------------------------------------------------------------------------ */

/* TDA_loss.forward's eight small terms (:42-86 via cal_loss_Rot1 :223, cal_cosine_dis :243, cal_loss_Rot2 :227,
 * cal_cosine_dis_sym :247, cal_rot_regular_angle :265, cal_loss_Tran :285, cal_loss_Size :288, cal_loss_R_con :205), UNWEIGHTED:
 * out[0..7] = Rot1, Rot1_cos, Rot2, Rot2_cos, Rot_regular, Tran, Size, R_con; out[8] = number of objects with sym0 != 1.
 * rot1, rot2, tran, size and their targets are (B,3); f1, f2 (B) the predicted confidences.  kind 0 = nn.L1Loss,
 * 1 = nn.SmoothL1Loss(beta) (FLAGS.fsnet_loss_type, :20-35). */
int tgp_pose_terms_fwd(const float *rot1, const float *rot2, const float *f1, const float *f2, const float *tran, const float *size,
                       const float *g_rot1, const float *g_rot2, const float *g_tran, const float *g_size, const int32_t *sym,
                       int sym_ld, int B, int kind, float beta, float *out, tgp_stream_t stream);
/* gradient of sum_k gw[k] out[k] (gw: 8 floats on the device) w.r.t. the six predictions; fwd_out = the forward's out */
int tgp_pose_terms_bwd(const float *rot1, const float *rot2, const float *f1, const float *f2, const float *tran, const float *size,
                       const float *g_rot1, const float *g_rot2, const float *g_tran, const float *g_size, const int32_t *sym,
                       int sym_ld, int B, int kind, float beta, const float *fwd_out, const float *gw, float *d_rot1, float *d_rot2,
                       float *d_f1, float *d_f2, float *d_tran, float *d_size, tgp_stream_t stream);

/* prop_sym_matching_loss (losses/consistency_loss.py:19-48 = TDA_loss_sym_recon.py:120-148): L1 between the reconstruction
 * PC_re (B,N,3) and the cloud PC (B,N,3) mapped by the object's symmetry in the ground-truth frame (half turn about y /
 * mirror in z / identity, :171-203), mean over B*N*3 -> loss[0].  workspace: tgp_sym_recon_workspace_floats(B, N) floats.
 * The backward writes dPC and / or dPC_re (either may be NULL) for the upstream gradient gloss[0]. */
int64_t tgp_sym_recon_workspace_floats(int B, int N);
int tgp_sym_recon_fwd(const float *PC, const float *PC_re, const float *gt_R, const float *gt_t, const int32_t *sym, int sym_ld,
                      int sym_cols, int B, int N, float *workspace, float *loss, tgp_stream_t stream);
int tgp_sym_recon_bwd(const float *PC, const float *PC_re, const float *gt_R, const float *gt_t, const int32_t *sym, int sym_ld,
                      int sym_cols, int B, int N, const float *gloss, float *dPC, float *dPC_re, tgp_stream_t stream);

/* ph_loss_fn / omega (TDA_loss_sym_recon.py:292-322): out[0] = mean(|a - b| * w), a, b, wsrc (B,D), w = 1 on rows with
 * sum(wsrc) > 0.  The reference's host-side has_nan_or_inf branch (|a - a| instead) is folded in: NaN when a holds a
 * NaN / Inf, 0 when only b does; out[1] = 1 when the plain mean was taken.  rows: 4*B floats kept for the backward, which
 * writes da (B,D) for the upstream gradient gout[0]. */
int tgp_rowl1_fwd(const float *a, const float *b, const float *wsrc, int B, int D, float *rows, float *out, tgp_stream_t stream);
int tgp_rowl1_bwd(const float *a, const float *b, const float *rows, const float *fwd_out, const float *gout, int B, int D, float *da,
                  tgp_stream_t stream);

/* feat_consistency_loss (losses/consistency_loss.py:11-16, unweighted): loss[0] = 2 - 2 sum_b <x1_b/|x1_b|, x2_b/|x2_b|> / B,
 * x1, x2 (B,C), norms clamped at 1e-12 as F.normalize.  rows: 3*B floats kept for the backward (d1 / d2 may be NULL). */
int tgp_feat_consistency_fwd(const float *x1, const float *x2, int B, int C, float *rows, float *loss, tgp_stream_t stream);
int tgp_feat_consistency_bwd(const float *x1, const float *x2, const float *rows, const float *gloss, int B, int C, float *d1, float *d2,
                             tgp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Pairwise metrics of the NOCS pose evaluation (evaluation/eval_utils_v1.py): every (prediction, ground truth) pair of a
 * result set in one launch, double precision as the numpy original.  RT: (P,4,4) row-major, scales: (P,3).
 * ------------------------------------------------------------------------------------------------------------------ */

/* compute_3d_iou_new (:829-887): the reference's IoU of the two posed boxes -- its amax / amin run over axis 0 of the [3, 8]
 * corner array (:842-845), so the overlap is taken over eight per-corner (min, max) coordinate ranges; reproduced as written.
 * The fourth RT row is honoured (transform_coordinates_3d divides by it, :1011).  symmetric[t] != 0 (bottle / bowl / can,
 * mug with a hidden handle) -> the maximum over 20 rotations of box 1 about its own y axis. */
int tgp_iou3d_pairs(const double *RT1, const double *RT2, const double *scales1, const double *scales2, const int *symmetric,
                    int P, double *iou, tgp_stream_t stream);

/* compute_RT_degree_cm_symmetry (:890-963): out[t] = {rotation error in degrees, translation error in cm}.
 * mode[t]: 0 general, 1 symmetric about y (angle between the y axes), 2 symmetric under a half turn about y. */
int tgp_rt_error_pairs(const double *RT1, const double *RT2, const int *mode, int P, double *out, tgp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Input side of the evaluation loader (evaluation/load_data_eval.py): depth image + detection
 * mask + box -> the (n_pts, 3) camera-frame cloud PoseNet9D.forward is fed.  Byte / integer work, HBM-bound.
 * ------------------------------------------------------------------------------------------------------------------ */

/* One detection per workgroup, replacing load_data_eval.py:302-355 (ROI resampling of depth / mask / pixel grid by
 * crop_resize_by_warp_affine with cv2.INTER_NEAREST, tools/dataset_utils.py:80-136; _depth_to_pcl :451-462; /1000; the cut
 * of points within a quarter of the extent's diagonal of point number 25, :341-355).
 *   depth   (I,H,W) uint16 millimetres          masks   the images' (H,W,n_i) byte masks (Mask-RCNN 'pred_masks'), any packing
 *   mask_off[d]  byte offset of detection d's channel within masks; mask_stride[d] = n_i (bytes between neighbouring pixels,
 *                < 128; H*W < 2^24: offsets inside one image's masks are 31-bit)
 *   det_img[d]   image of detection d           window[d] = {cmin+cmax, rmin+rmax, s}: get_bbox's window (tools.eval_utils),
 *                                                s = min(max(rmax-rmin, cmax-cmin), max(H,W)) (:309-316)
 *   camk    (I,4) fx, fy, cx, cy (float32, as the reference's intrinsics :158-161); fx, fy ordinary focal lengths (normal
 *           floats far from overflow / underflow: the quotients are correctly rounded under that assumption)
 *   roi_size     FLAGS.img_size; a power of two in [64, 256] (the fixed-point walk is then exact and a pixel index fits 16 bits)
 *   recs    (D, roi_size^2) uint32 scratch: on return entries [0, counts[d][2]) are detection d's cloud in ROI row-major order
 *           as records (ROI pixel index << 16) | depth; a record and the detection's window / intrinsics determine its point,
 *           which tgp_cloud_select / tgp_cloud_sample materialise (only the sampled points are ever written as floats)
 *   counts  (D,3): depth-valid ROI pixels (:332), valid points (:336), points kept by the cut; the last is -1 when there are
 *           fewer than 26 valid points (the reference raises IndexError at :350). */
int tgp_roi_cloud(const uint16_t *depth, const uint8_t *masks, const int64_t *mask_off, const int *mask_stride, const int *det_img,
                  const int *window, const float *camk, int D, int H, int W, int roi_size, uint32_t *recs, int *counts,
                  tgp_stream_t stream);

/* The same kernel for the TRAINING loader's device half (datasets/load_data.py:235-290, 395-407):
 *   tables    (D, 2, roi_size) int32 or NULL.  The training window comes from aug_bbox_DZI (tools/dataset_utils.py:24-61): a
 *             real-valued centre and scale, for which OpenCV's 10-bit fixed-point walk has no integer closed form.  The host
 *             evaluates the walk once per detection in double (as cv2.warpAffine does): tables[d][0][x] = source column of ROI
 *             column x, tables[d][1][y] = source row of ROI row y (rot = 0, so the map is separable).  With tables, `window` is
 *             not read (may be NULL).
 *   mask_val  (D) int32 or NULL: v > 0 -> a pixel is inside when its mask byte EQUALS v (the ground-truth instance mask
 *             `mask == inst_id`, :245-247, with mask_stride 1 and mask_off = the image's offset); 0 / NULL -> any non-zero byte.
 *   cut_frac  the outlier cut keeps the points farther than cut_frac x the extent's diagonal from point number 25: 0.25 in the
 *             evaluation loader (load_data_eval.py:352), 0.15 in the training loader (load_data.py:283); float32 product.
 * tgp_roi_cloud = tgp_roi_cloud_ex(..., NULL, NULL, 0.25f). */
int tgp_roi_cloud_ex(const uint16_t *depth, const uint8_t *masks, const int64_t *mask_off, const int *mask_stride, const int *det_img,
                     const int *window, const float *camk, int D, int H, int W, int roi_size, uint32_t *recs, int *counts,
                     const int *tables, const int *mask_val, float cut_frac, tgp_stream_t stream);
/* The training loader's mask deformation defor_2D (datasets/data_augmentation.py:319-342, applied at load_data.py:280), in two
 * launches.  M = the warped mask as tgp_roi_cloud_ex tests it; a pixel is in the BAND when M differs from its up or left ROI
 * neighbour (OpenCV's 2x2 ellipse [[0,1],[1,1]], anchor (1,1), one erode / dilate iteration, neighbours outside the ROI ignored).
 *
 * tgp_roi_band: band_counts (D,3) int32 = depth-valid ROI pixels, valid points with the UNDEFORMED mask (the reference's validity
 * tests, :259-264), band size l.  Other arguments as tgp_roi_cloud_ex.
 *
 * tgp_roi_cloud_defor: tgp_roi_cloud_ex with, per detection, defor_on (D) int32 (0: records and counts bit-identical to
 * tgp_roi_cloud_ex) and drop_bits (D, drop_words) uint32, bit r of row d set = the band pixel of row-major band rank r is dropped.
 * An applied detection keeps a pixel when depth > 0 and (band ? !drop[rank] : M): band pixels not dropped become 1, including
 * those where M was 0.  counts[1] stays the undeformed count; point 25, the cut and counts[2] follow the deformed mask; below 26
 * deformed points counts[2] = -(1 + the deformed count) (tgp_roi_cloud_ex writes -1).
 * cut_frac = -1: no cut, counts[2] = the deformed count (never -1).  drop_words in [0, 2048]; ranks past 32 x drop_words are
 * kept. */
int tgp_roi_band(const uint16_t *depth, const uint8_t *masks, const int64_t *mask_off, const int *mask_stride, const int *det_img,
                 const int *window, int D, int H, int W, int roi_size, int *band_counts, const int *tables, const int *mask_val,
                 tgp_stream_t stream);
int tgp_roi_cloud_defor(const uint16_t *depth, const uint8_t *masks, const int64_t *mask_off, const int *mask_stride,
                        const int *det_img, const int *window, const float *camk, int D, int H, int W, int roi_size, uint32_t *recs,
                        int *counts, const int *tables, const int *mask_val, float cut_frac, const int *defor_on,
                        const uint32_t *drop_bits, int drop_words, tgp_stream_t stream);
/* tgp_cloud_select with the detections' source-pixel tables (NULL: the window's closed form). */
int tgp_cloud_select_ex(const uint32_t *recs, const int32_t *sel, const int *det_img, const int *window, const float *camk, int D,
                        int roi_size, int n_pts, float *out, const int *tables, tgp_stream_t stream);

/* _sample_points (:404-417) as a gather with a host-drawn selection: out[d][i] = point(recs[d][sel[d][i]]), out (D,n_pts,3);
 * det_img / window / camk as given to tgp_roi_cloud.  An index outside [0, roi_size^2) produces NaNs, never a fault.
 * With sel[d] = 0..n-1 it materialises a cloud's first n points. */
int tgp_cloud_select(const uint32_t *recs, const int32_t *sel, const int *det_img, const int *window, const float *camk, int D,
                     int roi_size, int n_pts, float *out, tgp_stream_t stream);

/* The same resampling drawn on the device (no read-back of counts): the first n_pts elements of a keyed pseudo-random
 * permutation of each cloud (4-round Feistel bijection, cycle-walked); clouds with at most n_pts points are tiled exactly
 * as :411-412.  Not the draw np.random would make -- a documented deviation for throughput runs.  Rows of detections
 * whose count is <= 0 are NaN. */
int tgp_cloud_sample(const uint32_t *recs, const int *counts, const int *det_img, const int *window, const float *camk, int D,
                     int roi_size, int n_pts, uint64_t seed, float *out, tgp_stream_t stream);

/* Row order of the factored wide layers (this repo's engine; no reference counterpart): per object, the n fine rows sorted by
 * key = near2 * n1 + near1 with ties in point order -- torch.argsort(key, stable=True) -- and the sorted parents as global
 * row numbers: order / order64 (B,n) the permutation (int32 for tgp_gather_rows, int64 for torch scatter), near1_out = sorted
 * near1 + b*n1, near2_out = sorted near2 + b*n2.  n <= 2048, n1*n2 <= 2^21; near1 in [0,n1), near2 in [0,n2). */
int tgp_sort_by_parent(const int32_t *near1, const int32_t *near2, int B, int n, int n1, int n2, int32_t *order, int64_t *order64,
                       int32_t *near1_out, int32_t *near2_out, tgp_stream_t stream);

/* The pose heads' conv1 -> BatchNorm(eval) -> ReLU -> conv2 -> BatchNorm(eval) -> ReLU -> max over each object's points as one
 * kernel (PoseR.py:26-36 Rot_green / Rot_red, PoseTs.py:31-42 Pose_Ts; eval mode), on the factored form of conv1 (this repo's
 * engine): conv1(feat)[m] = W_fine . fine[m] + p1[idx1[m]] + p2[idx2[m]].  The (M, heads * 1024) activation is never written.
 *   fine (M, ldf) fp32, K = its live columns (256 < K <= 272 = ldf's first 17 K-tiles);
 *   wa_planes (ABI 7) = the heads' conv1 weights over fine, (heads * 1024) rows x 272 columns, as BLOCKED fp16 planes
 *   (tgp_planes_split with kts = 17: the layout of tgp_gemm_args.W_planes; one 32-channel block is 34 contiguous KB);
 *   p1 / p2: rows of per-coarse-point products, columns head * 1024 + channel at the pointers given, row strides ldp1 / ldp2;
 *   idx1 / idx2 (M) rows of p1 / p2 per point;
 *   w2p (ABI 7) = tgp_heads_pack_w2(conv2 weights, conv1 bias and BatchNorm fold): tgp_heads_w2_bytes(heads) bytes;
 *   bias2 / scale2 / shift2 (heads * 256); keys (heads, B, 256) order-preserving keys of the maxima (tgp_colmax_decode), zeroed by
 *   the caller; M = B * rows_per_obj. */
typedef struct tgp_heads_fused_args {
    const float *fine; int ldf; int K;
    const void *wa_planes;
    const float *p1; int ldp1; const int32_t *idx1;
    const float *p2; int ldp2; const int32_t *idx2;
    const void *w2p;
    const float *bias2; const float *scale2; const float *shift2;
    uint32_t *keys;
    int M; int rows_per_obj; int B; int heads;
    /* fp16 range: a wave whose fine features or conv1 activations leave fp16's range (a magnitude that rounds to infinity, a NaN: its
     * conv2 sums are then non-finite), or whose fine features all lie under 2^-4, writes no keys for its 32 points and sets
     * *overflow = 1 (device int, zeroed by the caller; NULL: such waves write whatever keys their sums give -- NaN keys are loud).
     * The caller then runs the two-launch form predicated on the flag (tgp_gemm_args.pred), which recomputes every key in guarded
     * arithmetic. */
    int *overflow;
    /* (ABI 4) rows > 0: only the first `rows` rows (a multiple of 128) of every head are processed here; the caller supplies the
     * keys of rows [rows, M) through tgp_gemm_f32 (row_base = rows), merging into the same key buffer.  The grid is
     * heads x 128-point workgroups, one per CU and round. */
    int rows;
    /* (ABI 5) fine_planes (may be NULL): the same features as blocked fp16 planes (tgp_gemm_args.A_planes' layout, fine_kt >= 17
     * K-tiles per row block, columns K.. zero; fine_amax: the per-row-block magnitude words, may be NULL): the kernel then loads its
     * points' operand fragments as 1 KB runs instead of splitting fp32 rows -- same bits.  `fine` is still required (the repair). */
    const void *fine_planes; int fine_kt; const uint32_t *fine_amax;
} tgp_heads_fused_args;
int tgp_heads_fused(const tgp_heads_fused_args *args, tgp_stream_t stream);
/* conv -> BatchNorm(eval) -> LeakyReLU -> max over each object's points of a factored layer whose activation only feeds the max
 * (FaceRecon.py:76-77 conv_5 and the `feat.max(1)` that follows, on the factored form of this repo's engine): operands as for
 * tgp_heads_fused with one "head" of C channels (C % 32 == 0; wa_planes / bias / scale / shift / p1 / p2 point at its first channel),
 * slope = the LeakyReLU slope, 0 <= slope <= 1; keys (B, C) row stride ldk zeroed by the caller; p1_rows / p2_rows: rows of p1 / p2
 * (p1_rows * ldp1 and p2_rows * ldp2 below 2^30: rows are addressed with 32-bit byte offsets); overflow as in tgp_heads_fused (the
 * caller's repair is tgp_gemm_f32 with `pred`).  A NaN or an infinity among an object's activations gives that (object, channel) a
 * NaN's key. */
typedef struct tgp_conv_max_fused_args {
    const float *fine; int ldf; int K;
    const void *wa_planes;     /* (ABI 7) the layer's (C, K) weight as blocked fp16 planes with 17 K-tiles: tgp_planes_split, the layout of tgp_gemm_args.W_planes */
    const float *p1; int ldp1; int p1_rows; const int32_t *idx1;
    const float *p2; int ldp2; int p2_rows; const int32_t *idx2;
    const float *bias; const float *scale; const float *shift; float slope;
    uint32_t *keys; int ldk;
    int M; int rows_per_obj; int C;
    int *overflow;
    const void *fine_planes; int fine_kt; const uint32_t *fine_amax;      /* (ABI 5) as in tgp_heads_fused_args */
} tgp_conv_max_fused_args;
int tgp_conv_max_fused(const tgp_conv_max_fused_args *args, tgp_stream_t stream);
/* (ABI 7) w2 (heads, 256, 1024) fp32 and the heads' conv1 bias / BatchNorm scale / shift (heads * 1024 each) -> the kernel's operand:
 * per (head, block of 32 conv1 channels) 33 KB = conv2's fp16 hi / lo planes in MFMA fragment order (K permuted to the order the
 * conv1 accumulators leave the channels in) + the block's bias | scale | shift.  out: tgp_heads_w2_bytes(heads) bytes, 16-byte aligned.
 * w2 == NULL: only the vectors are rewritten, in place (the BatchNorm fold follows the running statistics; the weights do not). */
int64_t tgp_heads_w2_bytes(int heads);
int tgp_heads_pack_w2(const float *w2, const float *bias1, const float *scale1, const float *shift1, int heads, void *out,
                      tgp_stream_t stream);

/* (ABI 7) An HS layer's last GEMM and the NEXT layer's projection GEMM as one kernel (gcn3d.py:87-89 / 108-112 / 147-155 followed by
 * gcn3d.py:170), csrc/hs_chain.hip, for the two shapes of Face_Enc without a pooling in between: (K1 in 129..144, N1 = 128, N2 = 1152)
 * and (K1 in 241..256, N1 = 256, N2 = 2304); other shapes: -1 from tgp_hs_chain_pack_bytes, an argument error from the launches.
 *   c1 = act(bn(A W1^T + rowbias[object] + res1 + res2)) (M, N1), the tile kernel's epilogue order; c2 = c1 W2^T + bias2 (M, N2).
 *   a_planes / a_kt / a_amax: A (M, K1) as blocked fp16 planes + magnitude words (tgp_gemm_args.A_planes' layout; a_kt >= ceil(K1 / 16));
 *   units = tgp_hs_chain_pack(W1 (N1, K1), W2 (N2, N1)); rowbias (M / rows_per_obj, N1) or NULL; res1 / res2 (M, N1) or NULL; scale1 /
 *   shift1 (N1) both or neither; relu != 0: ReLU; c1 also as planes (c1_planes, c1_kt K-tiles per row block, first K-tile c1_kt0) with
 *   magnitude words c1_amax (all may be NULL);
 *   flag: device int, zeroed by the caller, raised when the operand or the intermediate leaves the fp16 split's range (>= 65504, NaN, or
 *   a 32-row block wholly below 2^-4): c1 / c2 are then not to be trusted and the caller's two tgp_gemm_f32 launches follow with
 *   tgp_gemm_args.pred = flag.  While the flag stays 0 both results equal those two launches' on the same planes bit for bit. */
typedef struct tgp_hs_chain_args {
    const void *a_planes; int a_kt; const uint32_t *a_amax;
    int M; int K1; int N1; int N2;
    const void *units;
    const float *rowbias; int ldrb; int rows_per_obj;
    const float *res1; int ldr1;
    const float *res2; int ldr2;
    const float *scale1; const float *shift1;
    int relu;
    float *c1; int ldc1;
    void *c1_planes; int c1_kt; int c1_kt0; uint32_t *c1_amax;
    const float *bias2;
    float *c2; int ldc2;
    int *flag;
} tgp_hs_chain_args;
int64_t tgp_hs_chain_pack_bytes(int K1, int N1, int N2);
int tgp_hs_chain_pack(const float *w1, int ld1, int K1, int N1, const float *w2, int ld2, int N2, void *out, tgp_stream_t stream);
int tgp_hs_chain(const tgp_hs_chain_args *args, tgp_stream_t stream);

/* (ABI 7) C = A W^T (+ bias; NULL: none) for the projection shapes of the HS layers (gcn3d.py:170: K = 128 or 256, N % 128 == 0, e.g.
 * N = 9 x width) and the coarse products of the factored wide layers (K = 512),
 * csrc/hs_chain.hip hs_proj_kernel: the operand from its planes (a_planes / a_kt / a_amax as tgp_gemm_args.A_planes), a workgroup keeps
 * its 128 rows' fragments for all columns and streams the weights (units = tgp_proj_pack(W (N, K))) once.  Same bits as tgp_gemm_f32 on
 * the same planes, except in a 128-row tile that the fp16 range rule (a magnitude >= 65504 / NaN, or nothing >= 2^-4) sends to the exact
 * path: computed here from a (M, K, row stride lda) and w (N, K, ldw) by fp32 fma chains in ascending k.  a / w may be NULL when a_amax is. */
typedef struct tgp_proj_planes_args {
    const void *a_planes; int a_kt; const uint32_t *a_amax;
    const float *a; int lda;
    int M; int K; int N;
    const void *units;
    const float *w; int ldw;
    const float *bias;
    float *c; int ldc;
} tgp_proj_planes_args;
int64_t tgp_proj_pack_bytes(int K, int N);
int tgp_proj_pack(const float *w, int ld, int K, int N, void *out, tgp_stream_t stream);
int tgp_proj_planes(const tgp_proj_planes_args *args, tgp_stream_t stream);

/* (ABI 7) The decoder behind its first conv as ONE kernel (FaceRecon.py:105-117 Face_Dec in eval mode: conv 512 -> 512, 512 -> 256,
 * 256 -> 128, each + BatchNorm + ReLU, then conv 128 -> 3), csrc/dec_fused.hip: a wave owns 32 points for the whole chain, no activation
 * between the layers leaves its registers.
 *   h1_planes: the first conv's activation (M, 512) as blocked fp16 planes (tgp_gemm_args.C_planes of that launch, h1_kt >= 32 K-tiles
 *   per row block); h1_amax: its per-32-row-block magnitude words (may be NULL);
 *   units = tgp_dec_pack(W2 (512, 512), W3 (256, 512), W4 (128, 256)) (tgp_dec_pack_bytes() bytes, 16-byte aligned): the three weights
 *   as fp16 hi / lo MFMA fragments in staging order, W3 / W4 with K permuted to the order the accumulators hold the channels in;
 *   vec[l][0 / 1 / 2]: bias / BatchNorm scale / shift of layer l + 2 (512, 256, 128 floats; read at every launch: they follow a refold);
 *   w5 (3, 128) and b5 (3): the last conv; map (may be NULL) as tgp_rows_out's: out row of row i = (i / rows_per_obj) * rows_per_obj + map[i];
 *   out (M, 3);
 *   flag: device int (zeroed by the caller; required): raised when the operand's magnitude words or any sum of the chain leave fp16's
 *   range (or the operand's block lies wholly under 2^-4): `out` is then not to be trusted and the caller's predicated fp32 chain
 *   (tgp_gemm_args.pred) redoes the layers.  Layer 2's sums equal tgp_gemm_f32's on the same planes bit for bit; layers 3, 4 and the
 *   last conv add the same products in another order (agreement to rounding). */
typedef struct tgp_dec_fused_args {
    const void *h1_planes; int h1_kt; const uint32_t *h1_amax;
    const void *units;
    const float *vec[3][3];
    const float *w5; const float *b5;
    const int64_t *map; int rows_per_obj;
    float *out;
    int *flag;
    int M;
} tgp_dec_fused_args;
int tgp_dec_fused(const tgp_dec_fused_args *args, tgp_stream_t stream);
int64_t tgp_dec_pack_bytes(void);
/* h1_permuted: the operand's planes hold the channels in accumulator order (tgp_dec_l1's output) instead of the natural one
 * (tgp_gemm_args.C_planes): W2's K order is then permuted like W3's / W4's. */
int tgp_dec_pack(const float *w2, const float *w3, const float *w4, int h1_permuted, void *out, tgp_stream_t stream);
/* (ABI 7) The decoder's FIRST conv (FaceRecon.py:112, factored form: W_fine . fine[m] + p1[idx1[m]] + p2[idx2[m]] + rowbias[object],
 * BatchNorm(eval) + ReLU; 512 channels) in the fused heads kernel's style, writing the activation as the operand tgp_dec_fused loads:
 *   fine_planes (M rows, fine_kt >= 17 K-tiles) / fine_amax: the points' features as blocked planes; wa_planes: the conv's weights over
 *   fine (512, 272) as blocked planes with 17 K-tiles; p1 / p2 / idx1 / idx2 as tgp_heads_fused (pointers at the conv's first channel);
 *   bias / scale / shift (512); rowbias (may be NULL): (objects, >= 512) per-object bias, row stride ldrb, objects of rows_per_obj rows;
 *   h1_planes (M rows x 512, h1_kt >= 32 K-tiles) receives fp16 hi / lo planes whose K order is the ACCUMULATOR order (slot 8 h + t of
 *   K-tile 2 b + s = channel 32 b + 16 s + 8 (t >> 2) + 4 h + (t & 3)): consumed by tgp_dec_fused with tgp_dec_pack(h1_permuted = 1), not by
 *   tgp_gemm_f32; h1_amax: per-32-row-block magnitude words (zeroed by the caller; may be NULL); flag as tgp_dec_fused's.  Values equal
 *   the tile kernel's for the same layer bit for bit. */
typedef struct tgp_dec_l1_args {
    const void *fine_planes; int fine_kt; const uint32_t *fine_amax;
    const void *wa_planes;
    const float *p1; int ldp1; const int32_t *idx1;
    const float *p2; int ldp2; const int32_t *idx2;
    const float *bias; const float *scale; const float *shift;
    const float *rowbias; int ldrb; int rows_per_obj;
    void *h1_planes; int h1_kt; uint32_t *h1_amax;
    int *flag;
    int M;
} tgp_dec_l1_args;
int tgp_dec_l1(const tgp_dec_l1_args *args, tgp_stream_t stream);

/* ---- the factored wide layers in TRAINING (ABI 4; this repo's engine, no reference counterpart: the reference multiplies the
 * up-sampled copies, FaceRecon.py:70-77) -----------------------------------------------------------------------------------------
 * The layers that read the concat buffer run as  W_fine x fine[i] + P1[near1(i)] + P2[near2(i)]  (tgp_gemm_args.gres1 / gres2); the
 * backward of the two fetches is  d P[r] = sum of d Y[i] over the points i whose nearest coarse point is r.
 * tgp_child_lists inverts near (B, n) (parent of every point: ids in [0, R), or b*R + that when global_ids) into CSR child lists: ptr (B*R + 1) int32,
 * idx (B*n) int32 global rows b*n + i, children in point order.  R <= 4096, n <= 8192.
 * tgp_segsum_rows: out[r][:C] = sum of g[idx[k]][:C] over k in [ptr[r], ptr[r+1]) in list order -- no atomics, bit-repeatable.
 * C, ldg, ldo multiples of 4 and g, out 16-byte aligned (16-byte accesses), or multiples of 2 and 8-byte aligned (8-byte accesses). */
int tgp_child_lists(const int32_t *near, int B, int n, int R, int global_ids, int32_t *ptr, int32_t *idx, tgp_stream_t stream);
int tgp_segsum_rows(const float *g, int ldg, int C, const int32_t *ptr, const int32_t *idx, int R, float *out, int ldo,
                    tgp_stream_t stream);

/* ---- scatter-free backward of the graph layers (ABI 4; csrc/graph_bwd.hip) ---------------------------------------------------------
 * Same gradients as tgp_nbrmax_bwd / tgp_gconv_hs_bwd (the reference's autograd: max backward + index_add, gcn3d.py:157-180,210-245)
 * without float atomics: the neighbour lists are inverted once (tgp_reverse_graph), pass 1 stores every (row, channel)'s winning slot,
 * pass 2 sums per SOURCE row over its reverse list.  Outputs are written densely (no zero fill by the caller) and are bit-repeatable.
 * tgp_reverse_graph: idx (B, n_rows, k) int32 ids in [0, n_src) -> rptr (B*n_src + 1) int32, rent (B*n_rows*k) int32 = (row << 6) | slot,
 * each list ascending.  k <= 64, n_src <= 8192, (n_rows*k + 2*n_src) * 4 <= 150 KB (one workgroup sorts an object in LDS), else
 * TGP_EUNSUPPORTED.
 * tgp_nbrmax_bwd_gather: arg_ws B*n_rows*C bytes; C % 4 == 0, C / 4 a divisor of 256, strides % 4 == 0, 16-byte aligned, else
 * TGP_EUNSUPPORTED.  tgp_gconv_hs_bwd_gather: workspace as tgp_gconv_bwd_workspace_floats; arg_ws B*n*7C bytes, contrib_ws B*n*7C
 * floats; C in {128, 256, 512}, k <= 63, 16-byte aligned operands, else TGP_EUNSUPPORTED; have_slots: arg_ws was filled by
 * tgp_gconv_hs_fwd_slots (below) and the slot pass is skipped. */
int tgp_reverse_graph(const int32_t *idx, int B, int n_rows, int k, int n_src, int32_t *rptr, int32_t *rent, tgp_stream_t stream);
int tgp_nbrmax_bwd_gather(const float *src, int ld_src, const int32_t *idx, const int32_t *rptr, const int32_t *rent, int B, int n_src,
                          int n_rows, int k, int C, const float *dy, int lddy, int per_object, float scale, uint8_t *arg_ws,
                          float *dsrc, int ld_dsrc, tgp_stream_t stream);
int tgp_gconv_hs_bwd_gather(const float *xyz, const int32_t *idx, const int32_t *rptr, const int32_t *rent, const float *proj, int ldp,
                            const float *sdn, const float *dg, int ldg, int B, int n, int k, int S, int C, float *dproj, int lddp,
                            float *dsdn, float *workspace, uint8_t *arg_ws, float *contrib_ws, int have_slots, tgp_stream_t stream);
/* tgp_gconv_hs_fwd (same output, bit for bit) that also records the slots (B*n*7C bytes) for tgp_gconv_hs_bwd_gather(have_slots = 1):
 * the training forward then needs no slot pass in the backward.  Same shape limits as tgp_gconv_hs_bwd_gather. */
int tgp_gconv_hs_fwd_slots(const float *xyz, const int32_t *idx, const float *proj, int ldp, const float *sdn, int B, int n, int k, int S,
                           int C, float *out, int ldo, uint8_t *slots, tgp_stream_t stream);

/* ---- the rotation R_DCD canonicalises with, and its gradient (ABI 4; csrc/poserot.hip) --------------------------------------------
 * losses/TDA_loss_sym_recon.py:327-333 (get_vertical_rot_vec_in_batch :370-395 for the symmetric and the general case,
 * get_rot_mat_y_first :351-360) in one launch.  gR0 (B, 3) = g_R[:, :, 0]; p_g, p_r (B, 3) predicted axes; f_g, f_r (B) their
 * confidences; sym0 (B) = sym[:, 0] as float.  R (B, 3, 3) row-major; J (B, 9, 8) = d R / d (p_g, f_g, p_r, f_r), evaluated by
 * forward-mode differentiation of the same formulas.  tgp_pose_rotation_bwd: din (B, 8) = J^T dR per object. */
int tgp_pose_rotation_fwd(const float *gR0, const float *p_g, const float *f_g, const float *p_r, const float *f_r, const float *sym0,
                          int B, float *R, float *J, tgp_stream_t stream);
int tgp_pose_rotation_bwd(const float *dR, const float *J, int B, float *din, tgp_stream_t stream);
/* backward of tgp_head_post (PoseNet9D.py:57-66): dgreen (B, 4), dred (B, 4), dts (B, 6) contiguous, from the gradients of the six
 * outputs (contiguous; NULL = zero). */
int tgp_head_post_bwd(const float *green, const float *red, int ldg, int ldr, int B, const float *g_pg, const float *g_pr,
                      const float *g_fg, const float *g_fr, const float *g_T, const float *g_s, float *dgreen, float *dred, float *dts,
                      tgp_stream_t stream);

/* ---- dW = dy^T x on the fp16 split without transposed copies (ABI 4; csrc/gemm_tn_split.hip) --------------------------------------
 * a = dy (rows, N), b = x (rows, K), both row-major; scale = tgp_absmax_scale(a) ({s, 1/s, ...} on the device).  The reduction over
 * the rows is cut into Z chunks of `chunk` rows (Z * chunk >= rows); parts (Z, N, K) receives their partial products, which
 * tgp_sum_slabs adds in order and unscales.  N, K, lda, ldb multiples of 4 and 16-byte aligned operands, else TGP_EUNSUPPORTED
 * (the caller then takes the transposed-copy form: tgp_transpose_scaled + tgp_transpose_split_f16 + tgp_gemm_f32). */
int tgp_gemm_tn_split(const float *a, int lda, const float *b, int ldb, int rows, int N, int K, const float *scale, int Z, int chunk,
                      float *parts, tgp_stream_t stream);

/* ---- the optimizer step (ABI 8; csrc/ranger.hip) ----------------------------------------------------------------------------------
 * tools/torch_utils/solver/ranger2020.py:43-246 Ranger.step (RAdam + Lookahead + gradient centralisation) over many tensors in ONE
 * launch.  One descriptor per tensor that has a gradient; every pointer is a device pointer to numel fp32 elements (any 4-byte
 * alignment: 16-byte accesses where an array is 16-byte aligned at the same element as exp_avg, 4-byte ones otherwise).  Per element,
 * in the reference's order and rounding (fmaf exactly where the reference's torch op rounds once):
 *   flags & TGP_RANGER_GC:  g -= mean of its row (row_len elements: numel / size(0)); written back to g (the reference centralises
 *                           p.grad in place).  Otherwise g is only read.
 *   v = v b2 + (omb2 g) g;   m = fmaf(omb1, g, m b1)
 *   ADAPTIVE:  G = m / (sqrt(v) + eps), then G = fmaf(p, weight_decay, G) when weight_decay != 0
 *   otherwise: G IS m: m = fmaf(p, weight_decay, m) when weight_decay != 0 (the change persists in exp_avg, as in the reference)
 *   p = fmaf(G, neg_step_lr, p)                (neg_step_lr = float(-step_size * lr), computed by the caller in doubles)
 *   LOOKAHEAD: slow = fmaf(p - slow, alpha, slow); p = slow
 * The adaptive and lookahead decisions and step_size are the caller's (host doubles: N_sma crosses its threshold between steps 5 and
 * 6, where a device pow could round the other way); they are per tensor, since step counters differ between tensors whose grads
 * were None on some steps.  A row's mean is summed in an order fixed by numel, row_len and the 16-byte phase of m (never by the
 * other tensors of the launch): no atomics, bit-repeatable.
 * tgp_ranger_plan (host only, nothing launched): checks a HOST copy of the table (non-null pointers, numel >= 0, row_len >= 1 and
 * numel % row_len == 0 where GC is set) and fills every entry's unit0 (the tensor's first work unit); *units = the total.  The caller
 * then copies that table to the device; tgp_ranger_step launches over it (grid from the device's CU count). */
#define TGP_RANGER_GC 1
#define TGP_RANGER_ADAPTIVE 2
#define TGP_RANGER_LOOKAHEAD 4
typedef struct tgp_ranger_tensor {
    float *p; float *g; float *m; float *v; float *slow;   /* param, grad, exp_avg, exp_avg_sq, slow_buffer */
    int64_t numel;
    int row_len;        /* GC row length (read when flags & TGP_RANGER_GC) */
    int flags;          /* TGP_RANGER_GC | TGP_RANGER_ADAPTIVE | TGP_RANGER_LOOKAHEAD */
    int64_t unit0;      /* filled by tgp_ranger_plan */
    float beta1, one_minus_beta1, beta2, one_minus_beta2;
    float eps, weight_decay, neg_step_lr, alpha;
} tgp_ranger_tensor;    /* 96 bytes */
typedef struct tgp_ranger_args {
    const tgp_ranger_tensor *tensors;   /* device table of n descriptors, unit0 as tgp_ranger_plan filled it */
    int n;
    int64_t units;                      /* tgp_ranger_plan's total */
} tgp_ranger_args;
int tgp_ranger_plan(tgp_ranger_tensor *host_tensors, int n, int64_t *units);
int tgp_ranger_step(const tgp_ranger_args *args, tgp_stream_t stream);

/* ---- the training item's point-cloud augmentation (csrc/augment.hip; new symbols, ABI 8 unchanged) -------------------------------
 * datasets/data_augmentation.py PC_BasicAugment (:19-63) and the second view of load_data.py:345-350 (one of PcJitter, PcRandomCutout,
 * PcRandomCrop, PcRandomDropout), one workgroup per item.  The kernel draws nothing: every random number is an input, drawn by the
 * host in the reference's order (datasets/data_augmentation.py of this package).
 * Base augmentation (draws != NULL): pc (B, N, 3) -> pc_out (B, N, 3), R_out (B, 3, 3), t_out (B, 3), s_out (B, 3) (fsnet_scale
 * residual), flags_out (B, 4) int32 {bb, rt, bc, pc} or NULL.  draws (B, 6) = prob_bb, prob_rt, prob_bc, ey_up, ey_down, prob_pc
 * (torch.rand values); a stage is on when its prob < pro_*, bc also needs cat_id 1 (bowl) or 5 (mug).  defor (B, N, 3) = the
 * torch.rand rows of the points (read only where the pc stage is on); model_point (B, n_model, 3) for bc's extents.  sym (B, 4) =
 * sym_info.  pc_out may be pc.  Rounding as the reference's fp32 torch ops, the 3 x 3 products as (a0 b0 + a1 b1) + a2 b2.
 * Second view (op != NULL; N <= tgp_augment_max_points()): on the base-augmented cloud (or pc when draws is NULL) ->
 * view_out (B, N, 3): rows [0, M) the operator's cloud, rows [M, N) zero; count_out (B, 2) int32 = {M, accepted attempt or -1}.
 * op (B) int32 TGP_AUG_* (TGP_AUG_NONE: the operator's p skipped it, the cloud is copied; other values act as TGP_AUG_NONE).
 *   JITTER:  noise (B, N, 3) added (the clamped normal_ draw).
 *   DROPOUT: a row whose drop_u (B, N) float64 is <= drop_ratio (B) float64 takes row 0.
 *   CROP / CUTOUT: boxes (B, TGP_AUGMENT_MAX_TRY, 6) float64 = per attempt the unit-cube bounds {umin[3], umax[3]}; attempt t maps
 *   them to coord_min + coord_diff * u in float64 (coord_* the cloud's fp32 min / max); a point is inside when strictly inside on
 *   all three axes.  The first of attempts 0 .. *_max_try - 1 that is valid is taken (crop: crop_min_points <= inside < N, kept =
 *   inside; cutout: N - inside >= cutout_min_points and inside > 0, kept = outside), points in their order; none valid: the cloud.
 * pc_out / view_out rows are ld_out floats apart: 4 gives the padded rows tgp_gather_rows takes (C a multiple of 4).
 * noise / drop_ratio / drop_u / boxes are read only for the items whose op needs them, but must be non-NULL.  view_out != pc. */
#define TGP_AUGMENT_MAX_POINTS 2048
#define TGP_AUGMENT_MAX_TRY 16
#define TGP_AUG_NONE (-1)
#define TGP_AUG_JITTER 0
#define TGP_AUG_CUTOUT 1
#define TGP_AUG_CROP 2
#define TGP_AUG_DROPOUT 3
typedef struct tgp_augment_args {
    int B, N;
    const float *pc;                       /* (B, N, 3) */
    /* base augmentation */
    const float *draws;                    /* (B, 6); NULL: no base augmentation */
    const float *R, *t, *s, *mean_shape;   /* (B, 3, 3), (B, 3), (B, 3), (B, 3) */
    const float *sym, *aug_bb, *aug_rt_t, *aug_rt_R;   /* (B, 4), (B, 3), (B, 3), (B, 3, 3) */
    const float *cat_id, *nocs_scale;      /* (B), (B) */
    const float *model_point;              /* (B, n_model, 3) */
    int n_model;
    const float *defor;                    /* (B, N, 3) */
    float pro_bb, pro_rt, pro_bc, pro_pc, pc_r;
    float *pc_out, *R_out, *t_out, *s_out;
    int32_t *flags_out;
    /* second view */
    const int32_t *op;                     /* (B); NULL: no second view */
    const float *noise;                    /* (B, N, 3) */
    const double *drop_ratio;              /* (B) */
    const double *drop_u;                  /* (B, N) */
    const double *boxes;                   /* (B, TGP_AUGMENT_MAX_TRY, 6) */
    int crop_max_try, cutout_max_try;      /* the operators' max_try_num (< TGP_AUGMENT_MAX_TRY) */
    int crop_min_points, cutout_min_points;
    float *view_out;                       /* (B, N, 3) */
    int32_t *count_out;                    /* (B, 2) */
    int ld_out;                            /* row stride of pc_out and view_out: 3 (or 0) packed, 4 padded (4th column 0) */
} tgp_augment_args;
int tgp_augment_max_points(void);
int tgp_augment(const tgp_augment_args *args, tgp_stream_t stream);

/* ---- ground-truth persistence images of the training clouds (csrc/persistence.hip; new symbols, ABI 8 unchanged) -----------
 * datasets/compute_pd.py of the reference: per cloud pcl (B, N, 3) float32, N <= TGP_PD_MAX_POINTS, the alpha complex of the
 * unique points (Delaunay triangulation, squared-radius values), its H1 / H2 persistence pairs with death > birth, and the legacy
 * persim PersImage(spread=1e-2, pixels=[50, 50]) of each dimension, normalised to a maximum of 1.
 * Outputs per cloud: h1 / h2 (B, TGP_PD_MAX_PAIRS, 2) float64 (birth, death) rows [0, counts), counts (B, 2) int32 {H1, H2},
 * status (B) int32 (0 or TGP_PD_E*; a failed cloud has counts 0 and zero images), tets (B, TGP_PD_MAX_TETS, 4) int32 the finite
 * tetrahedra as indices into the cloud's rows (first occurrence of a duplicated point) and ntet (B), or NULL; pdh1 / pdh2
 * (B, 2500) float32 or both NULL (pairs only).  workspace: B * tgp_pd_workspace_bytes() bytes, 256-byte aligned.
 * tet_cap: 0 for TGP_PD_MAX_TETS, a smaller value caps the triangulation (the overflow path, for tests).
 * Two launches, no host synchronisation; a capacity overflow sets the cloud's status, it never writes out of bounds. */
#define TGP_PD_MAX_POINTS 1024
#define TGP_PD_MAX_TETS 8192
#define TGP_PD_MAX_PAIRS 4096
#define TGP_PD_PIXELS 2500
#define TGP_PD_ETETS 1        /* tetrahedron / simplex storage */
#define TGP_PD_ECAVITY 2      /* one insertion's cavity */
#define TGP_PD_EWALK 3        /* point location did not end */
#define TGP_PD_EPAIRS 4       /* more than TGP_PD_MAX_PAIRS pairs in one dimension */
#define TGP_PD_ECOLUMNS 5     /* H1 column storage */
#define TGP_PD_ERANGE 6       /* a coordinate is not finite, or too small against the cloud's extent for the exact grid */
#define TGP_PD_EFLAT 7        /* fewer than 4 affinely independent points */
#define TGP_PD_EINTERNAL 8    /* an inconsistency that a valid triangulation cannot produce */
typedef struct tgp_pd_args {
    int B, N;
    const float *pcl;          /* (B, N, 3) */
    void *workspace;
    double *h1, *h2;           /* (B, TGP_PD_MAX_PAIRS, 2) */
    int32_t *counts;           /* (B, 2) */
    int32_t *status;           /* (B) */
    int32_t *tets;             /* (B, TGP_PD_MAX_TETS, 4) or NULL */
    int32_t *ntet;             /* (B); read when tets != NULL */
    float *pdh1, *pdh2;        /* (B, TGP_PD_PIXELS) or NULL */
    int tet_cap;
} tgp_pd_args;
int64_t tgp_pd_workspace_bytes(void);
int tgp_pd_max_points(void);
int tgp_persistence(const tgp_pd_args *args, tgp_stream_t stream);

/* ---- gradients with respect to the point coordinates (csrc/xyz_bwd.hip): no float atomics, bit-repeatable ----
 * tgp_gconv_dirgrad: d(unit neighbour direction) ddir (B, n, k, 3) of HSlayer_surface.graph_conv (proj == NULL) or HS_layer.graph_conv
 * (proj (B, n, 8C) rows = [centre | support], slots = tgp_gconv_hs_fwd_slots' record or NULL: recomputed) from d g (B, n, C) rows:
 * for every (support s, channel c) whose first maximum over the neighbours j has theta > 0, d g[c] / 7 (x the winner's support value)
 * * sdn[:, s*C + c] lands on that j.  S == 7, k <= 64, 7 * C * 5 bytes of LDS <= 60 KB: TGP_EUNSUPPORTED otherwise. */
int tgp_gconv_dirgrad(const float *xyz, const int32_t *idx, const float *proj, int ldp, const float *sdn, const float *dg, int ldg,
                      const uint8_t *slots, int B, int n, int k, int S, int C, float *ddir, tgp_stream_t stream);
/* tgp_neighbor_dirs: get_neighbor_direction_norm's forward: unit (B, n, k, 3) = F.normalize(x[idx] - x), unnormed (same, or NULL) the
 * difference itself; idx (B, n, k) ids in [0, n). */
int tgp_neighbor_dirs(const float *xyz, const int32_t *idx, int B, int n, int k, float *unit, float *unnormed, tgp_stream_t stream);
/* tgp_dirs_to_xyz: backward of get_neighbor_direction_norm (gcn3d.py:48-58): ddir (B, n, k, 3) = d F.normalize(x[idx] - x), dun (same
 * shape, or NULL) = d of the unnormalised difference -> dxyz (B, n, 3) (accumulate != 0: added to its contents).  Reverse lists of idx:
 * rev_global == 0: tgp_reverse_graph's (rptr (B*n + 1), rent = (i << 6) | j); rev_global == 1: tgp_child_lists' over idx viewed as
 * (B, n*k) with R = n (rent = global entry (b*n + i) * k + j). */
int tgp_dirs_to_xyz(const float *xyz, const int32_t *idx, const int32_t *rptr, const int32_t *rent, int rev_global, const float *ddir,
                    const float *dun, int B, int n, int k, float *dxyz, int accumulate, tgp_stream_t stream);
/* tgp_center_bwd: backward of tgp_center: dpoints (B, n, 3) = dxyz + (dmean - sum_i dxyz_i) / n; dmean (B, 3) or NULL. */
int tgp_center_bwd(const float *dxyz, const float *dmean, int B, int n, float *dpoints, tgp_stream_t stream);
/* tgp_bn_eval_bwd: backward of y = act((x - mean) / sqrt(var + eps) * gamma + beta) with FIXED mean / var (eval-mode BatchNorm on the
 * running statistics; the forward is tgp_bn_apply): dx, dgamma, dbeta (C).  workspace: tgp_bn_eval_workspace_floats(C) floats. */
int64_t tgp_bn_eval_workspace_floats(int C);
int tgp_bn_eval_bwd(const float *dy, int lddy, const float *x, int ld, int64_t rows, int C, const float *mean, const float *var, float eps,
                    const float *gamma, const float *beta, int act, float slope, float *dx, int lddx, float *dgamma, float *dbeta,
                    float *workspace, tgp_stream_t stream);
/* tgp_bn_eval_bwd_pooled: the same for max over each object's points (tgp_colmax_arg with the running statistics): dpool (objects, C),
 * argrow (objects, C) global winning rows -> dense dx (objects*rows_per_obj, C), dgamma, dbeta.  workspace: objects * C floats. */
int tgp_bn_eval_bwd_pooled(const float *dpool, int ldp, const int32_t *argrow, int lda, const float *x, int ld, int objects, int rows_per_obj,
                           int C, const float *mean, const float *var, float eps, const float *gamma, const float *beta, int act, float slope,
                           float *dx, int lddx, float *dgamma, float *dbeta, float *workspace, tgp_stream_t stream);

/* ---- the training batch's random draws on the device (csrc/draws.hip; new symbols, ABI 8 unchanged) ----------------------------
 * datasets/load_data.py train_batch(draws='device').  Every draw is a pure function of (seed, key, site, counter): the four words
 * of Philox-4x32-10 with Philox key (seed low, seed high) and Philox counter (counter, site, key low, key high); `keys` (D) are
 * the items' 64-bit keys.  Transforms: float32 uniform (w >> 8) * 2^-24; float64 uniform ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53;
 * normals by Box-Muller on 24-bit uniforms.  Permutations: one Philox word (site, counter 0, word 0) keys the four-round
 * Feistel bijection tgp_cloud_sample walks; element i of the permutation of [0, total) is that bijection cycle-walked from i.
 * Sites: */
#define TGP_SITE_HOST 0      /* the per-item scalars, drawn on the host from the same words (datasets/device_draws.py) */
#define TGP_SITE_BAND 1      /* defor_2D's choice over the band */
#define TGP_SITE_SEL2K 2     /* _sample_points(PC, 2048) */
#define TGP_SITE_SEL1K 3     /* _sample_points(PC, 1024) */
#define TGP_SITE_DEFOR 4     /* defor_3D_pc's uniforms; counter = the selected point's slot */
#define TGP_SITE_NOISE 5     /* PcJitter's normals; counter = point */
#define TGP_SITE_DROP 6      /* PcRandomDropout's uniforms; counter = point */
#define TGP_SITE_SHUFFLE 7   /* pc_sampler's shuffle */
#define TGP_DRAW_MAX_ITEMS 4096
#define TGP_DRAW_MAX_TOTAL 65536
/* an item's status (tgp_draw_alive): the reference's reasons to abandon it (load_data.py:262-265, 288), the deformed cloud below
 * 26 points (the host path raises there), a window the host refused (source_tables) */
#define TGP_ITEM_ALIVE 0
#define TGP_ITEM_NO_DEPTH 1     /* n_depth <= 1 */
#define TGP_ITEM_NO_MASK 2      /* n_valid <= 1 */
#define TGP_ITEM_FEW_POINTS 3   /* fewer than min_points after the cut */
#define TGP_ITEM_BELOW_26 4     /* counts[2] < 0 */
#define TGP_ITEM_WINDOW 5       /* forced by the host */
/* out (D, n_counters, 4) uint32: the words of counters 0 .. n_counters - 1 at `site` (tests; the recorder of the host's golden words) */
int tgp_draw_words(const uint64_t *keys, int D, uint64_t seed, uint32_t site, int n_counters, uint32_t *out, tgp_stream_t stream);
/* defor_2D's draws (data_augmentation.py:327-336) from tgp_roi_band's band_counts (D, 3), read on the device: defor_on[d] = (validity
 * == 0 or n_depth > 1 and n_valid > 1) and not u[d] > pro and l >= 1 (u (D) float64: defor_2D's rand(), a per-item scalar); drop_bits
 * (D, drop_words) every word written: bit r set iff r < l and rank r's position in the item's permutation of [0, l) is below l / 2
 * -- exactly l / 2 bits, a uniformly chosen subset as choice(l, l // 2, replace=False).  drop_words a multiple of 8 in [8, 2048];
 * l is taken as min(l, 32 drop_words). */
int tgp_draw_band_subset(const int *band_counts, const double *u, double pro, const uint64_t *keys, uint64_t seed, int D, int validity,
                         int *defor_on, uint32_t *drop_bits, int drop_words, tgp_stream_t stream);
/* _item_total's rules (load_data.py of this package) on tgp_roi_cloud_ex / _defor's counts (D, 3): status (D) TGP_ITEM_* (forced (D)
 * or NULL: a non-zero entry is the item's status whatever its counts), slot_item (B) the first B alive items in item order, the
 * alive ones repeated cyclically when fewer than B are alive, -1 when none is; n_alive (1) = min(alive, B).  B <= D <=
 * TGP_DRAW_MAX_ITEMS.  One workgroup. */
int tgp_draw_alive(const int *counts, const int *forced, int D, int B, int min_points, int *status, int *slot_item, int *n_alive,
                   tgp_stream_t stream);
/* sel (D, n_out) int32 selections of [0, total_d), total_d = totals[d * ld_total] read on the device (totals NULL: total_const), taken
 * as min(total_d, TGP_DRAW_MAX_TOTAL); total_d <= 0: zeros.  shuffle_always == 0, _sample_points (load_data.py:366-380): i % total
 * when total < n_out, i when equal, else the first n_out elements of the item's permutation.  shuffle_always != 0, pc_sampler
 * (data_augmentation.py:12-16): element i % total of the permutation whatever total is (total < n_out: the shuffled rows, repeated). */
int tgp_draw_selection(const int *totals, int ld_total, int total_const, const uint64_t *keys, uint64_t seed, uint32_t site, int D,
                       int n_out, int shuffle_always, int32_t *sel, tgp_stream_t stream);
/* the per-point draws of D items of N points, each buffer optional: defor (D, N, 3) float32 uniforms in [0, 1); noise (D, N, 3) float32
 * normals of deviation std clamped to [-clip, clip]; drop_u (D, N) float64 uniforms in [0, 1) */
int tgp_draw_fill(const uint64_t *keys, uint64_t seed, int D, int N, float *defor, float *noise, float std, float clip, double *drop_u,
                  tgp_stream_t stream);
/* rows by slot, n tensors in one launch: dst[k] (B, row_words[k]) = src[k] (D, row_words[k]) rows slot_item[s] (32-bit words); a slot
 * whose item is -1 gets zeros */
#define TGP_GATHER_SLOTS_MAX 24
typedef struct tgp_gather_slots_args {
    const int32_t *slot_item;              /* (B) */
    int B, D, n;
    const void *src[TGP_GATHER_SLOTS_MAX];
    void *dst[TGP_GATHER_SLOTS_MAX];
    int row_words[TGP_GATHER_SLOTS_MAX];
} tgp_gather_slots_args;
int tgp_gather_slots(const tgp_gather_slots_args *args, tgp_stream_t stream);

/* ---- mesh surface sampling (csrc/meshsample.hip; additive, ABI stays 8) ---------------------------------------------------------
 * uniform_sample (network/point_sample/pc_sample_sphere.py:154-169) for a batch of jobs on a mesh set (verts, faces, vptr, fptr as
 * tgp_render_depth reads them).  DESIGN.md section 3 "Mesh surface sampling" is the contract; tests/mesh_sample_ref.py restates it in
 * NumPy and the two agree bit for bit.  All arithmetic is float64 on the float32 vertices, every product and sum rounded on its own.
 *
 * Area table: with a = v1 - v0, b = v2 - v0 of face f, cross = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x),
 * norm = sqrt((c_x c_x + c_y c_y) + c_z c_z), area = 0.5 norm.  cdf[fptr[m] + f] is the mesh's cumulative area in this FIXED order:
 * the faces are cut into chunks of TGP_MESH_AREA_CHUNK consecutive faces; local[f] is the serial sum of the areas from the chunk's
 * first face to f; T[c] is local at the chunk's last face; O[0] = 0, O[c] = O[c - 1] + T[c - 1] (serial); cdf[f] = O[c] + local[f].
 * The order depends on neither the launch shape nor the other meshes of the set.  A mesh whose vptr / fptr rows leave the arrays or
 * are empty is not written. */
#define TGP_MESH_AREA_CHUNK 64
#define TGP_MESH_SITE 8      /* the draw site of the device uniforms (after TGP_SITE_SHUFFLE) */
int tgp_mesh_area_cdf(const float *verts, const int32_t *faces, const int32_t *vptr, const int32_t *fptr, int M, int n_verts,
                      int n_faces, double *cdf, tgp_stream_t stream);
/* B jobs of n samples each in ONE launch.  Job b samples mesh job_mesh[b]; sample i takes three uniforms (u, r1, r2) in [0, 1):
 * from u (B,n,3) float64 when given (the reference's np.random.random(), then np.random.random(2)), else from the Philox words of
 * (seed, keys[b], TGP_MESH_SITE): counter 2i gives u = uniform_f64(w0, w1) and r1 = uniform_f64(w2, w3), counter 2i + 1 gives
 * r2 = uniform_f64(w0, w1).  Exactly one of u and keys is non-NULL.
 * With total = cdf at the mesh's last face: face = the first f with cdf[f] >= u total (binary search; np.searchsorted side='left'),
 * clamped to F - 1; s = sqrt(r1); point = ((1 - s) v0 + (s (1 - r2)) v1) + (s r2) v2 per component; normal = cross / norm (NaN for
 * a zero-area face).  sqrt and / are correctly rounded.
 * -> out (B,n,3) or with normals (B,n,6) [point, normal], float64, or with f32 != 0 float32 (the float64 value rounded once);
 * face (B,n) int32 or NULL; status (B) int32: 0, 1 when total is not a positive finite number (rows are still written), 2 when
 * job_mesh[b] is outside [0, M) or the mesh's rows leave the arrays (rows are zeros, face -1).  A vertex index outside its mesh is
 * clamped into it.  TGP_EINVAL: a NULL required pointer, M, n_verts, n_faces, B or n < 1, both or neither of u / keys.
 * TGP_EUNSUPPORTED: B > 65535.  Nothing is launched on an error. */
typedef struct tgp_mesh_sample_args {
    const float *verts;
    const int32_t *faces;
    const int32_t *vptr, *fptr;
    const double *cdf;          /* tgp_mesh_area_cdf's table (n_faces) */
    int M, n_verts, n_faces;
    const int32_t *job_mesh;    /* (B) */
    int B, n;
    const double *u;            /* (B,n,3) or NULL */
    const uint64_t *keys;       /* (B) or NULL */
    uint64_t seed;
    int normals, f32;
    void *out;
    int32_t *face;              /* may be NULL */
    int32_t *status;
} tgp_mesh_sample_args;
int tgp_mesh_sample(const tgp_mesh_sample_args *args, tgp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Ball crop (network/point_sample/pc_sample_sphere.py:258-280, 350-371: crop_ball_from_pts / crop_ball_from_depth_image): the
 * pixels of a depth frame whose point lies within a ball round a pose's centre, for J jobs in one launch.  Additive: the ABI
 * number stays.  DESIGN.md section 3 "Ball crop and tracking" is the contract; tests/ball_ref.py restates it in NumPy and the
 * kernel agrees with it bit for bit.
 *
 * Job j crops frame job_img[j] round centers[j] (3 float32, metres) with the radius ladder ladder[j] (TGP_BALL_LEVELS float32,
 * ascending: the reference's radius and its products by 1.10).  centers and ladder are DEVICE pointers.
 *   depth (I,H,W) uint16 millimetres; camk (I,4) fx, fy, cx, cy as tgp_roi_cloud takes it; H, W < 32768, H*W < 2^24.
 *   masks NULL: no mask.  Else mask_off (J) int64 / mask_stride (J) / mask_val (J, or NULL) address job j's mask exactly as
 *   tgp_roi_cloud_ex addresses a detection's: byte masks[mask_off[j] + pixel * mask_stride[j]], admitted when non-zero
 *   (mask_val NULL or 0) or when equal to mask_val[j] (> 0).
 * A pixel is VALID when depth > 0 and the mask admits it.  Its point is the one tgp_cloud_select gives for that source pixel and
 * depth (same bits).  d = sqrt((dx^2 + dy^2) + dz^2) against the centre, float32, each operation rounded on its own, the root
 * correctly rounded.  The point's level is the smallest i with d <= ladder[i]; L is the first level whose cumulative count of
 * valid pixels reaches 10, or TGP_BALL_LEVELS - 1 when none does; the crop is the valid pixels of level <= L in row-major order.
 *   recs   (J, cap) uint32: the crop's pixel indices y*W + x, the first min(count, cap) entries written
 *   counts (J, 4) int32: valid pixels of the frame under the mask; the crop's count (the true one, also above cap); L; status --
 *          0 ok, 1 nothing within ladder[last] (the reference then takes every valid point: call again with a ladder of 1e9),
 *          2 no valid pixel (the reference recurses without end), 3 job_img[j] outside [0, I) (nothing is read)
 * full_scan = 0: distances are evaluated only inside the pixel rectangle that can hold points within ladder[last] of the centre
 * (whole frame when the ball reaches z <= 0 or an argument is not finite); full_scan != 0: everywhere.  Same result either way.
 * One workgroup of TGP_BALL_THREADS threads per job; a job's result does not depend on the other jobs; no float atomics.
 * TGP_EINVAL (before any launch): a NULL required pointer, masks without mask_off / mask_stride, a size out of range, cap < 1.
 *
 * tgp_ball_cloud_pts: the same crop of point lists pts (I, N, 3) float32 (crop_ball_from_pts): every point is valid, a record is
 * the point's index, N <= 2^30 - 1024. */
#define TGP_BALL_LEVELS 10
#define TGP_BALL_THREADS 1024
int tgp_ball_cloud(const uint16_t *depth, const uint8_t *masks, const int64_t *mask_off, const int *mask_stride, const int *mask_val,
                   const int *job_img, const float *centers, const float *ladder, const float *camk, int J, int I, int H, int W, int cap,
                   int full_scan, uint32_t *recs, int *counts, tgp_stream_t stream);
int tgp_ball_cloud_pts(const float *pts, const int *job_img, const float *centers, const float *ladder, int J, int I, int N, int cap,
                       uint32_t *recs, int *counts, tgp_stream_t stream);
/* The reference's selection from the crop.  With n = min(counts[j][1], cap), the reference doubles its index list until it holds
 * n_pts entries: length n * 2^m, the first such >= n_pts, element e being entry e mod n.  tgp_ball_select: out[j][i] =
 * point(recs[j][sel[j][i] mod n]) and pix[j][i] = that pixel index (to gather image / coord rows); sel (J, n_pts) int32 indexes
 * the doubled list, an index outside it (or n = 0, or a record that names no pixel) gives NaNs and pix -1, never a fault.
 * tgp_ball_sample: the same with sel[j][i] = element i of the keyed permutation of the doubled list's length that
 * tgp_cloud_sample walks (no read-back); rows of jobs whose status is not 0 are NaN / -1.
 * Exactly one of depth (with camk; frames (I,H,W)) and pts (lists (I,W,3), H = 1) is non-NULL.  out (J, n_pts, 3) float32,
 * pix (J, n_pts) int32; cap, n_pts <= 2^29 (TGP_EINVAL above). */
int tgp_ball_select(const uint32_t *recs, const int *counts, const int32_t *sel, const int *job_img, const uint16_t *depth,
                    const float *camk, const float *pts, int J, int I, int H, int W, int cap, int n_pts, float *out, int32_t *pix,
                    tgp_stream_t stream);
int tgp_ball_sample(const uint32_t *recs, const int *counts, const int *job_img, const uint16_t *depth, const float *camk,
                    const float *pts, int J, int I, int H, int W, int cap, int n_pts, uint64_t seed, float *out, int32_t *pix,
                    tgp_stream_t stream);

/* ---- ICP pose refinement (csrc/icp.hip; additive, ABI stays 8) -------------------------------------------------------------------
 * Registration of point-and-normal models to observed clouds: J jobs in ONE launch, one workgroup per job, every iteration inside
 * the kernel.  No reference counterpart.  DESIGN.md section 3 "ICP refinement and model-based tracking" is the contract;
 * tests/icp_ref.py restates it in NumPy.  A job's result depends on neither the other jobs nor J; no float atomics: bit-repeatable.
 *
 * models (M, m_cap, 6) float32 [point, unit normal] in model units (tgp_mesh_sample's normals layout); model_count (M) int32 or NULL
 * (= m_cap), 1 <= count <= m_cap <= TGP_ICP_MAX_POINTS.  src (J, n_cap, 3) float32 camera-frame metres; src_count (J) int32 or NULL
 * (= n_cap), 0 <= count <= n_cap <= TGP_ICP_MAX_POINTS; a point with a non-finite coordinate is never an inlier.  job_model (J).
 * Start pose R (J,3,3), t (J,3), s (J): the similarity x = s R y + t from model to camera.  max_dist (J): the gate in metres.
 * mode 0 point-to-point (with_scale: Umeyama's scale), 1 point-to-plane; iters >= 1 the cap; tol_rot (radians) / tol_trans (metres):
 * the job stops after an iteration whose update is within both (both 0: exactly `iters` iterations); min_inliers (at least 6 is
 * enforced).  The state (R, t, s) is float64 throughout.  Per iteration:
 *   q_i = float32(R^T (p_i - t) / s), float64 arithmetic rounded once; the nearest model point y_j by tgp_nn1's float32 arithmetic
 *   (|q|^2, |y|^2 as three rounded products summed left to right, the inner product one product and two fmaf, (yy + qq) - 2 inner,
 *   first index on ties); an inlier when that value <= float32((max_dist / s)^2) and p_i is finite; fewer than min_inliers: status 1,
 *   the pose stays; mode 0: the closed-form similarity of the pairs (y_j, p_i) (Horn's quaternion of the centred cross-covariance);
 *   mode 1: one Gauss-Newton step on sum (n_j . (q_i + w x q_i + v - y_j))^2, damping 1e-9 trace(A) / 6, Cholesky (a non-positive
 *   pivot or a non-finite step: status 2, the pose stays), R <- R exp(w)^T, t <- t - s R v.
 * After the last iteration one more correspondence pass runs at the final pose.
 * -> R_out, t_out, s_out: the state rounded once; info (J,4) int32: status (0 ok, 1 too few inliers, 2 singular, 3 job_model or a
 * count out of range: nothing is read, the pose is copied through), final inliers, iterations done, 0; rmse (J): root mean square
 * of s |q_i - y_j| over the final inliers, NaN without any; corr (J, n_cap) int32 or NULL: the final pass's model index per source
 * point, -1 for a non-inlier and beyond src_count.
 * TGP_EINVAL (before any launch): a NULL required pointer, a size < 1, iters < 1, a mode outside 0 / 1, with_scale with mode 1.
 * TGP_EUNSUPPORTED: a cap above TGP_ICP_MAX_POINTS, J > 65535. */
#define TGP_ICP_MAX_POINTS 2048
typedef struct tgp_icp_args {
    const float *models;
    const int32_t *model_count;     /* may be NULL */
    int M, m_cap;
    const float *src;
    const int32_t *src_count;       /* may be NULL */
    const int32_t *job_model;
    int J, n_cap;
    const float *R, *t, *s;
    const float *max_dist;
    int mode, with_scale, iters;
    float tol_rot, tol_trans;
    int min_inliers;
    float *R_out, *t_out, *s_out;
    int32_t *info;
    float *rmse;
    int32_t *corr;                  /* may be NULL */
} tgp_icp_args;
int tgp_icp_max_points(void);
int tgp_icp_refine(const tgp_icp_args *args, tgp_stream_t stream);

/* ---- The supporting plane of depth frames (csrc/plane.hip; additive, ABI stays 8) ------------------------------------------------
 * The dominant plane of S depth frames by RANSAC and total least squares (tgp_plane_fit), its removal from the frames
 * (tgp_plane_cut), and the reference's weighted plane regression of point clouds (tgp_plane_lsq; tools/plane_utils.py).  DESIGN.md
 * section 3 "The supporting plane" is the contract; tests/plane_ref.py restates it in NumPy.  No float atomics anywhere: every
 * result is bit-repeatable, and a frame's (a cloud's) result depends on neither the other frames nor S.
 *
 * depth (S,H,W) uint16 millimetres, 0 invalid; camk (S,4) fx, fy, cx, cy; H, W < 32768, H*W < 2^24.  A valid pixel's point p is the
 * one tgp_cloud_select / tgp_ball_select give for that pixel and depth (csrc/pixel_point.h; same bits).  A plane is (n0, n1, n2, d)
 * float32 with n.p + d = 0, oriented so that d >= 0 (the camera, at the origin, is on the non-negative side).  The signed distance
 * of p is dist(p) = ((n0*px + n1*py) + n2*pz) + d in float32, every product and sum rounded on its own.
 *
 * tgp_plane_fit, frame s:
 *   Hypothesis h (0 <= h < hypotheses <= TGP_PLANE_MAX_HYPOTHESES): w = the Philox words of (seed, keys[s], TGP_PLANE_SITE, counter
 *   h); pixel i_k = (uint64(w[k]) * (H*W)) >> 32 for k = 0, 1, 2, a flat index y*W + x; a, b, c their points.  The hypothesis is VOID
 *   (count 0) when one of the three pixels is invalid, or when the cross product below has nn <= 1e-18.  Else, in float64 on the
 *   float32 points, every product and sum rounded on its own (no fma): e = b - a, f = c - a, cr = (e_y f_z - e_z f_y, e_z f_x - e_x f_z,
 *   e_x f_y - e_y f_x), nn = (cr_x cr_x + cr_y cr_y) + cr_z cr_z, n = cr / sqrt(nn), d = -((n_x a_x + n_y a_y) + n_z a_z); when d < 0
 *   both are negated; n and d are then rounded once to float32.
 *   Score: a valid pixel is an inlier of a plane when |dist(p)| <= tol.  counts[s][h] = the hypothesis's inliers over the frame
 *   (integers, added with integer atomics); best = the largest count, the first index on ties.
 *   Status 1 when counts[s][best] < max(min_inliers, 3) (no valid hypothesis included): plane = (0,0,0,0), final inliers 0.
 *   Else the plane is hypothesis `best`, and refine_iters (0..TGP_PLANE_MAX_REFITS) times: over the inliers of the current plane the
 *   float64 sums N, sum p (3) and sum p p^T (6, upper triangle) are taken in this FIXED order: the frame's flat pixels are cut into
 *   groups of 8 consecutive indices; thread t of TGP_PLANE_FIT_THREADS adds its groups t, t + THREADS, ... in that order, the pixels
 *   of a group in index order; the 64 lanes of a wave are joined by a shuffle tree (x += lane + 32, + 16, ... + 1), the waves in
 *   wave order.  m = sum p / N; C_ab = sum p_a p_b - (sum p_a)(sum p_b) / N; the normal is the unit eigenvector of C's smallest
 *   eigenvalue by cyclic Jacobi rotations in float64; d = -((n_x m_x + n_y m_y) + n_z m_z), negated with n when < 0, both rounded once
 *   to float32.  A non-finite result: status 2, the plane of before the refit stays and the refits end.  The inliers are selected
 *   again with the rounded plane.
 * -> plane (S,4) float32; info (S,4) int32: status, counts[s][best], the inliers of the returned plane, the frame's valid pixels;
 *    counts (S, hypotheses) int32: REQUIRED at this level, it is the accumulator of the scoring launch (ops.plane_fit allocates it
 *    and returns it on request).
 * TGP_EINVAL (before any launch): a NULL pointer, S, H or W < 1 or out of range, hypotheses outside [1, TGP_PLANE_MAX_HYPOTHESES],
 * refine_iters outside [0, TGP_PLANE_MAX_REFITS], tol negative or not finite, min_inliers < 0.  TGP_EUNSUPPORTED: S > 65535. */
#define TGP_PLANE_SITE 9      /* the draw site of the hypotheses (after TGP_MESH_SITE) */
#define TGP_PLANE_MAX_HYPOTHESES 1024
#define TGP_PLANE_MAX_REFITS 4
#define TGP_PLANE_FIT_THREADS 1024
typedef struct tgp_plane_fit_args {
    const uint16_t *depth;
    const float *camk;
    const uint64_t *keys;           /* (S) */
    uint64_t seed;
    int S, H, W;
    int hypotheses;
    float tol;
    int refine_iters, min_inliers;
    float *plane;
    int32_t *info;
    int32_t *counts;
} tgp_plane_fit_args;
int tgp_plane_fit(const tgp_plane_fit_args *args, tgp_stream_t stream);
/* out[s][y][x] = depth[s][y][x] when the pixel is valid and dist(p) > margin under plane[s], else 0: what is left is strictly
 * above the plane's band, on the camera's side.  A frame whose info[s][0] (tgp_plane_fit's status) is not 0 is copied through.
 * plane (S,4) and info (S,4) are DEVICE pointers: nothing visits the host between the fit and the cut.  side (S,H,W) uint8 or NULL:
 * 0 invalid pixel, 2 dist > margin, 3 dist < -margin, 1 otherwise (within the band); it is computed from plane[s] whatever the
 * status.  out may be depth itself.  margin >= 0.  Elementwise: bit-exact against the restatement. */
int tgp_plane_cut(const uint16_t *depth, const float *plane, const int32_t *info, const float *camk, int S, int H, int W,
                  float margin, uint16_t *out, uint8_t *side, tgp_stream_t stream);
/* The weighted regression z = a x + b y + c of B clouds pc (B,n,3) float32 with weights w (B,n) float32 (tools/plane_utils.py:
 * get_plane, get_plane_in_batch, get_plane_parameter), one workgroup per cloud.  M = sum w [x y 1]^T [x y 1] (six moments) and
 * r = sum w z [x y 1]^T are float64 sums, each term ((w * u) * v, the first product exact) rounded on its own, in the order of
 * tgp_plane_fit's sums with single points for groups and TGP_PLANE_LSQ_THREADS threads.  X = M^-1 r by the adjugate in float64.
 * The system counts as SINGULAR when |det M| <= 1e-12 |M00 M11 M22| or det M is not finite (n = 1 and n = 2 always are): every
 * output of that cloud is NaN -- the reference's torch.inverse raises on the CPU for an exactly singular matrix and returns
 * non-finite or meaningless numbers otherwise; nothing is raised from the device.
 * With q = ((a a + b b) + 1): dn = (a c, b c, -c) / (q + eps), normal = dn / |dn|, p2plane = c / sqrt(q), float64, rounded once.
 * eps is 0 in get_plane and 1e-8 in get_plane_in_batch.
 * -> X (B,3), normal (B,3), dn (B,3), p2plane (B) float32.  TGP_EINVAL: a NULL pointer, B or n < 1, eps negative or not
 * finite. */
#define TGP_PLANE_LSQ_THREADS 256
int tgp_plane_lsq(const float *pc, const float *w, int B, int n, double eps, float *X, float *normal, float *dn, float *p2plane,
                  tgp_stream_t stream);

/* ---- Segments of depth frames (csrc/segment.hip; additive, ABI stays 8) ------------------------------------------------------------
 * Connected-component labelling of S depth frames in one call: after tgp_plane_cut what is left of a frame are the objects on the
 * table, and this says which pixels belong to which.  No reference counterpart.  DESIGN.md section 3 "Segments of a depth frame" is
 * the contract; tests/segment_ref.py restates it in NumPy.  Every sum is an integer sum (integer atomics): the result is unique
 * whatever order the workgroups run in, equal to the restatement bit for bit, and a frame's result depends on neither the other
 * frames nor S.
 *
 * depth (S,H,W) uint16 millimetres, a pixel is valid when its depth is not 0 (tgp_plane_fit's rule); H, W < 32768, H*W < 2^24.
 * Two valid pixels that are neighbours (connectivity 4: left / right / up / down; 8: the diagonals too) are JOINED when
 * |z_p - z_q| <= max_step, on the millimetre values as ints (0 <= max_step <= 65535; 1 against 65535 is 65534 apart).  The
 * components are the classes of that relation.  A component's root is its smallest flat index y*W + x; it QUALIFIES with at least
 * min_pixels (>= 1) pixels; the qualifying components are ranked by ascending root; rank r < max_segments gets label r + 1, every
 * other pixel label 0.
 * -> labels (S,H,W) uint8;
 *    info (S,4) int32: status (1: more components qualified than max_segments, the first max_segments in root order are kept),
 *    segments kept, components that qualified, valid pixels;
 *    stats (S, max_segments, TGP_SEG_STAT_COLS) int64, row l - 1 for label l, rows past the kept count zero: pixels, y1, x1, y2, x2
 *    (the box, ends exclusive), root, sum x, sum y, sum z, sum x*z, sum y*z, min z (z in millimetres);
 *    centers (S, max_segments, 3) float32 or NULL (needs camk (S,4) fx, fy, cx, cy, else camk may be NULL): the centroid of the
 *    segment's points in metres, float64 on the integer sums with the float32 camk values widened, every operation rounded on its
 *    own, rounded once to float32: Z = sum z / n / 1000, X = (sum x*z - cx * sum z) / (fx * n) / 1000, Y likewise with cy, fy;
 *    rows past the kept count are NaN.
 * workspace: tgp_segment_workspace_bytes(S,H,W) bytes of device memory, 16-byte aligned (two words per pixel plus counters);
 * nothing in it needs initialising and nothing is kept between calls.
 * TGP_EINVAL (before any launch): a NULL required pointer, centers without camk, S, H or W < 1 or out of range, max_step outside
 * [0, 65535], connectivity not 4 or 8, min_pixels < 1, max_segments outside [1, TGP_SEG_MAX_SEGMENTS], workspace_bytes too small.
 * TGP_EUNSUPPORTED: S > 65535.  tgp_segment_workspace_bytes returns TGP_EINVAL / TGP_EUNSUPPORTED by the same rule. */
#define TGP_SEG_MAX_SEGMENTS 255
#define TGP_SEG_STAT_COLS 12
typedef struct tgp_segment_args {
    const uint16_t *depth;
    const float *camk;              /* may be NULL when centers is */
    int S, H, W;
    int max_step, connectivity, min_pixels, max_segments;
    uint8_t *labels;
    int32_t *info;
    int64_t *stats;
    float *centers;                 /* may be NULL */
    void *workspace;
    int64_t workspace_bytes;
} tgp_segment_args;
int64_t tgp_segment_workspace_bytes(int S, int H, int W);
int tgp_segment_depth(const tgp_segment_args *args, tgp_stream_t stream);

/* ---- Pose verification against depth frames (csrc/verify.hip; additive, ABI stays 8) -------------------------------------------------
 * Render-and-compare: J jobs in one call, job j = (frame job_img[j], mesh job_mesh[j], pose job_pose[j] (3,4) fp32 [s R | t]).  The
 * rendered surface of a job is what tgp_render_depth gives for a scene of that one instance -- the same vertex arithmetic, snapping,
 * drop rules, coverage, z and winner, d_r = rint(1000 z), 0 above 65535 -- but only inside the job's own projected box, and no
 * frame of it is written: every pixel the job covers is compared with the frame's d_o = depth[job_img[j], y, x] in registers and
 * falls in exactly one class, in this order:
 *    nodata     d_o == 0 or d_r == 0
 *    occluded   d_o + tau < d_r            (something stands in front; not held against the pose)
 *    match      |d_o - d_r| <= tau
 *    violation  d_o > d_r + tau            (the sensor saw through the model)
 * DESIGN.md section 3 "Pose verification" is the contract; tests/verify_ref.py restates it in NumPy on tests/render_ref.py.
 * depth (S,H,W) uint16 millimetres, camk (S,4) fp32 fx, fy, cx, cy, the mesh set as tgp_render_depth takes it, job_img / job_mesh
 * (J) int32, mask (S,H,W) uint8 with job_mask_val (J) uint8, or both NULL: all in device memory, read on the device only.
 * -> counts (J, TGP_VERIFY_COLS) int32: rendered (pixels covered), match, violation, occluded, nodata, in_mask (covered pixels whose
 *    mask byte is job_mask_val[j]; 0 without a mask), abs_sum (sum of |d_o - d_r| over the match pixels), dropped (triangles dropped
 *    by the near rule and by the guard band, summed); rendered == match + violation + occluded + nodata.
 *    score (J) fp32 = (float)match / (float)(rendered - occluded), correctly rounded; 0 when the denominator is 0.
 * A job whose job_img is outside [0,S) or whose mesh renders nothing by the renderer's rules gives a row of zeros.  Integer atomics
 * only: two calls give identical bytes.  workspace: tgp_verify_workspace_bytes(J, max_verts, max_faces) bytes, 16-byte aligned,
 * nothing in it needs initialising.  Four kernels on the caller's stream, nothing read by the host; graph-capturable.
 * TGP_EINVAL (before any launch): a NULL required pointer (with J > 0: the job arrays and the workspace), mask without job_mask_val,
 * S, M, H, W, n_verts, n_faces, max_verts or max_faces < 1, J < 0, tau < 0, near <= 0 or not finite, workspace_bytes too small.
 * TGP_EUNSUPPORTED: J > TGP_VERIFY_MAX_JOBS, tau > TGP_VERIFY_MAX_TAU (abs_sum <= tau * rendered stays below 2^31), H*W >= 2^24
 * (the conversions to fp32 stay exact), H or W > 16384, max_faces >= tgp_render_max_faces().  tgp_verify_workspace_bytes returns
 * TGP_EINVAL / TGP_EUNSUPPORTED by the same rule.  J == 0 launches nothing and returns 0. */
#define TGP_VERIFY_COLS 8
#define TGP_VERIFY_MAX_JOBS 65535
#define TGP_VERIFY_MAX_TAU 1000
typedef struct tgp_verify_args {
    const uint16_t *depth;
    const float *camk;
    const float *verts;
    const int32_t *faces;
    const int32_t *vptr, *fptr;
    int M, n_verts, n_faces, max_verts, max_faces;
    const int32_t *job_img, *job_mesh;
    const float *job_pose;
    const uint8_t *mask;            /* may be NULL */
    const uint8_t *job_mask_val;    /* required with mask, not read without */
    int S, H, W, J;
    int tau;
    float near;
    int32_t *counts;
    float *score;
    void *workspace;
    int64_t workspace_bytes;
} tgp_verify_args;
int64_t tgp_verify_workspace_bytes(int J, int max_verts, int max_faces);
int tgp_pose_verify(const tgp_verify_args *args, tgp_stream_t stream);

/* ---- BOP pose errors: the point-based errors (csrc/poseerr.hip; additive, ABI stays 8) -------------------------------------------
 * ADD, ADD-S (ADI), MSSD and MSPD of J (estimate, ground truth) pose pairs in one call.  DESIGN.md section 3 "BOP pose errors" is
 * the contract; tests/bop_ref.py restates it in NumPy.  Job j: the P vertices p_i of mesh job_mesh[j] of the packed mesh set (verts
 * (n_verts,3) float32, vptr (M+1) int32: tgp_render_depth's), the poses E = pose_est[j] and G = pose_gt[j], (3,4) float32 [s R | t],
 * model to camera in metres, the Q transforms S of symmetry group job_sym[j] of the packed table sym (n_syms,3,4) float32 [R | t] in
 * model units with sptr (G+1) int32, and camk[j] (4) float32 fx, fy, cx, cy (one row per JOB).  Everything is read on the device.
 *    add  = mean_i |E p_i - G p_i|
 *    adi  = mean_i min_k |E p_i - G p_k|
 *    mssd = min_S max_i |E p_i - G S p_i|
 *    mspd = min_S max_i |pi(E p_i) - pi(G S p_i)| in pixels, pi(x) = (fx x/z + cx, fy y/z + cy)
 * The float32 inputs are widened to float64 and every operation is float64, each product and sum rounded on its own; T p =
 * ((T0 x + T1 y) + T2 z) + T3 per row, G S p = G (S p); a distance is sqrt((dx dx + dy dy) + dz dz).  A job is spread over
 * TGP_POSEERR_SPLIT workgroups of 256 threads: workgroup b takes the points [b c, (b+1) c) with c = ceil(P / TGP_POSEERR_SPLIT) for
 * add and adi -- thread t adds its points b c + t, b c + t + 256, ... in that order, the threads are joined by a tree in LDS
 * (x[t] += x[t + 128], + 64, ... + 1), and the finishing launch adds the workgroups' sums in index order and divides by P -- and
 * wave w of workgroup b takes the symmetries 4 b + w, + 4 TGP_POSEERR_SPLIT, ...; max and min are exact in any order.  The
 * ground-truth points of adi pass through LDS in tiles of TGP_POSEERR_TILE points: no P x P matrix exists anywhere.  No
 * floating-point atomics: two calls give identical bytes, and a job's result depends on neither the other jobs nor J.
 * -> err (J,4) float64 = add, adi, mssd, mspd; sym_best (J,2) int32: the group-local index of the S that attains mssd and mspd,
 *    the lowest among equal computed values; status (J) int32, a bit set:
 *      1  job_mesh[j] or job_sym[j] out of range, rows of vptr / sptr that leave the arrays or are empty, or a group of more than
 *         max_syms transforms: nothing is read further, err is NaN and sym_best -1;
 *      2  a projected point (E p_i or a G S p_i) does not have z > near: mspd = +inf, sym_best[j][1] = -1, the rest is valid;
 *      4  (alone) a transformed point E p_i, G p_i or G S p_i, or an entry of camk[j], is not finite -- a pose, a transform, a vertex
 *         or an intrinsic holds an infinity or a NaN: err is NaN and sym_best -1, so no threshold counts the job as correct.
 * workspace: tgp_pose_errors_workspace_bytes(J) bytes, 16-byte aligned, nothing in it needs initialising.  Two kernels on the
 * caller's stream, nothing read by the host; graph-capturable.
 * TGP_EINVAL (before any launch): a NULL required pointer (with J > 0: the job arrays, the outputs and the workspace), M, n_verts,
 * G, n_syms or max_syms < 1, J < 0, near <= 0 or not finite, workspace_bytes too small.  TGP_EUNSUPPORTED: J > TGP_POSEERR_MAX_JOBS,
 * max_syms (the host's bound on a group's size) > TGP_POSEERR_MAX_SYMS.  J == 0 launches nothing and returns 0. */
#define TGP_POSEERR_COLS 4
#define TGP_POSEERR_MAX_JOBS 65535
#define TGP_POSEERR_MAX_SYMS 1024
#define TGP_POSEERR_SPLIT 32
#define TGP_POSEERR_TILE 1024
typedef struct tgp_poseerr_args {
    const float *verts;
    const int32_t *vptr;
    int M, n_verts;
    const float *sym;
    const int32_t *sptr;
    int G, n_syms, max_syms;
    const int32_t *job_mesh, *job_sym;
    const float *pose_est, *pose_gt;
    const float *camk;
    int J;
    float near;
    double *err;
    int32_t *sym_best;
    int32_t *status;
    void *workspace;
    int64_t workspace_bytes;
} tgp_poseerr_args;
int64_t tgp_pose_errors_workspace_bytes(int J);
int tgp_pose_errors(const tgp_poseerr_args *args, tgp_stream_t stream);

/* ---- BOP pose errors: two-pose VSD (csrc/vsd.hip on csrc/raster.h; additive, ABI stays 8) ------------------------------------------
 * Visible surface discrepancy of J jobs (frame job_img[j], mesh job_mesh[j], pose_est[j], pose_gt[j]) in one call.  The two
 * surfaces of a job, d_e and d_g in millimetres, are exactly what tgp_render_depth gives for a scene of that one instance at each
 * pose (tgp_pose_verify's sentence: the same vertex arithmetic, snapping, drop rules, coverage, z and winner, d = rint(1000 z), 0
 * above 65535); 0 -- nothing rendered, or over range -- means "not rendered".  No frame is written.  With d_o = depth[job_img[j], y,
 * x] (0: no data) and delta in millimetres, per pixel:
 *    vis(d)    = d > 0 and (d_o == 0 or d - d_o <= delta)
 *    visib_gt  = vis(d_g)
 *    visib_est = vis(d_e) or (visib_gt and d_e > 0)
 *    inter, union = visib_gt and / or visib_est
 *    within_k  = inter and |d_g - d_e| < job_tau[j][k]     for the job's n_tau integer thresholds (millimetres)
 * This is BOP's vsd with visib_mode 'bop19' and cost_type 'step', on depth along the optical axis instead of distance from the
 * camera centre (the deviation DESIGN.md "Pose verification" documents).
 * -> counts (J, TGP_VSD_COLS) int32: rendered_gt, rendered_est, visib_gt, visib_est, inter, union (pixel counts), dropped_gt,
 *    dropped_est (triangles dropped by the near rule and the guard band); within (J, n_tau) int32;
 *    err (J, n_tau) float32 = (float)(union - within_k) / (float)union, one correctly rounded division; 1 when union == 0.
 * A job whose job_img or job_mesh is out of range gives zeros and err 1.  All-integer up to the division, integer atomics only:
 * equal to the restatement (tests/bop_ref.py) bit for bit.  workspace: tgp_vsd_workspace_bytes(J, max_verts, max_faces) bytes,
 * 16-byte aligned, nothing in it needs initialising.  Four kernels on the caller's stream; graph-capturable.
 * TGP_EINVAL (before any launch): a NULL required pointer (with J > 0: the job arrays, the outputs and the workspace), S, M, H, W,
 * n_verts, n_faces, max_verts, max_faces or n_tau < 1, J < 0, delta < 0, near <= 0 or not finite, workspace_bytes too small.
 * TGP_EUNSUPPORTED: J > TGP_VERIFY_MAX_JOBS, n_tau > TGP_VSD_MAX_TAUS, delta > 65535, H*W >= 2^24, H or W > 16384, max_faces >=
 * tgp_render_max_faces().  A threshold is compared as the int it is; every useful one is in [0, 65535].  J == 0 returns 0. */
#define TGP_VSD_COLS 8
#define TGP_VSD_MAX_TAUS 16
typedef struct tgp_vsd_args {
    const uint16_t *depth;
    const float *camk;
    const float *verts;
    const int32_t *faces;
    const int32_t *vptr, *fptr;
    int M, n_verts, n_faces, max_verts, max_faces;
    const int32_t *job_img, *job_mesh;
    const float *pose_est, *pose_gt;
    const int32_t *job_tau;         /* (J, n_tau) */
    int S, H, W, J;
    int n_tau, delta;
    float near;
    int32_t *counts;
    int32_t *within;
    float *err;
    void *workspace;
    int64_t workspace_bytes;
} tgp_vsd_args;
int64_t tgp_vsd_workspace_bytes(int J, int max_verts, int max_faces);
int tgp_pose_vsd(const tgp_vsd_args *args, tgp_stream_t stream);

/* ---- Distance-field pose search (csrc/search.hip; additive, ABI stays 8) -----------------------------------------------------------
 * An exhaustive search of R rotations x D lattice translations per job against a quantised distance field of the job's model, held
 * in LDS.  DESIGN.md section 3 "Model-based acquisition" is the contract; tests/search_ref.py restates it in NumPy, bit for bit.
 *
 * tgp_field_build: models (M, m_cap, 6) float32 rows [point, normal] with model_count (M) int32 or NULL (= m_cap): tgp_icp_refine's
 * model set.  meta (M, 4) float32 = the cube's centre ctr (3) and the voxel edge: made by the host.  thresholds (M, cap) float32,
 * increasing, made by the host: T_l = ((l + 1) voxel / 4)^2.  -> field (M, G, G, G) uint8, voxel (ix, iy, iz) at (ix G + iy) G + iz:
 * with c_a = ctr_a + (i_a - G/2 + 0.5) voxel (float32, product and sum rounded on their own) and dv the least of tgp_nn1's float32
 * value (|y|^2 + |c|^2) - 2 fmaf(c_z, y_z, fmaf(c_y, y_y, c_x y_x)) over the model's points (a NaN value is skipped; no point: +inf),
 * the byte is the number of l with dv >= T_l.  One thread per voxel, the model in tiles through LDS; no square root, no division.
 *
 * tgp_pose_search: job j = (model job_model[j], cloud clouds[j] (n_cap, 3) float32 of which the first counts[j] rows are live (NULL:
 * n_cap) and a row with a non-finite coordinate contributes nothing, anchor anchors[j] (3), scale scales[j] metres per model unit).
 * rotations (R, 3, 3) float32 row-major, shared.  With inv = float32(1 / ((double)scale (double)voxel)) and, per rotation and point,
 *    e = p - anchor;  u_a = (R[0][a] e_0 + R[1][a] e_1) + R[2][a] e_2;  w_a = u_a inv + G/2;  b_a = floor(min(max(w_a, -512), 511))
 * -- float32, every product and sum rounded on its own, a NaN w_a giving -512 -- the cost of (rotation r, shift d) is the int32 sum
 * over the points of field[b + d], or cap where b + d leaves the grid; d = stride (a, b, c), a, b, c in [-K, K], shift index
 * ((a+K)(2K+1) + (b+K))(2K+1) + (c+K).  Per rotation the least cost and its shift (ties: the smaller index) go to the table
 * (J, R, 2) int32 = the workspace; per job the top rotations of least (cost, r) go to cost / rot / shift (J, top) int32 and poses
 * (J, top, 3, 4) float32 [R | t], t_i = anchor_i - s ((R_i0 m_0 + R_i1 m_1) + R_i2 m_2), m_a = ctr_a + (double)d_a voxel, float64
 * rounded once.  Rows beyond R, and every row of a job whose job_model is outside [0, M) or whose count is outside [0, n_cap], are
 * cost = INT32_MAX, rot = shift = -1 and a NaN pose (the table's rows of such a job are INT32_MAX, -1).  Integer arithmetic after
 * the floor, no atomics: two calls give identical bytes.  Two kernels on the caller's stream, nothing read by the host;
 * graph-capturable.  workspace: tgp_pose_search_workspace_bytes(J, R) bytes, 16-byte aligned, nothing in it needs initialising.
 * TGP_EINVAL: a NULL required pointer, M, J, R, n_cap or top < 1, K < 0, stride < 1, cap outside [1, 255], workspace_bytes too small.
 * TGP_EUNSUPPORTED: G not 16, 32 or 48, n_cap > TGP_SEARCH_MAX_POINTS, R > TGP_SEARCH_MAX_ROTATIONS, top > TGP_SEARCH_MAX_TOP,
 * K > TGP_SEARCH_MAX_K, K stride > TGP_SEARCH_MAX_REACH, J > 65535, m_cap > TGP_ICP_MAX_POINTS. */
#define TGP_SEARCH_MAX_POINTS 1024
#define TGP_SEARCH_MAX_ROTATIONS 4096
#define TGP_SEARCH_MAX_TOP 64
#define TGP_SEARCH_MAX_K 16
#define TGP_SEARCH_MAX_REACH 200
#define TGP_SEARCH_ROT_BLOCK 8
typedef struct tgp_field_args {
    const float *models;
    const int32_t *model_count;     /* may be NULL */
    int M, m_cap;
    const float *meta;
    const float *thresholds;
    int G, cap;
    uint8_t *field;
} tgp_field_args;
int tgp_field_build(const tgp_field_args *args, tgp_stream_t stream);
typedef struct tgp_pose_search_args {
    const uint8_t *field;
    const float *meta;
    int M, G, cap;
    const int32_t *job_model;
    const float *clouds;
    const int32_t *counts;          /* may be NULL */
    const float *anchors;
    const float *scales;
    int J, n_cap;
    const float *rotations;
    int R;
    int K, stride, top;
    int32_t *cost, *rot, *shift;
    float *poses;
    void *workspace;
    int64_t workspace_bytes;
} tgp_pose_search_args;
int64_t tgp_pose_search_workspace_bytes(int J, int R);
int tgp_pose_search(const tgp_pose_search_args *args, tgp_stream_t stream);

/* ---- Models from depth sequences: TSDF fusion and meshing (csrc/tsdf.hip; additive, ABI stays 8) ------------------------------------
 * DESIGN.md section 3 "Models from depth sequences" is the contract; tests/tsdf_ref.py restates both kernels in NumPy, bit for bit.
 * M cubes of G^3 voxels in model units: sum, weight (M, G, G, G) int32, voxel (ix, iy, iz) at (ix G + iy) G + iz, and meta (M, 4)
 * float32 = the cube's centre ctr (3) and the voxel edge (tgp_field_build's layout).  A voxel's centre along axis a is
 * c_a = ctr_a + (((float)i_a + 0.5f) - G/2) voxel: float32, the product and each sum rounded on their own.
 *
 * tgp_tsdf_integrate: job j = (frame job_img[j], volume job_model[j], pose job_pose[j] (3,4) float32 [s R | t], model to camera in
 * metres); depth, camk, mask and job_mask_val as tgp_pose_verify takes them.  Every voxel of the job's volume, in float32:
 *    p   = raster_vertex's pose of the centre: p_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3;          skipped unless p_z > near
 *    u   = K0 (p_x / p_z) + K2, v = K1 (p_y / p_z) + K3 (correctly rounded division, no contraction); the pixel is (rintf(u), rintf(v)),
 *          ties to even;                                 skipped unless 0 <= rintf(u) <= W - 1 and 0 <= rintf(v) <= H - 1 (a NaN is not)
 *    d   = depth[img, y, x];                             skipped if d == 0, or if a mask is given and mask[img, y, x] != job_mask_val[j]
 *    sdf = (float)d - p_z 1000.f;                        skipped if sdf < -trunc
 *    q   = (int)rintf(fminf(sdf, trunc) inv), inv = (float)(1024 / (double)trunc) made by the host;     sum += q, weight += 1
 * The volumes are ADDED to: integer sums, so the result depends on neither the order of the jobs nor how they are spread over calls.
 * A workgroup owns one 8 x 8 x 8 brick, walks all J jobs with the brick's sums in registers and adds them to memory once: no atomics.
 * A job whose job_img is outside [0, S) or whose job_model is outside [0, M) adds nothing.  -> status (J) int32: 0, or 1 for such a
 * job.  One kernel on the caller's stream, nothing read by the host; graph-capturable.
 * TGP_EINVAL (before any launch): a NULL required pointer (with J > 0: the job arrays and status), mask without job_mask_val, S, H,
 * W or M < 1, J < 0, trunc, inv or near <= 0 or not finite.  TGP_EUNSUPPORTED: G not a multiple of 8 in [TGP_TSDF_MIN_G,
 * TGP_TSDF_MAX_G], J > TGP_TSDF_MAX_JOBS (|sum| <= 1025 J stays below 2^31), H or W > 16384, M (G/8)^3 >= 2^31.  J == 0 returns 0.
 *
 * tgp_tsdf_mesh_count / tgp_tsdf_mesh_emit: marching tetrahedra over volume ``model``.  The cube with its corner (0,0,0) at voxel
 * (ix, iy, iz), ix, iy, iz < G - 1, takes part iff all eight corners have weight >= min_weight (>= 1); a corner is inside iff
 * sum < 0.  The cube is split into the six Kuhn tetrahedra: tetrahedron k walks from corner (0,0,0) to (1,1,1) by the three axis
 * steps in the order of the k-th permutation of (0, 1, 2) in lexicographic order; its corners in that walk are its path order.
 * One or three corners inside: one triangle, its vertices on the three cut edges in the path order of the edges' other ends (the
 * three outside corners, or the three inside ones).  Two inside (I0, I1) and two outside (O0, O1), each pair in path order: the quad
 * I0O0, I0O1, I1O1, I1O0 as the triangles (0,1,2), (0,2,3).  A triangle whose bit in the tetrahedron's word of csrc/tsdf.hip's
 * tsdf_flip (bit = the 4-bit case, bit c of which is path corner c inside) is set swaps its second and third vertex: every normal then points from
 * the inside corners to the outside ones.  The vertex on an edge is computed from the end a earlier in the path (the one with the
 * smaller flat index) to the other end b: f_a = (float)sum_a / (float)weight_a, t = f_a / (f_a - f_b), p = p_a + t (p_b - p_a) per
 * axis on the voxel centres above, float32, each operation rounded on its own -- every tetrahedron that shares the edge gets the
 * same bits.  Zero-area triangles are kept.
 * count: counts (G^3) int32 = the triangles of each cube at its (0,0,0) corner's flat index (0 where there is no cube).  The host
 * makes offsets (G^3) int64 = the inclusive prefix sum of counts.  emit: triangle n of the soup -- cube flat index, then
 * tetrahedron, then triangle -- goes to verts[9 n .. 9 n + 8] if n < face_cap; info (2) int64 = {min(total, face_cap), total >
 * face_cap}.  Rows of verts at and beyond 3 min(total, face_cap) are not written.  One kernel each; nothing read by the host.
 * TGP_EINVAL: a NULL required pointer (emit: verts may be NULL when face_cap is 0), M < 1, model outside [0, M), min_weight < 1,
 * face_cap < 0.  TGP_EUNSUPPORTED: G as above, face_cap > TGP_TSDF_MAX_FACES. */
#define TGP_TSDF_MIN_G 16
#define TGP_TSDF_MAX_G 256
#define TGP_TSDF_MAX_JOBS 65535
#define TGP_TSDF_MAX_FACES 100000000
typedef struct tgp_tsdf_integrate_args {
    const uint16_t *depth;
    const float *camk;
    int S, H, W;
    int32_t *sum, *weight;
    const float *meta;
    int M, G;
    const int32_t *job_img, *job_model;
    const float *job_pose;
    const uint8_t *mask;            /* may be NULL */
    const uint8_t *job_mask_val;    /* required with mask, not read without */
    int J;
    float trunc, inv, near;
    int32_t *status;
} tgp_tsdf_integrate_args;
int tgp_tsdf_integrate(const tgp_tsdf_integrate_args *args, tgp_stream_t stream);
typedef struct tgp_tsdf_mesh_args {
    const int32_t *sum, *weight;
    const float *meta;
    int M, G, model, min_weight;
    int32_t *counts;
    const int64_t *offsets;         /* emit only */
    float *verts;                   /* emit only */
    int64_t face_cap;               /* emit only */
    int64_t *info;                  /* emit only */
} tgp_tsdf_mesh_args;
int tgp_tsdf_mesh_count(const tgp_tsdf_mesh_args *args, tgp_stream_t stream);
int tgp_tsdf_mesh_emit(const tgp_tsdf_mesh_args *args, tgp_stream_t stream);

/* ---- Ray casting of TSDF volumes (csrc/raycast.hip; additive, ABI stays 8) ----------------------------------------------------------
 * DESIGN.md section 3 "Ray casting and frame-to-model tracking" is the contract; tests/raycast_ref.py restates the kernel in NumPy, bit
 * for bit.  The volumes are tgp_tsdf_integrate's (sum, weight, meta above).  Job j = (volume job_model[j], intrinsics camk[job_img[j]]
 * = fx, fy, cx, cy, inverse pose job_inv[j] (3,4) float32 = camera (metres) -> model units, the inverse of the [s R | t] that
 * tgp_tsdf_integrate takes, made in float64 and rounded once, window job_window[j] = (u0, v0, du, dv) float32); the call casts h x w
 * rays per job, ray (r, c) through the pixel coordinates u = u0 + (float)c du, v = v0 + (float)r dv (the loaders' convention: pixel
 * (x, y) is the ray ((x - cx) / fx, (y - cy) / fy, 1)).  float32, every operation rounded on its own, correctly rounded divisions and
 * square roots; I = job_inv[j], (c_a, voxel) = meta, h = (float)(G/2) - 0.5f, L = (float)(G - 1):
 *    d    = ((u - cx) / fx, (v - cy) / fy);    m_a = (I_a0 d_x + I_a1 d_y) + I_a2;    e_a = m_a / voxel;    o_a = (I_a3 - c_a) / voxel + h
 *           -- the ray in the volume's voxel coordinates (voxel centre i at coordinate i) is g_a(z) = o_a + z e_a, z the camera depth
 *    clip : z_in = near, z_out = +inf; per axis with e_a != 0: t0 = (0 - o_a) / e_a, t1 = (L - o_a) / e_a, z_in = fmaxf(z_in, fminf(t0,
 *           t1)), z_out = fminf(z_out, fmaxf(t0, t1)); with e_a == 0 the ray misses unless 0 <= o_a <= L.  len = sqrtf((e_x e_x + e_y e_y)
 *           + e_z e_z); dz = step / len.  The ray misses unless len > 0, dz > 0, z_in <= z_out and all of these are finite.
 *    march: sample k = 0, 1, ..., max_samples - 1 at z_k = z_in + (float)k dz while z_k <= z_out.  Its point g = o + z_k e; it is
 *           UNKNOWN unless -1 <= g_a <= G on every axis.  Its cell is i_a = clamp((int)floorf(g_a), 0, G - 2), t_a = g_a - (float)i_a;
 *           the cell's eight voxels must all have weight >= min_weight, else the sample is unknown; f_v = (float)sum / (float)weight.
 *           f = trilinear: along z first, c_xy = f_xy0 + t_z (f_xy1 - f_xy0); c_x = c_x0 + t_y (c_x1 - c_x0); f = c_0 + t_x (c_1 - c_0).
 *           An unknown sample forgets the previous one.  A known f > 0 becomes the previous one.  A known f <= 0 ends the ray: a hit
 *           iff the sample before it was known (and so positive), at z* = z_{k-1} + dz (f_{k-1} / (f_{k-1} - f_k)); else a miss.
 *    hit  : g* = o + z* e, its cell and t as above (a miss if g* is out of the range above or one of the eight is unseen);
 *           gradient n_x = c_1 - c_0;  n_y = d_0 + t_x (d_1 - d_0), d_x = c_x1 - c_x0;  n_z = q_0 + t_x (q_1 - q_0), q_x = r_x0 + t_y
 *           (r_x1 - r_x0), r_xy = f_xy1 - f_xy0;  s = sqrtf((n_x n_x + n_y n_y) + n_z n_z), a miss unless 0 < s < inf; normal = n / s
 *           (the TSDF is positive outside: outward);  vertex_a = c_a + ((g*_a + 0.5f) - (float)(G/2)) voxel (model units).
 * -> z (J,h,w) float32 = z* (0 on a miss); depth (J,h,w) uint16 = rintf(z* 1000.f), 0 beyond 65535 or on a miss; vertex, normal
 * (J,h,w,3) float32, zeros on a miss; count (J) int32 = the job's hits; status (J) int32 = 1 for a job whose job_model is outside
 * [0, M) or whose job_img is outside [0, S): all its rays miss.  A NaN anywhere makes a comparison false and the ray a miss; cell
 * indices are clamped as integers before every load.  One wave casts an 8 x 8 patch of rays; count is summed by wave ballots and one
 * integer atomic per wave on a zeroed word: two calls give identical bytes.  One memset and one kernel on the caller's stream, nothing
 * read by the host; graph-capturable.
 * TGP_EINVAL (before any launch): a NULL required pointer, S or M < 1, J < 0, h or w < 1, min_weight < 1, step or near <= 0 or not
 * finite.  TGP_EUNSUPPORTED: G not a multiple of 8 in [TGP_TSDF_MIN_G, TGP_TSDF_MAX_G], J > TGP_TSDF_MAX_JOBS, h or w >
 * TGP_RAYCAST_MAX_SIDE, step < 1/16 (the march is at most 16 sqrt(3) G + 2 samples).  J == 0 returns 0. */
#define TGP_RAYCAST_MAX_SIDE 16384
typedef struct tgp_tsdf_raycast_args {
    const int32_t *sum, *weight;
    const float *meta;
    int M, G;
    const float *camk;
    int S;
    const int32_t *job_img, *job_model;
    const float *job_inv, *job_window;
    int J, h, w, min_weight;
    float step, near;
    float *z;
    uint16_t *depth;
    float *vertex, *normal;
    int32_t *count, *status;
} tgp_tsdf_raycast_args;
int tgp_tsdf_raycast(const tgp_tsdf_raycast_args *args, tgp_stream_t stream);

/* ---- Dense projective ICP against ray-cast maps (csrc/icp_dense.hip; additive, ABI stays 9) -------------------------------------------
 * DESIGN.md section 3 "Dense projective registration" is the contract; tests/icp_dense_ref.py restates it in NumPy.  Registration of
 * depth frames to the vertex / normal maps of ONE tgp_tsdf_raycast call: the map is indexed by pixel, so a source pixel finds its
 * model point by projection, not by search.  J jobs in ONE launch, one workgroup per job, every iteration inside the kernel; nothing
 * allocated, nothing read by the host, graph-capturable.  A job's result depends on neither the other jobs nor J; no atomics:
 * bit-repeatable.
 *
 * depth (S,H,W) uint16 millimetres, camk (S,4) = fx, fy, cx, cy, mask (S,H,W) uint8 or NULL with job_mask_val (J), as
 * tgp_tsdf_integrate takes them.  The maps: vertex, normal (J,h,w,3) float32 in the MODEL frame, z (J,h,w) float32 (a cell is a hit
 * iff z > 0), job_window (J,4) = u0, v0, du, dv, job_ref (J,3,4) float32 = the [s R | t] the maps were cast from (the job_pose whose
 * inverse tgp_tsdf_raycast took).  job_img (J): the job's frame and intrinsics.  job_rect (J,4) int32 = x0, y0, x1, y1 inclusive and
 * stride >= 1: the job's source pixels are (x0 + i stride, y0 + k stride), i, k >= 0, that lie in the rectangle clipped to the frame
 * [0, W-1] x [0, H-1], numbered row-major among themselves, e = k' nx + i' (nx of them a row); no cap on their number.  Start pose R
 * (J,3,3), t (J,3), s (J): x = s R y + t from model to camera, as tgp_icp_refine takes it; max_dist (J): the gate in metres; iters,
 * tol_rot, tol_trans, min_inliers with tgp_icp_refine's meaning.  The state (R, t) is float64 throughout; s does not move.
 * Per iteration, for each source pixel (x, y) with d = depth[img, y, x] != 0 and (with a mask) mask[img, y, x] == job_mask_val[j];
 * float32, every operation rounded on its own, correctly rounded divisions, no contraction, except where float64 is named:
 *   p   = tgp_pixel_point of (x, y, d) (csrc/pixel_point.h: the crops' bits);
 *   q   = float32(R^T (p - t) / s): tgp_icp_refine's float64 sequence, rounded once;
 *   c_r = ((T_r0 q_x + T_r1 q_y) + T_r2 q_z) + T_r3, T = job_ref;                                skipped unless c_z > 1e-6f
 *   u   = K0 (c_x / c_z) + K2, v = K1 (c_y / c_z) + K3 (tgp_tsdf_integrate's projection);
 *   col = rintf((u - u0) / du), row = rintf((v - v0) / dv), ties to even; the pixel is ASSOCIATED iff 0 <= col <= w - 1, 0 <= row <=
 *         h - 1 and z[row, col] > 0 (a NaN fails every comparison);
 *   y, n = vertex, normal[row, col]; e = q - y; the pixel is an INLIER iff ((e_x e_x + e_y e_y) + e_z e_z) <= float32((max_dist / s)^2)
 *         (the threshold in float64, rounded once, as tgp_icp_refine forms it);
 *   the inliers' rows [q x n, n] and residuals (q - y) . n, in float64 on the float32 values, go into tgp_icp_refine's mode 1: the 21
 *   + 6 + 1 sums, fewer than max(min_inliers, 6) inliers: status 1; damping 1e-9 trace(A) / 6, Cholesky (a non-positive pivot or a
 *   non-finite step: status 2), R <- R exp(w)^T, t <- t - s R v, the same stop rule (csrc/icp_solve.h is the one text of both).
 * The sums are float64 in a fixed order: per lane over e = tid, tid + 512, ... in that order, a shuffle tree across the wave, the
 * waves serially.  After the last iteration one more association pass runs at the final pose.  A job that fails (status 1 or 2)
 * goes back to the pose it came with: R_out, t_out are the inputs' bits, and the final pass runs there.
 * -> R_out, t_out, s_out (s_out = s); info (J,4) int32 = status (0 ok, 1 too few inliers, 2 singular or not finite, 3 job_img
 * outside [0, S): nothing else is read, the pose is copied through, rmse NaN, corr -1), final inliers, iterations done, candidates =
 * the source pixels associated at the START pose, before the distance gate; rmse (J): root mean square of s |q - y| over the final
 * inliers (float64 on the float32 values), NaN without any; corr (J, corr_cap) int32 or NULL: for e < corr_cap the final pass's cell
 * row w + col of source pixel e if it is an inlier, else -1 (beyond the job's pixel count too).
 * TGP_EINVAL (before any launch, the outputs untouched): a NULL required pointer, mask without job_mask_val, S, H or W < 1, J < 0, h
 * or w < 1, stride < 1, iters < 1, a negative or NaN tolerance, min_inliers < 0, corr_cap < 0, corr_cap > 0 without corr.
 * TGP_EUNSUPPORTED: h or w > TGP_RAYCAST_MAX_SIDE, H or W > 16384, J > 65535.  J == 0 returns 0. */
typedef struct tgp_icp_dense_args {
    const uint16_t *depth;
    const float *camk;
    int S, H, W;
    const uint8_t *mask;            /* may be NULL */
    const uint8_t *job_mask_val;    /* required with mask, not read without */
    const float *vertex, *normal, *z;
    int h, w;
    const float *job_window, *job_ref;
    const int32_t *job_img, *job_rect;
    int J, stride;
    const float *R, *t, *s;
    const float *max_dist;
    int iters;
    float tol_rot, tol_trans;
    int min_inliers;
    float *R_out, *t_out, *s_out;
    int32_t *info;
    float *rmse;
    int32_t *corr;                  /* may be NULL */
    int corr_cap;
} tgp_icp_dense_args;
int tgp_icp_dense(const tgp_icp_dense_args *args, tgp_stream_t stream);

/* ---- Indexed meshes from volumes: welding and vertex normals (csrc/weld.hip; additive, ABI stays 8) ---------------------------------
 * DESIGN.md section 3 "Indexed meshes from volumes" is the contract; tests/weld_ref.py restates every kernel in NumPy, bit for bit.
 * The volumes, the cubes that mesh, the tetrahedra and the triangles' order are tgp_tsdf_mesh_count / _emit's above.
 *
 * A vertex is named by the voxel edge it cuts: key = flat(A) 8 + d, A the edge's componentwise smaller end (the end earlier in the
 * Kuhn path), flat(A) = (ix G + iy) G + iz, d = dx << 2 | dy << 1 | dz in 1..7 the step to the other end B = A + d (the 19 edges of
 * a cube are its axis edges, face diagonals and body diagonal).  The vertex (A, d) EXISTS iff (sum[A] < 0) != (sum[B] < 0) and at
 * least one cube that holds both ends meshes (all eight corners with weight >= min_weight, origin < G - 1 on every axis): the cubes
 * whose origin equals A on the axes where d steps and is A or A - 1 on the others.  Its position is tgp_tsdf_mesh_emit's, from A to
 * B: f_a = (float)sum_A / (float)weight_A, t = f_a / (f_a - f_b), p = p_A + t (p_B - p_A) per axis.  Vertices are numbered in
 * ascending key.  A corner whose sum is 0 is outside and gives t = 0 on each of its cut edges: those vertices have equal positions
 * and different names, and stay distinct vertices.
 *   mark : mask (G^3) uint8, bit d of mask[A] set iff (A, d) exists; vcounts (G^3) int32 = popcount(mask).  The host makes voffsets
 *          (G^3) int64 = the inclusive prefix sum of vcounts; index(A, d) = voffsets[A] - popcount(mask[A]) + popcount(mask[A] &
 *          ((1 << d) - 1)).
 *   count: fcounts (G^3) int32 = the cube's triangles whose three indices are all < vert_cap (0 where there is no cube).  The host
 *          makes foffsets (G^3) int64 = the inclusive prefix sum of fcounts.
 *   verts: vertex n goes to verts[3 n .. 3 n + 2] if n < vert_cap.
 *   faces: the counted triangles in tgp_tsdf_mesh_emit's order -- cube flat index, tetrahedron, triangle, the same winding --
 *          triangle n to faces[3 n .. 3 n + 2] (int32 indices, local to the mesh) if n < face_cap.  info (3) int64 = {min(vertices,
 *          vert_cap), min(counted triangles, face_cap), status}; status bit 1: counted triangles were dropped by face_cap, bit 2:
 *          vertices lie beyond vert_cap (a triangle that names one of them is not counted).
 * With vert_cap >= the vertices and face_cap >= the triangles, verts[faces] is tgp_tsdf_mesh_emit's soup byte for byte.  Rows at
 * and beyond the counts are not written.  One kernel each on the caller's stream; nothing read by the host.
 * TGP_EINVAL: a NULL pointer that the stage reads or writes (verts / faces may be NULL when their cap is 0), M < 1, model outside
 * [0, M), min_weight < 1, a cap < 0.  TGP_EUNSUPPORTED: G as above, vert_cap > TGP_WELD_MAX_VERTS, face_cap > TGP_TSDF_MAX_FACES.
 *
 * tgp_weld_cluster: decimation by voxel clusters, the device's share.  A vertex (A, d) belongs to the cell A / c per axis (integer
 * division) of a grid of side ceil(G / c), cell (cx, cy, cz) at (cx side + cy) side + cz; c = cluster in {2, 4, 8}.  Per vertex n <
 * vert_cap of tgp_tsdf_weld_verts' rows: vcell[n] = its cell, and per axis o = llrint(((double)p - (double)c0) (65536.0 /
 * (double)voxel)), c0 the float32 centre of voxel 0 on that axis, is added to cell_sums (side^3, 3) int64 and 1 to cell_counts (side^3)
 * int32, by integer atomics on words the call zeroes first.  The host numbers the occupied cells in ascending flat index and makes the
 * representative of a cell, float64 rounded to float32 once:  (float)((double)c0 + (((double)sum / (double)count) (double)voxel) /
 * 65536.0).  Two memsets and one kernel on the caller's stream; nothing read by the host.
 * TGP_EINVAL: a NULL pointer, M < 1, model outside [0, M), vert_cap < 0.  TGP_EUNSUPPORTED: G as above, cluster not 2, 4 or 8,
 * vert_cap > TGP_WELD_MAX_VERTS.
 *
 * tgp_mesh_vertex_normals: area-weighted vertex normals of a packed mesh set (tgp_render_depth's: verts (V,3) float32, faces (F,3)
 * int32 local to their mesh, vptr / fptr (M+1) int32).  Per face of mesh m, float32, each operation rounded on its own:
 *    u = p1 - p0, w = p2 - p0;  c = (u_y w_z - u_z w_y,  u_z w_x - u_x w_z,  u_x w_y - u_y w_x)
 *    q_k = llrint((double)c_k scale[m]) (ties to even; 0 unless |(double)c_k scale[m]| < 4e15)
 * and q is added to the three int64 sums of each of the face's three vertices by integer atomics (the sums are the same in any
 * order).  A face with an index outside its mesh adds nothing.  Then per vertex, float64: (0, 0, 0) if its three sums are zero, else
 * n = s / sqrt((s_x s_x + s_y s_y) + s_z s_z), correctly rounded square root and divisions, each component rounded to float32 once.
 * sums (V,3) int64 is workspace, zeroed by the call.  One memset and two kernels on the caller's stream; nothing read by the host.
 * TGP_EINVAL: a NULL required pointer, M < 1, V or F < 0.  TGP_EUNSUPPORTED: V > TGP_WELD_MAX_VERTS, F > TGP_TSDF_MAX_FACES. */
#define TGP_WELD_MAX_VERTS 300000000
typedef struct tgp_tsdf_weld_args {
    const int32_t *sum, *weight;
    const float *meta;
    int M, G, model, min_weight;
    uint8_t *mask;                  /* mark writes; count, verts and faces read */
    int32_t *vcounts;               /* mark only */
    const int64_t *voffsets;        /* count, verts, faces */
    int32_t *fcounts;               /* count writes; faces reads */
    const int64_t *foffsets;        /* faces only */
    int64_t vert_cap;               /* count, verts, faces */
    int64_t face_cap;               /* faces only */
    float *verts;                   /* verts only */
    int32_t *faces;                 /* faces only */
    int64_t *info;                  /* faces only */
} tgp_tsdf_weld_args;
int tgp_tsdf_weld_mark(const tgp_tsdf_weld_args *args, tgp_stream_t stream);
int tgp_tsdf_weld_count(const tgp_tsdf_weld_args *args, tgp_stream_t stream);
int tgp_tsdf_weld_verts(const tgp_tsdf_weld_args *args, tgp_stream_t stream);
int tgp_tsdf_weld_faces(const tgp_tsdf_weld_args *args, tgp_stream_t stream);
typedef struct tgp_weld_cluster_args {
    const uint8_t *mask;
    const int64_t *voffsets;
    const float *verts;
    const float *meta;
    int M, G, model, cluster;
    int64_t vert_cap;
    int32_t *vcell;                 /* (vert_cap) */
    int64_t *cell_sums;             /* (side^3, 3) */
    int32_t *cell_counts;           /* (side^3) */
} tgp_weld_cluster_args;
int tgp_weld_cluster(const tgp_weld_cluster_args *args, tgp_stream_t stream);
typedef struct tgp_mesh_normals_args {
    const float *verts;
    const int32_t *faces;
    const int32_t *vptr, *fptr;
    int M;
    int64_t V, F;
    const double *scale;            /* (M) */
    int64_t *sums;                  /* (V,3) workspace */
    float *normals;                 /* (V,3) */
} tgp_mesh_normals_args;
int tgp_mesh_vertex_normals(const tgp_mesh_normals_args *args, tgp_stream_t stream);

/* ---- Vertex / normal maps of posed meshes (csrc/meshmaps.hip; additive, ABI stays 9) -------------------------------------------------
 * DESIGN.md section 3 "Mesh maps and dense model-based tracking" is the contract; tests/meshmaps_ref.py restates it in NumPy on
 * tests/render_ref.py.  J jobs in one call; job j = (intrinsics camk[job_img[j]] = fx, fy, cx, cy, mesh job_mesh[j] of the packed
 * mesh set as tgp_pose_verify takes it, pose job_pose[j] (3,4) fp32 [s R | t], window job_window[j] = (u0, v0, du, dv)).  Cell (r, c) of
 * the job's h x w maps is the pixel coordinate (u0 + c du, v0 + r dv): tgp_tsdf_raycast's convention, so tgp_icp_dense takes the maps
 * (z, vertex, normal, with job_window and job_ref = job_pose) as it takes a ray cast's.
 * The window is a camera: K' = (fx / du, fy / dv, (cx - u0) / du, (cy - v0) / dv) in float32, correctly rounded divisions, every
 * operation rounded on its own.  The job is rasterised as a w x h frame under K' by tgp_render_depth's rules unchanged (the vertex
 * arithmetic, the 1/256 snapping, the near rule and the guard band, coverage, z, the smallest key {z bits, face}, both windings): with
 * window (0, 0, 1, 1) and (h, w) = (H, W), K' is K in every bit and z and face are tgp_render_depth's of a one-instance scene.  A
 * window holding a NaN or a zero step leaves no vertex inside the guard band, an infinite step leaves no triangle an area: every
 * triangle goes and every cell misses, by the arithmetic alone.
 * The winner of a cell, face f with snapped corner records v_0..v_2 and model corners p_0..p_2 (corners 1 and 2 change places where
 * the snapped area is negative), float32, every operation rounded on its own, no contraction:
 *    e_k = the edge integers at the cell's sample (256 c, 256 r), as the rasteriser's sweep forms them; w_k = (float)e_k / (float)area;
 *    z = the key's high word; b_k = (w_k iz_k) z; vertex_a = (b_0 p0_a + b_1 p1_a) + b_2 p2_a   (perspective-correct, MODEL frame)
 *    vnormals == NULL (face normals): u = p1 - p0, v = p2 - p0, n = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x);
 *    vnormals (n_verts,3) given: n_a = (b_0 n0_a + b_1 n1_a) + b_2 n2_a over the corners' rows;
 *    s = sqrtf((n_x n_x + n_y n_y) + n_z n_z); the cell is a MISS unless 0 < s < inf; normal = n / s.  Face normals only: m_r = (T_r0
 *    n_x + T_r1 n_y) + T_r2 n_z on the unit normal, T = job_pose; ray = (((float)c - K'2) / K'0, ((float)r - K'3) / K'1, 1); the normal
 *    is negated iff (m_x ray_x + m_y ray_y) + m_z > 0.  Vertex normals are not flipped.
 * -> z (J,h,w) fp32, 0 on a miss; depth (J,h,w) uint16 = rint(1000 z), 0 above 65535; vertex, normal (J,h,w,3) fp32, zeros on a miss;
 * face (J,h,w) int32 or NULL, -1 on a miss; count (J) int32 = the job's hits; dropped (J) int32 = triangles dropped by the near rule
 * and the guard band, summed; status (J) int32 = 1 for a job whose job_img is outside [0, S) or whose mesh renders nothing by the
 * renderer's rules: all its cells miss.  EVERY cell of every job is written, and count and dropped are zeroed by the call: no output
 * needs clearing.  Integer atomics only: two calls give identical bytes, and a job's bytes do not depend on the other jobs.
 * workspace: tgp_mesh_maps_workspace_bytes(J, max_verts, max_faces) bytes, 16-byte aligned, nothing in it needs initialising.  Three
 * kernels on the caller's stream, nothing read by the host; graph-capturable.
 * TGP_EINVAL (before any launch, the outputs untouched): a NULL required pointer (with J > 0: the job arrays, the outputs but face,
 * the workspace), S, M, h, w, n_verts, n_faces, max_verts or max_faces < 1, J < 0, near <= 0 or not finite, workspace_bytes too small.
 * TGP_EUNSUPPORTED: h or w > TGP_RAYCAST_MAX_SIDE, J > TGP_MAPS_MAX_JOBS, max_faces >= tgp_render_max_faces().
 * tgp_mesh_maps_workspace_bytes returns TGP_EINVAL / TGP_EUNSUPPORTED by the same rule.  J == 0 launches nothing and returns 0. */
#define TGP_MAPS_MAX_JOBS 65535
typedef struct tgp_mesh_maps_args {
    const float *camk;
    const float *verts;
    const int32_t *faces;
    const int32_t *vptr, *fptr;
    int M, n_verts, n_faces, max_verts, max_faces;
    const float *vnormals;          /* may be NULL: face normals */
    const int32_t *job_img, *job_mesh;
    const float *job_pose, *job_window;
    int S, J, h, w;
    float near;
    float *z;
    uint16_t *depth;
    float *vertex, *normal;
    int32_t *face;                  /* may be NULL */
    int32_t *count, *dropped, *status;
    void *workspace;
    int64_t workspace_bytes;
} tgp_mesh_maps_args;
int64_t tgp_mesh_maps_workspace_bytes(int J, int max_verts, int max_faces);
int tgp_mesh_maps(const tgp_mesh_maps_args *args, tgp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TGPOSE_H */
