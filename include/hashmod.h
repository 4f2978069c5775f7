/*
 * hashmod.h - C ABI of libhashmod.so, the MI355X (gfx950) implementation of the
 * hash-grid encode / SDF-MLP / sphere-tracing hot path of HashModNFFBanks-IDR.
 *
 * This is the drop-in boundary: plain C, raw device pointers and sizes, no torch types.
 * The reference has no native ABI on its live path (its PyTorch modules call ATen ops);
 * each entry point below names the reference Python interface it replaces
 * (paths relative to the reference's code/ directory).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; hm_last_error() returns a
 *     thread-local message for the last failing call on this thread (no exceptions cross
 *     the ABI; the reference reports the same conditions as Python exceptions);
 *   - the caller owns all memory; pointers are DEVICE pointers unless marked [host];
 *     nothing is retained after the call returns; workspace is passed in explicitly;
 *   - `stream` is a hipStream_t (as void*); kernels are launched on it asynchronously and
 *     the functions never synchronise;  NULL means the HIP default stream;
 *   - all tensors are fp32, contiguous, row-major unless a stride argument says otherwise;
 *   - functions are re-entrant; the only mutable global is the error string.
 */
#ifndef HASHMOD_H
#define HASHMOD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define HM_API __attribute__((visibility("default")))
#else
#define HM_API
#endif

#define HM_MAX_LEVELS 32
#define HM_MAX_LAYERS 16

/* frac_mode */
#define HM_FRAC_REFERENCE 0 /* reference behaviour: xf = x - x.float() == 0 (hashGridEmbedding.py:86) */
#define HM_FRAC_TRILINEAR 1 /* build-defined opt-in: floor + fractional weights (NOT a parity mode)    */

#define HM_OK 0
#define HM_ERR_INVALID (-1) /* bad argument (reference: ValueError / assert)      */
#define HM_ERR_HIP (-2)     /* HIP runtime / launch failure (reference: RuntimeError) */

HM_API int hm_version(void);
HM_API const char *hm_last_error(void);
/* number of HIP devices visible, or <0; never initialises a context */
HM_API int hm_device_count(void);

/* ---- level table ------------------------------------------------------------------------
 * Replaces the per-level bookkeeping of MultiResHashGridMLP.__init__
 * (model/embeddings/hashGridEmbedding.py:106-147): res[l], rows[l] = min(res^3, 2^T) and the
 * row offset of level l inside the fused [sum(rows), F] table.  The arrays are [host] and are
 * computed by the caller in double precision exactly as the reference does; the library never
 * recomputes them.  n_features is F (max_points_per_level).                                   */
typedef struct hm_grid_desc hm_grid_desc;
HM_API int hm_grid_desc_create(int n_levels, int n_features, const int32_t *res, const uint32_t *rows,
                        const uint64_t *row_off /* [n_levels+1] */, hm_grid_desc **out);
HM_API void hm_grid_desc_destroy(hm_grid_desc *desc);
HM_API int hm_grid_embed_dim(const hm_grid_desc *desc); /* 3 + 2L + L*F (hashGridEmbedding.py:143-145) */

/* ---- hash indices -----------------------------------------------------------------------
 * Replaces hash_func + the index half of _HashGridMLP.forward
 * (hashGridEmbedding.py:32-40, 84-98) for one level: xi = trunc(x*res) and the 8 corner
 * row ids in bin_mask order.  xi_out [n,3] int32 (may be NULL), ids_out [n,8] uint32.        */
HM_API int hm_corner_ids(const hm_grid_desc *desc, int level, const float *x, int64_t n, int32_t *xi_out,
                  uint32_t *ids_out, void *stream);

/* ---- diagnostic: PMC calibration of 8-byte row gathers ---------------------------------------------
 * Not part of the reference's interface.  Groups of `group` consecutive lanes read 8-byte rows of one pseudo-random
 * 128-B block of `table` (table_bytes >> Infinity Cache), lane g at byte offset g*stride_bytes: known bytes and
 * known 32/64/128-B units per block, against which FETCH_SIZE / TCC_EA0_RDREQ are read (profiles/r02_gather_calib.json).
 * out [n] receives a checksum per lane.                                                                  */
HM_API int hm_diag_gather_calib(const float *table, int64_t table_bytes, int64_t n, int group, int stride_bytes,
                                float *out, void *stream);

/* ---- diagnostic: what a stream of exact-fp32 MFMAs sustains --------------------------------------------
 * Not part of the reference's interface.  `workgroups` workgroups of 8 waves (two per SIMD, as the fused SDF kernel)
 * issue `iters` x 16 v_mfma_f32_32x32x2_f32 each on four independent accumulators, operands in registers, no memory
 * traffic: iters * 16 * 4096 flop per wave.  The rate it reaches (bench.py times the call) is the ceiling of the
 * matrix pipe under this instruction - below the nominal 256 flop / clk / CU x 2.4 GHz because the clock drops under
 * the load and an MFMA occupies the pipe for more than its 64 cycles.  out [workgroups * 512] receives checksums.   */
HM_API int hm_diag_mfma_f32_stream(int workgroups, int iters, float *out, void *stream);

/* ---- encoder forward --------------------------------------------------------------------
 * Replaces MultiResHashGridMLP.forward (hashGridEmbedding.py:150-155) including
 * FourierFeature.forward (frequency_enc.py:63-67):
 *   out[i] = [ x(3) | sin(2*pi*x@B)(L) | cos(2*pi*x@B)(L) | level features (L*F) ].
 * x [n,3]; table [sum(rows),F]; B_fourier [3,L]; out rows are out_stride floats apart
 * (out_stride >= E).  All 8 corners of every level are gathered in both frac modes.
 * B_fourier == NULL: only the L*F hash-feature columns are produced, out[i*out_stride + l*F + f]
 * (the torch.cat([level(x) ...]) half of hashGridEmbedding.py:153).                            */
HM_API int hm_encode_fwd(const hm_grid_desc *desc, const float *x, int64_t n, const float *table,
                  const float *B_fourier, float *out, int64_t out_stride, int frac_mode, void *stream);

/* Same operator with a caller-owned scratch buffer of hm_encode_workspace_bytes(desc, n) bytes.  Big launches
 * (n >= 131072 over tables larger than 8 MiB) then bucket the points by z first and gather in that order: the
 * reference hash puts every (x, y) corner of one z-plane into one 16-KB window of a level's table, so z-ordered
 * points share their table lines on every level (out[i] is still the embedding of x[i]; only the order of the
 * work changes).  Without a workspace (or for small launches) the call is identical to hm_encode_fwd.
 * Padded rows: with out_stride a multiple of 4 floats >= ceil(E/4)*4 (272 bytes at E = 67) and a 16-byte aligned `out`
 * every row leaves the z-ordered kernel as ONE dwordx4 store instruction (the pad floats of a row are written as zeros);
 * any other stride takes the dword path.                                                                          */
HM_API int64_t hm_encode_workspace_bytes(const hm_grid_desc *desc, int64_t n);
HM_API int hm_encode_fwd_ws(const hm_grid_desc *desc, const float *x, int64_t n, const float *table,
                     const float *B_fourier, float *out, int64_t out_stride, int frac_mode, void *workspace,
                     int64_t workspace_bytes, void *stream);

/* ---- encoder backward (table) -----------------------------------------------------------
 * Replaces the embedding_dense_backward that autograd runs for nn.Embedding in
 * _HashGridMLP.forward (hashGridEmbedding.py:99-102): d_table[row] += w * d_out.
 * d_feat points at the hash-feature columns of the upstream gradient: d_feat[i*d_feat_stride + l*F + f]
 * (for a full [n,E] gradient pass d_out + 3 + 2L and stride E);
 * d_table [sum(rows),F] is ACCUMULATED into (caller zeroes it, like the reference's
 * optimizer.zero_grad()).  fp32 atomics: the sum is order-dependent in the last bits.         */
HM_API int hm_encode_bwd_table(const hm_grid_desc *desc, const float *x, int64_t n, const float *d_feat,
                        int64_t d_feat_stride, float *d_table, int frac_mode, void *stream);

/* Same gradient with a caller-owned scratch buffer of hm_encode_bwd_workspace_bytes(desc, n) bytes.  Big launches
 * (F = 2, n >= 131072, tables > 8 MiB) bucket the points by z, lay x / d_feat out in that order and let one workgroup
 * per (z-slab, level) accumulate its contributions in LDS copies of the few 2^11-row blocks it touches before adding
 * them to d_table with dense, coalesced atomics; otherwise identical to hm_encode_bwd_table.                     */
HM_API int64_t hm_encode_bwd_workspace_bytes(const hm_grid_desc *desc, int64_t n);
HM_API int hm_encode_bwd_table_ws(const hm_grid_desc *desc, const float *x, int64_t n, const float *d_feat,
                                  int64_t d_feat_stride, float *d_table, int frac_mode, void *workspace,
                                  int64_t workspace_bytes, void *stream);

/* Deterministic form of the same gradient (no atomics).  hm_encode_rows lists, for every (point, level[, corner]),
 * the destination row in the fused table (keys_out [n*L*C] int32, C = 1 in reference frac mode - only corner 0 carries
 * weight - and 8 in trilinear mode, where weights_out [n*L*C] receives the interpolation weights).  The caller sorts
 * the keys with ANY stable sort (perm = the sorting permutation, int64; hm_sort_pairs_i32 below is the library's own);
 * hm_encode_bwd_table_sorted then sums each run
 * of equal keys in sorted order in one thread and adds it to d_table with a plain read-modify-write.  Bitwise
 * reproducible for a given contribution order (torch's embedding_dense_backward is deterministic on the CPU path the
 * reference oracle runs; the atomic kernel above is the fast default).                                                */
HM_API int hm_encode_rows(const hm_grid_desc *desc, const float *x, int64_t n, int frac_mode, int32_t *keys_out,
                          float *weights_out, void *stream);
HM_API int hm_encode_bwd_table_sorted(const hm_grid_desc *desc, const int32_t *keys_sorted, const int64_t *perm,
                                      int64_t n_keys, int corners, const float *d_feat, int64_t d_feat_stride,
                                      const float *weights, float *d_table, void *stream);

/* Stable sort of non-negative int32 keys (< 2^key_bits) with the sorting permutation - the library's own LSD radix sort
 * (8-bit digits, ceil(key_bits/8) passes of three kernel launches; csrc/hm_sort.hip) for the pair
 * hm_encode_rows -> hm_encode_bwd_table_sorted: keys_sorted[i] = keys[perm[i]], equal keys keep their input order.
 * keys and keys_sorted must not alias; workspace: hm_sort_workspace_bytes(n) bytes.  Sync-free, graph-capturable.   */
HM_API int64_t hm_sort_workspace_bytes(int64_t n);
HM_API int hm_sort_pairs_i32(const int32_t *keys, int64_t n, int key_bits, int32_t *keys_sorted, int64_t *perm,
                             void *workspace, int64_t workspace_bytes, void *stream);


/* ---- encoder input gradient (frac_mode = HM_FRAC_TRILINEAR only) ---------------------------------------------
 * In the reference d(hash features)/dx is identically zero (xf = x - x.float() == 0, hashGridEmbedding.py:86), so
 * autograd never runs anything here; these three entry points make the opt-in trilinear mode trainable under IDR's
 * eikonal / normal terms, where ImplicitNetwork.gradient differentiates the embedding with create_graph=True
 * (implicit_differentiable_renderer.py:116-127).  J_i = d feat[i,:] / d x[i,:]  [L*F, 3], exact inside a voxel.
 *   hm_encode_bwd_input      a == NULL: gx[i,:] = J_i^T d_feat[i,:]            (the embedding's backward w.r.t. x)
 *                            a != NULL: gx[i,:] = d/dx ( a[i,:] . J_i^T d_feat[i,:] )   (its second-order term)
 *   hm_encode_jvp            out[i,:] = J_i a[i,:]                              (backward of gx w.r.t. d_feat)
 *   hm_encode_bwd_table_jvp  d_table += d/dT ( sum_i a[i,:] . J_i^T d_feat[i,:] )  (fp32 atomics, accumulates)
 * x, a, gx [n,3]; d_feat / out rows of L*F floats with the given row stride.                                        */
HM_API int hm_encode_bwd_input(const hm_grid_desc *desc, const float *x, int64_t n, const float *table,
                               const float *d_feat, int64_t d_feat_stride, const float *a, float *gx, void *stream);
HM_API int hm_encode_jvp(const hm_grid_desc *desc, const float *x, int64_t n, const float *table, const float *a,
                         float *out, int64_t out_stride, void *stream);
HM_API int hm_encode_bwd_table_jvp(const hm_grid_desc *desc, const float *x, int64_t n, const float *a,
                                   const float *d_feat, int64_t d_feat_stride, float *d_table, void *stream);

/* ---- embedding row: input gradient of the Fourier-feature columns -------------------------------------------------
 * MultiResHashGridMLP.forward returns [x | sin(a) | cos(a) | level features] with a = 2 pi x B (hashGridEmbedding.py:
 * 150-155, frequency_enc.py:63-67).  In the reference autograd differentiates that expression w.r.t. x with
 * create_graph=True (ImplicitNetwork.gradient, implicit_differentiable_renderer.py:116-127: ~10 elementwise kernels
 * and a K=3 matmul per pass) and once more in loss.backward(); the hash features contribute nothing (:86).
 *   hm_fourier_bwd_input      gx[i,:] = d_row[i,0:3] + 2 pi sum_c B[:,c] (cos_c d_sin_c - sin_c d_cos_c)
 *   hm_fourier_bwd_input_bwd  given gg [n,3]:  dd_row = d(gg . gx)/d(d_row)  ([n,width], hash columns zero; may be NULL)
 *                                              d_x    = d(gg . gx)/dx        ([n,3]; may be NULL)
 * B_fourier [3, n_channels]; d_row rows [x(3) | sin(n_channels) | cos(n_channels) | ...] with the given stride.     */
HM_API int hm_fourier_bwd_input(const float *x, int64_t n, const float *B_fourier, int n_channels, const float *d_row,
                                int64_t d_row_stride, float *gx, void *stream);
HM_API int hm_fourier_bwd_input_bwd(const float *x, int64_t n, const float *B_fourier, int n_channels,
                                    const float *d_row, int64_t d_row_stride, const float *gg, float *d_x,
                                    float *dd_row, int64_t dd_row_stride, int width, void *stream);

/* ---- fused SDF network forward (no grad) ---------------------------------------------------
 * Replaces ImplicitNetwork.forward evaluated under torch.no_grad()
 * (model/implicit_differentiable_renderer.py:89-113 + density_net.py:20-30), i.e. the `sdf`
 * callable of RayTracing.forward (model/ray_tracing.py:26-95): embed -> L linear layers with
 * Softplus(beta=100) -> column 0 through tanh(s / (2 + LaplaceDensity(s))).
 *
 * The weight-norm fold W = g*v/||v|| (nn.utils.weight_norm, dim=0) is done by the caller; the
 * library takes each layer's folded matrix in a packed MFMA operand image:
 *   K space of a layer = its input segments back to back, each zero-padded to a multiple of 8:
 *     seg_src 1 = the embedding (E -> ceil(E/8)*8 slots), seg_src 0 = the previous layer's output;
 *     the skip layer (cat[x, emb]/sqrt(2), :99-100) lists {previous output, embedding}, and the
 *     layer BEFORE it sets post_div_sqrt2 (the embedding half is rescaled by the kernel);
 *   rows are zero-padded to n_tiles*32;  n_oct = seg_octets[0] + seg_octets[1];
 *   w_packed[((u*n_oct + g)*64 + l)*4 + s] = W[32u + (l&31)][8g + 4(l>>5) + s]
 *     for tile u < n_tiles, octet g < n_oct, lane l < 64, s < 4   (device pointer, 16-B aligned);
 *   bias: device pointer, n_tiles*32 floats, zero padded, 16-B aligned.
 * hm_mlp_desc itself is a [host] struct.                                                        */
typedef struct hm_mlp_layer {
    const float *w_packed;
    const float *bias;
    int32_t out_dim;        /* true number of output features            */
    int32_t n_tiles;        /* ceil(out_dim/32), at most 16              */
    int32_t seg_octets[2];  /* K octets per input segment (second may be 0) */
    int32_t seg_src[2];     /* 0 previous layer output, 1 embedding      */
    int32_t activation;     /* 1: Softplus(beta=100, threshold=20), 0: none */
    int32_t post_div_sqrt2; /* 1: outputs are divided by sqrt(2) (feeds the skip concat) */
    /* optional second image for the 16-point-tile kernel (small batches); NULL = not provided.
     * Same K space but every segment zero-padded to a multiple of 16; nb = seg_blocks16[0]+[1];
     * w_packed_m16[((u*nb + t)*64 + l)*4 + e] = W[16u + (l&15)][16t + 4(l>>4) + e],  u < 2*n_tiles. */
    const float *w_packed_m16;
    int32_t seg_blocks16[2];
    /* optional bf16 image for hm_sdf_fwd_bf16 (NULL = not provided): same K space as the 16-k image,
     * w_packed_bf16[((u*nb + t)*64 + l)*8 + j] = bf16(W[32u + (l&31)][16t + 8(l>>5) + j]),  u < n_tiles (2-byte elements). */
    const void *w_packed_bf16;
    /* optional SPLIT image for hm_sdf_fwd_split (NULL = not provided): every weight as a pair (hi, lo) of 2-byte floats of
     * the kind hm_mlp_desc.split_kind names, c_w W ~= hi + lo (c_w = 1 for bf16, 2^8 for fp16), same K space as the 16-k
     * image:  w_packed_split[(((u*nb + t)*2 + part)*64 + l)*8 + j] = part(c_w c * W[32u + (l&31)][16t + 8(l>>5) + j]),
     * part 0 = hi, 1 = lo, c = the segment's scale given to hm_pack_mlp_layer_split.                                      */
    const void *w_packed_split;
} hm_mlp_layer;

#define HM_SPLIT_NONE (-1)
#define HM_SPLIT_BF16X2 0 /* hi, lo bf16: 16 significant bits per operand */
#define HM_SPLIT_F16X2 1  /* hi, lo fp16 (activations scaled by 2^4, weights by 2^8): 22 significant bits, |x| <= 4094 */

typedef struct hm_mlp_desc {
    int32_t n_layers;
    float beta; /* LaplaceDensity: |beta_param| + beta_min (density_net.py:28-30) */
    hm_mlp_layer layer[HM_MAX_LAYERS];
    int32_t split_kind; /* kind of the layers' w_packed_split images (HM_SPLIT_*), HM_SPLIT_NONE when absent */
} hm_mlp_desc;

/* Builds the operand images of one layer from its folded matrix W [out_dim, seg_width0 + seg_width1]
 * (row stride ldw) and bias: w_packed (n_tiles*n_oct*256 floats), w_packed_m16 (2*n_tiles*nb*256 floats),
 * bias_padded (n_tiles*32 floats); seg_width1 = 0 when the layer has one input segment.             */
HM_API int hm_pack_mlp_layer(const float *W, int64_t ldw, const float *bias, int out_dim, int seg_width0,
                             int seg_width1, float *w_packed, float *w_packed_m16, float *bias_padded,
                             void *stream);
/* the same for every layer of a network in ONE launch (the per-step re-pack); items is a [host] array of at most
 * HM_MAX_LAYERS entries with the arguments of hm_pack_mlp_layer                                                  */
typedef struct hm_pack_item {
    const float *W;
    const float *bias;
    float *w_packed, *w_packed_m16, *bias_padded;
    int64_t ldw;
    int32_t out_dim, seg_width0, seg_width1, pad_;
} hm_pack_item;
HM_API int hm_pack_mlp_layers(const hm_pack_item *items, int n_items, void *stream);

HM_API int hm_pack_mlp_layer_bf16(const float *W, int64_t ldw, int out_dim, int seg_width0, int seg_width1,
                                  void *w_packed_bf16, void *stream);

/* x [n,3] -> out.  out_cols == 1: only the clamped sdf, out[i*out_stride];  out_cols == last
 * layer's out_dim: the whole [sdf | feature vector] row.
 * tile_points: 64 (one 8-wave workgroup per CU), 16 (small batches),
 * 8 or 4 (<= 2048 / 1024 points: bound by the weight stream alone), 0 = choose by n (on the device when n_dev is given),
 * -1 = like 0 but ONLY for n <= 8192 (larger batches are left to another launch, e.g. hm_sdf_fwd_bf16 with run_min 8193).
 * HM_SDF_TILE64_QUARTER = the 64-point launch with quarter tiles enabled: a live count of at most 16 points per workgroup
 * runs tiles of <= 16 points on v_mfma_f32_16x16x4_f32 in the 64-point tile's accumulation order (the values of
 * tile_points = 64 bit for bit, in about two thirds of the time of its 32-point half tiles); larger counts run as with 64.
 * n_dev: optional DEVICE int32; when non-NULL the kernel evaluates min(n, *n_dev) points, so a
 *        caller that compacts work on the device needs no host synchronisation (n is the capacity).
 * max_workgroups <= 0: fill the chip once (persistent grid-stride over tiles).                    */
#define HM_SDF_TILE64_QUARTER 1664
HM_API int hm_sdf_fwd(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *x, int64_t n,
                      const float *table, const float *B_fourier, float *out, int64_t out_stride, int out_cols,
                      int frac_mode, int tile_points, const int32_t *n_dev, int max_workgroups, void *stream);

/* bf16 variant (BASELINE configs[4]), sdf-only output out[i*out_stride]: hidden-layer weights and activations in bf16
 * on v_mfma_f32_32x32x16_bf16 (fp32 accumulate); the embedding, every product that consumes it (layer 0, the skip
 * segment), bias / Softplus, the last layer and the clamp stay fp32.  Meant for the tracer's coarse scans (sign-change
 * sampler, closest approach); runs only when the live point count is >= run_min (pair it with hm_sdf_fwd(tile_points
 * = -1) for the small counts).  Needs w_packed, bias and w_packed_bf16 in every layer.  hm_sdf_fwd_emb_bf16: the same
 * on precomputed embedding rows.  No reference behaviour exists for reduced precision: the error against
 * hm_sdf_fwd and the loss-curve criterion are measured in tests/test_bf16_gpu.py.                                      */
HM_API int hm_sdf_fwd_bf16(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *x, int64_t n,
                           const float *table, const float *B_fourier, float *out, int64_t out_stride, int frac_mode,
                           const int32_t *n_dev, int64_t run_min, void *stream);
HM_API int hm_sdf_fwd_emb_bf16(const hm_mlp_desc *mlp, const float *emb, int64_t emb_stride, int emb_width, int64_t n,
                               float *out, int64_t out_stride, const int32_t *n_dev, int64_t run_min, void *stream);

/* Split-operand variant, sdf-only output out[i*out_stride] (csrc/hm_sdf_split.hip): EVERY operand of every matrix product
 * (weights, hidden activations, embedding) is a (hi, lo) pair of 16-bit floats and W x is evaluated as
 * Wh xh + Wh xl + Wl xh on v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulation - three MFMAs at 16x the fp32
 * MFMA rate.  HM_SPLIT_BF16X2: relative product error 2^-16 (the "bf16" configuration, BASELINE configs[4], with 250x the
 * accuracy of plain bf16 operands); HM_SPLIT_F16X2: <= 3 * 2^-22, below the rounding noise of an fp32 accumulation over
 * K = 512.  Bias, Softplus, the last layer and the clamp are fp32.  Runs only when the live point count is >= run_min
 * (pair it with hm_sdf_fwd(tile_points = -1) for the small counts).  Needs w_packed, bias and w_packed_split in every
 * layer and mlp->split_kind.  hm_pack_mlp_layer_split builds one layer's split image (n_tiles*nb*1024 2-byte elements)
 * from the folded matrix; seg_scale0/1 multiply the two K segments (the skip layer's embedding segment carries the
 * 1/sqrt(2) of cat[x, emb]/sqrt(2), implicit_differentiable_renderer.py:99-100).  No reference behaviour exists for
 * these modes: tests/test_split_gpu.py measures them against hm_sdf_fwd and an fp64 evaluation.                        */
HM_API int hm_pack_mlp_layer_split(const float *W, int64_t ldw, int out_dim, int seg_width0, int seg_width1,
                                   float seg_scale0, float seg_scale1, int split_kind, void *w_packed_split,
                                   void *stream);
/* the same for every layer of a network in ONE launch (the per-step re-pack); items is a [host] array of at most
 * HM_MAX_LAYERS entries with the arguments of hm_pack_mlp_layer_split, all of the kind split_kind                 */
typedef struct hm_pack_split_item {
    const float *W;
    void *w_packed_split;
    int64_t ldw;
    int32_t out_dim, seg_width0, seg_width1;
    float seg_scale0, seg_scale1;
    int32_t pad_;
} hm_pack_split_item;
HM_API int hm_pack_mlp_layers_split(const hm_pack_split_item *items, int n_items, int split_kind, void *stream);
HM_API int hm_sdf_fwd_split(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *x, int64_t n,
                            const float *table, const float *B_fourier, float *out, int64_t out_stride, int frac_mode,
                            const int32_t *n_dev, int64_t run_min, void *stream);
HM_API int hm_sdf_fwd_emb_split(const hm_mlp_desc *mlp, const float *emb, int64_t emb_stride, int emb_width, int64_t n,
                                float *out, int64_t out_stride, const int32_t *n_dev, int64_t run_min, void *stream);

/* The same network evaluated on PRECOMPUTED embedding rows emb[i*emb_stride .. + emb_width) instead of encoding x in
 * the kernel: the SDF network on top of an embedder other than the plain hash grid (FourierFilterBanks via
 * hm_nffb_fwd; custom_embedder_decoder.py:147-164 + implicit_differentiable_renderer.py:96-113).  mlp's embedding
 * segments must span ceil(emb_width/8) octets (ceil(emb_width/16) 16-blocks).                                    */
HM_API int hm_sdf_fwd_emb(const hm_mlp_desc *mlp, const float *emb, int64_t emb_stride, int emb_width, int64_t n,
                          float *out, int64_t out_stride, int out_cols, int tile_points, const int32_t *n_dev,
                          int max_workgroups, void *stream);

/* Whether the fused SDF kernels of one family accept the network mlp over embedding rows of width emb_width, decided by
 * the host-side checks their launches make (descriptor, layer shapes, LDS tiles); host only, nothing is enqueued.
 *   HM_SDF_FP32:  hm_sdf_fwd / hm_sdf_fwd_emb at every tile size and the ray tracer's fp32 kernels;
 *   HM_SDF_BF16:  hm_sdf_fwd_bf16 / hm_sdf_fwd_emb_bf16;   HM_SDF_SPLIT: hm_sdf_fwd_split / hm_sdf_fwd_emb_split.
 * Returns 1 (accepted), 0 (refused: hm_last_error() says why) or -1 (bad argument).                              */
#define HM_SDF_FP32 0
#define HM_SDF_BF16 1
#define HM_SDF_SPLIT 2
HM_API int hm_sdf_net_fits(const hm_mlp_desc *mlp, int emb_width, int family);

/* Diagnostic: the dynamic LDS layout of one fused SDF tile body for the network mlp; host only.  tile_points 64, 16 or
 * 8 selects the HM_SDF_FP32 body (the 4-point tile uses the 8-point layout); the other families have one body and
 * ignore it.  regions[0..4] = byte offsets of the second activation region (image / lo plane; 0 where the
 * body has one), the embedding, its second region (== regions[1] where it has one), the raw points [points][4] and the
 * last layer's partial sums [parts][points]; regions[5] = the launch's dynamic LDS bytes.                          */
HM_API int hm_diag_sdf_lds(const hm_mlp_desc *mlp, int emb_width, int family, int tile_points, int32_t *regions);

/* ---- Fourier-filter-bank embedders ('FFB', 'StyleModNFFB') forward, no grad ------------------------------------
 * Replaces FourierFilterBanks.forward (model/embeddings/nffb3d.py:122-194, registry settings PositionalEncodingNET /
 * SIREN / has_out=False) with PositionalEncoding (frequency_enc.py:6-51), Sine (Sine.py:5-25) and StyleAttention
 * (style_Attention/styleMod.py:16-43) in ONE kernel:
 *   out[i] = [ u(3) | mean over the L grid levels of out_layer(e_l) (W = 8 + 8L) ],  u = (x + bound) / (2 bound).
 * desc: the embedder's own hash grid (n_levels == L in {6, 8}, F = 2); table / B_fourier as for hm_encode_fwd.
 * trunk_w[0] [W,3], trunk_w[1..L-2] [W,W], trunk_b[l] [W]: ff_lin{l};  out_w [W,W], out_b [W]: out_layer;
 * style_w / style_b: StyleAttention.linear_transform ([W,W], [W]) or both NULL for the plain 'FFB' embedder;
 * w0 = L^F - L (Sine); style_eps = 1e-5.  All DEVICE pointers, row-major fp32.  hm_nffb_desc itself is [host].
 * n_dev: optional device-side point count, as for hm_sdf_fwd.                                                   */
typedef struct hm_nffb_desc {
    int32_t n_levels;
    float bound, w0, style_eps;
    const float *trunk_w[HM_MAX_LEVELS];
    const float *trunk_b[HM_MAX_LEVELS];
    const float *out_w, *out_b;
    const float *style_w, *style_b;
} hm_nffb_desc;
HM_API int hm_nffb_fwd(const hm_grid_desc *desc, const hm_nffb_desc *nf, const float *x, int64_t n, const float *table,
                       const float *B_fourier, float *out, int64_t out_stride, int frac_mode, const int32_t *n_dev,
                       void *stream);

/* ---- ray / surface intersection search ------------------------------------------------------
 * Replaces RayTracing.forward and its helpers sphere_tracing / ray_sampler / secant /
 * minimal_sdf_points (model/ray_tracing.py:26-298) when the `sdf` callable is the network above:
 * bidirectional sphere tracing with line-search back-off, the n_steps sign-change sampler with
 * n_secant_steps secant iterations for rays that did not converge, and (training) the
 * closest-approach search for the mask-loss rays.  Same constructor values as the reference
 * class (ray_tracing.py:6-24); `training` = self.training.  One call enqueues the whole search
 * on `stream` without any host synchronisation (per-ray state machines + device-side compaction).
 *
 * cam_loc [B,3]; ray_dirs [N,3] (N = B*rays_per_image); object_mask [N] bytes;
 * t_sphere [N,2] / hit_mask [N]: near/far parameters and hit flags of the bounding sphere
 *   (utils/rend_util.py:141-162, computed by the caller);
 * sampler_fracs [n_steps] = linspace(0,1,n_steps) (ray_tracing.py:198);
 * steps_u [n_steps]: the U(0,1) fractions shared by all rays (ray_tracing.py:277; training only);
 * outputs: points [N,3], network_object_mask [N] bytes, dists [N];
 * stats_out (optional, 16 device int32): sampler rays, sampler points, secant rays, mask-loss rays,
 *   their points, any-iteration flag, total SDF evaluations, unfinished rays (must be 0), non-finite SDF
 *   values met by the search (must be 0), points of the big launch, lazy sampler: rays of the second pass, points of
 *   the first pass, points of the second pass, 3 reserved.                                          */
typedef struct hm_trace_cfg {
    float object_bounding_sphere;
    float sdf_threshold;
    double line_search_step;       /* back-off factors (1-step)/2^k are formed in double, like the reference */
    int32_t line_step_iters;       /* <= 3  */
    int32_t sphere_tracing_iters;  /* <= 15 */
    int32_t n_steps;
    int32_t n_secant_steps;
    int32_t training;
    int32_t coarse_bf16;           /* precision of the sampler / closest-approach scans: 0 exact fp32, 1 hm_sdf_fwd_bf16 (needs
                                      w_packed_bf16), 2 hm_sdf_fwd_split (needs w_packed_split; kind = mlp->split_kind),
                                      3 f16x2 behind an fp32 guard (needs the f16x2 w_packed_split; hash-grid networks):
                                      the rows are evaluated as in mode 2, the samples whose approximate value cannot
                                      settle what the search reads from a row (sign pattern up to the first negative
                                      sample, its bracket, the arg-min) are re-evaluated by the exact-fp32 kernel and
                                      written back before the rows are reduced - every output and counter is that of
                                      mode 0, bit for bit (hm_trace.hip: guard_select_sampler_kernel).  Statistics slot 14
                                      = samples re-evaluated, 15 = float bits of the largest |approximate - exact| met;
                                      above tau / 4 a sticky word in the workspace makes this and later calls re-evaluate
                                      every sample (hm_trace_guard_clear resets it).  HM_TRACE_GUARD_NOISE = f | nan:K
                                      (tests) perturbs the approximate values by up to f * tau / makes every K-th NaN, +Inf;
                                      sphere tracing and the secant refinement stay on the exact-fp32 kernels */
    int32_t sampler_head;          /* lazy sampler.  ray_sampler (ray_tracing.py:189-249) evaluates n_steps samples per
                                      unconverged ray but reads only those up to the FIRST negative one (:212-218, and
                                      its predecessor for the secant bracket, :238-243) unless the ray falls back to the
                                      minimal sample (:221-226).  h = sampler_head in [1, n_steps-2]: a first pass
                                      evaluates samples 0..h-1 and n_steps-1; rays with a negative head sample inside
                                      the object mask are finished, the others get samples h..n_steps-2 in a second
                                      pass.  Outputs are bit-identical to the single pass (0 / out of range).       */
} hm_trace_cfg;

HM_API int64_t hm_trace_workspace_bytes(int64_t n_rays, const hm_trace_cfg *cfg);
/* The first 256 bytes of a tracer workspace outlive the calls (the guard's sticky word): zero them once after allocating
 * the workspace, and to re-arm a tripped guard.  hm_trace_guard_tolerances: the guard width tau and the trip threshold. */
HM_API int hm_trace_guard_clear(void *workspace, int64_t workspace_bytes, void *stream);
HM_API int hm_trace_guard_tolerances(float *tau, float *tau_trip);
/* Diagnostic, host only: which split tiles of the closest-approach scan (n_scan points, 64 per tile, none at <= 8192
 * points) each launch of the guarded search owns - the rule the kernels evaluate from the device counters
 * (csrc/hm_scan_pool.h).  first[k], quota[k], k = 0, 1, 2: the refine-scan launch of the sampler's first pass (list of
 * n_ref1 points), of the lazy sampler's second pass (n_ref2 points; two_x = 0: no such launch) and the secant launch.
 * grid_x: workgroups of the refine-scan launches; n_sec_bound: rays handed to the sampler (the bound of the secant rays);
 * chain_tiles: tiles one workgroup finishes under the whole secant chain, -1 = derived from n_iters.                 */
HM_API int hm_trace_scan_pool_plan(int64_t n_scan, int64_t n_ref1, int64_t n_ref2, int two_x, int grid_x,
                                   int64_t n_sec_bound, int n_iters, int64_t chain_tiles, int64_t *first, int64_t *quota);
/* Diagnostic, host only: the launch sequence hm_trace_forward (has_nffb = 0) / hm_trace_forward_nffb (1) would enqueue
 * for n_rays rays - the plan the call itself computes (csrc/hm_trace.hip: trace_plan), with the HM_TRACE_* environment
 * switches read as a call reads them.  tests/test_trace_plan_cpu.py pins the decision table.
 *   sequence        how the sampler's rows and the closest-approach rows are evaluated:
 *     JOINT           one coarse launch over both point sets (any coarse_bf16 but 3)
 *     FILL            exact fp32: the closest-approach scan completes the sampler launches' last rounds and runs beside
 *                     the secant chain
 *     GUARD_SERIAL    guarded: every launch on its own, one refinement list per sampler pass
 *     GUARD_COSCHED   guarded: the sampler's refinement beside the whole closest-approach scan, that of the
 *                     closest-approach rows beside the secant chain
 *     GUARD_POOLED    guarded: the closest-approach scan shared out between the refinement launches and the chain's
 *   secant          none; inside the sequence's own launches; all iterations as one persistent launch (scan_rule: with
 *                   the tile rule of the scan-secant launch); an (SDF launch, update launch) pair per iteration          */
enum { HM_TRACE_SEQ_JOINT = 0, HM_TRACE_SEQ_FILL = 1, HM_TRACE_SEQ_GUARD_SERIAL = 2, HM_TRACE_SEQ_GUARD_COSCHED = 3,
       HM_TRACE_SEQ_GUARD_POOLED = 4 };
enum { HM_TRACE_SECANT_NONE = 0, HM_TRACE_SECANT_IN_SEQUENCE = 1, HM_TRACE_SECANT_PERSISTENT = 2,
       HM_TRACE_SECANT_PER_ITERATION = 3 };
typedef struct hm_trace_plan_info {
    int32_t sequence;         /* HM_TRACE_SEQ_*                                                                         */
    int32_t sel_own;          /* the closest-approach rows are evaluated by their own count, in a region of their own   */
    int32_t head;             /* lazy sampler: samples of the first pass in front of the last one (0: single pass)      */
    int32_t per_ray, c_first; /* first pass: samples per ray, and the statistics counter that receives its points       */
    int32_t k_tail;           /* pooled: secant rounds behind the cut of the chain (0: the chain is one launch)         */
    int32_t c_ref2;           /* pooled: counter of the second refine-scan launch's list (-1: there is none)            */
    int32_t march_tail;       /* the march hands over to the persistent kernel ...                                      */
    int32_t march_launched;   /* ... after this many (SDF launch, update launch) rounds ...                             */
    int32_t march_rounds;     /* ... of the search's 1 + sphere_tracing_iters * (1 + line_step_iters)                   */
    int32_t secant;           /* HM_TRACE_SECANT_*                                                                      */
    int32_t scan_rule;        /* persistent secant: tiles by the rule of the scan-secant launch                         */
    int32_t noise_nan;        /* HM_TRACE_GUARD_NOISE=nan:K (guarded sequences only)                                    */
    float noise_amp;          /* HM_TRACE_GUARD_NOISE=f: f * tau (guarded sequences only)                               */
    int64_t chain_tiles;      /* pooled: split tiles one workgroup finishes under the secant chain                      */
    int64_t guard_min;        /* guarded: launches of fewer live points were exact already and mark nothing             */
} hm_trace_plan_info;
HM_API int hm_diag_trace_plan(int64_t n_rays, const hm_trace_cfg *cfg, int tile_points, int has_nffb,
                              hm_trace_plan_info *info);
HM_API int hm_trace_forward(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *table,
                            const float *B_fourier, int frac_mode, int tile_points, const hm_trace_cfg *cfg,
                            const float *cam_loc, const float *ray_dirs, const uint8_t *object_mask,
                            const float *t_sphere, const uint8_t *hit_mask, int64_t n_rays, int64_t rays_per_image,
                            const float *sampler_fracs, const float *steps_u, float *out_points,
                            uint8_t *out_net_mask, float *out_dists, void *workspace, int64_t workspace_bytes,
                            int32_t *stats_out, void *stream);

/* The same search with the SDF network on a Fourier-filter-bank embedder (hm_nffb_fwd + hm_sdf_fwd_emb per round);
 * desc / table / B_fourier are the embedder's own hash grid; workspace of hm_trace_workspace_bytes_nffb() bytes.     */
HM_API int64_t hm_trace_workspace_bytes_nffb(int64_t n_rays, const hm_trace_cfg *cfg, int n_levels);
HM_API int hm_trace_forward_nffb(const hm_grid_desc *desc, const hm_nffb_desc *nffb, const hm_mlp_desc *mlp,
                                 const float *table, const float *B_fourier, int frac_mode, int tile_points,
                                 const hm_trace_cfg *cfg, const float *cam_loc, const float *ray_dirs,
                                 const uint8_t *object_mask, const float *t_sphere, const uint8_t *hit_mask,
                                 int64_t n_rays, int64_t rays_per_image, const float *sampler_fracs,
                                 const float *steps_u, float *out_points, uint8_t *out_net_mask, float *out_dists,
                                 void *workspace, int64_t workspace_bytes, int32_t *stats_out, void *stream);

/* ---- exact-fp32 GEMM (grad-enabled MLP path) ------------------------------------------------
 * Replaces the nn.Linear matmuls autograd runs for the SDF and rendering MLPs when gradients are
 * needed (implicit_differentiable_renderer.py:102,116-128,211-221): forward X*W^T + b, backward
 * dY*W and dY^T*X, and the same shapes again under create_graph=True.
 *   C[M,N] (+)= op(A)[M,K] * op(B)[K,N] (+ bias[N]);  row-major, leading dimensions in floats;
 *   transA: A is stored [K,M];  transB: B is stored [N,K];  bias may be NULL;
 *   accumulate != 0 adds into C (fp32 atomics), otherwise C is overwritten.
 *   K = 0 gives C = bias (or 0), C += bias with accumulate; A and B are not read (they may be NULL).  */
HM_API int hm_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                       const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int accumulate,
                       void *stream);

/* GEMM with a fused elementwise epilogue on v = (acc + bias) * scale - the Softplus passes that follow (forward)
 * or consume (backward / double backward) every nn.Linear of the SDF MLP, done on the accumulator registers
 * instead of as separate passes over [points, 512] tensors.  s1 / s2 = first / second derivative of
 * nn.Softplus(beta, threshold) at z.  C may be NULL (raw product not stored).  No split-K, no accumulate.
 *   HM_EPI_NONE      C = v
 *   HM_EPI_SOFTPLUS  C = v;  out1 = softplus(v)                                   (forward: z and h in one pass)
 *   HM_EPI_S1MUL     C = v;  out1[:, :nz] = v[:, :nz] * s1(z) (+ g)               (gradient sweeps: u = v * s1(z))
 *   HM_EPI_ADJOINT   out1 = v * s1(z);  out2 = v * g * s2(z);  out3 = g * s1(z)    (adjoint of u = g * s1(z); out3 optional)
 *   HM_EPI_RELU      C = v;  out1 = max(v, 0)                                     (rendering MLP forward, :214-219)
 *   HM_EPI_RELUMASK  C = v;  out1[:, :nz] = (z > 0 ? v : 0) (+ g)                (its backward; z = the layer's ReLU output) */
enum { HM_EPI_NONE = 0, HM_EPI_SOFTPLUS = 1, HM_EPI_S1MUL = 2, HM_EPI_ADJOINT = 3, HM_EPI_RELU = 4, HM_EPI_RELUMASK = 5 };
typedef struct hm_gemm_epilogue {
    int32_t mode;
    int32_t nz;               /* S1MUL: columns [0, nz) get the s1 product (z has nz columns)          */
    float scale, beta, threshold;
    const float *z;  int64_t ldz;
    const float *g;  int64_t ldg;  /* ADJOINT: second factor;  S1MUL: optional addend (may be NULL)    */
    float *out1;     int64_t ld1;
    float *out2;     int64_t ld2;
    float *out3;     int64_t ld3;
} hm_gemm_epilogue;
HM_API int hm_gemm_f32_ep(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                          const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc,
                          const hm_gemm_epilogue *ep, void *stream);

/* ---- diagnostic: the kernel hm_gemm_f32 / _ep / _det would launch ------------------------------------------------
 * Not part of the reference's interface.  Host only, reads no memory (A and B are used for their alignment alone, so
 * any pointer values will do): the same plan the launch uses - the kernel family, the K tail of the pipelined kernel,
 * the 16-byte operand loads of the generic / big kernel, the split-K decomposition and, with deterministic != 0,
 * whether the k-part kernels and their reduce launch run.  kernel = HM_GEMM_KERNEL_NONE (all zeros) when M or N is 0.  */
enum { HM_GEMM_KERNEL_NONE = 0, HM_GEMM_KERNEL_GENERIC = 1, HM_GEMM_KERNEL_BIG = 2, HM_GEMM_KERNEL_PIPE64 = 3,
       HM_GEMM_KERNEL_PIPE96 = 4 };
typedef struct hm_gemm_plan_info {
    int32_t kernel;           /* HM_GEMM_KERNEL_*: generic 64x64, big 128x128, pipelined 64x64 or 96x64        */
    int32_t k_tail;           /* pipelined: K is no multiple of 128 and runs to the next one (k >= K read as 0)  */
    int32_t vec_a, vec_b;     /* generic / big: operand fetched with 16-byte loads                              */
    int32_t part;             /* deterministic split-K: k-part slabs + reduce launch instead of atomics          */
    int32_t pad_;
    int64_t split, k_chunk;   /* workgroups along K and the K range of one                                       */
} hm_gemm_plan_info;
HM_API int hm_diag_gemm_plan(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                             const float *B, int64_t ldb, int has_epilogue, int deterministic, hm_gemm_plan_info *info);

/* ---- fused activation passes of the grad-enabled MLP path ------------------------------------
 * nn.Softplus(beta, threshold) (implicit_differentiable_renderer.py:84) over n contiguous floats:
 *   order 0: out0 = softplus(z)
 *   order 1: out0 = gy * s1(z)                         (its backward; s1 = d softplus / dz)
 *   order 2: out0 = gg * s1(z),  out1 = gg * gy * s2(z)  (backward of order 1 w.r.t. gy and z; the
 *            double backward autograd needs for ImplicitNetwork.gradient(create_graph=True), :116-128)
 * With every pointer 16-byte aligned the pass moves float4s; any other alignment (a contiguous view that
 * starts inside its storage) takes a scalar pass with the same arithmetic, so the results are bit-identical. */
HM_API int hm_softplus(int order, const float *z, const float *gy, const float *gg, float *out0, float *out1,
                       int64_t n, float beta, float threshold, void *stream);

/* The same three passes for the two elementwise pieces of the Fourier-filter-bank embedders (BASELINE configs 3 / 5):
 *   hm_sine    SIREN activation y = sin(w0 x) (embeddings/Sine.py:10-12) over n floats:
 *                order 0: out0 = sin(w0 x);  order 1: out0 = gy w0 cos(w0 x);
 *                order 2: out0 = gg w0 cos(w0 x) (d/d gy),  out1 = -gg gy w0^2 sin(w0 x) (d/d x)
 *   hm_posenc  NeRF positional encoding of rows c [n, dim] (frequency_enc.py:6-51 with include_input, sin / cos,
 *              `freqs` = HOST array of n_freq bands): row = [c | c | sin(f0 c) | cos(f0 c) | sin(f1 c) | ...],
 *              width W = 2 dim + 2 n_freq dim:
 *                order 0: out0 [n, W] = row;   order 1: out0 [n, dim] = (d row / d c)^T g  (g [n, W]);
 *                order 2 (given gg [n, dim] contiguous): out0 [n, W] = d(gg . order1)/d g,  out1 [n, dim] = d(gg . order1)/d c */
/*   hm_weight_norm_multi  W = g * v / ||v||_row (nn.utils.weight_norm with dim = 0, as every Linear of the SDF and
 *              rendering networks is wrapped, implicit_differentiable_renderer.py:95-97,205-206) for SEVERAL layers in
 *              one launch (backward == 0: w and norm are written) and its backward (backward != 0: grad_v, grad_g from
 *              grad_w and the stored norm); arithmetic of ATen's weight_norm first-dim kernels.  `layers` is a HOST array. */
typedef struct hm_wn_layer {
    const float *v;        /* [rows, cols] */
    const float *g;        /* [rows]       */
    float *w;              /* [rows, cols] forward output                  */
    float *norm;           /* [rows]       forward output / backward input */
    const float *grad_w;   /* [rows, cols] backward input                  */
    float *grad_v;         /* [rows, cols] backward output                 */
    float *grad_g;         /* [rows]       backward output                 */
    int32_t rows, cols;
} hm_wn_layer;
HM_API int hm_weight_norm_multi(int backward, int n_layers, const hm_wn_layer *layers, void *stream);

/*   hm_rownorm  (y - mean) / sqrt(var + eps) per row of a contiguous [rows, width] tensor, biased variance - the
 *              nn.InstanceNorm1d call of StyleAttention on a 2-D tensor (style_Attention/styleMod.py:41-43):
 *                order 0: out0 = normalised rows;  order 1: out0 = its backward applied to g;
 *                order 2 (given gg): out0 = d(gg . order1)/d g,  out1 = d(gg . order1)/d y                              */
HM_API int hm_rownorm(int order, const float *y, const float *g, const float *gg, float *out0, float *out1, int64_t rows,
                      int width, float eps, void *stream);
HM_API int hm_sine(int order, const float *x, const float *gy, const float *gg, float *out0, float *out1, int64_t n,
                   float w0, void *stream);
HM_API int hm_posenc(int order, const float *freqs, int n_freq, int dim, const float *c, int64_t c_stride,
                     const float *g, int64_t g_stride, const float *gg, float *out0, int64_t out0_stride, float *out1,
                     int64_t n, void *stream);

/* Soft clamp of the SDF column of the last layer's output zL [n, cols] (contiguous) and its backward
 * (implicit_differentiable_renderer.py:112, density_net.py:20-30; the density is evaluated without gradient):
 *   backward == 0:  out = zL with column 0 -> sdf = tanh(s / (2 + rho(s)));  sdf, denom = 2 + rho, c = d sdf/d s [n]
 *   backward != 0:  out = d_out with column 0 -> d_out[:,0] * c (+ cb * (-2 sdf c / denom) when cb != NULL);
 *                   sdf, c, denom are inputs here.                                                       */
HM_API int hm_sdf_head(int backward, const float *in, int64_t n, int64_t cols, float beta_rho, float *out, float *sdf,
                       float *c, float *denom, const float *cb, void *stream);

/* out[n] = sum over rows of x[M,N] (row stride ld) - the bias gradient of an nn.Linear.          */
HM_API int hm_colsum(const float *x, int64_t M, int64_t N, int64_t ld, float *out, void *stream);
/* same, added into out (no zeroing: the caller zeroes all its gradient buffers with one launch)  */
HM_API int hm_colsum_acc(const float *x, int64_t M, int64_t N, int64_t ld, float *out, void *stream);
/* out_i[n] += sum_m x_i[m, n] for a list of matrices in ONE launch (all bias gradients of one backward pass; the caller
 * zeroes the outputs).  items is a [host] array.                                                                 */
#define HM_COLSUM_MAX_ITEMS 16
typedef struct hm_colsum_item {
    const float *x;
    float *out;
    int64_t M, N, ld;
} hm_colsum_item;
HM_API int hm_colsum_acc_multi(const hm_colsum_item *items, int n_items, void *stream);

/* dst[r*ld_dst + c] = src[r*ld_src + c], r < rows, c < cols, as an ordinary kernel: the copies torch would issue as
 * hipMemcpyAsync (Tensor.copy_ / clone of contiguous tensors; the saved-activation stacking of the fused MLP-gradient
 * node, torch.cat in implicit_differentiable_renderer.py:99-100,280-284) become MEMCPY nodes of a captured HIP graph,
 * which this library keeps out of its captured training iteration (graph replay fault).            */
HM_API int hm_copy2d_f32(float *dst, int64_t ld_dst, const float *src, int64_t ld_src, int64_t rows, int64_t cols,
                         void *stream);

/* ---- IDRLoss: value and gradients in one launch (code/model/loss.py:4-70) --------------------------
 * terms[4] = {loss, rgb_loss, eikonal_loss, mask_loss};  d_rgb[n,3], d_sdf[n], d_grad[m,3] = d loss / d input.
 * rgb, rgb_gt [n,3]; sdf [n]; hit (network_object_mask), inside (object_mask) [n] as bytes; grad_theta [m,3].  */
HM_API int hm_idr_loss(const float *rgb, const float *rgb_gt, const float *sdf, const uint8_t *hit,
                       const uint8_t *inside, int64_t n_rays, const float *grad_theta, int64_t n_grad,
                       float eikonal_weight, float mask_weight, float alpha, float *terms, float *d_rgb, float *d_sdf,
                       float *d_grad, void *stream);
/* IDRLoss.forward with eikonal_weight, mask_weight, alpha read from hyper_dev[3] (device) when the kernel runs, so a
 * captured training step follows a schedule of them (training/idr_train.py:175-179,227-228: alpha doubled at its
 * milestones).  Equal values give bit-identical terms and gradients to hm_idr_loss.  The caller validates the values
 * (alpha > 0) where it writes them: device code cannot report an error.                                     */
HM_API int hm_idr_loss_dev(const float *rgb, const float *rgb_gt, const float *sdf, const uint8_t *hit,
                           const uint8_t *inside, int64_t n_rays, const float *grad_theta, int64_t n_grad,
                           const float *hyper_dev, float *terms, float *d_rgb, float *d_sdf, float *d_grad, void *stream);

/* ---- camera rays + bounding-sphere intersections --------------------------------------------------
 * Replaces rend_util.get_camera_params for 4x4 poses (utils/rend_util.py:48-75: lift, pose x pixel, normalise) and
 * rend_util.get_sphere_intersection (:141-162) for the rays it produces, as one launch: uv [B,N,2], pose / intrinsics
 * [B,4,4] -> ray_dirs [B,N,3], cam_loc [B,3], t_sphere [B,N,2] (clamped at 0), hit [B,N] (bytes).  Fixed cameras only:
 * nothing here is differentiated.                                                                        */
HM_API int hm_camera_rays(const float *uv, const float *pose, const float *intrinsics, int64_t n_images, int64_t n_pixels,
                          float radius, float *ray_dirs, float *cam_loc, float *t_sphere, uint8_t *hit, void *stream);

/* ---- optimizer tail of the training iteration ---------------------------------------------------
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) followed by torch.optim.Adam.step()
 * (training/idr_train.py:128,306-309; amsgrad / weight decay off as in the reference) over all tensors in
 * three launches.  In place: grad *= clip coefficient, exp_avg, exp_avg_sq, param.  max_norm <= 0 skips the
 * clipping.  Every tensor's step counter is incremented by the call (the bias corrections use the incremented
 * value); tensors left out of a call (no gradient) keep theirs, as in torch.  scratch_dev: hm_adam_scratch_floats()
 * device floats (2 + one partial sum per 8192 gradient elements); scratch_dev[1] receives the total gradient norm
 * (before clipping) when max_norm > 0.  The norm is summed in a fixed order (no float atomics): the whole update is
 * bitwise reproducible, so data-parallel replicas fed the same all-reduced gradients stay bitwise identical.
 * Sync-free and graph-capturable.                                                                     */
#define HM_ADAM_MAX_TENSORS 64
typedef struct hm_adam_tensor {
    float *param, *grad, *exp_avg, *exp_avg_sq;  /* device, fp32, contiguous, same numel */
    int64_t *step;                               /* device iteration counter of THIS tensor (torch: state['step']) */
    int64_t numel;
} hm_adam_tensor;
HM_API int64_t hm_adam_scratch_floats(const hm_adam_tensor *tensors, int n_tensors);
HM_API int hm_adam_step(const hm_adam_tensor *tensors, int n_tensors, float lr, float beta1, float beta2, float eps,
                        float max_norm, float *scratch_dev, void *stream);
/* torch.optim.Adam.step (after clip_grad_norm_) as hm_adam_step, with lr, beta1, beta2, eps, max_norm read from
 * hyper_dev[5] (device) when the kernels run, so a captured step follows lr / momentum schedules
 * (torch.optim.lr_scheduler).  The norm kernels run when clip != 0; a device max_norm <= 0 then gives clip
 * coefficient 1.  Equal values give bit-identical results to hm_adam_step.  The caller validates the values
 * (lr >= 0, 0 <= beta < 1, eps >= 0) where it writes them: device code cannot report an error.            */
HM_API int hm_adam_step_dev(const hm_adam_tensor *tensors, int n_tensors, const float *hyper_dev, int clip,
                            float *scratch_dev, void *stream);

/* Weight gradients of one backward pass in ONE launch: C_p += A_p^T B_p for every item (A_p [K, M] and B_p [K, N]
 * row-major with leading dimensions, C_p [M, N] accumulated with fp32 atomics - the caller zeroes it, like the
 * reference's optimizer.zero_grad()).  Replaces the per-layer grad_weight GEMMs autograd runs for nn.Linear in
 * ImplicitNetwork / RenderingNetwork (implicit_differentiable_renderer.py:102,211-221).  K a multiple of 128 takes the
 * grouped kernel, any other K falls back to hm_gemm_f32 for that item, and so does an item whose A or B spans 2 GB or
 * more (4 * lda * K or 4 * ldb * K >= 2^31: the grouped kernel forms 32-bit operand offsets).  Items with M, N or K
 * equal to 0 are skipped.  items is a [host] array.                                                                 */
#define HM_GEMM_GROUP_MAX 16
typedef struct hm_gemm_group_item {
    const float *A, *B;
    float *C;
    int64_t M, N, K, lda, ldb, ldc;
} hm_gemm_group_item;
HM_API int hm_gemm_f32_group_tn(const hm_gemm_group_item *items, int n_items, void *stream);

/* ---- deterministic mode (ops.deterministic; DESIGN.md "Deterministic mode") -------------------------------------
 * Bitwise reproducible forms of the reductions above: no fp32 atomics, a summation order that depends on shapes and
 * indices only.  Each takes a caller-owned device workspace of at least the matching *_workspace_bytes() bytes (0 when
 * nothing is split) and is sync-free and graph-capturable (kernel launches only).
 *
 * hm_gemm_f32 (the reference's grad_weight / grad_input / forward products, implicit_differentiable_renderer.py:102,
 * 116-128,211-221): the same tiles and split-K decomposition; every (tile, k part) stores its partial tile to the
 * workspace, a second launch forms C = C_old + (((p0 + p1) + p2) + ...) (accumulate) or C = ((p0 + p1) + ...) in k-part
 * order.  An unsplit K is the plain launch (one adder per element).  (hm_gemm_f32_ep never splits K.)              */
HM_API int64_t hm_gemm_f32_det_workspace_bytes(int transA, int transB, int64_t M, int64_t N, int64_t K, int64_t lda,
                                               int64_t ldb);
HM_API int hm_gemm_f32_det(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                           const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int accumulate,
                           void *workspace, int64_t workspace_bytes, void *stream);
/* hm_gemm_f32_group_tn (the weight gradients of one backward pass): the same problem table and k parts, partials of
 * every problem to the workspace in one launch, one reduce launch for all problems.  Items whose C windows overlap
 * (two terms of one weight gradient) go to consecutive launches and are added in item order - an item that falls back
 * to hm_gemm_f32_det included: the call gives the bits of consecutive one-item calls.  The workspace query returns -1
 * on a bad item.                                                                                                    */
HM_API int64_t hm_gemm_f32_group_tn_det_workspace_bytes(const hm_gemm_group_item *items, int n_items);
HM_API int hm_gemm_f32_group_tn_det(const hm_gemm_group_item *items, int n_items, void *workspace,
                                    int64_t workspace_bytes, void *stream);
/* The grouped product over operands with ADDENDS on a row range each: rows k in [a_k0, a_k1) of A are used as
 * A[k] + A2[k - a_k0] (A2 [a_k1 - a_k0, M], leading dimension lda2), rows [b_k0, b_k1) of B as B[k] + B2[k - b_k0] -
 * one fp32 add per element, formed where the kernel stages its operands, so the sum of two products over the same rows
 * (the weight gradients of two autograd nodes over shared activations) costs one.  An empty range (k0 == k1) is no
 * addend; A2 / B2 are then not read.  Everything else - tables, k parts, fall-back of an item to hm_gemm_f32, overlapping
 * C windows, the deterministic forms and their workspace - is hm_gemm_f32_group_tn's and hm_gemm_f32_group_tn_det's: a
 * call gives the values (deterministic: the bits) of that entry point on operands added beforehand.  A non-empty range
 * needs both ends multiples of 4, lda2 >= M (ldb2 >= N), 4 * ld2 * K < 2^31 and an item the grouped kernel takes (K a
 * multiple of 128, operands below 2 GB); otherwise the call fails with HM_ERR_INVALID at that item
 * (ops.gemm_group_tn_add adds such an addend beforehand).                                                          */
typedef struct hm_gemm_group_add_item {
    const float *A, *B;
    float *C;
    int64_t M, N, K, lda, ldb, ldc;
    const float *A2, *B2;
    int64_t lda2, ldb2, a_k0, a_k1, b_k0, b_k1;
} hm_gemm_group_add_item;
HM_API int hm_gemm_f32_group_tn_add(const hm_gemm_group_add_item *items, int n_items, void *stream);
HM_API int64_t hm_gemm_f32_group_tn_add_det_workspace_bytes(const hm_gemm_group_add_item *items, int n_items);
HM_API int hm_gemm_f32_group_tn_add_det(const hm_gemm_group_add_item *items, int n_items, void *workspace,
                                        int64_t workspace_bytes, void *stream);
/* hm_colsum / hm_colsum_acc / hm_colsum_acc_multi (nn.Linear bias gradients): slab partials to the workspace, then
 * summed per column in slab order - two launches per call (per HM_COLSUM_MAX_ITEMS items for the list form).       */
HM_API int64_t hm_colsum_det_workspace_bytes(int64_t M, int64_t N);
HM_API int hm_colsum_det(const float *x, int64_t M, int64_t N, int64_t ld, float *out, void *workspace,
                         int64_t workspace_bytes, void *stream);
HM_API int hm_colsum_acc_det(const float *x, int64_t M, int64_t N, int64_t ld, float *out, void *workspace,
                             int64_t workspace_bytes, void *stream);
HM_API int64_t hm_colsum_acc_multi_det_workspace_bytes(const hm_colsum_item *items, int n_items);
HM_API int hm_colsum_acc_multi_det(const hm_colsum_item *items, int n_items, void *workspace, int64_t workspace_bytes,
                                   void *stream);

/* ---- data-parallel gradient exchange (device side) ---------------------------------------------------
 * The reference runner is single-GPU (training/idr_train.py:92-93,278-321): there is no interface to
 * replace, the exchange is the build's own addition in the place the north star names - between loss.backward()
 * (idr_train.py:302) and clip_grad_norm_ / optimizer.step() (:306-308).  Everything except the collectives themselves
 * (RCCL, issued by the host side) is a kernel below, so that it can be captured into the training step's graphs.
 *
 * Hash-table gradient.  hm_encode_bwd_table_tracked is hm_encode_bwd_table (same atomics into d_table) that also lists
 * each row it touches ONCE: touched_bits [ceil(total_rows/32)] one claim bit per row (all zero between steps),
 * touched_count [1] the number of listed rows, touched_rows [cap] their ids in the fused table.  Several calls of one
 * step share the three buffers.  hm_rows_pack turns the list into this rank's payload [cap, 1+F] int32 (row id, then
 * the F gradient values as fp32 bits; entries beyond the count carry row -1), zeroing the listed rows of d_table and
 * their claim bits; status[0] (optional) receives the overflow if more than `cap` rows were claimed (the largest
 * count - cap seen so far; the first `cap` rows are packed as usual).  The rows claimed beyond `cap` keep their claim
 * bit and their dense value: they are never listed again, so after an overflow the three tracking buffers and
 * d_table have to be set up afresh.  After ONE
 * all-gather of the payloads hm_rows_apply adds list r = lists + r*list_stride (r = 0..n_lists-1, one launch each, in
 * that order) into d_table scaled by `scale` (1/world): rows are unique inside a list, so plain read-modify-writes
 * suffice and every replica sums every row in the same (rank) order - bitwise identical replicas, no sort.
 * hm_rows_clear (after the optimizer step) zeroes the rows named by all lists again and resets *touched_count.      */
HM_API int hm_encode_bwd_table_tracked(const hm_grid_desc *desc, const float *x, int64_t n, const float *d_feat,
                                       int64_t d_feat_stride, float *d_table, int frac_mode, uint32_t *touched_bits,
                                       int32_t *touched_count, int32_t *touched_rows, int64_t cap, void *stream);
/* Deterministic hm_encode_bwd_table_tracked (the hash-table scatter_add of hashGridEmbedding.py's backward, for the
 * data-parallel exchange): hm_encode_bwd_table_sorted's run sums over the output of hm_encode_rows ->
 * hm_sort_pairs_i32, and the head of every run with a nonzero weight claims its row's bit and a slot of touched_rows -
 * the same bits, count, cap and overflow semantics as hm_encode_bwd_table_tracked.  The dense values are
 * reproducible; the order of the list is not (hm_rows_apply does not depend on it).                              */
HM_API int hm_encode_bwd_table_sorted_tracked(const hm_grid_desc *desc, const int32_t *keys_sorted,
                                              const int64_t *perm, int64_t n_keys, int corners, const float *d_feat,
                                              int64_t d_feat_stride, const float *weights, float *d_table,
                                              uint32_t *touched_bits, int32_t *touched_count, int32_t *touched_rows,
                                              int64_t cap, void *stream);
HM_API int hm_rows_pack(float *d_table, int n_features, const int32_t *touched_rows, const int32_t *touched_count,
                        int64_t cap, uint32_t *touched_bits, int32_t *payload, int32_t *status, void *stream);
HM_API int hm_rows_apply(float *d_table, int64_t total_rows, int n_features, const int32_t *lists, int64_t cap,
                         int64_t list_stride, int n_lists, float scale, void *stream);
HM_API int hm_rows_clear(float *d_table, int64_t total_rows, int n_features, const int32_t *lists, int64_t cap,
                         int64_t list_stride, int n_lists, int32_t *touched_count, void *stream);

/* MLP gradients -> one flat bucket in ONE launch (the bucket is all-reduced in place; hm_adam_step then reads the
 * averaged gradients from it).  items is a [host] array, copied by value into the kernel arguments.              */
#define HM_COPY_MAX_ITEMS 96
typedef struct hm_copy_item {
    const float *src;
    float *dst;
    int64_t numel;
} hm_copy_item;
HM_API int hm_multi_copy_f32(const hm_copy_item *items, int n_items, void *stream);

/* ---- mesh extraction: marching cubes ------------------------------------------------------------
 * Replaces skimage.measure.marching_cubes(volume, level, spacing) as plots.py:122-128 (and
 * get_surface_high_res_mesh, plots.py:146-224) call it: vertices on the sign-changing lattice edges by linear
 * interpolation, t = (level - a)/(b - a), at ((i,j,k) + t e_axis) * spacing in the volume's axis order; triangles from
 * the generated case table (csrc/hm_mc_table.h; ambiguous faces cut every inside corner off on its own, so the
 * triangulation inside ambiguous cells may differ from marching_cubes_lewiner); normals = central differences
 * (one-sided at the border) over the spacing, interpolated with t and normalised, pointing toward increasing values
 * (the reference's -normals; (0,0,0) where the gradient is zero).
 * vol is fp32 [nx, ny, nz] with element strides sx, sy, sz >= 0 (a transposed view works without a copy); every
 * dimension >= 2 and nx*ny*nz < 2^31.  Output order does not depend on the strides: vertices by owning lattice point
 * ((i*ny + j)*nz + k), then axis x < y < z; faces by cell linear index, then table order.  No atomics: repeated calls
 * give the same bits.
 *   hm_mc_count: classifies the lattice into the workspace; counts [3] int64 (device) receive the number of vertices,
 *                the number of faces and 1 if any volume value is NaN (else 0).
 *   hm_mc_emit:  after hm_mc_count on the same stream, volume and workspace: verts [n_verts, 3], normals [n_verts, 3]
 *                fp32 and faces [n_faces, 3] int32 (vertex ids); n_verts / n_faces are the counts hm_mc_count wrote
 *                (read by the caller) and must fit int32 indices.  spacing is [host] [3].                          */
HM_API int64_t hm_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
HM_API int hm_mc_count(const float *vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz,
                       float level, void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream);
HM_API int hm_mc_emit(const float *vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz,
                      float level, const float *spacing, void *workspace, int64_t workspace_bytes, int64_t n_verts,
                      int64_t n_faces, float *verts, float *normals, int32_t *faces, void *stream);

/* ---- mesh extraction: brick-sparse marching cubes --------------------------------------------------
 * The same mesh from a lattice that is evaluated only near the surface (driver: ops.marching_cubes_sparse; scheme:
 * DESIGN.md, Mesh extraction).  The lattice [nx, ny, nz] (every dimension in [2, 65536]; nx*ny*nz may exceed 2^31) is
 * split into bricks of HM_MCS_BRICK^3 points: point (i, j, k) is value ((i%8)*8 + j%8)*8 + k%8 of brick
 * (i/8, j/8, k/8).  map is the dense int32 brick map [ceil(nx/8), ceil(ny/8), ceil(nz/8)]: the brick's slot in the
 * value pool [n_slots, 8, 8, 8] fp32, or -1 (any value outside [0, n_slots) reads as -1) while it is not evaluated.
 * Brick lists are int32 linear ids into the map, at most HM_MCS_MAX_LIST long; an id outside the map is skipped.
 * The cell block of a brick is its 8^3 cells; their corners are the points [8b, 8b + 8] clipped to the lattice.
 *   hm_mcs_points_bricks: points [n_bricks*512, 3] = the coordinates of the listed bricks' points, brick by brick in
 *                pool order; padding points of a border brick take the clamped index.  ax, ay, az are the device axis
 *                arrays [nx], [ny], [nz]; xform is [host] [12] (r [3][3] row-major, then s [3]) or NULL:
 *                p[c] = ((x*r[0][c] + y*r[1][c]) + z*r[2][c]) + s[c] in fp32, NULL: p = (x, y, z) - a point's
 *                coordinates depend on its lattice index alone.
 *   hm_mcs_points_index: the same for the n lattice points of linear index ((i*ny + j)*nz + k) index[.] (int64,
 *                device); NaN coordinates for an index outside the lattice.
 *   hm_mcs_status: status [n_bricks] int32 of the listed bricks: HM_MCS_BOTH - the cell block holds values on both
 *                sides of level (v < level, the rule of hm_mc_count); HM_MCS_FACE(f), f = 0..5 for -x +x -y +y -z +z -
 *                so does that face of the block and a brick lies across it; HM_MCS_NAN - a value of the block is NaN;
 *                HM_MCS_UNDECIDED - the brick or an upper neighbour the block reaches into is not evaluated (the other
 *                bits then cover the evaluated part).
 *   hm_mcs_count / hm_mcs_emit: hm_mc_count / hm_mc_emit over the points of the listed bricks - every listed point
 *                owns its +x, +y, +z lattice edges and the cell it is the lowest corner of, values are read through
 *                the map, and an edge or a cell with a corner that is not evaluated emits nothing; same arithmetic,
 *                same counts convention, same workspace rule (hm_mcs_workspace_bytes), same int32 limit.  list_pos is
 *                the int32 map-shaped inverse of the list (position of a brick in it, or -1).  Emit needs every brick
 *                that owns a crossing edge of a listed cell to be listed (a face gets vertex id -1 otherwise) and the
 *                +-1 points of every vertex' edge ends to be evaluated (NaN normals otherwise).  Outputs are in list
 *                order, with vert_keys [n_verts] = ((i*ny + j)*nz + k)*3 + axis and face_keys [n_faces] = (linear
 *                index of the cell's lowest corner)*8 + (triangle in table order), int64: sorted by key (faces
 *                renumbered) they are hm_mc_emit's outputs on the fully evaluated lattice, bit for bit.
 * No entry point synchronises; no atomics.                                                                         */
#define HM_MCS_BRICK 8
#define HM_MCS_MAX_DIM 65536
#define HM_MCS_MAX_LIST (1 << 22)
#define HM_MCS_BOTH 1
#define HM_MCS_FACE(f) (2 << (f))
#define HM_MCS_NAN 128
#define HM_MCS_UNDECIDED 256
typedef struct hm_mcs_lattice {
    int64_t nx, ny, nz;
    int64_t n_slots;
    const int32_t *map;
    const float *pool;
} hm_mcs_lattice;
HM_API int hm_mcs_points_bricks(const int32_t *bricks, int64_t n_bricks, const float *ax, const float *ay,
                                const float *az, int64_t nx, int64_t ny, int64_t nz, const float *xform, float *points,
                                void *stream);
HM_API int hm_mcs_points_index(const int64_t *index, int64_t n, const float *ax, const float *ay, const float *az,
                               int64_t nx, int64_t ny, int64_t nz, const float *xform, float *points, void *stream);
HM_API int hm_mcs_status(const int32_t *bricks, int64_t n_bricks, const hm_mcs_lattice *lat, float level,
                         int32_t *status, void *stream);
HM_API int64_t hm_mcs_workspace_bytes(int64_t n_bricks);
HM_API int hm_mcs_count(const int32_t *bricks, int64_t n_bricks, const hm_mcs_lattice *lat, float level,
                        void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream);
HM_API int hm_mcs_emit(const int32_t *bricks, int64_t n_bricks, const hm_mcs_lattice *lat, const int32_t *list_pos,
                       float level, const float *spacing, void *workspace, int64_t workspace_bytes, int64_t n_verts,
                       int64_t n_faces, float *verts, float *normals, int32_t *faces, int64_t *vert_keys,
                       int64_t *face_keys, void *stream);

/* ---- mesh cleanup: connected components, their areas, surface moments, one component's submesh ---------
 * Replaces what evaluation/eval.py does to every fine mesh on the host - components = mesh.split(only_watertight=
 * False); areas = [c.area for c in components]; mesh = components[areas.argmax()] - and the exact surface moments
 * (plots._surface_moments) that stand in for the reference's trimesh.sample.  Driver: ops.mesh_components,
 * ops.mesh_component_areas, ops.mesh_select, ops.mesh_largest_component, ops.mesh_surface_moments.
 * A mesh is verts [n_verts, 3] fp32 and faces [n_faces, 3] int32, contiguous (what hm_mc_emit writes); n_verts and
 * n_faces < 2^31.  status is one device int32 the CALLER has zeroed: bit 0 is set when a face index lies outside
 * [0, n_verts) (or a label / rank does not fit the mesh) - such an index is never dereferenced and its face is left
 * out; the caller reads the word with its counts and raises.  No entry point synchronises; the floating-point sums
 * use no atomics and a fixed order, so repeated calls give the same bits.
 *   hm_mesh_cc_labels (split): label [n_verts] int32 = the smallest vertex id of the vertex' component; two vertices
 *                are connected when a face holds both, a vertex of no face labels itself.  Lock-free union-find over
 *                the face edges (f0, f1), (f1, f2) in one pass, then a flatten launch (csrc/hm_mesh_cc.hip).
 *   hm_mesh_cc_face_stats (c.area, per face): face_area [n_faces] fp64 = 0.5 |(v1 - v0) x (v2 - v0)| of the vertices
 *                cast to fp64 (TriMesh.area_faces); used [n_verts] int32, zeroed by the caller, gets 1 at every vertex
 *                of a face.
 *   hm_mesh_cc_sums (c.area, per component): rank [n_verts] int32 is, at a root with used != 0, its position among
 *                those roots in ascending order (an exclusive prefix sum; other entries are not read); area
 *                [n_components] fp64 and count [n_components] int64 receive each such component's area and number of
 *                faces: the faces are sorted by their component's rank with hm_sort_pairs_i32 (stable) and every run
 *                is summed in a fixed order.  workspace: hm_mesh_cc_sums_workspace_bytes(n_faces).
 *   hm_mesh_moments: out [13] fp64 = total area, mean [3] and covariance [3][3] of the uniform distribution on the
 *                surface, the formula of plots._surface_moments in fp64: block partials, then one workgroup.  NaN mean
 *                and covariance when the area is 0.  workspace: hm_mesh_moments_workspace_bytes(n_faces).
 *   hm_mesh_select_mark (components[argmax]): fflag [n_faces] int32 = 1 for the faces whose first vertex has label
 *                == component, else 0; vflag [n_verts] int32, zeroed by the caller, gets 1 at their vertices.
 *   hm_mesh_select_emit: vpre / fpre are the exclusive prefix sums of vflag / fflag (int32) and n_verts_out /
 *                n_faces_out their totals, read by the caller: verts_out / normals_out [n_verts_out, 3] are the flagged
 *                rows in ascending order (normals may be NULL), faces_out [n_faces_out, 3] the flagged faces in order
 *                with index v replaced by vpre[v] - np.unique(faces, return_inverse=True) as TriMesh.split uses it. */
HM_API int hm_mesh_cc_labels(const int32_t *faces, int64_t n_faces, int64_t n_verts, int32_t *label, int32_t *status,
                             void *stream);
HM_API int hm_mesh_cc_face_stats(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                                 double *face_area, int32_t *used, int32_t *status, void *stream);
HM_API int64_t hm_mesh_cc_sums_workspace_bytes(int64_t n_faces);
HM_API int hm_mesh_cc_sums(const int32_t *faces, int64_t n_faces, int64_t n_verts, const int32_t *label,
                           const int32_t *rank, const double *face_area, int64_t n_components, double *area,
                           int64_t *count, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
HM_API int64_t hm_mesh_moments_workspace_bytes(int64_t n_faces);
HM_API int hm_mesh_moments(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, double *out,
                           void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
HM_API int hm_mesh_select_mark(const int32_t *faces, int64_t n_faces, int64_t n_verts, const int32_t *label,
                               int32_t component, int32_t *vflag, int32_t *fflag, int32_t *status, void *stream);
HM_API int hm_mesh_select_emit(const float *verts, const float *normals, const int32_t *faces, int64_t n_faces,
                               int64_t n_verts, const int32_t *vflag, const int32_t *vpre, const int32_t *fflag,
                               const int32_t *fpre, int64_t n_verts_out, int64_t n_faces_out, float *verts_out,
                               float *normals_out, int32_t *faces_out, void *stream);

/* ---- mesh simplification: vertex clustering on the uniform grid of the Chamfer evaluation ---------
 * Decimates a mesh to a chosen cell size on the device (DESIGN.md "Mesh simplification" states the contract,
 * tests/mesh_simplify_cases.py restates it in numpy).  Driver: ops.mesh_simplify, which also takes the prefix sums and
 * reads the counts between the entry points.  The mesh and the status word are those of the mesh cleanup above; the
 * grid (lo, h, g) is that of the Chamfer evaluation below: cell = clamp(floor((p - lo) / h), 0, g - 1) per axis in
 * fp32, key = (cx*g[1] + cy)*g[2] + cz, fewer than 2^31 cells.  No entry point synchronises; no floating-point atomic
 * is used and every sum has a fixed order, so repeated calls give the same bits (csrc/hm_mesh_simplify.hip).
 *   hm_mesh_simplify_keys: used [n_verts] int32, zeroed by the caller, gets 1 at every vertex of a face (a face index
 *                outside [0, n_verts) sets status bit 0 and is never dereferenced).  The used vertices' keys - unused
 *                ones get the number of cells, above every key - are sorted with hm_sort_pairs_i32 (stable) into
 *                keys_sorted [n_verts] int32 and perm [n_verts] int64: a cluster is one run, its members in ascending
 *                vertex id.  head [n_verts] int32 = 1 at the first position of every run of a used key, else 0.
 *                workspace: hm_mesh_simplify_keys_workspace_bytes(n_verts).
 *   hm_mesh_simplify_clusters: start [n_clusters + 1] int64 = the positions of head's ones in ascending order and then
 *                the number of used vertices.  For cluster c with the k members perm[start[c] .. start[c+1]), in fp64
 *                from the fp32 inputs: m = (sum p)/k; n^ = n/|n|, 0 for a zero or non-finite normal; the
 *                representative rep [n_clusters, 3] fp32 is m, or with quadric != 0 (normals required, reg > 0)
 *                m + A^-1 b, A = sum n^ n^T + reg k I, b = sum n^ (n^ . (p - m)), clamped per axis to [min(blo, m),
 *                max(bhi, m)], blo = lo + cell h, bhi = blo + h; rep_normals [n_clusters, 3] fp32 (with normals) is
 *                (sum n^)/|sum n^|, or 0 when that length is 0.  One rounding to fp32 at the end.  cluster_of
 *                [n_verts] int32, filled with -1 by the caller, gets c at every member.  One wave per run.
 *   hm_mesh_simplify_face_flags: fkeep [n_faces] int32 = 1 for the faces whose three vertices lie in three different
 *                clusters, else 0.
 *   hm_mesh_simplify_dedupe: fpre is the exclusive prefix sum of fkeep (int32) and n_tri its total.  tri [3, n_tri]
 *                int32 receives the kept faces' cluster triples in face order, one row per corner, each triple rotated
 *                cyclically so that its smallest id comes first.  Three stable sorts by the third, second and first id
 *                order them; tkeep [n_tri] int32 = 0 for a triple equal to its predecessor in that order (a repeat of
 *                an earlier face), else 1; cused [n_clusters] int32, zeroed by the caller, gets 1 at the clusters of
 *                the triples with tkeep = 1.  workspace: hm_mesh_simplify_dedupe_workspace_bytes(n_tri).
 *   hm_mesh_simplify_emit: cpre / tpre are the exclusive prefix sums of cused / tkeep (int32) and n_verts_out /
 *                n_faces_out their totals.  verts_out / normals_out [n_verts_out, 3] are the marked clusters' rep /
 *                rep_normals in ascending order (rep_normals may be NULL), faces_out [n_faces_out, 3] the triples with
 *                tkeep = 1 in order with id c replaced by cpre[c], vertex_map [n_verts] int32 = cpre of the vertex'
 *                cluster, or -1 for a vertex of no face or of an unmarked cluster. */
HM_API int64_t hm_mesh_simplify_keys_workspace_bytes(int64_t n_verts);
HM_API int hm_mesh_simplify_keys(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                                 const float *lo, float h, const int32_t *g, int32_t *used, int32_t *keys_sorted,
                                 int64_t *perm, int32_t *head, void *workspace, int64_t workspace_bytes,
                                 int32_t *status, void *stream);
HM_API int hm_mesh_simplify_clusters(const float *verts, const float *normals, int64_t n_verts,
                                     const int32_t *keys_sorted, const int64_t *perm, const int64_t *start,
                                     int64_t n_clusters, const float *lo, float h, const int32_t *g, int quadric,
                                     double reg, float *rep, float *rep_normals, int32_t *cluster_of, void *stream);
HM_API int hm_mesh_simplify_face_flags(const int32_t *faces, int64_t n_faces, int64_t n_verts,
                                       const int32_t *cluster_of, int64_t n_clusters, int32_t *fkeep, void *stream);
HM_API int64_t hm_mesh_simplify_dedupe_workspace_bytes(int64_t n_tri);
HM_API int hm_mesh_simplify_dedupe(const int32_t *faces, int64_t n_faces, int64_t n_verts, const int32_t *cluster_of,
                                   int64_t n_clusters, const int32_t *fkeep, const int32_t *fpre, int64_t n_tri,
                                   int32_t *tri, int32_t *tkeep, int32_t *cused, void *workspace,
                                   int64_t workspace_bytes, void *stream);
HM_API int hm_mesh_simplify_emit(const float *rep, const float *rep_normals, int64_t n_clusters, const int32_t *cused,
                                 const int32_t *cpre, int64_t n_verts_out, const int32_t *tri, int64_t n_tri,
                                 const int32_t *tkeep, const int32_t *tpre, int64_t n_faces_out,
                                 const int32_t *cluster_of, int64_t n_verts, float *verts_out, float *normals_out,
                                 int32_t *faces_out, int32_t *vertex_map, void *stream);

/* ---- Chamfer evaluation: exact nearest neighbours on a uniform grid, deterministic triangle upsampling ---------
 * The device side of the reference's DTU Chamfer evaluation (code/evaluation/dtu_eval): upsample every triangle to a
 * point density, nearest-neighbour distances between two clouds.  Driver: ops.nn_index, ops.nearest_neighbors,
 * ops.mesh_sample_surface, ops.chamfer_distance, evaluation.chamfer.mesh_chamfer.  status is one device int32 the
 * CALLER has zeroed; no entry point synchronises, none uses floating-point atomics, no atomic decides a position.
 *
 * The grid: origin lo[3], cell edge h > 0 and dimensions g[3] >= 1 are HOST values, g[0]*g[1]*g[2] < 2^31.  The cell
 * of a coordinate is clamp(floor((p - lo) / h), 0, g - 1) per axis in fp32, its key (cx*g[1] + cy)*g[2] + cz.
 *   hm_nn_workspace_bytes(n): the scratch of hm_nn_build over n points, and of hm_nn_query over n queries.
 *   hm_nn_build: points [n,3] fp32, 1 <= n < 2^31.  Writes cell_start [cells + 1] int32 (the points of cell c are
 *                records [cell_start[c], cell_start[c+1])) and records [n,4] fp32: the points ordered by cell with the
 *                library's stable sort (ascending original index inside a cell) as x, y, z and the original index as
 *                the int32 bits of the fourth word.  cell_start comes from a binary search of the sorted keys per
 *                cell: plain stores.  A non-finite coordinate sets status bit 0 and goes to cell 0.
 *   hm_nn_query: query [m,3] fp32, m >= 0.  For every query, index [m] int32 is the point that minimises the fp32
 *                value d2 = (dx*dx + dy*dy) + dz*dz (dx = q.x - p.x, ..., every operation rounded once), the smallest
 *                original index among equal d2, and d2 [m] that value: what a brute-force fp32 argmin over all points
 *                returns, bit for bit, whatever the grid, m and the thread order.  max_dist2 (fp32, +inf = none): a
 *                query whose minimum is > max_dist2 gets index -1 and d2 +inf; == max_dist2 is reported.  A non-finite
 *                query coordinate sets status bit 1.  The queries are sorted by cell, a wave takes 64 of them and
 *                searches a growing box of cells (csrc/hm_nn.hip states the stopping rule).  n_tests (may be NULL;
 *                a measurement aid): a device counter the caller has zeroed, receives the number of (query lane,
 *                candidate) distance evaluations of the launch.
 * Triangle upsampling (the DTU rule; fp64, every operation rounded once; a, b, c the face's fp32 vertices as fp64):
 *   v1 = b - a, v2 = c - a, l1 = sqrt((v1x^2 + v1y^2) + v1z^2), l2 likewise, A2 = |v1 x v2| (same sum order); no
 *   samples unless A2 > 0; thr = density*sqrt(l1*l2/A2), n1 = floor(l1/thr), n2 = floor(l2/thr); no samples unless
 *   n1 >= 1 and n2 >= 1; for i in 0..n1, j in 0..n2 (inclusive, i outer): u = (i + 0.5)/n1, v = (j + 0.5)/n2, keep
 *   when u + v < 1 the point fp32((v1*u + v2*v) + a).
 *   hm_mesh_sample_count: count [n_faces] int64 samples per face and rows [n_faces] int32 (n1 + 1, or 0 without
 *                samples).  A face index outside [0, n_verts) sets status bit 0 and is never dereferenced; a face whose
 *                n1*n2 exceeds 2^33 counts as 2^40 samples (the caller rejects totals >= 2^31 anyway).
 *   hm_mesh_sample_emit: prefix [n_faces] int64 = the exclusive prefix sum of count, n_samples its total (< 2^31),
 *                max_rows the maximum of rows.  Writes samples [n_samples,3] fp32 and face_of [n_samples] int32: faces
 *                ascending, then i, then j.  One wave per face and per 1024 rows of it, lanes over the samples. */
HM_API int64_t hm_nn_workspace_bytes(int64_t n);
HM_API int hm_nn_build(const float *points, int64_t n, const float *lo, float h, const int32_t *g, int32_t *cell_start,
                       float *records, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
HM_API int hm_nn_query(const float *query, int64_t m, const float *records, int64_t n, const int32_t *cell_start,
                       const float *lo, float h, const int32_t *g, float max_dist2, float *d2, int32_t *index,
                       void *workspace, int64_t workspace_bytes, int32_t *status, uint64_t *n_tests, void *stream);
HM_API int hm_mesh_sample_count(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                                double density, int64_t *count, int32_t *rows, int32_t *status, void *stream);
HM_API int hm_mesh_sample_emit(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                               double density, const int64_t *prefix, int64_t n_samples, int64_t max_rows,
                               float *samples, int32_t *face_of, void *stream);

/* ---- DTU evaluation: greedy radius down-sampling, observation-mask and ground-plane filters ---------------------
 * What the reference's evaluation/dtu_eval does between the sampled cloud and the mean distances.  Driver:
 * ops.radius_downsample, ops.dtu_point_flags, ops.one_sided_distance, evaluation.chamfer.dtu_chamfer.  As in the
 * Chamfer section: no entry point synchronises, no atomic decides a position (the thinning uses no atomic
 * read-modify-write at all), and no thread waits for another workgroup.
 *
 * Radius thinning (csrc/hm_nn_radius.hip) reproduces
 *     mask = ones; for i in index order: if mask[i]: mask[neighbours(i)] = 0; mask[i] = 1
 * where j is a neighbour of i when the fp32 value d2 = (dx*dx + dy*dy) + dz*dz of hm_nn_query is <= radius2 (equality
 * counts).  A point is kept exactly when none of its lower-index neighbours is kept - a unique set - and it is found in
 * rounds over a state per point: an undecided point with a kept lower-index neighbour is removed, one whose
 * lower-index neighbours are all removed is kept, any other waits.  The file's header comment gives the arguments:
 *   (a) the scan of a point reaches every j with d2 <= radius2 for ANY cell edge: per axis the cells from
 *       nn_cell(L) to nn_cell(H), L and H checked by the kernel to lie outside the radius by that axis alone, the cell
 *       function being monotone (points on cell faces and cells smaller than the radius included);
 *   (b) states only move from undecided to a final value that depends on final values of lower indices alone, so the
 *       result is the sequential loop's for any thread order, and concurrent reads of a state being written are benign;
 *   (c) the lowest-index undecided point is decided by the next round, so n rounds suffice; the driver loops until
 *       the remaining count is 0 and has no other exit.
 * records, cell_start, lo, h, g: what hm_nn_build made and was given.  info: 4 device int32; info[0], info[1] hold the
 * number of undecided points before even / odd rounds, info[2] the number of rounds that had something to decide.
 *   hm_nn_radius_workspace_bytes(n): the scratch all three calls share (states, two lists, block counts).
 *   hm_nn_radius_begin:  every point undecided, the list is all sorted positions, info = {n, 0, 0, 0}.
 *   hm_nn_radius_rounds: radius2 >= 0 the fp32 bound on d2; bound > 0 an estimate of the radius rounded outward (the
 *                kernel checks and widens it per point, see (a)); capacity in [1, n]: an upper bound of the current
 *                count, normally the count last read; round0: the rounds run so far (selects the list and info word).
 *                capacity > 1024: runs n_rounds (1..64) rounds - decide, exclusive scan of the blocks' waiting counts,
 *                ordered scatter of the waiting points into the other list; rounds past completion do nothing.  The
 *                caller then reads info[(round0 + n_rounds) & 1].  capacity <= 1024: one workgroup runs rounds until
 *                the list is empty, at most as many as it has points, and writes the count left (0) to info[round0 & 1].
 *   hm_nn_radius_finish: keep [n] uint8 by ORIGINAL index, 1 = kept; call when the count is 0.
 * Point flags (csrc/hm_dtu_filter.hip), flags [n] uint8; fp64 on the fp32 coordinates, every operation rounded once:
 *   bit 0  lo <= p < hi on all three axes (lo = BB0 - patch, hi = BB1 + 2*patch, formed by the caller in fp64)
 *   bit 1  k = rint((p - bb0)/res) per axis (half to even), 0 <= k < shape on all axes and mask[kx, ky, kz] != 0;
 *          mask is a contiguous uint8 [shape0, shape1, shape2] volume; an index outside it - from a huge coordinate
 *          included - is never dereferenced
 *   bit 2  ((P0*x + P1*y) + P2*z) + P3 > 0
 *   a non-finite coordinate gives 0.  shape: 3 host int64; params: 14 host doubles lo[3], hi[3], bb0[3], res, P[4]. */
HM_API int64_t hm_nn_radius_workspace_bytes(int64_t n);
HM_API int hm_nn_radius_begin(int64_t n, void *workspace, int64_t workspace_bytes, int32_t *info, void *stream);
HM_API int hm_nn_radius_rounds(const float *records, int64_t n, const int32_t *cell_start, const float *lo, float h,
                               const int32_t *g, float radius2, float bound, int64_t capacity, int64_t round0,
                               int32_t n_rounds, void *workspace, int64_t workspace_bytes, int32_t *info, void *stream);
HM_API int hm_nn_radius_finish(const float *records, int64_t n, void *workspace, int64_t workspace_bytes, uint8_t *keep,
                               void *stream);
HM_API int hm_dtu_point_flags(const float *points, int64_t n, const uint8_t *mask, const int64_t *shape,
                              const double *params, uint8_t *flags, void *stream);

/* ---- image metrics: PSNR over a mask and SSIM of rendered views ---------------------------------------------------
 * What the reference's evaluation/eval.py computes per view on the host (calculate_psnr; SSIM of Wang et al. 2004 with
 * a Gaussian window, the torchmetrics defaults).  Driver: ops.image_psnr, ops.image_ssim, evaluation.images.
 * csrc/hm_image.hip.  x, y: fp32 [B, H, W, C], contiguous, 1 <= C <= 4; B, H, W in [1, 2^31), B*H*W*C < 2^62.  Every
 * difference, product, sum and quotient is fp64 on the fp32 values.  Both reductions have a fixed order - per-workgroup
 * partials, then one workgroup per image over its partials in index order - and use no atomics: two calls give the
 * same bits.  No entry point synchronises and there is no device-side error path.
 *   hm_image_sqerr: out [B,2] fp64 = {sum over the set pixels and their channels of (x - y)^2, n = the number of set
 *                pixels}; mask [B,H,W] bytes (non-zero = set) or NULL for every pixel.  Pixels that are not set are not
 *                read.  The caller forms mse = sum / (n*C) and psnr = 10 log10(L^2 / mse).  One workgroup per 1024
 *                pixels of an image.  partial_ws: hm_image_sqerr_workspace_bytes(B, H, W) bytes.
 *   hm_image_ssim:  win odd in [3, 31], H >= win and W >= win; weights: win DEVICE fp64 that sum to 1, the window is
 *                weights[i]*weights[j]; c1, c2 finite and > 0.  For every window inside the image - (H-win+1)(W-win+1)
 *                positions per channel, no padding - the weighted moments mx, my, Exx, Eyy, Exy (horizontal pass, then
 *                vertical), sx2 = Exx - mx^2, sy2 = Eyy - my^2, sxy = Exy - mx my and
 *                    s = ((2 mx my + c1)(2 sxy + c2)) / ((mx^2 + my^2 + c1)(sx2 + sy2 + c2)).
 *                out [B] fp64 = the mean of s over positions and channels; map, unless NULL, [B, H-win+1, W-win+1, C]
 *                fp64 = s.  y == x gives exactly 1.  One workgroup per 16 x 16 positions; partial_ws:
 *                hm_image_ssim_workspace_bytes(B, H, W, win) bytes.  A window and channel count whose tile does not
 *                fit the CU's LDS is refused (none within the limits above: 99,456 bytes at win = 31, C = 4). */
HM_API int64_t hm_image_sqerr_workspace_bytes(int64_t B, int64_t H, int64_t W);
HM_API int hm_image_sqerr(const float *x, const float *y, const uint8_t *mask, int64_t B, int64_t H, int64_t W,
                          int64_t C, double *partial_ws, double *out, void *stream);
HM_API int64_t hm_image_ssim_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t win);
HM_API int hm_image_ssim(const float *x, const float *y, int64_t B, int64_t H, int64_t W, int64_t C, int64_t win,
                         const double *weights, double c1, double c2, double *map, double *partial_ws, double *out,
                         void *stream);

/* ---- mesh culling: camera-mask votes, depth maps of the mesh, visibility votes, compaction -------------------------
 * Removes what no camera could have constrained: geometry that projects outside the (dilated) object masks and geometry
 * hidden from every camera.  Driver: ops.mesh_mask_votes, ops.mesh_depth_maps, ops.mesh_visible_votes,
 * ops.mesh_keep_vertices, evaluation.cull.cull_mesh.  csrc/hm_mesh_cull.hip, csrc/hm_view_dev.h.  No entry point
 * synchronises; n_verts, n_faces, n_views in [0, 2^31); H, W in [1, 65536] with H*W < 2^31.
 * A view is proj [n_views, 3, 4] DEVICE fp64, P = K[:3,:3] @ inv(pose)[:3,:4]; pixel (col, row) has its centre at
 * uv = (col, row).  A vertex (fp32, cast to fp64; every operation rounded once, no contraction):
 *     p_a = ((P[a,0]*x + P[a,1]*y) + P[a,2]*z) + P[a,3],  w = p_2,  u = p_0 / w,  v = p_1 / w
 *   unprojectable: a non-finite coordinate, or w <= 0, or w not finite
 *   pixel          col = rint(u), row = rint(v) (half to even); in the image iff 0 <= col < W and 0 <= row < H
 *   fixed point    X = rint(256 u), Y = rint(256 v), valid iff |X| < 2^24 and |Y| < 2^24; pixel centres at (256 col, 256 row)
 * every range test is made on doubles before a value becomes an integer: a NaN or a huge value fails it, nothing is read.
 *   hm_mesh_mask_votes: sat [n_views, H+1, W+1] int32 the summed-area table of the masks (sat[v][r][c] = set pixels in
 *                rows < r and columns < c).  Per vertex: n_in_image = the views that have it in the image; n_in_mask =
 *                those where also a mask pixel (c, r') with |c - col| <= dilate and |r' - row| <= dilate inside the
 *                image is set (a (2 dilate + 1)^2 square element, zero outside the image).  accumulate != 0 adds to the
 *                arrays (the next chunk of views) instead of writing them.  No atomics.
 *   hm_mesh_depth_maps: depth [n_views, H, W] fp32 = the nearest surface per pixel, +inf where nothing is drawn;
 *                n_skipped [n_views] int32.  Per face and view: a face with an unprojectable corner or an invalid
 *                fixed-point position is skipped and counted (no clipping).  area = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) in
 *                int64; 0 draws nothing.  For the pixel centres (Xp, Yp) inside the face's bounding box clamped to the
 *                image, E_a = (X_c-X_b)(Yp-Y_b) - (Y_c-Y_b)(Xp-X_b), (b, c) = (a+1, a+2) mod 3; covered iff all E_a >= 0
 *                or all E_a <= 0 (both windings, inclusive edges).  b_a = double(E_a)/double(area), iw_a = 1/w_a,
 *                z = 1/((b_0 iw_0 + b_1 iw_1) + b_2 iw_2) rounded to fp32, stored when finite and > 0 by an unsigned
 *                atomicMin on its bits: independent of the order of the faces, two calls give the same bits.  A face
 *                whose clamped box has more than big_face (>= 1) pixels is drawn by one wave, any other by one lane.
 *                A face index outside [0, n_verts) sets bit 0 of status [1] int32 and is never dereferenced.
 *                workspace: hm_mesh_depth_workspace_bytes(n_verts, n_faces) bytes, reused view after view.
 *   hm_mesh_visible_votes: n_visible = the views that have the vertex in the image with
 *                float(w) <= m + tol (fp32), m = the maximum of depth over the (2 pad + 1)^2 pixels around (col, row),
 *                indices clamped to the image; pad in [0, 64].  accumulate as above.
 *   hm_mesh_keep_mark: fflag [n_faces] int32 = 1 for the faces whose three vertices have keep [n_verts] (bytes) set,
 *                vflag [n_verts] int32 (zeroed by the caller) = 1 for their vertices; out-of-range indices as above.
 *                hm_mesh_select_emit then writes the mesh. */
HM_API int hm_mesh_mask_votes(const float *verts, int64_t n_verts, const double *proj, int64_t n_views,
                              const int32_t *sat, int64_t H, int64_t W, int64_t dilate, int accumulate,
                              int32_t *n_in_image, int32_t *n_in_mask, void *stream);
HM_API int64_t hm_mesh_depth_workspace_bytes(int64_t n_verts, int64_t n_faces);
HM_API int hm_mesh_depth_maps(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                              const double *proj, int64_t n_views, int64_t H, int64_t W, int64_t big_face, float *depth,
                              int32_t *n_skipped, void *workspace, int64_t workspace_bytes, int32_t *status,
                              void *stream);
HM_API int hm_mesh_visible_votes(const float *verts, int64_t n_verts, const double *proj, int64_t n_views,
                                 const float *depth, int64_t H, int64_t W, int64_t pad, float tol, int accumulate,
                                 int32_t *n_visible, void *stream);
HM_API int hm_mesh_keep_mark(const int32_t *faces, int64_t n_faces, int64_t n_verts, const uint8_t *keep,
                             int32_t *vflag, int32_t *fflag, int32_t *status, void *stream);

/* ---- mesh colouring: per-vertex colour from the views that see the vertex ------------------------------------------
 * Driver: ops.mesh_vertex_colors, ops.mesh_colors_finish, evaluation.color.color_mesh.  csrc/hm_mesh_color.hip,
 * csrc/hm_view_dev.h.  Does not synchronise; sizes, proj, the projection and the pixel as for mesh culling above.
 *   hm_mesh_vertex_colors: verts [n_verts, 3] fp32; normals [n_verts, 3] fp32 or NULL; centers [n_views, 3] fp64 the
 *                camera centres (pose[:, :3, 3]); images [n_views, H, W, 3] fp32; depth [n_views, H, W] fp32 from
 *                hm_mesh_depth_maps; sat [n_views, H+1, W+1] int32 the masks' summed-area table or NULL.
 *                One lane per vertex visits the views in ascending order.  A view contributes iff, tested in this order,
 *                  1. the vertex is projectable and its pixel (col, row) is in the image;
 *                  2. float(w) <= m + tol, the rule of hm_mesh_visible_votes with the same pad in [0, 64];
 *                  3. (with sat) every pixel of the (2 erode + 1)^2 square around (col, row) inside the image is set:
 *                     the window's count from four table reads equals the clamped window's area; erode in [0, 65536];
 *                  4. (with normals) d = c - double(x) per component, dot = ((nx dx) + (ny dy)) + (nz dz), nn and dd
 *                     the squared lengths of the normal and of d in the same association, den = sqrt(nn dd),
 *                     cos = dot / den; den > 0, cos finite and cos > min_cos; min_cos in [0, 1).
 *                Weight: w = 1 without normals, else cos^power as `power` products from 1.0, left to right; power in
 *                [0, 8].  Sample: bilinear at (u, v): c0 = floor(u), r0 = floor(v), fu = u - c0, fv = v - r0, the tap
 *                indices c0, c0 + 1, r0, r0 + 1 clamped to the image; per channel top = (a (1 - fu)) + (b fu), bot
 *                likewise, val = (top (1 - fv)) + (bot fv).  Every operation is fp64 and rounded once.
 *                mode 0 (blend): acc[k] += w val[k] (k < 3), acc[3] += w, sequentially in view order.
 *                mode 1 (best): a view replaces (val, w) iff w > acc[3]: of equal weights the lowest view stays.
 *                acc [n_verts, 4] fp64, n_used [n_verts] int32 = the contributing views.  accumulate == 0 starts from
 *                zeros, else from what acc and n_used hold: views [0, n) in one call and [0, k), [k, n) in two give the
 *                same bits.  No atomics, no workspace.  n_views == 0 writes zeros (accumulate == 0) or nothing. */
HM_API int hm_mesh_vertex_colors(const float *verts, const float *normals, int64_t n_verts, const double *proj,
                                 const double *centers, const float *images, const float *depth, const int32_t *sat,
                                 int64_t n_views, int64_t H, int64_t W, int64_t pad, float tol, int64_t erode,
                                 double min_cos, int power, int mode, int accumulate, double *acc, int32_t *n_used,
                                 void *stream);

/* ---- mesh rendering: a visibility buffer of the mesh per view, resolved with interpolated vertex attributes ---------
 * Driver: ops.mesh_render, evaluation.mesh_views.  csrc/hm_mesh_render.hip, csrc/hm_raster_dev.h.  Does not
 * synchronise; sizes, proj, the projection, the fixed-point position, the skipped faces, coverage, b_a, iw_a and the
 * depth z of a covered pixel as for hm_mesh_depth_maps above (the same device functions).
 *   hm_mesh_render: per view, every pixel starts with the 64-bit key of all ones; a covered pixel whose z is finite and
 *                > 0 takes key = min(key, (uint64(float_bits(z)) << 32) | uint32(face)) by an unsigned 64-bit atomic
 *                minimum: the nearest sample and, among equal depths, the smallest face index, independent of the order
 *                of the faces.  Then, per pixel (written once, no atomics): an all-ones key gives face_id = -1,
 *                depth = +inf, weights = 0, image = background; any other key gives face_id = its low word, depth = its
 *                high word as a float, and with that face's corners m = 0, 1, 2:
 *                  t_m = b_m * iw_m,  s = (t_0 + t_1) + t_2,  weights[m] = float(t_m / s),
 *                  image[c] = float((((t_0 * a_0c) + (t_1 * a_1c)) + (t_2 * a_2c)) / s),  a_mc = double(attrs[v_m][c]),
 *                every operation fp64 and rounded once, in this order; a NaN attribute propagates.
 *                attrs [n_verts, n_attr] fp32 with n_attr in [0, 16], or NULL; background [n_attr] fp32 on the HOST
 *                (read before the launches) or NULL for zeros; face_id [n_views, H, W] int32; depth [n_views, H, W]
 *                fp32; weights [n_views, H, W, 3] fp32 or NULL; image [n_views, H, W, n_attr] fp32, NULL iff attrs is;
 *                n_skipped [n_views] int32.  A face whose clamped box has more than big_face (>= 1) pixels is drawn by
 *                one wave, any other by one lane.  A face index outside [0, n_verts) sets bit 0 of status [1] int32
 *                and is never dereferenced.  No clipping, no anti-aliasing, no lighting.
 *                workspace: hm_mesh_render_workspace_bytes(n_verts, n_faces, H, W) bytes, reused view after view. */
HM_API int64_t hm_mesh_render_workspace_bytes(int64_t n_verts, int64_t n_faces, int64_t H, int64_t W);
HM_API int hm_mesh_render(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                          const double *proj, int64_t n_views, int64_t H, int64_t W, int64_t big_face,
                          const float *attrs, int64_t n_attr, const float *background, int32_t *face_id, float *depth,
                          float *weights, float *image, int32_t *n_skipped, void *workspace, int64_t workspace_bytes,
                          int32_t *status, void *stream);

/* ---- point-to-mesh distance: the exact closest point of a triangle mesh on a uniform grid ------------------------
 * For a query point the nearest point of the mesh, the face it lies on, the face's feature and the squared distance.
 * Driver: ops.mesh_index, ops.mesh_closest_point, ops.point_mesh_distance, evaluation.chamfer.mesh_to_mesh and
 * mesh_chamfer(surface=True).  csrc/hm_mesh_dist.hip (it states the stopping rule of the search).  No entry point
 * synchronises, none uses floating-point atomics, no atomic decides a position.  status is one device int32 the CALLER
 * has zeroed.  The grid (lo, h, g) is hm_nn_build's above.
 *
 * THE DEFINITION.  The result is the brute-force fp32 argmin of the following, bit for bit, whatever the grid,
 * big_face, m and the thread order.  Every fp32 operation rounds once (no fused multiply-add);
 * dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z; cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x).
 * For a query q and a face with fp32 vertices a, b, c: lo, hi are the face's per-axis bounding box,
 * clamp(p) = min(max(p, lo), hi) per axis (min and max return the other operand for a NaN, so clamp(p) is always in
 * the box), d2_to(p) = dot(q - clamp(p), q - clamp(p)).  The face's value is the first minimum, in this order, of
 *   candidate 0, the interior: n = cross(b - a, c - a), nn = dot(n, n), wa = a - q, wb = b - q, wc = c - q; it exists
 *       iff nn > 0 and dot(n, cross(wa, wb)) >= 0 and dot(n, cross(wb, wc)) >= 0 and dot(n, cross(wc, wa)) >= 0; its
 *       point is q + (dot(wa, n) / nn) * n;
 *   candidates 1, 2, 3, the segments (a, b), (b, c), (c, a): for (p0, p1), e = p1 - p0, ee = dot(e, e),
 *       t = ee > 0 ? dot(q - p0, e) / ee : 0, clamped to [0, 1]; its point is p0 + t*e;
 * each with the value d2_to(point).  The face's closest point is the CLAMPED point of the winning candidate, its
 * feature the candidate's number.  Over the mesh the result is the minimum d2 and, among equal d2, the lowest face
 * index.  A segment always exists, so a zero-area face, a repeated vertex and a sliver all have a finite value.
 *   hm_mesh_dist_workspace_bytes(n): the scratch of hm_mesh_dist_build over n pairs, and of hm_mesh_dist_query over
 *                n queries.
 *   hm_mesh_dist_count: per face, its cell box (the cells of lo and of hi per axis) and count [n_faces] int32 = the
 *                number of cells in it - unless that exceeds big_face (>= 1): then count = 0 and big [n_faces] int32
 *                = 1 (else 0).  A face index outside [0, n_verts) sets status bit 0, a non-finite vertex of a face
 *                bit 1; such a face gets count 0, big 0, and no vertex is read through an unchecked index.
 *   hm_mesh_dist_build: prefix, big_prefix [n_faces] int32 = the exclusive prefix sums of count and big, n_pairs and
 *                n_big their totals (n_pairs + n_big in [1, 2^31)).  Writes the (cell key, face) pairs in ascending
 *                face order, sorts them with the library's stable sort, and writes records [n_pairs + n_big, 12] fp32:
 *                record r = ax ay az bx by bz cx cy cz, the face index as the int32 bits of word 9, two zero words -
 *                first the pairs in sorted order (ascending face inside a cell), then the big faces, ascending; and
 *                cell_start [cells + 1] int32 (the records of cell c are [cell_start[c], cell_start[c+1])).  Every
 *                store is checked against n_pairs and n_big.
 *   hm_mesh_dist_query: query [m,3] fp32, m >= 0.  Writes d2 [m] fp32 and face [m] int32 and, unless NULL,
 *                point [m,3] fp32 and feature [m] int32 (0 interior, 1..3 the segments).  max_dist2 (fp32, +inf =
 *                none): a query whose minimum is > max_dist2 gets d2 +inf, face -1, a NaN point and feature -1;
 *                == max_dist2 is reported.  A non-finite query coordinate sets status bit 2.  n_tests (may be NULL;
 *                a measurement aid): a device counter the caller has zeroed, receives the number of (query lane,
 *                face record) pairs the launch visited; a pair whose face's bounding box is farther than the lane's
 *                best is rejected after the box test, which cannot change the result (csrc/hm_mesh_dist.hip). */
HM_API int64_t hm_mesh_dist_workspace_bytes(int64_t n);
HM_API int hm_mesh_dist_count(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                              const float *lo, float h, const int32_t *g, int64_t big_face, int32_t *count,
                              int32_t *big, int32_t *status, void *stream);
HM_API int hm_mesh_dist_build(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                              const float *lo, float h, const int32_t *g, const int32_t *count, const int32_t *big,
                              const int32_t *prefix, int64_t n_pairs, const int32_t *big_prefix, int64_t n_big,
                              int32_t *cell_start, float *records, void *workspace, int64_t workspace_bytes,
                              void *stream);
HM_API int hm_mesh_dist_query(const float *query, int64_t m, const float *records, int64_t n_pairs, int64_t n_big,
                              const int32_t *cell_start, const float *lo, float h, const int32_t *g, float max_dist2,
                              float *d2, int32_t *face, float *point, int32_t *feature, void *workspace,
                              int64_t workspace_bytes, int32_t *status, uint64_t *n_tests, void *stream);

/* ---- rays against the mesh: the first hit of a ray on the triangle grid ------------------------------------------
 * For a ray (o, d, t_min, t_max) the nearest face it meets, the ray parameter t (a Euclidean distance when d has unit
 * length), the barycentric (u, v) and the hit point.  Driver: ops.mesh_index(pad=...).ray_cast, ops.mesh_ray_cast,
 * evaluation.mesh_rays.cast_camera_rays.  csrc/hm_mesh_ray.hip (it states why the walk over the grid is exact).  No
 * entry point synchronises, none uses floating-point atomics.  status is one device int32 the CALLER has zeroed.
 *
 * THE PADDED INDEX.  hm_mesh_index_count / hm_mesh_index_build are hm_mesh_dist_count / hm_mesh_dist_build with a
 * pad (fp32, finite, >= 0): a face is listed in the cells of fl(min - pad) .. fl(max + pad) per axis instead of its
 * bounding box's.  pad = 0 gives the same counts, pairs, records and cell_start, bit for bit, and that is what the
 * hm_mesh_dist_* entry points forward.  The records do not depend on pad.  A padded index lists a superset of the
 * cells, so hm_mesh_dist_query stays exact on it (its stopping rule needs a face to be listed in AT LEAST the cells
 * of its box).  hm_mesh_ray_cast must be given the pad its index was built with, or a smaller one.
 *
 * THE DEFINITION.  The result is the brute-force argmin over all faces of the following, bit for bit, whatever the
 * grid, big_face, m, the ray order and the thread order.  Every fp32 operation rounds once; dot and cross are those
 * of the point-to-mesh distance above.  For a face with fp32 vertices a, b, c:
 *   lo = fl(min(a, b, c) - pad), hi = fl(max(a, b, c) + pad) per axis;
 *   e1 = b - a, e2 = c - a, pv = cross(d, e2), det = dot(e1, pv), tv = o - a, u = dot(tv, pv) / det,
 *   qv = cross(tv, e1), v = dot(d, qv) / det, t = dot(e2, qv) / det, p = fl(o + fl(t * d)) per axis;
 *   hit <=> det != 0 and u >= 0 and v >= 0 and fl(u + v) <= 1 and t_min <= t <= t_max and lo <= p <= hi on every axis.
 * Both windings hit; any NaN makes a comparison false, a miss; both range ends are inclusive and t_max = +inf is
 * allowed; a zero direction misses.  The winner is the smallest t and, among equal t, the lowest face index.  The
 * last clause ties the hit point to the face's (padded) box: it makes the grid walk provably exact and discards the
 * garbage t of slivers; with pad = 0 a face that is flat along an axis is almost never hit, so ray casting wants
 * pad > 0 (ops.mesh_ray_pad: 2^-12 of the largest extent).  pad is part of the definition.  No claim of
 * watertightness: the edge tests of neighbouring faces are separate fp32 expressions.
 *   hm_mesh_ray_cast: origins, dirs [m,3] fp32, m >= 0 (m = 0 returns at once); t_min, t_max [m] fp32, or NULL for
 *                0 and +inf.  records, n_pairs, n_big, cell_start, lo, h, g: the index.  Writes t [m] fp32 and
 *                face [m] int32 and, unless NULL, uv [m,2] fp32 and point [m,3] fp32 (= p); a miss gets +inf, -1,
 *                NaN, NaN.  A non-finite origin or direction, a non-finite t_min or a NaN t_max sets status bit 2.
 *                n_tests (may be NULL; a measurement aid): a device counter the caller has zeroed, receives the
 *                number of (ray, face record) tests.  Every index read from cell_start is clamped into
 *                [0, n_pairs]. */
HM_API int hm_mesh_index_count(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                               const float *lo, float h, const int32_t *g, float pad, int64_t big_face,
                               int32_t *count, int32_t *big, int32_t *status, void *stream);
HM_API int hm_mesh_index_build(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                               const float *lo, float h, const int32_t *g, float pad, const int32_t *count,
                               const int32_t *big, const int32_t *prefix, int64_t n_pairs, const int32_t *big_prefix,
                               int64_t n_big, int32_t *cell_start, float *records, void *workspace,
                               int64_t workspace_bytes, void *stream);
HM_API int hm_mesh_ray_cast(const float *origins, const float *dirs, const float *t_min, const float *t_max, int64_t m,
                            const float *records, int64_t n_pairs, int64_t n_big, const int32_t *cell_start,
                            const float *lo, float h, const int32_t *g, float pad, float *t, int32_t *face, float *uv,
                            float *point, int32_t *status, uint64_t *n_tests, void *stream);

/* ---- signed distance to the mesh: angle-weighted pseudo-normals and the sign of a closest-point result -----------
 * On which side of the surface a query lies, from the closest-point result above and two tables of the mesh's
 * topology (Baerentzen and Aanaes, "Signed distance computation using the angle weighted pseudonormal"): no second
 * search, no ray parity.  Driver: ops.mesh_topology, ops.MeshIndex.signed_distance, ops.mesh_signed_distance,
 * ops.mesh_contains, evaluation.mesh_sdf.  csrc/hm_mesh_topo.hip.  No entry point synchronises, none uses
 * floating-point atomics; the three counts use integer atomics.  status is one device int32 the CALLER has zeroed.
 *
 * THE DEFINITION (numpy restatement: tests/mesh_sign_cases.topology_ref, sign_ref).
 * Per-face quantities, fp64 from the fp32 vertices a, b, c, every operation rounded once, no contraction, dot and
 * cross of the shape stated for the point-to-mesh distance:
 *   n = cross(b - a, c - a);  nu = n / sqrt(dot(n, n)), the zero vector when dot(n, n) == 0;
 *   the angle at corner p with neighbours p1, p2: atan2(sqrt(dot(x, x)), dot(e1, e2)), x = cross(e1, e2), e1 = p1 - p,
 *   e2 = p2 - p (corner a: b, c; corner b: c, a; corner c: a, b).
 * VN[v], the vertex pseudo-normal: the sum of angle * nu over all (face, corner) pairs with that vertex, in ascending
 *   face, then ascending corner order, starting from 0; zero for a vertex no face names.
 * EN[f][k], the edge pseudo-normal of half-edge k of face f (k = 0, 1, 2 for (a,b), (b,c), (c,a)): the sum of nu over
 *   ALL half-edges with the same unordered vertex pair - a run - in ascending (face, k) order, starting from 0; every
 *   member of a run stores the same sum.  A boundary edge gets its own face's normal, a non-manifold edge the sum of
 *   all its faces' normals; a face with a repeated vertex contributes its half-edges like any other (its nu is zero).
 * counts: boundary_edges = runs of length 1; nonmanifold_edges = runs longer than 2; flipped_edges = runs of length 2
 *   whose two half-edges traverse the pair in the SAME direction (first index > second index for both or for
 *   neither).  The mesh is closed when all three are 0.
 * The sign of a query q with closest-point result (face, feature, point, d2), a, b, c the face's fp32 vertices:
 *   feature 0: w = q - a (fp32, rounded once, then widened), N = n of the face (fp64, not normalised);
 *   feature k in 1..3 with end points p0, p1: t as the distance definition computes it in fp32, e = p1 - p0,
 *       ee = dot(e, e), t = ee > 0 ? dot(q - p0, e) / ee : 0;  t <= 0: N = VN[index of p0];  t >= 1: N = VN[index of
 *       p1];  otherwise N = EN[face][k-1];  in all three cases w = q - point (fp32, rounded once, then widened);
 *   s = (w.x*N.x + w.y*N.y) + w.z*N.z in fp64;  sign = -1 if s < 0, else +1 (a zero or NaN s - d2 == 0, a zero
 *   pseudo-normal - is outside);  sd = sign * sqrt(d2), the fp32 square root rounded once.
 *   A query that max_dist cut (face -1) gets sd = +inf, sign = 0.
 * The magnitude is the exact d2 of the closest-point query; the sign is a function of (face, feature, point) and the
 * two tables and of nothing else.  The tables do not depend on the thread order; VN depends on the device's atan2.
 *   hm_mesh_topology_workspace_bytes(n_faces): the scratch of hm_mesh_topology_build; 3 * n_faces < 2^31.
 *   hm_mesh_topology_build: verts [n_verts,3] fp32, faces [n_faces,3] int32, n_faces >= 1.  Writes
 *                vertex_normals [n_verts,3] fp64, edge_normals [n_faces,3,3] fp64 and counts [3] int64 (boundary,
 *                non-manifold, flipped).  The corners are sorted by vertex and the half-edges by two passes (max, then
 *                min) of the library's stable sort; the lane of every run head walks its run in sorted order and
 *                writes the sum to every member.  A face index outside [0, n_verts) sets status bit 0, a non-finite
 *                vertex of a face bit 1; no vertex is read through an unchecked index, and the outputs of such a call
 *                mean nothing.
 *   hm_mesh_sign: query [m,3] fp32, and face [m] int32, feature [m] int32, point [m,3] fp32, d2 [m] fp32 as
 *                hm_mesh_dist_query wrote them for the same mesh; m >= 0 (m = 0 returns at once).  Reads the face's
 *                indices and vertices from faces / verts.  Writes sd [m] fp32 and, unless NULL, sign [m] int32.  A
 *                face outside [0, n_faces), a feature outside [0, 3] or a face index outside [0, n_verts) is treated
 *                as a cut query. */
HM_API int64_t hm_mesh_topology_workspace_bytes(int64_t n_faces);
HM_API int hm_mesh_topology_build(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                                  double *vertex_normals, double *edge_normals, int64_t *counts, void *workspace,
                                  int64_t workspace_bytes, int32_t *status, void *stream);
HM_API int hm_mesh_sign(const float *query, int64_t m, const int32_t *face, const int32_t *feature, const float *point,
                        const float *d2, const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                        const double *vertex_normals, const double *edge_normals, float *sd, int32_t *sign,
                        void *stream);

/* ---- mesh texturing: a per-face texture atlas, its texels' points on the faces and its sampler -------------------
 * Driver: ops.mesh_texture_points, ops.mesh_texture_sample, ops.TextureAtlas, evaluation.texture.texture_mesh,
 * evaluation.mesh_views.render_mesh(texture=).  csrc/hm_mesh_texture.hip, csrc/hm_color_dev.h.  No entry point
 * synchronises; no atomics but the status word's, no workspace; two calls give the same bits.  status is one device
 * int32 the CALLER has zeroed.  Numpy restatement: tests/mesh_texture_cases.py.
 *
 * THE ATLAS.  n = res in [1, 4096] texel steps along a face edge, the same for every face.  Faces are packed two per
 * block: block b holds face 2b (lower) and face 2b + 1 (upper; absent in the last block of an odd face count);
 * n_blocks = (n_faces + 1) / 2 and n_blocks Hb Wb < 2^40.  A block is Wb = n + 3 texels wide and Hb = n + 2 high.
 * Texel (i, j) = (column, row) belongs to the lower face iff i + j <= n + 1, else to the upper face, which uses the
 * point-mirrored coordinates (i', j') = (n + 2 - i, n + 1 - j) and then the lower face's rule:
 *   the lower face's corners A, B, C sit at the texel centres (0, 0), (n, 0), (0, n); its texels with i + j = n + 1
 *   are its gutter.  Barycentric numerators (exact small integers): i + j <= n: S = 2i, T = 2j; otherwise
 *   S = clamp(2i - 1, 0, 2n), T = 2n - S, the nearest point of the hypotenuse.  b1 = S / 2n, b2 = T / 2n,
 *   b0 = (2n - S - T) / 2n, one fp64 division each.
 * Texel point: p_c = float(((b0 A_c) + (b1 B_c)) + (b2 C_c)), fp64 operations on the fp32 corners, each rounded
 * once, in this order; texel normal: the same expression over the corners' vertex normals, NOT normalised.
 * Storage is block-major: texel t = (b Hb + j) Wb + i.
 *   hm_mesh_texture_points: verts [n_verts, 3] fp32; normals [n_verts, 3] fp32 or NULL; faces [n_faces, 3] int32.
 *                Writes points [T, 3] fp32, tex_normals [T, 3] fp32 (NULL iff normals is) and face [T] int32,
 *                T = n_blocks Hb Wb; one lane per texel.  A texel of the absent face gets face = -1 and NaN point and
 *                normal: hm_mesh_vertex_colors cannot project it, so it collects nothing.  A face index outside
 *                [0, n_verts) sets bit 0 of status and is never dereferenced (its texels are written as absent).
 *   hm_mesh_texture_sample: texels [n_blocks, Hb, Wb, 3] fp32; face_id [n_samples] int32 and weights [n_samples, 3]
 *                fp32 as hm_mesh_render writes them; background [3] fp32 on the HOST (read before the launch) or NULL
 *                for zeros.  Writes out [n_samples, 3] fp32; one lane per sample:
 *                  1. face_id < 0 or a non-finite weight gives background;
 *                  2. face_id >= n_faces sets bit 0 of status (and gives background; nothing is read);
 *                  3. s = w1 n, t = w2 n in fp64 (w1, w2 = weights[1], weights[2] widened);
 *                  4. lower face (even): (px, py) = (s, t); upper face (odd): (px, py) = ((n + 2) - s, (n + 1) - t);
 *                  5. px is clamped to [0, Wb - 1] and py to [0, Hb - 1] as doubles, before any integer is formed;
 *                  6. the taps are x0 = floor(px), x1 = min(x0 + 1, Wb - 1), fx = px - x0, and y likewise;
 *                  7. per channel top = (a (1 - fx)) + (b fx) over row y0, bot likewise over row y1,
 *                     val = (top (1 - fy)) + (bot fy); every operation fp64 and rounded once; out = float(val).
 *                Weights exactly at a corner return that corner's texel; a point inside a face reads no texel of the
 *                other face with a weight above rounding. */
HM_API int hm_mesh_texture_points(const float *verts, const float *normals, int64_t n_verts, const int32_t *faces,
                                  int64_t n_faces, int64_t res, float *points, float *tex_normals, int32_t *face,
                                  int32_t *status, void *stream);
HM_API int hm_mesh_texture_sample(const float *texels, int64_t res, int64_t n_faces, const int32_t *face_id,
                                  const float *weights, int64_t n_samples, const float *background, float *out,
                                  int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HASHMOD_H */
