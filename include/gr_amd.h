/*
 * gr_amd.h — C ABI of the MI355X (gfx950) hot-path library libgr_amd.so.
 *
 * The reference (CatchMan1/AI-education-generative-recommendation) has no native layer: its hot
 * paths are sequences of ATen ops inside two nn.Modules.  This ABI is what those modules' methods
 * bottom out in here; each entry point names the reference code it replaces (paths relative to the
 * reference root).  The Python drop-in modules (RQVAE, SASRec) bind these through ctypes.
 *
 * Conventions
 *  - Every pointer argument named x/w/z/... is a DEVICE pointer to contiguous row-major data in the
 *    layout PyTorch uses (nn.Linear weight = [out, in], nn.Embedding weight = [rows, dim]).
 *    Arguments documented as "host array" are host arrays OF device pointers / sizes.
 *  - All work is enqueued on `stream` (a hipStream_t; NULL = the default stream).  No call
 *    synchronises, allocates or frees device memory: scratch comes from the caller's workspace
 *    (size from the matching *_workspace_bytes query).  Calls are reentrant and stateless.
 *  - Return 0 (GR_OK) on success, a negative GR_ERR_* code otherwise; gr_last_error() returns a
 *    thread-local message for the last failure on the calling thread.  No exceptions cross the ABI.
 *  - Floating point is fp32 throughout (f32-input MFMA, f32 accumulate); indices are int64.
 */
#ifndef GR_AMD_H
#define GR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_OK 0
#define GR_ERR_ARG (-1)          /* bad shape / null pointer / misalignment                   */
#define GR_ERR_UNSUPPORTED (-2)  /* shape outside what the kernels are built for               */
#define GR_ERR_HIP (-3)          /* a HIP runtime error at launch                              */
#define GR_ERR_WORKSPACE (-4)    /* workspace too small                                        */

#define GR_MAX_LEVELS 8          /* RQ levels supported by one gr_rq_* call                    */
#define GR_MAX_LINEAR 8          /* encoder Linear layers supported by gr_rq_encode_f32        */

#define GR_ACT_NONE 0
#define GR_ACT_RELU 1
#define GR_ACT_SIGMOID 2         /* the activations of RQ-VAE/models/layers.py:45-67 besides   */
#define GR_ACT_TANH 3            /* ReLU (nn.Sigmoid / nn.Tanh / nn.LeakyReLU(0.01)); gr_linear */
#define GR_ACT_LEAKYRELU 4       /* only, without a residual                                     */

/* Library identification ("gr_amd <version> gfx950"). */
const char* gr_version(void);
/* Message of the last failed call on this thread ("" if none). */
const char* gr_last_error(void);
/* Process-wide path switches (no reference counterpart).  Each selects between two kernel paths
 * that give BITWISE identical results, so the tests can run both; no option changes numerics, and
 * the defaults are what every caller wants.  (Round 5 removed the A/B knobs of slower variants and
 * the two numerics-changing ones: which form the final SASRec block of a last-position forward
 * runs follows from the shape alone, see below.)
 *   "rq_fused"      1 (default): gr_rq_encode_f32 runs the fused persistent kernel when the encoder
 *                   shape is in -> 256 -> 128 -> 32; 0: the layer-wise path (exact gr_linear +
 *                   quantize).
 *   "sas_fused"     2 (default): gr_sasrec_forward_f32 / gr_sasrec_predict_f32 run the fused
 *                   register-resident forward kernel when n <= 64, d <= 64 (d and the head width
 *                   multiples of 8), mlp <= 128, num_blocks <= 8: one wave per sequence, or two
 *                   (one per 32-token tile) when n > 32 and the batch size favours it; 3: two
 *                   waves whenever n > 32; 1: always one; 0: the layer-wise pipeline (the
 *                   workspace query follows the option in force when it is called).  The fused
 *                   forms give bitwise the same results.
 *   "sas_rowtile"   1 (default): d = 128 forwards on the row-tile kernels; 0: one kernel per op.
 *   "lin_wres"      1 (default): gr_linear_f32 with k = 128, n % 128 == 0, no residual and
 *                   m >= 96 x 256 runs a persistent kernel that keeps each wave's 32 columns of w in
 *                   registers (the C5 block-0 in-projection); 0: the tiled kernel.
 *   "emb_proj"      1 (default): the d = 128 forward's block 0 (embedding gather + LN_a0 +
 *                   in-projection) runs as one persistent kernel with W_in in registers; 0: the
 *                   embed_ln kernel then gr_linear_f32.
 *   "topk_half"     2 (default): gr_score_topk_f32's tile pass records the max of every 16-row
 *                   half tile when the catalog is below ~3,700 64-row chunks per 128 features (the
 *                   select kernel then re-scores half as many rows), else of every 32-row tile;
 *                   1: always half tiles; 0: never.
 *   "attn_k16"      1 (default): head width 128 attention on 32-query tiles over 16-key steps at
 *                   two waves per SIMD; 0: 32 x 32 steps at one wave per SIMD.  Different fp32
 *                   chains of the same attention (both within the logits tolerance).
 *   "rq_filter"     1 (default): index-only quantize calls (gr_rq_quantize_f32 and the encode entry
 *                   points with best_out = gap_out = NULL) at e_dim 32 and at most 1024 codes per
 *                   level run the filtered kernel: a split-bf16 pass bounds every distance, and the
 *                   exact fp32 formula runs only on the codes within the bound of the minimum;
 *                   0: every distance exact.  The IDs are bitwise the same, exact ties included.
 *   "kmeans_small"  1 (default): gr_kmeans_f32 runs the whole k-means in one launch of one
 *                   workgroup when n <= 256, n K e <= 2^20 (e padded) and the rows and
 *                   the workspace fit in LDS; 0: always one launch per phase over row tiles.  Both forms
 *                   run the same phase code in the same order: bitwise the same results.
 *   "rq_tail_merge" 1 (default): an encode call (gr_rq_encode_f32 / gr_rq_encode_packed_f32) that
 *                   runs the fused encoder with leftover tiles and the filtered quantizer is two
 *                   launches: the quantizer's workgroups finish the leftover tiles' layers 2-3
 *                   themselves before they quantize them; 0: rq_leftover_kernel runs between the two
 *                   (three launches).  z and the IDs are bitwise the same.
 *   "bert_tile"     0 (default): each GEMM of gr_bert_embed_f32 takes, of 128 x 128, 64 x 128 and
 *                   128 x 96 outputs per workgroup, the tile that leaves the fewest compute units idle at
 *                   its shape; 1 / 2 / 3: that tile on every GEMM.  One summation order: bitwise the
 *                   same results.  The bf16 entries' GEMMs take the same tiles the same way.
 * The final block of a last-position forward (predict, last_hidden; gr_sasrec_plan reports the
 * choice): the H form when the tail kernel takes the shape (d / 4, head width / 4 and mlp / 4 powers
 * of two, at most 8 heads, d and mlp <= 256, 16-byte aligned weights); otherwise the pruned final
 * block (attention on the last query tile, the rest on the B last rows) when n >= 2 and
 * n * mlp >= 2 d + mlp; otherwise the full block.  The H form is the one-query tail on
 * LN_a(X): q . K_j = (W_k^T q) . H_j (+ a term constant over j that cancels in the softmax) and
 * p . V = W_v (p . H) + b_v, so K|V of the B n rows are never projected (sas_tail_h2_kernel; the
 * fused d <= 64 kernel likewise).  The reassociated sums round differently from the reference
 * formulation: logits within the 1e-5 row-scaled tolerance (tests/test_sasrec_gpu.py::
 * test_tail_h_form_vs_full_block_and_oracle).
 * gr_set_option returns GR_ERR_ARG for an unknown name/value; gr_get_option returns -1 for an
 * unknown name. */
int gr_set_option(const char* name, int64_t value);
int64_t gr_get_option(const char* name);

/* ------------------------------------------------------------------------------------------ */
/* Dense layer  y[m, n] = act(x[m, k] . w[n, k]^T + bias[n]) (+ residual[m, n])
 * Replaces nn.Linear -> F.linear -> addmm (+ nn.ReLU): RQ-VAE/models/layers.py:23-30 (encoder),
 * SASRec/model.py:37-45 (FFN), torch functional.py:5785-5830 / :6600 (MHA in/out projections) and
 * SASRec/model.py:107 (scoring: w = item table, bias = NULL).
 * bias, residual may be NULL.  `residual` may alias `y` (in-place residual add).  act: GR_ACT_*
 * (SIGMOID / TANH / LEAKYRELU only with residual = NULL).
 * Requires k % 4 == 0 and 16-byte aligned x, w.  ldy / ldr are row strides (elements) of y / residual. */
int gr_linear_f32(const float* x, int64_t m, int32_t k, const float* w, int32_t n,
                  const float* bias, const float* residual, int64_t ldr, int32_t act,
                  float* y, int64_t ldy, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* RQ-VAE encode.
 * Squared norms of codebook rows, cn[c] = sum_k C[c,k]^2 (the `torch.sum(self.embedding.weight**2,
 * dim=1)` term of RQ-VAE/models/vq.py:72), computed once per codebook. */
int gr_rq_codebook_norms_f32(const float* codebook, int32_t K, int32_t e, float* cn_out, void* stream);

/* Residual quantization of latents z[n, e] over L levels (RQ-VAE/models/rq.py:39-56 with
 * VectorQuantizer.forward(use_sk=False), vq.py:63-99):
 *   d = (||r||^2 + ||C_l||^2) - 2 r.C_l^T ;  idx = first argmin ;  r <- r - (r + (C_l[idx] - r))
 * Every fp32 rounding is the reference's CPU one (r.C: one fma chain over k in order, as MKL's
 * sgemm at K = e; the squared norms in ATen's vectorised row-sum order; oracle/rq_exact.c), so
 * idx_out equals the reference's, exact ties included.
 * K, codebooks: host arrays of length L.  code_norms: accepted for ABI stability and ignored (may be
 * NULL); the kernel recomputes each code's norm from its LDS copy of the codebook.
 * idx_out[n, L] int64 row-major (the stacked `indices` of rq.py:54).
 * best_out[n, L], gap_out[n, L] (optional, may be NULL): the best fp32 distance and the gap to the
 * second best per level.
 * Supports 1 <= e <= 4096 (e > 64 and one-row calls on the per-row kernel), 1 <= L <= GR_MAX_LEVELS,
 * any K >= 1; z and the codebooks must be 16-byte aligned when e is 16, 32 or 64. */
int gr_rq_quantize_f32(const float* z, int64_t n, int32_t e, int32_t L, const int32_t* K,
                       const float* const* codebooks, const float* const* code_norms,
                       int64_t* idx_out, float* best_out, float* gap_out, void* stream);

/* Workspace for gr_rq_encode_f32 (bytes).  dims: host array of n_linear+1 layer widths
 * (in_dim, hidden..., e_dim) = RQVAE.encode_layer_dims (RQ-VAE/models/rqvae.py:45). */
size_t gr_rq_encode_workspace_bytes(int64_t n, int32_t n_linear, const int32_t* dims,
                                    int32_t L, const int32_t* K);

/* RQVAE.get_indices(xs, use_sk=False) (RQ-VAE/models/rqvae.py:67-71): encoder MLP
 * (layers.py:42-43; ReLU after every Linear but the last) followed by gr_rq_quantize_f32.
 * The encoder and the quantizer's r . c reproduce the reference's CPU sgemm order for a call of n
 * rows (gr_mkl_plan: k-block chains of >= 16-row calls on the MFMA kernels, the one-row and 2-15-row
 * 16-lane orders on a per-row kernel; widths whose order is not pinned, in_features % 4 != 0 and
 * e_dim > 64 also run there); any width is accepted. 
 * weights/biases: host arrays (n_linear) of device pointers; codebooks, K: host arrays (L).
 * best_out, gap_out: as gr_rq_quantize_f32 (optional).
 * z_out (optional, may be NULL): the encoder output [n, e]. */
int gr_rq_encode_f32(const float* x, int64_t n, int32_t n_linear, const int32_t* dims,
                     const float* const* weights, const float* const* biases, int32_t L,
                     const int32_t* K, const float* const* codebooks, int64_t* idx_out,
                     float* best_out, float* gap_out, float* z_out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The fused encoder's packed weight image (in -> 256 -> 128 -> 32 encoders; 0 floats otherwise):
 * W1 / W2 with every 32-deep k group in the order the 32x32x2 MFMA chains consume (feature
 * 8j + 2s + h at 16h + 4j + s), W3 in the 16x16x4 chain's (feature 4t + g of a 16-block at 4g + t).
 * gr_rq_encode_f32 writes it into its workspace on every call; a caller that keeps the weights
 * fixed between calls packs once (gr_rq_encoder_pack_f32, `packed` 16-byte aligned) and passes it
 * to gr_rq_encode_packed_f32 (same arguments as gr_rq_encode_f32 otherwise; packed = NULL: pack
 * per call), which saves a launch per call. */
size_t gr_rq_encoder_pack_floats(int32_t n_linear, const int32_t* dims);
int gr_rq_encoder_pack_f32(int32_t n_linear, const int32_t* dims, const float* const* weights,
                           float* packed, void* stream);
int gr_rq_encode_packed_f32(const float* x, int64_t n, int32_t n_linear, const int32_t* dims,
                            const float* const* weights, const float* const* biases,
                            const float* packed, int32_t L, const int32_t* K,
                            const float* const* codebooks, int64_t* idx_out, float* best_out,
                            float* gap_out, float* z_out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* The filtered quantizer's packed codebook image (e_dim 32, every K <= 1024; 0 floats otherwise): per
 * level exactly what the kernel's LDS holds after it has staged that level -- the split-bf16 image
 * (hi = rne(c), lo = rne(c - hi), one swizzled 128-byte row per code), the ATen-order norms (+inf past
 * K up to the rows the kernel sweeps), the level's largest norm, and the swizzled fp32 image when the
 * levels have at most 512 codes.  A caller that keeps the codebooks fixed between calls packs once
 * (gr_rq_codebook_pack_f32, `image` 16-byte aligned, gr_rq_codebook_image_floats floats) and passes
 * the image to gr_rq_encode_image_f32 (gr_rq_encode_packed_f32's arguments plus cb_image): the kernel
 * then stages a level by a straight copy.  cb_image = NULL, and every call the filtered kernel does not
 * take: the images are derived from `codebooks` in-kernel.  The image must have been packed from the
 * same K and the codebooks' current values; the IDs are bitwise the same either way. */
size_t gr_rq_codebook_image_floats(int32_t e, int32_t L, const int32_t* K);
int gr_rq_codebook_pack_f32(int32_t e, int32_t L, const int32_t* K, const float* const* codebooks,
                            float* image, void* stream);
int gr_rq_encode_image_f32(const float* x, int64_t n, int32_t n_linear, const int32_t* dims,
                           const float* const* weights, const float* const* biases,
                           const float* packed, int32_t L, const int32_t* K,
                           const float* const* codebooks, const float* cb_image, int64_t* idx_out,
                           float* best_out, float* gap_out, float* z_out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* MLPLayers.forward in eval mode (RQ-VAE/models/layers.py:42-43): z_out[n, dims[n_linear]] = the
 * encoder output alone (ReLU after every Linear but the last).  Same kernels as gr_rq_encode_f32. */
size_t gr_rq_mlp_workspace_bytes(int64_t n, int32_t n_linear, const int32_t* dims);
int gr_rq_mlp_f32(const float* x, int64_t n, int32_t n_linear, const int32_t* dims,
                  const float* const* weights, const float* const* biases, float* z_out,
                  void* workspace, size_t workspace_bytes, void* stream);

/* MLPLayers.forward in eval mode with the general layer options of RQ-VAE/models/layers.py:18-43,
 * in the reference's exact CPU order: per layer Linear, then (all but the last) an eval
 * BatchNorm1d when bn_mean / bn_var are given (host arrays of n_linear - 1 device pointers; bn_w /
 * bn_b may be NULL arrays = affine off; torch's CPU formula a = w / sqrt(var + eps),
 * y = fma(y, a, fma(-mean, a, b))) and act (GR_ACT_RELU / GR_ACT_LEAKYRELU / GR_ACT_NONE).
 * Workspace: gr_rq_mlp_workspace_bytes. */
int gr_mlp_exact_f32(const float* x, int64_t n, int32_t n_linear, const int32_t* dims,
                     const float* const* weights, const float* const* biases,
                     const float* const* bn_mean, const float* const* bn_var,
                     const float* const* bn_w, const float* const* bn_b, float bn_eps,
                     int32_t act, float* z_out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* MLPLayers.forward (eval) for consecutive row groups, each ONE reference call with its own MKL
 * accumulation order (the call's row count selects it, see gr_mkl_plan): the encoder half of
 * RQVAE.get_indices(group, use_sk=True) per collision group (RQ-VAE/infer.py:116-127).  group_ptr:
 * device int64 [n_groups + 1] offsets as gr_rq_encode_sk_f32.  Other arguments as gr_mlp_exact_f32
 * (no workspace). */
int gr_mlp_exact_groups_f32(const float* x, int64_t n, int32_t n_linear, const int32_t* dims,
                            const float* const* weights, const float* const* biases,
                            const float* const* bn_mean, const float* const* bn_var,
                            const float* const* bn_w, const float* const* bn_b, float bn_eps,
                            int32_t act, const int64_t* group_ptr, int64_t n_groups, float* z_out,
                            void* stream);

/* The accumulation order the reference's CPU sgemm (torch 2.10 / MKL 2024.2, 8 threads, AVX-512:
 * the golden-fixture host) uses for ONE call of M rows, inner size K, N outputs -- nn.Linear
 * (RQ-VAE/models/layers.py:23) and the quantizer's matmul (vq.py:73, K = e_dim, N = codebook size):
 *   *kind 0 = k-block chain of width *kb, 1 = one-row 16-lane gemv, 2 = 2-15-row 16-lane small
 * kernel (oracle/rq_exact.c rqx_plan).  Every gr_rq_* / gr_mlp_* entry point computes each call in
 * this order.  Returns 1 when (M, K, N) lies in the envelope checked bit for bit against torch on
 * that host, 0 outside it (the order is then mkl_plan's best restatement, parity unpinned). */
int32_t gr_mkl_plan(int64_t M, int32_t K, int32_t N, int32_t* kind, int32_t* kb);

/* The filtered quantizer ("rq_filter").  gr_rq_filter_bound_f32: the bound E the kernel uses, from
 * an item's |r|^2 and the level's largest |c|^2 (host arithmetic, no device): the split-bf16 value
 * a_k = |c_k|^2 - 2 r.c_k is within E of the exact kernel's distance minus |r|^2, and every code with
 * a_k <= min a + 2E is re-scored exactly.  gr_rq_filter_launches: launches of the filtered kernel by
 * this process so far.  gr_rq_filter_diag_counts: a device buffer [n][L] (uint32) that diagnostic
 * builds (-DGR_FDIAG=3) fill with the number of codes re-scored per item and level; NULL: none.
 * gr_rq_leftover_launches: launches of rq_leftover_kernel (the fused encoder's leftover tiles as a
 * launch of their own: every caller but the merged encode path of "rq_tail_merge") so far.
 * gr_rq_filter_plan: the filtered kernel's tile plan (host arithmetic, no device) for `tiles` 32-item
 * tiles whose last `left` are pending leftover tiles, from grid_in workgroups: *grid_out workgroups
 * (grid_in, or more while one would exceed its 16 register-resident tiles), workgroup b taking main
 * tiles [begins_out[b], begins_out[b] + counts_out[b] - (b < left)) plus, when b < left, leftover
 * tile tiles - left + b, counts_out[b] tiles in all.  begins_out / counts_out: *grid_out entries
 * (at most max(grid_in, tiles)), or NULL.  GR_ERR_UNSUPPORTED when left exceeds the grid or tiles. */
float gr_rq_filter_bound_f32(float rn, float cmax2);
int64_t gr_rq_filter_launches(void);
void gr_rq_filter_diag_counts(uint32_t* counts);
int64_t gr_rq_leftover_launches(void);
int gr_rq_filter_plan(int64_t tiles, int32_t grid_in, int32_t left, int32_t* begins_out, int32_t* counts_out,
                      int32_t* grid_out);

/* MLPLayers.forward in train mode (RQ-VAE/models/layers.py:18-43, [Dropout -> Linear -> ReLU] x
 * (n_linear - 1), then Dropout -> Linear; RQVAE.forward under RQ-VAE/train.py:113).  Dropout p_drop
 * on every layer input, masks from a counter-based hash of (*seed_dev, layer, element) -- torch's
 * distribution, not its random stream (seed_dev and xd0 may be null when p_drop = 0).  Outputs:
 * xd0[M, dims[0]] = the dropped input (p_drop > 0), outs[i][M, dims[i+1]] = the next layer's dropped
 * input drop(relu(X_i W_i^T + b_i)) for i < n_linear - 1 and the MLP output for the last layer --
 * the tensors the backward reads. */
int gr_mlp_train_fwd_f32(const float* x, int64_t M, int32_t n_linear, const int32_t* dims,
                         const float* const* weights, const float* const* biases, float p_drop,
                         const uint64_t* seed_dev, float* xd0, float* const* outs, void* stream);

/* Backward of layer i of such an MLP (the autograd of layers.py's Linear / ReLU / Dropout,
 * train.py:116), one launch, on the layer's dropped input xd_in (xd0, or outs[i-1] of the forward):
 * dweight[N, K] = dz^T xd_in, dbias[N] = column sums of dz (rows in order), and (dx_out non-null)
 * dx_out[M, K] = (dz W) * mask, mask per dx_mode: 1 = (xd_in > 0 ? 1 / (1 - p) : 0) (the input came
 * through ReLU: ReLU' and dropout), 2 = the dropout hash mask of `site` (the first layer), 0 = none.
 * dz[M, N] is the gradient of this layer's pre-activation output. */
int gr_mlp_train_bwd_layer_f32(const float* xd_in, int64_t M, int32_t K, const float* weight, int32_t N,
                               const float* dz, int32_t dx_mode, float p_drop, const uint64_t* seed_dev,
                               int32_t site, float* dweight, float* dbias, float* dx_out, void* stream);

/* RQVAE.get_indices(xs, use_sk=True) over independent row groups (the collision re-encode of
 * RQ-VAE/infer.py:108-130; vq.py:52-61, 76-84; layers.py:85-108).  z[n, e]: encoder outputs (as
 * gr_rq_encode_f32's z_out), rows grouped contiguously: group g = rows [group_ptr[g],
 * group_ptr[g+1]) (device int64 array of n_groups + 1, group_ptr[0] = 0, group_ptr[n_groups] = n).
 * Each group is one reference call: a level with sk_eps[l] > 0 (host array, float64) assigns by
 * sk_iters Sinkhorn iterations over the group's [rows, K] distances (batch-coupled), a level with
 * sk_eps[l] <= 0 by the plain argmin.  idx_out[n, L] int64.  K[l] <= 1024. */
size_t gr_rq_encode_sk_workspace_bytes(int64_t n, int32_t e, int32_t L, const int32_t* K);
int gr_rq_encode_sk_f32(const float* z, int64_t n, int32_t e, int32_t L, const int32_t* K,
                        const float* const* codebooks, const double* sk_eps, int32_t sk_iters,
                        const int64_t* group_ptr, int64_t n_groups, int64_t* idx_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The quantizer's training forward (RQ-VAE/models/rq.py:39-56, vq.py:63-99 under
 * RQ-VAE/train.py:113): gr_rq_encode_sk_f32's assignment (one group per call for a training batch)
 * plus, when non-null, xq_out[n, e] = x_q = sum_l (r_l + (C_l[idx_l] - r_l)) and
 * sq_out[n, L] = sum_j (C_l[idx_l] - r_l)^2 per row and level (the mse numerators).  Same
 * workspace as gr_rq_encode_sk_f32. */
int gr_rq_quantize_sk_train_f32(const float* z, int64_t n, int32_t e, int32_t L, const int32_t* K,
                                const float* const* codebooks, const double* sk_eps, int32_t sk_iters,
                                const int64_t* group_ptr, int64_t n_groups, int64_t* idx_out,
                                float* xq_out, float* sq_out, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Its backward for rq_loss = mean_l(mse(x_q_l, r_l.detach()) + beta * mse(x_q_l.detach(), r_l))
 * (vq.py:88-92) and the straight-through x_q (vq.py:95): dz_out[n, e] = g_xq + g * beta * 2 *
 * (z - C_0[idx_0]) / (n e L) (g_xq may be null: zero), dcodebooks_out[l][K_l, e] =
 * g * 2 / (n e L) * sum over the rows assigned to each code of (C_l[k] - r_l), rows in index order
 * (deterministic).  g_rq: device float scalar, the gradient of rq_loss. */
int gr_rq_quantize_sk_train_bwd_f32(const float* z, int64_t n, int32_t e, int32_t L, const int32_t* K,
                                    const float* const* codebooks, const int64_t* idx, const float* g_xq,
                                    const float* g_rq, float beta, float* dz_out,
                                    float* const* dcodebooks_out, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* SASRec.  Parameters of one model, as device pointers to the tensors of SASRec.state_dict()
 * (SASRec/model.py:17-47).  Per-block fields are host arrays of length n_blocks.  The dead
 * W_Q/W_K/W_V projections (model.py:23-25, 63-65) do not affect any output and are not passed. */
typedef struct gr_sasrec_params {
  int32_t d;            /* hidden size                          params['d']            */
  int32_t n_blocks;     /* params['num_blocks']                                        */
  int32_t n_heads;      /* params['num_heads'] (d % n_heads == 0)                      */
  int32_t mlp;          /* params['mlp_layer']                                         */
  int32_t max_len;      /* rows of pos_emb                      params['max_len']      */
  float eps;            /* params['layernorm_eps']                                     */
  int64_t item_rows;    /* item_num + 1 (row 0 = padding)                              */
  const float* item_emb;          /* [item_rows, d]   item_emb.weight                  */
  const float* pos_emb;           /* [max_len, d]     pos_emb.weight                   */
  const float* const* attn_ln_w;  /* attention_layernorms.{i}.weight  [d]              */
  const float* const* attn_ln_b;  /* attention_layernorms.{i}.bias    [d]              */
  const float* const* in_proj_w;  /* attention_layers.{i}.in_proj_weight  [3d, d]      */
  const float* const* in_proj_b;  /* attention_layers.{i}.in_proj_bias    [3d]         */
  const float* const* out_proj_w; /* attention_layers.{i}.out_proj.weight [d, d]       */
  const float* const* out_proj_b; /* attention_layers.{i}.out_proj.bias   [d]          */
  const float* const* ffn_ln_w;   /* forward_layernorms.{i}.weight  [d]                */
  const float* const* ffn_ln_b;   /* forward_layernorms.{i}.bias    [d]                */
  const float* const* ffn1_w;     /* forward_layers.{i}.0.weight [mlp, d]              */
  const float* const* ffn1_b;     /* forward_layers.{i}.0.bias   [mlp]                 */
  const float* const* ffn2_w;     /* forward_layers.{i}.3.weight [d, mlp]              */
  const float* const* ffn2_b;     /* forward_layers.{i}.3.bias   [d]                   */
  const float* last_ln_w;         /* last_layernorm.weight [d]                         */
  const float* last_ln_b;         /* last_layernorm.bias   [d]                         */
} gr_sasrec_params;

/* Workspace (bytes) for gr_sasrec_forward_f32 / gr_sasrec_predict_f32 at batch B, length n. */
size_t gr_sasrec_workspace_bytes(const gr_sasrec_params* p, int64_t B, int32_t n);

/* SASRec.forward(log_seqs) (SASRec/model.py:49-96) in eval mode: seqs[B, n] int64 ids ->
 * out[B, n, d] (last_only = 0) or only the last position out[B, d] (last_only = 1, the
 * `final_feats[:, -1, :]` of model.py:104).  err_flag (optional device int32, may be NULL) is set
 * to 1 when an id is outside [0, item_rows) (such ids read the zero padding row instead). */
int gr_sasrec_forward_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                          float* out, int32_t last_only, void* workspace, size_t workspace_bytes,
                          int32_t* err_flag, void* stream);

/* SASRec.predict(log_seqs) (SASRec/model.py:98-108): logits[B, item_rows] = h_last . item_emb^T. */
int gr_sasrec_predict_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                          float* logits, void* workspace, size_t workspace_bytes,
                          int32_t* err_flag, void* stream);

/* Same, logits rows ld floats apart (ld >= item_rows).  SASRec.predict allocates ld = item_rows
 * rounded up to 32 floats, so every row starts on a 128-byte line and the scoring kernel stores
 * whole lines straight from its accumulators; the caller gets the [B, item_rows]
 * view, on which evaluate.py:27-32 (in-place column-0 mask, gather, '>' count) work unchanged. */
int gr_sasrec_predict_ld_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                             float* logits, int64_t ld, void* workspace, size_t workspace_bytes,
                             int32_t* err_flag, void* stream);

/* One batch of SASRec/evaluate.py:26-32 in one call, the logits never written: ranks_out[b] =
 * #{j : l[b, j] > l[b, targets[b]]} + 1 with l = predict(seqs) and column 0 taken as -1e9 when
 * mask_col0 (evaluate.py:27) -- the forward's last hidden states, then the target logit and the
 * strict count on the scoring kernel's exact fp32 chain (gr_score_pairs_f32 /
 * gr_score_count_gt_ws_f32 below; bitwise the ranks of the materialised sequence).  d in {16, 32,
 * 64, 128}.  workspace: gr_sasrec_rank_workspace_bytes; count_ws (optional, may be NULL): zero on
 * entry and left zero, gr_score_count_workspace_bytes(B).  err_flag as gr_sasrec_forward_f32 (also
 * set for a target outside [0, item_rows)). */
size_t gr_sasrec_rank_workspace_bytes(const gr_sasrec_params* p, int64_t B, int32_t n);
int gr_sasrec_rank_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                       const int64_t* targets, int32_t mask_col0, int64_t* ranks_out, void* workspace,
                       size_t workspace_bytes, void* count_ws, size_t count_ws_bytes, int32_t* err_flag,
                       void* stream);

/* The kernels the three entry points above run for this model, batch and length under the options
 * in force (host only, nothing is launched): a non-negative mask of the GR_SAS_* bits below, or the
 * negative code of the parameter checks those entry points make.  One pipeline bit is always set. */
#define GR_SAS_FUSED 0x1            /* the register-resident forward kernel (option sas_fused)    */
#define GR_SAS_ROWTILE 0x2          /* d = 128 row-tile kernels (option sas_rowtile)              */
#define GR_SAS_LAYERWISE 0x4        /* one kernel per op                                          */
#define GR_SAS_FUSED_TWO_WAVES 0x8  /* fused: two waves per sequence (else one)                   */
#define GR_SAS_FUSED_MISALIGNED 0x10 /* fused shape, a parameter not 16-byte aligned: the forward
                                        returns GR_ERR_UNSUPPORTED before any launch              */
#define GR_SAS_B0_EMBED_PROJ 0x20   /* row-tile block 0: embed + LN_a0 + in-projection, one kernel */
#define GR_SAS_B0_EMBED_LN_LINEAR 0x40 /* row-tile block 0: embed + LN_a0, then gr_linear          */
#define GR_SAS_B0_EMBED_LN 0x80     /* row-tile block 0: embed + LN_a0 alone (the H-form tail of a
                                       one-block model reads it)                                  */
#define GR_SAS_ATTN_SCALAR 0x100    /* causal_attn_kernel (head widths other than 32 / 64 / 128)  */
#define GR_SAS_ATTN_MFMA 0x200      /* attn_mfma_kernel                                           */
#define GR_SAS_ATTN_PERSIST 0x400   /* attn_persist_kernel                                        */
#define GR_SAS_ATTN_K16 0x800       /* attn_k16_kernel (option attn_k16); no ATTN bit: no attention
                                       launch at all                                              */
#define GR_SAS_ATTN_LAST_TILE 0x1000 /* the final block's attention runs on the last query tile only */
#define GR_SAS_TAIL 0x2000          /* last-position forward: the final block is the H-form tail  */
#define GR_SAS_TAIL_VALU 0x4000     /* the tail's VALU reduction form (B <= compute units)        */
#define GR_SAS_PRUNED 0x8000        /* last-position forward: the final block after its attention
                                       runs on the B last rows only                               */
int32_t gr_sasrec_plan(const gr_sasrec_params* p, int64_t B, int32_t n, int32_t last_only);

/* SASRec training, the transformer part of one step (SASRec/train.py:131 `model.forward` in train
 * mode and the backward that `loss.backward()`, train.py:161-172, runs through model.py:49-96).
 * Two kernel sets with the same saved activations and dropout masks: gr_sasrec_train_fwd_f32 /
 * _bwd_f32, one workgroup per sequence, n <= 64, d <= 64 (d % num_heads == 0), mlp_layer <= 128,
 * <= 8 blocks; and gr_sasrec_train_tiled_fwd_f32 / _bwd_f32 below, n <= 256, d <= 128,
 * mlp_layer <= 256.  Dropout p (params['dropout']) on the attention probabilities, the FFN hidden layer and the FFN
 * output, as nn.MultiheadAttention / nn.Dropout apply it; masks from a counter-based hash keyed by
 * seed ^ *seed_dev (seed_dev optional), the same for the forward and the backward of one step.
 * Buffers (device, caller-allocated, fp32): nb = n_blocks, R = B * n rows (sequence-major). */
typedef struct gr_sasrec_train_bufs {
  float* xin;    /* [nb, R, d]    LN_a input of each block       (written by the forward) */
  float* hs;     /* [nb, R, d]    LN_a output = in-projection input                       */
  float* qkv;    /* [nb, R, 3d]   in-projection output q | k | v                          */
  float* prob;   /* [nb, B, H, n, n] softmax probabilities before dropout                 */
  float* os;     /* [nb, R, d]    attention output = out-projection input                 */
  float* x1;     /* [nb, R, d]    residual after attention = LN_f input                   */
  float* fs;     /* [nb, R, d]    LN_f output = FFN1 input                                */
  float* zs;     /* [nb, R, mlp]  FFN1 output before the ReLU                             */
  float* us;     /* [nb, R, mlp]  dropout(relu(FFN1)) = FFN2 input                        */
  float* xl;     /* [R, d]        last LayerNorm input                                    */
  float* g_vec;  /* [B, gr_sasrec_train_vec_width] (written by the backward; the tiled backward:
                    [gr_sasrec_train_tiled_parts, ...] split-k partials) per-sequence partial
                    gradients in SASRec's parameter order: per block [ln_a w, ln_a b, in_proj w
                    (3d x d), in_proj b, out_proj w (d x d), out_proj b, ln_f w, ln_f b, ffn1 w
                    (mlp x d), ffn1 b, ffn2 w (d x mlp), ffn2 b], then [last ln w, last ln b], then
                    pos_emb rows [n, d]; the parameter gradients are its sum over B             */
} gr_sasrec_train_bufs;

/* Floats per sequence in gr_sasrec_train_bufs.g_vec (csrc/sasrec_train_contract.h sas_vec_width). */
int32_t gr_sasrec_train_vec_width(const gr_sasrec_params* p, int32_t n);

/* Train-mode forward: seqs[B, n] -> out[B, n, d] (model.py:49-96 with dropout p), saving the
 * activations in bufs.  err_flag (optional) gets 1 for an id outside [0, item_rows). */
int gr_sasrec_train_fwd_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                            float p_drop, uint64_t seed, const uint64_t* seed_dev,
                            const gr_sasrec_train_bufs* bufs, float* out, int32_t* err_flag, void* stream);

/* Backward of the forward above (same seqs, p_drop, seed, bufs): d_out[B, n, d] -> the
 * per-sequence partial gradients in bufs.g_vec (sum over B = every parameter's gradient except
 * the item table's); item-embedding rows are added (atomically) into g_item[item_rows, d]
 * (optional; padding row 0 is left untouched). */
int gr_sasrec_train_bwd_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                            float p_drop, uint64_t seed, const uint64_t* seed_dev,
                            const gr_sasrec_train_bufs* bufs, const float* d_out, float* g_item,
                            void* stream);

/* The tiled training path (sasrec_train_tiled.hip) for shapes beyond one workgroup per sequence:
 * 1 <= d <= 128 (divisible by n_heads), 1 <= n <= min(256, max_len), 1 <= mlp <= 256, 1..8
 * blocks, any B >= 1 with B * n * n_heads < 2^31, dropout in [0, 1).  Same computation, saved activations
 * (gr_sasrec_train_bufs) and dropout masks as the pair above; the products run as tiled launches
 * over all B * n rows, and the backward writes bufs.g_vec as [parts, gr_sasrec_train_vec_width]
 * partial rows (split-k chunks of the rows; their sum over parts is every parameter's gradient
 * but the item table's).  Both calls need a caller-owned workspace. */
size_t gr_sasrec_train_tiled_workspace_bytes(const gr_sasrec_params* p, int64_t B, int32_t n);

/* Partial rows of bufs.g_vec the tiled backward writes (>= 1; 0 for bad arguments). */
int32_t gr_sasrec_train_tiled_parts(const gr_sasrec_params* p, int64_t B, int32_t n);

int gr_sasrec_train_tiled_fwd_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                                  float p_drop, uint64_t seed, const uint64_t* seed_dev,
                                  const gr_sasrec_train_bufs* bufs, float* out, int32_t* err_flag,
                                  void* workspace, size_t workspace_bytes, void* stream);

int gr_sasrec_train_tiled_bwd_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                                  float p_drop, uint64_t seed, const uint64_t* seed_dev,
                                  const gr_sasrec_train_bufs* bufs, const float* d_out, float* g_item,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Full-catalog (or catalog-shard) scoring logits[B, rows] = h[B, d] . table[rows, d]^T
 * (SASRec/model.py:107).  ld = row stride of logits. */
int gr_score_f32(const float* h, int64_t B, int32_t d, const float* table, int64_t rows,
                 float* logits, int64_t ld, void* stream);

/* Strict rank of each user's target (SASRec/evaluate.py:27-32) without mutating logits:
 * with column 0 taken as -1e9 (when mask_col0), rank[b] = #{j : l[b,j] > l[b,t_b]} + 1.
 * ld = row stride of logits, cols = number of columns. */
int gr_rank_f32(const float* logits, int64_t B, int64_t cols, int64_t ld, const int64_t* targets,
                int32_t mask_col0, int64_t* ranks_out, void* stream);

/* Catalog-shard helpers.  count: cnt[b] = #{j < cols : l[b,j] > thresholds[b]}
 * (the strict '>' of SASRec/evaluate.py:32; summed over shards it gives rank - 1).  B <= 65535. */
int gr_count_gt_f32(const float* logits, int64_t B, int64_t cols, int64_t ld,
                    const float* thresholds, int64_t* counts_out, void* stream);

/* Per-row top-k (k <= 64) of logits[B, cols]: values descending, ties to the lower column;
 * ids_out = column + id_offset (the shard's first catalog row); -1 pads rows with < k entries.
 * When thresholds / counts_out are given (both or neither), the same single pass over the logits
 * also produces gr_count_gt_f32's counts.  Rows are cut into segments (one workgroup each, local
 * top-k to the workspace) and merged per row.  B <= 65535. */
size_t gr_topk_workspace_bytes(int64_t B, int64_t cols, int32_t k);
int gr_topk_f32(const float* logits, int64_t B, int64_t cols, int64_t ld, int32_t k,
                int64_t id_offset, float* vals_out, int64_t* ids_out, const float* thresholds,
                int64_t* counts_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused rank without materialising logits (SASRec/evaluate.py:26-32).  Every
 * logit is evaluated with exactly the instruction sequence of gr_score_f32 (d in {16, 32, 64, 128}), so
 * the values below are bitwise the entries gr_score_f32 / gr_sasrec_predict_f32 would write.
 *
 * Target logits: out[b] = h[b] . table[ids[b]] (-1e9 when mask_col0 and ids[b] == 0, the
 * evaluate.py:27 mask).  err_flag (optional device int32) is set when an id is outside [0, rows). */
int gr_score_pairs_f32(const float* h, int64_t B, int32_t d, const float* table, int64_t rows,
                       const int64_t* ids, int32_t mask_col0, float* out, int32_t* err_flag,
                       void* stream);

/* counts_out[b] = #{j < rows : l[b, j] > thresholds[b]}, l = h . table^T with column 0 taken as
 * -1e9 when mask_col0 (strict '>', evaluate.py:32).  With thresholds = gr_score_pairs_f32 of the
 * targets, counts + 1 is the reference's rank.  On a catalog shard (rows = the shard's rows,
 * mask_col0 only on the shard holding row 0) the counts of all shards sum to the global count. */
int gr_score_count_gt_f32(const float* h, int64_t B, int32_t d, const float* table, int64_t rows,
                          const float* thresholds, int32_t mask_col0, int64_t* counts_out,
                          void* stream);

/* The same counts with a caller workspace of gr_score_count_workspace_bytes(B) bytes that must be
 * ZERO on entry and is left zero on return (one zeroed buffer serves every call on a stream).  Short
 * batches split the catalog over every CU, so hundreds of workgroups add into each user's word;
 * with the workspace the adds are spread over 16 copies and one more launch sums them (in copy
 * order: exact) -- at B 128 x 100k rows 65 -> ~25 us.  Null / short workspace: the form above. */
size_t gr_score_count_workspace_bytes(int64_t B);
int gr_score_count_gt_ws_f32(const float* h, int64_t B, int32_t d, const float* table, int64_t rows,
                             const float* thresholds, int32_t mask_col0, int64_t* counts_out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Fused top-k (+ strict counts) over the full catalog or a catalog shard without materialising
 * logits (SASRec/model.py:107 + evaluate.py:27-32; the per-shard candidate lists of SURVEY §8(e)).
 * Logits are l = h . table^T evaluated with exactly gr_score_f32's instruction sequence, column 0
 * taken as -1e9 when mask_col0.  vals_out[B, k] / ids_out[B, k]: the k largest, value descending,
 * ties to the lower column, ids = column + id_offset (-1 / -inf pad rows with fewer than k
 * columns).  thresholds / counts_out (both or neither): counts_out[b] = #{j : l[b, j] > thr[b]}.
 * d in {16, 32, 64, 128}, 1 <= k <= 16, rows < 2^31, B <= 65535.  Replaces gr_score_f32 + gr_topk_f32
 * (which read the logits back) when only the top-k / ranks are needed. */
size_t gr_score_topk_workspace_bytes(int64_t B, int32_t d, int64_t rows, int32_t k);
int gr_score_topk_f32(const float* h, int64_t B, int32_t d, const float* table, int64_t rows,
                      int64_t id_offset, int32_t mask_col0, int32_t k, const float* thresholds,
                      int64_t* counts_out, float* vals_out, int64_t* ids_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Merge of catalog shards' top-k lists (the catalog-sharded counterpart of
 * SASRec/evaluate.py's per-user ranking): per row b, the k best of C candidates (cand_vals[b, c],
 * cand_ids[b, c]) by (value desc, id asc) -- the id order compares all 64 bits, so any id in
 * [0, INT64_MAX) orders exactly; ids < 0 and NaN values are padding, emitted as (-inf, -1) when
 * fewer than k real candidates remain (the output always has k columns).  k >= 1, C <= 256.
 * ldv / ldi: row strides (elements). */
int gr_merge_topk_f32(const float* cand_vals, int64_t ldv, const int64_t* cand_ids, int64_t ldi,
                      int64_t B, int32_t C, int32_t k, float* vals_out, int64_t* ids_out, void* stream);
/* The same merge straight from the all-gathered exchange buffer: packed [world][B][2 kk] int64, per
 * (rank, row) kk ids then kk values (float bits in the low 32 bits of each word).  world kk <= 256. */
int gr_merge_topk_packed(const int64_t* packed, int32_t world, int64_t B, int32_t kk, int32_t k,
                         float* vals_out, int64_t* ids_out, void* stream);

/* Training-side scoring (SASRec/train.py:131-160) without the [B, n, rows]
 * score matrix.  feats[B, n, d] = model.forward(input_seqs), table[rows, d] = item_emb.weight,
 * targets[B, n] = o_t (0 = padding, masked), negs[B, num_neg] (shared by the user's n positions,
 * train.py:143-150).  With S = feats . table^T:
 *   row_loss[b*n+t] = m*(-log(sigmoid(S[b,t,o_t]) + eps)) + sum_j m*(-log(1 - sigmoid(S[b,t,neg_j]) + eps)),
 *   m = (o_t != 0);  sums[0] = batch_loss = sum of row_loss, sums[1] = mask.sum()  (train.py:155-158).
 * coef[B*n*(1+num_neg)] receives d row_loss / d S at the gathered entries (target first), the
 * saved state for the backward.  err_flag (optional device int32) is set for an id outside [0, rows). */
int gr_sampled_bce_fwd_f32(const float* feats, int64_t B, int32_t n, int32_t d, const float* table,
                           int64_t rows, const int64_t* targets, const int64_t* negs,
                           int32_t num_neg, float eps, float* row_loss, float* coef, float* sums,
                           int32_t* err_flag, void* stream);

/* Backward of batch_loss scaled by *grad_scale (device fp32 scalar, e.g. 1/valid of
 * `loss = batch_loss / batch_valid_t`): dfeats[B, n, d] (written) and dtable[rows, d] (zeroed,
 * then the gathered rows accumulated with fp32 atomics, so the summation order is not fixed). */
int gr_sampled_bce_bwd_f32(const float* feats, int64_t B, int32_t n, int32_t d, const float* table,
                           int64_t rows, const int64_t* targets, const int64_t* negs,
                           int32_t num_neg, const float* coef, const float* grad_scale,
                           float* dfeats, float* dtable, void* stream);

/* Negative items for SASRec training (SASRec/train.py:15-30 get_neg_samples): out[b, 0..num_neg)
 * = num_neg distinct items drawn uniformly from [1, item_num] minus the non-zero items of
 * seqs[b, 0..n) (the reference's np.random.choice(setdiff1d(...), num_neg, replace=False): same
 * distribution, own counter-based random stream keyed by seed).  num_neg <= 1024.  err_flag
 * (optional device int32) is set to 2 when a row has fewer than num_neg valid items (the reference
 * raises ValueError there); that row's ids are all -1. */
int gr_neg_samples(const int64_t* seqs, int64_t B, int32_t n, int64_t item_num, int32_t num_neg,
                   uint64_t seed, int64_t* out, int32_t* err_flag, void* stream);

/* gr_neg_samples keyed by seed ^ *seed_dev (a device uint64 the kernel only reads): the form a
 * captured graph (hipGraph / torch.cuda.graph) replays with fresh negatives, the caller advancing
 * *seed_dev on the stream between replays (SasTrainStep in the Python package does). */
int gr_neg_samples_dseed(const int64_t* seqs, int64_t B, int32_t n, int64_t item_num, int32_t num_neg,
                         uint64_t seed, const uint64_t* seed_dev, int64_t* out, int32_t* err_flag,
                         void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Semantic-ID emission: collision groups and dedup digit (RQ-VAE/infer.py:29-41 get_collision_item,
 * infer.py:139-162 the dedup digit, RQ-VAE/train.py:127-151 the collision rate) for codes[n, levels]
 * int64, 0 <= n < 2^31, 1 <= levels <= 16.  Rows are compared as whole rows of full int64 values.
 * Pure integer work: every output is a function of the input alone (no arrival-order dependence).
 *
 * gr_code_groups_i64 replaces the per-row Python dict of get_collision_item and train.py's set of
 * joined strings.  Per row r (all [n] int64):
 *   leader[r] = the smallest row whose code equals row r's,
 *   count[r]  = the rows that carry that code,
 *   digit[r]  = 0 (gr_code_segments_i64 fills the rows of shared codes in).
 * keys[n]: the rows with count > 1 as leader << 32 | row, in no particular order, in keys[0 .. M);
 * keys[M .. n) = INT64_MAX, so an ascending sort of all n keys leaves the M real ones first.
 * stats[4]: {distinct codes, largest count, M = rows with count > 1, G = codes with count > 1}.
 * workspace: gr_code_groups_workspace_bytes(n, levels) bytes, 8-byte aligned (an open-addressing
 * table of at least 2 n slots, cleared by the call itself); the query returns 0 for a bad shape and
 * does not decrease with n.  The same workspace is large enough for gr_code_segments_i64.
 * n = 0 succeeds and launches nothing (no output is written). */
size_t gr_code_groups_workspace_bytes(int64_t n, int32_t levels);
int gr_code_groups_i64(const int64_t* codes, int64_t n, int32_t levels, int64_t* leader, int64_t* count,
                       int64_t* digit, int64_t* keys, int64_t* stats, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The group listing from the ASCENDING-sorted keys of gr_code_groups_i64 (sorted_keys[n], the same
 * stats / count / digit; M and G are read from stats on the device, so the host need not know them):
 *   rows[n]      rows[0 .. M) = the rows with count > 1 ordered by leader (the code's first
 *                appearance), then by row -- get_collision_item's groups concatenated; the rest -1,
 *   sizes[n / 2] sizes[0 .. G) = the size of each group in the same order (the rest is not written),
 *   digit[row]   = the row's position in its group (infer.py:151-162's `codes_array[idx, -1] = i`),
 *                written for rows[0 .. M) only.
 * workspace: at least 8 ceil(n / 256) bytes, 8-byte aligned.  n = 0 succeeds and launches nothing. */
int gr_code_segments_i64(const int64_t* sorted_keys, int64_t n, const int64_t* stats, const int64_t* count,
                         int64_t* rows, int64_t* sizes, int64_t* digit, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Codebook k-means init (RQ-VAE/models/layers.py:69-82 kmeans(): scikit-learn's
 * KMeans(n_clusters = K, max_iter).fit(x).cluster_centers_, the call behind vq.py:39-47 init_emb)
 * for fp32 rows x[n, e], 1 <= e <= 64, 1 <= K <= 1024, K <= n < 2^31 (GR_ERR_UNSUPPORTED outside;
 * n < K is GR_ERR_ARG, scikit-learn's ValueError).  The whole run -- greedy k-means++ seeding, up to
 * max_iter Lloyd iterations, the final labels -- is enqueued by this one call; both stop rules are
 * evaluated on the device, and iterations enqueued past convergence do nothing.
 *   seeding   the first centre is a uniform row; each later one is the best (lowest resulting
 *             potential) of `trials` rows drawn with probability proportional to D^2, the squared
 *             distance to the nearest chosen centre (trials = 0: scikit-learn's 2 + floor(ln K);
 *             1: plain D^2 sampling; at most 16).  The draws are a counter-based hash of
 *             (seed, round, trial): a function of the seed and the data only.  Every centre is a row
 *             of x, and a row with D^2 = 0 is never drawn while one with D^2 > 0 exists.
 *             init_centers[K, e] (optional) replaces the seeding.
 *   E step    label = first index of the minimum of sum_f (x_f - c_f)^2 (direct form, fp32).
 *   M step    centre = mean of its members, summed in fp64 in a fixed order (no float atomics):
 *             the same inputs give the same bits on every run.
 *   empties   scikit-learn's relocation: the empty clusters in ascending id, the j-th taking the
 *             j-th farthest row (distance to its assigned old centre descending, ties to the lower
 *             row), which leaves its donor's sum and count; labels stay; a cluster whose count ends
 *             at 0 keeps its old centre.
 *   stop      when an E step repeats the previous labels, or when the summed squared centre shift
 *             is <= tol * mean over features of var(x).
 * Outputs (device): centers_out[K, e]; labels_out[n] (optional) and *inertia_out (optional, fp64)
 * of the rows against the returned centres; *n_iter_out (optional) = Lloyd iterations run.
 * max_iter = 0 with init_centers returns the labels and inertia of the given centres.
 * workspace: gr_kmeans_workspace_bytes(n, e, K) bytes, 16-byte aligned (0 for a shape outside the
 * envelope).  Option "kmeans_small" (gr_set_option) chooses the launch form; gr_kmeans_form
 * returns the form a call of this shape takes under the option in force: 1 = one workgroup,
 * 0 = tiled, -1 = outside the envelope. */
size_t gr_kmeans_workspace_bytes(int64_t n, int32_t e, int32_t K);
int32_t gr_kmeans_form(int64_t n, int32_t e, int32_t K);
int gr_kmeans_f32(const float* x, int64_t n, int32_t e, int32_t K, const float* init_centers,
                  uint64_t seed, int32_t trials, int32_t max_iter, double tol, float* centers_out,
                  int64_t* labels_out, double* inertia_out, int32_t* n_iter_out, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* TIGER generative retrieval (RQVAE-T5/model.py:62-81 TIGER.generate: a T5 encoder-decoder searched
 * by transformers' GenerationMixin._beam_search with num_return_sequences = num_beams,
 * length_penalty 1, early_stopping False, no sampling, decoder_start_token_id = pad).
 *
 * gr_tiger_params: dimensions and device pointers of the T5 weights (fp32, row-major [out, in] as
 * nn.Linear stores them, 16-byte aligned).  enc[l] = {layer.0.layer_norm, q, k, v, o,
 * layer.1.layer_norm, wi, wo}; dec[l] = {layer.0.layer_norm, q, k, v, o, layer.1.layer_norm,
 * EncDecAttention q, k, v, o, layer.2.layer_norm, wi, wo}.  enc_rel / dec_rel: block 0's
 * relative_attention_bias [n_buckets, n_heads].  enc_bucket[255]: the bucket of key - query distance
 * r at index r + 127 (bidirectional); dec_bucket[8]: the bucket of a key d positions behind the query
 * at index d (one-directional) -- T5Attention._relative_position_bucket's values, device int32.
 * lm_scale multiplies the decoder output before lm_head (d_model^-0.5 with tied embeddings, else 1).
 * fill_id is what unfilled positions of a hypothesis hold: the library's `pad_token_id or
 * eos_token_id`, i.e. the EOS id when the pad id is 0.
 *
 * Envelope (GR_ERR_UNSUPPORTED outside, with the limit named): d_model in {32, 64};
 * n_heads * d_kv in {32, 64} with d_kv in {8, 16, 32}; d_ff <= 256 and a multiple of 32; 1..4 layers
 * on each side; 2 * num_beams <= vocab <= 128 (below that the -1e9-masked dead beams would reach the
 * selection as exact fp32 ties); 1 <= S <= 128; 1 <= num_beams <= 32; 2 <= max_length <= 8; at most 2^21 users per call.
 * Preconditions (not checked): ids in [0, vocab) (out-of-range ids are clamped); every history has at
 * least one unmasked token.
 *
 * gr_tiger_generate_f32 enqueues two launches and never synchronises: an encoder kernel (one
 * workgroup per user; it also projects every decoder layer's cross-attention K and V once per user)
 * and a search kernel (one workgroup per user runs all max_length - 1 decode steps, the selection of
 * the 2 * num_beams continuations among num_beams * vocab, and the running / finished bookkeeping).
 * A user whose early-stop heuristic is satisfied runs no further step (the library runs them and
 * ignores their result).  Equal scores: the lower flat index (beam * vocab + token) first; an old finished hypothesis before
 * a new one.
 *   input_ids[B, S] int64, attention_mask[B, S] int64 (0 = padding; NULL: none)
 *   sequences[B, num_beams, max_length] int64: best first, never cropped; scores[B, num_beams]
 *   enc_out[B, S, d_model] (optional): the encoder output (rows of padding are unspecified)
 *   step_logits[B, max_length - 1, num_beams, vocab] (optional): lm_head logits of the running beams
 *   at each step (zero where a beam is not live or the user's search has stopped)
 * workspace: gr_tiger_workspace_bytes(...) bytes, 16-byte aligned (0 outside the envelope). */
#define GR_TIGER_MAX_LAYERS 4
typedef struct gr_tiger_params {
  int32_t vocab, d_model, d_kv, n_heads, d_ff, n_enc, n_dec, n_buckets;
  int32_t pad_id, eos_id, fill_id, reserved;
  float eps, lm_scale;
  const float* shared;
  const float* lm_head;
  const float* enc_rel;
  const float* dec_rel;
  const float* enc_final_ln;
  const float* dec_final_ln;
  const int32_t* enc_bucket;
  const int32_t* dec_bucket;
  const float* enc[GR_TIGER_MAX_LAYERS][8];
  const float* dec[GR_TIGER_MAX_LAYERS][13];
} gr_tiger_params;

size_t gr_tiger_workspace_bytes(const gr_tiger_params* p, int64_t B, int32_t S, int32_t num_beams,
                                int32_t max_length);
int gr_tiger_generate_f32(const gr_tiger_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                          int64_t B, int32_t S, int32_t num_beams, int32_t max_length, int64_t* sequences,
                          float* scores, float* enc_out, float* step_logits, void* workspace,
                          size_t workspace_bytes, void* stream);

/* TIGER prefix variant (RQVAE-T5-prefix/model.py: three ProfessionalAdapter modules, each turning the
 * history's token embeddings and the user's n_vec BERT vectors of one level of the professional
 * hierarchy into one prefix token; the three tokens are prepended to the encoder input and the beam
 * search runs on S + 3 encoder positions).  Inference only, eval-mode arithmetic (no dropout).
 *
 * gr_tiger_prefix_params: adapter[level] = {bert_proj.weight [d, bert_dim], bert_proj.bias,
 * cross_attn.in_proj_weight [3 d, d], in_proj_bias, cross_attn.out_proj.weight [d, d], out_proj.bias,
 * ffn.0.weight [4 d, d], ffn.0.bias, ffn.2.weight [d, 4 d], ffn.2.bias, norm1.weight, norm1.bias,
 * norm2.weight, norm2.bias}: fp32 device pointers, 16-byte aligned.  n_heads is the adapters'
 * nn.MultiheadAttention head count: the head width is d_model / n_heads (not d_kv) and the scores are
 * scaled by its inverse square root.  eps is the two LayerNorms' (biased variance).
 *
 * gr_tiger_generate_prefix_f32 enqueues three launches and never synchronises: tiger_adapter_kernel
 * (one workgroup per user and level; the embeddings of all S positions, padding included, are
 * attended to the n_vec projected vectors, normalised, fed forward and averaged over S in a fixed
 * order, so a call is bitwise repeatable; it also writes the [B, S + 3] key mask, whose first three
 * columns are 1), then gr_tiger_generate_f32's encoder and search kernels on S + 3 positions.
 *   prof1..3[B, n_vec, bert_dim] fp32, 16-byte aligned
 *   prefix_out[B, 3, d_model] (optional): the three prefix tokens
 *   enc_out[B, S + 3, d_model] (optional); the other arguments as in gr_tiger_generate_f32
 * Envelope: gr_tiger_generate_f32's with S + 3 in place of S (so S <= 125), bert_dim a multiple of 4
 * in [4, 1024], 1 <= n_vec <= 16, d_model % n_heads == 0.  The prefix variant's deployed width
 * (d_model 128, d_ff 512, 8 heads) is outside gr_tiger_params' envelope and is refused by it.
 * workspace: gr_tiger_prefix_workspace_bytes(...) = gr_tiger_workspace_bytes at S + 3, the int64 mask
 * and the prefix tokens (0 outside the envelope). */
typedef struct gr_tiger_prefix_params {
  int32_t bert_dim, n_vec, n_heads, reserved;
  float eps, reserved_f;
  const float* adapter[3][14];
} gr_tiger_prefix_params;

size_t gr_tiger_prefix_workspace_bytes(const gr_tiger_params* p, const gr_tiger_prefix_params* pp, int64_t B,
                                       int32_t S, int32_t num_beams, int32_t max_length);
int gr_tiger_generate_prefix_f32(const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                                 const int64_t* input_ids, const int64_t* attention_mask, const float* prof1,
                                 const float* prof2, const float* prof3, int64_t B, int32_t S, int32_t num_beams,
                                 int32_t max_length, int64_t* sequences, float* scores, float* prefix_out,
                                 float* enc_out, float* step_logits, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* TIGER teacher-forced forward: the evaluation-time call model(input_ids, attention_mask, labels) of
 * eval_loss (RQVAE-T5/train.py:40-51), i.e. T5ForConditionalGeneration.forward with labels under
 * model.eval() and torch.no_grad() -- gr_tiger_forward_f32; gr_tiger_forward_prefix_f32 is the same call
 * of RQVAE-T5-prefix/train.py's eval_loss with prof_lvl1..3 (RQVAE-T5-prefix/model.py TIGER.forward).
 * Forward only: no dropout, no gradient.
 *
 * The decoder input row is [pad_id, labels[:, :-1]] with every -100 replaced by pad_id (_shift_right).
 * The decoder runs over all Ld positions at once: causal self-attention with the decoder's relative
 * bias, cross-attention over the user's encoder keys (padding masked, no position bias), the ReLU
 * feed-forward, the final norm times lm_scale, lm_head.
 *   labels[B, Ld] int64; -100 marks a position that is not counted (anywhere in a row)
 *   loss: one fp32, the mean over the counted positions of -log_softmax(logits)[label]; NaN when no
 *   position of the batch is counted (torch's mean over nothing).  A label outside [0, vocab) that is
 *   not -100 never faults (every read uses a clamped index); its NLL, and so the loss, is NaN.
 *   logits[B, Ld, vocab] (optional); nll[B, Ld] (optional): the per-position NLL, 0 where not counted
 *   enc_out (optional) and the other arguments as in the generate entries
 * Launches, never synchronising: generate's encoder kernel (after generate's adapter kernel in the
 * prefix entry), a teacher kernel (one workgroup per four users; log-softmax and NLL per row, a
 * (sum, count) pair per user) and a one-workgroup loss kernel that adds the pairs in a fixed order in
 * double and rounds once: a call is bitwise repeatable, and a user's logits and NLLs do not depend on
 * the rest of the batch.
 * Envelope: the generate entries' without num_beams and max_length (vocab >= 2); 1 <= Ld <= 8.
 * workspace: gr_tiger_forward_workspace_bytes / gr_tiger_forward_prefix_workspace_bytes (cross K/V,
 * the pairs, and for the prefix entry the mask and the prefix tokens; 0 outside the envelope). */
size_t gr_tiger_forward_workspace_bytes(const gr_tiger_params* p, int64_t B, int32_t S, int32_t Ld);
int gr_tiger_forward_f32(const gr_tiger_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                         const int64_t* labels, int64_t B, int32_t S, int32_t Ld, float* loss, float* logits,
                         float* nll, float* enc_out, void* workspace, size_t workspace_bytes, void* stream);
size_t gr_tiger_forward_prefix_workspace_bytes(const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                                               int64_t B, int32_t S, int32_t Ld);
int gr_tiger_forward_prefix_f32(const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                                const int64_t* input_ids, const int64_t* attention_mask, const float* prof1,
                                const float* prof2, const float* prof3, const int64_t* labels, int64_t B,
                                int32_t S, int32_t Ld, float* loss, float* logits, float* nll, float* enc_out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* calculate_pos_index of RQVAE-T5/utils.py:6-32: hits[b, j] = 1 for the first beam j whose tokens
 * equal labels[b, :], 0 elsewhere.  preds: beam j of user b starts at preds + (b * k + j) * ld_pred
 * and holds pred_len tokens; positions past pred_len compare as 0 (evaluate_model's zero padding) and
 * positions past label_len are not compared (its cut).  hits[B, k] uint8. */
int gr_beam_hits_i64(const int64_t* preds, int64_t B, int32_t k, int32_t pred_len, int64_t ld_pred,
                     const int64_t* labels, int32_t label_len, uint8_t* hits, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* T5 embedding retriever (T5/model.py:46-65 TIGER.forward: input_proj, an eval-mode bidirectional
 * T5 encoder stack on inputs_embeds, masked mean pooling, output_proj, L2 normalisation).
 *
 * gr_t5_embed_params: dimensions and device pointers (fp32, row-major [out, in], 16-byte aligned).
 * in_w [d_model, in_dim], in_b [d_model]; out_w [out_dim, d_model], out_b [out_dim]; rel [n_buckets,
 * n_heads]: block 0's relative_attention_bias, used by every block; bucket[255]: the bucket of key -
 * query distance r at index r + 127 (bidirectional, device int32; gr_tiger_params' enc_bucket);
 * final_ln [d_model]; layer[l] = {layer.0.layer_norm, q, k, v, o, layer.1.layer_norm, wi, wo}.
 *
 * Math (all fp32, softmax in fp32, no 1/sqrt(d_kv) scale, no embedding scale):
 *   x = seq_embs . in_w^T + in_b
 *   per block: x += o(softmax(q k^T + bias + mask) v) on RMSNorm(x); x += wo(relu(wi(RMSNorm(x))))
 *   RMSNorm(x) = w * (x * rsqrt(mean(x^2) + eps)); bias[h, i, j] = rel[bucket(j - i), h] on the
 *   original positions; key j is removed wherever attention_mask[b, j] == 0 (any other value: live)
 *   hidden = RMSNorm_final(x); pooled = sum_j live hidden / max(count live, 1e-9)
 *   pred = pooled . out_w^T + out_b; pred_out = pred / max(|pred|_2, 1e-8)
 * Masks with holes are legal.  Rows with mask 0 are never keys and never pooled, so what seq_embs
 * holds there (any finite value) does not reach pred_out.  A user with no live position yields
 * pooled = 0 and pred_out = normalize(out_b); the reference's data never has one (position 0 is the
 * user vector).  hidden_out (optional): the final-norm hidden states; masked-out rows are unspecified.
 *
 * gr_t5_embed_f32 enqueues 1 + 4 n_layers + 3 launches and never synchronises: input_proj; per block
 * RMSNorm + q/k/v, per-user attention + o + residual, RMSNorm + wi + relu, wo + residual; then final
 * norm + pooling, output_proj, normalise.  No floating-point atomics: every output element has one
 * fixed summation order that depends on neither B nor the user's place in the batch, so two calls
 * give the same bits and a sub-batch gives the bits of the whole batch's rows.
 *   seq_embs[B, S, in_dim] fp32 16-byte aligned; attention_mask[B, S] int64 or NULL (all live)
 *   pred_out[B, out_dim]; hidden_out[B, S, d_model] or NULL
 * Envelope (GR_ERR_UNSUPPORTED outside, with the field named, before any launch): d_model a multiple
 * of 32 in [32, 512]; d_kv in {8, 16, 32, 64} with n_heads * d_kv <= 256; d_ff a multiple of 32 in
 * [32, 1024]; in_dim and out_dim multiples of 4 in [4, 1024]; n_layers 1..8; n_buckets 32; S 1..32;
 * B 0..2^20 (B = 0: GR_OK, no launch).
 * workspace: gr_t5_embed_workspace_bytes(p, B, S) bytes, 16-byte aligned (0 outside the envelope). */
#define GR_T5E_MAX_LAYERS 8
typedef struct gr_t5_embed_params {
  int32_t d_model, d_kv, n_heads, d_ff, n_layers, in_dim, out_dim, n_buckets;
  float eps, reserved;
  const float* in_w;
  const float* in_b;
  const float* out_w;
  const float* out_b;
  const float* rel;
  const int32_t* bucket;
  const float* final_ln;
  const float* layer[GR_T5E_MAX_LAYERS][8];
} gr_t5_embed_params;

size_t gr_t5_embed_workspace_bytes(const gr_t5_embed_params* p, int64_t B, int32_t S);
int gr_t5_embed_f32(const gr_t5_embed_params* p, const float* seq_embs, const int64_t* attention_mask,
                    int64_t B, int32_t S, float* pred_out, float* hidden_out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* The packed entry: sequences as ids into a table that input_proj went over once, live rows only.
 * In the reference every position is a row of one of two fixed tables (T5/data_vision.py:119-154: the
 * user's profile vector, then the history's item vectors), so the per-batch host gather, the upload
 * and the 768 -> d_model projection of vectors that never change are not needed.
 *
 * gr_t5_embed_project_f32: projected[r] = table[r] . in_w^T + in_b for table [R, in_dim] into projected
 * [R, d_model] -- the launch gr_t5_embed_f32 makes first, so row r holds the bits that call puts into x
 * for that vector.  R 1..2^24 (GR_ERR_ARG below, GR_ERR_UNSUPPORTED above); both pointers 16-byte
 * aligned.  One launch, no workspace.
 *
 * gr_t5_embed_rows_f32: user b is rows [offsets[b], offsets[b + 1]) of tokens [rows], 1..32 of them, at
 * positions 0..len_b - 1; tokens index projected [R, d_model]; offsets [B + 1] is device int64 with
 * offsets[0] = 0 and offsets[B] = rows; rows is the host's count (it sizes the workspace and the grids).
 * 1 + 4 n_layers + 3 launches, nothing synchronises: a gather x[row] = projected[tokens[row]]; the
 * blocks with M = rows (attention per user on its own rows and length); pooling over the user's rows;
 * output_proj; normalise.  pred_out [B, out_dim] holds the bits gr_t5_embed_f32 returns for the same
 * sequences right-padded to any S with the matching mask; hidden_out (optional) is [rows, d_model] and
 * holds that call's live rows.  Same repeatability and batch invariance.
 * Envelope: gr_t5_embed_f32's widths; B 0..2^20 (B = 0 with rows = 0: GR_OK, no launch); B <= rows <=
 * 32 B, else GR_ERR_UNSUPPORTED naming rows; R as above.
 * No input value leads outside the buffers: a token outside [0, R) reads the nearest table row, and
 * offsets that do not describe 1..32 rows inside [0, rows) are bounded to some that do; such a user's
 * pred_out row is NaN in every element (and with bad offsets it stores no hidden_out row).  Every other
 * user keeps the bits of the clean call as long as no other user's range overlaps its rows.
 * workspace: gr_t5_embed_rows_workspace_bytes(p, B, rows) bytes, 16-byte aligned (0 outside the
 * envelope); the dense layout with B * S replaced by rows, so (p, B, B * S) gives
 * gr_t5_embed_workspace_bytes(p, B, S). */
int gr_t5_embed_project_f32(const gr_t5_embed_params* p, const float* table, int64_t R, float* projected,
                            void* stream);
size_t gr_t5_embed_rows_workspace_bytes(const gr_t5_embed_params* p, int64_t B, int64_t rows);
int gr_t5_embed_rows_f32(const gr_t5_embed_params* p, const float* projected, int64_t R, const int64_t* tokens,
                         const int64_t* offsets, int64_t B, int64_t rows, float* pred_out, float* hidden_out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* BERT text encoder (transformers' BertModel in eval mode, eager attention, absolute positions) with
 * the reference's two poolings (T5/item_encode.py:11-34,59-78; major-encode/bert_emb.py:131-168).
 *
 * gr_bert_params: dimensions and device pointers (fp32, nn.Linear weights row-major [out, in]).
 * word [vocab_size, H], position [max_position, H], token_type [type_vocab_size, H], emb_ln_w / emb_ln_b
 * [H]; layer[l] = {query.weight, query.bias, key.weight, key.bias, value.weight, value.bias,
 * attention.output.dense.weight, .bias, attention.output.LayerNorm.weight, .bias, intermediate.dense.weight,
 * .bias, output.dense.weight, .bias, output.LayerNorm.weight, .bias}, each 16-byte aligned.
 *
 * Math (all fp32; H = hidden_size = num_heads * head_dim):
 *   x = LN((word[id] + token_type[type]) + position[s]); ids and type ids are clamped into their tables,
 *   token_type_ids NULL means type 0
 *   per layer: a = softmax_j((q_i . k_j) / sqrt(head_dim)) v per head, over the live keys: key j is removed
 *   wherever attention_mask[b, j] == 0 (any other value: live) and gets probability exactly 0 -- what HF's
 *   additive finfo.min gives whenever the sequence has a live key;
 *   x = LN(x + dense(a)); x = LN(x + output(gelu(intermediate(x)))), gelu(t) = t (1 + erf(t / sqrt 2)) / 2
 *   LN(t) = (t - mean) / sqrt(var + eps) * w + b, biased variance, two-pass
 *   GR_BERT_POOL_MEAN_NO_CLS: pooled = sum_{j >= 1, live} x_j / max(#{j >= 1, live}, 1e-9)  (0 when none is)
 *   GR_BERT_POOL_CLS: pooled = x_0.  The pooler (pooler.dense) is never evaluated.
 * Masks with holes are legal.  A sequence with no live key yields zeros in pooled_out and hidden_out.
 * Rows of hidden_out at masked positions are what the encoder computes there; nothing live reads them.
 *
 * gr_bert_embed_f32 enqueues 2 + 7 num_layers launches and never synchronises: embeddings + LN; per layer
 * q/k/v (one GEMM), attention, output dense + residual, LN, intermediate + gelu, output + residual, LN;
 * pooling.  No floating-point atomics: every output element has one fixed summation order that depends
 * on neither B nor the sequence's place in the batch, so two calls give the same bits and a sub-batch
 * gives the bits of the whole batch's rows.
 *   input_ids[B, S] int64; attention_mask[B, S] int64 or NULL (all live); token_type_ids[B, S] int64 or NULL
 *   pooled_out[B, H] (NULL only with GR_BERT_POOL_NONE); hidden_out[B, S, H] 16-byte aligned, or NULL (NULL
 *   with GR_BERT_POOL_NONE is GR_ERR_ARG: nothing to compute)
 * Envelope (GR_ERR_UNSUPPORTED outside, with the field named, before any launch): hidden_size a multiple
 * of 32 in [32, 1024] = num_heads * head_dim, head_dim 32 or 64; intermediate_size a multiple of 32 in
 * [32, 4096]; num_layers 1..24; hidden_act gelu; absolute positions; 1 <= S <= min(512,
 * max_position); B 0..65536 (B = 0: GR_OK, no launch).  B's bound keeps every 1-D grid (at most B * 512 / 64
 * row tiles x 32 column tiles = 2^24 workgroups) and B * num_heads * 4 attention workgroups below 2^31.
 * workspace: gr_bert_embed_workspace_bytes(p, B, S) bytes, 16-byte aligned (0 outside the envelope):
 * B * S * (6 H + intermediate_size) floats. */
#define GR_BERT_MAX_LAYERS 24
#define GR_BERT_ACT_GELU 0
#define GR_BERT_POS_ABSOLUTE 0
#define GR_BERT_POOL_NONE 0
#define GR_BERT_POOL_MEAN_NO_CLS 1
#define GR_BERT_POOL_CLS 2
typedef struct gr_bert_params {
  int32_t vocab_size, hidden_size, num_heads, head_dim, intermediate_size, num_layers, max_position,
      type_vocab_size, hidden_act, position_type;
  float eps, reserved;
  const float* word;
  const float* position;
  const float* token_type;
  const float* emb_ln_w;
  const float* emb_ln_b;
  const float* layer[GR_BERT_MAX_LAYERS][16];
} gr_bert_params;

size_t gr_bert_embed_workspace_bytes(const gr_bert_params* p, int64_t B, int32_t S);
int gr_bert_embed_f32(const gr_bert_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                      const int64_t* token_type_ids, int64_t B, int32_t S, int32_t pooling, float* pooled_out,
                      float* hidden_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same encoder over the rows that matter: gr_bert_embed_ragged_f32 keeps rows [0, len_b) of each
 * sequence, len_b = 1 + its last live position (0 for a sequence with no live key), packed one sequence
 * after the other: row s of sequence b is packed row off[b] + s, off = the exclusive prefix sum of len.
 * Holes inside [0, len_b) stay in as masked rows, position 0 is kept whenever a key is live.  The inputs
 * are gr_bert_embed_f32's [B, S] arrays (same envelope, same clamping, NULL mask = all live), the math
 * is the math above, and every kept row and every pooled vector has the bits gr_bert_embed_f32 gives
 * for the same inputs: a GEMM row's bits do not depend on where the row sits, the attention visits the
 * same key tiles in the same order, and the pooling adds the same rows in position order.
 *
 * rows_bound is the caller's upper bound on off[B] (a host-side mask gives it exactly; B * S is always
 * safe; above B * S counts as B * S; below 1 with B > 0 is GR_ERR_ARG).  It sizes the workspace and every
 * grid; the true count is computed on the device and read there, a workgroup or wave whose rows lie
 * past it exits, and the call never synchronises or reads anything back.  If the mask holds more rows
 * than rows_bound the host cannot know, so the call still returns GR_OK: the offsets kernel sets every
 * length to 0 and a flag, no later kernel touches a row, every element of pooled_out is NaN and
 * row_offsets_out is all zeros with -1 in its last slot.
 *
 * Launches: 2 (lengths: a wave per sequence; offsets: one workgroup, no atomics) + 2 + 7 num_layers.
 *   pooled_out[B, H] (NULL only with GR_BERT_POOL_NONE; zeros for a sequence with no live key)
 *   hidden_rows_out[rows_bound, H] 16-byte aligned or NULL: packed rows of the last hidden state, rows
 *   from off[B] on are left as they were; row_offsets_out[B + 1] = off, or NULL.  GR_BERT_POOL_NONE needs both.
 * Argument checks, error codes and their order are gr_bert_embed_f32's; messages start with
 * "gr_bert_embed_ragged_f32: ".  B = 0: GR_OK, no launch.
 * workspace: gr_bert_embed_ragged_workspace_bytes(p, B, S, rows_bound) bytes, 16-byte aligned (0 outside
 * the envelope or with rows_bound < 1 and B > 0), with R = min(rows_bound, B * S):
 *   4 R (6 H + intermediate_size) + up16(8 (B + 1)) + 16 + up16(4 B) + 16,  up16 = rounded up to 16. */
size_t gr_bert_embed_ragged_workspace_bytes(const gr_bert_params* p, int64_t B, int32_t S, int64_t rows_bound);
int gr_bert_embed_ragged_f32(const gr_bert_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                             const int64_t* token_type_ids, int64_t B, int32_t S, int64_t rows_bound,
                             int32_t pooling, float* pooled_out, float* hidden_rows_out,
                             int64_t* row_offsets_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same encoder with bf16 GEMM operands and fp32 accumulation: an opt-in second precision.  The fp32
 * entries above keep their bits (one GEMM kernel and one layer loop serve both precisions).  bf16 = the
 * upper 16 bits of the RNE-rounded fp32.
 *
 * Numerics contract:
 *   GEMM operands: the A and B operands of the four projections per layer (the fused q/k/v, the attention
 *     output, the intermediate and the output projection) are bf16, round-to-nearest-even from fp32;
 *     accumulation is fp32 in the MFMA accumulator.
 *   Epilogues: bias, exact-erf GELU, residual add, both LayerNorms (two-pass), the softmax's max / exp / sum
 *     and the pooling are fp32.
 *   Residual stream: it and the last hidden state stay fp32; pooled_out and hidden_out are float arrays
 *     exactly as above.
 *   q, k, v: rounded to bf16 once, in the q/k/v GEMM's epilogue, and stored as bf16.
 *   Scores: fp32 from a bf16 MFMA; the 1 / sqrt(head_dim) scale is applied in fp32.
 *   Probabilities: rounded to bf16 where they become the P . v operand: the online softmax rounds the
 *     un-normalised exp(s - running max), and the row sum is taken in fp32 from the same rounded values, so
 *     a row's weights sum to 1 within fp32.
 *   Masking: unchanged: a masked key has probability exactly 0, key tiles with no live key are skipped, a
 *     sequence with no live key gives zeros, masks with holes are legal.
 *   Context and GELU outputs: written as bf16 (they are only ever GEMM A operands).  Each LayerNorm writes
 *     its fp32 row for the residual and a bf16 copy for the next GEMM.
 *   Weights: the six [out, in] matrices per layer are bf16; embedding tables, biases and LayerNorm
 *     parameters stay fp32.
 *   Determinism: every output element has one summation order, which depends on neither B nor the row's
 *     position in a tile nor the tile chosen; no atomics.  A call is bitwise repeatable and batch-invariant,
 *     and the ragged form returns the padded form's bits.
 * Not built: fp16, fp8, a bf16 last hidden state, bf16 embedding tables, training.
 *
 * gr_bert_bf16_params: gr_bert_params' dimensions and fp32 tables;
 *   matrix[l] = {query, key, value, attention.output.dense, intermediate.dense, output.dense}.weight, bf16
 *     [out, in] row-major;
 *   vector[l] = {query.bias, key.bias, value.bias, attention.output.dense.bias, attention.output.LayerNorm.weight,
 *     .bias, intermediate.dense.bias, output.dense.bias, output.LayerNorm.weight, .bias}, fp32;
 *   each 16-byte aligned.
 * gr_bert_embed_bf16 and gr_bert_embed_ragged_bf16 take gr_bert_embed_f32's and gr_bert_embed_ragged_f32's
 * arguments.  The envelope, the clamping, the argument checks, the error codes and their order are those
 * entries'; messages start with the bf16 entry's name; a rows_bound below the mask's count shows the same
 * way (NaN in pooled_out, -1 in the last offset).  Launches: as the fp32 entries.
 * workspace (16-byte aligned; 0 from the query outside the envelope), R rows (B * S, or min(rows_bound, B * S)):
 *   R (18 H + 2 intermediate_size) bytes, each of its six parts rounded up to 16, + 16: the fp32 residual
 *   stream and pre-LayerNorm sum, and the bf16 copies of x, q/k/v, the context and the GELU output; the
 *   ragged query adds up16(8 (B + 1)) + 16 + up16(4 B).
 *   What a test may read after the call; not an interface for callers.  The six parts lie in this order from the
 *   workspace's start, each rounded up to 16 bytes, and on return hold the LAST layer's intermediates (R rows: B * S,
 *   or the packed rows in the ragged form; rows from the packed total on are not written):
 *     x    fp32 [R, H]   the last layer's post-attention LayerNorm output; with hidden_out NULL the final hidden
 *                        state instead
 *     t    fp32 [R, H]   the last layer's x + output.dense(ff) + bias, the input of the final LayerNorm
 *     x16  bf16 [R, H]   the RNE copy of the final LayerNorm's fp32 rows (not zeroed for a sequence with no live
 *                        key: only hidden_out is)
 *     qkv  bf16 [R, 3H]  the last layer's q | k | v
 *     ctx  bf16 [R, H]   the last layer's attention context
 *     ff   bf16 [R, I]   the last layer's GELU output
 *   tests/bert_bf16_stages.py checks each stage in float64 on these operands. */
typedef struct gr_bert_bf16_params {
  int32_t vocab_size, hidden_size, num_heads, head_dim, intermediate_size, num_layers, max_position,
      type_vocab_size, hidden_act, position_type;
  float eps, reserved;
  const float* word;
  const float* position;
  const float* token_type;
  const float* emb_ln_w;
  const float* emb_ln_b;
  const uint16_t* matrix[GR_BERT_MAX_LAYERS][6];
  const float* vector[GR_BERT_MAX_LAYERS][10];
} gr_bert_bf16_params;

size_t gr_bert_embed_bf16_workspace_bytes(const gr_bert_bf16_params* p, int64_t B, int32_t S);
int gr_bert_embed_bf16(const gr_bert_bf16_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                       const int64_t* token_type_ids, int64_t B, int32_t S, int32_t pooling, float* pooled_out,
                       float* hidden_out, void* workspace, size_t workspace_bytes, void* stream);
size_t gr_bert_embed_ragged_bf16_workspace_bytes(const gr_bert_bf16_params* p, int64_t B, int32_t S,
                                                 int64_t rows_bound);
int gr_bert_embed_ragged_bf16(const gr_bert_bf16_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                              const int64_t* token_type_ids, int64_t B, int32_t S, int64_t rows_bound,
                              int32_t pooling, float* pooled_out, float* hidden_rows_out,
                              int64_t* row_offsets_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GR_AMD_H */
