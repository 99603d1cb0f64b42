// SASRec eval forward / predict on gfx950 (replaces SASRec/model.py:49-108 and the
// nn.MultiheadAttention math of torch functional.py:6576-6600; the evaluate.py:27-32 rank tail).
//
// Layer-wise pipeline over the batch (B*n token rows), all buffers in the caller's workspace:
//   embed      X = M[s] + P[t]                                  (model.py:58-60, exact fp32 add)
//   per block  H = LN_a(X); QKV = H.W_in^T + b_in                (model.py:80, functional.py:5823)
//              O = causal softmax((q*sqrt(1/hd)).k^T) . v        (functional.py:6578-6594)
//              X = X + (O.W_o^T + b_o)                           (functional.py:6600, model.py:84)
//              H = LN_f(X); F = relu(H.W1^T + b1); X = X + (F.W2^T + b2)   (model.py:92-94)
//   last LN    on every row (forward) or on the last position only (predict, model.py:104)
//   scoring    logits = h . M^T                                   (model.py:107)
// The dead W_Q/W_K/W_V projections (model.py:63-65) are elided: no output depends on them.
#include <cmath>

#include "gr_common.h"

namespace gr {

// ---------------------------------------------------------------------------------- embedding
__global__ __launch_bounds__(256) void embed_kernel(const int64_t* __restrict__ seqs, int64_t rows,
                                                    int n, int d, const float* __restrict__ item,
                                                    int64_t item_rows,
                                                    const float* __restrict__ pos,
                                                    float* __restrict__ x, int32_t* err) {
  const int d4 = d >> 2;
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= rows * d4) return;
  const int64_t row = f / d4;
  const int c = (int)(f % d4) * 4;
  const int t = (int)(row % n);
  int64_t id = seqs[row];
  if (id < 0 || id >= item_rows) {  // torch raises IndexError here; flag it and read the pad row
    set_err(err, 1);
    id = 0;
  }
  const f32x4 a = *reinterpret_cast<const f32x4*>(item + id * d + c);
  const f32x4 p = *reinterpret_cast<const f32x4*>(pos + (int64_t)t * d + c);
  *reinterpret_cast<f32x4*>(x + row * d + c) = a + p;
}

// Row n-1 of every sequence of a [B, n, d] activation -> compact [B, d] (the last-position rows a
// last_only forward carries through its final block).
__global__ __launch_bounds__(256) void gather_last_kernel(const float* __restrict__ src, int64_t B,
                                                          int n, int d, float* __restrict__ dst) {
  const int d4 = d >> 2;
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= B * d4) return;
  const int64_t b = f / d4;
  const int c = (int)(f % d4) * 4;
  *reinterpret_cast<f32x4*>(dst + b * d + c) =
      *reinterpret_cast<const f32x4*>(src + (b * n + n - 1) * d + c);
}

// ---------------------------------------------------------------------------------- layernorm
// One wave per row: mean, biased variance, (x - mean) * rsqrt(var + eps) * w + b (F.layer_norm).
// Input row r is read at in + (r * in_stride + in_offset) * d (in_stride = n, in_offset = n-1
// selects the last position of every sequence).
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ in, int64_t rows,
                                                        int d, int64_t in_stride, int64_t in_offset,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ b, float eps,
                                                        float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = in + (row * in_stride + in_offset) * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xr[c];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)d;
  float v = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float t = xr[c] - mean;
    v = fmaf(t, t, v);
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const float rstd = 1.0f / sqrtf(v / (float)d + eps);
  float* yr = out + row * d;
  for (int c = lane; c < d; c += 64) yr[c] = (xr[c] - mean) * rstd * w[c] + b[c];
}

// ---------------------------------------------------------------------------------- attention
// Causal multi-head attention for one (sequence, head) and a tile of QT query rows.
// qkv: [B, n, 3d] rows (q | k | v, head h at columns h*hd); out: [B, n, d].
// Scores of the tile's rows against keys [0, q0+QT) live in LDS, softmax is exact (row max,
// exp, sum, divide), then O = P . V.  Keys beyond a row's causal limit are -inf -> weight 0.
constexpr int ATT_QT = 16;
constexpr int ATT_KC = 64;

__global__ __launch_bounds__(256) void causal_attn_kernel(const float* __restrict__ qkv,
                                                          float* __restrict__ out, int n, int H,
                                                          int hd, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int hp = hd + 1;
  float* Qs = sm;                        // [QT][hd+1]
  float* KVs = Qs + ATT_QT * hp;          // [KC][hd+1]
  float* S = KVs + ATT_KC * hp;           // [QT][n]
  const int tid = threadIdx.x;
  const int b = blockIdx.x / H, hh = blockIdx.x % H;
  const int q0 = blockIdx.y * ATT_QT;
  const int d = H * hd;
  const int64_t rs = 3LL * d;
  const float* base = qkv + (int64_t)b * n * rs + hh * hd;
  const int qn = min(ATT_QT, n - q0);
  const int kmax = q0 + qn;

  for (int i = tid; i < qn * hd; i += 256) {
    const int qi = i / hd, c = i % hd;
    Qs[qi * hp + c] = base[(int64_t)(q0 + qi) * rs + c] * scale;  // q * sqrt(1/hd) (functional.py:6578)
  }
  for (int k0 = 0; k0 < kmax; k0 += ATT_KC) {
    const int kn = min(ATT_KC, kmax - k0);
    __syncthreads();
    for (int i = tid; i < kn * hd; i += 256) {
      const int j = i / hd, c = i % hd;
      KVs[j * hp + c] = base[(int64_t)(k0 + j) * rs + d + c];
    }
    __syncthreads();
    for (int i = tid; i < ATT_QT * ATT_KC; i += 256) {
      const int qi = i / ATT_KC, j = i % ATT_KC;
      if (qi < qn && j < kn) {
        const int kj = k0 + j;
        float s = -__builtin_inff();
        if (kj <= q0 + qi) {
          s = 0.f;
          const float* qr = Qs + qi * hp;
          const float* kr = KVs + j * hp;
          for (int c = 0; c < hd; ++c) s = fmaf(qr[c], kr[c], s);
        }
        S[qi * n + kj] = s;
      }
    }
  }
  __syncthreads();
  // softmax: one wave per row
  const int lane = tid & 63, wave = tid >> 6;
  for (int qi = wave; qi < qn; qi += 4) {
    float* sr = S + qi * n;
    const int lim = q0 + qi + 1;  // causal keys [0, lim)
    float m = -__builtin_inff();
    for (int j = lane; j < lim; j += 64) m = fmaxf(m, sr[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.f;
    for (int j = lane; j < lim; j += 64) {
      const float e = expf(sr[j] - m);
      sr[j] = e;
      sum += e;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    for (int j = lane; j < lim; j += 64) sr[j] = sr[j] / sum;
    for (int j = lim + lane; j < kmax; j += 64) sr[j] = 0.f;
  }
  // O = P . V
  constexpr int MAXO = ATT_QT * 128 / 256;  // outputs per thread for hd <= 128
  float acc[MAXO];
#pragma unroll
  for (int u = 0; u < MAXO; ++u) acc[u] = 0.f;
  for (int k0 = 0; k0 < kmax; k0 += ATT_KC) {
    const int kn = min(ATT_KC, kmax - k0);
    __syncthreads();
    for (int i = tid; i < kn * hd; i += 256) {
      const int j = i / hd, c = i % hd;
      KVs[j * hp + c] = base[(int64_t)(k0 + j) * rs + 2 * d + c];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < MAXO; ++u) {
      const int i = tid + 256 * u;
      if (i < qn * hd) {
        const int qi = i / hd, c = i % hd;
        const float* pr = S + qi * n + k0;
        float a = acc[u];
        for (int j = 0; j < kn; ++j) a = fmaf(pr[j], KVs[j * hp + c], a);
        acc[u] = a;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < MAXO; ++u) {
    const int i = tid + 256 * u;
    if (i < qn * hd) {
      const int qi = i / hd, c = i % hd;
      out[((int64_t)b * n + q0 + qi) * d + hh * hd + c] = acc[u];
    }
  }
}

// ---------------------------------------------------------------------------------- rank
// rank[b] = 1 + #{j : l'[b,j] > l'[b,t]} with l'[b,0] = -1e9 when mask_col0 (evaluate.py:27-32).
__global__ __launch_bounds__(256) void rank_kernel(const float* __restrict__ logits, int64_t cols,
                                                   int64_t ld, const int64_t* __restrict__ targets,
                                                   int mask0, int64_t* __restrict__ ranks) {
  __shared__ int64_t part[4];
  const int64_t b = blockIdx.x;
  const float* row = logits + b * ld;
  const int64_t t = targets[b];
  if (t < 0 || t >= cols) {  // torch.gather raises here; report rank -1
    if (threadIdx.x == 0) ranks[b] = -1;
    return;
  }
  const float pad = -1e9f;
  float ts = (t == 0 && mask0) ? pad : row[t];
  int64_t cnt = 0;
  for (int64_t j = threadIdx.x; j < cols; j += 256) {
    const float v = (j == 0 && mask0) ? pad : row[j];
    cnt += v > ts ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) ranks[b] = part[0] + part[1] + part[2] + part[3] + 1;
}

// ---------------------------------------------------------------------------------- plan
// Everything a forward decides before it launches, from the shape, the batch, the options and the
// alignment of the parameters, as GR_SAS_* bits (gr_sasrec_plan returns their union).  The driver
// below only executes it: no launch is ever tried to find out whether it runs.
struct SasPlan {
  int pipe;     // GR_SAS_FUSED, GR_SAS_ROWTILE or GR_SAS_LAYERWISE
  int block0;   // row-tile: GR_SAS_B0_EMBED_PROJ, _EMBED_LN_LINEAR or _EMBED_LN
  int attn;     // GR_SAS_ATTN_* of the blocks that run attention; 0: no block does
  int flags;    // GR_SAS_FUSED_TWO_WAVES, _FUSED_MISALIGNED, _ATTN_LAST_TILE, _TAIL, _TAIL_VALU, _PRUNED
  bool has(int f) const { return flags & f; }
};

// What block i's post_attn kernel (row-tile) appends to the block: the LayerNorm its consumer reads
// (the next block's LN_a, or the last one) and that block's Q|K|V in-projection -- none (wn = null)
// after the final block and before an H-form tail, which works on LN_a(X): no K|V of its B n rows.
struct SasNext {
  const float *ln_w, *ln_b, *wn, *bn;
  int nout;
};
static SasNext next_of(const gr_sasrec_params* p, int i, bool tail) {
  const int nb = p->n_blocks;
  if (i == nb - 1) return {p->last_ln_w, p->last_ln_b, nullptr, nullptr, 0};
  if (tail && i == nb - 2) return {p->attn_ln_w[i + 1], p->attn_ln_b[i + 1], nullptr, nullptr, 0};
  return {p->attn_ln_w[i + 1], p->attn_ln_b[i + 1], p->in_proj_w[i + 1], p->in_proj_b[i + 1], 3 * p->d};
}

// p has passed check_params (the workspace queries: at least n_heads >= 1).
static SasPlan sas_plan(const gr_sasrec_params* p, int64_t B, int32_t n, int last_only) {
  const int d = p->d, H = p->n_heads, hd = d / H, nb = p->n_blocks, cus = cu_count();
  const int64_t rows = B * n, fused = option("sas_fused");
  if (const int ok = fused >= 1 ? gr_sasrec_fused_ok(p, n) : 0) {
    // Which form (sas_fused 2 = auto, 3 = always two waves).  The one-wave kernel runs in rounds of
    // 4 x CUs sequences (one wave per SIMD, ~58 us per round at C3's shape); the two-wave kernel takes
    // 0.63 of that round for up to 2 x CUs sequences (one wave per SIMD) and ~0.5 round per further
    // 2 x CUs (two waves per SIMD overlap little: the MFMA and VALU work per SIMD is the bound), so
    // it wins when k = ceil(B / 2 CUs) is odd (profiles/r05/ab_fused_waves.txt).
    const int64_t k2 = (B + 2 * cus - 1) / (2 * cus), k1 = (B + 4 * cus - 1) / (4 * cus);
    const double t2 = k2 == 1 ? 0.63 : 0.5 * (double)k2 + 0.03;
    const bool two = n > 32 && (fused == 3 || (fused == 2 && t2 < (double)k1));
    return {GR_SAS_FUSED, 0, 0, (two ? GR_SAS_FUSED_TWO_WAVES : 0) | (ok < 0 ? GR_SAS_FUSED_MISALIGNED : 0)};
  }
  const int form = gr_attn_form(B, n, H, hd, option("attn_k16") == 1);
  // the final block of a last-position forward: the one-query tail wherever its kernel runs (its
  // VALU reductions when B <= CUs: one sequence per CU is latency-bound)
  const bool tail = last_only && gr_sasrec_tail_ok(p, nb - 1, B, n);
  const int tail_bits = !tail ? 0 : B <= cus ? GR_SAS_TAIL | GR_SAS_TAIL_VALU : GR_SAS_TAIL;
  const int attn = nb - tail > 0 ? form : 0;   // the tail replaces the final block's attention
  // d = 128 (C5): the row-tile kernels, when each launch run_rowtile will make is one its launcher
  // takes; a last-position forward ends in the tail there.  Block 0: embed + LN_a0 + in-projection
  // in one kernel with 32-column slices of W_in resident in registers (embed_proj_kernel, option
  // emb_proj), else embed + LN_a0 -> H and a plain GEMM (folding the GEMM into embed_ln_kernel
  // measured slower: 218 us vs 37 + 133 at C5); later blocks fold it into post_attn (198 us vs
  // 115 + 97 for the final block's K|V).
  if (option("sas_rowtile") == 1 && nb >= 1 && gr_rowtile_shape_ok(p) && gr_attn_mfma_hd(hd) &&
      (!last_only || tail) && attn != GR_SAS_ATTN_SCALAR) {
    const bool ln = gr_embed_ln_ok(p, rows, nullptr, nullptr, 0);
    const int b0 = !attn ? (ln ? GR_SAS_B0_EMBED_LN : 0)
                   : option("emb_proj") == 1 && gr_embed_proj_ok(p, rows, p->in_proj_w[0], p->in_proj_b[0], 3 * d)
                       ? GR_SAS_B0_EMBED_PROJ
                       : (ln ? GR_SAS_B0_EMBED_LN_LINEAR : 0);
    bool ok = b0 != 0;
    for (int i = 0; ok && i < nb - tail; ++i) {
      const SasNext nx = next_of(p, i, tail);
      ok = gr_post_attn_ok(p, i, nx.ln_w, nx.ln_b, nx.wn, nx.bn, nx.nout, rows);
    }
    if (ok) return {GR_SAS_ROWTILE, b0, attn, tail_bits};
  }
  // layer-wise without the tail: only position n-1 of the final block is needed past its attention
  // (and of that only the last query tile, which the scalar kernel cannot select), when that saves work
  const bool pruned = last_only && !tail && nb >= 1 && n >= 2 && (int64_t)n * p->mlp >= 2LL * d + p->mlp;
  const int pruned_bits = !pruned ? 0 : attn != GR_SAS_ATTN_SCALAR ? GR_SAS_PRUNED | GR_SAS_ATTN_LAST_TILE : GR_SAS_PRUNED;
  return {GR_SAS_LAYERWISE, 0, attn, tail_bits | pruned_bits};
}

// ---------------------------------------------------------------------------------- driver
struct SasWs {
  float *x, *h, *qkv, *o, *f;
};

// The fused kernel (sasrec_fused.hip) needs only the [B, d] last hidden states.
static size_t ws_layout(const SasPlan& s, const gr_sasrec_params* p, int64_t B, int32_t n, char* base, SasWs* w) {
  auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  if (s.pipe == GR_SAS_FUSED) {
    if (w) *w = SasWs{nullptr, at(0), nullptr, nullptr, nullptr};
    return align_up((size_t)B * p->d * 4, 256) + 256;
  }
  const size_t rows = (size_t)B * n;
  const size_t sx = align_up(rows * p->d * 4, 256);
  const size_t sq = align_up(rows * 3 * p->d * 4, 256);
  const size_t sf = align_up(rows * (size_t)p->mlp * 4, 256);
  if (w) *w = SasWs{at(0), at(sx), at(3 * sx), at(2 * sx), at(3 * sx + sq)};   // in memory: x, h, o, qkv, f
  return 3 * sx + sq + sf + 256;
}

static int check_params(const gr_sasrec_params* p, int64_t B, int32_t n) {
  if (!p) return fail(GR_ERR_ARG, "sasrec: null params");
  if (p->d < 4 || p->d % 4 || p->n_heads < 1 || p->d % p->n_heads)
    return fail(GR_ERR_UNSUPPORTED, "sasrec: d must be a multiple of 4 and of num_heads");
  if (p->d / p->n_heads > 128) return fail(GR_ERR_UNSUPPORTED, "sasrec: head dim > 128");
  if (p->mlp < 4 || p->mlp % 4) return fail(GR_ERR_UNSUPPORTED, "sasrec: mlp_layer must be a multiple of 4");
  if (p->n_blocks < 0) return fail(GR_ERR_ARG, "sasrec: num_blocks < 0");
  if (n < 1 || n > p->max_len) return fail(GR_ERR_ARG, "sasrec: sequence length outside [1, max_len]");
  if (n > 1024) return fail(GR_ERR_UNSUPPORTED, "sasrec: sequence length > 1024");
  if (B < 0) return fail(GR_ERR_ARG, "sasrec: B < 0");
  if (!p->item_emb || !p->pos_emb || !p->last_ln_w || !p->last_ln_b || p->item_rows < 1)
    return fail(GR_ERR_ARG, "sasrec: null embedding / last layernorm");
  if (p->item_rows > 0x7fffffffLL) return fail(GR_ERR_UNSUPPORTED, "sasrec: item_rows >= 2^31");
  if (!aligned16(p->item_emb) || !aligned16(p->pos_emb))
    return fail(GR_ERR_ARG, "sasrec: embeddings must be 16-byte aligned");
  return GR_OK;
}

// The plan has asked every launcher's predicate: GR_ERR_UNSUPPORTED from one of them now is a bug
// of this file, reported as such and never answered with another path.
static int planned(int rc, const char* launcher) {
  if (rc != GR_ERR_UNSUPPORTED) return rc;
  return fail(rc, std::string("sasrec: ") + launcher + " refused a launch its predicate had accepted");
}

static int run_layernorm(const float* in, int64_t rows, int d, int64_t stride, int64_t off,
                         const float* w, const float* b, float eps, float* out, hipStream_t st) {
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, in, rows,
                     d, stride, off, w, b, eps, out);
  return check_launch("sasrec layernorm");
}

static int run_gather_last(const float* src, int64_t B, int n, int d, float* dst, hipStream_t st) {
  const int64_t tot = B * (d / 4);
  hipLaunchKernelGGL(gather_last_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, src, B, n, d, dst);
  return check_launch("sasrec gather");
}

static size_t scalar_attn_lds(int hd, int n) {
  return (size_t)(ATT_QT + ATT_KC) * (hd + 1) * 4 + (size_t)ATT_QT * n * 4;
}

// w.qkv -> w.o by the planned kernel; last_tile: the query tile of position n-1 only.
static int run_attention(const SasPlan& s, const SasWs& w, int64_t B, int n, int H, int hd, bool last_tile,
                         hipStream_t st) {
  if (s.attn != GR_SAS_ATTN_SCALAR)
    return planned(gr_attn_mfma_launch(s.attn, w.qkv, w.o, B, n, H, hd, sas_scale(hd), last_tile, st),
                   "gr_attn_mfma_launch");
  hipLaunchKernelGGL(causal_attn_kernel, dim3((unsigned)(B * H), (unsigned)((n + ATT_QT - 1) / ATT_QT)), dim3(256),
                     scalar_attn_lds(hd, n), st, w.qkv, w.o, n, H, hd, sas_scale(hd));
  return check_launch("sasrec attention");
}

// d = 128 (C5): row-tile fusions (sasrec_rowtile.hip) between the attention launches --
//   embed + LN_a0 + in-proj | per block: attention, post_attn (out-proj + residual + LN_f + FFN +
//   residual + the next LayerNorm + the next in-proj) | last position: the tail on LN_a(X) in w.qkv.
// h: the [B, d] (tail) or [B*n, d] output; the last block's post_attn writes LN_last(X) into it.
static int run_rowtile(const gr_sasrec_params* p, const SasPlan& s, const int64_t* seqs, int64_t B, int32_t n,
                       const SasWs& w, int32_t* err, float* h, hipStream_t st) {
  const int d = p->d, H = p->n_heads, nb = p->n_blocks;
  const int64_t rows = B * n;
  const bool tail = s.has(GR_SAS_TAIL);
  int rc;
  if (s.block0 == GR_SAS_B0_EMBED_PROJ) {
    rc = planned(gr_embed_proj_launch(p, seqs, rows, n, p->in_proj_w[0], p->in_proj_b[0], 3 * d, w.x, w.qkv, err, st),
                 "gr_embed_proj_launch");
  } else {   // LN_a0(X): block 0's in-projection reads it from w.h, a one-block tail from w.qkv
    float* ln = s.block0 == GR_SAS_B0_EMBED_LN ? w.qkv : w.h;
    rc = planned(gr_embed_ln_launch(p, seqs, rows, n, nullptr, nullptr, 0, w.x, ln, err, st), "gr_embed_ln_launch");
    if (!rc && ln == w.h)
      rc = gr_linear_launch(w.h, rows, d, p->in_proj_w[0], 3 * d, p->in_proj_b[0], nullptr, 0, GR_ACT_NONE, w.qkv, 3 * d, st);
  }
  for (int i = 0; !rc && i < nb; ++i) {
    const bool last = i == nb - 1;
    if (last && tail)
      return planned(gr_sasrec_tail_h_launch(p, i, w.x, w.qkv, B, n, h, s.has(GR_SAS_TAIL_VALU), st),
                     "gr_sasrec_tail_h_launch");
    rc = run_attention(s, w, B, n, H, d / H, false, st);
    if (rc) return rc;
    const SasNext nx = next_of(p, i, tail);
    rc = planned(gr_post_attn_launch(p, i, nx.ln_w, nx.ln_b, nx.wn, nx.bn, nx.nout, w.o, w.x, last ? h : w.qkv, rows, st),
                 "gr_post_attn_launch");
  }
  return rc;
}

// Block i past its attention, on m rows: x += o.W_o^T + b_o; h = LN_f(x); f = relu(h.W_1^T + b_1);
// x += f.W_2^T + b_2 (model.py:84-94).
static int run_block_rest(const gr_sasrec_params* p, int i, const float* o, float* x, float* h, float* f, int64_t m,
                          hipStream_t st) {
  const int d = p->d, mlp = p->mlp;
  int rc = gr_linear_launch(o, m, d, p->out_proj_w[i], d, p->out_proj_b[i], x, d, GR_ACT_NONE, x, d, st);
  if (!rc) rc = run_layernorm(x, m, d, 1, 0, p->ffn_ln_w[i], p->ffn_ln_b[i], p->eps, h, st);
  if (!rc) rc = gr_linear_launch(h, m, d, p->ffn1_w[i], mlp, p->ffn1_b[i], nullptr, 0, GR_ACT_RELU, f, mlp, st);
  if (!rc) rc = gr_linear_launch(f, m, mlp, p->ffn2_w[i], d, p->ffn2_b[i], x, d, GR_ACT_NONE, x, d, st);
  return rc;
}

// One kernel per op.  last_only: the caller needs position n-1 only (model.py:104), so the FINAL
// block is the one-query tail (sasrec_tail.hip) on LN_a(X), which writes the final hidden states,
// last LayerNorm included; or, pruned, its attention runs for the query tile holding n-1 and the
// rest of the block on the B last rows -- the same kernels and per-row instruction sequence as the
// full forward (bitwise equal).  Earlier blocks still produce every position (its keys and values).
static int run_layerwise(const gr_sasrec_params* p, const SasPlan& s, const int64_t* seqs, int64_t B, int32_t n,
                         const SasWs& w, int32_t* err, int last_only, float* h, hipStream_t st) {
  const int d = p->d, H = p->n_heads, nb = p->n_blocks;
  const int64_t rows = B * n, tot = rows * (d / 4);
  hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, seqs, rows, n, d,
                     p->item_emb, p->item_rows, p->pos_emb, w.x, err);
  int rc = check_launch("sasrec embed");
  if (rc) return rc;
  if (s.attn == GR_SAS_ATTN_SCALAR && scalar_attn_lds(d / H, n) > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&causal_attn_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)scalar_attn_lds(d / H, n)) != hipSuccess)
    return fail(GR_ERR_HIP, "sasrec attention: cannot raise the LDS limit");
  for (int i = 0; i < nb; ++i) {
    const bool last = i == nb - 1;
    rc = run_layernorm(w.x, rows, d, 1, 0, p->attn_ln_w[i], p->attn_ln_b[i], p->eps, w.h, st);
    if (rc) return rc;
    if (last && s.has(GR_SAS_TAIL))
      return planned(gr_sasrec_tail_h_launch(p, i, w.x, w.h, B, n, h, s.has(GR_SAS_TAIL_VALU), st),
                     "gr_sasrec_tail_h_launch");
    rc = gr_linear_launch(w.h, rows, d, p->in_proj_w[i], 3 * d, p->in_proj_b[i], nullptr, 0, GR_ACT_NONE, w.qkv, 3 * d, st);
    if (!rc) rc = run_attention(s, w, B, n, H, d / H, last && s.has(GR_SAS_ATTN_LAST_TILE), st);
    if (rc) return rc;
    if (last && s.has(GR_SAS_PRUNED)) {
      float* xl = w.f;                 // [B, d] residual stream of the last positions
      float* hl = w.f + B * d;         // [B, d] layernorm output
      float* fl = w.f + 2 * B * d;     // [B, mlp] FFN hidden
      float* ol = w.h;                 // [B, d] attention output rows
      rc = run_gather_last(w.o, B, n, d, ol, st);
      if (!rc) rc = run_gather_last(w.x, B, n, d, xl, st);
      if (!rc) rc = run_block_rest(p, i, ol, xl, hl, fl, B, st);
      if (!rc) rc = run_layernorm(xl, B, d, 1, 0, p->last_ln_w, p->last_ln_b, p->eps, h, st);
      return rc;
    }
    rc = run_block_rest(p, i, w.o, w.x, w.h, w.f, rows, st);
    if (rc) return rc;
  }
  // the last LayerNorm: on position n-1 of every sequence, or on every row
  return run_layernorm(w.x, last_only ? B : rows, d, last_only ? n : 1, last_only ? n - 1 : 0, p->last_ln_w,
                       p->last_ln_b, p->eps, h, st);
}

// Runs a plan.  *hidden: the final hidden states, last LayerNorm applied ([B, d] of a last-position
// forward, else [B*n, d]), in `out` or, without one, in the workspace: w.h after the fused kernel, else
// w.o (free by then).  init_ranks: gr_sasrec_rank_f32's ranks, which the fused kernel starts at 1.
static int sas_run(const gr_sasrec_params* p, const SasPlan& s, const int64_t* seqs, int64_t B, int32_t n,
                   const SasWs& w, int last_only, float* out, int32_t* err, hipStream_t st, float** hidden,
                   int64_t* init_ranks = nullptr) {
  float* h = *hidden = out ? out : s.pipe == GR_SAS_FUSED ? w.h : w.o;
  if (s.pipe != GR_SAS_FUSED)
    return s.pipe == GR_SAS_ROWTILE ? run_rowtile(p, s, seqs, B, n, w, err, h, st)
                                    : run_layerwise(p, s, seqs, B, n, w, err, last_only, h, st);
  if (s.has(GR_SAS_FUSED_MISALIGNED) || !aligned16(h))
    return fail(GR_ERR_UNSUPPORTED, "sasrec: the fused forward (n <= 64, d <= 64) needs every block parameter, the "
                                    "last layernorm and the output non-null and 16-byte aligned");
  return planned(gr_sasrec_fused_launch(p, seqs, B, n, h, last_only, s.has(GR_SAS_FUSED_TWO_WAVES), err, st, init_ranks, 1),
                 "gr_sasrec_fused_launch");
}

}  // namespace gr

extern "C" int32_t gr_sasrec_plan(const gr_sasrec_params* p, int64_t B, int32_t n, int32_t last_only) {
  gr::clear_error();
  if (const int rc = gr::check_params(p, B, n)) return rc;
  const gr::SasPlan s = gr::sas_plan(p, B, n, last_only);
  return s.pipe | s.block0 | s.attn | s.flags;
}

extern "C" size_t gr_sasrec_workspace_bytes(const gr_sasrec_params* p, int64_t B, int32_t n) {
  if (!p || B < 0 || n < 1 || p->n_heads < 1) return 0;
  return gr::ws_layout(gr::sas_plan(p, B, n, 0), p, B, n, nullptr, nullptr);
}

// Argument checks, the plan, and the workspace laid out for it.
static int sas_prepare(const gr_sasrec_params* p, int64_t B, int32_t n, int last_only, void* ws, size_t wsb,
                       gr::SasWs* w, gr::SasPlan* s) {
  using namespace gr;
  int rc = check_params(p, B, n);
  if (rc) return rc;
  *s = sas_plan(p, B, n, last_only);
  const size_t need = ws_layout(*s, p, B, n, nullptr, nullptr);
  if (!ws || wsb < need)
    return fail(GR_ERR_WORKSPACE, "sasrec: workspace too small (need " + std::to_string(need) + " bytes)");
  char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
  ws_layout(*s, p, B, n, base, w);
  return GR_OK;
}

extern "C" int gr_sasrec_forward_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B,
                                     int32_t n, float* out, int32_t last_only, void* workspace,
                                     size_t workspace_bytes, int32_t* err_flag, void* stream) {
  using namespace gr;
  clear_error();
  SasWs w;
  SasPlan s;
  const int rc = sas_prepare(p, B, n, last_only, workspace, workspace_bytes, &w, &s);
  if (rc) return rc;
  if (B == 0) return GR_OK;
  if (!seqs || !out) return fail(GR_ERR_ARG, "gr_sasrec_forward_f32: null seqs / out");
  float* h;
  return sas_run(p, s, seqs, B, n, w, last_only, out, err_flag, reinterpret_cast<hipStream_t>(stream), &h);
}

static int score_hidden(const gr_sasrec_params* p, const float* h, int64_t B, float* logits, int64_t ld,
                        hipStream_t st) {
  using namespace gr;
  int rc = gr_score_launch(h, B, p->d, p->item_emb, p->item_rows, logits, ld, st);
  if (rc != GR_ERR_UNSUPPORTED) return rc;
  clear_error();
  return gr_linear_launch(h, B, p->d, p->item_emb, (int32_t)p->item_rows, nullptr, nullptr, 0,
                          GR_ACT_NONE, logits, ld, st);
}

extern "C" int gr_sasrec_predict_ld_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B,
                                        int32_t n, float* logits, int64_t ld, void* workspace,
                                        size_t workspace_bytes, int32_t* err_flag, void* stream) {
  using namespace gr;
  clear_error();
  if (p && ld < p->item_rows)
    return fail(GR_ERR_ARG, "gr_sasrec_predict_ld_f32: ld < item_rows");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SasWs w;
  SasPlan s;
  int rc = sas_prepare(p, B, n, 1, workspace, workspace_bytes, &w, &s);
  if (rc) return rc;
  if (B == 0) return GR_OK;
  if (!seqs || !logits) return fail(GR_ERR_ARG, "gr_sasrec_predict: null seqs / logits");
  float* h;
  rc = sas_run(p, s, seqs, B, n, w, 1, nullptr, err_flag, st, &h);
  if (rc) return rc;
  return score_hidden(p, h, B, logits, ld, st);
}

extern "C" int gr_sasrec_predict_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B,
                                     int32_t n, float* logits, void* workspace,
                                     size_t workspace_bytes, int32_t* err_flag, void* stream) {
  return gr_sasrec_predict_ld_f32(p, seqs, B, n, logits, p ? p->item_rows : 0, workspace,
                                  workspace_bytes, err_flag, stream);
}

extern "C" int gr_rank_f32(const float* logits, int64_t B, int64_t cols, int64_t ld,
                           const int64_t* targets, int32_t mask_col0, int64_t* ranks_out,
                           void* stream) {
  using namespace gr;
  clear_error();
  if (B < 0 || cols < 1 || ld < cols) return fail(GR_ERR_ARG, "gr_rank_f32: bad shape");
  if (B == 0) return GR_OK;
  if (!logits || !targets || !ranks_out) return fail(GR_ERR_ARG, "gr_rank_f32: null pointer");
  if (B > 0x7fffffffLL) return fail(GR_ERR_UNSUPPORTED, "gr_rank_f32: B >= 2^31");
  hipLaunchKernelGGL(rank_kernel, dim3((unsigned)B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     logits, cols, ld, targets, mask_col0, ranks_out);
  return check_launch("gr_rank_f32");
}

// evaluate.py:26-32 for one batch in ONE call: the last hidden states of the
// forward (the fused kernel also writes every rank's starting 1, so the count needs no fill), then
// one count launch that forms each target logit with the scoring chain (gr_score_pairs_f32's tile)
// and counts the strictly greater logits (gr_score_count_gt_ws_f32's kernel) -- two launches (three
// when the count spreads over the workspace copies), the [B, item_rows] logits never written.
extern "C" size_t gr_sasrec_rank_workspace_bytes(const gr_sasrec_params* p, int64_t B, int32_t n) {
  const size_t fwd = gr_sasrec_workspace_bytes(p, B, n);
  return fwd ? fwd + gr::align_up((size_t)B * 4, 256) + 256 : 0;
}

extern "C" int gr_sasrec_rank_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                                  const int64_t* targets, int32_t mask_col0, int64_t* ranks_out,
                                  void* workspace, size_t workspace_bytes, void* count_ws,
                                  size_t count_ws_bytes, int32_t* err_flag, void* stream) {
  using namespace gr;
  clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!p) return fail(GR_ERR_ARG, "gr_sasrec_rank_f32: null params");
  const size_t need = gr_sasrec_rank_workspace_bytes(p, B, n);
  if (!workspace || workspace_bytes < need)
    return fail(GR_ERR_WORKSPACE, "gr_sasrec_rank_f32: workspace too small (need " + std::to_string(need) + " bytes)");
  SasWs w;
  SasPlan s;
  int rc = sas_prepare(p, B, n, 1, workspace, workspace_bytes, &w, &s);
  if (rc) return rc;
  if (B == 0) return GR_OK;
  if (!seqs || !targets || !ranks_out) return fail(GR_ERR_ARG, "gr_sasrec_rank_f32: null seqs / targets / ranks");
  if (p->d != 16 && p->d != 32 && p->d != 64 && p->d != 128)
    return fail(GR_ERR_UNSUPPORTED, "gr_sasrec_rank_f32: d must be 16, 32, 64 or 128 (the fused rank's widths)");
  float* h;
  rc = sas_run(p, s, seqs, B, n, w, 1, nullptr, err_flag, st, &h, ranks_out);
  if (rc) return rc;
  // the target logits and the strict count in one launch (score_count_kernel<D, true>)
  return gr_score_rank_launch(h, B, p->d, p->item_emb, p->item_rows, targets, mask_col0, ranks_out, count_ws,
                              count_ws_bytes, err_flag, s.pipe == GR_SAS_FUSED, st);
}
