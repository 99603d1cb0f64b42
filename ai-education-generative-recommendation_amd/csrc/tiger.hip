// TIGER generative retrieval (include/gr_amd.h: gr_tiger_generate_f32, gr_beam_hits_i64).
//
// Two launches, one workgroup per user in each:
//   tiger_encoder_kernel  T5 encoder over the user's S tokens with the [S, d_model] activations in
//                         LDS and the weights streamed from L2 (the whole model is under 1 MB); the
//                         relative bias is expanded once into an [H, 2S-1] LDS table; the kernel ends
//                         by projecting every decoder layer's cross-attention K and V, once per user.
//   tiger_search_kernel   all max_length - 1 decode steps of the beam search in one loop: the decoder
//                         blocks on the running beams' newest token, lm_head, fp32 log-softmax, the
//                         selection of the 2 * num_beams continuations and the running / finished
//                         bookkeeping of transformers' _beam_search, all in LDS.  Self-attention K/V
//                         of (layer, position, beam) stay where they were written: a beam carries
//                         the slot of each of its ancestors, so the library's cache reorder between
//                         steps is a copy of <= 8 small integers per beam.
// Every product is an fp32 fma chain over k in order; nothing is approximated.
//
// The prefix variant (gr_tiger_generate_prefix_f32) puts one launch ahead of the two:
//   tiger_adapter_kernel  grid (users, 3): the ProfessionalAdapter of one level for one user -- bert_proj of
//                         the n_vec vectors, then AD_ROWS history rows at a time the q projection, the
//                         attention over the n_vec keys, out_proj, LayerNorm, the GELU feed-forward and the
//                         second LayerNorm, and a compensated running sum of the rows in row order for
//                         the mean.  It writes the prefix token and (level 0) the [S + 3] key mask.
// tiger_encoder_kernel<true> is the encoder with rows 0..2 taken from those tokens (<false>: the plain
// entry's, whose code is what it was); the search kernel is launched unchanged on S + 3 keys.
//
// The teacher-forced forward (gr_tiger_forward_f32, gr_tiger_forward_prefix_f32) launches the same encoder
// (and adapter) kernels and then tiger_teacher_kernel and tiger_loss_kernel, further down in this file.
#include <atomic>

#include "gr_common.h"

namespace gr {
namespace {

// One workgroup per user owns a compute unit's LDS, so its waves are all the latency hiding there is:
// the search kernel runs 16 of them; the encoder 8, which is what its per-wave probability rows leave
// room for next to S = 128 rows of activations.
constexpr int TG_ENC_THREADS = 512, TG_SRCH_THREADS = 1024;
#define TG_THREADS ((int)blockDim.x)
#define TG_WAVES ((int)blockDim.x >> 6)
constexpr int TG_MAX_S = 128, TG_MAX_BEAMS = 32, TG_MAX_V = 128, TG_MAX_T = 8;
constexpr float TG_NEG = -1.0e9f;
constexpr int64_t TG_MAX_USERS = 1 << 21;   // one workgroup of 1024 threads each, under HIP's 2^32 threads per launch
// Makes a uniform value opaque to the optimiser at this point: what is derived from it is recomputed
// after it (a few scalar operations) instead of being hoisted out of the surrounding loop and held in
// scalar registers across it.
#define TG_OPAQUE(x) asm volatile("" : "+s"(x))
constexpr int TG_SRCH_STATE = 2048;   // floats of LDS the search kernel's small state takes

enum { E_LN0, E_Q, E_K, E_V, E_O, E_LN1, E_WI, E_WO };
enum { D_LN0, D_Q, D_K, D_V, D_O, D_LN1, D_CQ, D_CK, D_CV, D_CO, D_LN2, D_WI, D_WO };

// out[r * ldo + n] (op)= sum_k in[r * ldi + k] * W[n * K + k] for r < rows, n < N.  K % 4 == 0, W 16-byte
// aligned.  MODE 0: store, 1: add into out (the residual), 2: store relu.  One item = one column and
// four rows: the lanes of a wave share the rows (LDS broadcast) and differ in the weight row.
template <int MODE>
__device__ __forceinline__ void tg_gemm(float* out, int ldo, const float* in, int ldi,
                                        const float* __restrict__ W, int N, int K, int rows) {
  constexpr int RB = 4;
  const int nrb = (rows + RB - 1) / RB;
  for (int it = threadIdx.x; it < N * nrb; it += TG_THREADS) {
    const int n = it % N, r0 = (it / N) * RB;
    float acc[RB] = {0.f, 0.f, 0.f, 0.f};
    const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)n * K);
    const float* xr[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) xr[i] = in + (size_t)min(r0 + i, rows - 1) * ldi;
    for (int k = 0; k < K; k += 4) {
      const float4 w = w4[k >> 2];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        float a = acc[i];
        a = fmaf(xr[i][k], w.x, a);
        a = fmaf(xr[i][k + 1], w.y, a);
        a = fmaf(xr[i][k + 2], w.z, a);
        a = fmaf(xr[i][k + 3], w.w, a);
        acc[i] = a;
      }
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      if (r0 + i < rows) {
        float* o = out + (size_t)(r0 + i) * ldo + n;
        if (MODE == 0) *o = acc[i];
        else if (MODE == 1) *o += acc[i];
        else *o = fmaxf(acc[i], 0.f);
      }
    }
  }
}

// T5LayerNorm of rows [rows, D] (D <= 64): out = w * (x * rsqrt(mean(x^2) + eps)) * scale; a wave per row.
__device__ __forceinline__ void tg_rmsnorm(float* out, const float* x, const float* __restrict__ w, int rows,
                                           int D, float eps, float scale) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < rows; r += TG_WAVES) {
    const float v = lane < D ? x[r * D + lane] : 0.f;
    const float ms = wave_sum(v * v) / (float)D;
    if (lane < D) out[r * D + lane] = w[lane] * (v * rsqrtf(ms + eps)) * scale;
  }
}

__device__ __forceinline__ int tg_token(int64_t id, int vocab) {
  return (int)(id < 0 ? 0 : (id >= vocab ? vocab - 1 : id));
}

// Sum over the 64 / dkv lane groups that share a channel (lane % dkv): offsets dkv .. 32.
__device__ __forceinline__ float tg_group_sum(float v, int dkv) {
  for (int o = dkv; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

#define TG_ENC_PTRS \
  const int inner = H * dkv, dkp = dkv + 1; \
  const EncLayout L = enc_layout(S, D, inner, dkv, H, dff, TG_ENC_THREADS / 64); \
  float* x = lds + L.x; \
  float* xn = lds + L.xn; \
  float* ao = lds + L.ao; \
  float* hq = lds + L.hb; \
  float* hk = hq + S * dkp; \
  float* hv = hk + S * dkp; \
  float* bias = lds + L.bias; \
  float* prow = lds + L.prow; \
  int* kmask = reinterpret_cast<int*>(lds + L.mask); \
  (void)x; (void)xn; (void)ao; (void)hq; (void)hk; (void)hv; (void)bias; (void)prow; (void)kmask; (void)dkp;

struct EncLayout {
  int x, xn, ao, hb, bias, prow, mask, total;   // float offsets
  int hb_floats;
};

__host__ __device__ inline EncLayout enc_layout(int S, int D, int inner, int dkv, int H, int dff, int waves) {
  EncLayout L;
  const int dkp = dkv + 1;
  L.x = 0;
  L.xn = L.x + S * D;
  L.ao = L.xn + S * D;
  // ao | q k v of one head; the same floats hold the feed-forward's hidden rows, a tile of rows at a time
  int region = S * inner + 3 * S * dkp;
  if (region < dff) region = dff;
  L.hb = L.ao + S * inner;
  L.hb_floats = region;
  L.bias = L.ao + region;
  L.prow = L.bias + H * (2 * S - 1);
  L.mask = L.prow + waves * S;
  L.total = L.mask + S;
  return L;
}

// PFX: rows 0..2 of x are the user's prefix tokens (prefix[B, 3, D]) and rows 3.. the embeddings of its
// S - 3 history tokens; amask then is the [B, S] mask the adapter kernel wrote (its first three columns 1).
template <bool PFX>
__global__ __launch_bounds__(TG_ENC_THREADS) void tiger_encoder_kernel(gr_tiger_params p, const int64_t* __restrict__ ids,
                                                                   const int64_t* __restrict__ amask, int S,
                                                                   float* __restrict__ cross, float* __restrict__ enc_out,
                                                                   const float* __restrict__ prefix) {
  extern __shared__ __align__(16) float lds[];
  int D = p.d_model, dkv = p.d_kv, H = p.n_heads, dff = p.d_ff;

  // The layers' weight pointers go through LDS: read where they are used, they do not stay in
  // scalar registers across the kernel (the argument struct holds 80 of them).
  __shared__ const float* wtab[GR_TIGER_MAX_LAYERS * 13];
  const int64_t u = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  __shared__ int cint[2];
  __shared__ float ceps;
  for (int e = tid; e < p.n_enc * 8; e += TG_THREADS) wtab[e] = p.enc[e / 8][e % 8];
  for (int e = tid; e < p.n_dec * 2; e += TG_THREADS)
    wtab[GR_TIGER_MAX_LAYERS * 8 + e] = p.dec[e / 2][e % 2 ? D_CV : D_CK];
  if (tid == 0) {
    wtab[GR_TIGER_MAX_LAYERS * 8 + 8] = p.enc_final_ln;
    cint[0] = p.n_enc;
    cint[1] = p.n_dec;
    ceps = p.eps;
  }
  {
  TG_ENC_PTRS
  for (int e = tid; e < S * D; e += TG_THREADS) {
    if (PFX) {
      if (e < 3 * D) {
        x[e] = prefix[u * 3 * D + e];
      } else {
        const int tok = tg_token(ids[u * (S - 3) + e / D - 3], p.vocab);
        x[e] = p.shared[(size_t)tok * D + e % D];
      }
    } else {
      const int tok = tg_token(ids[u * S + e / D], p.vocab);
      x[e] = p.shared[(size_t)tok * D + e % D];
    }
  }
  for (int j = tid; j < S; j += TG_THREADS) kmask[j] = amask ? (amask[u * S + j] != 0) : 1;
  for (int e = tid; e < H * (2 * S - 1); e += TG_THREADS) {
    const int h = e / (2 * S - 1), r = e % (2 * S - 1) - (S - 1);   // r = key - query
    bias[e] = p.enc_rel[p.enc_bucket[r + 127] * H + h];
  }
  }
  __syncthreads();

  for (int l = 0; l < cint[0]; ++l) {
    TG_OPAQUE(D); TG_OPAQUE(dkv); TG_OPAQUE(H); TG_OPAQUE(dff); TG_OPAQUE(S);
    TG_ENC_PTRS
    const float eps = ceps;
    const float* const* W = wtab + l * 8;
    tg_rmsnorm(xn, x, W[E_LN0], S, D, eps, 1.f);
    __syncthreads();
    for (int h = 0; h < H; ++h) {
      tg_gemm<0>(hq, dkp, xn, D, W[E_Q] + (size_t)h * dkv * D, dkv, D, S);
      tg_gemm<0>(hk, dkp, xn, D, W[E_K] + (size_t)h * dkv * D, dkv, D, S);
      tg_gemm<0>(hv, dkp, xn, D, W[E_V] + (size_t)h * dkv * D, dkv, D, S);
      __syncthreads();
      const float* bh = bias + h * (2 * S - 1) + (S - 1);
      for (int i0 = 0; i0 < S; i0 += TG_WAVES) {
        const int i = i0 + wave;
        float* pr = prow + wave * S;
        if (i < S) {
          float s[2], mx = -INFINITY;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            s[t] = -INFINITY;
            if (j < S && kmask[j]) {
              float a = 0.f;
              for (int c = 0; c < dkv; ++c) a = fmaf(hq[i * dkp + c], hk[j * dkp + c], a);
              s[t] = a + bh[j - i];
            }
            mx = fmaxf(mx, s[t]);
          }
          mx = wave_max(mx);
          float sum = 0.f;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            s[t] = (s[t] == -INFINITY) ? 0.f : expf(s[t] - mx);
            sum += s[t];
          }
          sum = wave_sum(sum);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            if (j < S) pr[j] = s[t] / sum;
          }
        }
        __syncthreads();
        if (i < S) {
          const int c = lane % dkv, g = lane / dkv, G = 64 / dkv;
          float a = 0.f;
          for (int j = g; j < S; j += G) a = fmaf(pr[j], hv[j * dkp + c], a);
          a = tg_group_sum(a, dkv);
          if (lane < dkv) ao[i * inner + h * dkv + c] = a;
        }
        __syncthreads();
      }
    }
    tg_gemm<1>(x, D, ao, inner, W[E_O], D, inner, S);
    __syncthreads();
    tg_rmsnorm(xn, x, W[E_LN1], S, D, eps, 1.f);
    __syncthreads();
    // feed-forward over tiles of rows: the hidden rows take the attention buffers' place
    const int R = min(S, L.hb_floats / dff);
    for (int r0 = 0; r0 < S; r0 += R) {
      const int rows = min(R, S - r0);
      tg_gemm<2>(ao, dff, xn + r0 * D, D, W[E_WI], dff, D, rows);
      __syncthreads();
      tg_gemm<1>(x + r0 * D, D, ao, dff, W[E_WO], D, dff, rows);
      __syncthreads();
    }
  }
  TG_OPAQUE(D); TG_OPAQUE(dkv); TG_OPAQUE(H); TG_OPAQUE(dff); TG_OPAQUE(S);
  TG_ENC_PTRS
  const int n_dec = cint[1];
  tg_rmsnorm(xn, x, wtab[GR_TIGER_MAX_LAYERS * 8 + 8], S, D, ceps, 1.f);
  __syncthreads();
  if (enc_out)
    for (int e = tid; e < S * D; e += TG_THREADS) enc_out[u * S * D + e] = xn[e];
  // cross-attention K and V of every decoder layer: [n_dec][2][S][inner] per user
  float* cu = cross + (size_t)u * n_dec * 2 * S * inner;
  for (int l = 0; l < n_dec; ++l) {
    tg_gemm<0>(cu + (size_t)(2 * l) * S * inner, inner, xn, D, wtab[GR_TIGER_MAX_LAYERS * 8 + 2 * l], inner, D, S);
    tg_gemm<0>(cu + (size_t)(2 * l + 1) * S * inner, inner, xn, D, wtab[GR_TIGER_MAX_LAYERS * 8 + 2 * l + 1], inner, D,
               S);
  }
}

// The search kernel's LDS layout is fixed at the envelope's largest shapes (32 beams, d_model and
// heads * d_kv 64, d_ff 256, 128 keys, 16 waves), so every sub-array's address is an immediate:
// 88 KB per workgroup, one workgroup per compute unit.
constexpr int SR_H = TG_SRCH_STATE, SR_XN = SR_H + 2048, SR_Q = SR_XN + 2048, SR_AO = SR_Q + 2048,
              SR_FF = SR_AO + 2048, SR_PROW = SR_FF + 8192, SR_SATTN = SR_PROW + (TG_SRCH_THREADS / 64) * TG_MAX_S,
              SR_DBIAS = SR_SATTN + TG_MAX_BEAMS * 8 * TG_MAX_T, SR_TOTAL = SR_DBIAS + 8 * TG_MAX_T;

__global__ __launch_bounds__(TG_SRCH_THREADS) void tiger_search_kernel(gr_tiger_params p, const int64_t* __restrict__ amask,
                                                                  int S, int nb, int T, const float* __restrict__ cross,
                                                                  float* __restrict__ selfkv, int64_t* __restrict__ seq_out,
                                                                  float* __restrict__ score_out,
                                                                  float* __restrict__ step_logits) {
  extern __shared__ __align__(16) float lds[];
  int D = p.d_model, dkv = p.d_kv, H = p.n_heads, dff = p.d_ff, V = p.vocab;
  float* h = lds + SR_H;
  float* xn = lds + SR_XN;
  float* q = lds + SR_Q;
  float* ao = lds + SR_AO;
  float* ff = lds + SR_FF;         // feed-forward hidden rows, then the logits / candidate scores
  float* prow = lds + SR_PROW;
  float* sattn = lds + SR_SATTN;   // self-attention scores of (beam, head)
  float* dbias = lds + SR_DBIAS;   // decoder relative bias of (distance, head)
  // the small search state sits at fixed offsets (sized for 32 beams, 8 positions, 128 keys), so that its
  // addresses are immediates, not scalar registers
  float* run_score = lds;
  float* new_run_score = lds + TG_MAX_BEAMS;
  float* fin_score = lds + 2 * TG_MAX_BEAMS;
  float* new_fin_score = lds + 3 * TG_MAX_BEAMS;
  float* top_val = lds + 4 * TG_MAX_BEAMS;
  int* ist = reinterpret_cast<int*>(lds + 6 * TG_MAX_BEAMS);
  int* top_idx = ist;
  int* run_par = ist + 2 * TG_MAX_BEAMS;
  int* run_tok = ist + 3 * TG_MAX_BEAMS;
  int* fin_src = ist + 4 * TG_MAX_BEAMS;
  int* flags = ist + 5 * TG_MAX_BEAMS;          // [0] live beams, [1] finished count, [2] stop
  int* kmask = flags + 4;
  int* run_seq = kmask + TG_MAX_S;
  int* anc = run_seq + TG_MAX_BEAMS * TG_MAX_T;
  int* fin_seq = anc + TG_MAX_BEAMS * TG_MAX_T;
  int* tmp_run_seq = fin_seq + TG_MAX_BEAMS * TG_MAX_T;
  int* tmp_anc = tmp_run_seq + TG_MAX_BEAMS * TG_MAX_T;
  int* tmp_fin_seq = tmp_anc + TG_MAX_BEAMS * TG_MAX_T;
  static_assert(11 * TG_MAX_BEAMS + 4 + TG_MAX_S + 6 * TG_MAX_BEAMS * TG_MAX_T <= TG_SRCH_STATE, "search state");

  __shared__ const float* wtab[GR_TIGER_MAX_LAYERS * 13 + 3];   // as in the encoder kernel
  const float* const* gshared = wtab + GR_TIGER_MAX_LAYERS * 13;   // shared, lm_head, decoder final norm
  // pointers and constants that are read where they are used instead of living in scalar registers:
  // step logits, sequences, scores, cross K/V, self K/V; eos, fill, layers; eps, lm scale
  __shared__ void* gout[5];
  __shared__ int cint[3];
  __shared__ float cflt[2];
  const int64_t u = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int e = tid; e < p.n_dec * 13; e += TG_THREADS) wtab[e] = p.dec[e / 13][e % 13];
  if (tid == 0) {
    gout[0] = step_logits;
    gout[1] = seq_out;
    gout[2] = score_out;
    gout[3] = const_cast<float*>(cross);
    gout[4] = selfkv;
    cint[0] = p.eos_id;
    cint[1] = p.fill_id;
    cint[2] = p.n_dec;
    cflt[0] = p.eps;
    cflt[1] = p.lm_scale;
    wtab[GR_TIGER_MAX_LAYERS * 13] = p.shared;
    wtab[GR_TIGER_MAX_LAYERS * 13 + 1] = p.lm_head;
    wtab[GR_TIGER_MAX_LAYERS * 13 + 2] = p.dec_final_ln;
  }
  for (int e = tid; e < H * TG_MAX_T; e += TG_THREADS) dbias[e] = p.dec_rel[p.dec_bucket[e / H] * H + e % H];


  for (int j = tid; j < S; j += TG_THREADS) kmask[j] = amask ? (amask[u * S + j] != 0) : 1;
  for (int e = tid; e < nb * T; e += TG_THREADS) {
    run_seq[e] = (e % T == 0) ? p.pad_id : p.fill_id;
    fin_seq[e] = run_seq[e];
    anc[e] = 0;
  }
  for (int b = tid; b < nb; b += TG_THREADS) {
    run_score[b] = b == 0 ? 0.f : TG_NEG;
    fin_score[b] = TG_NEG;
  }
  if (tid == 0) {
    flags[0] = 1;   // at step 0 only beam 0 is live: the others carry -1e9 and V >= 2 nb candidates beat them
    flags[1] = 0;
    flags[2] = 0;
  }
  if (step_logits)
    for (int e = tid; e < (T - 1) * nb * V; e += TG_THREADS) step_logits[(size_t)u * (T - 1) * nb * V + e] = 0.f;
  __syncthreads();

  for (int t = 0; t + 1 < T; ++t) {
    TG_OPAQUE(D); TG_OPAQUE(dkv); TG_OPAQUE(H); TG_OPAQUE(dff); TG_OPAQUE(V);
    TG_OPAQUE(S); TG_OPAQUE(nb); TG_OPAQUE(T);
    const int live = flags[0];
    for (int e = tid; e < live * D; e += TG_THREADS) {
      const int tok = tg_token(run_seq[(e / D) * T + t], V);
      h[e] = gshared[0][(size_t)tok * D + e % D];
    }
    __syncthreads();
    for (int l = 0; l < cint[2]; ++l) {
      TG_OPAQUE(D); TG_OPAQUE(dkv); TG_OPAQUE(H); TG_OPAQUE(dff); TG_OPAQUE(S); TG_OPAQUE(nb);
      const int inner = H * dkv;
      const float* const* W = wtab + l * 13;
      const int n_dec = cint[2];
      const float eps = cflt[0];
      const float* cu = static_cast<const float*>(gout[3]) + (size_t)u * n_dec * 2 * S * inner;
      // self K/V: [n_dec][2][T-1][nb][inner] per user
      float* su = static_cast<float*>(gout[4]) + (size_t)u * n_dec * 2 * (T - 1) * nb * inner;
      const size_t kv_stride = (size_t)(T - 1) * nb * inner;
      float* sk = su + (size_t)(2 * l) * kv_stride;
      float* sv = su + (size_t)(2 * l + 1) * kv_stride;
      // self-attention over the beam's own prefix
      tg_rmsnorm(xn, h, W[D_LN0], live, D, eps, 1.f);
      __syncthreads();
      tg_gemm<0>(q, inner, xn, D, W[D_Q], inner, D, live);
      tg_gemm<0>(sk + (size_t)t * nb * inner, inner, xn, D, W[D_K], inner, D, live);
      tg_gemm<0>(sv + (size_t)t * nb * inner, inner, xn, D, W[D_V], inner, D, live);
      __syncthreads();
      for (int it = tid; it < live * H; it += TG_THREADS) {
        const int b = it / H, hd = it % H;
        const float* qv = q + b * inner + hd * dkv;
        float* s = sattn + it * TG_MAX_T;      // this thread's scores, then probabilities
        float mx = -INFINITY;
#pragma unroll 1
        for (int pos = 0; pos <= t; ++pos) {
          const int slot = pos == t ? b : anc[b * T + pos];
          const float* kr = sk + ((size_t)pos * nb + slot) * inner + hd * dkv;
          float a = 0.f;
          for (int c = 0; c < dkv; ++c) a = fmaf(qv[c], kr[c], a);
          a += dbias[(t - pos) * H + hd];
          s[pos] = a;
          mx = fmaxf(mx, a);
        }
        float sum = 0.f;
#pragma unroll 1
        for (int pos = 0; pos <= t; ++pos) {
          const float e = expf(s[pos] - mx);
          s[pos] = e;
          sum += e;
        }
#pragma unroll 1
        for (int pos = 0; pos <= t; ++pos) s[pos] = s[pos] / sum;
        for (int c = 0; c < dkv; ++c) {
          float a = 0.f;
#pragma unroll 1
          for (int pos = 0; pos <= t; ++pos) {
            const int slot = pos == t ? b : anc[b * T + pos];
            a = fmaf(s[pos], sv[((size_t)pos * nb + slot) * inner + hd * dkv + c], a);
          }
          ao[b * inner + hd * dkv + c] = a;
        }
      }
      __syncthreads();
      tg_gemm<1>(h, D, ao, inner, W[D_O], D, inner, live);
      __syncthreads();
      // cross-attention over the user's encoder keys (no position bias, padding masked)
      tg_rmsnorm(xn, h, W[D_LN1], live, D, eps, 1.f);
      __syncthreads();
      tg_gemm<0>(q, inner, xn, D, W[D_CQ], inner, D, live);
      __syncthreads();
      const float* ck = cu + (size_t)(2 * l) * S * inner;
      const float* cv = cu + (size_t)(2 * l + 1) * S * inner;
      for (int it0 = 0; it0 < live * H; it0 += TG_WAVES) {
        const int it = it0 + wave;
        const int b = it / H, hd = it % H;
        float* pr = prow + wave * S;
        if (it < live * H) {
          const float* qv = q + b * inner + hd * dkv;
          float s[2], mx = -INFINITY;
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2) {
            const int j = lane + 64 * k2;
            s[k2] = -INFINITY;
            if (j < S && kmask[j]) {
              const float4* kr = reinterpret_cast<const float4*>(ck + (size_t)j * inner + hd * dkv);
              float a = 0.f;
              for (int c = 0; c < dkv; c += 4) {
                const float4 kk = kr[c >> 2];
                a = fmaf(qv[c], kk.x, a);
                a = fmaf(qv[c + 1], kk.y, a);
                a = fmaf(qv[c + 2], kk.z, a);
                a = fmaf(qv[c + 3], kk.w, a);
              }
              s[k2] = a;
            }
            mx = fmaxf(mx, s[k2]);
          }
          mx = wave_max(mx);
          float sum = 0.f;
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2) {
            s[k2] = (s[k2] == -INFINITY) ? 0.f : expf(s[k2] - mx);
            sum += s[k2];
          }
          sum = wave_sum(sum);
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2) {
            const int j = lane + 64 * k2;
            if (j < S) pr[j] = s[k2] / sum;
          }
        }
        __syncthreads();
        if (it < live * H) {
          const int c = lane % dkv, g = lane / dkv, G = 64 / dkv;
          float a = 0.f;
          for (int j = g; j < S; j += G) a = fmaf(pr[j], cv[(size_t)j * inner + hd * dkv + c], a);
          a = tg_group_sum(a, dkv);
          if (lane < dkv) ao[b * inner + hd * dkv + c] = a;
        }
        __syncthreads();
      }
      tg_gemm<1>(h, D, ao, inner, W[D_CO], D, inner, live);
      __syncthreads();
      // feed-forward
      tg_rmsnorm(xn, h, W[D_LN2], live, D, eps, 1.f);
      __syncthreads();
      tg_gemm<2>(ff, dff, xn, D, W[D_WI], dff, D, live);
      __syncthreads();
      tg_gemm<1>(h, D, ff, dff, W[D_WO], D, dff, live);
      __syncthreads();
    }
    TG_OPAQUE(D); TG_OPAQUE(V); TG_OPAQUE(nb); TG_OPAQUE(T);
    const int keep = 2 * nb;
    // lm_head on the scaled final norm, log-softmax, plus the beam's running score
    tg_rmsnorm(xn, h, gshared[2], live, D, cflt[0], cflt[1]);
    __syncthreads();
    tg_gemm<0>(ff, V, xn, D, gshared[1], V, D, live);
    __syncthreads();
    if (float* sl0 = static_cast<float*>(gout[0])) {
      float* sl = sl0 + ((size_t)u * (T - 1) + t) * nb * V;
      for (int e = tid; e < live * V; e += TG_THREADS) sl[e] = ff[e];
      __syncthreads();   // the log-softmax below rewrites ff in place, a row per wave
    }
    for (int b = wave; b < live; b += TG_WAVES) {
      float v[2], mx = -INFINITY;
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const int j = lane + 64 * k2;
        v[k2] = j < V ? ff[b * V + j] : -INFINITY;
        mx = fmaxf(mx, v[k2]);
      }
      mx = wave_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) sum += (lane + 64 * k2 < V) ? expf(v[k2] - mx) : 0.f;
      const float lse = logf(wave_sum(sum));
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const int j = lane + 64 * k2;
        if (j < V) ff[b * V + j] = ((v[k2] - mx) - lse) + run_score[b];
      }
    }
    for (int e = tid; e < keep; e += TG_THREADS) {
      top_val[e] = TG_NEG;
      top_idx[e] = 0;
    }
    __syncthreads();
    // the 2 nb best of the live * V candidates, best first, equal scores by the lower flat index: a
    // candidate's rank is the number of candidates ahead of it
    TG_OPAQUE(V); TG_OPAQUE(nb); TG_OPAQUE(T);
    const int N = live * V;
    for (int i = tid; i < N; i += TG_THREADS) {
      const float v = ff[i];
      int cnt = 0;
      for (int j = 0; j < N && cnt < keep; ++j) {
        const float o = ff[j];
        cnt += (o > v) || (o == v && j < i);
      }
      if (cnt < keep) {
        top_val[cnt] = v;
        top_idx[cnt] = i;
      }
    }
    __syncthreads();
    if (tid == 0) {
      const bool last = t + 2 >= T;          // the continuation reaches max_length
      int nr = 0;
      for (int i = 0; i < keep; ++i) {
        const int tok = top_idx[i] % V, par = top_idx[i] / V;
        if (!(last || tok == cint[0]) && nr < nb) {
          run_par[nr] = par;
          run_tok[nr] = tok;
          new_run_score[nr] = top_val[i];
          ++nr;
        }
      }
      // finished: the old list and the hits among the first nb continuations, both best first; the
      // length-normalised score divides by the tokens generated so far
      const int fc = flags[1];
      const float len = (float)(t + 1);
      int a = 0, i = 0, n = 0;
      while (n < nb) {
        while (i < nb && !(last || top_idx[i] % V == cint[0])) ++i;
        const bool has_old = a < fc, has_new = i < nb;
        if (!has_old && !has_new) break;
        const float sn = has_new ? top_val[i] / len : 0.f;
        if (has_old && (!has_new || fin_score[a] >= sn)) {
          fin_src[n] = a;
          new_fin_score[n] = fin_score[a];
          ++a;
        } else {
          fin_src[n] = nb + i;
          new_fin_score[n] = sn;
          ++i;
        }
        ++n;
      }
      flags[1] = n;
      flags[0] = nr;
      // early stop (early_stopping False, length_penalty 1): every slot finished and the best running
      // beam, normalised at its current length, no better than the worst finished one
      int stop = last || nr == 0;
      if (!stop && n == nb && !(new_run_score[0] / len > new_fin_score[nb - 1])) stop = 1;
      flags[2] = stop;
    }
    __syncthreads();
    TG_OPAQUE(V); TG_OPAQUE(nb); TG_OPAQUE(T);
    const int nr = flags[0], nf = flags[1];
    for (int e = tid; e < nb * T; e += TG_THREADS) {
      const int b = e / T, pos = e % T;
      if (b < nr) {
        const int par = run_par[b];
        tmp_run_seq[e] = pos <= t ? run_seq[par * T + pos] : (pos == t + 1 ? run_tok[b] : cint[1]);
        tmp_anc[e] = pos < t ? anc[par * T + pos] : (pos == t ? par : 0);
      }
      if (b < nf) {
        const int src = fin_src[b];
        if (src < nb) {
          tmp_fin_seq[e] = fin_seq[src * T + pos];
        } else {
          const int ci = top_idx[src - nb], par = ci / V;
          tmp_fin_seq[e] = pos <= t ? run_seq[par * T + pos] : (pos == t + 1 ? ci % V : cint[1]);
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < nb * T; e += TG_THREADS) {
      const int b = e / T;
      if (b < nr) {
        run_seq[e] = tmp_run_seq[e];
        anc[e] = tmp_anc[e];
      }
      if (b < nf) fin_seq[e] = tmp_fin_seq[e];
    }
    for (int b = tid; b < nb; b += TG_THREADS) {
      if (b < nr) run_score[b] = new_run_score[b];
      if (b < nf) fin_score[b] = new_fin_score[b];
    }
    __syncthreads();
    if (flags[2]) break;
  }
  int64_t* so = static_cast<int64_t*>(gout[1]);
  float* co = static_cast<float*>(gout[2]);
  for (int e = tid; e < nb * T; e += TG_THREADS) so[(size_t)u * nb * T + e] = fin_seq[e];
  for (int b = tid; b < nb; b += TG_THREADS) co[(size_t)u * nb + b] = fin_score[b];
}

// ProfessionalAdapter (RQVAE-T5-prefix/model.py:8-48) in eval mode: one workgroup per (user, level).
// Every row of the history is independent until the final mean, so the S rows go through the block
// AD_ROWS at a time and the workgroup's LDS is 36 KB whatever S is (four workgroups per compute unit).
constexpr int AD_THREADS = 256, AD_ROWS = 16, AD_MAX_D = 64, AD_MAX_VEC = 16, AD_MAX_BERT = 1024;
enum { A_BERT_W, A_BERT_B, A_IN_W, A_IN_B, A_OUT_W, A_OUT_B, A_FF1_W, A_FF1_B, A_FF2_W, A_FF2_B, A_N1_W, A_N1_B,
       A_N2_W, A_N2_B };

// out[r * ldo + n] = act(bias[n] + sum_k in[r * ldi + k] * W[n * K + k]); tg_gemm's items.  GELU: exact erf.
template <bool GELU>
__device__ __forceinline__ void ad_linear(float* out, int ldo, const float* in, int ldi, const float* __restrict__ W,
                                          const float* __restrict__ bias, int N, int K, int rows) {
  constexpr int RB = 4;
  const int nrb = (rows + RB - 1) / RB;
  for (int it = threadIdx.x; it < N * nrb; it += TG_THREADS) {
    const int n = it % N, r0 = (it / N) * RB;
    float acc[RB] = {0.f, 0.f, 0.f, 0.f};
    const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)n * K);
    const float* xr[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) xr[i] = in + (size_t)min(r0 + i, rows - 1) * ldi;
    for (int k = 0; k < K; k += 4) {
      const float4 w = w4[k >> 2];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        float a = acc[i];
        a = fmaf(xr[i][k], w.x, a);
        a = fmaf(xr[i][k + 1], w.y, a);
        a = fmaf(xr[i][k + 2], w.z, a);
        a = fmaf(xr[i][k + 3], w.w, a);
        acc[i] = a;
      }
    }
    const float b = bias[n];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      if (r0 + i < rows) {
        float v = acc[i] + b;
        if (GELU) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
        out[(size_t)(r0 + i) * ldo + n] = v;
      }
    }
  }
}

// nn.LayerNorm of a + b over rows [rows, D] (D <= 64): biased variance; a wave per row.  out may be a.
__device__ __forceinline__ void ad_layernorm(float* out, const float* a, const float* b, const float* __restrict__ w,
                                             const float* __restrict__ bias, int rows, int D, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < rows; r += TG_WAVES) {
    const float v = lane < D ? a[r * D + lane] + b[r * D + lane] : 0.f;
    const float mean = wave_sum(v) / (float)D;
    const float c = lane < D ? v - mean : 0.f;
    const float var = wave_sum(c * c) / (float)D;
    if (lane < D) out[r * D + lane] = c * rsqrtf(var + eps) * w[lane] + bias[lane];
  }
}

__global__ __launch_bounds__(AD_THREADS) void tiger_adapter_kernel(
    gr_tiger_prefix_params pp, const float* __restrict__ shared, int vocab, int D, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ amask, const float* __restrict__ prof1, const float* __restrict__ prof2,
    const float* __restrict__ prof3, int S, int64_t* __restrict__ ext_mask, float* __restrict__ prefix_ws,
    float* __restrict__ prefix_out) {
  __shared__ __align__(16) float et[AD_ROWS * AD_MAX_D];        // embeddings, then the block's rows
  __shared__ __align__(16) float qt[AD_ROWS * AD_MAX_D];        // queries, then each sub-layer's output
  __shared__ __align__(16) float hid[AD_ROWS * 4 * AD_MAX_D];   // attention context, then the hidden rows
  __shared__ __align__(16) float kv[AD_MAX_VEC * AD_MAX_D];     // bert_proj(prof)
  __shared__ __align__(16) float kvp[AD_MAX_VEC * 2 * AD_MAX_D];   // its key | value projections
  __shared__ const float* wtab[14];
  const int64_t u = blockIdx.x;
  const int level = blockIdx.y, tid = threadIdx.x;
  const int nv = pp.n_vec, K = pp.bert_dim, nh = pp.n_heads, hd = D / nh;
  const float eps = pp.eps;
  if (tid < 14) wtab[tid] = pp.adapter[level][tid];
  if (level == 0)
    for (int j = tid; j < S + 3; j += AD_THREADS)
      ext_mask[u * (S + 3) + j] = (j < 3 || !amask) ? 1 : (amask[u * S + j - 3] != 0);
  __syncthreads();
  // kv = bert_proj(prof): one output per item, four interleaved fma chains over k summed pairwise
  const float* prof = (level == 0 ? prof1 : level == 1 ? prof2 : prof3) + (size_t)u * nv * K;
  for (int it = tid; it < nv * D; it += AD_THREADS) {
    const int n = it % D, r = it / D;
    const float4* w4 = reinterpret_cast<const float4*>(wtab[A_BERT_W] + (size_t)n * K);
    const float4* x4 = reinterpret_cast<const float4*>(prof + (size_t)r * K);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < (K >> 2); ++k) {
      const float4 w = w4[k], x = x4[k];
      a0 = fmaf(x.x, w.x, a0);
      a1 = fmaf(x.y, w.y, a1);
      a2 = fmaf(x.z, w.z, a2);
      a3 = fmaf(x.w, w.w, a3);
    }
    kv[r * D + n] = ((a0 + a1) + (a2 + a3)) + wtab[A_BERT_B][n];
  }
  __syncthreads();
  // keys and values: rows D .. 3 D of in_proj
  ad_linear<false>(kvp, 2 * D, kv, D, wtab[A_IN_W] + (size_t)D * D, wtab[A_IN_B] + D, 2 * D, D, nv);
  const float scale = sqrtf(1.f / (float)hd);
  // thread c < D: the running sum of channel c over the rows, in row order, compensated (Kahan): a history
  // of one item is all identical padding rows but four, and their plain running sum rounds the same way every time
  float msum = 0.f, mcomp = 0.f;
  for (int r0 = 0; r0 < S; r0 += AD_ROWS) {
    const int rows = min(AD_ROWS, S - r0);
    __syncthreads();
    for (int e = tid; e < rows * D; e += AD_THREADS) {
      const int tok = tg_token(ids[u * S + r0 + e / D], vocab);
      et[e] = shared[(size_t)tok * D + e % D];
    }
    __syncthreads();
    ad_linear<false>(qt, D, et, D, wtab[A_IN_W], wtab[A_IN_B], D, D, rows);
    __syncthreads();
    // softmax(q k^T * scale) v per (row, head) over the nv keys
    for (int it = tid; it < rows * nh; it += AD_THREADS) {
      const int r = it / nh, h = it % nh;
      const float* q = qt + r * D + h * hd;
      float s[AD_MAX_VEC], mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < AD_MAX_VEC; ++j) {
        s[j] = -INFINITY;
        if (j < nv) {
          const float* kr = kvp + j * 2 * D + h * hd;
          float a = 0.f;
          for (int c = 0; c < hd; ++c) a = fmaf(q[c] * scale, kr[c], a);
          s[j] = a;
        }
        mx = fmaxf(mx, s[j]);
      }
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < AD_MAX_VEC; ++j) {
        s[j] = j < nv ? expf(s[j] - mx) : 0.f;
        sum += s[j];
      }
      for (int c = 0; c < hd; ++c) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < AD_MAX_VEC; ++j)
          if (j < nv) a = fmaf(s[j] / sum, kvp[j * 2 * D + D + h * hd + c], a);
        hid[r * D + h * hd + c] = a;
      }
    }
    __syncthreads();
    ad_linear<false>(qt, D, hid, D, wtab[A_OUT_W], wtab[A_OUT_B], D, D, rows);
    __syncthreads();
    ad_layernorm(et, et, qt, wtab[A_N1_W], wtab[A_N1_B], rows, D, eps);
    __syncthreads();
    ad_linear<true>(hid, 4 * D, et, D, wtab[A_FF1_W], wtab[A_FF1_B], 4 * D, D, rows);
    __syncthreads();
    ad_linear<false>(qt, D, hid, 4 * D, wtab[A_FF2_W], wtab[A_FF2_B], D, 4 * D, rows);
    __syncthreads();
    ad_layernorm(et, et, qt, wtab[A_N2_W], wtab[A_N2_B], rows, D, eps);
    __syncthreads();
    if (tid < D)
      for (int r = 0; r < rows; ++r) {
        const float y = et[r * D + tid] - mcomp, t = msum + y;
        mcomp = (t - msum) - y;
        msum = t;
      }
  }
  if (tid < D) {
    const float v = msum / (float)S;
    prefix_ws[(u * 3 + level) * D + tid] = v;
    if (prefix_out) prefix_out[(u * 3 + level) * D + tid] = v;
  }
}

__global__ void beam_hits_kernel(const int64_t* __restrict__ preds, int64_t B, int k, int pred_len, int64_t ld,
                                 const int64_t* __restrict__ labels, int label_len, uint8_t* __restrict__ hits) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int found = -1;
  for (int j = 0; j < k && found < 0; ++j) {
    const int64_t* pr = preds + (b * k + j) * ld;
    bool eq = true;
    for (int c = 0; c < label_len && eq; ++c) eq = (c < pred_len ? pr[c] : 0) == labels[b * label_len + c];
    if (eq) found = j;
  }
  for (int j = 0; j < k; ++j) hits[b * k + j] = j == found;
}

const char* tiger_check(const gr_tiger_params* p, int64_t B, int S, int nb, int T) {
  if (!p) return "null params";
  if (p->d_model != 32 && p->d_model != 64) return "d_model must be 32 or 64";
  if (p->d_kv != 8 && p->d_kv != 16 && p->d_kv != 32) return "d_kv must be 8, 16 or 32";
  if (p->n_heads < 1 || (p->n_heads * p->d_kv != 32 && p->n_heads * p->d_kv != 64))
    return "num_heads * d_kv must be 32 or 64";
  if (p->d_ff < 32 || p->d_ff > 256 || p->d_ff % 32) return "d_ff must be a multiple of 32, at most 256";
  if (p->n_enc < 1 || p->n_enc > GR_TIGER_MAX_LAYERS) return "num_layers must be 1..4";
  if (p->n_dec < 1 || p->n_dec > GR_TIGER_MAX_LAYERS) return "num_decoder_layers must be 1..4";
  if (p->n_buckets != 32) return "relative_attention_num_buckets must be 32";
  if (nb < 1 || nb > TG_MAX_BEAMS) return "num_beams must be 1..32";
  if (p->vocab > TG_MAX_V) return "vocab_size must be at most 128";
  if (p->vocab < 2 * nb) return "vocab_size must be at least 2 * num_beams";
  if (S < 1 || S > TG_MAX_S) return "the history must hold 1..128 tokens";
  if (T < 2 || T > TG_MAX_T) return "max_length must be 2..8";
  if (B < 0 || B > TG_MAX_USERS) return "the batch must hold at most 2^21 users";
  return nullptr;
}

size_t tiger_cross_floats(const gr_tiger_params* p, int64_t B, int S) {
  return (size_t)B * p->n_dec * 2 * S * p->n_heads * p->d_kv;
}

size_t tiger_self_floats(const gr_tiger_params* p, int64_t B, int nb, int T) {
  return (size_t)B * p->n_dec * 2 * (T - 1) * nb * p->n_heads * p->d_kv;
}

}  // namespace
}  // namespace gr

namespace gr {
namespace {

constexpr int TG_PREFIX = 3;   // prefix tokens ahead of the history

const char* tiger_prefix_check(const gr_tiger_params* p, const gr_tiger_prefix_params* pp, int S) {
  if (!p) return "null params";
  if (!pp) return "null prefix params";
  if (pp->bert_dim < 4 || pp->bert_dim > AD_MAX_BERT || pp->bert_dim % 4)
    return "bert_dim must be a multiple of 4 in [4, 1024]";
  if (pp->n_vec < 1 || pp->n_vec > AD_MAX_VEC) return "n_vec must be 1..16";
  if (pp->n_heads < 1 || p->d_model % pp->n_heads) return "d_model must be a multiple of the adapters' num_heads";
  if (S < 1 || S > TG_MAX_S - TG_PREFIX)
    return "the history must hold 1..125 tokens (128 encoder positions with the three prefix tokens)";
  return nullptr;
}

size_t tiger_plain_bytes(const gr_tiger_params* p, int64_t B, int S, int nb, int T) {
  const size_t f = align_up(tiger_cross_floats(p, B, S), 4) + tiger_self_floats(p, B, nb, T);
  return align_up(f * sizeof(float), 16) + 16;
}

size_t tiger_mask_bytes(int64_t B, int S) { return align_up((size_t)B * (S + TG_PREFIX) * sizeof(int64_t), 16); }

size_t tiger_prefix_bytes(const gr_tiger_params* p, int64_t B) {
  return align_up((size_t)B * TG_PREFIX * p->d_model * sizeof(float), 16);
}

// The checks the generate and the forward entries share, in the order their callers make them.
int tiger_check_ids_and_prefix(const std::string& who, const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                               const float* const* prof, bool prefixed) {
  if (p->eos_id < 0 || p->eos_id >= p->vocab || p->pad_id < 0 || p->pad_id >= p->vocab || p->fill_id < 0 ||
      p->fill_id >= p->vocab)
    return fail(GR_ERR_ARG, who + "pad, eos and fill ids must lie in [0, vocab)");
  if (prefixed) {
    bool ok = true;
    for (int l = 0; l < 3; ++l)
      for (int i = 0; i < 14; ++i) ok = ok && pp->adapter[l][i] && aligned16(pp->adapter[l][i]);
    if (!ok) return fail(GR_ERR_ARG, who + "an adapter weight pointer is null or not 16-byte aligned");
    for (int l = 0; l < 3; ++l)
      if (!prof[l] || !aligned16(prof[l]))
        return fail(GR_ERR_ARG, who + "a prof_lvl pointer is null or not 16-byte aligned");
  }
  return GR_OK;
}

bool tiger_weights_ok(const gr_tiger_params* p) {
  bool ok = p->shared && p->lm_head && p->enc_rel && p->dec_rel && p->enc_final_ln && p->dec_final_ln &&
            p->enc_bucket && p->dec_bucket && aligned16(p->shared) && aligned16(p->lm_head);
  for (int l = 0; ok && l < p->n_enc; ++l)
    for (int i = 0; i < 8; ++i) ok = ok && p->enc[l][i] && aligned16(p->enc[l][i]);
  for (int l = 0; ok && l < p->n_dec; ++l)
    for (int i = 0; i < 13; ++i) ok = ok && p->dec[l][i] && aligned16(p->dec[l][i]);
  return ok;
}

constexpr size_t kTigerLdsMax = 159 * 1024;   // dynamic part; the kernels' static LDS is under 1 KB

size_t tiger_enc_lds(const gr_tiger_params* p, int St) {
  const EncLayout EL = enc_layout(St, p->d_model, p->n_heads * p->d_kv, p->d_kv, p->n_heads, p->d_ff, TG_ENC_THREADS / 64);
  return (size_t)EL.total * sizeof(float);
}

// Raises the dynamic LDS limit of the encoder, search and teacher kernels (defined below, after the last of them):
// the limit is a property of the kernel on the current device, raised on each device's first call.
int tiger_raise_lds(const std::string& who);

// Both entries: pp == nullptr is gr_tiger_generate_f32 (two launches); otherwise the adapter launch comes
// first and the encoder and the search run on S + 3 positions with the mask it wrote.
int tiger_generate(const char* fn, const gr_tiger_params* p, const gr_tiger_prefix_params* pp, const int64_t* input_ids,
                   const int64_t* attention_mask, const float* const* prof, int64_t B, int32_t S, int32_t num_beams,
                   int32_t max_length, int64_t* sequences, float* scores, float* prefix_out, float* enc_out,
                   float* step_logits, void* workspace, size_t workspace_bytes, void* stream, bool prefixed) {
  clear_error();
  const std::string who = std::string(fn) + ": ";
  if (prefixed) {
    if (const char* why = tiger_prefix_check(p, pp, S)) return fail(!p || !pp ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  }
  const int St = prefixed ? S + TG_PREFIX : S;   // encoder positions
  if (const char* why = tiger_check(p, B, St, num_beams, max_length)) {
    const bool arg = !p || B < 0;
    return fail(arg ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  }
  if (int rc = tiger_check_ids_and_prefix(who, p, pp, prof, prefixed)) return rc;
  const size_t plain = tiger_plain_bytes(p, B, St, num_beams, max_length);
  const size_t need = prefixed ? plain + tiger_mask_bytes(B, S) + tiger_prefix_bytes(p, B) : plain;
  if (!workspace || workspace_bytes < need || !aligned16(workspace))
    return fail(GR_ERR_WORKSPACE, who + "workspace missing, misaligned or smaller than " +
                                      (prefixed ? "gr_tiger_prefix_workspace_bytes" : "gr_tiger_workspace_bytes"));
  if (!input_ids || !sequences || !scores) return fail(GR_ERR_ARG, who + "null pointer");
  if (!tiger_weights_ok(p)) return fail(GR_ERR_ARG, who + "a weight pointer is null or not 16-byte aligned");
  if (B == 0) return GR_OK;
  const size_t enc_lds = tiger_enc_lds(p, St), srch_lds = (size_t)SR_TOTAL * sizeof(float);
  if (enc_lds > kTigerLdsMax || srch_lds > kTigerLdsMax)
    return fail(GR_ERR_UNSUPPORTED, who + "the per-user state does not fit in LDS");
  if (int rc = tiger_raise_lds(who)) return rc;
  float* cross = static_cast<float*>(workspace);
  float* selfkv = cross + align_up(tiger_cross_floats(p, B, St), 4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (prefixed) {
    int64_t* ext_mask = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + plain);
    float* prefix = reinterpret_cast<float*>(static_cast<char*>(workspace) + plain + tiger_mask_bytes(B, S));
    tiger_adapter_kernel<<<dim3((unsigned)B, TG_PREFIX), dim3(AD_THREADS), 0, st>>>(
        *pp, p->shared, p->vocab, p->d_model, input_ids, attention_mask, prof[0], prof[1], prof[2], S, ext_mask, prefix,
        prefix_out);
    if (int rc = check_launch("tiger_adapter_kernel")) return rc;
    tiger_encoder_kernel<true><<<dim3((unsigned)B), dim3(TG_ENC_THREADS), enc_lds, st>>>(*p, input_ids, ext_mask, St,
                                                                                     cross, enc_out, prefix);
    if (int rc = check_launch("tiger_encoder_kernel<true>")) return rc;
    attention_mask = ext_mask;
  } else {
    tiger_encoder_kernel<false><<<dim3((unsigned)B), dim3(TG_ENC_THREADS), enc_lds, st>>>(*p, input_ids, attention_mask, S,
                                                                                     cross, enc_out, nullptr);
    if (int rc = check_launch("tiger_encoder_kernel")) return rc;
  }
  tiger_search_kernel<<<dim3((unsigned)B), dim3(TG_SRCH_THREADS), srch_lds, st>>>(
      *p, attention_mask, St, num_beams, max_length, cross, selfkv, sequences, scores, step_logits);
  return check_launch("tiger_search_kernel");
}

}  // namespace
}  // namespace gr

// The teacher-forced forward (gr_tiger_forward_f32, gr_tiger_forward_prefix_f32): T5ForConditionalGeneration.forward
// with labels in eval mode -- the encoder launch (and the adapter launch) of generate, unchanged, then
//   tiger_teacher_kernel  the decoder over all Ld label positions at once.  A user has at most 8 rows, so a
//                         workgroup takes TF_USERS users (32 rows, the search kernel's row block); row r of a
//                         workgroup is (user r / Ld, position r % Ld).  The current layer's self-attention K/V
//                         stay in LDS; cross K/V are read per user from the workspace.  A wave per row does the
//                         fp32 log-softmax and the label's NLL; a thread per user adds its NLLs in position order.
//   tiger_loss_kernel     one workgroup: the per-user (sum, count) pairs added in a fixed order in double,
//                         loss = sum / count rounded to fp32 once; no atomics.
// Every value of a row is an fma chain over k in order (tg_gemm) or a per-row reduction, so a user's logits
// and NLLs do not depend on its group-mates or on its place in the batch.
namespace gr {
namespace {

constexpr int TF_USERS = 4, TF_ROWS = TF_USERS * TG_MAX_T, TF_LOSS_THREADS = 256;
constexpr int TF_IGNORE = -100, TF_BAD = -1;   // labels in LDS: ignored; outside [0, vocab)
// The LDS layout is fixed at the envelope's largest shapes (32 rows, d_model and heads * d_kv 64, d_ff 256,
// 128 keys, 16 waves), as SR_*: 67 KB per workgroup, two workgroups per compute unit.  q, k and v of the
// layer's attention take the place of the feed-forward's hidden rows (and of the logits).
constexpr int TF_H = 0, TF_XN = TF_H + TF_ROWS * 64, TF_AO = TF_XN + TF_ROWS * 64, TF_FF = TF_AO + TF_ROWS * 64,
              TF_Q = TF_FF, TF_K = TF_Q + TF_ROWS * 64, TF_V = TF_K + TF_ROWS * 64,
              TF_PROW = TF_FF + TF_ROWS * 256, TF_DBIAS = TF_PROW + (TG_SRCH_THREADS / 64) * TG_MAX_S,
              TF_NLL = TF_DBIAS + 8 * TG_MAX_T, TF_TOK = TF_NLL + TF_ROWS, TF_LAB = TF_TOK + TF_ROWS,
              TF_KMASK = TF_LAB + TF_ROWS, TF_TOTAL = TF_KMASK + TF_USERS * TG_MAX_S;
static_assert(TF_V + TF_ROWS * 64 <= TF_PROW && TF_ROWS * TG_MAX_V <= TF_ROWS * 256, "teacher layout");

__global__ __launch_bounds__(TG_SRCH_THREADS) void tiger_teacher_kernel(
    gr_tiger_params p, const int64_t* __restrict__ amask, const int64_t* __restrict__ labels, int64_t B, int S, int Ld,
    const float* __restrict__ cross, float* __restrict__ logits_out, float* __restrict__ nll_out,
    double* __restrict__ pairs) {
  extern __shared__ __align__(16) float lds[];
  int D = p.d_model, dkv = p.d_kv, H = p.n_heads, dff = p.d_ff, V = p.vocab;
  float* h = lds + TF_H;
  float* xn = lds + TF_XN;
  float* ao = lds + TF_AO;
  float* ff = lds + TF_FF;         // feed-forward hidden rows, then the logits
  float* q = lds + TF_Q;
  float* sk = lds + TF_K;
  float* sv = lds + TF_V;
  float* prow = lds + TF_PROW;
  float* dbias = lds + TF_DBIAS;   // decoder relative bias of (distance, head)
  float* nllrow = lds + TF_NLL;
  int* tok = reinterpret_cast<int*>(lds + TF_TOK);   // the shifted decoder input
  int* lab = reinterpret_cast<int*>(lds + TF_LAB);
  int* kmask = reinterpret_cast<int*>(lds + TF_KMASK);

  __shared__ const float* wtab[GR_TIGER_MAX_LAYERS * 13 + 3];   // as in the search kernel
  const float* const* gshared = wtab + GR_TIGER_MAX_LAYERS * 13;
  __shared__ int cint[1];
  __shared__ float cflt[2];
  const int64_t u0 = (int64_t)blockIdx.x * TF_USERS;
  const int nu = B - u0 < TF_USERS ? (int)(B - u0) : TF_USERS;
  int rows = nu * Ld;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int e = tid; e < p.n_dec * 13; e += TG_THREADS) wtab[e] = p.dec[e / 13][e % 13];
  if (tid == 0) {
    cint[0] = p.n_dec;
    cflt[0] = p.eps;
    cflt[1] = p.lm_scale;
    wtab[GR_TIGER_MAX_LAYERS * 13] = p.shared;
    wtab[GR_TIGER_MAX_LAYERS * 13 + 1] = p.lm_head;
    wtab[GR_TIGER_MAX_LAYERS * 13 + 2] = p.dec_final_ln;
  }
  for (int e = tid; e < H * TG_MAX_T; e += TG_THREADS) dbias[e] = p.dec_rel[p.dec_bucket[e / H] * H + e % H];
  for (int e = tid; e < nu * S; e += TG_THREADS)
    kmask[(e / S) * TG_MAX_S + e % S] = amask ? (amask[u0 * S + e] != 0) : 1;
  // T5's _shift_right: the start token, then the labels with -100 replaced by the pad id
  for (int r = tid; r < rows; r += TG_THREADS) {
    const int64_t lb = labels[u0 * Ld + r];
    const int64_t prev = r % Ld ? labels[u0 * Ld + r - 1] : (int64_t)p.pad_id;
    tok[r] = prev == TF_IGNORE ? p.pad_id : tg_token(prev, V);
    lab[r] = lb == TF_IGNORE ? TF_IGNORE : (lb < 0 || lb >= V ? TF_BAD : (int)lb);
  }
  __syncthreads();
  for (int e = tid; e < rows * D; e += TG_THREADS) h[e] = gshared[0][(size_t)tok[e / D] * D + e % D];
  __syncthreads();

  for (int l = 0; l < cint[0]; ++l) {
    TG_OPAQUE(D); TG_OPAQUE(dkv); TG_OPAQUE(H); TG_OPAQUE(dff); TG_OPAQUE(S); TG_OPAQUE(Ld); TG_OPAQUE(rows);
    const int inner = H * dkv;
    const float* const* W = wtab + l * 13;
    const int n_dec = cint[0];
    const float eps = cflt[0];
    // causal self-attention with the decoder's relative bias
    tg_rmsnorm(xn, h, W[D_LN0], rows, D, eps, 1.f);
    __syncthreads();
    tg_gemm<0>(q, inner, xn, D, W[D_Q], inner, D, rows);
    tg_gemm<0>(sk, inner, xn, D, W[D_K], inner, D, rows);
    tg_gemm<0>(sv, inner, xn, D, W[D_V], inner, D, rows);
    __syncthreads();
    for (int it = tid; it < rows * H; it += TG_THREADS) {
      const int r = it / H, hd = it % H, t = r % Ld, r0 = r - t;
      const float* qv = q + r * inner + hd * dkv;
      float s[TG_MAX_T], mx = -INFINITY;
#pragma unroll
      for (int pos = 0; pos < TG_MAX_T; ++pos) {
        s[pos] = -INFINITY;
        if (pos <= t) {
          const float* kr = sk + (r0 + pos) * inner + hd * dkv;
          float a = 0.f;
          for (int c = 0; c < dkv; ++c) a = fmaf(qv[c], kr[c], a);
          s[pos] = a + dbias[(t - pos) * H + hd];
        }
        mx = fmaxf(mx, s[pos]);
      }
      float sum = 0.f;
#pragma unroll
      for (int pos = 0; pos < TG_MAX_T; ++pos) {
        s[pos] = pos <= t ? expf(s[pos] - mx) : 0.f;
        sum += s[pos];
      }
#pragma unroll
      for (int pos = 0; pos < TG_MAX_T; ++pos) s[pos] = s[pos] / sum;
      for (int c = 0; c < dkv; ++c) {
        float a = 0.f;
#pragma unroll
        for (int pos = 0; pos < TG_MAX_T; ++pos)
          if (pos <= t) a = fmaf(s[pos], sv[(r0 + pos) * inner + hd * dkv + c], a);
        ao[r * inner + hd * dkv + c] = a;
      }
    }
    __syncthreads();
    tg_gemm<1>(h, D, ao, inner, W[D_O], D, inner, rows);
    __syncthreads();
    // cross-attention over each row's user's encoder keys (no position bias, padding masked)
    tg_rmsnorm(xn, h, W[D_LN1], rows, D, eps, 1.f);
    __syncthreads();
    tg_gemm<0>(q, inner, xn, D, W[D_CQ], inner, D, rows);
    __syncthreads();
    for (int it0 = 0; it0 < rows * H; it0 += TG_WAVES) {
      const int it = it0 + wave;
      const int r = it / H, hd = it % H, ug = r / Ld;
      float* pr = prow + wave * TG_MAX_S;
      const float* cu = cross + (size_t)(u0 + ug) * n_dec * 2 * S * inner;
      const float* ck = cu + (size_t)(2 * l) * S * inner;
      const float* cv = cu + (size_t)(2 * l + 1) * S * inner;
      if (it < rows * H) {
        const float* qv = q + r * inner + hd * dkv;
        const int* km = kmask + ug * TG_MAX_S;
        float s[2], mx = -INFINITY;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int j = lane + 64 * k2;
          s[k2] = -INFINITY;
          if (j < S && km[j]) {
            const float4* kr = reinterpret_cast<const float4*>(ck + (size_t)j * inner + hd * dkv);
            float a = 0.f;
            for (int c = 0; c < dkv; c += 4) {
              const float4 kk = kr[c >> 2];
              a = fmaf(qv[c], kk.x, a);
              a = fmaf(qv[c + 1], kk.y, a);
              a = fmaf(qv[c + 2], kk.z, a);
              a = fmaf(qv[c + 3], kk.w, a);
            }
            s[k2] = a;
          }
          mx = fmaxf(mx, s[k2]);
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          s[k2] = (s[k2] == -INFINITY) ? 0.f : expf(s[k2] - mx);
          sum += s[k2];
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int j = lane + 64 * k2;
          if (j < S) pr[j] = s[k2] / sum;
        }
      }
      __syncthreads();
      if (it < rows * H) {
        const int c = lane % dkv, g = lane / dkv, G = 64 / dkv;
        float a = 0.f;
        for (int j = g; j < S; j += G) a = fmaf(pr[j], cv[(size_t)j * inner + hd * dkv + c], a);
        a = tg_group_sum(a, dkv);
        if (lane < dkv) ao[r * inner + hd * dkv + c] = a;
      }
      __syncthreads();
    }
    tg_gemm<1>(h, D, ao, inner, W[D_CO], D, inner, rows);
    __syncthreads();
    // feed-forward
    tg_rmsnorm(xn, h, W[D_LN2], rows, D, eps, 1.f);
    __syncthreads();
    tg_gemm<2>(ff, dff, xn, D, W[D_WI], dff, D, rows);
    __syncthreads();
    tg_gemm<1>(h, D, ff, dff, W[D_WO], D, dff, rows);
    __syncthreads();
  }
  TG_OPAQUE(D); TG_OPAQUE(V); TG_OPAQUE(Ld); TG_OPAQUE(rows);
  // lm_head on the scaled final norm; rows of a workgroup are consecutive rows of [B, Ld]
  tg_rmsnorm(xn, h, gshared[2], rows, D, cflt[0], cflt[1]);
  __syncthreads();
  tg_gemm<0>(ff, V, xn, D, gshared[1], V, D, rows);
  __syncthreads();
  if (logits_out)
    for (int e = tid; e < rows * V; e += TG_THREADS) logits_out[(size_t)u0 * Ld * V + e] = ff[e];
  // -log_softmax(logits)[label]: 0 where the label is ignored, NaN where it is outside [0, vocab) (the
  // read itself uses a clamped index)
  for (int r = wave; r < rows; r += TG_WAVES) {
    float v[2], mx = -INFINITY;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const int j = lane + 64 * k2;
      v[k2] = j < V ? ff[r * V + j] : -INFINITY;
      mx = fmaxf(mx, v[k2]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) sum += (lane + 64 * k2 < V) ? expf(v[k2] - mx) : 0.f;
    const float lse = logf(wave_sum(sum));
    if (lane == 0) {
      const int lb = lab[r];
      const float lp = (ff[r * V + min(max(lb, 0), V - 1)] - mx) - lse;
      nllrow[r] = lb == TF_IGNORE ? 0.f : (lb == TF_BAD ? __builtin_nanf("") : -lp);
    }
  }
  __syncthreads();
  if (nll_out)
    for (int r = tid; r < rows; r += TG_THREADS) nll_out[u0 * Ld + r] = nllrow[r];
  if (tid < nu) {
    double s = 0.0;
    int n = 0;
    for (int t = 0; t < Ld; ++t)
      if (lab[tid * Ld + t] != TF_IGNORE) {
        s += (double)nllrow[tid * Ld + t];
        ++n;
      }
    pairs[2 * (u0 + tid)] = s;
    pairs[2 * (u0 + tid) + 1] = (double)n;
  }
}

// loss = sum of the users' NLL sums / sum of their counts (NaN when nothing is counted, as torch's mean over
// no element): thread i adds users i, i + 256, ... in order, then a fixed tree over the threads.
__global__ __launch_bounds__(TF_LOSS_THREADS) void tiger_loss_kernel(const double* __restrict__ pairs, int64_t B,
                                                                     float* __restrict__ loss) {
  __shared__ double ssum[TF_LOSS_THREADS], scnt[TF_LOSS_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0, n = 0.0;
  for (int64_t u = tid; u < B; u += TF_LOSS_THREADS) {
    s += pairs[2 * u];
    n += pairs[2 * u + 1];
  }
  ssum[tid] = s;
  scnt[tid] = n;
  __syncthreads();
  for (int o = TF_LOSS_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      ssum[tid] += ssum[tid + o];
      scnt[tid] += scnt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) *loss = (float)(ssum[0] / scnt[0]);
}

int tiger_raise_lds(const std::string& who) {
  static std::atomic<uint64_t> lds_raised{0};
  int devid = 0;
  if (hipGetDevice(&devid) != hipSuccess) return fail(GR_ERR_HIP, who + "no current device");
  const uint64_t bit = 1ull << (devid & 63);
  if (lds_raised.load() & bit) return GR_OK;
  for (const void* kernel : {reinterpret_cast<const void*>(tiger_encoder_kernel<false>),
                             reinterpret_cast<const void*>(tiger_encoder_kernel<true>),
                             reinterpret_cast<const void*>(tiger_search_kernel),
                             reinterpret_cast<const void*>(tiger_teacher_kernel)})
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTigerLdsMax) != hipSuccess)
      return fail(GR_ERR_HIP, who + "cannot raise the dynamic LDS limit");
  lds_raised.fetch_or(bit);
  return GR_OK;
}

size_t tiger_pairs_bytes(int64_t B) { return align_up((size_t)B * 2 * sizeof(double), 16); }

// cross K/V | per-user (sum, count) pairs [| the [B, S + 3] mask | the prefix tokens]
size_t tiger_forward_plain_bytes(const gr_tiger_params* p, int64_t B, int S) {
  return align_up(tiger_cross_floats(p, B, S) * sizeof(float), 16) + tiger_pairs_bytes(B) + 16;
}

const char* tiger_forward_check(const gr_tiger_params* p, int64_t B, int St, int Ld) {
  if (p && p->vocab < 2) return "vocab_size must be at least 2";
  if (const char* why = tiger_check(p, B, St, 1, 2)) return why;   // the envelope, without a beam or a length
  if (Ld < 1 || Ld > TG_MAX_T) return "labels must hold 1..8 positions (Ld)";
  return nullptr;
}

// Both forward entries, as tiger_generate: pp == nullptr is gr_tiger_forward_f32.
int tiger_forward(const char* fn, const gr_tiger_params* p, const gr_tiger_prefix_params* pp, const int64_t* input_ids,
                  const int64_t* attention_mask, const float* const* prof, const int64_t* labels, int64_t B, int32_t S,
                  int32_t Ld, float* loss, float* logits, float* nll, float* enc_out, void* workspace,
                  size_t workspace_bytes, void* stream, bool prefixed) {
  clear_error();
  const std::string who = std::string(fn) + ": ";
  if (prefixed) {
    if (const char* why = tiger_prefix_check(p, pp, S)) return fail(!p || !pp ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  }
  const int St = prefixed ? S + TG_PREFIX : S;   // encoder positions
  if (const char* why = tiger_forward_check(p, B, St, Ld)) {
    const bool arg = !p || B < 0;
    return fail(arg ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  }
  if (int rc = tiger_check_ids_and_prefix(who, p, pp, prof, prefixed)) return rc;
  const size_t plain = tiger_forward_plain_bytes(p, B, St);
  const size_t need = prefixed ? plain + tiger_mask_bytes(B, S) + tiger_prefix_bytes(p, B) : plain;
  if (!workspace || workspace_bytes < need || !aligned16(workspace))
    return fail(GR_ERR_WORKSPACE, who + "workspace missing, misaligned or smaller than " +
                                      (prefixed ? "gr_tiger_forward_prefix_workspace_bytes"
                                                : "gr_tiger_forward_workspace_bytes"));
  if (!input_ids || !labels || !loss) return fail(GR_ERR_ARG, who + "null pointer");
  if (!tiger_weights_ok(p)) return fail(GR_ERR_ARG, who + "a weight pointer is null or not 16-byte aligned");
  if (B == 0) return GR_OK;
  const size_t enc_lds = tiger_enc_lds(p, St), tf_lds = (size_t)TF_TOTAL * sizeof(float);
  static_assert((size_t)TF_TOTAL * sizeof(float) <= kTigerLdsMax, "teacher layout");
  if (enc_lds > kTigerLdsMax) return fail(GR_ERR_UNSUPPORTED, who + "the per-user state does not fit in LDS");
  if (int rc = tiger_raise_lds(who)) return rc;
  float* cross = static_cast<float*>(workspace);
  char* after = static_cast<char*>(workspace) + align_up(tiger_cross_floats(p, B, St) * sizeof(float), 16);
  double* pairs = reinterpret_cast<double*>(after);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (prefixed) {
    int64_t* ext_mask = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + plain);
    float* prefix = reinterpret_cast<float*>(static_cast<char*>(workspace) + plain + tiger_mask_bytes(B, S));
    tiger_adapter_kernel<<<dim3((unsigned)B, TG_PREFIX), dim3(AD_THREADS), 0, st>>>(
        *pp, p->shared, p->vocab, p->d_model, input_ids, attention_mask, prof[0], prof[1], prof[2], S, ext_mask, prefix,
        nullptr);
    if (int rc = check_launch("tiger_adapter_kernel")) return rc;
    tiger_encoder_kernel<true><<<dim3((unsigned)B), dim3(TG_ENC_THREADS), enc_lds, st>>>(*p, input_ids, ext_mask, St,
                                                                                     cross, enc_out, prefix);
    if (int rc = check_launch("tiger_encoder_kernel<true>")) return rc;
    attention_mask = ext_mask;
  } else {
    tiger_encoder_kernel<false><<<dim3((unsigned)B), dim3(TG_ENC_THREADS), enc_lds, st>>>(*p, input_ids, attention_mask, S,
                                                                                     cross, enc_out, nullptr);
    if (int rc = check_launch("tiger_encoder_kernel")) return rc;
  }
  tiger_teacher_kernel<<<dim3((unsigned)((B + TF_USERS - 1) / TF_USERS)), dim3(TG_SRCH_THREADS), tf_lds, st>>>(
      *p, attention_mask, labels, B, St, Ld, cross, logits, nll, pairs);
  if (int rc = check_launch("tiger_teacher_kernel")) return rc;
  tiger_loss_kernel<<<dim3(1), dim3(TF_LOSS_THREADS), 0, st>>>(pairs, B, loss);
  return check_launch("tiger_loss_kernel");
}

}  // namespace
}  // namespace gr

extern "C" size_t gr_tiger_forward_workspace_bytes(const gr_tiger_params* p, int64_t B, int32_t S, int32_t Ld) {
  if (gr::tiger_forward_check(p, B, S, Ld)) return 0;
  return gr::tiger_forward_plain_bytes(p, B, S);
}

extern "C" int gr_tiger_forward_f32(const gr_tiger_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                                    const int64_t* labels, int64_t B, int32_t S, int32_t Ld, float* loss, float* logits,
                                    float* nll, float* enc_out, void* workspace, size_t workspace_bytes, void* stream) {
  return gr::tiger_forward("gr_tiger_forward_f32", p, nullptr, input_ids, attention_mask, nullptr, labels, B, S, Ld, loss,
                           logits, nll, enc_out, workspace, workspace_bytes, stream, false);
}

extern "C" size_t gr_tiger_forward_prefix_workspace_bytes(const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                                                          int64_t B, int32_t S, int32_t Ld) {
  using namespace gr;
  if (tiger_prefix_check(p, pp, S) || tiger_forward_check(p, B, S + TG_PREFIX, Ld)) return 0;
  return tiger_forward_plain_bytes(p, B, S + TG_PREFIX) + tiger_mask_bytes(B, S) + tiger_prefix_bytes(p, B);
}

extern "C" int gr_tiger_forward_prefix_f32(const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                                           const int64_t* input_ids, const int64_t* attention_mask, const float* prof1,
                                           const float* prof2, const float* prof3, const int64_t* labels, int64_t B,
                                           int32_t S, int32_t Ld, float* loss, float* logits, float* nll, float* enc_out,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  const float* prof[3] = {prof1, prof2, prof3};
  return gr::tiger_forward("gr_tiger_forward_prefix_f32", p, pp, input_ids, attention_mask, prof, labels, B, S, Ld, loss,
                           logits, nll, enc_out, workspace, workspace_bytes, stream, true);
}

extern "C" size_t gr_tiger_workspace_bytes(const gr_tiger_params* p, int64_t B, int32_t S, int32_t num_beams,
                                           int32_t max_length) {
  if (gr::tiger_check(p, B, S, num_beams, max_length)) return 0;
  return gr::tiger_plain_bytes(p, B, S, num_beams, max_length);
}

extern "C" int gr_tiger_generate_f32(const gr_tiger_params* p, const int64_t* input_ids,
                                     const int64_t* attention_mask, int64_t B, int32_t S, int32_t num_beams,
                                     int32_t max_length, int64_t* sequences, float* scores, float* enc_out,
                                     float* step_logits, void* workspace, size_t workspace_bytes, void* stream) {
  return gr::tiger_generate("gr_tiger_generate_f32", p, nullptr, input_ids, attention_mask, nullptr, B, S, num_beams,
                            max_length, sequences, scores, nullptr, enc_out, step_logits, workspace, workspace_bytes,
                            stream, false);
}

extern "C" size_t gr_tiger_prefix_workspace_bytes(const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                                                  int64_t B, int32_t S, int32_t num_beams, int32_t max_length) {
  using namespace gr;
  if (tiger_prefix_check(p, pp, S) || tiger_check(p, B, S + TG_PREFIX, num_beams, max_length)) return 0;
  return tiger_plain_bytes(p, B, S + TG_PREFIX, num_beams, max_length) + tiger_mask_bytes(B, S) + tiger_prefix_bytes(p, B);
}

extern "C" int gr_tiger_generate_prefix_f32(const gr_tiger_params* p, const gr_tiger_prefix_params* pp,
                                            const int64_t* input_ids, const int64_t* attention_mask,
                                            const float* prof1, const float* prof2, const float* prof3, int64_t B,
                                            int32_t S, int32_t num_beams, int32_t max_length, int64_t* sequences,
                                            float* scores, float* prefix_out, float* enc_out, float* step_logits,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  const float* prof[3] = {prof1, prof2, prof3};
  return gr::tiger_generate("gr_tiger_generate_prefix_f32", p, pp, input_ids, attention_mask, prof, B, S, num_beams,
                            max_length, sequences, scores, prefix_out, enc_out, step_logits, workspace, workspace_bytes,
                            stream, true);
}

extern "C" int gr_beam_hits_i64(const int64_t* preds, int64_t B, int32_t k, int32_t pred_len, int64_t ld_pred,
                                const int64_t* labels, int32_t label_len, uint8_t* hits, void* stream) {
  using namespace gr;
  clear_error();
  if (B < 0 || k < 1 || pred_len < 0 || label_len < 1 || ld_pred < pred_len)
    return fail(GR_ERR_ARG, "gr_beam_hits_i64: needs B >= 0, k >= 1, pred_len >= 0, label_len >= 1, ld_pred >= pred_len");
  if (B >= (1ll << 31)) return fail(GR_ERR_UNSUPPORTED, "gr_beam_hits_i64: the batch must hold fewer than 2^31 users");
  if (!preds || !labels || !hits) return fail(GR_ERR_ARG, "gr_beam_hits_i64: null pointer");
  if (B == 0) return GR_OK;
  beam_hits_kernel<<<dim3((unsigned)((B + 127) / 128)), dim3(128), 0, static_cast<hipStream_t>(stream)>>>(
      preds, B, k, pred_len, ld_pred, labels, label_len, hits);
  return check_launch("beam_hits_kernel");
}
