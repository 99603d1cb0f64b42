// BERT text encoder (transformers' BertModel, eager attention, absolute positions, eval mode) with the
// reference's two poolings (T5/item_encode.py:11-34,59-78, major-encode/bert_emb.py:131-168) -- gr_bert_embed_f32.
//
// bert-base is 340 MB of fp32 weights over up to 512 positions, so every projection is a row-tiled GEMM
// over all B * S token rows (the weights are read once per call, not once per sequence) and only the
// attention step runs per sequence.
//
//   be_embed_ln_kernel   a wave per token row: (word[id] + token_type[type]) + position[s], LayerNorm.
//   be_gemm_kernel<T, WM, TM, TN, EPI>   y = epi(A . W^T + bias) per 256-thread workgroup, for two operand formats
//       T (BeF32: both entries' fp32; BeB16: the bf16 entries').  K is staged through a double-buffered LDS image
//       of 128-byte rows on a 144-byte pitch (t5_embed.hip's staging: 16-byte loads, conflict-free 16-byte
//       fragment reads): 32 floats or 64 bf16 deep.  Each wave owns TM x TN blocks of 32 x 32 outputs, one fp32
//       accumulator chain each: 128 x 128 outputs as 2 x 2 waves of four chains (the guide's 128 x 128 x 32 block),
//       64 x 128 as 2 x 2 waves of two, 128 x 96 as 4 x 1 waves of three.  be_gemm picks per launch the tile that
//       leaves the fewest compute units idle (option "bert_tile" forces one).  Up to three weight matrices side by
//       side (q/k/v: one launch).  Epilogues: bias; bias + exact-erf GELU; bias + residual.
//       BeF32 (v_mfma_f32_32x32x2_f32, one float4 per operand per 8-deep slice): each output element is a sum, in k
//       order, of fma chains of 256 consecutive k each (per 8-deep slice in the order 0 4 1 5 2 6 3 7): a chain is
//       closed into a second accumulator every eight stages, because one chain over K = 3072 rounds about three
//       times as much as the blocked sum.  fp32 output.
//       BeB16 (v_mfma_f32_32x32x16_bf16, eight bf16 per operand per 16-deep step): K is a multiple of 32, so the last
//       stage may be half zeros, never read from memory.  One fp32 chain per element, k ascending in steps of 16:
//       bf16 products are exact in fp32 and K <= 4096, so the 256-deep blocking buys nothing next to the operands'
//       2^-9.  Output bf16 (bias, GELU) or fp32 (residual).
//       Every tile uses its format's order, so the choice changes no bit.
//   be_attn_kernel<HD>   one workgroup per (sequence, head, 128 queries), a wave per 32 queries.  Key / value
//       tiles of 32 positions stream through a double-buffered LDS image shared by the four waves; tiles
//       with no live key are never loaded.  Scores are taken transposed (A rows are keys, B columns are
//       queries) so a query's 32 scores sit in one lane pair; fp32 online softmax (running max and sum per
//       query, the accumulator rescaled once per visited tile, tiles in ascending order); P . v takes the
//       probability registers as they stand as the A operand.
//   be_ln_kernel         a wave per row: LayerNorm of the GEMM's bias + residual output.
//   be_pool_kernel       a thread per feature, the live rows after position 0 added in position order with a
//       compensated sum (mean_no_cls) or row 0 (cls); zeros for a sequence with no live key.
//
// LayerNorm is two-pass (mean, then centred squares), biased variance, eps inside the square root.
// Every output element has one summation order that depends on neither B nor the row's tile position,
// and nothing uses atomics, so a call is bitwise repeatable and batch-invariant.
//
// gr_bert_embed_ragged_f32 runs the same kernels in their RAGGED instantiation over rows [0, len_b) of each sequence
// only (len_b: one past the last live position), packed at off[b] + s:
//   be_len_kernel        a wave per sequence: len_b by a ballot per 64 positions.
//   be_offsets_kernel    one workgroup: off = exclusive prefix sum of len, the total, the overflow flag.
// The caller's row bound sizes the workspace and the grids; the total is read on the device, and a tile, wave or
// query tile past it exits.  The sums' orders are the padded call's, so the kept rows and the pooled vectors have
// its bits.  The padded instantiations take the row map (BeRows) and never read it.
//
// gr_bert_embed_bf16 / gr_bert_embed_ragged_bf16: the same encoder, the same layer loop (be_forward) and the same
// GEMM on bf16 operands (opt-in; the fp32 entries keep their bits).  bf16 = the upper 16 bits of the RNE-rounded
// fp32.  The contract:
//   GEMM operands   A and W of the four projections per layer (fused q/k/v, attention output, intermediate, output)
//                   are bf16, accumulated in fp32 in the MFMA accumulator (v_mfma_f32_32x32x16_bf16).
//   epilogues       bias, exact-erf GELU, residual add (be_epilogue, the fp32 kernel's own expressions), both
//                   LayerNorms (two-pass), the softmax's max / exp / sum and the pooling are fp32.
//   residual        the residual stream and the last hidden state stay fp32.
//   q, k, v         rounded to bf16 once, in the q/k/v GEMM's epilogue.
//   scores          fp32 from a bf16 MFMA, the 1 / sqrt(head_dim) scale applied in fp32.
//   probabilities   the un-normalised exp(s - running max) is rounded to bf16 where it becomes the P . v operand; the
//                   row sum adds, in fp32, those same rounded values, so a row's weights sum to 1 within fp32.
//   masking         as the fp32 call: a masked key has probability exactly 0, tiles with no live key are skipped, a
//                   sequence with no live key gives zeros, holes are legal.
//   context, GELU   written as bf16 (they are only ever GEMM A operands); each LayerNorm writes its fp32 row for
//                   the residual and a bf16 copy for the next GEMM.
//   weights         the six [out, in] matrices per layer are bf16; tables, biases and LayerNorm parameters fp32.
//   determinism     one summation order per output element (k ascending in steps of 16, the order inside a step is
//                   the instruction's), whatever B, the row's place in a tile or the tile; no atomics: bitwise
//                   repeatable, batch-invariant, and the ragged form returns the padded form's bits.
//   be_attn_bf16_kernel<HD>   be_attn_kernel's grid and tile order on bf16 q/k/v.  Scores transposed (A rows are keys,
//       B columns are queries); the probability registers, rounded pairwise, are the B operand of
//       O^T = V^T . P^T, so a query's running max, sum and output column all sit in its own lane; v is staged
//       transposed, its keys in the order the accumulator's registers hold them.
//   workspace on return   what a test may read after the call; not an interface for callers.  The six parts of
//       BeLayout, in order, each rounded up to 16 bytes, hold the LAST layer's intermediates over R rows (B * S, or
//       the packed rows): x fp32 [R, H] the post-attention LayerNorm output (the final hidden state instead when
//       hidden_out is NULL); t fp32 [R, H] x + output.dense(ff) + bias, the final LayerNorm's input; x16 bf16 [R, H]
//       the RNE copy of the final LayerNorm's fp32 rows (be_pool_kernel zeroes hidden_out alone for a sequence with no
//       live key); qkv bf16 [R, 3H] q | k | v; ctx bf16 [R, H] the attention context; ff bf16 [R, I] the GELU output.
//       tests/bert_bf16_stages.py checks each stage in float64 on these operands.
#include <type_traits>

#include "gr_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace gr {
namespace {

constexpr int BE_MAX_S = 512, BE_MAX_H = 1024, BE_MAX_I = 4096;
constexpr int64_t BE_MAX_B = 1ll << 16;
constexpr int BE_NT = 256;
constexpr int BE_QT = 128, BE_KT = 32;     // queries per workgroup, keys per streamed tile
enum { BE_EPI_BIAS = 0, BE_EPI_GELU = 1, BE_EPI_RESID = 2 };

// The GEMM's two operand formats.  E: the element of A and W; V: the 16 bytes a thread stages and a lane reads per
// fragment; BK elements per staged row (128 bytes) on a pitch of PITCH (144 bytes); VE elements per 16-byte piece;
// KD: the k depth one fragment read covers; KFLUSH: stages per fma chain (0: one chain over all of K).
struct BeF32 {
  using E = float;
  using V = f32x4;
  static constexpr int BK = 32, PITCH = BK + 4, VE = 4, KD = 8;
  static constexpr int KFLUSH = 8;   // 32-deep stages per fma chain: 256 deep
};
struct BeB16 {
  using E = uint16_t;
  using V = u32x4;
  static constexpr int BK = 64, PITCH = BK + 8, VE = 8, KD = 16;
  static constexpr int KFLUSH = 0;   // bf16 products are exact in fp32 and K <= 4096: blocking buys nothing
};

// What follows a GEMM's sum, in either format: the bias, then exact-erf GELU or the residual add.
template <int EPI>
__device__ __forceinline__ float be_epilogue(float sum, float bias, const float* __restrict__ residual, int64_t at) {
  float o = sum + bias;
  if constexpr (EPI == BE_EPI_GELU) o = 0.5f * o * (1.0f + erff(o * 0.70710678118654752440f));
  if constexpr (EPI == BE_EPI_RESID) o = residual[at] + o;
  return o;
}

// bf16 = the upper 16 bits of the RNE-rounded fp32 (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint16_t be_bf16(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }
__device__ __forceinline__ f32x16 mfma32_bf16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// The ragged call's row map, in the workspace: len[b] kept rows of sequence b (one past its last live position),
// off[b] their first packed row, total = off[B], flag != 0 when the mask held more rows than the caller's bound
// (then every len is 0 and total is 0).  The padded kernels take it and never read it.
struct BeRows {
  const int32_t* len;
  const int64_t* off;
  const int64_t* total;
  const int32_t* flag;
};

template <typename E>
struct BeSeg {   // up to three [seg_n, K] weight matrices side by side, and their biases
  const E* w[3];
  const float* b[3];
};

// One 8-deep (fp32) or 16-deep (bf16) slice into every accumulator chain a wave owns.  fp32: step s, the outermost
// loop, takes k = s from lane half 0 and k = 4 + s from half 1: the contract's order 0 4 1 5 2 6 3 7.
template <int TM, int TN>
__device__ __forceinline__ void be_mma(const f32x4 (&a)[TM], const f32x4 (&b)[TN], f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(a[i][s], b[j][s], acc[i][j]);
}
template <int TM, int TN>
__device__ __forceinline__ void be_mma(const u32x4 (&a)[TM], const u32x4 (&b)[TN], f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = mfma32_bf16(a[i], b[j], acc[i][j]);
}

// y: fp32 from fp32 operands and after the residual add, bf16 otherwise (it is then only ever a GEMM A operand)
template <typename T, int EPI>
using BeOut = std::conditional_t<EPI == BE_EPI_RESID, float, typename T::E>;

// T: BeF32 or BeB16; x [M, K] and the weights [seg_n, K] of T::E, fp32 accumulation, be_epilogue.
// WM waves down the tile's rows (4 / WM across its columns), each owning TM x TN blocks of 32 x 32 outputs.  Lane
// (r, h) of a wave takes, per slice, the 16 bytes at k = VE h of row r of each operand from the LDS image.
// RAGGED: the grid covers the caller's row bound (M_), the row count is rg.total[0]; a tile at or past it exits.
template <typename T, int WM, int TM, int TN, int EPI, bool RAGGED>
__global__ __launch_bounds__(BE_NT, 2) void be_gemm_kernel(const typename T::E* __restrict__ x, BeSeg<typename T::E> sg,
                                                           int seg_n, const float* __restrict__ residual,
                                                           void* __restrict__ y_, int64_t M_, int N, int K,
                                                           int tiles_n, BeRows rg) {
  using E = typename T::E;
  using V = typename T::V;
  BeOut<T, EPI>* __restrict__ y = static_cast<BeOut<T, EPI>*>(y_);
  constexpr int WN = 4 / WM, BM = 32 * WM * TM, BN = 32 * WN * TN;
  int64_t M = M_;
  if constexpr (RAGGED) {
    M = rg.total[0];
    if ((int64_t)(blockIdx.x / tiles_n) * BM >= M) return;
  }
  __shared__ __attribute__((aligned(16))) E lds[2][(BM + BN) * T::PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, r = lane & 31, h = lane >> 5;
  const int tni = blockIdx.x % tiles_n;
  const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * BM;
  const int n0 = tni * BN;

  constexpr int AV = BM * T::BK / T::VE / BE_NT, BV = BN * T::BK / T::VE / BE_NT;
  V ra[AV], rb[BV];
  // eight 16-byte pieces per staged row.  K is a multiple of 32 and kk of VE: a piece lies inside the row or wholly
  // past it (then zeros, never read from memory: the last bf16 stage may be half zeros)
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < AV; ++i) {
      const int f = tid + BE_NT * i, row = f >> 3, kk = k0 + (f & 7) * T::VE;
      const int64_t g = m0 + row;
      ra[i] = (g < M && kk < K) ? *reinterpret_cast<const V*>(x + g * K + kk) : V{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < BV; ++i) {
      const int f = tid + BE_NT * i, row = f >> 3, kk = k0 + (f & 7) * T::VE;
      const int gn = n0 + row;
      V v = {0, 0, 0, 0};
      if (gn < N && kk < K) {
        const int seg = gn / seg_n, wr = gn - seg * seg_n;
        const E* wp = seg == 0 ? sg.w[0] : seg == 1 ? sg.w[1] : sg.w[2];
        v = *reinterpret_cast<const V*>(wp + (int64_t)wr * K + kk);
      }
      rb[i] = v;
    }
  };
  auto swrite = [&](int buf) {
    E* s = lds[buf];
#pragma unroll
    for (int i = 0; i < AV; ++i) {
      const int f = tid + BE_NT * i;
      *reinterpret_cast<V*>(s + (f >> 3) * T::PITCH + (f & 7) * T::VE) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < BV; ++i) {
      const int f = tid + BE_NT * i;
      *reinterpret_cast<V*>(s + (BM + (f >> 3)) * T::PITCH + (f & 7) * T::VE) = rb[i];
    }
  };

  f32x16 acc[TM][TN], tot[TM][TN];   // tot: the closed chains' sum, with KFLUSH only
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        acc[i][j][v] = 0.f;
        if constexpr (T::KFLUSH > 0) tot[i][j][v] = 0.f;
      }

  const int nk = (K + T::BK - 1) / T::BK;
  gload(0);
  swrite(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * T::BK);
    const E* As = lds[cur] + (wm * 32 * TM + r) * T::PITCH + T::VE * h;
    const E* Bs = lds[cur] + (BM + wn * 32 * TN + r) * T::PITCH + T::VE * h;
#pragma unroll
    for (int kc = 0; kc < T::BK / T::KD; ++kc) {
      V a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const V*>(As + i * 32 * T::PITCH + kc * T::KD);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const V*>(Bs + j * 32 * T::PITCH + kc * T::KD);
      be_mma(a, b, acc);
    }
    if constexpr (T::KFLUSH > 0) {
      if ((kt + 1) % T::KFLUSH == 0 || kt + 1 == nk) {   // close the 256-deep chain: a short chain rounds less
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            tot[i][j] += acc[i][j];
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
          }
      }
    }
    if (kt + 1 < nk) swrite(cur ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * 32 * TN + j * 32 + r;
    if (col >= N) continue;
    const int seg = col / seg_n;
    const float* bp = seg == 0 ? sg.b[0] : seg == 1 ? sg.b[1] : sg.b[2];
    const float bv = bp[col - seg * seg_n];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t row = m0 + wm * 32 * TM + i * 32 + mfma32_row(v, h);
        if (row < M) {
          float sum;
          if constexpr (T::KFLUSH > 0) sum = tot[i][j][v];
          else sum = acc[i][j][v];
          const float o = be_epilogue<EPI>(sum, bv, residual, row * N + col);
          if constexpr (std::is_same_v<BeOut<T, EPI>, float>) y[row * N + col] = o;
          else y[row * N + col] = be_bf16(o);
        }
      }
    }
  }
}

// LayerNorm of the row a wave holds as xv[t] = x[lane + 64 t] (0 past H), written to out and, BF16, rounded to out16.
template <bool BF16>
__device__ __forceinline__ void be_ln_row(float (&xv)[BE_MAX_H / 64], int lane, int H, const float* __restrict__ w,
                                          const float* __restrict__ b, float eps, float* __restrict__ out,
                                          uint16_t* __restrict__ out16) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < BE_MAX_H / 64; ++t) s += xv[t];
  const float mean = wave_sum(s) / (float)H;
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < BE_MAX_H / 64; ++t) {
    xv[t] = lane + 64 * t < H ? xv[t] - mean : 0.f;
    ss = fmaf(xv[t], xv[t], ss);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)H + eps);
#pragma unroll
  for (int t = 0; t < BE_MAX_H / 64; ++t) {
    const int c = lane + 64 * t;
    if (c < H) {
      const float o = (xv[t] * rstd) * w[c] + b[c];
      out[c] = o;
      if constexpr (BF16) out16[c] = be_bf16(o);
    }
  }
}

// RAGGED: grid (sequence, four positions); position s < len[b] of sequence b is written at packed row off[b] + s.
// BF16: the row is also written, rounded, to out16 (the next GEMM's operand); out16 is not read otherwise.
template <bool RAGGED, bool BF16>
__global__ __launch_bounds__(256) void be_embed_ln_kernel(const int64_t* __restrict__ ids,
                                                          const int64_t* __restrict__ type_ids,
                                                          const float* __restrict__ word, const float* __restrict__ pos,
                                                          const float* __restrict__ type, const float* __restrict__ lnw,
                                                          const float* __restrict__ lnb, float eps, int vocab,
                                                          int type_vocab, int S, int H, int64_t M, float* __restrict__ out,
                                                          uint16_t* __restrict__ out16, BeRows rg) {
  const int lane = threadIdx.x & 63;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // of ids
  int64_t orow = row;                                           // of out
  if constexpr (RAGGED) {
    const int sp = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (sp >= rg.len[blockIdx.x]) return;
    row = (int64_t)blockIdx.x * S + sp;
    orow = rg.off[blockIdx.x] + sp;
  } else if (row >= M) {
    return;
  }
  int64_t id = ids[row];
  id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
  int64_t tt = type_ids != nullptr ? type_ids[row] : 0;
  tt = tt < 0 ? 0 : tt >= type_vocab ? type_vocab - 1 : tt;
  const int s = (int)(row % S);
  const float* wr = word + id * H;
  const float* tr = type + tt * H;
  const float* pr = pos + (int64_t)s * H;
  float xv[BE_MAX_H / 64];
#pragma unroll
  for (int t = 0; t < BE_MAX_H / 64; ++t) {
    const int c = lane + 64 * t;
    xv[t] = c < H ? (wr[c] + tr[c]) + pr[c] : 0.f;
  }
  be_ln_row<BF16>(xv, lane, H, lnw, lnb, eps, out + orow * H, BF16 ? out16 + orow * H : nullptr);
}

template <bool RAGGED, bool BF16>
__global__ __launch_bounds__(256) void be_ln_kernel(const float* __restrict__ in, const float* __restrict__ lnw,
                                                    const float* __restrict__ lnb, float eps, int H, int64_t M_,
                                                    float* __restrict__ out, uint16_t* __restrict__ out16, BeRows rg) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  int64_t M = M_;
  if constexpr (RAGGED) M = rg.total[0];
  if (row >= M) return;
  float xv[BE_MAX_H / 64];
#pragma unroll
  for (int t = 0; t < BE_MAX_H / 64; ++t) {
    const int c = lane + 64 * t;
    xv[t] = c < H ? in[row * H + c] : 0.f;
  }
  be_ln_row<BF16>(xv, lane, H, lnw, lnb, eps, out + row * H, BF16 ? out16 + row * H : nullptr);
}

// RAGGED: the sequence's rows are the packed rows off[b] .. off[b] + len[b]; SL = len[b] takes S's place in the row
// and key clamps and in the store guard, and a query tile at or past it exits.  The mask, the key tiles and their
// order stay the padded call's (positions from len[b] on are dead), so the live rows get the padded call's bits.
template <int HD, bool RAGGED>
__global__ __launch_bounds__(256) void be_attn_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                      float* __restrict__ ctx, int S, int NH, int nqt, float scale,
                                                      BeRows rg) {
  constexpr int P = HD + 4, NKC = HD / 8, NDB = HD / 32, LV = 2 * BE_KT * HD / 4 / 256;
  __shared__ __attribute__((aligned(16))) float kv[2][2 * BE_KT * P];
  __shared__ uint32_t livebits[BE_MAX_S / BE_KT];
  __shared__ int tiles[BE_MAX_S / BE_KT];
  __shared__ int ntl_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int qt = blockIdx.x % nqt, head = (blockIdx.x / nqt) % NH;
  const int64_t b = blockIdx.x / (nqt * NH);
  const int Hd = NH * HD, ld = 3 * Hd;
  int SL = S;                 // rows of this sequence
  int64_t row0 = b * S;       // its first row in qkv and ctx
  if constexpr (RAGGED) {
    SL = rg.len[b];
    row0 = rg.off[b];
    if (qt * BE_QT >= SL) return;   // uniform over the workgroup, before any barrier
  }
  const float* base = qkv + row0 * ld + head * HD;
  const int nt = (S + BE_KT - 1) / BE_KT;

  // bit j of livebits[t]: position 32 t + j is a key; tiles[]: the tiles that hold one, ascending
  for (int t = wave; t < nt; t += 4) {
    const int j = BE_KT * t + lane;
    const bool live = lane < BE_KT && j < S && (mask == nullptr || mask[b * S + j] != 0);
    const uint32_t bits = (uint32_t)__ballot(live);
    if (lane == 0) livebits[t] = bits;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int t = 0; t < nt; ++t)
      if (livebits[t] != 0u) tiles[n++] = t;
    ntl_s = n;
  }
  __syncthreads();
  const int ntl = ntl_s;

  const int q0 = qt * BE_QT + 32 * wave;
  const bool active = q0 < SL;            // wave-uniform
  const int qrow = q0 + r < SL ? q0 + r : SL - 1;   // rows past SL read row SL - 1, never stored
  f32x4 q[NKC];
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) q[kc] = *reinterpret_cast<const f32x4*>(base + (int64_t)qrow * ld + 8 * kc + 4 * h);

  f32x4 rk[LV];
  auto gload = [&](int t) {
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = tid + 256 * i, mat = f / (BE_KT * HD / 4), rem = f % (BE_KT * HD / 4);
      const int row = rem / (HD / 4), c4 = rem % (HD / 4);
      const int key = BE_KT * t + row < SL ? BE_KT * t + row : SL - 1;   // past SL: finite, weighted 0
      rk[i] = *reinterpret_cast<const f32x4*>(base + (int64_t)key * ld + (1 + mat) * Hd + 4 * c4);
    }
  };
  auto swrite = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = tid + 256 * i, mat = f / (BE_KT * HD / 4), rem = f % (BE_KT * HD / 4);
      const int row = rem / (HD / 4), c4 = rem % (HD / 4);
      *reinterpret_cast<f32x4*>(&kv[buf][(mat * BE_KT + row) * P + 4 * c4]) = rk[i];
    }
  };

  f32x16 o[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int v = 0; v < 16; ++v) o[d][v] = 0.f;
  float m = -INFINITY, l = 0.f;   // of query r, the same in both lanes of the pair

  if (ntl > 0) {
    gload(tiles[0]);
    swrite(0);
  }
  __syncthreads();
  for (int it = 0; it < ntl; ++it) {
    const int cur = it & 1;
    if (it + 1 < ntl) gload(tiles[it + 1]);
    if (active) {
      const uint32_t bits = livebits[tiles[it]];
      const float* Ks = kv[cur] + r * P + 4 * h;
      const float* Vs = kv[cur] + BE_KT * P;
      // scores, transposed: D register v of lane (r, h) is key mfma32_row(v, h) against query r
      f32x16 sc;
#pragma unroll
      for (int v = 0; v < 16; ++v) sc[v] = 0.f;
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        const f32x4 kf = *reinterpret_cast<const f32x4*>(Ks + 8 * kc);
#pragma unroll
        for (int s = 0; s < 4; ++s) sc = mfma32(kf[s], q[kc][s], sc);
      }
      float mt = -INFINITY;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float a = ((bits >> mfma32_row(v, h)) & 1u) ? sc[v] * scale : -INFINITY;
        sc[v] = a;
        mt = fmaxf(mt, a);
      }
      mt = xmax<32>(mt);                       // the other sixteen keys of this query; finite: the tile has a live key
      const float mn = fmaxf(m, mt);
      const float alpha = expf(m - mn);        // 0 on the first visited tile (m = -inf)
      float sum = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        sc[v] = expf(sc[v] - mn);              // exactly 0 for a masked key
        sum += sc[v];
      }
      sum = xsum<32>(sum);
      l = fmaf(l, alpha, sum);
      m = mn;
      // the accumulator's rows are queries mfma32_row(v, h): fetch their alpha from the lanes that own them
      float av[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) av[v] = __shfl(alpha, mfma32_row(v, h), 64);
#pragma unroll
      for (int d = 0; d < NDB; ++d) {
#pragma unroll
        for (int v = 0; v < 16; ++v) o[d][v] = o[d][v] * av[v];
        // step s takes key mfma32_row(s, h) from lane half h: register s of the probabilities as they stand
#pragma unroll
        for (int s = 0; s < 16; ++s) o[d] = mfma32(sc[s], Vs[mfma32_row(s, h) * P + 32 * d + r], o[d]);
      }
    }
    if (it + 1 < ntl) swrite(cur ^ 1);
    __syncthreads();
  }

  if (active) {
    float lv[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) lv[v] = __shfl(l, mfma32_row(v, h), 64);
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int qi = q0 + mfma32_row(v, h);
        if (qi < SL) ctx[(row0 + qi) * Hd + head * HD + 32 * d + r] = lv[v] > 0.f ? o[d][v] / lv[v] : 0.f;
      }
  }
}

// be_attn_kernel on bf16 q/k/v (rows of 3 Hd bf16), bf16 context.  Per visited tile: S^T = K . Q^T (D register v of
// lane (r, h): key mfma32_row(v, h) against query r), the fp32 softmax step, then O^T += V^T . P^T with the rounded
// probabilities as the B operand: registers 8 s .. 8 s + 7 are k-step s, so element j of lane half h is key
// 16 s + 8 (j >> 2) + 4 h + (j & 3), and v is staged as vt[d][16 s + 8 h + j] = v[that key][d] to match.  O^T has
// query r on the lane and d = mfma32_row(v, h) in the registers: alpha and the row sum are the lane's own.
template <int HD, bool RAGGED>
__global__ __launch_bounds__(256) void be_attn_bf16_kernel(const uint16_t* __restrict__ qkv,
                                                           const int64_t* __restrict__ mask, uint16_t* __restrict__ ctx,
                                                           int S, int NH, int nqt, float scale, BeRows rg) {
  constexpr int PK = HD + 8, PV = BE_KT + 8, NKS = HD / 16, NDB = HD / 32, LV = 2 * BE_KT * HD / 8 / 256;
  constexpr int PER = BE_KT * HD / 8;   // 16-byte pieces per matrix per tile
  __shared__ __attribute__((aligned(16))) uint16_t ks[2][BE_KT * PK];
  __shared__ __attribute__((aligned(16))) uint16_t vt[2][HD * PV];
  __shared__ uint32_t livebits[BE_MAX_S / BE_KT];
  __shared__ int tiles[BE_MAX_S / BE_KT];
  __shared__ int ntl_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int qt = blockIdx.x % nqt, head = (blockIdx.x / nqt) % NH;
  const int64_t b = blockIdx.x / (nqt * NH);
  const int Hd = NH * HD, ld = 3 * Hd;
  int SL = S;                 // rows of this sequence
  int64_t row0 = b * S;       // its first row in qkv and ctx
  if constexpr (RAGGED) {
    SL = rg.len[b];
    row0 = rg.off[b];
    if (qt * BE_QT >= SL) return;   // uniform over the workgroup, before any barrier
  }
  const uint16_t* base = qkv + row0 * ld + head * HD;
  const int nt = (S + BE_KT - 1) / BE_KT;

  for (int t = wave; t < nt; t += 4) {
    const int j = BE_KT * t + lane;
    const bool live = lane < BE_KT && j < S && (mask == nullptr || mask[b * S + j] != 0);
    const uint32_t bits = (uint32_t)__ballot(live);
    if (lane == 0) livebits[t] = bits;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int t = 0; t < nt; ++t)
      if (livebits[t] != 0u) tiles[n++] = t;
    ntl_s = n;
  }
  __syncthreads();
  const int ntl = ntl_s;

  const int q0 = qt * BE_QT + 32 * wave;
  const bool active = q0 < SL;            // wave-uniform
  const int qrow = q0 + r < SL ? q0 + r : SL - 1;   // rows past SL read row SL - 1, never stored
  u32x4 q[NKS];
#pragma unroll
  for (int kc = 0; kc < NKS; ++kc) q[kc] = *reinterpret_cast<const u32x4*>(base + (int64_t)qrow * ld + 16 * kc + 8 * h);

  u32x4 rk[LV];
  auto gload = [&](int t) {
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = tid + 256 * i, mat = f / PER, rem = f % PER;
      const int row = rem / (HD / 8), c8 = rem % (HD / 8);
      const int key = BE_KT * t + row < SL ? BE_KT * t + row : SL - 1;   // past SL: finite, weighted 0
      rk[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)key * ld + (1 + mat) * Hd + 8 * c8);
    }
  };
  auto swrite = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = tid + 256 * i, mat = f / PER, rem = f % PER;
      const int row = rem / (HD / 8), c8 = rem % (HD / 8);
      if (mat == 0) {
        *reinterpret_cast<u32x4*>(&ks[buf][row * PK + 8 * c8]) = rk[i];
      } else {
        const int at = (row & 16) | (((row >> 2) & 1) << 3) | (((row >> 3) & 1) << 2) | (row & 3);
#pragma unroll
        for (int e = 0; e < 8; ++e) vt[buf][(8 * c8 + e) * PV + at] = (uint16_t)(rk[i][e >> 1] >> (16 * (e & 1)));
      }
    }
  };

  f32x16 o[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int v = 0; v < 16; ++v) o[d][v] = 0.f;
  float m = -INFINITY, l = 0.f;   // of query r, the same in both lanes of the pair

  if (ntl > 0) {
    gload(tiles[0]);
    swrite(0);
  }
  __syncthreads();
  for (int it = 0; it < ntl; ++it) {
    const int cur = it & 1;
    if (it + 1 < ntl) gload(tiles[it + 1]);
    if (active) {
      const uint32_t bits = livebits[tiles[it]];
      const uint16_t* Ks = ks[cur] + r * PK + 8 * h;
      const uint16_t* Vs = vt[cur] + r * PV + 8 * h;
      f32x16 sc;
#pragma unroll
      for (int v = 0; v < 16; ++v) sc[v] = 0.f;
#pragma unroll
      for (int kc = 0; kc < NKS; ++kc) sc = mfma32_bf16(*reinterpret_cast<const u32x4*>(Ks + 16 * kc), q[kc], sc);
      float mt = -INFINITY;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float a = ((bits >> mfma32_row(v, h)) & 1u) ? sc[v] * scale : -INFINITY;
        sc[v] = a;
        mt = fmaxf(mt, a);
      }
      mt = xmax<32>(mt);                       // the other sixteen keys of this query; finite: the tile has a live key
      const float mn = fmaxf(m, mt);
      const float alpha = expf(m - mn);        // 0 on the first visited tile (m = -inf)
      float sum = 0.f;
      bf16x8 pf[2];                            // the rounded weights: P . v's operand and the row sum's terms
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const __bf16 pb = (__bf16)expf(sc[v] - mn);   // exactly 0 for a masked key
        pf[v >> 3][v & 7] = pb;
        sum += (float)pb;
      }
      sum = xsum<32>(sum);
      l = fmaf(l, alpha, sum);
      m = mn;
#pragma unroll
      for (int d = 0; d < NDB; ++d) {
#pragma unroll
        for (int v = 0; v < 16; ++v) o[d][v] = o[d][v] * alpha;
#pragma unroll
        for (int s = 0; s < 2; ++s)
          o[d] = mfma32_bf16(*reinterpret_cast<const u32x4*>(Vs + 32 * d * PV + 16 * s),
                             __builtin_bit_cast(u32x4, pf[s]), o[d]);
      }
    }
    if (it + 1 < ntl) swrite(cur ^ 1);
    __syncthreads();
  }

  if (active && q0 + r < SL) {
    uint16_t* out = ctx + (row0 + q0 + r) * Hd + head * HD + 4 * h;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3: d = 32 d + 8 g + 4 h + 0 .. 3
        uint32_t w2[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float lo = l > 0.f ? o[d][4 * g + 2 * e] / l : 0.f, hi = l > 0.f ? o[d][4 * g + 2 * e + 1] / l : 0.f;
          w2[e] = (uint32_t)be_bf16(lo) | ((uint32_t)be_bf16(hi) << 16);
        }
        *reinterpret_cast<uint2*>(out + 32 * d + 8 * g) = make_uint2(w2[0], w2[1]);
      }
  }
}

// mode 0: no pooling; 1: mean over the live rows after position 0; 2: row 0.  A sequence with no live
// key gets zeros in pooled and in hidden_out.  hid: the last hidden state (hidden_out itself when given).
// RAGGED: hid holds packed rows (row i of the sequence at off[b] + i, i < len[b]; hidden_out is not used); NaN in
// pooled when the flag is set.
template <bool RAGGED>
__global__ __launch_bounds__(256) void be_pool_kernel(const float* hid, const int64_t* __restrict__ mask, int S, int H,
                                                      int mode, float* __restrict__ pooled, float* hidden_out, BeRows rg) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  const int64_t b = blockIdx.x;
  const bool col = c < H;
  int SL = S;
  int64_t row0 = 0;   // the sequence's first packed row
  if constexpr (RAGGED) {
    if (rg.flag[0] != 0) {
      if (col && mode != 0) pooled[b * H + c] = __builtin_nanf("");
      return;
    }
    SL = rg.len[b];
    row0 = rg.off[b];
  }
  bool any = false;
  int cnt = 0;
  float acc = 0.f, lost = 0.f;   // compensated (Kahan) sum in position order: up to 511 rows
  for (int i = 0; i < SL; ++i) {
    const bool lv = mask == nullptr || mask[b * S + i] != 0;
    any = any || lv;
    if (i >= 1 && lv) {
      ++cnt;
      if (mode == 1 && col) {
        float y;
        if constexpr (RAGGED) y = hid[(row0 + i) * H + c] - lost;
        else y = hid[(b * S + i) * H + c] - lost;
        const float t = acc + y;
        lost = (t - acc) - y;
        acc = t;
      }
    }
  }
  if (!col) return;
  if (mode == 1) pooled[b * H + c] = acc / fmaxf((float)cnt, 1e-9f);
  if constexpr (RAGGED) {
    if (mode == 2) pooled[b * H + c] = any ? hid[row0 * H + c] : 0.f;
  } else {
    if (mode == 2) pooled[b * H + c] = any ? hid[b * S * H + c] : 0.f;
    if (!any && hidden_out != nullptr)
      for (int i = 0; i < S; ++i) hidden_out[(b * S + i) * H + c] = 0.f;
  }
}

// len[b]: one past the last live position of sequence b (0: no live key; S with no mask).  A wave per sequence, a
// ballot per 64 positions.
__global__ __launch_bounds__(256) void be_len_kernel(const int64_t* __restrict__ mask, int64_t B, int S,
                                                     int32_t* __restrict__ len) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  int n = mask == nullptr ? S : 0;
  if (mask != nullptr)
    for (int s0 = 0; s0 < S; s0 += 64) {
      const bool live = s0 + lane < S && mask[b * S + s0 + lane] != 0;
      const uint64_t bits = __ballot(live);
      if (bits != 0) n = s0 + 64 - __builtin_clzll(bits);
    }
  if (lane == 0) len[b] = n;
}

// One workgroup: off = exclusive prefix sum of len, off[B] = total = the packed row count.  When it exceeds
// bound: every len and off 0, total 0, flag 1, and -1 in the caller's last offset.  No atomics.
constexpr int BE_SCAN_NT = 1024;
__global__ __launch_bounds__(BE_SCAN_NT) void be_offsets_kernel(int32_t* __restrict__ len, int64_t B, int64_t bound,
                                                               int64_t* __restrict__ off, int64_t* __restrict__ total,
                                                               int32_t* __restrict__ flag, int64_t* __restrict__ off_out) {
  __shared__ int64_t part[BE_SCAN_NT];
  __shared__ int64_t first[BE_SCAN_NT + 1];
  const int tid = threadIdx.x;
  const int64_t per = (B + BE_SCAN_NT - 1) / BE_SCAN_NT;
  const int64_t lo = tid * per < B ? tid * per : B, hi = lo + per < B ? lo + per : B;
  int64_t sum = 0;
  for (int64_t b = lo; b < hi; ++b) sum += len[b];
  part[tid] = sum;
  __syncthreads();
  if (tid < 64) {   // wave 0: sixteen parts per lane, a shuffle scan across the lanes
    int64_t mine = 0;
    for (int i = 0; i < BE_SCAN_NT / 64; ++i) mine += part[tid * (BE_SCAN_NT / 64) + i];
    int64_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(incl, d, 64);
      if (tid >= d) incl += up;
    }
    int64_t run = incl - mine;
    for (int i = 0; i < BE_SCAN_NT / 64; ++i) {
      first[tid * (BE_SCAN_NT / 64) + i] = run;
      run += part[tid * (BE_SCAN_NT / 64) + i];
    }
    if (tid == 63) first[BE_SCAN_NT] = run;
  }
  __syncthreads();
  const int64_t all = first[BE_SCAN_NT];
  const bool over = all > bound;
  int64_t run = first[tid];
  for (int64_t b = lo; b < hi; ++b) {
    const int32_t n = len[b];
    const int64_t o = over ? 0 : run;
    off[b] = o;
    if (off_out != nullptr) off_out[b] = o;
    if (over) len[b] = 0;
    run += n;
  }
  if (tid == 0) {
    off[B] = total[0] = over ? 0 : all;
    flag[0] = over ? 1 : 0;
    if (off_out != nullptr) off_out[B] = over ? -1 : all;
  }
}

// P: gr_bert_params or gr_bert_bf16_params (the same dimension fields): one envelope for the four entries.
template <typename P>
const char* be_check(const P* p, int64_t B, int S) {
  if (!p) return "null params";
  if (B < 0) return "negative batch size";
  if (p->hidden_size < 32 || p->hidden_size > BE_MAX_H || p->hidden_size % 32)
    return "hidden_size must be a multiple of 32 in [32, 1024]";
  if (p->head_dim != 32 && p->head_dim != 64) return "head_dim must be 32 or 64";
  if (p->num_heads < 1 || p->num_heads * p->head_dim != p->hidden_size)
    return "num_heads * head_dim must equal hidden_size";
  if (p->intermediate_size < 32 || p->intermediate_size > BE_MAX_I || p->intermediate_size % 32)
    return "intermediate_size must be a multiple of 32 in [32, 4096]";
  if (p->num_layers < 1 || p->num_layers > GR_BERT_MAX_LAYERS) return "num_layers must be 1..24";
  if (p->hidden_act != GR_BERT_ACT_GELU) return "hidden_act must be gelu";
  if (p->position_type != GR_BERT_POS_ABSOLUTE) return "position_embedding_type must be absolute";
  if (p->vocab_size < 1) return "vocab_size must be positive";
  if (p->type_vocab_size < 1) return "type_vocab_size must be positive";
  if (p->max_position < 1) return "max_position_embeddings must be positive";
  if (S < 1 || S > BE_MAX_S) return "S must be 1..512 positions";
  if (S > p->max_position) return "S must not exceed max_position_embeddings";
  if (B > BE_MAX_B) return "B must be at most 65536 sequences";
  return nullptr;
}

template <typename P>
using BePrec = std::conditional_t<std::is_same_v<P, gr_bert_bf16_params>, BeB16, BeF32>;   // a parameter struct's format

// The workspace's rows' part, byte offsets, each part rounded up to 16 bytes: the fp32 residual stream x and the
// pre-LN sum t, then what the GEMMs read and write in the format's element: x's bf16 copy (bf16 only: the fp32 GEMMs
// read x itself, so the part is empty), q/k/v, the context, the GELU output.
struct BeLayout {
  size_t x, t, x16, qkv, ctx, ff, total;
};

template <typename T>
BeLayout be_layout(size_t H, size_t I, size_t M) {
  constexpr size_t es = sizeof(typename T::E);
  BeLayout L;
  size_t o = 0;
  L.x = o;   o += align_up(M * H * 4, 16);
  L.t = o;   o += align_up(M * H * 4, 16);
  L.x16 = o; o += std::is_same_v<T, BeB16> ? align_up(M * H * 2, 16) : 0;
  L.qkv = o; o += align_up(M * 3 * H * es, 16);
  L.ctx = o; o += align_up(M * H * es, 16);
  L.ff = o;  o += align_up(M * I * es, 16);
  L.total = o;
  return L;
}

template <typename P>
size_t be_rows_bytes(const P* p, size_t M) {
  return be_layout<BePrec<P>>((size_t)p->hidden_size, (size_t)p->intermediate_size, M).total;
}

// The ragged call's workspace: the rows' part (be_rows_bytes(rows)), then off[B + 1] int64, total int64 + flag int32
// (16 bytes), len[B] int32, each on a 16-byte boundary.
struct BeRagged {
  int64_t rows;              // the caller's bound, at most B * S
  size_t off, total, len;    // byte offsets
  size_t bytes;
};

template <typename P>
BeRagged be_ragged(const P* p, int64_t B, int S, int64_t rows_bound) {
  BeRagged R;
  R.rows = rows_bound < B * S ? (rows_bound > 0 ? rows_bound : 0) : B * S;
  size_t o = be_rows_bytes(p, (size_t)R.rows);
  R.off = o;   o += align_up((size_t)(B + 1) * sizeof(int64_t), 16);
  R.total = o; o += 16;
  R.len = o;   o += align_up((size_t)B * sizeof(int32_t), 16);
  R.bytes = o + 16;
  return R;
}

template <typename P>
size_t be_bytes(const P* p, int64_t B, int S) { return be_rows_bytes(p, (size_t)B * S) + 16; }

// Three tiles, the same bits from each.  A compute unit works through its workgroups at one MFMA rate
// however many are resident, so a launch takes ceil(workgroups / compute units) rounds of one tile's
// work: take the tile with the least rounds x tile area (bert-base at 4096 rows: q/k/v is 2.25 rounds of
// 128 x 128 but exactly 3 of 128 x 96; the 768-wide outputs are 0.75 of 128 x 128 but exactly 1 of
// 128 x 96).  The factors charge the smaller tiles' extra operand traffic per multiply-add.
struct BeTile { int bm, bn; double cost; };
constexpr BeTile BE_TILES[3] = {{128, 128, 1.0}, {64, 128, 1.10}, {128, 96, 1.03}};

int be_pick_tile(int64_t M, int N) {
  const int64_t cus = cu_count();
  int pick = (int)option("bert_tile") - 1;
  if (pick < 0) {
    double best = 0.0;
    for (int t = 0; t < 3; ++t) {
      const int64_t wgs = ((M + BE_TILES[t].bm - 1) / BE_TILES[t].bm) * ((N + BE_TILES[t].bn - 1) / BE_TILES[t].bn);
      const double c = (double)((wgs + cus - 1) / cus) * BE_TILES[t].bm * BE_TILES[t].bn * BE_TILES[t].cost;
      if (pick < 0 || c < best) pick = t, best = c;
    }
  }
  return pick;
}

// y: fp32 with EPI_RESID or from BeF32, bf16 otherwise.
// RAGGED: M is the caller's row bound (it sizes the grid and picks the tile), the row count is rg.total[0].
template <typename T, int EPI, bool RAGGED>
int be_gemm(const char* what, const typename T::E* x, const BeSeg<typename T::E>& sg, int seg_n, const float* residual,
            BeOut<T, EPI>* y, int64_t M, int N, int K, hipStream_t st, const BeRows& rg) {
  const int pick = be_pick_tile(M, N);
  const int tn = (N + BE_TILES[pick].bn - 1) / BE_TILES[pick].bn;
  const dim3 grid((unsigned)(((M + BE_TILES[pick].bm - 1) / BE_TILES[pick].bm) * tn));
  if (pick == 0)
    be_gemm_kernel<T, 2, 2, 2, EPI, RAGGED><<<grid, dim3(BE_NT), 0, st>>>(x, sg, seg_n, residual, y, M, N, K, tn, rg);
  else if (pick == 1)
    be_gemm_kernel<T, 2, 1, 2, EPI, RAGGED><<<grid, dim3(BE_NT), 0, st>>>(x, sg, seg_n, residual, y, M, N, K, tn, rg);
  else
    be_gemm_kernel<T, 4, 1, 3, EPI, RAGGED><<<grid, dim3(BE_NT), 0, st>>>(x, sg, seg_n, residual, y, M, N, K, tn, rg);
  return check_launch(what);
}

template <int HD, bool RAGGED, typename E>
void be_attn(const E* qkv, const int64_t* mask, E* ctx, int64_t B, int S, int NH, hipStream_t st, const BeRows& rg) {
  const int nqt = (S + BE_QT - 1) / BE_QT;
  const dim3 grid((unsigned)(B * NH * nqt));
  if constexpr (std::is_same_v<E, float>)
    be_attn_kernel<HD, RAGGED><<<grid, dim3(256), 0, st>>>(qkv, mask, ctx, S, NH, nqt, sas_scale(HD), rg);
  else
    be_attn_bf16_kernel<HD, RAGGED><<<grid, dim3(256), 0, st>>>(qkv, mask, ctx, S, NH, nqt, sas_scale(HD), rg);
}

// A layer's parameters by role, whichever struct holds them: the six [out, in] matrices in the format's element and
// the ten fp32 vectors, in gr_bert_bf16_params' order.
enum { BE_W_Q, BE_W_K, BE_W_V, BE_W_ATTN_OUT, BE_W_INTER, BE_W_OUT };
enum { BE_B_Q, BE_B_K, BE_B_V, BE_B_ATTN_OUT, BE_LN1_W, BE_LN1_B, BE_B_INTER, BE_B_OUT, BE_LN2_W, BE_LN2_B };
template <typename E>
struct BeLayer {
  const E* w[6];
  const float* v[10];
};

BeLayer<float> be_layer(const gr_bert_params* p, int l) {   // layer[l]: each weight followed by its bias
  const float* const* a = p->layer[l];
  return {{a[0], a[2], a[4], a[6], a[10], a[12]}, {a[1], a[3], a[5], a[7], a[8], a[9], a[11], a[13], a[14], a[15]}};
}

BeLayer<uint16_t> be_layer(const gr_bert_bf16_params* p, int l) {
  BeLayer<uint16_t> y;
  for (int i = 0; i < 6; ++i) y.w[i] = p->matrix[l][i];
  for (int i = 0; i < 10; ++i) y.v[i] = p->vector[l][i];
  return y;
}

template <typename P>
bool be_weights_ok(const P* p) {
  bool ok = p->word && p->position && p->token_type && p->emb_ln_w && p->emb_ln_b;
  for (int l = 0; ok && l < p->num_layers; ++l) {
    const auto y = be_layer(p, l);
    for (int i = 0; i < 6; ++i) ok = ok && y.w[i] && aligned16(y.w[i]);
    for (int i = 0; i < 10; ++i) ok = ok && y.v[i] && aligned16(y.v[i]);
  }
  return ok;
}

// Embeddings + LayerNorm into the workspace's x, then the encoder stack over M rows (RAGGED: M bounds the packed
// rows, rg.total[0] counts them), the last LayerNorm into last (the workspace's x when null); returns through
// *last_out where the last hidden state lies.  2 + 7 num_layers launches with the caller's pooling.  P picks the
// format (the bf16 contract is at the head of this file): with bf16 each LayerNorm also writes the copy the next GEMM
// reads, with fp32 that GEMM reads x itself.
template <bool RAGGED, typename P>
int be_forward(const P* p, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* token_type_ids,
               int64_t B, int S, int64_t M, void* workspace, float* last, const float** last_out, hipStream_t st,
               const BeRows& rg) {
  using T = BePrec<P>;
  using E = typename T::E;
  constexpr bool B16 = std::is_same_v<T, BeB16>;
  const int H = p->hidden_size, I = p->intermediate_size, NH = p->num_heads, HD = p->head_dim;
  const BeLayout L = be_layout<T>((size_t)H, (size_t)I, (size_t)M);
  char* wb = static_cast<char*>(workspace);
  float *X = reinterpret_cast<float*>(wb + L.x), *SUM = reinterpret_cast<float*>(wb + L.t);
  uint16_t* X16 = B16 ? reinterpret_cast<uint16_t*>(wb + L.x16) : nullptr;
  E *QKV = reinterpret_cast<E*>(wb + L.qkv), *CTX = reinterpret_cast<E*>(wb + L.ctx);
  E* FF = reinterpret_cast<E*>(wb + L.ff);
  const E* XA;   // x as the GEMMs read it
  if constexpr (B16) XA = X16;
  else XA = X;
  const dim3 eg = RAGGED ? dim3((unsigned)B, (unsigned)((S + 3) / 4)) : dim3((unsigned)((M + 3) / 4));
  // RAGGED: B x ceil(S / 4) <= 65536 x 128 workgroups
  be_embed_ln_kernel<RAGGED, B16><<<eg, dim3(256), 0, st>>>(
      input_ids, token_type_ids, p->word, p->position, p->token_type, p->emb_ln_w, p->emb_ln_b, p->eps, p->vocab_size,
      p->type_vocab_size, S, H, M, X, X16, rg);
  if (int rc = check_launch("be_embed_ln_kernel")) return rc;
  if (!last) last = X;
  *last_out = last;
  auto ln = [&](const float* w, const float* b, float* out) {   // LayerNorm of SUM: a wave per row
    be_ln_kernel<RAGGED, B16><<<dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st>>>(SUM, w, b, p->eps, H, M, out, X16, rg);
    return check_launch("be_ln_kernel");
  };
  for (int l = 0; l < p->num_layers; ++l) {
    const BeLayer<E> y = be_layer(p, l);
    const BeSeg<E> qkv_w = {{y.w[BE_W_Q], y.w[BE_W_K], y.w[BE_W_V]}, {y.v[BE_B_Q], y.v[BE_B_K], y.v[BE_B_V]}};
    if (int rc = be_gemm<T, BE_EPI_BIAS, RAGGED>("bert q/k/v", XA, qkv_w, H, nullptr, QKV, M, 3 * H, H, st, rg)) return rc;
    if (HD == 64) be_attn<64, RAGGED>(QKV, attention_mask, CTX, B, S, NH, st, rg);
    else be_attn<32, RAGGED>(QKV, attention_mask, CTX, B, S, NH, st, rg);
    if (int rc = check_launch("bert attention")) return rc;
    const BeSeg<E> ao = {{y.w[BE_W_ATTN_OUT], nullptr, nullptr}, {y.v[BE_B_ATTN_OUT], nullptr, nullptr}};
    if (int rc = be_gemm<T, BE_EPI_RESID, RAGGED>("bert attention output + residual", CTX, ao, H, X, SUM, M, H, H, st, rg))
      return rc;
    if (int rc = ln(y.v[BE_LN1_W], y.v[BE_LN1_B], X)) return rc;
    const BeSeg<E> inter = {{y.w[BE_W_INTER], nullptr, nullptr}, {y.v[BE_B_INTER], nullptr, nullptr}};
    if (int rc = be_gemm<T, BE_EPI_GELU, RAGGED>("bert intermediate + gelu", XA, inter, I, nullptr, FF, M, I, H, st, rg))
      return rc;
    const BeSeg<E> outw = {{y.w[BE_W_OUT], nullptr, nullptr}, {y.v[BE_B_OUT], nullptr, nullptr}};
    if (int rc = be_gemm<T, BE_EPI_RESID, RAGGED>("bert output + residual", FF, outw, H, X, SUM, M, H, I, st, rg))
      return rc;
    if (int rc = ln(y.v[BE_LN2_W], y.v[BE_LN2_B], l + 1 == p->num_layers ? last : X)) return rc;
  }
  return GR_OK;
}

// The four entries' body: the checks in gr_bert_embed_f32's order, then the launches.  who: "<entry>: "; ws_query: the
// entry's workspace query, named in the workspace message.  hidden: hidden_out [B, S, H], or RAGGED hidden_rows_out
// [rows_bound, H]; rows_bound and row_offsets_out are the ragged entries' (the padded ones pass 0 and null).
template <bool RAGGED, typename P>
int be_embed(const std::string& who, const char* ws_query, const P* p, const int64_t* input_ids,
             const int64_t* attention_mask, const int64_t* token_type_ids, int64_t B, int32_t S, int64_t rows_bound,
             int32_t pooling, float* pooled_out, float* hidden, int64_t* row_offsets_out, void* workspace,
             size_t workspace_bytes, void* stream) {
  clear_error();
  if (const char* why = be_check(p, B, S)) return fail(!p || B < 0 ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  if (RAGGED && B > 0 && rows_bound < 1) return fail(GR_ERR_ARG, who + "rows_bound must be at least 1");
  if (pooling != GR_BERT_POOL_NONE && pooling != GR_BERT_POOL_MEAN_NO_CLS && pooling != GR_BERT_POOL_CLS)
    return fail(GR_ERR_ARG, who + "pooling must be GR_BERT_POOL_NONE, _MEAN_NO_CLS or _CLS");
  if (B == 0) return GR_OK;
  const BeRagged R = be_ragged(p, B, S, rows_bound);   // read by the ragged entries only
  if (!workspace || workspace_bytes < (RAGGED ? R.bytes : be_bytes(p, B, S)) || !aligned16(workspace))
    return fail(GR_ERR_WORKSPACE, who + "workspace missing, misaligned or smaller than " + ws_query);
  if (!input_ids) return fail(GR_ERR_ARG, who + "input_ids is null");
  if (pooling != GR_BERT_POOL_NONE && !pooled_out) return fail(GR_ERR_ARG, who + "pooled_out is null");
  if (pooling == GR_BERT_POOL_NONE && (!hidden || (RAGGED && !row_offsets_out)))
    return fail(GR_ERR_ARG, who + (RAGGED ? "hidden_rows_out or row_offsets_out" : "hidden_out") +
                                " is null and pooling is GR_BERT_POOL_NONE: nothing to compute");
  if (hidden && !aligned16(hidden))
    return fail(GR_ERR_ARG, who + (RAGGED ? "hidden_rows_out" : "hidden_out") + " must be 16-byte aligned");
  if (!be_weights_ok(p)) return fail(GR_ERR_ARG, who + "a weight pointer is null or not 16-byte aligned");

  const int H = p->hidden_size;
  hipStream_t st = static_cast<hipStream_t>(stream);
  BeRows rg = {nullptr, nullptr, nullptr, nullptr};
  if constexpr (RAGGED) {
    char* wb = static_cast<char*>(workspace);
    int64_t* off = reinterpret_cast<int64_t*>(wb + R.off);
    int64_t* total = reinterpret_cast<int64_t*>(wb + R.total);
    int32_t* flag = reinterpret_cast<int32_t*>(wb + R.total + sizeof(int64_t));
    int32_t* len = reinterpret_cast<int32_t*>(wb + R.len);
    rg = {len, off, total, flag};
    be_len_kernel<<<dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st>>>(attention_mask, B, S, len);
    if (int rc = check_launch("be_len_kernel")) return rc;
    be_offsets_kernel<<<dim3(1), dim3(BE_SCAN_NT), 0, st>>>(len, B, R.rows, off, total, flag, row_offsets_out);
    if (int rc = check_launch("be_offsets_kernel")) return rc;
  }
  const float* last = nullptr;
  if (int rc = be_forward<RAGGED>(p, input_ids, attention_mask, token_type_ids, B, S, RAGGED ? R.rows : B * S, workspace,
                                  hidden, &last, st, rg))
    return rc;
  be_pool_kernel<RAGGED><<<dim3((unsigned)B, (unsigned)((H + 255) / 256)), dim3(256), 0, st>>>(
      last, attention_mask, S, H, pooling, pooled_out, RAGGED ? nullptr : hidden, rg);
  return check_launch("be_pool_kernel");
}

}  // namespace
}  // namespace gr

extern "C" size_t gr_bert_embed_workspace_bytes(const gr_bert_params* p, int64_t B, int32_t S) {
  if (gr::be_check(p, B, S)) return 0;
  return gr::be_bytes(p, B, S);
}

extern "C" int gr_bert_embed_f32(const gr_bert_params* p, const int64_t* input_ids, const int64_t* attention_mask,
                                 const int64_t* token_type_ids, int64_t B, int32_t S, int32_t pooling,
                                 float* pooled_out, float* hidden_out, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return gr::be_embed<false>("gr_bert_embed_f32: ", "gr_bert_embed_workspace_bytes", p, input_ids, attention_mask,
                             token_type_ids, B, S, 0, pooling, pooled_out, hidden_out, nullptr, workspace,
                             workspace_bytes, stream);
}

extern "C" size_t gr_bert_embed_ragged_workspace_bytes(const gr_bert_params* p, int64_t B, int32_t S,
                                                       int64_t rows_bound) {
  if (gr::be_check(p, B, S) || (B > 0 && rows_bound < 1)) return 0;
  return gr::be_ragged(p, B, S, rows_bound).bytes;
}

extern "C" int gr_bert_embed_ragged_f32(const gr_bert_params* p, const int64_t* input_ids,
                                        const int64_t* attention_mask, const int64_t* token_type_ids, int64_t B,
                                        int32_t S, int64_t rows_bound, int32_t pooling, float* pooled_out,
                                        float* hidden_rows_out, int64_t* row_offsets_out, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return gr::be_embed<true>("gr_bert_embed_ragged_f32: ", "gr_bert_embed_ragged_workspace_bytes", p, input_ids,
                            attention_mask, token_type_ids, B, S, rows_bound, pooling, pooled_out, hidden_rows_out,
                            row_offsets_out, workspace, workspace_bytes, stream);
}

extern "C" size_t gr_bert_embed_bf16_workspace_bytes(const gr_bert_bf16_params* p, int64_t B, int32_t S) {
  if (gr::be_check(p, B, S)) return 0;
  return gr::be_bytes(p, B, S);
}

extern "C" int gr_bert_embed_bf16(const gr_bert_bf16_params* p, const int64_t* input_ids,
                                  const int64_t* attention_mask, const int64_t* token_type_ids, int64_t B, int32_t S,
                                  int32_t pooling, float* pooled_out, float* hidden_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return gr::be_embed<false>("gr_bert_embed_bf16: ", "gr_bert_embed_bf16_workspace_bytes", p, input_ids, attention_mask,
                             token_type_ids, B, S, 0, pooling, pooled_out, hidden_out, nullptr, workspace,
                             workspace_bytes, stream);
}

extern "C" size_t gr_bert_embed_ragged_bf16_workspace_bytes(const gr_bert_bf16_params* p, int64_t B, int32_t S,
                                                            int64_t rows_bound) {
  if (gr::be_check(p, B, S) || (B > 0 && rows_bound < 1)) return 0;
  return gr::be_ragged(p, B, S, rows_bound).bytes;
}

extern "C" int gr_bert_embed_ragged_bf16(const gr_bert_bf16_params* p, const int64_t* input_ids,
                                         const int64_t* attention_mask, const int64_t* token_type_ids, int64_t B,
                                         int32_t S, int64_t rows_bound, int32_t pooling, float* pooled_out,
                                         float* hidden_rows_out, int64_t* row_offsets_out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return gr::be_embed<true>("gr_bert_embed_ragged_bf16: ", "gr_bert_embed_ragged_bf16_workspace_bytes", p, input_ids,
                            attention_mask, token_type_ids, B, S, rows_bound, pooling, pooled_out, hidden_rows_out,
                            row_offsets_out, workspace, workspace_bytes, stream);
}

