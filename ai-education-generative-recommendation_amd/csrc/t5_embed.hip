// T5 embedding retriever (T5/model.py:46-65): input_proj, an eval-mode bidirectional T5 encoder stack on
// 768-wide input vectors, masked mean pooling, output_proj, L2 normalisation -- gr_t5_embed_f32.
//
// The model is wide and shallow (d_model 512, d_ff 256, 4 heads of 16, six blocks) over short
// sequences (S <= 32): 11 MB of fp32 weights, too many to re-read per user, so every projection is a
// row-tiled GEMM over all B * S token rows and only the attention step runs per user.
//
//   t5e_gemm_kernel<NORM, RELU>   y = act(A . W^T + bias) (+ residual), A = x or RMSNorm(x).  The norm
//       costs no pass of its own: the norm weight is applied while the A operand is staged, the
//       squares of the same registers are summed on the way (eight threads per row, combined at the
//       end), and the row's 1 / sqrt(mean(x^2) + eps) multiplies the finished sums in the epilogue
//       -- r * sum((w x) W) for HF's sum((w (x r)) W), the same number up to rounding.  A prologue
//       that read the tile's rows first measured 28 us for q/k/v and 38 us for wi at 256 users
//       (profiles/r20/t5_embed_kernels.txt): it re-read half as many bytes again as the GEMM itself
//       and nothing overlapped it.  64 x 64 outputs per 256-thread
//       workgroup, K staged 32 deep through a double-buffered LDS image (linear.hip's idiom: rows
//       padded to 36 floats, one float4 per operand per 8-deep slice).  Each wave owns 32 x 32 outputs
//       as FOUR v_mfma_f32_32x32x2_f32 accumulators, one per 8-deep slice of the 32-deep stage: four
//       independent chains (the f32 MFMA's issue rate from one wave) of a quarter of K each, added as
//       (a0 + a1) + (a2 + a3) -- a shorter chain rounds less than one chain over all of K.
//   t5e_attn_o_kernel   one workgroup per user: wave w runs heads w, w + 4, ... with everything in
//       registers: the transposed scores k q^T as one MFMA chain (a lane holds sixteen keys of one
//       query, its partner lane the other sixteen), relative bias and key mask, fp32 softmax inside
//       the lane pair, P . v as a second chain whose A operand is the probability registers as they
//       stand, into the user's [S, inner] tile in LDS; then the o projection of that tile on the
//       MFMA (o's rows straight from L2) and the residual add into x.
//   t5e_pool_kernel     final RMSNorm, masked mean over the live rows (a wave per row, waves combined
//       in a fixed order), optional hidden_out.
//   t5e_normalize_kernel  pred / max(|pred|, 1e-8).
//
// Every output element has one summation order that depends on neither B nor the row's tile position,
// and nothing uses atomics, so a call is bitwise repeatable and batch-invariant.
//
// The packed entry (gr_t5_embed_project_f32 once per table, gr_t5_embed_rows_f32 per batch) runs the same
// kernels on the live rows only, one user after the other: the first GEMM's output is a table
// (t5e_gemm<false, false> over the R table rows), x is gathered from it by t5e_gather_kernel, the GEMMs take
// M = rows, and the <ROWS = true> instantiations of the attention and pooling kernels find a user's rows
// and length through offsets[b], offsets[b + 1] (t5e_user_rows, which also bounds them).  A masked key weighs
// exactly 0 in the dense call and a dead row is never pooled, so the packed call returns the dense call's
// bits.  t5e_normalize_rows_kernel writes NaN for a user whose offsets or tokens were out of range.
#include "gr_common.h"

namespace gr {
namespace {

constexpr int TE_MAX_S = 32, TE_MAX_INNER = 256;
constexpr int64_t TE_MAX_USERS = 1ll << 20, TE_MAX_TABLE = 1ll << 24;
constexpr int TE_BM = 64, TE_BN = 64, TE_BK = 32, TE_PITCH = TE_BK + 4, TE_NT = 256;
constexpr float TE_MASKED = -3.4028234663852886e38f;   // finfo(float32).min: what HF adds for a masked key

template <bool NORM, bool RELU>
__global__ __launch_bounds__(TE_NT, 2) void t5e_gemm_kernel(
    const float* __restrict__ x, const float* __restrict__ lnw, float eps, const float* __restrict__ w0,
    const float* __restrict__ w1, const float* __restrict__ w2, int seg_n, const float* __restrict__ bias,
    const float* residual, float* y, int64_t M, int N, int K, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float lds[2][(TE_BM + TE_BN) * TE_PITCH];
  __shared__ float rs[TE_BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int tni = blockIdx.x % tiles_n;
  const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * TE_BM;
  const int n0 = tni * TE_BN;

  constexpr int AV = TE_BM * TE_BK / 4 / TE_NT, BV = TE_BN * TE_BK / 4 / TE_NT;
  f32x4 ra[AV], rl[AV], rb[BV];
  // NORM: the squares of every x element this thread stages, per row slot; eight threads share a row
  f32x4 sq[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) sq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < AV; ++i) {
      const int f = tid + TE_NT * i, row = f >> 3, kk = k0 + (f & 7) * 4;
      const int64_t g = m0 + row;
      const bool ok = g < M && kk < K;
      ra[i] = ok ? *reinterpret_cast<const f32x4*>(x + g * K + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (NORM) rl[i] = ok ? *reinterpret_cast<const f32x4*>(lnw + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < BV; ++i) {
      const int f = tid + TE_NT * i, row = f >> 3, kk = k0 + (f & 7) * 4;
      const int gn = n0 + row;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (gn < N && kk < K) {
        const int seg = gn / seg_n, wr = gn - seg * seg_n;
        const float* wp = seg == 0 ? w0 : seg == 1 ? w1 : w2;
        v = *reinterpret_cast<const f32x4*>(wp + (int64_t)wr * K + kk);
      }
      rb[i] = v;
    }
  };
  auto swrite = [&](int buf) {
    float* s = lds[buf];
#pragma unroll
    for (int i = 0; i < AV; ++i) {
      const int f = tid + TE_NT * i, row = f >> 3;
      f32x4 v = ra[i];
      if constexpr (NORM) {   // the norm weight now, the row's rsqrt(mean(x^2) + eps) on the finished sums
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          sq[i][c] = fmaf(v[c], v[c], sq[i][c]);
          v[c] = rl[i][c] * v[c];
        }
      }
      *reinterpret_cast<f32x4*>(s + row * TE_PITCH + (f & 7) * 4) = v;
    }
#pragma unroll
    for (int i = 0; i < BV; ++i) {
      const int f = tid + TE_NT * i;
      *reinterpret_cast<f32x4*>(s + (TE_BM + (f >> 3)) * TE_PITCH + (f & 7) * 4) = rb[i];
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[a][v] = 0.f;

  const int nk = (K + TE_BK - 1) / TE_BK;
  gload(0);
  swrite(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * TE_BK);
    const float* As = lds[cur] + (wm * 32 + r) * TE_PITCH + 4 * h;
    const float* Bs = lds[cur] + (TE_BM + wn * 32 + r) * TE_PITCH + 4 * h;
#pragma unroll
    for (int kc = 0; kc < TE_BK / 8; ++kc) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(As + kc * 8);
      const f32x4 b = *reinterpret_cast<const f32x4*>(Bs + kc * 8);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[kc] = mfma32(a[s], b[s], acc[kc]);
    }
    if (kt + 1 < nk) swrite(cur ^ 1);
    __syncthreads();
  }

  if constexpr (NORM) {
#pragma unroll
    for (int i = 0; i < AV; ++i) {
      float t = (sq[i][0] + sq[i][1]) + (sq[i][2] + sq[i][3]);
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      t += __shfl_xor(t, 4, 64);
      if ((tid & 7) == 0) rs[(tid + TE_NT * i) >> 3] = 1.0f / sqrtf(t / (float)K + eps);
    }
    __syncthreads();
  }

  const int col = n0 + wn * 32 + r;
  if (col < N) {
    const float bv = bias != nullptr ? bias[col] : 0.f;
    float rv[16];
    if (residual != nullptr) {   // may alias y element for element: all loads first, then the stores
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t row = m0 + wm * 32 + mfma32_row(v, h);
        rv[v] = row < M ? residual[row * N + col] : 0.f;
      }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t row = m0 + wm * 32 + mfma32_row(v, h);
      if (row < M) {
        float o = (acc[0][v] + acc[1][v]) + (acc[2][v] + acc[3][v]);
        if constexpr (NORM) o = o * rs[wm * 32 + mfma32_row(v, h)];
        if (bias != nullptr) o = o + bv;
        if (RELU) o = (o < 0.f) ? 0.f : o;
        if (residual != nullptr) o = rv[v] + o;
        y[row * N + col] = o;
      }
    }
  }
}

// The packed layout's user b: rows [row0, row0 + len) of the call's `rows`, from offsets[b], offsets[b + 1].
// Whatever the two hold, row0 and len come back inside [0, rows) and 1..TE_MAX_S; -> false when they had to be
// bounded (such a user reads the bounded range, stores into no row, and its pred row becomes NaN).
__device__ __forceinline__ bool t5e_user_rows(const int64_t* __restrict__ offsets, int64_t b, int64_t rows,
                                              int64_t& row0, int& len) {
  const int64_t s = offsets[b], e = offsets[b + 1];
  const bool ok = s >= 0 && s < rows && e > s && e <= rows && e - s <= TE_MAX_S;
  row0 = s < 0 ? 0 : s >= rows ? rows - 1 : s;
  const int64_t n = (e < 0 ? 0 : e > rows ? rows : e) - row0;
  len = n < 1 ? 1 : n > TE_MAX_S ? TE_MAX_S : (int)n;
  return ok;
}

// ROWS: the packed layout -- `mask` is offsets [B + 1], `S` arrives as the call's row count and becomes the
// user's own length, every one of its rows is live
template <bool ROWS>
__global__ __launch_bounds__(256) void t5e_attn_o_kernel(const float* __restrict__ qkv,
                                                         const int64_t* __restrict__ mask,
                                                         const float* __restrict__ rel,
                                                         const int32_t* __restrict__ bucket,
                                                         const float* __restrict__ ow, float* x, int S, int H,
                                                         int dkv, int D) {
  __shared__ __attribute__((aligned(16))) float AO[32 * (TE_MAX_INNER + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int inner = H * dkv, ap = inner + 4, ld = 3 * inner;
  const int64_t b = blockIdx.x;
  int64_t row0 = b * S;
  bool store = true;
  if constexpr (ROWS) store = t5e_user_rows(mask, b, /*rows=*/S, row0, /*len=*/S);
  const float* base = qkv + row0 * ld;
  // bit j: position j is a key (lanes 0..31 look at one position each)
  const bool mine = r < S && (ROWS || mask == nullptr || mask[row0 + r] != 0);
  const uint32_t livebits = (uint32_t)__ballot(mine);
  const int rc = r < S ? r : S - 1;   // rows past S read row S - 1: finite, weighted 0 as keys, never stored as queries
  const int nkc = dkv / 8;
  for (int hd = wave; hd < H; hd += 4) {
    // scores, transposed: A rows are keys, B columns are queries, so D register v of lane (r, h) is
    // key mfma32_row(v, h) against query r and a query's softmax stays inside its two lanes
    const float* qrow = base + rc * ld + hd * dkv + 4 * h;
    f32x16 sc;
#pragma unroll
    for (int v = 0; v < 16; ++v) sc[v] = 0.f;
    for (int kc = 0; kc < nkc; ++kc) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(qrow + inner + 8 * kc);
      const f32x4 qf = *reinterpret_cast<const f32x4*>(qrow + 8 * kc);
#pragma unroll
      for (int s = 0; s < 4; ++s) sc = mfma32(kf[s], qf[s], sc);
    }
    float m = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int j = mfma32_row(v, h);
      float a = sc[v] + rel[bucket[j - r + 127] * H + hd];
      if (!((livebits >> j) & 1u)) a = j < S ? TE_MASKED : -INFINITY;
      sc[v] = a;
      m = fmaxf(m, a);
    }
    m = xmax<32>(m);          // the other sixteen keys of this query
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      sc[v] = expf(sc[v] - m);
      sum += sc[v];
    }
    sum = xsum<32>(sum);
#pragma unroll
    for (int v = 0; v < 16; ++v) sc[v] = sc[v] / sum;
    // P . v: step s of the MFMA takes key mfma32_row(s, h) from lane half h, which is register s of the
    // probabilities this lane already holds; B is v[key][feature r] of the head
    for (int d0 = 0; d0 < dkv; d0 += 32) {
      const bool dok = d0 + r < dkv;
      const float* vcol = base + 2 * inner + hd * dkv + d0 + r;
      float vv[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int j = mfma32_row(s, h);
        vv[s] = dok ? vcol[(j < S ? j : S - 1) * ld] : 0.f;
      }
      f32x16 o;
#pragma unroll
      for (int v = 0; v < 16; ++v) o[v] = 0.f;
#pragma unroll
      for (int s = 0; s < 16; ++s) o = mfma32(sc[s], vv[s], o);
      if (dok) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int i = mfma32_row(v, h);
          if (i < S) AO[i * ap + hd * dkv + d0 + r] = o[v];
        }
      }
    }
  }
  __syncthreads();
  // x[b] += AO . o^T: 32-column tiles of d_model over the waves, rows past S read row S - 1 (never stored)
  const float* arow = AO + rc * ap + 4 * h;
  const int nko = inner / 8;
  for (int t = wave; t < D / 32; t += 4) {
    const int col = 32 * t + r;
    const float* wrow = ow + (int64_t)col * inner + 4 * h;
    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[a][v] = 0.f;
    for (int k0 = 0; k0 < nko; k0 += 4) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (k0 + c < nko) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 8 * (k0 + c));
          const f32x4 w = *reinterpret_cast<const f32x4*>(wrow + 8 * (k0 + c));
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[c] = mfma32(a[s], w[s], acc[c]);
        }
      }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = mfma32_row(v, h);
      if (row < S && store) {
        float* px = x + (row0 + row) * D + col;
        *px = *px + ((acc[0][v] + acc[1][v]) + (acc[2][v] + acc[3][v]));
      }
    }
  }
}

// ROWS: as in t5e_attn_o_kernel; hidden_out is then [rows, D]
template <bool ROWS>
__global__ __launch_bounds__(256) void t5e_pool_kernel(const float* __restrict__ x, const int64_t* __restrict__ mask,
                                                       const float* __restrict__ lnw, float eps, int S, int D,
                                                       float* __restrict__ pooled, float* __restrict__ hidden_out) {
  __shared__ float ps[4][512];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  int64_t row0 = 0;
  bool store = true;
  if constexpr (ROWS) store = t5e_user_rows(mask, b, /*rows=*/S, row0, /*len=*/S);
  const auto at = [&](int i) {   // position i of user b as a row of x
    if constexpr (ROWS) return row0 + i;
    else return b * S + i;
  };
  float part[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) part[t] = 0.f;
  for (int i = wave; i < S; i += 4) {
    const float* row = x + at(i) * D;
    float xv[8], ss = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int c = lane + 64 * t;
      xv[t] = c < D ? row[c] : 0.f;
      ss = fmaf(xv[t], xv[t], ss);
    }
    ss = wave_sum(ss);
    const float ri = 1.0f / sqrtf(ss / (float)D + eps);
    const bool lv = ROWS || mask == nullptr || mask[at(i)] != 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int c = lane + 64 * t;
      if (c < D) {
        const float hv = lnw[c] * (xv[t] * ri);
        if (hidden_out != nullptr && store) hidden_out[at(i) * D + c] = hv;
        if (lv) part[t] += hv;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) ps[wave][lane + 64 * t] = part[t];
  __syncthreads();
  int cnt = 0;
  for (int i = 0; i < S; ++i) cnt += (ROWS || mask == nullptr || mask[at(i)] != 0) ? 1 : 0;
  const float den = fmaxf((float)cnt, 1e-9f);
  for (int c = tid; c < D; c += 256) pooled[b * D + c] = ((ps[0][c] + ps[1][c]) + (ps[2][c] + ps[3][c])) / den;
}

// one wave per user
__global__ __launch_bounds__(256) void t5e_normalize_kernel(const float* __restrict__ pred, float* __restrict__ out,
                                                            int64_t B, int N) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* p = pred + b * N;
  float ss = 0.f;
  for (int c = lane; c < N; c += 64) ss = fmaf(p[c], p[c], ss);
  ss = wave_sum(ss);
  const float den = fmaxf(sqrtf(ss), 1e-8f);
  for (int c = lane; c < N; c += 64) out[b * N + c] = p[c] / den;
}

// x[row] = projected[tokens[row]], one float4 per thread; a token outside [0, R) reads the nearest table row
// (t5e_normalize_rows_kernel turns that user's result into NaN)
__global__ __launch_bounds__(256) void t5e_gather_kernel(const float* __restrict__ projected, int64_t R,
                                                         const int64_t* __restrict__ tokens, int64_t rows, int D,
                                                         float* __restrict__ x) {
  const int dv = D / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * dv) return;
  const int64_t row = i / dv;
  const int c = (int)(i - row * dv) * 4;
  int64_t t = tokens[row];
  t = t < 0 ? 0 : t >= R ? R - 1 : t;
  *reinterpret_cast<f32x4*>(x + row * D + c) = *reinterpret_cast<const f32x4*>(projected + t * D + c);
}

// t5e_normalize_kernel on the packed layout, one wave per user: the same arithmetic, and NaN in every
// element for a user whose offsets t5e_user_rows had to bound or one of whose tokens is outside [0, R)
__global__ __launch_bounds__(256) void t5e_normalize_rows_kernel(const float* __restrict__ pred, float* __restrict__ out,
                                                                 int64_t B, int N, const int64_t* __restrict__ tokens,
                                                                 const int64_t* __restrict__ offsets, int64_t rows,
                                                                 int64_t R) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  int64_t row0;
  int len;
  const bool ok = t5e_user_rows(offsets, b, rows, row0, len);
  const int64_t t = lane < len ? tokens[row0 + lane] : 0;
  const bool bad = !ok || __any(t < 0 || t >= R);
  const float* p = pred + b * N;
  float ss = 0.f;
  for (int c = lane; c < N; c += 64) ss = fmaf(p[c], p[c], ss);
  ss = wave_sum(ss);
  const float den = fmaxf(sqrtf(ss), 1e-8f);
  for (int c = lane; c < N; c += 64) out[b * N + c] = bad ? __builtin_nanf("") : p[c] / den;
}

const char* t5e_check(const gr_t5_embed_params* p, int64_t B, int S) {
  if (!p) return "null params";
  if (B < 0) return "negative batch size";
  if (p->d_model < 32 || p->d_model > 512 || p->d_model % 32) return "d_model must be a multiple of 32 in [32, 512]";
  if (p->d_kv != 8 && p->d_kv != 16 && p->d_kv != 32 && p->d_kv != 64) return "d_kv must be 8, 16, 32 or 64";
  if (p->n_heads < 1 || p->n_heads * p->d_kv > 256) return "n_heads * d_kv must be at most 256";
  if (p->d_ff < 32 || p->d_ff > 1024 || p->d_ff % 32) return "d_ff must be a multiple of 32 in [32, 1024]";
  if (p->in_dim < 4 || p->in_dim > 1024 || p->in_dim % 4) return "in_dim must be a multiple of 4 in [4, 1024]";
  if (p->out_dim < 4 || p->out_dim > 1024 || p->out_dim % 4) return "out_dim must be a multiple of 4 in [4, 1024]";
  if (p->n_layers < 1 || p->n_layers > GR_T5E_MAX_LAYERS) return "n_layers must be 1..8";
  if (p->n_buckets != 32) return "n_buckets must be 32";
  if (S < 1 || S > TE_MAX_S) return "S must be 1..32 positions";
  if (B > TE_MAX_USERS) return "B must be at most 2^20 users";
  return nullptr;
}

struct T5eLayout {   // float offsets into the workspace
  size_t x, qkv, ff, pooled, pred, total;
};

// M token rows (B * S dense, the live rows packed) of B users
T5eLayout t5e_layout(const gr_t5_embed_params* p, int64_t B, int64_t rows) {
  const size_t M = (size_t)rows;
  T5eLayout L;
  size_t o = 0;
  L.x = o;      o += align_up(M * p->d_model, 4);
  L.qkv = o;    o += align_up(M * 3 * p->n_heads * p->d_kv, 4);
  L.ff = o;     o += align_up(M * p->d_ff, 4);
  L.pooled = o; o += align_up((size_t)B * p->d_model, 4);
  L.pred = o;   o += align_up((size_t)B * p->out_dim, 4);
  L.total = o;
  return L;
}

size_t t5e_bytes(const gr_t5_embed_params* p, int64_t B, int64_t rows) {
  return t5e_layout(p, B, rows).total * sizeof(float) + 16;
}

// the packed entry's shape: the widths and B through t5e_check, then B <= rows <= 32 B
const char* t5e_rows_check(const gr_t5_embed_params* p, int64_t B, int64_t rows) {
  if (const char* why = t5e_check(p, B, 1)) return why;
  if (rows < B || rows > TE_MAX_S * B) return "rows must be B..32 B (1..32 rows per user)";
  return nullptr;
}

bool t5e_weights_ok(const gr_t5_embed_params* p) {
  bool ok = p->in_w && p->in_b && p->out_w && p->out_b && p->rel && p->bucket && p->final_ln && aligned16(p->in_w) &&
            aligned16(p->out_w) && aligned16(p->final_ln);
  for (int l = 0; ok && l < p->n_layers; ++l)
    for (int i = 0; i < 8; ++i) ok = ok && p->layer[l][i] && aligned16(p->layer[l][i]);
  return ok;
}

template <bool NORM, bool RELU>
int t5e_gemm(const char* what, const float* x, const float* lnw, float eps, const float* w0, const float* w1,
             const float* w2, int seg_n, const float* bias, const float* residual, float* y, int64_t M, int N, int K,
             hipStream_t st) {
  const int64_t tm = (M + TE_BM - 1) / TE_BM;
  const int tn = (N + TE_BN - 1) / TE_BN;
  t5e_gemm_kernel<NORM, RELU><<<dim3((unsigned)(tm * tn)), dim3(TE_NT), 0, st>>>(x, lnw, eps, w0, w1, w2, seg_n, bias,
                                                                              residual, y, M, N, K, tn);
  return check_launch(what);
}

struct T5eBuffers {
  float *X, *QKV, *FF, *pooled, *pred;
  T5eBuffers(void* workspace, const T5eLayout& L) {
    float* ws = static_cast<float*>(workspace);
    X = ws + L.x, QKV = ws + L.qkv, FF = ws + L.ff, pooled = ws + L.pooled, pred = ws + L.pred;
  }
};

// Everything between x's first value and the normalisation: the blocks, the pooling, output_proj.  Dense: users =
// the mask (or null), S the positions; ROWS: users = offsets, S the call's row count (M either way the GEMMs' rows).
template <bool ROWS>
int t5e_encode(const gr_t5_embed_params* p, const int64_t* users, int64_t B, int S, int64_t M, const T5eBuffers& buf,
               float* hidden_out, hipStream_t st) {
  const int D = p->d_model, inner = p->n_heads * p->d_kv, F = p->d_ff;
  float *X = buf.X, *QKV = buf.QKV, *FF = buf.FF;
  for (int l = 0; l < p->n_layers; ++l) {
    const float* const* w = p->layer[l];
    if (int rc = t5e_gemm<true, false>("t5e norm + qkv", X, w[0], p->eps, w[1], w[2], w[3], inner, nullptr, nullptr, QKV,
                                       M, 3 * inner, D, st))
      return rc;
    t5e_attn_o_kernel<ROWS><<<dim3((unsigned)B), dim3(256), 0, st>>>(QKV, users, p->rel, p->bucket, w[4], X, S,
                                                                     p->n_heads, p->d_kv, D);
    if (int rc = check_launch("t5e_attn_o_kernel")) return rc;
    if (int rc = t5e_gemm<true, true>("t5e norm + wi + relu", X, w[5], p->eps, w[6], nullptr, nullptr, F, nullptr, nullptr,
                                      FF, M, F, D, st))
      return rc;
    if (int rc = t5e_gemm<false, false>("t5e wo + residual", FF, nullptr, 0.f, w[7], nullptr, nullptr, D, nullptr, X, X, M,
                                        D, F, st))
      return rc;
  }
  t5e_pool_kernel<ROWS><<<dim3((unsigned)B), dim3(256), 0, st>>>(X, users, p->final_ln, p->eps, S, D, buf.pooled, hidden_out);
  if (int rc = check_launch("t5e_pool_kernel")) return rc;
  return t5e_gemm<false, false>("t5e output_proj", buf.pooled, nullptr, 0.f, p->out_w, nullptr, nullptr, p->out_dim,
                                p->out_b, nullptr, buf.pred, B, p->out_dim, D, st);
}

}  // namespace
}  // namespace gr

extern "C" size_t gr_t5_embed_workspace_bytes(const gr_t5_embed_params* p, int64_t B, int32_t S) {
  if (gr::t5e_check(p, B, S)) return 0;
  return gr::t5e_bytes(p, B, B * S);
}

extern "C" int gr_t5_embed_f32(const gr_t5_embed_params* p, const float* seq_embs, const int64_t* attention_mask,
                               int64_t B, int32_t S, float* pred_out, float* hidden_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
  using namespace gr;
  clear_error();
  const std::string who = "gr_t5_embed_f32: ";
  if (const char* why = t5e_check(p, B, S)) return fail(!p || B < 0 ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  if (B == 0) return GR_OK;
  const int64_t M = B * S;
  if (!workspace || workspace_bytes < t5e_bytes(p, B, M) || !aligned16(workspace))
    return fail(GR_ERR_WORKSPACE, who + "workspace missing, misaligned or smaller than gr_t5_embed_workspace_bytes");
  if (!seq_embs || !pred_out) return fail(GR_ERR_ARG, who + "null pointer");
  if (!aligned16(seq_embs)) return fail(GR_ERR_ARG, who + "seq_embs must be 16-byte aligned");
  if (!t5e_weights_ok(p)) return fail(GR_ERR_ARG, who + "a weight pointer is null or not 16-byte aligned");

  const T5eBuffers w(workspace, t5e_layout(p, B, M));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = t5e_gemm<false, false>("t5e input_proj", seq_embs, nullptr, 0.f, p->in_w, nullptr, nullptr, p->d_model,
                                      p->in_b, nullptr, w.X, M, p->d_model, p->in_dim, st))
    return rc;
  if (int rc = t5e_encode<false>(p, attention_mask, B, S, M, w, hidden_out, st)) return rc;
  t5e_normalize_kernel<<<dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st>>>(w.pred, pred_out, B, p->out_dim);
  return check_launch("t5e_normalize_kernel");
}

extern "C" int gr_t5_embed_project_f32(const gr_t5_embed_params* p, const float* table, int64_t R, float* projected,
                                       void* stream) {
  using namespace gr;
  clear_error();
  const std::string who = "gr_t5_embed_project_f32: ";
  if (const char* why = t5e_check(p, 0, 1)) return fail(!p ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  if (R < 1) return fail(GR_ERR_ARG, who + "R must be at least 1 table row");
  if (R > TE_MAX_TABLE) return fail(GR_ERR_UNSUPPORTED, who + "R must be at most 2^24 table rows");
  if (!table || !projected) return fail(GR_ERR_ARG, who + "null pointer");
  if (!aligned16(table) || !aligned16(projected)) return fail(GR_ERR_ARG, who + "table and projected must be 16-byte aligned");
  if (!p->in_w || !p->in_b || !aligned16(p->in_w))
    return fail(GR_ERR_ARG, who + "a weight pointer is null or not 16-byte aligned");
  return t5e_gemm<false, false>("t5e input_proj", table, nullptr, 0.f, p->in_w, nullptr, nullptr, p->d_model, p->in_b,
                                nullptr, projected, R, p->d_model, p->in_dim, static_cast<hipStream_t>(stream));
}

extern "C" size_t gr_t5_embed_rows_workspace_bytes(const gr_t5_embed_params* p, int64_t B, int64_t rows) {
  if (gr::t5e_rows_check(p, B, rows)) return 0;
  return gr::t5e_bytes(p, B, rows);
}

extern "C" int gr_t5_embed_rows_f32(const gr_t5_embed_params* p, const float* projected, int64_t R,
                                    const int64_t* tokens, const int64_t* offsets, int64_t B, int64_t rows,
                                    float* pred_out, float* hidden_out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  using namespace gr;
  clear_error();
  const std::string who = "gr_t5_embed_rows_f32: ";
  if (const char* why = t5e_rows_check(p, B, rows)) return fail(!p || B < 0 ? GR_ERR_ARG : GR_ERR_UNSUPPORTED, who + why);
  if (R < 1) return fail(GR_ERR_ARG, who + "R must be at least 1 table row");
  if (R > TE_MAX_TABLE) return fail(GR_ERR_UNSUPPORTED, who + "R must be at most 2^24 table rows");
  if (B == 0) return GR_OK;
  if (!workspace || workspace_bytes < t5e_bytes(p, B, rows) || !aligned16(workspace))
    return fail(GR_ERR_WORKSPACE, who + "workspace missing, misaligned or smaller than gr_t5_embed_rows_workspace_bytes");
  if (!projected || !tokens || !offsets || !pred_out) return fail(GR_ERR_ARG, who + "null pointer");
  if (!aligned16(projected)) return fail(GR_ERR_ARG, who + "projected must be 16-byte aligned");
  if (!t5e_weights_ok(p)) return fail(GR_ERR_ARG, who + "a weight pointer is null or not 16-byte aligned");

  const T5eBuffers w(workspace, t5e_layout(p, B, rows));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t vecs = rows * (p->d_model / 4);
  t5e_gather_kernel<<<dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st>>>(projected, R, tokens, rows, p->d_model, w.X);
  if (int rc = check_launch("t5e_gather_kernel")) return rc;
  if (int rc = t5e_encode<true>(p, offsets, B, (int)rows, rows, w, hidden_out, st)) return rc;
  t5e_normalize_rows_kernel<<<dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st>>>(w.pred, pred_out, B, p->out_dim, tokens,
                                                                                 offsets, rows, R);
  return check_launch("t5e_normalize_rows_kernel");
}

