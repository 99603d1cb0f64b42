// SASRec transformer training on gfx950 for the shapes that do not fit one workgroup per sequence
// (sasrec_train.hip: n, d <= 64, mlp_layer <= 128): d <= 128, n <= 256, mlp_layer <= 256.
//
// The same computation (SASRec/model.py:49-96 in train mode and its backward), the same saved
// activations, dropout masks and g_vec layout (sasrec_train_contract.h, shared with
// sasrec_train.hip), but tiled over all B * n rows instead of held in one workgroup's LDS:
//   - every product is one launch of gemm_kernel: 64 x 64 output tiles on v_mfma_f32_32x32x2_f32,
//     operands staged through LDS from any (row stride, k stride) layout, a two-level batch index
//     (sequence, head) for the attention products, causal tile / k-range skipping, and an epilogue
//     per use (bias, residual, ReLU + dropout, dropout + residual, ReLU' + dropout);
//   - LayerNorm rows, softmax rows (up to 256 keys: four per lane) and their backwards are one
//     wave per row;
//   - weight gradients dW = dG^T A are split-k launches of the same gemm_kernel over S chunks of
//     the B * n rows, bias / LayerNorm / positional sums are column sums over the same chunks: g_vec
//     holds S partial rows in the parameters' order (summed by the host, deterministic);
//   - item-table rows are scattered with fp32 atomics (padding row 0 excluded).
// Activation gradients (dX, dY, a [rows, d] temporary, dQ|dK|dV or dZ, LayerNorm row statistics,
// P' = dropout(P) and dS) live in the caller's workspace.  All global offsets are 64-bit.
#include "sasrec_train_contract.h"

namespace gr {
namespace stt {

constexpr int NMAX = 256, DMAX = 128;   // n, d; mlp_layer <= 256
constexpr SasTrainLimits LIMITS{"gr_sasrec_train_tiled", NMAX, DMAX, 256, true};
constexpr int GT = 256;                 // threads per workgroup: 4 waves, a 2 x 2 grid of 32 x 32 tiles
constexpr int TM = 64, TN = 64, TK = 32, LP = 65;   // tile, k step, LDS pitch of a k row
static_assert(TM == 64 && TN == 64 && GT % TK == 0 && (GT / TK) * (TK * 64 / GT) == 64 &&
                  (GT / 64) * (TK * 64 / GT) == TK && TK % 2 == 0,
              "gemm_kernel's staging map covers a [64][TK] tile exactly");
static_assert(NMAX <= 4 * 64 && DMAX <= 2 * 64, "softmax rows hold four keys per lane, LayerNorm rows two features");
constexpr int MAXPARTS = 32;           // partial rows of g_vec
constexpr int PART_ROWS = 256;          // at least this many rows per part

// ---- the product kernel --------------------------------------------------------------------
// C[z](r, c) = epilogue(sum_k A[z](r, k) B[z](k, c)), r < M, c < N, k in the batch's k range.
// A[z](r, k) = A[zo * sAo + zi * sAi + r * sar + k * sak] with z = zo * zdiv + zi, B and C alike.
enum { E_PLAIN = 0, E_RES = 1, E_FFN1 = 2, E_FFN2 = 3, E_DZ = 4 };

struct Gemm {
  const float* A;
  int64_t sar, sak, sAo, sAi;
  const float* B;
  int64_t sbk, sbc, sBo, sBi;
  float* C;
  int64_t ldc, sCo, sCi;
  int M, N, K, zdiv;
  int trn, tcn;
  int kchunk;       // > 0: split-k, batch z sums k in [z * kchunk, min(K, (z + 1) * kchunk))
  int kmode;        // 1: k < end of the row tile (causal P' V, dS K); 2: k >= start of the row tile
  int skip_upper;   // skip tiles wholly above the diagonal (scores, dP')
  const float* bias;
  float post;
  const float* R;   // E_RES / E_FFN2: the residual; E_DZ: the FFN1 pre-activation (pitch ldc)
  float* C2;        // E_FFN1: dropout(relu(.)) beside the pre-activation
  int site, n;      // dropout site; rows per sequence
  SasDrop dr;
};

template <int EPI>
__global__ __launch_bounds__(GT) void gemm_kernel(const Gemm g) {
  __shared__ float As[TK * LP];
  __shared__ float Bs[TK * LP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i32 = lane & 31, h = lane >> 5;
  const int64_t id = blockIdx.x;
  const int tc = (int)(id % g.tcn);
  const int tr = (int)((id / g.tcn) % g.trn);
  const int64_t z = id / ((int64_t)g.tcn * g.trn);
  if (g.skip_upper && tc * TN > tr * TM + TM - 1) return;
  int kbeg = 0, kend = g.K;
  if (g.kchunk > 0) {
    const int64_t k0 = z * g.kchunk;
    kbeg = (int)(k0 < g.K ? k0 : g.K);
    kend = (int)(k0 + g.kchunk < g.K ? k0 + g.kchunk : g.K);
  }
  if (g.kmode == 1) kend = min(kend, tr * TM + TM);
  if (g.kmode == 2) kbeg = max(kbeg, tr * TM);
  const int64_t zo = z / g.zdiv, zi = z - zo * g.zdiv;
  const float* A = g.A + zo * g.sAo + zi * g.sAi;
  const float* Bm = g.B + zo * g.sBo + zi * g.sBi;
  float* C = g.C + zo * g.sCo + zi * g.sCi;

  // staging: a [64][TK] operand tile is NE elements per thread; consecutive threads walk the
  // operand's unit stride: k (then thread tid holds k = tid % TK of rows tid / TK + (GT / TK) t) or
  // the row / column (row tid % 64 at k = tid / 64 + (GT / 64) t)
  const bool akf = g.sak == 1, bkf = g.sbk == 1;
  constexpr int NE = TK * 64 / GT;
  const int k_kf = tid % TK, r_kf = tid / TK, r_rf = tid & 63, k_rf = tid >> 6;
  float ra[NE], rb[NE];
  auto load = [&](int k0) {
#pragma unroll
    for (int t = 0; t < NE; ++t) {
      const int64_t row = (int64_t)tr * TM + (akf ? r_kf + (GT / TK) * t : r_rf);
      const int k = k0 + (akf ? k_kf : k_rf + (GT / 64) * t);
      ra[t] = (row < g.M && k < kend) ? A[row * g.sar + (int64_t)k * g.sak] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < NE; ++t) {
      const int64_t col = (int64_t)tc * TN + (bkf ? r_kf + (GT / TK) * t : r_rf);
      const int k = k0 + (bkf ? k_kf : k_rf + (GT / 64) * t);
      rb[t] = (col < g.N && k < kend) ? Bm[(int64_t)k * g.sbk + col * g.sbc] : 0.f;
    }
  };
  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  const int wr = wv >> 1, wc = wv & 1;
  if (kbeg < kend) load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += TK) {
#pragma unroll
    for (int t = 0; t < NE; ++t) {
      As[(akf ? k_kf : k_rf + (GT / 64) * t) * LP + (akf ? r_kf + (GT / TK) * t : r_rf)] = ra[t];
      Bs[(bkf ? k_kf : k_rf + (GT / 64) * t) * LP + (bkf ? r_kf + (GT / TK) * t : r_rf)] = rb[t];
    }
    __syncthreads();
    if (k0 + TK < kend) load(k0 + TK);   // in flight during this step's MFMAs
    const float* ap = As + h * LP + wr * 32 + i32;
    const float* bp = Bs + h * LP + wc * 32 + i32;
    const int pairs = (min(TK, kend - k0) + 1) >> 1;
    if (pairs == TK / 2) {
#pragma unroll
      for (int j = 0; j < TK / 2; ++j) acc = mfma32(ap[2 * j * LP], bp[2 * j * LP], acc);
    } else {   // a k tail (a narrow head's whole k range) stops early; the staged tail past kend is zero
      for (int j = 0; j < pairs; ++j) acc = mfma32(ap[2 * j * LP], bp[2 * j * LP], acc);
    }
    __syncthreads();
  }

  const int64_t col = (int64_t)tc * TN + wc * 32 + i32;
  if (col >= g.N) return;
  uint64_t seed = 0;
  if (EPI == E_FFN1 || EPI == E_FFN2 || EPI == E_DZ) seed = sas_seed_of(g.dr);
  const float bias = g.bias ? g.bias[col] : 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int64_t row = (int64_t)tr * TM + wr * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;   // (mfma32_row here moves the register allocation)
    if (row >= g.M) continue;
    const int64_t o = row * g.ldc + col;
    float x = acc[v] + bias;
    if (EPI == E_PLAIN) {
      C[o] = x * g.post;
    } else if (EPI == E_RES) {
      C[o] = g.R[o] + x;
    } else {
      const int64_t b = row / g.n;
      const float kf = sas_keep(g.dr, seed, b, g.site, sas_elem_row(row - b * g.n, col, g.N));
      if (EPI == E_FFN1) {
        C[o] = x;
        g.C2[o] = fmaxf(x, 0.f) * kf;
      } else if (EPI == E_FFN2) {
        C[o] = g.R[o] + x * kf;
      } else {
        C[o] = g.R[o] > 0.f ? x * kf : 0.f;
      }
    }
  }
}

// ---- row kernels: one wave per row ----------------------------------------------------------
// x0 = item_emb[s] + pos_emb[i] (model.py:58-60); an id outside the table is read as row 0
__global__ __launch_bounds__(GT) void embed_kernel(const int64_t* __restrict__ seqs, const float* __restrict__ item,
                                                   const float* __restrict__ pos, int64_t item_rows, int64_t rows,
                                                   int n, int d, float* __restrict__ X, int32_t* err) {
  const int64_t idx = (int64_t)blockIdx.x * GT + threadIdx.x;
  if (idx >= rows * d) return;
  const int64_t row = idx / d;
  const int f = (int)(idx - row * d);
  int64_t s = seqs[row];
  if (s < 0 || s >= item_rows) {
    set_err(err, 1);
    s = 0;
  }
  X[idx] = item[s * d + f] + pos[(row % n) * d + f];
}

// torch's LayerNorm: biased variance, (x - mean) * rsqrt(var + eps) * w + b; d <= 128: two features per lane
__global__ __launch_bounds__(GT) void ln_fwd_kernel(const float* __restrict__ X, float* __restrict__ Y,
                                                    const float* __restrict__ w, const float* __restrict__ bb,
                                                    int64_t rows, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (GT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float inv_d = 1.f / (float)d;
  float x[2], s = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int f = lane + 64 * t;
    x[t] = f < d ? X[row * d + f] : 0.f;
    s += x[t];
  }
  const float mean = wave_sum(s) * inv_d;
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float c = lane + 64 * t < d ? x[t] - mean : 0.f;
    q = fmaf(c, c, q);
  }
  const float rstd = rsqrtf(wave_sum(q) * inv_d + eps);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int f = lane + 64 * t;
    if (f < d) Y[row * d + f] = (x[t] - mean) * rstd * w[f] + bb[f];
  }
}

// LayerNorm backward of one row: DX = (ACC ? DX : 0) + dLN/dx; the row's (mean, rstd) go to stats
// for the dgamma / dbeta column sums; dy_out (optional) = new DX * sas_keep(site, row element): the
// gradient of the FFN output of the block below.
__global__ __launch_bounds__(GT) void ln_bwd_kernel(const float* __restrict__ X, const float* __restrict__ DY,
                                                    float* __restrict__ DX, int acc, const float* __restrict__ w,
                                                    float* __restrict__ stats, float* __restrict__ dy_out, int site,
                                                    int n, int64_t rows, int d, float eps, const SasDrop dr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (GT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float inv_d = 1.f / (float)d;
  float x[2], s = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int f = lane + 64 * t;
    x[t] = f < d ? X[row * d + f] : 0.f;
    s += x[t];
  }
  const float mean = wave_sum(s) * inv_d;
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float c = lane + 64 * t < d ? x[t] - mean : 0.f;
    q = fmaf(c, c, q);
  }
  const float rstd = rsqrtf(wave_sum(q) * inv_d + eps);
  float xh[2], dxh[2], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int f = lane + 64 * t;
    const bool on = f < d;
    xh[t] = on ? (x[t] - mean) * rstd : 0.f;
    dxh[t] = on ? DY[row * d + f] * w[f] : 0.f;
    s1 += dxh[t];
    s2 = fmaf(dxh[t], xh[t], s2);
  }
  s1 = wave_sum(s1) * inv_d;
  s2 = wave_sum(s2) * inv_d;
  if (lane == 0) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
  const uint64_t seed = dy_out ? sas_seed_of(dr) : 0;
  const int64_t b = row / n;
  const int i = (int)(row - b * n);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int f = lane + 64 * t;
    if (f < d) {
      float v = rstd * (dxh[t] - s1 - xh[t] * s2);
      if (acc) v += DX[row * d + f];
      DX[row * d + f] = v;
      if (dy_out) dy_out[row * d + f] = v * sas_keep(dr, seed, b, site, sas_elem_row(i, f, d));
    }
  }
}

// causal softmax of one query row of one (sequence, head): S holds the scaled scores of keys j <= i;
// P (the saved probabilities, zero past i) overwrites them, PK = P * keep
__global__ __launch_bounds__(GT) void softmax_fwd_kernel(float* __restrict__ P, float* __restrict__ PK, int64_t rows,
                                                         int n, int H, int site, const SasDrop dr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (GT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t bh = row / n;
  const int i = (int)(row - bh * n);
  const int64_t b = bh / H;
  const int hh = (int)(bh - b * H);
  const uint64_t seed = sas_seed_of(dr);
  float sv[4], mx = -__builtin_inff();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    sv[t] = j <= i ? P[row * n + j] : -__builtin_inff();
    mx = fmaxf(mx, sv[t]);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    sv[t] = lane + 64 * t <= i ? __expf(sv[t] - mx) : 0.f;
    sum += sv[t];
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    if (j < n) {
      const float pr = sv[t] / sum;
      P[row * n + j] = pr;
      PK[row * n + j] = pr * sas_keep(dr, seed, b, site, sas_elem_prob(hh, n, i, j));
    }
  }
}

// softmax backward of one row: DS holds dP' (keys j <= i); DS = P (dP' keep - sum_j dP' keep P),
// zero past i; PK = P * keep for dV = P'^T dO
__global__ __launch_bounds__(GT) void softmax_bwd_kernel(const float* __restrict__ P, float* __restrict__ DS,
                                                         float* __restrict__ PK, int64_t rows, int n, int H, int site,
                                                         const SasDrop dr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (GT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t bh = row / n;
  const int i = (int)(row - bh * n);
  const int64_t b = bh / H;
  const int hh = (int)(bh - b * H);
  const uint64_t seed = sas_seed_of(dr);
  float pr[4], dp[4], kf[4], sdp = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    const bool on = j <= i;
    kf[t] = on ? sas_keep(dr, seed, b, site, sas_elem_prob(hh, n, i, j)) : 0.f;
    pr[t] = on ? P[row * n + j] : 0.f;
    dp[t] = on ? DS[row * n + j] * kf[t] : 0.f;
    sdp = fmaf(dp[t], pr[t], sdp);
  }
  sdp = wave_sum(sdp);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    if (j < n) {
      DS[row * n + j] = pr[t] * (dp[t] - sdp);
      PK[row * n + j] = pr[t] * kf[t];
    }
  }
}

// dst[z * vw + c] = sum over rows [z * chunk, min(rows, (z + 1) * chunk)) of src[r * ld + c], c < width
// (a bias gradient's partial; the positional rows with a "row" = one sequence).  With X / stats:
// dst = sum dy * xhat (dgamma) and dst2 = sum dy (dbeta) of a LayerNorm.  A workgroup takes CS_C
// columns of one part with CS_R row lanes (a part has few hundred rows and there are at most
// MAXPARTS parts: the row lanes are what fills the chip), summed through LDS in lane order.
constexpr int CS_C = 32, CS_R = 32;
__global__ __launch_bounds__(CS_C * CS_R) void colsum_kernel(const float* __restrict__ src, int64_t ld, int64_t rows,
                                                             int width, int64_t chunk, float* __restrict__ dst,
                                                             float* __restrict__ dst2, int64_t vw,
                                                             const float* __restrict__ X,
                                                             const float* __restrict__ stats) {
  __shared__ float red[2][CS_R][CS_C + 1];
  const int tid = threadIdx.x, cl = tid % CS_C, rl = tid / CS_C;
  const int c = blockIdx.x * CS_C + cl;
  const int64_t z = blockIdx.y;
  const int64_t r0 = z * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  float s = 0.f, sg = 0.f;
  if (c < width) {
#pragma unroll 4
    for (int64_t r = r0 + rl; r < r1; r += CS_R) {
      const float v = src[r * ld + c];
      s += v;
      if (X) sg = fmaf(v, (X[r * ld + c] - stats[2 * r]) * stats[2 * r + 1], sg);
    }
  }
  red[0][rl][cl] = s;
  red[1][rl][cl] = sg;
  __syncthreads();
  if (rl < 2 && c < width) {   // row lane 0 adds up the plain sums, row lane 1 the LayerNorm's dgamma
    if (rl == 1 && !X) return;
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < CS_R; ++q) a += red[rl][q][cl];
    if (X) (rl == 1 ? dst : dst2)[z * vw + c] = a;
    else dst[z * vw + c] = a;
  }
}

// item-table rows by atomics (padding row 0 keeps a zero gradient, nn.Embedding(padding_idx=0))
__global__ __launch_bounds__(GT) void item_scatter_kernel(const int64_t* __restrict__ seqs, const float* __restrict__ DX,
                                                          int64_t item_rows, int64_t rows, int d,
                                                          float* __restrict__ g_item) {
  const int64_t idx = (int64_t)blockIdx.x * GT + threadIdx.x;
  if (idx >= rows * d) return;
  const int64_t row = idx / d;
  const int64_t s = seqs[row];
  if (s > 0 && s < item_rows) atomicAdd(g_item + s * d + (idx - row * d), DX[idx]);
}

// ---- host side ------------------------------------------------------------------------------
static int parts_of(int64_t rows) {
  const int64_t s = (rows + PART_ROWS - 1) / PART_ROWS;
  return (int)(s < 1 ? 1 : s > MAXPARTS ? MAXPARTS : s);
}

struct Ws {   // float offsets into the workspace
  size_t dx, t, y, g1, stats, pk, ds, total;
};
static Ws ws_layout(int64_t B, int n, int d, int H, int m) {
  const size_t R = (size_t)B * n, wide = (size_t)(3 * d > m ? 3 * d : m);
  const size_t pp = (size_t)B * H * n * n;
  Ws w;
  size_t o = 0;
  auto take = [&](size_t count) {
    const size_t at = o;
    o += align_up(count, 64);
    return at;
  };
  w.dx = take(R * d);
  w.t = take(R * d);
  w.y = take(R * d);
  w.g1 = take(R * wide);
  w.stats = take(2 * R);
  w.pk = take(pp);
  w.ds = take(pp);
  w.total = o;
  return w;
}

template <int EPI>
static void run(Gemm g, int64_t batches, hipStream_t st) {
  g.trn = (g.M + TM - 1) / TM;
  g.tcn = (g.N + TN - 1) / TN;
  if (g.zdiv < 1) g.zdiv = 1;
  const int64_t blocks = (int64_t)g.trn * g.tcn * batches;
  hipLaunchKernelGGL(gemm_kernel<EPI>, dim3((unsigned)blocks), dim3(GT), 0, st, g);
}

static Gemm gemm(const float* A, int64_t sar, int64_t sak, const float* B, int64_t sbk, int64_t sbc, float* C,
                 int64_t ldc, int64_t M, int N, int64_t K) {
  Gemm g{};
  g.A = A;
  g.sar = sar;
  g.sak = sak;
  g.B = B;
  g.sbk = sbk;
  g.sbc = sbc;
  g.C = C;
  g.ldc = ldc;
  g.M = (int)M;
  g.N = N;
  g.K = (int)K;
  g.zdiv = 1;
  g.post = 1.f;
  g.n = 1;
  return g;
}

static unsigned row_blocks(int64_t rows) { return (unsigned)((rows + GT / 64 - 1) / (GT / 64)); }

}  // namespace stt
}  // namespace gr

extern "C" size_t gr_sasrec_train_tiled_workspace_bytes(const gr_sasrec_params* p, int64_t B, int32_t n) {
  if (!p || B < 1 || n < 1 || p->d < 1 || p->n_heads < 1 || p->mlp < 1) return 0;
  return sizeof(float) * gr::stt::ws_layout(B, n, p->d, p->n_heads, p->mlp).total;
}

extern "C" int32_t gr_sasrec_train_tiled_parts(const gr_sasrec_params* p, int64_t B, int32_t n) {
  if (!p || B < 1 || n < 1) return 0;
  return gr::stt::parts_of(B * n);
}

extern "C" int gr_sasrec_train_tiled_fwd_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                                             float p_drop, uint64_t seed, const uint64_t* seed_dev,
                                             const gr_sasrec_train_bufs* bufs, float* out, int32_t* err_flag,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gr;
  using namespace gr::stt;
  clear_error();
  const int rc = sas_train_check(LIMITS, p, B, n, p_drop, bufs);
  if (rc) return rc;
  const gr_sasrec_train_bufs& g = *bufs;
  if (!seqs || !out || !workspace || null_acts(g)) return fail(GR_ERR_ARG, "gr_sasrec_train_tiled_fwd_f32: null pointer");
  const int d = p->d, m = p->mlp, H = p->n_heads, hd = d / H, d3 = 3 * d, nb = p->n_blocks;
  const Ws w = ws_layout(B, n, d, H, m);
  if (workspace_bytes < sizeof(float) * w.total)
    return fail(GR_ERR_WORKSPACE, "gr_sasrec_train_tiled_fwd_f32: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t R = B * n, BH = B * H;
  const int64_t nn = (int64_t)n * n;
  float* PK = static_cast<float*>(workspace) + w.pk;
  const SasDrop dr{p_drop, 1.f / (1.f - p_drop), seed, seed_dev};
  const float q_scale = sqrtf(1.f / (float)hd);   // F.multi_head_attention_forward: q * sqrt(1 / E)
  const unsigned eb = (unsigned)((R * d + GT - 1) / GT);

  hipLaunchKernelGGL(embed_kernel, dim3(eb), dim3(GT), 0, st, seqs, p->item_emb, p->pos_emb, p->item_rows, R, n, d,
                     g.xin, err_flag);
  for (int bk = 0; bk < nb; ++bk) {
    const SasOffs bo = sas_offs(bk, 0, B, n, d, m, H);
    float *X = g.xin + bo.rd, *hs = g.hs + bo.rd, *qkv = g.qkv + bo.r3, *prob = g.prob + bo.pp, *os = g.os + bo.rd;
    float *x1 = g.x1 + bo.rd, *fs = g.fs + bo.rd, *zs = g.zs + bo.rm, *us = g.us + bo.rm;
    float* xn = bk + 1 < nb ? g.xin + sas_offs(bk + 1, 0, B, n, d, m, H).rd : g.xl;
    hipLaunchKernelGGL(ln_fwd_kernel, dim3(row_blocks(R)), dim3(GT), 0, st, X, hs, p->attn_ln_w[bk], p->attn_ln_b[bk],
                       R, d, p->eps);                                                  // model.py:80
    Gemm q = gemm(hs, d, 1, p->in_proj_w[bk], 1, d, qkv, d3, R, d3, d);                // q | k | v
    q.bias = p->in_proj_b[bk];
    run<E_PLAIN>(q, 1, st);
    Gemm s = gemm(qkv, d3, 1, qkv + d, 1, d3, prob, n, n, n, hd);                      // (q k^T) * scale
    s.sAo = s.sBo = (int64_t)n * d3;
    s.sAi = s.sBi = hd;
    s.sCo = H * nn;
    s.sCi = nn;
    s.zdiv = H;
    s.post = q_scale;
    s.skip_upper = 1;
    run<E_PLAIN>(s, BH, st);
    hipLaunchKernelGGL(softmax_fwd_kernel, dim3(row_blocks(BH * n)), dim3(GT), 0, st, prob, PK, BH * n, n, H,
                       sas_site_prob(bk), dr);
    Gemm o = gemm(PK, n, 1, qkv + 2 * d, d3, 1, os, d, n, hd, n);                      // O = P' v
    o.sAo = H * nn;
    o.sAi = nn;
    o.sBo = (int64_t)n * d3;
    o.sBi = hd;
    o.sCo = (int64_t)n * d;
    o.sCi = hd;
    o.zdiv = H;
    o.kmode = 1;
    run<E_PLAIN>(o, BH, st);
    Gemm a = gemm(os, d, 1, p->out_proj_w[bk], 1, d, x1, d, R, d, d);                  // x + out_proj (model.py:84)
    a.bias = p->out_proj_b[bk];
    a.R = X;
    run<E_RES>(a, 1, st);
    hipLaunchKernelGGL(ln_fwd_kernel, dim3(row_blocks(R)), dim3(GT), 0, st, x1, fs, p->ffn_ln_w[bk], p->ffn_ln_b[bk],
                       R, d, p->eps);                                                  // model.py:92
    Gemm f1 = gemm(fs, d, 1, p->ffn1_w[bk], 1, d, zs, m, R, m, d);                     // FFN1, dropout(relu)
    f1.bias = p->ffn1_b[bk];
    f1.C2 = us;
    f1.site = sas_site_hidden(bk);
    f1.n = n;
    f1.dr = dr;
    run<E_FFN1>(f1, 1, st);
    Gemm f2 = gemm(us, m, 1, p->ffn2_w[bk], 1, m, xn, d, R, d, m);                     // x + dropout(FFN2) (model.py:94)
    f2.bias = p->ffn2_b[bk];
    f2.R = x1;
    f2.site = sas_site_out(bk);
    f2.n = n;
    f2.dr = dr;
    run<E_FFN2>(f2, 1, st);
  }
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(row_blocks(R)), dim3(GT), 0, st, g.xl, out, p->last_ln_w, p->last_ln_b, R, d,
                     p->eps);                                                          // model.py:96
  return check_launch("gr_sasrec_train_tiled_fwd_f32");
}

extern "C" int gr_sasrec_train_tiled_bwd_f32(const gr_sasrec_params* p, const int64_t* seqs, int64_t B, int32_t n,
                                             float p_drop, uint64_t seed, const uint64_t* seed_dev,
                                             const gr_sasrec_train_bufs* bufs, const float* d_out, float* g_item,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gr;
  using namespace gr::stt;
  clear_error();
  const int rc = sas_train_check(LIMITS, p, B, n, p_drop, bufs);
  if (rc) return rc;
  const gr_sasrec_train_bufs& g = *bufs;
  if (!seqs || !d_out || !workspace || !g.g_vec || null_acts(g))
    return fail(GR_ERR_ARG, "gr_sasrec_train_tiled_bwd_f32: null pointer");
  const int d = p->d, m = p->mlp, H = p->n_heads, hd = d / H, d3 = 3 * d, nb = p->n_blocks;
  const Ws w = ws_layout(B, n, d, H, m);
  if (workspace_bytes < sizeof(float) * w.total)
    return fail(GR_ERR_WORKSPACE, "gr_sasrec_train_tiled_bwd_f32: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t R = B * n, BH = B * H;
  const int64_t nn = (int64_t)n * n;
  float* base = static_cast<float*>(workspace);
  float *DX = base + w.dx, *T = base + w.t, *Y = base + w.y, *G1 = base + w.g1, *stats = base + w.stats;
  float *PK = base + w.pk, *DS = base + w.ds;
  const SasDrop dr{p_drop, 1.f / (1.f - p_drop), seed, seed_dev};
  const float q_scale = sqrtf(1.f / (float)hd);
  const VOff vo = voff(d, m, nb);
  const int S = parts_of(R);
  const int64_t chunk = (R + S - 1) / S;          // rows per part
  const int64_t bchunk = (B + S - 1) / S;         // sequences per part (positional rows)
  const int64_t vw = sas_vec_width(nb, d, m, n);
  float* gv = g.g_vec;
  float* glast = gv + vo.last;

  auto colsum = [&](const float* src, int64_t ld, int width, float* dst) {
    hipLaunchKernelGGL(colsum_kernel, dim3((width + CS_C - 1) / CS_C, S), dim3(CS_C * CS_R), 0, st, src, ld, R, width, chunk, dst,
                       (float*)nullptr, vw, (const float*)nullptr, (const float*)nullptr);
  };
  auto ln_sums = [&](const float* dy, const float* X, float* dgamma, float* dbeta) {
    hipLaunchKernelGGL(colsum_kernel, dim3((d + CS_C - 1) / CS_C, S), dim3(CS_C * CS_R), 0, st, dy, (int64_t)d, R, d, chunk, dgamma,
                       dbeta, vw, X, (const float*)stats);
  };
  // dW[M, N] = G^T A over the rows: G [R, M] (pitch ldg), A [R, N] (pitch lda); S partial rows of g_vec
  auto dweight = [&](const float* G, int64_t ldg, int M, const float* A, int64_t lda, int N, float* dst) {
    Gemm k = gemm(G, 1, ldg, A, lda, 1, dst, N, M, N, R);
    k.kchunk = (int)chunk;
    k.sCo = vw;
    run<E_PLAIN>(k, S, st);
  };

  // last LayerNorm (model.py:96); Y = the gradient of the top block's FFN output
  hipLaunchKernelGGL(ln_bwd_kernel, dim3(row_blocks(R)), dim3(GT), 0, st, (const float*)g.xl, d_out, DX, 0,
                     p->last_ln_w, stats, Y, sas_site_out(nb - 1), n, R, d, p->eps, dr);
  ln_sums(d_out, g.xl, glast, glast + d);
  for (int bk = nb - 1; bk >= 0; --bk) {
    float* gvb = gv + (int64_t)bk * vo.size;
    const SasOffs bo = sas_offs(bk, 0, B, n, d, m, H);
    const float *X = g.xin + bo.rd, *hs = g.hs + bo.rd, *qkv = g.qkv + bo.r3, *prob = g.prob + bo.pp, *os = g.os + bo.rd;
    const float *x1 = g.x1 + bo.rd, *fs = g.fs + bo.rd, *zs = g.zs + bo.rm, *us = g.us + bo.rm;
    // FFN: x2 = x1 + dropout(y), y = u W2^T + b2, u = dropout(relu(z)), z = f W1^T + b1
    colsum(Y, d, d, gvb + vo.b2);
    dweight(Y, d, d, us, m, m, gvb + vo.w2);                                           // dW2 = dY^T u
    Gemm du = gemm(Y, d, 1, p->ffn2_w[bk], m, 1, G1, m, R, m, d);                       // dZ = relu'(z) keep (dY W2)
    du.R = zs;
    du.site = sas_site_hidden(bk);
    du.n = n;
    du.dr = dr;
    run<E_DZ>(du, 1, st);
    colsum(G1, m, m, gvb + vo.b1);
    dweight(G1, m, m, fs, d, d, gvb + vo.w1);                                          // dW1 = dZ^T f
    run<E_PLAIN>(gemm(G1, m, 1, p->ffn1_w[bk], d, 1, T, d, R, d, m), 1, st);           // df = dZ W1
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(row_blocks(R)), dim3(GT), 0, st, x1, (const float*)T, DX, 1,
                       p->ffn_ln_w[bk], stats, (float*)nullptr, 0, n, R, d, p->eps, dr);   // LN_f
    ln_sums(T, x1, gvb + vo.lfw, gvb + vo.lfb);
    // attention output: x1 = x + O W_o^T + b_o
    colsum(DX, d, d, gvb + vo.ob);
    dweight(DX, d, d, os, d, d, gvb + vo.ow);                                          // dW_o = dX^T O
    run<E_PLAIN>(gemm(DX, d, 1, p->out_proj_w[bk], d, 1, T, d, R, d, d), 1, st);       // dO = dX W_o
    Gemm dp = gemm(T, d, 1, qkv + 2 * d, 1, d3, DS, n, n, n, hd);                      // dP' = dO v^T
    dp.sAo = (int64_t)n * d;
    dp.sBo = (int64_t)n * d3;
    dp.sAi = dp.sBi = hd;
    dp.sCo = H * nn;
    dp.sCi = nn;
    dp.zdiv = H;
    dp.skip_upper = 1;
    run<E_PLAIN>(dp, BH, st);
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3(row_blocks(BH * n)), dim3(GT), 0, st, prob, DS, PK, BH * n, n, H,
                       sas_site_prob(bk), dr);
    Gemm dv = gemm(PK, 1, n, T, d, 1, G1 + 2 * d, d3, n, hd, n);                       // dV = P'^T dO
    dv.sAo = H * nn;
    dv.sAi = nn;
    dv.sBo = (int64_t)n * d;
    dv.sBi = hd;
    dv.sCo = (int64_t)n * d3;
    dv.sCi = hd;
    dv.zdiv = H;
    dv.kmode = 2;
    run<E_PLAIN>(dv, BH, st);
    Gemm dq = gemm(DS, n, 1, qkv + d, d3, 1, G1, d3, n, hd, n);                        // dQ = dS k * scale
    dq.sAo = H * nn;
    dq.sAi = nn;
    dq.sBo = dq.sCo = (int64_t)n * d3;
    dq.sBi = dq.sCi = hd;
    dq.zdiv = H;
    dq.kmode = 1;
    dq.post = q_scale;
    run<E_PLAIN>(dq, BH, st);
    Gemm dk = gemm(DS, 1, n, qkv, d3, 1, G1 + d, d3, n, hd, n);                        // dK = dS^T q * scale
    dk.sAo = H * nn;
    dk.sAi = nn;
    dk.sBo = dk.sCo = (int64_t)n * d3;
    dk.sBi = dk.sCi = hd;
    dk.zdiv = H;
    dk.kmode = 2;
    dk.post = q_scale;
    run<E_PLAIN>(dk, BH, st);
    colsum(G1, d3, d3, gvb + vo.inb);
    dweight(G1, d3, d3, hs, d, d, gvb + vo.inw);                                       // dW_in = dQKV^T h
    run<E_PLAIN>(gemm(G1, d3, 1, p->in_proj_w[bk], d, 1, T, d, R, d, d3), 1, st);      // dh = dQKV W_in
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(row_blocks(R)), dim3(GT), 0, st, X, (const float*)T, DX, 1,
                       p->attn_ln_w[bk], stats, bk > 0 ? Y : (float*)nullptr, sas_site_out(bk - 1), n, R, d,
                       p->eps, dr);                                                           // LN_a
    ln_sums(T, X, gvb + vo.law, gvb + vo.lab);
  }
  // x0 = item_emb[s] + pos_emb[i]: positions as partial sums over each part's sequences
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)(((int64_t)n * d + CS_C - 1) / CS_C), S), dim3(CS_C * CS_R), 0, st,
                     (const float*)DX, (int64_t)n * d, B, n * d, bchunk, gv + vo.pos, (float*)nullptr, vw,
                     (const float*)nullptr, (const float*)nullptr);
  if (g_item)
    hipLaunchKernelGGL(item_scatter_kernel, dim3((unsigned)((R * d + GT - 1) / GT)), dim3(GT), 0, st, seqs,
                       (const float*)DX, p->item_rows, R, d, g_item);
  return check_launch("gr_sasrec_train_tiled_bwd_f32");
}
