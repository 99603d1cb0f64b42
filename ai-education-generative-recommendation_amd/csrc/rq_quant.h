// Device helpers shared by the RQ quantize kernels (rq.hip) and the fused encode kernel's quantize
// phase (rq_fused.hip): the de-interleaved, XOR-swizzled LDS codebook image, ||r||^2 in ATen's
// order, and the first-minimum merge.  See rq.hip's header for the arithmetic contract.
#pragma once
#include "gr_common.h"

namespace gr {

// Float offset of 16-byte slot q of row c of an LDS codebook image with EP/4 slots per row.
template <int EP>
__device__ __forceinline__ int cb_off(int c, int q) {
  constexpr int S = EP / 4;
  constexpr int M = S >= 8 ? 7 : S - 1;
  return c * EP + 4 * (q ^ (c & M));
}

// LDS float offset of feature f of row c: lane half f & 1, float4 f >> 3, element (f >> 1) & 3.
template <int EP>
__device__ __forceinline__ int feat_off(int c, int f) {
  return cb_off<EP>(c, (f & 1) * (EP / 8) + (f >> 3)) + ((f >> 1) & 3);
}

// ||r||^2 of this lane's item in ATen's order (aten_rowsq) with the features split over the lane
// halves (half h: features 8j + 2s + h in rr[j][s]); every lane of the pair returns the same value.
template <int EP>
__device__ __forceinline__ float rn_exact(const f32x4 (&rr)[EP / 8], int e, int h) {
#pragma clang fp contract(off)
  constexpr int HQ = EP / 8;
  const int nv = e >> 3, full = (nv >> 2) << 2, tail = e & 7;
  float A[4], T[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    T[s] = 0.f;
#pragma unroll
    for (int v = 0; v < HQ; ++v) {
      const float x = rr[v][s];
      const float q = x * x;
      if (v < nv) {
        const int a = v < full ? (v & 3) : 0;
        if (a == 0) a0 = a0 + q;
        else if (a == 1) a1 = a1 + q;
        else if (a == 2) a2 = a2 + q;
        else a3 = a3 + q;
      } else if (v == nv) {
        T[s] = q;                      // tail element 8 nv + 2s + h (zero past e)
      }
    }
    A[s] = ((a0 + a1) + a2) + a3;
  }
  float PA[4], PT[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    PA[s] = __shfl_xor(A[s], 32);
    PT[s] = __shfl_xor(T[s], 32);
  }
  if (e < 8) {   // ATen's scalar row sum (4 accumulators over rows of 4, leftovers into the first)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i)
      if (i < e) {
        const float q = ((i & 1) == h) ? T[i >> 1] : PT[i >> 1];
        const int k = i < ((e >> 2) << 2) ? (i & 3) : 0;
        if (k == 0) a0 = a0 + q;
        else if (k == 1) a1 = a1 + q;
        else if (k == 2) a2 = a2 + q;
        else a3 = a3 + q;
      }
    return ((a0 + a1) + a2) + a3;
  }
  float f = 0.f;
#pragma unroll
  for (int jj = 0; jj < 7; ++jj)
    if (jj < tail) f = f + (((jj & 1) == h) ? T[jj >> 1] : PT[jj >> 1]);
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) f = f + (((jj & 1) == h) ? A[jj >> 1] : PA[jj >> 1]);
  return f;
}

// (best, second, index) merge: the lower distance, then the lower index (branch-free selects).
template <bool SECOND>
__device__ __forceinline__ void merge_min(float& best, float& second, int& bi, float ob, float os, int oi) {
  const bool take = (ob < best) | ((ob == best) & (oi < bi));
  if (SECOND) second = take ? fminf(os, best) : fminf(second, ob);
  best = take ? ob : best;
  bi = take ? oi : bi;
}

// ---- the filtered quantizer (rq_filter_kernel, rq.hip) ----
//
// a_k = cn_k - 2 r.c_k from split-bf16 operands (x = hi + lo, the products hi.hi + hi.lo + lo.hi
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16) approximates T_k = cn_k - 2 r.c_k in real
// arithmetic, cn_k the ATen-order norm the exact formula uses; the exact kernel's distance is
// D_k = fl(fl(rn + cn_k) - 2 chain_k).  rq_filter_bound returns E with
//     |a_k - T_k| + |D_k - (rn + T_k)| <= E     for every code k of the level,
// so for the exact winner k* (D_k* <= D_j) and any j:  a_k* <= a_j + 2E.  Every code within 2E of
// the minimum of a is re-scored exactly, hence k* and every code that ties with it are.
//
// With R = |r|, C = max_k |c_k|, cn <= C^2, u = 2^-9 (bf16 RNE) and e <= 64:
//   split:   |x - hi| <= u |x|, x - hi is an fp32 number, |x - hi - lo| <= u^2 |x|, |lo| <= 1.01 u |x|.
//            r c - (hi hi + hi lo + lo hi) = (r c - (hi+lo)(hi+lo)) + lo lo, at most 3.01 u^2 |r||c|
//            per feature, so (Cauchy-Schwarz) 2 x 3.01 x 2^-18 R C            <= 2^-15.4 R C
//   MFMA:    the products are exact in fp32; 3 e/16 <= 12 instructions add at most 193 terms to
//            cn in an unspecified order, every add rounded or truncated to fp32 (2^-23 relative):
//            192 x 2^-23 x (cn + 2.02 R C)                       <= 2^-15.4 cn + 2^-14.4 R C
//            (e = 32: half of that)
//   exact:   chain: 64 x 2^-24 R C, doubled                                   <= 2^-17 R C
//            rn + cn and the final fma, 2^-24 each of at most rn + cn + 2 R C <= 2^-22 (rn + cn)
//   norms:   rn, cn stand for R^2, C^2 within 2^-18 relative (64 rounded adds): absorbed below
//   tiny:    operands or products that are denormal or flushed move every term by at most 2^-126:
//            at most 2^-119 + 2^-120 (R + C)
//   total <= 2^-13.5 R C + 2^-15.3 (rn + C^2) + tiny; the constants below leave a factor >= 1.2 for
//   the norms and for the rounding of m + 2E itself (2^-24 |m|, |m| <= C^2 + 2 R C).
// A non-finite rn or Cmax^2 gives a non-finite E: the kernel then re-scores every code.
__host__ __device__ inline float rq_filter_bound(float rn, float cmax2) {
#pragma clang fp contract(off)
  const float R = __builtin_sqrtf(rn), C = __builtin_sqrtf(cmax2);
  return (0x1p-13f * (R * C) + 0x1p-15f * (rn + cmax2)) + 0x1p-116f * ((R + C) + 1.f);
}

}  // namespace gr
