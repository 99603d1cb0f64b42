// The scoring chain: the one definition of how a logit h[u] . table[j] is evaluated, shared by every
// kernel that computes one (score.hip, rank_fused.hip, score_topk.hip).  DESIGN §1 (a8/a9) promises
// that a logit is bitwise the same wherever it is recomputed -- full scoring, pairs, count, the
// top-k tile pass, top-k re-scoring, any shard or batch position -- and the strict '>' rank relies
// on it.  The chain is: the sc_feat feature order, v_mfma_f32_32x32x2_f32 steps in (gq, s) order,
// and the D-register row map mfma32_row (gr_common.h).
//
// Two kernels write these helpers out in place instead of calling them, because the calls moved
// their register allocation and measured slower than the parent build (profiles/r14/): the fragment
// load and staging of score_direct_kernel, and the fragment load, staging and chunk chain of
// score_count_kernel.  Their text must stay this file's, line for line; test_score_layouts_identical
// and test_pairs_and_count_equal_materialised_logits compare them bitwise with the kernels that
// call the helpers.  The hand-scheduled MFMA loops of score_direct_kernel / score_rot_kernel and the
// VALU re-scoring of topk_select_kernel reproduce the (gq, s) order by hand.
#pragma once
#include <type_traits>

#include "gr_common.h"

namespace gr {

// The feature order: a d-vector is read as d / 8 float4 groups per lane, lane half hh of group gq
// holding features 8 gq + 4 hh .. +3, and step (gq, s) of the v_mfma_f32_32x32x2_f32 chain adds
// feature 8 gq + s (lane half 0) then 8 gq + 4 + s (lane half 1).  For d >= 32 this is the
// "32 g + 8 q + 4 hh" order of rounds 1-4 (gq = 4 g + q); d = 16 is the same chain over two groups.
__device__ __forceinline__ int sc_feat(int gq, int hh) { return 8 * gq + 4 * hh; }

// User fragment of lane (r, hh) for user u (= tile base + r): hf[gq] = h[u][sc_feat(gq, hh) .. +3],
// the load clamped to row B - 1 and the fragment zeroed when u >= B.
template <int D>
__device__ __forceinline__ void sc_load_user(f32x4 (&hf)[D / 8], const float* h, int64_t u, int64_t B,
                                             int hh) {
  const int64_t uc = u < B ? u : B - 1;
#pragma unroll
  for (int gq = 0; gq < D / 8; ++gq) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(h + uc * D + sc_feat(gq, hh));
    hf[gq] = u < B ? v : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// Table-chunk staging by 256 threads (thread t of the staging group): float4 slot f = t + 256 i of a
// CHUNK-row chunk is row f / (D/4), column 4 (f % (D/4)); LDS rows are padded to P = D + 4 floats
// (conflict-free ds_read_b128).  A 32-row chunk at d = 16 leaves half the threads idle (!FULL).
template <int D, int CHUNK>
struct ScStage {
  static constexpr int P = D + 4;
  static constexpr int NF = CHUNK * D / 4;
  static constexpr int LV = (NF + 255) / 256;
  static constexpr bool FULL = NF % 256 == 0;   // every thread stages LV whole float4s: no guard
  // chunk c of the table into registers; rows past the catalog are clamped to the last row (their
  // logits are masked or never stored)
  static __device__ __forceinline__ void gload(f32x4 (&st)[LV], const float* table, int64_t rows,
                                               int64_t c, int t) {
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = t + 256 * i, row = f / (D / 4), col = (f % (D / 4)) * 4;
      int64_t item = c * CHUNK + row;
      item = item < rows ? item : rows - 1;
      if (FULL || f < NF) st[i] = *reinterpret_cast<const f32x4*>(table + item * D + col);
    }
  }
  // registers -> the LDS chunk buffer tab[CHUNK * P]
  static __device__ __forceinline__ void swrite(float* tab, const f32x4 (&st)[LV], int t) {
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = t + 256 * i, row = f / (D / 4), col = (f % (D / 4)) * 4;
      if (FULL || f < NF) *reinterpret_cast<f32x4*>(&tab[row * P + col]) = st[i];
    }
  }
};

// The plain chunk chain: acc[it] = the 32 x 32 logits of the wave's 32 users against item tile it
// of the staged chunk, tb = &tab[r * P + 4 * hh] (lane r's row of tile 0, its lane half's
// features).  USERS_B = false: users are the MFMA A operand, register v of lane (r, hh) holds user
// mfma32_row(v, hh), item r; true: operands swapped, register v holds item mfma32_row(v, hh), user r
// (a0 b0 + a1 b1 with the factors swapped is the same fp32 value; score_topk.hip).
template <int D, int NT, bool USERS_B>
__device__ __forceinline__ void sc_chunk_chain(f32x16 (&acc)[NT], const f32x4 (&hf)[D / 8], const float* tb) {
  constexpr int P = D + 4;
#pragma unroll
  for (int it = 0; it < NT; ++it)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[it][v] = 0.f;
#pragma unroll
  for (int gq = 0; gq < D / 8; ++gq) {
    f32x4 bt[NT];
#pragma unroll
    for (int it = 0; it < NT; ++it) bt[it] = *reinterpret_cast<const f32x4*>(tb + it * 32 * P + 8 * gq);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int it = 0; it < NT; ++it)
        acc[it] = USERS_B ? mfma32(bt[it][s], hf[gq][s], acc[it]) : mfma32(hf[gq][s], bt[it][s], acc[it]);
  }
}

// The pairs tile: A = the tile's users (lane r = user u, clamped to B - 1), B = their target rows,
// so user r's target logit is the diagonal.  Returns it on the lane with ((r >> 2) & 1) == hh (the
// lane half whose register rows include r).  t = sc_pair_target: the user's target id, 0 and error
// code 1 when it is out of range.
__device__ __forceinline__ int64_t sc_pair_target(const int64_t* ids, int64_t u, int64_t B, int64_t rows,
                                                  int32_t* err) {
  int64_t t = ids[u < B ? u : B - 1];
  if (t < 0 || t >= rows) {
    if (u < B) set_err(err, 1);
    t = 0;
  }
  return t;
}
template <int D>
__device__ __forceinline__ float sc_pair_logit(const float* h, int64_t u, int64_t B, const float* table, int64_t t,
                                               int r, int hh) {
  const int64_t uc = u < B ? u : B - 1;
  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
  for (int gq = 0; gq < D / 8; ++gq) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(h + uc * D + sc_feat(gq, hh));
    const f32x4 b = *reinterpret_cast<const f32x4*>(table + t * D + sc_feat(gq, hh));
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma32(a[s], b[s], acc);
  }
  float d = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v)
    if (mfma32_row(v, hh) == r) d = acc[v];
  return d;
}

// ---- host side: the launch rules the scoring kernels share ----

// Catalog slices per user block: per_cu resident workgroups per CU over ublocks user blocks, rounded
// down so every workgroup is resident at once (rounding up put the last few in a second round),
// within [1, chunks].
inline int64_t sc_slices(int64_t per_cu, int64_t ublocks, int64_t chunks) {
  int64_t sl = per_cu * cu_count() / ublocks;
  if (sl > chunks) sl = chunks;
  return sl < 1 ? 1 : sl;
}

inline bool sc_d_ok(int32_t d) { return d == 16 || d == 32 || d == 64 || d == 128; }

// The shapes the chain is built for, reported under the entry point's name: the width, the operand
// alignment, or both in that order (gr_score_topk_f32 has checks of its own between the two).
inline int sc_check_d(const char* who, int32_t d) {
  return sc_d_ok(d) ? GR_OK : fail(GR_ERR_UNSUPPORTED, std::string(who) + ": d must be 16, 32, 64 or 128");
}
inline int sc_check_aligned(const char* who, const float* h, const float* table) {
  return aligned16(h) && aligned16(table) ? GR_OK
                                          : fail(GR_ERR_ARG, std::string(who) + ": h / table not 16-byte aligned");
}
inline int sc_check(const char* who, int32_t d, const float* h, const float* table) {
  if (int rc = sc_check_d(who, d)) return rc;
  return sc_check_aligned(who, h, table);
}

// f(std::integral_constant<int, D>{}) for the checked d.
template <typename F>
inline auto sc_dispatch_d(int32_t d, F&& f) {
  switch (d) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return f(std::integral_constant<int, 128>{});
  }
}

}  // namespace gr
