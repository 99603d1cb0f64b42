// Fused full-catalog rank (SASRec/evaluate.py:26-32 without the [B, N+1] logits):
//
//   pairs:     t[u]   = h[u] . table[ids[u]]                   (the target's logit, model.py:107)
//   count_gt:  cnt[u] = #{j : l'[u, j] > thr[u]}, l' = h . table^T with column 0 taken as -1e9 when
//              mask_col0 (evaluate.py:27), strict '>' (evaluate.py:32)
//   rank[u]  = count_gt(thr = pairs) + 1
//
// Both kernels evaluate every logit with EXACTLY the instruction sequence of the scoring kernel
// (score.hip): the same v_mfma_f32_32x32x2_f32 operand layout and k order (score_chain.h), so
// t[u] is bitwise the logit the full scoring would have produced and the target never counts
// itself (SURVEY §7 hard part 3).  d = 16, 32, 64 or 128.
//
// count_gt is the scoring kernel with the logits stream replaced by a compare-and-count epilogue:
// MFMA-bound (12.8 Mflop per user at C3) and reads only the table.  Workgroup = 4 waves x 32 users,
// one contiguous catalog slice walked in 64-item chunks (table chunk staged in LDS, prefetched into
// registers one chunk ahead); per-lane counters, reduced over the 32 item lanes at the end, one
// atomic add per (user, slice).
#include "score_chain.h"

namespace gr {

constexpr int RK_CHUNK = 64;
constexpr float RK_MASK = -1e9f;   // evaluate.py:27

template <int D>
__global__ __launch_bounds__(64) void score_pairs_kernel(const float* __restrict__ h, int64_t B,
                                                         const float* __restrict__ table,
                                                         int64_t rows, const int64_t* __restrict__ ids,
                                                         int mask_col0, float* __restrict__ out,
                                                         int32_t* err) {
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int64_t u0 = (int64_t)blockIdx.x * 32;
  const int64_t u = u0 + r;
  const int64_t t = sc_pair_target(ids, u, B, rows, err);
  const float d = sc_pair_logit<D>(h, u, B, table, t, r, hh);
  if (u < B && ((r >> 2) & 1) == hh) out[u] = (mask_col0 && t == 0) ? RK_MASK : d;
}

// One 32-user MFMA tile per wave (128 users per workgroup) and two workgroups per CU: one wave's
// compare-and-count epilogue overlaps another's MFMAs (as in score_topk.hip).
constexpr int RK_UT = 1;

// PAIRS: the thresholds are the users' target logits, computed here from the target ids with
// score_pairs_kernel's MFMA tile (the same operands in the same order: bitwise its values) instead of
// read from thr -- one launch less per rank call (gr_sasrec_rank_f32).  Every slice of a user block
// recomputes its users' pairs (one short MFMA chain per 32 users).
//
// The pairs tile is score_chain.h's.  The fragment load, chunk staging and chunk chain below are
// score_chain.h's sc_load_user / ScStage / sc_chunk_chain<D, 2, false> written out in place: calling
// the helpers changed this kernel's register allocation and measured outside the parent build's
// spread at d = 16 (profiles/r14/ab_chain_all_shared.txt), so the kernel keeps its own text and
// machine code; the torch.equal tests pin it to the definition.
template <int D, bool PAIRS = false>
__global__ __launch_bounds__(256, 2) void score_count_kernel(const float* __restrict__ h, int64_t B,
                                                            const float* __restrict__ table,
                                                            int64_t rows,
                                                            const float* __restrict__ thr,
                                                            int mask_col0,
                                                            unsigned long long* __restrict__ cnt_out,
                                                            int ublocks, int slices, int copies,
                                                            const int64_t* __restrict__ ids = nullptr,
                                                            int32_t* err = nullptr) {
  constexpr int NQ = D / 8;
  using Stage = ScStage<D, RK_CHUNK>;
  constexpr int P = Stage::P;
  static_assert(Stage::FULL, "chunk staging assumes d % 16 == 0");
  __shared__ __attribute__((aligned(16))) float tab[2][RK_CHUNK * P];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wgid = xcd_remap(blockIdx.x, gridDim.x);
  const int ub = wgid % ublocks, sl = wgid / ublocks;
  const int64_t chunks = (rows + RK_CHUNK - 1) / RK_CHUNK;
  const int64_t c_begin = chunks * sl / slices, c_end = chunks * (sl + 1) / slices;
  if (c_begin >= c_end) return;
  constexpr int UT = RK_UT;
  const int64_t u0 = ((int64_t)ub * 4 + w) * (32 * UT);

  f32x4 hf[UT][NQ];
  float th[UT][16];
#pragma unroll
  for (int ut = 0; ut < UT; ++ut) {
    const int64_t u = u0 + ut * 32 + r;
    const int64_t uc = u < B ? u : B - 1;
#pragma unroll
    for (int gq = 0; gq < NQ; ++gq) {   // score_chain.h sc_load_user, in place (see above)
      const f32x4 v = *reinterpret_cast<const f32x4*>(h + uc * D + sc_feat(gq, hh));
      hf[ut][gq] = u < B ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (PAIRS) {   // score_pairs_kernel's tile: user r's target logit on its diagonal lane
      const int64_t t = sc_pair_target(ids, u, B, rows, err);
      float dg = sc_pair_logit<D>(h, u, B, table, t, r, hh);
      if (mask_col0 && t == 0) dg = RK_MASK;
#pragma unroll
      for (int v = 0; v < 16; ++v) {   // register v's user mfma32_row(v, hh): from its diagonal lane
        const int uu = mfma32_row(v, hh);
        th[ut][v] = __shfl(dg, uu + 32 * ((uu >> 2) & 1));
      }
    } else {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t uu = u0 + ut * 32 + mfma32_row(v, hh);
        th[ut][v] = thr[uu < B ? uu : B - 1];
      }
    }
  }
  constexpr int LV = Stage::LV;
  f32x4 st[LV];
  auto gload = [&](int64_t c) {   // ScStage::gload / swrite, in place
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = tid + 256 * i, row = f / (D / 4), col = (f % (D / 4)) * 4;
      int64_t item = c * RK_CHUNK + row;
      item = item < rows ? item : rows - 1;
      st[i] = *reinterpret_cast<const f32x4*>(table + item * D + col);
    }
  };
  auto swrite = [&](int b) {
#pragma unroll
    for (int i = 0; i < LV; ++i) {
      const int f = tid + 256 * i, row = f / (D / 4), col = (f % (D / 4)) * 4;
      *reinterpret_cast<f32x4*>(&tab[b][row * P + col]) = st[i];
    }
  };
  gload(c_begin);
  swrite(0);
  __syncthreads();
  int cnt[UT][16];
#pragma unroll
  for (int ut = 0; ut < UT; ++ut)
#pragma unroll
    for (int v = 0; v < 16; ++v) cnt[ut][v] = 0;
  int buf = 0;
#pragma unroll 1
  for (int64_t c = c_begin; c < c_end; ++c) {
    if (c + 1 < c_end) gload(c + 1);
    f32x16 acc[UT][2];   // sc_chunk_chain<D, 2, false>, in place
#pragma unroll
    for (int ut = 0; ut < UT; ++ut)
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[ut][it][v] = 0.f;
    const float* tb = &tab[buf][r * P + 4 * hh];
#pragma unroll
    for (int gq = 0; gq < NQ; ++gq) {
      f32x4 bt[2];
#pragma unroll
      for (int it = 0; it < 2; ++it) bt[it] = *reinterpret_cast<const f32x4*>(tb + it * 32 * P + 8 * gq);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int ut = 0; ut < UT; ++ut) acc[ut][it] = mfma32(hf[ut][gq][s], bt[it][s], acc[ut][it]);
    }
    const int64_t c0 = c * RK_CHUNK;
    if (c0 + RK_CHUNK <= rows && !(mask_col0 && c0 == 0)) {   // steady state: no column masks
#pragma unroll
      for (int ut = 0; ut < UT; ++ut)
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int v = 0; v < 16; ++v) cnt[ut][v] += acc[ut][it][v] > th[ut][v] ? 1 : 0;
    } else {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int64_t col = c0 + it * 32 + r;
        const bool ok = col < rows;
        const bool m0 = mask_col0 && col == 0;
#pragma unroll
        for (int ut = 0; ut < UT; ++ut)
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const float l = m0 ? RK_MASK : acc[ut][it][v];
            cnt[ut][v] += (ok && l > th[ut][v]) ? 1 : 0;
          }
      }
    }
    if (c + 1 < c_end) swrite(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // reduce over the 32 item lanes of each half, one atomic per (user, slice)
#pragma unroll
  for (int ut = 0; ut < UT; ++ut)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      int x = cnt[ut][v];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) x += __shfl_xor(x, o);
      const int64_t u = u0 + ut * 32 + mfma32_row(v, hh);
      // slice sl adds into copy sl % copies: at most ceil(slices / copies) adds per address (a
      // short batch split over every CU's slices would otherwise queue hundreds of adds on one word)
      if (r == 0 && u < B && x) atomicAdd(&cnt_out[(int64_t)(sl % copies) * B + u], (unsigned long long)x);
    }
}

// counts[u] = sum of the copies' words in copy order (exact integer sums), which are cleared for the
// next call
__global__ __launch_bounds__(256) void count_copies_kernel(unsigned long long* __restrict__ ws, int64_t B, int copies,
                                                           int64_t* __restrict__ counts, int64_t base) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= B) return;
  unsigned long long s = (unsigned long long)base;
  for (int c = 0; c < copies; ++c) {
    s += ws[(int64_t)c * B + u];
    ws[(int64_t)c * B + u] = 0;
  }
  counts[u] = (int64_t)s;
}

constexpr int RK_COPIES = 16;   // count copies in the workspace form

}  // namespace gr

extern "C" int gr_score_pairs_f32(const float* h, int64_t B, int32_t d, const float* table,
                                  int64_t rows, const int64_t* ids, int32_t mask_col0, float* out,
                                  int32_t* err_flag, void* stream) {
  using namespace gr;
  clear_error();
  return gr_score_pairs_launch(h, B, d, table, rows, ids, mask_col0, out, err_flag, reinterpret_cast<hipStream_t>(stream));
}

int gr_score_pairs_launch(const float* h, int64_t B, int32_t d, const float* table, int64_t rows, const int64_t* ids,
                          int32_t mask_col0, float* out, int32_t* err_flag, hipStream_t st) {
  using namespace gr;
  if (B < 0 || rows < 1) return fail(GR_ERR_ARG, "gr_score_pairs_f32: bad shape");
  if (B == 0) return GR_OK;
  if (!h || !table || !ids || !out) return fail(GR_ERR_ARG, "gr_score_pairs_f32: null pointer");
  if (int rc = sc_check("gr_score_pairs_f32", d, h, table)) return rc;
  const unsigned grid = (unsigned)((B + 31) / 32);
  sc_dispatch_d(d, [&](auto dd) {
    constexpr int DD = decltype(dd)::value;
    hipLaunchKernelGGL(score_pairs_kernel<DD>, dim3(grid), dim3(64), 0, st, h, B, table, rows, ids, mask_col0,
                       out, err_flag);
  });
  return check_launch("gr_score_pairs_f32");
}

// counts_out[u] = base + #{j : l'[u, j] > thresholds[u]} (base 1: the 1-based rank of evaluate.py:32)
// pair_ids (rank mode): thresholds = the target logits of pair_ids, computed in the count kernel;
// preinit: counts_out already holds base (written by the forward), so the direct form skips its fill.
static int count_launch(const float* h, int64_t B, int32_t d, const float* table, int64_t rows,
                        const float* thresholds, int32_t mask_col0, int64_t* counts_out, void* workspace,
                        size_t workspace_bytes, hipStream_t st, int64_t base = 0,
                        const int64_t* pair_ids = nullptr, int32_t* err = nullptr, bool preinit = false) {
  using namespace gr;
  clear_error();
  if (B < 0 || rows < 0) return fail(GR_ERR_ARG, "gr_score_count_gt_f32: bad shape");
  if (B == 0) return GR_OK;
  if (!h || !table || !(thresholds || pair_ids) || !counts_out) return fail(GR_ERR_ARG, "gr_score_count_gt_f32: null pointer");
  if (int rc = sc_check("gr_score_count_gt_f32", d, h, table)) return rc;
  const int64_t ublocks = (B + 128 * RK_UT - 1) / (128 * RK_UT);
  const int64_t chunks = (rows + RK_CHUNK - 1) / RK_CHUNK;
  const int64_t slices = sc_slices(2, ublocks, chunks);   // two resident workgroups per CU (registers, LDS)
  if (ublocks * slices > 0x7fffffffLL) return fail(GR_ERR_UNSUPPORTED, "gr_score_count_gt_f32: grid too large");
  // the workspace form (a zeroed buffer of RK_COPIES copies) when many slices share each user: the
  // counts go to slice % RK_COPIES and one more launch sums the copies
  const bool copies = workspace && workspace_bytes >= gr_score_count_workspace_bytes(B) && slices > 4 * RK_COPIES;
  unsigned long long* cnt = copies ? reinterpret_cast<unsigned long long*>(align_up(reinterpret_cast<uintptr_t>(workspace), 256))
                                   : reinterpret_cast<unsigned long long*>(counts_out);
  if (!copies && !preinit && gr_fill64_launch(counts_out, (uint64_t)base, B, st) != GR_OK)
    return fail(GR_ERR_HIP, "gr_score_count_gt_f32: memset failed");
  if (rows == 0) {
    if (copies) return gr_fill64_launch(counts_out, (uint64_t)base, B, st) == GR_OK ? GR_OK : fail(GR_ERR_HIP, "memset");
    return GR_OK;
  }
  const int nc = copies ? RK_COPIES : 1;
  const dim3 g((unsigned)(ublocks * slices)), b(256);
  sc_dispatch_d(d, [&](auto dd) {
    constexpr int DD = decltype(dd)::value;
    if (pair_ids)
      hipLaunchKernelGGL((score_count_kernel<DD, true>), g, b, 0, st, h, B, table, rows, thresholds, mask_col0,
                         cnt, (int)ublocks, (int)slices, nc, pair_ids, err);
    else
      hipLaunchKernelGGL((score_count_kernel<DD, false>), g, b, 0, st, h, B, table, rows, thresholds, mask_col0,
                         cnt, (int)ublocks, (int)slices, nc, nullptr, nullptr);
  });
  int rc = check_launch("gr_score_count_gt_f32");
  if (rc || !copies) return rc;
  hipLaunchKernelGGL(count_copies_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, cnt, B, RK_COPIES,
                     counts_out, base);
  return check_launch("gr_score_count_gt_f32 (copies)");
}

extern "C" size_t gr_score_count_workspace_bytes(int64_t B) {
  return B <= 0 ? 0 : (size_t)gr::RK_COPIES * (size_t)B * 8 + 256;
}

extern "C" int gr_score_count_gt_f32(const float* h, int64_t B, int32_t d, const float* table,
                                     int64_t rows, const float* thresholds, int32_t mask_col0,
                                     int64_t* counts_out, void* stream) {
  return count_launch(h, B, d, table, rows, thresholds, mask_col0, counts_out, nullptr, 0,
                      reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gr_score_count_gt_ws_f32(const float* h, int64_t B, int32_t d, const float* table,
                                        int64_t rows, const float* thresholds, int32_t mask_col0,
                                        int64_t* counts_out, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return count_launch(h, B, d, table, rows, thresholds, mask_col0, counts_out, workspace, workspace_bytes,
                      reinterpret_cast<hipStream_t>(stream));
}

int gr_score_rank_launch(const float* h, int64_t B, int32_t d, const float* table, int64_t rows, const int64_t* ids,
                         int32_t mask_col0, int64_t* ranks_out, void* count_ws, size_t count_ws_bytes,
                         int32_t* err_flag, bool ranks_preinit, hipStream_t st) {
  if (rows < 1) return gr::fail(GR_ERR_ARG, "gr_sasrec_rank_f32: empty item table");
  if (!ids) return gr::fail(GR_ERR_ARG, "gr_sasrec_rank_f32: null targets");
  return count_launch(h, B, d, table, rows, nullptr, mask_col0, ranks_out, count_ws, count_ws_bytes, st, 1, ids,
                      err_flag, ranks_preinit);
}
