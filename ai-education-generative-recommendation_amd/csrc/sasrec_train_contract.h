// What makes the two SASRec training kernel sets (sasrec_train.hip: one workgroup per sequence;
// sasrec_train_tiled.hip: tiled launches) interchangeable, each defined once: the g_vec layout, the
// dropout key (site and element under gr_common.h's sas_keep()), the offsets into the saved
// activations (gr_sasrec_train_bufs) and the entry points' argument checks.  Index arithmetic only;
// every expression keeps the operand types of its call sites.
#pragma once
#include "gr_common.h"

namespace gr {

constexpr int SAS_TRAIN_MAXB = 8;   // transformer blocks

// ---- g_vec: one row per sequence (tiled: per split-k part), in the order gr_amd.h documents ------
struct VOff {
  int law, lab, inw, inb, ow, ob, lfw, lfb, w1, b1, w2, b2, size;   // within a block; a block's floats
  int last, pos;   // past the nb blocks: the last LayerNorm's weight (its bias d on), the n x d positional rows
};
__host__ __device__ __forceinline__ VOff voff(int d, int m, int nb) {
  VOff v;
  v.law = 0;
  v.lab = d;
  v.inw = 2 * d;
  v.inb = v.inw + 3 * d * d;
  v.ow = v.inb + 3 * d;
  v.ob = v.ow + d * d;
  v.lfw = v.ob + d;
  v.lfb = v.lfw + d;
  v.w1 = v.lfb + d;
  v.b1 = v.w1 + m * d;
  v.w2 = v.b1 + m;
  v.b2 = v.w2 + d * m;
  v.size = v.b2 + d;
  v.last = nb * v.size;
  v.pos = v.last + 2 * d;
  return v;
}
__host__ __device__ __forceinline__ int sas_vec_width(int nb, int d, int m, int n) { return voff(d, m, nb).pos + n * d; }

// ---- the dropout key: sites of block bk (attention probabilities, FFN hidden layer, FFN output) ----
__host__ __device__ __forceinline__ int sas_site_prob(int bk) { return 3 * bk; }
__host__ __device__ __forceinline__ int sas_site_hidden(int bk) { return 3 * bk + 1; }
__host__ __device__ __forceinline__ int sas_site_out(int bk) { return 3 * bk + 2; }
// elements: probability (head hh, query i, key j) of a sequence of n positions; feature f of row i
// of the sequence's [n, width] activation
__device__ __forceinline__ uint32_t sas_elem_prob(int hh, int n, int i, int j) { return (uint32_t)((hh * n + i) * n + j); }
template <typename I, typename F>
__device__ __forceinline__ uint32_t sas_elem_row(I i, F f, int width) {
  return (uint32_t)(i * width + f);
}

// ---- saved activations: float offsets of sequence b's rows of block bk (b = 0: the block's base) in
// the buffers of width d (xin, hs, os, x1, fs), 3d (qkv), mlp (zs, us) and in prob ------------------
struct SasOffs {
  int64_t rd, r3, rm, pp;
};
__host__ __device__ __forceinline__ SasOffs sas_offs(int bk, int64_t b, int64_t B, int n, int d, int mlp, int heads) {
  const int64_t rows = B * n, r0 = b * n;
  SasOffs o;
  o.rd = (int64_t)bk * rows * d + r0 * d;
  o.r3 = (int64_t)bk * rows * 3 * d + r0 * 3 * d;
  o.rm = (int64_t)bk * rows * mlp + r0 * mlp;
  o.pp = ((int64_t)bk * B + b) * heads * n * n;
  return o;
}

inline bool null_acts(const gr_sasrec_train_bufs& g) {
  return !g.xin || !g.hs || !g.qkv || !g.prob || !g.os || !g.x1 || !g.fs || !g.zs || !g.us || !g.xl;
}

// ---- argument checks ----------------------------------------------------------------------------
struct SasTrainLimits {
  const char* name;   // prefix of the messages
  int n_max, d_max, mlp_max;
  bool row_grids;     // launches with a workgroup row per (sequence, head, position): B * n * heads < 2^31
};

inline int sas_train_check(const SasTrainLimits& lim, const gr_sasrec_params* p, int64_t B, int32_t n, float p_drop,
                           const gr_sasrec_train_bufs* bufs) {
  const std::string w = std::string(lim.name) + ": ";
  const auto num = [](int v) { return std::to_string(v); };
  if (!p || !bufs) return fail(GR_ERR_ARG, w + "null params / buffers");
  if (p->n_blocks < 1 || p->n_blocks > SAS_TRAIN_MAXB)
    return fail(GR_ERR_UNSUPPORTED, w + "1.." + num(SAS_TRAIN_MAXB) + " blocks");
  if (p->d < 1 || p->d > lim.d_max || p->n_heads < 1 || p->d % p->n_heads)
    return fail(GR_ERR_UNSUPPORTED, w + "d <= " + num(lim.d_max) + ", divisible by num_heads");
  if (p->mlp < 1 || p->mlp > lim.mlp_max) return fail(GR_ERR_UNSUPPORTED, w + "mlp_layer <= " + num(lim.mlp_max));
  if (n < 1 || n > lim.n_max || n > p->max_len)
    return fail(GR_ERR_UNSUPPORTED, w + "1 <= n <= min(" + num(lim.n_max) + ", max_len)");
  if (B < 1 || B > (lim.row_grids ? 0x7fffffffLL / n / p->n_heads : 0x7fffffffLL)) return fail(GR_ERR_ARG, w + "bad batch");
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(GR_ERR_ARG, w + "dropout must be in [0, 1)");
  return GR_OK;
}

}  // namespace gr
