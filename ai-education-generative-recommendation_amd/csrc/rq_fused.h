// What the fused RQ encoder (rq_fused.hip) shares with the quantizer launch that follows it (rq.hip):
// the workgroup context, layers 2-3 of an item tile whose relu(h1) sits in LDS (rq_l23), the staging
// of a leftover tile's images, and the quantizer's tile plan.  rq_leftover_kernel (rq_fused.hip) and
// the prologue of rq_filter_kernel (rq.hip) finish a leftover tile with the same code.
#pragma once

#include "gr_common.h"

#ifndef GR_EDIAG
#define GR_EDIAG 0   // diagnostic builds only (scripts/build_variant.sh; wrong results, timing only): 1 no
#endif               // layer 2, 2 no layer 3 / z store, 3 no leftover pieces and no rq_leftover_kernel

namespace gr {

constexpr int FT = 32;            // items per tile
constexpr int FP = 2;             // tiles per pass
constexpr int FXC = 64;           // x k-chunk
constexpr int FXP = FXC + 4;      // LDS pitch of the x image (== 4 mod 64: conflict-free b128)
constexpr int FWV = 8;            // waves per workgroup

template <int H1, int H2>
struct FusedCfg {
  static constexpr int E = 32;
  static constexpr int NTH = 64 * FWV;   // threads per workgroup
  static constexpr int P1 = H1 + 4, P2 = H2 + 4, P3 = H2 + 4;
  static constexpr int PI = FP * FT;     // items per (full) pass
  static constexpr int XV = PI * 16 / NTH;
  static constexpr int LDS = 2 * PI * FXP + PI * P1 + PI * P2 + E * P3;
  static constexpr int TAIL_LDS = FT * P1 + FT * P2 + E * P3;   // floats of rq_leftover_tile's images
  static_assert(H1 == 32 * FWV && H2 == 128, "8-wave form: H1 = 256, H2 = 128");
  static_assert(XV == FP, "x staging: a thread's float4 i is a row of item tile i (XSrc)");
};

// A 16-byte load from a pointer known to be global memory.  The weight and bias pointers of the later
// phases pass through an empty asm (rq_fused_pass) and come out without their address space; a plain
// dereference is then a flat load, which counts on lgkmcnt as well as vmcnt -- every LDS wait behind
// it (the next ds_read's, a barrier's) waits out its L2 round trip too.
__device__ __forceinline__ f32x4 ldg4(const float* p) {
  return *reinterpret_cast<const __attribute__((address_space(1))) f32x4*>(reinterpret_cast<uintptr_t>(p));
}

// x staging: thread f of the workgroup moves 16 bytes (features 4u..4u+3, u = f & 15) of item row
// xrow(f) of a chunk.  The 16 lanes of a row are contiguous (256-byte global segments); the two rows
// of a half-wave are 4 apart, 4 x FXP = 16 floats mod 64 banks, so their packed 8-byte LDS writes
// ([0, 16) + [32, 48) and [16, 32) + [48, 64) of a row's window) never share a bank.  The compiler
// emits each 8-byte pair as ds_write2_b32 {v0 -> p, v2 -> p + 1} and {v1 -> p + 16, v3 -> p + 17}
// (put_packed: scalar stores, so no register pair has to be assembled): the same addresses, lanes
// and banks as the 8-byte writes.
// xrow(f + 64 FWV) = xrow(f) + FT: a thread's second float4 is the same row of the image's upper half.
__device__ __forceinline__ int xrow(int f) { return ((f >> 7) << 3) + ((f >> 5) & 3) + 4 * ((f >> 4) & 1); }

// Packed-order position of the 4 consecutive features k0..k0+3 (k0 % 4 == 0) of a 32-deep group:
// feature 8j + 2s + h sits at 16h + 4j + s, so a float4 {v0, v1, v2, v3} goes to p, p + 16, p + 1, p + 17.
__device__ __forceinline__ int packed_pos(int k0) {
  const int g = k0 & ~31, q = k0 & 31, j = q >> 3, e2 = (q >> 1) & 2;
  return g + 4 * j + e2;
}
__device__ __forceinline__ void put_packed(float* p, const f32x4& v) {
  p[0] = v[0];
  p[16] = v[1];
  p[1] = v[2];
  p[17] = v[3];
}

// Global operands of layer 1 come through buffer resources (scalar base + byte count, a loop-invariant
// per-lane byte offset, and a scalar offset for whatever moves from chunk to chunk), so the chunk loops
// carry no vector address arithmetic, and a lane whose byte offset is at or past the count reads zeros
// without touching memory (the hardware's range check; it sees the per-lane offset, not the scalar one).
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const float* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_ld4(rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
}

// The x rows a pass stages, as two resources: half[i] serves every thread's float4 i, i.e. image rows
// [FT i, FT i + FT).  A thread's byte offset into either is the same for the whole kernel,
// FusedCtx::xvo = (xrow(tid) D0 + 4 (tid & 15)) floats: row xrow(tid) of the half, and what differs
// between the halves and between the two image layouts is in the (scalar) base.  The byte count is
// that of the half's rows that exist AND belong to the pass -- rows past n, past the workgroup's
// range or of no pass at all are beyond it and read as zeros, and no address outside x is formed by
// a load that passes the check: with r = xrow(tid) < rows, base + xvo + chunk offset lies inside row
// r of the half (the chunk offset stays inside a row by the chunk counts of the loops).  The base is
// per pass: n x D0 x 4 bytes does not fit a resource's 32-bit count from 1.4 M rows of 768 on.
struct XSrc {
  rsrc_t half[2];
};

// Per-workgroup state that lives across passes (x staging registers, W1 prefetch, LDS buffer).
template <int H1, int H2>
struct FusedCtx {
  using C = FusedCfg<H1, H2>;
  const float* x;
  int64_t n;
  int D0, NC, csplit, t_end;
  const float *W2, *b1, *b2, *W3, *b3;
  float* z_out;
  float *xs, *h1s, *h2s, *w3s;
  int tid, w, r, h;
  rsrc_t w1rs;            // the packed W1
  int w1vo;               // this lane's byte offset into it: row 32 w + r, operand half h
  f32x4 awc[4];           // W1 fragments of the current 32-deep group
  f32x4 awc2[4];          // k-split pass: the same for the second MKL block's chain
  f32x4 w2f[4];           // L2: W2 fragments of the first four 16-deep blocks (the same every pass)
  f32x4 xr[C::XV];
  f32x4 bxa[4];           // L1: item tile 0's x fragments of the NEXT 32-deep group (read_bxa)
  int xvo;                // this thread's byte offset into an XSrc half
  // The x image is double-buffered.  Both LDS addresses a thread needs are carried, not rebuilt from a
  // parity: xrd = this lane's fragment row in the buffer being READ, xwr = this thread's packed
  // position in the buffer being WRITTEN (the other one), xflip = +- the buffer size.  flip() after
  // the chunk barrier costs one vector add each.
  const float* xrd;
  float* xwr;
  int xflip;
  __device__ __forceinline__ void flip() {
    xrd += xflip;
    xwr -= xflip;
    xflip = -xflip;
  }
  // The x source of the pass that starts at tile tb (tb < 0: no pass, every row reads as zero).
  // ks: the k-split layout -- ONE tile, image rows [FT, 2 FT) hold the same items at k + csplit FXC
  // (a k-split pass or a leftover-tile piece; the tile may lie past t_end).  Otherwise up to FP tiles
  // of this workgroup's range, image row = row of the pass.
  __device__ __forceinline__ XSrc xsrc_of(int tb, bool ks) const {
    const int64_t row0 = (int64_t)(tb < 0 ? 0 : tb) * FT;
    const int tl = ks ? 1 : (t_end - tb < FP ? t_end - tb : FP);
    int64_t left = n - row0;
    if (left > tl * FT) left = tl * FT;
    const int rows = (tb < 0 || left < 0) ? 0 : (int)left;
    const float* p = x + row0 * D0;
    const int lo = rows < FT ? rows : FT;
    XSrc s;
    s.half[0] = make_rsrc(p, lo * D0 * 4);
    s.half[1] = ks ? make_rsrc(p + csplit * FXC, lo * D0 * 4) : make_rsrc(p + (int64_t)FT * D0, (rows - lo) * D0 * 4);
    return s;
  }
  // chunk c of s into the staging registers (soff = the chunk's byte offset inside a row)
  __device__ __forceinline__ void gload_x(const XSrc& s, int soff) {
#pragma unroll
    for (int i = 0; i < C::XV; ++i) xr[i] = buf_ld4(s.half[i], xvo, soff);
  }
  // Item tile 0's fragments are read one 32-deep group ahead of their MFMAs: group 1's during group
  // 0 (the same image), group 0's right behind the barrier that publishes their image -- the next
  // chunk's, the next pass's chunk 0 (which stays in place through L2 / L3), or after a workgroup's
  // last chunk an image that nobody uses (always inside the x buffers).  A read issued at the head
  // of its own group is waited for with nothing queued on the MFMA pipe, by both waves of a SIMD at
  // once, since they leave the barrier together.
  __device__ __forceinline__ void read_bxa(int g) {
    const float* xb = xrd + g * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) bxa[j] = *reinterpret_cast<const f32x4*>(xb + 4 * j);
  }
  // the staging registers -> the buffer being written (cur: the one being read, before its barrier)
  __device__ __forceinline__ void swrite_x(bool cur = false) {
    float* p = cur ? xwr - xflip : xwr;
#pragma unroll
    for (int i = 0; i < C::XV; ++i) put_packed(p + i * FT * FXP, xr[i]);
  }
};

// The h1 image is in the 16x16x4 ("transposed") order L2 reads: within every 16-feature block,
// feature 4t + g sits at 4 (g ^ x) + t, where x = h1_swz(row) flips the block's k-group pairs in
// rows 4..11 of every 16.  A 16x16x4 lane (j, g) reads row 16 tile + j at 16b + 4 (g ^ x) as one
// float4 (four k steps); with a pitch == 4 mod 64 the sixteen lanes of every ds_read_b128 lane
// group ({0-3, 12-15} of one g with {4-11} of g ^ 1, MI355X LDS) then start at sixteen different
// multiples of four banks -- without the flip lanes 12 and 27 (and 19 and 8) share banks.
__device__ __forceinline__ int h1_swz(int row) { return ((row >> 2) ^ (row >> 3)) & 1; }

// L1 h^T accumulator (feature rows 8g4 + 4h + i of a 32-feature tile, item column r) -> the h1
// image row: feature 8g4 + 4h + i = 16 (g4 >> 1) + 4t + g with t = 2 (g4 & 1) + h, g = i.
__device__ __forceinline__ void store_h1(float* row, int x, int g4, int h, const f32x4& o) {
  float* p = row + 16 * (g4 >> 1) + 2 * (g4 & 1) + h;
#pragma unroll
  for (int i = 0; i < 4; ++i) p[4 * (i ^ x)] = o[i];
}

// Layers 2 and 3 of NR item tiles whose relu(h1) sits in cx.h1s (8 waves): z = W3 . relu(W2 . h1 +
// b2) + b3 for tiles tb .. tb + NR - 1, written to cx.z_out.  cx.W2 is the 16x16x4-order image.
// ZL (NR = 1): the tile's z also goes to the LDS image zl ([FT][ZLP], every row, natural order) for
// the quantizer that runs next in the same workgroup; zl may alias cx.h1s, which L3 does not read.
constexpr int ZLP = 36;   // pitch of the z hand-off image (16-byte rows, 4 banks apart)
template <int NR, int H1, int H2, bool ZL = false>
__device__ __forceinline__ void rq_l23(FusedCtx<H1, H2>& cx, int tb, float* zl = nullptr) {
#pragma clang fp contract(off)
  using C = FusedCfg<H1, H2>;
  constexpr int E = C::E, P1 = C::P1, P2 = C::P2;
  const int w = cx.w, lane = cx.tid & 63, j = lane & 15, g = lane >> 4;
  f32x4 bb3;   // L3's bias fragment (output half w & 1)
  // ------------------------------------------------------------------ L2: W2 . h1^T
  // v_mfma_f32_16x16x4_f32 (one fma chain over k in order, as L3): wave w owns features [16w, 16w +
  // 16) for the pass's NT 16-item tiles -- NT independent chains of K = 256 per wave on all 8 waves
  // (2 waves per SIMD), W2 fragments from L2 pipelined four 16-deep blocks ahead.
  {
    constexpr int NT = 2 * NR, UB = 4, NI = H1 / (16 * UB);
    f32x4 acc2[NT];
#pragma unroll
    for (int it = 0; it < NT; ++it) acc2[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* hb = cx.h1s + j * P1 + 4 * (g ^ h1_swz(j));
    const float* w2row = cx.W2 + (int64_t)(w * 16 + j) * H1 + 4 * g;
    // the first UB blocks' fragments are the same for every pass: loaded once per workgroup
    // (cx.w2f), so the phase does not start on an L2 round trip; the biases of this phase and of
    // L3 are fetched here, a whole phase before their use (a load placed after the loops would be
    // issued there, and both waves of a SIMD would wait for it together)
    f32x4 aw2[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) aw2[u] = cx.w2f[u];
    const f32x4 bb = ldg4(cx.b2 + w * 16 + 4 * g);
    bb3 = ldg4(cx.b3 + 16 * (w & 1) + 4 * g);
    asm volatile("" ::: "memory");
#pragma unroll 1
    for (int bi = 0; bi < (GR_EDIAG == 1 ? 0 : NI); ++bi) {
      const int bn = (bi + 1 < NI) ? bi + 1 : bi;
      f32x4 awn[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) awn[u] = ldg4(w2row + 16 * (bn * UB + u));
      f32x4 bx[UB][NT];
#pragma unroll
      for (int u = 0; u < UB; ++u)
#pragma unroll
        for (int it = 0; it < NT; ++it)
          bx[u][it] = *reinterpret_cast<const f32x4*>(hb + it * 16 * P1 + 16 * (bi * UB + u));
#pragma unroll
      for (int u = 0; u < UB; ++u)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int it = 0; it < NT; ++it) acc2[it] = mfma16(aw2[u][t], bx[u][it][t], acc2[it]);
      // same interleave as L1: the first block's h1 fragments, then one load per MFMA
      __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);
#pragma unroll
      for (int i = 0; i < UB; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
#pragma unroll
      for (int i = 0; i < (UB - 1) * NT; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * UB * NT - UB - (UB - 1) * NT, 0);
#pragma unroll
      for (int u = 0; u < UB; ++u) aw2[u] = awn[u];
    }
    // acc2[it][i]: feature 16w + 4g + i of item 16 it + j.  L3 layout: within each 16-feature
    // block, feature 4t + g at 4g + t (a lane of k group g reads four consecutive 16x16x4 steps
    // as one float4)
#pragma unroll
    for (int it = 0; it < NT; ++it) {
      float* row = cx.h2s + (it * 16 + j) * P2 + w * 16 + g;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float u = bb[i] + acc2[it][i];
        row[4 * i] = u < 0.f ? 0.f : u;
      }
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ L3: W3 . h2^T
  // 16x16x4 tiles (16 outputs x 16 items), one per wave: item tile w >> 2, item half (w >> 1) & 1,
  // output half w & 1; one k-ordered chain over k = 0..127 (32 MFMAs), z = b3 + chain, to HBM.
  // W3 arrives packed for this form: feature 16b + 4t + g of a row at 16b + 4g + t.
  if (GR_EDIAG != 2 && w < 4 * NR) {
    const int it = w >> 2, ih = (w >> 1) & 1, oh = w & 1;
    f32x4 acc3 = {0.f, 0.f, 0.f, 0.f};
    const float* hb = cx.h2s + (it * FT + 16 * ih + j) * P2 + 4 * g;
    const float* w3row = cx.w3s + (16 * oh + j) * C::P3 + 4 * g;   // LDS: rows 4 banks apart
#pragma unroll
    for (int b = 0; b < H2 / 16; ++b) {
      const f32x4 aw = *reinterpret_cast<const f32x4*>(w3row + 16 * b);
      const f32x4 bx = *reinterpret_cast<const f32x4*>(hb + 16 * b);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc3 = mfma16(aw[t], bx[t], acc3);
    }
    const int64_t item = (int64_t)(tb + it) * FT + 16 * ih + j;
    if constexpr (ZL) {
      static_assert(NR == 1, "z hand-off: one tile");
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = bb3[i] + acc3[i];
      *reinterpret_cast<f32x4*>(zl + (16 * ih + j) * ZLP + 16 * oh + 4 * g) = o;
      if (item < cx.n) *reinterpret_cast<f32x4*>(cx.z_out + item * E + 16 * oh + 4 * g) = o;
    } else if (item < cx.n) {
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = bb3[i] + acc3[i];
      *reinterpret_cast<f32x4*>(cx.z_out + item * E + 16 * oh + 4 * g) = o;
    }
  }
}

// One leftover tile from the pieces' relu(h1) (h1t: [FT][H1], natural order) to z: the h1 image in
// the 16x16x4 order and W3 staged into LDS (h1s [FT][P1], h2s [FT][P2], w3s [E][P3]: FusedCfg::TAIL_LDS
// floats in all), then rq_l23<1>.  All FWV waves of the workgroup; barriers inside, none at the end.
template <int H1, int H2, bool ZL = false>
__device__ __forceinline__ void rq_leftover_tile(const float* __restrict__ h1t, int64_t n, int tile,
                                                 const float* __restrict__ W2, const float* __restrict__ b2,
                                                 const float* __restrict__ W3, const float* __restrict__ b3,
                                                 float* __restrict__ z_out, float* h1s, float* h2s, float* w3s,
                                                 float* zl = nullptr) {
  using C = FusedCfg<H1, H2>;
  const int tid = threadIdx.x, lane = tid & 63;
  FusedCtx<H1, H2> cx;
#pragma unroll
  for (int u = 0; u < 4; ++u)   // in flight while the images are staged
    cx.w2f[u] = *reinterpret_cast<const f32x4*>(W2 + (int64_t)((tid >> 6) * 16 + (lane & 15)) * H1 + 4 * (lane >> 4) + 16 * u);
  for (int f = tid; f < FT * H1 / 4; f += C::NTH) {   // relu(h1) -> the h1 image (16x16x4 order)
    const int row = f / (H1 / 4), k0 = (f % (H1 / 4)) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(h1t + row * H1 + k0);
    float* p = h1s + row * C::P1 + (k0 & ~15) + ((k0 >> 2) & 3);   // features 16b + 4t + g, g = 0..3
#pragma unroll
    for (int g = 0; g < 4; ++g) p[4 * (g ^ h1_swz(row))] = v[g];
  }
  for (int f = tid; f < C::E * H2 / 4; f += C::NTH) {
    const int row = f / (H2 / 4), qq = f % (H2 / 4);
    *reinterpret_cast<f32x4*>(w3s + row * C::P3 + 4 * qq) = *reinterpret_cast<const f32x4*>(W3 + row * H2 + 4 * qq);
  }
  __syncthreads();
  cx.n = n; cx.W2 = W2; cx.b2 = b2; cx.W3 = W3; cx.b3 = b3; cx.z_out = z_out;
  cx.h1s = h1s; cx.h2s = h2s; cx.w3s = w3s;
  cx.tid = tid; cx.w = tid >> 6; cx.r = lane & 31; cx.h = lane >> 5;
  rq_l23<1, H1, H2, ZL>(cx, tile, zl);
}

// ---- the filtered quantizer's tile plan (rq_filter_kernel, rq.hip) ----
// T tiles over G workgroups of RQ_W waves; the last `left` tiles are the encoder's leftover tiles,
// whose layers 2-3 are still pending when the quantizer starts (left = 0: none).  Workgroup b < left
// owns leftover tile T - left + b, which it finishes itself before quantizing, plus `om` main tiles;
// the other workgroups share the remaining main tiles evenly.  Every range is contiguous.  An owner
// has max(1, T / G - RQ_TAIL_S) tiles in all, its leftover tile included.
constexpr int RQ_W = 8;   // waves per quantize workgroup
#ifndef GR_FMAXT
#define GR_FMAXT 2   // item tiles per wave held in registers (3: 238 VGPRs, 4 spills)
#endif
#ifndef GR_FTAIL_S
#define GR_FTAIL_S 2   // tiles an owner gives up for its prologue (0, 1, 2 timed: profiles/r19/ab_rq_parts.txt)
#endif
constexpr int RQ_TAIL_S = GR_FTAIL_S;

// Main tiles [mb, me) of workgroup b.
__host__ __device__ inline void rq_filter_range(int T, int G, int left, int b, int& mb, int& me) {
  if (left == 0) {
    mb = (int)((int64_t)b * T / G);
    me = (int)((int64_t)(b + 1) * T / G);
    return;
  }
  const int main = T - left, N = G - left;
  if (N == 0) {   // every workgroup owns a leftover tile (the short-call plan: main = 0)
    mb = (int)((int64_t)b * main / G);
    me = (int)((int64_t)(b + 1) * main / G);
    return;
  }
  int own = T / G - RQ_TAIL_S;
  if (own < 1) own = 1;
  const int om = own - 1;   // om left <= main, since left <= G
  if (b < left) {
    mb = b * om;
    me = mb + om;
    return;
  }
  const int R = main - om * left, k = b - left;
  mb = om * left + (int)((int64_t)k * R / N);
  me = om * left + (int)((int64_t)(k + 1) * R / N);
}

// The largest tile count of a workgroup under rq_filter_range (leftover tile included).
inline int rq_filter_max_count(int T, int G, int left) {
  if (left == 0) return (int)(((int64_t)T + G - 1) / G);
  const int main = T - left, N = G - left;
  if (N == 0) return 1 + (main + G - 1) / G;
  int own = T / G - RQ_TAIL_S;
  if (own < 1) own = 1;
  const int64_t R = (int64_t)main - (int64_t)(own - 1) * left, oth = (R + N - 1) / N;
  return own > oth ? own : (int)(oth < 0x7fffffff ? oth : 0x7fffffff);
}

}  // namespace gr
