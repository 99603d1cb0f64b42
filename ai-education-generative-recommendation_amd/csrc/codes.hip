// Collision groups and dedup digit of semantic IDs -- the integer tail of RQ-VAE/infer.py:
//
//   get_collision_item (infer.py:29-41): the rows that share a code, grouped in the order of each
//                      code's first appearance, members in row order;
//   the dedup digit    (infer.py:139-162): 0, 1, 2, ... over the members of every shared code;
//   the collision rate (RQ-VAE/train.py:127-151): (n - distinct codes) / n.
//
// codes[n, L] int64.  Per row r: leader[r] = the smallest row with r's code, count[r] = the rows
// with that code, digit[r] = the rows before r with that code.
//
//  1. code_init_kernel    clears the hash table, the key list and the stats (no host memset).
//  2. code_build_kernel   open addressing over {row, counter} slots, linear probing.  A row claims
//                         an empty slot by compare-and-swap of its own index; on a taken slot it
//                         compares its code with codes[slot's row] -- the key is the read-only input
//                         itself, so a half-written key cannot be observed -- and on a match lowers
//                         the slot to min(row) and bumps its counter.  A slot's row only ever changes
//                         to another row of the SAME code, so any value read from it, however stale,
//                         names the slot's code.  No thread waits on another; the table has at least
//                         2n slots, so a probe always ends.  min and count do not depend on arrival
//                         order: the outputs are a function of the input alone.
//  3. code_lookup_kernel  every row finds its slot again and writes leader / count (digit = 0); the
//                         stats are reduced per wave (ballots) and per workgroup (LDS) before one
//                         global atomic each, and the rows of shared codes are appended as keys
//                         leader << 32 | row behind one cursor add per workgroup.
//  4. the caller sorts the keys (they are unique; the unused tail holds INT64_MAX).
//  5. seg_* kernels       one scan over the sorted keys carrying (segment starts so far, index of
//                         the last start): the leader is the smallest row of its code, so it is
//                         first in its segment, and digit = position - position of the leader.
//                         Block sums, one block scanning them, then the write pass: no look-back.
//
// Codes are compared as whole rows of full int64 values: L log2(K) may exceed 64 bits.
#include "gr_common.h"

namespace gr {

constexpr uint32_t kEmptySlot = 0xFFFFFFFFu;
constexpr int32_t kMaxCodeLevels = 16;
constexpr int64_t kMinCodeSlots = 1024;

__device__ __forceinline__ uint64_t code_hash(const int64_t* __restrict__ c, int L) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int l = 0; l < L; ++l) {
    h = (h ^ (uint64_t)c[l]) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
  }
  h *= 0x94D049BB133111EBull;
  return h ^ (h >> 32);
}

__device__ __forceinline__ bool code_eq(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int L) {
  bool eq = true;
  for (int l = 0; l < L; ++l) eq &= a[l] == b[l];
  return eq;
}

// table[0 .. slots) = {row = empty, counter = 0}; keys[0 .. n) = INT64_MAX; stats[0 .. 4) = 0.
__global__ __launch_bounds__(256) void code_init_kernel(uint64_t* __restrict__ table, int64_t slots,
                                                        int64_t* __restrict__ keys, int64_t n,
                                                        int64_t* __restrict__ stats) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  for (int64_t i = i0; i < slots; i += step) table[i] = (uint64_t)kEmptySlot;   // low word: the row
  for (int64_t i = i0; i < n; i += step) keys[i] = INT64_MAX;
  if (i0 < 4) stats[i0] = 0;
}

__global__ __launch_bounds__(256) void code_build_kernel(const int64_t* __restrict__ codes, int64_t n, int L,
                                                         uint32_t* table, uint64_t mask) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int64_t* c = codes + r * L;
  uint64_t h = code_hash(c, L) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
    uint32_t* slot = table + 2 * h;
    // a plain read first: a stale "empty" is settled by the compare-and-swap, a stale row still
    // names the slot's code and is >= the slot's current row
    uint32_t prev = *slot;
    if (prev == kEmptySlot) prev = atomicCAS(slot, kEmptySlot, (uint32_t)r);
    if (prev != kEmptySlot) {
      if (prev >= n || !code_eq(c, codes + (int64_t)prev * L, L)) continue;
      if ((uint32_t)r < prev) atomicMin(slot, (uint32_t)r);
    }
    atomicAdd(slot + 1, 1u);
    return;
  }
}

// stats: [0] distinct codes, [1] largest count, [2] rows of shared codes (M; the key cursor),
// [3] shared codes (G).
__global__ __launch_bounds__(256) void code_lookup_kernel(const int64_t* __restrict__ codes, int64_t n, int L,
                                                          const uint32_t* __restrict__ table, uint64_t mask,
                                                          int64_t* __restrict__ leader, int64_t* __restrict__ count,
                                                          int64_t* __restrict__ digit, int64_t* __restrict__ keys,
                                                          unsigned long long* __restrict__ stats) {
  __shared__ uint32_t part[4][4];
  __shared__ unsigned long long key_base;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = r < n;
  uint32_t lead = (uint32_t)r, cnt = live ? 1u : 0u;
  if (live) {
    const int64_t* c = codes + r * L;
    uint64_t h = code_hash(c, L) & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
      const uint32_t s = table[2 * h];
      if (s == kEmptySlot || s >= n) break;   // cannot happen after the build: every row is in the table
      if (code_eq(c, codes + (int64_t)s * L, L)) {
        lead = s;
        cnt = table[2 * h + 1];
        break;
      }
    }
    leader[r] = lead;
    count[r] = cnt;
    digit[r] = 0;
  }
  const bool first = live && lead == (uint32_t)r, shared = live && cnt > 1;
  const uint64_t bf = __ballot(first), bs = __ballot(shared), bg = __ballot(first && shared);
  uint32_t mx = cnt;
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t v = __shfl_xor(mx, o);
    mx = v > mx ? v : mx;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[wave][0] = __popcll(bf);
    part[wave][1] = __popcll(bs);
    part[wave][2] = __popcll(bg);
    part[wave][3] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t d = 0, m = 0, g = 0, x = 0;
    for (int w = 0; w < 4; ++w) {
      d += part[w][0];
      m += part[w][1];
      g += part[w][2];
      x = part[w][3] > x ? part[w][3] : x;
    }
    if (d) atomicAdd(stats + 0, (unsigned long long)d);
    if (x) atomicMax(stats + 1, (unsigned long long)x);
    key_base = m ? atomicAdd(stats + 2, (unsigned long long)m) : 0ull;
    if (g) atomicAdd(stats + 3, (unsigned long long)g);
  }
  __syncthreads();
  if (shared) {
    uint64_t at = key_base + __popcll(bs & ((1ull << lane) - 1));
    for (int w = 0; w < wave; ++w) at += part[w][1];
    if (at < (uint64_t)n) keys[at] = (int64_t)(((uint64_t)lead << 32) | (uint32_t)r);
  }
}

// Inclusive scan over the workgroup's 256 (c, last) pairs: c adds, last takes the maximum.  On
// return sh[.][255] holds the workgroup's totals.
__device__ __forceinline__ void block_scan_pair(int32_t& c, int32_t& last, int32_t (*sh)[256]) {
  const int t = threadIdx.x;
  sh[0][t] = c;
  sh[1][t] = last;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    int32_t pc = 0, pl = -1;
    if (t >= o) {
      pc = sh[0][t - o];
      pl = sh[1][t - o];
    }
    __syncthreads();
    c += pc;
    last = pl > last ? pl : last;
    sh[0][t] = c;
    sh[1][t] = last;
    __syncthreads();
  }
}

// Entry i of the sorted keys: is it one of the m real keys, and does it start a segment?
struct SegItem {
  bool valid, start;
  uint32_t row;
};
__device__ __forceinline__ SegItem seg_item(const int64_t* __restrict__ sorted, int64_t i, int64_t m) {
  SegItem it{i < m, false, 0u};
  if (it.valid) {
    const uint64_t key = (uint64_t)sorted[i];
    it.row = (uint32_t)key;
    it.start = (uint32_t)(key >> 32) == it.row;
  }
  return it;
}

__device__ __forceinline__ int64_t seg_m(const int64_t* __restrict__ stats, int64_t n) {
  const int64_t m = stats[2];
  return m < 0 ? 0 : (m > n ? n : m);
}

// part[b] = (segment starts in block b's 256 entries, index of the last of them or -1)
__global__ __launch_bounds__(256) void seg_reduce_kernel(const int64_t* __restrict__ sorted, int64_t n,
                                                         const int64_t* __restrict__ stats,
                                                         int32_t* __restrict__ part) {
  __shared__ int32_t sh[2][256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const SegItem it = seg_item(sorted, i, seg_m(stats, n));
  int32_t c = it.start ? 1 : 0, last = it.start ? (int32_t)i : -1;
  block_scan_pair(c, last, sh);
  if (threadIdx.x == 255) {
    part[2 * (int64_t)blockIdx.x] = c;
    part[2 * (int64_t)blockIdx.x + 1] = last;
  }
}

// part[b] = the totals over the blocks before b (exclusive scan, in place); one workgroup.
__global__ __launch_bounds__(256) void seg_scan_kernel(int32_t* __restrict__ part, int64_t nb) {
  __shared__ int32_t sh[2][256];
  int32_t carry_c = 0, carry_last = -1;
  for (int64_t b0 = 0; b0 < nb; b0 += 256) {
    const int64_t b = b0 + threadIdx.x;
    const int32_t own_c = b < nb ? part[2 * b] : 0, own_last = b < nb ? part[2 * b + 1] : -1;
    int32_t c = own_c, last = own_last;
    block_scan_pair(c, last, sh);
    if (b < nb) {
      const int32_t before = threadIdx.x ? sh[1][threadIdx.x - 1] : -1;
      part[2 * b] = carry_c + c - own_c;
      part[2 * b + 1] = before > carry_last ? before : carry_last;
    }
    carry_c += sh[0][255];
    carry_last = sh[1][255] > carry_last ? sh[1][255] : carry_last;
    __syncthreads();
  }
}

// rows[i] = the row of sorted key i (-1 past the m keys); digit[row] = i - its segment's start;
// sizes[g] = count[leader] at the g-th start.
__global__ __launch_bounds__(256) void seg_write_kernel(const int64_t* __restrict__ sorted, int64_t n,
                                                        const int64_t* __restrict__ stats,
                                                        const int64_t* __restrict__ count,
                                                        const int32_t* __restrict__ part,
                                                        int64_t* __restrict__ rows, int64_t* __restrict__ sizes,
                                                        int64_t* __restrict__ digit) {
  __shared__ int32_t sh[2][256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const SegItem it = seg_item(sorted, i, seg_m(stats, n));
  int32_t c = it.start ? 1 : 0, last = it.start ? (int32_t)i : -1;
  block_scan_pair(c, last, sh);
  const int32_t g = part[2 * (int64_t)blockIdx.x] + c - 1;
  const int32_t before = part[2 * (int64_t)blockIdx.x + 1];
  const int32_t start = last > before ? last : before;
  if (i >= n) return;
  if (!it.valid) {
    rows[i] = -1;
    return;
  }
  rows[i] = it.row;
  if (it.row < n && start >= 0) {
    digit[it.row] = i - start;
    if (it.start && g >= 0 && g < (n >> 1)) sizes[g] = count[it.row];
  }
}

static int64_t code_slots(int64_t n) {
  int64_t t = kMinCodeSlots;
  while (t < 2 * n) t <<= 1;
  return t;
}

static bool code_shape_ok(int64_t n, int32_t levels) {
  return n >= 0 && n < (int64_t(1) << 31) && levels >= 1 && levels <= kMaxCodeLevels;
}

}  // namespace gr

extern "C" size_t gr_code_groups_workspace_bytes(int64_t n, int32_t levels) {
  if (!gr::code_shape_ok(n, levels)) return 0;
  return (size_t)gr::code_slots(n) * 8;
}

extern "C" int gr_code_groups_i64(const int64_t* codes, int64_t n, int32_t levels, int64_t* leader,
                                  int64_t* count, int64_t* digit, int64_t* keys, int64_t* stats,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  gr::clear_error();
  if (!gr::code_shape_ok(n, levels))
    return gr::fail(GR_ERR_ARG, "gr_code_groups_i64: bad shape (0 <= n < 2^31, 1 <= levels <= 16)");
  if (n == 0) return GR_OK;
  if (!codes || !leader || !count || !digit || !keys || !stats || !workspace)
    return gr::fail(GR_ERR_ARG, "gr_code_groups_i64: null pointer");
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
    return gr::fail(GR_ERR_ARG, "gr_code_groups_i64: workspace must be 8-byte aligned");
  const int64_t slots = gr::code_slots(n);
  if (workspace_bytes < (size_t)slots * 8)
    return gr::fail(GR_ERR_WORKSPACE, "gr_code_groups_i64: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned row_blocks = (unsigned)((n + 255) / 256);
  int64_t init_blocks = (slots + 255) / 256;
  if (init_blocks > 4096) init_blocks = 4096;
  hipLaunchKernelGGL(gr::code_init_kernel, dim3((unsigned)init_blocks), dim3(256), 0, st,
                     reinterpret_cast<uint64_t*>(workspace), slots, keys, n, stats);
  hipLaunchKernelGGL(gr::code_build_kernel, dim3(row_blocks), dim3(256), 0, st, codes, n, (int)levels,
                     reinterpret_cast<uint32_t*>(workspace), (uint64_t)(slots - 1));
  hipLaunchKernelGGL(gr::code_lookup_kernel, dim3(row_blocks), dim3(256), 0, st, codes, n, (int)levels,
                     reinterpret_cast<const uint32_t*>(workspace), (uint64_t)(slots - 1), leader, count, digit,
                     keys, reinterpret_cast<unsigned long long*>(stats));
  return gr::check_launch("gr_code_groups_i64");
}

extern "C" int gr_code_segments_i64(const int64_t* sorted_keys, int64_t n, const int64_t* stats,
                                    const int64_t* count, int64_t* rows, int64_t* sizes, int64_t* digit,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  gr::clear_error();
  if (n < 0 || n >= (int64_t(1) << 31))
    return gr::fail(GR_ERR_ARG, "gr_code_segments_i64: bad shape (0 <= n < 2^31)");
  if (n == 0) return GR_OK;
  if (!sorted_keys || !stats || !count || !rows || !sizes || !digit || !workspace)
    return gr::fail(GR_ERR_ARG, "gr_code_segments_i64: null pointer");
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
    return gr::fail(GR_ERR_ARG, "gr_code_segments_i64: workspace must be 8-byte aligned");
  const int64_t nb = (n + 255) / 256;
  if (workspace_bytes < (size_t)nb * 8)
    return gr::fail(GR_ERR_WORKSPACE, "gr_code_segments_i64: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int32_t* part = reinterpret_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(gr::seg_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, sorted_keys, n, stats, part);
  hipLaunchKernelGGL(gr::seg_scan_kernel, dim3(1), dim3(256), 0, st, part, nb);
  hipLaunchKernelGGL(gr::seg_write_kernel, dim3((unsigned)nb), dim3(256), 0, st, sorted_keys, n, stats, count,
                     part, rows, sizes, digit);
  return gr::check_launch("gr_code_segments_i64");
}
