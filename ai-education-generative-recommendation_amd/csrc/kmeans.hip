// Codebook k-means init on the device (replaces RQ-VAE/models/layers.py:69-82 kmeans(), the
// scikit-learn KMeans(n_clusters, max_iter) call behind vq.py:39-47 init_emb): greedy k-means++
// seeding, Lloyd iterations with scikit-learn's empty-cluster relocation and both of its stop
// rules, for fp32 rows x[n, e], 1 <= e <= 64, 1 <= K <= 1024, K <= n < 2^31.
//
// Distances are the direct form sum_f (x_f - c_f)^2 (one fp32 fma chain over f ascending), which
// has no cancellation under a common offset of the rows; the label is the first index of the
// minimum.  Everything that is summed across rows -- seeding potentials and the cumulative D^2,
// member sums, the centre shift, the inertia -- is summed in fp64 in an order that depends on the
// shape only: no float atomics anywhere (the only atomic is an integer OR of "a label changed").
//
// The work is cut into phases (pick / eval for seeding; assign / sums / reduce / update for Lloyd; finish).
// Each phase is a __device__ function over a tile of 256 rows, a (cluster, row range) work item or
// the whole problem.  The tiled form launches one kernel per phase (a grid over tiles; iterations
// after convergence see ctl->done and return).  The one-workgroup form runs the same phase functions
// in one launch with the rows and the whole workspace carved from LDS, so the two forms compute
// bit for bit the same values.
#include <cmath>

#include "gr_common.h"

namespace gr {

constexpr int KM_T = 256;      // threads per workgroup = rows per tile
constexpr int KM_MAXTR = 16;   // candidates per seeding round (2 + floor(ln 1024) = 8)
constexpr int KM_MAXS = 1024;  // workgroups of the variance pass
constexpr size_t KM_SMALL_LDS = 112 * 1024;   // dynamic LDS of the one-workgroup form (+ KmScr static)

struct KmCtl {
  int32_t done, n_iter, changed, pad;
  double thr;   // tol * mean over features of var(x)
};

struct KmWs {
  KmCtl* ctl;
  int32_t* cand;   // [2][KM_MAXTR] candidate rows of this / the previous seeding round
  float* cpad;     // [K][EP] current centres, zero padded to EP features
  float* d2;       // [n] squared distance to the nearest chosen centre (seeding)
  int32_t* lab;    // [n] labels of the previous E step
  float* mind;     // [n] squared distance to the assigned centre
  double* tpot;    // [KM_MAXTR][T] per-tile potential of each candidate; [T] per-tile inertia
  double* psum;    // [K * P][EP] member sums per (cluster, row range)
  int32_t* pcnt;   // [K * P] member counts
  double* pstat;   // [S][2][EP] sums of (x - x_0) and (x - x_0)^2
};

struct KmShape {
  int64_t n;
  int32_t e, K, xs;   // xs: row stride of x (e in global memory, e | 1 in LDS)
  int32_t T, P, S;    // row tiles; row ranges per cluster in the M step; variance workgroups
  int32_t vec;        // rows of x are 16-byte aligned (e % 4 == 0): a thread reads its row as float4s
};

// Scratch of one workgroup (static LDS).
struct KmScr {
  double red[KM_T];
  double red2[KM_T];
  double cp[KM_T + 1];
  float tile[KM_MAXTR][KM_T];
  float cnd[KM_MAXTR][64];
  int32_t emp[1024];
  int32_t cntl[1024];
  float rd[KM_T];
  int32_t ri[KM_T];
  double pots[KM_MAXTR];
  int32_t sel_tile[KM_MAXTR];
  double sel_base[KM_MAXTR], sel_pc[KM_MAXTR];
  int32_t misc[8];
};

__host__ __device__ inline size_t km_carve(char* base, const KmShape& s, int EP, KmWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += (bytes + 15) / 16 * 16;
    return p;
  };
  KmWs t;
  t.ctl = reinterpret_cast<KmCtl*>(take(sizeof(KmCtl)));
  t.cand = reinterpret_cast<int32_t*>(take(2 * KM_MAXTR * 4));
  t.cpad = reinterpret_cast<float*>(take((size_t)s.K * EP * 4));
  t.d2 = reinterpret_cast<float*>(take((size_t)s.n * 4));
  t.lab = reinterpret_cast<int32_t*>(take((size_t)s.n * 4));
  t.mind = reinterpret_cast<float*>(take((size_t)s.n * 4));
  t.tpot = reinterpret_cast<double*>(take((size_t)KM_MAXTR * s.T * 8));
  t.psum = reinterpret_cast<double*>(take((size_t)s.K * s.P * EP * 8));
  t.pcnt = reinterpret_cast<int32_t*>(take((size_t)s.K * s.P * 4));
  t.pstat = reinterpret_cast<double*>(take((size_t)s.S * 2 * EP * 8));
  if (w) *w = t;
  return off;
}

inline int km_ep(int e) { return e <= 8 ? 8 : e <= 16 ? 16 : e <= 32 ? 32 : 64; }

inline KmShape km_shape(int64_t n, int e, int K) {
  KmShape s;
  s.n = n, s.e = e, s.K = K, s.xs = e;
  s.T = (int32_t)((n + KM_T - 1) / KM_T);
  const int64_t blocks = (n + 63) / 64;
  int64_t P = (8192 + K - 1) / K;
  P = P > 128 ? 128 : P;
  P = P > blocks ? blocks : P;
  s.P = (int32_t)(P < 1 ? 1 : P);
  s.S = s.T < KM_MAXS ? s.T : KM_MAXS;
  s.vec = 0;
  return s;
}

// Uniform in [0, 1): a function of (seed, round, trial) only (gr_common.h mix64).
__device__ __forceinline__ double km_u01(uint64_t seed, int round, int trial) {
  const uint64_t h = mix64(mix64(seed ^ mix64((uint64_t)round)) + (uint64_t)trial);
  return (double)(h >> 11) * 0x1.0p-53;
}

template <int EP>
__device__ __forceinline__ void km_load_row(const float* x, int64_t row, const KmShape& s, float (&xr)[EP]) {
  const float* p = x + row * s.xs;
  if (s.vec) {   // a lane per row touches 64 cache lines per load instruction: make the loads wide
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int q = 0; q < EP / 4; ++q) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (4 * q < s.e) v = p4[q];
      xr[4 * q] = v[0], xr[4 * q + 1] = v[1], xr[4 * q + 2] = v[2], xr[4 * q + 3] = v[3];
    }
    return;
  }
#pragma unroll
  for (int f = 0; f < EP; ++f) xr[f] = f < s.e ? p[f] : 0.f;
}

// sum_f (x_f - c_f)^2, one fma chain over f ascending; c is padded to EP (padding adds exact zeros).
template <int EP>
__device__ __forceinline__ float km_dist2(const float (&xr)[EP], const float* c) {
  float d = 0.f;
#pragma unroll
  for (int f = 0; f < EP; ++f) {
    const float t = xr[f] - c[f];
    d = fmaf(t, t, d);
  }
  return d;
}

// Fixed-shape tree sum over the workgroup's 256 values.
__device__ __forceinline__ double km_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = KM_T / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- start: clear the control block, labels of "no previous E step", the given centres ----------
template <int EP>
__device__ void km_ph_start(const KmWs& w, const KmShape& s, const float* init, bool fill_labels) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    KmCtl c = {};
    *w.ctl = c;
  }
  if (init)
    for (int i = tid; i < s.K * EP; i += KM_T) {
      const int k = i / EP, f = i % EP;
      w.cpad[i] = f < s.e ? init[(size_t)k * s.e + f] : 0.f;
    }
  if (fill_labels)
    for (int64_t i = tid; i < s.n; i += KM_T) w.lab[i] = -1;
}

// ---- seeding, round r: settle round r - 1's best candidate as centre r - 1, draw round r's --------
// Round 0 draws one uniform row.  A later round draws `ntr` rows with probability proportional to
// D^2 = min over chosen centres of the squared distance.  The cumulative D^2 is the three-level sum
//   cp[chunk] + (pc[tile in chunk] + run[row in tile]),
// every level a sequential fp64 sum from zero whose last value IS the next level's addend (the tile
// totals are the eval phase's sequential sums of the same fp32 values).  Sequential sums of
// non-negative terms never decrease, so "the first row whose cumulative sum exceeds u * total"
// exists at every level, and its own D^2 is positive: a row that coincides with a chosen centre is
// never drawn while another row is left.
template <int EP>
__device__ void km_ph_pick(const KmWs& w, const KmShape& s, const float* x, uint64_t seed, int r, int ntr_prev,
                           int ntr, KmScr& scr) {
  const int tid = threadIdx.x;
  const int T = s.T;
  if (r >= 1) {
    for (int t = tid >> 6; t < ntr_prev; t += KM_T / 64) {   // one wavefront per candidate, fixed butterfly
      double v = 0.0;
      for (int j = tid & 63; j < T; j += 64) v += w.tpot[(size_t)t * T + j];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((tid & 63) == 0) scr.pots[t] = v;
    }
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      for (int t = 1; t < ntr_prev; ++t)
        if (scr.pots[t] < scr.pots[best]) best = t;
      scr.misc[0] = best;
      scr.misc[1] = w.cand[((r - 1) & 1) * KM_MAXTR + best];
    }
    __syncthreads();
    const int64_t row = scr.misc[1];
    if (tid < EP) w.cpad[(size_t)(r - 1) * EP + tid] = tid < s.e ? x[row * s.xs + tid] : 0.f;
    __syncthreads();
  }
  if (r == s.K) return;
  if (r == 0) {
    if (tid == 0) {
      int64_t i = (int64_t)(km_u01(seed, 0, 0) * (double)s.n);
      w.cand[0] = (int32_t)(i < s.n ? i : s.n - 1);
    }
    return;
  }
  const double* tt = w.tpot + (size_t)scr.misc[0] * T;
  const int chunk = (T + KM_T - 1) / KM_T, nch = (T + chunk - 1) / chunk;
  {
    double v = 0.0;
    const int j0 = tid * chunk;
    for (int j = j0; j < j0 + chunk && j < T; ++j) v += tt[j];
    scr.red2[tid] = v;
  }
  if (tid < KM_MAXTR) scr.sel_tile[tid] = 0, scr.sel_base[tid] = 0.0, scr.sel_pc[tid] = 0.0;   // (NaN rows: no chunk matches)
  __syncthreads();
  if (tid == 0) {
    scr.cp[0] = 0.0;
    for (int c = 0; c < nch; ++c) scr.cp[c + 1] = scr.cp[c] + scr.red2[c];
  }
  __syncthreads();
  const double total = scr.cp[nch];
  const float* cprev = w.cpad + (size_t)(r - 1) * EP;
  if (!(total > 0.0)) {   // every row coincides with a chosen centre: uniform rows
    if (tid < ntr) {
      const int64_t i = (int64_t)(km_u01(seed, r, tid) * (double)s.n);
      w.cand[(r & 1) * KM_MAXTR + tid] = (int32_t)(i < s.n ? i : s.n - 1);
    }
    return;
  }
  for (int t = 0; t < ntr; ++t) {   // the chunk, then the tile in it (one thread finds each)
    double val = km_u01(seed, r, t) * total;
    if (!(val < total)) val = 0.0;
    if (tid < nch && scr.cp[tid + 1] > val && scr.cp[tid] <= val) {
      const double base = scr.cp[tid];
      double pc = 0.0;
      int sel = -1;
      const int j0 = tid * chunk;
      for (int j = j0; j < j0 + chunk && j < T; ++j) {
        if (base + (pc + tt[j]) > val) {
          sel = j;
          break;
        }
        pc += tt[j];
      }
      scr.sel_tile[t] = sel < 0 ? j0 : sel;
      scr.sel_base[t] = base;
      scr.sel_pc[t] = pc;
    }
  }
  __syncthreads();
  for (int t = 0; t < ntr; ++t) {   // that tile's current D^2, as the eval phase formed it
    const int64_t row = (int64_t)scr.sel_tile[t] * KM_T + tid;
    float v = 0.f;
    if (row < s.n) {
      float xr[EP];
      km_load_row<EP>(x, row, s, xr);
      const float d = km_dist2<EP>(xr, cprev);
      v = r == 1 ? d : fminf(w.d2[row], d);
    }
    scr.tile[t][tid] = v;
  }
  __syncthreads();
  if (tid < ntr) {
    double val = km_u01(seed, r, tid) * total;
    if (!(val < total)) val = 0.0;
    const double base = scr.sel_base[tid], pc = scr.sel_pc[tid];
    const int64_t row0 = (int64_t)scr.sel_tile[tid] * KM_T;
    double run = 0.0;
    int sel = -1;
    const int lim = s.n - row0 < KM_T ? (int)(s.n - row0) : KM_T;   // (the rows past n add exact zeros)
#pragma unroll 8
    for (int i = 0; i < lim; ++i) {   // no early exit: the LDS reads run ahead of the fp64 chain
      run += (double)scr.tile[tid][i];
      sel = (sel < 0 && base + (pc + run) > val) ? i : sel;
    }
    int64_t row = row0 + (sel < 0 ? 0 : sel);
    if (row >= s.n) row = s.n - 1;
    w.cand[(r & 1) * KM_MAXTR + tid] = (int32_t)row;
  }
}

// ---- seeding, round r, one tile: apply centre r - 1 to D^2, then every candidate's potential ------
template <int EP>
__device__ void km_ph_eval(const KmWs& w, const KmShape& s, const float* x, int r, int ntr, int tile, KmScr& scr) {
  const int tid = threadIdx.x;
  for (int i = tid; i < ntr * EP; i += KM_T) {
    const int t = i / EP, f = i % EP;
    const int64_t cr = w.cand[(r & 1) * KM_MAXTR + t];
    scr.cnd[t][f] = f < s.e ? x[cr * s.xs + f] : 0.f;
  }
  __syncthreads();
  const int64_t row = (int64_t)tile * KM_T + tid;
  if (row < s.n) {
    float xr[EP];
    km_load_row<EP>(x, row, s, xr);
    float dcur = INFINITY;
    if (r >= 1) {
      const float d = km_dist2<EP>(xr, w.cpad + (size_t)(r - 1) * EP);
      dcur = r == 1 ? d : fminf(w.d2[row], d);
      w.d2[row] = dcur;
    }
    for (int t = 0; t < ntr; ++t) scr.tile[t][tid] = fminf(dcur, km_dist2<EP>(xr, scr.cnd[t]));
  } else {
    for (int t = 0; t < ntr; ++t) scr.tile[t][tid] = 0.f;
  }
  __syncthreads();
  if (tid < ntr) {
    double run = 0.0;
    for (int i = 0; i < KM_T; ++i) run += (double)scr.tile[tid][i];
    w.tpot[(size_t)tid * s.T + tile] = run;
  }
  __syncthreads();
}

// ---- E step, one tile: label = first index of the minimum squared distance ------------------------
template <int EP>
__device__ void km_ph_assign(const KmWs& w, const KmShape& s, const float* x, int tile, bool final,
                             int64_t* labels_out, KmScr& scr) {
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)tile * KM_T + tid;
  float best = INFINITY;
  bool moved = false;
  if (row < s.n) {
    float xr[EP];
    km_load_row<EP>(x, row, s, xr);
    int bk = 0;
    for (int k = 0; k < s.K; ++k) {
      const float d = km_dist2<EP>(xr, w.cpad + (size_t)k * EP);
      if (d < best) best = d, bk = k;
    }
    if (final) {
      if (labels_out) labels_out[row] = bk;
    } else {
      moved = w.lab[row] != bk;
      w.lab[row] = bk;
      w.mind[row] = best;
    }
  }
  if (__ballot(moved) != 0 && (tid & 63) == 0) atomicOr(&w.ctl->changed, 1);   // one per wavefront
  if (final) {
    const double tot = km_block_sum(row < s.n ? (double)best : 0.0, scr.red);
    if (tid == 0) w.tpot[tile] = tot;
  }
}

// ---- M step, work item (cluster k, row range p), one wavefront: members in ascending row order ----
__device__ void km_ph_sums(const KmWs& w, const KmShape& s, const float* x, int item, int EP) {
  const int lane = threadIdx.x & 63;
  const int k = item / s.P, p = item % s.P;
  const int64_t per = ((s.n + s.P - 1) / s.P + 63) / 64 * 64;
  const int64_t r0 = (int64_t)p * per, r1 = r0 + per < s.n ? r0 + per : s.n;
  double acc = 0.0;
  int c = 0;
  for (int64_t b = r0; b < r1; b += 64) {
    const int64_t row = b + lane;
    const bool m = row < r1 && w.lab[row] == k;
    uint64_t mask = __ballot(m);
    c += __popcll(mask);
    while (mask) {
      const int i = __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      if (lane < s.e) acc += (double)x[(b + i) * s.xs + lane];
    }
  }
  if (lane < EP) w.psum[(size_t)item * EP + lane] = lane < s.e ? acc : 0.0;
  if (lane == 0) w.pcnt[item] = c;
}

// ---- M step, element i = (cluster, feature): the total over the row ranges, ascending, into range 0's slot
__device__ __forceinline__ void km_ph_reduce(const KmWs& w, const KmShape& s, int i, int EP) {
  const int k = i / EP, f = i % EP;
  double v = 0.0;
  for (int p = 0; p < s.P; ++p) v += w.psum[((size_t)k * s.P + p) * EP + f];
  w.psum[((size_t)k * s.P) * EP + f] = v;
}

// ---- M step, whole problem: empty-cluster relocation, new centres, both stop rules ---------
// scikit-learn's _relocate_empty_clusters_dense with the pairing fixed: the empty clusters in
// ascending id; the j-th takes the j-th farthest row (squared distance to its assigned old centre,
// descending, ties to the lower row), which leaves its donor's sum and count.  A cluster whose
// count ends at 0 keeps its old centre.
__device__ void km_ph_update(const KmWs& w, const KmShape& s, const float* x, int it, int EP, KmScr& scr) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int K = s.K, P = s.P;
  for (int k = tid; k < K; k += KM_T) {
    int c = 0;
    for (int p = 0; p < P; ++p) c += w.pcnt[(size_t)k * P + p];
    scr.cntl[k] = c;
  }
  __syncthreads();
  if (tid < 64) {   // the empty clusters in ascending id
    int m = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane;
      const bool em = k < K && scr.cntl[k] == 0;
      const uint64_t mask = __ballot(em);
      if (em) scr.emp[m + __popcll(mask & ((1ull << lane) - 1))] = k;
      m += __popcll(mask);
    }
    if (lane == 0) scr.misc[2] = m;
  }
  __syncthreads();
  const int nemp = scr.misc[2];
  float pd = INFINITY;   // the previous pick: the next one comes after it in (distance desc, row asc)
  int64_t pi = -1;
  for (int j = 0; j < nemp; ++j) {
    float bd = -1.f;
    int64_t bi = -1;
    for (int64_t i = tid; i < s.n; i += KM_T) {
      const float d = w.mind[i];
      const bool after = d < pd || (d == pd && i > pi);
      if (after && (d > bd || bi < 0)) bd = d, bi = i;   // rows ascend per thread: ties keep the lower row
    }
    scr.rd[tid] = bd;
    scr.ri[tid] = (int32_t)bi;
    __syncthreads();
    for (int st = KM_T / 2; st > 0; st >>= 1) {
      if (tid < st) {
        const float d2 = scr.rd[tid + st];
        const int32_t i2 = scr.ri[tid + st];
        const float d1 = scr.rd[tid];
        const int32_t i1 = scr.ri[tid];
        if (i2 >= 0 && (i1 < 0 || d2 > d1 || (d2 == d1 && i2 < i1))) scr.rd[tid] = d2, scr.ri[tid] = i2;
      }
      __syncthreads();
    }
    pd = scr.rd[0];
    pi = scr.ri[0];
    __syncthreads();
    if (pi < 0) break;
    const int donor = w.lab[pi], to = scr.emp[j];
    if (tid < EP) {
      const double v = tid < s.e ? (double)x[pi * s.xs + tid] : 0.0;
      w.psum[((size_t)donor * P) * EP + tid] -= v;
      w.psum[((size_t)to * P) * EP + tid] = v;
    }
    if (tid == 0) {
      scr.cntl[donor] -= 1;
      scr.cntl[to] = 1;
    }
    __syncthreads();
  }
  double sh = 0.0;
  for (int i = tid; i < K * EP; i += KM_T) {
    const int k = i / EP, f = i % EP;
    const int c = scr.cntl[k];
    const float old = w.cpad[i];
    const float nw = c > 0 ? (float)(w.psum[((size_t)k * P) * EP + f] / (double)c) : old;
    const double dl = (double)nw - (double)old;
    sh += dl * dl;
    w.cpad[i] = nw;
  }
  const double shift = km_block_sum(sh, scr.red);
  if (tid == 0) {
    w.ctl->n_iter = it + 1;
    if (w.ctl->changed == 0 || shift <= w.ctl->thr) w.ctl->done = 1;
    w.ctl->changed = 0;
  }
  __syncthreads();
}

// ---- tolerance: thr = tol * mean over features of var(x), from sums shifted by row 0 --------------
__device__ void km_ph_stats(const KmWs& w, const KmShape& s, const float* x, int sidx, int EP, KmScr& scr) {
  const int tid = threadIdx.x, f = tid % EP, g = tid / EP, G = KM_T / EP;
  double s1 = 0.0, s2 = 0.0;
  if (f < s.e) {
    const double x0 = (double)x[f];
    for (int64_t t = sidx; t < s.T; t += s.S) {
      const int64_t r1 = (t + 1) * KM_T < s.n ? (t + 1) * KM_T : s.n;
      for (int64_t row = t * KM_T + g; row < r1; row += G) {
        const double v = (double)x[row * s.xs + f] - x0;
        s1 += v;
        s2 += v * v;
      }
    }
  }
  scr.red[tid] = s1;
  scr.red2[tid] = s2;
  __syncthreads();
  if (g == 0) {
    for (int q = 1; q < G; ++q) s1 += scr.red[q * EP + f], s2 += scr.red2[q * EP + f];
    w.pstat[((size_t)sidx * 2) * EP + f] = s1;
    w.pstat[((size_t)sidx * 2 + 1) * EP + f] = s2;
  }
  __syncthreads();
}

__device__ void km_ph_stats_fin(const KmWs& w, const KmShape& s, double tol, int EP, KmScr& scr) {
  const int tid = threadIdx.x;
  double var = 0.0;
  if (tid < s.e) {
    double s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < s.S; ++q) {
      s1 += w.pstat[((size_t)q * 2) * EP + tid];
      s2 += w.pstat[((size_t)q * 2 + 1) * EP + tid];
    }
    const double m = s1 / (double)s.n;
    var = s2 / (double)s.n - m * m;
    if (var < 0.0) var = 0.0;
  }
  const double tot = km_block_sum(var, scr.red);
  if (tid == 0) w.ctl->thr = tol * (tot / (double)s.e);
}

// ---- outputs ---------------------------------------------------------------------------------------
__device__ void km_ph_finish(const KmWs& w, const KmShape& s, int EP, float* centers_out, double* inertia_out,
                             int32_t* n_iter_out, KmScr& scr) {
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int j = tid; j < s.T; j += KM_T) v += w.tpot[j];
  const double tot = km_block_sum(v, scr.red);
  if (tid == 0) {
    if (inertia_out) *inertia_out = tot;
    if (n_iter_out) *n_iter_out = w.ctl->n_iter;
  }
  for (int i = tid; i < s.K * s.e; i += KM_T) centers_out[i] = w.cpad[(size_t)(i / s.e) * EP + i % s.e];
}

// ================================ tiled form: one kernel per phase ===================================
template <int EP>
__global__ __launch_bounds__(KM_T) void km_start_kernel(KmWs w, KmShape s, const float* init) {
  km_ph_start<EP>(w, s, init, false);
}
template <int EP>
__global__ __launch_bounds__(KM_T) void km_pick_kernel(KmWs w, KmShape s, const float* x, uint64_t seed, int r,
                                                       int ntr_prev, int ntr) {
  __shared__ KmScr scr;
  km_ph_pick<EP>(w, s, x, seed, r, ntr_prev, ntr, scr);
}
template <int EP>
__global__ __launch_bounds__(KM_T) void km_eval_kernel(KmWs w, KmShape s, const float* x, int r, int ntr) {
  __shared__ KmScr scr;
  km_ph_eval<EP>(w, s, x, r, ntr, blockIdx.x, scr);
}
template <int EP>
__global__ __launch_bounds__(KM_T) void km_assign_kernel(KmWs w, KmShape s, const float* x, int final,
                                                         int64_t* labels_out) {
  __shared__ KmScr scr;
  if (!final && w.ctl->done) return;
  km_ph_assign<EP>(w, s, x, blockIdx.x, final != 0, labels_out, scr);
}
__global__ __launch_bounds__(KM_T) void km_sums_kernel(KmWs w, KmShape s, const float* x, int EP) {
  if (w.ctl->done) return;
  const int item = blockIdx.x * (KM_T / 64) + (threadIdx.x >> 6);
  if (item < s.K * s.P) km_ph_sums(w, s, x, item, EP);
}
__global__ __launch_bounds__(KM_T) void km_reduce_kernel(KmWs w, KmShape s, int EP) {
  if (w.ctl->done) return;
  const int i = blockIdx.x * KM_T + threadIdx.x;
  if (i < s.K * EP) km_ph_reduce(w, s, i, EP);
}
__global__ __launch_bounds__(KM_T) void km_update_kernel(KmWs w, KmShape s, const float* x, int it, int EP) {
  __shared__ KmScr scr;
  if (w.ctl->done) return;
  km_ph_update(w, s, x, it, EP, scr);
}
__global__ __launch_bounds__(KM_T) void km_stats_kernel(KmWs w, KmShape s, const float* x, int EP) {
  __shared__ KmScr scr;
  km_ph_stats(w, s, x, blockIdx.x, EP, scr);
}
__global__ __launch_bounds__(KM_T) void km_stats_fin_kernel(KmWs w, KmShape s, double tol, int EP) {
  __shared__ KmScr scr;
  km_ph_stats_fin(w, s, tol, EP, scr);
}
__global__ __launch_bounds__(KM_T) void km_finish_kernel(KmWs w, KmShape s, int EP, float* centers_out,
                                                         double* inertia_out, int32_t* n_iter_out) {
  __shared__ KmScr scr;
  km_ph_finish(w, s, EP, centers_out, inertia_out, n_iter_out, scr);
}

// ============================ one-workgroup form: the whole run in one launch ========================
// The rows (stride e | 1: a thread per row reads without bank conflicts) and the workspace live in
// LDS; the phases are the tiled form's, separated by workgroup barriers.
template <int EP>
__global__ __launch_bounds__(KM_T) void km_small_kernel(KmShape s, const float* __restrict__ xg, const float* init,
                                                        uint64_t seed, int trials, int max_iter, double tol,
                                                        float* centers_out, int64_t* labels_out,
                                                        double* inertia_out, int32_t* n_iter_out) {
  extern __shared__ __attribute__((aligned(16))) char km_lds[];
  __shared__ KmScr scr;
  const int tid = threadIdx.x;
  char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(km_lds) + 15) & ~(uintptr_t)15);
  const int e = s.e;
  s.xs = e | 1;
  s.vec = 0;
  float* x = reinterpret_cast<float*>(base);
  const size_t xbytes = ((size_t)s.n * s.xs * 4 + 15) / 16 * 16;
  KmWs w;
  km_carve(base + xbytes, s, EP, &w);
  for (int64_t i = tid; i < s.n * e; i += KM_T) x[(i / e) * s.xs + i % e] = xg[i];
  km_ph_start<EP>(w, s, init, true);
  __syncthreads();
  const int T = s.T;
  if (!init) {
    for (int r = 0; r <= s.K; ++r) {
      const int ntr = r == 0 ? 1 : trials, ntr_prev = r == 1 ? 1 : trials;
      km_ph_pick<EP>(w, s, x, seed, r, ntr_prev, ntr, scr);
      __syncthreads();
      if (r == s.K) break;
      for (int t = 0; t < T; ++t) km_ph_eval<EP>(w, s, x, r, ntr, t, scr);
      __syncthreads();
    }
  }
  if (max_iter > 0 && tol > 0.0) {
    for (int q = 0; q < s.S; ++q) km_ph_stats(w, s, x, q, EP, scr);
    __syncthreads();
    km_ph_stats_fin(w, s, tol, EP, scr);
    __syncthreads();
  }
  for (int it = 0; it < max_iter; ++it) {
    for (int t = 0; t < T; ++t) km_ph_assign<EP>(w, s, x, t, false, nullptr, scr);
    __syncthreads();
    for (int item = tid >> 6; item < s.K * s.P; item += KM_T / 64) km_ph_sums(w, s, x, item, EP);
    __syncthreads();
    for (int i = tid; i < s.K * EP; i += KM_T) km_ph_reduce(w, s, i, EP);
    __syncthreads();
    km_ph_update(w, s, x, it, EP, scr);
    __syncthreads();
    if (w.ctl->done) break;
  }
  for (int t = 0; t < T; ++t) km_ph_assign<EP>(w, s, x, t, true, labels_out, scr);
  __syncthreads();
  km_ph_finish(w, s, EP, centers_out, inertia_out, n_iter_out, scr);
}

// The one-workgroup form takes one tile of rows: measured against the tiled form it wins up to there
// (2.3x at (256, 32) K 8, 1.2-1.4x at K 32-64) and loses beyond (0.87x at 600 rows, 0.56-0.63x at
// 1000 rows: every tile and every (cluster, range) item of each Lloyd iteration then runs on one CU).
static bool km_small_fits(const KmShape& s, int EP) {
  if (s.n > KM_T || (int64_t)s.n * s.K * EP > (1 << 20)) return false;
  const size_t xbytes = ((size_t)s.n * (s.e | 1) * 4 + 15) / 16 * 16;
  return 16 + xbytes + km_carve(nullptr, s, EP, nullptr) <= KM_SMALL_LDS;
}

template <int EP>
static int km_run(const float* x, const KmShape& s, const float* init, uint64_t seed, int trials, int max_iter,
                  double tol, float* centers_out, int64_t* labels_out, double* inertia_out, int32_t* n_iter_out,
                  void* workspace, hipStream_t st) {
  if (option("kmeans_small") == 1 && km_small_fits(s, EP)) {
    static bool lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(km_small_kernel<EP>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)KM_SMALL_LDS) == hipSuccess;
    if (!lds_ok) return fail(GR_ERR_HIP, "gr_kmeans_f32: cannot raise the LDS limit");
    hipLaunchKernelGGL(km_small_kernel<EP>, dim3(1), dim3(KM_T), KM_SMALL_LDS, st, s, x, init, seed, trials, max_iter,
                       tol, centers_out, labels_out, inertia_out, n_iter_out);
    return check_launch("gr_kmeans_f32");
  }
  KmWs w;
  km_carve(static_cast<char*>(workspace), s, EP, &w);
  const dim3 blk(KM_T), one(1), tiles((unsigned)s.T);
  hipLaunchKernelGGL(km_start_kernel<EP>, one, blk, 0, st, w, s, init);
  if (int rc = gr_fill32_launch(w.lab, 0xFFFFFFFFu, s.n, st)) return rc;
  if (!init)
    for (int r = 0; r <= s.K; ++r) {
      const int ntr = r == 0 ? 1 : trials, ntr_prev = r == 1 ? 1 : trials;
      hipLaunchKernelGGL(km_pick_kernel<EP>, one, blk, 0, st, w, s, x, seed, r, ntr_prev, ntr);
      if (r < s.K) hipLaunchKernelGGL(km_eval_kernel<EP>, tiles, blk, 0, st, w, s, x, r, ntr);
    }
  if (max_iter > 0 && tol > 0.0) {
    hipLaunchKernelGGL(km_stats_kernel, dim3((unsigned)s.S), blk, 0, st, w, s, x, EP);
    hipLaunchKernelGGL(km_stats_fin_kernel, one, blk, 0, st, w, s, tol, EP);
  }
  const unsigned sums_grid = (unsigned)((s.K * s.P + KM_T / 64 - 1) / (KM_T / 64));
  const unsigned red_grid = (unsigned)((s.K * EP + KM_T - 1) / KM_T);
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(km_assign_kernel<EP>, tiles, blk, 0, st, w, s, x, 0, (int64_t*)nullptr);
    hipLaunchKernelGGL(km_sums_kernel, dim3(sums_grid), blk, 0, st, w, s, x, EP);
    if (s.P > 1) hipLaunchKernelGGL(km_reduce_kernel, dim3(red_grid), blk, 0, st, w, s, EP);
    hipLaunchKernelGGL(km_update_kernel, one, blk, 0, st, w, s, x, it, EP);
  }
  hipLaunchKernelGGL(km_assign_kernel<EP>, tiles, blk, 0, st, w, s, x, 1, labels_out);
  hipLaunchKernelGGL(km_finish_kernel, one, blk, 0, st, w, s, EP, centers_out, inertia_out, n_iter_out);
  return check_launch("gr_kmeans_f32");
}

static bool km_envelope(int64_t n, int32_t e, int32_t K) {
  return e >= 1 && e <= 64 && K >= 1 && K <= 1024 && n <= 0x7fffffffLL;
}

}  // namespace gr

extern "C" size_t gr_kmeans_workspace_bytes(int64_t n, int32_t e, int32_t K) {
  using namespace gr;
  if (n < 1 || !km_envelope(n, e, K) || n < K) return 0;
  return km_carve(nullptr, km_shape(n, e, K), km_ep(e), nullptr);
}

extern "C" int32_t gr_kmeans_form(int64_t n, int32_t e, int32_t K) {
  using namespace gr;
  if (n < 1 || !km_envelope(n, e, K) || n < K) return -1;
  return option("kmeans_small") == 1 && km_small_fits(km_shape(n, e, K), km_ep(e)) ? 1 : 0;
}

extern "C" int gr_kmeans_f32(const float* x, int64_t n, int32_t e, int32_t K, const float* init_centers,
                             uint64_t seed, int32_t trials, int32_t max_iter, double tol, float* centers_out,
                             int64_t* labels_out, double* inertia_out, int32_t* n_iter_out, void* workspace,
                             size_t workspace_bytes, void* stream) {
  using namespace gr;
  clear_error();
  if (n < 0 || e < 1 || K < 1 || max_iter < 0 || trials < 0 || !(tol >= 0.0))
    return fail(GR_ERR_ARG, "gr_kmeans_f32: bad shape or argument");
  if (n < K) return fail(GR_ERR_ARG, "gr_kmeans_f32: n_samples < n_clusters");
  if (!km_envelope(n, e, K))
    return fail(GR_ERR_UNSUPPORTED, "gr_kmeans_f32: outside 1 <= e <= 64, 1 <= K <= 1024, K <= n < 2^31");
  if (trials == 0) trials = 2 + (int)std::floor(std::log((double)K));   // scikit-learn's n_local_trials
  if (trials > KM_MAXTR) return fail(GR_ERR_UNSUPPORTED, "gr_kmeans_f32: more than 16 trials");
  const int EP = km_ep(e);
  KmShape s = km_shape(n, e, K);
  s.vec = (e % 4 == 0 && aligned16(x)) ? 1 : 0;
  const size_t need = km_carve(nullptr, s, EP, nullptr);
  if (!workspace || workspace_bytes < need) return fail(GR_ERR_WORKSPACE, "gr_kmeans_f32: workspace too small");
  if (!aligned16(workspace)) return fail(GR_ERR_ARG, "gr_kmeans_f32: workspace not 16-byte aligned");
  if (!x || !centers_out) return fail(GR_ERR_ARG, "gr_kmeans_f32: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define KM_RUN(E)                                                                                              \
  return km_run<E>(x, s, init_centers, seed, trials, max_iter, tol, centers_out, labels_out, inertia_out, \
                   n_iter_out, workspace, st)
  if (EP == 8) KM_RUN(8);
  if (EP == 16) KM_RUN(16);
  if (EP == 32) KM_RUN(32);
  KM_RUN(64);
#undef KM_RUN
}
