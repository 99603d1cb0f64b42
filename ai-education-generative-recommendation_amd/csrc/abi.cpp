// Library identification and the thread-local error channel of the C ABI (include/gr_amd.h).
#include <atomic>
#include <cstring>
#include <string>

#include "gr_common.h"

namespace gr {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
void clear_error() { g_last_error.clear(); }

int cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = 256;
  }
  return cus;
}

// Path switches (gr_set_option), read by the launchers at each call.  Each selects between two
// kernel paths that give BITWISE the same results (the tests run both), except attn_k16: two fp32
// chains of the hd 128 attention, both tested against the oracle within the logits tolerance.
// Kernel variants measured slower and the options that selected them were removed in round 5
// (DESIGN.md §7 keeps their measurements).
struct Opt {
  const char* name;
  std::atomic<int64_t>* v;
  int64_t lo, hi;
};
// rq_fused (1: the fused persistent encoder kernel when the shape allows, 0: layer-wise kernels)
static std::atomic<int64_t> g_rq_fused{1};
// sas_fused (the fused SASRec forward when n <= 64 and d <= 64: 2 = one or two waves per sequence
// by batch size (two only when n > 32), 3 = two waves whenever n > 32, 1 = one wave per sequence;
// 0: layer-wise kernels)
static std::atomic<int64_t> g_sas_fused{2};
// sas_rowtile (1: d = 128 forwards on the row-tile kernels of sasrec_rowtile.hip, 0: one kernel per op)
static std::atomic<int64_t> g_sas_rowtile{1};
// lin_wres (1: gr_linear_f32 with k = 128, n % 128 == 0, no residual, m >= 96 x 256 keeps 32-column
// slices of w resident in registers, 0: the tiled kernel)
static std::atomic<int64_t> g_lin_wres{1};
// emb_proj (1: the d = 128 forward's block 0 runs embed + LN_a0 + in-projection as one persistent
// kernel, 0: embed_ln then gr_linear_f32)
static std::atomic<int64_t> g_emb_proj{1};
// topk_half (gr_score_topk_f32's tile maxima: 2 = 16-row half tiles where the re-scored bytes saved
// exceed the extra maxima traffic (short catalogs), 32-row tiles otherwise; 1 / 0 = forced)
static std::atomic<int64_t> g_topk_half{2};
// attn_k16 (hd 64 / 128 attention: 1 = 32-query tiles over 16-key steps at two waves per SIMD,
// 0 = the persistent 32 x 32-step kernel; a different fp32 chain, both within the logits tolerance)
static std::atomic<int64_t> g_attn_k16{1};
// rq_filter (index-only quantize calls at e = 32, codebooks up to 1024 codes: 1 = split-bf16 filter
// passes and the exact formula on the near-minimum codes only, 0 = every distance exact)
static std::atomic<int64_t> g_rq_filter{1};
// rq_tail_merge (encode calls that run the fused encoder with leftover tiles and the filtered
// quantizer: 1 = the quantizer's workgroups finish the leftover tiles' layers 2-3 themselves, two
// launches per call; 0 = rq_leftover_kernel between the two, three launches)
static std::atomic<int64_t> g_rq_tail_merge{1};

// kmeans_small (1: gr_kmeans_f32 in one launch of one workgroup when the rows fit in LDS, 0: always
// one launch per phase over row tiles; the same phase code either way)
static std::atomic<int64_t> g_kmeans_small{1};
// bert_tile (gr_bert_embed_f32's GEMM tile: 0 = per launch, the tile that leaves the fewest compute units
// idle; 1 = 128 x 128, 2 = 64 x 128, 3 = 128 x 96 everywhere; the same summation order in each)
static std::atomic<int64_t> g_bert_tile{0};

static const Opt kOpts[] = {
    {"rq_fused", &g_rq_fused, 0, 1},   {"sas_fused", &g_sas_fused, 0, 3}, {"sas_rowtile", &g_sas_rowtile, 0, 1},
    {"lin_wres", &g_lin_wres, 0, 1},   {"emb_proj", &g_emb_proj, 0, 1},   {"topk_half", &g_topk_half, 0, 2},
    {"attn_k16", &g_attn_k16, 0, 1},   {"rq_filter", &g_rq_filter, 0, 1}, {"kmeans_small", &g_kmeans_small, 0, 1},
    {"rq_tail_merge", &g_rq_tail_merge, 0, 1}, {"bert_tile", &g_bert_tile, 0, 3},
};

static const Opt* find_opt(const char* name) {
  for (const Opt& o : kOpts)
    if (!strcmp(name, o.name)) return &o;
  return nullptr;
}

int64_t option(const char* name) {
  const Opt* o = find_opt(name);
  return o ? o->v->load() : -1;
}
}  // namespace gr

extern "C" int gr_set_option(const char* name, int64_t value) {
  gr::clear_error();
  if (!name) return gr::fail(GR_ERR_ARG, "gr_set_option: null name");
  const gr::Opt* o = gr::find_opt(name);
  if (!o || value < o->lo || value > o->hi)
    return gr::fail(GR_ERR_ARG, std::string("gr_set_option: unknown option or value: ") + name);
  o->v->store(value);
  return GR_OK;
}

extern "C" int64_t gr_get_option(const char* name) { return name ? gr::option(name) : -1; }

extern "C" const char* gr_version(void) { return "gr_amd 0.1.0 gfx950"; }
extern "C" const char* gr_last_error(void) { return gr::g_last_error.c_str(); }
