// tpe_engine.hip -- C ABI (include/tpe_engine.h) over the gfx950 kernels.
//
// Host-side ownership: a tpe_engine binds one device and owns an internal
// stream plus a cached one-hp "operator plan" used by the operator-level
// entry points; a tpe_plan owns the device-resident history, the fitted
// mixtures of every hp and the per-suggestion results.  No global state.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tpe_anneal.hpp"
#include "tpe_group_plan.hpp"
#include "tpe_internal.hpp"
#include "tpe_level_plan.hpp"
#include "tpe_pareto_plan.hpp"
#include "tpe_hv_plan.hpp"
#include "tpe_switches.hpp"

using namespace tpe;
static_assert(sizeof(AnnealTrace) == sizeof(tpe_anneal_trace), "layout");

struct tpe_engine {
  int32_t device = 0;
  hipStream_t stream = nullptr;
  static constexpr int kAux = 4;
  hipStream_t aux[kAux] = {};  // concurrent scoring kinds of one level
  std::string err;
  tpe_plan *op = nullptr;  // cached single-hp plan for operator-level calls
};

// (PlanShape: the compiled space as plan_level reads it -- hps, conditions,
// levels, value lattices, kcap, act_frac)
struct tpe_plan : PlanShape {
  tpe_engine *eng = nullptr;
  int32_t P = 0;
  int64_t ncap = 0;
  int32_t last_nb = -1;  // n_below of the last tpe_plan_fit (below K <= n_below + 1)
  std::vector<double> pprior;
  std::vector<int32_t> level_off;  // offsets of each level in d_level_hps
  // device buffers
  tpe_hp *d_hps = nullptr;
  int32_t *d_cp = nullptr, *d_cb = nullptr, *d_level_hps = nullptr, *d_all_hps = nullptr;
  int32_t *d_level_off = nullptr;  // level_off on the device (k_prior)
  double *d_pprior = nullptr;
  double *d_losses = nullptr, *d_vals = nullptr;
  uint8_t *d_active = nullptr, *d_below = nullptr;
  double *d_mw = nullptr, *d_mmu = nullptr, *d_msig = nullptr, *d_scratch = nullptr;
  unsigned char *d_sortbuf = nullptr;  // [2P][16 * scap] fit sort scratch
  int64_t scap = 0;
  MixInfo *d_info = nullptr;
  Coef *d_coef = nullptr;
  Coef32 *d_coef32 = nullptr;  // [2P][kcap / kCoefBlock] block-local fp32 LSE terms
  CoefM *d_coefm = nullptr;    // [2P][mom_stride(kcap)] moment form of 16-component chunks
  CoefM8 *d_coefm8 = nullptr;  // [2P][kcap / kCoefBlock] moment form of 8-component blocks
  float4 *d_coefe = nullptr;   // [2P][kcap / kCoefBlock] compact log-sum-exp block envelopes
  CoefM8 *d_coefmh = nullptr;  // [2P][mom_stride(kcap)] degree-15 form of 16-component chunks
  // Chebyshev tables of the bounded continuous hps' mixtures (k_table_build):
  // built lazily, once per fit epoch, by the first scoring launch that takes
  // them (tab_built: the tables are those of the current mixtures)
  TabHdr *d_tab_hdr = nullptr;  // [2P]
  TabPanel *d_tab = nullptr;    // [2P][kTabMaxPanels]
  double *d_tab_max = nullptr;  // [s_cap][P] best table score per slot (ScoreArgs::tab_max)
  double *d_tab_wmax = nullptr; // [partial_cap][8] ... per wave tile
  int32_t *d_tie_list = nullptr; // [partial_cap][8] the direct pass's wave tiles (ScoreArgs::tie_list)
  int32_t *d_tie_cnt = nullptr;  // [s_cap][P] ... and their number per slot (-1: never gathered)
  int32_t tab_pstride = 0;       // pstride of the last launch that took the tables (tab_on 1)
  double *d_tab_bound = nullptr; // [P][kBndCells] bound lattices, built with the tables
  // per-component certificate terms and per-slot largest a^2 of the lean build
  // (table_terms_doubles; Switches::table_lean; null: k_table_build)
  double *d_tab_terms = nullptr;
  // [2P][kTabMaxPanels][3] debug: each panel's certificate (tpe_plan_tab_cert
  // allocates it; null in every normal run)
  double *d_tab_cert = nullptr;
  TabHot *d_tab_hot = nullptr;   // [s_cap][P] hot intervals of a launch (ScoreArgs::tab_hot)
  DrawZone *d_draw_zone = nullptr;  // [s_cap][P] the screened draw's zones (k_draw_zone)
  unsigned long long *d_screen_stats = nullptr;  // [2] tpe_plan_draw_screen_stats
  bool tab_built = false;
  bool graph_tab = false;       // the captured graph holds the build
  int64_t n = 0;  // history length
  // suggestion state
  int64_t s_cap = 0;
  Partial *d_results = nullptr;
  tpe_result *h_results = nullptr;  // pinned host staging of the results copy
  size_t h_results_cap = 0;
  uint64_t *h_flag = nullptr;       // pinned completion word of k_publish
  uint64_t seq = 0;
  // this call's last launch publishes its results itself (StepShape::publish,
  // tpe_plan_fit_suggest), with sequence seq
  bool pub_fired = false;
  uint64_t *d_seeds = nullptr;
  Partial *d_partial = nullptr;
  size_t partial_cap = 0;
  unsigned long long *d_census = nullptr;  // [kCensus] pair census (tpe_plan_census)
  bool census = false;
  uint32_t *d_ticket = nullptr;
  std::vector<uint64_t> h_seeds;  // this call's seeds (inline kernel args when <= 8)
  bool has_erf = false;
  // value lattices of the bounded quantized hps (KIND_LAT, k_lattice; PlanShape::lat)
  LatInfo *d_lat_info = nullptr;
  double2 *d_lat = nullptr;
  bool lattice_on = true;
  int32_t prune_mode = 3;  // log-sum-exp on bucketed tiles (tpe_plan_set_prune): 0 full,
                           // 1 block skip, 2 block skip + one exponent per wave,
                           // 3 the same with block-local fp32 pairs
  hipEvent_t ev_fork = nullptr, ev_join[8] = {};
  double *d_ext = nullptr, *d_lb = nullptr, *d_la = nullptr;
  size_t ext_cap = 0;
  // tpe_plan_score_points scratch: [P][m] values (host mode), terms and
  // activity (where the caller wants none back), [m] totals (host mode)
  double *d_pt_vals = nullptr, *d_pt_terms = nullptr, *d_pt_total = nullptr;
  uint8_t *d_pt_act = nullptr;
  int32_t *d_pt_idx = nullptr;     // [P][m] each hp's active configurations, compacted
  uint32_t *d_pt_count = nullptr;  // [P] their number
  size_t pt_cap = 0;  // configurations the scratch holds
  // tpe_plan_sample_points: [P] draw tables of the below mixtures;
  // tpe_plan_topk_points: the select's histograms and staging, [kTopkMax] picks
  void *d_pt_tab = nullptr;
  void *d_tk = nullptr;
  int32_t *d_tk_idx = nullptr;
  double *d_cand = nullptr;
  int32_t *d_cpos = nullptr;
  size_t cand_cap = 0;
  // the joint model over the root hps (tpe_plan_joint_*, tpe_joint.hip): the
  // dims and buffers are set up by the first tpe_plan_joint_fit; joint_ok: the
  // tables are those of the current fit epoch (fit_args clears it)
  std::vector<JointDim> jdims;
  std::vector<int32_t> jdim_of_hp;
  int32_t j_slots = 0;
  int64_t j_nopt = 0;
  bool joint_ok = false;
  int32_t jK[2] = {0, 0};    // components per side of the last joint fit
  double fit_pw = 1.0;       // prior_weight / lf of the last fit (fit_args)
  int32_t fit_lf = 0;
  JointDim *d_jdims = nullptr;
  int32_t *d_jdim_of_hp = nullptr, *d_jrows = nullptr, *d_jcount = nullptr, *d_jcomp = nullptr;
  JointSide *d_jside = nullptr;
  uint64_t *d_jkeys = nullptr;
  double *d_jw = nullptr, *d_jcw = nullptr, *d_jcmu = nullptr, *d_jcsig = nullptr;
  double *d_jtab = nullptr, *d_joptlog = nullptr, *d_jpick = nullptr, *d_joptcdf = nullptr;
  size_t joptcdf_cap = 0;
  void *d_jdraw = nullptr;   // [P] draw tables of a joint draw
  double *d_jsides = nullptr, *d_jjoint = nullptr;  // [2][m], [m] of the last joint score
  size_t jpt_cap = 0;
  int64_t jpt_m = 0;         // configurations of the last joint score (tpe_plan_joint_sides)
  // one joint model per group of hps that are active together (tpe_plan_group_*,
  // tpe_group.hip): the partition and the layout are set up by the first
  // tpe_plan_group_info / tpe_plan_group_fit; group_ok: the tables are those of
  // the current fit epoch
  GroupPartition gpart;
  GroupLayout glay;
  bool group_ready = false, group_ok = false;
  int32_t gkb_max = 0;       // below components of group 0, which holds every below row:
                             // a bound on every group's
  JointDim *d_gdims = nullptr;
  GroupDesc *d_ggroups = nullptr;
  int32_t *d_gdim_of_hp = nullptr, *d_ggroup_of_hp = nullptr, *d_grows = nullptr;
  int32_t *d_gcount = nullptr, *d_gcomp = nullptr;
  JointSide *d_gside = nullptr;
  uint64_t *d_gkeys = nullptr;
  double *d_gw = nullptr, *d_gcw = nullptr, *d_gcmu = nullptr, *d_gcsig = nullptr;
  double *d_gtab = nullptr, *d_goptlog = nullptr, *d_gpick = nullptr, *d_goptcdf = nullptr;
  size_t goptcdf_cap = 0;
  void *d_gdraw = nullptr;   // [P] draw tables of a group draw
  double *d_gsides = nullptr, *d_gjoint = nullptr;  // [G][2][m], [G][m] of the last group score
  size_t gpt_cap = 0;
  int64_t gpt_m = 0;         // configurations of the last group score (tpe_plan_group_sides)
  // tpe_plan_group_batch_points (tpe_batch.hip): the call's state for bt_cap
  // configurations, the picks of a host-mode call, and its trace rows
  double *d_bt_ja = nullptr, *d_bt_score = nullptr, *d_bt_gain = nullptr, *d_bt_trace = nullptr;
  uint8_t *d_bt_gact = nullptr, *d_bt_state = nullptr;
  void *d_bt_slot = nullptr, *d_bt_rec = nullptr;
  int32_t *d_bt_idx = nullptr;
  size_t bt_cap = 0, bt_trace_cap = 0;
  int64_t bt_m = -1;         // configurations of the last group score since the group fit
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // per-kind event ring around every scoring launch (tpe_plan_profile)
  struct Prof {
    std::vector<hipEvent_t> a, b;
    std::vector<double> pairs;  // candidate-component pairs the launch covers
    int64_t n = 0;
  };
  Prof prof[KIND_CAT + 1];
  int32_t prof_cap = 0;
  bool timed = false;
  bool evs = false;  // ev0/ev1 bracket the last suggest (recorded only while profiling:
                     // an event record costs a ~6 us pipeline drain between launches)
  int64_t last_ncand = 0, last_nsug = 0;
  int32_t last_level = -1;
  // the last sorted draw's layout in d_cand / d_cpos (tpe_plan_cand_dump)
  int64_t dump_cn = 0, dump_sstride = 0, dump_nsug = 0;
  int32_t dump_level = -1;
  // fit + suggest captured as one hipGraph (tpe_plan_fit_suggest): replayed
  // with the history length / n_below of the fit node and the seeds of the
  // draw nodes patched per call
  // The key of a captured step: the arguments baked into its nodes, and the
  // StepShape (capturing) every launch decision of the step is a function of
  // -- with the fit variant in it (mom_width grows with the history: a replay
  // must not keep the captured width)
  struct StepKey {
    double prior_weight = 0;
    int32_t lf = 0;
    void *stream = nullptr;
    StepShape shape;
    bool operator==(const StepKey &o) const {
      return prior_weight == o.prior_weight && lf == o.lf && stream == o.stream &&
             shape == o.shape;
    }
  };
  StepKey graph_key, pending_key;
  bool graph_ok = false, pending = false;
  int32_t mom_w = 0;       // moment table the last fit wrote: 16 (CoefM), 8 (CoefM8), 0 none
  bool mom_h = false;      // ... and with 16, the degree-15 table (CoefMH)
  bool graph_mom_h = false;
  int32_t graph_mom_w = 0; // ... the captured graph's fit (launch_step restores it)
  HistPatch pend{};        // a small history update not yet on the device: the next
  bool has_pend = false;   // fit writes it (k_fit's patch), anything else flushes it
  // annealing (tpe_plan_anneal): allocated by its first call
  uint64_t *d_an_keys = nullptr;    // [2][ncap] sort keys (ping-pong)
  int32_t *d_an_idx = nullptr;      // [2][ncap] rows; [0]: the loss order
  int32_t *d_an_T = nullptr;        // [P] rows in which each hp is active
  int32_t *d_an_hporder = nullptr;  // [P] hps in the host's evaluation order
  AnnealTrace *d_an_trace = nullptr;  // [an_cap][P]
  int64_t an_cap = 0, an_nsug = 0;
  bool an_ready = false;   // keys / idx / T allocated
  bool an_order = false;   // d_an_hporder holds the host's order (tpe_plan_set_anneal_order)
  // multi-objective TPE (tpe_plan_set_objectives, tpe_pareto.hip): allocated
  // by its first call
  double *d_obj = nullptr;      // [TPE_MAX_OBJ][ncap] the objective matrix
  int32_t *d_pcount = nullptr;  // [2][ncap] dominated_by, dominates
  int32_t obj_M = 0;            // objectives of the rows held (0: none)
  int64_t obj_n = 0;            // ... and their number
  int64_t pareto_n = -1;        // rows the counts are of (tpe_plan_pareto_get)
  int64_t pareto_force = 0;     // j-splits forced by tpe_plan_pareto_shape (0: the plan's)
  // hypervolume subset selection inside the front (tpe_plan_set_hv, tpe_hv.hip):
  // nothing allocated or launched while hv_mode is 0
  int32_t hv_mode = 0;          // 0 off, 1 on: read by the next tpe_plan_set_objectives
  int32_t hv_M = 0, hv_n_pick = 0, hv_S = 0, hv_method = 0;
  uint64_t hv_seed = 0;
  double hv_ref[TPE_MAX_OBJ] = {};
  int32_t *d_hv_i32 = nullptr;  // [2][ncap] state, cnt; then picks, counts [kHvMaxPick], R
  double *d_hv_f64 = nullptr;   // [3][ncap] vol, right, top; then keys [kHvMaxPick]
  uint64_t *d_hv_alive = nullptr;  // [hv_words_cap][ncap] alive words (Monte-Carlo)
  int64_t hv_words_cap = 0;
  double *d_hv_u = nullptr;     // [kHvMaxSamples][TPE_MAX_OBJ] the sample table
  bool hv_u_ok = false;         // ... holds (hv_u_seed, hv_u_S, hv_u_M)
  uint64_t hv_u_seed = 0;
  int32_t hv_u_S = 0, hv_u_M = 0;
  int32_t hv_last_pick = 0;     // n_pick of the last ranking's selection (0: it ran none)
  bool hv_last_exact = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  std::vector<hipGraphNode_t> fit_nodes, draw_nodes;
  std::vector<hipKernelNodeParams> fit_params, draw_params;
  std::vector<FitArgs> fit_args0;
  std::vector<ScoreArgs> draw_args0;
};

namespace {

#define CKH(expr)                                                        \
  do {                                                                   \
    hipError_t e_ = (expr);                                              \
    if (e_ != hipSuccess) {                                              \
      return fail(h, TPE_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    }                                                                    \
  } while (0)

int fail(tpe_engine *h, int code, const std::string &msg) {
  if (h) h->err = msg;
  return code;
}

template <typename T>
hipError_t dalloc(T **p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  return hipMalloc((void **)p, count * sizeof(T));
}

void dfree(void *p) {
  if (p) (void)hipFree(p);
}

// drop the captured fit + suggest graph (buffers it points to change)
void graph_reset(tpe_plan *p) {
  if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  p->graph_exec = nullptr;
  p->graph = nullptr;
  p->graph_ok = p->pending = false;
  p->fit_nodes.clear(); p->draw_nodes.clear();
  p->fit_params.clear(); p->draw_params.clear();
  p->fit_args0.clear(); p->draw_args0.clear();
}

hipStream_t pick_stream(tpe_engine *h, void *s) {
  return s ? (hipStream_t)s : h->stream;
}

void plan_free_buffers(tpe_plan *p) {
  void *bufs[] = {p->d_an_keys, p->d_an_idx, p->d_an_T, p->d_an_hporder, p->d_an_trace,
                  p->d_hps, p->d_cp, p->d_cb, p->d_level_hps, p->d_all_hps, p->d_pprior,
                  p->d_level_off,
                  p->d_losses, p->d_vals, p->d_active, p->d_below, p->d_mw, p->d_mmu,
                  p->d_msig, p->d_scratch, p->d_info, p->d_coef, p->d_results, p->d_seeds,
                  p->d_partial, p->d_ext, p->d_lb, p->d_la, p->d_cand, p->d_cpos,
                  p->d_ticket, p->d_sortbuf, p->d_census, p->d_lat_info, p->d_lat, p->d_coef32, p->d_coefm,
                  p->d_coefm8, p->d_coefe, p->d_coefmh, p->d_tab_hdr, p->d_tab,
                  p->d_tab_max, p->d_tab_wmax, p->d_tie_list, p->d_tie_cnt, p->d_tab_bound,
                  p->d_tab_terms, p->d_tab_cert,
                  p->d_tab_hot, p->d_draw_zone, p->d_screen_stats, p->d_pt_vals, p->d_pt_terms,
                  p->d_pt_total, p->d_pt_act, p->d_pt_idx, p->d_pt_count, p->d_pt_tab, p->d_tk,
                  p->d_tk_idx, p->d_jdims, p->d_jdim_of_hp, p->d_jrows, p->d_jcount, p->d_jcomp,
                  p->d_jside, p->d_jkeys, p->d_jw, p->d_jcw, p->d_jcmu, p->d_jcsig, p->d_jtab,
                  p->d_joptlog, p->d_jpick, p->d_joptcdf, p->d_jdraw, p->d_jsides, p->d_jjoint,
                  p->d_gdims, p->d_ggroups, p->d_gdim_of_hp, p->d_ggroup_of_hp, p->d_grows,
                  p->d_gcount, p->d_gcomp, p->d_gside, p->d_gkeys, p->d_gw, p->d_gcw, p->d_gcmu,
                  p->d_gcsig, p->d_gtab, p->d_goptlog, p->d_gpick, p->d_goptcdf, p->d_gdraw,
                  p->d_gsides, p->d_gjoint, p->d_bt_ja, p->d_bt_score, p->d_bt_gain,
                  p->d_bt_trace, p->d_bt_gact, p->d_bt_state, p->d_bt_slot, p->d_bt_rec,
                  p->d_bt_idx, p->d_obj, p->d_pcount, p->d_hv_i32, p->d_hv_f64, p->d_hv_alive,
                  p->d_hv_u};
  for (void *b : bufs) dfree(b);
  if (p->h_results) (void)hipHostFree(p->h_results);
  p->h_results = nullptr;
  p->h_results_cap = 0;
  if (p->h_flag) (void)hipHostFree(p->h_flag);
  p->h_flag = nullptr;
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  for (auto e : p->ev_join) if (e) (void)hipEventDestroy(e);
  for (auto &pr : p->prof) {
    for (auto e : pr.a) (void)hipEventDestroy(e);
    for (auto e : pr.b) (void)hipEventDestroy(e);
    pr.a.clear(); pr.b.clear(); pr.pairs.clear(); pr.n = 0;
  }
}

int validate_space(tpe_engine *h, const tpe_space *sp) {
  if (!sp || sp->n_hp <= 0 || !sp->hp) return fail(h, TPE_E_INVALID, "empty space");
  for (int i = 0; i < sp->n_hp; ++i) {
    const tpe_hp &x = sp->hp[i];
    if (x.family < TPE_GMM || x.family > TPE_CAT)
      return fail(h, TPE_E_INVALID, "hp " + std::to_string(i) + ": bad family");
    if (x.family == TPE_CAT && x.upper <= 0)
      return fail(h, TPE_E_INVALID, "hp " + std::to_string(i) + ": categorical upper <= 0");
    if (x.family != TPE_CAT) {
      const bool hl = x.flags & TPE_HAS_LOW, hh = x.flags & TPE_HAS_HIGH;
      if (hl != hh)
        return fail(h, TPE_E_INVALID, "hp " + std::to_string(i) + ": one-sided truncation");
      if (hl && !(x.low < x.high))
        return fail(h, TPE_E_BOUNDS, "low >= high");
      if (!(x.prior_sigma > 0))
        return fail(h, TPE_E_INVALID, "hp " + std::to_string(i) + ": prior_sigma <= 0");
    }
    if (x.cond_count < 0 || x.cond_begin < 0 || x.cond_begin + x.cond_count > sp->n_cond)
      return fail(h, TPE_E_INVALID, "hp " + std::to_string(i) + ": bad condition range");
    for (int c = 0; c < x.cond_count; ++c) {
      const int par = sp->cond_parent[x.cond_begin + c];
      if (par < 0 || par >= sp->n_hp || par == i)
        return fail(h, TPE_E_INVALID, "hp " + std::to_string(i) + ": bad condition parent");
    }
    if ((x.flags & TPE_PCHOICE) &&
        (x.pprior_begin < 0 || x.pprior_begin + x.upper > sp->n_pprior))
      return fail(h, TPE_E_INVALID, "hp " + std::to_string(i) + ": bad pchoice prior");
  }
  return TPE_OK;
}

// level(h) = 0 without conditions, else 1 + max(level(parent))
// The value lattice of a bounded quantized hp (LatInfo): drawn values lie in
// [low, high) (GMM) or [exp(low), exp(high)] (LGMM) before rounding to j * q;
// two indices of margin on each side absorb host/device exp and division
// rounding.  R = 0 (no lattice) for unbounded or huge ranges.
LatInfo lattice_of(const tpe_hp &x) {
  LatInfo L{0, 0, 0, 0};
  const int k = score_kind(x);
  if (k != KIND_ERF_G && k != KIND_ERF_L) return L;
  if (!(x.flags & TPE_HAS_LOW) || !(x.flags & TPE_HAS_HIGH) || !(x.q > 0.0)) return L;
  double lo = x.low, hi = x.high;
  if (k == KIND_ERF_L) {
    lo = std::exp(lo);
    hi = std::exp(hi);
  }
  const double a = std::rint(lo / x.q) - 2.0, b = std::rint(hi / x.q) + 2.0;
  if (!(std::fabs(a) < 1e15 && std::fabs(b) < 1e15) || b - a + 1.0 > (double)kLatMaxR)
    return L;
  L.j0 = (int64_t)a;
  L.R = (int32_t)(b - a + 1.0);
  return L;
}

int compute_levels(tpe_engine *h, tpe_plan *p) {
  std::vector<int> lev(p->P, -1);
  for (int iter = 0; iter <= p->P; ++iter) {
    bool changed = false;
    for (int i = 0; i < p->P; ++i) {
      const tpe_hp &x = p->hps[i];
      int l = 0;
      bool ready = true;
      for (int c = 0; c < x.cond_count; ++c) {
        const int par = p->cond_parent[x.cond_begin + c];
        if (lev[par] < 0) { ready = false; break; }
        l = std::max(l, lev[par] + 1);
      }
      if (ready && lev[i] != l) { lev[i] = l; changed = true; }
    }
    if (!changed) break;
  }
  int nl = 0;
  for (int i = 0; i < p->P; ++i) {
    if (lev[i] < 0 || lev[i] > p->P) return fail(h, TPE_E_INVALID, "cyclic conditions");
    nl = std::max(nl, lev[i] + 1);
  }
  p->levels.assign(nl, {});
  // quantized hps with a value lattice first (run_level scores them on it),
  // then the heaviest lpdf kind first: the scoring grid's low slots are
  // dispatched first, so the long quantized tiles do not form the launch's tail
  for (int lat : {1, 0})
    for (int kind : {KIND_ERF_L, KIND_ERF_G})
      for (int i = 0; i < p->P; ++i)
        if (score_kind(p->hps[i]) == kind && (lattice_of(p->hps[i]).R > 0) == (lat == 1))
          p->levels[lev[i]].push_back(i);
  for (int kind : {KIND_LSE_L, KIND_LSE_G, KIND_CAT})
    for (int i = 0; i < p->P; ++i)
      if (score_kind(p->hps[i]) == kind) p->levels[lev[i]].push_back(i);
  p->level_off.assign(nl + 1, 0);
  for (int l = 0; l < nl; ++l)
    p->level_off[l + 1] = p->level_off[l] + (int)p->levels[l].size();
  return TPE_OK;
}

int plan_build(tpe_engine *h, const tpe_space *sp, int64_t max_trials, tpe_plan *p) {
  int rc = validate_space(h, sp);
  if (rc) return rc;
  if (max_trials < 0) return fail(h, TPE_E_INVALID, "max_trials < 0");
  p->eng = h;
  p->P = sp->n_hp;

  p->hps.assign(sp->hp, sp->hp + sp->n_hp);
  p->cond_parent.assign(sp->cond_parent, sp->cond_parent + sp->n_cond);
  p->cond_branch.assign(sp->cond_branch, sp->cond_branch + sp->n_cond);
  p->pprior.assign(sp->pprior, sp->pprior + sp->n_pprior);
  rc = compute_levels(h, p);
  if (rc) return rc;
  p->ncap = std::max<int64_t>(max_trials, 1);
  int64_t kcap = p->ncap + 1;
  for (const auto &x : p->hps)
    if (x.family == TPE_CAT) kcap = std::max<int64_t>(kcap, x.upper);
  // whole coefficient blocks per slot (coef_at, tpe_internal.hpp)
  kcap = (kcap + kCoefBlock - 1) / kCoefBlock * kCoefBlock;
  p->kcap = kcap;
  for (const auto &x : p->hps) {
    const int k = score_kind(x);
    if (k == KIND_ERF_G || k == KIND_ERF_L) p->has_erf = true;
  }
  const int64_t slots = 2 * (int64_t)p->P;
  p->lat.assign(p->P, LatInfo{0, 0, 0, 0});
  int64_t lat_total = 0;
  for (int i = 0; i < p->P; ++i) {
    p->lat[i] = lattice_of(p->hps[i]);
    p->lat[i].off = lat_total;
    lat_total += p->lat[i].R;
  }
  CKH(hipSetDevice(h->device));
  CKH(dalloc(&p->d_lat_info, p->P));
  CKH(dalloc(&p->d_lat, std::max<int64_t>(1, lat_total)));
  CKH(dalloc(&p->d_hps, p->P));
  CKH(dalloc(&p->d_cp, p->cond_parent.size()));
  CKH(dalloc(&p->d_cb, p->cond_branch.size()));
  CKH(dalloc(&p->d_pprior, p->pprior.size()));
  CKH(dalloc(&p->d_level_hps, p->P));
  CKH(dalloc(&p->d_all_hps, p->P));
  CKH(dalloc(&p->d_level_off, p->level_off.size()));
  CKH(dalloc(&p->d_losses, p->ncap));
  CKH(dalloc(&p->d_vals, (size_t)p->ncap * p->P));
  CKH(dalloc(&p->d_active, (size_t)p->ncap * p->P));
  CKH(dalloc(&p->d_below, p->ncap));
  CKH(dalloc(&p->d_mw, (size_t)slots * kcap));
  CKH(dalloc(&p->d_mmu, (size_t)slots * kcap));
  CKH(dalloc(&p->d_msig, (size_t)slots * kcap));
  CKH(dalloc(&p->d_scratch, (size_t)slots * kcap));
  p->scap = p->ncap + 1;
  CKH(dalloc(&p->d_sortbuf, (size_t)slots * 16 * p->scap));
  CKH(dalloc(&p->d_info, slots));
  CKH(dalloc(&p->d_census, kCensus));
  CKH(hipMemset(p->d_census, 0, kCensus * sizeof(unsigned long long)));
  CKH(dalloc(&p->d_coef, (size_t)slots * kcap));
  CKH(dalloc(&p->d_coef32, (size_t)slots * (kcap / kCoefBlock)));
  CKH(dalloc(&p->d_coefm, (size_t)slots * mom_stride(kcap)));
  CKH(dalloc(&p->d_coefm8, (size_t)slots * (kcap / kCoefBlock)));
  CKH(dalloc(&p->d_coefe, (size_t)slots * (kcap / kCoefBlock)));
  CKH(dalloc(&p->d_coefmh, (size_t)slots * mom_stride(kcap)));
  CKH(dalloc(&p->d_tab_hdr, (size_t)slots));
  CKH(hipMemset(p->d_tab_hdr, 0, (size_t)slots * sizeof(TabHdr)));
  CKH(dalloc(&p->d_tab, (size_t)slots * kTabMaxPanels));
  CKH(dalloc(&p->d_tab_bound, (size_t)p->P * kBndCells));
  if (switches().table_lean) CKH(dalloc(&p->d_tab_terms, table_terms_doubles(p->P, kcap)));
  // expected activity of every hp (mom_width): an hp conditioned on branch b
  // of a categorical parent is active in ~1 / upper of the parent's trials
  // (levels are in dependency order: parents first)
  p->act_frac.assign(p->P, 1.0);
  for (const auto &lv : p->levels)
    for (int i : lv) {
      const tpe_hp &x = p->hps[i];
      if (x.cond_count == 0) continue;
      double f = 0.0;
      for (int c = 0; c < x.cond_count; ++c) {
        const int par = p->cond_parent[x.cond_begin + c];
        const tpe_hp &y = p->hps[par];
        f += p->act_frac[par] / (y.family == TPE_CAT ? std::max(1, (int)y.upper) : 1);
      }
      p->act_frac[i] = std::min(1.0, f);
    }
  p->finish();  // (the per-level data of plan_level)
  CKH(hipEventCreate(&p->ev0));
  CKH(hipEventCreate(&p->ev1));
  CKH(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
  for (auto &e : p->ev_join) CKH(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  std::vector<int32_t> lh;
  for (auto &l : p->levels) lh.insert(lh.end(), l.begin(), l.end());
  std::vector<int32_t> all(p->P);
  for (int i = 0; i < p->P; ++i) all[i] = i;
  hipStream_t st = h->stream;
  CKH(hipMemcpyAsync(p->d_hps, p->hps.data(), p->P * sizeof(tpe_hp), hipMemcpyHostToDevice, st));
  CKH(hipMemcpyAsync(p->d_lat_info, p->lat.data(), p->P * sizeof(LatInfo), hipMemcpyHostToDevice,
                     st));
  if (!p->cond_parent.empty()) {
    CKH(hipMemcpyAsync(p->d_cp, p->cond_parent.data(), p->cond_parent.size() * 4, hipMemcpyHostToDevice, st));
    CKH(hipMemcpyAsync(p->d_cb, p->cond_branch.data(), p->cond_branch.size() * 4, hipMemcpyHostToDevice, st));
  }
  if (!p->pprior.empty())
    CKH(hipMemcpyAsync(p->d_pprior, p->pprior.data(), p->pprior.size() * 8, hipMemcpyHostToDevice, st));
  CKH(hipMemcpyAsync(p->d_level_hps, lh.data(), lh.size() * 4, hipMemcpyHostToDevice, st));
  CKH(hipMemcpyAsync(p->d_all_hps, all.data(), all.size() * 4, hipMemcpyHostToDevice, st));
  CKH(hipMemcpyAsync(p->d_level_off, p->level_off.data(), p->level_off.size() * 4,
                     hipMemcpyHostToDevice, st));
  CKH(hipMemsetAsync(p->d_info, 0, slots * sizeof(MixInfo), st));
  CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

int ensure_suggest_state(tpe_engine *h, tpe_plan *p, int64_t n_sug, size_t partials) {
  if (n_sug > p->s_cap || partials > p->partial_cap) graph_reset(p);
  if (n_sug > p->s_cap) {
    dfree(p->d_results);
    dfree(p->d_seeds);
    dfree(p->d_ticket);
    p->d_results = nullptr;
    p->d_seeds = nullptr;
    p->d_ticket = nullptr;
    CKH(dalloc(&p->d_results, (size_t)n_sug * p->P));
    CKH(dalloc(&p->d_seeds, n_sug));
    // (+1: the launch-wide arrival counter of a publishing launch, pub_ticket)
    CKH(dalloc(&p->d_ticket, (size_t)n_sug * p->P + 1));
    CKH(hipMemset(p->d_ticket, 0, ((size_t)n_sug * p->P + 1) * sizeof(uint32_t)));
    dfree(p->d_tab_max);
    p->d_tab_max = nullptr;
    CKH(dalloc(&p->d_tab_max, (size_t)n_sug * p->P));
    dfree(p->d_tie_cnt);
    p->d_tie_cnt = nullptr;
    CKH(dalloc(&p->d_tie_cnt, (size_t)n_sug * p->P));
    CKH(hipMemset(p->d_tie_cnt, 0xff, (size_t)n_sug * p->P * sizeof(int32_t)));
    dfree(p->d_tab_hot);
    p->d_tab_hot = nullptr;
    CKH(dalloc(&p->d_tab_hot, (size_t)n_sug * p->P));
    dfree(p->d_draw_zone);
    p->d_draw_zone = nullptr;
    CKH(dalloc(&p->d_draw_zone, (size_t)n_sug * p->P));
    if (!p->d_screen_stats) {
      CKH(dalloc(&p->d_screen_stats, 2));
      CKH(hipMemset(p->d_screen_stats, 0, 2 * sizeof(unsigned long long)));
    }
    p->s_cap = n_sug;
  }
  if (partials > p->partial_cap) {
    dfree(p->d_partial);
    p->d_partial = nullptr;
    CKH(dalloc(&p->d_partial, partials));
    dfree(p->d_tab_wmax);
    p->d_tab_wmax = nullptr;
    CKH(dalloc(&p->d_tab_wmax, partials * 8));  // (one per wave of a tile)
    // (NaN: a slot the table pass never wrote shows no score and no -inf)
    CKH(hipMemset(p->d_tab_wmax, 0xff, partials * 8 * sizeof(double)));
    dfree(p->d_tie_list);
    p->d_tie_list = nullptr;
    CKH(dalloc(&p->d_tie_list, partials * 8));
    p->partial_cap = partials;
  }
  return TPE_OK;
}

int ensure_ext(tpe_engine *h, tpe_plan *p, size_t n) {
  if (n > p->ext_cap) {
    dfree(p->d_ext); dfree(p->d_lb); dfree(p->d_la);
    p->d_ext = p->d_lb = p->d_la = nullptr;
    CKH(dalloc(&p->d_ext, n));
    CKH(dalloc(&p->d_lb, n));
    CKH(dalloc(&p->d_la, n));
    p->ext_cap = n;
  }
  return TPE_OK;
}

// scratch of tpe_plan_score_points for m configurations (grows, never shrinks)
int ensure_points(tpe_engine *h, tpe_plan *p, size_t m) {
  if (m > p->pt_cap) {
    dfree(p->d_pt_vals); dfree(p->d_pt_terms); dfree(p->d_pt_total); dfree(p->d_pt_act);
    dfree(p->d_pt_idx);
    p->d_pt_vals = p->d_pt_terms = p->d_pt_total = nullptr;
    p->d_pt_act = nullptr;
    p->d_pt_idx = nullptr;
    p->pt_cap = 0;
    CKH(dalloc(&p->d_pt_vals, m * p->P));
    CKH(dalloc(&p->d_pt_terms, m * p->P));
    CKH(dalloc(&p->d_pt_act, m * p->P));
    CKH(dalloc(&p->d_pt_idx, m * p->P));
    CKH(dalloc(&p->d_pt_total, m));
    if (!p->d_pt_count) CKH(dalloc(&p->d_pt_count, (size_t)p->P));
    p->pt_cap = m;
  }
  return TPE_OK;
}

// scratch of tpe_plan_topk_points (fixed size, allocated by the first call)
int ensure_topk(tpe_engine *h, tpe_plan *p) {
  if (!p->d_tk) CKH(hipMalloc(&p->d_tk, topk_scratch_bytes()));
  if (!p->d_tk_idx) CKH(dalloc(&p->d_tk_idx, (size_t)kTopkMax));
  return TPE_OK;
}

// a launch's scoring grid (score_grid, tpe_level_plan.hpp) into its arguments
void copy_groups(ScoreArgs &a, const ScoreGrid &g) {
  a.n_groups = g.n_groups;
  a.pstride = g.pstride;
  for (int i = 0; i < kMaxGroups; ++i) {
    a.grp_slots[i] = g.grp_slots[i];
    a.grp_kind[i] = g.grp_kind[i];
    a.grp_slot0[i] = g.grp_slot0[i];
    a.grp_tiles[i] = g.grp_tiles[i];
  }
  for (int i = 0; i <= kMaxGroups; ++i) a.grp_block0[i] = g.grp_block0[i];
}

int ensure_cand(tpe_engine *h, tpe_plan *p, size_t n) {
  if (n > p->cand_cap) {
    graph_reset(p);
    dfree(p->d_cand);
    dfree(p->d_cpos);
    p->d_cand = nullptr;
    p->d_cpos = nullptr;
    CKH(dalloc(&p->d_cand, n));
    CKH(dalloc(&p->d_cpos, n));
    p->cand_cap = n;
  }
  return TPE_OK;
}

ScoreArgs base_args(tpe_plan *p, int64_t n_sug) {
  ScoreArgs a{};
  a.sort_log2 = kSortLog2Small;
  a.hps = p->d_hps;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.info = p->d_info;
  a.coef = p->d_coef;
  a.coef32 = p->d_coef32;
  a.coefm = p->d_coefm;
  a.coefm8 = p->d_coefm8;
  a.coefmh = p->d_coefmh;
  a.coefe = p->d_coefe;
  a.mw = p->d_mw;
  a.mmu = p->d_mmu;
  a.msig = p->d_msig;
  a.seeds = p->d_seeds;
  a.results = p->d_results;
  a.partial = p->d_partial;
  a.ticket = p->d_ticket;
  a.census = p->census ? p->d_census : nullptr;
  a.kcap = p->kcap;
  a.n_hp = p->P;
  a.n_suggest = (int32_t)n_sug;
  a.lat_info = p->d_lat_info;
  a.lat = p->d_lat;
  a.lse_mom = p->mom_w;
  a.lse_momh = p->mom_w == 16 && p->mom_h ? 1 : 0;
  // (round 2's L2 warm-up is off since round 6: the same-box A/B gave config 4
  // 127.3 -> 124.2 ms and config 5 543 -> 536 ms per step without it -- the
  // waves' first envelope reads waited on those loads, and the tables are
  // L2-resident after the first blocks anyway; the wave tiles always tighten
  // the skip threshold from the block of the highest bound)
  a.l2_warm = 0;
  a.lse_tight = 1;
  a.tab_hdr = p->d_tab_hdr;
  a.tab = p->d_tab;
  a.tab_max = p->d_tab_max;
  a.tab_wmax = p->d_tab_wmax;
  a.tie_list = p->d_tie_list;
  a.tie_cnt = p->d_tie_cnt;
  a.tab_tie = switches().table_tie();
  a.tab_bound = p->d_tab_bound;
  a.tab_hot = p->d_tab_hot;
  return a;
}

// the fit variant a call takes (fit_variant, tpe_level_plan.hpp)
FitVariant plan_fit_variant(const tpe_plan *p, bool moments) {
  return fit_variant(*p, switches(), p->n, fit_small(p->n), moments);
}

// f: the step's fit variant -- its moment table is written (only the wave
// tiles of sorted draws read it); plan.mom_w / mom_h record which tables the
// plan holds (the scoring launches read those: base_args)
FitArgs fit_args(tpe_plan *p, int32_t n_below, double prior_weight, int32_t lf,
                 const FitVariant &f) {
  p->mom_w = f.mom_w;
  p->mom_h = f.mom_h;
  p->tab_built = false;  // a new fit epoch
  p->joint_ok = false;
  p->group_ok = false;
  p->fit_pw = prior_weight;
  p->fit_lf = lf;
  FitArgs a{};
  a.hps = p->d_hps;
  a.vals = p->d_vals;
  a.active = p->d_active;
  a.losses = p->d_losses;
  a.n = p->n;
  a.ld = p->ncap;
  a.n_below = n_below;
  a.lf = lf;
  a.prior_weight = prior_weight;
  a.pprior = p->d_pprior;
  a.mw = p->d_mw;
  a.mmu = p->d_mmu;
  a.msig = p->d_msig;
  a.info = p->d_info;
  a.coef = p->d_coef;
  a.coef32 = p->d_coef32;
  a.coefm = p->mom_w == 16 ? p->d_coefm : nullptr;
  a.coefm8 = p->mom_w == 8 ? p->d_coefm8 : nullptr;
  a.coefmh = p->mom_h ? p->d_coefmh : nullptr;
  a.coefe = p->d_coefe;
  a.kcap = p->kcap;
  a.ob = p->d_scratch;
  a.tmp = p->d_scratch;
  a.sortbuf = p->d_sortbuf;
  a.scap = p->scap;
  return a;
}

// a deferred history update onto the device now (k_hist_patch), for every
// reader other than the fit
int flush_patch(tpe_engine *h, tpe_plan *p, hipStream_t st) {
  if (!p->has_pend) return TPE_OK;
  p->has_pend = false;
  CKH(launch_hist_patch(p->pend, p->d_vals, p->d_active, p->d_losses, st));
  return TPE_OK;
}
// the fit of a plan, with the deferred history update (if any) written by
// its blocks first
int fit_launch(tpe_engine *h, tpe_plan *p, const FitArgs &a, int32_t n_hp, hipStream_t st) {
  CKH(launch_fit(a, n_hp, st, p->has_pend ? &p->pend : nullptr));
  p->has_pend = false;
  return TPE_OK;
}

// the Chebyshev tables of the current mixtures, if this fit epoch has none yet
int table_build(tpe_engine *h, tpe_plan *p, hipStream_t st) {
  if (p->tab_built) return TPE_OK;
  CKH(launch_table_build(p->d_hps, p->P, p->d_info, p->d_coef, p->kcap, p->d_tab_hdr, p->d_tab,
                         p->census ? p->d_census : nullptr, st,
                         switches().table_prefilter ? p->d_tab_bound : nullptr, p->d_tab_terms,
                         p->d_tab_cert));
  p->tab_built = true;
  return TPE_OK;
}

// (a launch that takes the tables, tab_on, builds them first if need be --
// inside the profile bracket, so plan.profile times the build with it)
int score_launch(tpe_engine *h, tpe_plan *p, ScoreArgs a, bool has_erf, int64_t cn,
                 hipStream_t sg, bool record, int classes = 7) {
  tpe_plan::Prof *pr = nullptr;
  if (record && p->prof_cap > 0) {
    pr = &p->prof[0];
    if (pr->n >= p->prof_cap) pr = nullptr;  // ring full: stop recording
  }
  if (pr) CKH(hipEventRecord(pr->a[pr->n], sg));
  if (a.tab_on == 1 && (classes & 1)) {
    const int rc = table_build(h, p, sg);
    if (rc) return rc;
    p->tab_pstride = a.pstride;  // (tpe_plan_tab_wmax's row length)
  }
  // (a level mixing wave-tile log-sum-exp slots with other kinds: those run
  // beside it on an auxiliary stream; the events are free at scoring time)
  CKH(launch_score(a, has_erf, sg, switches().side_streams ? h->aux[1] : nullptr, p->ev_join[1],
                   p->ev_join[2], classes));
  if (pr) {
    CKH(hipEventRecord(pr->b[pr->n], sg));
    pr->pairs[pr->n] = (double)cn * (double)a.n_suggest;
    pr->n++;
  }
  return TPE_OK;
}

// what a call contributes to plan_level's decisions (StepShape): f: the tables
// in place when its levels run
StepShape step_shape(const tpe_plan *p, int64_t n_sug, int64_t n_cand, int64_t cand_begin,
                     int64_t n_total, int32_t last_nb, const FitVariant &f) {
  StepShape s;
  s.n_sug = n_sug;
  s.n_cand = n_cand;
  s.cand_begin = cand_begin;
  s.n_total = n_total;
  s.below = below_class(last_nb >= 0 ? (int64_t)last_nb + 1 : p->kcap);
  s.fit = f;
  s.prune_mode = p->prune_mode;
  s.lattice_on = p->lattice_on;
  s.screen_run = step_screen_run(switches());
  s.screen_halves = step_screen_halves(switches());
  s.screen_tail = (int32_t)switches().draw_screen_tail;
  s.screen_pool = switches().draw_screen_pool;
  s.table_lean = switches().table_lean;
  return s;
}

// One level of conditional hps: one draw(+bucket) launch and one scoring
// launch (every lpdf kind) for all of its hps, chunk by chunk, as
// plan_level lays them out (tpe_level_plan.hpp): this function only executes
// the plan -- buffers, arguments, streams, profiling brackets, launches.
int run_level(tpe_engine *h, tpe_plan *p, int level, const StepShape &s, hipStream_t st) {
  const LevelPlan lp = plan_level(*p, switches(), s, level);
  const int64_t n_sug = s.n_sug;
  const int32_t n_level = lp.n_level, n_lat = lp.n_lat;
  const int32_t *lvl = p->d_level_hps + p->level_off[level];
  if (lp.empty) {
    // no candidates (an empty shard of a small suggest, n_EI_candidates = 0):
    // broadcast_best of no samples is [] (tpe.py:750-759) -- every hp of the
    // level gets the neutral record (NaN, NaN, -1, inactive), which k_merge
    // treats as "nothing here" (a merge of zero records writes exactly that)
    if (n_level > 0) CKH(launch_merge(lvl, n_level, (int32_t)n_sug, p->P, 0, nullptr, p->d_results, st));
    return TPE_OK;
  }
  ScoreArgs la = base_args(p, n_sug);
  la.level_hps = lvl;
  la.n_slots = n_level;
  la.slot_rows = lp.slot_rows;
  la.compact = lp.compact ? 1 : 0;
  // profiling bracket of the lattice launches
  auto lat_bracket = [&](hipStream_t sl, auto launch) -> int {
    tpe_plan::Prof *pr = nullptr;
    if (p->prof_cap > 0 && p->prof[1].n < p->prof_cap) pr = &p->prof[1];
    if (pr) CKH(hipEventRecord(pr->a[pr->n], sl));
    CKH(launch());
    if (pr) {
      CKH(hipEventRecord(pr->b[pr->n], sl));
      pr->pairs[pr->n] = (double)level;
      pr->n++;
    }
    return TPE_OK;
  };
  auto lattice = [&](hipStream_t sl) -> int {
    return lat_bracket(sl, [&] {
      return launch_lattice(la, p->levels[level].data(), p->hps.data(), p->lat.data(), n_lat,
                            p->d_lat, sl, lp.lat_rows);
    });
  };
  const bool lat_side = lp.lat == LatRun::Side;
  bool lat_pending = lp.lat == LatRun::Deferred;
  if (lp.lat == LatRun::InOrder || lat_side) {
    hipStream_t sl = st;
    if (lat_side) {
      sl = h->aux[0];
      CKH(hipEventRecord(p->ev_fork, st));
      CKH(hipStreamWaitEvent(sl, p->ev_fork, 0));
    }
    // everything after the fork: a failure still records the join event on
    // the side stream and waits on it from st, so a captured graph is never
    // left forked (the chunk loop below joins on its own exits likewise)
    const int lrc = lattice(sl);
    if (lat_side) {
      const hipError_t e1 = hipEventRecord(p->ev_join[0], sl);
      if (lrc) {
        if (e1 == hipSuccess) (void)hipStreamWaitEvent(st, p->ev_join[0], 0);
        return lrc;
      }
      if (e1 != hipSuccess) return fail(h, TPE_E_HIP, "lattice side stream join event");
    } else if (lrc) {
      return lrc;
    }
  }
  bool joined = !lat_side;
  // every exit of the chunk loop (errors included) joins the lattice side
  // stream back, so a failed call never leaves a captured graph forked
  auto chunks = [&]() -> int {
  for (const ChunkPlan &c : lp.chunks) {
    const int64_t cn = c.cn;
    if (c.grid.pstride < 0) return fail(h, TPE_E_INVALID, "level slots not grouped by lpdf kind");
    int rc = ensure_suggest_state(h, p, n_sug, (size_t)n_sug * p->P * c.grid.pstride);
    if (rc) return rc;
    rc = ensure_cand(h, p, (size_t)std::max<int64_t>(1, n_sug * n_level * cn));
    if (rc) return rc;
    // buffers (re)allocated above: take their pointers only now
    ScoreArgs a = base_args(p, n_sug);
    copy_groups(a, c.grid);
    a.compact = lp.compact ? 1 : 0;
    a.cand = p->d_cand;
    a.cand_sstride = (int64_t)n_level * cn;
    a.n_cand = cn;
    a.cand_begin = s.cand_begin + c.c0;
    a.accumulate = c.accumulate ? 1 : 0;
    a.level_hps = lvl;
    a.n_slots = n_level;
    a.slot_rows = lp.slot_rows;
    a.cand_slot0 = 0;
    for (int i = 0; i < kInlineSeeds && i < n_sug; ++i) a.seed_inline[i] = p->h_seeds[i];
    a.n_inline_seeds = (int32_t)std::min<int64_t>(n_sug, kInlineSeeds);
    a.lse_pos = c.lse_pos;
    a.sort_log2 = c.sort_log2;
    a.lookup_draw = c.lookup_draw;
    a.lse_prune = c.lse_prune;
    a.lse_shift_min = lp.lse_shift_min;
    a.lse_f32 = c.lse_f32;
    a.tab_on = c.tab_on;
    a.tab_pref = c.tab_pref ? 1 : 0;  // (2, behind a pruning draw: once that has run)
    if (c.lk_fork) {
      CKH(hipEventRecord(p->ev_join[3], st));
      CKH(hipStreamWaitEvent(h->aux[2], p->ev_join[3], 0));
      int lrc = TPE_OK;
      if (lat_pending) {  // the deferred lattice, ahead of its readers
        lrc = lattice(h->aux[2]);
        lat_pending = false;
      }
      const hipError_t el = lrc ? hipErrorUnknown
                                : launch_score(a, lp.erf_level, h->aux[2], nullptr, nullptr, nullptr, 2);
      CKH(hipEventRecord(p->ev_join[4], h->aux[2]));
      if (el != hipSuccess) {
        (void)hipStreamWaitEvent(st, p->ev_join[4], 0);
        return fail(h, TPE_E_HIP, "lookup launch");
      }
    }
    if (lat_pending) {  // (no lookup fork after all: the lattice in order)
      lat_pending = false;
      const int lrc = lattice(st);
      if (lrc) return lrc;
    }
    // (every exit below joins the lookup stream back first)
    auto join_lk = [&]() {
      if (c.lk_fork) (void)hipStreamWaitEvent(st, p->ev_join[4], 0);
    };
    a.tile_draw = c.draw == Draw::Tiles ? 1 : 0;
    if (c.publish) {
      a.pub_dst = reinterpret_cast<uint64_t *>(p->h_results);
      a.pub_flag = p->h_flag;
      a.pub_ticket = p->d_ticket + (size_t)p->s_cap * p->P;
      a.pub_seq = ++p->seq;
      a.pub_words = (int32_t)(n_sug * p->P * (int64_t)(sizeof(tpe_result) / 8));
      a.pub_events = (int32_t)(n_sug * n_level);
      p->pub_fired = true;
    }
    switch (c.draw) {
      case Draw::Tiles:
        break;
      case Draw::Fused:
        rc = lat_bracket(st, [&] {
          return launch_lattice_draw(a, p->levels[level].data(), p->hps.data(), p->lat.data(),
                                     n_lat, p->d_lat, st, lp.lat_rows);
        });
        if (rc) return rc;
        break;
      case Draw::Plain:
        CKH(launch_draw(a, c.table_draw, st));
        break;
      default: {  // the sorted draws
        hipError_t e;
        if (c.draw == Draw::Sorted) {
          e = launch_draw_sorted(a, c.small_table, c.fast, p->d_cpos, st);
        } else {
          rc = table_build(h, p, st);
          if (rc) { join_lk(); return rc; }
          p->tab_pstride = a.pstride;
          e = launch_draw_sorted(a, c.small_table, c.fast, p->d_cpos, st, 1);
          if (e == hipSuccess) e = launch_table_pilot(a, st);
          if (c.draw == Draw::SortedScreened) {
            if (e == hipSuccess)
              e = launch_draw_zone(a, p->d_draw_zone, c.screen_tiles, c.screen_halves, c.screen_tail,
                                   kScreenMargin, c.screen_guide, st);
            if (e == hipSuccess)
              e = launch_draw_screened(a, p->d_cpos, p->d_draw_zone, p->d_screen_stats,
                                       c.screen_guide >= 0, c.screen_run, c.screen_pool, st);
          } else if (e == hipSuccess) {
            e = launch_draw_pruned(a, c.small_table, c.fast, p->d_cpos, st);
          }
        }
        if (e != hipSuccess) { join_lk(); return fail(h, TPE_E_HIP, hipGetErrorString(e)); }
        p->dump_cn = cn;
        p->dump_sstride = a.cand_sstride;
        p->dump_level = level;
        p->dump_nsug = n_sug;
      }
    }
    a.tab_pref = c.tab_pref;
    if (c.bucket) CKH(launch_bucket(a, n_lat, p->d_cpos, st));
    a.cand_pos = c.cand_pos ? p->d_cpos : nullptr;
    if (!joined) {
      CKH(hipStreamWaitEvent(st, p->ev_join[0], 0));
      joined = true;
    }
    rc = score_launch(h, p, a, lp.erf_level, cn, st, true, c.classes);
    join_lk();
    if (rc) return rc;
  }
  return TPE_OK;
  };
  const int rc = chunks();
  if (!joined) {
    const hipError_t e = hipStreamWaitEvent(st, p->ev_join[0], 0);
    if (!rc && e != hipSuccess) return fail(h, TPE_E_HIP, "join of the lattice side stream");
  }
  return rc;
}

// Externally supplied candidates of one hp (parity / operator path).
// sorted_mode < 0: every candidate scored on its own (exact sums, any
// tiling); >= 0: the large-draw production form -- value-bucketed in
// kSortedBlock blocks as k_draw_sorted writes them, log-sum-exp prune mode
// sorted_mode on the tiles run_level picks for it (4: those tiles scored from
// the hp's certified Chebyshev tables alone).
int run_external(tpe_engine *h, tpe_plan *p, int32_t hp, const double *ext, int64_t n,
                 double *lb, double *la, hipStream_t st, int32_t sorted_mode = -1) {
  int kind = score_kind(p->hps[hp]);
  const bool sorted = sorted_mode >= 0;
  if (sorted && sorted_mode > 1)
    kind = kind == KIND_LSE_G ? KIND_LSE_GW : kind == KIND_LSE_L ? KIND_LSE_LW : kind;
  // mode 4: prune mode 3's tiles scored from the hp's Chebyshev tables only
  const bool tab = sorted_mode == 4;
  if (tab) {
    sorted_mode = 3;
    if (!table_hp(p->hps[hp])) return fail(h, TPE_E_INVALID, "hp has no Chebyshev table");
    const int rc = table_build(h, p, st);
    if (rc) return rc;
    TabHdr th[2];
    CKH(hipMemcpyAsync(th, p->d_tab_hdr + 2 * (int64_t)hp, sizeof(th), hipMemcpyDeviceToHost, st));
    CKH(hipStreamSynchronize(st));
    for (const TabHdr &t : th)
      if (!(t.P > 0 && t.ncert == (uint32_t)t.P))
        return fail(h, TPE_E_INVALID, "Chebyshev table not certified");
  }
  const ScoreGrid grid =
      score_grid([&](int) { return kind; }, 1, n, [](int b, int e) { return e - b; });
  int rc = ensure_suggest_state(h, p, 1, (size_t)p->P * grid.pstride);
  if (rc) return rc;
  if (sorted) {
    rc = ensure_cand(h, p, (size_t)std::max<int64_t>(1, n));
    if (rc) return rc;
  }
  ScoreArgs a = base_args(p, 1);
  copy_groups(a, grid);
  a.cand = ext;
  a.cand_sstride = n;
  a.n_cand = n;
  a.level_hps = p->d_all_hps + hp;
  a.n_slots = 1;
  a.slot_rows = 1;
  a.out_lb = lb;
  a.out_la = la;
  a.force_active = 1;
  if (sorted) {
    a.cand = p->d_cand;
    a.sort_log2 = sort_log2_for(n);
    CKH(launch_sort_ext(a, ext, p->d_cpos, st));
    a.cand_pos = p->d_cpos;
    a.lse_pos = 1;
    a.lse_prune = sorted_mode;
    a.lse_shift_min = (int32_t)switches().lse_shift_min;
    a.tab_on = tab ? 2 : 0;
  }
  return score_launch(h, p, a, kind == KIND_ERF_G || kind == KIND_ERF_L, n, st, false);
}

int host_results(tpe_engine *h, tpe_plan *p, int64_t n_sug);

int copy_results(tpe_engine *h, tpe_plan *p, int64_t n_sug, tpe_result *out, int32_t on_dev,
                 hipStream_t st) {
  if (!out || on_dev) p->pub_fired = false;  // (armed for host output only)
  if (!out) return TPE_OK;
  const size_t bytes = (size_t)n_sug * p->P * sizeof(tpe_result);
  if (on_dev) {
    CKH(hipMemcpyAsync(out, p->d_results, bytes, hipMemcpyDeviceToDevice, st));
    return TPE_OK;
  }
  // to the host through a pinned staging buffer of the plan: a DMA copy
  // without the runtime's pageable-memory staging (a few hundred bytes; the
  // copy's latency is most of what the caller waits for after the kernels)
  // (fine-grained coherent pinned memory: the kernel's stores reach it
  // directly and the host reads them without a runtime copy)
  const int rc = host_results(h, p, n_sug);
  if (rc) return rc;
  if (!switches().publish) {
    CKH(hipMemcpyAsync(p->h_results, p->d_results, bytes, hipMemcpyDeviceToHost, st));
    CKH(hipStreamSynchronize(st));
    std::memcpy(out, p->h_results, bytes);
    return TPE_OK;
  }
  // (the call's last launch published already: pub_fired, sequence p->seq)
  const bool fired = p->pub_fired;
  p->pub_fired = false;
  const uint64_t seq = fired ? p->seq : ++p->seq;
  if (!fired) CKH(launch_publish(p->d_results, p->h_results, bytes, p->h_flag, seq, st));
  // spin on the completion word (a stream synchronize's wake-up is the
  // larger part of a small suggest's host-side wait); every 2^12 polls the
  // stream is asked for an error, so a failed launch cannot spin forever
  for (uint64_t it = 1;; ++it) {
    if (__atomic_load_n(p->h_flag, __ATOMIC_ACQUIRE) == seq) break;
    __builtin_ia32_pause();
    if ((it & 4095) == 0) {
      const hipError_t q = hipStreamQuery(st);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(h, TPE_E_HIP, hipGetErrorString(q));
      if (q == hipSuccess && __atomic_load_n(p->h_flag, __ATOMIC_ACQUIRE) != seq) {
        // a fused publish short of arrivals leaves its launch-wide ticket
        // counting: clear it, or the next fused publish of this plan would
        // fire early and copy records not yet written
        if (fired) {
          (void)hipMemsetAsync(p->d_ticket + (size_t)p->s_cap * p->P, 0, sizeof(uint32_t), st);
          (void)hipStreamSynchronize(st);
        }
        return fail(h, TPE_E_HIP, "k_publish finished without its completion word");
      }
    }
  }
  std::memcpy(out, p->h_results, bytes);
  return TPE_OK;
}

// the pinned host buffers of a call's results (copy_results; armed before a
// call whose last launch publishes them itself)
int host_results(tpe_engine *h, tpe_plan *p, int64_t n_sug) {
  const size_t bytes = (size_t)n_sug * p->P * sizeof(tpe_result);
  if (bytes > p->h_results_cap) {
    if (p->h_results) (void)hipHostFree(p->h_results);
    p->h_results = nullptr;
    p->h_results_cap = 0;
    const size_t cap = std::max<size_t>(bytes, 4096);
    CKH(hipHostMalloc((void **)&p->h_results, cap, hipHostMallocCoherent | hipHostMallocMapped));
    p->h_results_cap = cap;
  }
  if (switches().publish && !p->h_flag) {
    CKH(hipHostMalloc((void **)&p->h_flag, 64, hipHostMallocCoherent | hipHostMallocMapped));
    __atomic_store_n(p->h_flag, (uint64_t)0, __ATOMIC_RELEASE);
  }
  return TPE_OK;
}

// one-hp operator plan cached in the engine
int op_plan(tpe_engine *h, int32_t family, uint32_t flags, int32_t upper, double low,
            double high, double q, int64_t ncap, tpe_plan **out) {
  tpe_hp x{};
  x.family = family;
  x.flags = flags & (TPE_HAS_LOW | TPE_HAS_HIGH | TPE_HAS_Q);
  x.obs_transform = TPE_OBS_IDENT;
  x.upper = upper;
  x.prior_mu = 0.0;
  x.prior_sigma = 1.0;
  x.low = low;
  x.high = high;
  x.q = q;
  tpe_plan *p = h->op;
  const int64_t need_k = std::max<int64_t>(ncap + 1, upper);
  if (!p || p->ncap < ncap || p->kcap < need_k) {
    if (p) { plan_free_buffers(p); delete p; h->op = nullptr; }
    p = new tpe_plan();
    tpe_space sp{};
    sp.n_hp = 1;
    sp.hp = &x;
    x.upper = std::max<int32_t>(upper, 1);
    const int64_t cap = std::max<int64_t>(ncap, 1024);
    std::vector<double> pp_room((size_t)std::max<int64_t>(cap + 1, upper), 0.0);
    sp.n_pprior = (int64_t)pp_room.size();
    sp.pprior = pp_room.data();
    int rc = plan_build(h, &sp, cap, p);
    if (rc) { plan_free_buffers(p); delete p; return rc; }
    h->op = p;
  }
  p->hps[0] = x;
  CKH(hipMemcpyAsync(p->d_hps, &p->hps[0], sizeof(tpe_hp), hipMemcpyHostToDevice, h->stream));
  *out = p;
  return TPE_OK;
}

// upload an explicit mixture into slot `slot` of an operator plan
int put_mixture(tpe_engine *h, tpe_plan *p, int slot, const double *w, const double *mu,
                const double *sg, int64_t k, int32_t kind) {
  hipStream_t st = h->stream;
  CKH(hipMemcpyAsync(p->d_mw + slot * p->kcap, w, k * 8, hipMemcpyHostToDevice, st));
  if (mu) CKH(hipMemcpyAsync(p->d_mmu + slot * p->kcap, mu, k * 8, hipMemcpyHostToDevice, st));
  if (sg) CKH(hipMemcpyAsync(p->d_msig + slot * p->kcap, sg, k * 8, hipMemcpyHostToDevice, st));
  MixInfo mi{};
  mi.K = (int32_t)k;
  mi.kind = kind;
  CKH(hipMemcpyAsync(p->d_info + slot, &mi, sizeof(MixInfo), hipMemcpyHostToDevice, st));
  CKH(hipStreamSynchronize(st));  // mi lives on this frame
  p->tab_built = false;
  return TPE_OK;
}

bool bad_family(int32_t f) { return f < TPE_GMM || f > TPE_CAT; }

}  // namespace

// ======================================================================
// C ABI
// ======================================================================
extern "C" {

const char *tpe_version(void) { return "tpe-mi355x 0.1 (gfx950)"; }

int tpe_device_count(int32_t *n) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  if (n) *n = c;
  return TPE_OK;
}

int tpe_create(int32_t device, tpe_handle_t *out) {
  if (!out) return TPE_E_INVALID;
  *out = nullptr;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) return TPE_E_NODEVICE;
  if (device < 0 || device >= c) return TPE_E_NODEVICE;
  if (hipSetDevice(device) != hipSuccess) return TPE_E_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return TPE_E_HIP;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return TPE_E_NODEVICE;
  auto *h = new tpe_engine();
  h->device = device;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return TPE_E_HIP;
  }
  for (auto &a : h->aux)
    if (hipStreamCreateWithFlags(&a, hipStreamNonBlocking) != hipSuccess) {
      tpe_destroy(h);
      return TPE_E_HIP;
    }
  *out = h;
  return TPE_OK;
}

int tpe_destroy(tpe_handle_t h) {
  if (!h) return TPE_OK;
  (void)hipSetDevice(h->device);
  if (h->op) { plan_free_buffers(h->op); delete h->op; }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  for (auto a : h->aux) if (a) (void)hipStreamDestroy(a);
  delete h;
  return TPE_OK;
}

const char *tpe_last_error(tpe_handle_t h) { return h ? h->err.c_str() : "null handle"; }

int tpe_synchronize(tpe_handle_t h) {
  if (!h) return TPE_E_INVALID;
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  return TPE_OK;
}

int tpe_split(tpe_handle_t h, const double *losses, int64_t n, double gamma,
              int32_t gamma_cap, uint8_t *below_mask) {
  if (!h) return TPE_E_INVALID;
  if (n < 0 || (n > 0 && (!losses || !below_mask))) return fail(h, TPE_E_INVALID, "bad args");
  if (n == 0) return TPE_OK;
  CKH(hipSetDevice(h->device));
  tpe_plan *p;
  int rc = op_plan(h, TPE_GMM, 0, 1, 0, 0, 0, n, &p);
  if (rc) return rc;
  const int32_t nb = (int32_t)std::min<double>(std::ceil(gamma * std::sqrt((double)n)), gamma_cap);
  CKH(hipMemcpyAsync(p->d_losses, losses, n * 8, hipMemcpyHostToDevice, h->stream));
  p->n = n;
  CKH(launch_split(fit_args(p, std::max(nb, 0), 1.0, 25, plan_fit_variant(p, true)), p->d_below,
                   h->stream));
  CKH(hipMemcpyAsync(below_mask, p->d_below, n, hipMemcpyDeviceToHost, h->stream));
  CKH(hipStreamSynchronize(h->stream));
  return TPE_OK;
}

static int fit_one(tpe_handle_t h, int32_t family, const double *obs, int64_t n,
                   double prior_weight, double prior_mu, double prior_sigma, int32_t upper,
                   const double *pprior, int32_t lf, tpe_plan **pout) {
  tpe_plan *p;
  int rc = op_plan(h, family, 0, upper, 0, 0, 0, n, &p);
  if (rc) return rc;
  p->hps[0].prior_mu = prior_mu;
  p->hps[0].prior_sigma = prior_sigma;
  p->hps[0].upper = upper;
  if (pprior) {
    p->hps[0].flags |= TPE_PCHOICE;
    p->hps[0].pprior_begin = 0;
    CKH(hipMemcpyAsync(p->d_pprior, pprior, upper * 8, hipMemcpyHostToDevice, h->stream));
  }
  CKH(hipMemcpyAsync(p->d_hps, &p->hps[0], sizeof(tpe_hp), hipMemcpyHostToDevice, h->stream));
  if (n > 0) {
    CKH(hipMemcpyAsync(p->d_vals, obs, n * 8, hipMemcpyHostToDevice, h->stream));
    CKH(hipMemsetAsync(p->d_active, 1, n, h->stream));
    CKH(hipMemsetAsync(p->d_below, 1, n, h->stream));
  }
  if (n > 0) CKH(hipMemsetAsync(p->d_losses, 0, n * 8, h->stream));
  p->n = n;
  CKH(launch_fit(fit_args(p, (int32_t)n, prior_weight, lf, plan_fit_variant(p, true)), 1,
                 h->stream));
  *pout = p;
  return TPE_OK;
}

int tpe_parzen_fit(tpe_handle_t h, const double *obs, int64_t n, double prior_weight,
                   double prior_mu, double prior_sigma, int32_t lf, double *w, double *mu,
                   double *sigma) {
  if (!h) return TPE_E_INVALID;
  if (n < 0 || (n > 0 && !obs) || !w || !mu || !sigma) return fail(h, TPE_E_INVALID, "bad args");
  if (!(prior_sigma > 0)) return fail(h, TPE_E_INVALID, "prior_sigma <= 0");
  CKH(hipSetDevice(h->device));
  tpe_plan *p;
  int rc = fit_one(h, TPE_GMM, obs, n, prior_weight, prior_mu, prior_sigma, 1, nullptr, lf, &p);
  if (rc) return rc;
  const int64_t K = n + 1;
  CKH(hipMemcpyAsync(w, p->d_mw, K * 8, hipMemcpyDeviceToHost, h->stream));
  CKH(hipMemcpyAsync(mu, p->d_mmu, K * 8, hipMemcpyDeviceToHost, h->stream));
  CKH(hipMemcpyAsync(sigma, p->d_msig, K * 8, hipMemcpyDeviceToHost, h->stream));
  CKH(hipStreamSynchronize(h->stream));
  return TPE_OK;
}

int tpe_categorical_posterior(tpe_handle_t h, const int64_t *obs, int64_t n, int32_t upper,
                              double prior_weight, const double *pprior, int32_t lf,
                              double *p_out) {
  if (!h) return TPE_E_INVALID;
  if (n < 0 || (n > 0 && !obs) || upper <= 0 || !p_out) return fail(h, TPE_E_INVALID, "bad args");
  for (int64_t i = 0; i < n; ++i)
    if (obs[i] < 0) return fail(h, TPE_E_INVALID, "negative categorical observation");
  CKH(hipSetDevice(h->device));
  std::vector<double> dv(obs, obs + n);
  tpe_plan *p;
  int rc = fit_one(h, TPE_CAT, dv.data(), n, prior_weight, 0, 1, upper, pprior, lf, &p);
  if (rc) return rc;
  CKH(hipMemcpyAsync(p_out, p->d_mw, upper * 8, hipMemcpyDeviceToHost, h->stream));
  CKH(hipStreamSynchronize(h->stream));
  return TPE_OK;
}

int tpe_score(tpe_handle_t h, int32_t family, const double *x, int64_t n, const double *wb,
              const double *mb, const double *sb, int64_t kb, const double *wa, const double *ma,
              const double *sa, int64_t ka, double low, double high, double q, uint32_t flags,
              double *llik_b, double *llik_a, int64_t *best_index, double *best_score) {
  if (!h) return TPE_E_INVALID;
  if (bad_family(family) || n < 0 || kb <= 0 || ka <= 0 || !wb || !wa)
    return fail(h, TPE_E_INVALID, "bad args");
  if (family != TPE_CAT && (!mb || !sb || !ma || !sa)) return fail(h, TPE_E_INVALID, "bad args");
  if (family == TPE_CAT && kb != ka) return fail(h, TPE_E_INVALID, "p length mismatch");
  const bool hl = flags & TPE_HAS_LOW, hh = flags & TPE_HAS_HIGH;
  if (family != TPE_CAT && (hl || hh)) {
    if (hl != hh) return fail(h, TPE_E_INVALID, "one-sided truncation");
    if (!(low < high)) return fail(h, TPE_E_BOUNDS, "low >= high");
  }
  if (best_index) *best_index = -1;
  if (best_score) *best_score = NAN;
  if (n == 0) return TPE_OK;
  if (family == TPE_CAT) {
    for (int64_t i = 0; i < n; ++i)
      if (!(x[i] >= 0 && x[i] < kb && x[i] == std::floor(x[i])))
        return fail(h, TPE_E_INDEX, "categorical sample out of range");
  }
  if (family == TPE_LGMM && (flags & TPE_HAS_Q)) {
    const double hq = q / 2.0, eh = hh ? std::exp(high) : INFINITY;
    for (int64_t i = 0; i < n; ++i) {
      const double ub = std::min(x[i] + hq, eh);
      if (ub < 0) return fail(h, TPE_E_NEGATIVE, "negative arg to lognormal_cdf");
    }
  }
  CKH(hipSetDevice(h->device));
  tpe_plan *p;
  const int64_t kmax = std::max(kb, ka);
  int rc = op_plan(h, family, flags, family == TPE_CAT ? (int32_t)kb : 1, low, high, q,
                   std::max<int64_t>(kmax, 1), &p);
  if (rc) return rc;
  const int32_t kind = family == TPE_CAT ? 2 : ((flags & TPE_HAS_Q) ? 1 : 0);
  rc = put_mixture(h, p, 0, wb, mb, sb, kb, kind);
  if (rc) return rc;
  rc = put_mixture(h, p, 1, wa, ma, sa, ka, kind);
  if (rc) return rc;
  CKH(launch_prep(p->d_hps, 1, p->d_mw, p->d_mmu, p->d_msig, p->d_info, p->d_coef, p->d_coef32,
                  p->d_coefm, nullptr, p->d_coefe, p->kcap, p->d_scratch, h->stream));
  p->mom_w = switches().moment ? 16 : 0;
  p->mom_h = false;
  rc = ensure_ext(h, p, n);
  if (rc) return rc;
  CKH(hipMemcpyAsync(p->d_ext, x, n * 8, hipMemcpyHostToDevice, h->stream));
  rc = run_external(h, p, 0, p->d_ext, n, llik_b ? p->d_lb : nullptr,
                    llik_a ? p->d_la : nullptr, h->stream);
  if (rc) return rc;
  tpe_result r;
  CKH(hipMemcpyAsync(&r, p->d_results, sizeof(r), hipMemcpyDeviceToHost, h->stream));
  if (llik_b) CKH(hipMemcpyAsync(llik_b, p->d_lb, n * 8, hipMemcpyDeviceToHost, h->stream));
  if (llik_a) CKH(hipMemcpyAsync(llik_a, p->d_la, n * 8, hipMemcpyDeviceToHost, h->stream));
  CKH(hipStreamSynchronize(h->stream));
  if (best_index) *best_index = r.index;
  if (best_score) *best_score = r.score;
  return TPE_OK;
}

int tpe_lpdf(tpe_handle_t h, int32_t family, const double *x, int64_t n, const double *w,
             const double *mu, const double *sigma, int64_t k, double low, double high, double q,
             uint32_t flags, double *out) {
  if (!out && n > 0) return fail(h, TPE_E_INVALID, "bad args");
  return tpe_score(h, family, x, n, w, mu, sigma, k, w, mu, sigma, k, low, high, q, flags, out,
                   nullptr, nullptr, nullptr);
}

int tpe_sample(tpe_handle_t h, int32_t family, const double *w, const double *mu,
               const double *sigma, int64_t k, double low, double high, double q, uint32_t flags,
               uint64_t seed, uint64_t stream, int64_t offset, int64_t n, double *out) {
  if (!h) return TPE_E_INVALID;
  if (bad_family(family) || k <= 0 || !w || n < 0 || (n > 0 && !out))
    return fail(h, TPE_E_INVALID, "bad args");
  if (family != TPE_CAT && (!mu || !sigma)) return fail(h, TPE_E_INVALID, "bad args");
  const bool hl = flags & TPE_HAS_LOW, hh = flags & TPE_HAS_HIGH;
  if (family != TPE_CAT && (hl || hh)) {
    if (hl != hh) return fail(h, TPE_E_INVALID, "one-sided truncation");
    if (!(low < high)) return fail(h, TPE_E_BOUNDS, "low >= high");
  }
  if (n == 0) return TPE_OK;
  CKH(hipSetDevice(h->device));
  tpe_plan *p;
  int rc = op_plan(h, family, flags, family == TPE_CAT ? (int32_t)k : 1, low, high, q, k, &p);
  if (rc) return rc;
  const int32_t kind = family == TPE_CAT ? 2 : ((flags & TPE_HAS_Q) ? 1 : 0);
  rc = put_mixture(h, p, 0, w, mu, sigma, k, kind);
  if (rc) return rc;
  rc = put_mixture(h, p, 1, w, mu, sigma, k, kind);
  if (rc) return rc;
  CKH(launch_prep(p->d_hps, 1, p->d_mw, p->d_mmu, p->d_msig, p->d_info, p->d_coef, p->d_coef32,
                  p->d_coefm, nullptr, p->d_coefe, p->kcap, p->d_scratch, h->stream));
  p->mom_w = switches().moment ? 16 : 0;
  p->mom_h = false;
  rc = ensure_ext(h, p, n);
  if (rc) return rc;
  CKH(launch_sample(p->d_hps, p->d_mw, p->d_mmu, p->d_msig, p->d_info, seed, stream, offset, n,
                    p->d_ext, h->stream));
  CKH(hipMemcpyAsync(out, p->d_ext, n * 8, hipMemcpyDeviceToHost, h->stream));
  CKH(hipStreamSynchronize(h->stream));
  return TPE_OK;
}

// ---------------------------------------------------------------- plans
int tpe_plan_create(tpe_handle_t h, const tpe_space *space, int64_t max_trials, tpe_plan_t *out) {
  if (!h || !out) return TPE_E_INVALID;
  *out = nullptr;
  auto *p = new tpe_plan();
  int rc = plan_build(h, space, max_trials, p);
  if (rc) {
    plan_free_buffers(p);
    delete p;
    return rc;
  }
  *out = p;
  return TPE_OK;
}

int tpe_plan_destroy(tpe_plan_t p) {
  if (!p) return TPE_OK;
  (void)hipSetDevice(p->eng->device);
  graph_reset(p);
  plan_free_buffers(p);
  delete p;
  return TPE_OK;
}

int tpe_plan_num_levels(tpe_plan_t p, int32_t *n) {
  if (!p || !n) return TPE_E_INVALID;
  *n = (int32_t)p->levels.size();
  return TPE_OK;
}

int tpe_plan_set_history(tpe_plan_t p, const double *losses, const double *vals,
                         const uint8_t *active, int64_t n, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  return tpe_plan_update_history(p, n, 0, n, vals, active, n, 0, losses, on_device, stream);
}

// Rows live at stride ncap (FitArgs::ld), so appending trials leaves the rows
// already on the device in place: a call copies only the rows it is given.
int tpe_plan_update_history(tpe_plan_t p, int64_t n, int64_t row0, int64_t n_rows,
                            const double *vals, const uint8_t *active, int64_t src_ld,
                            int64_t loss0, const double *losses, int32_t on_device,
                            void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n < 0 || n > p->ncap) return fail(h, TPE_E_INVALID, "history larger than max_trials");
  if (row0 < 0 || n_rows < 0 || row0 + n_rows > n || loss0 < 0 || loss0 > n)
    return fail(h, TPE_E_INVALID, "history rows out of range");
  if (n_rows > 0 && (!vals || !active || src_ld < n_rows))
    return fail(h, TPE_E_INVALID, "bad history rows");
  if (loss0 < n && !losses) return fail(h, TPE_E_INVALID, "losses missing");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const int64_t n_loss = n - loss0;
  if (!on_device && n_rows * p->P <= kPatchVals && n_loss <= kPatchLoss) {
    // the fmin steady state (a row or two, a few losses): the values ride in
    // the kernel arguments -- no staging copy, no host synchronisation
    // -- and deferred: the next fit's blocks write it (one launch less per
    // fmin step); an earlier one still pending goes out first (an empty
    // update -- tpe.suggest's own push after the caller's -- keeps it)
    if (n_rows == 0 && n_loss == 0) {
      p->n = n;
      return TPE_OK;
    }
    int rc = flush_patch(h, p, st);
    if (rc) return rc;
    HistPatch &hp = p->pend;
    hp = HistPatch{};
    hp.row0 = row0; hp.n_rows = n_rows; hp.loss0 = loss0; hp.n_loss = n_loss;
    hp.ld = p->ncap; hp.P = p->P;
    for (int i = 0; i < p->P; ++i)
      for (int64_t r = 0; r < n_rows; ++r) {
        hp.vals[i * n_rows + r] = vals[(int64_t)i * src_ld + r];
        hp.active[i * n_rows + r] = active[(int64_t)i * src_ld + r];
      }
    for (int64_t i = 0; i < n_loss; ++i) hp.losses[i] = losses[i];
    p->has_pend = n_rows > 0 || n_loss > 0;
    p->n = n;
    return TPE_OK;
  }
  {
    const int rc = flush_patch(h, p, st);
    if (rc) return rc;
  }
  const hipMemcpyKind kd = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (n_rows > 0 && p->P > 0) {
    CKH(hipMemcpy2DAsync(p->d_vals + row0, (size_t)p->ncap * 8, vals, (size_t)src_ld * 8,
                         (size_t)n_rows * 8, (size_t)p->P, kd, st));
    CKH(hipMemcpy2DAsync(p->d_active + row0, (size_t)p->ncap, active, (size_t)src_ld,
                         (size_t)n_rows, (size_t)p->P, kd, st));
  }
  if (loss0 < n)
    CKH(hipMemcpyAsync(p->d_losses + loss0, losses, (size_t)(n - loss0) * 8, kd, st));
  p->n = n;
  if (!on_device) CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

// ---- hypervolume subset selection inside the front
namespace {

// the rounds and the surrogate column after the counts, on st (no host
// synchronisation); buffers at the plan's trial capacity on first use
int hv_rank(tpe_engine *h, tpe_plan *p, int64_t n, int32_t M, const int32_t *by,
            const int32_t *of, hipStream_t st) {
  const HvPlan hp = hv_plan(n, M, p->hv_n_pick, p->hv_S, p->hv_method);
  if (!hp.ok) return fail(h, TPE_E_INVALID, "set_objectives: the hypervolume setting is out of range");
  const size_t cap = (size_t)p->ncap;
  if (!p->d_hv_i32) {
    CKH(dalloc(&p->d_hv_i32, 2 * cap + 2 * (size_t)kHvMaxPick + 1));
    CKH(dalloc(&p->d_hv_f64, 3 * cap + (size_t)kHvMaxPick));
  }
  if (!hp.exact) {
    if (hp.words > p->hv_words_cap) {
      CKH(hipStreamSynchronize(st));  // (earlier rounds may still read the old words)
      dfree(p->d_hv_alive);
      p->d_hv_alive = nullptr;
      p->hv_words_cap = 0;
      CKH(dalloc(&p->d_hv_alive, hp.alive_words(p->ncap)));
      p->hv_words_cap = hp.words;
    }
    if (!p->d_hv_u) CKH(dalloc(&p->d_hv_u, (size_t)kHvMaxSamples * TPE_MAX_OBJ));
  }
  HvArgs a{};
  a.Y = p->d_obj; a.ld = p->ncap; a.n = n; a.M = M;
  for (int m = 0; m < TPE_MAX_OBJ; ++m) a.ref[m] = p->hv_ref[m];
  a.n_pick = hp.n_pick; a.S = hp.S; a.exact = hp.exact; a.seed = p->hv_seed;
  a.make_u = !hp.exact && !(p->hv_u_ok && p->hv_u_seed == p->hv_seed && p->hv_u_S == hp.S &&
                            p->hv_u_M == M);
  a.dominated_by = by; a.dominates = of;
  a.state = p->d_hv_i32; a.cnt = p->d_hv_i32 + cap;
  a.picks = p->d_hv_i32 + 2 * cap; a.counts = a.picks + kHvMaxPick;
  a.n_picked = a.counts + kHvMaxPick;
  a.vol = p->d_hv_f64; a.right = p->d_hv_f64 + cap; a.top = p->d_hv_f64 + 2 * cap;
  a.keys = p->d_hv_f64 + 3 * cap;
  a.alive = p->d_hv_alive; a.u = p->d_hv_u;
  a.losses = p->d_losses;
  if (a.make_u) p->hv_u_ok = false;
  CKH(launch_hv_select(a, st));
  if (!hp.exact) {
    p->hv_u_ok = true; p->hv_u_seed = p->hv_seed; p->hv_u_S = hp.S; p->hv_u_M = M;
  }
  p->hv_last_pick = hp.n_pick;
  p->hv_last_exact = hp.exact;
  return TPE_OK;
}

}  // namespace

int tpe_plan_set_hv(tpe_plan_t p, int32_t mode, const double *ref, int32_t n_obj, int32_t n_pick,
                    int32_t n_samples, uint64_t seed, int32_t method) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (mode == 0) {
    p->hv_mode = 0;
    return TPE_OK;
  }
  if (mode != 1) return fail(h, TPE_E_INVALID, "set_hv: mode is 0 or 1");
  if (n_obj < 1 || n_obj > TPE_MAX_OBJ)
    return fail(h, TPE_E_INVALID, "set_hv: need 1 <= n_obj <= TPE_MAX_OBJ");
  if (!ref) return fail(h, TPE_E_INVALID, "set_hv: ref must not be null");
  for (int m = 0; m < n_obj; ++m)
    if (!std::isfinite(ref[m])) return fail(h, TPE_E_INVALID, "set_hv: ref must be finite");
  if (n_pick < 1 || n_pick > kHvMaxPick)
    return fail(h, TPE_E_INVALID, "set_hv: need 1 <= n_pick <= 256");
  if (n_samples < kHvMinSamples || n_samples > kHvMaxSamples || n_samples % kHvWord != 0)
    return fail(h, TPE_E_INVALID, "set_hv: n_samples is a multiple of 64 in [64, 4096]");
  if (method != kHvAuto && method != kHvExact && method != kHvMc)
    return fail(h, TPE_E_INVALID, "set_hv: method is 0 (auto), 1 (exact) or 2 (Monte-Carlo)");
  if (method == kHvExact && n_obj != 2)
    return fail(h, TPE_E_INVALID, "set_hv: the exact method needs n_obj = 2");
  p->hv_mode = 1;
  p->hv_M = n_obj;
  p->hv_n_pick = n_pick;
  p->hv_S = n_samples;
  p->hv_seed = seed;
  p->hv_method = method;
  for (int m = 0; m < TPE_MAX_OBJ; ++m) p->hv_ref[m] = m < n_obj ? ref[m] : 0.0;
  return TPE_OK;
}

int tpe_plan_hv_get(tpe_plan_t p, int32_t *picks, double *keys, int32_t *counts,
                    int32_t *n_picked, int32_t cap) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (p->pareto_n < 0) return fail(h, TPE_E_INVALID, "hv_get: no ranking to read");
  if (cap < 0) return fail(h, TPE_E_INVALID, "hv_get: cap must not be negative");
  if (n_picked) *n_picked = 0;
  if (p->hv_last_pick == 0) return TPE_OK;  // the last ranking ran no selection
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const size_t ncap = (size_t)p->ncap;
  const size_t k = (size_t)std::min<int32_t>(cap, p->hv_last_pick);
  const int32_t *d_picks = p->d_hv_i32 + 2 * ncap;
  if (picks && k) CKH(hipMemcpy(picks, d_picks, k * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (counts && k)
    CKH(hipMemcpy(counts, d_picks + kHvMaxPick, k * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (keys && k) CKH(hipMemcpy(keys, p->d_hv_f64 + 3 * ncap, k * 8, hipMemcpyDeviceToHost));
  if (n_picked)
    CKH(hipMemcpy(n_picked, d_picks + 2 * kHvMaxPick, sizeof(int32_t), hipMemcpyDeviceToHost));
  return TPE_OK;
}

// ---- multi-objective TPE: the loss column from a Pareto ranking
// Order against the deferred history patch: the patch (if any) is written
// first, on the same stream, so the surrogate column is the last writer of
// losses [0, n).
int tpe_plan_set_objectives(tpe_plan_t p, const double *Y, int32_t n_obj, int64_t n, int64_t ld,
                            int64_t obj0, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n_obj < 1 || n_obj > TPE_MAX_OBJ)
    return fail(h, TPE_E_INVALID, "set_objectives: need 1 <= n_obj <= TPE_MAX_OBJ");
  if (n != p->n) return fail(h, TPE_E_INVALID, "set_objectives: n is not the history length");
  if (!Y) return fail(h, TPE_E_INVALID, "set_objectives: Y must not be null");
  if (obj0 < 0 || obj0 > n) return fail(h, TPE_E_INVALID, "set_objectives: need 0 <= obj0 <= n");
  if (ld < n - obj0) return fail(h, TPE_E_INVALID, "set_objectives: ld < n - obj0");
  if (obj0 > 0 && (p->obj_M != n_obj || obj0 > p->obj_n))
    return fail(h, TPE_E_INVALID,
                "set_objectives: the rows below obj0 are not on the device with this n_obj");
  if (p->hv_mode && p->hv_M != n_obj)
    return fail(h, TPE_E_INVALID, "set_objectives: n_obj is not that of tpe_plan_set_hv");
  if (n == 0) {  // an empty history: nothing to rank
    p->obj_M = n_obj;
    p->obj_n = 0;
    p->pareto_n = 0;
    p->hv_last_pick = 0;
    return TPE_OK;
  }
  const ParetoPlan pp = pareto_plan(n, n_obj, p->pareto_force);
  if (!pp.ok) return fail(h, TPE_E_INVALID, "set_objectives: need (n + 1)^2 < 2^53");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  if (!p->d_obj) {
    CKH(dalloc(&p->d_obj, (size_t)TPE_MAX_OBJ * (size_t)p->ncap));
    CKH(dalloc(&p->d_pcount, 2 * (size_t)p->ncap));
  }
  {
    const int rc = flush_patch(h, p, st);
    if (rc) return rc;
  }
  p->obj_M = 0;  // (not a consistent matrix until the copy is enqueued)
  if (obj0 < n)
    CKH(hipMemcpy2DAsync(p->d_obj + obj0, (size_t)p->ncap * 8, Y, (size_t)ld * 8,
                         (size_t)(n - obj0) * 8, (size_t)n_obj,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  p->obj_M = n_obj;
  p->obj_n = n;
  int32_t *by = p->d_pcount, *of = p->d_pcount + p->ncap;
  p->pareto_n = -1;
  CKH(hipMemsetAsync(p->d_pcount, 0, 2 * (size_t)p->ncap * sizeof(int32_t), st));
  CKH(launch_pareto_count(p->d_obj, p->ncap, n, n_obj, pp.per_split, pp.splits, by, of, st));
  p->hv_last_pick = 0;
  if (p->hv_mode && n_obj >= 2) {
    const int rc = hv_rank(h, p, n, n_obj, by, of, st);
    if (rc) return rc;
  } else {
    CKH(launch_pareto_loss(p->d_obj, p->ncap, n, n_obj, by, of, p->d_losses, st));
  }
  p->pareto_n = n;
  // a new loss column: nothing fitted on the old one stands
  p->last_nb = -1;
  p->tab_built = false;
  p->joint_ok = false;
  p->group_ok = false;
  if (!on_device) CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

int tpe_plan_pareto_get(tpe_plan_t p, int32_t *dominated_by, int32_t *dominates, double *loss,
                        int64_t n) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (p->pareto_n < 0 || n != p->pareto_n)
    return fail(h, TPE_E_INVALID, "pareto_get: n is not that of the last tpe_plan_set_objectives");
  if (n == 0) return TPE_OK;
  CKH(hipSetDevice(h->device));
  {
    const int rc = flush_patch(h, p, h->stream);
    if (rc) return rc;
  }
  CKH(hipDeviceSynchronize());
  if (dominated_by)
    CKH(hipMemcpy(dominated_by, p->d_pcount, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (dominates)
    CKH(hipMemcpy(dominates, p->d_pcount + p->ncap, (size_t)n * sizeof(int32_t),
                  hipMemcpyDeviceToHost));
  if (loss) CKH(hipMemcpy(loss, p->d_losses, (size_t)n * 8, hipMemcpyDeviceToHost));
  return TPE_OK;
}

int tpe_plan_pareto_shape(tpe_plan_t p, int64_t n, int32_t n_obj, int64_t force_splits,
                          int64_t *out) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (!out) return fail(h, TPE_E_INVALID, "pareto_shape: out must not be null");
  const int64_t force = force_splits < 0 ? p->pareto_force : force_splits;
  const ParetoPlan pp = pareto_plan(n, n_obj, force);
  if (!pp.ok) return fail(h, TPE_E_INVALID, "pareto_shape: (n, n_obj) out of range");
  p->pareto_force = force;
  out[0] = kParetoTile;
  out[1] = TPE_MAX_OBJ;
  out[2] = pp.splits;
  out[3] = pp.tiles;
  return TPE_OK;
}
static_assert(kParetoMaxObj == TPE_MAX_OBJ, "tpe_pareto_plan.hpp's constant is the header's");

int tpe_plan_fit(tpe_plan_t p, double gamma, int32_t gamma_cap, double prior_weight, int32_t lf,
                 void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const double nbf = std::ceil(gamma * std::sqrt((double)p->n));
  const int32_t nb = (int32_t)std::max(0.0, std::min<double>(nbf, gamma_cap));
  const FitVariant f = plan_fit_variant(p, true);
  const int rc = fit_launch(h, p, fit_args(p, nb, prior_weight, lf, f), p->P, st);
  if (rc) return rc;
  p->last_nb = nb;
  return TPE_OK;
}

int tpe_plan_get_mixture(tpe_plan_t p, int32_t hp, int32_t side, double *w, double *mu,
                         double *sigma, int64_t cap, int64_t *k) {
  if (!p || !k) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (hp < 0 || hp >= p->P || side < 0 || side > 1) return fail(h, TPE_E_INVALID, "bad hp/side");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const int64_t slot = 2 * (int64_t)hp + side;
  MixInfo mi;
  CKH(hipMemcpy(&mi, p->d_info + slot, sizeof(mi), hipMemcpyDeviceToHost));
  *k = mi.K;
  if (mi.K > cap) return fail(h, TPE_E_INVALID, "capacity too small");
  if (w) CKH(hipMemcpy(w, p->d_mw + slot * p->kcap, mi.K * 8, hipMemcpyDeviceToHost));
  if (mu) CKH(hipMemcpy(mu, p->d_mmu + slot * p->kcap, mi.K * 8, hipMemcpyDeviceToHost));
  if (sigma) CKH(hipMemcpy(sigma, p->d_msig + slot * p->kcap, mi.K * 8, hipMemcpyDeviceToHost));
  return TPE_OK;
}

int tpe_plan_get_table(tpe_plan_t p, int32_t hp, int32_t side, int32_t which, void *out,
                       int64_t cap_bytes, int64_t *bytes) {
  if (!p || !bytes) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (hp < 0 || hp >= p->P || side < 0 || side > 1 || which < 0 || which > 4)
    return fail(h, TPE_E_INVALID, "bad hp/side/table");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const int64_t slot = 2 * (int64_t)hp + side;
  const void *src = nullptr;
  if (which == 0) {
    *bytes = p->kcap * (int64_t)sizeof(Coef);
    src = p->d_coef + slot * p->kcap;
  } else if (which == 1) {
    *bytes = p->kcap / kCoefBlock * (int64_t)sizeof(Coef32);
    src = p->d_coef32 + slot * (p->kcap / kCoefBlock);
  } else if (which == 2) {
    *bytes = mom_stride(p->kcap) * (int64_t)sizeof(CoefM);
    src = p->d_coefm + slot * mom_stride(p->kcap);
  } else if (which == 3) {
    *bytes = p->kcap / kCoefBlock * (int64_t)sizeof(CoefM8);
    src = p->d_coefm8 + slot * (p->kcap / kCoefBlock);
  } else {
    *bytes = mom_stride(p->kcap) * (int64_t)sizeof(CoefM8);
    src = p->d_coefmh + slot * mom_stride(p->kcap);
  }
  if (!out) return TPE_OK;
  if (*bytes > cap_bytes) return fail(h, TPE_E_INVALID, "capacity too small");
  CKH(hipMemcpy(out, src, (size_t)*bytes, hipMemcpyDeviceToHost));
  return TPE_OK;
}

int tpe_plan_suggest(tpe_plan_t p, const uint64_t *seeds, int64_t n_sug, int64_t n_cand,
                     int64_t cand_begin, int32_t level, tpe_result *out, int32_t out_on_device,
                     void *stream) {
  return tpe_plan_suggest_shard(p, seeds, n_sug, cand_begin + n_cand, cand_begin, n_cand, level,
                                out, out_on_device, stream);
}

int tpe_plan_suggest_shard(tpe_plan_t p, const uint64_t *seeds, int64_t n_sug, int64_t n_total,
                           int64_t cand_begin, int64_t n_cand, int32_t level, tpe_result *out,
                           int32_t out_on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n_sug <= 0 || n_cand < 0 || cand_begin < 0 || !seeds || n_total < cand_begin + n_cand)
    return fail(h, TPE_E_INVALID, "bad args");
  if (level >= (int32_t)p->levels.size()) return fail(h, TPE_E_INVALID, "bad level");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  int rc = ensure_suggest_state(h, p, n_sug, 1);
  if (rc) return rc;
  p->h_seeds.assign(seeds, seeds + n_sug);
  if (n_sug > kInlineSeeds)
    CKH(hipMemcpyAsync(p->d_seeds, seeds, n_sug * 8, hipMemcpyHostToDevice, st));
  if (p->prof_cap > 0) CKH(hipEventRecord(p->ev0, st));
  const int l0 = level < 0 ? 0 : level;
  const int l1 = level < 0 ? (int)p->levels.size() : level + 1;
  // (the tables of the plan's last fit are the ones in place)
  const StepShape s = step_shape(p, n_sug, n_cand, cand_begin, n_total, p->last_nb,
                                 FitVariant{fit_small(p->n), p->mom_w, p->mom_h});
  for (int l = l0; l < l1; ++l) {
    rc = run_level(h, p, l, s, st);
    if (rc) return rc;
  }
  if (p->prof_cap > 0) CKH(hipEventRecord(p->ev1, st));
  p->timed = true;
  p->evs = p->prof_cap > 0;
  p->last_ncand = n_cand;
  p->last_nsug = n_sug;
  p->last_level = level;
  return copy_results(h, p, n_sug, out, out_on_device, st);
}

// ---- fit + suggest as one captured graph ---------------------------------
namespace {

// enqueue fit + every level's suggest on st (eager or under capture)
// s: the step's shape (tpe_plan_fit_suggest), its fit variant included
int enqueue_step(tpe_engine *h, tpe_plan *p, int32_t nb, double prior_weight, int32_t lf,
                 const StepShape &s, hipStream_t st) {
  {
    const int rc = fit_launch(h, p, fit_args(p, nb, prior_weight, lf, s.fit), p->P, st);
    if (rc) return rc;
  }
  p->last_nb = nb;
  for (int l = 0; l < (int)p->levels.size(); ++l) {
    const int rc = run_level(h, p, l, s, st);
    if (rc) return rc;
  }
  return TPE_OK;
}

// capture the step (s: its shape, capturing), instantiate it and find the
// nodes patched per call
int capture_step(tpe_engine *h, tpe_plan *p, int32_t nb, double prior_weight, int32_t lf,
                 const StepShape &s, hipStream_t st) {
  graph_reset(p);
  CKH(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue_step(h, p, nb, prior_weight, lf, s, st);
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(st, &g);
  if (rc || ec != hipSuccess || !g) {
    if (g) (void)hipGraphDestroy(g);
    return rc ? rc : fail(h, TPE_E_HIP, "graph capture failed");
  }
  p->graph = g;
  p->graph_mom_w = p->mom_w;  // the table the captured fit writes (its args are fixed)
  p->graph_mom_h = p->mom_h;
  p->graph_tab = p->tab_built;  // (the build node, if the step has one)
  CKH(hipGraphInstantiate(&p->graph_exec, g, nullptr, nullptr, 0));
  size_t nn = 0;
  CKH(hipGraphGetNodes(g, nullptr, &nn));
  std::vector<hipGraphNode_t> nodes(nn);
  CKH(hipGraphGetNodes(g, nodes.data(), &nn));
  for (hipGraphNode_t nd : nodes) {
    hipGraphNodeType ty;
    CKH(hipGraphNodeGetType(nd, &ty));
    if (ty != hipGraphNodeTypeKernel) continue;
    hipKernelNodeParams kp{};
    CKH(hipGraphKernelNodeGetParams(nd, &kp));
    if (kp.func == fit_kernel_fn(true) || kp.func == fit_kernel_fn(false)) {
      p->fit_nodes.push_back(nd);
      p->fit_params.push_back(kp);
      p->fit_args0.push_back(*static_cast<const FitArgs *>(kp.kernelParams[0]));
    } else if (is_draw_kernel_fn(kp.func) || kp.func == lattice_draw_kernel_fn()) {
      p->draw_nodes.push_back(nd);
      p->draw_params.push_back(kp);
      p->draw_args0.push_back(*static_cast<const ScoreArgs *>(kp.kernelParams[0]));
    }
  }
  if (p->fit_nodes.size() != 1) {
    graph_reset(p);
    return fail(h, TPE_E_HIP, "graph capture: fit node not found");
  }
  p->graph_ok = true;
  return TPE_OK;
}

// patch this call's history length / n_below and seeds, then launch
int launch_step(tpe_engine *h, tpe_plan *p, int32_t nb, const uint64_t *seeds, int64_t n_sug,
                hipStream_t st) {
  for (size_t i = 0; i < p->fit_nodes.size(); ++i) {
    FitArgs fa = p->fit_args0[i];
    fa.n = p->n;
    fa.n_below = nb;
    HistPatch none{};  // (the caller flushed any deferred history update)
    void *args[2] = {&fa, &none};
    hipKernelNodeParams kp = p->fit_params[i];
    kp.kernelParams = args;
    kp.extra = nullptr;
    CKH(hipGraphExecKernelNodeSetParams(p->graph_exec, p->fit_nodes[i], &kp));
  }
  for (size_t i = 0; i < p->draw_nodes.size(); ++i) {
    ScoreArgs da = p->draw_args0[i];
    for (int64_t j = 0; j < n_sug; ++j) da.seed_inline[j] = seeds[j];
    da.n_inline_seeds = (int32_t)n_sug;
    hipKernelNodeParams kp = p->draw_params[i];
    // k_lattice<true> (fused draw) also takes its jobs and output pointer,
    // k_draw_sorted its position buffer
    LatJobs jobs{};
    double2 *lat_out = nullptr;
    int32_t *pos_out = nullptr;
    const DrawZone *zones = nullptr;  // (k_draw_sorted_screen's zones and counters)
    unsigned long long *stats = nullptr;
    int32_t run = 0;  // (k_draw_sorted_screen_run's sort blocks per block)
    void *args[5] = {&da, &jobs, &lat_out, &stats, &run};
    if (kp.func == lattice_draw_kernel_fn()) {
      jobs = *static_cast<const LatJobs *>(kp.kernelParams[1]);
      lat_out = *static_cast<double2 *const *>(kp.kernelParams[2]);
    } else if (is_sorted_draw_kernel_fn(kp.func)) {
      pos_out = *static_cast<int32_t *const *>(kp.kernelParams[1]);
      args[1] = &pos_out;
      if (is_screen_draw_kernel_fn(kp.func)) {
        zones = *static_cast<const DrawZone *const *>(kp.kernelParams[2]);
        stats = *static_cast<unsigned long long *const *>(kp.kernelParams[3]);
        args[2] = &zones;
        if (is_screen_run_kernel_fn(kp.func)) run = *static_cast<const int32_t *>(kp.kernelParams[4]);
      }
    }
    kp.kernelParams = args;
    kp.extra = nullptr;
    CKH(hipGraphExecKernelNodeSetParams(p->graph_exec, p->draw_nodes[i], &kp));
  }
  CKH(hipGraphLaunch(p->graph_exec, st));
  p->last_nb = nb;
  p->mom_w = p->graph_mom_w;  // (no fit_args on replay: the captured fit's table)
  p->mom_h = p->graph_mom_h;
  p->tab_built = p->graph_tab;
  p->joint_ok = false;  // (a new fit epoch, fitted with the captured node's arguments)
  p->group_ok = false;
  p->fit_pw = p->fit_args0[0].prior_weight;
  p->fit_lf = p->fit_args0[0].lf;
  return TPE_OK;
}

}  // namespace

int tpe_plan_fit_suggest(tpe_plan_t p, double gamma, int32_t gamma_cap, double prior_weight,
                         int32_t lf, const uint64_t *seeds, int64_t n_sug, int64_t n_cand,
                         tpe_result *out, int32_t out_on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n_sug <= 0 || n_cand < 0 || !seeds) return fail(h, TPE_E_INVALID, "bad args");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const double nbf = std::ceil(gamma * std::sqrt((double)p->n));
  const int32_t nb = (int32_t)std::max(0.0, std::min<double>(nbf, gamma_cap));
  // (graph replay is opt-in: Switches::graph)
  const bool graphable =
      switches().graph && n_sug <= kInlineSeeds && p->prof_cap == 0 && !p->census;
  // the step's shape, built once: run_level plans every launch from it, and
  // with `capturing` set it is the key of the captured graph
  StepShape shape = step_shape(p, n_sug, n_cand, 0, n_cand, nb,
                               plan_fit_variant(p, step_reads_moments(*p, n_sug, n_cand)));
  tpe_plan::StepKey key;
  key.prior_weight = prior_weight;
  key.lf = lf;
  key.stream = (void *)st;
  key.shape = shape;
  key.shape.capturing = true;
  int rc = ensure_suggest_state(h, p, n_sug, 1);
  if (rc) return rc;
  p->h_seeds.assign(seeds, seeds + n_sug);
  if (graphable) {  // (a graph's fit node carries no history patch)
    rc = flush_patch(h, p, st);
    if (rc) return rc;
  }
  if (!graphable || !((p->graph_ok && p->graph_key == key) || (p->pending && p->pending_key == key))) {
    // eager (first sight of this shape: it also sizes every buffer)
    if (n_sug > kInlineSeeds)
      CKH(hipMemcpyAsync(p->d_seeds, seeds, n_sug * 8, hipMemcpyHostToDevice, st));
    if (p->prof_cap > 0) CKH(hipEventRecord(p->ev0, st));
    // results to the host: the step's last launch may publish them itself
    // (run_level, tile_draw levels), with the pinned buffers in place first
    p->pub_fired = false;
    shape.publish = out && !out_on_device && switches().publish && p->prof_cap == 0 && !p->census;
    if (shape.publish) {
      rc = host_results(h, p, n_sug);
      if (rc) return rc;
    }
    rc = enqueue_step(h, p, nb, prior_weight, lf, shape, st);
    if (rc) {
      // (a publishing launch that went out counts its arrivals: clear the
      // ticket for the plan's next fused publish)
      if (p->pub_fired)
        (void)hipMemsetAsync(p->d_ticket + (size_t)p->s_cap * p->P, 0, sizeof(uint32_t), st);
      p->pub_fired = false;
      return rc;
    }
    if (p->prof_cap > 0) CKH(hipEventRecord(p->ev1, st));
    if (graphable && !(p->graph_ok && p->graph_key == key)) {
      p->pending = true;
      p->pending_key = key;
    }
  } else {
    if (!(p->graph_ok && p->graph_key == key)) {
      rc = capture_step(h, p, nb, prior_weight, lf, key.shape, st);
      if (rc) return rc;
      p->graph_key = key;
    }
    if (p->prof_cap > 0) CKH(hipEventRecord(p->ev0, st));
    rc = launch_step(h, p, nb, seeds, n_sug, st);
    if (rc) return rc;
    if (p->prof_cap > 0) CKH(hipEventRecord(p->ev1, st));
  }
  p->timed = true;
  p->evs = p->prof_cap > 0;
  p->last_ncand = n_cand;
  p->last_nsug = n_sug;
  p->last_level = -1;
  return copy_results(h, p, n_sug, out, out_on_device, st);
}

int tpe_plan_get_results(tpe_plan_t p, tpe_result *out, int32_t out_on_device, void *stream) {
  if (!p || !out) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  CKH(hipSetDevice(h->device));
  return copy_results(h, p, p->last_nsug, out, out_on_device, pick_stream(h, stream));
}

const tpe_result *tpe_plan_results_device(tpe_plan_t p) {
  return p ? reinterpret_cast<const tpe_result *>(p->d_results) : nullptr;
}

int tpe_plan_merge(tpe_plan_t p, const tpe_result *gathered, int32_t world, int32_t level,
                   tpe_result *out, int32_t out_on_device, void *stream) {
  if (!p || !gathered || world <= 0) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (level < 0 || level >= (int32_t)p->levels.size()) return fail(h, TPE_E_INVALID, "bad level");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const int32_t ns = (int32_t)p->levels[level].size();
  // out_on_device 2: out already holds this plan's records but for the
  // level's merged slots (the level's tpe_plan_suggest_shard wrote them
  // there); k_merge stores those slots into out too, so no copy launch
  // follows the merge
  const bool direct = out && out_on_device == 2;
  CKH(launch_merge(p->d_level_hps + p->level_off[level], ns, (int32_t)p->last_nsug, p->P, world,
                   reinterpret_cast<const Partial *>(gathered), p->d_results, st,
                   direct ? reinterpret_cast<Partial *>(out) : nullptr));
  if (direct) {
    p->pub_fired = false;
    return TPE_OK;
  }
  return copy_results(h, p, p->last_nsug, out, out_on_device, st);
}

int tpe_plan_score_candidates(tpe_plan_t p, int32_t hp, const double *x, int64_t n,
                              double *llik_b, double *llik_a, int64_t *best_index,
                              double *best_score) {
  return tpe_plan_score_candidates_sorted(p, hp, -1, x, n, llik_b, llik_a, best_index,
                                          best_score);
}

int tpe_plan_score_candidates_sorted(tpe_plan_t p, int32_t hp, int32_t mode, const double *x,
                                     int64_t n, double *llik_b, double *llik_a,
                                     int64_t *best_index, double *best_score) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (hp < 0 || hp >= p->P || n < 0 || (n > 0 && !x) || mode < -1 || mode > 4)
    return fail(h, TPE_E_INVALID, "bad args");
  if (n > (int64_t)INT32_MAX) return fail(h, TPE_E_INVALID, "too many candidates");
  if (best_index) *best_index = -1;
  if (best_score) *best_score = NAN;
  if (n == 0) return TPE_OK;
  const tpe_hp &H = p->hps[hp];
  if (H.family == TPE_CAT) {
    for (int64_t i = 0; i < n; ++i)
      if (!(x[i] >= 0 && x[i] < H.upper && x[i] == std::floor(x[i])))
        return fail(h, TPE_E_INDEX, "categorical sample out of range");
  }
  CKH(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  CKH(hipDeviceSynchronize());
  int rc = ensure_ext(h, p, n);
  if (rc) return rc;
  CKH(hipMemcpyAsync(p->d_ext, x, n * 8, hipMemcpyHostToDevice, st));
  rc = run_external(h, p, hp, p->d_ext, n, llik_b ? p->d_lb : nullptr,
                    llik_a ? p->d_la : nullptr, st, mode);
  if (rc) return rc;
  tpe_result r;
  CKH(hipMemcpyAsync(&r, p->d_results + hp, sizeof(r), hipMemcpyDeviceToHost, st));
  if (llik_b) CKH(hipMemcpyAsync(llik_b, p->d_lb, n * 8, hipMemcpyDeviceToHost, st));
  if (llik_a) CKH(hipMemcpyAsync(llik_a, p->d_la, n * 8, hipMemcpyDeviceToHost, st));
  CKH(hipStreamSynchronize(st));
  if (best_index) *best_index = r.index;
  if (best_score) *best_score = r.score;
  return TPE_OK;
}

// Whole configurations under the last fit (tpe_points.hip).  Reads the fitted
// tables only: the history, a pending history patch, d_results and every other
// suggest state stay as they are.  Device mode enqueues three launches and
// returns; host mode stages through the plan's scratch and waits for its own
// stream only.
int tpe_plan_score_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld, double *total,
                          double *terms, uint8_t *active, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (m < 0 || ld < m) return fail(h, TPE_E_INVALID, "score_points: need 0 <= m <= ld");
  if (m > 0 && (!vals || !total))
    return fail(h, TPE_E_INVALID, "score_points: vals and total must not be null");
  if (m > (int64_t)INT32_MAX) return fail(h, TPE_E_INVALID, "score_points: too many configurations");
  if (m == 0) return TPE_OK;
  if (p->last_nb < 0)
    return fail(h, TPE_E_INVALID, "score_points: the plan has not been fitted (tpe_plan_fit first)");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  {
    const int rc = ensure_points(h, p, (size_t)m);
    if (rc) return rc;
  }
  CKH(hipMemsetAsync(p->d_pt_count, 0, (size_t)p->P * sizeof(uint32_t), st));
  PointsArgs a{};
  a.idx = p->d_pt_idx;
  a.count = p->d_pt_count;
  a.hps = p->d_hps;
  a.level_hps = p->d_level_hps;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.info = p->d_info;
  a.coef = p->d_coef;
  a.kcap = p->kcap;
  a.m = m;
  a.n_hp = p->P;
  if (dev) {
    a.vals = vals;
    a.ld = ld;
    a.total = total;
    a.terms = terms ? terms : p->d_pt_terms;
    a.term_ld = terms ? ld : m;
    a.active = active ? active : p->d_pt_act;
    a.act_ld = active ? ld : m;
    CKH(launch_points(a, st));
    return TPE_OK;
  }
  if (ld == m)  // (contiguous: one plain copy)
    CKH(hipMemcpyAsync(p->d_pt_vals, vals, (size_t)m * p->P * 8, hipMemcpyHostToDevice, st));
  else
    CKH(hipMemcpy2DAsync(p->d_pt_vals, (size_t)m * 8, vals, (size_t)ld * 8, (size_t)m * 8,
                         (size_t)p->P, hipMemcpyHostToDevice, st));
  a.vals = p->d_pt_vals;
  a.ld = m;
  a.total = p->d_pt_total;
  a.terms = p->d_pt_terms;
  a.active = p->d_pt_act;
  a.term_ld = a.act_ld = m;
  CKH(launch_points(a, st));
  CKH(hipMemcpyAsync(total, p->d_pt_total, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (terms)
    CKH(hipMemcpy2DAsync(terms, (size_t)ld * 8, p->d_pt_terms, (size_t)m * 8, (size_t)m * 8,
                         (size_t)p->P, hipMemcpyDeviceToHost, st));
  if (active)
    CKH(hipMemcpy2DAsync(active, (size_t)ld, p->d_pt_act, (size_t)m, (size_t)m, (size_t)p->P,
                         hipMemcpyDeviceToHost, st));
  CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

// Whole configurations drawn from the below mixtures of the last fit and
// scored (tpe_sample_points.hip, then tpe_points.hip's scoring launches).
// Reads d_info, d_coef and the mixtures only, as tpe_plan_score_points does.
int tpe_plan_sample_points(tpe_plan_t p, uint64_t seed, int64_t begin, int64_t m, int64_t ld,
                           double *vals, double *total, double *terms, uint8_t *active,
                           int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (m < 0 || ld < m) return fail(h, TPE_E_INVALID, "sample_points: need 0 <= m <= ld");
  if (begin < 0) return fail(h, TPE_E_INVALID, "sample_points: begin must not be negative");
  if (m > 0 && (!vals || !total))
    return fail(h, TPE_E_INVALID, "sample_points: vals and total must not be null");
  if (m > (int64_t)INT32_MAX) return fail(h, TPE_E_INVALID, "sample_points: too many configurations");
  if (m == 0) return TPE_OK;
  if (p->last_nb < 0)
    return fail(h, TPE_E_INVALID, "sample_points: the plan has not been fitted (tpe_plan_fit first)");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  {
    const int rc = ensure_points(h, p, (size_t)m);
    if (rc) return rc;
  }
  if (!p->d_pt_tab) CKH(hipMalloc(&p->d_pt_tab, sample_tables_bytes(p->P)));
  CKH(hipMemsetAsync(p->d_pt_count, 0, (size_t)p->P * sizeof(uint32_t), st));
  SampleArgs s{};
  PointsArgs &a = s.P;
  a.idx = p->d_pt_idx;
  a.count = p->d_pt_count;
  a.hps = p->d_hps;
  a.level_hps = p->d_level_hps;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.info = p->d_info;
  a.coef = p->d_coef;
  a.kcap = p->kcap;
  a.m = m;
  a.n_hp = p->P;
  s.mw = p->d_mw;
  s.mmu = p->d_mmu;
  s.msig = p->d_msig;
  s.tab = static_cast<DrawTableT<kTabCap> *>(p->d_pt_tab);
  s.seed = seed;
  s.begin = begin;
  if (dev) {
    s.out = vals;
    a.vals = vals;
    a.ld = ld;
    a.total = total;
    a.terms = terms ? terms : p->d_pt_terms;
    a.term_ld = terms ? ld : m;
    a.active = active ? active : p->d_pt_act;
    a.act_ld = active ? ld : m;
    CKH(launch_sample_points(s, st));
    return TPE_OK;
  }
  s.out = p->d_pt_vals;
  a.vals = p->d_pt_vals;
  a.ld = m;
  a.total = p->d_pt_total;
  a.terms = p->d_pt_terms;
  a.active = p->d_pt_act;
  a.term_ld = a.act_ld = m;
  CKH(launch_sample_points(s, st));
  CKH(hipMemcpy2DAsync(vals, (size_t)ld * 8, p->d_pt_vals, (size_t)m * 8, (size_t)m * 8,
                       (size_t)p->P, hipMemcpyDeviceToHost, st));
  CKH(hipMemcpyAsync(total, p->d_pt_total, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (terms)
    CKH(hipMemcpy2DAsync(terms, (size_t)ld * 8, p->d_pt_terms, (size_t)m * 8, (size_t)m * 8,
                         (size_t)p->P, hipMemcpyDeviceToHost, st));
  if (active)
    CKH(hipMemcpy2DAsync(active, (size_t)ld, p->d_pt_act, (size_t)m, (size_t)m, (size_t)p->P,
                         hipMemcpyDeviceToHost, st));
  CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

// ---- the joint model over the root hps (tpe_joint.hip) ----
namespace {

constexpr int64_t kJointLdsMax = 160 * 1024;  // k_joint_score's staged values (64 x 8 B a slot)

// the root dims of the plan's space and the buffers of its joint fit, once
int ensure_joint(tpe_engine *h, tpe_plan *p) {
  if (p->d_jtab) return TPE_OK;
  p->jdims.clear();
  p->jdim_of_hp.assign((size_t)p->P, -1);
  int32_t slot = 0;
  int64_t nopt = 0;
  for (int32_t i = 0; i < p->P; ++i) {
    const tpe_hp &x = p->hps[i];
    if (x.cond_count != 0) continue;
    JointDim d{};
    d.hp = i;
    d.kind = score_kind(x);
    d.slot = slot;
    d.upper = x.family == TPE_CAT ? x.upper : 0;
    d.opt_off = nopt;
    slot += joint_slots(d.kind);
    nopt += d.upper;
    p->jdim_of_hp[(size_t)i] = (int32_t)p->jdims.size();
    p->jdims.push_back(d);
  }
  p->j_slots = slot;
  p->j_nopt = nopt;
  const size_t D = p->jdims.size(), kc = (size_t)p->kcap;
  if ((int64_t)slot * 64 * 8 > kJointLdsMax)
    return fail(h, TPE_E_INVALID, "joint_fit: too many root hps for the scoring kernel's LDS");
  CKH(dalloc(&p->d_jdims, D));
  CKH(dalloc(&p->d_jdim_of_hp, (size_t)p->P));
  CKH(hipMemcpy(p->d_jdims, p->jdims.data(), D * sizeof(JointDim), hipMemcpyHostToDevice));
  CKH(hipMemcpy(p->d_jdim_of_hp, p->jdim_of_hp.data(), (size_t)p->P * 4, hipMemcpyHostToDevice));
  CKH(dalloc(&p->d_jrows, 2 * kc));
  CKH(dalloc(&p->d_jcount, (size_t)2));
  CKH(dalloc(&p->d_jside, (size_t)2));
  CKH(dalloc(&p->d_jkeys, 2 * D * kc));
  CKH(dalloc(&p->d_jw, 2 * kc));
  CKH(dalloc(&p->d_jcw, 2 * D * kc));
  CKH(dalloc(&p->d_jcmu, 2 * D * kc));
  CKH(dalloc(&p->d_jcsig, 2 * D * kc));
  CKH(dalloc(&p->d_joptlog, 2 * (size_t)nopt * 3));
  CKH(dalloc(&p->d_jpick, kc));
  CKH(dalloc(&p->d_jtab, 2 * (kc / kCoefBlock) * (size_t)joint_stride((int32_t)D)));
  return TPE_OK;
}

// per-call scratch of m joint scores
int ensure_joint_points(tpe_engine *h, tpe_plan *p, size_t m) {
  if (m > p->jpt_cap) {
    dfree(p->d_jsides); dfree(p->d_jjoint); dfree(p->d_jcomp);
    p->d_jsides = p->d_jjoint = nullptr;
    p->d_jcomp = nullptr;
    p->jpt_cap = 0;
    CKH(dalloc(&p->d_jsides, 2 * m));
    CKH(dalloc(&p->d_jjoint, m));
    CKH(dalloc(&p->d_jcomp, m));
    p->jpt_cap = m;
  }
  return TPE_OK;
}

PointsArgs points_args(tpe_plan *p, int64_t m) {
  PointsArgs a{};
  a.idx = p->d_pt_idx;
  a.count = p->d_pt_count;
  a.hps = p->d_hps;
  a.level_hps = p->d_level_hps;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.info = p->d_info;
  a.coef = p->d_coef;
  a.kcap = p->kcap;
  a.m = m;
  a.n_hp = p->P;
  return a;
}

// the joint launch arguments over a filled PointsArgs; joint: the caller's
// output or null (the plan's scratch)
JointScoreArgs joint_score_args(tpe_plan *p, const PointsArgs &a, double *joint) {
  JointScoreArgs j{};
  j.hps = p->d_hps;
  j.dims = p->d_jdims;
  j.n_dim = (int32_t)p->jdims.size();
  j.n_slots = p->j_slots;
  j.K[0] = p->jK[0];
  j.K[1] = p->jK[1];
  j.tab = p->d_jtab;
  j.tab_side = (p->kcap / kCoefBlock) * joint_stride(j.n_dim);
  j.optlog = p->d_joptlog;
  j.n_opt = p->j_nopt;
  j.vals = a.vals;
  j.m = a.m;
  j.ld = a.ld;
  j.sides = p->d_jsides;
  j.joint = joint ? joint : p->d_jjoint;
  j.terms = a.terms;
  j.term_ld = a.term_ld;
  j.n_hp = p->P;
  j.total = a.total;
  p->jpt_m = a.m;
  return j;
}

}  // namespace

int tpe_plan_joint_fit(tpe_plan_t p, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (p->last_nb < 0)
    return fail(h, TPE_E_INVALID, "joint_fit: the plan has not been fitted (tpe_plan_fit first)");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  {
    int rc = ensure_joint(h, p);
    if (rc) return rc;
    rc = flush_patch(h, p, st);
    if (rc) return rc;
  }
  // the split of the last fit, as a mask (k_split computes k_fit's threshold)
  FitArgs f{};
  f.losses = p->d_losses;
  f.n = p->n;
  f.n_below = p->last_nb;
  f.sortbuf = p->d_sortbuf;
  f.scap = p->scap;
  f.kcap = p->kcap;
  CKH(launch_split(f, p->d_below, st));
  JointFitArgs a{};
  a.hps = p->d_hps;
  a.dims = p->d_jdims;
  a.n_dim = (int32_t)p->jdims.size();
  a.n_hp = p->P;
  a.vals = p->d_vals;
  a.ld = p->ncap;
  a.n = p->n;
  a.below = p->d_below;
  a.lf = p->fit_lf;
  a.prior_weight = p->fit_pw;
  a.pprior = p->d_pprior;
  a.info = p->d_info;
  a.mw = p->d_mw;
  a.mmu = p->d_mmu;
  a.msig = p->d_msig;
  a.kcap = p->kcap;
  a.keys = p->d_jkeys;
  a.rows = p->d_jrows;
  a.count = p->d_jcount;
  a.side = p->d_jside;
  a.jw = p->d_jw;
  a.cw = p->d_jcw;
  a.cmu = p->d_jcmu;
  a.csig = p->d_jcsig;
  a.tab = p->d_jtab;
  a.optlog = p->d_joptlog;
  a.n_opt = p->j_nopt;
  CKH(launch_joint_fit(a, st));
  const int64_t nb = std::min<int64_t>(std::max<int64_t>(p->last_nb, 0), p->n);
  p->jK[0] = (int32_t)nb + 1;
  p->jK[1] = (int32_t)(p->n - nb) + 1;
  p->joint_ok = true;
  return TPE_OK;
}

int tpe_plan_joint_get_mixture(tpe_plan_t p, int32_t hp, int32_t side, double *w, double *mu,
                               double *sigma, int32_t *rows, int64_t cap, int64_t *k) {
  if (!p || !k) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (!p->joint_ok)
    return fail(h, TPE_E_INVALID, "joint_get_mixture: no joint fit (tpe_plan_joint_fit first)");
  if (hp < -1 || hp >= p->P || side < 0 || side > 1) return fail(h, TPE_E_INVALID, "bad hp/side");
  const int32_t d = hp < 0 ? -1 : p->jdim_of_hp[(size_t)hp];
  if (hp >= 0 && d < 0)
    return fail(h, TPE_E_INVALID, "joint_get_mixture: a conditional hp is not in the joint model");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const int64_t K = p->jK[side];
  *k = K;
  if (K > cap) return fail(h, TPE_E_INVALID, "capacity too small");
  const size_t bytes = (size_t)K * 8;
  if (rows)
    CKH(hipMemcpy(rows, p->d_jrows + side * p->kcap, (size_t)K * 4, hipMemcpyDeviceToHost));
  if (hp < 0) {  // the component weights themselves
    if (w) CKH(hipMemcpy(w, p->d_jw + side * p->kcap, bytes, hipMemcpyDeviceToHost));
    return TPE_OK;
  }
  const int64_t ds = ((int64_t)d * 2 + side) * p->kcap;
  if (w) CKH(hipMemcpy(w, p->d_jcw + ds, bytes, hipMemcpyDeviceToHost));
  if (mu) CKH(hipMemcpy(mu, p->d_jcmu + ds, bytes, hipMemcpyDeviceToHost));
  if (sigma) CKH(hipMemcpy(sigma, p->d_jcsig + ds, bytes, hipMemcpyDeviceToHost));
  return TPE_OK;
}

// Whole configurations under the joint model: tpe_plan_score_points' staging
// and conventions; the roots are scored together (k_joint_score), the
// conditional hps by k_score_points.
int tpe_plan_joint_score_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld,
                                double *total, double *joint, double *terms, uint8_t *active,
                                int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (m < 0 || ld < m) return fail(h, TPE_E_INVALID, "joint_score_points: need 0 <= m <= ld");
  if (m > 0 && (!vals || !total))
    return fail(h, TPE_E_INVALID, "joint_score_points: vals and total must not be null");
  if (m > (int64_t)INT32_MAX)
    return fail(h, TPE_E_INVALID, "joint_score_points: too many configurations");
  if (m == 0) return TPE_OK;
  if (!p->joint_ok)
    return fail(h, TPE_E_INVALID, "joint_score_points: no joint fit (tpe_plan_joint_fit first)");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  {
    int rc = ensure_points(h, p, (size_t)m);
    if (rc) return rc;
    rc = ensure_joint_points(h, p, (size_t)m);
    if (rc) return rc;
  }
  CKH(hipMemsetAsync(p->d_pt_count, 0, (size_t)p->P * sizeof(uint32_t), st));
  PointsArgs a = points_args(p, m);
  if (dev) {
    a.vals = vals;
    a.ld = ld;
    a.total = total;
    a.terms = terms ? terms : p->d_pt_terms;
    a.term_ld = terms ? ld : m;
    a.active = active ? active : p->d_pt_act;
    a.act_ld = active ? ld : m;
    CKH(launch_joint_points(joint_score_args(p, a, joint), a, true, st));
    return TPE_OK;
  }
  if (ld == m)  // (contiguous: one plain copy)
    CKH(hipMemcpyAsync(p->d_pt_vals, vals, (size_t)m * p->P * 8, hipMemcpyHostToDevice, st));
  else
    CKH(hipMemcpy2DAsync(p->d_pt_vals, (size_t)m * 8, vals, (size_t)ld * 8, (size_t)m * 8,
                         (size_t)p->P, hipMemcpyHostToDevice, st));
  a.vals = p->d_pt_vals;
  a.ld = m;
  a.total = p->d_pt_total;
  a.terms = p->d_pt_terms;
  a.active = p->d_pt_act;
  a.term_ld = a.act_ld = m;
  CKH(launch_joint_points(joint_score_args(p, a, nullptr), a, true, st));
  CKH(hipMemcpyAsync(total, p->d_pt_total, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (joint) CKH(hipMemcpyAsync(joint, p->d_jjoint, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (terms)
    CKH(hipMemcpy2DAsync(terms, (size_t)ld * 8, p->d_pt_terms, (size_t)m * 8, (size_t)m * 8,
                         (size_t)p->P, hipMemcpyDeviceToHost, st));
  if (active)
    CKH(hipMemcpy2DAsync(active, (size_t)ld, p->d_pt_act, (size_t)m, (size_t)m, (size_t)p->P,
                         hipMemcpyDeviceToHost, st));
  CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

int tpe_plan_joint_sides(tpe_plan_t p, double *below, double *above, int64_t m) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (m < 0 || m > p->jpt_m)
    return fail(h, TPE_E_INVALID, "joint_sides: more entries than the last joint score holds");
  if (m == 0) return TPE_OK;
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  if (below) CKH(hipMemcpy(below, p->d_jsides, (size_t)m * 8, hipMemcpyDeviceToHost));
  if (above)
    CKH(hipMemcpy(above, p->d_jsides + p->jpt_m, (size_t)m * 8, hipMemcpyDeviceToHost));
  return TPE_OK;
}

// Whole configurations drawn from the joint below model and scored: one
// component per configuration, every root value from it, the conditional hps
// by tpe_plan_sample_points' walk; then tpe_plan_joint_score_points' launches
// behind the draw's own lists.
int tpe_plan_joint_sample_points(tpe_plan_t p, uint64_t seed, int64_t begin, int64_t m, int64_t ld,
                                 double *vals, int32_t *comp, double *total, double *joint,
                                 double *terms, uint8_t *active, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (m < 0 || ld < m) return fail(h, TPE_E_INVALID, "joint_sample_points: need 0 <= m <= ld");
  if (begin < 0) return fail(h, TPE_E_INVALID, "joint_sample_points: begin must not be negative");
  if (m > 0 && (!vals || !total))
    return fail(h, TPE_E_INVALID, "joint_sample_points: vals and total must not be null");
  if (m > (int64_t)INT32_MAX)
    return fail(h, TPE_E_INVALID, "joint_sample_points: too many configurations");
  if (m == 0) return TPE_OK;
  if (!p->joint_ok)
    return fail(h, TPE_E_INVALID, "joint_sample_points: no joint fit (tpe_plan_joint_fit first)");
  const int64_t Kb = p->jK[0];
  if (Kb > kTabCap)
    return fail(h, TPE_E_INVALID, "joint_sample_points: more below components than a draw table holds");
  for (const JointDim &d : p->jdims)
    if (d.upper > kTabCap)
      return fail(h, TPE_E_INVALID, "joint_sample_points: a root choice has more options than a draw table holds");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  {
    int rc = ensure_points(h, p, (size_t)m);
    if (rc) return rc;
    rc = ensure_joint_points(h, p, (size_t)m);
    if (rc) return rc;
  }
  if (!p->d_jdraw) CKH(hipMalloc(&p->d_jdraw, joint_sample_tables_bytes(p->P)));
  const size_t need = (size_t)p->j_nopt * (size_t)Kb;
  if (need > p->joptcdf_cap) {
    dfree(p->d_joptcdf);
    p->d_joptcdf = nullptr;
    p->joptcdf_cap = 0;
    CKH(dalloc(&p->d_joptcdf, need));
    p->joptcdf_cap = need;
  }
  CKH(hipMemsetAsync(p->d_pt_count, 0, (size_t)p->P * sizeof(uint32_t), st));
  JointSampleArgs js{};
  SampleArgs &s = js.S;
  s.P = points_args(p, m);
  PointsArgs &a = s.P;
  s.mw = p->d_mw;
  s.mmu = p->d_mmu;
  s.msig = p->d_msig;
  s.tab = static_cast<DrawTableT<kTabCap> *>(p->d_jdraw);
  s.seed = seed;
  s.begin = begin;
  js.dims = p->d_jdims;
  js.n_dim = (int32_t)p->jdims.size();
  js.Kb = (int32_t)Kb;
  js.dim_of_hp = p->d_jdim_of_hp;
  js.jw = p->d_jw;
  js.cmu = p->d_jcmu;
  js.csig = p->d_jcsig;
  js.side = p->d_jside;
  js.pprior = p->d_pprior;
  js.prior_weight = p->fit_pw;
  js.pick_cdf = p->d_jpick;
  js.opt_cdf = p->d_joptcdf;
  if (dev) {
    s.out = vals;
    a.vals = vals;
    a.ld = ld;
    a.total = total;
    a.terms = terms ? terms : p->d_pt_terms;
    a.term_ld = terms ? ld : m;
    a.active = active ? active : p->d_pt_act;
    a.act_ld = active ? ld : m;
    js.comp = comp;
    CKH(launch_joint_sample(js, st));
    CKH(launch_joint_points(joint_score_args(p, a, joint), a, false, st));
    return TPE_OK;
  }
  s.out = p->d_pt_vals;
  a.vals = p->d_pt_vals;
  a.ld = m;
  a.total = p->d_pt_total;
  a.terms = p->d_pt_terms;
  a.active = p->d_pt_act;
  a.term_ld = a.act_ld = m;
  js.comp = comp ? p->d_jcomp : nullptr;
  CKH(launch_joint_sample(js, st));
  CKH(launch_joint_points(joint_score_args(p, a, nullptr), a, false, st));
  CKH(hipMemcpy2DAsync(vals, (size_t)ld * 8, p->d_pt_vals, (size_t)m * 8, (size_t)m * 8,
                       (size_t)p->P, hipMemcpyDeviceToHost, st));
  CKH(hipMemcpyAsync(total, p->d_pt_total, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (comp) CKH(hipMemcpyAsync(comp, p->d_jcomp, (size_t)m * 4, hipMemcpyDeviceToHost, st));
  if (joint) CKH(hipMemcpyAsync(joint, p->d_jjoint, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (terms)
    CKH(hipMemcpy2DAsync(terms, (size_t)ld * 8, p->d_pt_terms, (size_t)m * 8, (size_t)m * 8,
                         (size_t)p->P, hipMemcpyDeviceToHost, st));
  if (active)
    CKH(hipMemcpy2DAsync(active, (size_t)ld, p->d_pt_act, (size_t)m, (size_t)m, (size_t)p->P,
                         hipMemcpyDeviceToHost, st));
  CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

// ---- one joint model per group of hps (tpe_group.hip, tpe_group_plan.hpp) ----
namespace {

// the partition of the plan's space (host only; no device needed)
void ensure_group_shape(tpe_plan *p) {
  if (!p->gpart.group_of_hp.empty()) return;
  p->gpart = group_partition(p->hps, p->cond_parent, p->cond_branch);
  std::vector<int32_t> lh;
  for (auto &l : p->levels) lh.insert(lh.end(), l.begin(), l.end());
  p->glay = group_layout(p->gpart, p->hps, lh, p->kcap);
}

// the buffers of the plan's group fit
int alloc_group(tpe_engine *h, tpe_plan *p) {
  const GroupLayout &L = p->glay;
  if (p->gpart.members[0].empty())
    return fail(h, TPE_E_INVALID, "group_fit: the space has no unconditional hp");
  if ((int64_t)L.max_slots * 64 * 8 > kJointLdsMax)
    return fail(h, TPE_E_INVALID, "group_fit: a group has too many hps for the scoring kernel's LDS");
  const size_t P = (size_t)p->P, G = L.groups.size(), kc = (size_t)p->kcap;
  CKH(dalloc(&p->d_gdims, P));
  CKH(dalloc(&p->d_ggroups, G));
  CKH(dalloc(&p->d_gdim_of_hp, P));
  CKH(dalloc(&p->d_ggroup_of_hp, P));
  CKH(hipMemcpy(p->d_gdims, L.dims.data(), P * sizeof(JointDim), hipMemcpyHostToDevice));
  CKH(hipMemcpy(p->d_ggroups, L.groups.data(), G * sizeof(GroupDesc), hipMemcpyHostToDevice));
  CKH(hipMemcpy(p->d_gdim_of_hp, L.dim_of_hp.data(), P * 4, hipMemcpyHostToDevice));
  CKH(hipMemcpy(p->d_ggroup_of_hp, p->gpart.group_of_hp.data(), P * 4, hipMemcpyHostToDevice));
  CKH(dalloc(&p->d_grows, 2 * G * kc));
  CKH(dalloc(&p->d_gcount, 2 * G));
  CKH(dalloc(&p->d_gside, 2 * G));
  CKH(dalloc(&p->d_gkeys, 2 * P * kc));
  CKH(dalloc(&p->d_gw, 2 * G * kc));
  CKH(dalloc(&p->d_gcw, 2 * P * kc));
  CKH(dalloc(&p->d_gcmu, 2 * P * kc));
  CKH(dalloc(&p->d_gcsig, 2 * P * kc));
  CKH(dalloc(&p->d_goptlog, 2 * (size_t)L.n_opt * 3));
  CKH(dalloc(&p->d_gpick, G * kc));
  CKH(dalloc(&p->d_gtab, (size_t)L.tab_doubles));
  return TPE_OK;
}

// ... once; a failure part-way leaves none of them behind
int ensure_group(tpe_engine *h, tpe_plan *p) {
  if (p->group_ready) return TPE_OK;
  ensure_group_shape(p);
  const int rc = alloc_group(h, p);
  if (rc) {
    void **bufs[] = {(void **)&p->d_gdims, (void **)&p->d_ggroups, (void **)&p->d_gdim_of_hp,
                     (void **)&p->d_ggroup_of_hp, (void **)&p->d_grows, (void **)&p->d_gcount,
                     (void **)&p->d_gside, (void **)&p->d_gkeys, (void **)&p->d_gw,
                     (void **)&p->d_gcw, (void **)&p->d_gcmu, (void **)&p->d_gcsig,
                     (void **)&p->d_goptlog, (void **)&p->d_gpick, (void **)&p->d_gtab};
    for (void **b : bufs) { dfree(*b); *b = nullptr; }
    return rc;
  }
  p->group_ready = true;
  return TPE_OK;
}

// per-call scratch of m group scores
int ensure_group_points(tpe_engine *h, tpe_plan *p, size_t m) {
  if (m > p->gpt_cap) {
    dfree(p->d_gsides); dfree(p->d_gjoint); dfree(p->d_gcomp);
    p->d_gsides = p->d_gjoint = nullptr;
    p->d_gcomp = nullptr;
    p->gpt_cap = 0;
    const size_t G = p->glay.groups.size();
    CKH(dalloc(&p->d_gsides, 2 * G * m));
    CKH(dalloc(&p->d_gjoint, G * m));
    CKH(dalloc(&p->d_gcomp, G * m));
    p->gpt_cap = m;
  }
  return TPE_OK;
}

// the launch arguments of a group score or draw of m configurations, without
// the caller's arrays (ensure_points' lists serve the groups: G <= P)
GroupArgs group_args(tpe_plan *p, int64_t m) {
  GroupArgs a{};
  a.hps = p->d_hps;
  a.dims = p->d_gdims;
  a.groups = p->d_ggroups;
  a.dim_of_hp = p->d_gdim_of_hp;
  a.group_of_hp = p->d_ggroup_of_hp;
  a.level_hps = p->d_level_hps;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.n_hp = p->P;
  a.n_group = (int32_t)p->glay.groups.size();
  a.max_slots = p->glay.max_slots;
  a.kb_max = p->gkb_max;
  a.kcap = p->kcap;
  a.K = p->d_gcount;
  a.side = p->d_gside;
  a.jw = p->d_gw;
  a.cmu = p->d_gcmu;
  a.csig = p->d_gcsig;
  a.tab = p->d_gtab;
  a.optlog = p->d_goptlog;
  a.n_opt = p->glay.n_opt;
  a.pprior = p->d_pprior;
  a.prior_weight = p->fit_pw;
  a.m = m;
  a.idx = p->d_pt_idx;
  a.count = p->d_pt_count;
  a.sides = p->d_gsides;
  p->gpt_m = m;
  p->bt_m = m;
  return a;
}

// the host-mode copies back of a group score or draw
int group_copy_back(tpe_engine *h, tpe_plan *p, int64_t m, int64_t ld, double *total,
                    double *joint, uint8_t *active, hipStream_t st) {
  const size_t G = p->glay.groups.size();
  CKH(hipMemcpyAsync(total, p->d_pt_total, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (joint)
    CKH(hipMemcpy2DAsync(joint, (size_t)ld * 8, p->d_gjoint, (size_t)m * 8, (size_t)m * 8, G,
                         hipMemcpyDeviceToHost, st));
  if (active)
    CKH(hipMemcpy2DAsync(active, (size_t)ld, p->d_pt_act, (size_t)m, (size_t)m, (size_t)p->P,
                         hipMemcpyDeviceToHost, st));
  return TPE_OK;
}

}  // namespace

int tpe_plan_group_info(tpe_plan_t p, int32_t *group_of_hp, int32_t *n_groups) {
  if (!p) return TPE_E_INVALID;
  ensure_group_shape(p);
  if (group_of_hp)
    std::copy(p->gpart.group_of_hp.begin(), p->gpart.group_of_hp.end(), group_of_hp);
  if (n_groups) *n_groups = (int32_t)p->gpart.members.size();
  return TPE_OK;
}

int tpe_plan_group_fit(tpe_plan_t p, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (p->last_nb < 0)
    return fail(h, TPE_E_INVALID, "group_fit: the plan has not been fitted (tpe_plan_fit first)");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  {
    int rc = ensure_group(h, p);
    if (rc) return rc;
    rc = flush_patch(h, p, st);
    if (rc) return rc;
  }
  // the split of the last fit, as a mask (k_split computes k_fit's threshold)
  FitArgs f{};
  f.losses = p->d_losses;
  f.n = p->n;
  f.n_below = p->last_nb;
  f.sortbuf = p->d_sortbuf;
  f.scap = p->scap;
  f.kcap = p->kcap;
  CKH(launch_split(f, p->d_below, st));
  GroupFitArgs a{};
  a.hps = p->d_hps;
  a.dims = p->d_gdims;
  a.groups = p->d_ggroups;
  a.dim_of_hp = p->d_gdim_of_hp;
  a.group_of_hp = p->d_ggroup_of_hp;
  a.n_group = (int32_t)p->glay.groups.size();
  a.n_hp = p->P;
  a.vals = p->d_vals;
  a.active = p->d_active;
  a.ld = p->ncap;
  a.n = p->n;
  a.below = p->d_below;
  a.lf = p->fit_lf;
  a.prior_weight = p->fit_pw;
  a.pprior = p->d_pprior;
  a.info = p->d_info;
  a.mw = p->d_mw;
  a.mmu = p->d_mmu;
  a.msig = p->d_msig;
  a.kcap = p->kcap;
  a.keys = p->d_gkeys;
  a.rows = p->d_grows;
  a.count = p->d_gcount;
  a.side = p->d_gside;
  a.jw = p->d_gw;
  a.cw = p->d_gcw;
  a.cmu = p->d_gcmu;
  a.csig = p->d_gcsig;
  a.tab = p->d_gtab;
  a.optlog = p->d_goptlog;
  a.n_opt = p->glay.n_opt;
  CKH(launch_group_fit(a, st));
  // (group 0 holds every row of a side; a group's below rows are among them)
  p->gkb_max = (int32_t)std::min<int64_t>(std::max<int64_t>(p->last_nb, 0), p->n) + 1;
  p->group_ok = true;
  p->bt_m = -1;  // (the sides of an earlier fit's score are not this model's)
  return TPE_OK;
}

int tpe_plan_group_get_mixture(tpe_plan_t p, int32_t group, int32_t hp, int32_t side, double *w,
                               double *mu, double *sigma, int32_t *rows, int64_t cap,
                               int64_t *k) {
  if (!p || !k) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (!p->group_ok)
    return fail(h, TPE_E_INVALID, "group_get_mixture: no group fit (tpe_plan_group_fit first)");
  const int32_t G = (int32_t)p->glay.groups.size();
  if (group < 0 || group >= G || hp < -1 || hp >= p->P || side < 0 || side > 1)
    return fail(h, TPE_E_INVALID, "bad group/hp/side");
  if (hp >= 0 && p->gpart.group_of_hp[(size_t)hp] != group)
    return fail(h, TPE_E_INVALID, "group_get_mixture: the hp is not in that group");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const int64_t gs = (int64_t)group * 2 + side;
  int32_t K32 = 0;
  CKH(hipMemcpy(&K32, p->d_gcount + gs, 4, hipMemcpyDeviceToHost));
  const int64_t K = K32;
  *k = K;
  if (K > cap) return fail(h, TPE_E_INVALID, "capacity too small");
  const size_t bytes = (size_t)K * 8;
  if (rows)
    CKH(hipMemcpy(rows, p->d_grows + gs * p->kcap, (size_t)K * 4, hipMemcpyDeviceToHost));
  if (hp < 0) {  // the component weights themselves
    if (w) CKH(hipMemcpy(w, p->d_gw + gs * p->kcap, bytes, hipMemcpyDeviceToHost));
    return TPE_OK;
  }
  const int64_t ds = ((int64_t)hp * 2 + side) * p->kcap;
  if (w) CKH(hipMemcpy(w, p->d_gcw + ds, bytes, hipMemcpyDeviceToHost));
  if (mu) CKH(hipMemcpy(mu, p->d_gcmu + ds, bytes, hipMemcpyDeviceToHost));
  if (sigma) CKH(hipMemcpy(sigma, p->d_gcsig + ds, bytes, hipMemcpyDeviceToHost));
  return TPE_OK;
}

// Whole configurations under the group models: tpe_plan_score_points' staging
// and conventions; one walk, one scoring launch over all groups, one sum.
int tpe_plan_group_score_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld,
                                double *total, double *joint, uint8_t *active,
                                int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (m < 0 || ld < m) return fail(h, TPE_E_INVALID, "group_score_points: need 0 <= m <= ld");
  if (m > 0 && (!vals || !total))
    return fail(h, TPE_E_INVALID, "group_score_points: vals and total must not be null");
  if (m > (int64_t)INT32_MAX)
    return fail(h, TPE_E_INVALID, "group_score_points: too many configurations");
  if (m == 0) return TPE_OK;
  if (!p->group_ok)
    return fail(h, TPE_E_INVALID, "group_score_points: no group fit (tpe_plan_group_fit first)");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  {
    int rc = ensure_points(h, p, (size_t)m);
    if (rc) return rc;
    rc = ensure_group_points(h, p, (size_t)m);
    if (rc) return rc;
  }
  CKH(hipMemsetAsync(p->d_pt_count, 0, (size_t)p->P * sizeof(uint32_t), st));
  GroupArgs a = group_args(p, m);
  if (dev) {
    a.vals = vals;
    a.ld = ld;
    a.total = total;
    a.active = active ? active : p->d_pt_act;
    a.act_ld = active ? ld : m;
    a.joint = joint ? joint : p->d_gjoint;
    a.joint_ld = joint ? ld : m;
    CKH(launch_group_points(a, true, st));
    return TPE_OK;
  }
  if (ld == m)  // (contiguous: one plain copy)
    CKH(hipMemcpyAsync(p->d_pt_vals, vals, (size_t)m * p->P * 8, hipMemcpyHostToDevice, st));
  else
    CKH(hipMemcpy2DAsync(p->d_pt_vals, (size_t)m * 8, vals, (size_t)ld * 8, (size_t)m * 8,
                         (size_t)p->P, hipMemcpyHostToDevice, st));
  a.vals = p->d_pt_vals;
  a.ld = m;
  a.total = p->d_pt_total;
  a.active = p->d_pt_act;
  a.act_ld = m;
  a.joint = p->d_gjoint;
  a.joint_ld = m;
  CKH(launch_group_points(a, true, st));
  {
    const int rc = group_copy_back(h, p, m, ld, total, joint, active, st);
    if (rc) return rc;
  }
  CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

int tpe_plan_group_sides(tpe_plan_t p, int32_t group, double *below, double *above, int64_t m) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (group < 0 || group >= (int32_t)p->glay.groups.size())
    return fail(h, TPE_E_INVALID, "group_sides: no such group");
  if (!p->group_ok)
    return fail(h, TPE_E_INVALID, "group_sides: no group fit (a later tpe_plan_fit drops the sides)");
  if (m < 0 || m > p->gpt_m)
    return fail(h, TPE_E_INVALID, "group_sides: more entries than the last group score holds");
  if (m == 0) return TPE_OK;
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const double *s = p->d_gsides + (int64_t)group * 2 * p->gpt_m;
  if (below) CKH(hipMemcpy(below, s, (size_t)m * 8, hipMemcpyDeviceToHost));
  if (above) CKH(hipMemcpy(above, s + p->gpt_m, (size_t)m * 8, hipMemcpyDeviceToHost));
  return TPE_OK;
}

// Whole configurations drawn from the groups' below models and scored: the
// walk picks one component per active group and draws the group's hps from
// it; then tpe_plan_group_score_points' launches behind the draw's own lists.
int tpe_plan_group_sample_points(tpe_plan_t p, uint64_t seed, int64_t begin, int64_t m, int64_t ld,
                                 double *vals, int32_t *comp, double *total, double *joint,
                                 uint8_t *active, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (m < 0 || ld < m) return fail(h, TPE_E_INVALID, "group_sample_points: need 0 <= m <= ld");
  if (begin < 0) return fail(h, TPE_E_INVALID, "group_sample_points: begin must not be negative");
  if (m > 0 && (!vals || !total))
    return fail(h, TPE_E_INVALID, "group_sample_points: vals and total must not be null");
  if (m > (int64_t)INT32_MAX)
    return fail(h, TPE_E_INVALID, "group_sample_points: too many configurations");
  if (m == 0) return TPE_OK;
  if (!p->group_ok)
    return fail(h, TPE_E_INVALID, "group_sample_points: no group fit (tpe_plan_group_fit first)");
  if (p->gkb_max > kTabCap)
    return fail(h, TPE_E_INVALID, "group_sample_points: more below components than a draw table holds");
  for (const JointDim &d : p->glay.dims)
    if (d.upper > kTabCap)
      return fail(h, TPE_E_INVALID, "group_sample_points: a choice has more options than a draw table holds");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  {
    int rc = ensure_points(h, p, (size_t)m);
    if (rc) return rc;
    rc = ensure_group_points(h, p, (size_t)m);
    if (rc) return rc;
  }
  if (!p->d_gdraw) CKH(hipMalloc(&p->d_gdraw, joint_sample_tables_bytes(p->P)));
  const size_t need = (size_t)p->glay.n_opt * (size_t)p->gkb_max;
  if (need > p->goptcdf_cap) {
    dfree(p->d_goptcdf);
    p->d_goptcdf = nullptr;
    p->goptcdf_cap = 0;
    CKH(dalloc(&p->d_goptcdf, need));
    p->goptcdf_cap = need;
  }
  CKH(hipMemsetAsync(p->d_pt_count, 0, (size_t)p->P * sizeof(uint32_t), st));
  GroupArgs a = group_args(p, m);
  a.seed = seed;
  a.begin = begin;
  a.dtab = static_cast<DrawTableT<kTabCap> *>(p->d_gdraw);
  a.pick_cdf = p->d_gpick;
  a.opt_cdf = p->d_goptcdf;
  if (dev) {
    a.out = vals;
    a.vals = vals;
    a.ld = ld;
    a.total = total;
    a.active = active ? active : p->d_pt_act;
    a.act_ld = active ? ld : m;
    a.joint = joint ? joint : p->d_gjoint;
    a.joint_ld = joint ? ld : m;
    a.comp = comp ? comp : p->d_gcomp;
    a.comp_ld = comp ? ld : m;
    CKH(launch_group_sample(a, st));
    CKH(launch_group_points(a, false, st));
    return TPE_OK;
  }
  a.out = p->d_pt_vals;
  a.vals = p->d_pt_vals;
  a.ld = m;
  a.total = p->d_pt_total;
  a.active = p->d_pt_act;
  a.act_ld = m;
  a.joint = p->d_gjoint;
  a.joint_ld = m;
  a.comp = p->d_gcomp;
  a.comp_ld = m;
  CKH(launch_group_sample(a, st));
  CKH(launch_group_points(a, false, st));
  CKH(hipMemcpy2DAsync(vals, (size_t)ld * 8, p->d_pt_vals, (size_t)m * 8, (size_t)m * 8,
                       (size_t)p->P, hipMemcpyDeviceToHost, st));
  if (comp)
    CKH(hipMemcpy2DAsync(comp, (size_t)ld * 4, p->d_gcomp, (size_t)m * 4, (size_t)m * 4,
                         p->glay.groups.size(), hipMemcpyDeviceToHost, st));
  {
    const int rc = group_copy_back(h, p, m, ld, total, joint, active, st);
    if (rc) return rc;
  }
  CKH(hipStreamSynchronize(st));
  return TPE_OK;
}

namespace {

// the state of a greedy batch over m configurations
int ensure_batch(tpe_engine *h, tpe_plan *p, size_t m) {
  if (!p->d_bt_rec) {
    const size_t G = p->glay.groups.size();
    // [hdr | ng[G] | rec[P][kBatchRec] | pact[G]]: cleared as one range
    const size_t bytes = sizeof(BatchHdr) + G * 4 + ((G * 4) % 8 ? 4 : 0) +
                         (size_t)p->P * kBatchRec * 8 + G;
    CKH(hipMalloc(&p->d_bt_rec, bytes));
    CKH(dalloc(&p->d_bt_idx, (size_t)kBatchMax));
    CKH(dalloc(&p->d_bt_gain, (size_t)kBatchMax));
  }
  if (m > p->bt_cap) {
    dfree(p->d_bt_ja); dfree(p->d_bt_score); dfree(p->d_bt_gact); dfree(p->d_bt_state);
    dfree(p->d_bt_slot);
    p->d_bt_ja = p->d_bt_score = nullptr;
    p->d_bt_gact = p->d_bt_state = nullptr;
    p->d_bt_slot = nullptr;
    p->bt_cap = 0;
    const size_t G = p->glay.groups.size();
    CKH(dalloc(&p->d_bt_ja, G * m));
    CKH(dalloc(&p->d_bt_score, m));
    CKH(dalloc(&p->d_bt_gact, G * m));
    CKH(dalloc(&p->d_bt_state, m));
    CKH(hipMalloc(&p->d_bt_slot, ((m + kBtThreads - 1) / kBtThreads) * sizeof(BatchSlot)));
    p->bt_cap = m;
  }
  return TPE_OK;
}

}  // namespace

// A batch for parallel workers: k greedy picks over the configurations of the
// last group score or draw, each joining the above side of its active groups
// as a pending component (tpe_batch.hip).
int tpe_plan_group_batch_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld,
                                const uint8_t *eligible, int32_t k, int32_t *idx, double *gain,
                                double *trace, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (k < 1 || k > kBatchMax)
    return fail(h, TPE_E_INVALID, "group_batch_points: need 1 <= k <= 1024");
  if (m < 0 || m > (int64_t)INT32_MAX || ld < m)
    return fail(h, TPE_E_INVALID, "group_batch_points: need 0 <= m <= ld, m <= 2^31 - 1");
  if (!idx || !vals)
    return fail(h, TPE_E_INVALID, "group_batch_points: vals and idx must not be null");
  if (!p->group_ok)
    return fail(h, TPE_E_INVALID, "group_batch_points: no group fit (tpe_plan_group_fit first)");
  if (m != p->bt_m)
    return fail(h, TPE_E_INVALID,
                "group_batch_points: m is not that of the last group score or draw of this fit");
  if (m < k) return fail(h, TPE_E_INVALID, "group_batch_points: fewer than k selectable configurations");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  {
    const int rc = ensure_batch(h, p, (size_t)m);
    if (rc) return rc;
  }
  const size_t G = p->glay.groups.size();
  if (!dev && trace && (size_t)k * (size_t)m > p->bt_trace_cap) {
    dfree(p->d_bt_trace);
    p->d_bt_trace = nullptr;
    p->bt_trace_cap = 0;
    CKH(dalloc(&p->d_bt_trace, (size_t)k * (size_t)m));
    p->bt_trace_cap = (size_t)k * (size_t)m;
  }
  BatchArgs a{};
  a.hps = p->d_hps;
  a.dims = p->d_gdims;
  a.groups = p->d_ggroups;
  a.group_of_hp = p->d_ggroup_of_hp;
  a.level_hps = p->d_level_hps;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.n_hp = p->P;
  a.n_group = (int32_t)G;
  a.kcap = p->kcap;
  a.side = p->d_gside;
  a.optlog = p->d_goptlog;
  a.n_opt = p->glay.n_opt;
  a.info = p->d_info;
  a.mmu = p->d_mmu;
  a.m = m;
  a.sides = p->d_gsides;
  a.ja = p->d_bt_ja;
  a.gact = p->d_bt_gact;
  a.state = p->d_bt_state;
  a.slot = static_cast<BatchSlot *>(p->d_bt_slot);
  unsigned char *rec = static_cast<unsigned char *>(p->d_bt_rec);
  const size_t ng_bytes = G * 4 + ((G * 4) % 8 ? 4 : 0);
  const size_t rec_bytes = sizeof(BatchHdr) + ng_bytes + (size_t)p->P * kBatchRec * 8 + G;
  a.hdr = reinterpret_cast<BatchHdr *>(rec);
  a.ng = reinterpret_cast<int32_t *>(rec + sizeof(BatchHdr));
  a.rec = reinterpret_cast<double *>(rec + sizeof(BatchHdr) + ng_bytes);
  a.pact = rec + sizeof(BatchHdr) + ng_bytes + (size_t)p->P * kBatchRec * 8;
  a.k = k;
  CKH(hipMemsetAsync(rec, 0, rec_bytes, st));
  if (dev) {
    a.vals = vals;
    a.ld = ld;
    a.eligible = eligible;
    a.score = trace ? trace : p->d_bt_score;
    a.score_ld = trace ? ld : 0;
    a.idx = idx;
    a.gain = gain ? gain : p->d_bt_gain;
  } else {
    // (the scratch holds the last group score's m configurations: pt_cap >= m)
    if (ld == m)
      CKH(hipMemcpyAsync(p->d_pt_vals, vals, (size_t)m * p->P * 8, hipMemcpyHostToDevice, st));
    else
      CKH(hipMemcpy2DAsync(p->d_pt_vals, (size_t)m * 8, vals, (size_t)ld * 8, (size_t)m * 8,
                           (size_t)p->P, hipMemcpyHostToDevice, st));
    if (eligible)  // (k_batch_init turns the bytes into the state in place)
      CKH(hipMemcpyAsync(p->d_bt_state, eligible, (size_t)m, hipMemcpyHostToDevice, st));
    a.vals = p->d_pt_vals;
    a.ld = m;
    a.eligible = eligible ? p->d_bt_state : nullptr;
    a.score = trace ? p->d_bt_trace : p->d_bt_score;
    a.score_ld = trace ? m : 0;
    a.idx = p->d_bt_idx;
    a.gain = p->d_bt_gain;
  }
  CKH(launch_group_batch(a, st));
  // a short batch: one 4-byte read-back (in device mode too, as the masked top-k's count)
  BatchHdr hdr{};
  CKH(hipMemcpyAsync(&hdr.is_short, &a.hdr->is_short, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (!dev) {
    CKH(hipMemcpyAsync(idx, p->d_bt_idx, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (gain) CKH(hipMemcpyAsync(gain, p->d_bt_gain, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    if (trace)
      CKH(hipMemcpy2DAsync(trace, (size_t)ld * 8, p->d_bt_trace, (size_t)m * 8, (size_t)m * 8,
                           (size_t)k, hipMemcpyDeviceToHost, st));
  }
  CKH(hipStreamSynchronize(st));
  if (hdr.is_short)
    return fail(h, TPE_E_INVALID, "group_batch_points: fewer than k selectable configurations");
  return TPE_OK;
}

// The k best eligible totals (tpe_topk.hip).  With a mask the call waits for
// the first pass to learn how many entries are eligible.
int tpe_plan_topk_points(tpe_plan_t p, const double *total, const uint8_t *eligible, int64_t m,
                         int32_t k, int32_t *idx, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (k < 1 || k > kTopkMax) return fail(h, TPE_E_INVALID, "topk_points: need 1 <= k <= 4096");
  if (m < 0 || m > (int64_t)INT32_MAX)
    return fail(h, TPE_E_INVALID, "topk_points: need 0 <= m <= 2^31 - 1");
  if (!idx || (m > 0 && !total))
    return fail(h, TPE_E_INVALID, "topk_points: total and idx must not be null");
  if (m < k) return fail(h, TPE_E_INVALID, "topk_points: fewer than k eligible entries");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  const bool dev = on_device != 0;
  int rc = ensure_topk(h, p);
  if (rc) return rc;
  const double *d_total = total;
  const uint8_t *d_elig = eligible;
  if (!dev) {
    rc = ensure_points(h, p, (size_t)m);
    if (rc) return rc;
    CKH(hipMemcpyAsync(p->d_pt_total, total, (size_t)m * 8, hipMemcpyHostToDevice, st));
    if (eligible)
      CKH(hipMemcpyAsync(p->d_pt_act, eligible, (size_t)m, hipMemcpyHostToDevice, st));
    d_total = p->d_pt_total;
    d_elig = eligible ? p->d_pt_act : nullptr;
  }
  CKH(launch_topk_first(d_total, d_elig, m, k, p->d_tk, st));
  if (d_elig) {
    // (the first pass's histogram is the first member of the scratch)
    uint32_t hist[256];
    CKH(hipMemcpyAsync(hist, p->d_tk, sizeof(hist), hipMemcpyDeviceToHost, st));
    CKH(hipStreamSynchronize(st));
    int64_t n = 0;
    for (uint32_t c : hist) n += c;
    if (n < k) return fail(h, TPE_E_INVALID, "topk_points: fewer than k eligible entries");
  }
  CKH(launch_topk_rest(d_total, d_elig, m, k, p->d_tk, dev ? idx : p->d_tk_idx, st));
  if (!dev) {
    CKH(hipMemcpyAsync(idx, p->d_tk_idx, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CKH(hipStreamSynchronize(st));
  }
  return TPE_OK;
}

// out[n_hp][k] = the columns idx[0..k) of vals[n_hp][ld]
int tpe_plan_gather_points(tpe_plan_t p, const double *vals, int64_t ld, const int32_t *idx,
                           int32_t k, double *out, int32_t on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (k < 0 || ld < 0) return fail(h, TPE_E_INVALID, "gather_points: need k >= 0 and ld >= 0");
  if (k == 0) return TPE_OK;
  if (!vals || !idx || !out)
    return fail(h, TPE_E_INVALID, "gather_points: vals, idx and out must not be null");
  if (on_device) {
    CKH(hipSetDevice(h->device));
    CKH(launch_gather_points(vals, ld, p->P, idx, k, out, pick_stream(h, stream)));
    return TPE_OK;
  }
  for (int32_t j = 0; j < k; ++j)
    if (idx[j] < 0 || idx[j] >= ld) return fail(h, TPE_E_INDEX, "gather_points: index out of range");
  for (int32_t i = 0; i < p->P; ++i)
    for (int32_t j = 0; j < k; ++j) out[(int64_t)i * k + j] = vals[(int64_t)i * ld + idx[j]];
  return TPE_OK;
}

int tpe_plan_profile(tpe_plan_t p, int32_t capacity) {
  if (!p || capacity < 0) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  for (auto &pr : p->prof) {
    for (auto e : pr.a) (void)hipEventDestroy(e);
    for (auto e : pr.b) (void)hipEventDestroy(e);
    pr.a.assign(capacity, nullptr);
    pr.b.assign(capacity, nullptr);
    pr.pairs.assign(capacity, 0.0);
    pr.n = 0;
    for (int i = 0; i < capacity; ++i) {
      CKH(hipEventCreate(&pr.a[i]));
      CKH(hipEventCreate(&pr.b[i]));
    }
  }
  p->prof_cap = capacity;
  return TPE_OK;
}

int tpe_plan_profile_read(tpe_plan_t p, int32_t kind, double *avg_ms, int64_t *launches,
                          double *pairs_per_launch) {
  if (!p || kind < 0 || kind > KIND_LAT) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  if (kind == KIND_LAT) {  // k_lattice launches: lattice points x (K_b + K_a)
    auto &pl = p->prof[1];
    std::vector<MixInfo> info(2 * (size_t)p->P);
    CKH(hipMemcpy(info.data(), p->d_info, info.size() * sizeof(MixInfo), hipMemcpyDeviceToHost));
    double tot = 0.0, pairs = 0.0;
    for (int64_t i = 0; i < pl.n; ++i) {
      float ms = 0.f;
      CKH(hipEventElapsedTime(&ms, pl.a[i], pl.b[i]));
      tot += ms;
      for (int hp : p->levels[(int)pl.pairs[i]]) {
        const int k = score_kind(p->hps[hp]);
        if (k == KIND_ERF_G || k == KIND_ERF_L)
          pairs += (double)p->lat[hp].R * ((double)info[2 * hp].K + info[2 * hp + 1].K);
      }
    }
    if (avg_ms) *avg_ms = pl.n ? tot / pl.n : 0.0;
    if (launches) *launches = pl.n;
    if (pairs_per_launch) *pairs_per_launch = pl.n ? pairs / pl.n : 0.0;
    return TPE_OK;
  }
  auto &pr = p->prof[0];  // every scoring launch (all lpdf kinds of a level)
  double tot = 0.0, pairs = 0.0;
  // this kind's pairs in those launches: components per candidate of the
  // kind's hps (all levels), active in the last suggestion (levels' activity
  // is the same for every profiled step)
  std::vector<MixInfo> info(2 * (size_t)p->P);
  std::vector<Partial> res((size_t)std::max<int64_t>(1, p->last_nsug) * p->P);
  CKH(hipMemcpy(info.data(), p->d_info, info.size() * sizeof(MixInfo), hipMemcpyDeviceToHost));
  if (p->d_results)
    CKH(hipMemcpy(res.data(), p->d_results, res.size() * sizeof(Partial), hipMemcpyDeviceToHost));
  double kk = 0.0;  // sum over suggestions of active (K_b + K_a), per suggestion avg
  for (int hp = 0; hp < p->P; ++hp) {
    if (score_kind(p->hps[hp]) != kind || kind == KIND_CAT) continue;
    double act = 0;
    for (int64_t s = 0; s < std::max<int64_t>(1, p->last_nsug); ++s) act += res[s * p->P + hp].active;
    act /= (double)std::max<int64_t>(1, p->last_nsug);
    kk += act * ((double)info[2 * hp].K + info[2 * hp + 1].K);
  }
  for (int64_t i = 0; i < pr.n; ++i) {
    float ms = 0.f;
    CKH(hipEventElapsedTime(&ms, pr.a[i], pr.b[i]));
    tot += ms;
    pairs += pr.pairs[i] * kk;
  }
  if (avg_ms) *avg_ms = pr.n ? tot / pr.n : 0.0;
  if (launches) *launches = pr.n;
  if (pairs_per_launch) *pairs_per_launch = pr.n ? pairs / pr.n : 0.0;
  return TPE_OK;  // the ring is re-armed by tpe_plan_profile
}

int tpe_plan_set_lattice(tpe_plan_t p, int32_t enable) {
  if (!p) return TPE_E_INVALID;
  if (p->lattice_on != (enable != 0)) graph_reset(p);
  p->lattice_on = enable != 0;
  return TPE_OK;
}

int tpe_plan_census(tpe_plan_t p, int32_t enable, int64_t *counts) {
  return tpe_plan_census_n(p, enable, counts, 6);
}

int tpe_plan_census_n(tpe_plan_t p, int32_t enable, int64_t *counts, int32_t n_counts) {
  if (!p || n_counts < 0) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  if (counts) {
    unsigned long long c[kCensus];
    CKH(hipMemcpy(c, p->d_census, sizeof(c), hipMemcpyDeviceToHost));
    for (int i = 0; i < kCensus && i < n_counts; ++i) counts[i] = (int64_t)c[i];
  }
  CKH(hipMemset(p->d_census, 0, kCensus * sizeof(unsigned long long)));
  p->census = enable != 0;
  return TPE_OK;
}

int tpe_plan_tie_counts(tpe_plan_t p, int32_t n_suggest, int32_t *counts) {
  if (!p || !counts || n_suggest < 0) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n_suggest > p->s_cap) return fail(h, TPE_E_INVALID, "more suggestions than the last call's");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  if (n_suggest > 0)
    CKH(hipMemcpy(counts, p->d_tie_cnt, (size_t)n_suggest * p->P * sizeof(int32_t),
                  hipMemcpyDeviceToHost));
  return TPE_OK;
}

int tpe_plan_tab_wmax(tpe_plan_t p, int32_t n_suggest, double *out) {
  if (!p || n_suggest < 0) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  const size_t row = (size_t)p->tab_pstride * 8;
  if (!out) return (int)row;
  if (n_suggest > p->s_cap || (size_t)n_suggest * p->P * p->tab_pstride > p->partial_cap)
    return fail(h, TPE_E_INVALID, "more suggestions than the last call's");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  if (n_suggest > 0 && row > 0)
    CKH(hipMemcpy(out, p->d_tab_wmax, (size_t)n_suggest * p->P * row * sizeof(double),
                  hipMemcpyDeviceToHost));
  return TPE_OK;
}

int64_t tpe_plan_cand_dump(tpe_plan_t p, int32_t s, int32_t hp, double *values, int32_t *positions) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (p->dump_level < 0 || p->dump_cn <= 0) return fail(h, TPE_E_INVALID, "no sorted draw yet");
  if (!values && !positions) return p->dump_cn;
  const std::vector<int32_t> &lv = p->levels[p->dump_level];
  int64_t slot = -1;
  for (size_t i = 0; i < lv.size(); ++i)
    if (lv[i] == hp) slot = (int64_t)i;
  if (slot < 0 || s < 0 || s >= p->dump_nsug)
    return fail(h, TPE_E_INVALID, "hp / suggestion not of the last sorted draw");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const int64_t off = (int64_t)s * p->dump_sstride + slot * p->dump_cn;
  if (values)
    CKH(hipMemcpy(values, p->d_cand + off, (size_t)p->dump_cn * sizeof(double), hipMemcpyDeviceToHost));
  if (positions)
    CKH(hipMemcpy(positions, p->d_cpos + off, (size_t)p->dump_cn * sizeof(int32_t),
                  hipMemcpyDeviceToHost));
  return p->dump_cn;
}

int tpe_plan_tab_bound(tpe_plan_t p, int32_t hp, double *out) {
  if (!p) return TPE_E_INVALID;
  if (!out) return kBndCells;
  tpe_engine *h = p->eng;
  if (hp < 0 || hp >= p->P) return fail(h, TPE_E_INVALID, "bad args");
  if (!table_hp(p->hps[hp])) return fail(h, TPE_E_INVALID, "hp has no Chebyshev table");
  if (!switches().table_prefilter) return fail(h, TPE_E_INVALID, "no bound lattice: the prefilter is off");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const int rc = table_build(h, p, h->stream);  // (this fit epoch's, if no launch has built them)
  if (rc) return rc;
  TabHdr th[2];
  CKH(hipMemcpyAsync(th, p->d_tab_hdr + 2 * (int64_t)hp, sizeof(th), hipMemcpyDeviceToHost,
                     h->stream));
  CKH(hipStreamSynchronize(h->stream));
  for (const TabHdr &t : th)
    if (!(t.P > 0 && t.ncert == (uint32_t)t.P))
      return fail(h, TPE_E_INVALID, "Chebyshev table not certified");
  CKH(hipMemcpy(out, p->d_tab_bound + (int64_t)hp * kBndCells, kBndCells * sizeof(double),
                hipMemcpyDeviceToHost));
  return TPE_OK;
}

// the tables of the current fit, built if no launch has yet, and the header
// of (hp, side)
static int tab_header(tpe_plan *p, int32_t hp, int32_t side, TabHdr *th) {
  tpe_engine *h = p->eng;
  if (hp < 0 || hp >= p->P || side < 0 || side > 1) return fail(h, TPE_E_INVALID, "bad args");
  if (!table_hp(p->hps[hp])) return fail(h, TPE_E_INVALID, "hp has no Chebyshev table");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  const int rc = table_build(h, p, h->stream);
  if (rc) return rc;
  CKH(hipMemcpyAsync(th, p->d_tab_hdr + 2 * (int64_t)hp + side, sizeof(*th), hipMemcpyDeviceToHost,
                     h->stream));
  CKH(hipStreamSynchronize(h->stream));
  if (th->P < 0 || th->P > kTabMaxPanels) return fail(h, TPE_E_HIP, "table header out of range");
  return TPE_OK;
}

int tpe_plan_tab_panels(tpe_plan_t p, int32_t hp, int32_t side, double *y_lo, double *inv_w,
                        int32_t *ncert, void *panels) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  TabHdr th;
  const int rc = tab_header(p, hp, side, &th);
  if (rc) return rc;
  if (y_lo) *y_lo = th.y_lo;
  if (inv_w) *inv_w = th.inv_w;
  if (ncert) *ncert = (int32_t)th.ncert;
  if (panels && th.P > 0)
    CKH(hipMemcpy(panels, p->d_tab + (2 * (int64_t)hp + side) * kTabMaxPanels,
                  (size_t)th.P * sizeof(TabPanel), hipMemcpyDeviceToHost));
  return th.P;
}

int tpe_plan_tab_cert(tpe_plan_t p, int32_t hp, int32_t side, double *out) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (!p->d_tab_cert) {
    // the first read: the buffer, and a build that fills it (a captured step
    // holds the build without it)
    CKH(hipSetDevice(h->device));
    CKH(hipDeviceSynchronize());
    graph_reset(p);
    const size_t n = (size_t)2 * p->P * kTabMaxPanels * 3;
    CKH(dalloc(&p->d_tab_cert, n));
    CKH(hipMemset(p->d_tab_cert, 0xff, n * sizeof(double)));
    p->tab_built = false;
  }
  TabHdr th;
  const int rc = tab_header(p, hp, side, &th);
  if (rc) return rc;
  if (out && th.P > 0)
    CKH(hipMemcpy(out, p->d_tab_cert + (2 * (int64_t)hp + side) * kTabMaxPanels * 3,
                  (size_t)th.P * 3 * sizeof(double), hipMemcpyDeviceToHost));
  return th.P;
}

int tpe_plan_tie_list(tpe_plan_t p, int32_t s, int32_t hp, int32_t *out) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (hp < 0 || hp >= p->P || s < 0 || s >= p->s_cap || p->tab_pstride <= 0 ||
      ((size_t)s * p->P + hp + 1) * p->tab_pstride > p->partial_cap)
    return fail(h, TPE_E_INVALID, "hp / suggestion not of the last launch that took the tables");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  int32_t n = 0;
  CKH(hipMemcpy(&n, p->d_tie_cnt + (int64_t)s * p->P + hp, sizeof(n), hipMemcpyDeviceToHost));
  const int64_t row = (int64_t)p->tab_pstride * 8;
  if (n < 0) return 0;
  if (n > row) return fail(h, TPE_E_HIP, "tie count out of range");
  if (out && n > 0)
    CKH(hipMemcpy(out, p->d_tie_list + ((int64_t)s * p->P + hp) * row, (size_t)n * sizeof(int32_t),
                  hipMemcpyDeviceToHost));
  return n;
}

int tpe_plan_draw_screen_stats(tpe_plan_t p, int64_t *out) {
  if (!p || !out) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  out[0] = out[1] = out[2] = 0;
  if (!p->d_screen_stats) return TPE_OK;
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  unsigned long long v[2];
  CKH(hipMemcpy(v, p->d_screen_stats, sizeof(v), hipMemcpyDeviceToHost));
  CKH(hipMemset(p->d_screen_stats, 0, sizeof(v)));
  out[0] = (int64_t)(v[0] >> 40);
  out[1] = (int64_t)v[1];
  out[2] = (int64_t)(v[0] & ((1ull << 40) - 1));
  return TPE_OK;
}

int tpe_plan_tab_hot(tpe_plan_t p, int32_t n_suggest, double *out) {
  static_assert(sizeof(TabHot) == (2 + 2 * kHotIv) * sizeof(double), "y_lo, y_hi, lo[], hi[]");
  if (!p || !out || n_suggest < 0) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n_suggest > p->s_cap) return fail(h, TPE_E_INVALID, "more suggestions than the last call's");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  if (n_suggest > 0)
    CKH(hipMemcpy(out, p->d_tab_hot, (size_t)n_suggest * p->P * sizeof(TabHot),
                  hipMemcpyDeviceToHost));
  return TPE_OK;
}

int tpe_plan_sample_prior(tpe_plan_t p, const uint64_t *seeds, int64_t n_sug, tpe_result *out,
                          int32_t out_on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n_sug <= 0 || !seeds) return fail(h, TPE_E_INVALID, "bad args");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  int rc = ensure_suggest_state(h, p, n_sug, 1);
  if (rc) return rc;
  CKH(hipMemcpyAsync(p->d_seeds, seeds, n_sug * 8, hipMemcpyHostToDevice, st));
  PriorArgs a{};
  a.hps = p->d_hps;
  a.n_hp = p->P;
  a.n_levels = (int32_t)p->levels.size();
  a.level_hps = p->d_level_hps;
  a.level_off = p->d_level_off;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.pprior = p->d_pprior;
  a.seeds = p->d_seeds;
  a.results = p->d_results;
  CKH(launch_prior(a, (int32_t)n_sug, st));
  p->last_nsug = n_sug;
  if (!out_on_device) {
    // the host seeds buffer must outlive the async copy: synchronize here
    rc = copy_results(h, p, n_sug, out, 0, st);
    if (rc) return rc;
    return TPE_OK;
  }
  return copy_results(h, p, n_sug, out, out_on_device, st);
}

// ---------------------------------------------------------------- annealing
// The order in which a suggestion walks the hps is the host's: the reference
// interpreter's node-evaluation order (hyperopt/algobase.py:64-132 on the
// vectorized graph; space.CompiledSpace.draw_order, pinned by
// tests/golden/anneal.npz), compiled into the plan as an int array.
int tpe_plan_set_anneal_order(tpe_plan_t p, const int32_t *hp_order, int32_t n_hp) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (!hp_order || n_hp != p->P) return fail(h, TPE_E_INVALID, "anneal order: one entry per hp");
  std::vector<int32_t> pos(p->P, -1);
  for (int k = 0; k < n_hp; ++k) {
    const int hp = hp_order[k];
    if (hp < 0 || hp >= p->P || pos[hp] >= 0)
      return fail(h, TPE_E_INVALID, "anneal order: not a permutation of the hps");
    pos[hp] = k;
  }
  for (int hp = 0; hp < p->P; ++hp) {
    const tpe_hp &x = p->hps[hp];
    for (int c = 0; c < x.cond_count; ++c)
      if (pos[p->cond_parent[x.cond_begin + c]] > pos[hp])
        return fail(h, TPE_E_INVALID, "anneal order: an hp before the choice that leads to it");
  }
  CKH(hipSetDevice(h->device));
  p->an_order = false;
  if (!p->d_an_hporder) CKH(dalloc(&p->d_an_hporder, p->P));
  CKH(hipDeviceSynchronize());  // (no anneal call of any stream still reads the old order)
  CKH(hipMemcpy(p->d_an_hporder, hp_order, (size_t)n_hp * 4, hipMemcpyHostToDevice));
  p->an_order = true;
  return TPE_OK;
}

// sort scratch, counts and trace of an anneal call: all of it or none (a
// failed allocation leaves nothing half-built for the next call to launch on)
static int ensure_anneal_state(tpe_engine *h, tpe_plan *p, int64_t n_sug) {
  if (!p->an_ready) {
    auto drop = [p] {
      dfree(p->d_an_keys); dfree(p->d_an_idx); dfree(p->d_an_T);
      p->d_an_keys = nullptr; p->d_an_idx = nullptr; p->d_an_T = nullptr;
    };
    drop();
    const hipError_t e1 = dalloc(&p->d_an_keys, 2 * (size_t)p->ncap);
    const hipError_t e2 = e1 == hipSuccess ? dalloc(&p->d_an_idx, 2 * (size_t)p->ncap) : e1;
    const hipError_t e3 = e2 == hipSuccess ? dalloc(&p->d_an_T, p->P) : e2;
    if (e3 != hipSuccess) {
      drop();
      return fail(h, TPE_E_NOMEM, std::string("anneal scratch: ") + hipGetErrorString(e3));
    }
    p->an_ready = true;
  }
  if (n_sug > p->an_cap) {
    dfree(p->d_an_trace);
    p->d_an_trace = nullptr;
    p->an_cap = 0;
    CKH(dalloc(&p->d_an_trace, (size_t)n_sug * p->P));
    p->an_cap = n_sug;
  }
  return TPE_OK;
}

int tpe_plan_anneal(tpe_plan_t p, double avg_best_idx, double shrink_coef, const uint64_t *seeds,
                    int64_t n_sug, tpe_result *out, int32_t out_on_device, void *stream) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (!std::isfinite(avg_best_idx) || !std::isfinite(shrink_coef) || avg_best_idx < 1.0 ||
      shrink_coef < 0.0)
    return fail(h, TPE_E_INVALID, "anneal: avg_best_idx >= 1 and shrink_coef >= 0, finite");
  if (n_sug <= 0 || n_sug > INT32_MAX || !seeds) return fail(h, TPE_E_INVALID, "bad args");
  if (p->n > INT32_MAX) return fail(h, TPE_E_INVALID, "history too long");
  if (anneal_wave_lds(p->P) > 64 * 1024) return fail(h, TPE_E_INVALID, "anneal: too many hps");
  if (!p->an_order) return fail(h, TPE_E_INVALID, "anneal: tpe_plan_set_anneal_order first");
  CKH(hipSetDevice(h->device));
  hipStream_t st = pick_stream(h, stream);
  int rc = ensure_suggest_state(h, p, n_sug, 1);
  if (rc) return rc;
  rc = ensure_anneal_state(h, p, n_sug);
  if (rc) return rc;
  // the kernels read the history rows: a deferred update goes out first
  rc = flush_patch(h, p, st);
  if (rc) return rc;
  p->h_seeds.assign(seeds, seeds + n_sug);  // (outlives the async copy)
  CKH(hipMemcpyAsync(p->d_seeds, p->h_seeds.data(), n_sug * 8, hipMemcpyHostToDevice, st));
  const int32_t n = (int32_t)p->n;
  CKH(launch_anneal_order(p->d_losses, p->d_active, p->ncap, n, p->P, p->d_an_keys,
                          p->d_an_keys + p->ncap, p->d_an_idx, p->d_an_idx + p->ncap, p->d_an_T,
                          st));
  AnnealArgs a{};
  a.hps = p->d_hps;
  a.n_hp = p->P;
  a.n = n;
  a.hp_order = p->d_an_hporder;
  a.cond_parent = p->d_cp;
  a.cond_branch = p->d_cb;
  a.pprior = p->d_pprior;
  a.losses = p->d_losses;
  a.vals = p->d_vals;
  a.active = p->d_active;
  a.ld = p->ncap;
  a.order = p->d_an_idx;
  a.T = p->d_an_T;
  a.p_geo = 1.0 / avg_best_idx;
  a.log1p_mq = std::log1p(-a.p_geo);
  a.shrink_coef = shrink_coef;
  a.seeds = p->d_seeds;
  a.n_suggest = (int32_t)n_sug;
  a.results = p->d_results;
  a.trace = p->d_an_trace;
  CKH(launch_anneal(a, st));
  p->last_nsug = n_sug;
  p->an_nsug = n_sug;
  return copy_results(h, p, n_sug, out, out_on_device, st);
}

int tpe_plan_anneal_trace(tpe_plan_t p, int32_t n_suggest, tpe_anneal_trace *out) {
  if (!p || n_suggest < 0 || !out) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (n_suggest > p->an_nsug) return fail(h, TPE_E_INVALID, "more suggestions than the last call's");
  CKH(hipSetDevice(h->device));
  CKH(hipDeviceSynchronize());
  if (n_suggest > 0 && p->P > 0)
    CKH(hipMemcpy(out, p->d_an_trace, (size_t)n_suggest * p->P * sizeof(AnnealTrace),
                  hipMemcpyDeviceToHost));
  return TPE_OK;
}

int tpe_plan_set_prune(tpe_plan_t p, int32_t mode) {
  if (!p || mode < 0 || mode > 3) return TPE_E_INVALID;
  if (p->prune_mode != mode) graph_reset(p);
  p->prune_mode = mode;
  return TPE_OK;
}

int tpe_microbench(tpe_handle_t h, int32_t which, double *per_second) {
  if (!h || !per_second || which < 0 || which > 9) return TPE_E_INVALID;
  CKH(hipSetDevice(h->device));
  hipDeviceProp_t prop;
  CKH(hipGetDeviceProperties(&prop, h->device));
  const int blocks = prop.multiProcessorCount * 8;
  const int iters = which == 2 ? 256 : (which == 3 || which >= 5 ? 512 : (which == 4 ? 128 : 4096));
  double *sink = nullptr;
  CKH(dalloc(&sink, (size_t)blocks * 256));
  hipEvent_t a, b;
  CKH(hipEventCreate(&a));
  CKH(hipEventCreate(&b));
  CKH(launch_micro(which, blocks, iters, sink, h->stream));  // warm-up
  CKH(hipEventRecord(a, h->stream));
  for (int r = 0; r < 4; ++r) CKH(launch_micro(which, blocks, iters, sink, h->stream));
  CKH(hipEventRecord(b, h->stream));
  CKH(hipEventSynchronize(b));
  float ms = 0.f;
  CKH(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  dfree(sink);
  // results per thread-iteration: exp / FMA chains, erf chains, LSE pairs
  // (4 candidates x 8 components), quantized pairs (2 chains), shifted LSE
  // pairs (4 x 8), block-local fp32 one-exponent LSE pairs (4 x 2 blocks of
  // 8), the fp32 per-group-lift pairs (4 x 8), moment-form pairs (4 x 2
  // chunks of 16), 8-wide moment-form pairs (4 x 2 blocks of 8)
  static const double per_iter[10] = {8.0, 16.0, 4.0, 32.0, 2.0, 32.0, 64.0, 32.0, 128.0, 64.0};
  *per_second = 4.0 * blocks * 256.0 * iters * per_iter[which] / (ms * 1e-3);
  return TPE_OK;
}

int tpe_math_probe(tpe_handle_t h, int32_t which, const double *x, int64_t n, double *out) {
  if (!h) return TPE_E_INVALID;
  if (which < 0 || which > 3) return fail(h, TPE_E_INVALID, "unknown math helper");
  if (n < 0 || (n > 0 && (!x || !out))) return fail(h, TPE_E_INVALID, "bad args");
  if (n == 0) return TPE_OK;
  CKH(hipSetDevice(h->device));
  double *d = nullptr;
  CKH(dalloc(&d, 2 * (size_t)n));
  hipError_t e = hipMemcpyAsync(d, x, (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = launch_math_probe(which, d, n, d + n, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d + n, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  dfree(d);
  CKH(e);
  return TPE_OK;
}

int tpe_plan_last_stats(tpe_plan_t p, double *score_ms, double *pairs) {
  if (!p) return TPE_E_INVALID;
  tpe_engine *h = p->eng;
  if (!p->timed) return fail(h, TPE_E_INVALID, "no suggest recorded");
  CKH(hipSetDevice(h->device));
  if (p->evs) {
    CKH(hipEventSynchronize(p->ev1));
    float ms = 0.f;
    CKH(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    if (score_ms) *score_ms = ms;
  } else if (score_ms) {
    *score_ms = NAN;  // not timed: see tpe_plan_profile
  }
  if (pairs) {
    std::vector<MixInfo> info(2 * (size_t)p->P);
    std::vector<Partial> res((size_t)p->last_nsug * p->P);
    CKH(hipMemcpy(info.data(), p->d_info, info.size() * sizeof(MixInfo), hipMemcpyDeviceToHost));
    CKH(hipMemcpy(res.data(), p->d_results, res.size() * sizeof(Partial), hipMemcpyDeviceToHost));
    const int l0 = p->last_level < 0 ? 0 : p->last_level;
    const int l1 = p->last_level < 0 ? (int)p->levels.size() : p->last_level + 1;
    double acc = 0;
    for (int l = l0; l < l1; ++l)
      for (int hp : p->levels[l]) {
        if (p->hps[hp].family == TPE_CAT) continue;
        const double kk = (double)info[2 * hp].K + info[2 * hp + 1].K;
        for (int64_t s = 0; s < p->last_nsug; ++s)
          if (res[s * p->P + hp].active) acc += kk * (double)p->last_ncand;
      }
    *pairs = acc;
  }
  return TPE_OK;
}

}  // extern "C"
