// tpe_level_plan.hpp -- which launches one level of a suggest takes, as data.
// Pure host code: plan_level maps the compiled space (PlanShape), the process
// switches and what a call contributes (StepShape) to a LevelPlan; run_level
// (tpe_engine.hip) executes it, and the captured-graph key is the StepShape.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "tpe_internal.hpp"
#include "tpe_switches.hpp"

namespace tpe {

// candidate-slots (candidates x suggestions x level hps) of a chunk from which
// its draw is the sorted one
constexpr int64_t kSortedDrawMin = (int64_t)1 << 22;
constexpr int64_t kSmallSortMin = 2048;  // candidates per chunk worth bucketing a small draw
constexpr int64_t kTileDrawMax = 4096;   // candidates per chunk the scoring tiles draw themselves

// The most hps of hps[b, e) active together in one suggestion: the
// unconditional ones, plus, for every condition parent, the most hps that
// share one of its branch values.  (A parent takes one value per suggestion
// and an active hp has a true condition: charge it to that condition's
// parent; the hps charged to a parent share the branch it took.)
inline int32_t active_bound(const std::vector<tpe_hp> &all, const std::vector<int32_t> &cond_parent,
                            const std::vector<int32_t> &cond_branch, const int32_t *hps, int b,
                            int e) {
  int32_t n = 0;
  std::vector<std::pair<int32_t, int32_t>> pb;  // (parent, branch) of every condition
  for (int i = b; i < e; ++i) {
    const tpe_hp &x = all[hps[i]];
    if (x.cond_count == 0) { ++n; continue; }
    std::vector<std::pair<int32_t, int32_t>> mine;
    for (int c = 0; c < x.cond_count; ++c)
      mine.emplace_back(cond_parent[x.cond_begin + c], cond_branch[x.cond_begin + c]);
    std::sort(mine.begin(), mine.end());
    mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
    pb.insert(pb.end(), mine.begin(), mine.end());
  }
  std::sort(pb.begin(), pb.end());
  for (size_t i = 0; i < pb.size();) {
    int32_t best = 0;
    size_t j = i;
    while (j < pb.size() && pb[j].first == pb[i].first) {
      size_t k = j;
      while (k < pb.size() && pb[k] == pb[j]) ++k;
      best = std::max<int32_t>(best, (int32_t)(k - j));
      j = k;
    }
    n += best;
    i = j;
  }
  return std::min<int32_t>(n, e - b);
}

// What plan_level needs of one level, computed once (PlanShape::finish).
struct LevelShape {
  std::vector<int> kinds;  // score_kind of every slot
  int32_t n_lat = 0;       // leading quantized slots with a value lattice
  int64_t rmax = 0;        // ... the largest of those lattices
  int64_t cat_upper = 0;   // the largest categorical of the level
  bool table_slot = false; // a log-sum-exp slot has Chebyshev tables (table_hp)
  // active_bound of the ranges run_level sizes grids for: the whole level,
  // the leading lattice slots, and every run of equal-kind slots by its first
  // slot -- of the kinds as they are (rows_plain) and with the leading
  // lattice slots as one KIND_LAT run (rows_lat)
  int32_t rows_level = 0, rows_lead = 0;
  std::vector<int32_t> rows_plain, rows_lat;
};

// The static, host-side description of a compiled space.
struct PlanShape {
  std::vector<tpe_hp> hps;
  std::vector<int32_t> cond_parent, cond_branch;
  std::vector<std::vector<int32_t>> levels;
  std::vector<LatInfo> lat;      // value lattices of the bounded quantized hps (R = 0: none)
  int64_t kcap = 0;
  std::vector<double> act_frac;  // per hp: expected share of the trials it is active in
  std::vector<LevelShape> lv;    // derived from the above by finish()

  void finish() {
    lv.assign(levels.size(), {});
    for (size_t l = 0; l < levels.size(); ++l) {
      LevelShape &L = lv[l];
      const std::vector<int32_t> &hl = levels[l];
      const int n = (int)hl.size();
      for (int hp : hl) {
        const int k = score_kind(hps[hp]);
        L.kinds.push_back(k);
        if (k == KIND_CAT) L.cat_upper = std::max<int64_t>(L.cat_upper, hps[hp].upper);
        L.table_slot |= (k == KIND_LSE_G || k == KIND_LSE_L) && table_hp(hps[hp]);
      }
      while (L.n_lat < n && (L.kinds[L.n_lat] == KIND_ERF_G || L.kinds[L.n_lat] == KIND_ERF_L) &&
             lat[hl[L.n_lat]].R > 0) {
        L.rmax = std::max<int64_t>(L.rmax, lat[hl[L.n_lat]].R);
        ++L.n_lat;
      }
      auto bound = [&](int b, int e) {
        return active_bound(hps, cond_parent, cond_branch, hl.data(), b, e);
      };
      L.rows_level = bound(0, n);
      L.rows_lead = bound(0, L.n_lat);
      L.rows_plain.assign(n, 0);
      L.rows_lat.assign(n, 0);
      for (int with_lat = 0; with_lat < 2; ++with_lat) {
        auto kind = [&](int i) { return with_lat && i < L.n_lat ? (int)KIND_LAT : L.kinds[i]; };
        for (int j = 0; j < n;) {
          int k = j;
          while (k < n && kind(k) == kind(j)) ++k;
          (with_lat ? L.rows_lat : L.rows_plain)[j] = bound(j, k);
          j = k;
        }
      }
    }
  }
};

// size class of the largest below mixture a draw can meet
enum { BELOW_FUSE = 0,   // <= kFuseTab: the fused draw rows' and the tiles' LDS table
       BELOW_TABLE = 1,  // <= kTabCap: the LDS draw table
       BELOW_LARGE = 2 };
inline int below_class(int64_t k) {
  return k <= kFuseTab ? BELOW_FUSE : k <= kTabCap ? BELOW_TABLE : BELOW_LARGE;
}

// the fit a step takes, and with it the tables its scoring launches find
struct FitVariant {
  bool small = false;  // k_fit<true> serves the history (fit_small)
  int32_t mom_w = 0;   // the moment table written: 16 (CoefM), 8 (CoefM8), 0 none
  bool mom_h = false;  // ... and with 16, the degree-15 table (CoefMH)
  bool operator==(const FitVariant &o) const {
    return small == o.small && mom_w == o.mom_w && mom_h == o.mom_h;
  }
};

// The moment width of the plan's log-sum-exp mixtures (tpe_internal.hpp
// CoefM8): 16 when the largest expected above-side mixture (history length
// x the hp's expected activity) has >= kMom16MinK components (neighbour gaps
// << sigma floor: 16-component chunks qualify), 8 from the one-exponent size
// (lse_shift_min) up, else 0.  (tools/moment_error.py: at N = 5000 the 16-wide
// form covers 72 % of the live chunks at 0.6 VALU per pair, the 8-wide 99 %
// at ~1.7; at N = 3000, 36 % against 98 %.)  A function of the plan and its
// history length only, so tpe_plan_fit and fit_suggest write the same table.
inline int32_t mom_width(const PlanShape &ps, const Switches &sw, int64_t n_hist) {
  if (!sw.moment) return 0;
  double kmax = 0.0;
  for (size_t i = 0; i < ps.hps.size(); ++i) {
    const int k = score_kind(ps.hps[i]);
    if (k == KIND_LSE_G || k == KIND_LSE_L) kmax = std::max(kmax, (double)n_hist * ps.act_frac[i]);
  }
  if (kmax >= (double)kMom16MinK) return 16;
  if (kmax >= (double)sw.lse_shift_min) return 8;
  return 0;
}

// The moment table only for a step whose suggest takes a sorted draw on
// two-row wave tiles (> kWaveRowSplitMax candidates per suggestion), the only
// launches that read it; the others skip its ~3-5 us in k_fit.
inline bool step_reads_moments(const PlanShape &ps, int64_t n_sug, int64_t n_cand) {
  bool sorted = false;
  for (const auto &l : ps.levels) sorted |= n_cand * n_sug * (int64_t)l.size() >= kSortedDrawMin;
  return sorted && n_cand > kWaveRowSplitMax;
}

// small: fit_small(n_hist); moments: write the table of the plan's width
// (tpe_plan_fit: always; fit_suggest: step_reads_moments).  Whenever the table
// is read it is the one tpe_plan_fit writes, so a fit_suggest and a fit +
// suggest score alike.
inline FitVariant fit_variant(const PlanShape &ps, const Switches &sw, int64_t n_hist, bool small,
                              bool moments) {
  FitVariant f;
  f.small = small;
  f.mom_w = moments ? mom_width(ps, sw, n_hist) : 0;
  f.mom_h = f.mom_w == 16;
  return f;
}

// Everything a call contributes to plan_level's decisions, and nothing else:
// two calls with equal StepShapes take the same launches on the same grids
// (the captured-graph key of tpe_plan_fit_suggest).
struct StepShape {
  int64_t n_sug = 0, n_cand = 0, cand_begin = 0;
  // the candidates of the whole suggestion this call scores [cand_begin,
  // cand_begin + n_cand) of: it picks the wave-tile shape, so every shard and
  // batch of one suggestion takes the same
  int64_t n_total = 0;
  int32_t below = BELOW_LARGE;  // below_class of the last fit's n_below + 1
  FitVariant fit;               // the tables in place when the level runs
  int32_t prune_mode = 3;
  bool lattice_on = true;
  bool capturing = false;  // under graph capture: replays patch the seeds of the draw nodes only
  bool publish = false;    // results go to the host and the last launch may publish them
  // the run length of the integer screened draw (step_screen_run of the
  // process switches): its grid depends on it
  int32_t screen_run = 0;
  // the zones' rule and the pooled rows of the screened draw (step_screen_zone
  // and Switches::draw_screen_pool): halves < 0 is the whole-tile rule
  int32_t screen_halves = (int32_t)kDrawScreenHalves, screen_tail = (int32_t)kDrawScreenTail;
  bool screen_pool = false;
  // the lean table path (Switches::table_lean): the build takes a node more
  // (k_table_terms)
  bool table_lean = true;
  bool operator==(const StepShape &o) const {
    return n_sug == o.n_sug && n_cand == o.n_cand && cand_begin == o.cand_begin &&
           n_total == o.n_total && below == o.below && fit == o.fit &&
           prune_mode == o.prune_mode && lattice_on == o.lattice_on &&
           capturing == o.capturing && publish == o.publish && screen_run == o.screen_run &&
           screen_halves == o.screen_halves && screen_tail == o.screen_tail &&
           screen_pool == o.screen_pool && table_lean == o.table_lean;
  }
};
// StepShape::screen_run under the switches: TPE_DRAW_SCREEN_RUN for the integer
// screen, 0 (a block per sort block) for the float one
inline int32_t step_screen_run(const Switches &sw) {
  return sw.draw_screen && sw.draw_screen_int ? (int32_t)sw.draw_screen_run : 0;
}

// StepShape::screen_halves under the switches: -1 (the whole-tile rule, by
// draw_screen_tiles) when TPE_DRAW_SCREEN_TILES is set
inline int32_t step_screen_halves(const Switches &sw) {
  return sw.draw_screen_whole ? -1 : (int32_t)sw.draw_screen_halves;
}

// Scoring grid of one launch: runs of equal-kind slots become groups of the
// 1-D grid (tiles of tile_cands(kind) candidates); pstride: the partial-record
// stride (max tiles per slot), or -1 when there are more runs than kMaxGroups.
struct ScoreGrid {
  int32_t n_groups = 0, pstride = 1;
  int32_t grp_kind[kMaxGroups] = {}, grp_slot0[kMaxGroups] = {}, grp_tiles[kMaxGroups] = {};
  int32_t grp_block0[kMaxGroups + 1] = {}, grp_slots[kMaxGroups] = {};
  int32_t blocks() const { return grp_block0[n_groups]; }
};
// Groups are emitted heaviest kind first (per-candidate erf, then log-sum-exp,
// then the lattice / categorical lookups): the dispatcher hands out the long
// blocks first and the short ones fill the CUs that finish early.
// kind(j): slot j's kind; rows(b, e): block rows for the slots [b, e) of a
// group (e - b, or their active_bound on a compact grid).
template <typename Kind, typename Rows>
ScoreGrid score_grid(Kind kind, int n_slots, int64_t cn, Rows rows) {
  ScoreGrid g;
  int32_t blocks = 0;
  auto weight = [](int k) {
    if (k == KIND_ERF_G || k == KIND_ERF_L) return 0;
    if (kind_lse(k)) return 1;
    return k == KIND_LAT ? 2 : 3;
  };
  for (int pass = 0; pass < 4; ++pass) {
    for (int j = 0; j < n_slots;) {
      int k = j;
      while (k < n_slots && kind(k) == kind(j)) ++k;
      if (weight(kind(j)) != pass) { j = k; continue; }
      if (g.n_groups == kMaxGroups) { g.pstride = -1; return g; }
      const int i = g.n_groups++;
      const int64_t tc = tile_cands(kind(j));
      const int32_t nt = (int32_t)((std::max<int64_t>(cn, 0) + tc - 1) / tc);
      g.grp_kind[i] = kind(j);
      g.grp_slot0[i] = j;
      g.grp_slots[i] = k - j;
      g.grp_tiles[i] = nt;
      g.grp_block0[i] = blocks;
      blocks += nt * std::min<int32_t>(k - j, rows(j, k));
      g.pstride = std::max(g.pstride, nt);
      j = k;
    }
  }
  g.grp_block0[g.n_groups] = blocks;
  return g;
}

// the launch classes of a grid's groups (bit c: class c; 0 wave-tile
// log-sum-exp, 1 lookups drawing their own candidates, 2 the rest)
inline int grid_classes(const ScoreGrid &g, bool lookup_draw) {
  int m = 0;
  for (int i = 0; i < g.n_groups; ++i) {
    const int k = g.grp_kind[i];
    m |= 1 << (kind_wave_lse(k) ? 0 : lookup_draw && (k == KIND_CAT || k == KIND_LAT) ? 1 : 2);
  }
  return m;
}

// where the level's lattice launch runs
enum class LatRun {
  None,     // no slot is scored on a lattice
  InOrder,  // on the suggest stream, ahead of the chunks
  Side,     // on a side stream beside the draw; the scoring launch waits for it
  // first on the lookup stream of the first chunk -- in order before its
  // readers (the lookup tiles forked beside a sorted draw), one join after them
  Deferred,
  Fused,    // in the launch that also draws the candidates (k_lattice<true>)
};

// how a chunk's candidates are drawn
enum class Draw {
  Tiles,           // the scoring tiles draw their own (k_score_tdraw): no draw launch
  Fused,           // by extra blocks of the lattice launch
  Plain,           // k_draw
  Sorted,          // k_draw_sorted: value-bucketed, with positions
  SortedPruned,    // the first sort block, k_table_pilot, then k_draw_sorted_prune
  SortedScreened,  // the first sort block, the pilot, k_draw_zone, k_draw_sorted_screen
};

struct ChunkPlan {
  int64_t c0 = 0, cn = 0;  // candidates [c0, c0 + cn) of the call's
  bool accumulate = false; // merge with the results of the chunks before
  ScoreGrid grid;
  int32_t sort_log2 = 0, lse_pos = 0, lse_prune = 0, lse_f32 = 0, lookup_draw = 0;
  // the lookup tiles (class 1) forked onto the lookup stream ahead of the draw
  bool lk_fork = false;
  Draw draw = Draw::Plain;
  bool table_draw = false;   // below mixtures fit the LDS draw table (kTabCap)
  bool small_table = false;  // ... and the small one (kFuseTab)
  bool fast = false;         // the sorted draw without the out-of-line draws
  int32_t screen_tiles = 0;  // Draw::SortedScreened: the zones' widening
  int32_t screen_halves = 0; // ... in half tiles; -1: in screen_tiles whole tiles
  int32_t screen_tail = 128; // ... the tail zones' rank in the pilot's end tiles
  bool screen_pool = false;  // ... k_draw_sorted_screen_run's rows dense across the block
  int32_t screen_guide = -1; // ... the integer screen's guide bits; -1: the float screen
  int32_t screen_run = 0;    // ... its sort blocks per block (k_draw_sorted_screen_run); 0: one, as ever
  bool bucket = false;       // k_bucket follows the draw
  bool cand_pos = false;     // the scoring launch reads candidate positions
  // the main scoring launch: ScoreArgs::tab_on / tab_pref (2 behind a pruning
  // draw), its class mask, and whether its last record publishes the call
  int32_t tab_on = 0, tab_pref = 0;
  int classes = 7;
  bool publish = false;
};

struct LevelPlan {
  bool empty = false;  // no candidates: every hp of the level gets the neutral record
  int32_t n_level = 0;
  int32_t n_lat = 0;      // leading slots scored on their lattices (KIND_LAT)
  int32_t lat_rows = 0;   // grid rows of the lattice launch
  bool compact = false;   // grids sized for the hps that can be active together
  int32_t slot_rows = 0;
  bool erf_level = false; // per-candidate quantized slots (left after the lattice ones)
  LatRun lat = LatRun::None;
  int32_t lse_shift_min = 0;
  std::vector<ChunkPlan> chunks;
};

inline LevelPlan plan_level(const PlanShape &ps, const Switches &sw, const StepShape &s,
                            int level) {
  const LevelShape &L = ps.lv[level];
  const std::vector<int32_t> &hl = ps.levels[level];
  const int32_t n_level = (int32_t)hl.size();
  const int64_t n_sug = s.n_sug, n_cand = s.n_cand;
  LevelPlan lp;
  lp.n_level = n_level;
  lp.lse_shift_min = (int32_t)sw.lse_shift_min;
  if (n_cand == 0) {
    lp.empty = true;
    return lp;
  }
  // largest below mixture the draw can meet: the LDS table samplers fit it?
  const int below = std::max(s.below, below_class(L.cat_upper));
  const bool table_draw = below <= BELOW_TABLE, small_table = below == BELOW_FUSE;
  // the level's leading quantized hps with a value lattice are scored on it
  // (k_lattice once per call, then lookups) when no lattice is larger than
  // the candidate count; the other quantized hps per candidate (bucketed)
  const bool lat_level = L.n_lat > 0 && s.lattice_on && L.rmax <= n_cand * n_sug &&
                         2 * ((ps.kcap + 15) / 16) <= (int64_t)kLatChunks;
  const int32_t n_lat = lat_level ? L.n_lat : 0;
  lp.n_lat = n_lat;
  bool has_other = false;  // slots that are neither lattice nor categorical lookups
  for (int i = n_lat; i < n_level; ++i) {
    lp.erf_level |= L.kinds[i] == KIND_ERF_G || L.kinds[i] == KIND_ERF_L;
    has_other |= L.kinds[i] != KIND_CAT;
  }
  // conditional level: grids sized for the hps that can be active together
  // (ScoreArgs::compact), not one row per hp -- the other branches of a
  // choice cost no blocks
  lp.compact = L.rows_level < n_level;
  lp.slot_rows = lp.compact ? L.rows_level : n_level;
  lp.lat_rows = lp.compact && n_lat > 0
                    ? (int32_t)std::min<int64_t>(n_lat, n_sug * (int64_t)L.rows_lead)
                    : n_lat;
  auto rows = [&](int b, int e) {
    return lp.compact ? (lat_level ? L.rows_lat : L.rows_plain)[b] : e - b;
  };
  // candidates are processed in chunks so the buffer stays within the budget
  int64_t chunk = std::max<int64_t>(
      1, std::min<int64_t>(n_cand, sw.chunk_budget() / std::max<int64_t>(1, n_sug * n_level)));
  // several chunks: each a whole number of sorted-draw blocks, so the blocks
  // (and with them every pruned log-sum-exp) sit at the same global candidate
  // indices however [0, n) is chunked or sharded (TPE_SHARD_ALIGN)
  if (chunk < n_cand) chunk = std::max<int64_t>(kSortedBlock, chunk / kSortedBlock * kSortedBlock);
  auto sorted_size = [&](int64_t cn) { return cn * n_sug * n_level >= kSortedDrawMin; };
  // a small one-chunk draw whose tables fit kFuseTab runs in extra blocks of
  // the lattice launch (both only need the fitted mixtures): one launch less
  // and the draw hidden behind the lattice points
  const bool fuse_draw = lat_level && n_lat <= kLatJobs && small_table && chunk >= n_cand &&
                         !sorted_size(n_cand);
  // the lattice needs only the fitted mixtures: with side streams (and unless
  // it carries the draw) it runs beside the candidate draw (a parallel branch
  // of the captured graph).  Default: in order on the suggest stream -- round
  // 5, config 3: 0.193 ms per suggest in order against 0.201 ms forked (the
  // cross-stream joins cost more than the overlap saves; profiles/rd5h_*)
  const bool lookup_inline = small_table && !s.capturing && sw.lookup_draw;
  const bool lat_defer = lat_level && !fuse_draw && !sw.side_streams && has_other &&
                         table_draw && sorted_size(std::min(chunk, n_cand)) && lookup_inline &&
                         sw.lookup_fork;
  lp.lat = !lat_level ? LatRun::None
           : fuse_draw ? LatRun::Fused
           : lat_defer ? LatRun::Deferred
           : sw.side_streams ? LatRun::Side : LatRun::InOrder;
  // log-sum-exp tiles: two candidate rows per lane, unless that leaves fewer
  // than ~3 blocks per CU (then whole-block work units are few and coarse, and
  // a CU with one more of them than its neighbours sets the launch time):
  // one-row tiles double the count at the same per-pair arithmetic
  int64_t lse_slots = 0;
  for (int j = 0; j < n_level;) {  // active rows of the log-sum-exp runs
    int k = j;
    while (k < n_level && L.kinds[k] == L.kinds[j]) ++k;
    if (j >= n_lat && (L.kinds[j] == KIND_LSE_G || L.kinds[j] == KIND_LSE_L))
      lse_slots += rows(j, k);
    j = k;
  }
  const bool one_row = lse_slots > 0 && n_sug * lse_slots * ((n_cand + 127) / 128) < 3 * kNumCUs;
  // suggestions of <= kWaveRowSplitMax candidates: one-row wave tiles, 64
  // candidates per wave -- the dense windows' waves carry half the pairs; a
  // small level leaves the GPU room for twice the waves
  const bool wave1 = s.n_total <= kWaveRowSplitMax;

  for (int64_t c0 = 0; c0 < n_cand; c0 += chunk) {
    ChunkPlan c;
    c.c0 = c0;
    c.cn = std::min(chunk, n_cand - c0);
    c.accumulate = c0 > 0;
    c.table_draw = table_draw;
    c.small_table = small_table;
    // large draws: each draw block writes its candidates value-bucketed (LSE
    // and per-candidate erf slots) with their positions; the log-sum-exp
    // tiles then skip the component blocks that are exact zeros for them,
    // on wave tiles when the wave-wide exponent is on (prune mode 2)
    const bool sorted = !fuse_draw && table_draw && sorted_size(c.cn);
    // small draws of >= kSmallSortMin candidates: the log-sum-exp slots are
    // value-bucketed too (k_bucket, stable, <= 8192 per bucketing chunk) and
    // pruned on the 8-wave tiles
    const bool small_sort = !sorted && sw.small_sort && c.cn >= kSmallSortMin && lse_slots > 0;
    // pruned log-sum-exp slots on wave tiles: each wave its own 128
    // candidates and every live block, so its one exponent and its accuracy
    // guard see the whole sum.  (Round 4, config 3: 8-wave component-split
    // tiles below 2^18 candidates measured 0.265 ms with the one-exponent
    // form -- a wave's guard sees 1/8 of the components and 3e7 pairs per
    // launch were retried -- and 0.236 ms without it, against 0.234 ms here.)
    const bool wave = sorted && s.prune_mode > 1;
    // (small_sort: one-row tiles whatever the batch size: the pruned sums
    // depend on the tile's candidate window, so a batched suggestion stays
    // bit-identical to the same seed's single one)
    auto kind = [&](int i) -> int {
      if (i < n_lat) return KIND_LAT;
      const int k = L.kinds[i];
      if (k != KIND_LSE_G && k != KIND_LSE_L) return k;
      const bool lg = k == KIND_LSE_L;
      if (wave) return wave1 ? (lg ? KIND_LSE_LW1 : KIND_LSE_GW1) : (lg ? KIND_LSE_LW : KIND_LSE_GW);
      return one_row || small_sort ? (lg ? KIND_LSE_L1 : KIND_LSE_G1) : k;
    };
    c.grid = score_grid(kind, n_level, c.cn, rows);
    c.lse_pos = sorted || small_sort ? 1 : 0;
    c.sort_log2 = sort_log2_for(s.n_total);  // (the whole suggestion's: shards agree)
    // lookup slots drawn by their scoring tiles (no write / read-back of their
    // candidates); not in a captured graph, whose replays patch the seeds of
    // the draw nodes only.  (Every lookup slot's below mixture within the
    // tile's LDS table, so all of them are drawn in their tiles and none reads
    // the draw's output.)
    c.lookup_draw = sorted && lookup_inline ? 1 : 0;
    c.lse_prune = sorted || small_sort ? s.prune_mode : 0;
    // prune mode 3's block-local fp32 pairs on every log-sum-exp slot of the
    // suggest, pruned (large draws) or not (small draws: every pair, 8-wave
    // component-split tiles)
    c.lse_f32 = s.prune_mode == 3 ? 1 : 0;
    // Chebyshev tables (TabHdr): suggests of > kWaveRowSplitMax candidates
    // (n_total: shards agree) in prune mode 3 whose mixtures are in the
    // 16-wide moment class, for the level's bounded continuous hps on two-row
    // wave tiles -- the slots whose two tables are certified go through
    // k_score_table, and k_score_wave_tie scores directly only the waves near
    // the best table score
    c.tab_on = L.table_slot && wave && !wave1 && s.prune_mode == 3 && s.fit.mom_w == 16 && sw.table
                   ? 1 : 0;
    c.tab_pref = c.tab_on && sw.table_prefilter ? 1 : 0;
    // lookup tiles drawing their own candidates need nothing from this
    // chunk's draw: forked onto an auxiliary stream, they run beside the draw
    // and the log-sum-exp scoring, and the suggest stream waits for them
    // before the next chunk
    const int cls = grid_classes(c.grid, c.lookup_draw != 0);
    c.lk_fork = (cls & 2) && (cls & ~2) && sw.lookup_fork;
    c.classes = c.lk_fork ? 5 : 7;
    // tiny unsorted draws of levels with no lattice and no per-candidate erf
    // slots: the scoring tiles draw their own candidates (k_score_tdraw) --
    // one launch less (the config-1 shape: 24 candidates of one hp)
    const bool tdraw = !sorted && !small_sort && !fuse_draw && !lat_level && !lp.erf_level &&
                       small_table && c.cn <= kTileDrawMax && !s.capturing && sw.tile_draw;
    // the call's last launch (its last level, one chunk, a full grid): its
    // last final record publishes the call's results (k_publish's work)
    c.publish = tdraw && s.publish && level + 1 == (int)ps.levels.size() && c.cn == n_cand &&
                s.cand_begin == 0 && s.n_total == n_cand && !lp.compact && !c.lk_fork &&
                c.grid.n_groups > 0 && c.grid.blocks() > 0 && sw.publish_fuse;
    if (tdraw) {
      c.draw = Draw::Tiles;
    } else if (fuse_draw) {
      c.draw = Draw::Fused;
    } else if (sorted) {
      // the inline-draw kernel when every slot it draws is bounded continuous
      // (the lookup slots drawn in their tiles are skipped by it)
      c.fast = true;
      for (int i = 0; i < n_level && c.fast; ++i) {
        const tpe_hp &x = ps.hps[hl[i]];
        const bool lookup = i < n_lat || L.kinds[i] == KIND_CAT;
        c.fast = lookup ? c.lookup_draw != 0
                        : (x.family != TPE_CAT && (x.flags & TPE_HAS_LOW) && (x.flags & TPE_HAS_HIGH));
      }
      // The pruning draw: behind the prefilter the hot intervals
      // depend on the launch's first sort block alone, so that block is drawn
      // first (written in full), k_table_pilot reads it -- the tables and
      // bound lattices built ahead of it -- and the other sort blocks are
      // drawn by the kernel that drops the wave tiles the intervals rule out.
      // A chunk of one sort block has nothing to prune.
      const bool prune = c.tab_on == 1 && c.tab_pref && (cls & 1) && sw.draw_prune &&
                         c.sort_log2 == kSortLog2Large && c.cn > kSortedBlock;
      // the fast small-table pruning draws screen their candidates on u1 first
      // from draw_screen_min candidate-slots up: below, k_draw_zone's ~33 us
      // ahead of the draw cost more than the screen saves
      const bool screen = prune && c.fast && small_table && sw.draw_screen &&
                          c.cn * n_sug * n_level >= sw.draw_screen_min;
      c.draw = screen ? Draw::SortedScreened : prune ? Draw::SortedPruned : Draw::Sorted;
      c.screen_tiles = (int32_t)sw.draw_screen_tiles;
      c.screen_halves = s.screen_halves;
      c.screen_tail = s.screen_tail;
      c.screen_pool = s.screen_pool;
      c.screen_guide = sw.draw_screen_int ? (int32_t)sw.draw_screen_guide_bits : -1;
      c.screen_run = screen && c.screen_guide >= 0 ? s.screen_run : 0;
      if (prune) c.tab_pref = 2;
    } else {
      c.draw = Draw::Plain;
    }
    c.bucket = (lp.erf_level || small_sort) && !sorted;
    c.cand_pos = lp.erf_level || sorted || small_sort;
    lp.chunks.push_back(c);
  }
  return lp;
}

}  // namespace tpe
