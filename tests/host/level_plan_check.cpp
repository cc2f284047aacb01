// level_plan_check.cpp -- host-only checks of the launch plan of a level
// (tpe_level_plan.hpp) and of the switch table (tpe_switches.hpp).  Every
// expected value is written out from the constants of tpe_internal.hpp and the
// documented rules; none is computed by the code under test.
// Built and run by tests/test_level_plan.py; exit status 0: all checks passed.
#include <cstdio>
#include <cstring>

#include "../../hyperopt_amd/csrc/tpe_level_plan.hpp"
#include "../../hyperopt_amd/csrc/tpe_switches.hpp"

using namespace tpe;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static_assert(kFuseTab == 32 && kTabCap == 2048 && kSortedBlock == 8192, "constants the cases use");
static_assert(kWaveRowSplitMax == (1 << 18) && kMom16MinK == 4000, "constants the cases use");
static_assert(kSortLog2Small == 12 && kSortLog2Large == 13 && kNumCUs == 256, "constants");
static_assert(kSortedDrawMin == (1 << 22) && kDrawScreenMin == (1 << 26), "thresholds");

static tpe_hp uniform_hp(double lo, double hi) {
  tpe_hp x{};
  x.family = TPE_GMM;
  x.flags = TPE_HAS_LOW | TPE_HAS_HIGH;
  x.prior_mu = 0.5 * (lo + hi);
  x.prior_sigma = hi - lo;
  x.low = lo;
  x.high = hi;
  return x;
}
static tpe_hp quniform_hp(double lo, double hi, double q) {
  tpe_hp x = uniform_hp(lo, hi);
  x.flags |= TPE_HAS_Q;
  x.q = q;
  return x;
}
static tpe_hp loguniform_hp(double lo, double hi) {
  tpe_hp x = uniform_hp(lo, hi);
  x.family = TPE_LGMM;
  x.obs_transform = TPE_OBS_LOG;
  return x;
}
static tpe_hp choice_hp(int upper) {
  tpe_hp x{};
  x.family = TPE_CAT;
  x.upper = upper;
  return x;
}
static tpe_hp normal_hp() {
  tpe_hp x{};
  x.family = TPE_GMM;
  x.prior_sigma = 1.0;
  return x;
}

// a one-level unconditional space; R[i]: the value lattice of hp i (0: none)
static PlanShape flat_space(const std::vector<tpe_hp> &hps, const std::vector<int32_t> &R) {
  PlanShape ps;
  ps.hps = hps;
  ps.levels.assign(1, {});
  int64_t off = 0;
  for (size_t i = 0; i < hps.size(); ++i) {
    ps.levels[0].push_back((int32_t)i);
    ps.lat.push_back(LatInfo{0, off, R[i], 0});
    off += R[i];
  }
  ps.kcap = 1024;
  ps.act_frac.assign(hps.size(), 1.0);
  ps.finish();
  return ps;
}
static PlanShape uniform16() {
  return flat_space(std::vector<tpe_hp>(16, uniform_hp(-5, 5)), std::vector<int32_t>(16, 0));
}

static Switches default_switches() {
  return read_switches([](const char *) -> const char * { return nullptr; });
}

static StepShape step(int64_t n_sug, int64_t n_cand) {
  StepShape s;
  s.n_sug = n_sug;
  s.n_cand = n_cand;
  s.n_total = n_cand;
  s.below = BELOW_FUSE;
  return s;
}

static bool sorted_draw(const ChunkPlan &c) {
  return c.draw == Draw::Sorted || c.draw == Draw::SortedPruned || c.draw == Draw::SortedScreened;
}
// screened => pruned => tab_pref => tab_on => sorted draw, on every chunk
static void check_chain(const LevelPlan &lp) {
  for (const ChunkPlan &c : lp.chunks) {
    const bool screened = c.draw == Draw::SortedScreened;
    const bool pruned = screened || c.draw == Draw::SortedPruned;
    CHECK(!pruned || c.tab_pref == 2);
    CHECK(c.tab_pref != 2 || pruned);
    CHECK(!c.tab_pref || c.tab_on == 1);
    CHECK(!c.tab_on || sorted_draw(c));
  }
}
static bool one_group(const ChunkPlan &c, int kind) {
  return c.grid.n_groups == 1 && c.grid.grp_kind[0] == kind;
}

static void case_switches() {
  const Switches d = default_switches();
  CHECK(d.lookup_draw && d.lookup_fork && d.publish && d.tile_draw && d.publish_fuse && d.moment &&
        d.table && d.draw_prune && d.draw_screen && d.table_prefilter && d.table_scalar);
  CHECK(!d.small_sort && !d.side_streams && !d.graph);
  CHECK(d.table_tie() == 0x1p-16 && d.draw_screen_tiles == 2 &&
        d.draw_screen_min == ((int64_t)1 << 26) && d.chunk_budget() == ((int64_t)8192 << 17) &&
        d.lse_shift_min == 512);
  struct Env { const char *name, *text; };
  static const Env env[] = {
      {"TPE_TABLE", ""},           // empty counts as 0: off
      {"TPE_MOMENT", "1"},
      {"TPE_PUBLISH", "0"},
      {"TPE_DRAW_PRUNE", ""},      // empty: stays on
      {"TPE_DRAW_SCREEN", "0"},
      {"TPE_TABLE_SCALAR", "no"},  // non-empty, atoi 0: off
      {"TPE_SMALL_SORT", "1"},
      {"TPE_SIDE_STREAMS", "0"},   // set at all: on
      {"TPE_GRAPH", ""},
      {"TPE_TABLE_TIE_LOG2", "5000"},
      {"TPE_DRAW_SCREEN_TILES", "100"},
      {"TPE_DRAW_SCREEN_MIN", ""},  // empty: the default
      {"TPE_CHUNK_MB", "512"},
      {"TPE_SHIFT_MIN_K", "0"},
  };
  const Switches s = read_switches([](const char *name) -> const char * {
    for (const Env &e : env)
      if (!std::strcmp(e.name, name)) return e.text;
    return nullptr;
  });
  CHECK(!s.table && s.moment && !s.publish && s.draw_prune && !s.draw_screen && !s.table_scalar);
  CHECK(s.lookup_draw && s.table_prefilter);
  CHECK(s.small_sort && s.side_streams && s.graph);
  CHECK(s.table_tie_log2 == 4096 && s.draw_screen_tiles == 64 &&
        s.draw_screen_min == ((int64_t)1 << 26) && s.chunk_budget() == ((int64_t)512 << 17) &&
        s.lse_shift_min == 0);
  const Switches t = read_switches([](const char *name) -> const char * {
    if (!std::strcmp(name, "TPE_SMALL_SORT")) return "0";
    if (!std::strcmp(name, "TPE_TABLE_TIE_LOG2")) return "-2000";
    return nullptr;
  });
  CHECK(!t.small_sort && t.table_tie_log2 == -1074);
}

// a. sixteen bounded uniform hps, one suggestion
static void case_a() {
  const PlanShape ps = uniform16();
  const Switches sw = default_switches();
  {
    const LevelPlan lp = plan_level(ps, sw, step(1, 1 << 18), 0);
    CHECK(!lp.empty && lp.chunks.size() == 1 && lp.lat == LatRun::None && !lp.compact);
    const ChunkPlan &c = lp.chunks[0];
    CHECK(c.draw == Draw::Sorted && c.fast && c.small_table);
    CHECK(one_group(c, KIND_LSE_GW1) && c.sort_log2 == 12);
    // 512-candidate blocks: 512 tiles per slot, 16 slots
    CHECK(c.grid.pstride == 512 && c.grid.blocks() == 8192);
    CHECK(c.lse_pos == 1 && c.lse_prune == 3 && c.lse_f32 == 1 && c.cand_pos && !c.bucket);
    CHECK(c.tab_on == 0 && c.tab_pref == 0 && !c.lk_fork && c.classes == 7 && !c.publish);
    check_chain(lp);
  }
  {
    const LevelPlan lp = plan_level(ps, sw, step(1, (1 << 18) - 1), 0);
    const ChunkPlan &c = lp.chunks[0];
    CHECK(lp.chunks.size() == 1 && c.draw == Draw::Plain && c.table_draw);
    CHECK(one_group(c, KIND_LSE_G) && c.lse_pos == 0 && c.lse_prune == 0 && !c.cand_pos);
    check_chain(lp);
  }
  {
    const LevelPlan lp = plan_level(ps, sw, step(1, (1 << 18) + 8192), 0);
    const ChunkPlan &c = lp.chunks[0];
    CHECK(lp.chunks.size() == 1 && c.draw == Draw::Sorted);
    CHECK(one_group(c, KIND_LSE_GW) && c.sort_log2 == 13);
    // 1024-candidate blocks: 270336 / 1024 = 264 tiles per slot
    CHECK(c.grid.pstride == 264 && c.grid.blocks() == 264 * 16);
    check_chain(lp);
  }
  {
    StepShape s = step(1, 0);
    const LevelPlan lp = plan_level(ps, sw, s, 0);
    CHECK(lp.empty && lp.n_level == 16 && lp.chunks.empty());
  }
}

// b. the case-a space at 2^18 + 8192 with the 16-wide moment tables
static void case_b() {
  const PlanShape ps = uniform16();
  const Switches sw = default_switches();
  StepShape s = step(1, (1 << 18) + 8192);
  s.fit.mom_w = 16;
  s.fit.mom_h = true;
  auto first = [&](const Switches &w, const StepShape &st) {
    const LevelPlan lp = plan_level(ps, w, st, 0);
    check_chain(lp);
    CHECK(lp.chunks.size() == 1);
    return lp.chunks[0];
  };
  {
    const ChunkPlan c = first(sw, s);
    CHECK(c.tab_on == 1 && c.tab_pref == 2 && c.draw == Draw::SortedPruned && c.fast);
    // (4325376 candidate-slots < 2^26: not screened)
  }
  Switches w0 = sw;
  w0.draw_screen_min = 0;
  {
    const ChunkPlan c = first(w0, s);
    CHECK(c.tab_on == 1 && c.tab_pref == 2 && c.draw == Draw::SortedScreened);
    CHECK(c.screen_tiles == 2);
  }
  {
    Switches w = w0;
    w.draw_screen = false;
    CHECK(first(w, s).draw == Draw::SortedPruned);
  }
  {
    StepShape t = s;
    t.fit.mom_w = 8;
    t.fit.mom_h = false;
    const ChunkPlan c = first(w0, t);
    CHECK(c.tab_on == 0 && c.tab_pref == 0 && c.draw == Draw::Sorted && one_group(c, KIND_LSE_GW));
  }
  {
    StepShape t = s;
    t.prune_mode = 2;
    const ChunkPlan c = first(w0, t);
    CHECK(c.tab_on == 0 && c.tab_pref == 0 && c.draw == Draw::Sorted && one_group(c, KIND_LSE_GW));
    CHECK(c.lse_prune == 2 && c.lse_f32 == 0);
  }
  {
    Switches w = w0;
    w.table = false;
    const ChunkPlan c = first(w, s);
    CHECK(c.tab_on == 0 && c.tab_pref == 0 && c.draw == Draw::Sorted);
  }
  {
    Switches w = w0;
    w.table_prefilter = false;
    const ChunkPlan c = first(w, s);
    CHECK(c.tab_on == 1 && c.tab_pref == 0 && c.draw == Draw::Sorted);
  }
  {
    Switches w = w0;
    w.draw_prune = false;
    const ChunkPlan c = first(w, s);
    CHECK(c.tab_on == 1 && c.tab_pref == 1 && c.draw == Draw::Sorted);
  }
  {
    // below mixtures past kFuseTab: no screen (it needs the small table); the
    // pruning draw stays
    StepShape t = s;
    t.below = BELOW_TABLE;
    const ChunkPlan c = first(w0, t);
    CHECK(c.tab_on == 1 && c.tab_pref == 2 && c.draw == Draw::SortedPruned && !c.small_table);
    CHECK(c.lookup_draw == 0);
    t.below = BELOW_LARGE;  // past the draw table: no sorted draw at all
    const ChunkPlan d = first(w0, t);
    CHECK(d.draw == Draw::Plain && !d.table_draw && d.tab_on == 0);
  }
  {
    // chunks of one sort block (32 suggestions x 16 hps x 8192 = 2^22 slots:
    // still sorted draws): nothing to prune
    Switches w = w0;
    w.chunk_mb = 32;  // 2^22 doubles / (32 x 16) = 8192 candidates
    StepShape t = s;
    t.n_sug = 32;
    const LevelPlan lp = plan_level(ps, w, t, 0);
    check_chain(lp);
    CHECK(lp.chunks.size() == 33);
    for (const ChunkPlan &c : lp.chunks) {
      CHECK(c.cn == 8192 && one_group(c, KIND_LSE_GW));
      CHECK(c.tab_on == 1 && c.tab_pref == 1 && c.draw == Draw::Sorted);
    }
  }
}

// c. one uniform hp, 24 candidates
static void case_c() {
  const PlanShape ps = flat_space({uniform_hp(-5, 5)}, {0});
  const Switches sw = default_switches();
  StepShape s = step(1, 24);
  {
    const LevelPlan lp = plan_level(ps, sw, s, 0);
    const ChunkPlan &c = lp.chunks[0];
    CHECK(lp.chunks.size() == 1 && c.draw == Draw::Tiles && !c.publish && !c.bucket);
    CHECK(one_group(c, KIND_LSE_G1) && c.grid.blocks() == 1);  // 1 block < 3 per CU: one-row tiles
  }
  s.publish = true;
  CHECK(plan_level(ps, sw, s, 0).chunks[0].publish);
  {
    Switches w = sw;
    w.publish_fuse = false;
    CHECK(!plan_level(ps, w, s, 0).chunks[0].publish);
    w = sw;
    w.tile_draw = false;
    const ChunkPlan c = plan_level(ps, w, s, 0).chunks[0];
    CHECK(c.draw == Draw::Plain && !c.publish);
  }
  {
    StepShape t = s;  // a shard does not publish
    t.n_total = 48;
    CHECK(!plan_level(ps, sw, t, 0).chunks[0].publish);
  }
  s.capturing = true;
  {
    const ChunkPlan c = plan_level(ps, sw, s, 0).chunks[0];
    CHECK(c.draw == Draw::Plain && c.lookup_draw == 0 && !c.publish);
  }
}

// d. a small chunk budget on the case-a space
static void case_d() {
  const PlanShape ps = uniform16();
  Switches sw = default_switches();
  sw.chunk_mb = 4;  // 2^19 doubles
  const int64_t n = (1 << 18) + 8192;
  for (int64_t n_sug : {1, 3}) {
    // 2^19 / 16 = 32768 candidates per chunk; 2^19 / 48 = 10922 -> 8192
    const int64_t want = n_sug == 1 ? 32768 : 8192;
    const LevelPlan lp = plan_level(ps, sw, step(n_sug, n), 0);
    CHECK((int64_t)lp.chunks.size() == (n + want - 1) / want);
    int64_t at = 0;
    for (size_t i = 0; i < lp.chunks.size(); ++i) {
      const ChunkPlan &c = lp.chunks[i];
      CHECK(c.c0 == at && c.cn > 0);
      CHECK(c.accumulate == (i > 0));
      if (i + 1 < lp.chunks.size()) CHECK(c.cn == want && c.cn % kSortedBlock == 0);
      at += c.cn;
    }
    CHECK(at == n);
    check_chain(lp);
  }
}

// e. sharding: the shards take the whole suggestion's tiles
static void case_e() {
  const PlanShape ps = uniform16();
  const Switches sw = default_switches();
  const int64_t n = 1 << 19, a = 1 << 18;  // (a shard's own size would give one-row wave tiles)
  const ChunkPlan whole = plan_level(ps, sw, step(1, n), 0).chunks[0];
  CHECK(one_group(whole, KIND_LSE_GW) && whole.sort_log2 == 13);
  StepShape lo = step(1, a), hi = step(1, n - a);
  lo.n_total = hi.n_total = n;
  hi.cand_begin = a;
  for (const StepShape &s : {lo, hi}) {
    const LevelPlan lp = plan_level(ps, sw, s, 0);
    CHECK(lp.chunks.size() == 1);
    const ChunkPlan &c = lp.chunks[0];
    CHECK(one_group(c, KIND_LSE_GW) && c.sort_log2 == 13 && c.draw == Draw::Sorted);
    CHECK(c.lse_prune == whole.lse_prune && c.lse_pos == whole.lse_pos);
  }
}

// f. a quantized-plus-categorical level (config 2's quniform(0, 100, 1) and
// choice-of-4 hps; lattice of 105 points: rint(100) + 2 - (rint(0) - 2) + 1)
static void case_f() {
  std::vector<tpe_hp> hps;
  std::vector<int32_t> R;
  for (int i = 0; i < 5; ++i) { hps.push_back(quniform_hp(0, 100, 1)); R.push_back(105); }
  for (int i = 0; i < 5; ++i) { hps.push_back(choice_hp(4)); R.push_back(0); }
  const PlanShape ps = flat_space(hps, R);
  const Switches sw = default_switches();
  Switches side = sw;
  side.side_streams = true;
  {
    const LevelPlan lp = plan_level(ps, sw, step(1, 4096), 0);
    CHECK(lp.lat == LatRun::Fused && lp.n_lat == 5 && lp.lat_rows == 5 && !lp.erf_level);
    CHECK(lp.chunks.size() == 1 && lp.chunks[0].draw == Draw::Fused && !lp.chunks[0].bucket);
    CHECK(lp.chunks[0].grid.n_groups == 2 && lp.chunks[0].grid.grp_kind[0] == KIND_LAT &&
          lp.chunks[0].grid.grp_kind[1] == KIND_CAT);
    CHECK(plan_level(ps, side, step(1, 4096), 0).lat == LatRun::Fused);
  }
  {
    StepShape s = step(1, 4096);
    s.below = BELOW_TABLE;  // above the kFuseTab class
    const LevelPlan lp = plan_level(ps, sw, s, 0);
    CHECK(lp.lat == LatRun::InOrder && lp.chunks[0].draw == Draw::Plain);
    CHECK(plan_level(ps, side, s, 0).lat == LatRun::Side);
  }
  {
    const StepShape s = step(1, 1 << 19);  // 10 x 2^19 >= 2^22 candidate-slots
    const LevelPlan lp = plan_level(ps, sw, s, 0);
    CHECK(lp.lat == LatRun::InOrder && lp.chunks[0].draw == Draw::Sorted);
    CHECK(lp.chunks[0].lookup_draw == 1 && !lp.chunks[0].lk_fork);  // lookups only: no fork
    CHECK(plan_level(ps, side, s, 0).lat == LatRun::Side);
  }
  {
    StepShape s = step(1, 64);  // a lattice larger than the draw: per candidate
    const LevelPlan lp = plan_level(ps, sw, s, 0);
    CHECK(lp.lat == LatRun::None && lp.n_lat == 0 && lp.erf_level);
    CHECK(lp.chunks[0].draw == Draw::Plain && lp.chunks[0].bucket && lp.chunks[0].cand_pos);
    s = step(1, 4096);
    s.lattice_on = false;
    CHECK(plan_level(ps, sw, s, 0).lat == LatRun::None);
  }
  // with log-sum-exp slots in the level, the lookups are forked beside a
  // sorted draw and the lattice goes first on their stream
  hps.insert(hps.begin() + 5, 5, uniform_hp(-5, 5));
  R.insert(R.begin() + 5, 5, 0);
  const PlanShape pm = flat_space(hps, R);
  {
    const StepShape s = step(1, 1 << 19);
    const LevelPlan lp = plan_level(pm, sw, s, 0);
    CHECK(lp.lat == LatRun::Deferred && lp.chunks.size() == 1);
    const ChunkPlan &c = lp.chunks[0];
    CHECK(c.lk_fork && c.classes == 5 && c.lookup_draw == 1 && c.draw == Draw::Sorted && c.fast);
    CHECK(c.grid.n_groups == 3 && c.grid.grp_kind[0] == KIND_LSE_GW &&
          c.grid.grp_kind[1] == KIND_LAT && c.grid.grp_kind[2] == KIND_CAT);
    Switches w = sw;
    w.lookup_fork = false;
    CHECK(plan_level(pm, w, s, 0).lat == LatRun::InOrder);
    CHECK(!plan_level(pm, w, s, 0).chunks[0].lk_fork);
    CHECK(plan_level(pm, side, s, 0).lat == LatRun::Side);
    StepShape t = s;
    t.capturing = true;
    const LevelPlan lc = plan_level(pm, sw, t, 0);
    CHECK(lc.lat == LatRun::InOrder && !lc.chunks[0].lk_fork && lc.chunks[0].lookup_draw == 0);
    CHECK(!lc.chunks[0].fast);  // (the draw writes the lookup slots)
  }
}

// g. the graph key: history length moves it only across a class boundary
static void case_g() {
  const PlanShape ps = uniform16();
  const Switches sw = default_switches();
  auto at = [&](int64_t n_hist, int32_t nb) {
    StepShape s = step(1, (1 << 18) + 8192);
    s.below = below_class((int64_t)nb + 1);
    s.fit = fit_variant(ps, sw, n_hist, false, true);
    s.capturing = true;
    return s;
  };
  CHECK(at(600, 25).fit.mom_w == 8 && at(100, 25).fit.mom_w == 0 && at(5000, 25).fit.mom_w == 16);
  CHECK(at(5000, 25).fit.mom_h && !at(600, 25).fit.mom_h);
  CHECK(at(600, 25) == at(700, 25));
  CHECK(at(4000, 25) == at(9000, 25));
  CHECK(!(at(511, 25) == at(512, 25)));    // lse_shift_min
  CHECK(!(at(3999, 25) == at(4000, 25)));  // kMom16MinK
  CHECK(at(600, 20) == at(600, 31));
  CHECK(!(at(600, 31) == at(600, 32)));      // kFuseTab: n_below + 1 = 32 | 33
  CHECK(at(600, 32) == at(600, 2047));
  CHECK(!(at(600, 2047) == at(600, 2048)));  // kTabCap
  CHECK(fit_variant(ps, sw, 5000, true, false).mom_w == 0);
  Switches w = sw;
  w.moment = false;
  CHECK(fit_variant(ps, w, 5000, false, true).mom_w == 0);
  // the moment table only for steps with a sorted draw on two-row wave tiles
  CHECK(step_reads_moments(ps, 1, (1 << 18) + 8192) && !step_reads_moments(ps, 1, 1 << 18) &&
        !step_reads_moments(ps, 1, 4096));
  StepShape a = at(600, 25), b = a;
  b.publish = true;
  CHECK(!(a == b));
  b = a;
  b.prune_mode = 2;
  CHECK(!(a == b));
}

// h. a conditional level (tests/spaces.py cond_space: a choice of 3 branches,
// each with a loguniform, a qloguniform, a choice and a normal): grids of one
// row per kind run, not three
static void case_h() {
  PlanShape ps;
  ps.hps.push_back(choice_hp(3));
  ps.levels = {{0}, {}};
  ps.lat.push_back(LatInfo{0, 0, 0, 0});
  // level 1 in the engine's order: lattice quantized, then LSE_L, LSE_G, CAT
  const int32_t R = 1028;  // rint(1024) + 2 - (rint(1) - 2) + 1
  for (int kind = 0; kind < 4; ++kind)
    for (int b = 0; b < 3; ++b) {
      tpe_hp x = kind == 0 ? quniform_hp(0, 6.931471805599453, 1)
                 : kind == 1 ? loguniform_hp(-9.210340371976182, 0)
                 : kind == 2 ? normal_hp() : choice_hp(3);
      if (kind == 0) { x.family = TPE_LGMM; x.obs_transform = TPE_OBS_LOG_CLIP_EXPLOW; }
      x.cond_begin = (int32_t)ps.cond_parent.size();
      x.cond_count = 1;
      ps.cond_parent.push_back(0);
      ps.cond_branch.push_back(b);
      ps.levels[1].push_back((int32_t)ps.hps.size());
      ps.lat.push_back(LatInfo{0, (int64_t)b * R, kind == 0 ? R : 0, 0});
      ps.hps.push_back(x);
    }
  ps.kcap = 1024;
  ps.act_frac.assign(ps.hps.size(), 1.0 / 3);
  ps.act_frac[0] = 1.0;
  ps.finish();
  const Switches sw = default_switches();
  const LevelPlan lp = plan_level(ps, sw, step(2, 4096), 1);
  CHECK(lp.compact && lp.slot_rows == 4 && lp.n_lat == 3 && lp.lat_rows == 2);
  CHECK(lp.lat == LatRun::Fused && lp.chunks.size() == 1);
  const ScoreGrid &g = lp.chunks[0].grid;
  // two log-sum-exp rows x 2 suggestions x 32 two-row tiles = 128 blocks < 3
  // per CU (768): one-row tiles.  LSE_L1, LSE_G1 (64-candidate tiles: 64),
  // LAT, CAT (2048-candidate: 2), one row each
  CHECK(g.n_groups == 4 && g.grp_kind[0] == KIND_LSE_L1 && g.grp_kind[1] == KIND_LSE_G1 &&
        g.grp_kind[2] == KIND_LAT && g.grp_kind[3] == KIND_CAT);
  CHECK(g.grp_block0[1] == 64 && g.grp_block0[2] == 128 && g.grp_block0[3] == 130 &&
        g.blocks() == 132);
  CHECK(g.pstride == 64);
  CHECK(!plan_level(ps, sw, step(1, 24), 0).compact);
}

int main() {
  case_switches();
  case_a();
  case_b();
  case_c();
  case_d();
  case_e();
  case_f();
  case_g();
  case_h();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("level plan checks passed\n");
  return 0;
}
