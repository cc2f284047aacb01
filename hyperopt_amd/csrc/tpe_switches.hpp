// tpe_switches.hpp -- the process switches of the engine, read once from the
// environment through one table (host only).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "tpe_internal.hpp"

namespace tpe {

struct Switches {
  // lookup slots drawn inside their scoring tiles (ScoreArgs::lookup_draw);
  // 0 writes them from the sorted draw instead
  bool lookup_draw;
  // a chunk's self-drawing lookup launch beside its draw on an auxiliary
  // stream; 0: in order on the suggest stream
  bool lookup_fork;
  // results to the host by k_publish + a spin on its completion word; 0: a
  // runtime copy + stream synchronize
  bool publish;
  bool tile_draw;     // tiny unsorted draws by their tiles; 0: by k_draw
  // a call whose last launch is a tile_draw scoring launch publishes from it;
  // 0: it still ends with k_publish
  bool publish_fuse;
  bool moment;        // the moment form of equal-sigma chunks in prune mode 3
  bool table;         // large draws scored from certified Chebyshev tables
  bool draw_prune;    // the sorted draw drops the wave tiles the hot intervals rule out
  bool draw_screen;   // ... and screens its candidates on (component, u1) first
  // ... on the integer uniforms, the pick from a guide table; 0: the float
  // screen (k_draw_sorted_screen with k_draw_zone's float thresholds alone)
  bool draw_screen_int;
  bool table_prefilter;  // wave tiles a certified bound rules out are not table-scored
  bool table_scalar;  // the scalar-panel table kernels; 0: the per-lane ones
  // the lean table path: per-component certificate terms once per slot and no
  // no-op additions in the build, a block-wide live-tile list in the map behind
  // the pruning draw, a one-scan gather; 0: k_table_build, k_table_map_dp and
  // k_tie_gather as they were (the same bytes everywhere)
  bool table_lean;
  // value-bucketed, pruned log-sum-exp slots on small draws: opt-in.  Measured
  // at config 2 (4096 candidates): the skip drops 80 % of the pairs and k_score
  // from 33 to 23 us, but the extra k_bucket launch costs more (70 -> 78 us)
  bool small_sort;
  // the lattice launch and a mixed level's lookup launch on auxiliary streams
  // beside the draw / the wave-tile launch; default: in order
  bool side_streams;
  // fit + suggest replayed as one captured graph: opt-in (on the measured
  // ROCm 7 / MI355X stack a replayed graph starts ~18 us after the previous
  // one, against back-to-back eager launches; tools/host_cost.py)
  bool graph;
  // the direct pass behind the tables scores a wave again when its best table
  // score is within 2^table_tie_log2 max(1, |best|) of the slot's (kTabTie; a
  // huge value makes every wave hot: tests)
  int64_t table_tie_log2;
  // the screen's zones widen a hot interval by this many pilot wave tiles per
  // side (the sweep behind the default)
  int64_t draw_screen_tiles;
  // TPE_DRAW_SCREEN_TILES is set: the whole-tile rule with that many tiles.
  // Unset, the zones widen by draw_screen_halves half tiles of 64 positions
  // per side (the sweep behind the defaults)
  bool draw_screen_whole;
  int64_t draw_screen_halves;
  // the tail zones end at the r-th smallest value of the pilot's first wave
  // tile and the r-th largest of its last; 128: the tiles' maximum and minimum
  int64_t draw_screen_tail;
  // k_draw_sorted_screen_run inverts and buckets the listed elements of a sort
  // block in dense rows dealt to its waves: opt-in (the rows it saves
  // cost less than its barrier and the owner lookup); default: every wave its
  // own list
  bool draw_screen_pool;
  // the smallest launch (candidates x suggestions x slots) the screen takes: it
  // saves ~1.4 us per 2^20 candidate-slots, k_draw_zone costs ~33 us
  int64_t draw_screen_min;
  // the integer screen's pick guide: 2^bits buckets on the top bits of u0; a
  // slot with two distinct pick boundaries in one bucket is not screened
  // (the sweep behind the default)
  int64_t draw_screen_guide_bits;
  // the integer screen by runs: a block of k_draw_sorted_screen_run draws this
  // many consecutive sort blocks of its slot and reads the slot's state once
  // (the sweep behind the default); 0: k_draw_sorted_screen_int, a
  // block per sort block
  int64_t draw_screen_run;
  // candidate buffer per scoring chunk, MB.  8 GB (+ 4 GB of positions): config
  // 4's 1e9 candidates of a level in one draw + one scoring launch, config 5's
  // 32-suggestion calls in one chunk (config 4 79.3 -> 78.8 ms, config 5 461.3
  // -> 454.4 ms per step against 2 GB, profiles/rd6/r6_46)
  int64_t chunk_mb;
  // smallest mixture (components) scored in the one-exponent form on pruned
  // tiles; smaller ones keep the per-group lift.  Round 4: 2048 -> 512 (config 5
  // 997 -> 885 ms per 1024-suggestion step, config 3 0.266 -> 0.255 ms); below
  // ~128 components the guard's second attempt costs more than the lift saves
  int64_t lse_shift_min;

  double table_tie() const { return std::ldexp(1.0, (int)table_tie_log2); }
  int64_t chunk_budget() const { return chunk_mb << 17; }  // doubles
};

constexpr int64_t kDrawScreenMin = (int64_t)1 << 26;
constexpr int64_t kDrawScreenRun = 4;
constexpr int64_t kDrawScreenHalves = 4;
constexpr int64_t kDrawScreenTail = 24;

// how a variable's text becomes the switch
enum class SwitchRule {
  OffIfZero,          // off iff set and atoi == 0 (an empty value counts as 0)
  OffIfNonEmptyZero,  // off iff set, non-empty and atoi == 0
  OnIfNonZero,        // on iff set and atoi != 0
  OnIfSet,            // on iff set at all
  OnIfNonEmpty,       // on iff set and non-empty
  ValueIfSet,         // atoll of the text if set, clamped to [lo, hi]
  ValueIfNonEmpty,    // ... if set and non-empty
};

struct SwitchDef {
  const char *name;
  SwitchRule rule;
  int64_t dflt;
  bool Switches::*flag;
  int64_t Switches::*value;
  int64_t lo, hi;
};

constexpr int64_t kTabTieLog2 = -16;
static_assert(kTabTie == 0x1p-16, "kTabTie is 2^kTabTieLog2");

inline const SwitchDef *switch_table(int *n) {
  using R = SwitchRule;
  using S = Switches;
  constexpr int64_t lo = INT64_MIN, hi = INT64_MAX;
  static const SwitchDef defs[] = {
      {"TPE_LOOKUP_DRAW", R::OffIfZero, 1, &S::lookup_draw, nullptr, 0, 0},
      {"TPE_LOOKUP_FORK", R::OffIfZero, 1, &S::lookup_fork, nullptr, 0, 0},
      {"TPE_PUBLISH", R::OffIfZero, 1, &S::publish, nullptr, 0, 0},
      {"TPE_TILE_DRAW", R::OffIfZero, 1, &S::tile_draw, nullptr, 0, 0},
      {"TPE_PUBLISH_FUSE", R::OffIfZero, 1, &S::publish_fuse, nullptr, 0, 0},
      {"TPE_MOMENT", R::OffIfZero, 1, &S::moment, nullptr, 0, 0},
      {"TPE_TABLE", R::OffIfZero, 1, &S::table, nullptr, 0, 0},
      {"TPE_DRAW_PRUNE", R::OffIfNonEmptyZero, 1, &S::draw_prune, nullptr, 0, 0},
      {"TPE_DRAW_SCREEN", R::OffIfNonEmptyZero, 1, &S::draw_screen, nullptr, 0, 0},
      {"TPE_DRAW_SCREEN_INT", R::OffIfNonEmptyZero, 1, &S::draw_screen_int, nullptr, 0, 0},
      {"TPE_TABLE_PREFILTER", R::OffIfNonEmptyZero, 1, &S::table_prefilter, nullptr, 0, 0},
      {"TPE_TABLE_SCALAR", R::OffIfNonEmptyZero, 1, &S::table_scalar, nullptr, 0, 0},
      {"TPE_TABLE_LEAN", R::OffIfNonEmptyZero, 1, &S::table_lean, nullptr, 0, 0},
      {"TPE_SMALL_SORT", R::OnIfNonZero, 0, &S::small_sort, nullptr, 0, 0},
      {"TPE_SIDE_STREAMS", R::OnIfSet, 0, &S::side_streams, nullptr, 0, 0},
      {"TPE_GRAPH", R::OnIfSet, 0, &S::graph, nullptr, 0, 0},
      {"TPE_TABLE_TIE_LOG2", R::ValueIfSet, kTabTieLog2, nullptr, &S::table_tie_log2, -1074, 4096},
      {"TPE_DRAW_SCREEN_TILES", R::ValueIfNonEmpty, 2, nullptr, &S::draw_screen_tiles, 0,
       kPilotWaves},
      {"TPE_DRAW_SCREEN_TILES", R::OnIfNonEmpty, 0, &S::draw_screen_whole, nullptr, 0, 0},
      {"TPE_DRAW_SCREEN_HALVES", R::ValueIfNonEmpty, kDrawScreenHalves, nullptr,
       &S::draw_screen_halves, 0, 2 * kPilotWaves},
      {"TPE_DRAW_SCREEN_TAIL", R::ValueIfNonEmpty, kDrawScreenTail, nullptr, &S::draw_screen_tail, 1,
       128},
      {"TPE_DRAW_SCREEN_POOL", R::OnIfNonZero, 0, &S::draw_screen_pool, nullptr, 0, 0},
      {"TPE_DRAW_SCREEN_MIN", R::ValueIfNonEmpty, kDrawScreenMin, nullptr, &S::draw_screen_min, lo,
       hi},
      {"TPE_DRAW_SCREEN_GUIDE_BITS", R::ValueIfNonEmpty, 9, nullptr, &S::draw_screen_guide_bits, 0,
       kGuideBitsMax},
      {"TPE_DRAW_SCREEN_RUN", R::ValueIfNonEmpty, kDrawScreenRun, nullptr, &S::draw_screen_run, 0,
       kScreenRunMax},
      {"TPE_CHUNK_MB", R::ValueIfSet, 8192, nullptr, &S::chunk_mb, lo, hi},
      {"TPE_SHIFT_MIN_K", R::ValueIfSet, 512, nullptr, &S::lse_shift_min, lo, hi},
  };
  *n = (int)(sizeof(defs) / sizeof(defs[0]));
  return defs;
}

// the switches of an environment (get: a variable's text, or null)
template <typename Get>
Switches read_switches(Get get) {
  Switches s{};
  int n = 0;
  const SwitchDef *defs = switch_table(&n);
  for (int i = 0; i < n; ++i) {
    const SwitchDef &d = defs[i];
    const char *e = get(d.name);
    switch (d.rule) {
      case SwitchRule::OffIfZero: s.*d.flag = !(e && std::atoi(e) == 0); break;
      case SwitchRule::OffIfNonEmptyZero: s.*d.flag = !(e && *e && std::atoi(e) == 0); break;
      case SwitchRule::OnIfNonZero: s.*d.flag = e && std::atoi(e) != 0; break;
      case SwitchRule::OnIfSet: s.*d.flag = e != nullptr; break;
      case SwitchRule::OnIfNonEmpty: s.*d.flag = e && *e; break;
      case SwitchRule::ValueIfSet:
      case SwitchRule::ValueIfNonEmpty: {
        const bool set = e && (d.rule == SwitchRule::ValueIfSet || *e);
        const int64_t v = set ? (int64_t)std::atoll(e) : d.dflt;
        s.*d.value = v < d.lo ? d.lo : v > d.hi ? d.hi : v;
        break;
      }
    }
  }
  return s;
}

// this process's switches (read at the first call)
inline const Switches &switches() {
  static const Switches s = read_switches([](const char *name) { return std::getenv(name); });
  return s;
}

}  // namespace tpe
