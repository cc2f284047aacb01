// tpe_pareto_plan.hpp -- the launch of the Pareto ranking pass, as data.
// Pure host code: pareto_plan maps (n, M) -- history rows and objectives -- to
// the grid of k_pareto_count (tpe_pareto.hip): tiles of rows i, contiguous
// runs of j tiles per j-split, and the LDS a block stages a j tile in
// (DESIGN 5.17).  The counts are a function of Y alone; the plan only decides
// how the pairs are spread over blocks.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace tpe {

constexpr int kParetoTile = 256;     // rows per tile: one row per lane of a block
constexpr int kParetoMaxObj = 8;     // TPE_MAX_OBJ
// the largest history: s = dominated_by (n + 1) + (n - dominates) is an exact
// integer in a double while (n + 1)^2 < 2^53
constexpr int64_t kParetoMaxN = 94906264;
static_assert((kParetoMaxN + 1) * (kParetoMaxN + 1) < ((int64_t)1 << 53), "s is exact");
static_assert((kParetoMaxN + 2) * (kParetoMaxN + 2) >= ((int64_t)1 << 53), "the largest such n");
constexpr int64_t kParetoBlocks = 1024;      // blocks worth launching: 256 CUs x 4
constexpr int64_t kParetoMaxSplits = 65535;  // grid.y
constexpr size_t kParetoLdsLimit = 64 * 1024;

struct ParetoPlan {
  bool ok = false;        // (n, M) is in range
  int64_t n = 0;
  int32_t M = 0;
  int64_t tiles = 0;      // ceil(n / tile): tiles of rows i (grid.x) and of rows j
  int64_t per_split = 0;  // j tiles a block walks
  int64_t splits = 0;     // grid.y: ceil(tiles / per_split), none empty
  size_t lds_bytes = 0;   // the staged j tile, [M][tile] doubles

  // rows [begin, end) of tile t
  int64_t tile_begin(int64_t t) const { return t * kParetoTile; }
  int64_t tile_end(int64_t t) const { return std::min<int64_t>(n, (t + 1) * kParetoTile); }
  // j tiles [begin, end) of split s
  int64_t split_begin(int64_t s) const { return s * per_split; }
  int64_t split_end(int64_t s) const { return std::min<int64_t>(tiles, (s + 1) * per_split); }
};

// force_splits > 0: that many j-splits where the history has the tiles for it
// (tests); 0: enough to fill the machine.  Whatever is asked for, the result
// has no empty split: splits = ceil(tiles / per_split).
inline ParetoPlan pareto_plan(int64_t n, int32_t M, int64_t force_splits = 0) {
  ParetoPlan p;
  if (n < 1 || n > kParetoMaxN || M < 1 || M > kParetoMaxObj) return p;
  p.n = n;
  p.M = M;
  p.tiles = (n + kParetoTile - 1) / kParetoTile;
  int64_t want = force_splits > 0 ? force_splits : (kParetoBlocks + p.tiles - 1) / p.tiles;
  want = std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(p.tiles, kParetoMaxSplits)));
  p.per_split = (p.tiles + want - 1) / want;
  p.splits = (p.tiles + p.per_split - 1) / p.per_split;
  p.lds_bytes = (size_t)M * kParetoTile * sizeof(double);
  p.ok = p.lds_bytes <= kParetoLdsLimit;
  return p;
}

}  // namespace tpe
