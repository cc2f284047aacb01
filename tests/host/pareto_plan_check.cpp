// pareto_plan_check.cpp -- host-only checks of the launch plan of the Pareto
// ranking pass (tpe_pareto_plan.hpp): for every (n, M, forced j-splits) case
// the tiles of rows i cover [0, n) exactly once, the j-splits cover the j tiles
// exactly once with no empty split, the grid and the LDS stay within their
// limits, and out-of-range arguments are refused.  The expected values are
// written from the documented rules, not computed by the code under test.
// Built and run by tests/test_pareto_host.py; exit status 0: all checks passed.
#include <cstdio>
#include <vector>

#include "../../hyperopt_amd/csrc/tpe_pareto_plan.hpp"

using namespace tpe;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static_assert(kParetoTile == 256 && kParetoMaxObj == 8, "constants the cases use");
static_assert(kParetoLdsLimit == 65536, "constants the cases use");

// every row of [0, n) lies in exactly one tile, every tile in exactly one split
static void covers(int64_t n, int32_t M, int64_t force) {
  const ParetoPlan p = pareto_plan(n, M, force);
  CHECK(p.ok);
  if (!p.ok) return;
  CHECK(p.n == n && p.M == M);
  CHECK(p.tiles == (n + 255) / 256);
  CHECK(p.lds_bytes == (size_t)M * 256 * 8 && p.lds_bytes <= kParetoLdsLimit);
  CHECK(p.splits >= 1 && p.splits <= p.tiles && p.splits <= kParetoMaxSplits);
  CHECK(p.per_split >= 1);
  // rows: walk the tiles in order; each starts where the last one ended
  int64_t row = 0;
  bool tiles_ok = true;
  for (int64_t t = 0; t < p.tiles; ++t) {
    tiles_ok = tiles_ok && p.tile_begin(t) == row && p.tile_end(t) > p.tile_begin(t) &&
               p.tile_end(t) - p.tile_begin(t) <= 256;
    row = p.tile_end(t);
  }
  CHECK(tiles_ok);
  CHECK(row == n);
  // j tiles: the same over the splits, none empty
  int64_t tile = 0;
  bool splits_ok = true;
  for (int64_t s = 0; s < p.splits; ++s) {
    splits_ok = splits_ok && p.split_begin(s) == tile && p.split_end(s) > p.split_begin(s) &&
                p.split_end(s) - p.split_begin(s) <= p.per_split;
    tile = p.split_end(s);
  }
  CHECK(splits_ok);
  CHECK(tile == p.tiles);
}

static void small_sizes() {
  const int64_t ns[] = {1, 2, 255, 256, 257, 513, 1000, 10000, 100000};
  for (int64_t n : ns)
    for (int32_t M = 1; M <= 8; ++M) {
      covers(n, M, 0);
      const int64_t tiles = (n + 255) / 256;
      for (int64_t f = 1; f <= tiles && f <= 48; ++f) covers(n, M, f);
      covers(n, M, tiles + 7);  // more than the tiles: clamped
    }
}

static void written_out() {
  // one tile: one block, whatever is forced
  ParetoPlan p = pareto_plan(256, 2, 5);
  CHECK(p.ok && p.tiles == 1 && p.splits == 1 && p.per_split == 1 && p.lds_bytes == 4096);
  p = pareto_plan(257, 8);
  CHECK(p.ok && p.tiles == 2 && p.splits == 2 && p.per_split == 1 && p.lds_bytes == 16384);
  CHECK(p.tile_end(0) == 256 && p.tile_begin(1) == 256 && p.tile_end(1) == 257);
  // 1e4 rows: 40 tiles; ceil(1024 / 40) = 26 splits wanted, 2 tiles each -> 20 splits
  p = pareto_plan(10000, 2);
  CHECK(p.ok && p.tiles == 40 && p.per_split == 2 && p.splits == 20);
  CHECK(p.tiles * p.splits >= 512);  // the machine is filled: 2 blocks per CU and more
  // 1e5 rows: 391 tiles; ceil(1024 / 391) = 3 splits wanted, 131 tiles each
  p = pareto_plan(100000, 4);
  CHECK(p.ok && p.tiles == 391 && p.per_split == 131 && p.splits == 3);
  // forced: 4 tiles in 3 splits are 2 + 2: the plan rounds to 2 splits
  p = pareto_plan(1000, 3, 3);
  CHECK(p.ok && p.tiles == 4 && p.per_split == 2 && p.splits == 2);
  p = pareto_plan(1000, 3, 4);
  CHECK(p.ok && p.per_split == 1 && p.splits == 4);
}

static void largest() {
  // the largest n with (n + 1)^2 < 2^53
  const int64_t n = 94906264;
  CHECK(kParetoMaxN == n);
  CHECK((n + 1) * (n + 1) < ((int64_t)1 << 53));
  CHECK((n + 2) * (n + 2) >= ((int64_t)1 << 53));
  for (int32_t M = 1; M <= 8; M += 7) {
    covers(n, M, 0);
    covers(n, M, 65535);
    covers(n, M, 1 << 20);  // clamped to the grid's second dimension
  }
  const ParetoPlan p = pareto_plan(n, 8);
  CHECK(p.ok && p.tiles == 370728 && p.splits == 1);
  CHECK(!pareto_plan(n + 1, 1).ok);
}

static void refused() {
  CHECK(!pareto_plan(0, 1).ok);
  CHECK(!pareto_plan(-1, 1).ok);
  CHECK(!pareto_plan(10, 0).ok);
  CHECK(!pareto_plan(10, 9).ok);
  CHECK(!pareto_plan(10, -1).ok);
}

int main() {
  small_sizes();
  written_out();
  largest();
  refused();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("pareto plan checks passed\n");
  return 0;
}
