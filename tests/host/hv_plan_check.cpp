// hv_plan_check.cpp -- host-only checks of the launch plan of the hypervolume
// subset selection (tpe_hv_plan.hpp): for every (n, M, n_pick, S, method) case
// the row tiles cover [0, n) exactly once, the sample words cover [0, S)
// exactly once, the sample table is indexed without a gap or an overlap, the
// staged uniforms stay within the LDS limit, the buffer sizes are the
// documented ones, and out-of-range arguments are refused.  The expected
// values are written from the documented rules, not computed by the code
// under test.  Built and run by tests/test_hv_host.py; exit status 0: all
// checks passed.
#include <cstdio>
#include <vector>

#include "../../hyperopt_amd/csrc/tpe_hv_plan.hpp"

using namespace tpe;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static_assert(kHvTile == 256 && kHvWord == 64 && kHvMaxPick == 256, "constants the cases use");
static_assert(kHvMinSamples == 64 && kHvMaxSamples == 4096, "constants the cases use");
static_assert(kHvLdsLimit == 4096 && kHvStream == 0x60000000u, "constants the cases use");
static_assert(kHvAuto == 0 && kHvExact == 1 && kHvMc == 2, "the method codes of the header");

static void covers(int64_t n, int32_t M, int32_t n_pick, int32_t S, int32_t method) {
  const HvPlan p = hv_plan(n, M, n_pick, S, method);
  CHECK(p.ok);
  if (!p.ok) return;
  const bool exact = method == 1 || (method == 0 && M == 2);
  CHECK(p.n == n && p.M == M && p.n_pick == n_pick && p.S == S && p.exact == exact);
  CHECK(p.tiles == (n + 255) / 256);
  CHECK(p.words == (exact ? 1 : S / 64));
  CHECK(p.words >= 1 && p.words <= 64);  // grid.y
  CHECK(p.lds_bytes == (exact ? 0u : (size_t)M * 64 * 8) && p.lds_bytes <= kHvLdsLimit);
  CHECK(p.u_doubles == (exact ? 0u : (size_t)S * M));
  CHECK(p.alive_words(n) == (exact ? 0u : (size_t)(S / 64) * (size_t)n));
  CHECK(p.alive_words(n + 100) == (exact ? 0u : (size_t)(S / 64) * (size_t)(n + 100)));
  // at most S / 8 bytes of alive words per row
  CHECK(p.alive_words(n) * 8 <= (size_t)n * (size_t)(S / 8));
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
  if (exact) return;
  // samples: the words in order, 64 each
  int64_t s = 0;
  bool words_ok = true;
  for (int64_t w = 0; w < p.words; ++w) {
    words_ok = words_ok && p.word_begin(w) == s && p.word_end(w) - p.word_begin(w) == 64;
    s = p.word_end(w);
  }
  CHECK(words_ok);
  CHECK(s == S);
  // the table: every (s, m) has a slot of its own inside [0, S M), and a
  // word's uniforms are one contiguous run of 64 M doubles
  std::vector<char> hit(p.u_doubles, 0);
  bool table_ok = true;
  for (int64_t k = 0; k < S; ++k)
    for (int32_t m = 0; m < M; ++m) {
      const size_t at = p.u_index(k, m);
      table_ok = table_ok && at < p.u_doubles && !hit[at];
      if (at < p.u_doubles) hit[at] = 1;
      table_ok = table_ok && at / ((size_t)64 * M) == (size_t)(k / 64);
    }
  CHECK(table_ok);
}

static void sizes() {
  const int64_t ns[] = {1, 2, 63, 64, 65, 255, 256, 257, 600, 1000, 100000};
  const int32_t Ss[] = {64, 128, 1024, 4096};
  const int32_t picks[] = {1, 5, 32, 256};
  for (int64_t n : ns)
    for (int32_t M = 2; M <= 8; ++M)
      for (int32_t S : Ss)
        for (int32_t k : picks) {
          covers(n, M, k, S, 0);
          covers(n, M, k, S, 2);
          if (M == 2) covers(n, M, k, S, 1);
        }
}

static void written_out() {
  HvPlan p = hv_plan(600, 2, 32, 1024, 0);  // two objectives: exact
  CHECK(p.ok && p.exact && p.tiles == 3 && p.words == 1 && p.lds_bytes == 0 && p.u_doubles == 0);
  CHECK(p.tile_end(2) == 600);
  p = hv_plan(600, 2, 32, 1024, 2);  // forced Monte-Carlo
  CHECK(p.ok && !p.exact && p.words == 16 && p.lds_bytes == 1024 && p.u_doubles == 2048);
  CHECK(p.alive_words(1024) == 16 * 1024);
  p = hv_plan(257, 8, 5, 4096, 0);
  CHECK(p.ok && !p.exact && p.tiles == 2 && p.words == 64 && p.lds_bytes == 4096);
  CHECK(p.u_index(0, 0) == 0 && p.u_index(1, 0) == 1 && p.u_index(0, 1) == 64);
  CHECK(p.u_index(64, 0) == 512 && p.u_index(65, 7) == 512 + 7 * 64 + 1);
  // the largest history the ranking takes
  p = hv_plan(kParetoMaxN, 8, 256, 4096, 0);
  CHECK(p.ok && p.tiles == 370728);
  covers(kParetoMaxN, 3, 32, 64, 0);
}

static void refused() {
  CHECK(!hv_plan(0, 2, 32, 1024, 0).ok);
  CHECK(!hv_plan(-1, 2, 32, 1024, 0).ok);
  CHECK(!hv_plan(kParetoMaxN + 1, 2, 32, 1024, 0).ok);
  CHECK(!hv_plan(10, 1, 32, 1024, 0).ok);  // one objective: a total order, nothing to select
  CHECK(!hv_plan(10, 9, 32, 1024, 0).ok);
  CHECK(!hv_plan(10, 2, 0, 1024, 0).ok);
  CHECK(!hv_plan(10, 2, 257, 1024, 0).ok);
  CHECK(!hv_plan(10, 2, 32, 0, 0).ok);
  CHECK(!hv_plan(10, 2, 32, 32, 0).ok);
  CHECK(!hv_plan(10, 2, 32, 100, 0).ok);   // not a multiple of 64
  CHECK(!hv_plan(10, 2, 32, 4160, 0).ok);
  CHECK(!hv_plan(10, 2, 32, 1024, 3).ok);
  CHECK(!hv_plan(10, 2, 32, 1024, -1).ok);
  CHECK(!hv_plan(10, 3, 32, 1024, 1).ok);  // exact needs two objectives
  CHECK(hv_plan(10, 2, 32, 1024, 1).ok);
}

int main() {
  sizes();
  written_out();
  refused();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("hv plan checks passed\n");
  return 0;
}
