// tie_plan_check.cpp -- host-only check of tpe_tie_plan.hpp: the form that
// takes k_score_wave_tie_lean and the persistent grid of the direct pass.
// Built and run by tests/test_tie_plan_host.py; exit status 0: all passed.
#include <cstdint>
#include <cstdio>

#include "../../hyperopt_amd/csrc/tpe_tie_plan.hpp"

using namespace tpe;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (failures < 20)                                             \
        std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// the arguments of a suggest's tab_on 1 launch, as far as the form reads them
static ScoreArgs suggest_args() {
  static int32_t pos[1];
  ScoreArgs a{};
  a.lse_prune = 3;
  a.lse_mom = 16;
  a.lse_pos = 1;
  a.cand_pos = pos;
  return a;
}

int main() {
  static double out[1];
  // the form: every condition on its own sends the launch to the old kernel
  CHECK(tie_lean_form(true, suggest_args()));
  CHECK(!tie_lean_form(false, suggest_args()));
  for (int prune = 0; prune <= 3; ++prune) {
    ScoreArgs a = suggest_args();
    a.lse_prune = prune;
    CHECK(tie_lean_form(true, a) == (prune == 3));
  }
  for (int mom : {0, 8, 16}) {
    ScoreArgs a = suggest_args();
    a.lse_mom = mom;
    CHECK(tie_lean_form(true, a) == (mom == 16));
  }
  { ScoreArgs a = suggest_args(); a.lse_pos = 0; CHECK(!tie_lean_form(true, a)); }
  { ScoreArgs a = suggest_args(); a.cand_pos = nullptr; CHECK(!tie_lean_form(true, a)); }
  { ScoreArgs a = suggest_args(); a.out_lb = out; CHECK(!tie_lean_form(true, a)); }
  { ScoreArgs a = suggest_args(); a.out_la = out; CHECK(!tie_lean_form(true, a)); }
  { ScoreArgs a = suggest_args(); a.l2_warm = 1; CHECK(!tie_lean_form(true, a)); }

  // the grid.  tests/test_gpu_tie_lean.py's all-hot case: 3 rows, 24
  // suggestions, 265 gathered blocks per slot -- 114 persistent blocks (three
  // iterations), 57 for the old kernel (five)
  CHECK(kNumCUs == 256 && kTieBlocksPerCu == 16 && kTieLeanBlocksPerCu == 32);
  CHECK(tie_grid(true, 3, 24, 265) == 114);
  CHECK(tie_grid(false, 3, 24, 265) == 57);
  // config 4: 100 rows, one suggestion -- ceil(8192 / 100) and ceil(4096 / 100)
  CHECK(tie_grid(true, 100, 1, 1 << 20) == 82);
  CHECK(tie_grid(false, 100, 1, 1 << 20) == 41);
  // never more than a slot has gathered blocks, never none
  CHECK(tie_grid(true, 1, 1, 265) == 265);
  CHECK(tie_grid(true, 1, 1, 1) == 1);
  CHECK(tie_grid(true, 65535, 65535, 265) == 1);
  CHECK(tie_grid(false, 65535, 65535, 265) == 1);
  // an exact quotient takes no block more: 8192 / (32 x 8) = 32
  CHECK(tie_grid(true, 32, 8, 1000) == 32);
  CHECK(tie_grid(true, 32, 8, 31) == 31);
  // every (row, suggestion) count: enough blocks to cover blocks-per-CU x CUs, one fewer would not
  for (int64_t pairs = 1; pairs <= 9000; ++pairs)
    for (int lean = 0; lean < 2; ++lean) {
      const int64_t want = (int64_t)(lean ? kTieLeanBlocksPerCu : kTieBlocksPerCu) * kNumCUs;
      const int64_t g = tie_grid(lean != 0, pairs, 1, INT32_MAX);
      CHECK(g >= 1 && g * pairs >= want && (g == 1 || (g - 1) * pairs < want));
      CHECK(tie_grid(lean != 0, 1, pairs, INT32_MAX) == g);
    }
  if (failures) std::printf("%d failures\n", failures);
  else std::printf("tie_plan_check: ok\n");
  return failures ? 1 : 0;
}
