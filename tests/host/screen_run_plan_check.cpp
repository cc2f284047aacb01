// screen_run_plan_check.cpp -- host-only check that TPE_DRAW_SCREEN_RUN reaches
// the launch plan: the switch table reads it (default, clamp, empty), the
// chunk of a screened draw carries it as screen_run, and two steps that differ
// in it have different captured-graph keys.  Expected values are written out
// from the documented rules.
// Built and run by tests/test_screen_run_plan.py; exit status 0: all passed.
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

static_assert(kScreenRunMax == 16, "the cap the cases use");

struct Env { const char *name, *text; };
static Switches with(const Env *env, int n) {
  return read_switches([&](const char *name) -> const char * {
    for (int i = 0; i < n; ++i)
      if (!std::strcmp(env[i].name, name)) return env[i].text;
    return nullptr;
  });
}
static Switches run_env(const char *text) {
  const Env e[] = {{"TPE_DRAW_SCREEN_RUN", text}, {"TPE_DRAW_SCREEN_MIN", "0"}};
  return with(e, 2);
}

// sixteen bounded uniform hps at 2^18 + 8192 candidates with the 16-wide
// moment tables: the screened draw (level_plan_check.cpp, case b)
static PlanShape uniform16() {
  tpe_hp x{};
  x.family = TPE_GMM;
  x.flags = TPE_HAS_LOW | TPE_HAS_HIGH;
  x.prior_sigma = 10;
  x.low = -5;
  x.high = 5;
  PlanShape ps;
  ps.hps.assign(16, x);
  ps.levels.assign(1, {});
  for (int i = 0; i < 16; ++i) {
    ps.levels[0].push_back(i);
    ps.lat.push_back(LatInfo{0, 0, 0, 0});
  }
  ps.kcap = 1024;
  ps.act_frac.assign(16, 1.0);
  ps.finish();
  return ps;
}
static StepShape step_under(const Switches &sw) {
  StepShape s;
  s.n_sug = 1;
  s.n_cand = s.n_total = (1 << 18) + 8192;
  s.below = BELOW_FUSE;
  s.fit.mom_w = 16;
  s.fit.mom_h = true;
  s.capturing = true;
  s.screen_run = step_screen_run(sw);
  return s;
}

int main() {
  const Switches d = with(nullptr, 0);
  CHECK(d.draw_screen_run == kDrawScreenRun && kDrawScreenRun >= 0 && kDrawScreenRun <= 16);
  CHECK(run_env("3").draw_screen_run == 3 && run_env("0").draw_screen_run == 0);
  CHECK(run_env("99").draw_screen_run == 16 && run_env("-4").draw_screen_run == 0);
  CHECK(run_env("").draw_screen_run == kDrawScreenRun);  // empty: the default

  const PlanShape ps = uniform16();
  for (int r : {0, 1, 3, 16}) {
    char text[8];
    std::snprintf(text, sizeof text, "%d", r);
    const Switches sw = run_env(text);
    const StepShape s = step_under(sw);
    CHECK(s.screen_run == r);
    const LevelPlan lp = plan_level(ps, sw, s, 0);
    CHECK(lp.chunks.size() == 1);
    const ChunkPlan &c = lp.chunks[0];
    CHECK(c.draw == Draw::SortedScreened && c.screen_guide == 9 && c.screen_run == r);
  }
  // two steps that differ in the run length alone: different graph keys
  const StepShape a = step_under(run_env("0")), b = step_under(run_env("3"));
  CHECK(!(a == b) && a == step_under(run_env("0")) && b == step_under(run_env("3")));
  StepShape b0 = b;
  b0.screen_run = 0;
  CHECK(a == b0);
  {
    // the float screen has no runs: nothing in the key, nothing in the chunk
    const Env e[] = {{"TPE_DRAW_SCREEN_RUN", "3"}, {"TPE_DRAW_SCREEN_MIN", "0"},
                     {"TPE_DRAW_SCREEN_INT", "0"}};
    const Switches sw = with(e, 3);
    const StepShape s = step_under(sw);
    CHECK(s.screen_run == 0 && s == a);
    const ChunkPlan c = plan_level(ps, sw, s, 0).chunks[0];
    CHECK(c.draw == Draw::SortedScreened && c.screen_guide == -1 && c.screen_run == 0);
  }
  {
    // without the screen the pruning draw runs: no run length either
    const Env e[] = {{"TPE_DRAW_SCREEN_RUN", "3"}, {"TPE_DRAW_SCREEN_MIN", "0"},
                     {"TPE_DRAW_SCREEN", "0"}};
    const Switches sw = with(e, 3);
    const StepShape s = step_under(sw);
    CHECK(s.screen_run == 0);
    const ChunkPlan c = plan_level(ps, sw, s, 0).chunks[0];
    CHECK(c.draw == Draw::SortedPruned && c.screen_run == 0);
  }
  {
    // below the screen's smallest launch (the default 2^26 candidate-slots)
    const Env e[] = {{"TPE_DRAW_SCREEN_RUN", "3"}};
    const Switches sw = with(e, 1);
    const ChunkPlan c = plan_level(ps, sw, step_under(sw), 0).chunks[0];
    CHECK(c.draw == Draw::SortedPruned && c.screen_run == 0);
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("screen run plan checks passed\n");
  return 0;
}
