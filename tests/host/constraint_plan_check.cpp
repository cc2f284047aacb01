// constraint_plan_check.cpp -- the launch plan of the constrained-dominance pass
// (tpe_pareto_plan.hpp with extra_rows = 1): the grid of the plain Pareto pass,
// a staged tile of M + 1 rows within the LDS limit.  Built and run by
// tests/test_constraints_host.py; exit status 0: all checks passed.
#include <cstdio>

#include "../../hyperopt_amd/csrc/tpe_pareto_plan.hpp"

using namespace tpe;

static int failures = 0;
#define CHECK(cond) \
  do { if (!(cond)) { std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
  const int64_t ns[] = {1, 255, 256, 257, 700, 100000, kParetoMaxN};
  for (int64_t n : ns)
    for (int32_t M = 1; M <= 8; ++M)
      for (int64_t force = 0; force <= 4; ++force) {
        const ParetoPlan a = pareto_plan(n, M, force), b = pareto_plan(n, M, force, 1);
        CHECK(a.ok && b.ok);
        CHECK(b.tiles == a.tiles && b.per_split == a.per_split && b.splits == a.splits);
        CHECK(b.tiles == (n + 255) / 256 && b.splits >= 1 && b.splits <= b.tiles);
        CHECK((b.splits - 1) * b.per_split < b.tiles);  // no empty split
        CHECK(a.lds_bytes == (size_t)M * 2048);
        CHECK(b.lds_bytes == (size_t)(M + 1) * 2048 && b.lds_bytes <= kParetoLdsLimit);
      }
  CHECK(pareto_plan(700, 2, 2, 1).splits == 2 && pareto_plan(700, 2, 3, 1).splits == 3);
  CHECK(pareto_plan(257, 8, 0, 1).lds_bytes == 18432);
  CHECK(!pareto_plan(10, 9, 0, 1).ok && !pareto_plan(0, 1, 0, 1).ok);
  CHECK(!pareto_plan(10, 2, 0, 2).ok && !pareto_plan(10, 2, 0, -1).ok);
  std::printf("%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
