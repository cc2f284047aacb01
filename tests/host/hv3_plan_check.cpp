// hv3_plan_check.cpp -- host-only checks of method code 3 (exact gains, three
// objectives) in the launch plan of the hypervolume subset selection
// (tpe_hv_plan.hpp).  Built and run by tests/test_hv_exact3_host.py; exit
// status 0: all checks passed.
#include <cstdio>

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

static_assert(kHvExact3 == 3, "the method code of the header");
static_assert(kHv3LdsBytes == 256 * 48 && kHv3LdsBytes <= 64 * 1024, "the staged picks");

int main() {
  const int64_t ns[] = {1, 257, 65836, kParetoMaxN};
  for (int64_t n : ns) {
    const HvPlan p = hv_plan(n, 3, 256, 1024, 3);
    CHECK(p.ok && p.exact && p.tiles == (n + 255) / 256 && p.words == 1);
    CHECK(p.lds_bytes == 0 && p.u_doubles == 0 && p.alive_words(n) == 0);
  }
  CHECK(!hv_plan(10, 2, 32, 1024, 3).ok);
  CHECK(!hv_plan(10, 4, 32, 1024, 3).ok);
  CHECK(!hv_plan(10, 3, 257, 1024, 3).ok);
  CHECK(!hv_plan(10, 3, 32, 1024, 4).ok);
  CHECK(hv_plan(10, 3, 32, 1024, 0).ok && !hv_plan(10, 3, 32, 1024, 0).exact);  // auto: Monte-Carlo
  if (failures) return 1;
  std::printf("hv3 plan checks passed\n");
  return 0;
}
