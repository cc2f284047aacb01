// tab_add_skip_check.cpp -- host-only check of tpe_tab_add.hpp: tab_add_skip,
// which leaves out the ceil / ldexp / exp2 of a term 56 binades under the
// accumulator's exponent, against tab_add.  Fed the same sequence the two
// leave the same (m, s) bits after every term.
// Built and run by tests/test_tab_add_skip_host.py; exit status 0: all passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../hyperopt_amd/csrc/tpe_tab_add.hpp"

using namespace tpe;

static int failures = 0;
static long skipped = 0, added = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (failures < 20)                                             \
        std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}
static bool same(const TabAcc &a, const TabAcc &b) {
  return bits(a.m) == bits(b.m) && bits(a.s) == bits(b.s);
}

// both forms over one sequence, compared after every term (and before any)
static void run(const std::vector<double> &seq, const char *what) {
  TabAcc full{-INFINITY, 0.0}, lean{-INFINITY, 0.0};
  CHECK(same(full, lean));
  for (size_t i = 0; i < seq.size(); ++i) {
    if (tab_add_noop(lean, seq[i])) ++skipped; else ++added;
    tab_add(full, seq[i]);
    tab_add_skip(lean, seq[i]);
    if (!same(full, lean)) {
      if (failures < 20)
        std::printf("%s: term %zu (%a): full (%a, %a) lean (%a, %a)\n", what, i, seq[i], full.m,
                    full.s, lean.m, lean.s);
      ++failures;
      return;
    }
    // the invariant the skip rests on
    if (std::isfinite(full.m) && full.s == full.s) CHECK(full.s > 0.5);
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> wide(-3000.0, 1100.0), near(-80.0, 10.0), unit(0.0, 1.0);

  run({}, "empty");
  run({-12.75}, "single");
  run({-inf}, "single -inf");
  run({nan}, "single NaN");

  // random terms: over the whole log2 range, and within reach of the limit
  for (int rep = 0; rep < 200; ++rep) {
    std::vector<double> s;
    const int n = 1 + (int)(rng() % 400);
    for (int i = 0; i < n; ++i) s.push_back(rep & 1 ? near(rng) : wide(rng));
    run(s, "random");
  }
  // many equal terms: s grows far past 1
  run(std::vector<double>(5000, -3.25), "equal");

  // terms on either side of the limit, by one ulp and by 1, against integer
  // and non-integer leaders
  for (double lead : {0.0, -0.5, 7.0, 6.000000001, -1022.0, 900.25}) {
    const double m = std::ceil(lead);
    for (double off : {-57.0, -56.0, -55.0}) {
      const double t = m + off;
      for (double v : {std::nextafter(t, -inf), t, std::nextafter(t, inf), t - 1.0, t + 1.0}) {
        run({lead, v}, "limit");
        run({lead, lead, lead, v, v, v}, "limit, s > 1");
      }
    }
  }
  // a new maximum behind a run of skipped terms, then terms that the old
  // exponent kept and the new one skips
  for (int rep = 0; rep < 50; ++rep) {
    std::vector<double> s{10.0 * unit(rng)};
    for (int i = 0; i < 100; ++i) s.push_back(-60.0 - 500.0 * unit(rng));
    s.push_back(40.0 + 100.0 * unit(rng));
    for (int i = 0; i < 100; ++i) s.push_back(-60.0 * unit(rng));
    s.push_back(2000.0);
    for (int i = 0; i < 20; ++i) s.push_back(1900.0 + 100.0 * unit(rng));
    run(s, "new maximum");
  }
  // -inf first (a zero prior weight), -inf throughout
  {
    std::vector<double> s{-inf};
    for (int i = 0; i < 300; ++i) s.push_back(near(rng) - 60.0 * (i % 3));
    run(s, "-inf first");
    run(std::vector<double>(64, -inf), "-inf throughout");
    run({-inf, -inf, -70.0, -inf, -200.0, -inf}, "-inf between");
  }
  // a NaN in the middle: it takes the full path, and so does what follows in
  // bits (NaN stays NaN either way)
  {
    std::vector<double> s;
    for (int i = 0; i < 100; ++i) s.push_back(near(rng));
    s.push_back(nan);
    for (int i = 0; i < 100; ++i) s.push_back(near(rng) - 100.0 * (i & 1));
    run(s, "NaN in the middle");
    run({nan, -3.0, -300.0}, "NaN first");
  }
  // +inf: the accumulator's exponent is no longer finite, nothing is skipped
  run({-5.0, inf, -100.0, -1e300}, "+inf");

  CHECK(skipped > 1000 && added > 1000);  // (both paths were taken)
  if (failures) {
    std::printf("tab_add_skip_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("tab_add_skip_check: ok (%ld terms skipped, %ld added)\n", skipped, added);
  return 0;
}
