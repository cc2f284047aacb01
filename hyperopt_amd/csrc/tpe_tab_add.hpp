// tpe_tab_add.hpp -- the scaled accumulator of the Chebyshev tables' sums
// (k_table_build): value = 2^m * s in the log2 domain, where
// nothing overflows.  Plain C++ (no builtins), host and device: tests/host/
// tab_add_skip_check.cpp runs tab_add and tab_add_skip side by side on the CPU.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPE_TAB_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TPE_TAB_HD inline
#endif

namespace tpe {

struct TabAcc {
  double m, s;  // value = 2^m * s, m integer-valued or -inf
};

TPE_TAB_HD void tab_add(TabAcc &a, double t) {
  const double mn = fmax(a.m, ceil(t));
  a.s = ldexp(a.s, (int)fmax(a.m - mn, -2100.0));
  a.m = mn;
  a.s += exp2(t - (mn == -INFINITY ? 0.0 : mn));
}

// A term 56 binades under the accumulator's exponent changes no bit of it.
// Once a.m is finite, a.s > 0.5 after every addition (the term that set a.m
// gave exp2(t - a.m) in (0.5, 1], or the rescaled sum already held one, and
// additions only grow it), so half an ulp of a.s is at least 2^-54.  With
// t - a.m < -56 (so ceil(t) <= a.m: the exponent stays, the ldexp is by 0) the
// term's exp2 is below 2^-55 whatever it rounds to (a sound exp2 is within
// a factor 2 of 2^-56), under that half ulp: the rounded sum is a.s itself.
constexpr double kTabAddSkip = -56.0;

// whether tab_add(a, t) leaves a as it is, bit for bit: a NaN term, and any
// term while a.m is -inf (or +inf), compares false
TPE_TAB_HD bool tab_add_noop(const TabAcc &a, double t) {
  return fabs(a.m) < INFINITY && t - a.m < kTabAddSkip;
}

// tab_add without the ceil / ldexp / exp2 of a term that is a no-op
TPE_TAB_HD void tab_add_skip(TabAcc &a, double t) {
  if (tab_add_noop(a, t)) return;
  tab_add(a, t);
}

}  // namespace tpe
