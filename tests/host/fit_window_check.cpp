// fit_window_check.cpp -- host-only checks of tpe_fit_window.hpp: the 32-bit
// window of the large-history sort of k_fit, its stable LSD passes over the
// window's varying bytes, and the adjacent-pair check that decides whether the
// window's permutation is the full sort's.  The reference is std::stable_sort
// on (64-bit key, position).
// Built and run by tests/test_fit_window_host.py; exit status 0: all passed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../hyperopt_amd/csrc/tpe_fit_window.hpp"

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

// sort_key of tpe_device.hpp: the order of doubles as unsigned keys
static uint64_t sort_key(double v) {
  if (v != v) return ~0ull;
  if (v == 0.0) return 0x8000000000000000ull;
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

static uint64_t vary_of(const std::vector<uint64_t> &keys) {
  uint64_t a = ~0ull, o = 0ull;
  for (uint64_t k : keys) { a &= k; o |= k; }
  return a ^ o;
}

static std::vector<uint32_t> reference(const std::vector<uint64_t> &keys) {
  std::vector<uint32_t> p(keys.size());
  for (size_t i = 0; i < p.size(); ++i) p[i] = (uint32_t)i;
  std::stable_sort(p.begin(), p.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  return p;
}

struct WindowSort {
  FitWindow w;
  int passes;
  bool proven;  // not lossy, or every adjacent pair passed the check
  int fixed;    // elements the ranking of short runs moved
  std::vector<uint32_t> perm;
};

// the device's route: window keys once per element, a stable counting pass on
// (window key, position) pairs per varying byte, the check when lossy
static WindowSort window_sort(const std::vector<uint64_t> &keys) {
  const int n = (int)keys.size();
  WindowSort r;
  r.w = fit_window(vary_of(keys));
  std::vector<uint32_t> k0(n), p0(n), k1(n), p1(n);
  for (int i = 0; i < n; ++i) { k0[i] = fit_window_key(keys[i], r.w.shift); p0[i] = (uint32_t)i; }
  const int bytes = fit_window_bytes(r.w.vary);
  r.passes = 0;
  for (int b = 0; b < 4; ++b) {
    if (!((bytes >> b) & 1)) continue;
    ++r.passes;
    int cnt[257] = {0};
    for (int i = 0; i < n; ++i) ++cnt[((k0[i] >> (8 * b)) & 255u) + 1];
    for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
    for (int i = 0; i < n; ++i) {
      const int dst = cnt[(k0[i] >> (8 * b)) & 255u]++;
      k1[dst] = k0[i];
      p1[dst] = p0[i];
    }
    k0.swap(k1);
    p0.swap(p1);
  }
  r.proven = true;
  r.fixed = 0;
  if (r.w.lossy) {
    // runs of equal window keys are ranked by their full keys
    // (fit_window_place, each element from its own view of the run)
    const auto full = [&](uint32_t p) { return keys[p]; };
    for (int e = 0; e < n; ++e) {
      const int dst = fit_window_place(e, n, [&](int i) { return k0[i]; },
                                       [&](int i) { return p0[i]; }, full);
      r.fixed += dst != e;
      p1[dst] = p0[e];
    }
    p0.swap(p1);
    for (int i = 0; i + 1 < n; ++i)
      r.proven = r.proven && fit_window_pair_sorted(k0[i], p0[i], k0[i + 1], p0[i + 1], full);
  }
  r.perm = p0;
  return r;
}

// a proven window sort is the reference's permutation; an unproven one is not
// (the caller then takes the full sort)
static WindowSort run(const std::vector<uint64_t> &keys) {
  const WindowSort r = window_sort(keys);
  const std::vector<uint32_t> ref = reference(keys);
  CHECK(r.passes <= 4);
  CHECK(r.proven == (r.perm == ref));
  // the window keeps the order of every pair it tells apart
  const uint64_t vary = vary_of(keys);
  CHECK(r.w.shift >= 0 && r.w.shift <= 63);
  CHECK(r.w.shift + 32 >= 64 || (vary >> r.w.shift >> 32) == 0);
  CHECK(r.w.lossy == ((vary & ((1ull << r.w.shift) - 1ull)) != 0));
  return r;
}

static std::vector<uint64_t> keys_of(const std::vector<double> &v) {
  std::vector<uint64_t> k(v.size());
  for (size_t i = 0; i < v.size(); ++i) k[i] = sort_key(v[i]);
  return k;
}

static const int kSizes[] = {4097, 4160, 9999, 10000};

int main() {
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> uni(-5.0, 5.0);
  for (int n : kSizes) {
    {  // distinct keys: uniform doubles, the lossy window passes its check
      std::vector<double> v(n);
      for (double &x : v) x = uni(rng);
      const WindowSort r = run(keys_of(v));
      CHECK(r.w.lossy && r.proven);
      // (-5, 5): the sign and 11 exponent bits leave the window 20 of the
      // mantissa's: some keys meet in it, out of order, and are ranked
      if (n >= 9999) CHECK(r.fixed > 0);
    }
    {  // all keys equal: no varying bit, no pass, the identity
      const WindowSort r = run(keys_of(std::vector<double>(n, 1.25)));
      CHECK(!r.w.lossy && r.passes == 0 && r.proven);
    }
    {  // ~50 distinct values: massive ties, in position order
      std::vector<double> v(n);
      for (double &x : v) x = 0.2 * std::floor(uni(rng) / 0.2 + 0.5);
      const WindowSort r = run(keys_of(v));
      CHECK(r.proven);
    }
    {  // equal inside the window, different below it, out of order: 1 + i 2^-50
      // shuffled, and one value at 1e6 that lifts the window off those bits
      std::vector<double> v(n);
      for (int i = 0; i < n; ++i) v[i] = 1.0 + std::ldexp((double)i, -50);
      std::shuffle(v.begin(), v.end() - 1, rng);
      v[n - 1] = 1e6;
      const WindowSort r = run(keys_of(v));
      CHECK(r.w.lossy && !r.proven);
    }
    {  // the same values in ascending order: the window decides nothing either,
      // but position order is the key order and the check passes
      std::vector<double> v(n);
      for (int i = 0; i < n; ++i) v[i] = 1.0 + std::ldexp((double)i, -50);
      v[n - 1] = 1e6;
      const WindowSort r = run(keys_of(v));
      CHECK(r.w.lossy && r.proven);
    }
    {  // vary narrower than 32 bits: the values share all high bits
      std::vector<double> v(n);
      for (double &x : v) x = 1.0 + std::ldexp((double)(rng() & 0xFFFFFu), -52);
      const WindowSort r = run(keys_of(v));
      CHECK(!r.w.lossy && r.passes <= 3 && r.proven);
    }
    {  // one outlier widens hb - lb past 32
      std::vector<double> v(n);
      for (double &x : v) x = 1.0 + std::ldexp((double)(rng() & 0xFFFFFu), -52);
      CHECK(!fit_window(vary_of(keys_of(v))).lossy);
      v[n / 3] = -3.0;
      const WindowSort r = run(keys_of(v));
      CHECK(r.w.lossy);
    }
    {  // raw 64-bit keys, and keys that differ in one low byte only
      std::vector<uint64_t> k(n);
      for (uint64_t &x : k) x = rng();
      CHECK(run(k).w.shift == 32);
      for (uint64_t &x : k) x = 0xABCD000000000000ull | (rng() & 0xFFu);
      const WindowSort r = run(k);
      CHECK(!r.w.lossy && r.passes == 1 && r.proven);
    }
  }
  // the window rule itself
  CHECK(fit_window(0).shift == 0 && !fit_window(0).lossy && fit_window(0).vary == 0);
  CHECK(fit_window(1ull << 63).shift == 63 && !fit_window(1ull << 63).lossy);
  CHECK(fit_window(~0ull).shift == 32 && fit_window(~0ull).lossy && fit_window(~0ull).vary == ~0u);
  CHECK(fit_window(0xFFFFFFFF0ull).shift == 4 && !fit_window(0xFFFFFFFF0ull).lossy);
  CHECK(fit_window(0x1FFFFFFFF0ull).shift == 5 && fit_window(0x1FFFFFFFF0ull).lossy);
  CHECK(fit_window_bytes(0x00FF0001u) == 5 && fit_window_bytes(0) == 0);
  if (failures) std::printf("%d check(s) failed\n", failures);
  else std::printf("fit_window_check: all passed\n");
  return failures ? 1 : 0;
}
