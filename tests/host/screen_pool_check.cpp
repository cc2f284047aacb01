// screen_pool_check.cpp -- host-only checks of tpe_screen_pool.hpp: the owner
// (wave, index) of every element of the pooled sequence of a sort block's
// eight lists, against the sequence written out list by list.
// Built and run by tests/test_screen_pool_host.py; exit status 0: all passed.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../hyperopt_amd/csrc/tpe_screen_pool.hpp"

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

constexpr int NW = 8;
constexpr int kList = 640;  // (kScreenList: a wave's list at its fullest)

// every pooled index of the lists n[NW]: the owner is the element the
// sequence "wave 0's list, then wave 1's, ..." holds there, and the rows of 64
// dealt to the waves cover each element exactly once
static void check_lists(const int (&n)[NW]) {
  std::vector<PoolSlot> seq;
  for (int w = 0; w < NW; ++w)
    for (int j = 0; j < n[w]; ++j) seq.push_back(PoolSlot{w, j});
  const int total = pool_total<NW>(n);
  CHECK(total == (int)seq.size());
  const int rows = pool_rows(total);
  CHECK(rows * 64 >= total && (rows - 1) * 64 < total);
  std::vector<int> seen((size_t)NW * kList, 0);
  for (int wv = 0; wv < NW; ++wv)       // (the kernel's loops)
    for (int r = wv; r < rows; r += NW)
      for (int lane = 0; lane < 64; ++lane) {
        const int idx = r * 64 + lane;
        if (idx >= total) continue;
        const PoolSlot o = pool_slot<NW>(n, idx);
        CHECK(o.w >= 0 && o.w < NW);
        if (o.w < 0 || o.w >= NW) continue;
        CHECK(o.j >= 0 && o.j < n[o.w]);
        if (o.j < 0 || o.j >= n[o.w]) continue;
        CHECK(o.w == seq[idx].w && o.j == seq[idx].j);
        ++seen[(size_t)o.w * kList + o.j];
      }
  for (int w = 0; w < NW; ++w)
    for (int j = 0; j < kList; ++j) CHECK(seen[(size_t)w * kList + j] == (j < n[w] ? 1 : 0));
  // (an idle lane asks for index 0 of a sequence that is not empty)
  if (total > 0) {
    const PoolSlot o = pool_slot<NW>(n, 0);
    CHECK(o.j == 0 && n[o.w] > 0);
  }
}

int main() {
  {
    const int n[NW] = {0, 0, 0, 0, 0, 0, 0, 0};  // total 0
    check_lists(n);
    CHECK(pool_rows(0) == 0);
  }
  // one wave holds everything, every wave in turn, at the totals around a row
  for (int total : {1, 63, 64, 65, kList}) {
    for (int w = 0; w < NW; ++w) {
      int n[NW] = {};
      n[w] = total;
      check_lists(n);
    }
  }
  {
    const int n[NW] = {kList, kList, kList, kList, kList, kList, kList, kList};  // 8 x 640
    check_lists(n);
    CHECK(pool_rows(NW * kList) == NW * kList / 64);
  }
  // totals of 1, 63, 64 and 65 spread over waves, with empty lists at the
  // start, inside and at the end
  {
    const int a[NW] = {0, 1, 0, 0, 0, 0, 0, 0};
    const int b[NW] = {0, 0, 30, 0, 33, 0, 0, 0};
    const int c[NW] = {32, 0, 0, 0, 0, 0, 0, 32};
    const int d[NW] = {0, 64, 0, 1, 0, 0, 0, 0};
    const int e[NW] = {1, 1, 1, 1, 1, 1, 1, 1};
    const int f[NW] = {0, 0, 0, 0, 0, 0, 0, 65};
    const int g[NW] = {63, 0, 1, 0, 0, 0, 1, 0};
    check_lists(a);
    check_lists(b);
    check_lists(c);
    check_lists(d);
    check_lists(e);
    check_lists(f);
    check_lists(g);
  }
  std::mt19937 rng(8192);
  for (int it = 0; it < 2000; ++it) {
    int n[NW];
    for (int w = 0; w < NW; ++w) {
      const unsigned r = rng();
      n[w] = (r & 3u) == 0 ? 0 : (r & 3u) == 1 ? (int)((r >> 2) % 3) : (int)((r >> 2) % (kList + 1));
    }
    check_lists(n);
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("screen pool checks passed\n");
  return 0;
}
