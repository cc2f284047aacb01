// tpe_screen_pool.hpp -- the pooled rows of k_draw_sorted_screen_run (DESIGN
// 5.6): the lists of a sort block's waves taken as one sequence, wave 0's
// first, and the owner of an element of that sequence.  Plain C++ (no
// builtins), host and device: tests/host/screen_pool_check.cpp checks it on
// the CPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPE_POOL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TPE_POOL_HD inline
#endif

namespace tpe {

struct PoolSlot { int w, j; };  // element j of wave w's list

// the pooled sequence's length
template <int NW>
TPE_POOL_HD int pool_total(const int *n) {
  int sum = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) sum += n[q];
  return sum;
}

// The owner of pooled index idx, 0 <= idx < pool_total(n), n[q] >= 0 the
// length of wave q's list: the last wave whose first pooled index is at most
// idx -- the empty waves before it share that index and are passed over.
template <int NW>
TPE_POOL_HD PoolSlot pool_slot(const int *n, int idx) {
  int w = 0, first = 0, run = 0;
#pragma unroll
  for (int q = 0; q + 1 < NW; ++q) {
    run += n[q];
    const bool past = idx >= run;
    w = past ? q + 1 : w;
    first = past ? run : first;
  }
  return PoolSlot{w, idx - first};
}

// the rows of 64 the pooled sequence takes
TPE_POOL_HD int pool_rows(int total) { return (total + 63) >> 6; }

}  // namespace tpe
