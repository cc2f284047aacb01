// tpe_fit_window.hpp -- the 32-bit key window of the large-history sort of
// k_fit (tpe_fit.hip) and the check that proves a sort on it exact.
// Plain C++, host and device: tests/host/fit_window_check.cpp checks both
// against std::stable_sort on the CPU.
//
// vary holds the bits in which the 64-bit sort keys of a block differ (and of
// all keys, xor or): every other bit is the same in all of them, so the order
// of two keys is the order of their varying bits.  The window is 32 of those,
// from the lowest varying bit lb, or up to the highest hb when hb - lb > 31.
// In the first case it holds every varying bit and a stable sort on it is the
// stable sort on the keys.  In the second (lossy) the bits below the window
// are dropped: keys that differ in the window are still in their order, keys
// equal in it are left in position order, which is theirs only when their
// dropped bits say so (10^4 uniform doubles on (-5, 5) keep 20 mantissa bits
// in the window and a few of them meet there: the device ranks short runs of
// equal window keys by their full keys before the check).  (key, position) is a strict total order, so a
// permutation in which every adjacent pair ascends in it is the sorted one:
// the check below, over the m - 1 pairs, decides whether the window's result
// is the full sort's, bit for bit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPE_FW_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TPE_FW_HD inline
#endif

namespace tpe {

struct FitWindow {
  int shift;      // the window is bits [shift, shift + 32) of the key
  bool lossy;     // varying bits lie below it
  uint32_t vary;  // the window's varying bits: an LSD pass per byte that has one
};

TPE_FW_HD FitWindow fit_window(uint64_t vary) {
  const int hb = 63 - __builtin_clzll(vary | 1ull), lb = vary ? __builtin_ctzll(vary) : 0;
  const int shift = lb > hb - 31 ? lb : hb - 31;
  return FitWindow{shift, shift > lb, (uint32_t)(vary >> shift)};
}

// (the bits above the window are equal in all keys: the cut keeps the order)
TPE_FW_HD uint32_t fit_window_key(uint64_t key, int shift) { return (uint32_t)(key >> shift); }

// the LSD passes of a window: bit b set <=> byte b of it varies
TPE_FW_HD int fit_window_bytes(uint32_t vary32) {
  int m = 0;
  for (int b = 0; b < 4; ++b) m |= ((vary32 >> (8 * b)) & 255u) ? 1 << b : 0;
  return m;
}

// Place e of n in a window sort's result: the place it takes once its run of
// equal window keys is ordered by (full key, position).  win(r), pos(r): the
// window key and the position at place r; full(p): the 64-bit key of position
// p.  The run is looked for up to kFitWindowRunMax places back and one more
// ahead, so every element of a run of at most that many sees all of it and is
// ranked in it; every element of a longer run sees more than that many and
// keeps its place (right when the run's keys are all equal, the ties of a
// quantized hp; the pair check fails otherwise).
constexpr int kFitWindowRunMax = 16;
template <typename Win, typename Pos, typename Full>
TPE_FW_HD int fit_window_place(int e, int n, Win win, Pos pos, Full full) {
  const uint32_t k = win(e), p = pos(e);
  int s0 = e, s1 = e + 1;
  while (s0 > 0 && e - s0 < kFitWindowRunMax && win(s0 - 1) == k) --s0;
  while (s1 < n && s1 - e <= kFitWindowRunMax && win(s1) == k) ++s1;
  if (s1 - s0 == 1 || s1 - s0 > kFitWindowRunMax) return e;
  const uint64_t kf = full(p);
  int rank = 0;
  for (int v = s0; v < s1; ++v) {
    const uint32_t pv = pos(v);
    const uint64_t kv = full(pv);
    rank += (kv < kf || (kv == kf && pv < p)) ? 1 : 0;
  }
  return s0 + rank;
}

// whether the element at a sorted place (window key wa, position pa) precedes
// its successor (wb, pb) in the (full key, position) order.  full(p): the
// 64-bit key of position p, asked for only when the window does not decide.
template <typename Full>
TPE_FW_HD bool fit_window_pair_sorted(uint32_t wa, uint32_t pa, uint32_t wb, uint32_t pb,
                                      Full full) {
  if (wa != wb) return wa < wb;
  const uint64_t ka = full(pa), kb = full(pb);
  return ka < kb || (ka == kb && pa < pb);
}

}  // namespace tpe
