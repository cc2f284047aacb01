// tpe_topk.hip -- the k best of M totals on the device, and the gather of the
// picked configurations, gfx950 (tpe_plan_topk_points, tpe_plan_gather_points).
//
// The rule is tpe.rank_pool's: among the eligible entries the highest total
// first, ties to the lower index, -0.0 == +0.0, NaN last (by index).  Every
// entry gets a 96-bit composite (key, ~index): key is the total's bits mapped
// so that unsigned order is the ranking order (NaN 0, then -inf .. -0 = +0 ..
// +inf), and no two composites are equal.  A radix select walks the composite
// from its top byte, 12 passes of 8 bits: each pass counts, over the entries
// that match the digits chosen so far, the 256 values of the next digit
// (integer atomics on an LDS histogram, then on the global one), and the next
// launch picks the digit that holds the k-th largest.  After the last pass the
// prefix is the k-th composite itself; one launch collects the k entries at
// or above it (in arrival order) and one block sorts them (bitonic, in LDS).
// Counts are integers and the composites are distinct, so the result is the
// same for every launch shape; there is no floating-point atomic.
#include <math.h>

#include <algorithm>
#include <cstddef>

#include "tpe_device.hpp"

namespace tpe {

constexpr int kTkThreads = 256;
constexpr int kTkMaxBlocks = 1024;
constexpr int kTkSortThreads = 1024;

struct TopkState {
  uint64_t pk;    // the key digits chosen so far (top bytes)
  uint32_t pi;    // ... and those of ~index
  uint32_t need;  // entries still to take among the prefix's matches
};
struct TopkScratch {
  uint32_t hist[kTopkPasses][256];
  TopkState st[kTopkPasses + 1];  // st[p]: before pass p
  uint32_t taken;                 // the collect's cursor
  uint32_t pad[3];
  uint64_t key[kTopkMax];
  uint32_t nidx[kTopkMax];
};

// (topk_key: tpe_device.hpp)
__device__ __forceinline__ uint32_t topk_digit(uint64_t key, uint32_t nidx, int pass) {
  return pass < 8 ? (uint32_t)(key >> (56 - 8 * pass)) & 255u
                  : (nidx >> (24 - 8 * (pass - 8))) & 255u;
}
// the entry carries the first `pass` digits of the state
__device__ __forceinline__ bool topk_match(uint64_t key, uint32_t nidx, const TopkState &s,
                                           int pass) {
  if (pass == 0) return true;
  if (pass < 8) return (key >> (64 - 8 * pass)) == (s.pk >> (64 - 8 * pass));
  if (key != s.pk) return false;
  return pass == 8 || (nidx >> (32 - 8 * (pass - 8))) == (s.pi >> (32 - 8 * (pass - 8)));
}

// st[pass] from st[pass - 1] and the histogram of pass - 1: the digit d with
// (entries of larger digits) < need <= (those plus its own); every thread of
// a 256-thread block calls it.  k: the call's k (pass 0).
__device__ __forceinline__ TopkState topk_advance(const TopkScratch *W, int pass, int32_t k,
                                                  TopkState *sh, uint32_t *wtot) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (pass == 0) return TopkState{0ull, 0u, (uint32_t)k};
  const TopkState prev = W->st[pass - 1];
  const int d = 255 - t;  // thread order = descending digit
  const uint32_t cnt = W->hist[pass - 1][d];
  uint32_t v = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  if (lane == 63) wtot[wv] = v;
  if (t == 0) *sh = TopkState{prev.pk, prev.pi, 0u};  // (fewer than need: nothing more to take)
  __syncthreads();
  for (int w = 0; w < wv; ++w) v += wtot[w];
  const uint32_t excl = v - cnt;
  if (excl < prev.need && prev.need <= v) {
    TopkState s = prev;
    const int q = pass - 1;
    if (q < 8) s.pk |= (uint64_t)d << (56 - 8 * q);
    else s.pi |= (uint32_t)d << (24 - 8 * (q - 8));
    s.need = prev.need - excl;
    *sh = s;
  }
  __syncthreads();
  return *sh;
}

__global__ __launch_bounds__(kTkThreads) void k_topk_hist(const double *__restrict__ total,
                                                          const uint8_t *__restrict__ eligible,
                                                          int64_t m, int32_t k, int pass,
                                                          TopkScratch *W) {
  __shared__ uint32_t h[256];
  __shared__ TopkState sh;
  __shared__ uint32_t wtot[4];
  h[threadIdx.x] = 0u;
  const TopkState s = topk_advance(W, pass, k, &sh, wtot);
  if (blockIdx.x == 0 && threadIdx.x == 0) W->st[pass] = s;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kTkThreads + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * kTkThreads) {
    if (eligible && !eligible[i]) continue;
    const uint64_t key = topk_key(total[i]);
    const uint32_t nidx = ~(uint32_t)i;
    if (topk_match(key, nidx, s, pass)) atomicAdd(&h[topk_digit(key, nidx, pass)], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&W->hist[pass][threadIdx.x], h[threadIdx.x]);
}

// the entries at or above the k-th composite, in arrival order
__global__ __launch_bounds__(kTkThreads) void k_topk_collect(const double *__restrict__ total,
                                                             const uint8_t *__restrict__ eligible,
                                                             int64_t m, int32_t k,
                                                             TopkScratch *W) {
  __shared__ TopkState sh;
  __shared__ uint32_t wtot[4];
  const TopkState s = topk_advance(W, kTopkPasses, k, &sh, wtot);
  for (int64_t i = (int64_t)blockIdx.x * kTkThreads + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * kTkThreads) {
    if (eligible && !eligible[i]) continue;
    const uint64_t key = topk_key(total[i]);
    const uint32_t nidx = ~(uint32_t)i;
    if (key > s.pk || (key == s.pk && nidx >= s.pi)) {
      const uint32_t pos = atomicAdd(&W->taken, 1u);
      if (pos < (uint32_t)k) {  // (exactly k qualify: the composites are distinct)
        W->key[pos] = key;
        W->nidx[pos] = nidx;
      }
    }
  }
}

// one block: the k collected composites in descending order, as indices
__global__ __launch_bounds__(kTkSortThreads) void k_topk_sort(int32_t k, TopkScratch *W,
                                                              int32_t *__restrict__ idx) {
  __shared__ uint64_t key[kTopkMax];
  __shared__ uint32_t nidx[kTopkMax];
  int n2 = 2;
  while (n2 < k) n2 <<= 1;
  const uint32_t got = min(W->taken, (uint32_t)k);
  for (int i = threadIdx.x; i < n2; i += kTkSortThreads) {
    // (padding below every entry: an entry's ~index is >= 2^31)
    key[i] = (uint32_t)i < got ? W->key[i] : 0ull;
    nidx[i] = (uint32_t)i < got ? W->nidx[i] : 0u;
  }
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < n2 / 2; t += kTkSortThreads) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const uint64_t ka = key[lo], kb = key[hi];
        const uint32_t ia = nidx[lo], ib = nidx[hi];
        const bool a_less = ka < kb || (ka == kb && ia < ib);
        if (a_less == desc && !(ka == kb && ia == ib)) {
          key[lo] = kb; key[hi] = ka;
          nidx[lo] = ib; nidx[hi] = ia;
        }
      }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += kTkSortThreads) idx[i] = (int32_t)~nidx[i];
}

// out[hp][j] = vals[hp][idx[j]]; an index outside [0, ld) gives NaN
__global__ __launch_bounds__(kTkThreads) void k_gather_points(const double *__restrict__ vals,
                                                              int64_t ld, int32_t n_hp,
                                                              const int32_t *__restrict__ idx,
                                                              int32_t k, double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kTkThreads + threadIdx.x;
  if (e >= (int64_t)n_hp * k) return;
  const int64_t hp = e / k;
  const int64_t c = idx[e % k];
  out[e] = (c >= 0 && c < ld) ? vals[hp * ld + c] : NAN;
}

size_t topk_scratch_bytes() { return sizeof(TopkScratch); }

static unsigned topk_grid(int64_t m) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(kTkMaxBlocks, (m + kTkThreads - 1) / kTkThreads));
}

hipError_t launch_topk_first(const double *total, const uint8_t *eligible, int64_t m, int32_t k,
                             void *scratch, hipStream_t st) {
  TopkScratch *W = static_cast<TopkScratch *>(scratch);
  // histograms, states and the cursor (the staged entries need no clearing)
  const hipError_t e = hipMemsetAsync(W, 0, offsetof(TopkScratch, key), st);
  if (e != hipSuccess) return e;
  k_topk_hist<<<topk_grid(m), kTkThreads, 0, st>>>(total, eligible, m, k, 0, W);
  return hipGetLastError();
}

hipError_t launch_topk_rest(const double *total, const uint8_t *eligible, int64_t m, int32_t k,
                            void *scratch, int32_t *idx, hipStream_t st) {
  TopkScratch *W = static_cast<TopkScratch *>(scratch);
  const unsigned g = topk_grid(m);
  for (int pass = 1; pass < kTopkPasses; ++pass)
    k_topk_hist<<<g, kTkThreads, 0, st>>>(total, eligible, m, k, pass, W);
  k_topk_collect<<<g, kTkThreads, 0, st>>>(total, eligible, m, k, W);
  k_topk_sort<<<1, kTkSortThreads, 0, st>>>(k, W, idx);
  return hipGetLastError();
}

hipError_t launch_gather_points(const double *vals, int64_t ld, int32_t n_hp, const int32_t *idx,
                                int32_t k, double *out, hipStream_t st) {
  const int64_t n = (int64_t)n_hp * k;
  if (n <= 0) return hipSuccess;
  k_gather_points<<<(unsigned)((n + kTkThreads - 1) / kTkThreads), kTkThreads, 0, st>>>(
      vals, ld, n_hp, idx, k, out);
  return hipGetLastError();
}

}  // namespace tpe
