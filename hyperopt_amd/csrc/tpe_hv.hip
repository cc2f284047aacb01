// tpe_hv.hip -- multi-objective TPE: greedy hypervolume subset selection
// inside the Pareto front, gfx950 (tpe_plan_set_hv).
//
// After k_pareto_count (tpe_pareto.hip) the front rows are ordered by what
// they add to the hypervolume against a reference point r[M]: n_pick greedy
// rounds, each taking the row of largest gain given the rows taken so far.
// A row takes part when it is complete, nondominated, finite in every
// objective and strictly below r in every objective; w = r - y is its box and
// vol = w[0] * ... * w[M-1] the box's volume.
//   exact (M = 2)   the rows taken clip the box from the right (the smallest
//                   y_p[0] above y_i[0]) and from the top (the smallest y_p[1]
//                   above y_i[1]); front rows are mutually nondominated, so the
//                   clipped box is the area gain.  A row equal to a pick is dead.
//   Monte-Carlo     S samples z = y + u * w per row from one table u[S][M] of
//                   Philox uniforms (draw4, stream kHvStream); a sample is alive
//                   until a pick lies below it in every objective; the gain is
//                   vol * alive (no division on the device).
// Kernels, all on the caller's stream, no host synchronisation in between:
//   k_hv_uniforms  the table, u[word][M][64]
//   k_hv_init<M>   per row: participation, vol, alive words all ones, cnt = S
//                  (exact: right = r[0], top = r[1])
//   k_hv_round<M>  the previous pick (read from device memory; -1: nothing to
//                  do) against every live row.  Monte-Carlo: grid.x = row tiles,
//                  one row per lane with y and w in registers, grid.y = sample
//                  words; the block stages its 64 x M uniforms in LDS and every
//                  lane reads the same address (a broadcast); killed samples
//                  leave cnt[row] by an integer atomic, so the counts do not
//                  depend on the launch shape.  Exact: one lane per row.
//   k_hv_pick      one block: the largest (key bits, lower row) is pick t
//   k_hv_loss<M>   the surrogate column s = dominated_by (n + 1) + sec
// Keys are non-negative doubles compared as integers; z is formed by a rounded
// product and a rounded sum (no fused multiply-add), so every quantity is the
// one tests/hv_oracle.py computes in numpy.
#include <math.h>

#include "tpe_device.hpp"
#include "tpe_draw.hpp"
#include "tpe_hv_plan.hpp"

#pragma clang fp contract(off)

namespace tpe {

namespace {

// a row's state: >= 0 the round it was picked in
constexpr int32_t kHvLive = -1;   // takes part, not picked yet
constexpr int32_t kHvOut = -2;    // takes no part
constexpr int32_t kHvDead = -3;   // exact path: equal to a pick

template <int M>
struct HvRef { double r[M]; };

__global__ __launch_bounds__(kHvWord) void k_hv_uniforms(uint64_t seed, int32_t M,
                                                         double *__restrict__ u) {
  const int64_t s = (int64_t)blockIdx.x * kHvWord + threadIdx.x;  // (S is a multiple of 64)
  double *row = u + (int64_t)blockIdx.x * M * kHvWord + threadIdx.x;
  for (int it = 0; 4 * it < M; ++it) {
    const Draw d = draw4(seed, (uint64_t)s, kHvStream, (uint32_t)it);
    const double v[4] = {d.u0, d.u1, d.u2, d.u3};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (4 * it + c < M) row[(int64_t)(4 * it + c) * kHvWord] = v[c];
  }
}

// row i's objectives and box; true when it takes part
template <int M>
__device__ __forceinline__ bool hv_row(const double *__restrict__ Y, int64_t ld, int64_t i,
                                       const HvRef<M> &ref, int32_t dominated_by,
                                       double (&y)[M], double (&w)[M]) {
  bool part = dominated_by == 0;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    y[m] = Y[(int64_t)m * ld + i];
    w[m] = ref.r[m] - y[m];
    // (NaN fails every comparison; +inf and -inf fail the finite test)
    part = part && fabs(y[m]) < INFINITY && w[m] > 0.0;
  }
  return part;
}

template <int M>
__global__ __launch_bounds__(kHvTile) void k_hv_init(
    const double *__restrict__ Y, int64_t ld, int64_t n, HvRef<M> ref,
    const int32_t *__restrict__ dominated_by, int32_t S, bool exact, int32_t *__restrict__ state,
    int32_t *__restrict__ cnt, double *__restrict__ vol, double *__restrict__ right,
    double *__restrict__ top, uint64_t *__restrict__ alive, int32_t *__restrict__ n_picked) {
  const int64_t i = (int64_t)blockIdx.x * kHvTile + threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *n_picked = 0;
  if (i >= n) return;
  double y[M], w[M];
  const bool part = hv_row<M>(Y, ld, i, ref, dominated_by[i], y, w);
  if (!exact) alive[(int64_t)blockIdx.y * ld + i] = part ? ~0ull : 0ull;
  if (blockIdx.y != 0) return;
  double v = w[0];
#pragma unroll
  for (int m = 1; m < M; ++m) v = v * w[m];
  state[i] = part ? kHvLive : kHvOut;
  vol[i] = part ? v : 0.0;
  if (exact) {
    right[i] = ref.r[0];
    top[i] = ref.r[M > 1 ? 1 : 0];
  } else {
    cnt[i] = part ? S : 0;
  }
}

// Monte-Carlo round t >= 1: the pick of round t - 1 kills the samples it lies
// below
template <int M>
__global__ __launch_bounds__(kHvTile) void k_hv_round_mc(
    const double *__restrict__ Y, int64_t ld, int64_t n, HvRef<M> ref,
    const int32_t *__restrict__ prev_pick, const double *__restrict__ u,
    const int32_t *__restrict__ state, int32_t *__restrict__ cnt,
    uint64_t *__restrict__ alive) {
  __shared__ double su[M][kHvWord];
  static_assert(sizeof(su) <= kHvLdsLimit, "the staged uniforms fit the plan's LDS limit");
  const int32_t p = *prev_pick;  // (wave-uniform: a scalar load)
  if (p < 0) return;
  const int lane = threadIdx.x;
  const double *ub = u + (int64_t)blockIdx.y * M * kHvWord;
  for (int k = lane; k < M * kHvWord; k += kHvTile) su[k / kHvWord][k % kHvWord] = ub[k];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kHvTile + lane;
  if (i >= n || state[i] != kHvLive) return;
  uint64_t *word = alive + (int64_t)blockIdx.y * ld + i;
  const uint64_t a = *word;
  if (a == 0) return;
  double yp[M], y[M], w[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    yp[m] = Y[(int64_t)m * ld + p];
    y[m] = Y[(int64_t)m * ld + i];
    w[m] = ref.r[m] - y[m];
  }
  uint64_t below = 0;  // samples the pick lies below
#pragma unroll 4
  for (int s = 0; s < kHvWord; ++s) {
    bool b = true;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double z = __dadd_rn(y[m], __dmul_rn(su[m][s], w[m]));
      b = b && yp[m] <= z;
    }
    below |= (uint64_t)(b ? 1 : 0) << s;
  }
  const uint64_t killed = a & below;
  if (killed) {
    *word = a & ~killed;
    atomicSub(&cnt[i], __popcll(killed));
  }
}

// exact round t >= 1 (two objectives): the pick of round t - 1 clips the boxes
__global__ __launch_bounds__(kHvTile) void k_hv_round_exact(
    const double *__restrict__ Y, int64_t ld, int64_t n,
    const int32_t *__restrict__ prev_pick, int32_t *__restrict__ state,
    double *__restrict__ gain, double *__restrict__ right, double *__restrict__ top) {
  const int32_t p = *prev_pick;
  if (p < 0) return;
  const int64_t i = (int64_t)blockIdx.x * kHvTile + threadIdx.x;
  if (i >= n || state[i] != kHvLive) return;
  const double p0 = Y[p], p1 = Y[ld + p];
  const double y0 = Y[i], y1 = Y[ld + i];
  if (p0 == y0 && p1 == y1) {
    state[i] = kHvDead;
    gain[i] = 0.0;
    return;
  }
  double rt = right[i], tp = top[i];
  if (p0 > y0 && p0 < rt) right[i] = rt = p0;
  if (p1 > y1 && p1 < tp) top[i] = tp = p1;
  gain[i] = (rt - y0) * (tp - y1);
}

// a larger key wins, then the lower row
__device__ __forceinline__ bool hv_less(uint64_t ka, int32_t ra, uint64_t kb, int32_t rb) {
  return ka != kb ? ka < kb : ra > rb;
}

// round t's pick: cnt != nullptr the Monte-Carlo key vol * cnt, else the
// exact gain held in vol
__global__ __launch_bounds__(kHvPickThreads) void k_hv_pick(
    int64_t n, int32_t t, int32_t *__restrict__ state, const int32_t *__restrict__ cnt,
    const double *__restrict__ vol, int32_t *__restrict__ picks, double *__restrict__ keys,
    int32_t *__restrict__ counts, int32_t *__restrict__ n_picked) {
  __shared__ uint64_t rk[kHvPickThreads];
  __shared__ int32_t rr[kHvPickThreads];
  if (t > 0 && picks[t - 1] < 0) {  // the selection has ended
    if (threadIdx.x == 0) { picks[t] = -1; keys[t] = 0.0; counts[t] = -1; }
    return;
  }
  uint64_t bk = 0;
  int32_t br = 0x7fffffff;
  for (int64_t i = threadIdx.x; i < n; i += kHvPickThreads) {
    if (state[i] != kHvLive) continue;
    double key;
    if (cnt) {
      const int32_t c = cnt[i];
      key = c > 0 ? vol[i] * (double)c : 0.0;  // (vol may be +inf: no 0 * inf)
    } else {
      key = vol[i];
    }
    const uint64_t kb = (uint64_t)__double_as_longlong(key);
    if (hv_less(bk, br, kb, (int32_t)i)) { bk = kb; br = (int32_t)i; }
  }
  rk[threadIdx.x] = bk;
  rr[threadIdx.x] = br;
  __syncthreads();
  for (int w = kHvPickThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w &&
        hv_less(rk[threadIdx.x], rr[threadIdx.x], rk[threadIdx.x + w], rr[threadIdx.x + w])) {
      rk[threadIdx.x] = rk[threadIdx.x + w];
      rr[threadIdx.x] = rr[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double best = __longlong_as_double((long long)rk[0]);
  if (!(best > 0.0)) {
    picks[t] = -1; keys[t] = 0.0; counts[t] = -1;
    return;
  }
  const int32_t p = rr[0];  // (< n: only live rows carry a key above 0)
  picks[t] = p;
  keys[t] = best;
  counts[t] = cnt ? cnt[p] : -1;
  state[p] = t;
  *n_picked = t + 1;
}

template <int M>
__global__ __launch_bounds__(kHvTile) void k_hv_loss(
    const double *__restrict__ Y, int64_t ld, int64_t n,
    const int32_t *__restrict__ dominated_by, const int32_t *__restrict__ dominates,
    const int32_t *__restrict__ state, const int32_t *__restrict__ n_picked,
    double *__restrict__ losses) {
  const int64_t i = (int64_t)blockIdx.x * kHvTile + threadIdx.x;
  if (i >= n) return;
  bool complete = true;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double v = Y[(int64_t)m * ld + i];
    complete = complete && v == v && v != INFINITY;
  }
  const int64_t R = *n_picked;
  const int32_t st = state[i], by = dominated_by[i];
  int64_t sec = n - (int64_t)dominates[i];
  if (st >= 0) sec = st;
  else if (by == 0 && sec < R) sec = R;
  // (an exact integer: sec stays in [0, n], (n + 1)^2 < 2^53)
  const int64_t s = (int64_t)by * (n + 1) + sec;
  losses[i] = complete ? (double)s : INFINITY;
}

template <int M>
hipError_t select_m(const HvArgs &a, hipStream_t st) {
  HvRef<M> ref;
  for (int m = 0; m < M; ++m) ref.r[m] = a.ref[m];
  const unsigned tiles = (unsigned)((a.n + kHvTile - 1) / kHvTile);
  const unsigned words = a.exact ? 1u : (unsigned)(a.S / kHvWord);
  if (!a.exact && a.make_u) k_hv_uniforms<<<words, kHvWord, 0, st>>>(a.seed, M, a.u);
  k_hv_init<M><<<dim3(tiles, words), kHvTile, 0, st>>>(a.Y, a.ld, a.n, ref, a.dominated_by, a.S,
                                                       a.exact, a.state, a.cnt, a.vol, a.right,
                                                       a.top, a.alive, a.n_picked);
  hipError_t e = hipGetLastError();
  for (int t = 0; t < a.n_pick && e == hipSuccess; ++t) {
    if (t > 0) {
      if (a.exact) {
        if constexpr (M == 2)
          k_hv_round_exact<<<tiles, kHvTile, 0, st>>>(a.Y, a.ld, a.n, a.picks + (t - 1), a.state,
                                                      a.vol, a.right, a.top);
      } else {
        k_hv_round_mc<M><<<dim3(tiles, words), kHvTile, 0, st>>>(
            a.Y, a.ld, a.n, ref, a.picks + (t - 1), a.u, a.state, a.cnt, a.alive);
      }
    }
    k_hv_pick<<<1, kHvPickThreads, 0, st>>>(a.n, t, a.state, a.exact ? nullptr : a.cnt, a.vol,
                                            a.picks, a.keys, a.counts, a.n_picked);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return e;
  k_hv_loss<M><<<tiles, kHvTile, 0, st>>>(a.Y, a.ld, a.n, a.dominated_by, a.dominates, a.state,
                                          a.n_picked, a.losses);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_hv_select(const HvArgs &a, hipStream_t st) {
  const HvPlan hp = hv_plan(a.n, a.M, a.n_pick, a.S, a.exact ? kHvExact : kHvMc);
  if (!hp.ok || a.n > a.ld) return hipErrorInvalidValue;
  switch (a.M) {
    case 2: return select_m<2>(a, st);
    case 3: return select_m<3>(a, st);
    case 4: return select_m<4>(a, st);
    case 5: return select_m<5>(a, st);
    case 6: return select_m<6>(a, st);
    case 7: return select_m<7>(a, st);
    case 8: return select_m<8>(a, st);
    default: return hipErrorInvalidValue;
  }
}
static_assert(kParetoMaxObj == 8, "one instantiation per objective count");

}  // namespace tpe
