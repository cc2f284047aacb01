// tpe_points.hip -- EI of whole configurations under the fitted model, gfx950
// (tpe_plan_score_points).
//
// A configuration is a row across all hyperparameters, in the history's own
// columnar layout vals[n_hp][ld]; its activity follows the space's condition
// tables and its score is the sum over its active hps of
//   term = below_llik(v) - above_llik(v)          (broadcast_best, tpe.py:749-759)
// with the lpdfs of the fitted mixtures (GMM1_lpdf tpe.py:104-166, LGMM1_lpdf
// tpe.py:259-301, categorical_lpdf tpe.py:50-57).  Three launches:
//   k_points_active  activity of every (hp, configuration), one thread per
//                    configuration walking the hps in level order; each hp's
//                    active configurations are compacted into a dense list;
//   k_score_points   term[n_hp][M]: one wave per (hp, 64 list entries), every
//                    component of both mixtures, coefficients through
//                    wave-uniform scalar loads; a wave past its hp's list
//                    leaves before it touches a table;
//   k_points_sum     total[M], the terms added in ascending hp index.
// A column of configurations is not value-sorted, so none of the sorted
// draw's block skips, moment forms or tables applies: every (configuration,
// component) pair is evaluated, with the exact path's arithmetic
// (tpe_lpdf.hpp).  Nothing depends on the grid: a configuration's numbers are
// a function of its own values.
#include <math.h>

#include "tpe_lpdf.hpp"

namespace tpe {

constexpr int kPtThreads = 256;  // 4 waves, each with its own 64 configurations

// Activity of configuration c for every hp, parents first (level_hps lists the
// plan's levels in dependency order): active iff unconditional, or some
// condition's parent is active with value == branch.  A thread reads back only
// its own stores.  A branch is an option index in [0, upper), so an active
// categorical value that is not such an integer (NaN, 1.5, upper) equals no
// branch: none of its children is activated, and its own term -- hence the
// configuration's total -- is NaN (points_cat).
//
// Compaction: in a conditional space most (hp, configuration) pairs are
// inactive (6 of 7 at config 3) and scattered, so nearly every 64-configuration
// wave of the column would hold a few active lanes and pay for 64.  Each wave
// here appends its active configurations of an hp to that hp's dense list (one
// atomic add per wave and hp reserves the range; the order of the ranges is
// arbitrary, which changes no number: a configuration's term depends on its
// own value only), and writes the +0.0 terms of the inactive ones itself.
__global__ __launch_bounds__(kPtThreads) void k_points_active(PointsArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
  const bool in = c < A.m;
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < A.n_hp; ++j) {
    const int hp = A.level_hps[j];
    const int c0 = A.hps[hp].cond_begin, nc = A.hps[hp].cond_count;
    bool act = in && nc == 0;
    if (in) {
      for (int q = 0; q < nc && !act; ++q) {
        const int64_t par = A.cond_parent[c0 + q];
        act = A.active[par * A.act_ld + c] != 0 &&
              A.vals[par * A.ld + c] == (double)A.cond_branch[c0 + q];
      }
      A.active[(int64_t)hp * A.act_ld + c] = act ? 1 : 0;
      if (!act) A.terms[(int64_t)hp * A.term_ld + c] = 0.0;
    }
    const uint64_t mk = __ballot(act);
    if (mk == 0) continue;  // (wave-uniform)
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(A.count + hp, (uint32_t)__popcll(mk));
    base = __shfl(base, 0, 64);
    if (act)
      A.idx[(int64_t)hp * A.m + base + __popcll(mk & ((1ull << lane) - 1ull))] = (int32_t)c;
  }
}

// log-sum-exp lpdf of one mixture at the lane's value: every block of 8
// components in order (the padding of the last block has alpha = -inf), the
// next block's coefficients loaded while this block's terms are folded
template <bool LOGN>
__device__ __forceinline__ double points_lse_mix(KDbl *__restrict__ cs, int K, double x,
                                                 const double (&y)[1], const double (&y2)[1]) {
  if (K <= 0) return NAN;  // (a fitted mixture has its prior component)
  double m[1] = {-INFINITY}, s[1] = {0.0};
  const int last = ((K - 1) >> 3) << 3;
  CoefGroup g;
  load_group(cs, 0, g);
  for (int kg = 0; kg < K; kg += kGroup) {
    double t[1][kGroup];
    lse_terms<1>(g, y, y2, t);
    load_group(cs, min(kg + kGroup, last), g);
    __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the fold
    lse_fold<1>(t, m, s);
  }
  // (the exact path's finalize, score_tile: a NaN value or no finite term
  // scores NaN)
  const double LN2 = 0.6931471805599453;
  if (y[0] != y[0] || m[0] == -INFINITY) return NAN;
  double lp = (m[0] + log2(s[0])) * LN2;
  if constexpr (LOGN) lp -= log(x);
  return lp;
}

template <bool LOGN>
__device__ __forceinline__ double points_lse(const PointsArgs &A, const tpe_hp &H, int hp,
                                             double x) {
  const double y[1] = {(LOGN ? fast_log(x) : x) - H.prior_mu};
  const double y2[1] = {y[0] * y[0]};
  double lp[2];
#pragma unroll
  for (int mix = 0; mix < 2; ++mix) {
    const int64_t slot = 2 * (int64_t)hp + mix;
    lp[mix] = points_lse_mix<LOGN>(uniform_ptr(A.coef + slot * A.kcap), A.info[slot].K, x, y, y2);
  }
  return lp[0] - lp[1];
}

// quantized lpdf of both mixtures, sum_k w (Phi(ub) - Phi(lb)) (tpe.py:146-160,
// 284-299): chunks of 16 components summed in component order, the chunk sums
// added in order; a component whose term is an exact zero for every active
// lane of the wave is skipped
template <bool LOGN>
__device__ __forceinline__ double points_erf(const PointsArgs &A, const tpe_hp &H, int hp,
                                             double x, bool act) {
#pragma clang fp contract(off)
  double ub, lb;
  quant_bounds<LOGN>(H, x, ub, lb);
  double lp[2];
#pragma unroll
  for (int mix = 0; mix < 2; ++mix) {
    const int64_t slot = 2 * (int64_t)hp + mix;
    KDbl *cs = uniform_ptr(A.coef + slot * A.kcap);
    const int K = A.info[slot].K;
    double prob = 0.0;
    for (int k0 = 0; k0 < K; k0 += 16) {
      const int k1 = min(K, k0 + 16);
      double pc = 0.0;
      for (int k = k0; k < k1; ++k) {
        const double cx = cs[coef_off(k, 0)], cy = cs[coef_off(k, 1)];
        const double zu = (ub - cx) * cy, zl = (lb - cx) * cy;
        if (__all(!act || erf_dead(zu, zl))) continue;
        pc += erf_term<LOGN>(zu, zl, cs[coef_off(k, 2)]);
      }
      prob += pc;
    }
    lp[mix] = log(prob) - A.info[slot].log_pacc;
  }
  return lp[0] - lp[1];
}

// categorical lookup: log p of option x, NaN unless x is an integer in [0, upper)
__device__ __forceinline__ double points_cat(const PointsArgs &A, int hp, double x) {
  const int64_t sb = 2 * (int64_t)hp;
  const int K = A.info[sb].K;
  bool in = x >= 0.0 && x < (double)K;
  const int64_t c = in ? (int64_t)x : 0;
  in = in && (double)c == x;
  const double *tb = reinterpret_cast<const double *>(A.coef + sb * A.kcap);
  const double *ta = reinterpret_cast<const double *>(A.coef + (sb + 1) * A.kcap);
  const double lpb = in ? tb[coef_off(c, 0)] : NAN;
  const double lpa = in ? ta[coef_off(c, 0)] : NAN;
  return lpb - lpa;
}

// term[hp][c] of one hp (blockIdx.y): each wave takes 64 entries of the hp's
// list of active configurations; a wave past the list's end leaves before it
// touches a table (the grid has rows for M entries per hp).  The lanes past
// the end of a last, partial wave compute on a harmless value and store
// nothing: lanes never exchange data, so what an inactive slot holds (NaN,
// garbage) is never read.
__global__ __launch_bounds__(kPtThreads) void k_score_points(PointsArgs A) {
  const int hp = blockIdx.y;
  const int64_t n = A.count[hp];  // block-uniform
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t p0 = (int64_t)blockIdx.x * kPtThreads + wave * 64;
  if (p0 >= n) return;
  const int64_t pos = p0 + (threadIdx.x & 63);
  const bool act = pos < n;
  const int64_t c = act ? A.idx[(int64_t)hp * A.m + pos] : 0;
  double *out = A.terms + (int64_t)hp * A.term_ld + c;
  const tpe_hp H = A.hps[hp];
  const int kind = score_kind(H);  // wave-uniform
  const double x = act ? A.vals[(int64_t)hp * A.ld + c] : (kind_logn(kind) ? 1.0 : 0.0);
  double term;
  switch (kind) {
    case KIND_LSE_G: term = points_lse<false>(A, H, hp, x); break;
    case KIND_LSE_L: term = points_lse<true>(A, H, hp, x); break;
    case KIND_ERF_G: term = points_erf<false>(A, H, hp, x, act); break;
    case KIND_ERF_L: term = points_erf<true>(A, H, hp, x, act); break;
    default: term = points_cat(A, hp, x); break;
  }
  if (act) *out = term;
}

// total[c] = the terms of configuration c added in ascending hp index
// (inactive ones are +0.0): one thread per configuration, no atomics
__global__ __launch_bounds__(kPtThreads) void k_points_sum(PointsArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
  if (c >= A.m) return;
  double t = 0.0;
  for (int i = 0; i < A.n_hp; ++i) t += A.terms[(int64_t)i * A.term_ld + c];
  A.total[c] = t;
}

hipError_t launch_points(const PointsArgs &a, hipStream_t st) {
  const unsigned gx = (unsigned)((a.m + kPtThreads - 1) / kPtThreads);
  k_points_active<<<dim3(gx), dim3(kPtThreads), 0, st>>>(a);
  k_score_points<<<dim3(gx, (unsigned)a.n_hp), dim3(kPtThreads), 0, st>>>(a);
  k_points_sum<<<dim3(gx), dim3(kPtThreads), 0, st>>>(a);
  return hipGetLastError();
}

// the two scoring launches alone, behind a launch that has written the
// activity, the inactive terms and the lists itself (tpe_sample_points.hip)
hipError_t launch_points_score(const PointsArgs &a, hipStream_t st) {
  const unsigned gx = (unsigned)((a.m + kPtThreads - 1) / kPtThreads);
  k_score_points<<<dim3(gx, (unsigned)a.n_hp), dim3(kPtThreads), 0, st>>>(a);
  k_points_sum<<<dim3(gx), dim3(kPtThreads), 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace tpe
