// tpe_points_dev.hpp -- the per-hp term of a whole configuration, device side:
// the lpdf pair of one value under the two mixtures of an (info, coef) table
// set, shared by k_score_points (tpe_points.hip) and k_ctpe_score
// (tpe_ctpe.hip), so that both compute a term with the same arithmetic.
#pragma once
#include <math.h>

#include "tpe_lpdf.hpp"

namespace tpe {

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

// ---- the same terms with the two lpdfs handed back separately (lb below, la
// above) for k_importance (tpe_importance.hip): the arithmetic, statement for
// statement, of the three functions above, which stay as they are so that the
// kernels built on them keep their code
template <bool LOGN>
__device__ __forceinline__ void points_lse_pair(const PointsArgs &A, const tpe_hp &H, int hp,
                                                double x, double &lb, double &la) {
  const double y[1] = {(LOGN ? fast_log(x) : x) - H.prior_mu};
  const double y2[1] = {y[0] * y[0]};
  double lp[2];
#pragma unroll
  for (int mix = 0; mix < 2; ++mix) {
    const int64_t slot = 2 * (int64_t)hp + mix;
    lp[mix] = points_lse_mix<LOGN>(uniform_ptr(A.coef + slot * A.kcap), A.info[slot].K, x, y, y2);
  }
  lb = lp[0];
  la = lp[1];
}

template <bool LOGN>
__device__ __forceinline__ void points_erf_pair(const PointsArgs &A, const tpe_hp &H, int hp,
                                                double x, bool act, double &lb, double &la) {
#pragma clang fp contract(off)
  double ub, lo;
  quant_bounds<LOGN>(H, x, ub, lo);
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
        const double zu = (ub - cx) * cy, zl = (lo - cx) * cy;
        if (__all(!act || erf_dead(zu, zl))) continue;
        pc += erf_term<LOGN>(zu, zl, cs[coef_off(k, 2)]);
      }
      prob += pc;
    }
    lp[mix] = log(prob) - A.info[slot].log_pacc;
  }
  lb = lp[0];
  la = lp[1];
}

__device__ __forceinline__ void points_cat_pair(const PointsArgs &A, int hp, double x, double &lb,
                                                double &la) {
  const int64_t sb = 2 * (int64_t)hp;
  const int K = A.info[sb].K;
  bool in = x >= 0.0 && x < (double)K;
  const int64_t c = in ? (int64_t)x : 0;
  in = in && (double)c == x;
  const double *tb = reinterpret_cast<const double *>(A.coef + sb * A.kcap);
  const double *ta = reinterpret_cast<const double *>(A.coef + (sb + 1) * A.kcap);
  lb = in ? tb[coef_off(c, 0)] : NAN;
  la = in ? ta[coef_off(c, 0)] : NAN;
}

}  // namespace tpe
