// tpe_lpdf.hpp -- the per-pair lpdf arithmetic shared by the scoring kernels
// of candidates (tpe_score.hip) and of whole configurations (tpe_points.hip):
// the log-sum-exp accumulator and its group fold, the wave-uniform
// coefficient loads, and the quantized kinds' bounds and CDF-difference term.
#pragma once
#include <math.h>

#include "tpe_device.hpp"

namespace tpe {

// A log-sum-exp partial in log2 units: value = m + log2(s).  The exponent m
// is kept integer-valued (or -inf), so every rescale of s to a new exponent is
// an exact power-of-two ldexp; the only rounding is in the terms themselves.
struct LseAcc {
  double m, s;
};

// merge b into a (a then b): the order every path uses
__device__ __forceinline__ void lse_merge(LseAcc &a, const LseAcc &b) {
  if (b.m == -INFINITY && b.s == 0.0) return;
  if (a.m == -INFINITY && a.s == 0.0) { a = b; return; }
  if (a.m != a.m || b.m != b.m) { a = LseAcc{NAN, NAN}; return; }
  const double M = fmax(a.m, b.m);
  a.s = ldexp(a.s, (int)fmax(a.m - M, -2100.0)) + ldexp(b.s, (int)fmax(b.m - M, -2100.0));
  a.m = M;
}

// Coefficients read through the constant address space: the component loops
// below index them with wave-uniform addresses, so they compile to scalar
// loads (s_load into SGPRs, one per wave, no LDS or VGPR traffic per lane).
typedef const double __attribute__((address_space(4))) KDbl;

// a wave-uniform table pointer as a scalar (the compiler cannot always prove it)
__device__ __forceinline__ KDbl *uniform_ptr(const Coef *p) {
  const uint64_t u = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return (KDbl *)(((uint64_t)hi << 32) | lo);
}

constexpr int kGroup = kCoefBlock;  // components per scalar-load group: one table block

struct CoefGroup {
  double x[kGroup], y[kGroup], z[kGroup];
};

// three 64-B scalar loads: the x, y, z rows of the table block at k (whole
// blocks are allocated, entries past the mixture are masked by the caller)
__device__ __forceinline__ void load_group(KDbl *__restrict__ cs, int k, CoefGroup &g) {
  KDbl *b = cs + (((unsigned)k >> 3) << 5);  // k >= 0: coef_off(k, 0) of a block start
#pragma unroll
  for (int j = 0; j < kGroup; ++j) {
    g.x[j] = b[j];
    g.y[j] = b[kCoefBlock + j];
    g.z[j] = b[2 * kCoefBlock + j];
  }
}

// Single-pass log-sum-exp over the wave's chunks of a mixture of nb
// components against the lane's KR candidates (log2 units, t = alpha +
// y'(beta + gamma y'), make_coef).  Per group of kGroup components: the group
// max lifts the integer exponent m to ceil(max) if larger (exact ldexp rescale
// of s), then s += 2^(t - m) with v_exp_f32 on the fp64 difference (every
// term <= 1, the largest > 1/2).  A NaN term makes its 2^(t - m) NaN, which
// reaches the lpdf as the reference's NaN (logsum_rows, tpe.py:37-40); fmax
// drops it from the exponent, so a lane whose terms are all NaN keeps
// m = -inf and scores NaN as well.
template <int KR>
__device__ __forceinline__ void lse_terms(const CoefGroup &g, const double (&y)[KR],
                                          const double (&y2)[KR], double (&t)[KR][kGroup]) {
#pragma unroll
  for (int r = 0; r < KR; ++r)
#pragma unroll
    for (int j = 0; j < kGroup; ++j)
      // alpha + beta y' + gamma y'^2, one scalar coefficient per FMA
      t[r][j] = fma(g.z[j], y2[r], fma(g.y[j], y[r], g.x[j]));
}
template <int KR>
__device__ __forceinline__ void lse_fold(const double (&t)[KR][kGroup], double (&m)[KR],
                                         double (&s)[KR]) {
#pragma unroll
  for (int r = 0; r < KR; ++r) {
    // group max as a tree (fmax drops NaN terms)
    double mx[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) mx[j] = t[r][j];
#pragma unroll
    for (int w = kGroup / 2; w > 0; w >>= 1)
#pragma unroll
      for (int j = 0; j < w; ++j) mx[j] = fmax(mx[j], mx[j + w]);
    // lift the integer exponent; s == 0 while m == -inf, and the clamp turns
    // the -inf / NaN differences of that state into a harmless ldexp of 0
    const double mn = fmax(m[r], ceil(mx[0]));
    s[r] = ldexp(s[r], (int)fmax(m[r] - mn, -2100.0));
    m[r] = mn;
    const double ms = mn == -INFINITY ? 0.0 : mn;  // all terms -inf / NaN so far
    // terms 2^(t - m) <= 1 summed as an fp32 tree (<= kGroup), then in fp64
    float e[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) e[j] = __builtin_amdgcn_exp2f((float)(t[r][j] - ms));
#pragma unroll
    for (int w = kGroup / 2; w > 0; w >>= 1)
#pragma unroll
      for (int j = 0; j < w; ++j) e[j] += e[j + w];
    s[r] += (double)e[0];
  }
}

// Candidate-side bounds of the quantized lpdf, tpe.py:146-152 (GMM) and
// 284-293 (LGMM: on log scale, lb clipped at 0, both floored at EPS).
template <bool LOGN>
__device__ __forceinline__ void quant_bounds(const tpe_hp &H, double x, double &ub, double &lb) {
  const double hq = H.q / 2.0;
  if constexpr (!LOGN) {
    ub = (H.flags & TPE_HAS_HIGH) ? np_minimum(x + hq, H.high) : x + hq;
    lb = (H.flags & TPE_HAS_LOW) ? np_maximum(x - hq, H.low) : x - hq;
  } else {
    const double u = (H.flags & TPE_HAS_HIGH) ? np_minimum(x + hq, exp(H.high)) : x + hq;
    double l = (H.flags & TPE_HAS_LOW) ? np_maximum(x - hq, exp(H.low)) : x - hq;
    l = np_maximum(0.0, l);
    ub = u < 0.0 ? NAN : log(np_maximum(u, kEPS));
    lb = log(np_maximum(l, kEPS));
  }
}

// one quantized term w (Phi(ub) - Phi(lb)) in the reference's operation
// order (GMM: 0.5 * (1 + erf), LGMM: .5 + .5 * erf; two-stage difference)
template <bool LOGN>
__device__ __forceinline__ double erf_term(double zu, double zl, double w) {
#pragma clang fp contract(off)
  double cu, cl;
  if (LOGN) {
    cu = .5 + .5 * erf(zu);
    cl = .5 + .5 * erf(zl);
  } else {
    cu = 0.5 * (1.0 + erf(zu));
    cl = 0.5 * (1.0 + erf(zl));
  }
  double inc = w * cu;
  inc -= w * cl;
  return inc;
}

// a term whose two erf arguments are beyond 6.5 on one side is an exact 0
// (erf saturates to +-1 from 5.93)
__device__ __forceinline__ bool erf_dead(double zu, double zl) {
  return (zu >= 6.5 && zl >= 6.5) || (zu <= -6.5 && zl <= -6.5);
}

}  // namespace tpe
