// tpe_joint_dev.hpp -- device helpers shared by the two joint Parzen models:
// the one over the root hps (tpe_joint.hip) and the one per group of hps that
// are active together (tpe_group.hip).
#pragma once
#include <math.h>

#include "tpe_draw.hpp"
#include "tpe_lpdf.hpp"

namespace tpe {

constexpr int kJtThreads = 256;    // the fit kernels, and the draw tables' scan order
constexpr int kJsThreads = 64;     // the scoring kernels: one wave, its staged values in LDS
constexpr uint32_t kJointStream = 1u << 29;

__device__ __forceinline__ double joint_cat_a(double prior_weight, int upper, double tot) {
#pragma clang fp contract(off)
  return prior_weight * (double)(upper - 1) / tot;
}
// kappa of a categorical component with observation o (o < 0: the prior) at
// option c, in the model's operation order
__device__ __forceinline__ double joint_kappa(bool hit, double a, double pi) {
#pragma clang fp contract(off)
  return ((hit ? 1.0 : 0.0) + a * pi) / (1.0 + a);
}
__device__ __forceinline__ double joint_pi(const tpe_hp &H, const double *pprior, int c) {
  return (H.flags & TPE_PCHOICE) ? pprior[H.pprior_begin + c] : 1.0 / (double)H.upper;
}

// block-wide sum: per-thread strided partials, then a fixed tree (256 threads)
__device__ __forceinline__ double jt_block_sum(double v, double *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = kJtThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ KDbl *joint_uniform(const double *p) {
  const uint64_t u = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return (KDbl *)(((uint64_t)hi << 32) | lo);
}

// One quantized kernel term log2(Phi(ub) - Phi(lb)) per component of the
// block, erf_term's operation order with w = 1
template <bool LOGN>
__device__ __forceinline__ void joint_erf(KDbl *__restrict__ f, double ub, double lb,
                                          double (&t)[1][kGroup]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < kGroup; ++j) {
    const double cx = f[j], cy = f[kCoefBlock + j];
    const double zu = (ub - cx) * cy, zl = (lb - cx) * cy;
    t[0][j] += fast_log2(erf_term<LOGN>(zu, zl, 1.0));
  }
}

}  // namespace tpe
