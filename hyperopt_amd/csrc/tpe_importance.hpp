// tpe_importance.hpp -- hyperparameter importances from the fitted Parzen
// models (tpe_importance.hip; tpe_plan_importance): per live
// model m and hp d the Pearson divergence between the below density l and the
// model's density of all trials q = ghat l + (1 - ghat) g, integrated on nodes
// the kernel generates from the hp descriptor.  Not part of the ABI.
//
// The node rule (include/tpe_engine.h states it in words) lives here as one
// host/device function, so that the host can size a call and a CPU program can
// check the rule without a device.
#pragma once
#include <math.h>

#include "tpe_ctpe.hpp"

namespace tpe {

constexpr int kImpThreads = 256;  // 4 waves; a tile is 256 nodes of one (hp, model)
constexpr int32_t kImpMinNodes = 64, kImpMaxNodes = 65536;
constexpr double kImpSpan = 6.0;          // unbounded kinds: prior sigmas beyond the end means
constexpr double kImpMaxCount = 0x1p52;   // lattice values counted (j0 + i s stays exact)

// The nodes of one (hp, model): node i < count is
//   continuous (kind LSE):  y = lo + (i + 0.5) h; x = y, w = h, or for the log
//                           kinds x = node_exp(y), w = h x;
//   lattice (ERF, CAT):     x = q (j0 + i s), w = s (CAT: q = 1, j0 = 0).
struct ImpNodes {
  double lo, h;   // continuous
  double j0, s;   // lattice
  int32_t count;  // nodes, <= G
  int32_t pad;
};

// min_mu / max_mu: the first / last component mean over the model's two sorted
// mixtures of the hp (read only by the unbounded kinds).  Every product and sum
// is rounded on its own (nothing contracted): tests/importance_oracle.py
// restates the rule in numpy and must give the same bits.
__host__ __device__ inline ImpNodes importance_nodes(const tpe_hp &H, int kind, double min_mu,
                                                     double max_mu, int32_t G) {
#pragma clang fp contract(off)
  ImpNodes n;
  n.lo = 0.0; n.h = 0.0; n.j0 = 0.0; n.s = 1.0; n.count = G; n.pad = 0;
  double count;
  if (kind == KIND_CAT) {
    count = (double)H.upper;
  } else {
    // the fit's space: y for the normal / uniform kinds, log x for the log kinds
    const bool bounded = (H.flags & TPE_HAS_LOW) && (H.flags & TPE_HAS_HIGH);
    const double span = kImpSpan * H.prior_sigma;
    const double lo = bounded ? H.low : min_mu - span;
    const double hi = bounded ? H.high : max_mu + span;
    if (kind == KIND_LSE_G || kind == KIND_LSE_L) {
      n.lo = lo;
      n.h = (hi - lo) / (double)G;
      return n;
    }
    const bool logn = kind == KIND_ERF_L;
    const double lox = logn ? exp(lo) : lo, hix = logn ? exp(hi) : hi;
    const double hq = H.q / 2.0;
    double j0 = ceil(lox / H.q - 0.5), j1 = floor(hix / H.q + 0.5);
    if (logn) j0 = fmax(j0, 0.0);
    // a value whose cell [x - q/2, x + q/2] misses the support by a rounding
    // has no mass to give (quant_bounds would hand back ub < lb)
    if (bounded && H.q * j0 + hq < lox) j0 += 1.0;
    if (bounded && H.q * j1 - hq > hix) j1 -= 1.0;
    n.j0 = j0;
    count = j1 - j0 + 1.0;
  }
  count = fmin(fmax(count, 0.0), kImpMaxCount);
  if (count > (double)G) n.s = ceil(count / (double)G);
  n.count = (int32_t)ceil(count / n.s);
  return n;
}

// exp(y) of a continuous log-kind node as a fixed sequence of fp64 operations
// (each rounded on its own), so that a node has the same bits wherever the
// rule is restated: k = rint(y log2 e), r = (y - k ln2_hi) - k ln2_lo (|r| <=
// 0.35, k ln2_hi exact: ln2_hi has 21 trailing zero bits), the degree-13 Taylor
// polynomial of exp(r) by Horner's rule (truncation below 4e-18), then an
// exact ldexp.  Within 2 ulp of exp(y): the node is the rule's x, and its
// weight h x is taken at that x.
__device__ __forceinline__ double node_exp(double y) {
#pragma clang fp contract(off)
  constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0,
                            1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0,
                            1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
  const double k = rint(y * 1.4426950408889634);
  const double r = (y - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33;
  double p = c[13];
#pragma unroll
  for (int j = 12; j >= 0; --j) p = p * r + c[j];
  return ldexp(p, (int)fmin(fmax(k, -2200.0), 2200.0));
}

// node i < N.count of the rule above and its weight
__device__ __forceinline__ void importance_node(const ImpNodes &N, const tpe_hp &H, int kind, int i,
                                                double &x, double &w) {
#pragma clang fp contract(off)
  if (kind == KIND_LSE_G || kind == KIND_LSE_L) {
    const double y = N.lo + ((double)i + 0.5) * N.h;
    x = kind == KIND_LSE_L ? node_exp(y) : y;
    w = kind == KIND_LSE_L ? N.h * x : N.h;
  } else {
    x = (kind == KIND_CAT ? 1.0 : H.q) * (N.j0 + (double)i * N.s);
    w = N.s;
  }
}

struct ImportanceArgs {
  PointsArgs P;               // hps, n_hp, kcap and model 0's info / coef; the rest unused
  const MixInfo *bk_info;     // the bank (live positions l >= 1 at l - 1; tpe_ctpe.hpp)
  const Coef *bk_coef;
  const double *mmu;          // [2P][kcap] model 0's component means, ascending per slot
  const double *bk_mmu;       // the bank's
  int32_t n_live;
  int32_t G;                  // n_nodes: a multiple of 64
  int32_t tiles;              // ceil(G / 256)
  int32_t pad;
  double ghat[kCtpeModels];   // by live position
  double *part;               // [n_live][n_hp][tiles][2] tile sums of f and of q w
  double *D, *norm, *mass;    // [n_live][n_hp] out
  double *x, *lb, *la;        // [n_live][n_hp][G] out, each nullable (NaN past the nodes)
};
// k_importance, k_importance_sum in stream order
hipError_t launch_importance(const ImportanceArgs &a, hipStream_t st);

}  // namespace tpe
