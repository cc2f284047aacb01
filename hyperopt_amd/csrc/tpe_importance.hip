// tpe_importance.hip -- hyperparameter importances from the fitted Parzen
// models, gfx950 (tpe_plan_importance).
//
// PED-ANOVA's density form: for live model m (0 the plan's own fit, l >= 1 the
// c-TPE bank's) and hp d, with l and g the fitted below and above densities
// and q = ghat l + (1 - ghat) g the model's density of all trials,
//   D[m][d]    = (1 - ghat)^2 sum_i w_i (l_i - g_i)^2 / q_i   (the Pearson
//                divergence int (l / q - 1)^2 q on the nodes),
//   mass[m][d] = sum_i w_i q_i                                (1 when the nodes
//                cover the density).
// Launches:
//   k_importance      grid (tiles of 256 nodes, hp, live model), as
//                     k_ctpe_score lays out its grid.  The model's table base
//                     is block-uniform; a wave is 64 nodes of its (hp, model):
//                     each lane builds its node from the descriptor
//                     (importance_nodes), evaluates both mixtures -- the
//                     coefficient blocks come through wave-uniform scalar
//                     loads, 8 components at a time, and the arithmetic is
//                     k_score_points' own (tpe_points_dev.hpp) -- and forms
//                     f_i and q_i w_i from the two log densities.  The block
//                     adds its 256 values of each in a fixed LDS tree and
//                     writes part[model][hp][tile][2].  Nodes are never
//                     stored unless the caller asks for the curves;
//   k_importance_sum  one block per live model: per hp the tiles added in
//                     ascending order, D and mass; then norm = D / sum_d D
//                     with d ascending (0 where that sum is 0).
// No floating-point atomics; a number depends on the fixed 256-node tile only.
#include <math.h>

#include "tpe_importance.hpp"
#include "tpe_points_dev.hpp"

namespace tpe {

// the model's tables (ctpe_model of tpe_ctpe.hip) and its component means
__device__ __forceinline__ const double *imp_model(const ImportanceArgs &I, int l, PointsArgs &B) {
  if (l == 0) return I.mmu;
  const int64_t slots = 2 * (int64_t)I.P.n_hp;
  B.info = I.bk_info + (int64_t)(l - 1) * slots;
  B.coef = I.bk_coef + (int64_t)(l - 1) * slots * I.P.kcap;
  return I.bk_mmu + (int64_t)(l - 1) * slots * I.P.kcap;
}

__global__ __launch_bounds__(kImpThreads) void k_importance(ImportanceArgs I) {
  __shared__ double red[2][kImpThreads];
  const int hp = blockIdx.y;
  const int l = blockIdx.z;
  PointsArgs A = I.P;
  const double *mmu = imp_model(I, l, A);
  const tpe_hp H = A.hps[hp];
  const int kind = score_kind(H);  // block-uniform
  const int64_t sb = 2 * (int64_t)hp;
  double min_mu = 0.0, max_mu = 0.0;
  if (kind != KIND_CAT && !((H.flags & TPE_HAS_LOW) && (H.flags & TPE_HAS_HIGH))) {
    const double *mb = mmu + sb * A.kcap, *ma = mmu + (sb + 1) * A.kcap;
    const int Kb = A.info[sb].K, Ka = A.info[sb + 1].K;
    if (Kb > 0 && Ka > 0) {
      min_mu = fmin(mb[0], ma[0]);
      max_mu = fmax(mb[Kb - 1], ma[Ka - 1]);
    }
  }
  const ImpNodes N = importance_nodes(H, kind, min_mu, max_mu, I.G);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i0 = (int)blockIdx.x * kImpThreads + wave * 64;
  const int i = i0 + (int)(threadIdx.x & 63);
  const bool act = i < N.count;
  double x = kind_logn(kind) ? 1.0 : 0.0, w = 0.0;
  double lb = NAN, la = NAN, f = 0.0, qw = 0.0;
  if (i0 < N.count) {  // wave-uniform: a wave past the nodes only joins the tree
    if (act) importance_node(N, H, kind, i, x, w);
    switch (kind) {
      case KIND_LSE_G: points_lse_pair<false>(A, H, hp, x, lb, la); break;
      case KIND_LSE_L: points_lse_pair<true>(A, H, hp, x, lb, la); break;
      case KIND_ERF_G: points_erf_pair<false>(A, H, hp, x, act, lb, la); break;
      case KIND_ERF_L: points_erf_pair<true>(A, H, hp, x, act, lb, la); break;
      default: points_cat_pair(A, hp, x, lb, la); break;
    }
    {
      // f = w e^hi (e^(a - hi) - e^(b - hi))^2 / (ghat e^(a - hi) + (1 - ghat) e^(b - hi)),
      // q w = w e^hi times that denominator; nothing where both densities are 0
#pragma clang fp contract(off)
      const double ghat = I.ghat[l];
      const double hi = fmax(lb, la);
      if (act && hi != -INFINITY) {
        const double ea = exp(lb - hi), eb = exp(la - hi);
        const double d = ea - eb;
        const double den = ghat * ea + (1.0 - ghat) * eb;
        const double we = w * exp(hi);
        f = we * (d * d) / den;
        qw = we * den;
      }
    }
  }
  if (i < I.G) {
    const int64_t o = ((int64_t)l * A.n_hp + hp) * I.G + i;
    if (I.x) I.x[o] = act ? x : NAN;
    if (I.lb) I.lb[o] = act ? lb : NAN;
    if (I.la) I.la[o] = act ? la : NAN;
  }
  // the fixed tree: v[t] += v[t + s] for s = 128, 64, .. 1
  red[0][threadIdx.x] = f;
  red[1][threadIdx.x] = qw;
  __syncthreads();
#pragma unroll
  for (int s = kImpThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2)
    I.part[(((int64_t)l * A.n_hp + hp) * I.tiles + blockIdx.x) * 2 + threadIdx.x] =
        red[threadIdx.x][0];
}

__global__ __launch_bounds__(kImpThreads) void k_importance_sum(ImportanceArgs I) {
#pragma clang fp contract(off)
  __shared__ double tot;
  const int l = blockIdx.x;
  const int P = I.P.n_hp;
  const double ghat = I.ghat[l];
  const double c = (1.0 - ghat) * (1.0 - ghat);
  double *D = I.D + (int64_t)l * P;
  for (int hp = threadIdx.x; hp < P; hp += kImpThreads) {
    const double *pt = I.part + ((int64_t)l * P + hp) * I.tiles * 2;
    double sf = 0.0, sq = 0.0;
    for (int t = 0; t < I.tiles; ++t) {
      sf += pt[2 * t];
      sq += pt[2 * t + 1];
    }
    D[hp] = ghat == 1.0 ? 0.0 : c * sf;
    I.mass[(int64_t)l * P + hp] = sq;
  }
  __syncthreads();  // (the block's own stores to D are visible to it)
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int hp = 0; hp < P; ++hp) t += D[hp];
    tot = t;
  }
  __syncthreads();
  const double t = tot;
  for (int hp = threadIdx.x; hp < P; hp += kImpThreads)
    I.norm[(int64_t)l * P + hp] = t == 0.0 ? 0.0 : D[hp] / t;
}

hipError_t launch_importance(const ImportanceArgs &a, hipStream_t st) {
  if (a.P.n_hp <= 0 || a.n_live <= 0) return hipSuccess;
  k_importance<<<dim3((unsigned)a.tiles, (unsigned)a.P.n_hp, (unsigned)a.n_live),
                 dim3(kImpThreads), 0, st>>>(a);
  k_importance_sum<<<dim3((unsigned)a.n_live), dim3(kImpThreads), 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace tpe
