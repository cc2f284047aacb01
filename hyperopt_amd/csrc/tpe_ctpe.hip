// tpe_ctpe.hip -- c-TPE: whole configurations scored under, and drawn from, a
// bank of Parzen models, gfx950 (tpe_plan_ctpe_*).
//
// Beside the objective's pair of mixtures per hp (model 0, the plan's own fit)
// stands one pair per constraint, split at the feasibility threshold and
// fitted by the same k_fit on the constraint's key column.  With T_m(c) the
// whole-configuration total of tpe_points.hip under model m and ghat_m the
// share of the history on m's good side, the acquisition is
//   acq(c) = - sum over the live models of L_m,
//   L_m    = log(ghat_m + (1 - ghat_m) exp(-T_m)),
// the log of the relative density ratio's reciprocal.  Launches:
//   k_ctpe_keys           key column of every live constraint model, one lane
//                         per row, grid.y the model; feasible rows counted by
//                         ballot, one integer atomic per wave;
//   k_ctpe_score          terms[live][hp][c]: grid (256 list entries, hp, live
//                         model); a wave takes 64 entries of its hp's list of
//                         active configurations -- activity does not depend
//                         on the model, so k_points_active's lists serve every
//                         model -- and evaluates both mixtures of its model.
//                         The model's table base is block-uniform: the
//                         coefficient blocks come through wave-uniform scalar
//                         loads, and the arithmetic is k_score_points' own
//                         (tpe_points_dev.hpp);
//   k_ctpe_combine        one thread per configuration: per live model the
//                         terms added in ascending hp index, L_m, and acq;
//   k_ctpe_sample_points  k_sample_points with the lane's model: configuration
//                         g = begin + c draws from live model g % n_live.
// Nothing depends on the grid or on how a range is cut into calls or chunks.
#include <math.h>

#include "tpe_ctpe.hpp"
#include "tpe_draw.hpp"
#include "tpe_points_dev.hpp"

namespace tpe {

constexpr int kCtThreads = 256;  // 4 waves; k_score_points' block

__global__ __launch_bounds__(kCtThreads) void k_ctpe_keys(CtpeKeyArgs A) {
  const int l = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kCtThreads + threadIdx.x;
  bool feas = false;
  if (i < A.n) {
    const double loss = A.losses[i];
    const bool complete = fabs(loss) < INFINITY;
    if (l == 0) {
      feas = complete;
    } else {
      const double g = A.G[(int64_t)A.con[l] * A.ld + i];
      feas = complete && g <= 0.0;
      // pending rows and NaN values sort behind every number, as a pending
      // row does in the loss column
      A.keys[(int64_t)(l - 1) * A.ld + i] = (complete && g == g) ? g : INFINITY;
    }
  }
  const uint64_t mk = __ballot(feas);
  if ((threadIdx.x & 63) == 0 && mk != 0) atomicAdd(A.feas + l, (int32_t)__popcll(mk));
}

// the tables of live position l
__device__ __forceinline__ void ctpe_model(const CtpeArgs &C, int l, PointsArgs &B) {
  if (l > 0) {
    const int64_t slots = 2 * (int64_t)C.P.n_hp;
    B.info = C.bk_info + (int64_t)(l - 1) * slots;
    B.coef = C.bk_coef + (int64_t)(l - 1) * slots * C.P.kcap;
  }
}

// k_score_points with the block's model (blockIdx.z) and its layer of terms
__global__ __launch_bounds__(kCtThreads) void k_ctpe_score(CtpeArgs C) {
  const int hp = blockIdx.y;
  const int l = blockIdx.z;
  const int64_t n = C.P.count[hp];  // block-uniform
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t p0 = (int64_t)blockIdx.x * kCtThreads + wave * 64;
  if (p0 >= n) return;
  PointsArgs A = C.P;
  ctpe_model(C, l, A);
  const int64_t pos = p0 + (threadIdx.x & 63);
  const bool act = pos < n;
  const int64_t c = act ? A.idx[(int64_t)hp * A.m + pos] : 0;
  double *out = A.terms + ((int64_t)l * A.n_hp + hp) * A.term_ld + c;
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

// L = log(ghat + (1 - ghat) exp(-T)) as hi + log1p(exp(lo - hi)) over
// u = log(ghat), v = log1p(-ghat) - T: plain fp64 library calls, nothing
// contracted.  T = +inf gives u, T = -inf gives +inf, a NaN T gives NaN.
__device__ __forceinline__ double ctpe_L(double ghat, double T) {
#pragma clang fp contract(off)
  const double u = log(ghat);
  const double v = log1p(-ghat) - T;
  const bool ug = u > v;
  const double hi = ug ? u : v, lo = ug ? v : u;
  if (hi == INFINITY) return INFINITY;  // (lo - hi would be NaN for lo = +inf)
  return hi + log1p(exp(lo - hi));
}

// acq[c], and T[l][c] where wanted: per live model the terms of configuration
// c added in ascending hp index (an inactive hp adds +0.0: only layer 0 holds
// those stores, so the activity decides), then the models in ascending order
__global__ __launch_bounds__(kCtThreads) void k_ctpe_combine(CtpeArgs C) {
#pragma clang fp contract(off)
  const PointsArgs &A = C.P;
  const int64_t c = (int64_t)blockIdx.x * kCtThreads + threadIdx.x;
  if (c >= A.m) return;
  double acq = 0.0;
  for (int l = 0; l < C.n_live; ++l) {
    const double *tr = A.terms + (int64_t)l * A.n_hp * A.term_ld + c;
    double t = 0.0;
    for (int i = 0; i < A.n_hp; ++i)
      t += A.active[(int64_t)i * A.act_ld + c] ? tr[(int64_t)i * A.term_ld] : 0.0;
    if (C.T) C.T[(int64_t)l * C.t_ld + c] = t;
    acq -= ctpe_L(C.ghat[l], t);
  }
  C.acq[c] = acq;
}

// k_sample_points with the lane's model: configuration g = begin + c takes its
// values from the below mixtures of live position g % n_live.  The draws are
// inline: k_sample_points' out-of-line draw functions call out-of-line helpers
// of their own, and that nested call is what costs it a 16-byte frame; inline,
// every call left is a leaf and the kernel uses no scratch.  FALLBACK false
// (the host has checked that every below mixture fits a table): the table draw
// alone, 138 VGPRs; true: with k_sample_points' rejection sampler for a mixture
// past the table (a constraint whose good side holds more than 2047 rows) --
// the same values for the tables' mixtures, at one wave per SIMD
template <bool FALLBACK>
__global__ __launch_bounds__(kCtThreads) void k_ctpe_sample_points(CtpeSampleArgs S) {
  const PointsArgs &A = S.C.P;
  const int64_t c = (int64_t)blockIdx.x * kCtThreads + threadIdx.x;
  const bool in = c < A.m;
  const int lane = threadIdx.x & 63;
  const uint64_t gi = (uint64_t)(S.begin + c);
  const int l = (int)(gi % (uint64_t)S.C.n_live);
  const int64_t slots = 2 * (int64_t)A.n_hp;
  const int64_t mo = (int64_t)(l - 1) * slots * A.kcap;
  const double *mw = l ? S.bk_mw + mo : S.mw;
  const double *mmu = l ? S.bk_mmu + mo : S.mmu;
  const double *msig = l ? S.bk_msig + mo : S.msig;
  const MixInfo *info = l ? S.C.bk_info + (int64_t)(l - 1) * slots : A.info;
  const DrawTableT<kTabCap> *tab = S.tab + (int64_t)l * A.n_hp;
  for (int j = 0; j < A.n_hp; ++j) {
    const int hp = A.level_hps[j];
    const int c0 = A.hps[hp].cond_begin, nc = A.hps[hp].cond_count;
    bool act = in && nc == 0;
    if (in) {
      for (int q = 0; q < nc && !act; ++q) {
        const int64_t par = A.cond_parent[c0 + q];
        act = A.active[par * A.act_ld + c] != 0 &&
              S.out[par * A.ld + c] == (double)A.cond_branch[c0 + q];
      }
    }
    double x = NAN;
    if (act) {
      const int64_t sb = 2 * (int64_t)hp;
      const double *bmu = mmu + sb * A.kcap, *bsg = msig + sb * A.kcap;
      const int K = info[sb].K;
      if (K >= 1 && K <= kTabCap)
        x = draw_table_from(A.hps[hp], K, bmu, bsg, tab[hp], draw_block0(S.seed, gi, (uint32_t)hp),
                            S.seed, gi, (uint32_t)hp);
      else if (FALLBACK)
        x = draw_one(A.hps[hp], info[sb], mw + sb * A.kcap, bmu, bsg, S.seed, gi, (uint32_t)hp);
    }
    if (in) {
      S.out[(int64_t)hp * A.ld + c] = x;
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

hipError_t launch_ctpe_keys(const CtpeKeyArgs &a, hipStream_t st) {
  if (a.n <= 0 || a.n_live <= 0) return hipSuccess;
  const unsigned gx = (unsigned)((a.n + kCtThreads - 1) / kCtThreads);
  k_ctpe_keys<<<dim3(gx, (unsigned)a.n_live), dim3(kCtThreads), 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_ctpe_score(const CtpeArgs &c, hipStream_t st) {
  const unsigned gx = (unsigned)((c.P.m + kCtThreads - 1) / kCtThreads);
  k_ctpe_score<<<dim3(gx, (unsigned)c.P.n_hp, (unsigned)c.n_live), dim3(kCtThreads), 0, st>>>(c);
  k_ctpe_combine<<<dim3(gx), dim3(kCtThreads), 0, st>>>(c);
  return hipGetLastError();
}

hipError_t launch_ctpe_sample(const CtpeSampleArgs &s, bool fallback, hipStream_t st) {
  const unsigned gx = (unsigned)((s.C.P.m + kCtThreads - 1) / kCtThreads);
  if (fallback) k_ctpe_sample_points<true><<<dim3(gx), dim3(kCtThreads), 0, st>>>(s);
  else k_ctpe_sample_points<false><<<dim3(gx), dim3(kCtThreads), 0, st>>>(s);
  return hipGetLastError();
}

}  // namespace tpe
