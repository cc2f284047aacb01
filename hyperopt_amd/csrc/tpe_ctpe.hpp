// tpe_ctpe.hpp -- c-TPE (tpe_ctpe.hip; tpe_plan_ctpe_*): one pair
// of Parzen models per constraint beside the objective's, scored and drawn
// from together.  Not part of the ABI.
//
// Models are m = 0 (the objective) .. n_con (constraint m - 1).  A model whose
// good side is the whole history is dead: it is not fitted and adds nothing.
// The live ones are numbered by live position l = 0 .. n_live - 1 in ascending
// m; position 0 is always model 0, whose tables are the plan's own fit
// storage.  Positions l >= 1 live in the plan's bank at index l - 1:
//   mw / mmu / msig [n_live - 1][2P][kcap], info [n_live - 1][2P],
//   coef [n_live - 1][2P][kcap], keys [n_live - 1][ncap].
#pragma once
#include "tpe_internal.hpp"

namespace tpe {

constexpr int kCtpeModels = TPE_MAX_CON + 1;

// the key columns of the live constraint models and every live model's count
// of rows on the feasible side (k_ctpe_keys)
struct CtpeKeyArgs {
  const double *G;            // [n_con][ld] the constraint matrix
  const double *losses;       // [n] the loss column: a row is complete when it is finite
  int64_t n, ld;
  int32_t n_live;
  int32_t con[kCtpeModels];   // G row of live position l (l >= 1)
  double *keys;               // [n_live - 1][ld] out
  int32_t *feas;              // [n_live] out (zero before the call): l = 0 the complete rows,
                              // l >= 1 the complete rows with G <= 0
};
hipError_t launch_ctpe_keys(const CtpeKeyArgs &a, hipStream_t st);

// scoring m configurations under every live model, then the acquisition
struct CtpeArgs {
  PointsArgs P;               // model 0's info / coef; terms: [n_live][n_hp][term_ld], of
                              // which k_points_active / k_ctpe_sample_points write layer 0's
                              // inactive +0.0; total unused
  const MixInfo *bk_info;     // the bank
  const Coef *bk_coef;
  int32_t n_live;
  int32_t pad;
  double ghat[kCtpeModels];   // by live position
  double *acq;                // [m] out
  double *T;                  // [n_live][t_ld] out (null: not wanted)
  int64_t t_ld;
};
// k_ctpe_score, k_ctpe_combine (the caller's launch wrote activity and lists)
hipError_t launch_ctpe_score(const CtpeArgs &c, hipStream_t st);

// whole configurations drawn from the live models' below mixtures in turn
struct CtpeSampleArgs {
  CtpeArgs C;                 // C.P.vals == out
  double *out;                // [n_hp][ld] the drawn values (NaN where inactive)
  const double *mw, *mmu, *msig;           // model 0's mixtures
  const double *bk_mw, *bk_mmu, *bk_msig;  // the bank's
  DrawTableT<kTabCap> *tab;   // [n_live][n_hp] draw tables of the below mixtures
  uint64_t seed;
  int64_t begin;              // configuration j of the launch is draw begin + j
};
// k_ctpe_sample_points (values, activity, lists); the caller scores.  fallback:
// some below mixture is past the draw table (the variant with the rejection sampler)
hipError_t launch_ctpe_sample(const CtpeSampleArgs &s, bool fallback, hipStream_t st);

}  // namespace tpe
