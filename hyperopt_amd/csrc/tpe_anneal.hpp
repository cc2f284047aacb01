// tpe_anneal.hpp -- host interface of the annealing kernels (tpe_anneal.hip).
#pragma once
#include "tpe_internal.hpp"

namespace tpe {

// == tpe_anneal_trace (tpe_engine.h)
struct AnnealTrace {
  int32_t row;
  int32_t rank;
  double u[4];
};

constexpr int kAnnealDigitBits = 4;                       // radix of the loss order
constexpr int kAnnealPasses = 64 / kAnnealDigitBits;      // even: the order ends in idx[0]

struct AnnealArgs {
  const tpe_hp *hps;
  int32_t n_hp;
  int32_t n;                  // history rows
  const int32_t *hp_order;    // [P] hp ids in evaluation order (parents first)
  const int32_t *cond_parent;
  const int32_t *cond_branch;
  const double *pprior;
  const double *losses;       // [n]
  const double *vals;         // [P][ld]
  const uint8_t *active;      // [P][ld]
  int64_t ld;
  const int32_t *order;       // [n] rows in ascending (loss, row)
  const int32_t *T;           // [P] rows in which the hp is active
  double p_geo;               // 1 / avg_best_idx
  double log1p_mq;            // log1p(-p_geo) (unused when p_geo >= 1)
  double shrink_coef;
  const uint64_t *seeds;      // [S]
  int32_t n_suggest;
  Partial *results;           // [S][P]
  AnnealTrace *trace;         // [S][P]
};

// order[n] (keys / idx: ping-pong scratch of n entries each, idx[0] == order)
// and T[P] of the history; one block sorts, the others count
hipError_t launch_anneal_order(const double *losses, const uint8_t *active, int64_t ld, int32_t n,
                               int32_t n_hp, uint64_t *keys0, uint64_t *keys1, int32_t *idx0,
                               int32_t *idx1, int32_t *T, hipStream_t st);
// LDS bytes per wave (suggestion) of k_anneal, and its launch
size_t anneal_wave_lds(int32_t n_hp);
hipError_t launch_anneal(const AnnealArgs &a, hipStream_t st);

}  // namespace tpe
