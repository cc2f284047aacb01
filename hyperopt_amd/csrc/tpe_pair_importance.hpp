// tpe_pair_importance.hpp -- pairwise (2-D) importances under the group models
// (tpe_pair_importance.hip; tpe_plan_group_importance_pairs): the
// layout of the call's workspace and its launch arguments.  Not part of the ABI.
//
// For a pair (a, b) of hps of one group and side s the pair density on the node
// grid is L_s[i][j] = sum_k w_k kappa_ak(x_a,i) kappa_bk(x_b,j): a G x K x G
// matrix product in fp64, issued as v_mfma_f64_16x16x4_f64.
#pragma once
#include <cstdint>

#include "tpe_importance.hpp"

namespace tpe {

constexpr int kPairThreads = 256;  // 4 waves
constexpr int kPairTile = 64;      // a block's tile of the node grid, 32 x 32 per wave
constexpr int kPairSlab = 16;      // components per LDS slab (4 MFMA steps)
constexpr int kPairLd = kPairTile + 16;  // slab row stride in doubles: rows k and k + 1
                                         // of one MFMA operand fall into different banks
constexpr int32_t kPairMinNodes = 16, kPairMaxNodes = 256;  // a multiple of 16
constexpr int64_t kPairMaxBytes = (int64_t)1 << 30;         // workspace cap of a call

// Workspace of a call, in doubles.  A slot is an hp that some requested pair
// names.  The component capacity of a side is a host-side bound on every
// group's K (group 0 holds every row of the side), padded to the MFMA's k = 4.
struct PairLayout {
  int32_t G, T, n_slot, n_pair;
  int64_t fk[2];    // padded component capacity per side
  int64_t f_side1;  // F: side 0 [n_slot][fk[0]][G], then side 1 [n_slot][fk[1]][G]
  int64_t nodes;    // xs, ws: [n_slot][G] each
  int64_t L;        // [n_pair][2][G][G]
  int64_t zpart;    // [n_pair][2][T * T]
  int64_t dpart;    // [n_pair][T * T]
  int64_t total;
};

inline PairLayout pair_layout(int32_t G, int32_t n_slot, int32_t n_pair, int64_t kb, int64_t ka) {
  PairLayout P{};
  P.G = G;
  P.T = (G + kPairTile - 1) / kPairTile;
  P.n_slot = n_slot;
  P.n_pair = n_pair;
  P.fk[0] = (kb + 3) / 4 * 4;
  P.fk[1] = (ka + 3) / 4 * 4;
  P.f_side1 = (int64_t)n_slot * P.fk[0] * G;
  const int64_t F = (int64_t)n_slot * (P.fk[0] + P.fk[1]) * G;
  const int64_t tiles = (int64_t)P.T * P.T;
  P.nodes = F;
  P.L = P.nodes + 2 * (int64_t)n_slot * G;
  P.zpart = P.L + 2 * (int64_t)n_pair * G * G;
  P.dpart = P.zpart + 2 * (int64_t)n_pair * tiles;
  P.total = P.dpart + (int64_t)n_pair * tiles;
  return P;
}

struct PairArgs {
  // the marginal fit (the node rule's end means) and the group fit
  const tpe_hp *hps;
  const MixInfo *info;        // [2P]
  const double *mmu;          // [2P][kcap]
  const double *pprior;
  const int32_t *group_of_hp; // [P]
  const int32_t *gK;          // [groups][2]
  const double *gw;           // [groups][2][kcap] component weights
  const double *cmu, *csig;   // [P][2][kcap] per hp, component order
  int64_t kcap;
  // the call
  const int32_t *slot_hp;     // [n_slot] ascending hp index
  const int32_t *pair_slot;   // [n_pair][2]
  PairLayout lay;
  double ghat;
  double *ws;                 // the workspace (lay)
  // out
  double *D, *Zb, *Za;        // [n_pair]
  double *xa, *xb;            // [n_pair][G] nullable (NaN past a dim's last node)
  double *logL;               // [n_pair][2][G][G] nullable (NaN past the nodes)
};
// k_pair_factors, k_pair_gemm, k_pair_z, k_pair_div, k_pair_sum in stream order
hipError_t launch_pair_importance(const PairArgs &a, hipStream_t st);

}  // namespace tpe
