// tpe_hv_plan.hpp -- the launches and buffers of the hypervolume subset
// selection inside the Pareto front, as data.  Pure host code: hv_plan maps
// (n, M, n_pick, S, method) -- history rows, objectives, greedy rounds,
// Monte-Carlo samples per row, estimator -- to the grids of k_hv_init /
// k_hv_round (tpe_hv.hip), the LDS a round block stages its uniforms in and
// the sizes of the per-row state.  What is selected is a
// function of (Y, r, n_pick, S, seed, method) alone; the plan only decides how
// the rows and the sample words are spread over blocks.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "tpe_pareto_plan.hpp"

namespace tpe {

constexpr int kHvTile = 256;          // rows per tile: one row per lane of a block
constexpr int kHvWord = 64;           // samples per alive word
constexpr int kHvMaxPick = 256;       // greedy rounds at most
constexpr int kHvMinSamples = 64;     // S is a multiple of kHvWord in [min, max]
constexpr int kHvMaxSamples = 4096;
constexpr int kHvPickThreads = 1024;  // k_hv_pick: one block strides the rows
constexpr uint32_t kHvStream = 0x60000000u;  // draw4's stream word of the sample table
constexpr size_t kHvLdsLimit = 4 * 1024;     // the staged uniforms, [M][64] doubles
// method: who estimates a row's gain
constexpr int kHvAuto = 0;   // exact when M == 2, Monte-Carlo when M >= 3
constexpr int kHvExact = 1;  // M == 2 only
constexpr int kHvMc = 2;     // any M >= 2

struct HvPlan {
  bool ok = false;       // the arguments are in range
  int64_t n = 0;
  int32_t M = 0;
  int32_t n_pick = 0;
  int32_t S = 0;
  bool exact = false;    // the M == 2 area gain; otherwise the Monte-Carlo count
  int64_t tiles = 0;     // ceil(n / tile): grid.x of k_hv_init / k_hv_round / k_hv_loss
  int64_t words = 0;     // grid.y: S / 64 sample words (1 on the exact path)
  size_t lds_bytes = 0;  // uniforms a round block stages (0 on the exact path)
  size_t u_doubles = 0;  // the sample table u[word][M][64] (0 on the exact path)

  // rows [begin, end) of tile t
  int64_t tile_begin(int64_t t) const { return t * kHvTile; }
  int64_t tile_end(int64_t t) const { return std::min<int64_t>(n, (t + 1) * kHvTile); }
  // samples [begin, end) of word w
  int64_t word_begin(int64_t w) const { return w * kHvWord; }
  int64_t word_end(int64_t w) const { return (w + 1) * kHvWord; }
  // alive words of a plan with row capacity ncap: alive[word][row]
  size_t alive_words(int64_t ncap) const { return exact ? 0 : (size_t)words * (size_t)ncap; }
  // uniform (sample s, objective m) in the table
  size_t u_index(int64_t s, int32_t m) const {
    return ((size_t)(s / kHvWord) * (size_t)M + (size_t)m) * kHvWord + (size_t)(s % kHvWord);
  }
};

inline HvPlan hv_plan(int64_t n, int32_t M, int32_t n_pick, int32_t S, int32_t method) {
  HvPlan p;
  if (n < 1 || n > kParetoMaxN || M < 2 || M > kParetoMaxObj) return p;
  if (n_pick < 1 || n_pick > kHvMaxPick) return p;
  if (S < kHvMinSamples || S > kHvMaxSamples || S % kHvWord != 0) return p;
  if (method != kHvAuto && method != kHvExact && method != kHvMc) return p;
  if (method == kHvExact && M != 2) return p;
  p.n = n;
  p.M = M;
  p.n_pick = n_pick;
  p.S = S;
  p.exact = method == kHvExact || (method == kHvAuto && M == 2);
  p.tiles = (n + kHvTile - 1) / kHvTile;
  p.words = p.exact ? 1 : S / kHvWord;
  p.lds_bytes = p.exact ? 0 : (size_t)M * kHvWord * sizeof(double);
  p.u_doubles = p.exact ? 0 : (size_t)S * (size_t)M;
  p.ok = p.lds_bytes <= kHvLdsLimit;
  return p;
}

}  // namespace tpe
