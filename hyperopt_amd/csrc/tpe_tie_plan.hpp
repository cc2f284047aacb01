// tpe_tie_plan.hpp -- what launch_class decides on the host for the direct pass
// behind the Chebyshev tables: which kernel scores the gathered
// blocks, and on how many persistent blocks per slot.  Plain C++, host only:
// tests/host/tie_plan_check.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>

#include "tpe_internal.hpp"

namespace tpe {

// k_score_wave_tie's persistent blocks per CU.  Config 4, ms per step at
// 4 / 6 / 8 / 12 / 16 / 32: 26.86 / 26.52 / 26.44 / 26.33 / 26.29 / 26.29, two
// rounds within 0.07 ms of each other (profiles/tiegather_blocks_sweep.txt)
constexpr int kTieBlocksPerCu = 16;
// ... and k_score_wave_tie_lean's, whose blocks run two to a CU: 4 / 8 / 16 /
// 32 swept again for it
constexpr int kTieLeanBlocksPerCu = 32;

// The form k_score_wave_tie_lean is compiled for -- what a suggest's tab_on 1
// launch always has: prune mode 3 on the 16-wide moment tables, bucketed
// candidates with their positions, the score alone, no L2 warm-up.  Any other
// launch, and the switch off, keep k_score_wave_tie.
inline bool tie_lean_form(bool tie_lean_switch, const ScoreArgs &a) {
  return tie_lean_switch && a.lse_prune == 3 && a.lse_mom == 16 && a.lse_pos && a.cand_pos &&
         !a.out_lb && !a.out_la && !a.l2_warm;
}

// Persistent blocks per slot (grid x): ~blocks-per-CU blocks per CU over the
// launch's (row, suggestion) pairs, so that a single all-hot slot still fills
// the chip; never more than a slot has gathered blocks (ntmax), at least one
inline unsigned tie_grid(bool lean, int64_t rows, int64_t n_suggest, int64_t ntmax) {
  const int64_t pairs = rows * n_suggest;
  const int64_t per = ((int64_t)(lean ? kTieLeanBlocksPerCu : kTieBlocksPerCu) * kNumCUs + pairs - 1) /
                      pairs;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ntmax, per));
}

}  // namespace tpe
