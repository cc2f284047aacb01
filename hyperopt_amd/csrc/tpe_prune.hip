// tpe_prune.hip -- the pruning sorted draw in a
// translation unit of its own: the draw kernels of tpe_kernels.hip keep their
// code and register allocation.
#include <math.h>

#include "tpe_draw.hpp"
#include "tpe_internal.hpp"

namespace tpe {

// (k_draw_sorted_fast's block: 512 threads, two blocks per CU by LDS)
constexpr int kPruneThreads = 512;

// The sort blocks behind the first of a tab_on 1 launch with the prefilter
// (launch_draw_pruned): block x draws sort block x + 1 and drops the wave
// tiles the slot's hot intervals rule out before they are ranked or written
// (sorted_block_prune_body).  Sort block 0 -- the pilot's, written in full by
// k_draw_sorted_fast ahead of k_table_pilot -- gets its "pending" marks from
// block 0 here, so that no entry of the launch's tab_wmax rows is stale.
// (FAST: every drawn slot is a bounded continuous one with a table, as
// k_draw_sorted_fast; otherwise k_draw_sorted's out-of-line draws are compiled
// in for the other slots, with that kernel's occupancy hint)
template <int CAP, bool FAST>
__global__ __launch_bounds__(kPruneThreads)
__attribute__((amdgpu_waves_per_eu(CAP <= kFuseTab ? (FAST ? 4 : 2) : 1)))
void k_draw_sorted_prune(ScoreArgs A, int32_t *__restrict__ pos_out) {
  __shared__ PruneDrawLds<CAP, kPruneThreads> L;
  const int s = blockIdx.z;
  const int slot = row_slot(A, s, 0, A.n_slots, blockIdx.y);
  if (slot < 0) return;
  const int hp = A.level_hps[slot];
  if (!A.force_active && !A.compact &&
      !hp_active(A.hps[hp], A.results + (int64_t)s * A.n_hp, A.cond_parent, A.cond_branch))
    return;
  const int kind = slot_kind(A, slot);
  if ((kind == KIND_CAT || kind == KIND_LAT) && lookup_inline(A, A.info[2 * hp].K)) return;
  const bool tabk = kind == KIND_LSE_GW || kind == KIND_LSE_LW;
  if (tabk && blockIdx.x == 0 && threadIdx.x < (1 << A.sort_log2) / 128 &&
      (int64_t)threadIdx.x * 128 < A.n_cand)
    A.tab_wmax[((int64_t)s * A.n_hp + hp) * A.pstride * 8 + threadIdx.x] = INFINITY;
  sorted_block_prune_body<CAP, kPruneThreads, FAST>(
      A, slot, s, (int64_t)(blockIdx.x + 1) << A.sort_log2,
      kind_lse(kind) || kind == KIND_ERF_G || kind == KIND_ERF_L, kind_logn(kind), tabk, pos_out,
      L);
}

bool is_prune_draw_kernel_fn(const void *f) {
  return f == reinterpret_cast<const void *>(&k_draw_sorted_prune<kFuseTab, true>) ||
         f == reinterpret_cast<const void *>(&k_draw_sorted_prune<kTabCap, true>) ||
         f == reinterpret_cast<const void *>(&k_draw_sorted_prune<kFuseTab, false>) ||
         f == reinterpret_cast<const void *>(&k_draw_sorted_prune<kTabCap, false>) ||
         is_screen_draw_kernel_fn(f);
}

hipError_t launch_draw_pruned(const ScoreArgs &a, bool small_table, bool fast, int32_t *pos_out,
                              hipStream_t st) {
  const int64_t sbk = (int64_t)1 << a.sort_log2;
  if (a.n_slots <= 0 || a.n_suggest <= 0 || a.n_cand <= sbk) return hipSuccess;
  if (sbk != kSortedBlock || !a.tab_wmax || !a.tab_hot || !a.tab_hdr) return hipErrorInvalidValue;
  const dim3 g((unsigned)((a.n_cand + sbk - 1) / sbk - 1), (unsigned)a.slot_rows, a.n_suggest);
  if (fast) {
    if (small_table) k_draw_sorted_prune<kFuseTab, true><<<g, kPruneThreads, 0, st>>>(a, pos_out);
    else k_draw_sorted_prune<kTabCap, true><<<g, kPruneThreads, 0, st>>>(a, pos_out);
  } else {
    if (small_table) k_draw_sorted_prune<kFuseTab, false><<<g, kPruneThreads, 0, st>>>(a, pos_out);
    else k_draw_sorted_prune<kTabCap, false><<<g, kPruneThreads, 0, st>>>(a, pos_out);
  }
  return hipGetLastError();
}

}  // namespace tpe
