// tpe_sample_points.hip -- whole configurations drawn from the fitted below
// mixtures, gfx950 (tpe_plan_sample_points).
//
// Configuration c takes, hp by hp in level order (parents first), the value
// tpe_sample returns for that hp's below mixture with Philox key `seed`,
// stream hp and offset c -- where the hp is active under the values the
// configuration has drawn so far -- and NaN elsewhere.  Two launches ahead of
// tpe_points.hip's k_score_points and k_points_sum:
//   k_sample_tables  one block per hp builds the below mixture's draw table
//                    (tpe_draw.hpp build_table) in LDS with k_sample's 256
//                    threads -- block_inclusive_scan's addition order depends
//                    on blockDim.x once K > blockDim.x, so the CDF is
//                    k_sample's bit for bit -- and copies it to global memory;
//   k_sample_points  one thread per configuration walks the hps: activity
//                    (k_points_active's rule, from its own stores), the draw
//                    through the out-of-line draw_table_from / draw_one, the
//                    value or NaN, the +0.0 term of an inactive pair, and each
//                    hp's compacted list (per-wave ballot, one atomic add per
//                    wave and hp) for k_score_points.
// The tables are built once per call and read by every block: a draw is one
// binary search and three loads of an L2-resident table.  A draw depends on
// (seed, hp, c) only, so any split of a range of configurations into calls
// gives the same numbers.
#include <math.h>

#include "tpe_draw.hpp"

namespace tpe {

constexpr int kSpThreads = 256;  // k_sample's block: the table's scan order

__global__ __launch_bounds__(kSpThreads) void k_sample_tables(SampleArgs S) {
  __shared__ DrawTable T;
  const int hp = blockIdx.x;
  const int64_t sb = 2 * (int64_t)hp;
  const int K = S.P.info[sb].K;
  if (K < 1 || K > kTabCap) return;  // (block-uniform: draw_one takes the hp)
  const tpe_hp H = S.P.hps[hp];
  build_table(H, K, S.mw + sb * S.P.kcap, S.mmu + sb * S.P.kcap, S.msig + sb * S.P.kcap, T);
  DrawTable &G = S.tab[hp];
  for (int k = threadIdx.x; k < K; k += kSpThreads) {
    G.cdf[k] = T.cdf[k];
    G.base[k] = T.base[k];
    G.mass[k] = T.mass[k];
    G.mode[k] = T.mode[k];
  }
}

__global__ __launch_bounds__(kSpThreads) void k_sample_points(SampleArgs S) {
  const PointsArgs &A = S.P;
  const int64_t c = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
  const bool in = c < A.m;
  const int lane = threadIdx.x & 63;
  const uint64_t gi = (uint64_t)(S.begin + c);
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
      const double *bmu = S.mmu + sb * A.kcap, *bsg = S.msig + sb * A.kcap;
      const int K = A.info[sb].K;
      x = (K >= 1 && K <= kTabCap)
              ? draw_table_ool<kTabCap>(A.hps + hp, K, bmu, bsg, S.tab + hp,
                                        draw_block0(S.seed, gi, (uint32_t)hp), S.seed, gi,
                                        (uint32_t)hp)
              : draw_one_ool(A.hps + hp, A.info + sb, S.mw + sb * A.kcap, bmu, bsg, S.seed, gi,
                             (uint32_t)hp);
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

size_t sample_tables_bytes(int32_t n_hp) { return (size_t)n_hp * sizeof(DrawTable); }

hipError_t launch_sample_points(const SampleArgs &s, hipStream_t st) {
  const unsigned gx = (unsigned)((s.P.m + kSpThreads - 1) / kSpThreads);
  k_sample_tables<<<dim3((unsigned)s.P.n_hp), dim3(kSpThreads), 0, st>>>(s);
  k_sample_points<<<dim3(gx), dim3(kSpThreads), 0, st>>>(s);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : launch_points_score(s.P, st);
}

}  // namespace tpe
