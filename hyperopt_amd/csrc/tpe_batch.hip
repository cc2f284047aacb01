// tpe_batch.hip -- a batch of k configurations for parallel workers, picked
// greedily under the group models with a pending-trial penalty, gfx950
// (tpe_plan_group_batch_points).
//
// The input is the m configurations and the per-group sides J_g,below,
// J_g,above of the plan's last group score or draw.  Round t scores every
// configuration, score_t(c) = the float64 sum in group order from +0.0 of
// J_g,below(c) - Ja_g(c) over the groups active in c (k_group_sum's operation
// order: score_0 is the call's total), and picks the first selectable one in
// tpe.rank_pool's order, the configurations equal to a taken one last.  The
// pick then counts as a bad trial that is out for evaluation: every group g
// active in it gets one more above component of unnormalised weight 1,
//   Ja_g(c) <- logaddexp(Ja_g(c) + log(W_g + n_g), sum_{d in g} log kappa_d(c_d; p_d))
//              - log(W_g + n_g + 1),
// W_g = S_g,above + prior_weight, n_g the earlier picks that activated g; the
// kernel kappa_d is the one a refit would give the pick's value appended to
// the hp's above observations, every fitted component frozen.
// Kernels:
//   k_batch_init   Ja = J_above, the groups' activity, the state bytes;
//   k_batch_round  one lane per configuration: the previous pick's component
//                  joins Ja of the shared active groups, equality with the
//                  pick is marked, score_t is formed and the block's best
//                  (tier, key, ~index) goes to the block's slot;
//   k_batch_pick   one block: the best slot is the pick; its record for the
//                  next round -- per hp of an active group the value and the
//                  pending kernel (one sigma search in the hp's sorted above
//                  mixture per continuous hp).
// 2k + 1 launches, none cooperative; every comparison is on integers, there is
// no floating-point atomic, and a configuration's Ja depends on its own values
// and the picks alone.
#include "tpe_joint_dev.hpp"

namespace tpe {

__device__ __forceinline__ bool slot_less(const BatchSlot &a, const BatchSlot &b) {
  if (a.tier != b.tier) return a.tier < b.tier;
  if (a.key != b.key) return a.key < b.key;
  return a.nidx < b.nidx;
}

// the block's largest slot, in every thread (kBtThreads threads)
__device__ __forceinline__ BatchSlot block_best(BatchSlot v, BatchSlot *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = kBtThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w && slot_less(red[threadIdx.x], red[threadIdx.x + w]))
      red[threadIdx.x] = red[threadIdx.x + w];
    __syncthreads();
  }
  const BatchSlot r = red[0];
  __syncthreads();
  return r;
}

// _row_keys' equality of two values: their bits, the sign of zero ignored
__device__ __forceinline__ bool same_value(double a, double b) {
  return __double_as_longlong(a + 0.0) == __double_as_longlong(b + 0.0);
}

__device__ __forceinline__ double log_add_exp(double a, double b) {
  if (a == b) return a + 0.6931471805599453;  // (also both -inf or both +inf)
  const double hi = fmax(a, b);               // (a NaN operand gives NaN below)
  return hi + log1p(exp(-fabs(a - b)));
}

// log kappa_d(x; the pick) from the pick's record r of the hp, DimFit.log_kernel's
// forms; NaN for a value the group score rejects as well
__device__ __forceinline__ double pending_log_kernel(const BatchArgs &A, const JointDim &D,
                                                     const tpe_hp &H, double x, const double *r) {
  switch (D.kind) {
    case KIND_LSE_G: {
      const double z = (x - r[1]) * r[2];
      return -0.5 * (z * z) - r[3];
    }
    case KIND_LSE_L: {
      const double lx = log(x);
      const double z = (lx - r[1]) * r[2];
      return -0.5 * (z * z) - r[3] - lx;
    }
    case KIND_ERF_G: {
      double ub, lb;
      quant_bounds<false>(H, x, ub, lb);
      return log(erf_term<false>((ub - r[1]) * r[2], (lb - r[1]) * r[2], 1.0));
    }
    case KIND_ERF_L: {
      double ub, lb;
      quant_bounds<true>(H, x, ub, lb);
      return log(erf_term<true>((ub - r[1]) * r[2], (lb - r[1]) * r[2], 1.0));
    }
    default: {
      // an option index in [0, upper) (k_group_score's rule), else no table entry
      bool ok = x >= 0.0 && x < (double)H.upper;
      const int64_t o = ok ? (int64_t)x : 0;
      ok = ok && (double)o == x;
      if (!ok) return NAN;
      // the above side's log2 kappa of the option: hit, miss
      const double *ol = A.optlog + (A.n_opt + D.opt_off + o) * 3;
      return 0.6931471805599453 * (x == r[0] ? ol[0] : ol[1]);
    }
  }
}

__global__ __launch_bounds__(kBtThreads) void k_batch_init(BatchArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kBtThreads + threadIdx.x;
  if (c >= A.m) return;
  A.state[c] = (!A.eligible || A.eligible[c]) ? 1 : 0;
  // k_group_active's walk, per group at its lead hp: some (parent, branch)
  // alternative holds with the parent's group active
  for (int j = 0; j < A.n_hp; ++j) {
    const int hp = A.level_hps[j];
    const int g = A.group_of_hp[hp];
    if (A.groups[g].lead != hp) continue;
    const int c0 = A.hps[hp].cond_begin, nc = A.hps[hp].cond_count;
    bool act = nc == 0;
    for (int q = 0; q < nc && !act; ++q) {
      const int64_t par = A.cond_parent[c0 + q];
      act = A.gact[(int64_t)A.group_of_hp[par] * A.m + c] != 0 &&
            A.vals[par * A.ld + c] == (double)A.cond_branch[c0 + q];
    }
    A.gact[(int64_t)g * A.m + c] = act ? 1 : 0;
  }
  for (int g = 0; g < A.n_group; ++g)
    A.ja[(int64_t)g * A.m + c] = A.sides[((int64_t)g * 2 + 1) * A.m + c];
}

__global__ __launch_bounds__(kBtThreads) void k_batch_round(BatchArgs A, int t) {
  __shared__ BatchSlot red[kBtThreads];
  const BatchHdr hdr = *A.hdr;
  if (hdr.is_short) return;  // (uniform over the grid: the later rounds do nothing)
  const int64_t c = (int64_t)blockIdx.x * kBtThreads + threadIdx.x;
  BatchSlot mine{0ull, 0u, 0u};
  if (c < A.m) {
    uint8_t st = A.state[c];
    bool same = t > 0;  // equal to the previous pick, so far
    double sc = 0.0;
    for (int g = 0; g < A.n_group; ++g) {
      const bool ac = A.gact[(int64_t)g * A.m + c] != 0;
      const bool ap = t > 0 && A.pact[g] != 0;
      same = same && ac == ap;
      if (!ac) {
        sc += 0.0;
        continue;
      }
      double ja = A.ja[(int64_t)g * A.m + c];
      if (ap) {
        const GroupDesc G = A.groups[g];
        double lk = 0.0;
        for (int d = 0; d < G.n_dim; ++d) {
          const JointDim D = A.dims[G.dim_begin + d];
          const double x = A.vals[(int64_t)D.hp * A.ld + c];
          const double *r = A.rec + (int64_t)D.hp * kBatchRec;
          same = same && same_value(x, r[0]);
          lk += pending_log_kernel(A, D, A.hps[D.hp], x, r);
        }
        const double W = A.side[g * 2 + 1].tot + (double)A.ng[g];
        ja = log_add_exp(ja + log(W), lk) - log(W + 1.0);
        A.ja[(int64_t)g * A.m + c] = ja;
      }
      sc += A.sides[(int64_t)g * 2 * A.m + c] - ja;
    }
    if (same) st |= c == (int64_t)hdr.pick ? 2 : 4;
    A.state[c] = st;
    A.score[(int64_t)t * A.score_ld + c] = sc;
    const bool sel = (st & 1) && !(st & 2);
    mine.tier = sel ? ((st & 4) ? 1u : 2u) : 0u;
    mine.key = topk_key(sc);
    mine.nidx = ~(uint32_t)c;
  }
  const BatchSlot best = block_best(mine, red);
  if (threadIdx.x == 0) A.slot[blockIdx.x] = best;
}

// the pick's record of a continuous hp: the kernel a refit would give the
// value appended to the hp's above observations.  In the sorted above
// mixture (the prior in it) the left neighbour is the last mu_k <= mu, the
// right one the first mu_k > mu: sigma = the larger gap (one-sided at an
// end), clipped to [prior_sigma / min(100, 2 + K), prior_sigma]; the prior
// alone: prior_sigma / 2.
__device__ __forceinline__ void pending_record(const BatchArgs &A, int hp, const tpe_hp &H,
                                               double x, double *r) {
#pragma clang fp contract(off)
  const double mu = obs_transform(x, H.obs_transform, obs_floor(H.obs_transform, H.low));
  const int64_t slot = 2 * (int64_t)hp + 1;
  const int K = A.info[slot].K;
  const double *mus = A.mmu + slot * A.kcap;
  double sigma = 0.5 * H.prior_sigma;
  if (K > 1) {
    int lo = 0, hi = K;  // the number of mu_k <= mu
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (mus[mid] <= mu) lo = mid + 1; else hi = mid;
    }
    const double gl = lo > 0 ? mu - mus[lo - 1] : -INFINITY;
    const double gr = lo < K ? mus[lo] - mu : -INFINITY;
    sigma = np_maximum(gl, gr);
    const double fl = H.prior_sigma / fmin(100.0, 2.0 + (double)K);
    sigma = np_minimum(np_maximum(sigma, fl), H.prior_sigma);
  }
  r[1] = mu;
  if (H.flags & TPE_HAS_Q) {
    r[2] = 1.0 / np_maximum(1.4142135623730951 * sigma, kEPS);
    r[3] = 0.0;
  } else if (H.family == TPE_GMM) {
    r[2] = 1.0 / np_maximum(sigma, kEPS);
    r[3] = log(sqrt(2.0 * 3.141592653589793 * (sigma * sigma)));
  } else {
    const double sp = np_maximum(sigma, kEPS);
    r[2] = 1.0 / sp;
    r[3] = log(sp * 2.5066282746310002);
  }
}

__global__ __launch_bounds__(kBtThreads) void k_batch_pick(BatchArgs A, int t, int n_slot) {
  __shared__ BatchSlot red[kBtThreads];
  if (A.hdr->is_short) {
    if (threadIdx.x == 0) { A.idx[t] = -1; A.gain[t] = NAN; }
    return;
  }
  BatchSlot mine{0ull, 0u, 0u};
  for (int i = threadIdx.x; i < n_slot; i += kBtThreads) {
    const BatchSlot s = A.slot[i];
    if (slot_less(mine, s)) mine = s;
  }
  const BatchSlot best = block_best(mine, red);
  if (best.tier == 0u) {  // no selectable configuration left: the batch is short
    if (threadIdx.x == 0) { A.idx[t] = -1; A.gain[t] = NAN; A.hdr->is_short = 1; }
    return;
  }
  const int64_t p = (int64_t)~best.nidx;  // (< m: only lanes inside the draw carry a tier)
  if (threadIdx.x == 0) {
    A.idx[t] = (int32_t)p;
    A.gain[t] = A.score[(int64_t)t * A.score_ld + p];
    A.state[p] |= 2;
    A.hdr->pick = (int32_t)p;
  }
  for (int g = threadIdx.x; g < A.n_group; g += kBtThreads) {
    if (A.pact[g]) A.ng[g] += 1;
    A.pact[g] = A.gact[(int64_t)g * A.m + p];
  }
  for (int hp = threadIdx.x; hp < A.n_hp; hp += kBtThreads) {
    if (!A.gact[(int64_t)A.group_of_hp[hp] * A.m + p]) continue;
    const tpe_hp H = A.hps[hp];
    const double x = A.vals[(int64_t)hp * A.ld + p];
    double *r = A.rec + (int64_t)hp * kBatchRec;
    r[0] = x;
    if (H.family == TPE_CAT) r[1] = r[2] = r[3] = 0.0;
    else pending_record(A, hp, H, x, r);
  }
}

hipError_t launch_group_batch(const BatchArgs &a, hipStream_t st) {
  const unsigned gx = (unsigned)((a.m + kBtThreads - 1) / kBtThreads);
  k_batch_init<<<dim3(gx), dim3(kBtThreads), 0, st>>>(a);
  hipError_t e = hipGetLastError();
  for (int t = 0; t < a.k && e == hipSuccess; ++t) {
    k_batch_round<<<dim3(gx), dim3(kBtThreads), 0, st>>>(a, t);
    k_batch_pick<<<dim3(1), dim3(kBtThreads), 0, st>>>(a, t, (int)gx);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace tpe
