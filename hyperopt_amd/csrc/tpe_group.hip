// tpe_group.hip -- multivariate TPE over conditional spaces: one joint Parzen
// model per group of hps that are always active together, gfx950
// (tpe_plan_group_*; tpe_group_plan.hpp).
//
// The root model (tpe_joint.hip) is the special case "the group that is always
// active".  Group g's side s holds the rows of the split side in which the
// group is active, in row order; K_gs = n_gs + 1 components, component 0 the
// prior; per dim the kernels are the root model's, so
//   J_gs(c) = logsumexp_k [ log w_k + sum_{d in g} log kappa_{d,k}(c_d) ],
//   joint_g(c) = J_g,below(c) - J_g,above(c),
//   EI(c) = sum over the groups active in c, in group order, of joint_g(c).
// Kernels:
//   k_group_rows    per (group, side): k_joint_rows with the group's history
//                   activity as a further predicate;
//   k_group_dims    per (hp, side): k_joint_dims on its group's rows and S;
//   k_group_active  k_points_active's walk: active[P][m], and per non-root
//                   group the list of its active configurations;
//   k_group_score   blockIdx.y = group: one lane per listed configuration
//                   (group 0: every configuration), k_joint_score's walk;
//   k_group_sum     total = the groups' joint in group order;
//   k_group_tables, k_group_sample   the draw: one component per active
//                   group, every hp of the group from that component.
#include "tpe_joint_dev.hpp"

namespace tpe {

__device__ __forceinline__ int pad_block(int K) {
  return (K + kCoefBlock - 1) / kCoefBlock * kCoefBlock;
}

// ---------------------------------------------------------------- the fit
__global__ __launch_bounds__(kJtThreads) void k_group_rows(GroupFitArgs A) {
  __shared__ double red[kJtThreads];
  __shared__ int wcnt[kJtThreads / 64];
  __shared__ int base;
  const int g = blockIdx.x, side = blockIdx.y;
  const GroupDesc G = A.groups[g];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t gs = (int64_t)g * 2 + side;
  int32_t *rows = A.rows + gs * A.kcap;
  const uint8_t *act = A.active + (int64_t)G.lead * A.ld;
  if (threadIdx.x == 0) { base = 0; rows[0] = -1; }
  __syncthreads();
  // the side's rows in which the group is active, ascending (ordered
  // compaction, 256 rows a step); the roots are active in every row
  for (int64_t j0 = 0; j0 < A.n; j0 += kJtThreads) {
    const int64_t j = j0 + threadIdx.x;
    const bool f = j < A.n && (A.below[j] != 0) == (side == 0) && (g == 0 || act[j] != 0);
    const uint64_t b = __ballot(f);
    if (lane == 0) wcnt[wv] = (int)__popcll(b);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wv; ++w) off += wcnt[w];
    if (f) rows[1 + off + (int)__popcll(b & ((1ull << lane) - 1ull))] = (int32_t)j;
    __syncthreads();
    if (threadIdx.x == 0) base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  const int ns = base, K = ns + 1;
  // weights: prior_weight and the linear-forgetting ramp over the group's rows
  const bool lfw = A.lf && A.lf < ns;
  const LfRamp lr = lf_ramp(ns, A.lf);
  double part = 0.0;
  for (int i = threadIdx.x; i < ns; i += kJtThreads) part += lfw ? lf_weight(lr, i) : 1.0;
  const double tot = jt_block_sum(part, red) + A.prior_weight;
  double *jw = A.jw + gs * A.kcap;
  const int64_t stride = joint_stride(G.n_dim);
  double *tab = A.tab + G.tab_off + side * (A.kcap / kCoefBlock) * stride;
  const int Kp = pad_block(K);
  for (int k = threadIdx.x; k < Kp; k += kJtThreads) {
    double w = 0.0;
    if (k < K) {
      w = (k == 0 ? A.prior_weight : (lfw ? lf_weight(lr, k - 1) : 1.0)) / tot;
      jw[k] = w;
    }
    tab[(int64_t)(k / kCoefBlock) * stride + (k % kCoefBlock)] = k < K ? log2(w) : -INFINITY;
  }
  if (threadIdx.x == 0) {
    A.count[gs] = K;
    A.side[gs] = JointSide{tot, A.prior_weight / tot};
  }
}

__global__ __launch_bounds__(kJtThreads) void k_group_dims(GroupFitArgs A) {
  const int hp = blockIdx.x, side = blockIdx.y;
  const int g = A.group_of_hp[hp];
  const GroupDesc G = A.groups[g];
  const int d = A.dim_of_hp[hp];
  const JointDim D = A.dims[d];
  const tpe_hp H = A.hps[hp];
  const int64_t gs = (int64_t)g * 2 + side;
  const int K = A.count[gs], Kp = pad_block(K);
  const int32_t *rows = A.rows + gs * A.kcap;
  const double *col = A.vals + (int64_t)hp * A.ld;
  const int64_t ds = ((int64_t)hp * 2 + side) * A.kcap;
  double *cw = A.cw + ds, *cmu = A.cmu + ds, *csig = A.csig + ds;
  const int64_t stride = joint_stride(G.n_dim);
  double *tab = A.tab + G.tab_off + side * (A.kcap / kCoefBlock) * stride +
                kCoefBlock * (1 + kJointFields * (int64_t)(d - G.dim_begin));
  auto field = [&](int k, int f) -> double & {
    return tab[(int64_t)(k / kCoefBlock) * stride + f * kCoefBlock + (k % kCoefBlock)];
  };
  if (H.family == TPE_CAT) {
    const double a = joint_cat_a(A.prior_weight, H.upper, A.side[gs].tot);
    const double *jw = A.jw + gs * A.kcap;
    for (int k = threadIdx.x; k < Kp; k += kJtThreads) {
      const double o = (k >= 1 && k < K) ? col[rows[k]] : -1.0;
      field(k, 0) = o;
      field(k, 1) = 0.0;
      field(k, 2) = 0.0;
      if (k < K) { cw[k] = jw[k]; cmu[k] = o; csig[k] = a; }
    }
    double *ol = A.optlog + ((int64_t)side * A.n_opt + D.opt_off) * 3;
    for (int c = threadIdx.x; c < H.upper; c += kJtThreads) {
      const double pi = joint_pi(H, A.pprior, c);
      ol[3 * c + 0] = log2(joint_kappa(true, a, pi));
      ol[3 * c + 1] = log2(joint_kappa(false, a, pi));
      ol[3 * c + 2] = log2(pi);
    }
    return;
  }
  // The hp's marginal fit sorted these rows' transformed observations stably
  // and put the prior at info.probe: row k's place is the number of rows that
  // sort before it, counted on the fit's own sort keys (k_joint_dims).
  const int64_t slot = 2 * (int64_t)hp + side;
  uint64_t *keys = A.keys + ds;
  const double ofloor = obs_floor(H.obs_transform, H.low);
  for (int k = 1 + threadIdx.x; k < K; k += kJtThreads)
    keys[k] = sort_key(obs_transform(col[rows[k]], H.obs_transform, ofloor));
  __syncthreads();
  const int pos0 = A.info[slot].probe;
  const double *mw = A.mw + slot * A.kcap, *mmu = A.mmu + slot * A.kcap,
               *msg = A.msig + slot * A.kcap;
  for (int k = threadIdx.x; k < Kp; k += kJtThreads) {
    Coef c{0.0, 0.0, 0.0, 0.0};
    if (k < K) {
      int pos = pos0;
      if (k >= 1) {
        const uint64_t me = keys[k];
        int rank = 0;
        for (int j = 1; j < K; ++j) {
          const uint64_t o = keys[j];
          rank += (o < me || (o == me && j < k)) ? 1 : 0;
        }
        pos = rank + (rank >= pos0 ? 1 : 0);
      }
      const double mu = mmu[pos], sg = msg[pos];
      cw[k] = mw[pos];
      cmu[k] = mu;
      csig[k] = sg;
      c = make_coef(H, 1.0, mu, sg, 1.0);
      if (H.flags & TPE_HAS_Q) c.z = 0.0;
    }
    field(k, 0) = c.x;
    field(k, 1) = c.y;
    field(k, 2) = c.z;
  }
}

hipError_t launch_group_fit(const GroupFitArgs &a, hipStream_t st) {
  k_group_rows<<<dim3((unsigned)a.n_group, 2), dim3(kJtThreads), 0, st>>>(a);
  k_group_dims<<<dim3((unsigned)a.n_hp, 2), dim3(kJtThreads), 0, st>>>(a);
  return hipGetLastError();
}

// ------------------------------------------------------------- the score
// What the walk does where it reaches a group's lead hp: an active
// configuration joins the group's list, an inactive one gets its +0.0 and NaN
// sides here (k_group_score only visits the list).  Group 0 is active
// everywhere and needs no list.  Called by every lane of the wave.
__device__ __forceinline__ void group_route(const GroupArgs &A, int g, int64_t c, bool in,
                                            bool act, int lane) {
  if (g == 0) return;
  if (in && !act) {
    A.joint[(int64_t)g * A.joint_ld + c] = 0.0;
    A.sides[((int64_t)g * 2 + 0) * A.m + c] = NAN;
    A.sides[((int64_t)g * 2 + 1) * A.m + c] = NAN;
  }
  const uint64_t mk = __ballot(in && act);
  if (mk == 0) return;  // (wave-uniform)
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(A.count + g, (uint32_t)__popcll(mk));
  base = __shfl(base, 0, 64);
  if (in && act)
    A.idx[(int64_t)g * A.m + base + __popcll(mk & ((1ull << lane) - 1ull))] = (int32_t)c;
}

// k_points_active's rule: some (parent, branch) alternative holds with the
// parent active (the parent's row of `active` was written earlier in the walk)
__device__ __forceinline__ bool group_cond(const GroupArgs &A, const double *vals, int hp,
                                           int64_t c) {
  const int c0 = A.hps[hp].cond_begin, nc = A.hps[hp].cond_count;
  bool act = nc == 0;
  for (int q = 0; q < nc && !act; ++q) {
    const int64_t par = A.cond_parent[c0 + q];
    act = A.active[par * A.act_ld + c] != 0 && vals[par * A.ld + c] == (double)A.cond_branch[c0 + q];
  }
  return act;
}

__global__ __launch_bounds__(kJtThreads) void k_group_active(GroupArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kJtThreads + threadIdx.x;
  const bool in = c < A.m;
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < A.n_hp; ++j) {
    const int hp = A.level_hps[j];
    const bool act = in && group_cond(A, A.vals, hp, c);
    if (in) A.active[(int64_t)hp * A.act_ld + c] = act ? 1 : 0;
    const int g = A.group_of_hp[hp];
    if (A.groups[g].lead == hp) group_route(A, g, c, in, act, lane);  // (uniform)
  }
}

// k_joint_score on the group's dims and tables.  One wave a block, one lane per
// configuration of the group's list; the lane's transformed values are staged
// in LDS, [slot][lane] (a lane reads back only its own stores: no barrier).
// A configuration's numbers depend on its own values and the fit alone.
__global__ __launch_bounds__(kJsThreads) void k_group_score(GroupArgs A) {
  extern __shared__ __attribute__((aligned(16))) double stage[];
  const int lane = threadIdx.x;
  const int g = blockIdx.y;
  const int64_t cnt = g == 0 ? A.m : (int64_t)A.count[g];
  const int64_t li = (int64_t)blockIdx.x * kJsThreads + lane;
  if ((int64_t)blockIdx.x * kJsThreads >= cnt) return;  // (block-uniform)
  const bool in = li < cnt;
  const int64_t lj = in ? li : cnt - 1;  // (a lane past the end repeats the last one)
  const int64_t cc = g == 0 ? lj : (int64_t)A.idx[(int64_t)g * A.m + lj];
  const GroupDesc G = A.groups[g];
  const JointDim *dims = A.dims + G.dim_begin;
  double sumlog = 0.0;  // sum of log x over the log-normal dims (lognormal_lpdf's norm)
  bool bad = false;
#pragma unroll 1
  for (int d = 0; d < G.n_dim; ++d) {
    const JointDim D = dims[d];
    const tpe_hp H = A.hps[D.hp];
    const double x = A.vals[(int64_t)D.hp * A.ld + cc];
    double *s = stage + (int64_t)D.slot * kJsThreads + lane;
    bad |= x != x;
    switch (D.kind) {
      case KIND_LSE_G: s[0] = x - H.prior_mu; break;
      case KIND_LSE_L: {
        const double lx = fast_log(x);
        s[0] = lx - H.prior_mu;
        sumlog += lx;
        break;
      }
      case KIND_ERF_G: {
        double ub, lb;
        quant_bounds<false>(H, x, ub, lb);
        s[0] = ub; s[kJsThreads] = lb;
        break;
      }
      case KIND_ERF_L: {
        double ub, lb;
        quant_bounds<true>(H, x, ub, lb);
        s[0] = ub; s[kJsThreads] = lb;
        break;
      }
      default: {
        // an option index in [0, upper), else NaN (k_points_active's rule)
        bool ok = x >= 0.0 && x < (double)H.upper;
        const int64_t o = ok ? (int64_t)x : 0;
        ok = ok && (double)o == x;
        bad |= !ok;
        s[0] = (double)o;
        s[kJsThreads] = s[2 * kJsThreads] = s[3 * kJsThreads] = NAN;
        break;
      }
    }
  }
  const int64_t stride = joint_stride(G.n_dim);
  const int64_t tab_side = (A.kcap / kCoefBlock) * stride;
  const double LN2 = 0.6931471805599453;
  double J[2];
#pragma unroll 1
  for (int side = 0; side < 2; ++side) {
    // the option logs of this side for the categorical dims
#pragma unroll 1
    for (int d = 0; d < G.n_dim; ++d) {
      const JointDim D = dims[d];
      if (D.kind != KIND_CAT) continue;
      double *s = stage + (int64_t)D.slot * kJsThreads + lane;
      const double *ol = A.optlog + ((int64_t)side * A.n_opt + D.opt_off + (int64_t)s[0]) * 3;
      s[kJsThreads] = ol[0];
      s[2 * kJsThreads] = ol[1];
      s[3 * kJsThreads] = ol[2];
    }
    const int K = __builtin_amdgcn_readfirstlane(A.K[g * 2 + side]);
    KDbl *tab = joint_uniform(A.tab + G.tab_off + side * tab_side);
    double m[1] = {-INFINITY}, sum[1] = {0.0};
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += kGroup) {
      KDbl *blk = tab + (int64_t)(k0 / kGroup) * stride;
      double t[1][kGroup];
#pragma unroll
      for (int j = 0; j < kGroup; ++j) t[0][j] = blk[j];
#pragma unroll 1
      for (int d = 0; d < G.n_dim; ++d) {
        const JointDim D = dims[d];
        KDbl *f = blk + kCoefBlock * (1 + kJointFields * (int64_t)d);
        const double *s = stage + (int64_t)D.slot * kJsThreads + lane;
        switch (D.kind) {  // (wave-uniform)
          case KIND_LSE_G:
          case KIND_LSE_L: {
            const double y = s[0], y2 = y * y;
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
              t[0][j] += fma(f[2 * kCoefBlock + j], y2, fma(f[kCoefBlock + j], y, f[j]));
            break;
          }
          case KIND_ERF_G: joint_erf<false>(f, s[0], s[kJsThreads], t); break;
          case KIND_ERF_L: joint_erf<true>(f, s[0], s[kJsThreads], t); break;
          default: {
            const double o = s[0], hit = s[kJsThreads], miss = s[2 * kJsThreads],
                         pri = s[3 * kJsThreads];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
              const double ok = f[j];
              t[0][j] += ok < 0.0 ? pri : (ok == o ? hit : miss);
            }
            break;
          }
        }
      }
      lse_fold<1>(t, m, sum);
    }
    // (score_points' finalize: a NaN value or no finite term scores NaN)
    J[side] = (bad || m[0] == -INFINITY) ? NAN : (m[0] + log2(sum[0])) * LN2 - sumlog;
  }
  if (in) {
    A.sides[((int64_t)g * 2 + 0) * A.m + cc] = J[0];
    A.sides[((int64_t)g * 2 + 1) * A.m + cc] = J[1];
    A.joint[(int64_t)g * A.joint_ld + cc] = J[0] - J[1];
  }
}

// total[c] = the groups' joint of configuration c in ascending group order
// (an inactive group's entry is +0.0)
__global__ __launch_bounds__(kJtThreads) void k_group_sum(GroupArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kJtThreads + threadIdx.x;
  if (c >= A.m) return;
  double t = 0.0;
  for (int g = 0; g < A.n_group; ++g) t += A.joint[(int64_t)g * A.joint_ld + c];
  A.total[c] = t;
}

hipError_t launch_group_points(const GroupArgs &a, bool walk, hipStream_t st) {
  const unsigned gx = (unsigned)((a.m + kJtThreads - 1) / kJtThreads);
  if (walk) k_group_active<<<dim3(gx), dim3(kJtThreads), 0, st>>>(a);
  const unsigned gs = (unsigned)((a.m + kJsThreads - 1) / kJsThreads);
  const size_t lds = (size_t)(a.max_slots > 0 ? a.max_slots : 1) * kJsThreads * sizeof(double);
  hipError_t e = hipSuccess;
  if (lds > 48 * 1024)  // (beyond the default dynamic limit)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_group_score),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  k_group_score<<<dim3(gs, (unsigned)a.n_group), dim3(kJsThreads), lds, st>>>(a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_group_sum<<<dim3(gx), dim3(kJtThreads), 0, st>>>(a);
  return hipGetLastError();
}

// --------------------------------------------------------------- the draw
// Tables of one call, 256 threads a block (block_inclusive_scan's addition
// order depends on the block size, and the CDFs must be tpe_sample's bits):
//   block hp < P      a continuous hp: the truncation constants of its group's
//                     below components (each a one-component mixture: base,
//                     mass and mode do not depend on the weight); a
//                     categorical hp: per component the CDF of its kappa vector;
//   block P + g       the CDF of group g's below component weights.
__global__ __launch_bounds__(kJtThreads) void k_group_tables(GroupArgs A) {
  __shared__ DrawTable T;
  const int b = blockIdx.x;
  if (b >= A.n_hp) {
    const int g = b - A.n_hp;
    const int Kb = A.K[g * 2];
    const double *jw = A.jw + (int64_t)g * 2 * A.kcap;
    double *cdf = A.pick_cdf + (int64_t)g * A.kcap;
    for (int k = threadIdx.x; k < Kb; k += kJtThreads) cdf[k] = jw[k];
    __syncthreads();
    block_inclusive_scan(cdf, Kb, T.wtot);
    return;
  }
  const int hp = b, g = A.group_of_hp[hp];
  const tpe_hp H = A.hps[hp];
  const int Kb = A.K[g * 2];
  const int64_t ds = (int64_t)hp * 2 * A.kcap;  // side 0
  if (H.family != TPE_CAT) {
    DrawTable &Gt = A.dtab[hp];
    build_table(H, Kb, A.jw + (int64_t)g * 2 * A.kcap, A.cmu + ds, A.csig + ds, T);
    for (int k = threadIdx.x; k < Kb; k += kJtThreads) {
      Gt.base[k] = T.base[k];
      Gt.mass[k] = T.mass[k];
      Gt.mode[k] = T.mode[k];
    }
    return;
  }
  const JointDim D = A.dims[A.dim_of_hp[hp]];
  const double a = joint_cat_a(A.prior_weight, H.upper, A.side[g * 2].tot);
  for (int k = 0; k < Kb; ++k) {
    double *cdf = A.opt_cdf + D.opt_off * A.kb_max + (int64_t)k * H.upper;
    const double o = A.cmu[ds + k];
    for (int c = threadIdx.x; c < H.upper; c += kJtThreads) {
      const double pi = joint_pi(H, A.pprior, c);
      cdf[c] = k == 0 ? pi : joint_kappa((double)c == o, a, pi);
    }
    __syncthreads();
    block_inclusive_scan(cdf, H.upper, T.wtot);
  }
}

// k_joint_sample's walk with every group drawn as the roots are: the group's
// component is picked where the walk reaches its lead hp
__global__ __launch_bounds__(kJtThreads) void k_group_sample(GroupArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kJtThreads + threadIdx.x;
  const bool in = c < A.m;
  const int lane = threadIdx.x & 63;
  const uint64_t gi = (uint64_t)(A.begin + c);
  for (int j = 0; j < A.n_hp; ++j) {
    const int hp = A.level_hps[j];
    const int g = A.group_of_hp[hp];
    const bool act = in && group_cond(A, A.out, hp, c);
    int32_t *cp = A.comp + (int64_t)g * A.comp_ld + c;
    int comp = -1;
    if (A.groups[g].lead == hp) {  // (uniform)
      if (act) {
        const U4 r0 = draw_block0(A.seed, gi, kJointStream | (uint32_t)(A.n_hp + g));
        comp = pick_cdf(A.pick_cdf + (int64_t)g * A.kcap, A.K[g * 2], u53(r0.x, r0.y));
      }
      if (in) *cp = comp;
      group_route(A, g, c, in, act, lane);
    } else if (act) {
      comp = *cp;
    }
    double x = NAN;
    if (act) {
      const uint32_t stream = kJointStream | (uint32_t)hp;
      const U4 r0 = draw_block0(A.seed, gi, stream);
      const tpe_hp H = A.hps[hp];
      if (H.family == TPE_CAT) {
        const double *cdf = A.opt_cdf + A.dims[A.dim_of_hp[hp]].opt_off * A.kb_max +
                            (int64_t)comp * H.upper;
        x = (double)pick_cdf(cdf, H.upper, u53(r0.x, r0.y));
      } else {
        const int64_t ds = (int64_t)hp * 2 * A.kcap;
        x = draw_table_value<kTabCap>(H, comp, A.cmu + ds, A.csig + ds, A.dtab[hp],
                                      u53(r0.z, r0.w), A.seed, gi, stream);
      }
    }
    if (in) {
      A.out[(int64_t)hp * A.ld + c] = x;
      A.active[(int64_t)hp * A.act_ld + c] = act ? 1 : 0;
    }
  }
}

hipError_t launch_group_sample(const GroupArgs &a, hipStream_t st) {
  const unsigned gx = (unsigned)((a.m + kJtThreads - 1) / kJtThreads);
  k_group_tables<<<dim3((unsigned)(a.n_hp + a.n_group)), dim3(kJtThreads), 0, st>>>(a);
  k_group_sample<<<dim3(gx), dim3(kJtThreads), 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace tpe
