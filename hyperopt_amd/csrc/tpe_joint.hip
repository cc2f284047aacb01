// tpe_joint.hip -- multivariate TPE: a joint Parzen model over the root
// (unconditional) hps, gfx950 (tpe_plan_joint_*).
//
// The marginal model scores a configuration hp by hp, so an interaction
// between two hps is invisible to it.  Here each side of the split is one
// mixture over whole rows: component 0 is the prior, component k the side's
// k-th row, and a component's density is the product over the root hps of the
// kernel the marginal fit gave that row's observation -- the multiset of
// (w, mu, sigma) per hp is the marginal mixture, the joint model only keeps
// which row owns which component.
//   J_s(c) = logsumexp_k [ log w_k + sum_d log kappa_{d,k}(c_d) ],
//   joint(c) = J_below(c) - J_above(c).
// Kernels:
//   k_joint_rows    per side: its rows in row order, the component weights
//                   and their log2 in the scoring table;
//   k_joint_dims    per (root hp, side): every row's rank in the marginal
//                   fit's stable sort (re-derived by counting), hence its
//                   (w, mu, sigma) there, and the scoring fields;
//   k_joint_active  k_points_active with the roots left out of the lists;
//   k_joint_score   one lane per configuration, both sides: per block of 8
//                   components 8 fp64 accumulators seeded with log2 w, the
//                   root dims' kernel terms added, the block folded into a
//                   running (max, sum);
//   k_joint_sum     total = joint + the conditional terms in hp order;
//   k_joint_tables, k_joint_sample   the draw: one component per
//                   configuration, every root value from that component.
// (the helpers the group model shares are in tpe_joint_dev.hpp)
#include "tpe_joint_dev.hpp"

namespace tpe {

// ---------------------------------------------------------------- the fit
__global__ __launch_bounds__(kJtThreads) void k_joint_rows(JointFitArgs A) {
  __shared__ double red[kJtThreads];
  __shared__ int wcnt[kJtThreads / 64];
  __shared__ int base;
  const int side = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int32_t *rows = A.rows + side * A.kcap;
  if (threadIdx.x == 0) { base = 0; rows[0] = -1; }
  __syncthreads();
  // the side's rows, ascending (ordered compaction, 256 rows a step)
  for (int64_t j0 = 0; j0 < A.n; j0 += kJtThreads) {
    const int64_t j = j0 + threadIdx.x;
    const bool f = j < A.n && (A.below[j] != 0) == (side == 0);
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
  // weights: prior_weight and the linear-forgetting ramp over the side's rows
  const bool lfw = A.lf && A.lf < ns;
  const LfRamp lr = lf_ramp(ns, A.lf);
  double part = 0.0;
  for (int i = threadIdx.x; i < ns; i += kJtThreads) part += lfw ? lf_weight(lr, i) : 1.0;
  const double tot = jt_block_sum(part, red) + A.prior_weight;
  double *jw = A.jw + side * A.kcap;
  double *tab = A.tab + side * (A.kcap / kCoefBlock) * joint_stride(A.n_dim);
  const int Kp = (K + kCoefBlock - 1) / kCoefBlock * kCoefBlock;
  for (int k = threadIdx.x; k < Kp; k += kJtThreads) {
    double w = 0.0;
    if (k < K) {
      w = (k == 0 ? A.prior_weight : (lfw ? lf_weight(lr, k - 1) : 1.0)) / tot;
      jw[k] = w;
    }
    tab[(int64_t)(k / kCoefBlock) * joint_stride(A.n_dim) + (k % kCoefBlock)] =
        k < K ? log2(w) : -INFINITY;
  }
  if (threadIdx.x == 0) {
    A.count[side] = K;
    A.side[side] = JointSide{tot, A.prior_weight / tot};
  }
}

__global__ __launch_bounds__(kJtThreads) void k_joint_dims(JointFitArgs A) {
  const int d = blockIdx.x, side = blockIdx.y;
  const JointDim D = A.dims[d];
  const tpe_hp H = A.hps[D.hp];
  const int K = A.count[side], Kp = (K + kCoefBlock - 1) / kCoefBlock * kCoefBlock;
  const int32_t *rows = A.rows + side * A.kcap;
  const double *col = A.vals + (int64_t)D.hp * A.ld;
  const int64_t ds = ((int64_t)d * 2 + side) * A.kcap;
  double *cw = A.cw + ds, *cmu = A.cmu + ds, *csig = A.csig + ds;
  const int64_t stride = joint_stride(A.n_dim);
  double *tab = A.tab + side * (A.kcap / kCoefBlock) * stride +
                kCoefBlock * (1 + kJointFields * (int64_t)d);
  auto field = [&](int k, int f) -> double & {
    return tab[(int64_t)(k / kCoefBlock) * stride + f * kCoefBlock + (k % kCoefBlock)];
  };
  if (H.family == TPE_CAT) {
    const double a = joint_cat_a(A.prior_weight, H.upper, A.side[side].tot);
    const double *jw = A.jw + side * A.kcap;
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
  // The marginal fit sorted the side's transformed observations stably and
  // put the prior at info.probe; row k's place among the observations is the
  // number of rows that sort before it, counted on the fit's own sort keys.
  const int64_t slot = 2 * (int64_t)D.hp + side;
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

hipError_t launch_joint_fit(const JointFitArgs &a, hipStream_t st) {
  k_joint_rows<<<dim3(2), dim3(kJtThreads), 0, st>>>(a);
  if (a.n_dim > 0)
    k_joint_dims<<<dim3((unsigned)a.n_dim, 2), dim3(kJtThreads), 0, st>>>(a);
  return hipGetLastError();
}

// ------------------------------------------------------------- the score
// k_points_active's walk (tpe_points.hip) with the root hps left out of the
// lists: they are active in every configuration, their terms are +0.0 and
// k_joint_score takes their values
__global__ __launch_bounds__(kJtThreads) void k_joint_active(PointsArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kJtThreads + threadIdx.x;
  const bool in = c < A.m;
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < A.n_hp; ++j) {
    const int hp = A.level_hps[j];
    const int c0 = A.hps[hp].cond_begin, nc = A.hps[hp].cond_count;
    bool act = false;
    if (in) {
      for (int q = 0; q < nc && !act; ++q) {
        const int64_t par = A.cond_parent[c0 + q];
        act = A.active[par * A.act_ld + c] != 0 &&
              A.vals[par * A.ld + c] == (double)A.cond_branch[c0 + q];
      }
      A.active[(int64_t)hp * A.act_ld + c] = (act || nc == 0) ? 1 : 0;
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

// One lane per configuration; the lane's transformed root values are staged
// in LDS, [slot][lane] (a lane reads back only its own stores: no barrier).
// A configuration's numbers depend on its own values and the fit alone.
__global__ __launch_bounds__(kJsThreads) void k_joint_score(JointScoreArgs A) {
  extern __shared__ __attribute__((aligned(16))) double stage[];
  const int lane = threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * kJsThreads + lane;
  const bool in = c < A.m;
  const int64_t cc = in ? c : A.m - 1;  // (a lane past the end repeats the last one)
  double sumlog = 0.0;  // sum of log x over the log-normal dims (lognormal_lpdf's norm)
  bool bad = false;
#pragma unroll 1
  for (int d = 0; d < A.n_dim; ++d) {
    const JointDim D = A.dims[d];
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
  const int64_t stride = joint_stride(A.n_dim);
  const double LN2 = 0.6931471805599453;
  double J[2];
#pragma unroll 1
  for (int side = 0; side < 2; ++side) {
    // the option logs of this side for the categorical dims
#pragma unroll 1
    for (int d = 0; d < A.n_dim; ++d) {
      const JointDim D = A.dims[d];
      if (D.kind != KIND_CAT) continue;
      double *s = stage + (int64_t)D.slot * kJsThreads + lane;
      const double *ol = A.optlog + ((int64_t)side * A.n_opt + D.opt_off + (int64_t)s[0]) * 3;
      s[kJsThreads] = ol[0];
      s[2 * kJsThreads] = ol[1];
      s[3 * kJsThreads] = ol[2];
    }
    const int K = A.K[side];
    KDbl *tab = joint_uniform(A.tab + side * A.tab_side);
    double m[1] = {-INFINITY}, sum[1] = {0.0};
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += kGroup) {
      KDbl *blk = tab + (int64_t)(k0 / kGroup) * stride;
      double t[1][kGroup];
#pragma unroll
      for (int j = 0; j < kGroup; ++j) t[0][j] = blk[j];
#pragma unroll 1
      for (int d = 0; d < A.n_dim; ++d) {
        const JointDim D = A.dims[d];
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
    A.sides[c] = J[0];
    A.sides[A.m + c] = J[1];
    A.joint[c] = J[0] - J[1];
  }
}

// total[c] = joint[c] + the terms of configuration c in ascending hp index
// (the roots' and the inactive ones are +0.0)
__global__ __launch_bounds__(kJtThreads) void k_joint_sum(JointScoreArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kJtThreads + threadIdx.x;
  if (c >= A.m) return;
  double t = A.joint[c];
  for (int i = 0; i < A.n_hp; ++i) t += A.terms[(int64_t)i * A.term_ld + c];
  A.total[c] = t;
}

hipError_t launch_joint_points(const JointScoreArgs &j, const PointsArgs &a, bool walk,
                               hipStream_t st) {
  const unsigned gx = (unsigned)((a.m + kJtThreads - 1) / kJtThreads);
  if (walk) k_joint_active<<<dim3(gx), dim3(kJtThreads), 0, st>>>(a);
  const unsigned gs = (unsigned)((j.m + kJsThreads - 1) / kJsThreads);
  const size_t lds = (size_t)(j.n_slots > 0 ? j.n_slots : 1) * kJsThreads * sizeof(double);
  hipError_t e = hipSuccess;
  if (lds > 48 * 1024)  // (beyond the default dynamic limit: 100 quantized dims take 100 KB)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_joint_score),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  k_joint_score<<<dim3(gs), dim3(kJsThreads), lds, st>>>(j);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_points_score(a, st);  // (its k_points_sum's total is overwritten below)
  if (e != hipSuccess) return e;
  k_joint_sum<<<dim3(gx), dim3(kJtThreads), 0, st>>>(j);
  return hipGetLastError();
}

// --------------------------------------------------------------- the draw
// Tables of one call, 256 threads a block (block_inclusive_scan's addition
// order depends on the block size, and the CDFs must be tpe_sample's bits):
//   block hp < P       a conditional hp: its below mixture's table, as
//                      k_sample_tables builds it; a continuous root: the
//                      truncation constants of its Kb joint components (each
//                      a one-component mixture: base, mass and mode do not
//                      depend on the weight); a categorical root: per
//                      component the CDF of its kappa vector;
//   block P            the CDF of the component weights.
__global__ __launch_bounds__(kJtThreads) void k_joint_tables(JointSampleArgs J) {
  __shared__ DrawTable T;
  const SampleArgs &S = J.S;
  const int hp = blockIdx.x;
  if (hp == S.P.n_hp) {
    for (int k = threadIdx.x; k < J.Kb; k += kJtThreads) J.pick_cdf[k] = J.jw[k];
    __syncthreads();
    block_inclusive_scan(J.pick_cdf, J.Kb, T.wtot);
    return;
  }
  const tpe_hp H = S.P.hps[hp];
  const int d = J.dim_of_hp[hp];
  DrawTable &G = S.tab[hp];
  if (d < 0) {
    const int64_t sb = 2 * (int64_t)hp;
    const int K = S.P.info[sb].K;
    if (K < 1 || K > kTabCap) return;  // (block-uniform: draw_one takes the hp)
    build_table(H, K, S.mw + sb * S.P.kcap, S.mmu + sb * S.P.kcap, S.msig + sb * S.P.kcap, T);
    for (int k = threadIdx.x; k < K; k += kJtThreads) {
      G.cdf[k] = T.cdf[k];
      G.base[k] = T.base[k];
      G.mass[k] = T.mass[k];
      G.mode[k] = T.mode[k];
    }
    return;
  }
  const int64_t ds = (int64_t)d * 2 * S.P.kcap;  // side 0
  if (H.family != TPE_CAT) {
    build_table(H, J.Kb, J.jw, J.cmu + ds, J.csig + ds, T);
    for (int k = threadIdx.x; k < J.Kb; k += kJtThreads) {
      G.base[k] = T.base[k];
      G.mass[k] = T.mass[k];
      G.mode[k] = T.mode[k];
    }
    return;
  }
  const JointDim D = J.dims[d];
  const double a = joint_cat_a(J.prior_weight, H.upper, J.side[0].tot);
  for (int k = 0; k < J.Kb; ++k) {
    double *cdf = J.opt_cdf + D.opt_off * J.Kb + (int64_t)k * H.upper;
    const double o = J.cmu[ds + k];
    for (int c = threadIdx.x; c < H.upper; c += kJtThreads) {
      const double pi = joint_pi(H, J.pprior, c);
      cdf[c] = k == 0 ? pi : joint_kappa((double)c == o, a, pi);
    }
    __syncthreads();
    block_inclusive_scan(cdf, H.upper, T.wtot);
  }
}

// k_sample_points' walk (tpe_sample_points.hip) with the roots drawn from the
// configuration's one joint component
__global__ __launch_bounds__(kJtThreads) void k_joint_sample(JointSampleArgs J) {
  const SampleArgs &S = J.S;
  const PointsArgs &A = S.P;
  const int64_t c = (int64_t)blockIdx.x * kJtThreads + threadIdx.x;
  const bool in = c < A.m;
  const int lane = threadIdx.x & 63;
  const uint64_t gi = (uint64_t)(S.begin + c);
  int comp = 0;
  if (in) {
    const U4 r0 = draw_block0(S.seed, gi, kJointStream | (uint32_t)A.n_hp);
    comp = pick_cdf(J.pick_cdf, J.Kb, u53(r0.x, r0.y));
    if (J.comp) J.comp[c] = comp;
  }
  for (int j = 0; j < A.n_hp; ++j) {
    const int hp = A.level_hps[j];
    const int c0 = A.hps[hp].cond_begin, nc = A.hps[hp].cond_count;
    bool act = false;
    double x = NAN;
    if (in && nc == 0) {
      const int d = J.dim_of_hp[hp];
      const uint32_t stream = kJointStream | (uint32_t)hp;
      const U4 r0 = draw_block0(S.seed, gi, stream);
      const tpe_hp H = A.hps[hp];
      if (H.family == TPE_CAT) {
        const double *cdf = J.opt_cdf + J.dims[d].opt_off * J.Kb + (int64_t)comp * H.upper;
        x = (double)pick_cdf(cdf, H.upper, u53(r0.x, r0.y));
      } else {
        const int64_t ds = (int64_t)d * 2 * A.kcap;
        x = draw_table_value<kTabCap>(H, comp, J.cmu + ds, J.csig + ds, S.tab[hp],
                                      u53(r0.z, r0.w), S.seed, gi, stream);
      }
    } else if (in) {
      for (int q = 0; q < nc && !act; ++q) {
        const int64_t par = A.cond_parent[c0 + q];
        act = A.active[par * A.act_ld + c] != 0 &&
              S.out[par * A.ld + c] == (double)A.cond_branch[c0 + q];
      }
    }
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
      A.active[(int64_t)hp * A.act_ld + c] = (act || nc == 0) ? 1 : 0;
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

size_t joint_sample_tables_bytes(int32_t n_hp) { return (size_t)n_hp * sizeof(DrawTable); }

hipError_t launch_joint_sample(const JointSampleArgs &s, hipStream_t st) {
  const unsigned gx = (unsigned)((s.S.P.m + kJtThreads - 1) / kJtThreads);
  k_joint_tables<<<dim3((unsigned)s.S.P.n_hp + 1), dim3(kJtThreads), 0, st>>>(s);
  k_joint_sample<<<dim3(gx), dim3(kJtThreads), 0, st>>>(s);
  return hipGetLastError();
}

}  // namespace tpe
