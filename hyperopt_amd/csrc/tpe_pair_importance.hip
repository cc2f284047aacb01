// tpe_pair_importance.hip -- pairwise (2-D) importances under the group models
// on the fp64 matrix cores, gfx950 (tpe_plan_group_importance_pairs; DESIGN
// 5.22).
//
// For a pair (a, b), a < b, of hps of one group, side s of the group fit and the
// nodes x_a,i / x_b,j of tpe_importance.hpp's rule (weights w_a,i, w_b,j),
//   L_s[i][j] = sum_k w_k kappa_ak(x_a,i) kappa_bk(x_b,j)   (k over the K_gs components),
//   Z_s = sum_ij W_ij L_s[i][j],  W_ij = w_a,i w_b,j,
//   l = L_below / Z_below, g = L_above / Z_above, q = ghat l + (1 - ghat) g,
//   D_ab = (1 - ghat)^2 sum_ij W_ij (l - g)^2 / q.
// L_s is a G x K x G matrix product.  Launches:
//   k_pair_factors  once per call: F[side][slot][k][i] = kappa_dk(x_i) in the
//                   linear domain, node index fastest, rows K .. pad4(K) zero;
//                   a wave is 64 nodes of one hp and walks 16 components whose
//                   (mu, sigma) come through wave-uniform scalar loads.  Every
//                   factor is computed once, whatever the number of pairs;
//   k_pair_gemm     grid (tile, pair, side): a 256-thread block owns a 64 x 64
//                   tile of the node grid, each wave a 32 x 32 sub-tile as 2 x 2
//                   accumulators of v_mfma_f64_16x16x4_f64.  The block walks k
//                   in slabs of 16 staged in LDS, double-buffered (the next
//                   slab's global loads are in flight while the MFMAs of this
//                   one issue; one barrier a slab); w_k is folded into a's slab
//                   as it is staged.  k ascends.  It writes L and the tile's
//                   sum of W L from a fixed tree;
//   k_pair_z        Z_s: the tiles in ascending order;
//   k_pair_div      f = W (l - g)^2 / q elementwise over a tile, the same tree;
//                   the optional x_a, x_b and log L planes;
//   k_pair_sum      D: the tiles in ascending order.
// No floating-point atomics; a pair's numbers depend on the fit and n_nodes alone.
//
// v_mfma_f64_16x16x4_f64 (D = A B + C, A 16 x 4, B 4 x 16), lane t of the wave:
//   A[t % 16][t / 16], B[t / 16][t % 16], D register v = 0 .. 3: D[4 v + t / 16][t % 16].
#include <math.h>

#include "tpe_joint_dev.hpp"
#include "tpe_pair_importance.hpp"

namespace tpe {

typedef double pair_acc __attribute__((ext_vector_type(4)));

// Phi(zu) - Phi(zl) of a standard normal in erf arguments (z / sqrt 2), zu >= zl,
// taken in the tail's own complement so that a cell far from the mean keeps its
// relative precision
__device__ __forceinline__ double pair_cell(double zu, double zl) {
  if (zl >= 0.0) return 0.5 * (erfc(zl) - erfc(zu));
  if (zu <= 0.0) return 0.5 * (erfc(-zu) - erfc(-zl));
  return 0.5 * (erf(zu) - erf(zl));
}

// the block's sum of v in the fixed tree red[t] += red[t + s], s = 128 .. 1
__device__ __forceinline__ double pair_tree(double v, double *red) {
#pragma clang fp contract(off)
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kPairThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kPairThreads) void k_pair_factors(PairArgs A) {
  const int G = A.lay.G;
  const int IG = (G + 63) / 64;
  const int side = blockIdx.z;
  const int slot = (int)blockIdx.y / IG, ig = (int)blockIdx.y % IG;
  const int hp = A.slot_hp[slot];
  const tpe_hp H = A.hps[hp];
  const int kind = score_kind(H);  // block-uniform
  const int K = min(A.gK[2 * A.group_of_hp[hp] + side], (int)A.lay.fk[side]);
  const int Kp = (K + 3) & ~3;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i = ig * 64 + (int)(threadIdx.x & 63);
  // the node, as k_importance builds it
  const int64_t sb = 2 * (int64_t)hp;
  double min_mu = 0.0, max_mu = 0.0;
  if (kind != KIND_CAT && !((H.flags & TPE_HAS_LOW) && (H.flags & TPE_HAS_HIGH))) {
    const double *mb = A.mmu + sb * A.kcap, *ma = A.mmu + (sb + 1) * A.kcap;
    const int Kb = A.info[sb].K, Ka = A.info[sb + 1].K;
    if (Kb > 0 && Ka > 0) {
      min_mu = fmin(mb[0], ma[0]);
      max_mu = fmax(mb[Kb - 1], ma[Ka - 1]);
    }
  }
  const ImpNodes N = importance_nodes(H, kind, min_mu, max_mu, G);
  const bool act = i < N.count;
  double x = kind_logn(kind) ? 1.0 : 0.0, w = 0.0;
  if (act) importance_node(N, H, kind, i, x, w);
  if (blockIdx.x == 0 && wave == 0 && side == 0 && i < G) {
    double *xs = A.ws + A.lay.nodes;
    xs[(int64_t)slot * G + i] = act ? x : NAN;
    xs[(int64_t)(A.lay.n_slot + slot) * G + i] = w;
  }
  const int k0 = ((int)blockIdx.x * 4 + wave) * kPairSlab;
  if (k0 >= Kp) return;  // (wave-uniform)
  // what the lane keeps of its node, by kind
  double u = x, v = x, pi = 0.0;
  switch (kind) {
    case KIND_LSE_L: u = log(x); break;
    case KIND_ERF_G: quant_bounds<false>(H, x, u, v); break;
    case KIND_ERF_L: quant_bounds<true>(H, x, u, v); break;
    case KIND_CAT: pi = act ? joint_pi(H, A.pprior, (int)x) : 0.0; break;
    default: break;
  }
  const int64_t ds = (sb + side) * A.kcap;
  KDbl *cmu = joint_uniform(A.cmu + ds), *csig = joint_uniform(A.csig + ds);
  double *F = A.ws + (side ? A.lay.f_side1 : 0) + (int64_t)slot * A.lay.fk[side] * G;
  const int k1 = min(k0 + kPairSlab, Kp);
  for (int k = k0; k < k1; ++k) {
    double f = 0.0;
    if (k < K) {  // (wave-uniform)
#pragma clang fp contract(off)
      const double mu = cmu[k], sg = csig[k];
      switch (kind) {
        case KIND_LSE_G: {
          const double z = (u - mu) / fmax(sg, kEPS);
          f = exp(-0.5 * (z * z)) / (2.5066282746310002 * sg);
          break;
        }
        case KIND_LSE_L: {
          const double s = fmax(sg, kEPS);
          const double z = (u - mu) / s;
          f = exp(-0.5 * (z * z)) / (2.5066282746310002 * s * x);
          break;
        }
        case KIND_ERF_G:
        case KIND_ERF_L: {
          const double d = fmax(1.4142135623730951 * sg, kEPS);
          f = pair_cell((u - mu) / d, (v - mu) / d);
          break;
        }
        default:  // mu: the component's observed option (the prior: -1), sigma: a
          f = k == 0 ? pi : joint_kappa(mu == x, sg, pi);
          break;
      }
    }
    if (i < G) F[(int64_t)k * G + i] = act ? f : 0.0;
  }
}

// the slab [k0, k0 + 16) of one dim's tile columns [c0, c0 + 64): thread t loads
// rows t / 64 + 4 q of column t % 64 (zero past pad4(K) and past G)
__device__ __forceinline__ void pair_slab_load(const double *F, int G, int Kp, int k0, int c0,
                                               double (&r)[4]) {
  const int c = c0 + (int)(threadIdx.x & 63);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k0 + (int)(threadIdx.x >> 6) + 4 * q;
    r[q] = (k < Kp && c < G) ? F[(int64_t)k * G + c] : 0.0;
  }
}

__global__ __launch_bounds__(kPairThreads) void k_pair_gemm(PairArgs A) {
  __shared__ double sA[2][kPairSlab][kPairLd], sB[2][kPairSlab][kPairLd];
  __shared__ double red[kPairThreads];
  const int G = A.lay.G, T = A.lay.T;
  const int tile = blockIdx.x, pair = blockIdx.y;
  const int side = 1 - (int)blockIdx.z;  // the long above side is scheduled first
  const int i0 = (tile / T) * kPairTile, j0 = (tile % T) * kPairTile;
  const int sa = A.pair_slot[2 * pair], sbb = A.pair_slot[2 * pair + 1];
  const int g = A.group_of_hp[A.slot_hp[sa]];
  const int K = min(A.gK[2 * g + side], (int)A.lay.fk[side]);  // (fk bounds K: tpe_engine.hip)
  const int Kp = (K + 3) & ~3;
  const double *Fs = A.ws + (side ? A.lay.f_side1 : 0);
  const double *Fa = Fs + (int64_t)sa * A.lay.fk[side] * G;
  const double *Fb = Fs + (int64_t)sbb * A.lay.fk[side] * G;
  const double *wk = A.gw + (2 * (int64_t)g + side) * A.kcap;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ra = 32 * (wv >> 1) + (lane & 15), rb = 32 * (wv & 1) + (lane & 15);
  const int kq = lane >> 4;
  const int sr = threadIdx.x >> 6, sc = threadIdx.x & 63;  // the thread's staging rows / column

  pair_acc acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = pair_acc{0.0, 0.0, 0.0, 0.0};

  double va[4], vb[4];
  auto load = [&](int k0) {
    pair_slab_load(Fa, G, Kp, k0, i0, va);
    pair_slab_load(Fb, G, Kp, k0, j0, vb);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + sr + 4 * q;
      va[q] *= k < K ? wk[k] : 0.0;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sA[buf][sr + 4 * q][sc] = va[q];
      sB[buf][sr + 4 * q][sc] = vb[q];
    }
  };
  load(0);
  store(0);
  __syncthreads();
  const int n_slab = (Kp + kPairSlab - 1) / kPairSlab;
  for (int s = 0; s < n_slab; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < n_slab;  // (block-uniform)
    if (more) load((s + 1) * kPairSlab);
#pragma unroll
    for (int step = 0; step < kPairSlab / 4; ++step) {
      const int kr = 4 * step + kq;
      const double a0 = sA[buf][kr][ra], a1 = sA[buf][kr][ra + 16];
      const double b0 = sB[buf][kr][rb], b1 = sB[buf][kr][rb + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    // (the other buffer was last read before the barrier that ended slab s - 1)
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // L and the tile's sum of W L: the lane's 16 values in (m, n, v) order, then the tree
  const double *xw = A.ws + A.lay.nodes + (int64_t)A.lay.n_slot * G;
  const double *wa = xw + (int64_t)sa * G, *wb = xw + (int64_t)sbb * G;
  double *L = A.ws + A.lay.L + (2 * (int64_t)pair + side) * G * G;
  double part = 0.0;
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int j = j0 + 32 * (wv & 1) + 16 * n + (lane & 15);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = i0 + 32 * (wv >> 1) + 16 * m + 4 * v + kq;
          if (i < G && j < G) {
            const double l = acc[m][n][v];
            L[(int64_t)i * G + j] = l;
            part += (wa[i] * wb[j]) * l;
          }
        }
      }
  }
  const double tot = pair_tree(part, red);
  if (threadIdx.x == 0)
    A.ws[A.lay.zpart + (2 * (int64_t)pair + side) * T * T + tile] = tot;
}

__global__ __launch_bounds__(kPairThreads) void k_pair_z(PairArgs A) {
#pragma clang fp contract(off)
  const int e = (int)blockIdx.x * kPairThreads + (int)threadIdx.x;
  if (e >= 2 * A.lay.n_pair) return;
  const int tiles = A.lay.T * A.lay.T;
  const double *pt = A.ws + A.lay.zpart + (int64_t)e * tiles;
  double z = 0.0;
  for (int t = 0; t < tiles; ++t) z += pt[t];
  ((e & 1) ? A.Za : A.Zb)[e >> 1] = z;
}

__global__ __launch_bounds__(kPairThreads) void k_pair_div(PairArgs A) {
  __shared__ double red[kPairThreads];
  const int G = A.lay.G, T = A.lay.T;
  const int tile = blockIdx.x, pair = blockIdx.y;
  const int i0 = (tile / T) * kPairTile, j0 = (tile % T) * kPairTile;
  const int sa = A.pair_slot[2 * pair], sbb = A.pair_slot[2 * pair + 1];
  const double *xs = A.ws + A.lay.nodes, *xw = xs + (int64_t)A.lay.n_slot * G;
  const double *Lb = A.ws + A.lay.L + 2 * (int64_t)pair * G * G, *La = Lb + (int64_t)G * G;
  const double zb = A.Zb[pair], za = A.Za[pair];
  const double ghat = A.ghat;
  const int j = j0 + (int)(threadIdx.x & 63);
  if (threadIdx.x < 64) {
    const int c = threadIdx.x;
    if (A.xa && j0 == 0 && i0 + c < G)
      A.xa[(int64_t)pair * G + i0 + c] = xs[(int64_t)sa * G + i0 + c];
    if (A.xb && i0 == 0 && j0 + c < G)
      A.xb[(int64_t)pair * G + j0 + c] = xs[(int64_t)sbb * G + j0 + c];
  }
  double part = 0.0;
  if (j < G) {
#pragma clang fp contract(off)
    const double wj = xw[(int64_t)sbb * G + j];
    const bool on_j = xs[(int64_t)sbb * G + j] == xs[(int64_t)sbb * G + j];
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int i = i0 + (int)(threadIdx.x >> 6) + 4 * q;
      if (i >= G) break;
      const int64_t o = (int64_t)i * G + j;
      const double lb = Lb[o], la = La[o];
      const double l = zb > 0.0 ? lb / zb : 0.0, g = za > 0.0 ? la / za : 0.0;
      const double den = ghat * l + (1.0 - ghat) * g;
      const double d = l - g;
      if (den > 0.0) part += (xw[(int64_t)sa * G + i] * wj) * (d * d) / den;
      if (A.logL) {
        const bool on = on_j && xs[(int64_t)sa * G + i] == xs[(int64_t)sa * G + i];
        double *out = A.logL + 2 * (int64_t)pair * G * G + o;
        out[0] = on ? log(lb) : NAN;
        out[(int64_t)G * G] = on ? log(la) : NAN;
      }
    }
  }
  const double tot = pair_tree(part, red);
  if (threadIdx.x == 0) A.ws[A.lay.dpart + (int64_t)pair * T * T + tile] = tot;
}

__global__ __launch_bounds__(kPairThreads) void k_pair_sum(PairArgs A) {
#pragma clang fp contract(off)
  const int pair = (int)blockIdx.x * kPairThreads + (int)threadIdx.x;
  if (pair >= A.lay.n_pair) return;
  const int tiles = A.lay.T * A.lay.T;
  const double *pt = A.ws + A.lay.dpart + (int64_t)pair * tiles;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += pt[t];
  const double c = (1.0 - A.ghat) * (1.0 - A.ghat);
  A.D[pair] = A.ghat == 1.0 ? 0.0 : c * s;
}

hipError_t launch_pair_importance(const PairArgs &a, hipStream_t st) {
  const PairLayout &P = a.lay;
  if (P.n_pair <= 0) return hipSuccess;
  const unsigned tiles = (unsigned)(P.T * P.T);
  const int64_t kmax = P.fk[0] > P.fk[1] ? P.fk[0] : P.fk[1];
  const unsigned kblocks = (unsigned)((kmax + 4 * kPairSlab - 1) / (4 * kPairSlab));
  const unsigned IG = (unsigned)((P.G + 63) / 64);
  k_pair_factors<<<dim3(kblocks, (unsigned)P.n_slot * IG, 2), dim3(kPairThreads), 0, st>>>(a);
  k_pair_gemm<<<dim3(tiles, (unsigned)P.n_pair, 2), dim3(kPairThreads), 0, st>>>(a);
  k_pair_z<<<dim3((unsigned)((2 * P.n_pair + kPairThreads - 1) / kPairThreads)),
             dim3(kPairThreads), 0, st>>>(a);
  k_pair_div<<<dim3(tiles, (unsigned)P.n_pair), dim3(kPairThreads), 0, st>>>(a);
  k_pair_sum<<<dim3((unsigned)((P.n_pair + kPairThreads - 1) / kPairThreads)),
               dim3(kPairThreads), 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace tpe
