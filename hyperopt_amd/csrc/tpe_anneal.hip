// tpe_anneal.hip -- annealing suggestions on the device-resident history
// (anneal.suggest; hyperopt/anneal.py:43-408).
//   k_anneal_order : the history rows in ascending (loss, row) order -- built
//                    once per call, shared by every suggestion -- and T[hp],
//                    the rows in which each hp is active
//   k_anneal       : one wave per suggestion walks the hps parents first,
//                    picks each active hp's anchor row (anneal.py:151-184) and
//                    draws its value from the prior narrowed around the
//                    anchor's value (anneal.py:232-408)
//
// Draws: Philox4x32-10 through draw4, key = the suggestion seed, counter
// gi = 0, stream = 2^30 | hp (candidate draws use stream hp, prior draws
// 2^31 | hp), iteration 0.  Of the four uniforms of that one draw4,
//   u0       the rank draw (consumed only when a fresh anchor is drawn),
//   u1       the value draw of the bounded and the categorical kinds,
//   u2, u3   the Box-Muller pair of the normal kinds.
// The trace keeps the consumed ones in that order (tpe_anneal_trace).
#include <math.h>

#include "tpe_anneal.hpp"
#include "tpe_draw.hpp"

// the value formulas are compared bit for bit with their fp64 statement on the
// host (tests/test_gpu_anneal.py): one rounding per operation, no FMA
#pragma clang fp contract(off)

namespace tpe {

// ------------------------------------------------------------------------
// Loss order.  One block, a stable LSD radix sort of (key, row) pairs in
// global ping-pong buffers: 16 passes of 4 bits over the 64-bit order-
// preserving image of the loss.  Wave w owns a contiguous run of 64-row chunks
// of the source and reads them coalesced, lane l taking row 64 c + l.  Four
// ballots give every lane the mask of the chunk's lanes with its digit: its
// popcount is the digit's count (count phase: the group's first lane adds it
// to hist[d][w]), the popcount below the lane its rank in the chunk (scatter
// phase: position = hist[d][w] + rank, then the first lane advances
// hist[d][w]).  Between the phases hist is scanned in (digit, wave) order.
// Equal digits therefore keep their source order -- wave run, chunk, lane --
// so every pass is stable, equal losses keep their row order (the sort starts
// from the identity), and the result does not depend on timing or on the
// grid: it is exact for every n.  Latency-bound: 16 x (count, scan, scatter)
// by 1024 threads, the same path for every history size.
// The other blocks of the grid count T[hp], one wave per hp.
// ------------------------------------------------------------------------
constexpr int kOrdThreads = 1024;
constexpr int kOrdDigits = 1 << kAnnealDigitBits;
constexpr int kOrdWaves = kOrdThreads / 64;
constexpr int kOrdBatch = 4;  // chunks a wave loads ahead of its dependent LDS steps
static_assert(kAnnealPasses % 2 == 0, "the order must end in buffer 0");
static_assert(kOrdDigits * kOrdWaves == 4 * 64, "the scan takes four entries per lane of one wave");

__device__ __forceinline__ uint64_t loss_key(double l) {
  const uint64_t b = (uint64_t)__double_as_longlong(l + 0.0);  // (-0 sorts as +0)
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the lanes of the wave that are `ok` and hold digit d (every lane calls it)
__device__ __forceinline__ uint64_t same_digit(bool ok, int d) {
  uint64_t m = __ballot(ok);
#pragma unroll
  for (int b = 0; b < kAnnealDigitBits; ++b) {
    const uint64_t mb = __ballot(ok && ((d >> b) & 1));
    m &= ((d >> b) & 1) ? mb : ~mb;
  }
  return m;
}

__global__ __launch_bounds__(kOrdThreads) void k_anneal_order(
    const double *__restrict__ losses, const uint8_t *__restrict__ active, int64_t ld, int32_t n,
    int32_t n_hp, uint64_t *keys0, uint64_t *keys1, int32_t *idx0, int32_t *idx1,
    int32_t *__restrict__ T) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (blockIdx.x > 0) {  // activity counts
    const int hp = ((int)blockIdx.x - 1) * kOrdWaves + wv;
    if (hp >= n_hp) return;
    const uint8_t *col = active + (int64_t)hp * ld;
    int c = 0;
    for (int r0 = lane; r0 < n; r0 += 64 * 8) {
      uint8_t a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = r0 + 64 * j < n ? col[r0 + 64 * j] : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) c += a[j] != 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) T[hp] = c;
    return;
  }
  __shared__ int32_t hist[kOrdDigits * kOrdWaves];  // [digit][wave]
  for (int i = t; i < n; i += kOrdThreads) {
    keys0[i] = loss_key(losses[i]);
    idx0[i] = i;
  }
  __syncthreads();
  const int nchunks = (n + 63) / 64;
  const int cpw = (nchunks + kOrdWaves - 1) / kOrdWaves;
  const int c0 = min(nchunks, wv * cpw), c1 = min(nchunks, c0 + cpw);
  const uint64_t below = (1ull << lane) - 1;
#pragma unroll 1
  for (int pass = 0; pass < kAnnealPasses; ++pass) {
    const uint64_t *sk = (pass & 1) ? keys1 : keys0;
    const int32_t *si = (pass & 1) ? idx1 : idx0;
    uint64_t *dk = (pass & 1) ? keys0 : keys1;
    int32_t *di = (pass & 1) ? idx0 : idx1;
    const int sh = pass * kAnnealDigitBits;
    // a wave counts and scatters through its own column of hist only
    if (lane < kOrdDigits) hist[lane * kOrdWaves + wv] = 0;
    for (int c = c0; c < c1; c += kOrdBatch) {
      uint64_t kk[kOrdBatch];
#pragma unroll
      for (int j = 0; j < kOrdBatch; ++j) {
        const int i = (c + j) * 64 + lane;
        kk[j] = (c + j < c1 && i < n) ? sk[i] : 0;
      }
#pragma unroll
      for (int j = 0; j < kOrdBatch; ++j) {
        if (c + j >= c1) break;
        const bool ok = (c + j) * 64 + lane < n;
        const int d = (int)((kk[j] >> sh) & (kOrdDigits - 1));
        const uint64_t m = same_digit(ok, d);
        if (ok && (m & below) == 0) hist[d * kOrdWaves + wv] += __popcll(m);
      }
    }
    __syncthreads();
    // exclusive scan of hist[0, 256) in place by wave 0, four entries per lane
    if (wv == 0) {
      int32_t v[4];
      int32_t sum = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = hist[lane * 4 + j];
        sum += v[j];
      }
      int32_t inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      int32_t base = inc - sum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hist[lane * 4 + j] = base;
        base += v[j];
      }
    }
    __syncthreads();
    for (int c = c0; c < c1; c += kOrdBatch) {
      uint64_t kk[kOrdBatch];
      int32_t ii[kOrdBatch];
#pragma unroll
      for (int j = 0; j < kOrdBatch; ++j) {
        const int i = (c + j) * 64 + lane;
        const bool ok = c + j < c1 && i < n;
        kk[j] = ok ? sk[i] : 0;
        ii[j] = ok ? si[i] : 0;
      }
#pragma unroll
      for (int j = 0; j < kOrdBatch; ++j) {  // (in source order: the pass is stable)
        if (c + j >= c1) break;
        const bool ok = (c + j) * 64 + lane < n;
        const int d = (int)((kk[j] >> sh) & (kOrdDigits - 1));
        const uint64_t m = same_digit(ok, d);
        if (ok) {
          const int32_t at = hist[d * kOrdWaves + wv];
          const int32_t pos = at + __popcll(m & below);
          if (pos >= 0 && pos < n) {  // (always: the counts sum to n)
            dk[pos] = kk[j];
            di[pos] = ii[j];
          }
          if ((m & below) == 0) hist[d * kOrdWaves + wv] = at + __popcll(m);
        }
      }
    }
    __syncthreads();  // the next pass reads what every wave scattered
  }
}

hipError_t launch_anneal_order(const double *losses, const uint8_t *active, int64_t ld, int32_t n,
                               int32_t n_hp, uint64_t *keys0, uint64_t *keys1, int32_t *idx0,
                               int32_t *idx1, int32_t *T, hipStream_t st) {
  const int blocks = 1 + (n_hp + kOrdWaves - 1) / kOrdWaves;
  k_anneal_order<<<blocks, kOrdThreads, 0, st>>>(losses, active, ld, n, n_hp, keys0, keys1, idx0,
                                                 idx1, T);
  return hipGetLastError();
}

// ------------------------------------------------------------------------
// k_anneal: one wave per suggestion.  Every lane carries the same scalar
// state (the computation is wave-uniform); the lanes spread out only over
// the anchor list (reuse test: one ballot over active[hp][best[i]]) and over
// the loss order (fresh anchor: 64 rows per step, ballot + popcount until the
// running count of active rows passes the rank).  Per wave in LDS: the value
// each hp drew (NaN: inactive; the children's activity test reads it) and
// the anchor list `best` (at most one entry per hp).
// ------------------------------------------------------------------------
constexpr int kAnnealWaves = 4;

size_t anneal_wave_lds(int32_t n_hp) { return (size_t)n_hp * (sizeof(double) + sizeof(int32_t)); }

__global__ __launch_bounds__(64 * kAnnealWaves) void k_anneal(AnnealArgs A) {
  extern __shared__ __attribute__((aligned(16))) double an_smem[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int s = (int)blockIdx.x * nw + w;
  if (s >= A.n_suggest) return;  // (whole waves; the kernel has no block barrier)
  const int P = A.n_hp;
  double *val = an_smem + (size_t)w * P;
  int32_t *best = reinterpret_cast<int32_t *>(an_smem + (size_t)nw * P) + (size_t)w * P;
  const uint64_t seed = A.seeds[s];
  Partial *res = A.results + (int64_t)s * P;
  AnnealTrace *trc = A.trace + (int64_t)s * P;
  int nbest = 0;
#pragma unroll 1
  for (int k = 0; k < P; ++k) {
    const int hp = A.hp_order[k];
    const tpe_hp H = A.hps[hp];
    bool act = H.cond_count == 0;
    for (int c = 0; c < H.cond_count; ++c)
      act |= val[A.cond_parent[H.cond_begin + c]] == (double)A.cond_branch[H.cond_begin + c];
    if (!act) {
      val[hp] = NAN;
      if (lane == 0) {
        res[hp] = Partial{NAN, NAN, -1, 0, 0};
        trc[hp] = AnnealTrace{-1, -1, {NAN, NAN, NAN, NAN}};
      }
      continue;
    }
    const Draw d = draw4(seed, 0, 0x40000000u | (uint32_t)hp, 0);
    const int T = A.T[hp];
    const uint8_t *col = A.active + (int64_t)hp * A.ld;
    int row = -1, rank = -1;
    if (T > 0) {
      // anchor reuse: the first entry of `best` whose row has the hp active
      for (int b0 = 0; b0 < nbest && row < 0; b0 += 64) {
        const int i = b0 + lane;
        const int rr = i < nbest ? best[i] : -1;
        const uint64_t m = __ballot(rr >= 0 && rr < A.n && col[rr] != 0);
        if (m) row = __shfl(rr, __builtin_ctzll(m), 64);
      }
      if (row < 0) {
        // fresh anchor: geometric(p) on {1, 2, ...} by inversion, rank
        // r = clip(g - 1, 0, T - 1) among the hp's rows in (loss, row) order
        const double g = A.p_geo >= 1.0 ? 1.0 : ceil(log1p(-d.u0) / A.log1p_mq);
        rank = (int)fmin(fmax(g - 1.0, 0.0), (double)(T - 1));
        int seen = 0, last = -1;
        for (int c0 = 0; c0 < A.n; c0 += 64) {
          const int i = c0 + lane;
          const int rr = i < A.n ? A.order[i] : -1;
          uint64_t m = __ballot(rr >= 0 && rr < A.n && col[rr] != 0);
          const int cnt = __popcll(m);
          if (seen + cnt > rank) {
            for (int j = seen; j < rank; ++j) m &= m - 1;
            row = __shfl(rr, __builtin_ctzll(m), 64);
            break;
          }
          if (m) last = __shfl(rr, 63 - __builtin_clzll(m), 64);
          seen += cnt;
        }
        if (row < 0) row = last;  // (T counts the rows the walk sees: not reached)
        if (row >= 0) best[nbest++] = row;
      }
    }
    // the consumed uniforms, packed: [rank draw,] value draw(s)
    const bool fresh = row >= 0 && rank >= 0;
    const bool two = H.family != TPE_CAT && !(H.flags & (TPE_HAS_LOW | TPE_HAS_HIGH));
    const double ua = two ? d.u2 : d.u1, ub = two ? d.u3 : (double)NAN;
    const AnnealTrace tr{row, fresh ? rank : -1,
                         {fresh ? d.u0 : ua, fresh ? ua : ub, fresh ? ub : (double)NAN, NAN}};
    const bool prior = row < 0;
    const double shrink = prior ? 1.0 : 1.0 / (1.0 + (double)T * A.shrink_coef);
    const double v = prior ? 0.0 : A.vals[(int64_t)hp * A.ld + row];
    double x;
    if (H.family == TPE_CAT) {
      const int up = H.upper;
      if (prior && !(H.flags & TPE_PCHOICE)) {
        x = fmin(floor(d.u1 * (double)up), (double)(up - 1));  // randint prior
      } else {
        // p = (1 - shrink) onehot(v) + shrink prior; inverse CDF over the
        // fp64 partial sums in index order
        const double *pp = A.pprior + H.pprior_begin;
        const bool pc = (H.flags & TPE_PCHOICE) != 0;
        const double pu = 1.0 / (double)up;
        const int vi = prior ? -1 : (int)v;
        double tot = 0.0;
        for (int c = 0; c < up; ++c)
          tot += (1.0 - shrink) * (c == vi ? 1.0 : 0.0) + shrink * (pc ? pp[c] : pu);
        const double t = d.u1 * tot;
        double acc = 0.0;
        int pick = up - 1;
        for (int c = 0; c < up - 1; ++c) {
          acc += (1.0 - shrink) * (c == vi ? 1.0 : 0.0) + shrink * (pc ? pp[c] : pu);
          if (t < acc) { pick = c; break; }
        }
        x = (double)pick;
      }
    } else {
      const bool lg = H.family == TPE_LGMM;
      if (H.flags & (TPE_HAS_LOW | TPE_HAS_HIGH)) {
        // hp_uniform (anneal.py:232-291); low / high are log-space for LGMM
        double a = H.low, b = H.high;
        if (!prior) {
          const double width = (H.high - H.low) * shrink;
          const double half = 0.5 * width;
          const double mid = fmin(fmax(lg ? log(v) : v, H.low + half), H.high - half);
          a = mid - half;
          b = mid + half;
        }
        x = a + (b - a) * d.u1;
        if (!(x < b)) x = nextafter(b, -INFINITY);
      } else {
        double mu = H.prior_mu;
        if (!prior) {
          if (!lg) mu = v;
          else mu = (H.flags & TPE_HAS_Q) ? log(1e-16 + v) : log(v);  // anneal.py:377-397
        }
        const double z = sqrt(-2.0 * log(1.0 - d.u2)) * cospi(2.0 * d.u3);
        x = mu + (H.prior_sigma * shrink) * z;
      }
      if (lg) x = exp(x);
      if (H.flags & TPE_HAS_Q) x = rint(x / H.q) * H.q;
    }
    val[hp] = x;
    if (lane == 0) {
      res[hp] = prior ? Partial{0.0, x, 0, 1, 0} : Partial{A.losses[row], x, (int64_t)row, 1, 0};
      trc[hp] = tr;
    }
  }
}

hipError_t launch_anneal(const AnnealArgs &a, hipStream_t st) {
  if (a.n_suggest <= 0 || a.n_hp <= 0) return hipSuccess;
  // four suggestions per block while their LDS state fits, else one
  const size_t per = anneal_wave_lds(a.n_hp);
  const int nw = per * kAnnealWaves <= 48 * 1024 ? kAnnealWaves : 1;
  const int blocks = (a.n_suggest + nw - 1) / nw;
  k_anneal<<<blocks, 64 * nw, per * nw, st>>>(a);
  return hipGetLastError();
}

}  // namespace tpe
