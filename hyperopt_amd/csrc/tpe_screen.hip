// tpe_screen.hip -- the screened pruning draw in a translation
// unit of its own: the kernels of tpe_prune.hip and tpe_kernels.hip keep their
// code and register allocation.
//
// k_draw_sorted_prune inverts the CDF of every candidate and buckets it, and
// then drops most wave tiles unread.  For a fixed component k the drawn value
// is nondecreasing in u1, so whether a candidate can lie near a hot interval
// is decided from (k, u1): k_draw_zone leaves, per (suggestion, slot), value
// zones outside which nothing is hot and the u1 thresholds of their edges per
// component; k_draw_sorted_screen draws Philox and the pick for every
// candidate, inverts only the ones inside a zone, and composes the kept tiles
// from those alone where it can prove that the layout is the full draw's.
// Where it cannot, the sort block runs sorted_block_prune_body from scratch.
// k_draw_sorted_screen_int makes the same decisions on the uniforms' 53-bit
// integers: the pick from a guide table on the top bits of U0, the class from
// integer thresholds on U1, no double before the inversion.
// k_draw_sorted_screen_run (the default) is that kernel by runs of sort blocks:
// the slot's state once per run, its table from k_draw_zone, Philox in the row
// form and the uniforms in their word form (tpe_philox_row.hpp).
#include <float.h>
#include <math.h>

#include "tpe_draw.hpp"
#include "tpe_internal.hpp"
#include "tpe_philox_row.hpp"
#include "tpe_screen_pool.hpp"

namespace tpe {

constexpr double kScreenQMin = 0x1p-24;  // w = 15.25 at q = 2^-24
constexpr int kScreenThreads = 512;  // (k_draw_sorted_prune's block)
constexpr int kZoneThreads = 256;
constexpr int kZoneCand = kHotIv + 2;  // zones before merging: the hot intervals and two tails
// a wave's inverted elements (of at most kSortedBlock / 8 = 1024): room for 62 %
constexpr int kScreenList = 640;

// ------------------------------------------------------------------------
// k_draw_zone
// ------------------------------------------------------------------------
// "the draw of component k at u1 certainly lies above v" (up: an upper zone
// edge, v = edge + delta) or "... does not certainly lie below v" (a lower
// zone edge, v = edge - delta): false, then true as u1 grows.  The tail
// probability is computed from u1 by draw_bounded_invert's own operations
// (monotone in u1 as floating-point functions) and compared with the normal
// tail probability of v, so the screen relies on nothing but
// |draw_bounded_invert's x - the true quantile at that probability| <= delta.
__device__ __forceinline__ bool zone_crossed(double u1, double b, double m, int md, double z,
                                             double tail, bool up) {
  double pu, pp, q1;
  {
#pragma clang fp contract(off)
    const double um = u1 * m;
    pu = b - um;
    pp = b + um;
    q1 = 1.0 - pp;
  }
  constexpr double rho = 1e-13;  // (erfc's own error, a few ulp)
  const double t_hi = tail * (1.0 + rho), t_lo = tail * (1.0 - rho);
  bool above, below;
  if (md == 1) {                       // tail = Q(z); x grows as pu falls
    above = pu < t_lo;
    below = pu > t_hi;
  } else if (md == 2 || z < 0.0) {     // tail = Phi(z); below the mean, x grows with pp
    above = pp > t_hi;
    below = pp < t_lo;
  } else {                             // tail = Q(z) at or above the mean
    above = pp >= 0.5 && q1 < t_lo;
    below = pp < 0.5 || q1 > t_hi;
  }
  // erfcinv_fast holds that bound only for w = -log(2q (2 - 2q)) < 16 (its
  // tail polynomial drifts beyond: tools/table_error.py --erfcinv), so a tail
  // probability under kScreenQMin is never cold: every threshold is clamped
  // into the u1 range with q >= kScreenQMin
  const bool ok_lo = md == 1 || pp >= kScreenQMin;
  const bool deep_hi = md == 1 ? pu < kScreenQMin : md == 0 && pp >= 0.5 && q1 < kScreenQMin;
  return deep_hi || (ok_lo && (up ? above : !below));
}

// One block per (suggestion, slot row), the grid rows of the draw.  Reads the
// slot's TabHot and the pilot's sort block (block 0 of A.cand, whole) and
// writes the slot's DrawZone.  gbits >= 0: its integer form too (thrI, pickB
// and the guide of 2^gbits buckets), and no zones for a slot whose guide is
// not valid: the draw's table not finite and nondecreasing with a positive
// total, or two distinct pick boundaries inside one bucket.
//
// The zones are the hot intervals, each widened to where the tiles the draw
// keeps can reach, and two tails that give a sort block's key range inverted
// elements.  Both are heuristics of the fallback rate alone: the draw checks
// per sort block that its key range comes from inverted elements and that no
// live bucket lies in a gap's bucket range (screen_compose), so any zones that
// contain the hot intervals are sound.
//  - halves >= 0: a hot interval [a, b] reaches down to the minimum of the
//    half tile (64 positions of the pilot's sorted block) `halves` before the
//    first one whose maximum is at least a, and up likewise; halves < 0: the
//    same rule in whole tiles, `tiles` of them.
//  - tail: the low tail ends at the tail-th smallest value of the pilot's
//    first wave tile, the high tail starts at the tail-th largest of its last
//    (128: the tiles' maximum and minimum).
__global__ __launch_bounds__(kZoneThreads) void k_draw_zone(ScoreArgs A, DrawZone *zones,
                                                            int32_t tiles, int32_t halves,
                                                            int32_t tail, double margin,
                                                            int32_t gbits) {
  __shared__ DrawTableT<kFuseTab> T;
  __shared__ double tmin[kPilotWaves], tmax[kPilotWaves];
  __shared__ double hmin[2 * kPilotWaves], hmax[2 * kPilotWaves];
  __shared__ double tail_s[2];
  __shared__ double zlo[kZoneCand], zhi[kZoneCand];
  __shared__ uint64_t pb[kFuseTab];
  __shared__ int nz_s, bad_s;
  const int s = blockIdx.y;
  const int slot = row_slot(A, s, 0, A.n_slots, blockIdx.x);
  if (slot < 0) return;
  const int hp = A.level_hps[slot];
  const tpe_hp H = A.hps[hp];
  if (!A.force_active && !A.compact &&
      !hp_active(H, A.results + (int64_t)s * A.n_hp, A.cond_parent, A.cond_branch))
    return;
  const int kind = slot_kind(A, slot);
  if ((kind == KIND_CAT || kind == KIND_LAT) && lookup_inline(A, A.info[2 * hp].K)) return;
  DrawZone *Z = zones + ((int64_t)s * A.n_hp + hp);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t sb = 2 * (int64_t)hp;
  const int K = A.info[sb].K;
  const TabHot *hot = A.tab_hot + ((int64_t)s * A.n_hp + hp);
  // the slots the screen takes: two-row wave-tile GMM slots, bounded, not
  // quantized, with a small table, two certified Chebyshev tables and hot
  // intervals that are not "everything" (sorted_block_prune_body's `prune`)
  bool scr = kind == KIND_LSE_GW && H.family == TPE_GMM && (H.flags & TPE_HAS_LOW) &&
             (H.flags & TPE_HAS_HIGH) && !(H.flags & TPE_HAS_Q) && K >= 1 && K <= kFuseTab &&
             tab_valid(A.tab_hdr[sb]) && tab_valid(A.tab_hdr[sb + 1]);
  int nh = 0;
  if (scr) {
    while (nh < kHotIv && hot->lo[nh] <= hot->hi[nh]) ++nh;
    scr = !(nh > 0 && hot->lo[0] == -INFINITY && hot->hi[0] == INFINITY);
  }
  if (!scr) {  // (block-uniform)
    if (t == 0) Z->nz = 0;
    return;
  }
  // minimum and maximum of the pilot's 64 wave tiles
  const double *pc = A.cand + (int64_t)s * A.cand_sstride + (int64_t)slot * A.n_cand;
  for (int w = wv; w < kPilotWaves; w += kZoneThreads / 64) {
    const double a = pc[w * 128 + lane], b = pc[w * 128 + 64 + lane];
    double mn = fmin(a, b), mx = fmax(a, b);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = fmin(mn, __shfl_xor(mn, o, 64));
      mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) { tmin[w] = mn; tmax[w] = mx; }
    if (halves >= 0) {  // (block-uniform) ... and of its two half tiles
      double an = a, ax = a, bn = b, bx = b;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        an = fmin(an, __shfl_xor(an, o, 64));
        ax = fmax(ax, __shfl_xor(ax, o, 64));
        bn = fmin(bn, __shfl_xor(bn, o, 64));
        bx = fmax(bx, __shfl_xor(bx, o, 64));
      }
      if (lane == 0) { hmin[2 * w] = an; hmax[2 * w] = ax; hmin[2 * w + 1] = bn; hmax[2 * w + 1] = bx; }
    }
  }
  __syncthreads();
  // the tails' edges: wave 0 the tail-th smallest of tile 0, wave 1 the
  // tail-th largest of tile 63, by counting each element's rank in its tile
  // (equal values in index order; rank tail - 1 from its end is the edge)
  static_assert(kZoneThreads >= 128, "a wave per tail");
  if (wv < 2) {
    const int w = wv == 0 ? 0 : kPilotWaves - 1;
    if (lane == 0) tail_s[wv] = wv == 0 ? tmax[w] : tmin[w];
    if (tail < 128) {
      const double a = pc[w * 128 + lane], b = pc[w * 128 + 64 + lane];
      int ra = 0, rb = 0;  // the elements ahead of a and of b in ascending order
      for (int i = 0; i < 64; ++i) {
        const double ua = __shfl(a, i, 64), ub = __shfl(b, i, 64);
        ra += (ua < a || (ua == a && i < lane) ? 1 : 0) + (ub < a ? 1 : 0);
        rb += (ua <= b ? 1 : 0) + (ub < b || (ub == b && i < lane) ? 1 : 0);
      }
      const int want = wv == 0 ? tail - 1 : 128 - tail;
      if (ra == want) tail_s[wv] = a;
      if (rb == want) tail_s[wv] = b;
    }
  }
  __syncthreads();
  if (t == 0) {
    const double pm = H.prior_mu, y_lo = hot->y_lo, y_hi = hot->y_hi;
    int nz = 0;
    // the tails: the block's key range comes from inverted elements alone
    zlo[nz] = -INFINITY; zhi[nz] = tail_s[0]; ++nz;
    zlo[nz] = tail_s[1]; zhi[nz] = INFINITY; ++nz;
    for (int j = 0; j < nh; ++j) {
      // the values whose y' = x - prior_mu, clamped into [y_lo, y_hi], can
      // lie in the interval (a few ulp wider: the rounding of y')
      const double l = hot->lo[j], h = hot->hi[j];
      const double a = l <= y_lo ? -INFINITY : (l + pm) - 8.0 * DBL_EPSILON * (fabs(l) + fabs(pm));
      const double b = h >= y_hi ? INFINITY : (h + pm) + 8.0 * DBL_EPSILON * (fabs(h) + fabs(pm));
      // ... widened by `tiles` pilot wave tiles (`halves` half tiles) on each
      // side: the tiles the draw keeps reach that far beyond the interval
      const int nt = halves >= 0 ? 2 * kPilotWaves : kPilotWaves;
      const int wide = halves >= 0 ? halves : tiles;
      const double *vmin = halves >= 0 ? hmin : tmin, *vmax = halves >= 0 ? hmax : tmax;
      int tf = 0, tl = nt - 1;
      while (tf < nt && !(vmax[tf] >= a)) ++tf;
      while (tl >= 0 && !(vmin[tl] <= b)) --tl;
      double za = a, zb = b;
      if (a != -INFINITY) {
        const int w = tf - wide;
        za = w < 0 ? -INFINITY : w < nt ? fmin(a, vmin[w]) : a;
      }
      if (b != INFINITY) {
        const int w = tl + wide;
        zb = w >= nt ? INFINITY : w >= 0 ? fmax(b, vmax[w]) : b;
      }
      zlo[nz] = za; zhi[nz] = zb; ++nz;
    }
    // by lower edge, overlapping or touching ones merged
    for (int i = 1; i < nz; ++i)
      for (int j = i; j > 0 && zlo[j] < zlo[j - 1]; --j) {
        const double a = zlo[j], b = zhi[j];
        zlo[j] = zlo[j - 1]; zhi[j] = zhi[j - 1];
        zlo[j - 1] = a; zhi[j - 1] = b;
      }
    int m = 0;
    for (int i = 1; i < nz; ++i) {
      if (zlo[i] <= zhi[m]) zhi[m] = fmax(zhi[m], zhi[i]);
      else { ++m; zlo[m] = zlo[i]; zhi[m] = zhi[i]; }
    }
    nz = m + 1;
    while (nz > kZoneMax) {  // the narrowest gap goes
      int g = 0;
      for (int i = 1; i + 1 < nz; ++i)
        if (zlo[i + 1] - zhi[i] < zlo[g + 1] - zhi[g]) g = i;
      zhi[g] = zhi[g + 1];
      for (int i = g + 1; i + 1 < nz; ++i) { zlo[i] = zlo[i + 1]; zhi[i] = zhi[i + 1]; }
      --nz;
    }
    // (one zone: everything would be inverted; the first zone starts at -inf
    // and the last ends at +inf by the tails)
    if (nz < 2 || zlo[0] != -INFINITY || zhi[nz - 1] != INFINITY) nz = 0;
    nz_s = nz;
    bad_s = 0;
    Z->nz = nz;
    for (int g = 0; g + 1 < nz; ++g) { Z->gap_lo[g] = zhi[g]; Z->gap_hi[g] = zlo[g + 1]; }
  }
  __syncthreads();
  const int nz = nz_s;
  if (nz == 0) return;
  const double *bw = A.mw + sb * A.kcap, *bmu = A.mmu + sb * A.kcap, *bsg = A.msig + sb * A.kcap;
  build_table(H, K, bw, bmu, bsg, T);
  // the table for k_draw_sorted_screen_run.  The draw's own build_table gives
  // these bits: with K <= kFuseTab every element sits in wave 0, one per
  // thread, in this block of 256 threads as in the draw's of 512
  static_assert(kFuseTab <= 64 && kFuseTab <= kZoneThreads, "the table's scan stays in wave 0");
  if (t < K) {
    Z->tcdf[t] = T.cdf[t];
    Z->tbase[t] = T.base[t];
    Z->tmass[t] = T.mass[t];
    Z->tmode[t] = T.mode[t];
  }
  if (gbits >= 0) {
    // pick boundary j: the smallest U in [0, 2^53] with cdf[j] <= fl(U 2^-53
    // cdf_last) -- the draw's own product, monotone in U -- by bisection
    const double cl = T.cdf[K - 1];
    if (t < kFuseTab) {
      uint64_t lo = 1ull << 53;
      if (t < K - 1) {
        const double cj = T.cdf[t];
        uint64_t hi = lo;
        lo = 0;
#pragma unroll 1
        while (lo < hi) {
          const uint64_t mid = (lo + hi) >> 1;
          if (cj <= ((double)mid * 0x1p-53) * cl) hi = mid;
          else lo = mid + 1;
        }
      }
      pb[t] = lo;
      if (t < K) {
        const double c = T.cdf[t];
        if (!(fabs(c) < INFINITY) || (t > 0 && !(c >= T.cdf[t - 1])) || !(cl > 0.0)) bad_s = 1;
      }
    }
    __syncthreads();
    const int sh = 53 - gbits;
    for (int b = t; b < (1 << gbits); b += kZoneThreads) {
      const uint64_t s0 = (uint64_t)b << sh, s1 = s0 + (1ull << sh);
      uint32_t kl = 0, c = 0;
      uint64_t val = 0;
      bool two = false;
      for (int j = 0; j < K - 1; ++j) {
        const uint64_t bj = pb[j];
        if (bj <= s0) ++kl;
        else if (bj < s1) {
          two |= c > 0 && bj != val;
          val = bj;
          ++c;
        }
      }
      Z->guide[b] = (uint16_t)(kl | (c << 8));
      if (two) bad_s = 1;
    }
    __syncthreads();
    if (bad_s) {  // (block-uniform)
      if (t == 0) Z->nz = 0;
      return;
    }
    if (t < kFuseTab) Z->pickB[t] = pb[t];
    if (t == 0) Z->gbits = gbits;
  }
  // threshold (k, e): the smallest u1 = j 2^-53 at which the edge is crossed
  // (1: none), by bisection on j
  const int E = 2 * (nz - 1);
  for (int idx = t; idx < K * E; idx += kZoneThreads) {
    const int k = idx / E, e = idx - k * E;
    const bool up = !(e & 1);
    const double edge = up ? zhi[e >> 1] : zlo[(e >> 1) + 1];
    const double mu = bmu[k], sg = bsg[k], b = T.base[k], m = T.mass[k];
    const int md = T.mode[k];
    uint64_t thr = 1ull << 53;
    if (m > 0.0 && fabs(m) < INFINITY && fabs(b) < INFINITY && sg > 0.0 && fabs(sg) < INFINITY &&
        fabs(mu) < INFINITY) {
      const double delta = margin * sg + 8.0 * DBL_EPSILON * (fabs(edge) + fabs(mu));
      const double v = up ? edge + delta : edge - delta;
      const double z = (v - mu) / (1.4142135623730951 * sg);
      const double tail = (md == 1 || (md == 0 && z >= 0.0)) ? 0.5 * erfc(z) : 0.5 * erfc(-z);
      uint64_t lo = 0, hi = 1ull << 53;
#pragma unroll 1
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (zone_crossed((double)mid * 0x1p-53, b, m, md, z, tail, up)) hi = mid;
        else lo = mid + 1;
      }
      thr = lo;
      if (!(tail == tail)) thr = 1ull << 53;
    }
    Z->thr[k][e] = (double)thr * 0x1p-53;
    if (gbits >= 0) Z->thrI[k][e] = thr;
  }
  __syncthreads();
  // nondecreasing in the edge (the margins of two close edges may cross: that
  // gap is empty); a component with a threshold of 1 at its first edge is
  // never cold
  for (int k = t; k < K; k += kZoneThreads) {
    double run = 0.0;
    for (int e = 0; e < E; ++e) {
      run = fmax(run, Z->thr[k][e]);
      Z->thr[k][e] = run;
    }
    if (gbits >= 0) {
      uint64_t runI = 0;
      for (int e = 0; e < E; ++e) {
        runI = max(runI, Z->thrI[k][e]);
        Z->thrI[k][e] = runI;
      }
    }
  }
}

hipError_t launch_draw_zone(const ScoreArgs &a, DrawZone *zones, int32_t tiles, int32_t halves,
                            int32_t tail, double margin, int32_t guide_bits, hipStream_t st) {
  const int64_t sbk = (int64_t)1 << a.sort_log2;
  if (a.n_slots <= 0 || a.n_suggest <= 0 || a.n_cand <= sbk) return hipSuccess;
  if (sbk != kSortedBlock || sbk != kPilotWaves * 128 || !zones || !a.tab_hot || !a.tab_hdr ||
      tiles < 0 || tail < 1 || tail > 128 || guide_bits > kGuideBitsMax)
    return hipErrorInvalidValue;
  k_draw_zone<<<dim3((unsigned)a.slot_rows, a.n_suggest), kZoneThreads, 0, st>>>(
      a, zones, tiles, halves < 0 ? -1 : halves, tail, margin, guide_bits < 0 ? -1 : guide_bits);
  return hipGetLastError();
}

// ------------------------------------------------------------------------
// k_draw_sorted_screen
// ------------------------------------------------------------------------
template <int NT>
struct ScreenLds {
  DrawTableT<kFuseTab> T;
  union {  // (a component's row: 80 bytes, so 16-byte reads of threshold pairs)
    double thr[kFuseTab * kZoneEdges];
    uint64_t thrI[kFuseTab * kZoneEdges];
  };
  uint32_t cnt[NT / 64 * kSortBuckets / 2];  // (SortedDrawLds::cnt)
  double red[2][NT / 64];
  unsigned char hotb[kSortBuckets], liveb[kSortBuckets];  // (PruneDrawLds')
  unsigned long long keep;
  int fail;
  int gapc[NT / 64][kZoneMax - 1];  // a wave's cold elements per gap
  int ncl[NT / 64];                 // a wave's inverted elements
  // a wave's inverted elements in index order: u1 (the integer screen: U1's
  // bits), then the value; the index in the block with the component, then
  // with the bucket, above bit 16
  double cx[NT / 64][kScreenList];
  uint32_t ci[NT / 64][kScreenList];
  // the integer screen's pick (DrawZone's)
  uint64_t pickB[kFuseTab];
  uint16_t guide[1 << kGuideBitsMax];
  // the slot's hot intervals (k_draw_sorted_screen_run: once per run)
  double hlo[kHotIv], hhi[kHotIv];
};
template <int CAP, int NT>
union ScreenUnion {
  PruneDrawLds<CAP, NT> P;
  ScreenLds<NT> S;
};
static_assert(sizeof(ScreenUnion<kFuseTab, kScreenThreads>) ==
                  sizeof(PruneDrawLds<kFuseTab, kScreenThreads>),
              "the screen's layout lies inside the pruning draw's");

// sorted_block_prune_body's bucket of a key in the block range
__device__ __forceinline__ int screen_bucket(double key, double lo, double scale) {
  int b = kSortBuckets - 1;
  if (fabs(key) < INFINITY) b = min(kSortBuckets - 1, max(0, (int)((key - lo) * scale)));
  return b;
}

// Phase 2 of a screened sort block and the composition of its kept tiles, for
// screened_block and screened_block_run: the wave's ncl inverted elements sit
// in its list, [lo, hi] is the block's key range and (y_lo, y_hi, nh) the head
// of the slot's hot intervals.  False: a live bucket may hold a cold element
// (nothing is written).
// HOTLDS: the hot intervals are in L.hlo, L.hhi (run_slot_lds).  POOL: phase 2
// takes the block's lists as one sequence in rows of 64 dealt to the waves
// (pool_slot); an element's count goes to its owner's row, so every count, byte
// and flag is the per-wave loop's.
template <int NT, bool POOL = false, bool HOTLDS = false>
__device__ __forceinline__ bool screen_compose(const ScoreArgs &A, int s, int hp, int64_t base,
                                               int64_t off, int n, int nz, int ncl, double lo,
                                               double hi, double mu, const TabHot *hot,
                                               double y_lo, double y_hi, int nh,
                                               const DrawZone *__restrict__ Z,
                                               int32_t *__restrict__ pos_out, ScreenLds<NT> &L,
                                               int t) {
  constexpr int NW = NT / 64;
  const int lane = t & 63, wv = t >> 6;
  double *cx = L.cx[wv];
  uint32_t *ci = L.ci[wv];
  uint32_t *mine = L.cnt + wv * (kSortBuckets / 2);
  double *out = const_cast<double *>(A.cand) + off;
  // phase 2: buckets and the hot test of the inverted elements, as
  // sorted_block_prune_body's second pass
  const double scale = hi > lo ? (double)kSortBuckets / (hi - lo) : 0.0;
  // element e of the lists (cx and ci as one array each), counted in row
  auto bucket_and_hot = [&](int e, uint32_t *row) {
    const double x = (&L.cx[0][0])[e];
    const int b = screen_bucket(x, lo, scale);
    uint32_t *ce = &L.ci[0][0] + e;
    *ce = (*ce & 0xffffu) | ((uint32_t)b << 16);
    __hip_atomic_fetch_add(&row[b >> 1], 1u << ((b & 1) * 16), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    const double y = x - mu;
    const double yc = fmin(fmax(y, y_lo), y_hi);
    bool hit = y != y;
    if constexpr (HOTLDS) {
      for (int q = 0; q < nh; ++q) hit |= yc >= L.hlo[q] && yc <= L.hhi[q];
    } else {
      for (int q = 0; q < nh; ++q) hit |= yc >= hot->lo[q] && yc <= hot->hi[q];
    }
    if (hit) L.hotb[b] = 1;
  };
  if constexpr (POOL) {
    const int total = pool_total<NW>(L.ncl), rows = pool_rows(total);
#pragma unroll 1
    for (int r = wv; r < rows; r += NW) {
      const int idx = r * 64 + lane;
      if (idx < total) {
        const PoolSlot o = pool_slot<NW>(L.ncl, idx);
        bucket_and_hot(o.w * kScreenList + o.j, L.cnt + o.w * (kSortBuckets / 2));
      }
    }
  } else {
#pragma unroll 1
    for (int j0 = 0; j0 < ncl; j0 += 64) {
      const int j = j0 + lane;
      if (j < ncl) bucket_and_hot(wv * kScreenList + j, mine);
    }
  }
  // a gap's cold elements: counted in the bucket of the zone edge below them
  // (their own buckets lie between that and the bucket of the edge above)
  if (lane < nz - 1) {
    const int c = L.gapc[wv][lane];
    if (c > 0) {
      const int b = screen_bucket(Z->gap_lo[lane], lo, scale);
      __hip_atomic_fetch_add(&mine[b >> 1], (uint32_t)c << ((b & 1) * 16), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  bucket_bases_scan<NW>(L.cnt);
  int bb = 0, be = 0;
  if (t < kSortBuckets) {
    bb = (int)((L.cnt[t >> 1] >> ((t & 1) * 16)) & 0xffffu);
    be = t == kSortBuckets - 1 ? n : (int)((L.cnt[(t + 1) >> 1] >> (((t + 1) & 1) * 16)) & 0xffffu);
    if (be > bb && L.hotb[t]) atomicOr(&L.keep, tile_bits(bb >> 7, (be - 1) >> 7));
  }
  __syncthreads();
  const unsigned long long keep = L.keep;
  if (t < kSortBuckets) {
    const bool live = be > bb && (keep & tile_bits(bb >> 7, (be - 1) >> 7)) != 0ull;
    L.liveb[t] = live ? 1 : 0;
    // a live bucket inside the bucket range a gap's cold elements can occupy:
    // its base or its members may differ from the full draw's
    if (live) {
      for (int g = 0; g < nz - 1; ++g) {
        int c = 0;
        for (int w = 0; w < NW; ++w) c += L.gapc[w][g];
        if (c > 0 && t >= screen_bucket(Z->gap_lo[g], lo, scale) &&
            t <= screen_bucket(Z->gap_hi[g], lo, scale))
          L.fail = 1;
      }
    }
  }
  __syncthreads();
  if (L.fail) return false;
  // every hot and every live bucket holds inverted elements only, and each
  // cold element's bucket is on its proxy's side of every live bucket: keep,
  // the live buckets' bases and the ranks are the full draw's
  int32_t *po = pos_out + off;
  double *__restrict__ wm = A.tab_wmax + ((int64_t)s * A.n_hp + hp) * A.pstride * 8 + (base >> 7);
  const int ntile = (n + 127) >> 7;
  if (t < ntile) wm[t] = ((keep >> t) & 1ull) ? INFINITY : -INFINITY;
#pragma unroll 1
  for (int j0 = 0; j0 < ncl; j0 += 64) {
    const int j = j0 + lane;
    const uint32_t ik = j < ncl ? ci[j] : 0u;
    const bool lv = j < ncl && L.liveb[ik >> 16] != 0;
    const int p = bucket_rank(mine, lv ? ik >> 16 : 0u, lv);
    if (lv && ((keep >> (p >> 7)) & 1ull)) {
      out[p] = cx[j];
      po[p] = (int32_t)(base + (ik & 0xffffu));
    }
  }
  return true;
}

// One sort block of a screened slot (Z.nz >= 2: a bounded GMM slot, not
// quantized, K <= CAP, pruned by sorted_block_prune_body).  True: the block's
// kept tiles and tab_wmax marks are written, as that body writes them.
// False: nothing is written (the caller runs that body).  Every thread of the
// block calls it; the result is block-uniform.  nexact: the inverted elements.
// INT: phase 1 on the integer uniforms (DrawZone's integer form): the same
// component and the same class of every element, without a double.
template <int CAP, int NT, bool INT>
__device__ __forceinline__ bool screened_block(const ScoreArgs &A, int slot, int s, int64_t base,
                                               int32_t *__restrict__ pos_out,
                                               const DrawZone *__restrict__ Z, int nz,
                                               ScreenLds<NT> &L, int &nexact) {
  constexpr int NW = NT / 64;
  const int hp = A.level_hps[slot];
  const tpe_hp H = A.hps[hp];
  const int64_t sb = 2 * (int64_t)hp;
  const double *bw = A.mw + sb * A.kcap, *bmu = A.mmu + sb * A.kcap, *bsg = A.msig + sb * A.kcap;
  const int K = A.info[sb].K;
  build_table(H, K, bw, bmu, bsg, L.T);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int E = 2 * (nz - 1);
  int gsh = 0;  // (the guide's bucket of r.x: (r.x >> 1) >> gsh)
  if constexpr (INT) {
    // (the edges from E up: none, so that phase 1 reads them in fixed groups)
    for (int idx = t; idx < K * kZoneEdges; idx += NT)
      L.thrI[idx] = idx % kZoneEdges < E ? (&Z->thrI[0][0])[idx] : 1ull << 53;
    const int G = min(max(__builtin_amdgcn_readfirstlane(Z->gbits), 0), kGuideBitsMax);
    gsh = 31 - G;
    for (int idx = t; idx < (1 << G); idx += NT) L.guide[idx] = Z->guide[idx];
    if (t < kFuseTab) L.pickB[t] = Z->pickB[t];
  } else {
    for (int idx = t; idx < K * kZoneEdges; idx += NT) L.thr[idx] = (&Z->thr[0][0])[idx];
  }
  if (t < kSortBuckets) L.hotb[t] = 0;
  if (t == 0) { L.keep = 0ull; L.fail = 0; }
  __syncthreads();
  const uint64_t seed = suggestion_seed(A, s);
  const int n = (int)min<int64_t>((int64_t)1 << A.sort_log2, A.n_cand - base);
  const int64_t off = (int64_t)s * A.cand_sstride + (int64_t)slot * A.n_cand + base;
  // the wave's rows: bucket_bases' [r0, r1)
  const int per = ((n + NW * 64 - 1) / (NW * 64)) * 64;
  int r0 = wv * per, r1 = min(n, r0 + per);
  if constexpr (INT) {  // (wave-uniform: the row loop and its counters stay scalar)
    r0 = __builtin_amdgcn_readfirstlane(r0);
    r1 = __builtin_amdgcn_readfirstlane(r1);
  }
  const double cdf_last = L.T.cdf[K - 1];
  const double high_prev = nextafter(H.high, -INFINITY);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  double *cx = L.cx[wv];
  uint32_t *ci = L.ci[wv];
  // phase 1: Philox and the pick of every element; the ones inside a zone to
  // the wave's list, the others counted per gap
  int ncl = 0;  // (wave-uniform)
  int gc[kZoneMax - 1];
#pragma unroll
  for (int g = 0; g < kZoneMax - 1; ++g) gc[g] = 0;
#pragma unroll 1
  for (int rb = r0; rb < r1; rb += 64) {
    const int i = rb + lane;
    const bool v = i < r1;
    const uint64_t gi = (uint64_t)(A.cand_begin + base + i);
    const U4 r = philox(U4{(uint32_t)gi, (uint32_t)(gi >> 32), (uint32_t)hp, 0u}, k0, k1);
    double u1;
    int k, c = 0;
    if constexpr (INT) {
      // u53's integers: u0 = U0 2^-53, u1 = U1 2^-53
      const uint64_t U0 = ((uint64_t)(r.x >> 5) << 26) | (r.y >> 6);
      const uint64_t U1 = ((uint64_t)(r.z >> 5) << 26) | (r.w >> 6);
      const uint32_t ge = L.guide[(r.x >> 1) >> gsh];
      const uint32_t kl = ge & 0xffu;
      k = (int)(kl + (U0 >= L.pickB[kl] ? ge >> 8 : 0u));
      // the first two gaps' edges in one group of reads, the others (wave-
      // uniform: more than three zones) in a second
      const ulonglong2 *th = reinterpret_cast<const ulonglong2 *>(L.thrI + k * kZoneEdges);
      static_assert(kZoneEdges == 10, "five threshold pairs");
      {
        const ulonglong2 a = th[0], b = th[1];
        c = (U1 >= a.x ? 1 : 0) + (U1 >= a.y ? 1 : 0) + (U1 >= b.x ? 1 : 0) + (U1 >= b.y ? 1 : 0);
      }
      if (E > 4) {
        const ulonglong2 a = th[2], b = th[3], d = th[4];
        c += (U1 >= a.x ? 1 : 0) + (U1 >= a.y ? 1 : 0) + (U1 >= b.x ? 1 : 0) + (U1 >= b.y ? 1 : 0) +
             (U1 >= d.x ? 1 : 0) + (U1 >= d.y ? 1 : 0);
      }
      u1 = __longlong_as_double((long long)U1);  // (the list keeps U1's bits)
    } else {
      k = draw_bounded_pick<CAP>(L.T, K, cdf_last, r, u1);
      const double *th = L.thr + k * kZoneEdges;
      for (int e = 0; e < E; ++e) c += u1 >= th[e] ? 1 : 0;
    }
    // (the integer screen: lane masks of plain compares, combined as scalars,
    // and the lane's own bit back from the mask)
    const uint64_t vm = INT ? __builtin_amdgcn_ballot_w64(v) : 0ull;
    bool exact;
    uint64_t bal;
    if constexpr (INT) {
      bal = __builtin_amdgcn_ballot_w64((c & 1) == 0) & vm;
      exact = __builtin_amdgcn_inverse_ballot_w64(bal);
    } else {
      exact = v && !(c & 1);
      bal = __ballot(exact);
    }
    const int pos = ncl + __popcll(bal & below);
    if (exact && pos < kScreenList) {
      cx[pos] = u1;
      ci[pos] = (uint32_t)i | ((uint32_t)k << 16);
    }
    ncl += __popcll(bal);
    const int gap = (v && (c & 1)) ? (c >> 1) : -1;
#pragma unroll
    for (int g = 0; g < kZoneMax - 1; ++g) {
      if (g >= nz - 1) continue;
      if constexpr (INT) gc[g] += __popcll(__builtin_amdgcn_ballot_w64(c == 2 * g + 1) & vm);
      else gc[g] += __popcll(__ballot(gap == g));
    }
  }
  const bool over = ncl > kScreenList;  // (a list overflow: the block falls back)
  if (over) ncl = 0;
  if (lane == 0) {
    L.ncl[wv] = ncl;
#pragma unroll
    for (int g = 0; g < kZoneMax - 1; ++g) L.gapc[wv][g] = gc[g];
    if (over) L.fail = 1;
  }
  // the inversion of the listed elements, in dense rows
  double lo = INFINITY, hi = -INFINITY;
#pragma unroll 1
  for (int j0 = 0; j0 < ncl; j0 += 64) {
    const int j = j0 + lane;
    const bool v = j < ncl;
    double u1 = v ? cx[j] : 0.5;
    if constexpr (INT) {  // u53's value of U1, by its operations
      const uint64_t U1 = v ? (uint64_t)__double_as_longlong(cx[j]) : 1ull << 52;
      u1 = ((double)(uint32_t)(U1 >> 26) * 67108864.0 + (double)(uint32_t)(U1 & 0x3ffffffu)) *
           (1.0 / 9007199254740992.0);
    }
    const int k = v ? (int)(ci[j] >> 16) : 0;
    const double x = draw_bounded_invert<CAP>(L.T, k, u1, bmu, bsg, H.low, H.high, high_prev, false,
                                              false, 0.0);
    if (v) {
      cx[j] = x;
      if (fabs(x) < INFINITY) { lo = fmin(lo, x); hi = fmax(hi, x); }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) { L.red[0][wv] = lo; L.red[1][wv] = hi; }
  uint32_t *mine = L.cnt + wv * (kSortBuckets / 2);
  for (int b = lane; b < kSortBuckets / 2; b += 64) mine[b] = 0u;
  __syncthreads();
  lo = INFINITY; hi = -INFINITY;
  nexact = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    lo = fmin(lo, L.red[0][w]);
    hi = fmax(hi, L.red[1][w]);
    nexact += L.ncl[w];
  }
  // every cold element lies strictly between the tails' edges: with an
  // inverted element at or beyond each, the key range is the full draw's
  if (L.fail || !(lo <= Z->gap_lo[0]) || !(hi >= Z->gap_hi[nz - 2])) return false;
  const double mu = H.prior_mu;
  const TabHot *hot = A.tab_hot + ((int64_t)s * A.n_hp + hp);
  const double y_lo = hot->y_lo, y_hi = hot->y_hi;
  int nh = 0;
  while (nh < kHotIv && hot->lo[nh] <= hot->hi[nh]) ++nh;
  return screen_compose<NT>(A, s, hp, base, off, n, nz, ncl, lo, hi, mu, hot, y_lo, y_hi, nh, Z,
                            pos_out, L, t);
}

// k_draw_sorted_prune with the screen: the same grid, the same slots; a slot
// k_draw_zone left no zones for, and a sort block whose screen cannot prove
// its layout, run sorted_block_prune_body.
template <int CAP, bool FAST, bool INT>
__device__ __forceinline__ void draw_sorted_screen_body(const ScoreArgs &A,
                                                        int32_t *__restrict__ pos_out,
                                                        const DrawZone *__restrict__ zones,
                                                        unsigned long long *stats) {
  static_assert(CAP == kFuseTab && FAST, "the small-table inline draw only");
  // (16-byte aligned: the integer screen reads ScreenLds::thrI in pairs)
  __shared__ __attribute__((aligned(16))) ScreenUnion<CAP, kScreenThreads> U;
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
  const int64_t base = (int64_t)(blockIdx.x + 1) << A.sort_log2;
  const DrawZone *Z = zones + ((int64_t)s * A.n_hp + hp);
  // (k_draw_zone leaves zones for KIND_LSE_GW slots only)
  const int nz = kind == KIND_LSE_GW ? __builtin_amdgcn_readfirstlane(Z->nz) : 0;
  if (nz >= 2 && nz <= kZoneMax) {
    int nexact = 0;
    const bool done = screened_block<CAP, kScreenThreads, INT>(A, slot, s, base, pos_out, Z, nz,
                                                               U.S, nexact);
    if (threadIdx.x == 0)
      atomicAdd(stats + (done ? 0 : 1), done ? (1ull << 40) | (unsigned long long)nexact : 1ull);
    if (done) return;
    __syncthreads();
  }
  sorted_block_prune_body<CAP, kScreenThreads, FAST>(
      A, slot, s, base, kind_lse(kind) || kind == KIND_ERF_G || kind == KIND_ERF_L,
      kind_logn(kind), tabk, pos_out, U.P);
}
template <int CAP, bool FAST>
__global__ __launch_bounds__(kScreenThreads) __attribute__((amdgpu_waves_per_eu(4)))
void k_draw_sorted_screen(ScoreArgs A, int32_t *__restrict__ pos_out,
                          const DrawZone *__restrict__ zones, unsigned long long *stats) {
  draw_sorted_screen_body<CAP, FAST, false>(A, pos_out, zones, stats);
}
// ... on the integer uniforms (zones of a k_draw_zone with gbits >= 0)
template <int CAP, bool FAST>
__global__ __launch_bounds__(kScreenThreads) __attribute__((amdgpu_waves_per_eu(4)))
void k_draw_sorted_screen_int(ScoreArgs A, int32_t *__restrict__ pos_out,
                              const DrawZone *__restrict__ zones, unsigned long long *stats) {
  draw_sorted_screen_body<CAP, FAST, true>(A, pos_out, zones, stats);
}

// ------------------------------------------------------------------------
// k_draw_sorted_screen_run
// ------------------------------------------------------------------------
// The integer screen with what the sort blocks of a slot share taken out of
// them.  A block draws a run of consecutive sort blocks of its (suggestion,
// slot row) and reads the slot's descriptors, seed, hot intervals' head and
// DrawZone once per run -- the draw table included, which k_draw_zone leaves
// there, so no sort block builds it.  Philox runs in the row form and the
// uniforms are compared in their word form (tpe_philox_row.hpp).  Every kept
// tile, position and mark is k_draw_sorted_screen_int's.

// a block-uniform value into scalar registers (a load behind the kernel's
// first store is a vector load, whatever its address)
__device__ __forceinline__ int run_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double run_uniform(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return __longlong_as_double((long long)(
      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32)) << 32) |
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b)));
}

// what the sort blocks of a run share (wave-uniform, but for m0lane)
struct RunSlot {
  int hp, K, nz, gsh, nh;
  uint32_t k0, k1;
  double low, high, high_prev, mu, y_lo, y_hi;
  double gap_first, gap_last;  // Z->gap_lo[0], Z->gap_hi[nz - 2]
  const double *bmu, *bsg;
  const TabHot *hot;
  uint64_t m0lane;             // philox_row_lane_term of the lane
};

// The slot's state in LDS: the draw table from the DrawZone, the thresholds
// and the pick boundaries in word form (the edges from E up: none), the guide.
// and the nh hot intervals.  The caller's barrier follows.
template <int NT>
__device__ __forceinline__ void run_slot_lds(const DrawZone *__restrict__ Z, int K, int nz, int G,
                                             const TabHot *hot, int nh, ScreenLds<NT> &L, int t) {
  const int E = 2 * (nz - 1);
  if (t < K) {
    L.T.cdf[t] = Z->tcdf[t];
    L.T.base[t] = Z->tbase[t];
    L.T.mass[t] = Z->tmass[t];
    L.T.mode[t] = Z->tmode[t];
  }
  for (int idx = t; idx < K * kZoneEdges; idx += NT)
    L.thrI[idx] = u53_word_threshold(idx % kZoneEdges < E ? (&Z->thrI[0][0])[idx] : 1ull << 53);
  for (int idx = t; idx < (1 << G); idx += NT) L.guide[idx] = Z->guide[idx];
  if (t < kFuseTab) L.pickB[t] = u53_word_threshold(Z->pickB[t]);
  if (t < nh) { L.hlo[t] = hot->lo[t]; L.hhi[t] = hot->hi[t]; }
}

// screened_block<CAP, NT, true> for one sort block of a run: the slot's LDS
// state is in place (run_slot_lds) and hotb, keep and fail are reset, both
// behind a barrier.  t: the thread's index in the block.  POOL: the inversion
// and phase 2 in rows of 64 across the block's lists (tpe_screen_pool.hpp), one
// barrier more; the rank and store loop stays per wave, in list order.
template <int CAP, int NT, bool POOL>
__device__ __forceinline__ bool screened_block_run(const ScoreArgs &A, const RunSlot &R, int slot,
                                                   int s, int64_t base,
                                                   int32_t *__restrict__ pos_out,
                                                   const DrawZone *__restrict__ Z,
                                                   ScreenLds<NT> &L, int t, int &nexact) {
  constexpr int NW = NT / 64;
  const int lane = t & 63, wv = t >> 6;
  const int nz = R.nz, E = 2 * (nz - 1), gsh = R.gsh;
  const int n = (int)min<int64_t>((int64_t)1 << A.sort_log2, A.n_cand - base);
  const int64_t off = (int64_t)s * A.cand_sstride + (int64_t)slot * A.n_cand + base;
  const int per = ((n + NW * 64 - 1) / (NW * 64)) * 64;
  const int r0 = __builtin_amdgcn_readfirstlane(wv * per);
  const int r1 = __builtin_amdgcn_readfirstlane(min(n, wv * per + per));
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  double *cx = L.cx[wv];
  uint32_t *ci = L.ci[wv];
  // phase 1, as screened_block's integer one
  int ncl = 0;  // (wave-uniform)
  int gc[kZoneMax - 1];
#pragma unroll
  for (int g = 0; g < kZoneMax - 1; ++g) gc[g] = 0;
#pragma unroll 1
  for (int rb = r0; rb < r1; rb += 64) {
    const int i = rb + lane;
    const bool v = i < r1;
    // the row's first counter, wave-uniform; its lanes' are g0 + lane
    const uint64_t gr = (uint64_t)(A.cand_begin + base + rb);
    const uint64_t g0 =
        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(gr >> 32)) << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)gr);
    PhiloxWords r;
    if (philox_row_ok((uint32_t)g0)) {  // (a scalar branch)
      PhiloxRow row = philox_row_setup(g0, (uint32_t)R.hp, R.k0, R.k1);
      // (the uniform product through an empty asm statement: it stays a scalar
      // one, not folded with the lane's term into a per-lane multiply-add)
      asm volatile("" : "+s"(row.p0));
      r = philox_row(row, R.m0lane, R.k0, R.k1);
    } else {  // the low word wraps inside the row
      const uint64_t gi = g0 + (uint64_t)lane;
      const U4 q = philox(U4{(uint32_t)gi, (uint32_t)(gi >> 32), (uint32_t)R.hp, 0u}, R.k0, R.k1);
      r = PhiloxWords{q.x, q.y, q.z, q.w};
    }
    const uint64_t W0 = u53_word(r.x, r.y), W1 = u53_word(r.z, r.w);
    const uint32_t ge = L.guide[(r.x >> 1) >> gsh];
    const uint32_t kl = ge & 0xffu;
    const int k = (int)(kl + (W0 >= L.pickB[kl] ? ge >> 8 : 0u));
    const ulonglong2 *th = reinterpret_cast<const ulonglong2 *>(L.thrI + k * kZoneEdges);
    static_assert(kZoneEdges == 10, "five threshold pairs");
    int c;
    {
      const ulonglong2 a = th[0], b = th[1];
      c = (W1 >= a.x ? 1 : 0) + (W1 >= a.y ? 1 : 0) + (W1 >= b.x ? 1 : 0) + (W1 >= b.y ? 1 : 0);
    }
    if (E > 4) {
      const ulonglong2 a = th[2], b = th[3], d = th[4];
      c += (W1 >= a.x ? 1 : 0) + (W1 >= a.y ? 1 : 0) + (W1 >= b.x ? 1 : 0) + (W1 >= b.y ? 1 : 0) +
           (W1 >= d.x ? 1 : 0) + (W1 >= d.y ? 1 : 0);
    }
    const uint64_t vm = __builtin_amdgcn_ballot_w64(v);
    const uint64_t bal = __builtin_amdgcn_ballot_w64((c & 1) == 0) & vm;
    const bool exact = __builtin_amdgcn_inverse_ballot_w64(bal);
    const int pos = ncl + __popcll(bal & below);
    if (exact && pos < kScreenList) {
      cx[pos] = __longlong_as_double((long long)W1);  // (the list keeps U1's word form)
      ci[pos] = (uint32_t)i | ((uint32_t)k << 16);
    }
    ncl += __popcll(bal);
#pragma unroll
    for (int g = 0; g < kZoneMax - 1; ++g) {
      if (g >= nz - 1) continue;
      gc[g] += __popcll(__builtin_amdgcn_ballot_w64(c == 2 * g + 1) & vm);
    }
  }
  const bool over = ncl > kScreenList;  // (a list overflow: the block falls back)
  if (over) ncl = 0;
  if (lane == 0) {
    L.ncl[wv] = ncl;
#pragma unroll
    for (int g = 0; g < kZoneMax - 1; ++g) L.gapc[wv][g] = gc[g];
    if (over) L.fail = 1;
  }
  uint32_t *mine = L.cnt + wv * (kSortBuckets / 2);
  // the inversion of the listed elements, in dense rows
  double lo = INFINITY, hi = -INFINITY;
  // element e of the lists (cx and ci as one array each; an idle lane inverts
  // u1 = 0.5)
  auto invert = [&](int e, bool v) {
    double *xe = &L.cx[0][0] + e;
    const double u1 = u53_word_value(v ? (uint64_t)__double_as_longlong(*xe) : 1ull << 58);
    const int k = v ? (int)((&L.ci[0][0])[e] >> 16) : 0;
    const double x = draw_bounded_invert<CAP>(L.T, k, u1, R.bmu, R.bsg, R.low, R.high, R.high_prev,
                                              false, false, 0.0);
    if (v) {
      *xe = x;
      if (fabs(x) < INFINITY) { lo = fmin(lo, x); hi = fmax(hi, x); }
    }
  };
  if constexpr (POOL) {
    // the block's lists as one sequence, wave 0's first, in rows of 64 dealt
    // to the waves: ceil(sum / 64) rows, not a wave's own ceil(ncl / 64).  The
    // inversion is element by element and [lo, hi] a minimum and a maximum, so
    // every bit is the per-wave loop's.  (The counts are zeroed ahead of the
    // barrier: phase 2 adds to other waves' rows.)
    for (int b = lane; b < kSortBuckets / 2; b += 64) mine[b] = 0u;
    __syncthreads();
    const int total = pool_total<NW>(L.ncl), rows = pool_rows(total);
#pragma unroll 1
    for (int r = wv; r < rows; r += NW) {
      const int idx = r * 64 + lane;
      const bool v = idx < total;
      const PoolSlot o = pool_slot<NW>(L.ncl, v ? idx : 0);
      invert(o.w * kScreenList + o.j, v);
    }
  } else {
#pragma unroll 1
    for (int j0 = 0; j0 < ncl; j0 += 64) {
      const int j = j0 + lane;
      invert(wv * kScreenList + j, j < ncl);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) { L.red[0][wv] = lo; L.red[1][wv] = hi; }
  if constexpr (!POOL)
    for (int b = lane; b < kSortBuckets / 2; b += 64) mine[b] = 0u;
  __syncthreads();
  lo = INFINITY; hi = -INFINITY;
  nexact = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    lo = fmin(lo, L.red[0][w]);
    hi = fmax(hi, L.red[1][w]);
    nexact += L.ncl[w];
  }
  if (L.fail || !(lo <= R.gap_first) || !(hi >= R.gap_last)) return false;
  return screen_compose<NT, POOL, true>(A, s, R.hp, base, off, n, nz, ncl, lo, hi, R.mu, R.hot,
                                        R.y_lo, R.y_hi, R.nh, Z, pos_out, L, t);
}

// Block x of the grid takes the sort blocks x run + 1 .. min(x run + run, the
// last) of its row.  A sort block whose screen cannot prove its layout runs
// sorted_block_prune_body, which overwrites the union: those run behind the
// run's last screened sort block, so the slot's LDS state is loaded once.  The
// two counters get the run's totals.
template <int CAP, bool FAST, bool POOL>
__device__ __forceinline__ void draw_sorted_screen_run_body(const ScoreArgs &A,
                                                            int32_t *__restrict__ pos_out,
                                                            const DrawZone *__restrict__ zones,
                                                            unsigned long long *stats, int run) {
  static_assert(CAP == kFuseTab && FAST, "the small-table inline draw only");
  __shared__ __attribute__((aligned(16))) ScreenUnion<CAP, kScreenThreads> U;
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
  // the sort blocks behind the pilot's: 1 .. nsb; this block's: j0 + 1 .. j1
  const int nsb = (int)(((A.n_cand + ((int64_t)1 << A.sort_log2) - 1) >> A.sort_log2) - 1);
  const int j0 = (int)blockIdx.x * run, j1 = min(j0 + run, nsb);
  const bool bucket = kind_lse(kind) || kind == KIND_ERF_G || kind == KIND_ERF_L;
  const bool lg = kind_logn(kind);
  const DrawZone *Z = zones + ((int64_t)s * A.n_hp + hp);
  const int nz = kind == KIND_LSE_GW ? __builtin_amdgcn_readfirstlane(Z->nz) : 0;
  const bool scr = nz >= 2 && nz <= kZoneMax;  // (block-uniform)
  RunSlot R{};
  if (scr) {
    const tpe_hp &H = A.hps[hp];
    const int64_t sb = 2 * (int64_t)hp;
    const uint64_t seed = suggestion_seed(A, s);
    R.hp = hp;
    R.K = run_uniform(A.info[sb].K);
    R.nz = nz;
    R.gsh = 31 - min(max(__builtin_amdgcn_readfirstlane(Z->gbits), 0), kGuideBitsMax);
    R.k0 = (uint32_t)run_uniform((int)(uint32_t)seed);
    R.k1 = (uint32_t)run_uniform((int)(uint32_t)(seed >> 32));
    R.low = run_uniform(H.low);
    R.high = run_uniform(H.high);
    R.high_prev = run_uniform(nextafter(H.high, -INFINITY));
    R.mu = run_uniform(H.prior_mu);
    R.bmu = A.mmu + sb * A.kcap;
    R.bsg = A.msig + sb * A.kcap;
    R.hot = A.tab_hot + ((int64_t)s * A.n_hp + hp);
    R.y_lo = run_uniform(R.hot->y_lo);
    R.y_hi = run_uniform(R.hot->y_hi);
    while (R.nh < kHotIv && R.hot->lo[R.nh] <= R.hot->hi[R.nh]) ++R.nh;
    R.nh = run_uniform(R.nh);
    R.gap_first = run_uniform(Z->gap_lo[0]);
    R.gap_last = run_uniform(Z->gap_hi[nz - 2]);
    R.m0lane = philox_row_lane_term(threadIdx.x & 63);
  }
  unsigned long long screened = 0ull;  // (blocks screened << 40 | elements inverted)
  // the run's sort blocks left to sorted_block_prune_body (bit j - j0): all of
  // a slot without zones, else the ones whose screen could not prove its layout
  static_assert(kScreenRunMax <= 31, "a run's sort blocks: one mask");
  uint32_t todo = scr ? 0u : (1u << (j1 - j0)) - 1u;
  if (scr) {
    run_slot_lds(Z, R.K, nz, 31 - R.gsh, R.hot, R.nh, U.S, (int)threadIdx.x);
#pragma unroll 1
    for (int j = j0; j < j1; ++j) {
      // (the thread's index through an empty asm statement: what a sort block
      // derives from it -- its lane masks and addresses -- is computed per
      // sort block, not kept in registers, phase beside phase, across the run)
      int t = threadIdx.x;
      asm volatile("" : "+v"(t));
      // (the sort block before this one may still be read)
      if (j > j0) __syncthreads();
      if (t < kSortBuckets) U.S.hotb[t] = 0;
      if (t == 0) { U.S.keep = 0ull; U.S.fail = 0; }
      __syncthreads();
      int nexact = 0;
      if (screened_block_run<CAP, kScreenThreads, POOL>(A, R, slot, s, (int64_t)(j + 1) << A.sort_log2,
                                                  pos_out, Z, U.S, t, nexact))
        screened += (1ull << 40) | (unsigned long long)nexact;
      else
        todo |= 1u << (j - j0);
    }
  }
  // (behind the run's screened sort blocks, in a loop of their own: that body
  // overwrites the union, and its registers stay out of the loop above)
  const int fallen = scr ? __popc(todo) : 0;
#pragma unroll 1
  for (int j = j0; todo != 0u; ++j, todo >>= 1) {
    if (__builtin_expect_with_probability(!(todo & 1u), 1, 0.9999999)) continue;
    __syncthreads();
    // (the slot and the LDS address through an empty asm statement: nothing
    // of what that body derives from them is kept in registers across this
    // loop)
    int fslot = slot, fs = s;
    typedef PruneDrawLds<CAP, kScreenThreads> __attribute__((address_space(3))) *PruneLds;
    PruneLds lds = (PruneLds)&U.P;
    asm volatile("" : "+s"(fslot), "+s"(fs), "+v"(lds));
    sorted_block_prune_body<CAP, kScreenThreads, FAST>(A, fslot, fs, (int64_t)(j + 1) << A.sort_log2,
                                                       bucket, lg, tabk, pos_out,
                                                       *(PruneDrawLds<CAP, kScreenThreads> *)lds);
  }
  if (threadIdx.x == 0) {
    if (screened) atomicAdd(stats, screened);
    if (fallen) atomicAdd(stats + 1, (unsigned long long)fallen);
  }
}
template <int CAP, bool FAST, bool POOL>
__global__ __launch_bounds__(kScreenThreads) __attribute__((amdgpu_waves_per_eu(4)))
void k_draw_sorted_screen_run(ScoreArgs A, int32_t *__restrict__ pos_out,
                              const DrawZone *__restrict__ zones, unsigned long long *stats,
                              int32_t run) {
  draw_sorted_screen_run_body<CAP, FAST, POOL>(A, pos_out, zones, stats, run);
}

bool is_screen_run_kernel_fn(const void *f) {
  return f == reinterpret_cast<const void *>(&k_draw_sorted_screen_run<kFuseTab, true, false>) ||
         f == reinterpret_cast<const void *>(&k_draw_sorted_screen_run<kFuseTab, true, true>);
}
bool is_screen_draw_kernel_fn(const void *f) {
  return f == reinterpret_cast<const void *>(&k_draw_sorted_screen<kFuseTab, true>) ||
         f == reinterpret_cast<const void *>(&k_draw_sorted_screen_int<kFuseTab, true>) ||
         is_screen_run_kernel_fn(f);
}

hipError_t launch_draw_screened(const ScoreArgs &a, int32_t *pos_out, const DrawZone *zones,
                                unsigned long long *stats, bool integer, int32_t run, bool pool,
                                hipStream_t st) {
  const int64_t sbk = (int64_t)1 << a.sort_log2;
  if (a.n_slots <= 0 || a.n_suggest <= 0 || a.n_cand <= sbk) return hipSuccess;
  if (sbk != kSortedBlock || !a.tab_wmax || !a.tab_hot || !a.tab_hdr || !zones || !stats ||
      run < 0 || run > kScreenRunMax)
    return hipErrorInvalidValue;
  const int64_t nsb = (a.n_cand + sbk - 1) / sbk - 1;
  if (integer && run >= 1) {
    const dim3 gr((unsigned)((nsb + run - 1) / run), (unsigned)a.slot_rows, a.n_suggest);
    if (pool)
      k_draw_sorted_screen_run<kFuseTab, true, true><<<gr, kScreenThreads, 0, st>>>(a, pos_out, zones,
                                                                                    stats, run);
    else
      k_draw_sorted_screen_run<kFuseTab, true, false><<<gr, kScreenThreads, 0, st>>>(
          a, pos_out, zones, stats, run);
    return hipGetLastError();
  }
  const dim3 g((unsigned)nsb, (unsigned)a.slot_rows, a.n_suggest);
  if (integer)
    k_draw_sorted_screen_int<kFuseTab, true><<<g, kScreenThreads, 0, st>>>(a, pos_out, zones, stats);
  else
    k_draw_sorted_screen<kFuseTab, true><<<g, kScreenThreads, 0, st>>>(a, pos_out, zones, stats);
  return hipGetLastError();
}

}  // namespace tpe
