// tpe_constraint.hip -- constrained TPE: the history ranked by constrained
// dominance on the device, gfx950 (tpe_plan_set_constraints).
//
// Beside the objective matrix Y[M][n] of DESIGN 5.17 stands a constraint matrix
// G[C][n]; trial i is feasible when every G[c][i] <= 0.  Its violation is
//   v_i = ((0.0 + max0(G[0][i])) + max0(G[1][i])) + ...,  max0(g) = g > 0 ? g : 0.0
// in ascending c (additions only: nothing to fuse), +inf when any G[c][i] is
// NaN.  For complete rows i and j (5.17's rule, on Y alone), j c-dominates i
// when v_j < v_i, or when both are feasible (v = 0) and j Pareto-dominates i.
// The two counts and the surrogate column are 5.17's with c-dominance in the
// place of dominance; k_pareto_loss / k_hv_loss write the column.
//
// k_violation: one lane per row, a runtime loop over the C constraint rows
// (lane-contiguous, coalesced loads), one plain store of v.
//
// k_cdom_count: a block owns a tile of kParetoTile rows i, one per lane, the
// row's v and M objectives in registers, and walks its share of the j tiles,
// each staged in LDS as [M + 1][tile] (row 0: v) and read by broadcast.  Rows
// are held so that IEEE comparison alone decides every case:
//   pending / out of range:  v = NaN,   every y = NaN
//   infeasible:              v = v_i,   every y = NaN
//   feasible:                v = 0.0,   y = its objectives
// With a = (y_j <= y_i for all m) and b = (y_i <= y_j for all m),
//   j c-dominates i  iff  (v_j < v_i) || (a && !b)
//   i c-dominates j  iff  (v_i < v_j) || (b && !a).
// Feasible against infeasible: the v test fires, a and b are false (NaN).  Both
// infeasible: only the v test can fire (two +inf tie).  Both feasible: v ties
// at 0 and the Pareto test decides.  Pending: nothing fires.  No branch, one
// comparison pair per row pair over k_pareto_count.  The partial counts of the
// j-splits are combined with integer atomics: the counts depend on (Y, G)
// alone, not on the launch shape.
#include <math.h>

#include "tpe_device.hpp"
#include "tpe_pareto_plan.hpp"

namespace tpe {

namespace {

constexpr int kViolationBlock = 256;

__global__ __launch_bounds__(kViolationBlock) void k_violation(
    const double *__restrict__ G, int64_t ld, int64_t n, int32_t C, double *__restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * kViolationBlock + threadIdx.x;
  if (i >= n) return;
  double sum = 0.0;
  bool nan = false;
  for (int32_t c = 0; c < C; ++c) {
    const double g = G[(int64_t)c * ld + i];
    nan = nan || g != g;
    sum = sum + (g > 0.0 ? g : 0.0);
  }
  v[i] = nan ? INFINITY : sum;
}

// row r as the count kernel holds it (the table above); hv is the held v
template <int M>
__device__ __forceinline__ void cdom_row(const double *__restrict__ Y,
                                         const double *__restrict__ v, int64_t ld, int64_t n,
                                         int64_t r, double &hv, double (&y)[M]) {
  const bool in = r < n;
  bool complete = in;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double x = in ? Y[(int64_t)m * ld + r] : NAN;
    y[m] = x;
    complete = complete && x == x && x != INFINITY;
  }
  const double vr = in ? v[r] : NAN;            // >= 0 or +inf, never NaN (k_violation)
  const bool feasible = complete && !(vr > 0.0);
  hv = complete ? (feasible ? 0.0 : vr) : NAN;
  if (!feasible) {
#pragma unroll
    for (int m = 0; m < M; ++m) y[m] = NAN;
  }
}

template <int M>
__global__ __launch_bounds__(kParetoTile) void k_cdom_count(
    const double *__restrict__ Y, const double *__restrict__ v, int64_t ld, int64_t n,
    int64_t per_split, int32_t *__restrict__ dominated_by, int32_t *__restrict__ dominates) {
  __shared__ double sy[M + 1][kParetoTile];     // row 0: v, rows 1..M: the objectives
  static_assert(sizeof(sy) <= kParetoLdsLimit, "the staged tile fits the plan's LDS limit");
  const int lane = threadIdx.x;
  const int64_t tiles = (n + kParetoTile - 1) / kParetoTile;
  const int64_t i = (int64_t)blockIdx.x * kParetoTile + lane;
  double vi, yi[M];
  cdom_row<M>(Y, v, ld, n, i, vi, yi);
  int32_t by = 0, of = 0;  // rows that c-dominate i, rows i c-dominates
  const int64_t t0 = (int64_t)blockIdx.y * per_split;
  const int64_t t1 = t0 + per_split < tiles ? t0 + per_split : tiles;
  for (int64_t t = t0; t < t1; ++t) {
    double vj, yj[M];
    cdom_row<M>(Y, v, ld, n, t * kParetoTile + lane, vj, yj);
    __syncthreads();  // (the last tile's readers are done)
    sy[0][lane] = vj;
#pragma unroll
    for (int m = 0; m < M; ++m) sy[m + 1][lane] = yj[m];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < kParetoTile; ++j) {
      const double w = sy[0][j];
      bool a = true, b = true;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const double x = sy[m + 1][j];
        a = a && x <= yi[m];
        b = b && yi[m] <= x;
      }
      by += (w < vi || (a && !b)) ? 1 : 0;
      of += (vi < w || (b && !a)) ? 1 : 0;
    }
  }
  if (i < n) {
    if (by) atomicAdd(&dominated_by[i], by);
    if (of) atomicAdd(&dominates[i], of);
  }
}

template <int M>
hipError_t cdom_m(const double *Y, const double *v, int64_t ld, int64_t n, int64_t per_split,
                  int64_t splits, int32_t *dominated_by, int32_t *dominates, hipStream_t st) {
  const int64_t tiles = (n + kParetoTile - 1) / kParetoTile;
  k_cdom_count<M><<<dim3((unsigned)tiles, (unsigned)splits), kParetoTile, 0, st>>>(
      Y, v, ld, n, per_split, dominated_by, dominates);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_violation(const double *G, int64_t ld, int64_t n, int32_t C, double *v,
                            hipStream_t st) {
  if (n < 1 || n > kParetoMaxN || n > ld || C < 1 || C > kConstraintMax)
    return hipErrorInvalidValue;
  const int64_t blocks = (n + kViolationBlock - 1) / kViolationBlock;
  k_violation<<<(unsigned)blocks, kViolationBlock, 0, st>>>(G, ld, n, C, v);
  return hipGetLastError();
}

hipError_t launch_cdom_count(const double *Y, const double *v, int64_t ld, int64_t n, int32_t M,
                             int64_t per_split, int64_t splits, int32_t *dominated_by,
                             int32_t *dominates, hipStream_t st) {
  if (n < 1 || n > kParetoMaxN || n > ld || per_split < 1 || splits < 1 ||
      splits > kParetoMaxSplits)
    return hipErrorInvalidValue;
  switch (M) {
    case 1: return cdom_m<1>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    case 2: return cdom_m<2>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    case 3: return cdom_m<3>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    case 4: return cdom_m<4>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    case 5: return cdom_m<5>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    case 6: return cdom_m<6>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    case 7: return cdom_m<7>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    case 8: return cdom_m<8>(Y, v, ld, n, per_split, splits, dominated_by, dominates, st);
    default: return hipErrorInvalidValue;
  }
}
static_assert(kParetoMaxObj == 8, "one instantiation per objective count");

}  // namespace tpe
