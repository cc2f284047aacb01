// tpe_pareto.hip -- multi-objective TPE: the history ranked by Pareto
// dominance on the device, gfx950 (tpe_plan_set_objectives).
//
// Every objective is minimised.  A row of Y[M][n] is complete when none of its
// objectives is NaN or +inf, pending otherwise.  For complete rows i and j,
// j dominates i when y_j[m] <= y_i[m] for every m and y_j[m] < y_i[m] for some
// m (IEEE comparison: -0.0 == +0.0, -inf an ordinary value).  k_pareto_count
// counts, for every row, the complete rows that dominate it (dominated_by: the
// Fonseca-Fleming rank, 0 on the nondominated set) and the complete rows it
// dominates; k_pareto_loss turns the two into the surrogate loss
//   s_i = dominated_by[i] (n + 1) + (n - dominates[i])
// (+inf for a pending row), whose order the good / bad split of the fit reads.
//
// k_pareto_count: a block owns a tile of kParetoTile rows i, one per lane, the
// row's M objectives in registers, and walks its share of the j tiles.  A j
// tile is staged in LDS as [M][tile]; in the pair loop every lane of a wave
// reads the same LDS address (a broadcast, no bank conflict).  A pending or
// out-of-range row is held as NaN in every objective, on both sides: every
// comparison with it is false, so it takes no part and needs no flag.  With
// a = (y_j <= y_i for all m) and b = (y_i <= y_j for all m), j dominates i iff
// a and not b, i dominates j iff b and not a: two comparisons per objective
// and pair.  The partial counts of the j-splits are combined with integer
// atomics, so the counts depend on Y alone, not on the launch shape.
#include <math.h>

#include "tpe_device.hpp"
#include "tpe_pareto_plan.hpp"

namespace tpe {

namespace {

// row r of Y as the count kernel holds it: NaN everywhere unless complete
template <int M>
__device__ __forceinline__ void pareto_row(const double *__restrict__ Y, int64_t ld, int64_t n,
                                           int64_t r, double (&y)[M]) {
  bool complete = r < n;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double v = r < n ? Y[(int64_t)m * ld + r] : NAN;
    y[m] = v;
    complete = complete && v == v && v != INFINITY;
  }
  if (!complete) {
#pragma unroll
    for (int m = 0; m < M; ++m) y[m] = NAN;
  }
}

template <int M>
__global__ __launch_bounds__(kParetoTile) void k_pareto_count(
    const double *__restrict__ Y, int64_t ld, int64_t n, int64_t per_split,
    int32_t *__restrict__ dominated_by, int32_t *__restrict__ dominates) {
  __shared__ double sy[M][kParetoTile];
  static_assert(sizeof(sy) <= kParetoLdsLimit, "the staged tile fits the plan's LDS limit");
  const int lane = threadIdx.x;
  const int64_t tiles = (n + kParetoTile - 1) / kParetoTile;
  const int64_t i = (int64_t)blockIdx.x * kParetoTile + lane;
  double yi[M];
  pareto_row<M>(Y, ld, n, i, yi);
  int32_t by = 0, of = 0;  // rows that dominate i, rows i dominates
  const int64_t t0 = (int64_t)blockIdx.y * per_split;
  const int64_t t1 = t0 + per_split < tiles ? t0 + per_split : tiles;
  for (int64_t t = t0; t < t1; ++t) {
    double yj[M];
    pareto_row<M>(Y, ld, n, t * kParetoTile + lane, yj);
    __syncthreads();  // (the last tile's readers are done)
#pragma unroll
    for (int m = 0; m < M; ++m) sy[m][lane] = yj[m];
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < kParetoTile; ++j) {
      bool a = true, b = true;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const double v = sy[m][j];
        a = a && v <= yi[m];
        b = b && yi[m] <= v;
      }
      by += (a && !b) ? 1 : 0;
      of += (b && !a) ? 1 : 0;
    }
  }
  if (i < n) {
    if (by) atomicAdd(&dominated_by[i], by);
    if (of) atomicAdd(&dominates[i], of);
  }
}

template <int M>
__global__ __launch_bounds__(kParetoTile) void k_pareto_loss(
    const double *__restrict__ Y, int64_t ld, int64_t n,
    const int32_t *__restrict__ dominated_by, const int32_t *__restrict__ dominates,
    double *__restrict__ losses) {
  const int64_t i = (int64_t)blockIdx.x * kParetoTile + threadIdx.x;
  if (i >= n) return;
  bool complete = true;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double v = Y[(int64_t)m * ld + i];
    complete = complete && v == v && v != INFINITY;
  }
  // (an exact integer: (n + 1)^2 < 2^53, tpe_pareto_plan.hpp)
  const int64_t s = (int64_t)dominated_by[i] * (n + 1) + (n - (int64_t)dominates[i]);
  losses[i] = complete ? (double)s : INFINITY;
}

template <int M>
hipError_t count_m(const double *Y, int64_t ld, int64_t n, int64_t per_split, int64_t splits,
                   int32_t *dominated_by, int32_t *dominates, hipStream_t st) {
  const int64_t tiles = (n + kParetoTile - 1) / kParetoTile;
  k_pareto_count<M><<<dim3((unsigned)tiles, (unsigned)splits), kParetoTile, 0, st>>>(
      Y, ld, n, per_split, dominated_by, dominates);
  return hipGetLastError();
}

template <int M>
hipError_t loss_m(const double *Y, int64_t ld, int64_t n, const int32_t *dominated_by,
                  const int32_t *dominates, double *losses, hipStream_t st) {
  const int64_t tiles = (n + kParetoTile - 1) / kParetoTile;
  k_pareto_loss<M><<<(unsigned)tiles, kParetoTile, 0, st>>>(Y, ld, n, dominated_by, dominates,
                                                            losses);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_pareto_count(const double *Y, int64_t ld, int64_t n, int32_t M,
                               int64_t per_split, int64_t splits, int32_t *dominated_by,
                               int32_t *dominates, hipStream_t st) {
  if (n < 1 || n > kParetoMaxN || n > ld || per_split < 1 || splits < 1 ||
      splits > kParetoMaxSplits)
    return hipErrorInvalidValue;
  switch (M) {
    case 1: return count_m<1>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    case 2: return count_m<2>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    case 3: return count_m<3>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    case 4: return count_m<4>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    case 5: return count_m<5>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    case 6: return count_m<6>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    case 7: return count_m<7>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    case 8: return count_m<8>(Y, ld, n, per_split, splits, dominated_by, dominates, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_pareto_loss(const double *Y, int64_t ld, int64_t n, int32_t M,
                              const int32_t *dominated_by, const int32_t *dominates,
                              double *losses, hipStream_t st) {
  if (n < 1 || n > kParetoMaxN || n > ld) return hipErrorInvalidValue;
  switch (M) {
    case 1: return loss_m<1>(Y, ld, n, dominated_by, dominates, losses, st);
    case 2: return loss_m<2>(Y, ld, n, dominated_by, dominates, losses, st);
    case 3: return loss_m<3>(Y, ld, n, dominated_by, dominates, losses, st);
    case 4: return loss_m<4>(Y, ld, n, dominated_by, dominates, losses, st);
    case 5: return loss_m<5>(Y, ld, n, dominated_by, dominates, losses, st);
    case 6: return loss_m<6>(Y, ld, n, dominated_by, dominates, losses, st);
    case 7: return loss_m<7>(Y, ld, n, dominated_by, dominates, losses, st);
    case 8: return loss_m<8>(Y, ld, n, dominated_by, dominates, losses, st);
    default: return hipErrorInvalidValue;
  }
}
static_assert(kParetoMaxObj == 8, "one instantiation per objective count");

}  // namespace tpe
