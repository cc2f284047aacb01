// tpe_philox_row.hpp -- Philox4x32-10 over a wave row of 64 consecutive
// counters, and the word form of the 53-bit uniforms (k_draw_sorted_screen_run,
// DESIGN 5.6).  Plain C++ (no builtins), host and device: tests/host/
// philox_row_check.cpp checks both against the reference forms on the CPU.
//
// The draw's counter is (lo32(gi), hi32(gi), hp, 0) under the key (k0, k1).
// Over a row gi = g0 + lane with lo32(g0) <= 2^32 - 64 the second word and the
// key are the same in every lane and the first word is lo32(g0) + lane without
// a carry, so
//  - round 1's M0 * (lo32(g0) + lane) is a uniform 64-bit product plus the
//    lane's constant M0 * lane (below 2^38; the sum is the product itself, so
//    it cannot overflow), and its M1 * hp is uniform: the round multiplies
//    nothing per lane;
//  - round 2's M0 * x is uniform, M1 * z its one per-lane multiply;
//  - round 3 still takes one uniform word, folded with its key.
// Rounds 4 to 10 are the general ones.  A row whose low word wraps
// (philox_row_ok false) takes the general form lane by lane.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TPE_HD inline
#endif

namespace tpe {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct PhiloxWords { uint32_t x, y, z, w; };

// rounds `from` .. 9 of Philox4x32-10 (k0, k1: the key of round `from`)
TPE_HD PhiloxWords philox_rounds(PhiloxWords c, uint32_t k0, uint32_t k1, int from) {
#pragma unroll
  for (int r = from; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c.x;
    const uint64_t p1 = (uint64_t)kPhiloxM1 * c.z;
    c = PhiloxWords{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1,
                    (uint32_t)p0};
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return c;
}

// the row form serves g0 when no lane's low word wraps
TPE_HD bool philox_row_ok(uint32_t g0_lo) { return g0_lo <= 0xFFFFFFFFu - 63u; }

// the row's uniform part (scalar registers on the device)
struct PhiloxRow {
  uint64_t p0;    // M0 * lo32(g0)
  uint32_t y2;    // round 2: lo(M1 hp) ^ its k0
  uint32_t z2;    // round 2: hi(M0 x1) ^ its k1
  uint32_t z3;    // round 3: lo(M0 x1) ^ its k1
};
TPE_HD PhiloxRow philox_row_setup(uint64_t g0, uint32_t hp, uint32_t k0, uint32_t k1) {
  const uint64_t p1 = (uint64_t)kPhiloxM1 * hp;
  const uint32_t x1 = (uint32_t)(p1 >> 32) ^ (uint32_t)(g0 >> 32) ^ k0;
  const uint64_t q0 = (uint64_t)kPhiloxM0 * x1;
  PhiloxRow R;
  R.p0 = (uint64_t)kPhiloxM0 * (uint32_t)g0;
  R.y2 = (uint32_t)p1 ^ (k0 + kPhiloxW0);
  R.z2 = (uint32_t)(q0 >> 32) ^ (k1 + kPhiloxW1);
  R.z3 = (uint32_t)q0 ^ (k1 + 2u * kPhiloxW1);
  return R;
}
// the lane's constant
TPE_HD uint64_t philox_row_lane_term(uint32_t lane) { return (uint64_t)kPhiloxM0 * lane; }
// the four words of counter g0 + lane (m0lane: philox_row_lane_term(lane))
TPE_HD PhiloxWords philox_row(const PhiloxRow &R, uint64_t m0lane, uint32_t k0, uint32_t k1) {
  const uint64_t p0 = R.p0 + m0lane;
  const uint32_t z1 = (uint32_t)(p0 >> 32) ^ k1, w1 = (uint32_t)p0;
  const uint64_t p1 = (uint64_t)kPhiloxM1 * z1;  // (round 2's only per-lane product)
  const uint32_t x2 = (uint32_t)(p1 >> 32) ^ R.y2, y2 = (uint32_t)p1, z2 = R.z2 ^ w1;
  const uint64_t a0 = (uint64_t)kPhiloxM0 * x2, a1 = (uint64_t)kPhiloxM1 * z2;
  const PhiloxWords c3{(uint32_t)(a1 >> 32) ^ y2 ^ (k0 + 2u * kPhiloxW0), (uint32_t)a1,
                       (uint32_t)(a0 >> 32) ^ R.z3, (uint32_t)a0};
  return philox_rounds(c3, k0 + 3u * kPhiloxW0, k1 + 3u * kPhiloxW1, 3);
}

// ------------------------------------------------------------------------
// The word form of a uniform.  u53(a, b) = U 2^-53 with the 53-bit integer
// U = (a >> 5) 2^26 + (b >> 6).  Its word form is the register pair
// (a >> 5 : b) read as one unsigned 64-bit number, a threshold's is
// (T >> 26 : (T mod 2^26) 2^6): U >= T iff the word forms compare so (equal
// high words leave b >= 64 (T mod 2^26), which is b >> 6 >= T mod 2^26).  The
// sentinel 2^53 becomes (2^27 : 0), above every uniform's (a >> 5 < 2^27).
// ------------------------------------------------------------------------
TPE_HD uint64_t u53_word(uint32_t a, uint32_t b) { return ((uint64_t)(a >> 5) << 32) | b; }
TPE_HD uint64_t u53_word_threshold(uint64_t T) {
  return ((T >> 26) << 32) | ((T & 0x3ffffffull) << 6);
}
// u53(a, b) of a uniform's word form, by u53's operations
TPE_HD double u53_word_value(uint64_t w) {
  return ((double)(uint32_t)(w >> 32) * 67108864.0 + (double)((uint32_t)w >> 6)) *
         (1.0 / 9007199254740992.0);
}

}  // namespace tpe
