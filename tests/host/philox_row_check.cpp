// philox_row_check.cpp -- host-only checks of tpe_philox_row.hpp: the row form
// of Philox4x32-10 against the general one, and the word form of the 53-bit
// uniforms against the integers it stands for.  The reference below is
// Philox4x32-10 written out from its definition (Salmon et al., "Parallel
// random numbers: as easy as 1, 2, 3", SC'11) -- the arithmetic of the
// device's philox() in tpe_draw.hpp -- and is itself checked against the
// known answers of the Random123 distribution.
// Built and run by tests/test_philox_row_host.py; exit status 0: all passed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../hyperopt_amd/csrc/tpe_philox_row.hpp"

using namespace tpe;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (failures < 20)                                             \
        std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

struct W4 { uint32_t x, y, z, w; };
static W4 philox_ref(W4 c, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c = W4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
static bool same(const PhiloxWords &a, const W4 &b) {
  return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}
// u53 of tpe_draw.hpp and its integer
static uint64_t u53_int(uint32_t a, uint32_t b) { return ((uint64_t)(a >> 5) << 26) | (b >> 6); }
static double u53_ref(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

static void known_answers() {
  // Random123 kat_vectors, philox4x32 10 rounds
  W4 r = philox_ref(W4{0, 0, 0, 0}, 0, 0);
  CHECK(r.x == 0x6627e8d5u && r.y == 0xe169c58du && r.z == 0xbc57ac4cu && r.w == 0x9b00dbd8u);
  r = philox_ref(W4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, 0xffffffffu, 0xffffffffu);
  CHECK(r.x == 0x408f276du && r.y == 0x41c83b0eu && r.z == 0xa20bc7c6u && r.w == 0x6d5451fdu);
  r = philox_ref(W4{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, 0xa4093822u, 0x299f31d0u);
  CHECK(r.x == 0xd16cfe09u && r.y == 0x94fdccebu && r.z == 0x5001e420u && r.w == 0x24126ea1u);
  // philox_rounds from round 0 is the general form
  const PhiloxWords g = philox_rounds(PhiloxWords{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u},
                                      0xa4093822u, 0x299f31d0u, 0);
  CHECK(same(g, r));
}

// all 64 lanes of the row at g0: the row form where the predicate allows it,
// the general form (as the kernel takes it) otherwise
static void check_row(uint64_t g0, uint32_t hp, uint32_t k0, uint32_t k1, bool want_row) {
  const bool ok = philox_row_ok((uint32_t)g0);
  CHECK(ok == want_row);
  const PhiloxRow R = philox_row_setup(g0, hp, k0, k1);
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint64_t gi = g0 + lane;
    const W4 want = philox_ref(W4{(uint32_t)gi, (uint32_t)(gi >> 32), hp, 0u}, k0, k1);
    const uint64_t term = philox_row_lane_term(lane);
    CHECK(term < ((uint64_t)1 << 38));
    PhiloxWords got;
    if (ok) {
      CHECK(R.p0 <= UINT64_MAX - term);  // (the sum cannot overflow)
      got = philox_row(R, term, k0, k1);
    } else {
      got = philox_rounds(PhiloxWords{(uint32_t)gi, (uint32_t)(gi >> 32), hp, 0u}, k0, k1, 0);
    }
    CHECK(same(got, want));
  }
}

static void rows() {
  std::mt19937_64 rng(20240607);
  const uint32_t lows[] = {0u, 64u, 0x80000000u, 0xFFFFFF80u, 0xFFFFFFC0u};  // .., 2^32-128, 2^32-64
  const uint32_t highs[] = {0u, 1u, 0x7FFFFFFFu};
  const uint32_t hps[] = {0u, 1u, 99u, 0x7FFFFFFFu};
  for (int key = 0; key < 1000; ++key) {
    const uint64_t seed = rng();
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (uint32_t lo : lows)
      for (uint32_t hi : highs)
        for (uint32_t hp : hps) check_row(((uint64_t)hi << 32) | lo, hp, k0, k1, true);
  }
  // every low word whose row wraps goes to the general path, which is the
  // reference lane by lane across the wrap (the high word moves with it)
  for (uint32_t lo = 0xFFFFFFFFu - 62u;; ++lo) {
    const uint64_t seed = rng();
    for (uint32_t hi : highs)
      check_row(((uint64_t)hi << 32) | lo, 99u, (uint32_t)seed, (uint32_t)(seed >> 32), false);
    if (lo == 0xFFFFFFFFu) break;
  }
  CHECK(philox_row_ok(0xFFFFFFFFu - 63u) && !philox_row_ok(0xFFFFFFFFu - 62u));
}

static void check_word(uint32_t a, uint32_t b, uint64_t T) {
  const uint64_t U = u53_int(a, b);
  CHECK((u53_word(a, b) >= u53_word_threshold(T)) == (U >= T));
  const double got = u53_word_value(u53_word(a, b)), want = u53_ref(a, b);
  CHECK(std::memcmp(&got, &want, sizeof got) == 0);
}

static void words() {
  std::mt19937_64 rng(977);
  const uint64_t fixed[] = {0ull, 1ull, (1ull << 26) - 1, 1ull << 26, (1ull << 53) - 1, 1ull << 53};
  CHECK(u53_word_threshold(1ull << 53) == ((uint64_t)1 << 59) && u53_word_threshold(0) == 0);
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t q0 = rng(), q1 = rng();
    const uint32_t w[4] = {(uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32)};
    for (int p = 0; p < 2; ++p) {  // (both uniforms of the quadruple)
      const uint32_t a = w[2 * p], b = w[2 * p + 1];
      check_word(a, b, rng() % ((1ull << 53) + 1));
      const uint64_t U = u53_int(a, b);
      check_word(a, b, U);
      check_word(a, b, U + 1);
      if (U > 0) check_word(a, b, U - 1);
      if (i < 1000)
        for (uint64_t T : fixed) check_word(a, b, T);
    }
  }
  // the extreme uniforms against every fixed threshold
  for (uint64_t T : fixed) {
    check_word(0u, 0u, T);
    check_word(0xFFFFFFFFu, 0xFFFFFFFFu, T);
    check_word(0x1Fu, 0x3Fu, T);              // (the dropped low bits alone: U = 0)
    check_word(0x20u, 0u, T);                 // U = 2^26
    check_word(0u, 0xFFFFFFFFu, T);           // U = 2^26 - 1
  }
}

int main() {
  known_answers();
  rows();
  words();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("philox row checks passed\n");
  return 0;
}
