// dropout_check.cpp — the Dropout mask function (ignnition_amd/csrc/dropout_rng.h) on the CPU, as a
// stand-alone program: Philox4x32-10 known answers, the counter / key / word layout of an element,
// a 64-bit group index, and the u == rate boundary.  Built with g++ (no HIP), plain and sanitized.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../ignnition_amd/csrc/dropout_rng.h"

using namespace ign;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static bool same(const Philox4& r, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  if (r.w[0] == a && r.w[1] == b && r.w[2] == c && r.w[3] == d) return true;
  printf("  got %08x %08x %08x %08x, expected %08x %08x %08x %08x\n", r.w[0], r.w[1], r.w[2], r.w[3], a, b, c, d);
  return false;
}

int main() {
  // known answers of Philox4x32-10 (counter, key -> output), as published with the algorithm
  CHECK(same(philox4x32_10(0, 0, 0, 0, 0, 0), 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u));
  CHECK(same(philox4x32_10(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu), 0x408f276du,
             0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu));
  CHECK(same(philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u), 0xd16cfe09u,
             0x94fdccebu, 0x5001e420u, 0x24126ea1u));

  // key = (seed low, seed high), counter = (g low, g high, site, step)
  const uint64_t seed = 0x299f31d0a4093822ull;
  CHECK(same(dropout_words(seed, 0x13198a2eu, 0x03707344u, 0x85a308d3243f6a88ull), 0xd16cfe09u, 0x94fdccebu, 0x5001e420u,
             0x24126ea1u));

  // element i: group i >> 2 (one generator call per four consecutive elements), word i & 3
  const uint32_t site = 3, step = 17;
  const float rate = 0.5f;
  for (uint64_t i = 0; i < 8; ++i) {
    const Philox4 r = philox4x32_10((uint32_t)(i >> 2), 0, site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t w = r.w[i & 3];
    CHECK(dropout_words(seed, site, step, i >> 2).w[i & 3] == w);
    CHECK(dropout_keep_at(seed, site, step, i, rate) == ((float)(w >> 8) * (1.0f / 16777216.0f) >= rate));
  }
  CHECK(dropout_words(seed, site, step, 0).w[0] != dropout_words(seed, site, step, 1).w[0]);
  // site and step are counter words of their own
  CHECK(dropout_words(seed, site + 1, step, 0).w[0] != dropout_words(seed, site, step, 0).w[0]);
  CHECK(dropout_words(seed, site, step + 1, 0).w[0] != dropout_words(seed, site, step, 0).w[0]);

  // a group index above 2^32: its high word is counter word 1, not dropped
  const uint64_t g = (1ull << 33) + 12345u;
  const Philox4 hi = dropout_words(seed, site, step, g);
  CHECK(same(hi, philox4x32_10(12345u, 2u, site, step, (uint32_t)seed, (uint32_t)(seed >> 32)).w[0],
             philox4x32_10(12345u, 2u, site, step, (uint32_t)seed, (uint32_t)(seed >> 32)).w[1],
             philox4x32_10(12345u, 2u, site, step, (uint32_t)seed, (uint32_t)(seed >> 32)).w[2],
             philox4x32_10(12345u, 2u, site, step, (uint32_t)seed, (uint32_t)(seed >> 32)).w[3]));
  CHECK(hi.w[0] != dropout_words(seed, site, step, 12345u).w[0]);
  const uint64_t i_big = (g << 2) | 1;   // element index above 2^34
  CHECK(dropout_keep_at(seed, site, step, i_big, rate) == dropout_keep_word(hi.w[1], rate));

  // the uniform: 24 bits, [0, 1); u == rate keeps the element (tf: random_uniform >= rate)
  CHECK(dropout_uniform(0u) == 0.0f);
  CHECK(dropout_uniform(0xffu) == 0.0f);
  CHECK(dropout_uniform(0x100u) == 1.0f / 16777216.0f);
  CHECK(dropout_uniform(0xffffffffu) == 16777215.0f / 16777216.0f);
  CHECK(dropout_uniform(0x80000000u) == 0.5f);
  CHECK(dropout_keep_word(0x80000000u, 0.5f));
  CHECK(!dropout_keep_word(0x7fffff00u, 0.5f));
  for (uint64_t k = 0; k < 64; ++k) {
    const uint32_t w = dropout_words(seed, site, step, k).w[k & 3];
    const float u = dropout_uniform(w);
    CHECK(u >= 0.0f && u < 1.0f);
    CHECK(dropout_keep_word(w, u));                          // u == rate: kept
    CHECK(!dropout_keep_word(w, std::nextafterf(u, 2.0f)));   // the next rate up: dropped
    CHECK(dropout_keep_word(w, 0.0f));
  }
  CHECK(dropout_scale(0.5f) == 2.0f);
  CHECK(dropout_scale(0.25f) == (float)(1.0 / 0.75));

  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("dropout_check: all checks passed\n");
  return 0;
}
