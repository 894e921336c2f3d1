// dropout_rng.h — the Dropout keep mask as a pure function of (seed, site, step, element), shared by
// the host (ign_dropout_keep, the tests' stand-alone check) and the device (dropout_kernels.hip).
// Plain C++17 with no HIP include; under hipcc the functions are __host__ __device__.
//
//   generator  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
//   key        (seed & 0xffffffff, seed >> 32)
//   counter    (g & 0xffffffff, g >> 32, site, step),  g = i >> 2,  i = row * units + unit (64-bit)
//   uniform    element i takes output word i & 3:  u = (word >> 8) * 2^-24  in [0, 1)
//   keep       u >= rate   (tf.nn.dropout: random_uniform >= rate)
// No mask is stored: the backward regenerates it from the same arguments.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IGN_RNG_HD __host__ __device__ inline
#else
#define IGN_RNG_HD inline
#endif

namespace ign {

struct Philox4 {
  uint32_t w[4];
};

IGN_RNG_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;   // Weyl increments between rounds
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the four output words of element group g = i >> 2
IGN_RNG_HD Philox4 dropout_words(uint64_t seed, uint32_t site, uint32_t step, uint64_t g) {
  return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
}

IGN_RNG_HD float dropout_uniform(uint32_t word) { return (float)(word >> 8) * 5.9604644775390625e-8f; }   // 2^-24, exact

IGN_RNG_HD bool dropout_keep_word(uint32_t word, float rate) { return dropout_uniform(word) >= rate; }

// element i of a site's mask
IGN_RNG_HD bool dropout_keep_at(uint64_t seed, uint32_t site, uint32_t step, uint64_t i, float rate) {
  return dropout_keep_word(dropout_words(seed, site, step, i >> 2).w[i & 3], rate);
}

// 1 / (1 - rate), once, in float32
IGN_RNG_HD float dropout_scale(float rate) { return 1.0f / (1.0f - rate); }

}  // namespace ign
