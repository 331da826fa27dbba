// =====================================================================================================
// mw_feistel.h -- the integer-defined permutations of the surrogate trainers (mw_train.hip: the fixed models; mw_train_stack.hip: the
// dense stacks): splitmix64, the 32-bit round function, and the cycle-walked four-round Feistel network.  Restated in
// miniweatherml_amd/surrogate_train.py (feistel_permutation); the tests replay them.  Only inline functions: no kernel lives here.
// =====================================================================================================
#pragma once
#include <cstdint>

namespace mw {

// ---- the permutations (restated in miniweatherml_amd/surrogate_train.py; the tests replay them) ----
__host__ __device__ __forceinline__ uint64_t sm64(uint64_t z) {         // splitmix64 (include/mw_cdna4.h, "Substitutions")
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {        // round function: a 32-bit integer hash (lowbias32)
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
static constexpr uint64_t TAG_PRESHUFFLE = ~0ull;                        // stream tags: epoch e uses tag e

struct Feistel { uint32_t k[4]; uint32_t mask; int h; long long n; };
// The permutation of [0, n) for the stream (a, tag): base = sm64(sm64(a) ^ tag), round key r = high word of sm64(base + r); the domain is
// 4^h >= n (h >= 1), x = (L << h) | R, four rounds (L, R) <- (R, L ^ (mix32(R ^ k_r) & mask)), then cycle-walking until the value is < n.
__host__ __device__ inline Feistel make_feistel(uint64_t a, uint64_t tag, long long n) {
  Feistel F;
  const uint64_t base = sm64(sm64(a) ^ tag);
  for (int r = 0; r < 4; r++) F.k[r] = (uint32_t)(sm64(base + (uint64_t)r) >> 32);
  int h = 1;
  while (h < 32 && (1ll << (2 * h)) < n) h++;
  F.h = h; F.mask = (uint32_t)((1ull << h) - 1); F.n = n;
  return F;
}
__device__ __forceinline__ long long feistel_index(const Feistel &F, long long p) {
  uint64_t x = (uint64_t)p;
  do {
    uint32_t L = (uint32_t)(x >> F.h), R = (uint32_t)x & F.mask;
#pragma unroll
    for (int r = 0; r < 4; r++) { const uint32_t t = L ^ (mix32(R ^ F.k[r]) & F.mask); L = R; R = t; }
    x = ((uint64_t)L << F.h) | R;
  } while (x >= (uint64_t)F.n);
  return (long long)x;
}

} // namespace mw
