// Pattern and operand generators shared by the gpucheck kernels and the host
// reference. Everything here is plain integer C++ so device and host compute
// bit-identical values.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GPUCHECK_HD __host__ __device__
#else
#define GPUCHECK_HD
#endif

namespace gpucheck {

struct Vec16 {
  uint64_t lo;
  uint64_t hi;
};

// splitmix64 finalizer: a full-avalanche 64-bit mixing hash.
GPUCHECK_HD inline uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The 16 bytes stored at logical vector `vec_index` (base_index + i, 64-bit)
// in pass `pass`. An odd pass is the bitwise complement of the even pass
// before it, so every cell is tested holding a 0 and a 1.
GPUCHECK_HD inline Vec16 pattern(uint64_t seed, uint32_t pass,
                                 uint64_t vec_index) {
  const uint64_t key = mix64(seed ^ (static_cast<uint64_t>(pass & ~1u) << 32));
  Vec16 v;
  v.lo = mix64(vec_index ^ key);
  v.hi = mix64(v.lo + vec_index);
  if (pass & 1u) {
    v.lo = ~v.lo;
    v.hi = ~v.hi;
  }
  return v;
}

// MFMA self-test operands: integers in [-3, 3], a function of
// (seed, global wave id, which matrix, element index).
constexpr int kMfmaM = 32;
constexpr int kMfmaN = 32;
constexpr int kMfmaK = 128;  // 8 chained 32x32x16 steps

GPUCHECK_HD inline uint64_t mfma_key(uint64_t seed, uint32_t wave,
                                     uint32_t which) {
  return mix64(seed ^ mix64((static_cast<uint64_t>(wave) << 1) | which));
}

GPUCHECK_HD inline int mfma_value(uint64_t key, uint32_t elem) {
  return static_cast<int>(mix64(key + elem) % 7u) - 3;
}

// A is [32][128] row-major, B is [128][32] row-major; B[k][c] and B[c][k]
// hash different element indices, so B is not symmetric.
GPUCHECK_HD inline int mfma_a(uint64_t key_a, int row, int k) {
  return mfma_value(key_a, static_cast<uint32_t>(row * kMfmaK + k));
}
GPUCHECK_HD inline int mfma_b(uint64_t key_b, int k, int col) {
  return mfma_value(key_b, static_cast<uint32_t>(k * kMfmaN + col));
}

// bf16 bit pattern of an integer in [-3, 3] (all exactly representable).
GPUCHECK_HD inline uint16_t bf16_bits_small_int(int v) {
  const int a = v < 0 ? -v : v;
  const uint16_t mag = a == 0 ? 0x0000 : a == 1 ? 0x3F80 : a == 2 ? 0x4000
                                                                  : 0x4040;
  return static_cast<uint16_t>(mag | (v < 0 ? 0x8000 : 0));
}

}  // namespace gpucheck
