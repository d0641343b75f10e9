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

// MX self-test: block-scaled FP8/BF8/FP4 operands for the 32x32x64 scaled
// MFMA. A is [32][256] row-major, B is [256][32] row-major, and every 32-wide
// k-block of a row of A (column of B) carries one E8M0 scale.
//
// Exactness. Element magnitudes are at most 7.5 (e4m3: m/2, m <= 15), 3.5
// (e5m2: m/2, m <= 7) and 6 (e2m1); all are multiples of 1/2. Scales are
// 2^-1, 1 and 2. A scaled product a.sa.b.sb is therefore a multiple of
// (1/2)^4 = 2^-4 of magnitude at most 7.5^2 . 4 = 225, and the magnitudes of
// the K = 256 products of one output sum to at most 256 . 225 = 57600. In
// units of 2^-4 that is 57600 . 16 = 921600 < 2^24, so every partial sum, in
// any order and grouping, is an integer below 2^24 in those units and exact in
// f32: the device result has one correct value and the host compares with ==.
constexpr int kMxK = 256;  // 4 chained 32x32x64 steps
constexpr int kMxBlock = 32;
constexpr int kMxFormats = 4;

// Element types, numbered as the instruction's cbsz/blgp fields number them.
constexpr int kMxE4M3 = 0;
constexpr int kMxE5M2 = 1;
constexpr int kMxE2M1 = 4;

struct MxFormat {
  const char* name;
  int a;  // element type of A
  int b;  // element type of B
};
constexpr MxFormat kMxFormatTable[kMxFormats] = {
    {"fp8", kMxE4M3, kMxE4M3},
    {"bf8", kMxE5M2, kMxE5M2},
    {"fp4", kMxE2M1, kMxE2M1},
    {"fp8xfp4", kMxE4M3, kMxE2M1},
};

// Bit 40 keeps these keys apart from mfma_key's (wave << 1 | which).
GPUCHECK_HD inline uint64_t mx_key(uint64_t seed, uint32_t wave,
                                   uint32_t format, uint32_t which) {
  return mix64(seed ^ mix64((1ull << 40) | (static_cast<uint64_t>(wave) << 3) |
                            (format << 1) | which));
}

// Bits of +m/2 in a format with `mant` mantissa bits and exponent bias
// `bias`, for 0 <= m < 2^(mant+1): m = 2^e . (1 + f) gives the exponent
// field e - 1 + bias and the fraction f in the top bits of the mantissa.
GPUCHECK_HD inline uint32_t mx_half_steps_bits(uint32_t m, int mant, int bias) {
  if (m == 0) return 0;
  int e = 0;
  while ((m >> (e + 1)) != 0) ++e;
  return (static_cast<uint32_t>(e - 1 + bias) << mant) |
         ((m - (1u << e)) << (mant - e));
}

// The code of one element from its hash: e2m1 takes any of its 16 codes;
// e4m3 is +-m/2 for m = 0..15 and e5m2 +-m/2 for m = 0..7, sign in bit 7.
// Only the low kMxHashBits bits of the hash are used.
constexpr int kMxHashBits = 5;
GPUCHECK_HD inline uint32_t mx_code_from_hash(int type, uint64_t h) {
  const uint32_t sign = static_cast<uint32_t>(h >> 4) & 1u;
  if (type == kMxE2M1) return static_cast<uint32_t>(h) & 15u;
  if (type == kMxE4M3)
    return (sign << 7) |
           mx_half_steps_bits(static_cast<uint32_t>(h) & 15u, 3, 7);
  return (sign << 7) | mx_half_steps_bits(static_cast<uint32_t>(h) & 7u, 2, 15);
}

// As above but never +-0 (which becomes +-1): the rate kernels' operands.
GPUCHECK_HD inline uint32_t mx_nonzero_code_from_hash(int type, uint64_t h) {
  const uint32_t c = mx_code_from_hash(type, h);
  if (type == kMxE2M1) return (c & 7u) ? c : (c | 2u);
  if ((c & 0x7Fu) != 0) return c;
  return c | (type == kMxE4M3 ? 0x38u : 0x3Cu);
}

// The hash of A[row][k] and of B[k][col]. B[k][c] and B[c][k] hash different
// element indices: B is not symmetric.
GPUCHECK_HD inline uint64_t mx_a_hash(uint64_t key_a, int row, int k) {
  return mix64(key_a + static_cast<uint32_t>(row * kMxK + k));
}
GPUCHECK_HD inline uint64_t mx_b_hash(uint64_t key_b, int k, int col) {
  return mix64(key_b + static_cast<uint32_t>(k * 32 + col));
}

// E8M0 scale byte (126, 127 or 128) of k-block `block` (k / 32) of row or
// column `rc`. The offset keeps the scale indices clear of the 8192 elements.
GPUCHECK_HD inline uint32_t mx_scale_byte(uint64_t key, int rc, int block) {
  return 126u + static_cast<uint32_t>(
                    mix64(key + 0x10000u +
                          static_cast<uint32_t>(rc * (kMxK / kMxBlock) + block)) %
                    3u);
}

// LDS self-test: one workgroup fills a compute unit's whole 160 KiB LDS with
// 10240 16-byte vectors. Vector i of workgroup `group` in `round` and `pass`
// holds pattern(lds_key(seed, group, round), pass, i), so an odd pass is the
// complement of the even one and every address has its own value: an
// aliased address bit (the 64 KiB line is vector 4096) cannot read back right.
constexpr int kLdsVectors = 10240;
constexpr int kLdsBytes = 16 * kLdsVectors;

// Bit 41 keeps these keys apart from mfma_key's and mx_key's.
GPUCHECK_HD inline uint64_t lds_key(uint64_t seed, uint32_t group,
                                    uint32_t round) {
  return mix64(seed ^ mix64((1ull << 41) |
                            (static_cast<uint64_t>(round) << 20) | group));
}

// Dense self-test: the non-scaled matrix instructions tenants issue most,
// one format per instruction. Every wave computes one square tile D = A.B of
// side `mn` with A [mn][k] and B [k][mn], both row-major, in k / step_k
// chained instructions.
//
// Exactness, per format (a product's magnitude times K bounds the sum of the
// magnitudes of one output's products, so every partial sum in any order and
// grouping is bounded by it):
//   f16, bf16x16: integers in [-15, 15]; |sum| <= 128 . 225 = 28800 < 2^24,
//                 exact in the f32 accumulator.
//   fp8, bf8:     multiples of 1/2 of magnitude at most 7.5 (e4m3) and 3.5
//                 (e5m2); a product is a multiple of 1/4 and the sum at most
//                 128 . 56.25 = 7200, 28800 quarter-units < 2^24: exact in f32.
//   i8:           all 256 codes; |sum| <= 128 . 2^14 = 2^21, exact in i32.
//   f32:          integers in [-511, 511]; |sum| <= 32 . 511^2 = 8355872
//                 < 2^24. The instruction is an fmaf chain, and every product
//                 and partial sum is an integer below 2^24: no rounding.
//   f64:          integers in [-(2^20 - 1), 2^20 - 1]; |sum| < 32 . 2^40 = 2^45
//                 < 2^53, exact in f64.
// So the device result has one correct value per element and the host
// compares with ==; NaN compares unequal. The wide f32, f64 and i8 ranges are
// deliberate: they put bits through the whole multiplier.
constexpr int kDenseFormats = 7;
constexpr int kDenseF16 = 0;
constexpr int kDenseBf16x16 = 1;
constexpr int kDenseFp8 = 2;
constexpr int kDenseBf8 = 3;
constexpr int kDenseI8 = 4;
constexpr int kDenseF32 = 5;
constexpr int kDenseF64 = 6;

struct DenseFormat {
  const char* name;
  int mn;      // the tile is mn x mn
  int k;       // summed over by k / step_k instructions
  int step_k;  // K of one instruction
  int scale;   // a result times this is an integer
};
constexpr DenseFormat kDenseFormatTable[kDenseFormats] = {
    {"f16", 32, 128, 16, 1},  {"bf16x16", 16, 128, 32, 1},
    {"fp8", 32, 128, 16, 4},  {"bf8", 32, 128, 16, 4},
    {"i8", 32, 128, 32, 1},   {"f32", 32, 32, 2, 1},
    {"f64", 16, 32, 4, 1},
};

// Bit 42 keeps these keys apart from mfma_key's, mx_key's and lds_key's.
GPUCHECK_HD inline uint64_t dense_key(uint64_t seed, uint32_t wave,
                                      uint32_t format, uint32_t which) {
  return mix64(seed ^ mix64((1ull << 42) | (static_cast<uint64_t>(wave) << 4) |
                            (format << 1) | which));
}

// The hash of A[row][k] and of B[k][col] of format `f`. B[k][c] and B[c][k]
// hash different element indices: B is not symmetric.
GPUCHECK_HD inline uint64_t dense_a_hash(int f, uint64_t key_a, int row, int k) {
  return mix64(key_a + static_cast<uint32_t>(row * kDenseFormatTable[f].k + k));
}
GPUCHECK_HD inline uint64_t dense_b_hash(int f, uint64_t key_b, int k, int col) {
  return mix64(key_b + static_cast<uint32_t>(k * kDenseFormatTable[f].mn + col));
}

// The element of an integer-valued format from its hash.
GPUCHECK_HD inline long long dense_int_from_hash(int f, uint64_t h) {
  if (f == kDenseI8) return static_cast<int8_t>(h & 0xFFu);
  if (f == kDenseF32) return static_cast<long long>(h % 1023u) - 511;
  if (f == kDenseF64)
    return static_cast<long long>(h % ((1ull << 21) - 1)) - ((1ll << 20) - 1);
  return static_cast<long long>(h % 31u) - 15;
}

// The element code of fp8 (e4m3) and bf8 (e5m2) from its hash: the MX stage's.
GPUCHECK_HD inline uint32_t dense_code_from_hash(int f, uint64_t h) {
  return mx_code_from_hash(f == kDenseFp8 ? kMxE4M3 : kMxE5M2, h);
}

// As above but never zero (0 becomes 1, +-0 becomes +-1): the rate kernels'
// operands.
GPUCHECK_HD inline long long dense_nonzero_int_from_hash(int f, uint64_t h) {
  const long long v = dense_int_from_hash(f, h);
  return v ? v : 1;
}
GPUCHECK_HD inline uint32_t dense_nonzero_code_from_hash(int f, uint64_t h) {
  return mx_nonzero_code_from_hash(f == kDenseFp8 ? kMxE4M3 : kMxE5M2, h);
}

}  // namespace gpucheck
