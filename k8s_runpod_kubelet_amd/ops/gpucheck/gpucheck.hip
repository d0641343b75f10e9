// gpucheck — active GPU self-test run between tenants.
//
// Tests visible device 0 (the caller scopes visibility with
// ROCR_VISIBLE_DEVICES) in six stages:
//   1. HBM fill + verify with a hashed 16-byte pattern and its complement,
//   2. device-to-device copy bandwidth, with the copied half verified against
//      the pattern its source holds,
//   3. an exact-integer MFMA self-test (bf16 32x32x16, no memory loads),
//   4. an exact self-test of the block-scaled MX path (scaled 32x32x64 MFMA
//      with e4m3, e5m2 and e2m1 operands and E8M0 scales, in the format pairs
//      fp8, bf8, fp4 and fp8xfp4) and its measured rate per format pair,
//   5. an LDS self-test: workgroups that each hold a compute unit's whole
//      160 KiB LDS fill it with the hashed pattern and its complement and
//      read it back from another wave; the host counts which compute units
//      were covered and names the compute unit of a mismatch,
//   6. an exact self-test of the dense (non-scaled) matrix formats, one
//      instruction each: f16 and fp8/bf8 32x32x16, bf16 16x16x32, i8
//      32x32x32 (i32 accumulators), f32 32x32x2 and f64 16x16x4, and the
//      measured rate of each.
// Every wave of stages 3 to 6 records where it ran (XCC, shader engine,
// shader array, compute unit, SIMD), so coverage is reported and a bad wave
// is located in the hardware.
// Prints exactly one JSON object as the last stdout line and exits with a
// stage-specific code (the first that applies, in this order):
//   0 pass, 2 usage, 11 HIP error, 20 HBM mismatch, 23 copy mismatch,
//   21 MFMA mismatch, 24 MX mismatch, 26 LDS mismatch, 28 dense mismatch,
//   22 copy bandwidth below --min-copy-gbs, 25 an MX rate below its
//   --min-mx-tflops, 29 a dense rate below its --min-dense-tflops, 27 LDS
//   coverage partial under --lds-require-coverage.
// `--cpu` runs the HBM stage as host loops over malloc'ed memory and makes no
// HIP call, so the CLI, JSON and mismatch localisation are testable without
// a GPU. With an explicit --mfma-waves it also fills the MFMA tiles with a
// host integer matmul and runs the same comparison over them, and with an
// explicit --mx-waves it does the same for the MX tiles (rates stay 0 and
// their floors are ignored), and with an explicit --lds-groups it runs the
// LDS stage's write order, rotated read, injection and judging over a host
// buffer per group, reporting compute unit `group % 5` for every wave, and
// with an explicit --dense-waves it fills the dense tiles from the host
// integer product and judges them (rates stay 0, floors are ignored).
//
// Flags that exist for the test suite: --dump-pattern, --dump-vectors,
// --store-variant, --inject-flip, --inject-pass, --inject-copy-flip,
// --dump-mfma-tile, --inject-mfma, --dump-mx-tile, --inject-mx, --dump-lds,
// --dump-lds-where, --inject-lds, --dump-dense-tile, --inject-dense. The
// injections flip bits in the region or in the LDS, or change the host copy
// of the MFMA, MX or dense result; they test the checkers.
//
// Build: hipcc --offload-arch=gfx950 -O2 -std=c++17 gpucheck.hip -o gpucheck

#include <hip/hip_runtime.h>

#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "gpucheck_pattern.h"

using gpucheck::Vec16;

namespace {

struct HipError {
  std::string what;
};

#define HIP_CHECK(expr)                                                  \
  do {                                                                   \
    hipError_t err_ = (expr);                                            \
    if (err_ != hipSuccess)                                              \
      throw HipError{std::string(#expr) + ": " + hipGetErrorString(err_)}; \
  } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kBlock = 256;
constexpr size_t kMaxGrid = 2048;
constexpr uint64_t kNoBad = ~0ull;
constexpr long long kNotAnInteger = INT64_MIN;  // below every exact value
constexpr size_t kCacheResidentBelow = 512ull << 20;

// ---------------------------------------------------------------- kernels

__host__ __device__ inline u32x4 pattern_vec(uint64_t seed, uint32_t pass,
                                             uint64_t index) {
  const Vec16 v = gpucheck::pattern(seed, pass, index);
  u32x4 x;
  x.x = static_cast<unsigned int>(v.lo);
  x.y = static_cast<unsigned int>(v.lo >> 32);
  x.z = static_cast<unsigned int>(v.hi);
  x.w = static_cast<unsigned int>(v.hi >> 32);
  return x;
}

// Where a wave runs, from two scalar register reads. The fields of HW_ID are
// the GFX9 layout; a CU key packs the XCC id with the shader engine, shader
// array and compute unit and leaves out everything that differs between the
// waves of one compute unit (wave, SIMD, pipe, queue).
//
// Measured on an MI355X (256 compute units) with 512 workgroups of
// lds_selftest, three runs alike: the four waves of every workgroup report
// one CU key and the SIMD ids {0, 1, 2, 3}; the keys are exactly 256,
// 32 per XCC id 0..7 and 64 per se_id 0..3 (bit 15 is always 0), sh_id is
// always 0, and cu_id runs 0..8 with 19 to 32 compute units per value (the
// harvested ones differ between shader engines). So this table is right for
// gfx950: no mask below lets a per-wave bit in or drops a bit that tells two
// compute units apart.
struct HwField {
  int shift, bits;
};
constexpr int kHwRegHwId = 4;
constexpr int kHwRegXccId = 20;
constexpr HwField kHwSimd{4, 2};
constexpr HwField kHwCu{8, 4};
constexpr HwField kHwSh{12, 1};
constexpr HwField kHwSe{13, 3};
constexpr HwField kXccId{0, 4};
// CU key: cu [3:0], sh [4], se [7:5], xcc [11:8].
constexpr int kKeyShShift = 4, kKeySeShift = 5, kKeyXccShift = 8;

// The immediate of s_getreg_b32: register id, first bit, field width - 1.
constexpr int hwreg(int id, int offset, int bits) {
  return id | (offset << 6) | ((bits - 1) << 11);
}

constexpr uint32_t hw_field(uint32_t reg, HwField f) {
  return (reg >> f.shift) & ((1u << f.bits) - 1);
}

struct WaveWhere {
  uint32_t cu_key, simd;
};

__device__ inline WaveWhere wave_where() {
  const uint32_t hw = __builtin_amdgcn_s_getreg(hwreg(kHwRegHwId, 0, 32));
  const uint32_t xcc = __builtin_amdgcn_s_getreg(
      hwreg(kHwRegXccId, kXccId.shift, kXccId.bits));
  WaveWhere w;
  w.cu_key = hw_field(hw, kHwCu) | (hw_field(hw, kHwSh) << kKeyShShift) |
             (hw_field(hw, kHwSe) << kKeySeShift) | (xcc << kKeyXccShift);
  w.simd = hw_field(hw, kHwSimd);
  return w;
}

// where[2 * wave] = CU key, where[2 * wave + 1] = SIMD id: two ordinary
// vector stores from the calling lane (one lane per wave calls this).
__device__ inline void store_where(uint32_t* __restrict__ where, size_t wave) {
  const WaveWhere w = wave_where();
  where[2 * wave] = w.cu_key;
  where[2 * wave + 1] = w.simd;
}

// One 16-byte vector per lane per trip; consecutive lanes write consecutive
// vectors. All indices are size_t: regions exceed 4 GiB.
template <bool kNonTemporal>
__global__ __launch_bounds__(kBlock) void hbm_fill(u32x4* __restrict__ p,
                                                   size_t nvec,
                                                   uint64_t base_index,
                                                   uint64_t seed,
                                                   uint32_t pass) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < nvec; i += stride) {
    const u32x4 x = pattern_vec(seed, pass, base_index + i);
    if (kNonTemporal)
      __builtin_nontemporal_store(x, &p[i]);
    else
      p[i] = x;
  }
}

// counters[0] += bad vectors, counters[1] = min(bad vector index). One
// integer atomic pair per wave, and only from waves that saw a mismatch.
__global__ __launch_bounds__(kBlock) void hbm_verify(
    const u32x4* __restrict__ p, size_t nvec, uint64_t base_index,
    uint64_t seed, uint32_t pass, unsigned long long* counters) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  unsigned long long bad = 0;
  unsigned long long first = kNoBad;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < nvec; i += stride) {
    const u32x4 got = p[i];
    const u32x4 want = pattern_vec(seed, pass, base_index + i);
    if (got.x != want.x || got.y != want.y || got.z != want.z ||
        got.w != want.w) {
      ++bad;
      if (i < first) first = i;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_xor(bad, off);
    const unsigned long long other = __shfl_xor(first, off);
    first = other < first ? other : first;
  }
  if ((threadIdx.x & 63) == 0 && bad != 0) {
    atomicAdd(&counters[0], bad);
    atomicMin(&counters[1], first);
  }
}

__global__ __launch_bounds__(kBlock) void vec_copy(u32x4* __restrict__ dst,
                                                   const u32x4* __restrict__ src,
                                                   size_t nvec) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < nvec; i += stride)
    dst[i] = src[i];
}

// The tile a wave of a *_selftest kernel computes: four waves per workgroup.
__device__ inline uint32_t selftest_wave() {
  return blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
}

// The C/D map of the 32x32 f32 forms: lane (r, h) stores accumulator register
// g to out[wave][(g & 3) + 8 (g >> 2) + 4 h][r].
__device__ inline void store_tile_32x32(float* __restrict__ out, uint32_t wave,
                                        int r, int h, const f32x16& acc) {
  float* tile = out + static_cast<size_t>(wave) * (32 * 32);
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
    tile[row * 32 + r] = acc[g];
  }
}

// Each wave computes one 32x32 tile D = A.B with K = 128 from operands
// generated in registers, then stores it to out[wave][row][col]. Lane l
// (r = l & 31, h = l >> 5) holds A[r][8h+j] and B[8h+j][r] of each 16-wide
// k-step in element j; accumulator register g is D[(g&3)+8(g>>2)+4h][r].
// Lane 0 also stores where the wave ran to where[wave].
__global__ __launch_bounds__(kBlock) void mfma_selftest(
    float* __restrict__ out, uint32_t* __restrict__ where, uint32_t nwaves,
    uint64_t seed) {
  const uint32_t wave = selftest_wave();
  // Wave-uniform: surplus waves of the last workgroup leave whole, so every
  // MFMA below runs with a full EXEC mask.
  if (wave >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int r = lane & 31;
  const int h = lane >> 5;
  const uint64_t key_a = gpucheck::mfma_key(seed, wave, 0);
  const uint64_t key_b = gpucheck::mfma_key(seed, wave, 1);
  f32x16 acc;
  for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
#pragma unroll
  for (int s = 0; s < gpucheck::kMfmaK / 16; ++s) {
    s16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * s + 8 * h + j;
      a[j] = static_cast<short>(
          gpucheck::bf16_bits_small_int(gpucheck::mfma_a(key_a, r, k)));
      b[j] = static_cast<short>(
          gpucheck::bf16_bits_small_int(gpucheck::mfma_b(key_b, k, r)));
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
        __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0,
        0, 0);
  }
  store_tile_32x32(out, wave, r, h, acc);
  if (lane == 0) store_where(where, wave);
}

// One lane's 32 elements of an MX operand for one 64-wide k-step, packed
// the way the scaled MFMA reads them (measured on an MI355X with the exact
// asymmetric data of this test; h = lane >> 5, k counted from the step's
// first):
//   e2m1: nibble j = 0..31 of the low four dwords holds k = 32h + j (the
//         other four dwords are zero);
//   8-bit types: byte 16c + i (c = 0, 1; i = 0..15) holds k = 32c + 16h + i.
//         A 32-wide k-block is thus 16-byte chunk c of BOTH lane halves, not
//         the 32 bytes of one lane.
// `first` is the hash index of the step's first k and `stride` the step to
// the next k (1 along a row of A, 32 down a column of B).
template <int kType, bool kNonZero>
__device__ inline i32x8 mx_fragment(uint64_t key, uint32_t first,
                                    uint32_t stride, int h) {
  constexpr int bits = kType == gpucheck::kMxE2M1 ? 4 : 8;
  constexpr int per_dword = 32 / bits;
  i32x8 frag;
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    uint32_t word = 0;
    if (d < 32 / per_dword) {
#pragma unroll
      for (int i = 0; i < per_dword; ++i) {
        const int j = d * per_dword + i;
        const int k = bits == 4 ? 32 * h + j : 32 * (j >> 4) + 16 * h + (j & 15);
        const uint64_t hash = gpucheck::mix64(key + first + k * stride);
        const uint32_t code =
            kNonZero ? gpucheck::mx_nonzero_code_from_hash(kType, hash)
                     : gpucheck::mx_code_from_hash(kType, hash);
        word |= code << (bits * i);
      }
    }
    frag[d] = static_cast<int>(word);
  }
  return frag;
}

// K-step kStep of the MX self-test. The step index is a template argument
// because the byte selects (like cbsz and blgp) are immediates.
template <int kFmt, int kStep>
__device__ inline f32x16 mx_step(f32x16 acc, uint64_t key_a, uint64_t key_b,
                                 int r, int h, int scale_a, int scale_b) {
  constexpr int ta = gpucheck::kMxFormatTable[kFmt].a;
  constexpr int tb = gpucheck::kMxFormatTable[kFmt].b;
  const int k0 = 64 * kStep;
  const i32x8 a = mx_fragment<ta, false>(
      key_a, static_cast<uint32_t>(r * gpucheck::kMxK + k0), 1, h);
  const i32x8 b =
      mx_fragment<tb, false>(key_b, static_cast<uint32_t>(k0 * 32 + r), 32, h);
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
      a, b, acc, ta, tb, kStep, scale_a, kStep, scale_b);
}

// Each wave computes one 32x32 tile D = (A scaled).(B scaled) with K = 256 in
// four 32x32x64 block-scaled steps, operands generated in registers, and
// stores it to out[wave][row][col]. Lane l (r = l & 31, h = l >> 5) holds
// elements of row r of A and of column r of B; which k they are depends on
// the element width (mx_fragment). Byte s of the lane's scale register is the
// E8M0 scale of k-block 2s + h of that row or column, k = 64s + 32h ..
// 64s + 32h + 31, for every element width, and step s selects byte s. For
// e2m1 those are the lane's own 32 elements; for 8-bit types they are chunk h
// of both lanes r and r + 32.
// The C/D map depends on the shape only, so it is mfma_selftest's.
template <int kFmt>
__global__ __launch_bounds__(kBlock) void mx_selftest(
    float* __restrict__ out, uint32_t* __restrict__ where, uint32_t nwaves,
    uint64_t seed) {
  const uint32_t wave = selftest_wave();
  // Wave-uniform, as in mfma_selftest: EXEC is full at every MFMA.
  if (wave >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int r = lane & 31;
  const int h = lane >> 5;
  const uint64_t key_a = gpucheck::mx_key(seed, wave, kFmt, 0);
  const uint64_t key_b = gpucheck::mx_key(seed, wave, kFmt, 1);
  uint32_t scale_a = 0, scale_b = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    scale_a |= gpucheck::mx_scale_byte(key_a, r, 2 * s + h) << (8 * s);
    scale_b |= gpucheck::mx_scale_byte(key_b, r, 2 * s + h) << (8 * s);
  }
  const int sa = static_cast<int>(scale_a), sb = static_cast<int>(scale_b);
  f32x16 acc;
  for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
  acc = mx_step<kFmt, 0>(acc, key_a, key_b, r, h, sa, sb);
  acc = mx_step<kFmt, 1>(acc, key_a, key_b, r, h, sa, sb);
  acc = mx_step<kFmt, 2>(acc, key_a, key_b, r, h, sa, sb);
  acc = mx_step<kFmt, 3>(acc, key_a, key_b, r, h, sa, sb);
  store_tile_32x32(out, wave, r, h, acc);
  if (lane == 0) store_where(where, wave);
}

// Timed: every wave issues 4 * trips scaled MFMAs of one format over four
// independent accumulators, from hashed non-zero operands and unit scales,
// and writes one float per lane to sink[global thread] so the work is live.
template <int kFmt>
__global__ __launch_bounds__(kBlock) void mx_rate(float* __restrict__ sink,
                                                  uint32_t trips,
                                                  uint64_t seed) {
  constexpr int ta = gpucheck::kMxFormatTable[kFmt].a;
  constexpr int tb = gpucheck::kMxFormatTable[kFmt].b;
  const uint32_t tid = blockIdx.x * kBlock + threadIdx.x;
  const uint64_t key = gpucheck::mx_key(seed, tid >> 6, kFmt, 0);
  const uint32_t lane = threadIdx.x & 63;
  const i32x8 a = mx_fragment<ta, true>(key, lane * 128, 1, 0);
  const i32x8 b = mx_fragment<tb, true>(key, lane * 128 + 64, 1, 0);
  const int unit = 0x7F7F7F7F;  // E8M0 127 = 2^0 in every byte
  f32x16 acc0, acc1, acc2, acc3;
  // Different starting values: four chains the compiler cannot fold into one.
  for (int g = 0; g < 16; ++g) {
    acc0[g] = 0.0f;
    acc1[g] = 1.0f;
    acc2[g] = 2.0f;
    acc3[g] = 3.0f;
  }
  for (uint32_t t = 0; t < trips; ++t) {
    acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc0, ta, tb,
                                                           0, unit, 0, unit);
    acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc1, ta, tb,
                                                           0, unit, 0, unit);
    acc2 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc2, ta, tb,
                                                           0, unit, 0, unit);
    acc3 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc3, ta, tb,
                                                           0, unit, 0, unit);
  }
  float sum = 0.0f;
  for (int g = 0; g < 16; ++g) sum += acc0[g] + acc1[g] + acc2[g] + acc3[g];
  sink[tid] = sum;
}

// ------------------------------------------------------- dense formats
//
// One instruction per format (gpucheck::kDenseFormatTable):
//   f16      v_mfma_f32_32x32x16_f16       bf16x16  v_mfma_f32_16x16x32_bf16
//   fp8      v_mfma_f32_32x32x16_fp8_fp8   bf8      v_mfma_f32_32x32x16_bf8_bf8
//   i8       v_mfma_i32_32x32x32_i8        f32      v_mfma_f32_32x32x2_f32
//   f64      v_mfma_f64_16x16x4_f64
//
// How the kernels fill the operands, one rule for all seven. With mn the
// tile side, lane l has rc = l & (mn - 1) and g = l / mn (g = 0, 1 for 32x32,
// 0..3 for 16x16), and holds per = step_k . mn / 64 elements of row rc of A
// and of column rc of B per instruction (8 f16, bf16, fp8 or bf8 values; 16
// int8; one f32 or f64). Into slot (g, j) of step s, element j of the lane's
// fragment (16-bit elements in ascending halves of the dwords, 8-bit elements
// in ascending bytes), both A and B put k = step_k . s + per . g + j.
//
// That k is THIS KERNEL'S LABELLING of the slots, not the instruction's
// documented k order: do not load real A or B data from memory by it. A sum
// over k is the same for any order that A and B share, so a product cannot
// see which k of a step the hardware takes a slot for (for bf16, f32 and f64
// the labelling happens to be the documented map; for f16, the 8-bit floats
// and i8 nothing here says so). What the tiles, which on an MI355X equal the
// independent reference for every format, do fix: the row of A and the
// column of B sit on lane & (mn - 1), and the instruction multiplies slot
// (g, j) of A with slot (g, j) of B, for 8 and 16 bytes per lane as for bf16.
//
// C/D map: 32x32 forms, register v is row (v & 3) + 8 (v >> 2) + 4 g; the
// 16x16 f32-accumulator form, row 4 g + v; f64, row g + 4 v. Column rc.
template <int kFmt>
struct DenseTypes {
  static constexpr gpucheck::DenseFormat fmt = gpucheck::kDenseFormatTable[kFmt];
  static constexpr int regs = fmt.mn * fmt.mn / 64;
  static constexpr int per = fmt.step_k * fmt.mn / 64;
  // What a lane stores per result: i32 for i8, f64 for f64, else f32.
  using Elem = std::conditional_t<
      kFmt == gpucheck::kDenseI8, int,
      std::conditional_t<kFmt == gpucheck::kDenseF64, double, float>>;
  typedef Elem Acc __attribute__((ext_vector_type(regs)));
};

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// One lane's elements of one instruction: element j hashes index
// first + j . stride (stride 1 along a row of A, mn down a column of B).
template <int kFmt, bool kNonZero>
__device__ inline auto dense_fragment(uint64_t key, uint32_t first,
                                      uint32_t stride) {
  using namespace gpucheck;
  constexpr int per = DenseTypes<kFmt>::per;
  auto hash = [&](int j) { return mix64(key + first + j * stride); };
  auto value = [&](int j) {
    return kNonZero ? dense_nonzero_int_from_hash(kFmt, hash(j))
                    : dense_int_from_hash(kFmt, hash(j));
  };
  (void)value;  // the 8-bit float formats take codes, not values
  if constexpr (kFmt == kDenseF16) {
    f16x8 frag;
#pragma unroll
    for (int j = 0; j < per; ++j)
      frag[j] = static_cast<_Float16>(static_cast<float>(value(j)));
    return frag;
  } else if constexpr (kFmt == kDenseBf16x16) {
    // |value| <= 15 has four significant bits: the top half of its f32 bits
    // is its bf16, exactly.
    s16x8 frag;
#pragma unroll
    for (int j = 0; j < per; ++j)
      frag[j] = static_cast<short>(
          __builtin_bit_cast(uint32_t, static_cast<float>(value(j))) >> 16);
    return __builtin_bit_cast(bf16x8, frag);
  } else if constexpr (kFmt == kDenseFp8 || kFmt == kDenseBf8) {
    uint64_t frag = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) {
      const uint64_t code = kNonZero
                                ? dense_nonzero_code_from_hash(kFmt, hash(j))
                                : dense_code_from_hash(kFmt, hash(j));
      frag |= code << (8 * j);
    }
    return static_cast<long>(frag);
  } else if constexpr (kFmt == kDenseI8) {
    i32x4 frag;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        word |= (static_cast<uint32_t>(value(4 * d + i)) & 0xFFu) << (8 * i);
      frag[d] = static_cast<int>(word);
    }
    return frag;
  } else if constexpr (kFmt == kDenseF32) {
    return static_cast<float>(value(0));
  } else {
    return static_cast<double>(value(0));
  }
}

template <int kFmt, typename Frag>
__device__ inline typename DenseTypes<kFmt>::Acc dense_mfma(
    Frag a, Frag b, typename DenseTypes<kFmt>::Acc acc) {
  using namespace gpucheck;
  if constexpr (kFmt == kDenseF16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
  else if constexpr (kFmt == kDenseBf16x16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  else if constexpr (kFmt == kDenseFp8)
    return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a, b, acc, 0, 0, 0);
  else if constexpr (kFmt == kDenseBf8)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(a, b, acc, 0, 0, 0);
  else if constexpr (kFmt == kDenseI8)
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
  else if constexpr (kFmt == kDenseF32)
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
}

// Each wave computes one tile of format kFmt from operands generated in
// registers and stores it to out[wave][row][col]; lane 0 also stores where
// the wave ran. The maps are in the comment above.
template <int kFmt>
__global__ __launch_bounds__(kBlock) void dense_selftest(
    typename DenseTypes<kFmt>::Elem* __restrict__ out,
    uint32_t* __restrict__ where, uint32_t nwaves, uint64_t seed) {
  using T = DenseTypes<kFmt>;
  constexpr int mn = T::fmt.mn, K = T::fmt.k, step_k = T::fmt.step_k;
  const uint32_t wave = selftest_wave();
  // Wave-uniform, as in mfma_selftest: EXEC is full at every MFMA.
  if (wave >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int rc = lane & (mn - 1);
  const int g = lane / mn;
  const uint64_t key_a = gpucheck::dense_key(seed, wave, kFmt, 0);
  const uint64_t key_b = gpucheck::dense_key(seed, wave, kFmt, 1);
  typename T::Acc acc;
  for (int v = 0; v < T::regs; ++v) acc[v] = 0;
#pragma unroll
  for (int s = 0; s < K / step_k; ++s) {
    const int k0 = step_k * s + T::per * g;
    const auto a = dense_fragment<kFmt, false>(
        key_a, static_cast<uint32_t>(rc * K + k0), 1);
    const auto b = dense_fragment<kFmt, false>(
        key_b, static_cast<uint32_t>(k0 * mn + rc), mn);
    acc = dense_mfma<kFmt>(a, b, acc);
  }
  typename T::Elem* tile = out + static_cast<size_t>(wave) * (mn * mn);
#pragma unroll
  for (int v = 0; v < T::regs; ++v) {
    const int row = mn == 32 ? (v & 3) + 8 * (v >> 2) + 4 * g
                    : kFmt == gpucheck::kDenseF64 ? g + 4 * v
                                                  : 4 * g + v;
    tile[row * mn + rc] = acc[v];
  }
  if (lane == 0) store_where(where, wave);
}

// Timed: every wave issues 4 * trips MFMAs of one format over four
// independent accumulators (the 16x16 forms' dependent latency exceeds their
// issue interval), from hashed non-zero operands, and writes one value per
// lane to sink[global thread] so the work is live. The i8 sums wrap. The
// timed loop must hold nothing but the MFMAs and its counter (see below).
template <int kFmt>
__global__ __launch_bounds__(kBlock) void dense_rate(
    typename DenseTypes<kFmt>::Elem* __restrict__ sink, uint32_t trips,
    uint64_t seed) {
  using T = DenseTypes<kFmt>;
  const uint32_t tid = blockIdx.x * kBlock + threadIdx.x;
  const uint64_t key = gpucheck::dense_key(seed, tid >> 6, kFmt, 0);
  const uint32_t lane = threadIdx.x & 63;
  const auto a = dense_fragment<kFmt, true>(key, lane * 32, 1);
  const auto b = dense_fragment<kFmt, true>(key, lane * 32 + 16, 1);
  typename T::Acc acc0, acc1, acc2, acc3;
  // Different starting values: four chains the compiler cannot fold into one.
  for (int v = 0; v < T::regs; ++v) {
    acc0[v] = 0;
    acc1[v] = 1;
    acc2[v] = 2;
    acc3[v] = 3;
  }
  // An empty statement that holds the four accumulators in accumulation
  // registers before the loop. Without it hipcc keeps the loop-carried values
  // of the bf16x16 and f64 kernels in VGPRs and copies them to and from the
  // MFMAs' registers on every trip (8 to 64 moves and the waits they need),
  // which halves the rate measured. With it the loop of every format is the
  // four MFMAs, the counter and one s_nop; tests/test_gpucheck_dense_isa.py
  // holds the compiled loops to that.
  asm volatile("" : "+a"(acc0), "+a"(acc1), "+a"(acc2), "+a"(acc3));
  for (uint32_t t = 0; t < trips; ++t) {
    acc0 = dense_mfma<kFmt>(a, b, acc0);
    acc1 = dense_mfma<kFmt>(a, b, acc1);
    acc2 = dense_mfma<kFmt>(a, b, acc2);
    acc3 = dense_mfma<kFmt>(a, b, acc3);
  }
  // Unsigned for i8: the sums wrap, in the accumulators and here.
  using Sum = std::conditional_t<std::is_same_v<typename T::Elem, int>,
                                 unsigned int, typename T::Elem>;
  Sum sum = 0;
  for (int v = 0; v < T::regs; ++v)
    sum += static_cast<Sum>(acc0[v]) + static_cast<Sum>(acc1[v]) +
           static_cast<Sum>(acc2[v]) + static_cast<Sum>(acc3[v]);
  sink[tid] = static_cast<typename T::Elem>(sum);
}

// The LDS self-test. One record per workgroup, updated only by waves that
// saw a mismatch.
struct LdsRecord {
  unsigned long long bad;    // mismatching vectors
  unsigned long long first;  // min of lds_pack(round, pass, vector); kNoBad
  u32x4 first_xor;           // got ^ want of that vector
};

constexpr int kMaxLdsInject = 4;
struct LdsInjections {
  uint32_t n;
  struct {
    uint32_t group, round, pass, dword, mask;
  } at[kMaxLdsInject];
};

__host__ __device__ inline unsigned long long lds_pack(uint32_t round,
                                                       uint32_t pass,
                                                       uint32_t vector) {
  return (static_cast<unsigned long long>(round) << 15) | (pass << 14) | vector;
}

// One 256-thread workgroup owns all 160 KiB of its compute unit's LDS (so no
// second workgroup of this kernel shares the compute unit) and, `rounds`
// times, for the pattern and then its complement: thread t writes vectors
// t + 256 j (consecutive lanes, consecutive ds_write_b128), thread 0 applies
// a matching injection, and thread t reads back and compares vectors
// ((t + 64) & 255) + 256 j, those the next wave wrote. Every LDS index is
// below 256 * 40 = kLdsVectors by construction; an injection's dword is
// checked against the array besides.
//
// The whole LDS is the array under test, so the reduction uses none of it:
// shuffles within a wave, then one integer atomic pair per wave that saw a
// mismatch; after a barrier the lane whose own first mismatch is the
// workgroup's minimum stores that vector's XOR. Each vector is read by one
// lane, so exactly one lane matches. Lane 0 of each wave stores where the
// wave ran to where[4 * group + wave]; the four must share one CU key.
// `dump`, when not null, receives what the chosen workgroup read back in the
// chosen round and pass (kLdsVectors vectors) and after them, per vector,
// the thread that read it (kLdsVectors dwords): the only trace of which
// wave did the reading.
//
// The HW_ID fields as measured on an MI355X are at wave_where. There 512
// workgroups (two per compute unit) reached all 256 compute units in one
// launch, every time: the first 256 workgroups already sat on 256 different
// compute units.
__global__ __launch_bounds__(kBlock) void lds_selftest(
    LdsRecord* __restrict__ records, uint32_t* __restrict__ where,
    uint64_t seed, uint32_t round_base, uint32_t rounds, LdsInjections inj,
    u32x4* __restrict__ dump, uint32_t dump_group, uint32_t dump_round,
    uint32_t dump_pass) {
  __shared__ u32x4 lds[gpucheck::kLdsVectors];
  constexpr int trips = gpucheck::kLdsVectors / kBlock;
  const uint32_t t = threadIdx.x;
  const uint32_t reader = (t + 64) & (kBlock - 1);
  const uint32_t group = blockIdx.x;
  unsigned long long bad = 0;
  unsigned long long first = kNoBad;
  u32x4 first_xor = {0, 0, 0, 0};
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t round = round_base + r;
    const uint64_t key = gpucheck::lds_key(seed, group, round);
    for (uint32_t pass = 0; pass < 2; ++pass) {
      for (int j = 0; j < trips; ++j) {
        const uint32_t i = t + kBlock * j;
        lds[i] = pattern_vec(key, pass, i);
      }
      __syncthreads();
      // Uniform over the workgroup: every thread takes the barrier or none.
      bool hit = false;
      for (uint32_t k = 0; k < inj.n && k < kMaxLdsInject; ++k)
        hit = hit || (inj.at[k].group == group && inj.at[k].round == round &&
                      inj.at[k].pass == pass);
      if (hit) {
        if (t == 0)
          for (uint32_t k = 0; k < inj.n && k < kMaxLdsInject; ++k)
            if (inj.at[k].group == group && inj.at[k].round == round &&
                inj.at[k].pass == pass &&
                inj.at[k].dword < 4u * gpucheck::kLdsVectors)
              lds[inj.at[k].dword >> 2][inj.at[k].dword & 3] ^= inj.at[k].mask;
        __syncthreads();
      }
      const bool dumping = dump != nullptr && group == dump_group &&
                           round == dump_round && pass == dump_pass;
      for (int j = 0; j < trips; ++j) {
        const uint32_t i = reader + kBlock * j;
        const u32x4 got = lds[i];
        const u32x4 want = pattern_vec(key, pass, i);
        if (got.x != want.x || got.y != want.y || got.z != want.z ||
            got.w != want.w) {
          ++bad;
          const unsigned long long packed = lds_pack(round, pass, i);
          if (packed < first) {
            first = packed;
            first_xor = got ^ want;
          }
        }
        if (dumping) {
          dump[i] = got;
          reinterpret_cast<uint32_t*>(dump + gpucheck::kLdsVectors)[i] = t;
        }
      }
      __syncthreads();
    }
  }
  unsigned long long wave_bad = bad;
  unsigned long long wave_first = first;
  for (int off = 32; off > 0; off >>= 1) {
    wave_bad += __shfl_xor(wave_bad, off);
    const unsigned long long other = __shfl_xor(wave_first, off);
    wave_first = other < wave_first ? other : wave_first;
  }
  LdsRecord* rec = &records[group];
  if (wave_bad != 0) {  // wave-uniform
    if ((t & 63) == 0) {
      atomicAdd(&rec->bad, wave_bad);
      atomicMin(&rec->first, wave_first);
    }
    // The atomics have reached memory before this wave passes the barrier.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  }
  __syncthreads();
  if (first != kNoBad &&
      __hip_atomic_load(&rec->first, __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT) == first)
    rec->first_xor = first_xor;
  if ((t & 63) == 0) store_where(where, 4 * static_cast<size_t>(group) + (t >> 6));
}

// ------------------------------------------------------- tile-stage families
//
// The MFMA, MX and dense stages are one thing on the host: one wave per tile,
// tiles compared exactly with a host product, a rate kernel per format. What
// differs between them is in this table and in their kernels.

enum { kMfma, kMx, kDense, kFamilies };
constexpr int kMaxFormats = gpucheck::kDenseFormats;

// The tile wave `w` must produce in format `f`, times the format's scale,
// row-major.
void mfma_expected_tile(int f, uint64_t seed, long w, double* out);
void mx_expected_tile(int f, uint64_t seed, long w, double* out);
void dense_expected_tile(int f, uint64_t seed, long w, double* out);

struct Family {
  const char* prefix;  // of its flags and JSON keys
  int formats;
  const char* names[kMaxFormats];  // MFMA's one format has no name
  int elems[kMaxFormats];          // of one tile
  int scale[kMaxFormats];          // a result times this is an integer
  // A dumped value times the scale is printed if it is an integer of at most
  // this magnitude.
  double dump_bound;
  void (*expected_tile)(int f, uint64_t seed, long w, double* out);
  bool optional;            // --X-waves 0 skips the stage
  int waves_per_cu;         // default waves, per compute unit
  uint64_t rate_instr;      // default timed MFMAs per wave and launch; 0: no rate
};

Family mx_family() {
  Family fam = {"mx", gpucheck::kMxFormats, {}, {}, {}, 1e15,
                mx_expected_tile, true, 4, 65536};
  for (int f = 0; f < fam.formats; ++f) {
    fam.names[f] = gpucheck::kMxFormatTable[f].name;
    fam.elems[f] = 32 * 32;
    fam.scale[f] = 16;
  }
  return fam;
}

Family dense_family() {
  Family fam = {"dense", gpucheck::kDenseFormats, {}, {}, {}, 9e18,
                dense_expected_tile, true, 4, 16384};
  for (int f = 0; f < fam.formats; ++f) {
    const gpucheck::DenseFormat& fmt = gpucheck::kDenseFormatTable[f];
    fam.names[f] = fmt.name;
    fam.elems[f] = fmt.mn * fmt.mn;
    fam.scale[f] = fmt.scale;
  }
  return fam;
}

const Family kFamilyTable[kFamilies] = {
    {"mfma", 1, {nullptr}, {32 * 32}, {1}, 16777216.0, mfma_expected_tile,
     false, 8, 0},
    mx_family(),
    dense_family(),
};

// ---------------------------------------------------------------- options

// One changed element of the host copy of a tile.
struct Inject {
  int format;
  long wave;
  int elem;
};

// The flags of one family: --X-waves, --dump-X-tile, --inject-X,
// --min-X-tflops and --X-rate-instr.
struct TileOptions {
  // -1: the family's waves_per_cu x multiProcessorCount, capped by an explicit
  // --mfma-waves so that a small run stays small.
  long waves = -1;
  int dump_format = -1;
  long dump_wave = -1;
  std::vector<Inject> inject;
  double min_tflops[kMaxFormats] = {};
  uint64_t rate_instr = 0;
};

struct Options {
  bool cpu = false;
  size_t bytes = 1ull << 30;
  uint32_t passes = 2;
  uint64_t base_index = 0;
  uint64_t seed = 0x6770756368656B31ull;
  double min_copy_gbs = 0.0;
  struct Flip {
    size_t offset;
    int bit;
  };
  std::vector<Flip> flips;  // applied after the fill of pass inject_pass
  uint32_t inject_pass = 0;
  bool copy_flip = false;  // applied to the destination half after the copy
  Flip copy_flip_at{0, 0};
  bool dump_pattern = false;
  std::vector<size_t> dump_vectors;
  int store_variant = -1;  // -1 auto, 0 plain, 1 non-temporal
  // MFMA, MX and dense stages. Formats are indices into the family's names.
  TileOptions tile[kFamilies];
  Options() {
    for (int fam = 0; fam < kFamilies; ++fam)
      tile[fam].rate_instr = kFamilyTable[fam].rate_instr;
  }
  // LDS stage.
  long lds_groups = -1;  // -1: 2 x multiProcessorCount (0 under --cpu)
  uint32_t lds_rounds = 4;
  uint32_t lds_max_launches = 8;
  bool lds_require_coverage = false;
  bool dump_lds = false;
  uint32_t dump_lds_group = 0, dump_lds_round = 0, dump_lds_pass = 0;
  bool dump_lds_where = false;
  struct LdsInject {
    uint32_t group, round, pass, byte, bit;
  };
  std::vector<LdsInject> lds_inject;
};

constexpr size_t kMaxFlips = 16;
constexpr size_t kMaxDumpVectors = 16;
constexpr size_t kMaxInject = 8;  // per family
const char* const kVariantNames[2] = {"plain", "nontemporal"};

bool parse_u64(const char* s, uint64_t* out, bool allow_suffix) {
  if (s == nullptr || *s == '\0' || *s == '-' || *s == '+') return false;
  errno = 0;
  char* end = nullptr;
  unsigned long long v = strtoull(s, &end, 0);
  if (errno != 0 || end == s) return false;
  int shift = 0;
  if (allow_suffix && *end != '\0') {
    switch (*end) {
      case 'k': case 'K': shift = 10; break;
      case 'm': case 'M': shift = 20; break;
      case 'g': case 'G': shift = 30; break;
      case 't': case 'T': shift = 40; break;
      default: return false;
    }
    ++end;
    if (*end == 'i') ++end;
    if (*end == 'B' || *end == 'b') ++end;
  }
  if (*end != '\0') return false;
  if (shift && v > (~0ull >> shift)) return false;
  *out = v << shift;
  return true;
}

bool parse_double(const char* s, double* out) {
  if (s == nullptr || *s == '\0') return false;
  errno = 0;
  char* end = nullptr;
  double v = strtod(s, &end);
  if (errno != 0 || end == s || *end != '\0' || !(v >= 0.0)) return false;
  *out = v;
  return true;
}

int usage(const char* why, const char* arg) {
  fprintf(stderr,
          "gpucheck: %s%s%s\n"
          "usage: gpucheck [--cpu] [--bytes N[K|M|G]] [--passes P] "
          "[--base-index N] [--seed S]\n"
          "                [--min-copy-gbs X] [--mfma-waves W] "
          "[--store-variant plain|nontemporal|auto]\n"
          "                [--mx-waves W] [--min-mx-tflops FORMAT:X]... "
          "[--mx-rate-instr N]\n"
          "                (FORMAT: fp8, bf8, fp4 or fp8xfp4; --mx-waves 0 "
          "skips the MX stage)\n"
          "                [--dense-waves W] [--min-dense-tflops FORMAT:X]... "
          "[--dense-rate-instr N]\n"
          "                (FORMAT: f16, bf16x16, fp8, bf8, i8, f32 or f64; "
          "--dense-waves 0 skips the dense stage)\n"
          "                [--lds-groups N] [--lds-rounds R] "
          "[--lds-max-launches L] [--lds-require-coverage]\n"
          "                (--lds-groups 0 skips the LDS stage)\n"
          "       checks of the checkers:\n"
          "                [--dump-pattern] [--dump-vectors I[,J,...]] "
          "[--dump-mfma-tile W]\n"
          "                [--inject-flip OFFSET:BIT]... [--inject-pass P] "
          "[--inject-copy-flip OFFSET:BIT]\n"
          "                [--inject-mfma WAVE:ELEM]... "
          "[--dump-mx-tile FORMAT:WAVE]\n"
          "                [--inject-mx FORMAT:WAVE:ELEM]... "
          "[--dump-lds GROUP:ROUND:PASS] [--dump-lds-where]\n"
          "                [--inject-lds GROUP:ROUND:PASS:BYTE:BIT]...\n"
          "                [--dump-dense-tile FORMAT:WAVE] "
          "[--inject-dense FORMAT:WAVE:ELEM]...\n"
          "exit: 0 pass, 2 usage, 11 HIP error, 20 HBM mismatch, "
          "23 copy mismatch, 21 MFMA mismatch,\n"
          "      24 MX mismatch, 26 LDS mismatch, 28 dense mismatch, "
          "22 copy bandwidth below --min-copy-gbs,\n"
          "      25 MX rate below --min-mx-tflops, 29 dense rate below "
          "--min-dense-tflops,\n"
          "      27 LDS coverage partial under --lds-require-coverage\n",
          why, arg ? " " : "", arg ? arg : "");
  return 2;
}

// "A:B", both unsigned integers.
bool parse_pair(const char* v, uint64_t* a, uint64_t* b) {
  const char* colon = v ? strchr(v, ':') : nullptr;
  return colon != nullptr &&
         parse_u64(std::string(v, colon - v).c_str(), a, false) &&
         parse_u64(colon + 1, b, false);
}

// "A:B:...": exactly `n` unsigned integers.
bool parse_fields(const char* v, size_t n, uint64_t* out) {
  if (v == nullptr) return false;
  std::string rest = v;
  for (size_t k = 0; k < n; ++k) {
    const size_t colon = rest.find(':');
    if ((colon == std::string::npos) != (k + 1 == n)) return false;
    if (!parse_u64(rest.substr(0, colon).c_str(), &out[k], false)) return false;
    if (k + 1 < n) rest = rest.substr(colon + 1);
  }
  return true;
}

// "FORMAT:REST": the index of the family's named format, or -1; *rest is
// REST. A family whose one format has no name takes all of `v` as REST.
int parse_format(const Family& fam, const char* v, const char** rest) {
  *rest = v;
  if (fam.names[0] == nullptr) return 0;
  const char* colon = v ? strchr(v, ':') : nullptr;
  if (colon == nullptr) return -1;
  const std::string name(v, colon - v);
  *rest = colon + 1;
  for (int f = 0; f < fam.formats; ++f)
    if (name == fam.names[f]) return f;
  return -1;
}

// The five flags of every family. `next` yields the flag's value. Returns -1
// where `a` is none of them, else 0, or 2 on a usage error.
template <typename Next>
int parse_tile_flag(const std::string& a, Next&& next, Options* o) {
  for (int i = 0; i < kFamilies; ++i) {
    const Family& fam = kFamilyTable[i];
    TileOptions& t = o->tile[i];
    const std::string x = fam.prefix;
    const char* rest = nullptr;
    uint64_t u = 0, elem = 0;
    if (a == "--" + x + "-waves") {
      if (!parse_u64(next(), &u, false) || (u == 0 && !fam.optional) ||
          u > 65536)
        return usage("bad value for", a.c_str());
      t.waves = static_cast<long>(u);
    } else if (a == "--dump-" + x + "-tile") {
      const int f = parse_format(fam, next(), &rest);
      if (f < 0 || !parse_u64(rest, &u, false) || u >= 65536)
        return usage("bad value for", a.c_str());
      t.dump_format = f;
      t.dump_wave = static_cast<long>(u);
    } else if (a == "--inject-" + x) {
      const int f = parse_format(fam, next(), &rest);
      if (f < 0 || !parse_pair(rest, &u, &elem) || u >= 65536 ||
          elem >= static_cast<uint64_t>(fam.elems[f]))
        return usage("bad value for", a.c_str());
      if (t.inject.size() == kMaxInject) return usage("too many", a.c_str());
      t.inject.push_back({f, static_cast<long>(u), static_cast<int>(elem)});
    } else if (fam.rate_instr != 0 && a == "--min-" + x + "-tflops") {
      const int f = parse_format(fam, next(), &rest);
      if (f < 0 || !parse_double(rest, &t.min_tflops[f]))
        return usage("bad value for", a.c_str());
    } else if (fam.rate_instr != 0 && a == "--" + x + "-rate-instr") {
      if (!parse_u64(next(), &u, false) || u == 0 || u > (1ull << 30))
        return usage("bad value for", a.c_str());
      t.rate_instr = u;
    } else {
      continue;
    }
    return 0;
  }
  return -1;
}

// Returns 0 on success, 2 on a usage error.
int parse_args(int argc, char** argv, Options* o) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* {
      return (i + 1 < argc) ? argv[++i] : nullptr;
    };
    uint64_t u = 0;
    if (const int rc = parse_tile_flag(a, next, o); rc >= 0) {
      if (rc != 0) return rc;
    } else if (a == "--cpu") {
      o->cpu = true;
    } else if (a == "--dump-pattern") {
      o->dump_pattern = true;
    } else if (a == "--bytes") {
      if (!parse_u64(next(), &u, true)) return usage("bad value for", "--bytes");
      o->bytes = static_cast<size_t>(u);
    } else if (a == "--passes") {
      if (!parse_u64(next(), &u, false) || u == 0 || u > 1024)
        return usage("bad value for", "--passes");
      o->passes = static_cast<uint32_t>(u);
    } else if (a == "--base-index") {
      if (!parse_u64(next(), &u, false))
        return usage("bad value for", "--base-index");
      o->base_index = u;
    } else if (a == "--seed") {
      if (!parse_u64(next(), &u, false)) return usage("bad value for", "--seed");
      o->seed = u;
    } else if (a == "--min-copy-gbs") {
      if (!parse_double(next(), &o->min_copy_gbs))
        return usage("bad value for", "--min-copy-gbs");
    } else if (a == "--inject-flip") {
      uint64_t bit = 0;
      if (!parse_pair(next(), &u, &bit) || bit > 7)
        return usage("bad value for", "--inject-flip");
      if (o->flips.size() == kMaxFlips)
        return usage("too many", "--inject-flip");
      o->flips.push_back({static_cast<size_t>(u), static_cast<int>(bit)});
    } else if (a == "--inject-pass") {
      if (!parse_u64(next(), &u, false) || u >= 1024)
        return usage("bad value for", "--inject-pass");
      o->inject_pass = static_cast<uint32_t>(u);
    } else if (a == "--inject-copy-flip") {
      uint64_t bit = 0;
      if (!parse_pair(next(), &u, &bit) || bit > 7)
        return usage("bad value for", "--inject-copy-flip");
      o->copy_flip = true;
      o->copy_flip_at = {static_cast<size_t>(u), static_cast<int>(bit)};
    } else if (a == "--dump-vectors") {
      const char* v = next();
      if (v == nullptr) return usage("bad value for", "--dump-vectors");
      std::string rest = v;
      for (;;) {
        const size_t comma = rest.find(',');
        if (!parse_u64(rest.substr(0, comma).c_str(), &u, false))
          return usage("bad value for", "--dump-vectors");
        if (o->dump_vectors.size() == kMaxDumpVectors)
          return usage("too many indices for", "--dump-vectors");
        o->dump_vectors.push_back(static_cast<size_t>(u));
        if (comma == std::string::npos) break;
        rest = rest.substr(comma + 1);
      }
    } else if (a == "--store-variant") {
      const char* v = next();
      const std::string s = v ? v : "";
      if (s == "auto") o->store_variant = -1;
      else if (s == kVariantNames[0]) o->store_variant = 0;
      else if (s == kVariantNames[1]) o->store_variant = 1;
      else return usage("bad value for", "--store-variant");
    } else if (a == "--lds-groups") {
      if (!parse_u64(next(), &u, false) || u > 65536)
        return usage("bad value for", "--lds-groups");
      o->lds_groups = static_cast<long>(u);
    } else if (a == "--lds-rounds") {
      if (!parse_u64(next(), &u, false) || u == 0 || u > 1024)
        return usage("bad value for", "--lds-rounds");
      o->lds_rounds = static_cast<uint32_t>(u);
    } else if (a == "--lds-max-launches") {
      if (!parse_u64(next(), &u, false) || u == 0 || u > 64)
        return usage("bad value for", "--lds-max-launches");
      o->lds_max_launches = static_cast<uint32_t>(u);
    } else if (a == "--lds-require-coverage") {
      o->lds_require_coverage = true;
    } else if (a == "--dump-lds-where") {
      o->dump_lds_where = true;
    } else if (a == "--dump-lds") {
      uint64_t f[3];
      if (!parse_fields(next(), 3, f) || f[0] >= 65536 || f[1] >= 1024 ||
          f[2] > 1)
        return usage("bad value for", "--dump-lds");
      o->dump_lds = true;
      o->dump_lds_group = static_cast<uint32_t>(f[0]);
      o->dump_lds_round = static_cast<uint32_t>(f[1]);
      o->dump_lds_pass = static_cast<uint32_t>(f[2]);
    } else if (a == "--inject-lds") {
      uint64_t f[5];
      if (!parse_fields(next(), 5, f) || f[0] >= 65536 || f[1] >= 1024 ||
          f[2] > 1 || f[3] >= static_cast<uint64_t>(gpucheck::kLdsBytes) ||
          f[4] > 7)
        return usage("bad value for", "--inject-lds");
      if (o->lds_inject.size() == kMaxLdsInject)
        return usage("too many", "--inject-lds");
      o->lds_inject.push_back({static_cast<uint32_t>(f[0]),
                               static_cast<uint32_t>(f[1]),
                               static_cast<uint32_t>(f[2]),
                               static_cast<uint32_t>(f[3]),
                               static_cast<uint32_t>(f[4])});
    } else {
      return usage("unknown argument", a.c_str());
    }
  }
  if (o->bytes < 16) o->bytes = 16;
  o->bytes &= ~static_cast<size_t>(15);
  const size_t nvec = o->bytes / 16;
  for (const Options::Flip& f : o->flips)
    if (f.offset >= o->bytes)
      return usage("--inject-flip offset is outside the region", nullptr);
  if (o->inject_pass >= o->passes)
    return usage("--inject-pass must be below --passes", nullptr);
  for (size_t i : o->dump_vectors)
    if (i >= nvec)
      return usage("--dump-vectors index is outside the region", nullptr);
  // The copy moves vectors [0, half) to [half, 2*half).
  const size_t half = nvec / 2;
  if (o->copy_flip && (o->copy_flip_at.offset < half * 16 ||
                       o->copy_flip_at.offset >= 2 * half * 16))
    return usage("--inject-copy-flip offset is outside the destination half",
                 nullptr);
  return 0;
}

int wave_outside_run(const std::string& flag) {
  return usage((flag + " wave is outside the run").c_str(), nullptr);
}

// A family's flags name waves, and how many waves run is known only once the
// device is. 0 waves: the stage does not run.
int check_tile_args(const Family& fam, const TileOptions& t, long nwaves) {
  const std::string x = fam.prefix;
  if (t.dump_wave >= nwaves) return wave_outside_run("--dump-" + x + "-tile");
  for (const Inject& m : t.inject)
    if (m.wave >= nwaves) return wave_outside_run("--inject-" + x);
  return 0;
}


// The same for the LDS flags: they name workgroups and rounds of the run.
int check_lds_args(const Options& o, long groups) {
  if (o.dump_lds && (o.dump_lds_group >= groups || o.dump_lds_round >= o.lds_rounds))
    return usage("--dump-lds group or round is outside the run", nullptr);
  for (const Options::LdsInject& m : o.lds_inject)
    if (m.group >= groups || m.round >= o.lds_rounds)
      return usage("--inject-lds group or round is outside the run", nullptr);
  return 0;
}

// ----------------------------------------------------------------- report

struct Report {
  std::string device = "cpu";
  int compute_units = 0;
  // HBM
  uint64_t mismatch_vectors = 0;
  bool have_first_bad = false;
  uint64_t first_bad_offset = 0;
  uint32_t first_bad_pass = 0;
  Vec16 first_bad_xor{0, 0};
  double write_gbs = 0, read_gbs = 0;
  double write_gbs_plain = 0, write_gbs_nontemporal = 0;
  const char* store_variant = "plain";
  std::vector<std::string> pattern_dump;
  struct VecDump {
    size_t index;
    uint32_t pass;
    std::string value;
  };
  std::vector<VecDump> vector_dump;  // as read back from the region
  // copy: bandwidth and the verification of what was copied
  const char* bandwidth = "skipped";
  double copy_gbs = 0;
  const char* copy = "skipped";
  uint64_t copy_mismatch_vectors = 0;
  bool have_copy_first_bad = false;
  uint64_t copy_first_bad_offset = 0;  // within the whole region
  Vec16 copy_first_bad_xor{0, 0};
  // MFMA, MX and dense
  struct TileResult {
    const char* verdict = "skipped";
    const char* rate = "skipped";
    long waves = 0;
    struct Format {
      long bad_waves = 0, first_bad_wave = -1;
      double tflops = 0, launch_ms = 0;
    };
    Format formats[kMaxFormats];
    // The dumped tile, values times the format's scale; kNotAnInteger where
    // that is none within the family's bound.
    std::vector<long long> dump;
    // Where the waves ran: [cu key, simd] per format and wave, format-major.
    // Empty under --cpu.
    std::vector<uint32_t> where;
    double seconds = 0;  // wall time of the stage, host product included
  };
  TileResult tile[kFamilies];
  int clock_mhz = 0;  // the device's reported clock; 0 under --cpu
  // LDS
  const char* lds = "skipped";
  std::string lds_skip_reason;
  long lds_groups = 0, lds_launches = 0, lds_bad_groups = 0;
  std::set<uint32_t> lds_cus;  // CU keys seen
  struct LdsBadCu {
    uint64_t bad_vectors = 0;
    unsigned long long first = kNoBad;  // lds_pack(round, pass, vector)
    Vec16 first_xor{0, 0};
  };
  std::map<uint32_t, LdsBadCu> lds_bad_cus;  // by CU key
  double lds_gbs = 0;
  std::vector<uint32_t> lds_where;  // first launch: [cu key, simd] per wave
  bool lds_dump_valid = false;
  uint64_t lds_dump_fnv64 = 0;
  long lds_dump_same_wave_reads = 0;
  std::vector<std::string> lds_dump_vectors;
};

std::string where_name(uint32_t key) {
  char buf[64];
  snprintf(buf, sizeof(buf), "xcc%u.se%u.sh%u.cu%u", key >> kKeyXccShift,
           (key >> kKeySeShift) & ((1u << kHwSe.bits) - 1),
           (key >> kKeyShShift) & ((1u << kHwSh.bits) - 1),
           key & ((1u << kHwCu.bits) - 1));
  return buf;
}

std::string hex128(const Vec16& v) {
  char buf[40];
  snprintf(buf, sizeof(buf), "%016llx%016llx",
           static_cast<unsigned long long>(v.hi),
           static_cast<unsigned long long>(v.lo));
  return buf;
}

double gbs(double bytes, double seconds) {
  return seconds > 0 ? bytes / 1e9 / seconds : 0.0;
}

// ---------------------------------------------------------------- backends

struct Backend {
  virtual ~Backend() {}
  virtual int store_variants() const = 0;
  // Both return elapsed seconds.
  virtual double fill(uint32_t pass, int variant) = 0;
  virtual double verify(uint32_t pass, uint64_t* bad, uint64_t* first) = 0;
  virtual Vec16 read_vec(size_t i) = 0;
  virtual void write_vec(size_t i, const Vec16& v) = 0;
};

struct CpuBackend : Backend {
  const Options& o;
  size_t nvec;
  Vec16* mem;
  explicit CpuBackend(const Options& opt)
      : o(opt), nvec(opt.bytes / 16),
        mem(static_cast<Vec16*>(malloc(opt.bytes))) {}
  ~CpuBackend() override { free(mem); }
  int store_variants() const override { return 1; }
  static double since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0)
        .count();
  }
  double fill(uint32_t pass, int) override {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < nvec; ++i)
      mem[i] = gpucheck::pattern(o.seed, pass, o.base_index + i);
    return since(t0);
  }
  double verify(uint32_t pass, uint64_t* bad, uint64_t* first) override {
    const auto t0 = std::chrono::steady_clock::now();
    *bad = 0;
    *first = kNoBad;
    for (size_t i = 0; i < nvec; ++i) {
      const Vec16 want = gpucheck::pattern(o.seed, pass, o.base_index + i);
      if (mem[i].lo != want.lo || mem[i].hi != want.hi) {
        ++*bad;
        if (i < *first) *first = i;
      }
    }
    return since(t0);
  }
  Vec16 read_vec(size_t i) override { return mem[i]; }
  void write_vec(size_t i, const Vec16& v) override { mem[i] = v; }
};

unsigned int grid_for(size_t nvec) {
  const size_t blocks = (nvec + kBlock - 1) / kBlock;
  return static_cast<unsigned int>(std::max<size_t>(1, std::min(blocks, kMaxGrid)));
}

struct GpuTimer {
  hipEvent_t start = nullptr, stop = nullptr;
  void init() {
    HIP_CHECK(hipEventCreate(&start));
    HIP_CHECK(hipEventCreate(&stop));
  }
  void begin() { HIP_CHECK(hipEventRecord(start, 0)); }
  double end() {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(stop, 0));
    HIP_CHECK(hipEventSynchronize(stop));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, start, stop));
    return ms / 1e3;
  }
  ~GpuTimer() {
    if (start) (void)hipEventDestroy(start);
    if (stop) (void)hipEventDestroy(stop);
  }
};

// The median of five timed launches after one that warms up.
template <typename Launch>
double median_launch_seconds(GpuTimer& timer, Launch&& launch) {
  std::vector<double> times;
  for (int rep_i = 0; rep_i < 6; ++rep_i) {
    timer.begin();
    launch();
    const double s = timer.end();
    if (rep_i > 0) times.push_back(s);
  }
  std::sort(times.begin(), times.end());
  return times[times.size() / 2];
}

struct GpuBackend : Backend {
  const Options& o;
  size_t nvec;
  u32x4* mem = nullptr;
  unsigned long long* counters = nullptr;
  GpuTimer timer;
  explicit GpuBackend(const Options& opt) : o(opt), nvec(opt.bytes / 16) {
    HIP_CHECK(hipMalloc(&mem, o.bytes));
    HIP_CHECK(hipMalloc(&counters, 2 * sizeof(unsigned long long)));
    timer.init();
    // Load both fill kernels before anything is timed.
    const size_t warm = std::min<size_t>(nvec, kBlock);
    hipLaunchKernelGGL(hbm_fill<false>, dim3(1), dim3(kBlock), 0, 0, mem, warm,
                       o.base_index, o.seed, 0u);
    hipLaunchKernelGGL(hbm_fill<true>, dim3(1), dim3(kBlock), 0, 0, mem, warm,
                       o.base_index, o.seed, 0u);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
  }
  ~GpuBackend() override {
    if (mem) (void)hipFree(mem);
    if (counters) (void)hipFree(counters);
  }
  int store_variants() const override { return 2; }
  double fill(uint32_t pass, int variant) override {
    const dim3 grid(grid_for(nvec)), block(kBlock);
    timer.begin();
    if (variant == 1)
      hipLaunchKernelGGL(hbm_fill<true>, grid, block, 0, 0, mem, nvec,
                         o.base_index, o.seed, pass);
    else
      hipLaunchKernelGGL(hbm_fill<false>, grid, block, 0, 0, mem, nvec,
                         o.base_index, o.seed, pass);
    return timer.end();
  }
  double verify(uint32_t pass, uint64_t* bad, uint64_t* first) override {
    return verify_range(0, nvec, pass, bad, first);
  }
  // Checks that vectors [at, at + n) hold the pattern of logical indices
  // base_index + 0..n-1; *first is relative to `at`.
  double verify_range(size_t at, size_t n, uint32_t pass, uint64_t* bad,
                      uint64_t* first) {
    const unsigned long long init[2] = {0ull, kNoBad};
    HIP_CHECK(hipMemcpy(counters, init, sizeof(init), hipMemcpyHostToDevice));
    timer.begin();
    hipLaunchKernelGGL(hbm_verify, dim3(grid_for(n)), dim3(kBlock), 0, 0,
                       mem + at, n, o.base_index, o.seed, pass, counters);
    const double s = timer.end();
    unsigned long long got[2];
    HIP_CHECK(hipMemcpy(got, counters, sizeof(got), hipMemcpyDeviceToHost));
    *bad = got[0];
    *first = got[1];
    return s;
  }
  Vec16 read_vec(size_t i) override {
    Vec16 v;
    HIP_CHECK(hipMemcpy(&v, mem + i, sizeof(v), hipMemcpyDeviceToHost));
    return v;
  }
  void write_vec(size_t i, const Vec16& v) override {
    HIP_CHECK(hipMemcpy(mem + i, &v, sizeof(v), hipMemcpyHostToDevice));
  }
};

// ------------------------------------------------------------------ stages

void flip_bit(Backend& be, const Options::Flip& f) {
  const size_t vi = f.offset / 16;
  Vec16 v = be.read_vec(vi);
  unsigned char raw[16];
  memcpy(raw, &v, 16);
  raw[f.offset % 16] ^= static_cast<unsigned char>(1u << f.bit);
  memcpy(&v, raw, 16);
  be.write_vec(vi, v);
}

void run_hbm(Backend& be, const Options& o, Report* rep) {
  const size_t nvec = o.bytes / 16;
  const double bytes = static_cast<double>(o.bytes);
  const bool forced = o.store_variant >= 0;
  int variant = forced ? o.store_variant : 0;
  if (forced) rep->store_variant = kVariantNames[variant];
  if (o.dump_pattern) {
    // What the host expects, not what the region holds: see --dump-vectors.
    for (size_t i = 0; i < std::min<size_t>(nvec, 4); ++i)
      rep->pattern_dump.push_back(
          hex128(gpucheck::pattern(o.seed, 0, o.base_index + i)));
  }
  for (uint32_t pass = 0; pass < o.passes; ++pass) {
    double write_s;
    if (pass == 0 && !forced && be.store_variants() > 1) {
      // Both variants write the same data; keep the faster for later passes.
      const double plain_s = be.fill(0, 0);
      const double nt_s = be.fill(0, 1);
      rep->write_gbs_plain = gbs(bytes, plain_s);
      rep->write_gbs_nontemporal = gbs(bytes, nt_s);
      variant = nt_s < plain_s ? 1 : 0;
      rep->store_variant = variant ? "nontemporal" : "plain";
      write_s = variant ? nt_s : plain_s;
    } else {
      write_s = be.fill(pass, variant);
    }
    rep->write_gbs = std::max(rep->write_gbs, gbs(bytes, write_s));
    if (pass == o.inject_pass)
      for (const Options::Flip& f : o.flips) flip_bit(be, f);
    uint64_t bad = 0, first = kNoBad;
    const double read_s = be.verify(pass, &bad, &first);
    rep->read_gbs = std::max(rep->read_gbs, gbs(bytes, read_s));
    rep->mismatch_vectors += bad;
    if (bad != 0 && !rep->have_first_bad && first < nvec) {
      const Vec16 got = be.read_vec(static_cast<size_t>(first));
      const Vec16 want = gpucheck::pattern(o.seed, pass, o.base_index + first);
      rep->have_first_bad = true;
      rep->first_bad_offset = first * 16;
      rep->first_bad_pass = pass;
      rep->first_bad_xor = Vec16{got.lo ^ want.lo, got.hi ^ want.hi};
    }
  }
  // A run of one variant reports that variant's bandwidth and 0 for the other.
  if (forced)
    (variant ? rep->write_gbs_nontemporal : rep->write_gbs_plain) =
        rep->write_gbs;
  else if (be.store_variants() == 1)
    rep->write_gbs_plain = rep->write_gbs;
  for (size_t i : o.dump_vectors)
    rep->vector_dump.push_back({i, o.passes - 1, hex128(be.read_vec(i))});
}

void run_copy(GpuBackend& be, const Options& o, Report* rep) {
  const size_t half = be.nvec / 2;
  if (half == 0) return;  // a one-vector region has nothing to copy
  const dim3 grid(grid_for(half)), block(kBlock);
  const double seconds = median_launch_seconds(be.timer, [&] {
    hipLaunchKernelGGL(vec_copy, grid, block, 0, 0, be.mem + half, be.mem, half);
  });
  rep->copy_gbs = gbs(2.0 * 16.0 * static_cast<double>(half), seconds);
  rep->bandwidth =
      (o.min_copy_gbs > 0 && rep->copy_gbs < o.min_copy_gbs) ? "fail" : "pass";

  // The source half still holds the last pass's pattern for indices
  // 0..half-1, so the destination half must verify against exactly that.
  // With an odd vector count the last vector belongs to neither half.
  if (o.copy_flip) flip_bit(be, o.copy_flip_at);
  const uint32_t pass = o.passes - 1;
  uint64_t bad = 0, first = kNoBad;
  be.verify_range(half, half, pass, &bad, &first);
  rep->copy_mismatch_vectors = bad;
  rep->copy = bad ? "fail" : "pass";
  if (bad != 0 && first < half) {
    const Vec16 got = be.read_vec(half + static_cast<size_t>(first));
    const Vec16 want = gpucheck::pattern(o.seed, pass, o.base_index + first);
    rep->have_copy_first_bad = true;
    rep->copy_first_bad_offset = (half + first) * 16;
    rep->copy_first_bad_xor = Vec16{got.lo ^ want.lo, got.hi ^ want.hi};
  }
}

// The 32x32 tile wave `w` must produce, row-major: integers of magnitude
// <= 1152.
void mfma_expected_tile(int, uint64_t seed, long w, double* out) {
  using gpucheck::kMfmaK;
  std::vector<int> a(32 * kMfmaK), bt(32 * kMfmaK);
  const uint64_t key_a = gpucheck::mfma_key(seed, static_cast<uint32_t>(w), 0);
  const uint64_t key_b = gpucheck::mfma_key(seed, static_cast<uint32_t>(w), 1);
  for (int r = 0; r < 32; ++r)
    for (int k = 0; k < kMfmaK; ++k) {
      a[r * kMfmaK + k] = gpucheck::mfma_a(key_a, r, k);
      bt[r * kMfmaK + k] = gpucheck::mfma_b(key_b, k, r);  // B transposed
    }
  for (int row = 0; row < 32; ++row)
    for (int col = 0; col < 32; ++col) {
      int sum = 0;
      for (int k = 0; k < kMfmaK; ++k)
        sum += a[row * kMfmaK + k] * bt[col * kMfmaK + k];
      out[row * 32 + col] = sum;
    }
}

// A family's tiles in host memory, per format: tiles[f][w * elems + e].
// Whatever the device stored (f32, i32 or f64) is held as a double, which
// every one of them converts to exactly, NaN included; so one judge serves
// all formats.
using Tiles = std::vector<double>[kMaxFormats];

// Everything after the tiles are in host memory: the dump, the injections,
// the comparison and the verdict.
void judge_tiles(const Family& fam, Tiles& tiles, long nwaves,
                 const TileOptions& t, uint64_t seed, Report::TileResult* r) {
  r->waves = nwaves;
  if (t.dump_wave >= 0) {
    const int f = t.dump_format;
    const double* tile = tiles[f].data() + t.dump_wave * fam.elems[f];
    for (int e = 0; e < fam.elems[f]; ++e) {
      const double scaled = tile[e] * fam.scale[f];
      // Not a finite integer within the bound: no value in the dump (the
      // comparison below finds the wave bad: every expected value is an
      // integer within the bound).
      const bool integer =
          scaled >= -fam.dump_bound && scaled <= fam.dump_bound &&
          scaled == static_cast<double>(static_cast<long long>(scaled));
      r->dump.push_back(integer ? static_cast<long long>(scaled)
                                : kNotAnInteger);
    }
  }
  for (const Inject& m : t.inject)
    tiles[m.format][m.wave * fam.elems[m.format] + m.elem] += 1.0;
  std::vector<double> want(32 * 32);
  bool any = false;
  for (int f = 0; f < fam.formats; ++f) {
    Report::TileResult::Format& fr = r->formats[f];
    for (long w = 0; w < nwaves; ++w) {
      fam.expected_tile(f, seed, w, want.data());
      const double* tile = tiles[f].data() + w * fam.elems[f];
      // Exact by the bounds in gpucheck_pattern.h (MFMA: integers of magnitude
      // <= 1152): == is bit-exactness, and NaN compares unequal. want holds
      // the value times the scale.
      bool bad = false;
      for (int e = 0; e < fam.elems[f] && !bad; ++e)
        bad = !(tile[e] * fam.scale[f] == want[e]);
      if (bad) {
        if (fr.bad_waves == 0) fr.first_bad_wave = w;
        ++fr.bad_waves;
        any = true;
      }
    }
  }
  r->verdict = any ? "fail" : "pass";
}

// --cpu: the tiles come from the host product, so this exercises the
// decoders, judge_tiles and the JSON, not a device. No rate is measured.
void run_tiles_cpu(const Family& fam, long nwaves, const TileOptions& t,
                   uint64_t seed, Report::TileResult* r) {
  Tiles tiles;
  std::vector<double> want(32 * 32);
  for (int f = 0; f < fam.formats; ++f) {
    tiles[f].resize(static_cast<size_t>(nwaves) * fam.elems[f]);
    for (long w = 0; w < nwaves; ++w) {
      fam.expected_tile(f, seed, w, want.data());
      for (int e = 0; e < fam.elems[f]; ++e)
        tiles[f][w * fam.elems[f] + e] = want[e] / fam.scale[f];
    }
  }
  judge_tiles(fam, tiles, nwaves, t, seed, r);
}


// [cu key, simd] per wave on the device, preset to all ones.
struct WhereBuffer {
  uint32_t* dev = nullptr;
  size_t nwaves;
  explicit WhereBuffer(size_t n) : nwaves(n) {
    HIP_CHECK(hipMalloc(&dev, 2 * n * sizeof(uint32_t)));
    HIP_CHECK(hipMemset(dev, 0xFF, 2 * n * sizeof(uint32_t)));
  }
  ~WhereBuffer() {
    if (dev) (void)hipFree(dev);
  }
  std::vector<uint32_t> fetch() {
    std::vector<uint32_t> host(2 * nwaves);
    HIP_CHECK(hipMemcpy(host.data(), dev, host.size() * sizeof(uint32_t),
                        hipMemcpyDeviceToHost));
    return host;
  }
};

// Distinct CU keys and distinct (CU key, SIMD) pairs of a where list.
void count_where(const std::vector<uint32_t>& where, size_t* cus, size_t* simds) {
  std::set<uint32_t> keys;
  std::set<std::pair<uint32_t, uint32_t>> pairs;
  for (size_t w = 0; 2 * w + 1 < where.size(); ++w) {
    keys.insert(where[2 * w]);
    pairs.insert({where[2 * w], where[2 * w + 1]});
  }
  *cus = keys.size();
  *simds = pairs.size();
}

// "xcc2.se1.sh0.cu5" of wave `w` of a where list, "" without one.
std::string where_of(const std::vector<uint32_t>& where, long w) {
  if (w < 0 || 2 * static_cast<size_t>(w) + 1 >= where.size()) return "";
  return where_name(where[2 * w]);
}

// One format's device round trip: `launch(blocks, tiles, where)` starts its
// self-test, one wave per tile of `elems` values of type Elem. The tiles come
// back into *tiles as doubles and the where list is appended to *where_all.
template <typename Elem, typename Launch>
void fetch_tiles(long nwaves, int elems, Launch&& launch,
                 std::vector<double>* tiles, std::vector<uint32_t>* where_all) {
  const size_t n = static_cast<size_t>(nwaves) * elems;
  Elem* dev = nullptr;
  HIP_CHECK(hipMalloc(&dev, n * sizeof(Elem)));
  HIP_CHECK(hipMemset(dev, 0xFF, n * sizeof(Elem)));
  WhereBuffer where(static_cast<size_t>(nwaves));
  launch(static_cast<unsigned int>((nwaves + 3) / 4), dev, where.dev);
  HIP_CHECK(hipGetLastError());
  const std::unique_ptr<Elem[]> host(new Elem[n]);  // not zeroed first
  HIP_CHECK(hipMemcpy(host.get(), dev, n * sizeof(Elem), hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(dev));
  tiles->assign(host.get(), host.get() + n);
  const std::vector<uint32_t> ran = where.fetch();
  where_all->insert(where_all->end(), ran.begin(), ran.end());
}

// call(std::integral_constant<int, 0>{}) ... call(<int, kCount - 1>{}), in
// order: the format index is a template argument of the kernels.
template <typename Call, int... kIndex>
void for_each_index(std::integer_sequence<int, kIndex...>, Call&& call) {
  (call(std::integral_constant<int, kIndex>{}), ...);
}
template <int kCount, typename Call>
void for_each_format(Call&& call) {
  for_each_index(std::make_integer_sequence<int, kCount>{}, call);
}

// The rate kernels of one family: two workgroups of four waves per compute
// unit put waves on every SIMD. The sink holds the widest element, one per
// lane.
struct RateRun {
  unsigned int blocks;
  uint32_t trips;
  void* sink = nullptr;
  GpuTimer timer;
  RateRun(const TileOptions& t, int compute_units)
      : blocks(static_cast<unsigned int>(2 * std::max(1, compute_units))),
        trips(static_cast<uint32_t>((t.rate_instr + 3) / 4)) {
    HIP_CHECK(hipMalloc(&sink, static_cast<size_t>(blocks) * kBlock * sizeof(double)));
    timer.init();
  }
  ~RateRun() {
    if (sink) (void)hipFree(sink);
  }
  // `launch` issues 4 * trips MFMAs of `flop_each` per wave. For i8 the
  // figure is 10^12 integer operations per second.
  template <typename Launch>
  void time(double flop_each, Launch&& launch, Report::TileResult::Format* fr) {
    const double seconds = median_launch_seconds(timer, launch);
    const double flop = flop_each * 4.0 * trips * (blocks * 4.0);
    fr->tflops = seconds > 0 ? flop / seconds / 1e12 : 0.0;
    fr->launch_ms = seconds * 1e3;
  }
};

// Holds every format's measured rate to its floor, where one is set.
void check_rate_floors(const Family& fam, const TileOptions& t,
                       Report::TileResult* r) {
  r->rate = "pass";
  for (int f = 0; f < fam.formats; ++f)
    if (t.min_tflops[f] > 0 && r->formats[f].tflops < t.min_tflops[f])
      r->rate = "fail";
}

// A family's kernels: Elem<kFmt> is what a lane of format kFmt stores per
// result, selftest<kFmt>() and rate<kFmt>() are its kernels, and flop_each(f)
// is the operations of one of its MFMAs. MFMA has no rate kernel.
struct MfmaKernels {
  static constexpr int kFamily = kMfma, kFormats = 1;
  static constexpr bool kRated = false;
  template <int>
  using Elem = float;
  template <int>
  static constexpr auto selftest() { return mfma_selftest; }
};

struct MxKernels {
  static constexpr int kFamily = kMx, kFormats = gpucheck::kMxFormats;
  static constexpr bool kRated = true;
  template <int>
  using Elem = float;
  template <int kFmt>
  static constexpr auto selftest() { return mx_selftest<kFmt>; }
  template <int kFmt>
  static constexpr auto rate() { return mx_rate<kFmt>; }
  static double flop_each(int) { return 2.0 * 32 * 32 * 64; }
};

struct DenseKernels {
  static constexpr int kFamily = kDense, kFormats = gpucheck::kDenseFormats;
  static constexpr bool kRated = true;
  template <int kFmt>
  using Elem = typename DenseTypes<kFmt>::Elem;
  template <int kFmt>
  static constexpr auto selftest() { return dense_selftest<kFmt>; }
  template <int kFmt>
  static constexpr auto rate() { return dense_rate<kFmt>; }
  static double flop_each(int f) {
    const gpucheck::DenseFormat& fmt = gpucheck::kDenseFormatTable[f];
    return 2.0 * fmt.mn * fmt.mn * fmt.step_k;
  }
};

// One family's stage on the device: every format's tiles, judged, then every
// format's rate, held to its floor.
template <typename Kernels>
void run_tiles(const Options& o, long nwaves, int compute_units, Report* rep) {
  const auto s0 = std::chrono::steady_clock::now();
  const Family& fam = kFamilyTable[Kernels::kFamily];
  const TileOptions& t = o.tile[Kernels::kFamily];
  Report::TileResult& r = rep->tile[Kernels::kFamily];
  Tiles tiles;
  for_each_format<Kernels::kFormats>([&](auto format) {
    constexpr int kFmt = decltype(format)::value;
    using Elem = typename Kernels::template Elem<kFmt>;
    fetch_tiles<Elem>(
        nwaves, fam.elems[kFmt],
        [&](unsigned int blocks, Elem* dev, uint32_t* where) {
          const auto kernel = Kernels::template selftest<kFmt>();
          hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, 0, dev,
                             where, static_cast<uint32_t>(nwaves), o.seed);
        },
        &tiles[kFmt], &r.where);
  });
  judge_tiles(fam, tiles, nwaves, t, o.seed, &r);
  if constexpr (Kernels::kRated) {
    RateRun run(t, compute_units);
    for_each_format<Kernels::kFormats>([&](auto format) {
      constexpr int kFmt = decltype(format)::value;
      using Elem = typename Kernels::template Elem<kFmt>;
      static_assert(sizeof(Elem) <= sizeof(double));
      run.time(
          Kernels::flop_each(kFmt),
          [&] {
            const auto kernel = Kernels::template rate<kFmt>();
            hipLaunchKernelGGL(kernel, dim3(run.blocks), dim3(kBlock), 0, 0,
                               static_cast<Elem*>(run.sink), run.trips, o.seed);
          },
          &r.formats[kFmt]);
    });
    check_rate_floors(fam, t, &r);
  }
  r.seconds = CpuBackend::since(s0);
}

// Decoders of the MX element and scale codes, from the OCP formulas: sign,
// exponent field e with its bias, mantissa field m; e = 0 is subnormal.
double decode_minifloat(uint32_t code, int exp_bits, int mant_bits, int bias) {
  const uint32_t m = code & ((1u << mant_bits) - 1);
  const uint32_t e = (code >> mant_bits) & ((1u << exp_bits) - 1);
  const bool neg = (code >> (exp_bits + mant_bits)) & 1u;
  const double frac = static_cast<double>(m) / (1u << mant_bits);
  const double mag = e == 0 ? ldexp(frac, 1 - bias)
                            : ldexp(1.0 + frac, static_cast<int>(e) - bias);
  return neg ? -mag : mag;
}

double decode_e2m1(uint32_t code) { return decode_minifloat(code, 2, 1, 1); }

// e4m3fn: no infinities, and S.1111.111 is the only NaN.
double decode_e4m3(uint32_t code) {
  if ((code & 0x7Fu) == 0x7Fu) return NAN;
  return decode_minifloat(code, 4, 3, 7);
}

// e5m2: IEEE-like, exponent field 31 is infinity or NaN.
double decode_e5m2(uint32_t code) {
  if ((code & 0x7Cu) == 0x7Cu)
    return (code & 3u) ? NAN : ((code & 0x80u) ? -INFINITY : INFINITY);
  return decode_minifloat(code, 5, 2, 15);
}

double decode_e8m0(uint32_t code) {
  return code == 255 ? NAN : ldexp(1.0, static_cast<int>(code) - 127);
}

// The 32x32 tile wave `w` must produce in format `f`, times 16, row-major:
// decode every element and scale, multiply, sum over k. Operands are held
// times 4 (exact: an element is a multiple of 1/2 and a scale at least 1/2)
// and every sum is an integer below 2^24, so the float arithmetic is exact;
// the loop order keeps the inner loop free of a reduction.
void mx_expected_tile(int f, uint64_t seed, long w, double* out) {
  using gpucheck::kMxBlock;
  using gpucheck::kMxK;
  const gpucheck::MxFormat& fmt = gpucheck::kMxFormatTable[f];
  const uint64_t key_a = gpucheck::mx_key(seed, static_cast<uint32_t>(w), f, 0);
  const uint64_t key_b = gpucheck::mx_key(seed, static_cast<uint32_t>(w), f, 1);
  // Thousands of tiles draw on the same few codes, so each is generated and
  // decoded once: an element's code depends on kMxHashBits bits of its hash.
  constexpr uint32_t nhash = 1u << gpucheck::kMxHashBits;
  static const std::vector<double> table = [] {
    std::vector<double> t(3 * nhash + 256);
    for (uint32_t h = 0; h < nhash; ++h) {
      t[h] = decode_e4m3(gpucheck::mx_code_from_hash(gpucheck::kMxE4M3, h));
      t[nhash + h] =
          decode_e5m2(gpucheck::mx_code_from_hash(gpucheck::kMxE5M2, h));
      t[2 * nhash + h] =
          decode_e2m1(gpucheck::mx_code_from_hash(gpucheck::kMxE2M1, h));
    }
    for (uint32_t c = 0; c < 256; ++c) t[3 * nhash + c] = decode_e8m0(c);
    return t;
  }();
  auto values_of = [&](int type) {
    return &table[type == gpucheck::kMxE2M1 ? 2 * nhash : nhash * type];
  };
  const double* dec_a = values_of(fmt.a);
  const double* dec_b = values_of(fmt.b);
  const double* dec_scale = &table[3 * nhash];
  // Kept across the thousands of calls: every element is written below.
  static std::vector<float> a(32 * kMxK), b(kMxK * 32);
  for (int r = 0; r < 32; ++r)
    for (int blk = 0; blk < kMxK / kMxBlock; ++blk) {
      const double sa = dec_scale[gpucheck::mx_scale_byte(key_a, r, blk)];
      const double sb = dec_scale[gpucheck::mx_scale_byte(key_b, r, blk)];
      for (int k = blk * kMxBlock; k < (blk + 1) * kMxBlock; ++k) {
        a[r * kMxK + k] = static_cast<float>(
            4.0 * sa * dec_a[gpucheck::mx_a_hash(key_a, r, k) & (nhash - 1)]);
        b[k * 32 + r] = static_cast<float>(
            4.0 * sb * dec_b[gpucheck::mx_b_hash(key_b, k, r) & (nhash - 1)]);
      }
    }
  for (int row = 0; row < 32; ++row) {
    float sums[32] = {};
    for (int k = 0; k < kMxK; ++k) {
      const float av = a[row * kMxK + k];
      const float* brow = &b[k * 32];
      for (int col = 0; col < 32; ++col) sums[col] += av * brow[col];
    }
    for (int col = 0; col < 32; ++col) out[row * 32 + col] = sums[col];
  }
}

// ------------------------------------------------------------ dense stage

// The tile wave `w` must produce in format `f`, times the format's scale,
// row-major: an integer matrix product. The operands of fp8 and bf8 are
// decoded from their codes and held times 2 (exact: multiples of 1/2), so
// their product is in quarter-units. The arithmetic is floating point that
// holds these integers exactly, by the bounds in gpucheck_pattern.h: Acc is
// float below 2^24 (all but f64) and double below 2^53 for f64. As in
// mx_expected_tile, the loop order keeps the inner loop free of a reduction.
template <typename Acc>
void dense_expected_tile_as(int f, uint64_t seed, long w, double* out) {
  using namespace gpucheck;
  const DenseFormat& fmt = kDenseFormatTable[f];
  const int mn = fmt.mn, K = fmt.k;
  const uint64_t key_a = dense_key(seed, static_cast<uint32_t>(w), f, 0);
  const uint64_t key_b = dense_key(seed, static_cast<uint32_t>(w), f, 1);
  // An 8-bit float element depends on kMxHashBits bits of its hash: each
  // code is generated and decoded once.
  constexpr uint32_t nhash = 1u << kMxHashBits;
  static const std::vector<int> doubled = [] {
    std::vector<int> t(2 * nhash);
    for (uint32_t h = 0; h < nhash; ++h) {
      t[h] = static_cast<int>(
          2.0 * decode_e4m3(dense_code_from_hash(kDenseFp8, h)));
      t[nhash + h] = static_cast<int>(
          2.0 * decode_e5m2(dense_code_from_hash(kDenseBf8, h)));
    }
    return t;
  }();
  auto element = [&](uint64_t h) -> int {
    if (f == kDenseFp8) return doubled[h & (nhash - 1)];
    if (f == kDenseBf8) return doubled[nhash + (h & (nhash - 1))];
    return static_cast<int>(dense_int_from_hash(f, h));
  };
  std::vector<Acc> a(static_cast<size_t>(mn) * K), b(static_cast<size_t>(K) * mn);
  for (int r = 0; r < mn; ++r)
    for (int k = 0; k < K; ++k) {
      a[r * K + k] = element(dense_a_hash(f, key_a, r, k));
      b[k * mn + r] = element(dense_b_hash(f, key_b, k, r));
    }
  std::vector<Acc> sums(mn);
  for (int row = 0; row < mn; ++row) {
    for (int col = 0; col < mn; ++col) sums[col] = 0;
    for (int k = 0; k < K; ++k) {
      const Acc av = a[row * K + k];
      const Acc* brow = &b[k * mn];
      for (int col = 0; col < mn; ++col) sums[col] += av * brow[col];
    }
    for (int col = 0; col < mn; ++col) out[row * mn + col] = sums[col];
  }
}

void dense_expected_tile(int f, uint64_t seed, long w, double* out) {
  if (f == gpucheck::kDenseF64)
    dense_expected_tile_as<double>(f, seed, w, out);
  else
    dense_expected_tile_as<float>(f, seed, w, out);
}

// -------------------------------------------------------------- LDS stage

uint64_t fnv1a64(const unsigned char* p, size_t n) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
  return h;
}

constexpr int kLdsDumpVectors[] = {0, 1, 255, 256, 4095, 4096, 4097, 10238, 10239};

constexpr size_t kLdsDumpBytes =
    gpucheck::kLdsBytes + gpucheck::kLdsVectors * sizeof(uint32_t);

// `bytes`: the kLdsBytes one workgroup read back in the dumped round and
// pass; `readers`: the thread that read each vector. Thread i % 256 wrote
// vector i, so a vector whose reader is in that thread's wave was not read
// back across waves.
void record_lds_dump(const unsigned char* bytes, const uint32_t* readers,
                     Report* rep) {
  rep->lds_dump_valid = true;
  rep->lds_dump_same_wave_reads = 0;
  for (uint32_t i = 0; i < static_cast<uint32_t>(gpucheck::kLdsVectors); ++i)
    if (readers[i] >= kBlock || (readers[i] >> 6) == ((i % kBlock) >> 6))
      ++rep->lds_dump_same_wave_reads;
  rep->lds_dump_fnv64 = fnv1a64(bytes, gpucheck::kLdsBytes);
  for (int i : kLdsDumpVectors) {
    Vec16 v;
    memcpy(&v, bytes + 16 * static_cast<size_t>(i), 16);
    rep->lds_dump_vectors.push_back(hex128(v));
  }
}

LdsInjections lds_injections(const Options& o) {
  LdsInjections inj = {};
  for (const Options::LdsInject& m : o.lds_inject) {
    auto& at = inj.at[inj.n++];
    at.group = m.group;
    at.round = m.round;
    at.pass = m.pass;
    at.dword = m.byte / 4;
    at.mask = 1u << (8 * (m.byte % 4) + m.bit);
  }
  return inj;
}

// One launch's records and where list (four waves per group) into the
// report: the CU keys seen, and the mismatches merged by compute unit.
void judge_lds(const std::vector<LdsRecord>& records,
               const std::vector<uint32_t>& where, Report* rep) {
  for (size_t g = 0; g < records.size(); ++g) {
    for (int w = 0; w < 4; ++w) rep->lds_cus.insert(where[2 * (4 * g + w)]);
    const LdsRecord& rec = records[g];
    if (rec.bad == 0) continue;
    ++rep->lds_bad_groups;
    Report::LdsBadCu& cu = rep->lds_bad_cus[where[2 * (4 * g)]];
    cu.bad_vectors += rec.bad;
    if (rec.first < cu.first) {
      cu.first = rec.first;
      cu.first_xor.lo = rec.first_xor.x | (static_cast<uint64_t>(rec.first_xor.y) << 32);
      cu.first_xor.hi = rec.first_xor.z | (static_cast<uint64_t>(rec.first_xor.w) << 32);
    }
  }
  rep->lds = rep->lds_bad_groups ? "fail" : "pass";
}

// --cpu: what lds_selftest does, in its order, over a host buffer per group:
// this exercises the injection, the record, judge_lds and the JSON, not a
// device. Every wave of group g reports compute unit g % 5 and its own
// number as the SIMD.
void run_lds_cpu(const Options& o, long groups, Report* rep) {
  constexpr int trips = gpucheck::kLdsVectors / kBlock;
  rep->lds_groups = groups;
  rep->lds_launches = 1;
  const LdsInjections inj = lds_injections(o);
  std::vector<LdsRecord> records(static_cast<size_t>(groups));
  std::vector<uint32_t> where(static_cast<size_t>(groups) * 8);
  std::vector<u32x4> lds(gpucheck::kLdsVectors), dump(gpucheck::kLdsVectors);
  std::vector<uint32_t> readers(gpucheck::kLdsVectors);
  for (long g = 0; g < groups; ++g) {
    const uint32_t group = static_cast<uint32_t>(g);
    LdsRecord rec = {0, kNoBad, {0, 0, 0, 0}};
    for (uint32_t round = 0; round < o.lds_rounds; ++round) {
      const uint64_t key = gpucheck::lds_key(o.seed, group, round);
      for (uint32_t pass = 0; pass < 2; ++pass) {
        for (uint32_t t = 0; t < kBlock; ++t)
          for (int j = 0; j < trips; ++j)
            lds[t + kBlock * j] = pattern_vec(key, pass, t + kBlock * j);
        for (uint32_t k = 0; k < inj.n; ++k)
          if (inj.at[k].group == group && inj.at[k].round == round &&
              inj.at[k].pass == pass)
            lds[inj.at[k].dword >> 2][inj.at[k].dword & 3] ^= inj.at[k].mask;
        const bool dumping = o.dump_lds && group == o.dump_lds_group &&
                             round == o.dump_lds_round && pass == o.dump_lds_pass;
        for (uint32_t t = 0; t < kBlock; ++t)
          for (int j = 0; j < trips; ++j) {
            const uint32_t i = ((t + 64) & (kBlock - 1)) + kBlock * j;
            const u32x4 got = lds[i];
            const u32x4 want = pattern_vec(key, pass, i);
            if (got.x != want.x || got.y != want.y || got.z != want.z ||
                got.w != want.w) {
              ++rec.bad;
              const unsigned long long packed = lds_pack(round, pass, i);
              if (packed < rec.first) {
                rec.first = packed;
                rec.first_xor = got ^ want;
              }
            }
            if (dumping) {
              dump[i] = got;
              readers[i] = t;
            }
          }
        if (dumping)
          record_lds_dump(reinterpret_cast<const unsigned char*>(dump.data()),
                          readers.data(), rep);
      }
    }
    records[g] = rec;
    for (uint32_t w = 0; w < 4; ++w) {
      where[2 * (4 * g + w)] = group % 5;
      where[2 * (4 * g + w) + 1] = w;
    }
  }
  rep->lds_where = where;
  judge_lds(records, where, rep);
}

// Launches `groups` workgroups, again with fresh rounds while compute units
// remain unseen and launches remain: a workgroup holds a whole LDS, so two
// never share a compute unit, and which compute units the dispatcher picked
// is known only from the CU keys that come back.
void run_lds(const Options& o, long groups, const hipDeviceProp_t& prop,
             Report* rep) {
  rep->lds_groups = groups;
  hipFuncAttributes attr;
  HIP_CHECK(hipFuncGetAttributes(&attr,
                                 reinterpret_cast<const void*>(lds_selftest)));
  if (prop.sharedMemPerBlock < static_cast<size_t>(gpucheck::kLdsBytes) ||
      attr.sharedSizeBytes != static_cast<size_t>(gpucheck::kLdsBytes)) {
    rep->lds_skip_reason =
        "needs 163840 bytes of LDS per workgroup: the device offers " +
        std::to_string(prop.sharedMemPerBlock) + ", the kernel uses " +
        std::to_string(attr.sharedSizeBytes);
    return;
  }
  const size_t n = static_cast<size_t>(groups);
  LdsRecord* records = nullptr;
  u32x4* dump = nullptr;
  HIP_CHECK(hipMalloc(&records, n * sizeof(LdsRecord)));
  if (o.dump_lds) {
    HIP_CHECK(hipMalloc(&dump, kLdsDumpBytes));
    HIP_CHECK(hipMemset(dump, 0xFF, kLdsDumpBytes));
  }
  WhereBuffer where(4 * n);
  GpuTimer timer;
  timer.init();
  const LdsInjections inj = lds_injections(o);
  const std::vector<LdsRecord> clean(n, LdsRecord{0, kNoBad, {0, 0, 0, 0}});
  std::vector<LdsRecord> host(n);
  double seconds = 0;
  for (uint32_t launch = 0; launch < o.lds_max_launches; ++launch) {
    HIP_CHECK(hipMemcpy(records, clean.data(), n * sizeof(LdsRecord),
                        hipMemcpyHostToDevice));
    timer.begin();
    // Injections and the dump name rounds of the first launch.
    hipLaunchKernelGGL(lds_selftest, dim3(static_cast<unsigned int>(n)),
                       dim3(kBlock), 0, 0, records, where.dev, o.seed,
                       launch * o.lds_rounds, o.lds_rounds, inj,
                       launch == 0 ? dump : nullptr, o.dump_lds_group,
                       o.dump_lds_round, o.dump_lds_pass);
    seconds = timer.end();
    HIP_CHECK(hipMemcpy(host.data(), records, n * sizeof(LdsRecord),
                        hipMemcpyDeviceToHost));
    const std::vector<uint32_t> ran = where.fetch();
    if (launch == 0) rep->lds_where = ran;
    ++rep->lds_launches;
    judge_lds(host, ran, rep);
    if (rep->lds_cus.size() >= static_cast<size_t>(prop.multiProcessorCount))
      break;
  }
  rep->lds_gbs = gbs(2.0 * 2.0 * gpucheck::kLdsBytes * o.lds_rounds *
                         static_cast<double>(n), seconds);
  if (o.dump_lds) {
    std::vector<uint32_t> words(kLdsDumpBytes / sizeof(uint32_t));
    HIP_CHECK(hipMemcpy(words.data(), dump, kLdsDumpBytes, hipMemcpyDeviceToHost));
    record_lds_dump(reinterpret_cast<const unsigned char*>(words.data()),
                    words.data() + gpucheck::kLdsBytes / sizeof(uint32_t), rep);
    HIP_CHECK(hipFree(dump));
  }
  HIP_CHECK(hipFree(records));
}

// ------------------------------------------------------------------- JSON

std::string json_escape(const std::string& s) {
  std::string out;
  for (char c : s) {
    if (c == '"' || c == '\\') {
      out += '\\';
      out += c;
    } else if (static_cast<unsigned char>(c) < 0x20) {
      out += ' ';
    } else {
      out += c;
    }
  }
  return out;
}

constexpr size_t kMaxLdsBadCus = 8;

// Every compute unit's LDS was visited. Under --cpu there are no compute
// units, so a stage that ran is complete.
bool lds_coverage_full(const Report& r) {
  return strcmp(r.lds, "skipped") != 0 &&
         r.lds_cus.size() >= static_cast<size_t>(r.compute_units);
}

// Exit 27: an untested compute unit is a failure only on request, and never
// under --cpu, which has no compute units.
bool lds_coverage_required_and_partial(const Options& o, const Report& r) {
  return o.lds_require_coverage && !o.cpu && !lds_coverage_full(r);
}

// "name":[[[key,simd] x per_group] per group], (flat pairs when per_group
// is 1)
void print_where_list(const char* name, const std::vector<uint32_t>& where,
                      size_t per_group) {
  printf("\"%s\":[", name);
  const size_t waves = where.size() / 2;
  for (size_t w = 0; w < waves; ++w) {
    if (per_group > 1 && w % per_group == 0) printf("%s[", w ? "," : "");
    printf("%s[%u,%u]", (per_group > 1 ? w % per_group : w) ? "," : "",
           where[2 * w], where[2 * w + 1]);
    if (per_group > 1 && w % per_group == per_group - 1) printf("]");
  }
  printf("],");
}

// "X_cus_covered":n,"X_simds_covered":n,
void print_covered(const Family& fam, const Report::TileResult& t) {
  size_t cus = 0, simds = 0;
  count_where(t.where, &cus, &simds);
  printf("\"%s_cus_covered\":%zu,\"%s_simds_covered\":%zu,", fam.prefix, cus,
         fam.prefix, simds);
}

// Where the first bad wave of format `f` ran, "" without one.
std::string first_bad_where(const Report::TileResult& t, int f) {
  const long w = t.formats[f].first_bad_wave;
  return w < 0 ? "" : where_of(t.where, f * t.waves + w);
}

// "X_formats":{"name":{...},...},
void print_formats(const Family& fam, const Report::TileResult& t,
                   bool launch_ms) {
  printf("\"%s_formats\":{", fam.prefix);
  for (int f = 0; f < fam.formats; ++f) {
    const Report::TileResult::Format& fr = t.formats[f];
    printf("%s\"%s\":{\"bad_waves\":%ld,\"first_bad_wave\":%ld,"
           "\"first_bad_where\":\"%s\",\"tflops\":%.3f",
           f ? "," : "", fam.names[f], fr.bad_waves, fr.first_bad_wave,
           first_bad_where(t, f).c_str(), fr.tflops);
    if (launch_ms) printf(",\"launch_ms\":%.4f", fr.launch_ms);
    printf("}");
  }
  printf("},");
}

bool all_integers(const std::vector<long long>& dump) {
  return std::find(dump.begin(), dump.end(), kNotAnInteger) == dump.end();
}

// [v,v,...], null for a value that is no integer within the family's bound
void print_tile_values(const std::vector<long long>& dump) {
  printf("[");
  for (size_t i = 0; i < dump.size(); ++i)
    if (dump[i] == kNotAnInteger)
      printf("%snull", i ? "," : "");
    else
      printf("%s%lld", i ? "," : "", dump[i]);
  printf("]");
}

void print_report(const Options& o, const Report& r, int code, double wall_s) {
  const bool hbm_fail = r.mismatch_vectors != 0;
  const Report::TileResult& mfma = r.tile[kMfma];
  const Report::TileResult& mx = r.tile[kMx];
  const Report::TileResult& dense = r.tile[kDense];
  std::string failed;
  auto add_failed = [&](const char* name) {
    failed += failed.empty() ? "\"" : ",\"";
    failed += name;
    failed += "\"";
  };
  if (hbm_fail) add_failed("hbm");
  if (!strcmp(r.copy, "fail")) add_failed("copy");
  if (!strcmp(mfma.verdict, "fail")) add_failed("mfma");
  if (!strcmp(mx.verdict, "fail")) add_failed("mx");
  if (!strcmp(r.lds, "fail")) add_failed("lds");
  if (!strcmp(dense.verdict, "fail")) add_failed("dense");
  if (!strcmp(r.bandwidth, "fail")) add_failed("bandwidth");
  if (!strcmp(mx.rate, "fail")) add_failed("mx_rate");
  if (!strcmp(dense.rate, "fail")) add_failed("dense_rate");
  if (lds_coverage_required_and_partial(o, r)) add_failed("lds_coverage");

  printf("{\"tool\":\"gpucheck\",\"mode\":\"%s\",\"device\":\"%s\","
         "\"compute_units\":%d,\"ok\":%s,\"exit_code\":%d,"
         "\"failed_stages\":[%s],",
         o.cpu ? "cpu" : "gpu", json_escape(r.device).c_str(), r.compute_units,
         code == 0 ? "true" : "false", code, failed.c_str());
  printf("\"bytes\":%zu,\"vectors\":%zu,\"passes\":%u,\"base_index\":%llu,"
         "\"seed\":%llu,",
         o.bytes, o.bytes / 16, o.passes,
         static_cast<unsigned long long>(o.base_index),
         static_cast<unsigned long long>(o.seed));
  printf("\"hbm\":\"%s\",\"mismatch_vectors\":%llu,", hbm_fail ? "fail" : "pass",
         static_cast<unsigned long long>(r.mismatch_vectors));
  if (r.have_first_bad)
    printf("\"first_bad_offset\":%llu,\"first_bad_pass\":%u,"
           "\"first_bad_xor\":\"%s\",",
           static_cast<unsigned long long>(r.first_bad_offset), r.first_bad_pass,
           hex128(r.first_bad_xor).c_str());
  else
    printf("\"first_bad_offset\":null,\"first_bad_pass\":null,"
           "\"first_bad_xor\":null,");
  printf("\"write_gbs\":%.3f,\"read_gbs\":%.3f,\"write_gbs_plain\":%.3f,"
         "\"write_gbs_nontemporal\":%.3f,\"store_variant\":\"%s\",",
         r.write_gbs, r.read_gbs, r.write_gbs_plain, r.write_gbs_nontemporal,
         r.store_variant);
  printf("\"bandwidth\":\"%s\",\"copy_gbs\":%.3f,\"min_copy_gbs\":%.3f,"
         "\"cache_resident\":%s,",
         r.bandwidth, r.copy_gbs, o.min_copy_gbs,
         o.bytes < kCacheResidentBelow ? "true" : "false");
  printf("\"copy\":\"%s\",\"copy_mismatch_vectors\":%llu,", r.copy,
         static_cast<unsigned long long>(r.copy_mismatch_vectors));
  if (r.have_copy_first_bad)
    printf("\"copy_first_bad_offset\":%llu,\"copy_first_bad_xor\":\"%s\",",
           static_cast<unsigned long long>(r.copy_first_bad_offset),
           hex128(r.copy_first_bad_xor).c_str());
  else
    printf("\"copy_first_bad_offset\":null,\"copy_first_bad_xor\":null,");
  printf("\"mfma\":\"%s\",\"mfma_waves\":%ld,\"mfma_bad_waves\":%ld,"
         "\"mfma_first_bad_wave\":%ld,",
         mfma.verdict, mfma.waves, mfma.formats[0].bad_waves,
         mfma.formats[0].first_bad_wave);
  if (o.dump_pattern) {
    printf("\"pattern_dump\":[");
    for (size_t i = 0; i < r.pattern_dump.size(); ++i)
      printf("%s\"%s\"", i ? "," : "", r.pattern_dump[i].c_str());
    printf("],");
  }
  if (!o.dump_vectors.empty()) {
    printf("\"vector_dump\":[");
    for (size_t i = 0; i < r.vector_dump.size(); ++i)
      printf("%s{\"index\":%zu,\"pass\":%u,\"value\":\"%s\"}", i ? "," : "",
             r.vector_dump[i].index, r.vector_dump[i].pass,
             r.vector_dump[i].value.c_str());
    printf("],");
  }
  const TileOptions& mfma_o = o.tile[kMfma];
  const TileOptions& mx_o = o.tile[kMx];
  const TileOptions& dense_o = o.tile[kDense];
  // A value that is no integer: MFMA and MX print no tile, dense prints null
  // in its place.
  if (mfma_o.dump_wave >= 0) {
    if (all_integers(mfma.dump)) {
      printf("\"mfma_tile\":{\"wave\":%ld,\"values\":", mfma_o.dump_wave);
      print_tile_values(mfma.dump);
      printf("},");
    } else {
      printf("\"mfma_tile\":null,");
    }
  }
  printf("\"mx\":\"%s\",\"mx_waves\":%ld,\"mx_rate\":\"%s\",", mx.verdict,
         mx.waves, mx.rate);
  print_formats(kFamilyTable[kMx], mx, false);
  if (mx_o.dump_wave >= 0) {
    if (all_integers(mx.dump)) {
      printf("\"mx_tile\":{\"format\":\"%s\",\"wave\":%ld,\"values_x16\":",
             kFamilyTable[kMx].names[mx_o.dump_format], mx_o.dump_wave);
      print_tile_values(mx.dump);
      printf("},");
    } else {
      printf("\"mx_tile\":null,");
    }
  }
  print_covered(kFamilyTable[kMfma], mfma);
  printf("\"mfma_first_bad_where\":\"%s\",", first_bad_where(mfma, 0).c_str());
  print_covered(kFamilyTable[kMx], mx);
  printf("\"clock_mhz\":%d,\"mx_s\":%.4f,\"dense_s\":%.4f,", r.clock_mhz,
         mx.seconds, dense.seconds);
  printf("\"dense\":\"%s\",\"dense_waves\":%ld,\"dense_rate\":\"%s\",",
         dense.verdict, dense.waves, dense.rate);
  print_covered(kFamilyTable[kDense], dense);
  printf("\"dense_rate_instr\":%llu,",
         static_cast<unsigned long long>(dense_o.rate_instr));
  print_formats(kFamilyTable[kDense], dense, true);
  if (dense_o.dump_wave >= 0) {
    const gpucheck::DenseFormat& fmt =
        gpucheck::kDenseFormatTable[dense_o.dump_format];
    printf("\"dense_tile\":{\"format\":\"%s\",\"wave\":%ld,\"rows\":%d,"
           "\"cols\":%d,\"scale\":%d,\"values\":",
           fmt.name, dense_o.dump_wave, fmt.mn, fmt.mn, fmt.scale);
    print_tile_values(dense.dump);
    printf("},");
  }
  printf("\"lds\":\"%s\",", r.lds);
  if (!r.lds_skip_reason.empty())
    printf("\"lds_skipped_reason\":\"%s\",",
           json_escape(r.lds_skip_reason).c_str());
  printf("\"lds_groups\":%ld,\"lds_rounds\":%u,\"lds_launches\":%ld,"
         "\"lds_bytes_per_cu\":%d,\"lds_cus_covered\":%zu,"
         "\"lds_coverage\":\"%s\",\"lds_bad_groups\":%ld,\"lds_bad_cus\":[",
         r.lds_groups, o.lds_rounds, r.lds_launches, gpucheck::kLdsBytes,
         r.lds_cus.size(), lds_coverage_full(r) ? "full" : "partial",
         r.lds_bad_groups);
  size_t listed = 0;
  for (const auto& kv : r.lds_bad_cus) {
    if (listed == kMaxLdsBadCus) break;
    const Report::LdsBadCu& cu = kv.second;
    printf("%s{\"where\":\"%s\",\"key\":%u,\"bad_vectors\":%llu,"
           "\"first_bad_offset\":%llu,\"first_bad_xor\":\"%s\","
           "\"round\":%llu,\"pass\":%llu}",
           listed++ ? "," : "", where_name(kv.first).c_str(), kv.first,
           static_cast<unsigned long long>(cu.bad_vectors),
           16 * (cu.first & 0x3FFF), hex128(cu.first_xor).c_str(),
           cu.first >> 15, (cu.first >> 14) & 1);
  }
  printf("],\"lds_gbs\":%.3f,", r.lds_gbs);
  if (o.dump_lds) {
    if (r.lds_dump_valid) {
      printf("\"lds_dump\":{\"group\":%u,\"round\":%u,\"pass\":%u,"
             "\"fnv64\":\"%016llx\",\"same_wave_reads\":%ld,\"vectors\":{",
             o.dump_lds_group, o.dump_lds_round, o.dump_lds_pass,
             static_cast<unsigned long long>(r.lds_dump_fnv64),
             r.lds_dump_same_wave_reads);
      for (size_t i = 0; i < r.lds_dump_vectors.size(); ++i)
        printf("%s\"%d\":\"%s\"", i ? "," : "", kLdsDumpVectors[i],
               r.lds_dump_vectors[i].c_str());
      printf("}},");
    } else {
      printf("\"lds_dump\":null,");
    }
  }
  if (o.dump_lds_where) {
    print_where_list("lds_where", r.lds_where, 4);
    print_where_list("mfma_where", mfma.where, 1);
  }
  printf("\"wall_s\":%.4f}\n", wall_s);
  fflush(stdout);
}

// How many waves a family runs on a device of `compute_units`. Under --cpu a
// family runs only with an explicit --X-waves.
long tile_waves(const Options& o, int fam, int compute_units) {
  const long asked = o.tile[fam].waves;
  if (asked >= 0 || o.cpu) return std::max(asked, 0L);
  long waves = static_cast<long>(kFamilyTable[fam].waves_per_cu) * compute_units;
  // An explicit --mfma-waves caps the default, so a small run stays small.
  if (o.tile[kMfma].waves > 0) waves = std::min(waves, o.tile[kMfma].waves);
  return waves;
}

}  // namespace

int main(int argc, char** argv) {
  const auto t0 = std::chrono::steady_clock::now();
  Options o;
  if (int rc = parse_args(argc, argv, &o)) return rc;

  Report rep;
  try {
    hipDeviceProp_t prop = {};
    if (!o.cpu) {
      int count = 0;
      HIP_CHECK(hipGetDeviceCount(&count));
      if (count < 1) throw HipError{"no visible GPU"};
      HIP_CHECK(hipSetDevice(0));
      HIP_CHECK(hipGetDeviceProperties(&prop, 0));
      rep.device = std::string(prop.name) + " " + prop.gcnArchName;
      rep.compute_units = prop.multiProcessorCount;
      rep.clock_mhz = prop.clockRate / 1000;  // reported in kHz
    }
    long waves[kFamilies];
    for (int fam = 0; fam < kFamilies; ++fam)
      waves[fam] = tile_waves(o, fam, rep.compute_units);
    const long lds_groups = o.lds_groups >= 0 || o.cpu
                                ? std::max(o.lds_groups, 0L)
                                : 2L * rep.compute_units;
    auto check_tiles = [&](int fam) {
      return check_tile_args(kFamilyTable[fam], o.tile[fam], waves[fam]);
    };
    if (int rc = check_tiles(kMfma)) return rc;
    if (int rc = check_tiles(kMx)) return rc;
    if (int rc = check_lds_args(o, lds_groups)) return rc;
    if (int rc = check_tiles(kDense)) return rc;
    if (o.cpu) {
      CpuBackend be(o);
      if (be.mem == nullptr) {
        fprintf(stderr, "gpucheck: cannot allocate %zu bytes\n", o.bytes);
        return 2;
      }
      run_hbm(be, o, &rep);
      auto run_tiles_on_host = [&](int fam) {
        if (waves[fam] > 0)
          run_tiles_cpu(kFamilyTable[fam], waves[fam], o.tile[fam], o.seed,
                        &rep.tile[fam]);
      };
      run_tiles_on_host(kMfma);
      run_tiles_on_host(kMx);
      if (lds_groups > 0) run_lds_cpu(o, lds_groups, &rep);
      run_tiles_on_host(kDense);
    } else {
      {
        GpuBackend be(o);
        run_hbm(be, o, &rep);
        run_copy(be, o, &rep);
      }
      const int cus = rep.compute_units;
      run_tiles<MfmaKernels>(o, waves[kMfma], cus, &rep);
      if (waves[kMx] > 0) run_tiles<MxKernels>(o, waves[kMx], cus, &rep);
      if (lds_groups > 0) run_lds(o, lds_groups, prop, &rep);
      if (waves[kDense] > 0) run_tiles<DenseKernels>(o, waves[kDense], cus, &rep);
    }
  } catch (const HipError& e) {
    fprintf(stderr, "gpucheck: %s\n", e.what.c_str());
    printf("{\"tool\":\"gpucheck\",\"ok\":false,\"exit_code\":11,"
           "\"failed_stages\":[\"hip\"],\"error\":\"%s\"}\n",
           json_escape(e.what).c_str());
    fflush(stdout);
    return 11;
  }

  int code = 0;
  if (rep.mismatch_vectors != 0) code = 20;
  else if (!strcmp(rep.copy, "fail")) code = 23;
  else if (!strcmp(rep.tile[kMfma].verdict, "fail")) code = 21;
  else if (!strcmp(rep.tile[kMx].verdict, "fail")) code = 24;
  else if (!strcmp(rep.lds, "fail")) code = 26;
  else if (!strcmp(rep.tile[kDense].verdict, "fail")) code = 28;
  else if (!strcmp(rep.bandwidth, "fail")) code = 22;
  else if (!strcmp(rep.tile[kMx].rate, "fail")) code = 25;
  else if (!strcmp(rep.tile[kDense].rate, "fail")) code = 29;
  else if (lds_coverage_required_and_partial(o, rep)) code = 27;
  const double wall_s =
      std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  print_report(o, rep, code, wall_s);
  return code;
}
