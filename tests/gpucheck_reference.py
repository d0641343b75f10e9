"""An independent reference for what gpucheck computes: the 16-byte HBM
pattern and the MFMA self-test's operands and product.

Written with Python integers masked to 64 bits and one numpy int64 matmul. It
includes nothing from ``gpucheck_pattern.h``, so a test that compares the
binary's output with this module checks the header and the kernels against a
second implementation, not against themselves. The injection cases that
the CPU and the GPU tests share are at the end."""

import numpy as np

MASK64 = (1 << 64) - 1
DEFAULT_SEED = 0x6770756368656B31

MFMA_M = 32
MFMA_N = 32
MFMA_K = 128


def mix64(x):
    """The splitmix64 finalizer."""
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def pattern_int(seed, pass_, index):
    """The 128-bit value stored at logical vector ``index`` in pass
    ``pass_``: an odd pass is the complement of the even pass before it."""
    index &= MASK64
    key = mix64((seed ^ ((pass_ & ~1 & 0xFFFFFFFF) << 32)) & MASK64)
    lo = mix64(index ^ key)
    hi = mix64((lo + index) & MASK64)
    if pass_ & 1:
        lo ^= MASK64
        hi ^= MASK64
    return (hi << 64) | lo


def pattern(seed, pass_, index):
    """As the binary prints it: 32 hex digits, high half first."""
    return f"{pattern_int(seed, pass_, index):032x}"


def mfma_key(seed, wave, which):
    return mix64(seed ^ mix64(((wave << 1) | which) & MASK64))


def _mfma_value(key, elem):
    return mix64((key + elem) & MASK64) % 7 - 3


def mfma_a(key_a, row, k):
    """A is 32 x 128, row-major."""
    return _mfma_value(key_a, row * MFMA_K + k)


def mfma_b(key_b, k, col):
    """B is 128 x 32, row-major."""
    return _mfma_value(key_b, k * MFMA_N + col)


def mfma_tile(seed, wave):
    """The 32 x 32 product wave ``wave`` must produce, as numpy.int64."""
    key_a = mfma_key(seed, wave, 0)
    key_b = mfma_key(seed, wave, 1)
    a = np.array([[mfma_a(key_a, r, k) for k in range(MFMA_K)]
                  for r in range(MFMA_M)], dtype=np.int64)
    b = np.array([[mfma_b(key_b, k, c) for c in range(MFMA_N)]
                  for k in range(MFMA_K)], dtype=np.int64)
    return a @ b


# ---------------------------------------------------------------- cases
# Injection cases that the --cpu tests and the GPU tests both run, so the
# host loops and the kernels are held to the same answers.

GRID = 2048 * 256  # vectors in one trip of a full grid of hbm_verify

# More than one bad vector: hbm_verify folds the count and the minimum over
# a wave and does one atomic pair per wave. (offset, bit) lists; the vector
# is offset // 16.
MULTI_FLIP_REGION = 16 * (GRID + 300)
MULTI_FLIP_CASES = {
    # lanes 3 and 40 of wave 0
    "two-lanes-one-wave": [(16 * 3, 0), (16 * 40 + 5, 2)],
    # waves 1 and 3 of workgroup 0
    "two-waves-one-workgroup": [(16 * 70 + 1, 1), (16 * 200 + 15, 7)],
    # trip 2 of workgroup 0, and the lower vector in the last workgroup of
    # trip 1: the minimum must not depend on who reaches the atomic first
    "later-trip-listed-first": [(16 * (GRID + 5), 3),
                                (16 * (256 * 2047 + 9) + 7, 6)],
    # descending offsets over both trips, two flips in the lowest vector
    "seven-descending": [
        (16 * (GRID + 299) + 15, 7), (16 * (GRID + 64) + 3, 1),
        (16 * (GRID - 1), 0), (16 * 70000 + 8, 4), (16 * 4097 + 9, 6),
        (16 * 257 + 12, 5), (16 * 257 + 1, 3)],
}


def flip_args(flips):
    return [a for off, bit in flips for a in ("--inject-flip", f"{off}:{bit}")]


def expect_flips(out, flips, pass_=0):
    """Each flipped vector counted once, the lowest located, and exactly the
    bits flipped in it reported."""
    by_vector = {}
    for off, bit in flips:
        by_vector[off // 16] = by_vector.get(off // 16, 0) ^ (
            1 << (8 * (off % 16) + bit))
    first = min(by_vector)
    assert out["failed_stages"][0] == "hbm" and out["hbm"] == "fail"
    assert out["mismatch_vectors"] == len(by_vector)
    assert out["first_bad_offset"] == 16 * first
    assert out["first_bad_pass"] == pass_
    assert int(out["first_bad_xor"], 16) == by_vector[first]


# --inject-mfma values in the order given, bad waves, first bad wave; for a
# run of 5 waves.
MFMA_INJECT_CASES = [
    (["0:0"], 1, 0),
    (["4:1023"], 1, 4),          # last element of the last wave
    (["3:5", "1:700"], 2, 1),
    (["2:31", "2:32"], 1, 2),    # two in one wave
]


def mfma_inject_args(injections):
    return [a for inj in injections for a in ("--inject-mfma", inj)]
