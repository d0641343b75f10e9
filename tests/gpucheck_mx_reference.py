"""An independent reference for gpucheck's MX stage: the block-scaled
FP8/BF8/FP4 operands, their E8M0 scales and the 32 x 32 x 256 product.

Nothing here is translated from ``gpucheck_pattern.h`` or from the decoders
in ``gpucheck.hip``. The decoders are written from the OCP formulas (OCP 8-bit
Floating Point Specification, OCP Microscaling Formats Specification); the
encodings are found by searching the decoder for the wanted value, not by
bit arithmetic; the product is one float64 numpy matmul. The injection cases
that the CPU and the GPU tests share are at the end."""

import functools
import math

import numpy as np

from tests.gpucheck_reference import DEFAULT_SEED, MASK64, mix64  # noqa: F401

MX_M = 32
MX_N = 32
MX_K = 256
MX_BLOCK = 32

# name -> (element type of A, element type of B), in the binary's order
FORMATS = {
    "fp8": ("e4m3", "e4m3"),
    "bf8": ("e5m2", "e5m2"),
    "fp4": ("e2m1", "e2m1"),
    "fp8xfp4": ("e4m3", "e2m1"),
}
FORMAT_NAMES = list(FORMATS)


# ------------------------------------------------------------- decoders

def _decode(code, exp_bits, mant_bits, bias):
    """(-1)^S 2^(E-bias) (1 + M/2^m) for E > 0, (-1)^S 2^(1-bias) M/2^m for
    E = 0."""
    mant = code & ((1 << mant_bits) - 1)
    exp = (code >> mant_bits) & ((1 << exp_bits) - 1)
    sign = -1.0 if (code >> (exp_bits + mant_bits)) & 1 else 1.0
    if exp == 0:
        return sign * 2.0 ** (1 - bias) * mant / 2 ** mant_bits
    return sign * 2.0 ** (exp - bias) * (1 + mant / 2 ** mant_bits)


def decode_e2m1(code):
    assert 0 <= code < 16
    return _decode(code, 2, 1, 1)


def decode_e4m3fn(code):
    """No infinities; S.1111.111 is NaN."""
    assert 0 <= code < 256
    if code & 0x7F == 0x7F:
        return math.nan
    return _decode(code, 4, 3, 7)


def decode_e5m2(code):
    """Exponent field 31: infinity (mantissa 0) or NaN."""
    assert 0 <= code < 256
    if (code >> 2) & 31 == 31:
        if code & 3:
            return math.nan
        return -math.inf if code & 0x80 else math.inf
    return _decode(code, 5, 2, 15)


def decode_e8m0(code):
    assert 0 <= code < 256
    return math.nan if code == 255 else 2.0 ** (code - 127)


DECODERS = {"e2m1": decode_e2m1, "e4m3": decode_e4m3fn, "e5m2": decode_e5m2}


@functools.lru_cache(maxsize=None)
def _encode(elem_type, negative, magnitude):
    """The code whose decoded value has this sign bit and magnitude, found by
    search over the decoder."""
    decode = DECODERS[elem_type]
    ncodes = 16 if elem_type == "e2m1" else 256
    hits = [c for c in range(ncodes)
            if decode(c) == (-magnitude if negative else magnitude)
            and (math.copysign(1.0, decode(c)) < 0) == bool(negative)]
    assert len(hits) == 1, (elem_type, negative, magnitude, hits)
    return hits[0]


# ----------------------------------------------------------- generators

def mx_key(seed, wave, fmt_index, which):
    return mix64(seed ^ mix64((1 << 40) | (wave << 3) | (fmt_index << 1)
                              | which))


def _code(elem_type, h):
    """e2m1: any of the 16 codes. e4m3: +-m/2 for m = 0..15. e5m2: +-m/2 for
    m = 0..7. The sign is hash bit 4."""
    if elem_type == "e2m1":
        return h & 15
    m = h & (15 if elem_type == "e4m3" else 7)
    return _encode(elem_type, (h >> 4) & 1, m / 2)


def a_code(elem_type, key_a, row, k):
    """A is 32 x 256, row-major."""
    return _code(elem_type, mix64((key_a + row * MX_K + k) & MASK64))


def b_code(elem_type, key_b, k, col):
    """B is 256 x 32, row-major."""
    return _code(elem_type, mix64((key_b + k * MX_N + col) & MASK64))


def scale_byte(key, rc, block):
    return 126 + mix64((key + 0x10000 + rc * (MX_K // MX_BLOCK) + block)
                       & MASK64) % 3


def operands(fmt, seed, wave):
    """(A, B) as float64 with the block scales applied."""
    type_a, type_b = FORMATS[fmt]
    fi = FORMAT_NAMES.index(fmt)
    key_a = mx_key(seed, wave, fi, 0)
    key_b = mx_key(seed, wave, fi, 1)
    a = np.array([[decode_e8m0(scale_byte(key_a, r, k // MX_BLOCK))
                   * DECODERS[type_a](a_code(type_a, key_a, r, k))
                   for k in range(MX_K)] for r in range(MX_M)])
    b = np.array([[decode_e8m0(scale_byte(key_b, c, k // MX_BLOCK))
                   * DECODERS[type_b](b_code(type_b, key_b, k, c))
                   for c in range(MX_N)] for k in range(MX_K)])
    return a, b


_tiles = {}


def mx_tile(fmt, seed, wave):
    """The 32 x 32 tile wave ``wave`` must produce in ``fmt``, times 16, as
    numpy.int64. Computed once per (fmt, seed, wave); do not modify."""
    key = (fmt, seed, wave)
    if key not in _tiles:
        a, b = operands(fmt, seed, wave)
        # The exactness bound, on these very operands: every scaled product
        # is a multiple of 2**-4 and the magnitudes of one output's products
        # sum to less than 2**24 of those units, so any summation order in
        # float32 (and this one in float64) is exact.
        assert (a * 4 == np.round(a * 4)).all()
        assert (b * 4 == np.round(b * 4)).all()
        assert (np.abs(a) @ np.abs(b)).max() * 16 < 2 ** 24
        x16 = (a @ b) * 16
        tile = x16.astype(np.int64)
        assert (tile == x16).all()
        tile.setflags(write=False)
        _tiles[key] = tile
    return _tiles[key]


# ---------------------------------------------------------------- cases
# --inject-mx values (without the format) in the order given, bad waves,
# first bad wave; for a run of 5 waves.
MX_INJECT_CASES = [
    (["0:0"], 1, 0),             # one element
    (["2:31", "2:32"], 1, 2),    # two in one wave
    (["3:5", "1:700"], 2, 1),    # two waves
    (["4:1023"], 1, 4),          # last element of the last wave
]


def mx_inject_args(fmt, injections):
    return [a for inj in injections for a in ("--inject-mx", f"{fmt}:{inj}")]


def expect_formats(out, failing=None, bad=0, first=-1):
    """``failing`` has the given counts; every other format is clean."""
    assert list(out["mx_formats"]) == FORMAT_NAMES
    for name, got in out["mx_formats"].items():
        if name == failing:
            assert got["bad_waves"] == bad and got["first_bad_wave"] == first
        else:
            assert got["bad_waves"] == 0 and got["first_bad_wave"] == -1
