"""An independent reference for gpucheck's dense stage: the key, the hashed
operands of the seven formats and the tile each wave must produce.

It knows nothing of lanes, registers or k-steps: ``dense_tile`` is a plain
integer matrix product in numpy int64 over A [M][K] and B [K][N], both
row-major. The fp8 and bf8 elements are found by searching the MX
reference's OCP decoders for the wanted value and are held times 2, so their
tile is in quarter-units (``scale`` 4). The injection cases that the CPU and
the GPU tests share are at the end."""

import numpy as np

from tests.gpucheck_mx_reference import DECODERS, _encode
from tests.gpucheck_reference import DEFAULT_SEED, MASK64, mix64  # noqa: F401

# name -> (tile side, K, scale, bound on sum |a.b| times scale), in the
# binary's order. The bounds are the ones gpucheck_pattern.h states.
FORMATS = {
    "f16": (32, 128, 1, 128 * 225),
    "bf16x16": (16, 128, 1, 128 * 225),
    "fp8": (32, 128, 4, 28800),
    "bf8": (32, 128, 4, 28800),
    "i8": (32, 128, 1, 2 ** 21),
    "f32": (32, 32, 1, 8355872),
    "f64": (16, 32, 1, 2 ** 45),
}
FORMAT_NAMES = list(FORMATS)
# What the accumulator holds exactly: integers below this magnitude.
EXACT_BELOW = {"f16": 2 ** 24, "bf16x16": 2 ** 24, "fp8": 2 ** 24,
               "bf8": 2 ** 24, "i8": 2 ** 31, "f32": 2 ** 24, "f64": 2 ** 53}


def dense_key(seed, wave, fmt_index, which):
    return mix64(seed ^ mix64((1 << 42) | (wave << 4) | (fmt_index << 1)
                              | which))


def value(fmt, h):
    """The element with hash ``h``, times the square root of the scale (2
    for fp8 and bf8, 1 otherwise), as a Python int."""
    if fmt in ("f16", "bf16x16"):
        return h % 31 - 15
    if fmt == "i8":
        code = h & 0xFF
        return code - 256 if code >= 128 else code
    if fmt == "f32":
        return h % 1023 - 511
    if fmt == "f64":
        return h % (2 ** 21 - 1) - (2 ** 20 - 1)
    # +-m/2, m <= 15 (e4m3) or m <= 7 (e5m2), sign in hash bit 4: encoded by
    # search over the OCP decoder and decoded again, as the device would.
    elem_type = "e4m3" if fmt == "fp8" else "e5m2"
    m = h & (15 if fmt == "fp8" else 7)
    doubled = 2 * DECODERS[elem_type](_encode(elem_type, (h >> 4) & 1, m / 2))
    assert doubled == int(doubled)
    return int(doubled)


def mix64_array(x):
    """``mix64`` over a numpy.uint64 array (its arithmetic wraps mod 2^64);
    the tests hold it against the scalar one."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def values(fmt, h):
    """``value`` over a numpy.uint64 array of hashes, as numpy.int64."""
    if fmt in ("f16", "bf16x16"):
        return (h % np.uint64(31)).astype(np.int64) - 15
    if fmt == "i8":
        return (h & np.uint64(0xFF)).astype(np.uint8).view(np.int8) \
            .astype(np.int64)
    if fmt == "f32":
        return (h % np.uint64(1023)).astype(np.int64) - 511
    if fmt == "f64":
        return (h % np.uint64(2 ** 21 - 1)).astype(np.int64) - (2 ** 20 - 1)
    # only hash bits 0..4 matter: one decoded element per 5-bit pattern
    table = np.array([value(fmt, low) for low in range(32)], dtype=np.int64)
    return table[(h & np.uint64(31)).astype(np.int64)]


def operands(fmt, seed, wave):
    """(A, B) as numpy.int64, times the square root of the scale: A[r][k]
    hashes element r K + k of its key, B[k][c] element k N + c."""
    mn, k_total, _, _ = FORMATS[fmt]
    fi = FORMAT_NAMES.index(fmt)
    index = np.arange(mn * k_total, dtype=np.uint64)
    with np.errstate(over="ignore"):
        hash_a = mix64_array(np.uint64(dense_key(seed, wave, fi, 0)) + index)
        hash_b = mix64_array(np.uint64(dense_key(seed, wave, fi, 1)) + index)
    return (values(fmt, hash_a).reshape(mn, k_total),
            values(fmt, hash_b).reshape(k_total, mn))


_tiles = {}


def dense_tile(fmt, seed, wave):
    """The tile wave ``wave`` must produce in ``fmt``, times the format's
    scale, as numpy.int64. Computed once per (fmt, seed, wave); do not
    modify."""
    key = (fmt, seed, wave)
    if key not in _tiles:
        a, b = operands(fmt, seed, wave)
        tile = a @ b
        tile.setflags(write=False)
        _tiles[key] = tile
    return _tiles[key]


def abs_product_max(fmt, seed, wave):
    """max over the tile of sum_k |a.b|, times the scale: what bounds every
    partial sum in any order."""
    a, b = operands(fmt, seed, wave)
    return int((np.abs(a) @ np.abs(b)).max())


# ---------------------------------------------------------------- cases
# --inject-dense values (without the format) in the order given, bad waves,
# first bad wave; for a run of 5 waves. Element 255 is the last of a 16 x 16
# tile and exists in every format.
DENSE_INJECT_CASES = [
    (["0:0"], 1, 0),
    (["3:5", "1:200"], 2, 1),
    (["4:255"], 1, 4),
]


def dense_inject_args(fmt, injections):
    return [a for inj in injections
            for a in ("--inject-dense", f"{fmt}:{inj}")]


def expect_formats(out, failing=None, bad=0, first=-1):
    """``failing`` has the given counts; every other format is clean."""
    assert list(out["dense_formats"]) == FORMAT_NAMES
    for name, got in out["dense_formats"].items():
        if name == failing:
            assert got["bad_waves"] == bad and got["first_bad_wave"] == first
        else:
            assert got["bad_waves"] == 0 and got["first_bad_wave"] == -1
