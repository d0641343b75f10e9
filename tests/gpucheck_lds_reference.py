"""An independent reference for gpucheck's LDS stage: the key of a workgroup
and round, the 16-byte vectors a workgroup's LDS holds, the FNV-1a hash of
the 163,840 bytes and what an injected bit flip must be reported as.

Like ``gpucheck_reference`` (whose ``mix64`` and pattern it uses) it includes
nothing from ``gpucheck_pattern.h``. The cases that the ``--cpu`` tests and
the GPU tests share are at the end."""

import functools

from tests.gpucheck_reference import DEFAULT_SEED, MASK64, mix64, pattern_int

LDS_VECTORS = 10240
LDS_BYTES = 16 * LDS_VECTORS  # 163,840: the whole LDS of a gfx950 CU
DUMP_VECTORS = (0, 1, 255, 256, 4095, 4096, 4097, 10238, 10239)


def lds_key(seed, group, round_):
    return mix64(seed ^ mix64(((1 << 41) | (round_ << 20) | group) & MASK64))


def vector_int(seed, group, round_, pass_, index):
    """The 128-bit value of LDS vector ``index`` of workgroup ``group``."""
    return pattern_int(lds_key(seed, group, round_), pass_, index)


def vector(seed, group, round_, pass_, index):
    return f"{vector_int(seed, group, round_, pass_, index):032x}"


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for byte in data:
        h = ((h ^ byte) * 0x100000001B3) & MASK64
    return h


@functools.lru_cache(maxsize=None)
def dump(seed, group, round_, pass_):
    """What ``--dump-lds group:round:pass`` must print for a clean LDS:
    computed once per case and shared by the tests."""
    data = b"".join(
        vector_int(seed, group, round_, pass_, i).to_bytes(16, "little")
        for i in range(LDS_VECTORS))
    assert len(data) == LDS_BYTES
    return {
        "group": group, "round": round_, "pass": pass_,
        "fnv64": f"{fnv1a64(data):016x}",
        # thread i % 256 wrote vector i; no thread of its wave may read it
        "same_wave_reads": 0,
        "vectors": {str(i): vector(seed, group, round_, pass_, i)
                    for i in DUMP_VECTORS},
    }


def expected_injection(byte, bit):
    """-> (first_bad_offset, first_bad_xor as an int): the vector's offset,
    and bit 8 (byte mod 16) + bit of the little-endian 128-bit vector."""
    return byte & ~15, 1 << (8 * (byte & 15) + bit)


def inject_args(injections):
    """(group, round, pass, byte, bit) tuples -> ``--inject-lds`` flags."""
    return [a for inj in injections
            for a in ("--inject-lds", ":".join(map(str, inj)))]


# ---------------------------------------------------------------- cases
# (byte, bit): the first cell, the first above the 64 KiB line, the last.
INJECT_POSITIONS = [(0, 0), (65536, 0), (163839, 7)]


def where_name(key):
    """The CU key as the binary prints it."""
    return (f"xcc{key >> 8}.se{(key >> 5) & 7}.sh{(key >> 4) & 1}"
            f".cu{key & 15}")


__all__ = ["DEFAULT_SEED", "LDS_BYTES", "LDS_VECTORS", "DUMP_VECTORS",
           "INJECT_POSITIONS", "dump", "expected_injection", "fnv1a64",
           "inject_args", "lds_key", "vector", "vector_int", "where_name"]
