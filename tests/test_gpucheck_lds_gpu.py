"""gpucheck's LDS stage and wave locations on a real MI355X: what the LDS of
a compute unit reads back against the independent reference, injected flips
located by offset, bit and compute unit, the invariants that fix the HW_ID
field table (one CU key per workgroup, as many keys as compute units), full
coverage, and where the MFMA and MX tiles ran.

As in test_gpucheck_mx_gpu.py, every test starts the binary as a fresh child
with a 60 s limit of its own, and once a child ends with a HIP error (11), a
signal or its time limit the remaining gpucheck GPU tests skip. The coverage
cases need a GPU that runs nothing else, as gpucheck has in production."""

import pytest

from tests import gpucheck_helpers
from tests import gpucheck_lds_reference as ref
from tests.gpucheck_helpers import (  # noqa: F401 (fixtures)
    _stop_after_trouble, binary)

pytestmark = pytest.mark.gpu

SEED = ref.DEFAULT_SEED
# The smallest region the binary accepts, four MFMA waves, no MX stage.
SMALL = ["--bytes", "16", "--mfma-waves", "4", "--mx-waves", "0"]
LDS_SMALL = ["--lds-groups", "8", "--lds-rounds", "2"]

# Every key of the report before the LDS stage and the location keys.
KEYS_BEFORE = {
    "tool", "mode", "device", "compute_units", "ok", "exit_code",
    "failed_stages", "bytes", "vectors", "passes", "base_index", "seed",
    "hbm", "mismatch_vectors", "first_bad_offset", "first_bad_pass",
    "first_bad_xor", "write_gbs", "read_gbs", "write_gbs_plain",
    "write_gbs_nontemporal", "store_variant", "bandwidth", "copy_gbs",
    "min_copy_gbs", "cache_resident", "copy", "copy_mismatch_vectors",
    "copy_first_bad_offset", "copy_first_bad_xor", "mfma", "mfma_waves",
    "mfma_bad_waves", "mfma_first_bad_wave", "mx", "mx_waves", "mx_rate",
    "mx_formats", "wall_s"}
MX_FORMAT_KEYS_BEFORE = {"bad_waves", "first_bad_wave", "tflops"}


def run_gpu(binary, *args):
    """-> (exit code, parsed last stdout line)."""
    return gpucheck_helpers.run_gpu(binary, *args,
                                    hide=("lds_where", "mfma_where"))[:2]


@pytest.mark.parametrize("pass_", [0, 1])
def test_lds_dump_matches_reference(binary, pass_):
    """What the last wave-rotated read of group 2 returned, every byte of it
    (fnv64), against the port: the write and read index maps and the 64 KiB
    line."""
    rc, out = run_gpu(binary, *SMALL, "--lds-groups", 3, "--lds-rounds", 2,
                      "--dump-lds", f"2:1:{pass_}")
    assert out["lds"] != "skipped", out.get("lds_skipped_reason")
    want = ref.dump(SEED, 2, 1, pass_)
    assert out["lds_dump"]["vectors"] == want["vectors"]
    assert out["lds_dump"] == want
    assert out["lds_bytes_per_cu"] == 163840
    assert out["lds_groups"] == 3 and out["lds_rounds"] == 2
    assert rc == 0 and out["lds"] == "pass" and out["lds_bad_cus"] == []


@pytest.mark.parametrize("round_,pass_", [(0, 0), (1, 1)])
@pytest.mark.parametrize("byte,bit", ref.INJECT_POSITIONS)
def test_lds_injection_is_located(binary, byte, bit, round_, pass_):
    group = 5
    rc, out = run_gpu(binary, *SMALL, *LDS_SMALL, "--dump-lds-where",
                      *ref.inject_args([(group, round_, pass_, byte, bit)]))
    assert rc == 26, out
    assert out["ok"] is False and out["failed_stages"] == ["lds"]
    assert out["lds"] == "fail"
    # every other group, in every launch, is clean
    assert out["lds_bad_groups"] == 1
    (cu,) = out["lds_bad_cus"]
    offset, xor = ref.expected_injection(byte, bit)
    assert cu["first_bad_offset"] == offset
    assert len(cu["first_bad_xor"]) == 32
    assert int(cu["first_bad_xor"], 16) == xor
    assert cu["round"] == round_ and cu["pass"] == pass_
    assert cu["bad_vectors"] == 1
    assert len(out["lds_where"]) == 8
    assert cu["key"] == out["lds_where"][group][0][0]
    assert cu["where"] == ref.where_name(cu["key"])
    assert out["hbm"] == "pass" and out["mfma"] == "pass"


def test_location_invariants(binary):
    """A workgroup lives on one compute unit, so its four waves share a CU
    key (a mask that lets SIMD or wave bits in breaks this), and there are
    no more keys than compute units (stray bits give more)."""
    rc, out = run_gpu(binary, *SMALL, "--dump-lds-where")
    assert rc == 0, out
    cus = out["compute_units"]
    assert cus > 0 and out["lds_groups"] == 2 * cus
    assert len(out["lds_where"]) == 2 * cus
    keys = set()
    for group, waves in enumerate(out["lds_where"]):
        assert len(waves) == 4
        assert len({w[0] for w in waves}) == 1, (group, waves)
        assert all(0 <= w[1] <= 3 for w in waves), (group, waves)
        keys.add(waves[0][0])
    assert len(keys) <= cus
    assert out["lds_cus_covered"] >= len(keys)
    # the MFMA waves ran on compute units the LDS stage also names
    if len(keys) == cus:
        assert {w[0] for w in out["mfma_where"]} <= keys


def test_lds_covers_every_compute_unit(binary):
    rc, out = run_gpu(binary, *SMALL, "--lds-require-coverage")
    assert out["lds_rounds"] == 4 and out["lds_groups"] == 2 * out["compute_units"]
    assert out["lds_cus_covered"] == out["compute_units"]
    assert out["lds_coverage"] == "full"
    assert out["lds_launches"] <= 8
    assert rc == 0 and out["failed_stages"] == []
    assert out["lds_gbs"] > 0


def test_mfma_and_mx_locations(binary):
    """Default sizes of the MFMA and MX stages; the bad wave is named by the
    compute unit that its own record holds."""
    wave = 777
    rc, out = run_gpu(binary, "--bytes", "16", "--dump-lds-where",
                      "--inject-mfma", f"{wave}:5",
                      "--inject-mx", "fp4:3:0")
    assert rc == 21, out
    cus = out["compute_units"]
    assert 0 < out["mfma_cus_covered"] <= cus
    assert 0 < out["mfma_simds_covered"] <= 4 * cus
    assert out["mfma_simds_covered"] >= out["mfma_cus_covered"]
    assert 0 < out["mx_cus_covered"] <= cus
    assert 0 < out["mx_simds_covered"] <= 4 * cus
    assert len(out["mfma_where"]) == out["mfma_waves"] == 8 * cus
    assert all(0 <= w[1] <= 3 for w in out["mfma_where"])
    assert out["mfma_first_bad_wave"] == wave
    assert out["mfma_first_bad_where"] != ""
    assert out["mfma_first_bad_where"] == \
        ref.where_name(out["mfma_where"][wave][0])
    lds_keys = {waves[0][0] for waves in out["lds_where"]}
    if out["lds_coverage"] == "full":
        assert out["mfma_where"][wave][0] in lds_keys
    fp4 = out["mx_formats"]["fp4"]
    assert fp4["first_bad_wave"] == 3 and fp4["first_bad_where"].startswith("xcc")
    assert out["mx_formats"]["fp8"]["first_bad_where"] == ""


def test_default_run_keeps_every_key(binary):
    rc, out = run_gpu(binary)
    assert rc == 0 and out["ok"] is True and out["failed_stages"] == []
    assert KEYS_BEFORE <= set(out)
    for name, got in out["mx_formats"].items():
        assert MX_FORMAT_KEYS_BEFORE <= set(got), name
    assert out["lds"] == "pass" and out["lds_bad_groups"] == 0
    assert out["mfma_first_bad_where"] == ""
    assert "lds_where" not in out and "lds_dump" not in out
