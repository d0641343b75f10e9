"""gpucheck's dense stage on a real MI355X: the seven dense MFMA kernels
against the independent reference (which is what fixes their lane maps), the
host judge over device-produced tiles, the rate figures with their ceiling
and floor, and one check through the DiagnosticsManager.

As in test_gpucheck_mx_gpu.py, every test starts the binary as a fresh child
with a 60 s limit of its own, and once a child ends with a HIP error (11), a
signal or its time limit the remaining gpucheck GPU tests skip."""

import math

import pytest

from tests import gpucheck_dense_reference as ref
from tests import gpucheck_helpers
from tests.gpucheck_helpers import (  # noqa: F401 (fixtures)
    CHILD_TIMEOUT_S, _card_suspect, _stop_after_trouble, binary)

pytestmark = pytest.mark.gpu

# A small run: 5 waves per matrix stage, no MX and no LDS stage.
SMALL = ["--mfma-waves", 5, "--mx-waves", 0, "--lds-groups", 0]


def run_gpu(binary, *args):
    """-> (exit code, parsed last stdout line); always --bytes 4096."""
    return gpucheck_helpers.run_gpu(binary, "--bytes", 4096, *args,
                                    hide=("dense_tile",))[:2]


_seen = {}  # compute_units, once a child has reported it


def expect_tile(out, fmt, wave):
    """The tile as copied back from the device against the reference: the
    test of which lane holds which row of A and column of B, that the
    instruction pairs the k slots of A and B the way the kernel fills them,
    and of the C/D map (f64's own included)."""
    mn, _, scale, _ = ref.FORMATS[fmt]
    tile = out["dense_tile"]
    assert (tile["format"], tile["wave"]) == (fmt, wave)
    assert (tile["rows"], tile["cols"], tile["scale"]) == (mn, mn, scale)
    want = ref.dense_tile(fmt, ref.DEFAULT_SEED, wave).reshape(-1).tolist()
    got = tile["values"]
    assert len(got) == len(want)
    wrong = [e for e in range(len(want)) if got[e] != want[e]]
    assert not wrong, (f"{len(wrong)} of {len(want)} elements differ, first "
                       f"at {wrong[0]}: {got[wrong[0]]} != {want[wrong[0]]}")


@pytest.mark.parametrize("wave", [0, 4])
@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
def test_dense_tile_matches_reference(binary, fmt, wave):
    """Wave 4 of 5 is the lone wave of a second workgroup."""
    rc, out = run_gpu(binary, *SMALL, "--dump-dense-tile", f"{fmt}:{wave}")
    _seen["compute_units"] = out["compute_units"]
    assert out["dense_waves"] == 5
    expect_tile(out, fmt, wave)
    assert rc == 0, out


@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
def test_dense_tile_of_last_default_wave_matches_reference(binary, fmt):
    if "compute_units" not in _seen:  # run alone: ask the device first
        _, out = run_gpu(binary, *SMALL)
        _seen["compute_units"] = out["compute_units"]
    wave = 4 * _seen["compute_units"] - 1
    rc, out = run_gpu(binary, "--mx-waves", 0, "--lds-groups", 0,
                      "--dump-dense-tile", f"{fmt}:{wave}")
    assert out["dense_waves"] == wave + 1
    expect_tile(out, fmt, wave)
    assert rc == 0 and out["dense"] == "pass"


@pytest.mark.parametrize("args,waves", [
    (["--dense-waves", 1, *SMALL], 1),
    (SMALL, 5),                                  # capped by --mfma-waves
    (["--dense-waves", 9, *SMALL], 9),
    (["--mx-waves", 0, "--lds-groups", 0], None),  # 4 x compute units
])
def test_dense_bit_exact(binary, args, waves):
    rc, out = run_gpu(binary, *args)
    cus = out["compute_units"]
    assert cus > 0
    if waves is None:
        waves = 4 * cus
    assert out["dense_waves"] == waves
    ref.expect_formats(out)
    assert out["dense"] == "pass" and out["dense_rate"] == "pass"
    assert rc == 0 and out["failed_stages"] == []
    assert out["hbm"] == "pass" and out["mfma"] == "pass"
    assert 0 < out["dense_cus_covered"] <= min(cus, 7 * waves)
    assert out["dense_cus_covered"] <= out["dense_simds_covered"] \
        <= 4 * out["dense_cus_covered"]
    for name, got in out["dense_formats"].items():
        assert math.isfinite(got["tflops"]) and got["tflops"] > 0, name
        assert got["first_bad_where"] == ""


# FLOP per instruction and cycles per instruction and SIMD, for the formats
# whose cycles the microarchitecture guide gives; none for f64.
CEILING = {
    "f16": (2 * 32 * 32 * 16, 32),
    "bf16x16": (2 * 16 * 16 * 32, 16),
    "fp8": (2 * 32 * 32 * 16, 32),
    "bf8": (2 * 32 * 32 * 16, 32),
    "i8": (2 * 32 * 32 * 32, 32),
    "f32": (2 * 32 * 32 * 2, 64),
}


# The least a rate may be, as a share of its ceiling. The timed loops hold
# nothing but MFMAs (tests/test_gpucheck_dense_isa.py), so a rate is its
# ceiling times the clock the chip holds over the nominal one, less what a
# short launch loses. The microarchitecture guide has healthy MI355Xs holding
# 1.51 to 1.69 GHz of 2.4 in MFMA loops on random data, 0.63 at the least,
# and the MX stage found a 1 ms launch to read 15 % under a long one:
# 0.63 x 0.85 = 0.53. A loop that spends as long again on other
# instructions as on its MFMAs falls under 0.5.
FLOOR_SHARE = 0.5


def test_dense_rates_stay_under_the_issue_ceiling(binary):
    """A rate above FLOP per instruction / cycles x 4 SIMDs x compute units x
    clock means the timed work was optimised away. 1.05: the reported clock
    is nominal. A rate under FLOOR_SHARE of it means the loop issues more
    than its MFMAs."""
    rc, out = run_gpu(binary, *SMALL)
    assert rc == 0 and out["dense_rate"] == "pass"
    clock_hz = out["clock_mhz"] * 1e6
    assert clock_hz > 0
    for name, (flop, cycles) in CEILING.items():
        ceiling = flop / cycles * 4 * out["compute_units"] * clock_hz / 1e12
        rate = out["dense_formats"][name]["tflops"]
        print(f"{name}: {rate:.1f} of at most {ceiling:.1f} TFLOP/s")
        assert FLOOR_SHARE * ceiling <= rate <= 1.05 * ceiling, name
    assert out["dense_formats"]["f64"]["tflops"] > 0


@pytest.mark.parametrize("fmt,injection,wave", [
    ("f16", "0:0", 0), ("fp8", "4:1023", 4), ("i8", "2:31", 2),
    ("f64", "3:255", 3)])
def test_dense_injection_is_caught(binary, fmt, injection, wave):
    """The host comparison over tiles the real kernels produced."""
    rc, out = run_gpu(binary, *SMALL,
                      *ref.dense_inject_args(fmt, [injection]))
    assert rc == 28, out
    assert out["ok"] is False and out["failed_stages"] == ["dense"]
    assert out["dense"] == "fail" and out["dense_waves"] == 5
    ref.expect_formats(out, fmt, 1, wave)
    assert out["dense_formats"][fmt]["first_bad_where"].startswith("xcc")
    assert out["hbm"] == "pass" and out["copy"] == "pass"
    assert out["mfma"] == "pass"


def test_dense_rate_floor_fails(binary):
    rc, out = run_gpu(binary, *SMALL, "--min-dense-tflops", "f16:1e9",
                      "--min-dense-tflops", "f64:0.001")
    assert rc == 29, out
    assert out["failed_stages"] == ["dense_rate"]
    assert out["dense_rate"] == "fail"
    assert out["dense"] == "pass" and out["bandwidth"] == "pass"


def test_copy_floor_comes_before_the_dense_floor(binary):
    rc, out = run_gpu(binary, *SMALL, "--min-copy-gbs", "1e9",
                      "--min-dense-tflops", "f16:1e9")
    assert rc == 22, out
    assert out["failed_stages"] == ["bandwidth", "dense_rate"]


def test_dense_stage_can_be_skipped(binary):
    rc, out = run_gpu(binary, *SMALL, "--dense-waves", 0,
                      "--min-dense-tflops", "f16:1e9")
    assert rc == 0, out
    assert out["dense"] == "skipped" and out["dense_rate"] == "skipped"
    assert out["dense_waves"] == 0 and out["dense_cus_covered"] == 0
    assert all(v["tflops"] == 0 for v in out["dense_formats"].values())


def test_manager_check_runs_the_dense_stage():
    from k8s_runpod_kubelet_amd.config import Config
    from k8s_runpod_kubelet_amd.gpu.diagnostics import DiagnosticsManager
    from k8s_runpod_kubelet_amd.gpu.inventory import Inventory
    from k8s_runpod_kubelet_amd.gpu.ledger import Ledger

    inv = Inventory(sysfs_root="/sys", allow_synthetic=False)
    if not inv.discover():
        pytest.skip("KFD topology reports no GPUs")
    ledger = Ledger(inv)
    ledger.sync_inventory()
    mgr = DiagnosticsManager(ledger, inv,
                             Config(gpu_check_timeout_s=CHILD_TIMEOUT_S))
    res = mgr.check(0)
    if res.reason in ("timeout", "hip") or res.reason.startswith("signal"):
        _card_suspect.append(f"manager check: {res.reason}")
    assert res.ok, res.to_dict()
    assert res.data["dense"] == "pass" and res.data["dense_rate"] == "pass"
    assert res.data["dense_waves"] == 4 * res.data["compute_units"]
    assert 0 < res.data["dense_cus_covered"] <= res.data["compute_units"]
    assert not ledger.reservations
