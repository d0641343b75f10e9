"""gpucheck's MX stage on a real MI355X: the block-scaled 32x32x64 MFMA
kernels against the independent reference, the host judge over
device-produced tiles, the rate figures and their floor, and one check
through the DiagnosticsManager.

As in test_gpucheck_gpu.py, every test starts the binary as a fresh child
with a 60 s limit of its own, and once a child ends with a HIP error (11), a
signal or its time limit the remaining gpucheck GPU tests skip."""

import math

import pytest

from tests import gpucheck_helpers
from tests import gpucheck_mx_reference as ref
from tests.gpucheck_helpers import (  # noqa: F401 (fixtures)
    CHILD_TIMEOUT_S, _card_suspect, _stop_after_trouble, binary)

pytestmark = pytest.mark.gpu


def run_gpu(binary, *args):
    """-> (exit code, parsed last stdout line); always --bytes 4096."""
    return gpucheck_helpers.run_gpu(binary, "--bytes", 4096, *args)[:2]


_seen = {}  # compute_units, once a child has reported it


def expect_tile(out, fmt, wave):
    """The tile as copied back from the device against the reference: the
    test of the lane, byte and nibble maps of both operands, of which block
    each scale byte scales, and of the byte select of every k-step."""
    assert out["mx_tile"] is not None, "a value is not a multiple of 1/16"
    assert out["mx_tile"]["format"] == fmt and out["mx_tile"]["wave"] == wave
    want = ref.mx_tile(fmt, ref.DEFAULT_SEED, wave).reshape(-1).tolist()
    got = out["mx_tile"]["values_x16"]
    wrong = [e for e in range(1024) if got[e] != want[e]]
    assert not wrong, (f"{len(wrong)} of 1024 elements differ, first at "
                       f"{wrong[0]}: {got[wrong[0]]} != {want[wrong[0]]}")


@pytest.mark.parametrize("wave", [0, 4])
@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
def test_mx_tile_matches_reference(binary, fmt, wave):
    """Wave 4 of 5 is the lone wave of a second workgroup."""
    rc, out = run_gpu(binary, "--mx-waves", 5, "--dump-mx-tile",
                      f"{fmt}:{wave}")
    _seen["compute_units"] = out["compute_units"]
    expect_tile(out, fmt, wave)
    assert rc == 0, out


@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
def test_mx_tile_of_last_default_wave_matches_reference(binary, fmt):
    if "compute_units" not in _seen:  # run alone: ask the device first
        _, out = run_gpu(binary, "--mfma-waves", 1)
        _seen["compute_units"] = out["compute_units"]
    wave = 4 * _seen["compute_units"] - 1
    rc, out = run_gpu(binary, "--dump-mx-tile", f"{fmt}:{wave}")
    assert out["mx_waves"] == wave + 1
    expect_tile(out, fmt, wave)
    assert rc == 0 and out["mx"] == "pass"


@pytest.mark.parametrize("args,waves", [
    (["--mx-waves", 1], 1),
    (["--mx-waves", 5], 5),
    ([], None),                             # 4 x compute units
    (["--mfma-waves", 5], 5),               # capped by --mfma-waves
    (["--mfma-waves", 5, "--mx-waves", 9], 9),
])
def test_mx_bit_exact(binary, args, waves):
    rc, out = run_gpu(binary, *args)
    assert out["compute_units"] > 0
    assert out["mx_waves"] == (waves if waves is not None
                               else 4 * out["compute_units"])
    ref.expect_formats(out)
    assert out["mx"] == "pass" and out["mx_rate"] == "pass"
    assert rc == 0 and out["failed_stages"] == []
    assert out["hbm"] == "pass" and out["mfma"] == "pass"
    for name, got in out["mx_formats"].items():
        assert math.isfinite(got["tflops"]) and got["tflops"] > 0, name


def test_mx_stage_can_be_skipped(binary):
    rc, out = run_gpu(binary, "--mfma-waves", 1, "--mx-waves", 0,
                      "--min-mx-tflops", "fp4:1e9")
    assert rc == 0, out
    assert out["mx"] == "skipped" and out["mx_rate"] == "skipped"
    assert out["mx_waves"] == 0


@pytest.mark.parametrize("fmt,injection,wave", [
    ("fp8", "0:0", 0), ("bf8", "4:1023", 4), ("fp4", "2:31", 2),
    ("fp8xfp4", "3:512", 3)])
def test_mx_injection_is_caught(binary, fmt, injection, wave):
    """The host comparison over tiles the real kernels produced."""
    rc, out = run_gpu(binary, "--mfma-waves", 5,
                      *ref.mx_inject_args(fmt, [injection]))
    assert rc == 24, out
    assert out["ok"] is False and out["failed_stages"] == ["mx"]
    assert out["mx"] == "fail" and out["mx_waves"] == 5
    ref.expect_formats(out, fmt, 1, wave)
    assert out["hbm"] == "pass" and out["copy"] == "pass"
    assert out["mfma"] == "pass"


def test_mx_rate_floor_fails(binary):
    rc, out = run_gpu(binary, "--mfma-waves", 1, "--min-mx-tflops", "fp4:1e9",
                      "--min-mx-tflops", "fp8:0.001")
    assert rc == 25, out
    assert out["failed_stages"] == ["mx_rate"] and out["mx_rate"] == "fail"
    assert out["mx"] == "pass" and out["bandwidth"] == "pass"
    for name, got in out["mx_formats"].items():
        assert math.isfinite(got["tflops"]) and got["tflops"] > 0, name


def test_manager_check_runs_the_mx_stage():
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
    assert res.data["mx"] == "pass" and res.data["mx_rate"] == "pass"
    assert res.data["mx_waves"] == 4 * res.data["compute_units"]
    assert not ledger.reservations
