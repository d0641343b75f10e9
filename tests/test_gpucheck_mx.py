"""gpucheck's MX stage — everything that needs no GPU: ``--cpu --mx-waves``
(host decode, scale and multiply against the independent reference, the
judge, the JSON, exit codes 24 and their order), the decoders of the
reference itself, and the manager, config, CLI and metrics plumbing with a
fake runner."""

import json
import math
import subprocess
import time

import pytest

from k8s_runpod_kubelet_amd.config import Config, load_config
from k8s_runpod_kubelet_amd.gpu.diagnostics import (
    EXIT_STAGES, DiagnosticsManager, GpuCheckResult, first_bad_mx,
    mx_floor_args, run_gpucheck)
from tests import gpucheck_helpers
from tests import gpucheck_mx_reference as ref
from tests.gpucheck_helpers import gpucheck  # noqa: F401 (fixture)


def run_cpu(binary, *args):
    return gpucheck_helpers.run_cpu(binary, "--bytes", 4096, *args)


# ------------------------------------------------------------ reference

def test_reference_decodes_every_e2m1_code():
    positive = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    for code, value in enumerate(positive):
        assert ref.decode_e2m1(code) == value
        assert ref.decode_e2m1(code | 8) == -value
    assert math.copysign(1.0, ref.decode_e2m1(8)) == -1.0  # -0 is a code


def test_reference_decoder_spot_checks():
    assert ref.decode_e4m3fn(0b0_1001_111) == 7.5
    assert ref.decode_e4m3fn(0b1_0110_000) == -0.5
    assert ref.decode_e5m2(0b0_10000_11) == 3.5
    # the formats' documented extremes and specials
    assert ref.decode_e4m3fn(0x7E) == 448.0 and ref.decode_e4m3fn(0x01) == 2.0 ** -9
    assert math.isnan(ref.decode_e4m3fn(0x7F)) and math.isnan(ref.decode_e4m3fn(0xFF))
    assert ref.decode_e5m2(0x7B) == 57344.0 and ref.decode_e5m2(0x01) == 2.0 ** -16
    assert ref.decode_e5m2(0x7C) == math.inf and ref.decode_e5m2(0xFC) == -math.inf
    assert math.isnan(ref.decode_e5m2(0x7D))
    assert [ref.decode_e8m0(c) for c in (126, 127, 128)] == [0.5, 1.0, 2.0]
    assert math.isnan(ref.decode_e8m0(255))


def test_reference_operands_cover_the_value_sets():
    """All 16 e2m1 codes, both signs of every multiple of 1/2, all three
    scales; B is not symmetric in any sense a transposed read could hide."""
    seed = ref.DEFAULT_SEED
    key_a = ref.mx_key(seed, 0, 2, 0)
    assert {ref.a_code("e2m1", key_a, r, k)
            for r in range(4) for k in range(ref.MX_K)} == set(range(16))
    a, b = ref.operands("fp8", seed, 0)
    assert (a * 4 == (a * 4).round()).all() and abs(a).max() <= 15
    key = ref.mx_key(seed, 0, 0, 0)
    assert {ref.scale_byte(key, r, blk) for r in range(32)
            for blk in range(8)} == {126, 127, 128}
    assert (b[:32, :] != b[:32, :].T).any()
    tile = ref.mx_tile("fp8", seed, 0)
    assert tile.shape == (32, 32) and tile.dtype == "int64"
    assert (tile != tile.T).any()


# ------------------------------------------------------- binary, --cpu

@pytest.mark.parametrize("wave", [0, 4])
@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
def test_cpu_mx_tile_matches_reference(gpucheck, fmt, wave):
    rc, out = run_cpu(gpucheck, "--mx-waves", 5, "--dump-mx-tile",
                      f"{fmt}:{wave}")
    assert rc == 0, out
    assert out["mx"] == "pass" and out["mx_waves"] == 5
    assert out["mx_rate"] == "skipped"
    assert out["mx_tile"]["format"] == fmt and out["mx_tile"]["wave"] == wave
    assert out["mx_tile"]["values_x16"] == \
        ref.mx_tile(fmt, ref.DEFAULT_SEED, wave).reshape(-1).tolist()
    ref.expect_formats(out)
    assert all(v["tflops"] == 0 for v in out["mx_formats"].values())


def test_cpu_mx_tile_follows_the_seed(gpucheck):
    seed = 0x0123456789ABCDEF
    rc, out = run_cpu(gpucheck, "--mx-waves", 2, "--seed", seed,
                      "--dump-mx-tile", "fp8xfp4:1")
    assert rc == 0
    assert out["mx_tile"]["values_x16"] == \
        ref.mx_tile("fp8xfp4", seed, 1).reshape(-1).tolist()


@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
@pytest.mark.parametrize("injections,bad,first", ref.MX_INJECT_CASES)
def test_cpu_mx_injection_is_caught(gpucheck, fmt, injections, bad, first):
    rc, out = run_cpu(gpucheck, "--mx-waves", 5,
                      *ref.mx_inject_args(fmt, injections))
    assert rc == 24, out
    assert out["ok"] is False and out["exit_code"] == 24
    assert out["failed_stages"] == ["mx"]
    assert out["mx"] == "fail" and out["mx_waves"] == 5
    ref.expect_formats(out, fmt, bad, first)
    assert out["hbm"] == "pass" and out["mfma"] == "skipped"


def test_cpu_failure_order(gpucheck):
    """20 before 21 before 24; failed_stages lists all in that order."""
    rc, out = run_cpu(gpucheck, "--passes", 1, "--mx-waves", 2,
                      "--inject-flip", "0:0", "--inject-mx", "fp4:1:0")
    assert rc == 20 and out["failed_stages"] == ["hbm", "mx"]
    rc, out = run_cpu(gpucheck, "--mfma-waves", 2, "--mx-waves", 2,
                      "--inject-mfma", "1:0", "--inject-mx", "fp4:1:0")
    assert rc == 21 and out["failed_stages"] == ["mfma", "mx"]
    rc, out = run_cpu(gpucheck, "--mfma-waves", 2, "--mx-waves", 2,
                      "--inject-mx", "fp4:1:0")
    assert rc == 24 and out["failed_stages"] == ["mx"]
    assert out["mfma"] == "pass"


@pytest.mark.parametrize("args", [
    ["--mx-waves", "5", "--inject-mx", "fp6:0:0"],       # unknown format
    ["--mx-waves", "5", "--dump-mx-tile", "mxfp8:0"],
    ["--mx-waves", "5", "--min-mx-tflops", "int8:1"],
    ["--mx-waves", "5", "--inject-mx", "fp8:5:0"],       # wave outside the run
    ["--mx-waves", "5", "--dump-mx-tile", "fp8:5"],
    ["--inject-mx", "fp8:0:0"],                          # --cpu runs no wave
    ["--mfma-waves", "5", "--dump-mx-tile", "fp8:0"],    # the cap is GPU-only
    ["--mx-waves", "0", "--inject-mx", "fp8:0:0"],
    ["--mx-waves", "5", "--inject-mx", "fp8:0:1024"],    # element >= 1024
    ["--mx-waves", "5"] + ["--inject-mx", "bf8:0:0"] * 9,  # a ninth injection
    ["--mx-waves", "65537"],
    ["--mx-waves", "5", "--inject-mx", "fp8:0"],
    ["--mx-waves", "5", "--min-mx-tflops", "fp8:-1"],
])
def test_bad_mx_flags_exit_2(gpucheck, args):
    proc = subprocess.run([gpucheck, "--cpu", *args], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 2
    assert "usage:" in proc.stderr and "24 MX mismatch" in proc.stderr
    assert proc.stdout == ""


@pytest.mark.parametrize("args", [[], ["--mx-waves", 0],
                                  ["--mfma-waves", 3]])
def test_cpu_mx_skipped(gpucheck, args):
    rc, out = run_cpu(gpucheck, *args)
    assert rc == 0
    assert out["mx"] == "skipped" and out["mx_rate"] == "skipped"
    assert out["mx_waves"] == 0 and "mx_tile" not in out
    ref.expect_formats(out)


def test_cpu_floors_are_ignored(gpucheck):
    rc, out = run_cpu(gpucheck, "--mx-waves", 1, "--min-mx-tflops", "fp4:1e9",
                      "--min-mx-tflops", "fp8:1e9")
    assert rc == 0 and out["mx"] == "pass" and out["mx_rate"] == "skipped"


def test_runner_maps_exit_24(gpucheck, synthetic_ledger):
    assert EXIT_STAGES[24] == "mx" and EXIT_STAGES[25] == "mx_rate"
    res = run_gpucheck(0, synthetic_ledger.inventory, nbytes=4096,
                       timeout_s=30, binary=gpucheck,
                       extra_args=["--cpu", "--mx-waves", "5",
                                   "--inject-mx", "fp4:3:9"])
    assert not res.ok and res.exit_code == 24 and res.reason == "mx"
    assert first_bad_mx(res.data) == "fp4 wave 3"


def test_operator_cli_passes_mx_floor(gpucheck, capsys):
    from k8s_runpod_kubelet_amd.gpu import diagnostics

    code = diagnostics.main(["--gpu", "0", "--bytes", "4K",
                             "--sysfs-root", "/nonexistent-sysfs",
                             "--min-mx-tflops", "fp4:100",
                             "--", "--cpu", "--mx-waves", "2",
                             "--inject-mx", "bf8:1:0"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert code == 24 and out["reason"] == "mx"
    assert out["mx_formats"]["bf8"]["first_bad_wave"] == 1


# ---------------------------------------------- manager, config, metrics

MX_FORMATS_OK = {name: {"bad_waves": 0, "first_bad_wave": -1,
                        "tflops": 1000.0 + i}
                 for i, name in enumerate(ref.FORMAT_NAMES)}
GOOD = {"tool": "gpucheck", "ok": True, "exit_code": 0, "mx": "pass",
        "mx_rate": "pass", "mx_waves": 1024, "mx_formats": MX_FORMATS_OK}


class FakeRunner:
    def __init__(self):
        self.calls = []
        self.result = (0, "", GOOD)

    def __call__(self, gpu, inventory, *, nbytes, timeout_s, extra_args=()):
        self.calls.append(tuple(extra_args))
        code, reason, data = self.result
        return GpuCheckResult(gpu=gpu, ok=code == 0, exit_code=code,
                              reason=reason, data=dict(data),
                              duration_s=0.01, timestamp=time.time())


class Recorder:
    def __init__(self):
        self.events = []

    def event(self, obj, event_type, reason, message):
        self.events.append((event_type, reason, message))


@pytest.fixture
def manager(synthetic_ledger):
    runner, rec = FakeRunner(), Recorder()
    mgr = DiagnosticsManager(synthetic_ledger, synthetic_ledger.inventory,
                             Config(gpu_check_bytes=1 << 20), runner=runner,
                             recorder=rec, node_name="node-a")
    return mgr, runner, rec, synthetic_ledger


def test_config_defaults_and_manager_flags(manager):
    mgr, runner, _, _ = manager
    assert Config().gpu_check_mx is True
    assert Config().gpu_check_min_mx_tflops == {}
    mgr.check(0)
    assert runner.calls[-1] == ()
    mgr.config.gpu_check_min_mx_tflops = {"fp4": 4000, "fp8": 2000.5,
                                          "bf8": 0}
    mgr.config.gpu_check_min_copy_gbs = 1500.0
    mgr.check(0)
    assert runner.calls[-1] == ("--min-copy-gbs", "1500.0",
                                "--min-mx-tflops", "fp8:2000.5",
                                "--min-mx-tflops", "fp4:4000.0")
    mgr.config.gpu_check_mx = False  # the floors go with the stage
    mgr.check(0)
    assert runner.calls[-1] == ("--min-copy-gbs", "1500.0", "--mx-waves", "0")
    with pytest.raises(ValueError):
        mx_floor_args({"fp6": 1})


def test_manager_flags_are_accepted_by_the_binary(gpucheck):
    proc = subprocess.run(
        [gpucheck, "--cpu", "--bytes", "4096",
         *mx_floor_args({"fp8": 2000.5, "bf8": 1, "fp4": 4000, "fp8xfp4": 3}),
         "--mx-waves", "0"], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr


@pytest.mark.parametrize("code,reason", [(24, "mx"), (25, "mx_rate")])
def test_manager_mx_failure_fences_and_names_the_wave(manager, code, reason):
    mgr, runner, rec, ledger = manager
    formats = dict(MX_FORMATS_OK)
    data = dict(GOOD, ok=False, exit_code=code, failed_stages=[reason])
    if reason == "mx":
        formats["fp4"] = {"bad_waves": 3, "first_bad_wave": 17, "tflops": 9.0}
        data.update(mx="fail", mx_formats=formats)
    else:
        data.update(mx_rate="fail")
    runner.result = (code, reason, data)
    res = mgr.check(2)
    assert not res.ok and res.reason == reason
    assert not ledger.states[2].schedulable
    assert ledger.states[2].gpu.diag_reason == reason
    (etype, why, message), = rec.events
    assert etype == "Warning" and why == "GpuCheckFailed"
    assert f"stage={reason}" in message
    assert ("fp4 wave 17" in message) == (reason == "mx")


def test_metrics_gauge(manager):
    from k8s_runpod_kubelet_amd.server import metrics

    mgr, runner, _, _ = manager
    mgr.check(5)
    text = metrics.render().decode()
    for i, name in enumerate(ref.FORMAT_NAMES):
        assert (f'amdvk_gpu_check_mx_tflops{{format="{name}",gpu="5"}} '
                f'{1000.0 + i}') in text
    # a run without rates (stage off, or --cpu) sets nothing
    runner.result = (0, "", dict(GOOD, mx="skipped", mx_rate="skipped"))
    mgr.check(6)
    assert 'gpu="6"}' not in "\n".join(
        ln for ln in metrics.render().decode().splitlines()
        if ln.startswith("amdvk_gpu_check_mx_tflops"))


def test_cli_and_provider_config(tmp_path):
    from k8s_runpod_kubelet_amd.cli import build_parser, parse_mx_floors

    args = build_parser().parse_args([])
    assert args.gpu_check_mx is None and args.gpu_check_min_mx_tflops is None
    args = build_parser().parse_args([
        "--no-gpu-check-mx", "--gpu-check-min-mx-tflops", "fp4:4000",
        "--gpu-check-min-mx-tflops", "fp8:2000"])
    assert args.gpu_check_mx is False
    assert parse_mx_floors(args.gpu_check_min_mx_tflops, {"bf8": 5}) == {
        "bf8": 5, "fp4": 4000.0, "fp8": 2000.0}
    with pytest.raises(SystemExit):
        parse_mx_floors(["fp6:1"])
    path = tmp_path / "provider.yaml"
    path.write_text("gpu_check_mx: false\n"
                    "gpu_check_min_mx_tflops:\n  fp4: 4000\n  fp8xfp4: 2500\n")
    cfg = load_config(str(path))
    assert cfg.gpu_check_mx is False
    assert cfg.gpu_check_min_mx_tflops == {"fp4": 4000, "fp8xfp4": 2500}
    path.write_text("gpu_check_min_mx_tflops: 7\n")
    with pytest.raises(ValueError):
        load_config(str(path))
