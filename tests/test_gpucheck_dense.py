"""gpucheck's dense stage — everything that needs no GPU: ``--cpu
--dense-waves`` (the host integer product against the independent reference,
the judge, the JSON, exit code 28 and its order among the others), the
exactness bounds asserted from the reference, and the manager, config, CLI,
metrics and chart plumbing with a fake runner."""

import json
import pathlib
import subprocess
import time

import pytest

from k8s_runpod_kubelet_amd.config import Config, load_config
from k8s_runpod_kubelet_amd.gpu.diagnostics import (
    DENSE_FORMATS, EXIT_STAGES, DiagnosticsManager, GpuCheckResult,
    dense_floor_args, first_bad_dense, run_gpucheck)
from tests import gpucheck_dense_reference as ref
from tests import gpucheck_helpers
from tests.gpucheck_helpers import gpucheck  # noqa: F401 (fixture)

REPO = pathlib.Path(__file__).resolve().parent.parent


def run_cpu(binary, *args):
    return gpucheck_helpers.run_cpu(binary, "--bytes", 4096, *args)


# ------------------------------------------------------------ reference

def test_reference_formats_are_the_binarys():
    assert tuple(ref.FORMAT_NAMES) == DENSE_FORMATS


def test_reference_array_forms_agree_with_the_scalar_ones():
    import numpy as np

    xs = [0, 1, 2 ** 63, ref.MASK64, ref.DEFAULT_SEED, 0x0123456789ABCDEF]
    hashes = ref.mix64_array(np.array(xs, dtype=np.uint64))
    assert hashes.tolist() == [ref.mix64(x) for x in xs]
    for fmt in ref.FORMAT_NAMES:
        key = ref.dense_key(ref.DEFAULT_SEED, 3, ref.FORMAT_NAMES.index(fmt), 1)
        hs = [ref.mix64((key + i) & ref.MASK64) for i in range(300)]
        assert ref.values(fmt, np.array(hs, dtype=np.uint64)).tolist() == \
            [ref.value(fmt, h) for h in hs]


def test_reference_operands_cover_the_value_sets():
    seed = ref.DEFAULT_SEED
    a, b = ref.operands("i8", seed, 0)
    assert set(a.reshape(-1).tolist()) == set(range(-128, 128))
    a, _ = ref.operands("f16", seed, 0)
    assert set(a.reshape(-1).tolist()) == set(range(-15, 16))
    a, _ = ref.operands("fp8", seed, 0)   # twice +-m/2, m <= 15
    assert set(a.reshape(-1).tolist()) == set(range(-15, 16))
    a, _ = ref.operands("bf8", seed, 0)
    assert set(a.reshape(-1).tolist()) == set(range(-7, 8))
    a, b = ref.operands("f32", seed, 0)
    assert a.min() >= -511 and a.max() <= 511 and abs(a).max() > 500
    a, b = ref.operands("f64", seed, 0)
    assert abs(a).max() <= 2 ** 20 - 1 and abs(a).max() > 2 ** 19
    assert (b[:16, :] != b[:16, :].T).any()      # B is not symmetric
    for fmt in ref.FORMAT_NAMES:
        tile = ref.dense_tile(fmt, seed, 0)
        mn = ref.FORMATS[fmt][0]
        assert tile.shape == (mn, mn) and tile.dtype == "int64"
        assert (tile != tile.T).any()
    # one key per (wave, format, matrix)
    keys = {ref.dense_key(seed, w, f, which) for w in range(4)
            for f in range(7) for which in (0, 1)}
    assert len(keys) == 4 * 7 * 2


@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
def test_exactness_bound_holds(fmt):
    """The largest sum of |a.b| over 256 tiles stays under the bound the
    header states, and that bound under what the accumulator holds exactly:
    so every partial sum, in any order, is exact."""
    _, _, _, bound = ref.FORMATS[fmt]
    assert bound <= ref.EXACT_BELOW[fmt]
    worst = max(ref.abs_product_max(fmt, ref.DEFAULT_SEED, w)
                for w in range(256))
    print(f"{fmt}: max sum |a.b| = {worst}, bound {bound}")
    assert 0 < worst <= bound


# ------------------------------------------------------- binary, --cpu

@pytest.mark.parametrize("wave", [0, 4])
@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
def test_cpu_dense_tile_matches_reference(gpucheck, fmt, wave):
    rc, out = run_cpu(gpucheck, "--dense-waves", 5, "--dump-dense-tile",
                      f"{fmt}:{wave}")
    assert rc == 0, out
    assert out["dense"] == "pass" and out["dense_waves"] == 5
    assert out["dense_rate"] == "skipped"
    assert out["dense_cus_covered"] == 0 and out["dense_simds_covered"] == 0
    mn, _, scale, _ = ref.FORMATS[fmt]
    tile = out["dense_tile"]
    assert (tile["format"], tile["wave"]) == (fmt, wave)
    assert (tile["rows"], tile["cols"], tile["scale"]) == (mn, mn, scale)
    assert tile["values"] == \
        ref.dense_tile(fmt, ref.DEFAULT_SEED, wave).reshape(-1).tolist()
    ref.expect_formats(out)
    assert all(v["tflops"] == 0 and v["first_bad_where"] == ""
               for v in out["dense_formats"].values())


def test_cpu_dense_tile_follows_the_seed(gpucheck):
    seed = 0x0123456789ABCDEF
    rc, out = run_cpu(gpucheck, "--dense-waves", 2, "--seed", seed,
                      "--dump-dense-tile", "f64:1")
    assert rc == 0
    assert out["dense_tile"]["values"] == \
        ref.dense_tile("f64", seed, 1).reshape(-1).tolist()


@pytest.mark.parametrize("args", [[], ["--dense-waves", 0],
                                  ["--mfma-waves", 3]])
def test_cpu_dense_skipped(gpucheck, args):
    rc, out = run_cpu(gpucheck, *args)
    assert rc == 0
    assert out["dense"] == "skipped" and out["dense_rate"] == "skipped"
    assert out["dense_waves"] == 0 and "dense_tile" not in out
    ref.expect_formats(out)


@pytest.mark.parametrize("fmt", ref.FORMAT_NAMES)
@pytest.mark.parametrize("injections,bad,first", ref.DENSE_INJECT_CASES)
def test_cpu_dense_injection_is_caught(gpucheck, fmt, injections, bad, first):
    rc, out = run_cpu(gpucheck, "--dense-waves", 5,
                      *ref.dense_inject_args(fmt, injections))
    assert rc == 28, out
    assert out["ok"] is False and out["exit_code"] == 28
    assert out["failed_stages"] == ["dense"]
    assert out["dense"] == "fail" and out["dense_waves"] == 5
    ref.expect_formats(out, fmt, bad, first)
    assert out["hbm"] == "pass" and out["mx"] == "skipped"


def test_cpu_failure_order(gpucheck):
    """20, 21, 24 and 26 before 28; failed_stages lists all in that order.
    (22 needs a device: test_gpucheck_dense_gpu.py.)"""
    dense = ["--dense-waves", 2, "--inject-dense", "i8:1:0"]
    rc, out = run_cpu(gpucheck, "--passes", 1, "--inject-flip", "0:0", *dense)
    assert rc == 20 and out["failed_stages"] == ["hbm", "dense"]
    rc, out = run_cpu(gpucheck, "--mfma-waves", 2, "--inject-mfma", "1:0",
                      *dense)
    assert rc == 21 and out["failed_stages"] == ["mfma", "dense"]
    rc, out = run_cpu(gpucheck, "--mx-waves", 2, "--inject-mx", "fp4:1:0",
                      *dense)
    assert rc == 24 and out["failed_stages"] == ["mx", "dense"]
    rc, out = run_cpu(gpucheck, "--lds-groups", 2, "--lds-rounds", 1,
                      "--inject-lds", "1:0:0:0:0", *dense)
    assert rc == 26 and out["failed_stages"] == ["lds", "dense"]
    rc, out = run_cpu(gpucheck, "--mfma-waves", 2, "--mx-waves", 2, *dense)
    assert rc == 28 and out["failed_stages"] == ["dense"]
    assert out["mfma"] == "pass" and out["mx"] == "pass"


def test_cpu_floors_are_ignored(gpucheck):
    rc, out = run_cpu(gpucheck, "--dense-waves", 1, "--min-dense-tflops",
                      "f16:1e9", "--min-dense-tflops", "f64:1e9")
    assert rc == 0 and out["dense"] == "pass"
    assert out["dense_rate"] == "skipped" and out["clock_mhz"] == 0


@pytest.mark.parametrize("args", [
    ["--dense-waves", "5", "--inject-dense", "bf16:0:0"],   # unknown format
    ["--dense-waves", "5", "--dump-dense-tile", "fp4:0"],
    ["--dense-waves", "5", "--min-dense-tflops", "int8:1"],
    ["--dense-waves", "5", "--inject-dense", "f16:5:0"],    # wave >= waves
    ["--dense-waves", "5", "--dump-dense-tile", "f16:5"],
    ["--inject-dense", "f16:0:0"],                          # --cpu: no wave
    ["--mfma-waves", "5", "--dump-dense-tile", "f16:0"],    # GPU-only cap
    ["--dense-waves", "0", "--inject-dense", "f16:0:0"],
    ["--dense-waves", "5", "--inject-dense", "f16:0:1024"],  # >= rows.cols
    ["--dense-waves", "5", "--inject-dense", "bf16x16:0:256"],
    ["--dense-waves", "5", "--inject-dense", "f64:0:256"],
    ["--dense-waves", "5"] + ["--inject-dense", "i8:0:0"] * 9,  # a ninth
    ["--dense-waves", "65537"],
    ["--dense-waves", "5", "--inject-dense", "f16:0"],
    ["--dense-waves", "5", "--min-dense-tflops", "f16:-1"],
    ["--dense-rate-instr", "0"],
])
def test_bad_dense_flags_exit_2(gpucheck, args):
    proc = subprocess.run([gpucheck, "--cpu", *args], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 2
    assert "usage:" in proc.stderr and "28 dense mismatch" in proc.stderr
    assert "29 dense rate" in proc.stderr
    assert proc.stdout == ""


def test_eight_injections_are_accepted(gpucheck):
    rc, out = run_cpu(gpucheck, "--dense-waves", 1,
                      *ref.dense_inject_args("f32", ["0:1023"] * 8))
    assert rc == 28 and out["dense_formats"]["f32"]["bad_waves"] == 1


def test_runner_maps_exit_28(gpucheck, synthetic_ledger):
    assert EXIT_STAGES[28] == "dense" and EXIT_STAGES[29] == "dense_rate"
    res = run_gpucheck(0, synthetic_ledger.inventory, nbytes=4096,
                       timeout_s=30, binary=gpucheck,
                       extra_args=["--cpu", "--dense-waves", "5",
                                   "--inject-dense", "bf8:3:9"])
    assert not res.ok and res.exit_code == 28 and res.reason == "dense"
    assert first_bad_dense(res.data) == "bf8 wave 3"   # --cpu: no where


def test_first_bad_dense():
    assert first_bad_dense({}) == ""
    assert first_bad_dense({"dense_formats": DENSE_FORMATS_OK}) == ""
    formats = dict(DENSE_FORMATS_OK)
    formats["f64"] = {"bad_waves": 2, "first_bad_wave": 9,
                      "first_bad_where": "xcc1.se2.sh0.cu3", "tflops": 1.0}
    assert first_bad_dense({"dense_formats": formats}) == \
        "f64 wave 9 on xcc1.se2.sh0.cu3"


def test_operator_cli_passes_dense_floor(gpucheck, capsys):
    from k8s_runpod_kubelet_amd.gpu import diagnostics

    code = diagnostics.main(["--gpu", "0", "--bytes", "4K",
                             "--sysfs-root", "/nonexistent-sysfs",
                             "--min-dense-tflops", "f16:100",
                             "--", "--cpu", "--dense-waves", "2",
                             "--inject-dense", "i8:1:0"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert code == 28 and out["reason"] == "dense"
    assert out["dense_formats"]["i8"]["first_bad_wave"] == 1
    # the floor reaches the binary as given: an MX format is a usage error
    code = diagnostics.main(["--gpu", "0", "--bytes", "4K", "--sysfs-root",
                             "/nonexistent-sysfs", "--min-dense-tflops",
                             "fp4:1", "--", "--cpu"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert code != 0 and out["exit_code"] == 2


# ---------------------------------------------- manager, config, metrics

DENSE_FORMATS_OK = {name: {"bad_waves": 0, "first_bad_wave": -1,
                           "first_bad_where": "", "tflops": 100.0 + i}
                    for i, name in enumerate(ref.FORMAT_NAMES)}
GOOD = {"tool": "gpucheck", "ok": True, "exit_code": 0, "dense": "pass",
        "dense_rate": "pass", "dense_waves": 1024,
        "dense_formats": DENSE_FORMATS_OK}


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


def test_dense_floor_args():
    assert dense_floor_args(None) == [] and dense_floor_args({}) == []
    assert dense_floor_args({"f64": 40, "f16": 1200.5, "i8": 0}) == [
        "--min-dense-tflops", "f16:1200.5", "--min-dense-tflops", "f64:40.0"]
    with pytest.raises(ValueError):
        dense_floor_args({"fp4": 1})


def test_config_defaults_and_manager_flags(manager):
    mgr, runner, _, _ = manager
    assert Config().gpu_check_dense is True
    assert Config().gpu_check_min_dense_tflops == {}
    mgr.check(0)
    assert runner.calls[-1] == ()
    mgr.config.gpu_check_min_dense_tflops = {"f16": 1200, "bf16x16": 900.5,
                                             "f32": 0}
    mgr.config.gpu_check_min_mx_tflops = {"fp4": 4000}
    mgr.check(0)
    assert runner.calls[-1] == ("--min-mx-tflops", "fp4:4000.0",
                                "--min-dense-tflops", "f16:1200.0",
                                "--min-dense-tflops", "bf16x16:900.5")
    mgr.config.gpu_check_dense = False  # the floors go with the stage
    mgr.check(0)
    assert runner.calls[-1] == ("--min-mx-tflops", "fp4:4000.0",
                                "--dense-waves", "0")


def test_manager_flags_are_accepted_by_the_binary(gpucheck):
    floors = {name: 1.5 + i for i, name in enumerate(DENSE_FORMATS)}
    proc = subprocess.run(
        [gpucheck, "--cpu", "--bytes", "4096", *dense_floor_args(floors),
         "--dense-waves", "0"], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr


@pytest.mark.parametrize("code,reason", [(28, "dense"), (29, "dense_rate")])
def test_manager_dense_failure_fences_and_names_the_wave(manager, code,
                                                         reason):
    mgr, runner, rec, ledger = manager
    formats = dict(DENSE_FORMATS_OK)
    data = dict(GOOD, ok=False, exit_code=code, failed_stages=[reason])
    if reason == "dense":
        formats["i8"] = {"bad_waves": 3, "first_bad_wave": 17,
                         "first_bad_where": "xcc2.se1.sh0.cu5", "tflops": 9.0}
        data.update(dense="fail", dense_formats=formats)
    else:
        data.update(dense_rate="fail")
    runner.result = (code, reason, data)
    res = mgr.check(2)
    assert not res.ok and res.reason == reason
    assert not ledger.states[2].schedulable
    assert ledger.states[2].gpu.diag_reason == reason
    (etype, why, message), = rec.events
    assert etype == "Warning" and why == "GpuCheckFailed"
    assert f"stage={reason}" in message
    assert ("first_bad_dense=i8 wave 17 on xcc2.se1.sh0.cu5" in message) == \
        (reason == "dense")


def test_metrics_gauge(manager):
    from k8s_runpod_kubelet_amd.server import metrics

    mgr, runner, _, _ = manager
    mgr.check(5)
    text = metrics.render().decode()
    for i, name in enumerate(ref.FORMAT_NAMES):
        assert (f'amdvk_gpu_check_dense_tflops{{format="{name}",gpu="5"}} '
                f'{100.0 + i}') in text
    # a run without rates (stage off, or --cpu) sets nothing
    runner.result = (0, "", dict(GOOD, dense="skipped",
                                 dense_rate="skipped"))
    mgr.check(6)
    assert 'gpu="6"}' not in "\n".join(
        ln for ln in metrics.render().decode().splitlines()
        if ln.startswith("amdvk_gpu_check_dense_tflops"))


def test_cli_and_provider_config(tmp_path):
    from k8s_runpod_kubelet_amd.cli import build_parser, parse_dense_floors

    args = build_parser().parse_args([])
    assert args.gpu_check_dense is None
    assert args.gpu_check_min_dense_tflops is None
    args = build_parser().parse_args([
        "--no-gpu-check-dense", "--gpu-check-min-dense-tflops", "f16:1200",
        "--gpu-check-min-dense-tflops", "f64:40"])
    assert args.gpu_check_dense is False
    assert parse_dense_floors(args.gpu_check_min_dense_tflops, {"i8": 5}) == {
        "i8": 5, "f16": 1200.0, "f64": 40.0}
    with pytest.raises(SystemExit):
        parse_dense_floors(["fp4:1"])
    with pytest.raises(SystemExit):
        parse_dense_floors(["f16"])
    path = tmp_path / "provider.yaml"
    path.write_text("gpu_check_dense: false\n"
                    "gpu_check_min_dense_tflops:\n  f16: 1200\n  i8: 2500\n")
    cfg = load_config(str(path))
    assert cfg.gpu_check_dense is False
    assert cfg.gpu_check_min_dense_tflops == {"f16": 1200, "i8": 2500}
    path.write_text("gpu_check_min_dense_tflops:\n")
    assert load_config(str(path)).gpu_check_min_dense_tflops == {}
    for bad in ("gpu_check_min_dense_tflops: 7\n",
                "gpu_check_min_dense_tflops:\n  fp4: 1\n",    # an MX format
                "gpu_check_min_dense_tflops:\n  f16: fast\n"):
        path.write_text(bad)
        with pytest.raises(ValueError):
            load_config(str(path))


def test_chart_comments_name_the_keys():
    text = (REPO / "helm/amd-virtual-kubelet/values.yaml").read_text()
    lines = text.splitlines()
    at = {key: next(i for i, ln in enumerate(lines) if f"#   {key}:" in ln)
          for key in ("gpu_check_min_mx_tflops", "gpu_check_dense",
                      "gpu_check_min_dense_tflops", "gpu_check_lds")}
    assert at["gpu_check_min_mx_tflops"] < at["gpu_check_dense"] \
        < at["gpu_check_min_dense_tflops"] < at["gpu_check_lds"]
    block = lines[at["gpu_check_min_dense_tflops"] + 1:at["gpu_check_lds"]]
    assert [ln.split("#")[1].strip() for ln in block] == \
        [f"{name}: 0" for name in DENSE_FORMATS]
