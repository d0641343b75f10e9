"""gpucheck's LDS stage — everything that needs no GPU: ``--cpu --lds-groups``
(the write order, the rotated read, the injection, the record and the merge
by compute unit against the independent reference, the JSON, exit codes 26
and 27 and their order), and the manager, config, CLI, metrics and chart
plumbing with a fake runner."""

import json
import os
import subprocess
import time

import pytest

from k8s_runpod_kubelet_amd.config import Config, load_config
from k8s_runpod_kubelet_amd.gpu.diagnostics import (
    EXIT_STAGES, DiagnosticsManager, GpuCheckResult, first_bad_lds,
    run_gpucheck)
from tests import gpucheck_helpers
from tests import gpucheck_lds_reference as ref
from tests.gpucheck_helpers import gpucheck  # noqa: F401 (fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = ref.DEFAULT_SEED


def run_cpu(binary, *args):
    return gpucheck_helpers.run_cpu(binary, "--bytes", 4096, *args)


# ------------------------------------------------------------ reference

def test_reference_fnv_and_injection_arithmetic():
    # published FNV-1a 64 test vectors
    assert ref.fnv1a64(b"") == 0xCBF29CE484222325
    assert ref.fnv1a64(b"a") == 0xAF63DC4C8601EC8C
    assert ref.fnv1a64(b"foobar") == 0x85944171F73967E8
    assert ref.expected_injection(0, 0) == (0, 1)
    assert ref.expected_injection(65536, 0) == (65536, 1)
    assert ref.expected_injection(163839, 7) == (163824, 1 << 127)
    assert ref.expected_injection(21, 3) == (16, 1 << 43)
    assert ref.LDS_BYTES == 163840


def test_reference_pattern_properties():
    """Pass 1 complements pass 0; no 64 KiB alias; every group and round has
    its own values."""
    mask = (1 << 128) - 1
    for i in ref.DUMP_VECTORS:
        assert ref.vector_int(SEED, 0, 0, 1, i) == \
            ref.vector_int(SEED, 0, 0, 0, i) ^ mask
    assert ref.vector(SEED, 0, 0, 0, 0) != ref.vector(SEED, 0, 0, 0, 4096)
    assert ref.vector(SEED, 0, 0, 0, 7) != ref.vector(SEED, 1, 0, 0, 7)
    assert ref.vector(SEED, 0, 0, 0, 7) != ref.vector(SEED, 0, 1, 0, 7)


# ------------------------------------------------------- binary, --cpu

@pytest.mark.parametrize("pass_", [0, 1])
@pytest.mark.parametrize("round_", [0, 1])
@pytest.mark.parametrize("group", [0, 2])
def test_cpu_lds_dump_matches_reference(gpucheck, group, round_, pass_):
    rc, out = run_cpu(gpucheck, "--lds-groups", 3, "--lds-rounds", 2,
                      "--dump-lds", f"{group}:{round_}:{pass_}")
    assert rc == 0, out
    assert out["lds"] == "pass" and out["lds_groups"] == 3
    assert out["lds_rounds"] == 2 and out["lds_launches"] == 1
    assert out["lds_bytes_per_cu"] == 163840
    assert out["lds_bad_groups"] == 0 and out["lds_bad_cus"] == []
    assert out["lds_dump"] == ref.dump(SEED, group, round_, pass_)


def test_cpu_lds_dumps_differ_where_they_must(gpucheck):
    def dump(spec):
        rc, out = run_cpu(gpucheck, "--lds-groups", 3, "--lds-rounds", 2,
                          "--dump-lds", spec)
        assert rc == 0
        return out["lds_dump"]

    base, comp = dump("0:0:0"), dump("0:0:1")
    mask = (1 << 128) - 1
    for i, value in base["vectors"].items():
        assert int(comp["vectors"][i], 16) == int(value, 16) ^ mask
    assert base["vectors"]["0"] != base["vectors"]["4096"]
    assert base["vectors"]["1"] != base["vectors"]["4097"]
    for other in ("2:0:0", "0:1:0"):  # another group, another round
        got = dump(other)
        assert got["fnv64"] != base["fnv64"]
        assert all(got["vectors"][i] != base["vectors"][i]
                   for i in base["vectors"])


def test_cpu_lds_follows_the_seed(gpucheck):
    seed = 0x0123456789ABCDEF
    rc, out = run_cpu(gpucheck, "--lds-groups", 2, "--lds-rounds", 1,
                      "--seed", seed, "--dump-lds", "1:0:1")
    assert rc == 0
    assert out["lds_dump"] == ref.dump(seed, 1, 0, 1)


@pytest.mark.parametrize("round_,pass_", [(0, 0), (0, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize("byte,bit", ref.INJECT_POSITIONS)
def test_cpu_lds_injection_is_located(gpucheck, byte, bit, round_, pass_):
    rc, out = run_cpu(gpucheck, "--lds-groups", 4, "--lds-rounds", 3,
                      *ref.inject_args([(3, round_, pass_, byte, bit)]))
    assert rc == 26, out
    assert out["ok"] is False and out["exit_code"] == 26
    assert out["failed_stages"] == ["lds"] and out["lds"] == "fail"
    assert out["lds_bad_groups"] == 1
    (cu,) = out["lds_bad_cus"]
    offset, xor = ref.expected_injection(byte, bit)
    assert cu["first_bad_offset"] == offset
    assert len(cu["first_bad_xor"]) == 32
    assert int(cu["first_bad_xor"], 16) == xor
    assert cu["round"] == round_ and cu["pass"] == pass_
    assert cu["bad_vectors"] == 1
    assert cu["key"] == 3 and cu["where"] == ref.where_name(3)
    assert out["hbm"] == "pass" and out["mfma"] == "skipped"


def test_cpu_two_injections_in_one_group_report_the_lowest(gpucheck):
    """Listed highest first: the order of (round, pass, offset) decides."""
    rc, out = run_cpu(gpucheck, "--lds-groups", 2, "--lds-rounds", 2,
                      *ref.inject_args([(1, 1, 0, 32, 1), (1, 0, 1, 70001, 5)]))
    assert rc == 26
    (cu,) = out["lds_bad_cus"]
    assert cu["bad_vectors"] == 2 and out["lds_bad_groups"] == 1
    offset, xor = ref.expected_injection(70001, 5)
    assert (cu["round"], cu["pass"], cu["first_bad_offset"]) == (0, 1, offset)
    assert int(cu["first_bad_xor"], 16) == xor
    # the same round and pass: the lower offset; two bits of one vector
    rc, out = run_cpu(gpucheck, "--lds-groups", 2, "--lds-rounds", 2,
                      *ref.inject_args([(0, 1, 1, 4096 * 16 + 3, 2),
                                        (0, 1, 1, 4095 * 16 + 15, 7),
                                        (0, 1, 1, 4095 * 16, 0)]))
    (cu,) = out["lds_bad_cus"]
    assert cu["bad_vectors"] == 2
    assert cu["first_bad_offset"] == 4095 * 16
    assert int(cu["first_bad_xor"], 16) == (1 << 127) | 1


def test_cpu_groups_on_one_cu_merge(gpucheck):
    """Groups 1 and 6 both report compute unit 1 (group % 5)."""
    rc, out = run_cpu(gpucheck, "--lds-groups", 7, "--lds-rounds", 1,
                      "--dump-lds-where",
                      *ref.inject_args([(6, 0, 0, 160, 4), (1, 0, 1, 48, 0),
                                        (3, 0, 0, 16, 0)]))
    assert rc == 26
    assert out["lds_bad_groups"] == 3 and out["lds_cus_covered"] == 5
    by_key = {cu["key"]: cu for cu in out["lds_bad_cus"]}
    assert sorted(by_key) == [1, 3]
    assert by_key[1]["bad_vectors"] == 2
    assert (by_key[1]["round"], by_key[1]["pass"],
            by_key[1]["first_bad_offset"]) == (0, 0, 160)
    assert int(by_key[1]["first_bad_xor"], 16) == 1 << 4
    assert by_key[3]["bad_vectors"] == 1
    assert len(out["lds_where"]) == 7
    for group, waves in enumerate(out["lds_where"]):
        assert [w[0] for w in waves] == [group % 5] * 4
        assert [w[1] for w in waves] == [0, 1, 2, 3]


def test_cpu_failure_order(gpucheck):
    """20 and 21 before 26; failed_stages lists all in that order."""
    inj = ref.inject_args([(0, 0, 0, 0, 0)])
    rc, out = run_cpu(gpucheck, "--lds-groups", 1, "--mfma-waves", 2,
                      "--inject-mfma", "1:0", *inj)
    assert rc == 21 and out["failed_stages"] == ["mfma", "lds"]
    rc, out = run_cpu(gpucheck, "--lds-groups", 1, "--passes", 1,
                      "--inject-flip", "0:0", *inj)
    assert rc == 20 and out["failed_stages"] == ["hbm", "lds"]
    rc, out = run_cpu(gpucheck, "--lds-groups", 1, "--mx-waves", 1,
                      "--inject-mx", "fp4:0:0", *inj)
    assert rc == 24 and out["failed_stages"] == ["mx", "lds"]
    rc, out = run_cpu(gpucheck, "--lds-groups", 1, "--mfma-waves", 2, *inj)
    assert rc == 26 and out["failed_stages"] == ["lds"]


@pytest.mark.parametrize("args", [[], ["--lds-groups", 0]])
def test_cpu_lds_skipped(gpucheck, args):
    rc, out = run_cpu(gpucheck, *args)
    assert rc == 0 and out["ok"] is True
    assert out["lds"] == "skipped" and out["lds_groups"] == 0
    assert out["lds_launches"] == 0 and out["lds_cus_covered"] == 0
    assert out["lds_bad_cus"] == [] and "lds_dump" not in out
    assert "lds_where" not in out
    # the location keys of the other stages, without a device
    assert out["mfma_cus_covered"] == 0 and out["mfma_simds_covered"] == 0
    assert out["mfma_first_bad_where"] == ""
    assert out["mx_cus_covered"] == 0 and out["mx_simds_covered"] == 0
    assert all(f["first_bad_where"] == "" for f in out["mx_formats"].values())


@pytest.mark.parametrize("groups", [0, 3])
def test_cpu_never_fails_coverage(gpucheck, groups):
    rc, out = run_cpu(gpucheck, "--lds-groups", groups,
                      "--lds-require-coverage")
    assert rc == 0 and out["ok"] is True and out["compute_units"] == 0
    assert out["lds_cus_covered"] == min(groups, 5)
    if groups:
        assert out["lds_coverage"] == "full"


@pytest.mark.parametrize("args", [
    ["--lds-groups", "3", "--inject-lds", "3:0:0:0:0"],      # group >= groups
    ["--lds-groups", "3", "--lds-rounds", "2", "--inject-lds", "0:2:0:0:0"],
    ["--lds-groups", "3", "--inject-lds", "0:0:2:0:0"],      # pass > 1
    ["--lds-groups", "3", "--inject-lds", "0:0:0:163840:0"],  # byte
    ["--lds-groups", "3", "--inject-lds", "0:0:0:0:8"],      # bit
    ["--lds-groups", "3"] + ["--inject-lds", "0:0:0:0:0"] * 5,  # a fifth
    ["--lds-groups", "3", "--inject-lds", "0:0:0:0"],        # four fields
    ["--lds-groups", "3", "--inject-lds", "0:0:0:0:0:0"],
    ["--lds-groups", "3", "--dump-lds", "3:0:0"],            # no such group
    ["--lds-groups", "3", "--lds-rounds", "2", "--dump-lds", "0:2:0"],
    ["--lds-groups", "3", "--dump-lds", "0:0:2"],
    ["--lds-groups", "3", "--dump-lds", "0:0"],
    ["--dump-lds", "0:0:0"],                                 # --cpu: no group
    ["--inject-lds", "0:0:0:0:0"],
    ["--lds-groups", "0", "--inject-lds", "0:0:0:0:0"],
    ["--lds-groups", "-1"],
    ["--lds-groups", "65537"],
    ["--lds-rounds", "0"],
    ["--lds-max-launches", "0"],
    ["--lds-groups"],
])
def test_bad_lds_flags_exit_2(gpucheck, args):
    proc = subprocess.run([gpucheck, "--cpu", *args], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 2
    assert "usage:" in proc.stderr and "26 LDS mismatch" in proc.stderr
    assert "27 LDS coverage" in proc.stderr
    assert proc.stdout == ""


def test_runner_maps_exit_26(gpucheck, synthetic_ledger):
    assert EXIT_STAGES[26] == "lds" and EXIT_STAGES[27] == "lds_coverage"
    res = run_gpucheck(0, synthetic_ledger.inventory, nbytes=4096,
                       timeout_s=30, binary=gpucheck,
                       extra_args=["--cpu", "--lds-groups", "3",
                                   "--lds-rounds", "1",
                                   *ref.inject_args([(2, 0, 0, 65536, 0)])])
    assert not res.ok and res.exit_code == 26 and res.reason == "lds"
    assert first_bad_lds(res.data) == \
        "xcc0.se0.sh0.cu2 offset 65536 xor " + "0" * 31 + "1"
    assert first_bad_lds({}) == "" and first_bad_lds({"lds_bad_cus": []}) == ""


def test_operator_cli_lds_flags(gpucheck, capsys):
    from k8s_runpod_kubelet_amd.gpu import diagnostics

    base = ["--gpu", "0", "--bytes", "4K", "--sysfs-root", "/nonexistent-sysfs"]
    code = diagnostics.main(base + ["--lds-require-coverage", "--", "--cpu",
                                    "--lds-groups", "2", "--lds-rounds", "1",
                                    "--inject-lds", "1:0:1:5:5"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert code == 26 and out["reason"] == "lds"
    assert out["lds_bad_cus"][0]["first_bad_offset"] == 0
    # --no-lds comes after the pass-through arguments and wins
    code = diagnostics.main(base + ["--no-lds", "--", "--cpu",
                                    "--lds-groups", "2"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert code == 0 and out["lds"] == "skipped"


# ---------------------------------------------- manager, config, metrics

BAD_CU = {"where": "xcc2.se1.sh0.cu5", "key": 0x225, "bad_vectors": 3,
          "first_bad_offset": 65536,
          "first_bad_xor": "0" * 31 + "1", "round": 1, "pass": 0}
GOOD = {"tool": "gpucheck", "ok": True, "exit_code": 0, "mfma": "pass",
        "mfma_cus_covered": 256, "mfma_simds_covered": 1019, "lds": "pass",
        "lds_cus_covered": 256, "lds_coverage": "full", "lds_bad_groups": 0,
        "lds_bad_cus": []}


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


LDS_ARG_CASES = [
    (True, False, ()),
    (False, False, ("--lds-groups", "0")),
    (True, True, ("--lds-require-coverage",)),
    (False, True, ("--lds-groups", "0", "--lds-require-coverage")),
]


@pytest.mark.parametrize("lds,require,want", LDS_ARG_CASES)
def test_manager_flags(manager, gpucheck, lds, require, want):
    mgr, runner, _, _ = manager
    assert Config().gpu_check_lds is True
    assert Config().gpu_check_lds_require_coverage is False
    mgr.config.gpu_check_lds = lds
    mgr.config.gpu_check_lds_require_coverage = require
    mgr.check(0)
    assert runner.calls[-1] == want
    # after the MX arguments
    mgr.config.gpu_check_mx = False
    mgr.config.gpu_check_min_copy_gbs = 1500.0
    mgr.check(0)
    assert runner.calls[-1] == ("--min-copy-gbs", "1500.0", "--mx-waves", "0",
                                *want)
    proc = subprocess.run([gpucheck, "--cpu", "--bytes", "4096",
                           *runner.calls[-1]],
                          capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr
    assert json.loads(proc.stdout.splitlines()[-1])["lds"] == "skipped"


@pytest.mark.parametrize("code,reason", [(26, "lds"), (27, "lds_coverage")])
def test_manager_lds_failure_fences_and_names_the_cu(manager, code, reason):
    mgr, runner, rec, ledger = manager
    data = dict(GOOD, ok=False, exit_code=code, failed_stages=[reason])
    if reason == "lds":
        data.update(lds="fail", lds_bad_groups=1, lds_bad_cus=[BAD_CU])
    else:
        data.update(lds_cus_covered=255, lds_coverage="partial")
    runner.result = (code, reason, data)
    res = mgr.check(2)
    assert not res.ok and res.reason == reason
    assert not ledger.states[2].schedulable
    assert ledger.states[2].gpu.diag_reason == reason
    (etype, why, message), = rec.events
    assert etype == "Warning" and why == "GpuCheckFailed"
    assert f"stage={reason}" in message
    text = "lds: xcc2.se1.sh0.cu5 offset 65536 xor " + "0" * 31 + "1"
    assert (text in message) == (reason == "lds")


def test_metrics_gauges(manager):
    from k8s_runpod_kubelet_amd.server import metrics

    mgr, runner, _, _ = manager
    mgr.check(5)
    text = metrics.render().decode()
    assert 'amdvk_gpu_check_lds_cus_covered{gpu="5"} 256.0' in text
    assert 'amdvk_gpu_check_lds_bad_cus{gpu="5"} 0.0' in text
    assert 'amdvk_gpu_check_mfma_simds_covered{gpu="5"} 1019.0' in text
    runner.result = (26, "lds", dict(GOOD, ok=False, lds="fail",
                                     lds_bad_cus=[BAD_CU]))
    mgr.check(5)
    assert 'amdvk_gpu_check_lds_bad_cus{gpu="5"} 1.0' in \
        metrics.render().decode()
    # a run without the stages sets nothing
    runner.result = (0, "", dict(GOOD, lds="skipped", mfma="skipped",
                                 lds_cus_covered=0, mfma_simds_covered=0))
    mgr.check(6)
    assert not [ln for ln in metrics.render().decode().splitlines()
                if 'gpu="6"' in ln and ("_lds_" in ln or "_simds_" in ln)]


def test_cli_and_provider_config(tmp_path):
    from k8s_runpod_kubelet_amd.cli import build_parser

    args = build_parser().parse_args([])
    assert args.gpu_check_lds is None
    assert args.gpu_check_lds_require_coverage is None
    args = build_parser().parse_args(["--no-gpu-check-lds",
                                      "--gpu-check-lds-require-coverage"])
    assert args.gpu_check_lds is False
    assert args.gpu_check_lds_require_coverage is True
    path = tmp_path / "provider.yaml"
    path.write_text("gpu_check_lds: false\n"
                    "gpu_check_lds_require_coverage: true\n")
    cfg = load_config(str(path))
    assert cfg.gpu_check_lds is False
    assert cfg.gpu_check_lds_require_coverage is True


def test_chart_values_name_the_keys():
    with open(os.path.join(REPO, "helm", "amd-virtual-kubelet",
                           "values.yaml"), encoding="utf-8") as fh:
        text = fh.read()
    assert "gpu_check_lds: true" in text
    assert "gpu_check_lds_require_coverage: false" in text
    names = {f for f in Config.__dataclass_fields__}
    assert {"gpu_check_lds", "gpu_check_lds_require_coverage"} <= names
