"""Active GPU self-test on a real MI355X: the gpucheck binary's HBM, copy
bandwidth and MFMA stages, and one end-to-end check through the
DiagnosticsManager followed by a pod on the checked GPU.

Every test starts the binary as a child with a 60 s limit of its own. Once a
child ends with a HIP error (11), a signal or its time limit, the rest of the
file skips: nothing more is started on a card that may be in trouble."""

import json
import math
import os
import subprocess
import time

import pytest

pytestmark = pytest.mark.gpu

MIB = 1024**2
GIB = 1024**3
CHILD_TIMEOUT_S = 60

_card_suspect = []  # reason, once a child ended badly


@pytest.fixture(autouse=True)
def _stop_after_trouble():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no /dev/kfd on this box")
    if _card_suspect:
        pytest.skip(f"an earlier gpucheck child ended badly: {_card_suspect[0]}")


@pytest.fixture(scope="module")
def binary():
    from k8s_runpod_kubelet_amd.ops import gpucheck_binary

    return gpucheck_binary()


def run_gpu(binary, *args):
    """-> (exit code, parsed last stdout line, wall seconds)."""
    argv = [binary, *map(str, args)]
    t0 = time.monotonic()
    proc = subprocess.Popen(argv, stdin=subprocess.DEVNULL,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _card_suspect.append(f"timeout: {argv}")
        try:
            os.killpg(proc.pid, 9)
        except ProcessLookupError:
            pass
        proc.communicate()
        pytest.fail(f"gpucheck exceeded {CHILD_TIMEOUT_S} s: {argv}")
    wall = time.monotonic() - t0
    if proc.returncode == 11 or proc.returncode < 0:
        _card_suspect.append(f"exit {proc.returncode}: {argv}")
        pytest.fail(f"gpucheck exit {proc.returncode}: {argv}\n{out}\n{err}")
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert lines, err
    data = json.loads(lines[-1])
    print(f"{' '.join(map(str, args))} -> rc={proc.returncode} "
          f"wall={wall:.3f}s {lines[-1]}")
    return proc.returncode, data, wall


HBM_SIZES = [
    16,                        # a single vector
    16 * 255,                  # one partial workgroup
    16 * (2048 * 256 + 1),     # one vector past a full grid: a second trip
    64 * MIB + 16,
    4 * GIB + 32,              # byte offsets past 2**32
]


@pytest.mark.parametrize("nbytes", HBM_SIZES)
def test_hbm_clean(binary, nbytes):
    rc, out, _ = run_gpu(binary, "--bytes", nbytes, "--mfma-waves", 1)
    assert rc == 0, out
    assert out["mode"] == "gpu" and "gfx950" in out["device"]
    assert out["bytes"] == nbytes and out["vectors"] == nbytes // 16
    assert out["hbm"] == "pass" and out["mismatch_vectors"] == 0
    assert out["first_bad_offset"] is None
    assert out["store_variant"] in ("plain", "nontemporal")
    assert out["write_gbs_plain"] > 0 and out["write_gbs_nontemporal"] > 0


def test_hbm_flip_at_last_byte_past_4gib(binary):
    nbytes = 4 * GIB + 32
    rc, out, _ = run_gpu(binary, "--bytes", nbytes, "--mfma-waves", 1,
                         "--inject-flip", f"{nbytes - 1}:7")
    assert rc == 20, out
    assert out["failed_stages"] == ["hbm"]
    assert out["mismatch_vectors"] == 1
    assert out["first_bad_offset"] == nbytes - 16
    assert int(out["first_bad_xor"], 16) == 1 << 127
    assert out["first_bad_pass"] == 0
    assert out["mfma"] == "pass"  # later stages still ran and reported


def test_hbm_flip_at_offset_zero_of_one_vector(binary):
    rc, out, _ = run_gpu(binary, "--bytes", 16, "--mfma-waves", 1,
                         "--inject-flip", "0:0")
    assert rc == 20, out
    assert out["mismatch_vectors"] == 1
    assert out["first_bad_offset"] == 0
    assert int(out["first_bad_xor"], 16) == 1


def test_hbm_matches_cpu_pattern_at_high_base_index(binary):
    """Device and host compute the same pattern for indices above 2**32: the
    same flip reports the same XOR and offset in both modes, and the GPU run
    over a high base index verifies clean."""
    args = ["--bytes", 4096, "--base-index", 2**32 - 3, "--mfma-waves", 1,
            "--dump-pattern"]
    rc, gpu, _ = run_gpu(binary, *args)
    assert rc == 0 and gpu["mismatch_vectors"] == 0
    cpu = subprocess.run([binary, "--cpu", *map(str, args)],
                         capture_output=True, text=True, timeout=60)
    assert cpu.returncode == 0
    assert json.loads(cpu.stdout.splitlines()[-1])["pattern_dump"] \
        == gpu["pattern_dump"]


@pytest.mark.parametrize("waves", [1, 5, None])
def test_mfma_bit_exact(binary, waves):
    args = ["--bytes", 4096]
    if waves is not None:
        args += ["--mfma-waves", waves]
    rc, out, _ = run_gpu(binary, *args)
    assert rc == 0, out
    expect = waves if waves is not None else 8 * out["compute_units"]
    assert out["compute_units"] > 0
    assert out["mfma"] == "pass"
    assert out["mfma_waves"] == expect
    assert out["mfma_bad_waves"] == 0
    assert out["mfma_first_bad_wave"] == -1


def test_bandwidth_1gib(binary):
    rc, out, wall = run_gpu(binary, "--bytes", GIB, "--min-copy-gbs", 1)
    assert rc == 0, out
    for key in ("copy_gbs", "read_gbs", "write_gbs", "write_gbs_plain",
                "write_gbs_nontemporal"):
        assert math.isfinite(out[key]) and out[key] > 0, key
    assert out["write_gbs"] >= max(out["write_gbs_plain"],
                                   out["write_gbs_nontemporal"]) - 1e-3
    assert out["cache_resident"] is False
    assert out["bandwidth"] == "pass"


def test_bandwidth_64mib_is_cache_resident_and_floor_fails(binary):
    rc, out, _ = run_gpu(binary, "--bytes", 64 * MIB, "--min-copy-gbs", "1e9")
    assert rc == 22, out
    assert out["cache_resident"] is True
    assert out["failed_stages"] == ["bandwidth"]
    assert out["bandwidth"] == "fail"
    assert out["hbm"] == "pass" and out["mfma"] == "pass"
    assert math.isfinite(out["copy_gbs"]) and out["copy_gbs"] > 0


def test_check_then_pod_on_the_checked_gpu(tmp_path):
    from k8s_runpod_kubelet_amd.config import Config
    from k8s_runpod_kubelet_amd.gpu.diagnostics import DiagnosticsManager
    from k8s_runpod_kubelet_amd.gpu.inventory import Inventory
    from k8s_runpod_kubelet_amd.gpu.ledger import Ledger
    from k8s_runpod_kubelet_amd.runtime.process_runtime import ProcessRuntime
    from k8s_runpod_kubelet_amd.runtime.types import (
        ContainerSpec, DeployParams, PodStatus)

    inv = Inventory(sysfs_root="/sys", allow_synthetic=False)
    if not inv.discover():
        pytest.skip("KFD topology reports no GPUs")
    ledger = Ledger(inv)
    ledger.sync_inventory()
    cfg = Config(gpu_check_timeout_s=CHILD_TIMEOUT_S)
    mgr = DiagnosticsManager(ledger, inv, cfg)
    res = mgr.check(0)
    if res.reason in ("timeout", "hip") or res.reason.startswith("signal"):
        _card_suspect.append(f"manager check: {res.reason}")
    assert res.ok, res.to_dict()
    assert res.data["mismatch_vectors"] == 0
    assert res.data["mfma_bad_waves"] == 0
    assert res.data["bytes"] == GIB
    assert ledger.states[0].schedulable
    assert ledger.states[0].gpu.diag_last["ok"] is True
    assert not ledger.reservations

    for idx in ledger.states:  # the pod must land on the checked GPU
        if idx != 0:
            ledger.set_cordoned(idx, True)
    rt = ProcessRuntime(ledger, str(tmp_path), enable_cgroups=False)
    try:
        st = rt.deploy(DeployParams(
            pod_key="default-after-check", name="after-check", gpu_count=1,
            containers=[ContainerSpec(
                name="main", command=["podworker"],
                args=["--expect-gpus", "1", "--run-for", "0.1"])],
        ))
        assert st.gpu_indices == [0]
        deadline = time.time() + CHILD_TIMEOUT_S
        while time.time() < deadline:
            s = rt.get_detailed_status(st.id)
            if s.desired_status == PodStatus.EXITED:
                break
            time.sleep(0.05)
        assert s.desired_status == PodStatus.EXITED
        assert s.exit_code == 0, rt.get_logs(st.id)
    finally:
        rt.close()
