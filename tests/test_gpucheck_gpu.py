"""Active GPU self-test on a real MI355X: the gpucheck binary's HBM, copy
bandwidth and MFMA stages, and one end-to-end check through the
DiagnosticsManager followed by a pod on the checked GPU.

Every test starts the binary as a child with a 60 s limit of its own. Once a
child ends with a HIP error (11), a signal or its time limit, the remaining
gpucheck GPU tests skip (tests/gpucheck_helpers.py): nothing more is started
on a card that may be in trouble."""

import json
import math
import subprocess
import time

import pytest

from tests import gpucheck_reference as ref
from tests.gpucheck_helpers import (  # noqa: F401 (fixtures)
    CHILD_TIMEOUT_S, _card_suspect, _stop_after_trouble, binary, run_gpu)

pytestmark = pytest.mark.gpu

MIB = 1024**2
GIB = 1024**3

GRID = ref.GRID                # vectors in one trip of a full grid

HBM_SIZES = [
    16,                        # a single vector
    32,                        # two vectors: the smallest copy
    16 * 255,                  # one partial workgroup; 127 copied, one over
    16 * (GRID + 1),           # one vector past a full grid: a second trip
    16 * (2 * GRID + 3),       # the copy takes a second trip, one vector over
    64 * MIB + 16,
    4 * GIB + 32,              # byte offsets past 2**32
]


def expect_vector_dump(out, indices, seed=ref.DEFAULT_SEED):
    """vector_dump is what the region holds after the last pass, read back
    with a plain copy; the reference is the Python port of the pattern."""
    last = out["passes"] - 1
    assert out["vector_dump"] == [
        {"index": i, "pass": last,
         "value": ref.pattern(seed, last, out["base_index"] + i)}
        for i in indices]


@pytest.mark.parametrize("nbytes", HBM_SIZES)
def test_hbm_clean(binary, nbytes):
    args = ["--bytes", nbytes, "--mfma-waves", 1]
    # The vectors around byte offset 2**32 ride in the 4 GiB child that runs
    # anyway: a second child of that size would double its cost.
    around_4gib = [2**28 - 1, 2**28, 2**28 + 1]
    if nbytes == 4 * GIB + 32:
        args += ["--dump-vectors", ",".join(map(str, around_4gib))]
    rc, out, _ = run_gpu(binary, *args)
    assert rc == 0, out
    if nbytes == 4 * GIB + 32:
        expect_vector_dump(out, around_4gib)
    # the copied half was verified against the pattern, not only timed
    assert out["copy"] == ("pass" if nbytes >= 32 else "skipped")
    assert out["copy_mismatch_vectors"] == 0
    assert out["copy_first_bad_offset"] is None
    assert out["bandwidth"] == out["copy"]
    if nbytes >= 32:
        assert math.isfinite(out["copy_gbs"]) and out["copy_gbs"] > 0
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
    """The GPU run over a base index that crosses 2**32 verifies clean, that
    is, hbm_fill and hbm_verify agree with each other. pattern_dump is
    computed on the host in both modes, so its comparison only shows that the
    two modes print the same host values; what the device stored is compared
    with an independent reference in test_stored_vectors_match_reference."""
    args = ["--bytes", 4096, "--base-index", 2**32 - 3, "--mfma-waves", 1,
            "--dump-pattern"]
    rc, gpu, _ = run_gpu(binary, *args)
    assert rc == 0 and gpu["mismatch_vectors"] == 0
    cpu = subprocess.run([binary, "--cpu", *map(str, args)],
                         capture_output=True, text=True, timeout=60)
    assert cpu.returncode == 0
    assert json.loads(cpu.stdout.splitlines()[-1])["pattern_dump"] \
        == gpu["pattern_dump"]


# The logical index crosses 2**32 inside the first workgroup; 255/256 is a
# wave and workgroup edge; GRID is the first vector of the second trip.
DUMP_REGION = 16 * (GRID + 1)
DUMP_BASE = 2**32 - 3
DUMP_INDICES = [0, 2, 3, 255, 256, GRID - 1, GRID]


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("variant", ["auto", "plain", "nontemporal"])
def test_stored_vectors_match_reference(binary, variant, passes):
    """What each fill kernel left in device memory, read back with hipMemcpy,
    against the Python port of the pattern. --passes 2 checks the complement
    as stored; a forced variant checks that fill kernel on its own."""
    rc, out, _ = run_gpu(
        binary, "--bytes", DUMP_REGION, "--base-index", DUMP_BASE,
        "--passes", passes, "--store-variant", variant, "--mfma-waves", 1,
        "--dump-vectors", ",".join(map(str, DUMP_INDICES)))
    assert rc == 0, out
    assert out["mismatch_vectors"] == 0 and out["copy_mismatch_vectors"] == 0
    expect_vector_dump(out, DUMP_INDICES)
    if variant == "auto":
        assert out["store_variant"] in ("plain", "nontemporal")
        assert out["write_gbs_plain"] > 0 and out["write_gbs_nontemporal"] > 0
    else:
        other = "nontemporal" if variant == "plain" else "plain"
        assert out["store_variant"] == variant
        assert out[f"write_gbs_{variant}"] > 0
        assert out[f"write_gbs_{other}"] == 0


COPY_FLIP_REGION = 16 * (2 * GRID + 3)   # destination half: vectors
COPY_HALF = (2 * GRID + 3) // 2          # COPY_HALF .. 2*COPY_HALF-1


@pytest.mark.parametrize("offset,bit", [
    (16 * COPY_HALF, 0),                 # first byte of the destination half
    (16 * 2 * COPY_HALF - 1, 7),         # its last byte, on the second trip
])
def test_copy_mismatch_is_caught_and_localised(binary, offset, bit):
    rc, out, _ = run_gpu(binary, "--bytes", COPY_FLIP_REGION,
                         "--mfma-waves", 1,
                         "--inject-copy-flip", f"{offset}:{bit}")
    assert rc == 23, out
    assert out["ok"] is False and out["failed_stages"] == ["copy"]
    assert out["copy"] == "fail" and out["copy_mismatch_vectors"] == 1
    assert out["copy_first_bad_offset"] == offset - offset % 16
    assert int(out["copy_first_bad_xor"], 16) == \
        1 << (8 * (offset % 16) + bit)
    assert out["hbm"] == "pass" and out["mismatch_vectors"] == 0
    assert out["mfma"] == "pass"
    assert math.isfinite(out["copy_gbs"]) and out["copy_gbs"] > 0


@pytest.mark.parametrize("case", sorted(ref.MULTI_FLIP_CASES))
def test_hbm_multiple_flips_count_and_minimum(binary, case):
    flips = ref.MULTI_FLIP_CASES[case]
    rc, out, _ = run_gpu(binary, "--bytes", ref.MULTI_FLIP_REGION,
                         "--mfma-waves", 1, *ref.flip_args(flips))
    assert rc == 20, out
    ref.expect_flips(out, flips)
    if case == "seven-descending":
        assert out["mismatch_vectors"] == 6
    # pass 1 rewrote everything, so the copy of the last pass is clean
    assert out["copy"] == "pass" and out["mfma"] == "pass"


def test_hbm_flip_on_a_complement_pass(binary):
    flips = [(16 * (GRID + 7) + 4, 5)]
    rc, out, _ = run_gpu(binary, "--bytes", ref.MULTI_FLIP_REGION,
                         "--mfma-waves", 1, "--passes", 3, "--inject-pass", 1,
                         *ref.flip_args(flips))
    assert rc == 20, out
    ref.expect_flips(out, flips, pass_=1)  # the XOR is against the complement


def test_hbm_counts_add_across_passes(binary):
    """One flip at pass 0, nothing at pass 1: the total stays 1."""
    flips = [(16 * 300, 0)]
    rc, out, _ = run_gpu(binary, "--bytes", ref.MULTI_FLIP_REGION,
                         "--mfma-waves", 1, "--passes", 2, "--inject-pass", 0,
                         *ref.flip_args(flips))
    assert rc == 20, out
    ref.expect_flips(out, flips)
    assert out["mismatch_vectors"] == 1


@pytest.mark.parametrize("injections,bad,first", ref.MFMA_INJECT_CASES)
def test_mfma_injection_is_caught(binary, injections, bad, first):
    """The host comparison over tiles the real kernel produced."""
    rc, out, _ = run_gpu(binary, "--bytes", 4096, "--mfma-waves", 5,
                         *ref.mfma_inject_args(injections))
    assert rc == 21, out
    assert out["ok"] is False and out["failed_stages"] == ["mfma"]
    assert out["mfma"] == "fail" and out["mfma_waves"] == 5
    assert out["mfma_bad_waves"] == bad
    assert out["mfma_first_bad_wave"] == first
    assert out["hbm"] == "pass" and out["copy"] == "pass"


_seen = {}  # compute_units, once a child has reported it


@pytest.mark.parametrize("wave", [0, 4])
def test_mfma_tile_matches_reference(binary, wave):
    """The tile as copied back from the device against numpy's product of the
    reference operands: a wrong lane-to-element mapping or accumulator layout
    shows here even if kernel and host checker share it. Wave 4 of 5 is the
    lone wave of a second workgroup."""
    rc, out, _ = run_gpu(binary, "--bytes", 4096, "--mfma-waves", 5,
                         "--dump-mfma-tile", wave)
    assert rc == 0, out
    _seen["compute_units"] = out["compute_units"]
    assert out["mfma_tile"]["wave"] == wave
    assert out["mfma_tile"]["values"] == \
        ref.mfma_tile(ref.DEFAULT_SEED, wave).reshape(-1).tolist()


def test_mfma_tile_of_last_default_wave_matches_reference(binary):
    if "compute_units" not in _seen:  # run alone: ask the device first
        _, out, _ = run_gpu(binary, "--bytes", 16, "--mfma-waves", 1)
        _seen["compute_units"] = out["compute_units"]
    wave = 8 * _seen["compute_units"] - 1
    rc, out, _ = run_gpu(binary, "--bytes", 4096, "--dump-mfma-tile", wave)
    assert rc == 0, out
    assert out["mfma_waves"] == wave + 1 and out["mfma"] == "pass"
    assert out["mfma_tile"]["wave"] == wave
    assert out["mfma_tile"]["values"] == \
        ref.mfma_tile(ref.DEFAULT_SEED, wave).reshape(-1).tolist()


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
