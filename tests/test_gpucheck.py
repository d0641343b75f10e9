"""Active GPU self-test — everything that needs no GPU: the gpucheck binary
in ``--cpu`` mode (CLI, JSON, exit codes, tail handling, 64-bit indices,
mismatch localisation), the child-process runner against stub executables,
the DiagnosticsManager gating placement, and the operator surfaces."""

import json
import os
import stat
import subprocess
import threading
import time
import urllib.error
import urllib.request

import pytest

from k8s_runpod_kubelet_amd.config import Config
from k8s_runpod_kubelet_amd.gpu.binder import Binder, BindRequest, PlacementError
from k8s_runpod_kubelet_amd.gpu.diagnostics import (
    DiagnosticsManager, GpuBusyError, GpuCheckResult, UnknownGpuError,
    run_gpucheck)
from tests import gpucheck_helpers
from tests import gpucheck_reference as ref
from tests.conftest import wait_until
from tests.gpucheck_helpers import gpucheck, run_cpu  # noqa: F401 (fixture)


# ------------------------------------------------------------------ binary

def test_builds_through_ops_build(gpucheck):
    from k8s_runpod_kubelet_amd.ops import build, gpucheck_binary

    assert gpucheck_binary() == gpucheck
    # the content stamp makes a second build a no-op
    before = os.stat(gpucheck).st_mtime_ns
    build.build_gpucheck()
    assert os.stat(gpucheck).st_mtime_ns == before


def test_cpu_clean_region_with_tail(gpucheck):
    rc, out = run_cpu(gpucheck, "--bytes", 4112)
    assert rc == 0
    assert out["ok"] is True and out["mode"] == "cpu"
    assert out["bytes"] == 4112 and out["vectors"] == 257
    assert out["mismatch_vectors"] == 0
    assert out["first_bad_offset"] is None
    # no GPU in --cpu mode: those stages are reported, not silently dropped
    assert out["mfma"] == "skipped" and out["bandwidth"] == "skipped"


def test_cpu_injected_flip_is_localised(gpucheck):
    rc, out = run_cpu(gpucheck, "--bytes", 4112, "--inject-flip", "4100:3")
    assert rc == 20
    assert out["ok"] is False and out["failed_stages"] == ["hbm"]
    assert out["mismatch_vectors"] == 1
    assert out["first_bad_offset"] == 4096
    assert len(out["first_bad_xor"]) == 32
    assert int(out["first_bad_xor"], 16) == 1 << (8 * (4100 - 4096) + 3)


@pytest.mark.parametrize("nbytes", [16, 31])
def test_cpu_single_vector_regions(gpucheck, nbytes):
    rc, out = run_cpu(gpucheck, "--bytes", nbytes)
    assert rc == 0
    assert out["bytes"] == 16 and out["vectors"] == 1
    # ...and that one vector really is tested
    rc, out = run_cpu(gpucheck, "--bytes", nbytes, "--inject-flip", "15:7")
    assert rc == 20
    assert out["mismatch_vectors"] == 1 and out["first_bad_offset"] == 0
    assert int(out["first_bad_xor"], 16) == 1 << 127


def test_cpu_odd_pass_is_complement(gpucheck):
    """A flip injected after the pass-0 fill is seen by pass 0 only: pass 1
    rewrites every cell with the complement and verifies clean."""
    rc, out = run_cpu(gpucheck, "--bytes", 256, "--passes", 3,
                      "--inject-flip", "0:0")
    assert rc == 20
    assert out["mismatch_vectors"] == 1 and out["first_bad_pass"] == 0


def test_cpu_base_index_is_64_bit(gpucheck):
    base = 4294967295
    rc, hi = run_cpu(gpucheck, "--bytes", 64, "--base-index", base,
                     "--dump-pattern")
    assert rc == 0 and hi["mismatch_vectors"] == 0
    # Vector 1 has logical index 2**32. Its 32-bit-truncated twin is logical
    # index 0 (vector 1 of a run based at 4294967295 - 2**32 = -1), which is
    # vector 0 of a base-index-0 run.
    rc, zero = run_cpu(gpucheck, "--bytes", 64, "--base-index", 0,
                       "--dump-pattern")
    assert rc == 0
    assert len(hi["pattern_dump"]) == 4
    assert hi["pattern_dump"][1] != zero["pattern_dump"][0]
    # vector 0 of the high run is logical index 2**32-1, which a 32-bit
    # index would also reach: both runs agree there.
    rc, wrap = run_cpu(gpucheck, "--bytes", 64, "--base-index", base - 1,
                       "--dump-pattern")
    assert wrap["pattern_dump"][1] == hi["pattern_dump"][0]
    assert len(set(hi["pattern_dump"])) == 4


@pytest.mark.parametrize("args", [
    ["--bogus"],
    ["--bytes"],
    ["--bytes", "12x"],
    ["--passes", "0"],
    ["--inject-flip", "5"],
    ["--inject-flip", "0:8"],
    ["--bytes", "64", "--inject-flip", "64:0"],
    ["--min-copy-gbs", "-1"],
    ["--mfma-waves", "0"],
])
def test_bad_flags_exit_2(gpucheck, args):
    proc = subprocess.run([gpucheck, "--cpu", *args], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 2
    assert "usage:" in proc.stderr


@pytest.mark.parametrize("args", [
    ["--bytes", "64", "--dump-vectors", "4"],          # 4 vectors: 0..3
    ["--bytes", "64", "--dump-vectors", "0,,1"],
    ["--bytes", "4096", "--dump-vectors", ",".join(map(str, range(17)))],
    ["--store-variant", "fast"],
    ["--passes", "2", "--inject-pass", "2"],
    ["--bytes", "4096"] + ["--inject-flip", "0:0"] * 17,
    ["--bytes", "64", "--inject-copy-flip", "31:0"],   # source half
    ["--bytes", "80", "--inject-copy-flip", "64:0"],   # the odd vector out
    ["--bytes", "16", "--inject-copy-flip", "0:0"],    # no halves at all
    ["--mfma-waves", "5", "--inject-mfma", "5:0"],
    ["--mfma-waves", "5", "--inject-mfma", "0:1024"],
    ["--mfma-waves", "5"] + ["--inject-mfma", "0:0"] * 9,
    ["--mfma-waves", "5", "--dump-mfma-tile", "5"],
    ["--dump-mfma-tile", "0"],                         # --cpu runs no wave
    ["--inject-mfma", "0:0"],
])
def test_bad_test_flags_exit_2(gpucheck, args):
    proc = subprocess.run([gpucheck, "--cpu", *args], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 2
    assert "usage:" in proc.stderr
    assert proc.stdout == ""


# ------------------------------------------- against the Python reference

OTHER_SEED = 0x0123456789ABCDEF


@pytest.mark.parametrize("seed", [ref.DEFAULT_SEED, OTHER_SEED])
@pytest.mark.parametrize("base", [0, 2**32 - 1, 2**40])
def test_cpu_pattern_matches_reference(gpucheck, base, seed):
    """Pins gpucheck_pattern.h to the independent port: the host's expected
    values (pattern_dump, pass 0) and what the region holds after an even and
    an odd last pass (vector_dump)."""
    for passes in (1, 2):
        rc, out = run_cpu(gpucheck, "--bytes", 64, "--base-index", base,
                          "--seed", seed, "--passes", passes,
                          "--dump-pattern", "--dump-vectors", "0,1,2,3")
        assert rc == 0 and out["seed"] == seed and out["base_index"] == base
        assert out["pattern_dump"] == [ref.pattern(seed, 0, base + i)
                                       for i in range(4)]
        assert out["vector_dump"] == [
            {"index": i, "pass": passes - 1,
             "value": ref.pattern(seed, passes - 1, base + i)}
            for i in range(4)]


def test_reference_odd_pass_is_complement_and_passes_differ():
    """The reference itself: pass 1 complements pass 0, pass 2 is a new
    pattern, and the index is used at its full 64 bits."""
    seed = ref.DEFAULT_SEED
    full = (1 << 128) - 1
    assert ref.pattern_int(seed, 1, 7) == ref.pattern_int(seed, 0, 7) ^ full
    assert ref.pattern_int(seed, 3, 7) == ref.pattern_int(seed, 2, 7) ^ full
    assert ref.pattern_int(seed, 2, 7) != ref.pattern_int(seed, 0, 7)
    assert ref.pattern_int(seed, 0, 2**32) != ref.pattern_int(seed, 0, 0)
    assert len(ref.pattern(seed, 0, 0)) == 32


def test_cpu_dump_vectors_shows_memory_not_expectation(gpucheck):
    """A flip in the last pass is visible in vector_dump (what the region
    holds) and absent from pattern_dump (what the host expects)."""
    rc, out = run_cpu(gpucheck, "--bytes", 64, "--passes", 1,
                      "--inject-flip", "17:2", "--dump-pattern",
                      "--dump-vectors", "1,0")
    assert rc == 20
    want1 = ref.pattern_int(ref.DEFAULT_SEED, 0, 1)
    assert out["pattern_dump"][1] == f"{want1:032x}"
    assert [d["index"] for d in out["vector_dump"]] == [1, 0]
    assert int(out["vector_dump"][0]["value"], 16) == want1 ^ (1 << 10)
    assert out["vector_dump"][1]["value"] == \
        ref.pattern(ref.DEFAULT_SEED, 0, 0)


@pytest.mark.parametrize("variant", ["plain", "nontemporal"])
def test_cpu_forced_store_variant_is_reported(gpucheck, variant):
    rc, out = run_cpu(gpucheck, "--bytes", 4096, "--store-variant", variant)
    assert rc == 0 and out["store_variant"] == variant
    other = "nontemporal" if variant == "plain" else "plain"
    assert out[f"write_gbs_{other}"] == 0
    rc, out = run_cpu(gpucheck, "--bytes", 4096, "--store-variant", "auto")
    assert rc == 0 and out["store_variant"] == "plain"


# The multi-flip cases the GPU suite runs through hbm_verify's reduction
# (tests/test_gpucheck_gpu.py); here the host loops are held to the same
# answers.

@pytest.mark.parametrize("case", sorted(ref.MULTI_FLIP_CASES))
def test_cpu_multiple_flips_count_and_minimum(gpucheck, case):
    flips = ref.MULTI_FLIP_CASES[case]
    rc, out = run_cpu(gpucheck, "--bytes", ref.MULTI_FLIP_REGION,
                      *ref.flip_args(flips))
    assert rc == 20
    ref.expect_flips(out, flips)
    if case == "seven-descending":
        assert out["mismatch_vectors"] == 6


def test_cpu_flip_on_a_complement_pass(gpucheck):
    flips = [(16 * 300 + 4, 5)]
    rc, out = run_cpu(gpucheck, "--bytes", 16 * 1024, "--passes", 3,
                      "--inject-pass", 1, *ref.flip_args(flips),
                      "--dump-vectors", "300")
    assert rc == 20
    ref.expect_flips(out, flips, pass_=1)
    # pass 2 rewrote the vector: the flip is gone from memory
    assert out["vector_dump"][0] == {
        "index": 300, "pass": 2,
        "value": ref.pattern(ref.DEFAULT_SEED, 2, 300)}


def test_cpu_counts_add_across_passes(gpucheck):
    rc, out = run_cpu(gpucheck, "--bytes", 16 * 1024, "--passes", 2,
                      "--inject-flip", "4100:3")
    assert rc == 20
    assert out["mismatch_vectors"] == 1 and out["first_bad_pass"] == 0


# --------------------------------------------------- MFMA checker, --cpu

def test_reference_tile_is_a_product_of_small_integers():
    tile = ref.mfma_tile(ref.DEFAULT_SEED, 4)
    assert tile.shape == (32, 32) and tile.dtype == "int64"
    assert abs(tile).max() <= 147  # far below 2**24: float32 holds it exactly
    key_a = ref.mfma_key(ref.DEFAULT_SEED, 4, 0)
    key_b = ref.mfma_key(ref.DEFAULT_SEED, 4, 1)
    assert tile[31, 0] == sum(
        ref.mfma_a(key_a, 31, k) * ref.mfma_b(key_b, k, 0)
        for k in range(ref.MFMA_K))
    assert (tile != tile.T).any()


def test_cpu_mfma_clean_five_waves(gpucheck):
    rc, out = run_cpu(gpucheck, "--bytes", 4096, "--mfma-waves", 5)
    assert rc == 0 and out["failed_stages"] == []
    assert out["mfma"] == "pass" and out["mfma_waves"] == 5
    assert out["mfma_bad_waves"] == 0 and out["mfma_first_bad_wave"] == -1
    assert "mfma_tile" not in out


@pytest.mark.parametrize("injections,bad,first", ref.MFMA_INJECT_CASES)
def test_cpu_mfma_injection_is_caught(gpucheck, injections, bad, first):
    rc, out = run_cpu(gpucheck, "--bytes", 4096, "--mfma-waves", 5,
                      *ref.mfma_inject_args(injections))
    assert rc == 21
    assert out["ok"] is False and out["failed_stages"] == ["mfma"]
    assert out["mfma"] == "fail" and out["mfma_waves"] == 5
    assert out["mfma_bad_waves"] == bad
    assert out["mfma_first_bad_wave"] == first
    assert out["hbm"] == "pass"


def test_cpu_hbm_mismatch_outranks_mfma(gpucheck):
    rc, out = run_cpu(gpucheck, "--bytes", 4096, "--passes", 1,
                      "--mfma-waves", 2, "--inject-flip", "0:0",
                      "--inject-mfma", "1:0")
    assert rc == 20 and out["failed_stages"] == ["hbm", "mfma"]


@pytest.mark.parametrize("seed", [ref.DEFAULT_SEED, OTHER_SEED])
def test_cpu_mfma_tile_matches_reference(gpucheck, seed):
    rc, out = run_cpu(gpucheck, "--bytes", 4096, "--mfma-waves", 5,
                      "--seed", seed, "--dump-mfma-tile", 4)
    assert rc == 0
    assert out["mfma_tile"]["wave"] == 4
    assert out["mfma_tile"]["values"] == \
        ref.mfma_tile(seed, 4).reshape(-1).tolist()


# ------------------------------------------------------------------ runner

GOOD_JSON = {"tool": "gpucheck", "ok": True, "exit_code": 0,
             "mismatch_vectors": 0, "copy_gbs": 3210.5, "read_gbs": 2100.25,
             "write_gbs": 1900.75, "mfma_bad_waves": 0}


def write_stub(tmp_path, name, body):
    path = tmp_path / name
    path.write_text("#!/bin/sh\n" + body)
    path.chmod(path.stat().st_mode | stat.S_IXUSR)
    return str(path)


def test_gpu_guard_skips_after_a_child_exits_11(tmp_path, monkeypatch):
    """The GPU files' runner and guard, with a stub for the binary and a
    list of this test's own: no GPU is touched, and the real list stays
    clean."""
    suspect = []
    monkeypatch.setattr(gpucheck_helpers, "_card_suspect", suspect)
    gpucheck_helpers.skip_if_card_suspect()  # nothing happened yet: no skip
    good = write_stub(tmp_path, "good", "echo '{\"ok\":true,\"big\":[1,2]}'\n")
    assert gpucheck_helpers.run_gpu(good, "--x", 1, hide=("big",))[:2] == \
        (0, {"ok": True, "big": [1, 2]})
    assert suspect == []
    stub = write_stub(tmp_path, "hip_error", "echo '{\"ok\":false}'\nexit 11\n")
    with pytest.raises(pytest.fail.Exception, match="gpucheck exit 11"):
        gpucheck_helpers.run_gpu(stub, "--bytes", 16)
    assert len(suspect) == 1 and suspect[0].startswith("exit 11:")
    assert stub in suspect[0]
    with pytest.raises(pytest.skip.Exception, match="ended badly: exit 11"):
        gpucheck_helpers.skip_if_card_suspect()


@pytest.fixture
def inventory(synthetic_ledger):
    return synthetic_ledger.inventory


def test_runner_pass(tmp_path, inventory):
    stub = write_stub(tmp_path, "good", f"""echo "warming up"
echo "$ROCR_VISIBLE_DEVICES $HIP_VISIBLE_DEVICES $@" > {tmp_path}/seen
echo '{json.dumps(GOOD_JSON)}'
""")
    os.environ["ROCR_VISIBLE_DEVICES"] = "7"  # inherited scoping is dropped
    try:
        res = run_gpucheck(3, inventory, nbytes=4096, timeout_s=10,
                           extra_args=["--passes", "1"], binary=stub)
    finally:
        del os.environ["ROCR_VISIBLE_DEVICES"]
    assert isinstance(res, GpuCheckResult)
    assert res.ok and res.reason == "" and res.exit_code == 0 and res.gpu == 3
    assert res.data["copy_gbs"] == 3210.5
    assert (tmp_path / "seen").read_text().split() == [
        "3", "3", "--bytes", "4096", "--passes", "1"]
    assert res.to_dict()["ok"] is True and res.to_dict()["gpu"] == 3


def test_runner_fail_exit_20(tmp_path, inventory):
    bad = dict(GOOD_JSON, ok=False, exit_code=20, mismatch_vectors=1,
               first_bad_offset=4096, failed_stages=["hbm"])
    stub = write_stub(tmp_path, "bad", f"echo '{json.dumps(bad)}'\nexit 20\n")
    res = run_gpucheck(0, inventory, nbytes=4096, timeout_s=10, binary=stub)
    assert not res.ok and res.exit_code == 20 and res.reason == "hbm"
    assert res.data["first_bad_offset"] == 4096


def test_runner_fail_exit_23(tmp_path, inventory):
    bad = dict(GOOD_JSON, ok=False, exit_code=23, copy_mismatch_vectors=1,
               copy_first_bad_offset=8192, failed_stages=["copy"])
    stub = write_stub(tmp_path, "bad", f"echo '{json.dumps(bad)}'\nexit 23\n")
    res = run_gpucheck(0, inventory, nbytes=4096, timeout_s=10, binary=stub)
    assert not res.ok and res.exit_code == 23 and res.reason == "copy"
    assert res.data["copy_first_bad_offset"] == 8192


def test_runner_timeout_kills_the_group(tmp_path, inventory):
    stub = write_stub(tmp_path, "slow",
                      f"echo $$ > {tmp_path}/pid\nsleep 600 &\n"
                      f"echo $! > {tmp_path}/childpid\nwait\n")
    t0 = time.monotonic()
    res = run_gpucheck(0, inventory, nbytes=4096, timeout_s=0.5, binary=stub)
    assert time.monotonic() - t0 < 10
    assert not res.ok and res.reason == "timeout"
    for name in ("pid", "childpid"):
        pid = int((tmp_path / name).read_text())

        def gone(pid=pid):
            try:
                os.kill(pid, 0)
            except ProcessLookupError:
                return True
            # a zombie awaiting its reaper counts as gone
            with open(f"/proc/{pid}/stat") as fh:
                return fh.read().rsplit(")", 1)[1].split()[0] == "Z"

        assert wait_until(gone, timeout_s=5), name


def test_runner_garbage_and_signal(tmp_path, inventory):
    stub = write_stub(tmp_path, "garbage", "echo 'not json at all'\n")
    res = run_gpucheck(0, inventory, nbytes=4096, timeout_s=10, binary=stub)
    assert not res.ok and res.reason == "bad-output"
    stub = write_stub(tmp_path, "empty", "exit 0\n")
    res = run_gpucheck(0, inventory, nbytes=4096, timeout_s=10, binary=stub)
    assert not res.ok and res.reason == "bad-output"
    stub = write_stub(tmp_path, "segv", "kill -SEGV $$\n")
    res = run_gpucheck(0, inventory, nbytes=4096, timeout_s=10, binary=stub)
    assert not res.ok and res.reason == "signal 11"


def test_runner_real_binary_cpu_mode(gpucheck, inventory):
    res = run_gpucheck(0, inventory, nbytes=4112, timeout_s=30,
                       extra_args=["--cpu"], binary=gpucheck)
    assert res.ok and res.data["vectors"] == 257
    res = run_gpucheck(0, inventory, nbytes=4112, timeout_s=30,
                       extra_args=["--cpu", "--inject-flip", "4100:3"])
    assert not res.ok and res.reason == "hbm" and res.exit_code == 20


# ----------------------------------------------------------------- manager

class StubRunner:
    """Stands in for run_gpucheck; records calls and what the ledger looked
    like while the 'check' was running."""

    def __init__(self, ledger):
        self.ledger = ledger
        self.calls = []
        self.fail = {}          # idx -> (exit_code, reason, data)
        self.during = []        # (idx, reservation, occupied) per call
        self.gate = None        # optional threading.Event to block on
        self.active = 0
        self.max_active = 0
        self._lock = threading.Lock()

    def __call__(self, gpu, inventory, *, nbytes, timeout_s, extra_args=()):
        with self._lock:
            self.calls.append((gpu, nbytes, timeout_s, tuple(extra_args)))
            self.active += 1
            self.max_active = max(self.max_active, self.active)
        res = self.ledger.get_reservation(f"amdvk-system/gpucheck-{gpu}")
        self.during.append((gpu, res, self.ledger.states[gpu].occupied))
        if self.gate is not None:
            assert self.gate.wait(10)
        with self._lock:
            self.active -= 1
        now = time.time()
        if gpu in self.fail:
            code, reason, data = self.fail[gpu]
            return GpuCheckResult(gpu=gpu, ok=False, exit_code=code,
                                  reason=reason, data=dict(data),
                                  duration_s=0.01, timestamp=now)
        return GpuCheckResult(gpu=gpu, ok=True, exit_code=0,
                              data=dict(GOOD_JSON), duration_s=0.01,
                              timestamp=now)


HBM_FAIL = (20, "hbm", {"ok": False, "mismatch_vectors": 1,
                        "first_bad_offset": 4096, "failed_stages": ["hbm"]})


class Recorder:
    def __init__(self):
        self.events = []

    def event(self, obj, event_type, reason, message):
        self.events.append((obj, event_type, reason, message))


@pytest.fixture
def manager(synthetic_ledger):
    cfg = Config(gpu_check_bytes=1 << 20, gpu_check_interval_s=3600.0)
    runner = StubRunner(synthetic_ledger)
    rec = Recorder()
    mgr = DiagnosticsManager(synthetic_ledger, synthetic_ledger.inventory, cfg,
                             runner=runner, recorder=rec, node_name="node-a")
    return mgr, runner, rec, synthetic_ledger


def test_manager_failed_check_fences_gpu(manager):
    mgr, runner, rec, ledger = manager
    runner.fail[2] = HBM_FAIL
    res = mgr.check(2)
    assert not res.ok
    st = ledger.states[2]
    assert not st.schedulable and st.gpu.healthy and not st.cordoned
    assert st.gpu.diag_ok is False and st.gpu.diag_reason == "hbm"
    assert st.gpu.diag_last["first_bad_offset"] == 4096
    assert ledger.schedulable_count() == 7
    # the binder never returns it: fill the node one GPU at a time
    binder = Binder(ledger)
    picked = []
    for i in range(7):
        picked += binder.bind(BindRequest(f"default-p{i}", 1, 0, max_cost=1.0))
    assert sorted(picked) == [0, 1, 3, 4, 5, 6, 7]
    with pytest.raises(PlacementError):
        binder.select(BindRequest("default-p8", 1, 0, max_cost=1.0))
    # Warning Event on the node with the stage and the offset
    (obj, etype, reason, message), = rec.events
    assert obj["kind"] == "Node" and obj["metadata"]["name"] == "node-a"
    assert etype == "Warning" and reason == "GpuCheckFailed"
    assert "stage=hbm" in message and "first_bad_offset=4096" in message


def test_manager_refuses_occupied_and_unknown(manager):
    mgr, runner, _, ledger = manager
    ledger.reserve("default-tenant", [1], 1 << 30)
    with pytest.raises(GpuBusyError):
        mgr.check(1)
    with pytest.raises(UnknownGpuError):
        mgr.check(99)
    assert runner.calls == []
    assert ledger.get_reservation("default-tenant") is not None


def test_manager_reservation_held_then_released(manager):
    mgr, runner, _, ledger = manager
    before = time.monotonic()
    res = mgr.check(4)
    assert res.ok
    (gpu, held, occupied), = runner.during
    assert gpu == 4 and occupied
    assert held is not None and held.gpu_indices == [4]
    assert held.bytes_per_gpu == 1 << 20
    assert runner.calls == [(4, 1 << 20, 60.0, ())]
    # released, with the settle stamp any freed GPU gets
    assert ledger.get_reservation("amdvk-system/gpucheck-4") is None
    assert not ledger.states[4].occupied
    assert ledger.states[4].reserved_bytes == 0
    assert ledger.states[4].last_freed_at >= before
    assert ledger.states[4].schedulable


def test_manager_binder_cannot_place_during_check(manager):
    mgr, runner, _, ledger = manager
    for i in range(7):  # leave only GPU 7 free
        ledger.reserve(f"default-t{i}", [i], 0)
    runner.gate = threading.Event()
    t = threading.Thread(target=mgr.check, args=(7,))
    t.start()
    try:
        assert wait_until(lambda: runner.during, timeout_s=5)
        with pytest.raises(PlacementError):
            Binder(ledger).select(BindRequest("default-x", 1, 0, max_cost=1.0))
        # one check per GPU at a time
        with pytest.raises(GpuBusyError):
            mgr.check(7)
    finally:
        runner.gate.set()
        t.join(10)
    assert Binder(ledger).select(
        BindRequest("default-x", 1, 0, max_cost=1.0)) == [7]


def test_manager_failed_state_survives_refresh_and_rediscovery(manager):
    mgr, runner, _, ledger = manager
    runner.fail[5] = HBM_FAIL
    mgr.check(5)
    ledger.inventory.refresh_dynamic()
    ledger.sync_inventory()
    assert not ledger.states[5].schedulable
    # a re-discovery hands the ledger brand-new Gpu records
    ledger.inventory.discover()
    ledger.sync_inventory()
    assert ledger.states[5].gpu is ledger.inventory.get(5)
    assert ledger.states[5].gpu.diag_ok is False
    assert ledger.states[5].gpu.diag_reason == "hbm"
    assert not ledger.states[5].schedulable
    assert ledger.states[4].schedulable


def test_manager_only_operator_recheck_clears_failure(manager):
    mgr, runner, _, ledger = manager
    runner.fail[6] = HBM_FAIL
    mgr.check(6)
    del runner.fail[6]
    # a passing non-operator check does not clear it, and takes no
    # reservation (the GPU is unschedulable anyway)
    runner.during.clear()
    assert mgr.check(6).ok
    assert runner.during == [(6, None, False)]
    assert not ledger.states[6].schedulable
    assert ledger.states[6].gpu.diag_reason == "hbm"
    assert mgr.check(6, operator=True).ok
    assert ledger.states[6].schedulable
    assert ledger.states[6].gpu.diag_reason == ""
    assert ledger.states[6].gpu.diag_last["ok"] is True


def test_manager_periodic_skips_failed_occupied_and_fresh(manager):
    mgr, runner, _, ledger = manager
    runner.fail[0] = HBM_FAIL
    mgr.check(0)
    ledger.reserve("default-tenant", [1], 0)
    ledger.set_cordoned(2, True)
    mgr.check(3)  # fresh result: younger than the interval
    runner.calls.clear()
    results = mgr.periodic()
    assert sorted(c[0] for c in runner.calls) == [4, 5, 6, 7]
    assert [r.gpu for r in results] == [4, 5, 6, 7]
    assert runner.max_active <= 2  # gpu_check_parallel default
    # nothing is stale any more
    runner.calls.clear()
    assert mgr.periodic() == [] and runner.calls == []
    # interval 0 = off
    mgr.config.gpu_check_interval_s = 0
    mgr._last_checked.clear()
    assert mgr.periodic() == [] and runner.calls == []


def test_manager_passes_copy_floor(manager):
    mgr, runner, _, _ = manager
    mgr.config.gpu_check_min_copy_gbs = 1500.0
    mgr.check(0)
    assert runner.calls[0][3] == ("--min-copy-gbs", "1500.0")


# ---------------------------------------------------------------- surfaces

def post(url, headers=None):
    req = urllib.request.Request(url, method="POST", headers=headers or {})
    try:
        with urllib.request.urlopen(req, timeout=10) as resp:
            return resp.status, resp.read().decode()
    except urllib.error.HTTPError as exc:
        return exc.code, exc.read().decode()


def get(url, headers=None):
    req = urllib.request.Request(url, headers=headers or {})
    try:
        with urllib.request.urlopen(req, timeout=10) as resp:
            return resp.status, resp.read().decode()
    except urllib.error.HTTPError as exc:
        return exc.code, exc.read().decode()


def test_gpucheck_endpoints(manager, fake_kube):
    from k8s_runpod_kubelet_amd.provider.provider import Provider
    from k8s_runpod_kubelet_amd.runtime.fake import FakeRuntime
    from k8s_runpod_kubelet_amd.server.health import HealthServer

    mgr, runner, _, ledger = manager
    hs = HealthServer("127.0.0.1:0", None, ledger=ledger, diagnostics=mgr)
    hs.start()
    base = f"http://127.0.0.1:{hs.port}"
    try:
        code, body = get(f"{base}/gpucheck")
        assert code == 200
        assert json.loads(body)["3"] == {"ok": True, "reason": "",
                                         "lastCheck": None}
        code, body = post(f"{base}/gpucheck/3")
        assert code == 200
        out = json.loads(body)
        assert out["ok"] is True and out["gpu"] == 3
        assert out["copy_gbs"] == 3210.5

        assert post(f"{base}/gpucheck/99")[0] == 404
        assert post(f"{base}/gpucheck/x")[0] == 400
        ledger.reserve("default-tenant", [1], 0)
        assert post(f"{base}/gpucheck/1")[0] == 409

        runner.fail[2] = HBM_FAIL
        code, body = post(f"{base}/gpucheck/2")
        assert code == 200 and json.loads(body)["reason"] == "hbm"
        assert not ledger.states[2].schedulable
        # an operator re-check that passes restores it
        del runner.fail[2]
        runner.fail[4] = HBM_FAIL
        post(f"{base}/gpucheck/4")
        code, body = post(f"{base}/gpucheck/2")
        assert code == 200 and ledger.states[2].schedulable

        code, body = get(f"{base}/gpucheck")
        last = json.loads(body)
        assert last["3"]["ok"] is True and last["3"]["lastCheck"]["gpu"] == 3
        assert last["4"]["ok"] is False and last["4"]["reason"] == "hbm"
        assert last["4"]["lastCheck"]["first_bad_offset"] == 4096
        assert last["0"]["lastCheck"] is None

        code, text = get(f"{base}/metrics")
        assert code == 200
        assert 'amdvk_gpu_check_ok{gpu="3"} 1.0' in text
        assert 'amdvk_gpu_check_ok{gpu="4"} 0.0' in text
        assert 'amdvk_gpu_check_copy_gbs{gpu="3"} 3210.5' in text
        assert 'amdvk_gpu_check_read_gbs{gpu="3"} 2100.25' in text
        assert 'amdvk_gpu_check_write_gbs{gpu="3"} 1900.75' in text
        assert 'amdvk_gpu_check_timestamp_seconds{gpu="3"}' in text
        assert ('amdvk_gpu_check_failures_total{gpu="4",stage="hbm"}'
                in text)

        prov = Provider(fake_kube, Config(notify_interval_s=0),
                        FakeRuntime(gpu_count=8), ledger=ledger,
                        inventory=ledger.inventory)
        gpus = {g["index"]: g for g in prov.get_stats_summary()["gpus"]}
        assert gpus[3]["lastCheck"]["ok"] is True
        assert gpus[4]["lastCheck"]["reason"] == "hbm"
        assert gpus[0]["lastCheck"] is None
    finally:
        hs.stop()


def test_gpucheck_endpoint_absent_without_manager(synthetic_ledger):
    from k8s_runpod_kubelet_amd.server.health import HealthServer

    hs = HealthServer("127.0.0.1:0", None, ledger=synthetic_ledger)
    hs.start()
    try:
        base = f"http://127.0.0.1:{hs.port}"
        assert post(f"{base}/gpucheck/0")[0] == 404
        assert get(f"{base}/gpucheck")[0] == 404
    finally:
        hs.stop()


def _nonloopback_ip():
    import socket

    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        s.connect(("10.255.255.255", 1))
        ip = s.getsockname()[0]
        return None if ip.startswith("127.") else ip
    except OSError:
        return None
    finally:
        s.close()


def test_gpucheck_admin_requires_loopback_or_token(manager):
    from k8s_runpod_kubelet_amd.server.health import HealthServer

    mgr, runner, _, ledger = manager
    ip = _nonloopback_ip()
    if ip is None:
        pytest.skip("no non-loopback interface")
    hs = HealthServer("0.0.0.0:0", None, ledger=ledger, admin_token="sekrit",
                      diagnostics=mgr)
    hs.start()
    try:
        base = f"http://{ip}:{hs.port}"
        assert post(f"{base}/gpucheck/3")[0] == 403
        assert post(f"{base}/gpucheck/3",
                    {"Authorization": "Bearer nope"})[0] == 403
        assert get(f"{base}/gpucheck")[0] == 403
        assert runner.calls == []
        assert post(f"{base}/gpucheck/3",
                    {"Authorization": "Bearer sekrit"})[0] == 200
        assert get(f"{base}/gpucheck",
                   {"Authorization": "Bearer sekrit"})[0] == 200
        # loopback needs no token
        assert post(f"http://127.0.0.1:{hs.port}/gpucheck/3")[0] == 200
        assert [c[0] for c in runner.calls] == [3, 3]
    finally:
        hs.stop()


# ------------------------------------------------------------- full stack

def _stack(tmp_path, **cfg_kw):
    from k8s_runpod_kubelet_amd.app import build_stack
    from k8s_runpod_kubelet_amd.kube.fake import FakeKube

    cfg = Config(state_dir=str(tmp_path), notify_interval_s=0,
                 gpu_count_override=8, **cfg_kw)
    stack = build_stack(cfg, client=FakeKube())
    runner = StubRunner(stack.ledger)
    stack.diagnostics.runner = runner
    return stack, runner


def test_defaults_never_run_a_check(tmp_path):
    cfg = Config()
    assert cfg.gpu_check_on_start is False
    assert cfg.gpu_check_interval_s == 0
    assert cfg.gpu_check_bytes == 1 << 30
    assert cfg.gpu_check_timeout_s == 60
    assert cfg.gpu_check_min_copy_gbs == 0
    assert cfg.gpu_check_parallel == 2
    stack, runner = _stack(tmp_path)
    stack.start(serve_http=False)
    try:
        stack.provider._periodic_reconcile()
        assert not any(t.name == "gpu-check" for t in stack.provider._tickers)
        assert stack.diagnostics.periodic() == []
        assert runner.calls == []
        assert stack.ledger.schedulable_count() == 8
    finally:
        stack.stop()


def test_check_on_start_gates_capacity(tmp_path):
    stack, runner = _stack(tmp_path, gpu_check_on_start=True,
                           gpu_check_interval_s=3600.0,
                           gpu_check_bytes=1 << 20)
    runner.fail[5] = HBM_FAIL
    stack.start(serve_http=False)
    try:
        assert sorted(c[0] for c in runner.calls) == list(range(8))
        assert any(t.name == "gpu-check" for t in stack.provider._tickers)
        node = stack.provider.get_node_status()
        assert node["status"]["capacity"]["amd.com/gpu"] == "8"
        assert node["status"]["allocatable"]["amd.com/gpu"] == "7"
        assert not stack.ledger.reservations
        # the real EventRecorder put a Warning on the node
        events = [e for e in stack.client.events.objects.values()
                  if e["reason"] == "GpuCheckFailed"]
        assert len(events) == 1
        assert events[0]["type"] == "Warning"
        assert events[0]["involvedObject"]["kind"] == "Node"
        assert events[0]["involvedObject"]["name"] == stack.config.node_name
        assert "stage=hbm" in events[0]["message"]
        assert "first_bad_offset=4096" in events[0]["message"]
    finally:
        stack.stop()


def test_cli_flags_reach_config():
    from k8s_runpod_kubelet_amd.cli import build_parser

    args = build_parser().parse_args([])
    assert args.gpu_check_on_start is None and args.gpu_check_interval is None
    args = build_parser().parse_args([
        "--gpu-check-on-start", "--gpu-check-interval", "6h",
        "--gpu-check-bytes", "4G", "--gpu-check-timeout", "90s",
        "--gpu-check-min-copy-gbs", "1500", "--gpu-check-parallel", "3"])
    assert args.gpu_check_on_start is True
    assert args.gpu_check_interval == "6h"
    from k8s_runpod_kubelet_amd.gpu.diagnostics import parse_size

    assert parse_size(args.gpu_check_bytes) == 4 << 30
    assert parse_size("4096") == 4096 and parse_size("512MiB") == 512 << 20


def test_operator_cli_runs_binary(gpucheck, capsys):
    from k8s_runpod_kubelet_amd.gpu import diagnostics

    code = diagnostics.main(["--gpu", "0", "--bytes", "4112",
                             "--sysfs-root", "/nonexistent-sysfs",
                             "--", "--cpu", "--inject-flip", "4100:3"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert code == 20 and out["reason"] == "hbm"
    assert out["first_bad_offset"] == 4096
    code = diagnostics.main(["--gpu", "0", "--bytes", "4K",
                             "--sysfs-root", "/nonexistent-sysfs",
                             "--", "--cpu"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert code == 0 and out["ok"] is True and out["bytes"] == 4096


def test_gpucheck_as_pod_command(gpucheck, process_runtime):
    from k8s_runpod_kubelet_amd.runtime.types import (
        ContainerSpec, DeployParams, PodStatus)

    st = process_runtime.deploy(DeployParams(
        pod_key="default-diag", name="diag", gpu_count=0,
        containers=[ContainerSpec(
            name="main", command=["gpucheck", "--cpu", "--bytes", "4096"])],
    ))

    def exited():
        s = process_runtime.get_detailed_status(st.id)
        return s if s.desired_status == PodStatus.EXITED else None

    s = wait_until(exited, timeout_s=30)
    assert s is not None, process_runtime.get_logs(st.id)
    assert s.exit_code == 0, process_runtime.get_logs(st.id)
    assert '"mismatch_vectors":0' in process_runtime.get_logs(st.id)
