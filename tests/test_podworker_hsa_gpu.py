"""The ROCr podworker on a real MI355X: both kernels through the AQL queue at
the sizes where the index arithmetic, the tail block or the sample set can go
wrong, the report line, the count mismatch, the timing switch and SIGTERM.

Expected values are the closed form 2*i+1 mod 2**32, checked twice: by the
binary itself (--verify-all brings every element back through the gather
kernel), and by the tests here, which have the binary print the words the
gather kernel wrote (--dump-samples) and compare them with (2*i+1) &
0xFFFFFFFF and with a Python statement of the sample set. --inject-store has
one more touch dispatch overwrite a chosen word with 1 in device memory, which
shows that the gather loads what is stored there, that the host comparison can
fail at all (exit 13), and which indices a sampled run does and does not
cover. Everything is compared with ==; nothing here needs a tolerance.

Every test starts the binary as a child with a 60 s limit of its own. Once a
child ends with a runtime error (11), a signal or its time limit, the rest of
the file skips: nothing more is started on a card that may be in trouble."""

import os
import re
import select
import signal
import subprocess
import time

import pytest

from tests.podworker_reference import reference_sample_set

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 60

_card_suspect = []  # reason, once a child ended badly


@pytest.fixture(autouse=True)
def _stop_after_trouble():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no /dev/kfd on this box")
    if _card_suspect:
        pytest.skip(f"an earlier podworker child ended badly: {_card_suspect[0]}")


@pytest.fixture(scope="module")
def binary():
    from k8s_runpod_kubelet_amd.ops import podworker_binary

    return podworker_binary()


def _one_gpu_env(**extra):
    """The environment for a child that must see exactly one GPU: the first
    of those already selected for this process, or GPU 0."""
    visible = os.environ.get("ROCR_VISIBLE_DEVICES", "").split(",")[0].strip()
    return dict(os.environ, ROCR_VISIBLE_DEVICES=visible or "0", **extra)


def _kill_group(proc):
    try:
        os.killpg(proc.pid, signal.SIGKILL)
    except ProcessLookupError:
        pass
    proc.communicate()


def run_gpu(binary, *args, env=None, visible=None):
    """-> (exit code, stdout lines, stderr, wall seconds). The child sees one
    GPU unless `visible` names the devices it is to see."""
    argv = [binary, *map(str, args)]
    child_env = _one_gpu_env(**(env or {}))
    if visible is not None:
        child_env["ROCR_VISIBLE_DEVICES"] = visible
    t0 = time.monotonic()
    proc = subprocess.Popen(argv, stdin=subprocess.DEVNULL,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True, start_new_session=True, env=child_env)
    try:
        out, err = proc.communicate(timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _card_suspect.append(f"timeout: {argv}")
        _kill_group(proc)
        pytest.fail(f"podworker exceeded {CHILD_TIMEOUT_S} s: {argv}")
    wall = time.monotonic() - t0
    if proc.returncode == 11 or proc.returncode < 0:
        _card_suspect.append(f"exit {proc.returncode}: {argv}")
        pytest.fail(f"podworker exit {proc.returncode}: {argv}\n{out}\n{err}")
    print(f"{' '.join(map(str, args))} -> rc={proc.returncode} "
          f"wall={wall:.3f}s\n{out}{err}")
    return proc.returncode, out.splitlines(), err, wall


def ok_lines(lines):
    return [ln for ln in lines
            if ln.startswith("podworker: dev ") and ln.endswith(" ok")]


# a single thread; one short block; one exact block; a one-element tail
# block; the first sample stride; one past the head window
VERIFY_ALL_SIZES = [1, 255, 256, 257, 4099, 65537]


@pytest.mark.parametrize("n", VERIFY_ALL_SIZES)
def test_verify_all(binary, n):
    rc, lines, err, _ = run_gpu(binary, "--expect-gpus", 1, "--verify-all",
                                "--run-for", 0, "--touch-elems", n)
    assert rc == 0, (lines, err)
    assert len(ok_lines(lines)) == 1, lines
    assert "podworker: ready (gpus=1 ports=0)" in lines
    assert lines[-1] == "podworker: exiting code=0"


def test_default_size_and_sampling_report_line(binary):
    rc, lines, err, _ = run_gpu(binary, "--expect-gpus", 1, "--run-for", 0)
    assert rc == 0, (lines, err)
    reports = ok_lines(lines)
    assert len(reports) == 1, lines
    # the product name is empty where the host has no marketing-name table
    m = re.fullmatch(r"podworker: dev 0 (.*) gcnArch=(\S+) vram=(\d+)MB ok",
                     reports[0])
    assert m, reports[0]
    assert "gfx950" in m.group(2)
    assert "amdgcn" not in m.group(2)
    assert int(m.group(3)) > 100000


def test_count_mismatch_exits_12(binary):
    rc, lines, err, _ = run_gpu(binary, "--expect-gpus", 99, "--run-for", 0)
    assert rc == 12, (lines, err)
    assert "podworker: visible GPU count 1 != expected 99" in err
    assert not ok_lines(lines)
    assert "podworker: ready" not in "\n".join(lines)


TIMING_FIELDS = ("runtime_init_ms", "queue_ms", "load_ms", "alloc_ms",
                 "dispatch_verify_ms", "to_ready_ms")


def test_timing_line(binary):
    rc, lines, err, _ = run_gpu(binary, "--expect-gpus", 1, "--run-for", 0,
                                env={"AMDVK_PODWORKER_TIMING": "1"})
    assert rc == 0, (lines, err)
    timing = [ln for ln in lines if ln.startswith("podworker: timing ")]
    assert len(timing) == 1, lines
    assert not timing[0].endswith(" ok")
    assert lines.index(timing[0]) < lines.index(
        "podworker: ready (gpus=1 ports=0)")
    pairs = dict(kv.split("=") for kv in timing[0].split()[2:])
    assert tuple(pairs) == TIMING_FIELDS, timing[0]
    values = {k: float(v) for k, v in pairs.items()}
    assert all(v >= 0 for v in values.values()), values
    parts = sum(v for k, v in values.items() if k != "to_ready_ms")
    # each field is printed rounded to a microsecond
    assert values["to_ready_ms"] >= parts - 0.001 * len(TIMING_FIELDS), values


def test_no_timing_line_by_default(binary):
    env = {k: v for k, v in os.environ.items()
           if k != "AMDVK_PODWORKER_TIMING"}
    proc = subprocess.run([binary, "--run-for", "0"], env=env,
                          capture_output=True, text=True, timeout=30)
    assert proc.returncode == 0
    assert "timing" not in proc.stdout


def test_sigterm_while_holding(binary):
    rfd, wfd = os.pipe()
    os.set_inheritable(wfd, True)
    env = _one_gpu_env(AMDVK_READY_FD=str(wfd))
    argv = [binary, "--expect-gpus", "1", "--hold"]
    proc = subprocess.Popen(argv, stdin=subprocess.DEVNULL,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True, start_new_session=True, env=env,
                            pass_fds=(wfd,))
    os.close(wfd)
    try:
        # the child writes READY and closes its end, or dies and closes it
        with os.fdopen(rfd, "rb") as ready_pipe:
            if not select.select([ready_pipe], [], [], CHILD_TIMEOUT_S)[0]:
                raise subprocess.TimeoutExpired(argv, CHILD_TIMEOUT_S)
            ready = ready_pipe.read()
        if ready != b"READY\n":
            out, err = proc.communicate(timeout=CHILD_TIMEOUT_S)
            _card_suspect.append(f"no READY, exit {proc.returncode}: {argv}")
            pytest.fail(f"podworker never became ready: rc={proc.returncode}"
                        f"\n{out}\n{err}")
        t0 = time.monotonic()
        proc.send_signal(signal.SIGTERM)
        out, err = proc.communicate(timeout=10)
        wall = time.monotonic() - t0
    except subprocess.TimeoutExpired:
        _card_suspect.append(f"timeout: {argv}")
        _kill_group(proc)
        pytest.fail(f"podworker did not leave within its limit: {argv}")
    print(f"SIGTERM -> gone in {wall * 1e3:.1f} ms\n{out}{err}")
    if proc.returncode == 11 or proc.returncode < 0:
        _card_suspect.append(f"exit {proc.returncode}: {argv}")
    assert proc.returncode == 0, (out, err)
    assert wall < 10
    assert len(ok_lines(out.splitlines())) == 1
    assert out.splitlines()[-1] == "podworker: exiting code=0"


# ---- the words the kernels stored, against a reference outside the binary --

def reference_value(i):
    """The 32-bit word touch_kernel must leave in element i."""
    return (2 * i + 1) & 0xFFFFFFFF


INJECTED = 0x00000001  # what --inject-store I leaves in element I

_SAMPLE_LINE = re.compile(
    r"podworker: sample dev (\d+) (\d+) (\d+) 0x([0-9A-F]{8})")


def dumped_samples(lines, dev=0):
    """-> [(position J, element I, value)] of one device, in printed order."""
    rows = []
    for ln in lines:
        if ln.startswith("podworker: sample "):
            m = _SAMPLE_LINE.fullmatch(ln)
            assert m, ln
            if int(m.group(1)) == dev:
                rows.append((int(m.group(2)), int(m.group(3)),
                             int(m.group(4), 16)))
    return rows


def assert_dump(lines, n, verify_all, injected=(), dev=0):
    """The dump names exactly the reference sample set, in order, and every
    word is the reference value, but for the injected elements, which hold 1
    at every position that samples them."""
    rows = dumped_samples(lines, dev)
    sample = reference_sample_set(n, verify_all)
    assert [(j, i) for j, i, _ in rows] == list(enumerate(sample))
    wrong = [(j, i, hex(v)) for j, i, v in rows
             if v != (INJECTED if i in injected else reference_value(i))]
    assert not wrong, wrong[:8]


def run_dump(binary, n, *extra, verify_all=False):
    flags = ("--verify-all",) if verify_all else ()
    return run_gpu(binary, "--expect-gpus", 1, "--run-for", 0, *flags,
                   "--touch-elems", n, "--dump-samples", *extra)


def assert_verify_failed(rc, lines, err, where):
    assert rc == 13, (lines[-3:], err)
    assert err.count("verify failed") == 1, err
    assert f"podworker: kernel verify failed at {where} on dev 0\n" in err
    assert not ok_lines(lines)
    assert "podworker: ready" not in "\n".join(lines)


# with --verify-all: the sizes of test_verify_all below the head window.
# Sampled: the tail equal to a stride index; the head window's edge and one
# past it; the default; the largest grid with an idle lane in its tail block
# (the largest size, 1<<28, fills its last block)
@pytest.mark.parametrize("n,verify_all", [
    (1, True), (255, True), (256, True), (257, True), (4099, True),
    (4100, False), (65536, False), (65537, False), (1 << 20, False),
    ((1 << 28) - 1, False)])
def test_dumped_values_equal_the_reference(binary, n, verify_all):
    rc, lines, err, _ = run_dump(binary, n, verify_all=verify_all)
    assert rc == 0, (lines[-3:], err)
    assert len(ok_lines(lines)) == 1
    assert_dump(lines, n, verify_all)


def test_injected_store_is_seen_in_device_memory(binary):
    """A gather that recomputed 2*idx[j]+1, or a touch whose stores went
    nowhere the gather reads, would not show the 1."""
    rc, lines, err, _ = run_dump(binary, 4099, "--inject-store", 300,
                                 verify_all=True)
    assert_verify_failed(rc, lines, err, 300)
    assert (300, 300, INJECTED) in dumped_samples(lines)
    assert_dump(lines, 4099, True, injected={300})


def test_sampled_injection_at_a_stride_index(binary):
    rc, lines, err, _ = run_dump(binary, 65537, "--inject-store", 4099)
    assert_verify_failed(rc, lines, err, 4099)
    assert_dump(lines, 65537, False, injected={4099})


def test_sampled_injection_at_the_tail(binary):
    rc, lines, err, _ = run_dump(binary, 65537, "--inject-store", 65536)
    assert_verify_failed(rc, lines, err, "tail")
    assert_dump(lines, 65537, False, injected={65536})


def test_sampling_does_not_cover_an_unsampled_index(binary):
    """What a sampled run does not see: 4098 is in no sample set of 65537."""
    assert 4098 not in reference_sample_set(65537)
    rc, lines, err, _ = run_dump(binary, 65537, "--inject-store", 4098)
    assert rc == 0, (lines[-3:], err)
    assert len(ok_lines(lines)) == 1
    assert_dump(lines, 65537, False)


def test_verify_all_covers_the_unsampled_index(binary):
    rc, lines, err, _ = run_dump(binary, 65537, "--inject-store", 4098,
                                 verify_all=True)
    assert_verify_failed(rc, lines, err, 4098)
    assert_dump(lines, 65537, True, injected={4098})


def test_duplicate_index_reports_its_first_position(binary):
    """n=4100 samples 4099 twice, as a stride index and as the tail."""
    rc, lines, err, _ = run_dump(binary, 4100, "--inject-store", 4099)
    assert_verify_failed(rc, lines, err, 4099)
    assert dumped_samples(lines)[1:] == [(1, 4099, INJECTED),
                                         (2, 4099, INJECTED)]
    assert_dump(lines, 4100, False, injected={4099})


def test_lowest_failing_position_is_reported(binary):
    rc, lines, err, _ = run_dump(binary, 257, "--inject-store", 256,
                                 "--inject-store", 3, verify_all=True)
    assert_verify_failed(rc, lines, err, 3)
    rows = dumped_samples(lines)
    assert rows[3] == (3, 3, INJECTED) and rows[256] == (256, 256, INJECTED)
    assert_dump(lines, 257, True, injected={3, 256})


# the last lane of the first block; the one live lane of the tail block
@pytest.mark.parametrize("at", [255, 256])
def test_injection_at_a_block_boundary(binary, at):
    rc, lines, err, _ = run_dump(binary, 257, "--inject-store", at,
                                 verify_all=True)
    assert_verify_failed(rc, lines, err, at)
    assert_dump(lines, 257, True, injected={at})


def _visible_gpus():
    """The devices this process may use, as ROCR_VISIBLE_DEVICES entries."""
    if os.environ.get("ROCR_VISIBLE_DEVICES", "").strip():
        return [e.strip() for e in os.environ["ROCR_VISIBLE_DEVICES"].split(",")
                if e.strip()]
    from k8s_runpod_kubelet_amd.gpu.inventory import Inventory

    found = Inventory(sysfs_root="/sys", allow_synthetic=False).discover()
    return [str(k) for k in range(len(found))]


def test_two_devices_each_store_the_reference(binary):
    """The queue, executable, allocations and access grants are rebuilt per
    device; the second pass gets the same scrutiny as the first."""
    gpus = _visible_gpus()
    if len(gpus) < 2:
        pytest.skip(f"needs two visible GPUs, have {len(gpus)}")
    rc, lines, err, _ = run_gpu(
        binary, "--expect-gpus", 2, "--run-for", 0, "--verify-all",
        "--touch-elems", 257, "--dump-samples", visible=",".join(gpus[:2]))
    assert rc == 0, (lines[-3:], err)
    reports = ok_lines(lines)
    assert len(reports) == 2, reports
    assert reports[0].startswith("podworker: dev 0 ")
    assert reports[1].startswith("podworker: dev 1 ")
    for dev in (0, 1):
        assert_dump(lines, 257, True, dev=dev)
    assert len([ln for ln in lines
                if ln.startswith("podworker: sample ")]) == 2 * 257
