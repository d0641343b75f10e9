"""The ROCr podworker on a real MI355X: both kernels through the AQL queue at
the sizes where the index arithmetic, the tail block or the sample set can go
wrong, the report line, the count mismatch, the timing switch and SIGTERM.

Expected values are the closed form 2*i+1 mod 2**32, checked by the binary
itself (--verify-all brings every element back through the gather kernel), so
nothing here needs a tolerance.

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


def run_gpu(binary, *args, env=None):
    """-> (exit code, stdout lines, stderr, wall seconds)."""
    argv = [binary, *map(str, args)]
    child_env = _one_gpu_env(**(env or {}))
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
