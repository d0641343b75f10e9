"""What the gpucheck test files share: the build fixture and ``--cpu`` runner,
and for the GPU files the child runner and its guard.

Every GPU test starts the binary as a fresh child with a 60 s limit of its
own. Once a child ends with a HIP error (11), a signal or its time limit, every
later gpucheck GPU test skips, in whichever file it lives: nothing more is
started on a card that may be in trouble."""

import json
import os
import subprocess
import time

import pytest

CHILD_TIMEOUT_S = 60

_card_suspect = []  # reason, once a child ended badly; one list for all files


@pytest.fixture(scope="module")
def gpucheck():
    from k8s_runpod_kubelet_amd.ops import build

    path = build.build_gpucheck()
    assert path == build.gpucheck_path() and path.exists()
    assert os.access(path, os.X_OK)
    return str(path)


def run_cpu(binary, *args):
    """-> (exit code, parsed last stdout line or None)."""
    proc = subprocess.run([binary, "--cpu", *map(str, args)],
                          capture_output=True, text=True, timeout=60)
    lines = [ln for ln in proc.stdout.splitlines() if ln.strip()]
    return proc.returncode, (json.loads(lines[-1]) if lines else None)


@pytest.fixture(scope="module")
def binary():
    from k8s_runpod_kubelet_amd.ops import gpucheck_binary

    return gpucheck_binary()


def skip_if_card_suspect():
    if _card_suspect:
        pytest.skip(f"an earlier gpucheck child ended badly: {_card_suspect[0]}")


@pytest.fixture(autouse=True)
def _stop_after_trouble():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no /dev/kfd on this box")
    skip_if_card_suspect()


def run_gpu(binary, *args, hide=()):
    """-> (exit code, parsed last stdout line, wall seconds). The keys in
    `hide` are left out of the printed line."""
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
    shown = {k: v for k, v in data.items() if k not in hide}
    print(f"{' '.join(map(str, args))} -> rc={proc.returncode} "
          f"wall={wall:.3f}s {json.dumps(shown)}")
    return proc.returncode, data, wall
