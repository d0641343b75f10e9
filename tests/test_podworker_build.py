"""The podworker binary as built: a plain C++ host program on ROCr with its
gfx950 code object embedded, no HIP runtime in the process. Everything here
runs without a GPU."""

import os
import subprocess
import time

import pytest


@pytest.fixture(scope="module")
def binary():
    from k8s_runpod_kubelet_amd.ops import build as build_mod

    path = build_mod.build_podworker(force=True)
    assert path.exists()
    return str(path)


def run(binary, *args, timeout=30):
    return subprocess.run([binary, *map(str, args)], stdin=subprocess.DEVNULL,
                          capture_output=True, text=True, timeout=timeout)


def test_links_rocr_and_not_the_hip_runtime(binary):
    ldd = subprocess.run(["ldd", binary], capture_output=True, text=True,
                         check=True).stdout
    assert "libhsa-runtime64" in ldd, ldd
    assert "libamdhip64" not in ldd, ldd
    assert "not found" not in ldd, ldd


def test_generated_include_carries_metadata_offsets():
    from k8s_runpod_kubelet_amd.ops import build as build_mod

    notes = """\
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         8
        .size:           4
        .value_kind:     by_value
      - .offset:         16
        .size:           4
        .value_kind:     hidden_block_count_x
    .kernarg_segment_size: 272
    .name:           touch_kernel
    .symbol:         touch_kernel.kd
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         24
        .size:           4
        .value_kind:     by_value
    .name:           other_kernel
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""
    assert build_mod._kernarg_offsets(notes) == {
        "touch_kernel": [0, 8], "other_kernel": [0, 24]}


def test_cpu_mode_reaches_ready_and_exits_with_exit_code(binary):
    proc = run(binary, "--exit-code", 7)
    assert proc.returncode == 7, proc.stderr
    lines = proc.stdout.splitlines()
    assert lines == ["podworker: ready (gpus=-1 ports=0)",
                     "podworker: exiting code=7"]


def test_without_kfd_gpu_mode_fails_fast_with_the_call_name(binary):
    if os.path.exists("/dev/kfd"):
        pytest.skip("/dev/kfd exists: the no-GPU failure path is not reachable")
    t0 = time.monotonic()
    proc = run(binary, "--expect-gpus", 1, "--run-for", 0, timeout=5)
    assert time.monotonic() - t0 < 5
    assert proc.returncode == 11, (proc.stdout, proc.stderr)
    assert "podworker: hsa_init() failed: " in proc.stderr, proc.stderr
    assert "podworker: ready" not in proc.stdout


def test_verify_all_refuses_more_than_a_mebi_element(binary):
    proc = run(binary, "--verify-all", "--touch-elems", 2000000)
    assert proc.returncode == 2, (proc.stdout, proc.stderr)
    assert "--verify-all" in proc.stderr
    assert "podworker: ready" not in proc.stdout


def test_touch_elems_must_be_positive(binary):
    proc = run(binary, "--touch-elems", 0)
    assert proc.returncode == 2, (proc.stdout, proc.stderr)
