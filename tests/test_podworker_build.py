"""The podworker binary as built: a plain C++ host program on ROCr with its
gfx950 code object embedded, no HIP runtime in the process. Everything here
runs without a GPU."""

import os
import re
import subprocess
import time

import pytest

from tests.podworker_reference import reference_sample_set


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


# ---- the sample set, against an independent statement of the rule ----------

def parse_sample_set(stdout):
    """-> (m from the header line, the indices in printed order); checks the
    layout: one header, then 16 indices per line, nothing else."""
    lines = stdout.splitlines()
    header = re.fullmatch(r"podworker: sample-set m=(\d+)", lines[0])
    assert header, lines[0]
    indices = []
    for k, ln in enumerate(lines[1:]):
        assert ln.startswith("podworker: sample-set "), ln
        row = [int(tok) for tok in ln.split()[2:]]
        assert len(row) == 16 or (k == len(lines) - 2 and 1 <= len(row) < 16), ln
        indices += row
    return int(header.group(1)), indices


SAMPLED_SIZES = [1, 2, 4099, 4100, 65536, 65537, 1 << 20, (1 << 28) - 1,
                 1 << 28]


@pytest.mark.parametrize("n,verify_all",
                         [(n, False) for n in SAMPLED_SIZES]
                         + [(1, True), (257, True)])
def test_dumped_sample_set_follows_the_rule(binary, n, verify_all):
    flags = ["--verify-all"] if verify_all else []
    # --expect-gpus shows that the dump leaves before the GPU section
    proc = run(binary, "--expect-gpus", 1, "--dump-sample-set", *flags,
               "--touch-elems", n)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    assert proc.stderr == ""
    m, indices = parse_sample_set(proc.stdout)
    expected = reference_sample_set(n, verify_all)
    assert m == len(expected) == len(indices)
    assert indices == expected
    assert indices[-1] == n - 1


def test_reference_sample_set_edge_cases():
    """The Python rule itself, at the cases where it is easy to get wrong."""
    assert reference_sample_set(1) == [0, 0]
    assert reference_sample_set(4100) == [0, 4099, 4099]
    assert reference_sample_set(4099) == [0, 4098]
    assert reference_sample_set(65537) == (
        [4099 * k for k in range(16)] + [65536])
    assert reference_sample_set(1 << 28)[-2:] == [61485, (1 << 28) - 1]
    assert reference_sample_set(3, verify_all=True) == [0, 1, 2]


@pytest.mark.parametrize("flag,args", [
    ("--inject-store", ("--inject-store", 0)),
    ("--inject-store", ("--touch-elems", 4099, "--inject-store", 4099)),
    ("--inject-store", ("--touch-elems", 1, "--inject-store", 1)),
    ("--inject-store", ("--inject-store", 1, "--inject-store", 2,
                        "--inject-store", 3, "--inject-store", 4,
                        "--inject-store", 5)),
    ("--dump-samples", ("--dump-samples", "--verify-all", "--touch-elems",
                        200000)),
], ids=["inject-0", "inject-n", "inject-into-one-element", "fifth-inject",
        "dump-too-many"])
def test_test_only_flags_are_validated(binary, flag, args):
    proc = run(binary, *args)
    assert proc.returncode == 2, (proc.stdout, proc.stderr)
    assert proc.stderr.startswith(f"podworker: {flag} "), proc.stderr
    assert proc.stdout == ""


def test_four_injections_and_a_small_dump_are_accepted(binary):
    """The limits sit where the issue puts them: four injections, and
    1<<17 dumped samples, pass validation (CPU mode: nothing is dispatched)."""
    proc = run(binary, "--inject-store", 1, "--inject-store", 2,
               "--inject-store", 3, "--inject-store", (1 << 20) - 1,
               "--dump-samples", "--verify-all", "--touch-elems", 1 << 17)
    assert proc.returncode == 2, proc.stderr  # 2**20-1 >= 2**17
    proc = run(binary, "--inject-store", 1, "--inject-store", 2,
               "--inject-store", 3, "--inject-store", (1 << 17) - 1,
               "--dump-samples", "--verify-all", "--touch-elems", 1 << 17)
    assert proc.returncode == 0, proc.stderr


# ---- the metadata of the code object that was actually built ---------------

def _scalar(text):
    text = text.strip()
    return int(text) if re.fullmatch(r"-?\d+", text) else text


def parse_kernel_metadata(notes):
    """{kernel name: {key: value, ".args": [{key: value}]}} from the text of
    llvm-readelf --notes; written for this test, independent of build.py."""
    body = notes.split("amdhsa.kernels:\n", 1)[1]
    kernels, entry, arg, in_args = {}, None, None, False
    for line in body.splitlines():
        if not line.startswith("  "):
            break  # the next top-level key ends the kernel list
        if line.startswith("  - "):
            entry, in_args = {".args": []}, False
            kernels[len(kernels)] = entry
            line = "    " + line[4:]
        indent = len(line) - len(line.lstrip())
        text = line.strip()
        if indent == 4:
            key, _, value = text.partition(":")
            in_args = key == ".args"
            if not in_args:
                entry[key] = _scalar(value)
        elif in_args and indent >= 6:
            if text.startswith("- "):
                arg = {}
                entry[".args"].append(arg)
                text = text[2:]
            key, _, value = text.partition(":")
            arg[key] = _scalar(value)
    return {k[".name"]: k for k in kernels.values()}


@pytest.fixture(scope="module")
def built_notes(binary):
    from k8s_runpod_kubelet_amd.ops import build as build_mod

    readelf = subprocess.run(
        [build_mod.HIPCC, "-print-prog-name=llvm-readelf"], check=True,
        capture_output=True, text=True).stdout.strip()
    code_object = build_mod.PODWORKER_DIR / "podworker_kernels.co"
    return subprocess.run([readelf, "--notes", str(code_object)], check=True,
                          capture_output=True, text=True).stdout


@pytest.mark.parametrize("kernel,segment_size,offsets,inc_array", [
    ("touch_kernel", 12, [0, 8], "kTouchArgOffsets"),
    ("gather_kernel", 28, [0, 8, 16, 24], "kGatherArgOffsets"),
])
def test_built_code_object_metadata(built_notes, kernel, segment_size,
                                    offsets, inc_array):
    from k8s_runpod_kubelet_amd.ops import build as build_mod

    meta = parse_kernel_metadata(built_notes)
    assert set(meta) == {"touch_kernel", "gather_kernel"}
    k = meta[kernel]
    kinds = [a[".value_kind"] for a in k[".args"]]
    # the host fills in no hidden arguments: the kernels must ask for none
    assert not [v for v in kinds if v.startswith("hidden_")], kinds
    assert k[".kernarg_segment_size"] == segment_size
    assert [a[".offset"] for a in k[".args"]] == offsets
    assert build_mod._kernarg_offsets(built_notes)[kernel] == offsets
    inc = (build_mod.PODWORKER_DIR / "podworker_kernels.inc").read_text()
    written = re.search(
        rf"^static const size_t {inc_array}\[\] = \{{([^}}]*)\}};$", inc,
        flags=re.M)
    assert written, inc_array
    assert [int(v) for v in written.group(1).split(",")] == offsets
    assert k[".max_flat_workgroup_size"] == 256
    assert k[".group_segment_fixed_size"] == 0
    assert k[".private_segment_fixed_size"] == 0
    assert k[".uses_dynamic_stack"] == "false"
    assert k[".wavefront_size"] == 64
    assert k[".symbol"] == kernel + ".kd"


def test_metadata_parser_sees_hidden_arguments():
    """The test's own parser on a kernel that does have hidden arguments, so
    the 'none' above is not the parser's blindness."""
    notes = """\
amdhsa.kernels:
  - .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         16
        .size:           4
        .value_kind:     hidden_block_count_x
    .kernarg_segment_size: 272
    .name:           k
    .uses_dynamic_stack: false
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""
    k = parse_kernel_metadata(notes)["k"]
    assert [a[".value_kind"] for a in k[".args"]] == [
        "global_buffer", "hidden_block_count_x"]
    assert k[".kernarg_segment_size"] == 272
    assert k[".uses_dynamic_stack"] == "false"


def test_kernarg_offsets_rejects_an_entry_without_a_name():
    from k8s_runpod_kubelet_amd.ops import build as build_mod

    notes = """\
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .kernarg_segment_size: 8
    .symbol:         touch_kernel.kd
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""
    with pytest.raises(RuntimeError, match=r"without a \.name"):
        build_mod._kernarg_offsets(notes)


def test_write_kernels_inc_rejects_a_wrong_argument_count(tmp_path):
    from k8s_runpod_kubelet_amd.ops import build as build_mod

    def kernel(name, offsets):
        args = "".join(f"      - .offset:         {o}\n"
                       f"        .size:           8\n"
                       f"        .value_kind:     global_buffer\n"
                       for o in offsets)
        return (f"  - .agpr_count:     0\n    .args:\n{args}"
                f"    .name:           {name}\n")

    notes = ("amdhsa.kernels:\n" + kernel("touch_kernel", [0, 8])
             + kernel("gather_kernel", [0, 8, 16])
             + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n")
    code_object = tmp_path / "podworker_kernels.co"
    code_object.write_bytes(b"\x7fELF")
    inc = tmp_path / "podworker_kernels.inc"
    with pytest.raises(RuntimeError, match="gather_kernel"):
        build_mod._write_kernels_inc(code_object, notes, inc)
    assert not inc.exists()
    # the same metadata with the fourth argument back is accepted
    notes = notes.replace(kernel("gather_kernel", [0, 8, 16]),
                          kernel("gather_kernel", [0, 8, 16, 24]))
    build_mod._write_kernels_inc(code_object, notes, inc)
    assert "kGatherArgOffsets[] = {0, 8, 16, 24};" in inc.read_text()
