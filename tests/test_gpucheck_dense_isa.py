"""What gpucheck's timed rate loops contain, read from the compiled gfx950
code: needs the compiler the build needs, no GPU.

A rate figure is the MFMA issue rate only if the timed loop issues nothing
but the MFMAs. hipcc is free to keep the loop-carried accumulators in VGPRs
and copy them to and from the MFMAs' accumulation registers on every trip;
it did that for two of the seven formats, which halved their figures without
any test noticing. So the device code is compiled the way the build compiles
it and every rate kernel's loop is held to: four MFMAs of the format's
instruction, the scalar loop counter (add, compare, branch) and at most one
s_nop; no vector instruction besides the MFMAs."""

import collections
import re
import subprocess

import pytest

from k8s_runpod_kubelet_amd.gpu.diagnostics import DENSE_FORMATS, MX_FORMATS
from k8s_runpod_kubelet_amd.ops import build

DENSE_MNEMONICS = {
    "f16": "v_mfma_f32_32x32x16_f16",
    "bf16x16": "v_mfma_f32_16x16x32_bf16",
    "fp8": "v_mfma_f32_32x32x16_fp8_fp8",
    "bf8": "v_mfma_f32_32x32x16_bf8_bf8",
    "i8": "v_mfma_i32_32x32x32_i8",
    "f32": "v_mfma_f32_32x32x2_f32",
    "f64": "v_mfma_f64_16x16x4_f64",
}
MX_MNEMONIC = "v_mfma_scale_f32_32x32x64_f8f6f4"


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    """{(kernel, format index): Counter of the mnemonics in its loop}."""
    out = tmp_path_factory.mktemp("isa") / "gpucheck.s"
    subprocess.run(
        [build.HIPCC, f"--offload-arch={build.GFX_ARCH}", "-O2", "-std=c++17",
         "-S", "--cuda-device-only",
         str(build.GPUCHECK_DIR / "gpucheck.hip"), "-o", str(out)],
        check=True, capture_output=True, timeout=600)
    lines = out.read_text().splitlines()
    found = {}
    for start, line in enumerate(lines):
        head = re.match(r"^_ZN\S*?(dense_rate|mx_rate)ILi(\d+)E\S*:", line)
        if not head:
            continue
        end = next(i for i in range(start, len(lines))
                   if "s_endpgm" in lines[i])
        labels = {}
        for i in range(start, end):
            label = re.match(r"^(\.LBB\d+_\d+):", lines[i])
            if label:
                labels[label.group(1)] = i
        bodies = []
        for i in range(start, end):
            branch = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", lines[i])
            if branch and labels.get(branch.group(1), end) < i:  # backward
                body = [ln.split(";")[0].strip()
                        for ln in lines[labels[branch.group(1)] + 1:i + 1]]
                bodies.append(collections.Counter(
                    ln.split()[0] for ln in body
                    if ln and not ln.startswith(".")))
        assert len(bodies) == 1, (line, bodies)   # one loop: the timed one
        found[(head.group(1), int(head.group(2)))] = bodies[0]
    return found


def expect_bare_loop(ops, mnemonic):
    print(mnemonic, dict(ops))
    assert ops[mnemonic] == 4
    vector = {op: n for op, n in ops.items()
              if op.startswith(("v_", "ds_", "global_", "buffer_", "flat_",
                                "scratch_"))}
    assert vector == {mnemonic: 4}, "the loop issues more than its MFMAs"
    assert ops["s_nop"] <= 1
    assert set(ops) <= {mnemonic, "s_nop", "s_add_i32", "s_sub_i32",
                        "s_add_u32", "s_sub_u32", "s_cmp_eq_u32",
                        "s_cmp_lg_u32", "s_cmp_eq_i32", "s_cmp_lg_i32",
                        "s_cbranch_scc0", "s_cbranch_scc1"}, dict(ops)
    assert sum(ops.values()) <= 8


@pytest.mark.parametrize("fmt", DENSE_FORMATS)
def test_dense_rate_loop_is_mfmas_and_a_counter(loops, fmt):
    expect_bare_loop(loops[("dense_rate", DENSE_FORMATS.index(fmt))],
                     DENSE_MNEMONICS[fmt])


def test_every_rate_kernel_was_found(loops):
    assert sorted(loops) == (
        [("dense_rate", i) for i in range(len(DENSE_FORMATS))]
        + [("mx_rate", i) for i in range(len(MX_FORMATS))])


@pytest.mark.parametrize("fmt", MX_FORMATS)
def test_mx_rate_loop_is_mfmas_and_a_counter(loops, fmt):
    expect_bare_loop(loops[("mx_rate", MX_FORMATS.index(fmt))], MX_MNEMONIC)
