"""Active GPU self-test: runner and manager for the ``gpucheck`` binary.

The passive health signal (sysfs/RAS, ``Inventory.refresh_dynamic``) cannot
see a GPU that still enumerates but no longer stores bits or multiplies
matrices. ``gpucheck`` (ops/gpucheck/gpucheck.hip) runs real work on an idle
GPU — an HBM pattern fill/verify, a copy-bandwidth measurement, an exact
MFMA self-test, an exact self-test of the block-scaled MX (FP8/BF8/FP4)
matrix path, a per-CU LDS self-test that names the compute unit of a
fault and an exact self-test of the dense matrix formats (F16, BF16 16x16,
FP8, BF8, INT8, F32, F64) with their rates — and this module turns its
verdict into the per-GPU schedulability gate.

The binary always runs as a fresh child process scoped to one GPU, exactly
like a pod (``device_env``); the kubelet process itself never opens the GPU.
Everything here is off unless configured (``gpu_check_on_start``,
``gpu_check_interval_s``) or triggered by an operator (``POST /gpucheck/<i>``
or ``python -m k8s_runpod_kubelet_amd.gpu.diagnostics --gpu 0``).
"""

from __future__ import annotations

import json
import logging
import os
import signal
import subprocess
import threading
import time
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence

from .binder import device_env

log = logging.getLogger("gpu.diagnostics")

# gpucheck exit codes (ops/gpucheck/gpucheck.hip)
EXIT_STAGES = {2: "usage", 11: "hip", 20: "hbm", 21: "mfma", 22: "bandwidth",
               23: "copy", 24: "mx", 25: "mx_rate", 26: "lds",
               27: "lds_coverage", 28: "dense", 29: "dense_rate"}
MX_FORMATS = ("fp8", "bf8", "fp4", "fp8xfp4")
DENSE_FORMATS = ("f16", "bf16x16", "fp8", "bf8", "i8", "f32", "f64")
RESERVATION_PREFIX = "amdvk-system/gpucheck-"


class GpuBusyError(Exception):
    """The GPU is bound to a pod, or a check is already running on it."""


class UnknownGpuError(Exception):
    pass


@dataclass
class GpuCheckResult:
    gpu: int
    ok: bool
    exit_code: Optional[int] = None
    # "" on a pass; otherwise the failing stage ("hbm", "copy", "mfma",
    # "mx", "lds", "dense", "bandwidth", "mx_rate", "dense_rate",
    # "lds_coverage", "hip", "usage")
    # or "timeout", "signal N", "bad-output".
    reason: str = ""
    data: Dict[str, Any] = field(default_factory=dict)  # the binary's JSON
    duration_s: float = 0.0
    timestamp: float = 0.0  # wall clock at completion

    def to_dict(self) -> Dict[str, Any]:
        out = dict(self.data)
        out.update({
            "gpu": self.gpu,
            "ok": self.ok,
            "exit_code": self.exit_code,
            "reason": self.reason,
            "duration_s": round(self.duration_s, 4),
            "timestamp": self.timestamp,
        })
        return out


def _floor_args(floors, formats, flag: str, what: str) -> List[str]:
    floors = dict(floors or {})
    unknown = sorted(set(floors) - set(formats))
    if unknown:
        raise ValueError(f"unknown {what} format(s) {unknown}; "
                         f"expected {list(formats)}")
    out: List[str] = []
    for name in formats:
        floor = float(floors.get(name) or 0.0)
        if floor > 0:
            out += [flag, f"{name}:{floor!r}"]
    return out


def mx_floor_args(floors) -> List[str]:
    """{format: TFLOP/s floor} -> ``--min-mx-tflops`` flags, in the binary's
    format order; floors of 0 are off. Raises ``ValueError`` for an unknown
    format."""
    return _floor_args(floors, MX_FORMATS, "--min-mx-tflops", "MX")


def dense_floor_args(floors) -> List[str]:
    """The same for the dense formats and ``--min-dense-tflops``."""
    return _floor_args(floors, DENSE_FORMATS, "--min-dense-tflops", "dense")


def first_bad_mx(data: Dict[str, Any]) -> str:
    """"fp4 wave 17" for the first format with a bad wave in the binary's
    JSON, or ""."""
    formats = data.get("mx_formats")
    if isinstance(formats, dict):
        for name, got in formats.items():
            if isinstance(got, dict) and got.get("bad_waves"):
                return f"{name} wave {got.get('first_bad_wave')}"
    return ""


def first_bad_dense(data: Dict[str, Any]) -> str:
    """"i8 wave 17 on xcc2.se1.sh0.cu5" for the first dense format with a
    bad wave in the binary's JSON (without the compute unit where the binary
    names none), or ""."""
    formats = data.get("dense_formats")
    if isinstance(formats, dict):
        for name, got in formats.items():
            if isinstance(got, dict) and got.get("bad_waves"):
                where = got.get("first_bad_where")
                return (f"{name} wave {got.get('first_bad_wave')}"
                        + (f" on {where}" if where else ""))
    return ""


def first_bad_lds(data: Dict[str, Any]) -> str:
    """"xcc2.se1.sh0.cu5 offset 65536 xor 00..01" for the first compute unit
    with a bad LDS vector in the binary's JSON, or ""."""
    cus = data.get("lds_bad_cus")
    if isinstance(cus, list):
        for cu in cus:
            if isinstance(cu, dict) and cu.get("bad_vectors"):
                return (f"{cu.get('where')} offset {cu.get('first_bad_offset')} "
                        f"xor {cu.get('first_bad_xor')}")
    return ""


def _kill_group(proc: subprocess.Popen) -> None:
    try:
        os.killpg(proc.pid, signal.SIGKILL)
    except (ProcessLookupError, PermissionError):
        pass


def run_gpucheck(gpu, inventory, *, nbytes: int, timeout_s: float,
                 extra_args: Sequence[str] = (),
                 binary: Optional[str] = None) -> GpuCheckResult:
    """Run one check on ``gpu`` (an index or a ``Gpu``) as a fresh child
    process and map the outcome to a ``GpuCheckResult``. Never retries."""
    index = int(getattr(gpu, "index", gpu))
    if binary is None:
        from ..ops import gpucheck_binary

        binary = gpucheck_binary()
    # Same scoping as a pod (runtime/process_runtime.py): drop whatever the
    # kubelet inherited, then expose exactly this GPU as device 0.
    env = dict(os.environ)
    env.pop("ROCR_VISIBLE_DEVICES", None)
    env.pop("HIP_VISIBLE_DEVICES", None)
    env.update(device_env([index], inventory))
    argv = [binary, "--bytes", str(int(nbytes)), *[str(a) for a in extra_args]]

    t0 = time.monotonic()
    proc = subprocess.Popen(
        argv, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
        stderr=subprocess.PIPE, start_new_session=True)
    timed_out = False
    try:
        stdout, stderr = proc.communicate(timeout=timeout_s)
    except subprocess.TimeoutExpired:
        timed_out = True
        _kill_group(proc)
        stdout, stderr = proc.communicate()
    except BaseException:
        _kill_group(proc)
        proc.wait()
        raise
    result = GpuCheckResult(gpu=index, ok=False, exit_code=proc.returncode,
                            duration_s=time.monotonic() - t0,
                            timestamp=time.time())
    if timed_out:
        result.exit_code = None
        result.reason = "timeout"
        return result
    if proc.returncode < 0:
        result.reason = f"signal {-proc.returncode}"
        return result

    lines = [ln for ln in stdout.decode("utf-8", "replace").splitlines()
             if ln.strip()]
    try:
        data = json.loads(lines[-1]) if lines else None
    except ValueError:
        data = None
    if not isinstance(data, dict):
        result.reason = "bad-output"
        tail = stderr.decode("utf-8", "replace").strip().splitlines()[-3:]
        if tail:
            result.data = {"stderr": " | ".join(tail)}
        return result
    result.data = data
    if proc.returncode == 0 and data.get("ok") is True:
        result.ok = True
    else:
        result.reason = EXIT_STAGES.get(proc.returncode,
                                        f"exit {proc.returncode}")
    return result


Runner = Callable[..., GpuCheckResult]


class DiagnosticsManager:
    """Runs checks against idle GPUs and gates placement on the verdict.

    While a schedulable GPU is being checked it holds an ordinary ledger
    reservation (``amdvk-system/gpucheck-<idx>``), so the binder cannot place
    a pod on it; releasing the reservation stamps ``last_freed_at`` and the
    binder's settle preference applies as after any pod. A failed check sets
    ``Gpu.diag_ok = False``; only a passing operator-triggered check clears
    it."""

    def __init__(self, ledger, inventory, config, runner: Runner = run_gpucheck,
                 recorder=None, node_name: str = ""):
        self.ledger = ledger
        self.inventory = inventory
        self.config = config
        self.runner = runner
        self.recorder = recorder
        self.node_name = node_name or getattr(config, "node_name", "")
        self._lock = threading.Lock()
        self._running: set = set()
        self._last_checked: Dict[int, float] = {}  # monotonic
        self._slots = threading.BoundedSemaphore(
            max(1, int(getattr(config, "gpu_check_parallel", 2))))

    # -- single check ---------------------------------------------------

    def _extra_args(self) -> List[str]:
        floor = float(getattr(self.config, "gpu_check_min_copy_gbs", 0.0) or 0.0)
        args = ["--min-copy-gbs", repr(floor)] if floor > 0 else []
        if not getattr(self.config, "gpu_check_mx", True):
            args += ["--mx-waves", "0"]
        else:
            args += mx_floor_args(
                getattr(self.config, "gpu_check_min_mx_tflops", None))
        if not getattr(self.config, "gpu_check_dense", True):
            args += ["--dense-waves", "0"]
        else:
            args += dense_floor_args(
                getattr(self.config, "gpu_check_min_dense_tflops", None))
        if not getattr(self.config, "gpu_check_lds", True):
            args += ["--lds-groups", "0"]
        if getattr(self.config, "gpu_check_lds_require_coverage", False):
            args += ["--lds-require-coverage"]
        return args

    def check(self, idx: int, operator: bool = False) -> GpuCheckResult:
        """Check one idle GPU. Raises ``UnknownGpuError`` / ``GpuBusyError``.
        ``operator=True`` marks an operator-triggered check, the only kind
        whose pass clears an earlier failure."""
        state = self.ledger.get_state(idx)
        if state is None:
            raise UnknownGpuError(f"no GPU {idx}")
        with self._lock:
            if idx in self._running:
                raise GpuBusyError(f"a check is already running on GPU {idx}")
            self._running.add(idx)
        nbytes = int(self.config.gpu_check_bytes)
        key = f"{RESERVATION_PREFIX}{idx}"
        reserved = False
        try:
            if state.occupied:
                raise GpuBusyError(f"GPU {idx} is bound to {state.pod_keys}")
            if state.schedulable:
                try:
                    self.ledger.reserve(key, [idx], nbytes)
                except ValueError as exc:  # lost a race with the binder
                    raise GpuBusyError(str(exc)) from exc
                reserved = True
            # An unschedulable GPU (failed earlier, cordoned, unhealthy)
            # cannot receive a pod, so the in-progress mark is enough.
            with self._slots:
                result = self.runner(
                    idx, self.inventory, nbytes=nbytes,
                    timeout_s=float(self.config.gpu_check_timeout_s),
                    extra_args=self._extra_args())
            # Verdict first, release second: a failed GPU is never
            # schedulable in between.
            self._record(idx, result, operator)
        finally:
            if reserved:
                self.ledger.release(key)
            with self._lock:
                self._running.discard(idx)
        return result

    def _record(self, idx: int, result: GpuCheckResult, operator: bool) -> None:
        from ..server import metrics

        state = self.ledger.get_state(idx)
        was_ok = state.gpu.diag_ok if state is not None else True
        with self._lock:
            self._last_checked[idx] = time.monotonic()
        if result.ok:
            if was_ok or operator:
                self.ledger.set_diag(idx, True, "", result.to_dict())
            else:
                self.ledger.set_diag(idx, False, state.gpu.diag_reason,
                                     result.to_dict())
        else:
            self.ledger.set_diag(idx, False, result.reason, result.to_dict())
            metrics.gpu_check_failures.labels(str(idx), result.reason).inc()
            log.warning("gpu self-test failed",
                        extra={"gpu": idx, "reason": result.reason,
                               "first_bad_offset":
                                   result.data.get("first_bad_offset")})
            self._emit_event(idx, result)
        state = self.ledger.get_state(idx)
        metrics.observe_gpu_check(idx, result,
                                  state.gpu.diag_ok if state else result.ok)

    def _emit_event(self, idx: int, result: GpuCheckResult) -> None:
        if self.recorder is None:
            return
        node = {"kind": "Node",
                "metadata": {"name": self.node_name, "namespace": "default"}}
        where = first_bad_mx(result.data) if result.reason == "mx" else ""
        lds = first_bad_lds(result.data) if result.reason == "lds" else ""
        dense = (first_bad_dense(result.data) if result.reason == "dense"
                 else "")
        message = (f"GPU {idx} failed self-test: stage={result.reason} "
                   + (f"first_bad_mx={where} " if where else "")
                   + (f"lds: {lds} " if lds else "")
                   + (f"first_bad_dense={dense} " if dense else "") +
                   f"first_bad_offset={result.data.get('first_bad_offset')} "
                   f"mismatch_vectors={result.data.get('mismatch_vectors')}; "
                   f"GPU fenced until an operator re-check passes")
        try:
            self.recorder.event(node, "Warning", "GpuCheckFailed", message)
        except Exception:
            log.exception("could not emit GpuCheckFailed event")

    # -- sweeps ---------------------------------------------------------

    def _idle_candidates(self, max_age_s: Optional[float]) -> List[int]:
        now = time.monotonic()
        out = []
        for state in self.ledger.snapshot():
            idx = state.gpu.index
            # Failed GPUs wait for an operator; occupied, cordoned and
            # RAS-unhealthy ones are left alone.
            if not state.gpu.diag_ok or state.occupied or not state.schedulable:
                continue
            with self._lock:
                last = self._last_checked.get(idx)
                running = idx in self._running
            if running:
                continue
            if max_age_s is not None and last is not None \
                    and now - last < max_age_s:
                continue
            out.append(idx)
        return out

    def _sweep(self, indices: List[int]) -> List[GpuCheckResult]:
        results: List[GpuCheckResult] = []
        res_lock = threading.Lock()

        def one(idx: int) -> None:
            try:
                r = self.check(idx)
            except (GpuBusyError, UnknownGpuError) as exc:
                log.info("gpu self-test skipped",
                         extra={"gpu": idx, "why": str(exc)})
                return
            with res_lock:
                results.append(r)

        # check() itself bounds concurrency with gpu_check_parallel.
        threads = [threading.Thread(target=one, args=(i,),
                                    name=f"gpucheck-{i}", daemon=True)
                   for i in indices]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        return sorted(results, key=lambda r: r.gpu)

    def check_all_idle(self) -> List[GpuCheckResult]:
        """Start-up sweep: every idle, schedulable GPU."""
        return self._sweep(self._idle_candidates(None))

    def periodic(self) -> List[GpuCheckResult]:
        """One periodic pass: idle GPUs whose last check is older than
        ``gpu_check_interval_s``. No-op when the interval is 0."""
        interval = float(getattr(self.config, "gpu_check_interval_s", 0) or 0)
        if interval <= 0:
            return []
        return self._sweep(self._idle_candidates(interval))

    def last_results(self) -> Dict[str, Any]:
        return {
            str(s.gpu.index): {
                "ok": s.gpu.diag_ok,
                "reason": s.gpu.diag_reason,
                "lastCheck": s.gpu.diag_last,
            }
            for s in self.ledger.snapshot()
        }


# ----------------------------------------------------------- operator CLI

def parse_size(text: str) -> int:
    """"4G", "512M", "4096" -> bytes (binary multiples)."""
    t = text.strip()
    mult = 1
    if t and t[-1] in "bB":
        t = t[:-1]
    if t and t[-1] == "i":
        t = t[:-1]
    if t and t[-1].upper() in "KMGT":
        mult = 1024 ** ("KMGT".index(t[-1].upper()) + 1)
        t = t[:-1]
    return int(t, 0) * mult


def main(argv=None) -> int:
    import argparse
    import sys

    from .inventory import Inventory

    p = argparse.ArgumentParser(
        prog="python -m k8s_runpod_kubelet_amd.gpu.diagnostics",
        description="Run the active GPU self-test on one GPU and print its "
                    "JSON. Exits with the gpucheck exit code (0 pass, 20 HBM, "
                    "23 copy mismatch, 21 MFMA, 24 MX mismatch, 26 LDS "
                    "mismatch, 28 dense mismatch, 22 bandwidth, 25 MX rate "
                    "below its floor, 29 dense rate below its floor, "
                    "27 LDS coverage partial, 11 HIP error; 1 for a "
                    "timeout, signal or unparsable output).")
    p.add_argument("--gpu", type=int, required=True)
    p.add_argument("--bytes", default="1G")
    p.add_argument("--timeout", type=float, default=60.0)
    p.add_argument("--min-copy-gbs", type=float, default=0.0)
    p.add_argument("--min-mx-tflops", action="append", default=[],
                   metavar="FORMAT:X",
                   help="fail if the MX rate of FORMAT (fp8, bf8, fp4, "
                        "fp8xfp4) is below X TFLOP/s; repeatable")
    p.add_argument("--min-dense-tflops", action="append", default=[],
                   metavar="FORMAT:X",
                   help="fail if the dense rate of FORMAT (f16, bf16x16, "
                        "fp8, bf8, i8, f32, f64) is below X TFLOP/s; "
                        "repeatable")
    p.add_argument("--no-lds", action="store_true",
                   help="skip the per-CU LDS stage")
    p.add_argument("--lds-require-coverage", action="store_true",
                   help="fail (27) unless every compute unit's LDS was tested")
    p.add_argument("--sysfs-root", default="/sys")
    p.add_argument("extra", nargs="*",
                   help="further gpucheck arguments (after --)")
    args = p.parse_args(argv)

    inventory = Inventory(sysfs_root=args.sysfs_root, allow_synthetic=True)
    inventory.discover()
    if inventory.get(args.gpu) is None:
        print(f"no GPU {args.gpu}", file=sys.stderr)
        return 2
    extra = list(args.extra)
    if args.min_copy_gbs > 0:
        extra += ["--min-copy-gbs", repr(args.min_copy_gbs)]
    for floor in args.min_mx_tflops:
        extra += ["--min-mx-tflops", floor]
    for floor in args.min_dense_tflops:
        extra += ["--min-dense-tflops", floor]
    if args.no_lds:
        extra += ["--lds-groups", "0"]
    if args.lds_require_coverage:
        extra += ["--lds-require-coverage"]
    result = run_gpucheck(args.gpu, inventory, nbytes=parse_size(args.bytes),
                          timeout_s=args.timeout, extra_args=extra)
    print(json.dumps(result.to_dict(), sort_keys=True))
    if result.exit_code is not None and result.exit_code >= 0 \
            and result.reason != "bad-output":
        return result.exit_code
    return 1


if __name__ == "__main__":
    raise SystemExit(main())
