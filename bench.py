#!/usr/bin/env python3
"""Flagship benchmark: GPU-pod scheduling throughput + pod-Ready latency.

Measures the BASELINE.json metric ("p50 pod-Ready latency + GPU-pods
scheduled/sec at 1/2/4/8 concurrent") on one node: an in-process apiserver
(hermetic, no cluster available in this environment — the reference's own
integration test needs a live cluster and cloud account and publishes no
numbers), the real informer → PodController → Provider pipeline,
and the real ProcessRuntime launching one HIP `podworker` per pod bound to
its GPU via ROCR_VISIBLE_DEVICES.

One *step* = a wave of N pods (one per GPU, each requesting 1×amd.com/gpu):
create all → wait all Ready (podworker initializes HIP on its bound GPU,
runs a gfx950 kernel, then signals readiness) → delete all → wait all gone.
Throughput counts the FULL lifecycle; latency is per-pod create→Ready.

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W
  torchrun --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
Under torchrun, rank 0 runs the kubelet stack managing GPUs 0..N-1 (one
kubelet per node is the product architecture); other ranks only participate
in barriers. Weak scaling: each extra GPU adds one pod per wave.

A plain run sets up, warms up, times the K waves and prints one JSON result
line. `--dump-outputs DIR` also writes what the last timed wave returned
(pod_state.npy, wave_summary.npy, workload_report.npy; float32; no timings,
so two builds can be compared file for file). `--full` is where measurements
beyond the headline figure belong; none exist today (`--burst` and
`--settle-gap` select other configurations and are runs of their own).
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO_ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO_ROOT)


def _dist_env():
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    return rank, world


def _barrier(dist, device_sync: bool):
    if device_sync:
        import torch

        torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    if device_sync:
        import torch

        torch.cuda.synchronize()


# Columns of pod_state.npy (one row per pod of the last timed wave, in
# creation order), read off the pod object the apiserver held at Ready.
POD_STATE_COLUMNS = (
    "phase_running", "cond_pod_scheduled", "cond_initialized", "cond_ready",
    "cond_containers_ready", "n_containers", "containers_ready",
    "containers_started", "containers_running", "restart_count",
    "gpus_requested", "gpus_bound",
)


def _pod_state_row(pod):
    status = pod.get("status", {})
    conds = {c["type"]: float(c["status"] == "True")
             for c in status.get("conditions", [])}
    cs = status.get("containerStatuses", [])
    requested = sum(
        int(c.get("resources", {}).get("limits", {}).get("amd.com/gpu", 0))
        for c in pod["spec"]["containers"])
    return [
        float(status.get("phase") == "Running"),
        conds.get("PodScheduled", 0.0), conds.get("Initialized", 0.0),
        conds.get("Ready", 0.0), conds.get("ContainersReady", 0.0),
        float(len(cs)),
        float(sum(bool(c.get("ready")) for c in cs)),
        float(sum(bool(c.get("started")) for c in cs)),
        float(sum("running" in c.get("state", {}) for c in cs)),
        float(sum(int(c.get("restartCount", 0)) for c in cs)),
        float(requested), float(len(_bound_gpu_ids(pod))),
    ]


def _bound_gpu_ids(pod):
    ids = pod["metadata"].get("annotations", {}).get("amd.com/gpu-ids", "")
    return [int(x) for x in ids.split(",") if x.strip()]


def _outputs_of_wave(ready_pods, logs, use_gpu):
    """What a caller of one wave receives, as arrays: each pod's state at
    Ready, how many distinct GPUs the wave was bound to, and what each pod's
    workload reported (devices it verified its kernel on). Timings are left
    out: they differ from run to run and are in the result line."""
    import numpy as np

    return {
        "pod_state": np.array([_pod_state_row(p) for p in ready_pods],
                              dtype=np.float32),
        # which GPUs a wave gets depends on timing (placement prefers GPUs
        # whose last pod left a while ago); how many distinct ones does not
        "wave_summary": np.array(
            [len(ready_pods),
             len({i for p in ready_pods for i in _bound_gpu_ids(p)})],
            dtype=np.float32),
        "workload_report": np.array(
            [[float(sum(line.startswith("podworker: dev ")
                        and line.endswith(" ok")
                        for line in text.splitlines())),
              float(f"podworker: ready (gpus={1 if use_gpu else -1} ports=0)"
                    in text)]
             for text in logs], dtype=np.float32),
    }


def dump_outputs(outputs, directory):
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    for name, arr in outputs.items():
        np.save(os.path.join(directory, f"{name}.npy"), arr)


def run_bench(n_gpus: int, steps: int, warmup: int, use_gpu: bool,
              hold_pods: bool = True, burst_size: int = 0,
              settle_gap_s: float = 0.0, want_outputs: bool = False):
    from k8s_runpod_kubelet_amd.app import build_stack
    from k8s_runpod_kubelet_amd.config import Config
    from k8s_runpod_kubelet_amd.kube.client import NotFoundError
    from k8s_runpod_kubelet_amd.kube.fake import FakeKube
    from k8s_runpod_kubelet_amd.kube.objects import parse_rfc3339

    state_dir = tempfile.mkdtemp(prefix="amdvk-bench-")
    cfg = Config(
        state_dir=state_dir,
        gpu_count_override=(-1 if use_gpu else max(n_gpus, 8)),
        pending_retry_interval_s=0.2,
        reconcile_interval_s=30.0,
        notify_interval_s=0.0,  # push path only; no polling needed
        pod_controller_workers=max(8, n_gpus),
    )
    kube = FakeKube()
    stack = build_stack(cfg, client=kube)
    if stack.ledger is not None and stack.ledger.total_gpus() < n_gpus:
        raise SystemExit(
            f"bench needs {n_gpus} GPUs; inventory has {stack.ledger.total_gpus()}"
        )
    stack.start(serve_http=False)

    args = ["--hold"] if hold_pods else ["--run-for", "0.05"]
    if use_gpu:
        args = ["--expect-gpus", "1"] + args

    def make_pod(name):
        return {
            "apiVersion": "v1", "kind": "Pod",
            "metadata": {"name": name, "namespace": "default"},
            "spec": {
                "nodeName": cfg.node_name,
                # run-to-completion pods (a user would set this on Job-style
                # pods; the k8s default Always would crash-loop them)
                "restartPolicy": "Never",
                "containers": [{
                    "name": "main",
                    "image": "amdvk/podworker:bench",
                    "command": ["podworker"],
                    "args": args,
                    "resources": {"limits": {"amd.com/gpu": "1"}},
                }],
            },
        }

    def pod_ready(name):
        try:
            pod = kube.get_pod("default", name)
        except NotFoundError:
            return None
        conds = {c["type"]: c["status"]
                 for c in pod.get("status", {}).get("conditions", [])}
        return pod if conds.get("Ready") == "True" else None

    def pod_gone(name):
        try:
            kube.get_pod("default", name)
            return False
        except NotFoundError:
            return True

    captured = {}

    def ready_log(name, timeout_s=5.0):
        # the workload signals readiness just before it flushes stdout
        deadline = time.monotonic() + timeout_s
        while True:
            text = stack.provider.get_container_logs("default", name)
            if "podworker: ready" in text or time.monotonic() > deadline:
                return text
            time.sleep(0.002)

    def wave(tag, timeout_s=120.0, capture=False):
        names = [f"bench-{tag}-{i}" for i in range(n_gpus)]
        created_at = {}
        ready_at = {}
        ready_pods = {}
        for name in names:
            created_at[name] = time.monotonic()
            kube.create_pod("default", make_pod(name))
        deadline = time.monotonic() + timeout_s
        pending = set(names)
        while pending and time.monotonic() < deadline:
            for name in list(pending):
                pod = pod_ready(name)
                if pod is not None:
                    ready_at[name] = time.monotonic()
                    ready_pods[name] = pod
                    pending.remove(name)
            if pending:
                time.sleep(0.002)
        if pending:
            raise SystemExit(f"pods never became Ready: {sorted(pending)}")
        if capture:
            # the pods' logs go away with the pods; reading them is not part
            # of the lifecycle, so its time is taken off the step
            t_cap = time.monotonic()
            captured["pods"] = [ready_pods[n] for n in names]
            captured["logs"] = [ready_log(n) for n in names]
            captured["seconds"] = time.monotonic() - t_cap
        for name in names:
            kube.delete_pod("default", name)
        pending = set(names)
        while pending and time.monotonic() < deadline:
            for name in list(pending):
                if pod_gone(name):
                    pending.remove(name)
            if pending:
                time.sleep(0.002)
        if pending:
            raise SystemExit(f"pods never finalized: {sorted(pending)}")
        return [(ready_at[n] - created_at[n]) for n in names]

    def burst(tag, count, timeout_s=600.0):
        """BASELINE config 5: queue `count` run-to-completion pods at once,
        FIFO-drain across the node's GPUs (placement backpressure)."""
        names = [f"burst-{tag}-{i:03d}" for i in range(count)]
        t0 = time.monotonic()
        for name in names:
            pod = make_pod(name)
            pod["spec"]["containers"][0]["args"] = (
                (["--expect-gpus", "1"] if use_gpu else []) + ["--run-for", "0.05"]
            )
            kube.create_pod("default", pod)
        deadline = time.monotonic() + timeout_s
        pending = set(names)
        while pending and time.monotonic() < deadline:
            for name in list(pending):
                try:
                    pod = kube.get_pod("default", name)
                except NotFoundError:
                    pending.remove(name)
                    continue
                if pod.get("status", {}).get("phase") in ("Succeeded", "Failed"):
                    pending.remove(name)
            if pending:
                time.sleep(0.005)
        if pending:
            raise SystemExit(f"burst never drained: {len(pending)} left")
        drain = time.monotonic() - t0
        for name in names:
            try:
                kube.delete_pod("default", name)
            except NotFoundError:
                pass
        t_gone = time.monotonic() + timeout_s
        while time.monotonic() < t_gone:
            if all(pod_gone(n) for n in names):
                break
            time.sleep(0.005)
        return drain

    try:
        if burst_size > 0:
            for w in range(warmup):
                burst(f"w{w}", max(n_gpus, burst_size // 4))
            t0 = time.monotonic()
            drains = [burst(f"s{k}", burst_size) for k in range(steps)]
            elapsed = time.monotonic() - t0
            total_pods = burst_size * steps
            return {
                "elapsed_s": elapsed,
                "pods": total_pods,
                "pods_per_sec": total_pods / sum(drains),
                "p50_ready_ms": statistics.median(drains) * 1000 / burst_size,
                "p99_ready_ms": max(drains) * 1000 / burst_size,
                "max_ready_ms": max(drains) * 1000,
                "drain_s_per_burst": statistics.median(drains),
            }
        for w in range(warmup):
            wave(f"w{w}")
        latencies = []
        step_s = []
        t0 = time.monotonic()
        for k in range(steps):
            if settle_gap_s > 0:
                # Experiment mode (never set by the driver): let the freed
                # GPU's KFD teardown drain so p50 reflects a non-churn pod
                # (profiles/pw_timing.txt). Throughput output still includes
                # the gaps — only the latency numbers are meaningful here.
                time.sleep(settle_gap_s)
            t_step = time.monotonic()
            latencies.extend(wave(
                f"s{k}", capture=want_outputs and k == steps - 1))
            step_s.append(time.monotonic() - t_step)
        elapsed = time.monotonic() - t0 - captured.get("seconds", 0.0)
        step_s[-1] -= captured.get("seconds", 0.0)
    finally:
        stack.stop()

    lat_ms = sorted(x * 1000 for x in latencies)
    from k8s_runpod_kubelet_amd.server import metrics as m

    return {
        "outputs": (_outputs_of_wave(captured["pods"], captured["logs"],
                                     use_gpu) if want_outputs else None),
        "mean_translate_ms": m.hist_mean_ms(m.translate_seconds),
        "mean_bind_ms": m.hist_mean_ms(m.bind_seconds),
        "mean_launch_ms": m.hist_mean_ms(m.launch_seconds),
        "mean_cgroup_ms": m.hist_mean_ms(m.cgroup_migrate_seconds),
        "elapsed_s": elapsed,
        "step_ms": [s * 1000 for s in step_s],
        "pods": n_gpus * steps,
        "pods_per_sec": (n_gpus * steps) / elapsed,
        "p50_ready_ms": statistics.median(lat_ms),
        "p99_ready_ms": lat_ms[min(len(lat_ms) - 1, int(len(lat_ms) * 0.99))],
        "max_ready_ms": lat_ms[-1],
        # control-plane share of Ready latency: translate+bind+launch
        # (the rest is the workload's own HIP context init)
        "mean_deploy_ms": m.hist_mean_ms(m.deploy_seconds),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=["auto", "gpu", "cpu"], default="auto")
    ap.add_argument("--burst", type=int, default=0,
                    help="BASELINE config 5: pods per burst (0 = wave mode)")
    ap.add_argument("--settle-gap", type=float, default=0.0,
                    help="experiment only: sleep S s between waves so pod-Ready "
                         "reflects a settled GPU (throughput then meaningless)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last wave "
                         "returned (pod states at Ready, GPUs bound, workload "
                         "reports) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements a plain run leaves out; "
                         "there are none yet: the burst and settle-gap "
                         "configurations are separate runs behind their own "
                         "options, so the result is that of a plain run")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.dump_outputs and args.burst:
        ap.error("--dump-outputs applies to wave mode, not --burst")

    rank, world = _dist_env()
    dist = None
    device_sync = False
    use_gpu = False
    if args.mode == "auto":
        try:
            import torch

            use_gpu = torch.cuda.is_available()
        except ImportError:
            use_gpu = False
    else:
        use_gpu = args.mode == "gpu"

    if world > 1:
        import torch
        import torch.distributed as tdist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # Control plane has no collectives; gloo barriers coordinate ranks
        # without claiming HBM that the benchmarked pods need.
        tdist.init_process_group(backend="gloo")
        dist = tdist
        device_sync = use_gpu
        if use_gpu:
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))

    _barrier(dist, device_sync)
    result = None
    if rank == 0:
        result = run_bench(args.gpus, args.steps, args.warmup, use_gpu,
                           burst_size=args.burst,
                           settle_gap_s=args.settle_gap,
                           want_outputs=bool(args.dump_outputs))
    _barrier(dist, device_sync)
    if rank == 0 and args.dump_outputs:
        dump_outputs(result["outputs"], args.dump_outputs)

    if rank == 0 and result is not None:
        # burst mode times whole drains, not waves
        step_ms = result.get("step_ms") or [
            result["elapsed_s"] / args.steps * 1000]
        out = {
            "metric": "gpu_pods_scheduled_per_sec",
            # the exact composite metric BASELINE.json names; `value` carries
            # the throughput half, p50_pod_ready_ms the latency half
            "baseline_metric": "p50 pod-Ready latency + GPU-pods "
                               "scheduled/sec at 1/2/4/8 concurrent",
            "value": round(result["pods_per_sec"], 3),
            "unit": "pods/s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(result["elapsed_s"] / args.steps * 1000, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "n/a",  # control-plane benchmark: no tensor math
            "data": "synthetic",
            "p50_pod_ready_ms": round(result["p50_ready_ms"], 3),
            "p99_pod_ready_ms": round(result["p99_ready_ms"], 3),
            "config": {
                "model": "gpu-pod-lifecycle",
                "global_batch": args.gpus,  # pods per wave
                "seq_len": 0,
                "parallelism": f"1 kubelet x {args.gpus} GPUs, "
                               f"{max(8, args.gpus)} sync workers",
                "workload": ("podworker HIP init+kernel per pod (gfx950)"
                             if use_gpu else "podworker CPU mode"),
                "lifecycle": ("32-pod FIFO burst drain" if args.burst
                              else "create->bind->launch->Ready->delete->finalized"),
                "burst_size": args.burst,
                "settle_gap_s": args.settle_gap,
                "pods_total": result["pods"],
                # spread of the timed steps: one step's time is dominated
                # by the workload's HIP context start, which varies by tens
                # of ms from pod to pod, so a short run's mean is noisy
                "step_ms_min": round(min(step_ms), 3),
                "step_ms_p50": round(statistics.median(step_ms), 3),
                "step_ms_max": round(max(step_ms), 3),
                "mean_deploy_ms": round(result.get("mean_deploy_ms", 0), 3),
                "mean_translate_ms": round(result.get("mean_translate_ms", 0), 3),
                "mean_bind_ms": round(result.get("mean_bind_ms", 0), 3),
                "mean_launch_ms": round(result.get("mean_launch_ms", 0), 3),
                "mean_cgroup_ms": round(result.get("mean_cgroup_ms", 0), 3),
                "p50_pod_ready_ms": round(result["p50_ready_ms"], 3),
                "p99_pod_ready_ms": round(result["p99_ready_ms"], 3),
                "reference_poll_floor_ms": 10000.0,  # kubelet.go:719 10 s tick
            },
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if use_gpu:
        # ROCm static destructors can std::terminate at interpreter exit
        # after a fully successful run (see tests/conftest.py note); the
        # result line is already printed and flushed — exit cleanly before
        # they run, but through the guard, so that atexit hooks registered
        # at process start (instrumentation, coverage) still run; a bare
        # os._exit() skipped them.
        from k8s_runpod_kubelet_amd.utils.exit_guard import install

        install(0)


if __name__ == "__main__":
    main()
