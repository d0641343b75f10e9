"""Provider core: pod lifecycle, reconcile loops, node identity.

Counterpart of the reference's Provider (pkg/virtual_kubelet/kubelet.go,
2066 LoC) re-designed for a local MI355X backend:

- the status sync core (reference updateAllPodStatuses, kubelet.go:816-974)
  still exists as a periodic reconcile, but the *primary* path is push: the
  runtime's pidfd/epoll events call :meth:`_on_runtime_event`, which syncs
  exactly the affected pod within microseconds of the state change —
  replacing one REST round-trip per pod per 10 s tick with O(changes),
- backend health is per-GPU (ledger schedulability) instead of one global
  ``runpodAvailable`` boolean (kubelet.go:320-331),
- node capacity is enumerated dynamically from the GPU inventory and
  /proc/meminfo instead of hardcoded 20 CPU/100 Gi/4 nvidia.com/gpu
  (kubelet.go:1125-1136),
- GPU assignments are written back as the ``amd.com/gpu-ids`` annotation so
  the ledger is reconstructible after restart (reference persists
  ``runpod.io/pod-id`` the same way, kubelet.go:505-562).
"""

from __future__ import annotations

import logging
import os
import threading
import time
from typing import Any, Callable, Dict, List, Optional

from ..config import Config
from ..gpu.binder import PlacementError
from ..gpu.ledger import Ledger
from ..kube.client import K8sClient, is_not_found
from ..kube.objects import (
    annotations as obj_annotations,
    deletion_timestamp,
    full_key,
    meta,
    now_rfc3339,
    parse_rfc3339,
    phase_of,
    pod_key as pod_key_of,
    ts_rfc3339,
)
from ..runtime.base import Runtime
from ..runtime.types import DetailedStatus, PodStatus
from ..server import metrics
from ..utils.backoff import Ticker
from ..version import __version__
from . import annotations as ann
from .instance import InstanceInfo
from .ports import check_ports_exposed
from .registration import Registrar
from .selector import GpuOfferCatalog
from .status import merge_container_status, translate_status
from .translate import ValidationError, prepare_deploy_params

log = logging.getLogger("provider")

NotifyFunc = Callable[[Dict[str, Any]], None]
NodeNotifyFunc = Callable[[Dict[str, Any]], None]


class Provider:
    """PodLifecycleHandler + PodNotifier + NodeProvider
    (reference Provider struct, kubelet.go:27-52)."""

    def __init__(
        self,
        client: K8sClient,
        config: Config,
        runtime: Runtime,
        ledger: Optional[Ledger] = None,
        inventory=None,
    ):
        self.client = client
        self.config = config
        self.runtime = runtime
        self.ledger = ledger
        self.inventory = inventory
        self.node_name = config.node_name
        self.catalog = GpuOfferCatalog(ledger) if ledger is not None else None

        # Tracking maps (reference kubelet.go:33-37: pods, podStatus keyed
        # "ns-name"; deletedPods keyed "ns/name").
        self._pods: Dict[str, Dict[str, Any]] = {}
        self._pod_status: Dict[str, InstanceInfo] = {}
        self._deleted_pods: Dict[str, str] = {}
        self._pods_lock = threading.RLock()
        self._deleted_lock = threading.RLock()
        self._notify_lock = threading.RLock()
        self._notify_fn: Optional[NotifyFunc] = None
        self._node_notify_fn: Optional[NodeNotifyFunc] = None

        self.backend_available = True
        self._tickers: List[Ticker] = []
        self._started = False
        # Optional EventRecorder (set by app.build_stack): lifecycle events
        # the reference gets from the virtual-kubelet library's recorder
        # (main.go:172-177).
        self.recorder = None
        # Optional DiagnosticsManager (set by app.build_stack); drives the
        # start-up and periodic GPU self-tests when configured.
        self.diagnostics = None
        self.meminfo_reader = None  # injectable memory.available source
        self._port_rechecks: Dict[str, int] = {}
        self._eviction = None
        # Set by the PodController: re-enqueue a deleted pod ("ns/name")
        # when its instance turns terminal, completing the API delete.
        self.deletion_resync: Optional[Callable[[str], None]] = None

        self.registrar = Registrar(
            config.registration_endpoint,
            config.node_name,
            config.namespace,
            ledger.total_gpus() if ledger is not None else 0,
            config.heartbeat_interval_s,
        )

    # ------------------------------------------------------------------
    # lifecycle wiring (reference NewProvider, kubelet.go:334-379)
    # ------------------------------------------------------------------

    def start(self) -> None:
        if self._started:
            return
        self._started = True
        # Rebuild runtime state from the instance journal BEFORE any
        # controller can call create_pod, so existing pods adopt instead of
        # redeploying (reference orders this differently — main.go:410 starts
        # controllers before LoadRunning at :426 — and relies on timing).
        adopt = getattr(self.runtime, "adopt_persisted", None)
        if callable(adopt):
            try:
                adopt()
            except Exception:
                log.exception("instance adoption failed")
        if self.diagnostics is not None and self.config.gpu_check_on_start:
            # Before the node controller reports capacity: a GPU that fails
            # here is never counted allocatable. Adopted pods keep their
            # GPUs (occupied GPUs are skipped).
            try:
                self.diagnostics.check_all_idle()
            except Exception:
                log.exception("start-up gpu self-test failed to run")
        self.check_backend_health()
        self.cleanup_stuck_terminating_pods()
        self.registrar.register()  # optional, non-fatal (unlike kubelet.go:369)
        self.runtime.subscribe(self._on_runtime_event)
        # Fallback/periodic loops; the push path does the real-time work.
        self._tickers = [
            Ticker(self.config.reconcile_interval_s, self._periodic_reconcile,
                   "status-reconcile").start(),
            Ticker(self.config.cleanup_interval_s, self._periodic_cleanup,
                   "cleanup").start(),
            Ticker(self.config.pending_retry_interval_s, self.process_pending_pods,
                   "pending-pods").start(),
        ]
        if self.diagnostics is not None and self.config.gpu_check_interval_s > 0:
            # wake often enough to honour the interval, never busier than 1 Hz
            self._tickers.append(
                Ticker(max(1.0, min(60.0, self.config.gpu_check_interval_s / 4)),
                       self.diagnostics.periodic, "gpu-check").start())
        if self.config.eviction_memory_threshold_mb > 0:
            from .eviction import EvictionManager

            self._eviction = EvictionManager(
                self,
                self.config.eviction_memory_threshold_mb * 1024 * 1024,
                meminfo_reader=self.meminfo_reader)
            self._tickers.append(
                Ticker(self.config.eviction_interval_s,
                       self._eviction.check, "eviction").start())

    def stop(self) -> None:
        for t in self._tickers:
            t.stop()
        self.registrar.stop_heartbeat()
        self._started = False

    def _periodic_reconcile(self) -> None:
        """Reference startPeriodicStatusUpdates (kubelet.go:292-303) — with
        ctx-cancellation fixed (the reference's loop leaks on shutdown)."""
        if self.inventory is not None:
            try:
                self.inventory.refresh_dynamic()
                if self.ledger is not None:
                    self.ledger.sync_inventory()
                    metrics.observe_gpus(self.ledger.snapshot())
            except Exception:
                log.exception("inventory refresh failed")
            if self.config.evict_on_gpu_failure:
                try:
                    self._evict_gpu_failure_pods()
                except Exception:
                    log.exception("gpu-failure eviction failed")
        self.update_all_pod_statuses()
        self.check_backend_health()

    def _periodic_cleanup(self) -> None:
        """Reference startPeriodicCleanup (kubelet.go:306-317)."""
        self.cleanup_deleted_pods()
        self.cleanup_stuck_terminating_pods()

    def check_backend_health(self) -> bool:
        """Backend health probe (reference checkRunPodAPIHealth,
        kubelet.go:320-331) — locally: runtime healthy and at least one GPU
        schedulable (or a GPU-less dev node)."""
        healthy = self.runtime.healthy()
        self.backend_available = healthy
        return healthy

    # ------------------------------------------------------------------
    # PodLifecycleHandler
    # ------------------------------------------------------------------

    def create_pod(self, pod: Dict[str, Any]) -> None:
        """CreatePod (reference kubelet.go:384-418): track the pod, then
        deploy; deploy failure leaves the pod Pending for the retry loop."""
        key = pod_key_of(pod)
        from .ports import get_requested_ports

        requested = get_requested_ports(pod)
        info = InstanceInfo(
            status=PodStatus.STARTING,
            requested_ports=requested,
            creation_time=self._creation_ts(pod),
        )
        with self._pods_lock:
            self._pods[key] = pod
            self._pod_status[key] = info
        metrics.pods_created.inc()
        # Adoption path: the pod already names a live instance (kubelet
        # restarted between deploy and now) — do not redeploy.
        existing_id = obj_annotations(pod).get(ann.POD_ID, "")
        if existing_id:
            detailed = self.runtime.get_detailed_status(existing_id)
            if detailed.desired_status != PodStatus.NOT_FOUND:
                with self._pods_lock:
                    info.instance_id = existing_id
                    info.status = detailed.desired_status
                    info.gpu_indices = list(detailed.gpu_indices)
                    info.cost_per_hr = detailed.cost_per_hr
                log.info("adopted existing instance in CreatePod",
                         extra={"pod": key, "instance": existing_id})
                self._sync_pod_status(key)
                return
            self.handle_missing_instance(pod, info)
            return
        try:
            self.deploy_pod(pod)
        except (PlacementError, ValidationError) as exc:
            # Normal backpressure: no GPU free right now — the pod queues and
            # places on the next free event (reference kubelet.go:412-415
            # semantics: CreatePod returns nil, retry loop re-deploys).
            log.info("pod queued: no placement yet",
                     extra={"pod": key, "reason": str(exc)})
            self._emit(pod, "Normal", "PlacementPending", str(exc))
        except Exception as exc:
            log.warning("deploy failed; pod stays pending",
                        extra={"pod": key, "err": str(exc)})
            self._emit(pod, "Warning", "DeployError", str(exc))

    def update_pod(self, pod: Dict[str, Any]) -> None:
        """UpdatePod (reference kubelet.go:421-432): refresh the cached
        copy — and start any newly added spec.ephemeralContainers
        (kubectl debug attaches by updating the pod spec)."""
        key = pod_key_of(pod)
        with self._pods_lock:
            if key in self._pods:
                self._pods[key] = pod
            info = self._pod_status.get(key)
        if info is not None and info.instance_id:
            self._sync_ephemeral_containers(pod, info)

    def _sync_ephemeral_containers(self, pod: Dict[str, Any], info) -> None:
        fn = getattr(self.runtime, "add_ephemeral_container", None)
        eph = pod.get("spec", {}).get("ephemeralContainers", []) or []
        if fn is None or not eph:
            return
        from ..runtime.types import ContainerSpec

        det = self.runtime.get_detailed_status(info.instance_id)
        existing = {c.name for c in det.ephemeral_containers}
        for ec in eph:
            name = ec.get("name", "")
            if not name or name in existing:
                continue
            cspec = ContainerSpec(
                name=name, image=ec.get("image", ""),
                command=list(ec.get("command", []) or []),
                args=list(ec.get("args", []) or []),
                env={e["name"]: str(e.get("value", ""))
                     for e in ec.get("env", []) or [] if e.get("name")},
            )
            try:
                fn(info.instance_id, cspec)
                self._emit(pod, "Normal", "Started",
                           f"ephemeral container {name}")
            except Exception as exc:
                log.warning("ephemeral container start failed",
                            extra={"pod": pod_key_of(pod), "err": str(exc)})
                self._emit(pod, "Warning", "Failed",
                           f"ephemeral container {name}: {exc}")

    def delete_pod(self, pod: Dict[str, Any]) -> None:
        """DeletePod (reference kubelet.go:621-651): record in deletedPods,
        best-effort terminate, drop tracking."""
        key = pod_key_of(pod)
        fkey = full_key(pod)
        instance_id = obj_annotations(pod).get(ann.POD_ID, "")
        with self._pods_lock:
            info = self._pod_status.get(key)
            if not instance_id and info is not None:
                instance_id = info.instance_id
        if instance_id:
            with self._deleted_lock:
                self._deleted_pods[fkey] = instance_id
            try:
                self.runtime.terminate(instance_id)
            except Exception:
                log.exception("terminate failed", extra={"instance": instance_id})
        with self._pods_lock:
            self._pods.pop(key, None)
            self._pod_status.pop(key, None)
        metrics.pods_deleted.inc()

    def _memory_pressure(self) -> bool:
        """node.status MemoryPressure condition: the eviction signal is
        below threshold right now (kubelet sets the condition from the
        same memory.available signal that drives eviction)."""
        if self.config.eviction_memory_threshold_mb <= 0:
            return False
        from .eviction import read_available_memory_bytes

        reader = self.meminfo_reader or read_available_memory_bytes
        avail = reader()
        return 0 <= avail < (
            self.config.eviction_memory_threshold_mb * 1024 * 1024)

    def eviction_candidates(self):
        """(pod_key, pod_obj, memory_usage_bytes) for every live local pod
        (eviction.py ranks them). Pending pods are skipped — they hold no
        node memory yet."""
        stats_fn = getattr(self.runtime, "get_stats", None)
        with self._pods_lock:
            items = [(k, dict(p), self._pod_status.get(k))
                     for k, p in self._pods.items()]
        out = []
        for key, pod, info in items:
            if info is None or not info.instance_id:
                continue
            if phase_of(pod) in ("Succeeded", "Failed"):
                continue
            usage = 0
            if callable(stats_fn):
                try:
                    usage = int(stats_fn(info.instance_id).get(
                        "memoryUsageBytes", 0) or 0)
                except Exception:
                    usage = 0
            out.append((key, pod, usage))
        return out

    def evict_pod(self, key: str, message: str,
                  reason: str = "Evicted") -> None:
        """Node-pressure eviction of one pod: kill its instance now (hard
        eviction has no grace) and mark the API object Failed/Evicted —
        the object is NOT deleted (kubectl keeps showing Evicted pods,
        k8s semantics). GPU-failure eviction reuses this with
        reason=GPUFailure."""
        with self._pods_lock:
            pod = self._pods.get(key)
            info = self._pod_status.get(key)
        if pod is None or info is None or not info.instance_id:
            return
        self._emit(pod, "Warning", reason, message)
        try:
            # hard eviction: no grace (kubelet memory hard-eviction
            # semantics) — TERM immediately, KILL right behind it
            self.runtime.terminate(info.instance_id, grace_override_s=0.0)
        except Exception:
            log.exception("eviction terminate failed",
                          extra={"instance": info.instance_id})
        info.status = PodStatus.TERMINATED
        status = {
            "phase": "Failed",
            "reason": reason,
            "message": message,
            "startTime": ts_rfc3339(info.creation_time),
        }
        self._push_status(pod, status)
        metrics.pods_evicted.inc()

    def _evict_gpu_failure_pods(self) -> None:
        """Pods bound to a GPU that lost health (RAS uncorrectable seen by
        the per-tick re-probe) fail fast with reason GPUFailure, so a Job/
        Deployment controller reschedules the work — leaving them running
        against a dead device would wedge them silently. The GPU stays
        cordoned by the ledger until an operator intervenes."""
        if self.inventory is None:
            return
        bad = {g.index for g in self.inventory.gpus if not g.healthy}
        if not bad:
            return
        with self._pods_lock:
            items = [(k, dict(p), self._pod_status.get(k))
                     for k, p in self._pods.items()]
        for key, pod, info in items:
            if info is None or not info.instance_id:
                continue
            if phase_of(pod) in ("Succeeded", "Failed"):
                continue
            hit = sorted(bad.intersection(info.gpu_indices))
            if hit:
                self.evict_pod(
                    key,
                    f"GPU {hit} became unhealthy (RAS uncorrectable "
                    f"errors); pod failed so it can be rescheduled",
                    reason="GPUFailure")

    def deletion_finalized(self, namespace: str, name: str) -> bool:
        """True once the pod's instance is actually dead (terminal or
        unknown) — the gate the PodController uses before removing the API
        object. Real k8s keeps a pod Terminating until its containers are
        gone; deleting the object while a TERM-ignoring container waits out
        its grace period would lie to kubectl (found by the image-pod
        churn soak: pid-1-in-namespace entrypoints ignore SIGTERM)."""
        with self._deleted_lock:
            instance_id = self._deleted_pods.get(f"{namespace}/{name}")
        if not instance_id:
            return True
        try:
            status = self.runtime.get_status(instance_id)
        except Exception:
            return True
        return status in (PodStatus.EXITED, PodStatus.TERMINATED,
                          PodStatus.NOT_FOUND)

    def get_pod(self, namespace: str, name: str) -> Optional[Dict[str, Any]]:
        """GetPod (reference kubelet.go:654-667)."""
        with self._pods_lock:
            return self._pods.get(f"{namespace}-{name}")

    def get_pods(self) -> List[Dict[str, Any]]:
        """GetPods (reference kubelet.go:699-710)."""
        with self._pods_lock:
            return list(self._pods.values())

    def get_running_pods(self) -> List[Dict[str, Any]]:
        """Pods whose instance is live right now (the kubelet's
        /runningpods debug endpoint reports runtime truth, not the
        apiserver's possibly-stale phase)."""
        with self._pods_lock:
            items = [(dict(p), self._pod_status.get(k))
                     for k, p in self._pods.items()]
        return [p for p, info in items
                if info is not None and info.instance_id
                and info.status == PodStatus.RUNNING]

    def get_pod_status(self, namespace: str, name: str) -> Optional[Dict[str, Any]]:
        """GetPodStatus (reference kubelet.go:670-696): live port re-check for
        RUNNING pods with requested ports."""
        key = f"{namespace}-{name}"
        with self._pods_lock:
            pod = self._pods.get(key)
            info = self._pod_status.get(key)
        if pod is None or info is None:
            return None
        detailed = None
        if info.instance_id:
            detailed = self.runtime.get_detailed_status(info.instance_id)
            if info.status == PodStatus.RUNNING:
                # Same readiness rule as the sync path: ports exposed AND
                # every container ready (pipe signal or readinessProbe).
                ports_ok = check_ports_exposed(
                    info.requested_ports, detailed.port_mappings
                )
                containers_ready = bool(detailed.containers) and all(
                    c.ready for c in detailed.containers
                )
                info.ports_exposed = ports_ok and containers_ready
        return translate_status(pod, info, detailed, self.config.internal_ip)

    def notify_pods(self, fn: NotifyFunc) -> None:
        """NotifyPods (reference kubelet.go:713-731). The reference spawns a
        10 s poll loop here; our fast path is the runtime event subscription,
        so this only stores the callback — the notify_interval ticker exists
        as a safety net."""
        with self._notify_lock:
            self._notify_fn = fn
        if self.config.notify_interval_s > 0 and self._started:
            self._tickers.append(
                Ticker(self.config.notify_interval_s, self.update_all_pod_statuses,
                       "notify-reconcile").start()
            )

    # ------------------------------------------------------------------
    # deploy pipeline (reference DeployPodToRunPod, kubelet.go:435-502)
    # ------------------------------------------------------------------

    def deploy_pod(self, pod: Dict[str, Any]) -> None:
        key = pod_key_of(pod)
        # Claim the deploy: the pending-retry ticker and the controller can
        # race here (the reference's single worker serializes this at the cost
        # of throughput; with N workers the claim flag does it instead).
        with self._pods_lock:
            claim = self._pod_status.get(key)
            if claim is not None:
                if claim.instance_id or claim.deploying:
                    return
                claim.deploying = True
        try:
            self._deploy_pod_locked(pod)
        finally:
            with self._pods_lock:
                claim = self._pod_status.get(key)
                if claim is not None:
                    claim.deploying = False

    def _deploy_pod_locked(self, pod: Dict[str, Any]) -> None:
        key = pod_key_of(pod)
        # Inject node-level datacenter annotation if missing
        # (kubelet.go:437-455).
        if self.config.datacenter_ids and ann.DATACENTER_IDS not in obj_annotations(pod):
            try:
                fresh = self.client.get_pod(meta(pod)["namespace"], meta(pod)["name"])
                obj_annotations(fresh)[ann.DATACENTER_IDS] = ",".join(
                    self.config.datacenter_ids
                )
                pod = self.client.update_pod(meta(fresh)["namespace"], fresh)
                with self._pods_lock:
                    self._pods[key] = pod
            except Exception:
                log.exception("datacenter annotation injection failed")

        if not self.backend_available and not self.check_backend_health():
            raise RuntimeError("backend unavailable (no schedulable GPUs)")

        t0 = time.monotonic()
        params = prepare_deploy_params(pod, self.client, self.config, self.catalog)
        metrics.translate_seconds.observe(time.monotonic() - t0)
        env_count = len(params.env)
        log.info(
            "deploying pod",
            extra={  # env values redacted to count (kubelet.go:473-488)
                "pod": key, "gpus": params.gpu_count,
                "gpu_mem_gb": params.gpu_memory_bytes >> 30,
                "env_vars": env_count, "ports": params.requested_ports,
                "cloud_type": params.cloud_type,
            },
        )
        detailed = self.runtime.deploy(params)
        metrics.deploy_seconds.observe(time.monotonic() - t0)
        # kubelet-style container lifecycle events: Pulled for image-backed
        # containers (the store resolved it locally), then Started with the
        # placement info (kubectl describe surface).
        images_by_name = {c.name: c.image for c in params.containers}
        for c in detailed.containers:
            if c.image_id and c.pull_seconds > 0:
                self._emit(pod, "Normal", "Pulled",
                           f'Successfully pulled image '
                           f'"{images_by_name.get(c.name, "")}" in '
                           f"{c.pull_seconds:.3f}s ({c.image_id})")
            elif c.image_id:
                self._emit(pod, "Normal", "Pulled",
                           f'Container image "{images_by_name.get(c.name, "")}"'
                           f" already present on machine ({c.image_id})")
        self._emit(pod, "Normal", "Started",
                   f"instance {detailed.id} on GPUs {detailed.gpu_indices}"
                   if detailed.gpu_indices else f"instance {detailed.id}")

        with self._pods_lock:
            info = self._pod_status.get(key)
            if info is not None:
                info.instance_id = detailed.id
                info.status = detailed.desired_status
                info.gpu_indices = list(detailed.gpu_indices)
                info.cost_per_hr = detailed.cost_per_hr
        self._update_pod_with_instance_info(pod, detailed)
        # Immediate first sync so a fast-starting pod goes Ready without
        # waiting for any tick.
        self._sync_pod_status(key)

    def _update_pod_with_instance_info(self, pod: Dict[str, Any],
                                       detailed: DetailedStatus) -> None:
        """Annotation write-back (reference updatePodWithRunPodInfo,
        kubelet.go:505-562) via PATCH instead of Get+Update — one round-trip,
        no resourceVersion conflicts."""
        namespace, name = meta(pod)["namespace"], meta(pod)["name"]
        patch = {
            "metadata": {
                "annotations": {
                    ann.POD_ID: detailed.id,
                    ann.COST_PER_HR: f"{detailed.cost_per_hr:.3f}",
                    ann.GPU_IDS: ",".join(str(i) for i in detailed.gpu_indices),
                }
            }
        }
        try:
            updated = self.client.patch_pod(namespace, name, patch)
            with self._pods_lock:
                self._pods[pod_key_of(updated)] = updated
        except Exception as exc:
            if is_not_found(exc):
                return
            log.exception("annotation write-back failed")

    # ------------------------------------------------------------------
    # status sync (reference updateAllPodStatuses, kubelet.go:816-974)
    # ------------------------------------------------------------------

    def _on_runtime_event(self, instance_id: str) -> None:
        """Push path: the runtime just told us this instance changed."""
        key = None
        with self._pods_lock:
            for k, info in self._pod_status.items():
                if info.instance_id == instance_id:
                    key = k
                    break
        if key is not None:
            try:
                self._sync_pod_status(key)
            except Exception:
                log.exception("event-driven sync failed", extra={"pod": key})
        # A terminal instance freed its GPUs: place pending pods NOW instead
        # of on the next retry tick (this is what keeps back-to-back waves —
        # BASELINE config 5's FIFO burst — GPU-bound rather than tick-bound).
        try:
            status = self.runtime.get_status(instance_id)
        except Exception:
            status = PodStatus.NOT_FOUND
        if status in (PodStatus.EXITED, PodStatus.TERMINATED, PodStatus.NOT_FOUND):
            self._nudge_pending()
            # Deletion finalize: a deleted pod's API object is held until
            # its instance is dead (deletion_finalized); this event is what
            # re-enqueues it so the PodController can complete the delete.
            if self.deletion_resync is not None:
                with self._deleted_lock:
                    fkey = next((k for k, iid in self._deleted_pods.items()
                                 if iid == instance_id), None)
                if fkey is not None:
                    try:
                        self.deletion_resync(fkey)
                    except Exception:
                        log.exception("deletion resync failed")

    def _emit(self, pod: Dict[str, Any], etype: str, reason: str,
              message: str) -> None:
        if self.recorder is not None:
            try:
                self.recorder.event(pod, etype, reason, message)
            except Exception:
                log.debug("event emit failed", extra={"reason": reason})

    def _nudge_pending(self) -> None:
        with self._pods_lock:
            has_pending = any(
                not info.instance_id and not info.deploying
                for info in self._pod_status.values()
            )
        if has_pending:
            try:
                self.process_pending_pods()
            except Exception:
                log.exception("event-driven pending processing failed")

    def update_all_pod_statuses(self) -> None:
        with self._pods_lock:
            keys = list(self._pods.keys())
        for key in keys:
            try:
                self._sync_pod_status(key)
            except Exception:
                log.exception("status sync failed", extra={"pod": key})

    def _schedule_port_recheck(self, key: str, delay_s: float = 0.25,
                               max_rechecks: int = 40) -> None:
        with self._pods_lock:
            n = self._port_rechecks.get(key, 0)
            if n >= max_rechecks:
                return
            self._port_rechecks[key] = n + 1
        t = threading.Timer(delay_s, self._sync_pod_status, args=(key,))
        t.daemon = True
        t.start()

    def _sync_pod_status(self, key: str) -> None:
        with self._pods_lock:
            pod = self._pods.get(key)
            info = self._pod_status.get(key)
        if pod is None or info is None:
            return
        if phase_of(pod) in ("Succeeded", "Failed"):  # kubelet.go:836
            return
        if not info.instance_id:  # not deployed yet (pending retry loop owns it)
            return

        detailed = self.runtime.get_detailed_status(info.instance_id)
        if detailed.desired_status == PodStatus.NOT_FOUND:
            self.handle_missing_instance(pod, info)  # kubelet.go:861-864
            return

        ports_exposed = check_ports_exposed(info.requested_ports, detailed.port_mappings)
        if ports_exposed:
            with self._pods_lock:
                self._port_rechecks.pop(key, None)
        if (not ports_exposed and info.requested_ports
                and detailed.desired_status == PodStatus.RUNNING):
            # Port-gated pod whose listen socket is not visible yet: the
            # push event fires once (at container-ready), and /proc/net
            # scans can transiently miss entries — re-check shortly
            # instead of waiting for the 30 s reconcile tick.
            self._schedule_port_recheck(key)
        # Readiness also requires container readiness (our event signal).
        containers_ready = bool(detailed.containers) and all(
            c.ready for c in detailed.containers
        )
        if detailed.desired_status == PodStatus.RUNNING and not containers_ready:
            ports_exposed = False

        # restartPolicy transitions (crash → backoff → restarted) keep the
        # pod RUNNING; the signature makes them visible to change detection
        # so CrashLoopBackOff/restartCount reach the apiserver.
        restart_sig = (
            sum(c.restart_count for c in detailed.containers) * 2
            + sum(1 for c in detailed.containers if c.backoff_until),
            # ephemeral (kubectl debug) containers appear/terminate without
            # touching pod phase — their transitions must still patch status
            len(detailed.ephemeral_containers),
            sum(1 for c in detailed.ephemeral_containers
                if c.exit_code is not None),
        )
        changed = (
            detailed.desired_status != info.status
            or ports_exposed != info.ports_exposed
            or restart_sig != info.restart_sig
        )
        if not changed:
            return

        if restart_sig != info.restart_sig:
            # a container just entered crash backoff: kubectl-visible
            # BackOff event, like a real kubelet's
            for c in detailed.containers:
                if c.backoff_until:
                    self._emit(pod, "Warning", "BackOff",
                               f"Back-off restarting failed container "
                               f"{c.name} (exit {c.exit_code}, "
                               f"restarts {c.restart_count})")
        info.status = detailed.desired_status
        info.ports_exposed = ports_exposed
        info.restart_sig = restart_sig
        if info.status == PodStatus.RUNNING and ports_exposed and info.ready_time is None:
            info.ready_time = time.time()
            metrics.pod_ready_seconds.observe(info.ready_time - info.creation_time)

        if info.status == PodStatus.EXITED:
            self.handle_pod_completion(pod, info, detailed)  # kubelet.go:909-911
            return

        new_status = translate_status(pod, info, detailed, self.config.internal_ip)
        old = pod.get("status", {})
        new_status["containerStatuses"] = merge_container_status(
            new_status.get("containerStatuses", []), old.get("containerStatuses", [])
        )
        self._push_status(pod, new_status)

    def _push_status(self, pod: Dict[str, Any], status: Dict[str, Any]) -> None:
        """PATCH pods/status, fall back to the notify callback
        (reference kubelet.go:915-970 incl. the recover-guarded notify)."""
        namespace, name = meta(pod)["namespace"], meta(pod)["name"]
        pod = dict(pod)
        pod["status"] = status
        with self._pods_lock:
            self._pods[pod_key_of(pod)] = pod
        try:
            updated = self.client.patch_pod_status(namespace, name, {"status": status})
            with self._pods_lock:
                self._pods[pod_key_of(updated)] = updated
        except Exception as exc:
            if is_not_found(exc):
                return
            log.warning("status PATCH failed; using notify fallback",
                        extra={"pod": f"{namespace}/{name}", "err": str(exc)})
            with self._notify_lock:
                fn = self._notify_fn
            if fn is not None:
                try:
                    fn(pod)
                except Exception:
                    log.exception("notify callback panicked")  # kubelet.go:938-954

    def handle_pod_completion(self, pod: Dict[str, Any], info: InstanceInfo,
                              detailed: DetailedStatus) -> None:
        """Reference handlePodCompletion (kubelet.go:998-1065)."""
        status = translate_status(pod, info, detailed, self.config.internal_ip)
        self._push_status(pod, status)
        if status.get("phase") == "Failed":
            self._emit(pod, "Warning", "Failed",
                       detailed.completion_message or "workload failed")
        log.info(
            "pod completed",
            extra={
                "pod": full_key(pod),
                "phase": status.get("phase"),
                "exit_code": detailed.exit_code,
            },
        )

    def handle_missing_instance(self, pod: Dict[str, Any], info: InstanceInfo) -> None:
        """Reference handleMissingRunPodInstance (kubelet.go:1708-1773): strip
        backend annotations, mark Failed/PodDeleted so the pod is not
        redeployed."""
        namespace, name = meta(pod)["namespace"], meta(pod)["name"]
        info.status = PodStatus.NOT_FOUND
        info.last_error = "instance not found"
        try:
            self.client.patch_pod(namespace, name, {
                "metadata": {"annotations": {ann.POD_ID: None, ann.COST_PER_HR: None,
                                             ann.GPU_IDS: None}}
            })
        except Exception as exc:
            if not is_not_found(exc):
                log.exception("annotation strip failed")
        status = translate_status(pod, info, None, self.config.internal_ip)
        self._push_status(pod, status)

    # ------------------------------------------------------------------
    # pending retry loop (reference startPendingPodProcessor,
    # kubelet.go:734-814)
    # ------------------------------------------------------------------

    def process_pending_pods(self) -> None:
        now = time.time()
        with self._pods_lock:
            items = [
                (key, pod, self._pod_status.get(key))
                for key, pod in self._pods.items()
            ]
        # Placement order: spec.priority descending (scheduler-resolved
        # priorityClass), FIFO within a class — the reference retries in map
        # order (kubelet.go:760), which starves nothing but also respects
        # nothing.
        items.sort(key=lambda t: (
            -int(t[1].get("spec", {}).get("priority", 0) or 0),
            t[2].creation_time if t[2] is not None else now,
        ))
        for key, pod, info in items:
            if info is None or info.instance_id:
                continue
            if phase_of(pod) in ("Succeeded", "Failed"):
                continue
            age = now - info.creation_time
            if age > self.config.pending_pod_timeout_s:
                # 15 min cutoff → PodFailed/RunPodDeploymentFailed
                # (kubelet.go:788-806) — the timeout is configurable here.
                log.warning("pending pod timed out", extra={"pod": key, "age_s": int(age)})
                self._emit(pod, "Warning", "FailedDeployment",
                           f"not placed within {int(age)}s")
                info.status = PodStatus.EXITED
                status = {
                    "phase": "Failed",
                    "reason": "DeploymentFailed",
                    "message": f"could not place pod within "
                               f"{int(self.config.pending_pod_timeout_s)}s",
                    "startTime": ts_rfc3339(info.creation_time),
                }
                self._push_status(pod, status)
                continue
            try:
                self.deploy_pod(pod)
                log.info("pending pod deployed on retry", extra={"pod": key})
            except (PlacementError, ValidationError) as exc:
                log.debug("pending pod still unplaceable",
                          extra={"pod": key, "err": str(exc)})
            except Exception:
                log.exception("pending retry failed", extra={"pod": key})

    # ------------------------------------------------------------------
    # GC ladders (reference kubelet.go:1190-1377)
    # ------------------------------------------------------------------

    def cleanup_deleted_pods(self) -> None:
        """Reference cleanupDeletedPods (kubelet.go:1190-1227): when the K8s
        pod is really gone, make sure the backend instance is too — plus an
        orphan sweep for terminal instance records whose pod no longer
        exists anywhere (accumulates otherwise after kubelet restarts: the
        in-memory deletedPods map dies with the old process)."""
        try:
            terminal = self.runtime.list_instances(
                [PodStatus.EXITED, PodStatus.TERMINATED])
        except Exception:
            terminal = []
        with self._pods_lock:
            referenced = {info.instance_id
                          for info in self._pod_status.values()}
        for st in terminal:
            if st.id in referenced or not st.name:
                continue
            try:
                self.client.get_pod(st.namespace or "default", st.name)
                continue  # pod still exists; normal paths own this record
            except Exception as exc:
                if not is_not_found(exc):
                    continue
            try:
                self.runtime.remove(st.id)
                log.info("removed orphan terminal instance",
                         extra={"instance": st.id,
                                "pod": f"{st.namespace}/{st.name}"})
            except Exception:
                log.exception("orphan instance removal failed",
                              extra={"instance": st.id})
        with self._deleted_lock:
            items = list(self._deleted_pods.items())
        for fkey, instance_id in items:
            namespace, name = fkey.split("/", 1)
            try:
                self.client.get_pod(namespace, name)
                continue  # pod still exists in K8s — keep the entry
            except Exception as exc:
                if not is_not_found(exc):
                    continue
            try:
                status = self.runtime.get_status(instance_id)
                if status not in (PodStatus.NOT_FOUND, PodStatus.TERMINATED):
                    self.runtime.terminate(instance_id)
                else:
                    self.runtime.remove(instance_id)
            except Exception:
                log.exception("backend cleanup failed", extra={"instance": instance_id})
                continue
            with self._deleted_lock:
                self._deleted_pods.pop(fkey, None)

    def cleanup_stuck_terminating_pods(self) -> None:
        """Reference cleanupStuckTerminatingPods escalation ladder
        (kubelet.go:1231-1377): thresholds are configurable
        (stuck_reterminate_after_s / stuck_statuserr_force_after_s /
        stuck_force_after_s ≙ 5/10/15 min)."""
        try:
            pods = self.client.list_pods(
                field_selector=f"spec.nodeName={self.node_name}"
            )
        except Exception:
            log.exception("list pods for stuck-terminating GC failed")
            return
        now = time.time()
        for pod in pods:
            ts = deletion_timestamp(pod)
            if not ts:
                continue
            age = now - parse_rfc3339(ts)
            namespace, name = meta(pod)["namespace"], meta(pod)["name"]
            instance_id = obj_annotations(pod).get(ann.POD_ID, "")
            if not instance_id:
                self.force_delete_pod(namespace, name)  # kubelet.go:1268-1278
                continue
            try:
                status = self.runtime.get_status(instance_id)
            except Exception:
                if age > self.config.stuck_statuserr_force_after_s:
                    self.force_delete_pod(namespace, name)  # kubelet.go:1285
                continue
            if status in (PodStatus.NOT_FOUND, PodStatus.EXITED, PodStatus.TERMINATED):
                self.force_delete_pod(namespace, name)  # kubelet.go:1300-1330
            elif age > self.config.stuck_force_after_s:
                self.force_delete_pod(namespace, name)  # kubelet.go:1350
            elif age > self.config.stuck_reterminate_after_s:
                try:
                    self.runtime.terminate(instance_id)  # kubelet.go:1333
                except Exception:
                    log.exception("re-terminate failed")

    def force_delete_pod(self, namespace: str, name: str) -> None:
        """Reference ForceDeletePod (kubelet.go:1776-1796)."""
        try:
            self.client.delete_pod(namespace, name, grace_period_s=0)
        except Exception as exc:
            if not is_not_found(exc):
                log.exception("force delete failed", extra={"pod": f"{namespace}/{name}"})

    # ------------------------------------------------------------------
    # startup reconciliation (reference LoadRunning, kubelet.go:1380-1535)
    # ------------------------------------------------------------------

    def load_running(self) -> None:
        adopt = getattr(self.runtime, "adopt_persisted", None)
        if callable(adopt):
            adopt()
        try:
            k8s_pods = self.client.list_pods(
                field_selector=f"spec.nodeName={self.node_name}"
            )
        except Exception:
            log.exception("LoadRunning: list pods failed")
            k8s_pods = []

        instances = {
            s.id: s
            for s in self.runtime.list_instances(
                [PodStatus.RUNNING, PodStatus.EXITED, PodStatus.STARTING]
            )
        }
        matched = set()
        for pod in k8s_pods:
            if phase_of(pod) in ("Succeeded", "Failed") or deletion_timestamp(pod):
                continue
            key = pod_key_of(pod)
            with self._pods_lock:
                if key in self._pods:
                    continue
            instance_id = obj_annotations(pod).get(ann.POD_ID, "")
            from .ports import get_requested_ports

            info = InstanceInfo(
                requested_ports=get_requested_ports(pod),
                creation_time=self._creation_ts(pod),
            )
            if instance_id and instance_id in instances:
                detailed = instances[instance_id]
                info.instance_id = instance_id
                info.status = detailed.desired_status
                info.gpu_indices = list(detailed.gpu_indices)
                matched.add(instance_id)
                gpu_ids = obj_annotations(pod).get(ann.GPU_IDS, "")
                if gpu_ids and self.ledger is not None:
                    indices = [int(x) for x in gpu_ids.split(",") if x.strip()]
                    # gpu memory per gpu unknown here; ledger was already
                    # rebuilt by runtime adoption when possible.
                    self.ledger.adopt(key, indices, 0)
                with self._pods_lock:
                    self._pods[key] = pod
                    self._pod_status[key] = info
                self._sync_pod_status(key)
                log.info("adopted running pod", extra={"pod": key, "instance": instance_id})
            elif instance_id:
                with self._pods_lock:
                    self._pods[key] = pod
                    self._pod_status[key] = info
                self.handle_missing_instance(pod, info)  # kubelet.go:1486
            else:
                info.status = PodStatus.STARTING
                with self._pods_lock:
                    self._pods[key] = pod
                    self._pod_status[key] = info  # retry loop deploys later
                log.info("adopted pending pod", extra={"pod": key})

        # Backend instances with no K8s pod → import as virtual pods
        # (reference kubelet.go:1513-1524 → CreateVirtualPod :1564-1634).
        for instance_id, detailed in instances.items():
            if instance_id in matched:
                continue
            if detailed.desired_status == PodStatus.RUNNING:
                self.create_virtual_pod(detailed)

    def create_virtual_pod(self, detailed: DetailedStatus) -> None:
        """Reference CreateVirtualPod (kubelet.go:1564-1634) — imports an
        orphan backend instance as pod ``runpod-<id>`` in ``default``; the
        nodeName is *this* node (the reference hardcodes a mismatched
        "runpod-virtual-node", a quirk not replicated)."""
        name = f"runpod-{detailed.id}"
        pod = {
            "apiVersion": "v1",
            "kind": "Pod",
            "metadata": {
                "name": name,
                "namespace": "default",
                "annotations": {
                    ann.POD_ID: detailed.id,
                    ann.EXTERNAL: "true",
                    ann.GPU_IDS: ",".join(str(i) for i in detailed.gpu_indices),
                },
                "labels": {"app": "runpod-external"},
            },
            "spec": {
                "nodeName": self.node_name,
                "containers": [{
                    "name": "external-workload",
                    "image": "amdvk/external:latest",
                    "command": ["sleep", "infinity"],
                }],
                "tolerations": [{
                    "key": ann.TAINT_KEY, "operator": "Equal",
                    "value": ann.TAINT_VALUE, "effect": "NoSchedule",
                }],
            },
            "status": {
                "phase": "Running",
                "conditions": [{"type": "Ready", "status": "True",
                                "lastTransitionTime": now_rfc3339()}],
            },
        }
        try:
            created = self.client.create_pod("default", pod)
        except Exception:
            log.exception("virtual pod import failed", extra={"instance": detailed.id})
            return
        key = pod_key_of(created)
        info = InstanceInfo(
            instance_id=detailed.id,
            status=detailed.desired_status,
            gpu_indices=list(detailed.gpu_indices),
            creation_time=detailed.created_at or time.time(),
        )
        with self._pods_lock:
            self._pods[key] = created
            self._pod_status[key] = info
        log.info("imported orphan instance as virtual pod",
                 extra={"pod": key, "instance": detailed.id})

    @staticmethod
    def _creation_ts(pod: Dict[str, Any]) -> float:
        ts = meta(pod).get("creationTimestamp")
        if ts:
            try:
                return parse_rfc3339(ts)
            except ValueError:
                pass
        return time.time()

    # ------------------------------------------------------------------
    # NodeProvider (reference kubelet.go:1070-1186)
    # ------------------------------------------------------------------

    def ping(self) -> None:
        """Ping (reference kubelet.go:1070-1076): raises when the backend is
        unavailable so the node goes NotReady."""
        if not self.check_backend_health():
            raise RuntimeError("backend unhealthy: no schedulable GPUs")

    def notify_node_status(self, fn: NodeNotifyFunc) -> None:
        """NotifyNodeStatus (reference kubelet.go:1079-1095). The node
        controller's ticker drives pushes; this stores the callback."""
        with self._notify_lock:
            self._node_notify_fn = fn

    def get_node_status(self) -> Dict[str, Any]:
        """Node object builder (reference GetNodeStatus, kubelet.go:1098-1186)
        with dynamic capacity: real CPU/memory from the host, ``amd.com/gpu``
        from the ledger (the reference hardcodes 20 CPU/100 Gi/4
        nvidia.com/gpu — kubelet.go:1125-1136)."""
        gpu_total = self.ledger.total_gpus() if self.ledger is not None else 0
        gpu_sched = self.ledger.schedulable_count() if self.ledger is not None else 0
        cpu = os.cpu_count() or 1
        mem_kb = 0
        try:
            with open("/proc/meminfo", "r", encoding="ascii") as fh:
                for line in fh:
                    if line.startswith("MemTotal:"):
                        mem_kb = int(line.split()[1])
                        break
        except OSError:
            mem_kb = 16 * 1024 * 1024

        ready = self.backend_available
        conditions = [
            {"type": "Ready", "status": "True" if ready else "False",
             "reason": "KubeletReady" if ready else "BackendUnavailable",
             "message": f"{gpu_sched}/{gpu_total} GPUs schedulable",
             "lastHeartbeatTime": now_rfc3339(),
             "lastTransitionTime": now_rfc3339()},
            {"type": "OutOfDisk", "status": "False", "reason": "KubeletHasSufficientDisk",
             "lastHeartbeatTime": now_rfc3339(), "lastTransitionTime": now_rfc3339()},
            {"type": "MemoryPressure",
             "status": "True" if self._memory_pressure() else "False",
             "reason": ("KubeletHasInsufficientMemory"
                        if self._memory_pressure()
                        else "KubeletHasSufficientMemory"),
             "lastHeartbeatTime": now_rfc3339(), "lastTransitionTime": now_rfc3339()},
            {"type": "DiskPressure", "status": "False", "reason": "KubeletHasNoDiskPressure",
             "lastHeartbeatTime": now_rfc3339(), "lastTransitionTime": now_rfc3339()},
            {"type": "PIDPressure", "status": "False", "reason": "KubeletHasSufficientPID",
             "lastHeartbeatTime": now_rfc3339(), "lastTransitionTime": now_rfc3339()},
        ]
        capacity = {
            "cpu": str(cpu),
            "memory": f"{mem_kb}Ki",
            "pods": "110",
            ann.GPU_RESOURCE: str(gpu_total),
        }
        allocatable = dict(capacity)
        allocatable[ann.GPU_RESOURCE] = str(gpu_sched)
        hbm_annotations = {}
        if self.ledger is not None:
            for state in self.ledger.snapshot():
                hbm_annotations[f"amd.com/gpu-{state.gpu.index}-hbm-free-bytes"] = str(
                    state.headroom_bytes
                )
        return {
            "apiVersion": "v1",
            "kind": "Node",
            "metadata": {
                "name": self.node_name,
                "labels": {
                    # reference labels (kubelet.go:1105-1110)
                    "type": "virtual-kubelet",
                    "kubernetes.io/role": "agent",
                    "kubernetes.io/os": self.config.operating_system.lower(),
                    "kubernetes.io/hostname": self.node_name,
                    "node.kubernetes.io/instance-type": "amd-mi355x",
                    "amd.com/gpu.family": "CDNA4",
                },
                "annotations": hbm_annotations,
            },
            "spec": {
                # taint kept reference-compatible (kubelet.go:1111-1117)
                "taints": [{
                    "key": ann.TAINT_KEY,
                    "value": ann.TAINT_VALUE,
                    "effect": "NoSchedule",
                }],
            },
            "status": {
                "nodeInfo": {
                    "operatingSystem": self.config.operating_system.lower(),
                    "architecture": "amd64",
                    "kubeletVersion": f"v1.29.0-amdvk-{__version__}",
                },
                "capacity": capacity,
                "allocatable": allocatable,
                "conditions": conditions,
                "addresses": [{"type": "InternalIP", "address": self.config.internal_ip}],
                "daemonEndpoints": {"kubeletEndpoint": {"Port": self.config.listen_port}},
                # node.status.images from the local OCI store (kubectl
                # describe node surface; a real kubelet lists its cache)
                "images": self._node_images(),
            },
        }

    def _node_images(self) -> List[Dict[str, Any]]:
        store = getattr(self.runtime, "image_store", None)
        if store is None:
            return []
        try:
            return [{"names": [ref], "sizeBytes": size}
                    for ref, size in store.image_sizes()]
        except Exception:
            return []

    # ------------------------------------------------------------------
    # logs / exec (reference stubs kubelet.go:2027-2066 — real here)
    # ------------------------------------------------------------------

    def get_container_logs(self, namespace: str, name: str, container: str = "",
                           tail: int = -1, previous: bool = False) -> str:
        with self._pods_lock:
            info = self._pod_status.get(f"{namespace}-{name}")
        if info is None or not info.instance_id:
            return ""
        try:
            return self.runtime.get_logs(info.instance_id, container, tail,
                                         previous=previous)
        except TypeError:
            return self.runtime.get_logs(info.instance_id, container, tail)

    def get_container_log_path(self, namespace: str, name: str,
                               container: str = "") -> Optional[str]:
        """Local log-file path for follow-mode streaming (None when the pod
        has no instance or the runtime keeps no files)."""
        with self._pods_lock:
            info = self._pod_status.get(f"{namespace}-{name}")
        if info is None or not info.instance_id:
            return None
        fn = getattr(self.runtime, "get_log_path", None)
        if fn is None:
            return None
        return fn(info.instance_id, container)

    def pod_log_finished(self, namespace: str, name: str) -> bool:
        """True when no more log output can appear (instance terminal or
        untracked) — the follow-stream stop condition."""
        with self._pods_lock:
            info = self._pod_status.get(f"{namespace}-{name}")
        if info is None or not info.instance_id:
            return True
        return info.status in (PodStatus.EXITED, PodStatus.TERMINATED,
                               PodStatus.NOT_FOUND)

    def run_in_container(self, namespace: str, name: str, command: List[str],
                         timeout_s: float = 30.0, container: str = "") -> tuple:
        """One-shot exec in the pod's environment (GPU binding included).

        The reference returns "not supported by RunPod" (kubelet.go:2027-2047);
        local pods make a non-interactive exec cheap. Returns
        (exit_code, combined_output)."""
        with self._pods_lock:
            info = self._pod_status.get(f"{namespace}-{name}")
        if info is None:
            return 127, f"pod {namespace}/{name} not tracked by this node"
        if not info.instance_id:
            # Pending pod with no backend instance yet: report the pod
            # state instead of a confusing 'instance  not found'.
            return 126, (f"pod {namespace}/{name} has no running instance "
                         f"(status {info.status}); retry once it is Running")
        exec_fn = getattr(self.runtime, "exec_in_instance", None)
        if exec_fn is None:
            return 501, "runtime does not support exec"
        return exec_fn(info.instance_id, command, timeout_s,
                       container=container)

    def instance_info(self, namespace: str, name: str) -> Optional[InstanceInfo]:
        with self._pods_lock:
            return self._pod_status.get(f"{namespace}-{name}")

    def get_stats_summary(self) -> Dict[str, Any]:
        """Kubelet Summary-API-shaped stats (the reference stubs these hooks
        off, main.go:233-235): node CPU/memory, per-pod usage from the
        runtime, and an MI355X extension block with per-GPU HBM/busy/temp."""
        mem_total_kb = mem_avail_kb = 0
        try:
            with open("/proc/meminfo", "r", encoding="ascii") as fh:
                for line in fh:
                    if line.startswith("MemTotal:"):
                        mem_total_kb = int(line.split()[1])
                    elif line.startswith("MemAvailable:"):
                        mem_avail_kb = int(line.split()[1])
        except OSError:
            pass
        summary: Dict[str, Any] = {
            "node": {
                "nodeName": self.node_name,
                "cpu": {"numCores": os.cpu_count() or 1},
                "memory": {
                    "availableBytes": mem_avail_kb * 1024,
                    "usageBytes": max(0, (mem_total_kb - mem_avail_kb) * 1024),
                },
            },
            "pods": [],
        }
        stats_fn = getattr(self.runtime, "get_stats", None)
        with self._pods_lock:
            items = []
            for k, p in self._pods.items():
                info = self._pod_status.get(k)
                items.append((
                    k, dict(meta(p)),
                    info.instance_id if info else "",
                    list(info.gpu_indices) if info else [],
                ))
        for _key, md, instance_id, gpu_indices in items:
            entry: Dict[str, Any] = {
                "podRef": {"name": md.get("name", ""),
                           "namespace": md.get("namespace", "default")},
            }
            if instance_id and callable(stats_fn):
                entry.update(stats_fn(instance_id))
            if gpu_indices:
                entry["gpus"] = gpu_indices
            summary["pods"].append(entry)
        if self.ledger is not None:
            summary["gpus"] = [
                {
                    "index": s.gpu.index,
                    "hbmTotalBytes": s.gpu.vram_total_bytes,
                    "hbmUsedBytes": s.gpu.vram_used_bytes,
                    "busyPercent": s.gpu.busy_percent,
                    "temperatureCelsius": (s.gpu.temperature_mc / 1000.0
                                           if s.gpu.temperature_mc >= 0 else None),
                    "lastCheck": s.gpu.diag_last,
                }
                for s in self.ledger.snapshot()
            ]
        return summary
