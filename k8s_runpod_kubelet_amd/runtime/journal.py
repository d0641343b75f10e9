"""Instance journal: <state_dir>/instances/<id>.json records.

Pure functions between ``Instance`` and the JSON record a restarted kubelet
re-adopts pods from (ProcessRuntime.adopt_persisted does the part that needs
the runtime: pidfds, ledger, timers). No native module, no threads, and no
I/O except ``write_record``.

Record layout (kept stable so a rolled-back kubelet can still adopt): flat
instance and pod-level keys, ``pod_env``, ``volumes``, the three spec lists
``container_specs`` / ``init_specs`` / ``ephemeral_specs`` and the three
runtime-info lists ``containers`` / ``init_containers`` /
``ephemeral_containers``. Specs are written from their dataclasses and read
back into them field by field, so a field added to ContainerSpec, ProbeSpec,
VolumeMount or VolumeSource is journaled without touching this file, and a
key absent from an older record takes the dataclass default.
"""

from __future__ import annotations

import dataclasses
import functools
import json
import threading
import typing
from pathlib import Path

from .types import (
    ContainerRuntimeInfo,
    ContainerSpec,
    DeployParams,
    Instance,
    PodStatus,
    VolumeSource,
)

# terminationGracePeriodSeconds assumed for records older than the key
TERM_GRACE_S = 10.0

# Flat top-level keys, named like the attribute they hold.
_INSTANCE_KEYS = ("id", "pod_key", "gpu_indices", "desired_status",
                  "cgroup_dir", "created_at", "cost_per_hr", "init_index",
                  "deadline_exceeded", "image_mode")
_PARAMS_KEYS = ("name", "namespace", "gpu_count", "gpu_memory_bytes",
                "restart_policy", "active_deadline_s", "termination_grace_s",
                "resolv_conf", "hostname", "fs_group")
# Runtime info that survives a kubelet restart. Everything else (message,
# backoff_until, crash_streak, pull_seconds) restarts from its default:
# the restart machinery keys off backoff_until, and a pending backoff does
# not outlive the timer that owned it.
_MAIN_INFO_KEYS = ("name", "pid", "started_at", "finished_at", "exit_code",
                   "ready", "restart_count", "image_id")
_AUX_INFO_KEYS = _MAIN_INFO_KEYS[:5]  # init and ephemeral containers


# ------------- spec codec -------------

spec_to_record = dataclasses.asdict


@functools.lru_cache(maxsize=None)
def _dataclass_fields(cls) -> dict:
    """field name -> (container origin, dataclass) for the fields of `cls`
    annotated as a dataclass, Optional/List of one, or Dict[str, one]."""
    out = {}
    for name, hint in typing.get_type_hints(cls).items():
        for arg in (hint, *typing.get_args(hint)):
            if dataclasses.is_dataclass(arg):
                out[name] = (typing.get_origin(hint), arg)
    return out


def spec_from_record(cls, rec: dict):
    """Construct dataclass `cls` from its ``spec_to_record`` dict. Absent
    and null keys take the dataclass default; unknown keys are ignored."""
    nested = _dataclass_fields(cls)
    kwargs = {}
    for f in dataclasses.fields(cls):
        value = rec.get(f.name)
        if value is None:
            continue
        if f.name in nested:
            origin, sub = nested[f.name]
            if origin is list:
                value = [spec_from_record(sub, v) for v in value]
            elif origin is dict:
                value = {k: spec_from_record(sub, v)
                         for k, v in value.items()}
            else:
                value = spec_from_record(sub, value)
        kwargs[f.name] = value
    return cls(**kwargs)


# ------------- instance records -------------

def instance_to_record(inst: Instance) -> dict:
    params = inst.params
    record = {k: getattr(inst, k) for k in _INSTANCE_KEYS}
    record.update((k, getattr(params, k)) for k in _PARAMS_KEYS)
    record["pod_env"] = params.env
    record["host_aliases"] = [[ip, list(names)]
                              for ip, names in params.host_aliases]
    record["volumes"] = {n: spec_to_record(v)
                         for n, v in params.volumes.items()}
    for key, specs in (("container_specs", params.containers),
                       ("init_specs", params.init_containers),
                       ("ephemeral_specs", inst.ephemeral_specs)):
        record[key] = [spec_to_record(c) for c in specs]
    for key, infos, keep in (
            ("containers", inst.containers, _MAIN_INFO_KEYS),
            ("init_containers", inst.init_containers, _AUX_INFO_KEYS),
            ("ephemeral_containers", inst.ephemeral_containers,
             _AUX_INFO_KEYS)):
        record[key] = [{k: getattr(c, k) for k in keep} for c in infos]
    return record


def _present(rec: dict, keys) -> dict:
    return {k: rec[k] for k in keys if rec.get(k) is not None}


def instance_from_record(rec: dict) -> Instance:
    """Inverse of instance_to_record. Four keys default to something other
    than their dataclass default when absent: ``name`` (the pod key),
    ``desired_status`` (RUNNING: only deployed pods are journaled),
    ``termination_grace_s`` (TERM_GRACE_S) and ``created_at`` (now)."""
    def specs(key):
        return [spec_from_record(ContainerSpec, c)
                for c in rec.get(key) or []]

    def infos(key, keep):
        return [ContainerRuntimeInfo(**_present(c, keep))
                for c in rec.get(key) or []]

    params = DeployParams(**{
        "name": rec["pod_key"],
        "termination_grace_s": TERM_GRACE_S,
        **_present(rec, _PARAMS_KEYS),
        "pod_key": rec["pod_key"],
        "env": rec.get("pod_env") or {},
        "host_aliases": [(ip, list(names))
                         for ip, names in rec.get("host_aliases") or []],
        "volumes": {n: spec_from_record(VolumeSource, v)
                    for n, v in (rec.get("volumes") or {}).items()},
        "containers": specs("container_specs"),
        "init_containers": specs("init_specs"),
    })
    return Instance(**{
        "desired_status": PodStatus.RUNNING,
        **_present(rec, _INSTANCE_KEYS),
        "id": rec["id"],
        "pod_key": rec["pod_key"],
        "params": params,
        "ephemeral_specs": specs("ephemeral_specs"),
        "containers": infos("containers", _MAIN_INFO_KEYS),
        "init_containers": infos("init_containers", _AUX_INFO_KEYS),
        "ephemeral_containers": infos("ephemeral_containers",
                                      _AUX_INFO_KEYS),
    })


def write_record(instances_dir: Path, inst: Instance) -> None:
    # Unique temp name: the event thread and API threads may persist the
    # same instance concurrently; rename is atomic, last writer wins.
    tmp = instances_dir / f".{inst.id}.{threading.get_ident()}.tmp"
    tmp.write_text(json.dumps(instance_to_record(inst)))
    try:
        tmp.rename(instances_dir / f"{inst.id}.json")
    except FileNotFoundError:
        pass  # state dir torn down during shutdown
