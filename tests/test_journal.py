"""Instance journal (runtime/journal.py): on-disk compatibility with the
records the previous release wrote, round trips, and the writer.

CPU-only; starts no processes.

The fixtures under tests/fixtures/journal/ were written by the commit
*before* journal.py existed (its hand-written ``ProcessRuntime._persist``).
To regenerate them, check that commit out together with this file and run

    python tests/test_journal.py tests/fixtures/journal

which calls that ``_persist`` on the instances built below. ``minimal.json``
is hand-written.
"""

import copy
import dataclasses
import json
import shutil
import socket
import sys
import threading
import time
import types
from pathlib import Path

import pytest

from k8s_runpod_kubelet_amd.runtime.probes import ProbeSpec
from k8s_runpod_kubelet_amd.runtime.types import (
    ContainerRuntimeInfo,
    ContainerSpec,
    DeployParams,
    Instance,
    PodStatus,
    VolumeMount,
    VolumeSource,
)

FIXTURES = Path(__file__).parent / "fixtures" / "journal"
GIB = 1024 ** 3


# ------------- the instances the fixtures were made from -------------

def bench_instance() -> Instance:
    """(a) The one-container podworker pod bench.py deploys, Ready."""
    params = DeployParams(
        pod_key="default-bench-0-0", name="bench-0-0", namespace="default",
        containers=[ContainerSpec(
            name="main", image="amdvk/podworker:bench",
            command=["podworker"], args=["--expect-gpus", "1", "--hold"])],
        restart_policy="Never", termination_grace_s=30.0,
        gpu_count=1, gpu_memory_bytes=16 * GIB, max_gpu_cost=0.75,
        hostname="bench-0-0",
    )
    return Instance(
        id="amdvk-0123456789ab", pod_key=params.pod_key, params=params,
        gpu_indices=[3], desired_status=PodStatus.RUNNING,
        containers=[ContainerRuntimeInfo(
            name="main", pid=41001, started_at=1750000000.25, ready=True)],
        cgroup_dir="/sys/fs/cgroup/amdvk.slice/slot1",
        created_at=1750000000.125, cost_per_hr=0.1,
    )


def full_instance() -> Instance:
    """(b) Every persisted field at a non-default value (and a few
    never-persisted ones, to show they come back as defaults)."""
    def probe(kind, **kw):
        return ProbeSpec(kind=kind, initial_delay_s=2.0, period_s=3.0,
                         timeout_s=4.0, failure_threshold=5,
                         success_threshold=2, **kw)

    web = ContainerSpec(
        name="web", image="registry.local/web:1.2",
        command=["/bin/web"], args=["--port", "8080"],
        env={"MODE": "prod", "ROCR_VISIBLE_DEVICES": "9"},
        working_dir="/srv", tcp_ports=[8080, 8443],
        volume_mounts=[
            VolumeMount(name="scratch", mount_path="/scratch",
                        sub_path="web"),
            VolumeMount(name="conf", mount_path="/etc/web", read_only=True,
                        sub_path="site"),
        ],
        run_as_uid=1000, run_as_gid=2000,
        liveness=probe("tcp", port=8080),
        readiness=probe("http", port=8080, path="/healthz"),
        startup=probe("exec", command=["/bin/check", "--startup"]),
        termination_message_path="/tmp/last-words",
        termination_message_policy="FallbackToLogsOnError",
        image_pull_policy="Always", run_as_non_root=True,
        read_only_root_fs=True,
        post_start=probe("exec", command=["/bin/warm"]),
        pre_stop=ProbeSpec(kind="sleep", timeout_s=1.5),
    )
    sidecar = ContainerSpec(
        name="sidecar", image="registry.local/side@sha256:" + "ab" * 32,
        command=["side"], env={"LEVEL": "debug"}, working_dir="/side",
        tcp_ports=[9100],
        volume_mounts=[VolumeMount(name="host", mount_path="/host",
                                   read_only=True, sub_path="logs")],
        run_as_uid=1001, run_as_gid=2001,
        liveness=probe("exec", command=["side", "--alive"]),
        readiness=probe("tcp", port=9100),
        startup=probe("http", port=9100, path="/started"),
        termination_message_path="/run/side.msg",
        termination_message_policy="FallbackToLogsOnError",
        image_pull_policy="Never", run_as_non_root=True,
        read_only_root_fs=True,
        post_start=probe("http", port=9100, path="/hook"),
        pre_stop=probe("exec", command=["side", "--drain"]),
    )
    inits = [
        ContainerSpec(
            name=f"init{i}", image="registry.local/init:3",
            command=["/bin/setup"], args=["--step", str(i)],
            env={"STEP": str(i)}, working_dir="/setup",
            volume_mounts=[VolumeMount(name="scratch",
                                       mount_path="/scratch")],
            run_as_uid=1500 + i, run_as_gid=2500 + i)
        for i in (0, 1)
    ]
    debugger = ContainerSpec(
        name="debugger", image="busybox:1.36", command=["sh"],
        args=["-c", "sleep 600"], env={"DEBUG": "1"}, working_dir="/tmp",
        volume_mounts=[VolumeMount(name="scratch", mount_path="/scratch",
                                   read_only=True)],
        run_as_uid=0, run_as_gid=0)
    params = DeployParams(
        pod_key="team-a-full", name="full", namespace="team-a",
        containers=[web, sidecar], init_containers=inits,
        resolv_conf="nameserver 10.0.0.10\nsearch team-a.svc\n",
        restart_policy="OnFailure", termination_grace_s=45.0,
        active_deadline_s=3600.0,
        env={"POD_TIER": "gold", "SHARED": "1"},
        gpu_count=2, gpu_memory_bytes=96 * GIB,
        volumes={
            "scratch": VolumeSource(kind="emptyDir", medium="Memory",
                                    size_limit_bytes=64 * 1024 * 1024),
            "host": VolumeSource(kind="hostPath", host_path="/var/log"),
            "conf": VolumeSource(kind="files", file_mode=0o400,
                                 files={"site/web.conf": "listen 8080;\n",
                                        "token": "s3cr3t"}),
        },
        hostname="full-host", fs_group=3000,
        host_aliases=[("10.1.2.3", ["db.local", "db"]),
                      ("10.1.2.4", ["cache.local"])],
        # never persisted:
        max_gpu_cost=0.9, requested_ports=["8080/tcp"],
        cpu_limit="200000 100000", memory_limit="1073741824",
        labels={"app": "full"},
    )
    return Instance(
        id="amdvk-fedcba987654", pod_key=params.pod_key, params=params,
        gpu_indices=[1, 6], desired_status=PodStatus.TERMINATING,
        containers=[
            ContainerRuntimeInfo(
                name="web", pid=52001, started_at=1750000100.5, ready=True,
                restart_count=3,
                image_id="registry.local/web:1.2@sha256:" + "cd" * 32,
                # never restored:
                message="liveness probe failed", crash_streak=2,
                pull_seconds=1.25),
            ContainerRuntimeInfo(
                name="sidecar", pid=52002, started_at=1750000101.5,
                finished_at=1750000190.0, exit_code=7, restart_count=1,
                image_id="registry.local/side@sha256:" + "ab" * 32,
                message="exit code 7", backoff_until=1750000200.0),
        ],
        init_containers=[
            ContainerRuntimeInfo(name="init0", pid=51001,
                                 started_at=1750000050.0,
                                 finished_at=1750000060.0, exit_code=0),
            ContainerRuntimeInfo(name="init1", pid=51002,
                                 started_at=1750000060.5),
        ],
        ephemeral_containers=[
            ContainerRuntimeInfo(name="debugger", pid=53001,
                                 started_at=1750000150.0)],
        ephemeral_specs=[debugger],
        init_index=1, cgroup_dir="/sys/fs/cgroup/amdvk.slice/slot17",
        created_at=1750000040.0, cost_per_hr=0.2,
        last_error="DeadlineExceeded",  # never persisted
        deadline_exceeded=True, image_mode="mountns",
    )


# What the previous release wrote for init / ephemeral specs: seven fields
# each. Records it wrote therefore read back with the rest at defaults.
_OLD_INIT_FIELDS = ("name", "image", "command", "args", "run_as_uid",
                    "run_as_gid", "working_dir")
_OLD_EPHEMERAL_FIELDS = ("name", "image", "command", "args", "env",
                         "run_as_uid", "run_as_gid")
# DeployParams fields the journal has never carried
_UNPERSISTED_PARAMS = ("max_gpu_cost", "requested_ports", "cloud_type",
                       "datacenter_ids", "template_id", "registry_auth_id",
                       "cpu_limit", "memory_limit", "labels")


def _only(obj, names):
    """A fresh instance of obj's class keeping just `names`."""
    return type(obj)(**{n: copy.deepcopy(getattr(obj, n)) for n in names})


def restored(inst: Instance, old_writer: bool = False) -> Instance:
    """`inst` as the reader must hand it back: never-restored fields at
    their dataclass defaults. old_writer=True additionally narrows the
    init/ephemeral specs to what the previous release's writer kept."""
    main = ("name", "pid", "started_at", "finished_at", "exit_code",
            "ready", "restart_count", "image_id")
    params = _only(inst.params,
                   [f.name for f in dataclasses.fields(DeployParams)
                    if f.name not in _UNPERSISTED_PARAMS])
    out = dataclasses.replace(
        copy.deepcopy(inst), params=params, last_error="",
        containers=[_only(c, main) for c in inst.containers],
        init_containers=[_only(c, main[:5]) for c in inst.init_containers],
        ephemeral_containers=[_only(c, main[:5])
                              for c in inst.ephemeral_containers],
    )
    if old_writer:
        params.init_containers = [_only(c, _OLD_INIT_FIELDS)
                                  for c in params.init_containers]
        out.ephemeral_specs = [_only(c, _OLD_EPHEMERAL_FIELDS)
                               for c in out.ephemeral_specs]
    return out


def _fixture(name: str) -> dict:
    return json.loads((FIXTURES / name).read_text())


CASES = [("bench.json", bench_instance), ("full.json", full_instance)]


# ------------- 1. records written by the previous release -------------

@pytest.mark.parametrize("fname,build", CASES)
def test_reads_previous_release_record(fname, build):
    from k8s_runpod_kubelet_amd.runtime.journal import instance_from_record

    assert instance_from_record(_fixture(fname)) == restored(
        build(), old_writer=True)


def test_reads_minimal_record():
    from k8s_runpod_kubelet_amd.runtime.journal import instance_from_record

    t0 = time.time()
    inst = instance_from_record(_fixture("minimal.json"))
    t1 = time.time()
    assert t0 <= inst.created_at <= t1
    assert inst == Instance(
        id="amdvk-00000000000c", pod_key="default-tiny",
        params=DeployParams(pod_key="default-tiny", name="default-tiny",
                            termination_grace_s=10.0),
        desired_status=PodStatus.RUNNING,
        containers=[ContainerRuntimeInfo(name="main", pid=4242)],
        created_at=inst.created_at,
    )


def _assert_contains(new, old, path="$"):
    """Every key path of `old` is in `new` with an equal value."""
    if isinstance(old, dict):
        assert isinstance(new, dict), path
        for k, v in old.items():
            assert k in new, f"{path}.{k} missing"
            _assert_contains(new[k], v, f"{path}.{k}")
    elif isinstance(old, list):
        assert isinstance(new, list) and len(new) == len(old), path
        for i, (n, o) in enumerate(zip(new, old)):
            _assert_contains(n, o, f"{path}[{i}]")
    else:
        assert new == old, f"{path}: {new!r} != {old!r}"


@pytest.mark.parametrize("fname,build", CASES)
def test_writes_every_key_the_previous_release_wrote(fname, build):
    """The rollback condition: the previous release can adopt our records."""
    from k8s_runpod_kubelet_amd.runtime.journal import instance_to_record

    new = json.loads(json.dumps(instance_to_record(build())))
    _assert_contains(new, _fixture(fname))


# ------------- 2. round trip -------------

@pytest.mark.parametrize("fname,build", CASES)
def test_round_trip(fname, build):
    from k8s_runpod_kubelet_amd.runtime.journal import (
        instance_from_record,
        instance_to_record,
    )

    inst = build()
    back = instance_from_record(
        json.loads(json.dumps(instance_to_record(inst))))
    assert back == restored(inst)
    for spec in back.params.init_containers + back.ephemeral_specs:
        # the one deliberate difference from the previous release
        assert spec.env and spec.volume_mounts


# ------------- 3. no hand-copied field lists -------------

@dataclasses.dataclass
class _WiderSpec(ContainerSpec):
    gpu_profile: str = "balanced"


def test_spec_codec_follows_the_dataclass():
    from k8s_runpod_kubelet_amd.runtime.journal import (
        spec_from_record,
        spec_to_record,
    )

    spec = _WiderSpec(name="c", gpu_profile="latency",
                      readiness=ProbeSpec(kind="tcp", port=80),
                      volume_mounts=[VolumeMount("v", "/v")])
    rec = json.loads(json.dumps(spec_to_record(spec)))
    assert rec["gpu_profile"] == "latency"
    assert spec_from_record(_WiderSpec, rec) == spec
    del rec["gpu_profile"]
    assert spec_from_record(_WiderSpec, rec).gpu_profile == "balanced"
    assert spec_from_record(ContainerSpec, {"name": "c"}) == ContainerSpec(
        name="c")


# ------------- 4. the writer -------------

def test_write_record_tolerates_vanished_directory(tmp_path, monkeypatch):
    from k8s_runpod_kubelet_amd.runtime.journal import write_record

    d = tmp_path / "instances"
    d.mkdir()
    real_write = Path.write_text

    def write_then_vanish(self, *a, **kw):
        n = real_write(self, *a, **kw)
        shutil.rmtree(d)  # state dir torn down between write and rename
        return n

    monkeypatch.setattr(Path, "write_text", write_then_vanish)
    write_record(d, bench_instance())  # must not raise
    assert not d.exists()


def test_write_record_concurrent_writers(tmp_path):
    from k8s_runpod_kubelet_amd.runtime.journal import write_record

    inst = bench_instance()
    errors = []

    def writer():
        try:
            for _ in range(50):
                write_record(tmp_path, inst)
        except Exception as exc:  # surfaced below
            errors.append(exc)

    threads = [threading.Thread(target=writer) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert [p.name for p in tmp_path.iterdir()] == [f"{inst.id}.json"]
    assert json.loads((tmp_path / f"{inst.id}.json").read_text())["id"] \
        == inst.id


# ------------- procfs -------------

def test_listening_ports_attributed_to_pids():
    import os

    from k8s_runpod_kubelet_amd.runtime.procfs import pod_listening_ports

    with socket.socket() as srv:
        srv.bind(("127.0.0.1", 0))
        srv.listen(1)
        port = srv.getsockname()[1]
        assert port in pod_listening_ports("", {os.getpid()})
        # a pid set without this process (no such pid): nothing reported
        assert pod_listening_ports("", {2 ** 30}) == set()
        assert pod_listening_ports("", set()) == set()


if __name__ == "__main__":
    # Fixture regeneration; run on the commit before journal.py (see the
    # module docstring).
    from k8s_runpod_kubelet_amd.runtime.process_runtime import ProcessRuntime

    out = Path(sys.argv[1])
    out.mkdir(parents=True, exist_ok=True)
    for fname, build in CASES:
        inst = build()
        ProcessRuntime._persist(types.SimpleNamespace(instances_dir=out),
                                inst)
        (out / f"{inst.id}.json").rename(out / fname)
