"""bench.py's launcher logic on the CPU (no GPU, no processes started): `python bench.py --gpus N` without a launcher must re-exec
itself under torch.distributed.run with N ranks on 127.0.0.1 and pass its own arguments through; with fewer visible devices than
ranks it must exit non-zero instead (the one-device smoke flag aside).  The GPU side of the same contract — two real ranks, the
`n_gpus` / `ranks_seen` fields of the line — is tests/test_gpu_two_ranks_one_device.py."""
import importlib
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    sys.path.insert(0, ROOT)
    mod = importlib.import_module("bench")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    return mod


def _args(n):
    return types.SimpleNamespace(gpus=n)


def test_self_launch_builds_the_documented_command(bench, monkeypatch):
    import subprocess
    seen = {}
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2"])
    monkeypatch.delenv("PFK_BENCH_SHARED_DEVICE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.self_launch(_args(4))
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    # torchrun picks the free port itself (`--standalone`), on 127.0.0.1: no probe socket of ours, no window for a port race
    assert "--standalone" in cmd and cmd[cmd.index("--local-addr") + 1] == "127.0.0.1"
    assert "--master-port" not in cmd
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"]           # its own arguments, unchanged
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def test_self_launch_refuses_more_ranks_than_devices(bench, monkeypatch):
    import subprocess
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(subprocess, "call", lambda *a, **k: pytest.fail("must not launch"))
    monkeypatch.delenv("PFK_BENCH_SHARED_DEVICE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.self_launch(_args(8))
    assert e.value.code not in (0, None) and "only 1 GPU" in str(e.value.code)


def test_self_launch_shared_device_smoke_flag(bench, monkeypatch):
    import subprocess
    seen = {}
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd) or 0)
    monkeypatch.setenv("PFK_BENCH_SHARED_DEVICE", "1")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit):
        bench.self_launch(_args(2))
    assert "--nproc-per-node=2" in seen["cmd"]


def test_dump_outputs_writes_float32_arrays_within_budget(bench, tmp_path):
    """`--dump-outputs DIR`: every tensor of the output dict as DIR/<name>.npy in float32 (bf16 widened, lists left out); above the
    64 MB budget the same seeded sample on every call, so that two builds compare file for file."""
    import numpy as np
    small = {"flows": torch.randn(2, 1, 2, 8, 16), "flow_small": torch.randn(2, 2, 1, 2).bfloat16(), "flow_preds": [torch.zeros(1)]}
    shapes = bench.dump_outputs(small, str(tmp_path / "a"))
    assert shapes == {"flows": [2, 1, 2, 8, 16], "flow_small": [2, 2, 1, 2]}
    got = np.load(tmp_path / "a" / "flows.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small["flows"].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "flow_small.npy"), small["flow_small"].float().numpy())
    big = {"flows": torch.randn(24, 1, 2, 436, 1024), "flow_small": torch.randn(24, 2, 55, 128)}
    bench.dump_outputs(big, str(tmp_path / "b"))
    bench.dump_outputs(big, str(tmp_path / "c"))
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["flow_small.npy", "flows.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= bench.DUMP_BUDGET_BYTES
    for f in files:
        a, b = np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f)
        assert a.dtype == np.float32 and a.size > 0 and np.array_equal(a, b)
        assert np.isin(a, big[f[:-4]].numpy().reshape(-1)).all()


def test_full_is_off_by_default(bench, monkeypatch):
    """A plain run times the headline only; the legs beside it (roofline, CPU baseline, other precisions, sizes and models) run
    with `--full`, which every switch that thins them out leaves alone."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-extra-legs", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.full is True and a.no_extra_legs and a.no_cpu_baseline
