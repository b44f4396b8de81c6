"""bench.py's two modes on a small configuration: a plain run prints the headline fields only (no leg beside it runs), and
`--full` adds the legs that apply to that configuration (the reference-protocol, dropin, config 3 / 4 and training legs need the
default 436x1024 RAFT configuration and stay out here)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--iters", "4", "--height", "184", "--width", "320"]
# every key a leg beside the headline writes into the line
_LEGS = {"batch1", "batch16", "roofline", "roofline_lookup", "kernels", "cpu_baseline", "epe_vs_cpu", "split_bf16",
         "skip_dead_upsample", "single_chain_gru", "model_benchmark_protocol", "dropin", "config3", "config4", "train",
         "roofline_bf16"}


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *_SMALL, *extra], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(r):
    assert r["metric"] == "frame-pairs/sec, raft 4-iter 184x320" and r["unit"] == "frame-pairs/s"
    assert r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["steps"] == 2 and r["warmup"] == 1 and r["streamk_faults"] == 0
    assert r["value"] == pytest.approx(2 * 1e3 / r["ms_per_step"], rel=1e-6)


def test_plain_run_prints_the_headline_only(gpu):
    r = _run()
    _check_headline(r)
    assert not _LEGS & set(r), sorted(_LEGS & set(r))


def test_full_run_adds_the_legs(gpu):
    r = _run("--full")
    _check_headline(r)
    assert {"batch1", "roofline", "cpu_baseline", "epe_vs_cpu", "split_bf16", "skip_dead_upsample", "single_chain_gru"} <= set(r)
    assert r["epe_vs_cpu"]["mean"] <= r["epe_vs_cpu"]["gate"]
