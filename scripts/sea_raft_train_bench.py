#!/usr/bin/env python3
"""One SEA-RAFT training step of the refinement loop — the torch stand-in of tests/sea_seam_model.py (the reference's module layout,
no encoders): forward, a fixed linear loss over `flows` / `info` / `flow_small`, `zero_grad`, backward — GPU box.
    python scripts/sea_raft_train_bench.py [--samples 9] [--batch 8] [--iters 4] [--grids 46x62,55x128] [--legs native,native_up]
The legs alternating in one process, device events around the whole Python step (so the host's launch overhead is in: a whole-step
figure), median of `--samples` with the min-max spread, and each leg's peak memory (torch.cuda.max_memory_allocated over one step).

* ``modules``  `accelerate(model)` as it was: seam B1 only (correlation volume and lookup, their native backward); the motion encoder,
  both ConvNeXt blocks and both heads are the model's own modules: MIOpen / rocBLAS under torch's autograd.
* ``native``   `accelerate(model, sea_raft_update=True, sea_raft_train=True)`: those calls on ptlflow_amd/train_sea.py (K12d).
  `upsample_data` is the model's own method in both.
* ``native_up``  the same with `train_upsample=True`: `upsample_data` on `train_sea.upsample_data_train` (K12e) — ``native`` is its
  baseline.
* ``native_bf16``  ``native_up`` with `train_precision="bf16"` (K12f): the update block and heads on bf16 rows — the dense convolutions
  on the bf16 matrix cores, depthwise + LayerNorm and GELU on the `_b16` row kernels; ``native_up`` is its baseline.
* ``modules_autocast``  ``modules`` with the whole step's forward under `torch.autocast("cuda", bfloat16)`: what the reference trains
  with, the model's own modules in 16 bits.

`--trace-leg LEG` runs warm-up and then `--samples` steps of ONE leg at the first grid only (for a rocprofv3 --kernel-trace run)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptlflow_amd  # noqa: E402
from ptlflow_amd import patch  # noqa: E402
from sea_seam_model import SeaRaftLoop, load_seeded  # noqa: E402

ptlflow_amd.load_native()
LEGS = ("modules", "native", "native_up", "native_bf16", "modules_autocast")


def timed_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(batch, h, w, iters, samples, legs, warmup=2):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(99)
    x = [torch.tanh(torch.randn(batch, 128, h, w, generator=g)), torch.relu(torch.randn(batch, 128, h, w, generator=g)),
         torch.randn(batch, 256, h, w, generator=g) * 0.3, torch.randn(batch, 256, h, w, generator=g) * 0.3]
    x = [t.to(dev) for t in x]
    R = {"flows": torch.randn(batch, 1, 2, 8 * h, 8 * w, generator=g).to(dev), "info": torch.randn(batch, 4, 8 * h, 8 * w, generator=g).to(dev),
         "flow_small": torch.randn(batch, 2, h, w, generator=g).to(dev)}
    # one model per leg, the same weights; seam B1 (a global of the model's module) serves both
    models = {"modules": patch.accelerate(load_seeded(SeaRaftLoop(iters=iters), 7).to(dev).train()),
              "native": patch.accelerate(load_seeded(SeaRaftLoop(iters=iters), 7).to(dev).train(), sea_raft_update=True, sea_raft_train=True),
              "native_up": patch.accelerate(load_seeded(SeaRaftLoop(iters=iters), 7).to(dev).train(), sea_raft_update=True,
                                            sea_raft_train=True, train_upsample=True),
              "native_bf16": patch.accelerate(load_seeded(SeaRaftLoop(iters=iters), 7).to(dev).train(), sea_raft_update=True,
                                              sea_raft_train=True, train_upsample=True, train_precision="bf16"),
              "modules_autocast": patch.accelerate(load_seeded(SeaRaftLoop(iters=iters), 7).to(dev).train())}

    def step(leg):
        m = models[leg]
        with torch.autocast("cuda", torch.bfloat16, enabled=leg == "modules_autocast"):
            out = m(*x)
        loss = sum((out[k] * R[k]).sum() for k in R)
        m.zero_grad(set_to_none=True)
        loss.backward()

    for leg in legs:
        for _ in range(warmup):
            step(leg)
    torch.cuda.synchronize()
    t, peak = {k: [] for k in legs}, {}
    for _ in range(samples):
        for leg in legs:
            torch.cuda.reset_peak_memory_stats()
            t[leg].append(timed_ms(lambda: step(leg)))
            peak[leg] = torch.cuda.max_memory_allocated()
    assert "native" not in legs or models["native"].update_block.train_calls > 0 and models["native"].flow_head.train_calls > 0
    assert "native_up" not in legs or models["native_up"].upsample_data.train_calls == (warmup + samples) * (iters + 1)
    assert models["native"].upsample_data.train_calls == 0
    nb = models["native_bf16"]
    assert nb.update_block.train_precision == "bf16" and models["native_up"].update_block.train_precision == "fp32"
    assert "native_bf16" not in legs or (nb.update_block.train_calls == (warmup + samples) * iters
                                         and nb.flow_head.train_calls == nb.upsample_weight.train_calls == (warmup + samples) * (iters + 1)
                                         and nb.upsample_data.train_calls == (warmup + samples) * (iters + 1))
    assert not hasattr(models["modules_autocast"].update_block, "train_calls")      # the model's own modules
    for m in models.values():
        patch.restore(m)
    return t, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--grids", default="46x62,55x128")
    ap.add_argument("--trace-leg", default="")
    ap.add_argument("--legs", default=",".join(LEGS))
    args = ap.parse_args()
    legs = [args.trace_leg] if args.trace_leg else args.legs.split(",")
    assert all(k in LEGS for k in legs), f"legs are {LEGS}"
    grids = [tuple(map(int, s.split("x"))) for s in args.grids.split(",")]
    if args.trace_leg:
        grids = grids[:1]
    for h, w in grids:
        t, peak = run(args.batch, h, w, args.iters, args.samples, legs)
        print(f"SEA-RAFT refinement training step, batch {args.batch}, grid {h}x{w}, {args.iters} iterations, {torch.cuda.get_device_name(0)}, "
              f"torch {torch.__version__}, median of {args.samples}")
        for k in legs:
            v = t[k]
            print(f"  {k:9s}: median {statistics.median(v):8.2f} ms  (min {min(v):8.2f} - max {max(v):8.2f}), peak memory {peak[k] / 2**20:8.0f} MiB")
        print(json.dumps({"batch": args.batch, "grid": [h, w], "iters": args.iters, "median_ms": {k: statistics.median(v) for k, v in t.items()},
                          "min_ms": {k: min(v) for k, v in t.items()}, "max_ms": {k: max(v) for k, v in t.items()}, "peak_bytes": peak}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
