#!/usr/bin/env python3
"""One GMA training step of the mirror (forward, sequence loss, backward) at BASELINE config 5's shape — 368x496 crops, 12
iterations, the largest batch of {10, 8, 4} that fits — GPU box.
    python scripts/gma_train_bench.py [--samples 9] [--batches 10,8,4] [--iters 12] [--legs parent-fp32,fp32,bf16]
Three legs alternating in one process, device events, median of `--samples` steps with the min-max spread, and each leg's peak
memory (torch.cuda.max_memory_allocated over one step; the models' parameters are resident throughout).  The timed region is the
whole Python step — forward, loss, `zero_grad`, backward — so it includes the host's launch overhead: a whole-step figure.

* ``parent-fp32``  what the mirror ran before K12c: the attention map on torch ops (`_Attention.forward`) and the aggregate as
  ``torch.bmm`` under torch's autograd (one rocBLAS batched GEMM forward and two backward per iteration, one [B,1,N,N] gradient of
  the map per iteration).  That composition lives HERE only (`parent_path`): the library no longer contains it.
* ``fp32``         `_AttentionMap` + `_AttnMatmul` with the step sink (ptlflow_amd/train.py)
* ``bf16``         the same with ``train_precision="bf16"``

`--trace-leg LEG` runs warm-up and then `--samples` steps of ONE leg only (for a rocprofv3 --kernel-trace run)."""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptlflow_amd  # noqa: E402
import ptlflow_amd.train as TR  # noqa: E402
from ptlflow_amd.raft import GMA  # noqa: E402

ptlflow_amd.load_native()
H, W = 368, 496


@contextlib.contextmanager
def parent_path(model):
    """The parent commit's GMA pieces, put in place of the new nodes for the duration of one step."""
    state, matmul, amap = TR._attention_state, TR._AttnMatmul, TR.attention_map_train

    class Map:
        def target(self, attention):
            return attention

    class Bmm:
        @staticmethod
        def apply(attention, v, _state):
            B, _, N, _ = attention.shape
            return torch.bmm(attention.reshape(B, N, N).float(), v.view(B, N, v.shape[1])).reshape(B * N, v.shape[1])

    def torch_attention(ipm, weight, B, h, w, scale, packs=None):
        return model.att(ipm.view(B, h, w, ipm.shape[1]).permute(0, 3, 1, 2))

    TR._attention_state = lambda attention, *a, **k: Map()
    TR._AttnMatmul, TR.attention_map_train = Bmm, torch_attention
    try:
        yield
    finally:
        TR._attention_state, TR._AttnMatmul, TR.attention_map_train = state, matmul, amap


def timed_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(batch, iters, samples, legs, warmup=2):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(99)
    inputs = {"images": torch.rand(batch, 2, 3, H, W, generator=g).to(dev)}
    gt = (torch.rand(batch, 2, H, W, generator=g) * 20 - 10).to(dev)
    valid = torch.ones(batch, 1, H, W, device=dev)
    models = {"fp32": GMA(iters=iters).load_synthetic(1234).to(dev).train()}
    if "bf16" in legs:
        models["bf16"] = GMA(iters=iters, train_precision="bf16").load_synthetic(1234).to(dev).train()
    models["parent-fp32"] = models["fp32"]

    def step(k):
        m = models[k]
        with (parent_path(m) if k == "parent-fp32" else contextlib.nullcontext()):
            out = m(inputs)
            loss = TR.sequence_loss(out["flow_preds"], gt, valid, 0.8, 400.0)
            m.zero_grad(set_to_none=True)
            loss.backward()

    for k in legs:
        for _ in range(warmup):
            step(k)
    torch.cuda.synchronize()
    t, peak = {k: [] for k in legs}, {}
    for _ in range(samples):
        for k in legs:
            torch.cuda.reset_peak_memory_stats()
            t[k].append(timed_ms(lambda: step(k)))
            peak[k] = torch.cuda.max_memory_allocated()
    return t, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--batches", default="10,8,4")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--legs", default="parent-fp32,fp32,bf16")
    ap.add_argument("--trace-leg", default="")
    args = ap.parse_args()
    legs = [args.trace_leg] if args.trace_leg else args.legs.split(",")
    for batch in map(int, args.batches.split(",")):
        try:
            t, peak = run(batch, args.iters, args.samples, legs)
            break
        except torch.cuda.OutOfMemoryError:
            print(f"batch {batch} does not fit", flush=True)
            torch.cuda.empty_cache()
    else:
        raise SystemExit("no batch of --batches fits")
    N = (H // 8) * (W // 8)
    print(f"GMA training step, batch {batch}, {H}x{W} (N = {N}), {args.iters} iterations, {torch.cuda.get_device_name(0)}, "
          f"torch {torch.__version__}, median of {args.samples}")
    for k in legs:
        v = t[k]
        print(f"  {k:12s}: median {statistics.median(v):8.2f} ms  (min {min(v):8.2f} - max {max(v):8.2f}), "
              f"{batch / statistics.median(v) * 1e3:6.2f} samples/s, peak memory {peak[k] / 2**20:8.0f} MiB")
    if "parent-fp32" in t and "fp32" in t:
        print(f"  fp32 / parent-fp32 (medians): {statistics.median(t['fp32']) / statistics.median(t['parent-fp32']):.3f};  peak memory "
              f"{(peak['parent-fp32'] - peak['fp32']) / 2**20:.0f} MiB lower  ((T-1) B N^2 4 bytes = {(args.iters - 1) * batch * N * N * 4 / 2**20:.0f} MiB)")
    print(json.dumps({"batch": batch, "iters": args.iters, "median_ms": {k: statistics.median(v) for k, v in t.items()},
                      "min_ms": {k: min(v) for k, v in t.items()}, "max_ms": {k: max(v) for k, v in t.items()},
                      "peak_bytes": peak}))


if __name__ == "__main__":
    main()
