#!/usr/bin/env python3
"""One training step of the RAFT mirror at BASELINE config 5 (batch 10, 368x496 crops, 12 iterations; forward, sequence loss,
backward, clipping, AdamW step — bench.py's `train` leg) with `train_precision="bf16"` against `"fp32"` — GPU box.
    python scripts/train_bf16_bench.py [--samples 9] [--batch 10] [--iters 12]
Device events, the two legs alternating in one process, median of `--samples` steps with the min-max spread, and each leg's peak
memory (torch.cuda.max_memory_allocated over one step; both models' parameters and optimizer states are resident throughout).
Second table: the update block's forward + backward alone (12 chained `update_block_train_pm` calls on the inputs recorded
from one real forward, step-scoped weight-gradient accumulation on), same protocol."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptlflow_amd  # noqa: E402
import ptlflow_amd.train as TR  # noqa: E402
from ptlflow_amd.raft import RAFT  # noqa: E402

ptlflow_amd.load_native()
LEGS = ("fp32", "bf16")


def timed_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(legs, samples, warmup=2):
    for f in legs.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    t, peak = {k: [] for k in legs}, {}
    for _ in range(samples):
        for k, f in legs.items():
            torch.cuda.reset_peak_memory_stats()
            t[k].append(timed_ms(f))
            peak[k] = torch.cuda.max_memory_allocated()
    return t, peak


def report(title, t, peak, per_step=None):
    print(title)
    for k, v in t.items():
        extra = f", {per_step / statistics.median(v) * 1e3:7.1f} samples/s" if per_step else ""
        print(f"  {k}: median {statistics.median(v):8.2f} ms  (min {min(v):8.2f} - max {max(v):8.2f}){extra}, peak memory {peak[k] / 2**20:8.0f} MiB")
    a, b = t["fp32"], t["bf16"]
    print(f"  fp32 / bf16 (medians): {statistics.median(a) / statistics.median(b):.3f}x;  bf16 range entirely below fp32's: {max(b) < min(a)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=12)
    args = ap.parse_args()
    dev = torch.device("cuda")
    H, W = 368, 496
    g = torch.Generator().manual_seed(99)
    inputs = {"images": torch.rand(args.batch, 2, 3, H, W, generator=g).to(dev)}
    gt = (torch.rand(args.batch, 2, H, W, generator=g) * 20 - 10).to(dev)
    valid = torch.ones(args.batch, 1, H, W, device=dev)
    models = {k: RAFT(iters=args.iters, train_precision=k).load_synthetic(1234).to(dev).train() for k in LEGS}
    opts = {k: torch.optim.AdamW(m.parameters(), lr=4e-4, weight_decay=1e-4, eps=1e-8) for k, m in models.items()}

    def step(k):
        out = models[k](inputs)
        loss = TR.sequence_loss(out["flow_preds"], gt, valid, 0.8, 400.0)
        opts[k].zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(models[k].parameters(), 1.0)
        opts[k].step()

    t, peak = alternate({k: (lambda k=k: step(k)) for k in LEGS}, args.samples)
    report(f"training step, batch {args.batch}, {H}x{W}, {args.iters} iterations", t, peak, per_step=args.batch)

    # ---- the update block alone, on the inputs one real forward hands it
    rec = []
    real = TR.update_block_train_pm

    def recorder(P, spec, h, i, c, f, *a, **kw):
        rec.append((h.detach().clone(), i.detach().clone(), c.detach().clone(), f.detach().clone()))
        return real(P, spec, h, i, c, f, *a, **kw)

    TR.update_block_train_pm = recorder
    try:
        with torch.enable_grad():
            models["fp32"](inputs)
    finally:
        TR.update_block_train_pm = real
    h0, i0 = rec[0][0], rec[0][1]
    B, hh, ww = args.batch, H // 8, W // 8

    def block(k):
        m = models[k]
        P = dict(m.update_block.named_parameters())
        h, i, cache, loss = h0.clone().requires_grad_(), i0.clone().requires_grad_(), {}, 0.0
        for _, _, c, f in rec:
            h, mask, delta = real(P, m.spec, h, i, c, f, B, hh, ww, cache, accumulate_wgrad=True, precision=k)
            loss = loss + mask.square().mean() + delta.square().mean()
        (loss + h.square().mean()).backward()
        opts[k].zero_grad(set_to_none=True)

    t, peak = alternate({k: (lambda k=k: block(k)) for k in LEGS}, args.samples)
    report(f"update block alone: {len(rec)} chained calls, forward + backward", t, peak)


if __name__ == "__main__":
    main()
