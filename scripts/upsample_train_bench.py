#!/usr/bin/env python3
"""Training through the upsampling seams (K12e) — GPU box.
    python scripts/upsample_train_bench.py [--samples 9] [--batch 8] [--grid 55x128] [--iters 12] [--only kernel|raft]

1. ``kernel``: `torch.ops.pfk.convex_upsample_info_bwd` alone (its two launches and the workspace from the caching allocator) at
   n_info = 4 and 0, next to the wave-per-pixel `convex_upsample_bwd` (RAFT's, two channels).  Device events around `--calls`
   back-to-back calls, median of `--samples`; the achieved HBM rate is the ALGORITHMIC bytes over that time: per coarse pixel 576 * 4
   mask bytes read, 576 * 4 gradient bytes written and 64 * C * 4 upsampled-gradient bytes read (the flow / info rows, the partial
   sums and their gather are not counted), against the 8.0 TB/s peak.
2. ``raft``: one training step (forward + backward, device events around both) of tests/seam_model.py's SeamRAFT in train mode,
   `accelerate(model)` (``off``: `upsample_flow` in a gradient graph is the model's own torch method) against
   `accelerate(model, train_upsample=True)` (``on``), legs alternating in one process, median of `--samples`.
The SEA-RAFT pair is scripts/sea_raft_train_bench.py's ``native`` / ``native_up`` legs."""
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

ptlflow_amd.load_native()
HBM_PEAK = 8.0e12


def timed_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def algorithmic_bytes(M, C):
    return M * (576 * 4 + 576 * 4 + 64 * C * 4)


def kernel(batch, h, w, samples, calls):
    dev, ops = torch.device("cuda"), torch.ops.pfk
    g = torch.Generator().manual_seed(1)
    M = batch * h * w
    fo = torch.randn(M, 8, generator=g).to(dev)
    mask = torch.randn(M, 576, generator=g).to(dev)
    gf = torch.randn(batch, 2, 8 * h, 8 * w, generator=g).to(dev)
    gi = torch.randn(batch, 4, 8 * h, 8 * w, generator=g).to(dev)
    gmask, gfo = torch.empty(M, 576, device=dev), torch.empty(M, 8, device=dev)
    gflow_nchw = torch.empty(batch, 2, h, w, device=dev)
    legs = {
        "info_bwd n_info=4": (6, lambda: ops.convex_upsample_info_bwd(fo[:, :2], fo[:, 2:6], mask, gf, gi, gmask, gfo[:, :2], gfo[:, 2:6])),
        "info_bwd n_info=0": (2, lambda: ops.convex_upsample_info_bwd(fo[:, :2], fo[:, 2:2], mask, gf, None, gmask, gfo[:, :2], gfo[:, 2:2])),
        "convex_upsample_bwd (wave per pixel)": (2, lambda: ops.convex_upsample_bwd(fo[:, :2], mask, gf, gmask, gflow_nchw)),
    }
    for _, f in legs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(samples):
        for k, (_, f) in legs.items():
            t[k].append(timed_ms(lambda: [f() for _ in range(calls)]) / calls * 1e3)
    print(f"convex-upsampling backward alone, batch {batch}, grid {h}x{w} (M = {M}), {torch.cuda.get_device_name(0)}, "
          f"median of {samples} x {calls} calls")
    res = {}
    for k, (C, _) in legs.items():
        us, nbytes = statistics.median(t[k]), algorithmic_bytes(M, C)
        rate = nbytes / (us * 1e-6)
        res[k] = {"median_us": us, "min_us": min(t[k]), "max_us": max(t[k]), "algorithmic_bytes": nbytes, "hbm_fraction": rate / HBM_PEAK}
        print(f"  {k:38s}: {us:8.1f} us (min {min(t[k]):8.1f} - max {max(t[k]):8.1f}); {nbytes / 1e6:6.0f} MB algorithmic -> "
              f"{rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of the 8.0 TB/s peak")
    print(json.dumps({"kernel": res, "batch": batch, "grid": [h, w]}), flush=True)


def raft(batch, h, w, iters, samples, warmup=2):
    from seam_model import SeamRAFT
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(2)
    images = torch.rand(batch, 2, 3, 8 * h, 8 * w, generator=g).to(dev)
    R = (torch.randn(batch, 1, 2, 8 * h, 8 * w, generator=g).to(dev), torch.randn(batch, 2, h, w, generator=g).to(dev))
    torch.manual_seed(3)
    models = {"off": SeamRAFT(iters=iters).to(dev).train(), "on": SeamRAFT(iters=iters).to(dev).train()}
    models["on"].load_state_dict(models["off"].state_dict())
    patch.accelerate(models["off"])
    patch.accelerate(models["on"], train_upsample=True)

    def step(leg):
        m = models[leg]
        out = type(m).forward.__wrapped__(m, {"images": images})      # the stand-in's forward is wrapped in no_grad for its eval callers
        loss = (out["flows"] * R[0]).sum() + (out["flow_small"] * R[1]).sum()
        m.zero_grad(set_to_none=True)
        loss.backward()

    for leg in models:
        for _ in range(warmup):
            step(leg)
    torch.cuda.synchronize()
    t = {k: [] for k in models}
    for _ in range(samples):
        for leg in models:
            t[leg].append(timed_ms(lambda: step(leg)))
    on, off = models["on"].upsample_flow, models["off"].upsample_flow
    assert on.train_calls == (warmup + samples) * iters and off.train_calls == 0 and off.calls == 0, (on.train_calls, off.train_calls, off.calls)
    for m in models.values():
        patch.restore(m)
    print(f"SeamRAFT training step (forward + backward), batch {batch}, grid {h}x{w}, {iters} iterations, {torch.cuda.get_device_name(0)}, "
          f"torch {torch.__version__}, median of {samples}")
    for k, v in t.items():
        print(f"  train_upsample {k:3s}: median {statistics.median(v):8.2f} ms  (min {min(v):8.2f} - max {max(v):8.2f})")
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"  on / off = {med['on'] / med['off']:.4f}")
    print(json.dumps({"raft": {"median_ms": med, "min_ms": {k: min(v) for k, v in t.items()}, "max_ms": {k: max(v) for k, v in t.items()}},
                      "batch": batch, "grid": [h, w], "iters": iters}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", default="55x128")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--only", default="", choices=["", "kernel", "raft"])
    args = ap.parse_args()
    h, w = map(int, args.grid.split("x"))
    if args.only in ("", "kernel"):
        kernel(args.batch, h, w, args.samples, args.calls)
    if args.only in ("", "raft"):
        raft(args.batch, h, w, args.iters, args.samples)


if __name__ == "__main__":
    main()
