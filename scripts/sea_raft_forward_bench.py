"""SEA-RAFT whole forward, from the two frames to the last prediction: stock PyTorch-ROCm against `accelerate(model,
sea_raft_update=...)` alone and against both options (`sea_raft_update=...` and `sea_raft_encoders=...`, ptlflow_amd/sea_encoder.py).

    python scripts/sea_raft_forward_bench.py [--out sea_forward.json] [--reps 5]

The model is the torch-only stand-in of tests/sea_full_model.py (ResNet-18 encoders, seeded weights) at 440 x 1024 — what SEA-RAFT's
padder makes of 436 x 1024 frames — at batch 1 and 8, 4 and 12 iterations, in fp32 and under torch.autocast("cuda", bfloat16) (the
kernel legs then use the "bf16" value of both options).  Device events around the whole forward, warm-up first, the three legs
alternating in one process, median of `--reps` runs.  The stock leg keeps the stand-in's own torch correlation block: the B1 hook that
`accelerate` installs is a global of the model's module, so it is taken out for the stock runs and put back for the others.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 440, 1024


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sea_raft_forward_bench.py measures on the GPU; there is none")
    import ptlflow_amd
    import sea_full_model as M
    from ptlflow_amd import patch
    ptlflow_amd.load_native()
    dev = torch.device("cuda:0")
    torch_corr = M.get_corr_block
    res = {"frame": [H, W], "runs": []}
    for precision in ("fp32", "bf16"):
        models = {name: M.seeded_full(21).to(dev) for name in ("stock", "update", "both")}
        patch.accelerate(models["update"], sea_raft_update=precision)
        patch.accelerate(models["both"], sea_raft_update=precision, sea_raft_encoders=precision)
        hook = M.get_corr_block

        def run(name, x, iters):
            M.get_corr_block = torch_corr if name == "stock" else hook
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
                return models[name](*x, iters=iters)

        for B in (1, 8):
            x = [t.to(dev) for t in M.smooth_images(B, H, W, seed=7)]
            for iters in (4, 12):
                for _ in range(2):                                   # warm-up (MIOpen find, packing, probes)
                    for name in models:
                        run(name, x, iters)
                torch.cuda.synchronize()
                t = {name: [] for name in models}
                for _ in range(args.reps):                           # alternating
                    for name in models:
                        t[name].append(_time(lambda: run(name, x, iters)))
                ms = {name: statistics.median(v) for name, v in t.items()}
                both = models["both"]
                row = {"precision": precision, "B": B, "iters": iters, "stock_ms": round(ms["stock"], 3),
                       "update_ms": round(ms["update"], 3), "both_ms": round(ms["both"], 3),
                       "both_vs_update": round(ms["update"] / ms["both"], 3), "both_vs_stock": round(ms["stock"] / ms["both"], 3),
                       "spread_ms": {name: [round(min(v), 3), round(max(v), 3)] for name, v in t.items()},
                       "kernel_calls": [both.fnet.calls, both.cnet.calls, both.init_conv.calls, both.flow_head.calls]}
                res["runs"].append(row)
                print(json.dumps(row), flush=True)
        M.get_corr_block = hook
        for m in models.values():
            patch.restore(m)
        M.get_corr_block = torch_corr
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
