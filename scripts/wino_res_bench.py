"""The encoder's 3x3 stride-1 convolutions: Winograd F(2x2,3x3) (`pfk_conv2d_wino_f32`, `pfk_conv2d_wino_res_f32`) against the direct
implicit GEMM (`pfk_conv2d_f32`) on ResNetFPN's shapes.

    python scripts/wino_res_bench.py [--out wino_res.json]

    python scripts/wino_res_bench.py --encoder raft      # RAFT's BasicEncoder: 64 at 218 x 512, 96 at 109 x 256, 128 at 55 x 128

Shapes: cin = cout = 64 at 220 x 512, 128 at 110 x 256, 256 at 55 x 128 (440 x 1024 frames), 1, 2, 8 and 16 images (one pair is one
6-channel `cnet` pass of B images and two `fnet` passes of B images each).  Two forms per shape, as ResNetFPNEngine launches them: a
block's conv1 (bias + relu) and its conv2 (bias + relu, + residual, relu).  Alternating in one process, median of `--reps` timings of 10
back-to-back launches (device events).  The selection rule of sea_encoder.py is read off this table.
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

LAUNCHES = 10
SHAPES = ((64, 220, 512), (128, 110, 256), (256, 55, 128))
# BasicEncoder (ptlflow_amd/encoder.py) on 436 x 1024 frames; 96 columns are padded to 128 by the Winograd kernel
RAFT_SHAPES = ((64, 218, 512), (96, 109, 256), (128, 55, 128))


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES * 1e3        # us per launch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--encoder", choices=("sea", "raft"), default="sea", help="whose shapes: ResNetFPN's or BasicEncoder's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wino_res_bench.py measures on the GPU; there is none")
    import ptlflow_amd
    from ptlflow_amd.packing import pack_conv_weight, pack_wino_weight
    ptlflow_amd.load_native()
    ops = torch.ops.pfk
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for C, H, W in (RAFT_SHAPES if args.encoder == "raft" else SHAPES):
        wt = torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5
        wd = pack_conv_weight(wt, [(0, C, C)]).to(dev)
        ww = pack_wino_weight(wt).to(dev)
        bias = torch.zeros(C, device=dev)
        for N in (1, 2, 8, 16):
            M = N * H * W
            x = torch.randn(M, C, generator=g).to(dev)
            res = torch.randn(M, C, generator=g).to(dev)
            out = torch.empty(M, C, device=dev)
            legs = {
                "conv1_direct": lambda: ops.conv2d([x], N, H, W, 3, 3, wd, bias, C, 0, True, 1.0, out, None, None, None, None, None, 1, False),
                "conv1_wino": lambda: ops.conv2d_wino(x, N, H, W, ww, bias, C, True, 1.0, out, 0),
                "conv2_direct": lambda: ops.conv2d([x], N, H, W, 3, 3, wd, bias, C, 0, True, 1.0, out, None, None, None, None, res, 1, True),
                "conv2_wino_res": lambda: ops.conv2d_wino_res(x, N, H, W, ww, bias, C, True, 1.0, out, res, True),
            }
            t = {k: [] for k in legs}
            for rep in range(args.reps + 1):             # the first round is the warm-up
                for k, f in legs.items():
                    us = _time(f)
                    if rep:
                        t[k].append(us)
            row = {"C": C, "H": H, "W": W, "images": N, **{k: round(statistics.median(v), 1) for k, v in t.items()}}
            row["conv1_speedup"] = round(row["conv1_direct"] / row["conv1_wino"], 3)
            row["conv2_speedup"] = round(row["conv2_direct"] / row["conv2_wino_res"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"us_per_launch": rows}, f, indent=1)


if __name__ == "__main__":
    main()
