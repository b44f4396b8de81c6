#!/usr/bin/env python3
"""In-isolation timing of the update block's 3x3 convolutions (fm 128 -> 512, c2 256 -> 192, cv 256 -> 126, f2 128 -> 64 at 55x128) on the
direct implicit-GEMM kernel (`pfk_conv2d_f32`, tile grid, and with the stream-K workspace as the engine passes it) and on the Winograd
F(2x2,3x3) kernel (`pfk_conv2d_wino_f32`), at several batch sizes: the measurement behind update.py's WINO_MIN_WORK and WINO_F2_MIN_PIXELS.

    python scripts/wino_bench.py [--batches 1 2 4 8] [--reps 50] [--grid 55x128] [--keys fm c2 cv f2] [--rounds 1]

`--rounds N` times direct and Winograd alternately N times and prints the median of each with the direct kernel's max - min.
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import ptlflow_amd  # noqa: E402
from ptlflow_amd.packing import pack_conv_weight, pack_wino_weight  # noqa: E402

SHAPES = {"fm": (128, 512), "c2": (256, 192), "cv": (256, 126), "f2": (128, 64)}


def timed(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--grid", default="55x128", help="HxW of the 1/8 grid")
    ap.add_argument("--keys", nargs="+", default=["fm", "c2", "cv"], choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    ptlflow_amd.load_native()
    ops = torch.ops.pfk
    H, W = map(int, args.grid.split("x"))
    ws = torch.zeros(ops.conv_workspace_bytes(), device="cuda", dtype=torch.uint8)
    for B in args.batches:
        M = B * H * W
        for key in args.keys:
            cin, cout = SHAPES[key]
            g = torch.Generator().manual_seed(0)
            wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
            bias = torch.randn(cout, generator=g).cuda()
            x = torch.randn(M, cin, device="cuda")
            out = torch.zeros(M, cout, device="cuda")
            wd = pack_conv_weight(wt, [(0, cin, cin)]).cuda()
            ww = pack_wino_weight(wt).cuda()
            ds, wsn = [], []
            for _ in range(args.rounds):
                ds.append(timed(lambda: ops.conv2d([x], B, H, W, 3, 3, wd, bias, cout, 0, True, 1.0, out, None, None, None, ws), args.reps))
                wsn.append(timed(lambda: ops.conv2d_wino(x, B, H, W, ww, bias, cout, True, 1.0, out, 0), args.reps))
            t_d, t_w = statistics.median(ds), statistics.median(wsn)
            direct_gf = 2.0 * M * cout * 9 * cin / 1e9
            tiles = B * ((H + 1) // 2) * ((W + 1) // 2)
            wino_gf = 16 * 2.0 * tiles * cin * ((cout + 63) // 64 * 64) / 1e9
            print(f"B={B} pixels={M:6d} {key}: direct {t_d:8.1f} us ({direct_gf / t_d * 1e3:6.1f} TF/s)  "
                  f"wino {t_w:8.1f} us ({wino_gf / t_w * 1e3:6.1f} TF/s of its own {wino_gf:.1f} GFLOP, "
                  f"{direct_gf / t_w * 1e3:6.1f} effective)  speed-up {t_d / t_w:.2f}"
                  + (f"  [direct max - min {max(ds) - min(ds):.1f}, wino {max(wsn) - min(wsn):.1f}]" if args.rounds > 1 else ""), flush=True)


if __name__ == "__main__":
    main()
