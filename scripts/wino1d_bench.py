#!/usr/bin/env python3
"""In-isolation timing of the SepConvGRU's four per-iteration gate launches (z|r and q, 1x5 and 5x1, context term hoisted) on the
direct implicit-GEMM kernel (`pfk_conv2d_f32` with the engine's stream-K workspace) and on the 1-D Winograd F(4,5) kernel
(`pfk_conv1d_wino_f32`), raft and gma widths: the measurement behind update.py's WINO1D_MIN_PIXELS.

    python scripts/wino1d_bench.py [--grids 1x55x128 2x55x128 4x55x128 8x55x128 8x47x156] [--reps 40] [--rounds 3]

Each figure is the median of `--rounds` timings of `--reps` launches; `spread` is max - min of the direct kernel's rounds.
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import ptlflow_amd  # noqa: E402
from ptlflow_amd.packing import pack_conv_weight, pack_wino1d_weight  # noqa: E402

EPI_GRU_ZR, EPI_GRU_Q = 1, 2
WIDTHS = {"raft": 128, "gma": 256}      # channels behind the context slice (motion features [| aggregated ones] | pad)
CH, CI = 128, 128


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
    ap.add_argument("--grids", nargs="+", default=["1x55x128", "2x55x128", "4x55x128", "8x55x128", "8x47x156"])
    ap.add_argument("--models", nargs="+", default=list(WIDTHS))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    ptlflow_amd.load_native()
    ops = torch.ops.pfk
    ws = torch.zeros(ops.conv_workspace_bytes(), device="cuda", dtype=torch.uint8)
    for grid in args.grids:
        B, H, W = map(int, grid.split("x"))
        M = B * H * W
        for model in args.models:
            rest = WIDTHS[model]
            K = CH + rest
            act = torch.randn(M, CH + CI + rest, device="cuda")
            act[:, :CH].tanh_()
            h0 = act[:, :CH].clone()
            z, rh = torch.rand(M, CH, device="cuda"), torch.randn(M, CH, device="cuda")
            segs = [(0, CH, CH), (CH + CI, rest, rest)]
            for kh, kw in ((1, 5), (5, 1)):
                for name, epi, cout in (("zr", EPI_GRU_ZR, 2 * CH), ("q", EPI_GRU_Q, CH)):
                    g = torch.Generator().manual_seed(0)
                    wt = torch.randn(cout, CH + CI + rest, kh, kw, generator=g) / math.sqrt(5 * K)
                    ctx = torch.randn(M, cout, device="cuda") * 0.5
                    wd, ww = pack_conv_weight(wt, segs).cuda(), pack_wino1d_weight(wt, segs).cuda()
                    srcs = [act[:, :CH] if epi == EPI_GRU_ZR else rh, act[:, CH + CI:]]
                    # z|r writes r*h, which q reads: the z|r timing gets a buffer of its own
                    aux_rh = torch.empty(M, CH, device="cuda") if epi == EPI_GRU_ZR else None
                    direct = lambda: ops.conv2d(srcs, B, H, W, kh, kw, wd, None, cout, epi, False, 1.0, None, act[:, :CH], z, aux_rh,  # noqa: E731
                                                ws, ctx)
                    wino = lambda: ops.conv2d_wino1d(srcs, B, H, W, kh, kw, ww, None, cout, epi, False, 1.0, None, act[:, :CH], z,  # noqa: E731
                                                     aux_rh, ctx)
                    td, tw = [], []
                    for _ in range(args.rounds):      # alternating, so that a drift of the clocks hits both alike
                        td.append(timed(direct, args.reps))
                        act[:, :CH].copy_(h0)         # q blends into h: keep it from drifting to its fixed point
                        tw.append(timed(wino, args.reps))
                        act[:, :CH].copy_(h0)
                    t_d, t_w = statistics.median(td), statistics.median(tw)
                    direct_gf = 2.0 * M * cout * 5 * K / 1e9
                    L, lines = (H, B * W) if kh == 5 else (W, B * H)
                    tiles = lines * ((L + 3) // 4)
                    wino_gf = 8 * 2.0 * tiles * K * ((cout + 127) // 128 * 128) / 1e9
                    blocks = (tiles + 31) // 32 * ((cout + 127) // 128)
                    print(f"{grid} pixels={M:6d} {model:4s} {name:2s} {kh}x{kw}: direct {t_d:7.1f} us (spread {max(td) - min(td):4.1f}, "
                          f"{direct_gf / t_d * 1e3:5.1f} TF/s)  wino1d {t_w:7.1f} us (spread {max(tw) - min(tw):4.1f}, {blocks:4d} blocks, "
                          f"{wino_gf / t_w * 1e3:5.1f} TF/s of its own {wino_gf:.1f} GFLOP)  speed-up {t_d / t_w:.2f}", flush=True)


if __name__ == "__main__":
    main()
