"""One convolution of the fp32 feature encoder with the instance norms around it: separate passes against the fused launch.

    python scripts/enc_norm_fusion_bench.py [--rounds 3] [--out fusion.json]

Shapes: cin = cout = 64 at 220 x 512, 96 at 110 x 256, 128 at 55 x 128, 16 and 2 images.  Two legs per shape, both from a raw input
with its statistics to a raw output with its statistics (what a block's conv2 is handed and hands on):
  separate  `norm_apply` (the norm in front, in place on a copy's buffer) + `conv2d_wino` + `instnorm_stats` (the norm behind)
  fused     `conv2d_wino_stats` with the input's statistics: normalise on load, sums in the epilogue, `chunk_reduce`
`stats_only` is `conv2d_wino_stats` without input statistics against `conv2d_wino` + `instnorm_stats` (a block's conv1 behind a
normalised input).  The legs alternate in one process; a round is the median of `--reps` timings of 10 back-to-back repetitions
(device events); reported: the median of the rounds and their spread (max - min).
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
SHAPES = ((64, 220, 512), (96, 110, 256), (128, 55, 128))
EPS = 1e-5


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES * 1e3        # us per repetition


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("enc_norm_fusion_bench.py measures on the GPU; there is none")
    import ptlflow_amd
    from ptlflow_amd.packing import pack_wino_weight
    ptlflow_amd.load_native()
    ops = torch.ops.pfk
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for C, H, W in SHAPES:
        ww = pack_wino_weight(torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(dev)
        bias = torch.randn(C, generator=g).to(dev)
        for N in (16, 2):
            M, HW = N * H * W, H * W
            x = (torch.randn(M, C, generator=g) + 0.5).to(dev)
            xn, out = torch.empty_like(x), torch.empty(M, C, device=dev)
            im, ir, om, orr = (torch.empty(N * C, device=dev) for _ in range(4))
            ws = torch.empty(max(ops.instnorm_workspace_bytes(N, C), ops.conv_wino_stats_workspace_bytes(N, H, W, C)), device=dev,
                             dtype=torch.uint8)
            ops.instnorm_stats(x, N, HW, EPS, im, ir, ws)

            def separate():
                ops.norm_apply(x, im, ir, None, xn, N, HW, True, False)
                ops.conv2d_wino(xn, N, H, W, ww, bias, C, False, 1.0, out, 0)
                ops.instnorm_stats(out, N, HW, EPS, om, orr, ws)

            def separate_stats():
                ops.conv2d_wino(xn, N, H, W, ww, bias, C, False, 1.0, out, 0)
                ops.instnorm_stats(out, N, HW, EPS, om, orr, ws)

            legs = {
                "separate": separate,
                "fused": lambda: ops.conv2d_wino_stats(x, N, H, W, ww, bias, C, out, im, ir, True, EPS, om, orr, ws),
                "stats_only_separate": separate_stats,
                "stats_only_fused": lambda: ops.conv2d_wino_stats(xn, N, H, W, ww, bias, C, out, None, None, False, EPS, om, orr, ws),
                "plain": lambda: ops.conv2d_wino(xn, N, H, W, ww, bias, C, False, 1.0, out, 0),
                "norm_only": lambda: ops.conv2d_wino_norm(x, N, H, W, ww, bias, C, False, 1.0, out, im, ir, True),
            }
            rounds = {k: [] for k in legs}
            for rnd in range(args.rounds + 1):               # the first round is the warm-up
                t = {k: [] for k in legs}
                for _ in range(args.reps):
                    for k, f in legs.items():
                        t[k].append(_time(f))
                if rnd:
                    for k in legs:
                        rounds[k].append(statistics.median(t[k]))
            row = {"C": C, "H": H, "W": W, "images": N}
            for k, v in rounds.items():
                row[k] = round(statistics.median(v), 1)
                row[k + "_spread"] = round(max(v) - min(v), 1)
            row["fused_saves_us"] = round(row["separate"] - row["fused"], 1)
            row["stats_only_saves_us"] = round(row["stats_only_separate"] - row["stats_only_fused"], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"us": rows}, f, indent=1)


if __name__ == "__main__":
    main()
