#!/usr/bin/env python3
"""Micro-benchmark of the bf16 weight gradient (K12b, torch.ops.pfk.conv_wgrad_unpacked_b16) against the fp32 one
(K12, conv_wgrad_unpacked) on the update-block layers of BASELINE config 5 (batch 10, 46x62 grid) — GPU box.
    python scripts/wgrad_b16_bench.py [--samples 9] [--reps 10] [--splits 0]
Device events, the two legs alternating in one process; per layer the median of `--samples` samples (each `--reps` launches) in
us per launch, with the min-max spread.  `--splits n` forces n pixel slices in the bf16 kernel (pfk_debug_set_wgrad_b16)."""
import argparse
import os
os.environ.setdefault("PFK_DEBUG_KNOBS", "1")   # tuning script: uses the pfk_debug_set_* knobs
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptlflow_amd  # noqa: E402

ptlflow_amd.load_native()
ops = torch.ops.pfk

UB = (10, 46, 62)
# name, real channels per source, cout (real), kh, kw — the training step's launches (context term hoisted: the GRU nodes see h and
# the motion features; the context part is one launch per step, "zrc" / "qc")
LAYERS = [
    ("convc1", [324], 256, 1, 1), ("convc2", [256], 192, 3, 3), ("convf2", [128], 64, 3, 3), ("conv", [192, 64], 126, 3, 3),
    ("zr 1x5", [128, 128], 256, 1, 5), ("q 1x5", [128, 128], 128, 1, 5), ("zr 5x1", [128, 128], 256, 5, 1), ("q 5x1", [128, 128], 128, 5, 1),
    ("zrc 1x5", [128], 256, 1, 5), ("qc 1x5", [128], 128, 1, 5),
    ("fh.conv1", [128], 256, 3, 3), ("fh.conv2", [256], 2, 3, 3), ("mask.0", [128], 256, 3, 3), ("mask.2", [256], 576, 1, 1),
]


def up(x, m):
    return (x + m - 1) // m * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--splits", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    B, H, W = UB
    M = B * H * W
    ops.debug_set_wgrad_b16(args.splits)
    tot = {"fp32": 0.0, "bf16": 0.0}
    print(f"{'layer':9s} {'GFLOP':>6s} | {'fp32 us (min-max)':>26s} | {'bf16 us (min-max)':>26s} | speed-up | bf16 TFLOP/s | max |diff|/scale")
    for name, reals, cout, kh, kw in LAYERS:
        x32 = [torch.randn(M, up(c, 4), device=dev) for c in reals]
        x16 = [torch.randn(M, up(c, 8), device=dev).bfloat16() for c in reals]
        for a, b, c in zip(x32, x16, reals):
            a[:, :c] = b[:, :c].float()
        dy16 = torch.randn(M, up(cout, 8), device=dev).bfloat16()
        dy32 = dy16[:, :up(cout, 4)].float().contiguous()
        dw = {k: torch.empty(cout, sum(reals), kh, kw, device=dev) for k in tot}
        db = {k: torch.empty(cout, device=dev) for k in tot}
        legs = {
            "fp32": lambda: ops.conv_wgrad_unpacked(x32, dy32, B, H, W, kh, kw, dw["fp32"], db["fp32"], reals, 1, False),
            "bf16": lambda: ops.conv_wgrad_unpacked_b16(x16, dy16, B, H, W, kh, kw, dw["bf16"], db["bf16"], reals, False),
        }
        for f in legs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        diff = float((dw["bf16"] - dw["fp32"]).abs().max()) / float(dw["fp32"].abs().max())     # same bf16-exact operands in both legs
        t = {k: [] for k in legs}
        for _ in range(args.samples):
            for k, f in legs.items():         # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                t[k].append(1e3 * e0.elapsed_time(e1) / args.reps)
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in tot:
            tot[k] += med[k]
        gf = 2.0 * M * cout * kh * kw * sum(reals) / 1e9
        print(f"{name:9s} {gf:6.1f} | {med['fp32']:8.1f} ({min(t['fp32']):7.1f}-{max(t['fp32']):7.1f}) | "
              f"{med['bf16']:8.1f} ({min(t['bf16']):7.1f}-{max(t['bf16']):7.1f}) | {med['fp32'] / med['bf16']:7.2f}x | "
              f"{gf / med['bf16'] * 1e3:10.1f} | {diff:.1e}", flush=True)
    ops.debug_set_wgrad_b16(0)
    print(f"sum of medians: fp32 {tot['fp32']:.1f} us, bf16 {tot['bf16']:.1f} us ({tot['fp32'] / tot['bf16']:.2f}x)")


if __name__ == "__main__":
    main()
