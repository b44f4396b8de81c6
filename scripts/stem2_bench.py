"""The stem for one or two images (`pfk_conv_stem2_*`) against the 3-channel stem it stands beside (`pfk_conv_stem_f32`).

    python scripts/stem2_bench.py [--out stem2.json]

440 x 1024 frames, cout 64, fp32 rows out, N = 1, 2, 8, 16, 24 images.  Per N, alternating in one process, median of `--reps` timings
of 20 back-to-back launches each (device events): the 3-channel MFMA stem on N images (the kernel the 6-channel one is compared with,
scaled by K: 294 / 147 = 2), `pfk_conv_stem2` on N 3-channel images and on N 6-channel images.
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

H, W, LAUNCHES = 440, 1024, 20


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stem2_bench.py measures on the GPU; there is none")
    import ptlflow_amd
    ptlflow_amd.load_native()
    ops = torch.ops.pfk
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    w3 = (torch.randn(49, 3, 64, generator=g) / 12).to(dev)
    w6 = (torch.randn(49, 6, 64, generator=g) / 17).to(dev)
    bias = torch.zeros(64, device=dev)
    rows = []
    for N in (1, 2, 8, 16, 24):
        x = torch.rand(N, 6, H, W, generator=g).to(dev)
        x3 = x[:, :3].contiguous()
        out = torch.empty(N * (H // 2) * (W // 2), 64, device=dev)

        legs = {"stem3": lambda: ops.conv_stem(x3, w3, bias, out, True),
                "stem2_3ch": lambda: ops.conv_stem2(x3, None, w3, bias, out, True),
                "stem2_6ch": lambda: ops.conv_stem2(x[:, :3], x[:, 3:], w6, bias, out, True)}
        t = {k: [] for k in legs}
        for rep in range(args.reps + 1):                 # the first round is the warm-up
            for k, f in legs.items():
                us = _time(f)
                if rep:
                    t[k].append(us)
        row = {"images": N, **{k: round(statistics.median(v), 1) for k, v in t.items()}}
        row["6ch_over_2x_stem3"] = round(row["stem2_6ch"] / (2 * row["stem3"]), 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"frame": [H, W], "us_per_launch": rows}, f, indent=1)


if __name__ == "__main__":
    main()
