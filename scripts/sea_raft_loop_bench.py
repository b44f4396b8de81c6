"""SEA-RAFT refinement loop: stock PyTorch-ROCm against `accelerate(model, sea_raft_update=True)` (ptlflow_amd/sea_update.py).

    python scripts/sea_raft_loop_bench.py [--out sea_loop.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python scripts/sea_raft_loop_bench.py --trace   # kernel times
    python scripts/sea_raft_loop_bench.py --precision bf16 [--out sea_loop_bf16.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python scripts/sea_raft_loop_bench.py --precision bf16 --trace

Times the loop body of sea_raft.py:217-236 without the lookup — update block, flow_head, 0.25 * upsample_weight, the flow update
and upsample_data — on a 55 x 128 grid (436 x 1024 frames) with a fixed correlation input, at B = 1 and 8 and 4 and 12 iterations.
Device events, warm-up, stock and accelerated runs alternating in one process; reported: ms per iteration (median of the runs).
The accelerated runs also time the engine's GEMM launches with events (`UpdateEngine.profile`): pwconv1 / pwconv2 / final as
shares of the fp32 MFMA peak.  dwconv + LayerNorm's time comes from the separate `--trace` run (kernel `dwconv_ln_kernel`), its
share of the HBM roof is computed from it by hand (2 x M x 384 x 4 bytes per launch).

`--precision bf16` times three loops, alternating in one process: the stock loop under torch.autocast("cuda", bfloat16),
`accelerate(model, sea_raft_update="bf16")` run as that same autocast loop, and the fp32 kernel loop (`sea_raft_update=True`);
`--trace` then runs the bf16 kernel loop only (kernel `dwconv_ln_b16_kernel`: 2 x M x 384 x 2 bytes per launch).
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

PEAK_FP32_MFMA = 157.3e12
H8, W8 = 55, 128


def _inputs(B, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(B, 128, H8, W8, generator=g)).to(dev)
    ctx = torch.relu(torch.randn(B, 128, H8, W8, generator=g)).to(dev)
    corr = torch.randn(B, 324, H8, W8, generator=g).to(dev)
    flow = torch.randn(B, 2, H8, W8, generator=g).to(dev)
    return net, ctx, corr, flow


def _loop(model, net, ctx, corr, flow, iters):
    for _ in range(iters):
        net = model.update_block(net, ctx, corr, flow)
        fu = model.flow_head(net)
        wu = 0.25 * model.upsample_weight(net)
        flow = flow + fu[:, :2]
        up = model.upsample_data(flow, fu[:, 2:], wu)
    return up


def _time(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="accelerated loop only, B = 1 and 8, 12 iterations (for rocprofv3)")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32",
                    help="bf16: stock autocast loop vs the bf16 kernel loop vs the fp32 kernel loop")
    args = ap.parse_args()
    if args.precision == "bf16":
        return main_bf16(args)
    import ptlflow_amd
    from ptlflow_amd import patch
    from sea_seam_model import SeaRaftLoop, load_seeded
    ptlflow_amd.load_native()
    dev = torch.device("cuda:0")
    stock = load_seeded(SeaRaftLoop(), 11).eval().to(dev)
    fast = load_seeded(SeaRaftLoop(), 11).eval().to(dev)
    patch.accelerate(fast, sea_raft_update=True)
    res = {"grid": [H8, W8], "peak_fp32_mfma_tflops": PEAK_FP32_MFMA / 1e12, "runs": []}
    with torch.no_grad():
        for B in (1, 8):
            net, ctx, corr, flow = _inputs(B, dev)
            corr_cl = corr.contiguous(memory_format=torch.channels_last)    # the channel view the B1 hook hands out
            for iters in (4, 12):
                if args.trace:
                    _loop(fast, net, ctx, corr_cl, flow, iters)
                    torch.cuda.synchronize()
                    continue
                run_s = lambda: _loop(stock, net, ctx, corr, flow, iters)       # noqa: E731
                run_f = lambda: _loop(fast, net, ctx, corr_cl, flow, iters)     # noqa: E731
                for f in (run_s, run_f, run_s, run_f):                          # warm-up (MIOpen find, packing, probes)
                    f()
                torch.cuda.synchronize()
                ts, tf = [], []
                for _ in range(args.reps):                                      # alternating
                    ts += _time(run_s, 1)
                    tf += _time(run_f, 1)
                ms_s, ms_f = statistics.median(ts) / iters, statistics.median(tf) / iters
                row = {"B": B, "iters": iters, "stock_ms_per_iter": round(ms_s, 4), "pfk_ms_per_iter": round(ms_f, 4),
                       "speedup": round(ms_s / ms_f, 3)}
                if iters == 12:
                    eng = fast.update_block._engine
                    eng.profile = {}
                    run_f()
                    torch.cuda.synchronize()
                    per = {}
                    for key, evs in eng.profile.items():
                        ms = sum(a.elapsed_time(b) for a, b in evs) / len(evs)
                        fl = eng.flops.get(key, 0.0)
                        per[key] = {"us": round(ms * 1e3, 2), "mfma_share": round(fl / (ms * 1e-3) / PEAK_FP32_MFMA, 3) if fl else None}
                    eng.profile = None
                    row["launches"] = per
                res["runs"].append(row)
                print(json.dumps(row), flush=True)
    if args.out and not args.trace:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def main_bf16(args) -> None:
    import ptlflow_amd
    from ptlflow_amd import patch
    from sea_seam_model import SeaRaftLoop, load_seeded
    ptlflow_amd.load_native()
    dev = torch.device("cuda:0")
    stock = load_seeded(SeaRaftLoop(), 11).eval().to(dev)
    k16 = load_seeded(SeaRaftLoop(), 11).eval().to(dev)
    k32 = load_seeded(SeaRaftLoop(), 11).eval().to(dev)
    patch.accelerate(k16, sea_raft_update="bf16")
    patch.accelerate(k32, sea_raft_update=True)
    res = {"grid": [H8, W8], "precision": "bf16", "runs": []}

    def autocast_loop(model, *a):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return _loop(model, *a)

    with torch.no_grad():
        for B in (1, 8):
            net, ctx, corr, flow = _inputs(B, dev)
            corr_cl = corr.contiguous(memory_format=torch.channels_last)    # the channel view the B1 hook hands out
            for iters in (4, 12):
                run_16 = lambda: autocast_loop(k16, net, ctx, corr_cl, flow, iters)       # noqa: E731
                if args.trace:
                    run_16()
                    torch.cuda.synchronize()
                    continue
                run_s = lambda: autocast_loop(stock, net, ctx, corr, flow, iters)        # noqa: E731
                run_32 = lambda: _loop(k32, net, ctx, corr_cl, flow, iters)             # noqa: E731
                for f in (run_s, run_16, run_32) * 2:                                   # warm-up (MIOpen find, packing, probes)
                    f()
                torch.cuda.synchronize()
                c0 = k16.update_block.calls
                ts, t16, t32 = [], [], []
                for _ in range(args.reps):                                              # alternating
                    ts += _time(run_s, 1)
                    t16 += _time(run_16, 1)
                    t32 += _time(run_32, 1)
                assert k16.update_block.calls - c0 == args.reps * iters, "the bf16 loop left the kernels"
                ms_s, ms_16, ms_32 = (statistics.median(t) / iters for t in (ts, t16, t32))
                row = {"B": B, "iters": iters, "stock_autocast_ms_per_iter": round(ms_s, 4), "pfk_bf16_ms_per_iter": round(ms_16, 4),
                       "pfk_fp32_ms_per_iter": round(ms_32, 4), "speedup_vs_stock_autocast": round(ms_s / ms_16, 3),
                       "speedup_vs_pfk_fp32": round(ms_32 / ms_16, 3)}
                res["runs"].append(row)
                print(json.dumps(row), flush=True)
    if args.out and not args.trace:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
