#!/usr/bin/env python3
"""The multi-scale GroupNorm encoders (`fnet` / `cnet` of CCMR, CCMR+ and MS-RAFT+) with `multiscale_encoders` off — the stock torch
module, which is the parent's behaviour — and on (the engine of ptlflow_amd/ms_encoder.py), on the torch stand-in
tests/msenc_model.py: the measurement behind DESIGN.md K15.

    python scripts/ms_encoder_bench.py [--out table.md]                     # every step below, each in a child process of its own
    python scripts/ms_encoder_bench.py --step encoder:msraft_cnet           # one step, in this process
    python scripts/ms_encoder_bench.py --step encoder:ccmr_fnet --images 2 --side engine --calls 10      # one side alone, for a kernel trace

Steps: `encoder:<key>` for the six encoders (a feature encoder on one 448 x 1024 pair and on 8 pairs, a context encoder on 1 and on
8 images), `kernels` (the three row kernels alone: bytes moved over time) and `ccmr` (where the reference is importable: whole-forward
`CCMR()` at 436 x 1024, batch 1, with accelerate(m), + ccmr_aggregator=True, + multiscale_encoders=True).  The driver runs each step
as a fresh child under its own time limit and stops at the first one that fails.  Per size the two sides alternate; each figure is the
median of `--rounds` timings between device events, with max - min in brackets.  Before timing, the two sides' outputs are compared
on the same input."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12        # bytes / s, MI355X (HBM3E)
STEP_LIMIT = 240         # seconds per child


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def med(ts):
    return f"{statistics.median(ts):9.1f} [{max(ts) - min(ts):7.1f}]"


def flat(outs):
    import torch
    return [torch.cat(list(o), 0) if isinstance(o, (tuple, list)) else o for o in outs]


def step_encoder(args, key):
    import torch
    from msenc_model import SEEDS, make, randomize
    from ptlflow_amd.ms_encoder import PfkMultiScaleEncoder, describe_multiscale_encoder
    stock = randomize(make(key), SEEDS[key]).cuda().eval()
    for p in stock.parameters():
        p.requires_grad_(False)
    wrapped = PfkMultiScaleEncoder(stock, describe_multiscale_encoder(stock), stock.split_pairs).eval()
    g = torch.Generator().manual_seed(7)
    for images in ((2, 16) if stock.split_pairs else (1, 8)):
        if args.images and images != args.images:
            continue
        x = torch.rand(images, 3, 448, 1024, generator=g).cuda()
        feed = [x[:images // 2], x[images // 2:]] if stock.split_pairs else x
        sides = {"stock": lambda: stock(feed), "engine": lambda: wrapped(feed)}
        with torch.no_grad():
            if args.side:
                for _ in range(2 + args.calls):
                    sides[args.side]()
                torch.cuda.synchronize()
                print(f"{key} x{images}: {args.calls} calls of side {args.side}", flush=True)
                continue
            want, got = flat(sides["stock"]()), flat(sides["engine"]())
            errs = []
            for a, b in zip(got, want):
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                assert err <= 5e-4 * scale, (key, images, err, scale)
                errs.append(err / scale)
            assert wrapped.engine_calls > 0 and wrapped.fallback_calls == 0
            for fn in sides.values():
                fn()
            t = {"stock": [], "engine": []}
            for _ in range(args.rounds):      # alternating, so that a drift of the clocks hits both alike
                for name, fn in sides.items():
                    t[name].append(timed(torch, fn, args.reps))
        ratio = statistics.median(t["engine"]) / statistics.median(t["stock"])
        print(f"| {key} | {images}x3x448x1024 | {med(t['stock'])} | {med(t['engine'])} | {ratio:.2f} | {max(errs):.1e} |", flush=True)


def step_kernels(args):
    """the three row kernels alone at the encoders' largest shapes: algorithmic bytes (every operand once) over time"""
    import torch
    import ptlflow_amd
    ptlflow_amd.load_native()
    ops = torch.ops.pfk
    for B, H, W, C in ((2, 224, 512, 64), (16, 224, 512, 64), (8, 224, 512, 256), (16, 112, 256, 96)):
        M = B * H * W
        x, res, out = (torch.randn(M, C, device="cuda") for _ in range(3))
        gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        scale, shift = torch.empty(B * C, device="cuda"), torch.empty(B * C, device="cuda")
        ws = torch.empty(ops.groupnorm_workspace_bytes(B, H * W, C), dtype=torch.uint8, device="cuda")
        small = torch.randn(B * (H // 2) * (W // 2), C, device="cuda")
        cases = {
            "groupnorm_stats": (lambda: ops.groupnorm_stats(x, B, H * W, 8, gamma, beta, 1e-5, scale, shift, ws), M * C * 4),
            "affine_apply": (lambda: ops.affine_apply(x, scale, shift, None, out, B, H * W, True, False), 2 * M * C * 4),
            "affine_apply + residual": (lambda: ops.affine_apply(x, scale, shift, res, out, B, H * W, True, True), 3 * M * C * 4),
            "resize 2x": (lambda: ops.resize_bilinear_pm(small, out, B, H // 2, W // 2, H, W), (M + M // 4) * C * 4),
        }
        for name, (fn, nbytes) in cases.items():
            for _ in range(3):
                fn()
            ts = [timed(torch, fn, 10) for _ in range(args.rounds)]
            bw = nbytes / (statistics.median(ts) * 1e-6)
            print(f"| {name} | {B}x{H}x{W}x{C} | {nbytes / 1e6:.1f} | {med(ts)} | {bw / 1e12:.2f} | {100 * bw / HBM_PEAK:.0f}% |", flush=True)


def step_ccmr(args):
    import torch
    from oracle import ref_loader
    if not ref_loader.reference_available():
        print("ccmr: no reference on this machine, step left out", flush=True)
        return
    from ptlflow_amd import patch
    M = ref_loader.ref_module("ptlflow.models.ccmr.ccmr")
    torch.manual_seed(1234)
    model = M.CCMR().eval()
    for p in model.parameters():
        p.requires_grad_(False)
    model.cuda()
    x = torch.rand(1, 2, 3, 436, 1024, generator=torch.Generator().manual_seed(3)).cuda()
    configs = (("accelerate(m)", {}), ("+ ccmr_aggregator=True", {"ccmr_aggregator": True}),
               ("+ multiscale_encoders=True", {"ccmr_aggregator": True, "multiscale_encoders": True}))
    fwd = lambda: model({"images": x})["flows"]  # noqa: E731
    first, times = None, {name: [] for name, _ in configs}
    with torch.no_grad():
        for name, kw in configs:      # outputs first: every configuration against plain accelerate
            patch.accelerate(model, **kw)
            out = fwd().float()
            first = out if first is None else first
            err = float((out - first).norm(dim=2).mean())
            print(f"ccmr {name}: mean EPE to accelerate(m) {err:.2e}", flush=True)
            assert bool(torch.isfinite(out).all()), name
        for _ in range(args.rounds):
            for name, kw in configs:
                patch.accelerate(model, **kw)
                fwd()
                times[name].append(timed(torch, fwd, 1))
    base = statistics.median(times[configs[0][0]])
    for name, _ in configs:
        m = statistics.median(times[name])
        print(f"| CCMR 436x1024 b1 | {name} | {m / 1e3:8.1f} [{(max(times[name]) - min(times[name])) / 1e3:6.1f}] | {1e6 / m:.2f} | {m / base:.3f} |",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, help="encoder:<key> | kernels | ccmr (default: all, each in a child process)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--side", choices=["stock", "engine"], default=None, help="run --calls calls of one side only (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--images", type=int, default=0, help="an encoder step at this batch only (0: both sizes)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        kind, _, key = args.step.partition(":")
        {"encoder": lambda: step_encoder(args, key), "kernels": lambda: step_kernels(args), "ccmr": lambda: step_ccmr(args)}[kind]()
        return
    from msenc_model import ENCODERS
    lines = []
    for step in [f"encoder:{k}" for k in ENCODERS] + ["kernels", "ccmr"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--rounds", str(args.rounds)]
        try:
            r = subprocess.run(cmd, timeout=STEP_LIMIT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {STEP_LIMIT} s; nothing more is started", flush=True)
            sys.exit(124)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            print(r.stderr[-3000:], flush=True)
            print(f"{step}: exit status {r.returncode}; nothing more is started", flush=True)
            sys.exit(r.returncode if r.returncode > 0 else 1)
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("|")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
