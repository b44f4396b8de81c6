#!/usr/bin/env python3
"""`accelerate(model, ccmr_context=True)` — CCMR's per-scale context grouping `model.xcit[i]` on the kernels: the measurement behind
DESIGN.md K17.  Every "off" side is the parent's behaviour (the module in torch, the launches K14's `prepare` makes, `fold_attention`),
never the code under test.

    python scripts/ccmr_context_bench.py [--out table.md]                  # every step below, each in a child process of its own
    python scripts/ccmr_context_bench.py --step module                     # one step, in this process
    python scripts/ccmr_context_bench.py --step forward --config 1 --calls 3      # one configuration alone, for a kernel trace

Steps:
  module      `XCiT(128, depth 1, 8 heads, mlp_ratio 1, separate=False)` in torch (the reference's class where importable, else the
              stand-in tests/xcit_model.py) against `PfkXcitContext` on the same tensor, at 28x64, 56x128, 112x256 (batch 1 and 8) and
              224x512 (batch 1)
  tokens      `pfk_xcit_tokens_f32` against the four launches it replaces (`nchw_to_pm`, `+= pos`, `layernorm_rows` with and without
              affine) on the same tensors, same grids
  fold        `pfk_xca_fold_f32` against `xcit.fold_attention` on the GPU, batch 1 and 8
  forward     the reference's `CCMR()` forward at 436 x 1024, batch 1, where it is importable (otherwise the stand-in loop of
              tests/ms_loop_model.py with `XCiT` context modules, at 448 x 1024): ccmr_aggregator + multiscale_encoders +
              multiscale_upsample, against the same three + ccmr_context
The driver runs each step as a fresh child under its own time limit and stops at the first one that fails.  The sides of a step
alternate; each figure is the median of `--rounds` timings between device events, with max - min in brackets."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_LIMIT = 240         # seconds per child
GRIDS = ((1, 28, 64), (1, 56, 128), (1, 112, 256), (1, 224, 512), (8, 28, 64), (8, 56, 128), (8, 112, 256))
STEPS = ("module", "tokens", "fold", "forward")
BASE = {"ccmr_aggregator": True, "multiscale_encoders": True, "multiscale_upsample": True}


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


def alternate(torch, sides, rounds, reps):
    for fn in sides.values():
        for _ in range(2):
            fn()
    t = {name: [] for name in sides}
    for _ in range(rounds):      # alternating, so that a drift of the clocks hits every side alike
        for name, fn in sides.items():
            t[name].append(timed(torch, fn, reps))
    return t


def context_class():
    """(the XCiT class, where it comes from)"""
    from oracle import ref_loader
    if ref_loader.reference_available() and ref_loader.ensure_family("ccmr"):
        return ref_loader.ref_module("ptlflow.models.ccmr.xcit").XCiT, "reference"
    from xcit_model import XCiT
    return XCiT, "stand-in"


def make_module(torch):
    from xcit_model import randomize
    cls, origin = context_class()
    m = randomize(cls(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=False), 61).cuda().eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m, origin


def step_module(args):
    import torch
    import ptlflow_amd
    from ptlflow_amd.xcit import PfkXcitContext, match_xcit_context
    ptlflow_amd.load_native()
    ref, origin = make_module(torch)
    assert match_xcit_context(ref)
    wrap = PfkXcitContext(ref).eval()
    print(f"module: the torch side is the {origin}'s XCiT(separate=False)", flush=True)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for B, H, W in GRIDS:
            x = torch.relu(torch.randn(B, 128, H, W, generator=g)).cuda()
            sides = {"torch": lambda: ref(x), "wrapper": lambda: wrap(x)}
            want, got = sides["torch"](), sides["wrapper"]()
            err, scale = float((got - want).abs().max()), float(want.abs().max())
            assert err <= 5e-4 * scale and wrap.fallback_calls == 0, (B, H, W, err, scale)
            t = alternate(torch, sides, args.rounds, args.reps)
            ratio = statistics.median(t["torch"]) / statistics.median(t["wrapper"])
            print(f"| module | {B}x{H}x{W} | {med(t['torch'])} | {med(t['wrapper'])} | {ratio:.2f} | {err / scale:.1e} |", flush=True)


def step_tokens(args):
    import torch
    import ptlflow_amd
    ptlflow_amd.load_native()
    ops = torch.ops.pfk
    g = torch.Generator().manual_seed(4)
    lw, lb = (torch.rand(128, generator=g) + 0.5).cuda(), (torch.rand(128, generator=g) - 0.5).cuda()
    with torch.no_grad():
        for B, H, W in GRIDS:
            M = B * H * W
            x = torch.relu(torch.randn(B, 128, H, W, generator=g)).cuda()
            pos = torch.randn(H * W, 128, generator=g).cuda()
            pos_b = pos.repeat(B, 1)                        # the B-copy form K14's `prepare` adds
            a0, at, ah, k0, kh = (torch.zeros(M, 128, device="cuda") for _ in range(5))

            def four():
                ops.nchw_to_pm(x, a0)
                a0.add_(pos_b)
                ops.layernorm_rows(a0, lw, lb, 1e-6, at)
                ops.layernorm_rows(a0, None, None, 1e-6, ah)

            def one():
                ops.xcit_tokens(x, pos, 1e-6, k0, kh)

            four()
            one()
            assert torch.equal(a0, k0), (B, H, W)
            err = float((ah - kh).abs().max())
            assert err <= 1e-5, (B, H, W, err)
            t = alternate(torch, {"four launches": four, "kernel": one}, args.rounds, max(args.reps, 20))
            ratio = statistics.median(t["four launches"]) / statistics.median(t["kernel"])
            # the kernel's own traffic: one read of the input, two row writes (and pos, which stays in cache at batch 8)
            gbs = 3 * M * 128 * 4 / statistics.median(t["kernel"]) / 1e3
            print(f"| tokens | {B}x{H}x{W} | {med(t['four launches'])} | {med(t['kernel'])} | {ratio:.2f} | {gbs:.0f} GB/s |", flush=True)


def step_fold(args):
    import torch
    import ptlflow_amd
    from ptlflow_amd.xcit import XcitContextEngine, fold_attention, split_qkv
    ptlflow_amd.load_native()
    ref, _ = make_module(torch)
    eng = XcitContextEngine(ref, torch.device("cuda"))
    P = split_qkv(eng.P)
    w = eng.w
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for B in (1, 8):
            A = torch.softmax(torch.randn(B, 8, 16, 16, generator=g) * 2, -1).cuda()
            M, c = torch.zeros(B, 128, 128, device="cuda"), torch.zeros(B, 128, device="cuda")
            sides = {"fold_attention": lambda: fold_attention(A, P),
                     "kernel": lambda: torch.ops.pfk.xca_fold(A, w["v.w"], w["v.b"], w["proj.w"], w["proj.b"], M, c)}
            Mt, ct = sides["fold_attention"]()
            sides["kernel"]()
            err = max(float((M - Mt).abs().max() / Mt.abs().max()), float((c - ct).abs().max() / ct.abs().max()))
            assert err <= 1e-5, (B, err)
            t = alternate(torch, sides, args.rounds, max(args.reps, 20))
            ratio = statistics.median(t["fold_attention"]) / statistics.median(t["kernel"])
            print(f"| fold | B={B} | {med(t['fold_attention'])} | {med(t['kernel'])} | {ratio:.2f} | {err:.1e} |", flush=True)


def forward_model():
    """(model, images, where the model comes from)"""
    import torch
    from oracle import ref_loader
    g = torch.Generator().manual_seed(3)
    if ref_loader.reference_available():
        torch.manual_seed(1234)
        return ref_loader.ref_module("ptlflow.models.ccmr.ccmr").CCMR().eval(), torch.rand(1, 2, 3, 436, 1024, generator=g), "reference"
    import xcit_model
    from ccmr_context_refs import context_loop_model
    xcit_model.register()
    return context_loop_model((8, 10, 15), aggregators=True), torch.rand(1, 2, 3, 448, 1024, generator=g), "stand-in"


def step_forward(args):
    import torch
    from ptlflow_amd import patch
    from ptlflow_amd.xcit import PfkXcitContext
    model, x, origin = forward_model()
    for p in model.parameters():
        p.requires_grad_(False)
    model.cuda()
    x = x.cuda()
    configs = (("three options", dict(BASE)), ("+ ccmr_context", dict(BASE, ccmr_context=True)))
    fwd = lambda: model({"images": x})["flows"]  # noqa: E731
    with torch.no_grad():
        if args.config is not None:
            name, kw = configs[args.config]
            patch.accelerate(model, **kw)
            for _ in range(1 + args.calls):
                fwd()
            torch.cuda.synchronize()
            print(f"ccmr ({origin}) {name}: {args.calls} forwards", flush=True)
            return
        outs, times = {}, {name: [] for name, _ in configs}
        for name, kw in configs:      # outputs first
            patch.accelerate(model, **kw)
            outs[name] = fwd().float().clone()
            assert bool(torch.isfinite(outs[name]).all()), name
        names = [n for n, _ in configs]
        served = [(m.engine_calls, m.fallback_calls) for m in model.xcit if isinstance(m, PfkXcitContext)]
        again = fwd().float()
        epe = float((outs[names[1]] - outs[names[0]]).norm(dim=2).mean())
        print(f"ccmr ({origin}): option on against off mean EPE {epe:.2e} px of mean |flow| {float(outs[names[0]].norm(dim=2).mean()):.2e}; "
              f"wrappers (engine, fallback) calls {served}; two option-on forwards bit-identical: {bool(torch.equal(again, outs[names[1]]))}",
              flush=True)
        assert served and all(e >= 1 and f == 0 for e, f in served), served
        for _ in range(args.rounds):
            for name, kw in configs:
                patch.accelerate(model, **kw)
                fwd()
                times[name].append(timed(torch, fwd, 1))
    t0 = statistics.median(times[names[0]])
    for name in names:
        m = statistics.median(times[name])
        print(f"| ccmr ({origin}) {x.shape[3]}x{x.shape[4]} b1 | {name} | {m / 1e3:8.2f} [{(max(times[name]) - min(times[name])) / 1e3:6.2f}] | "
              f"{1e6 / m:.2f} | {m / t0:.3f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=STEPS, help="default: all, each in a child process")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--config", type=int, choices=[0, 1], default=None, help="the forward step: run --calls forwards of one configuration only")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        {"module": step_module, "tokens": step_tokens, "fold": step_fold, "forward": step_forward}[args.step](args)
        return
    lines = []
    for step in STEPS:
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
