#!/usr/bin/env python3
"""`accelerate(model, multiscale_upsample=True)` — the x2 convex-upsampling kernel and the per-scale dead-work skip of the multi-scale
families (CCMR, CCMR+, MS-RAFT+): the measurement behind DESIGN.md K16.

    python scripts/ms_upsample_bench.py [--out table.md]                  # every step below, each in a child process of its own
    python scripts/ms_upsample_bench.py --step kernel                     # one step, in this process
    python scripts/ms_upsample_bench.py --step forward:ccmr --config 2 --calls 3      # one configuration alone, for a kernel trace

Steps:
  kernel                 `pfk_convex_upsample2_f32` (through seam B5's `_kernel2`) against the torch method (the reference's `CCMR.upsample_flow` where importable) on the same tensors, at
                         28x64, 56x128, 112x256 and 224x512, batch 1 and 8
  block:<family>         one update-block call of `ccmr_spec` / `ms_raft_plus_spec` with and without the mask half (fh|mask conv1's mask
                         columns and mask conv2) at the same grids, batch 1
  forward:<family>       whole forwards at 436 x 1024, batch 1: the existing options on; + multiscale_upsample=True with
                         skip_dead_upsample=False; + the skip.  The reference's `CCMR()` / `MSRAFTPlus()` where it is importable,
                         otherwise the stand-in loop of tests/ms_loop_model.py with the same `iters` (at 448 x 1024: it does no padding)
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
GRIDS = ((28, 64), (56, 128), (112, 256), (224, 512))
FAMILIES = ("ccmr", "ms_raft_plus")


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
        fn()
    t = {name: [] for name in sides}
    for _ in range(rounds):      # alternating, so that a drift of the clocks hits every side alike
        for name, fn in sides.items():
            t[name].append(timed(torch, fn, reps))
    return t


def step_kernel(args):
    import torch
    import ptlflow_amd
    from ms_loop_model import MsLoopModel
    from ptlflow_amd.patch import _UpsampleSeam
    ptlflow_amd.load_native()
    from oracle import ref_loader
    if ref_loader.reference_available():      # the method reads nothing of `self`
        method, origin = ref_loader.ref_module("ptlflow.models.ccmr.ccmr").CCMR.upsample_flow, "reference"
    else:
        method, origin = MsLoopModel.upsample_flow, "stand-in"
    print(f"upsample x2: the torch side is the {origin}'s method", flush=True)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for B in (1, 8):
            for H, W in GRIDS:
                flow = (torch.randn(B, 2, H, W, generator=g) * 3).cuda()
                # the update block's mask view: pixel-major rows seen as NCHW
                mask = torch.randn(B, H, W, 36, generator=g).cuda().permute(0, 3, 1, 2)
                sides = {"torch": lambda: method(None, flow, mask, scale=2),
                         "kernel": lambda: _UpsampleSeam._kernel2(flow, mask)}
                want, got = sides["torch"](), sides["kernel"]()
                err = float((got - want).abs().max())
                assert err <= 1e-5 * max(1.0, float(want.abs().max())), (B, H, W, err)
                t = alternate(torch, sides, args.rounds, args.reps)
                ratio = statistics.median(t["torch"]) / statistics.median(t["kernel"])
                print(f"| upsample x2 | {B}x{H}x{W} | {med(t['torch'])} | {med(t['kernel'])} | {ratio:.2f} | {err:.1e} |", flush=True)


class _MaskSwitch:
    """stands where `PfkUpdateBlock` looks for the dead-work schedule: every call's mask half on (`dead` False) or off"""
    dead = False

    def begin_forward(self, **kw):
        pass

    def next_call(self):
        return self.dead

    def may_defer(self):
        return False


def step_block(args, family):
    import torch
    import ptlflow_amd
    from ms_loop_model import CORR_CHANNELS, CcmrUpdateBlock, MsUpdateBlock
    from ptlflow_amd.patch import match_update_block
    from ptlflow_amd.update import PfkUpdateBlock
    ptlflow_amd.load_native()
    torch.manual_seed(5)
    ref = (CcmrUpdateBlock(4) if family == "ccmr" else MsUpdateBlock()).cuda().eval()
    for p in ref.parameters():
        p.requires_grad_(False)
    spec = match_update_block(ref)
    assert spec is not None and spec.mask_channels == 36
    ub = PfkUpdateBlock(ref, spec).eval()
    switch = ub._skip = _MaskSwitch()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for H, W in GRIDS:
            net = torch.tanh(torch.randn(1, 128, H, W, generator=g)).cuda()
            inp = torch.relu(torch.randn(1, 128, H, W, generator=g)).cuda()
            corr = torch.randn(1, H, W, CORR_CHANNELS + 2, generator=g).cuda()[..., :CORR_CHANNELS].permute(0, 3, 1, 2)
            flow = torch.randn(1, 2, H, W, generator=g).cuda()
            extra = (torch.randn(1, 128, H, W, generator=g).cuda(),) if family == "ccmr" else ()
            state = {"net": ub(net, inp, corr, flow, *extra)[0]}

            def call(dead):
                switch.dead = dead
                state["net"] = ub(state["net"], inp, corr, flow, *extra)[0]      # the view handed back: the next iteration of one forward

            t = alternate(torch, {"with mask": lambda: call(False), "without": lambda: call(True)}, args.rounds, args.reps)
            a, b = statistics.median(t["with mask"]), statistics.median(t["without"])
            print(f"| {family} block | 1x{H}x{W} | {med(t['with mask'])} | {med(t['without'])} | {a - b:.1f} | {b / a:.3f} |", flush=True)


def forward_model(family):
    """(model, images, the family's existing options, where the model comes from)"""
    import torch
    from oracle import ref_loader
    g = torch.Generator().manual_seed(3)
    if ref_loader.reference_available():
        if family == "ccmr":
            model = ref_loader.ref_module("ptlflow.models.ccmr.ccmr").CCMR
            base = {"ccmr_aggregator": True, "multiscale_encoders": True}
        else:
            model = ref_loader.ref_module("ptlflow.models.ms_raft_plus.ms_raft_plus").MSRAFTPlus
            base = {"multiscale_encoders": True}
        torch.manual_seed(1234)
        return model().eval(), torch.rand(1, 2, 3, 436, 1024, generator=g), base, "reference"
    from ms_loop_model import MsLoopModel
    model = MsLoopModel("ccmr", (8, 10, 15)) if family == "ccmr" else MsLoopModel("ms_raft", (4, 6, 5, 10))
    return model.eval(), torch.rand(1, 2, 3, 448, 1024, generator=g), {"multiscale_encoders": True}, "stand-in"


def step_forward(args, family):
    import torch
    from ptlflow_amd import patch
    model, x, base, origin = forward_model(family)
    for p in model.parameters():
        p.requires_grad_(False)
    model.cuda()
    x = x.cuda()
    configs = (("existing options", dict(base)),
               ("+ multiscale_upsample, every iteration", dict(base, multiscale_upsample=True, skip_dead_upsample=False)),
               ("+ multiscale_upsample, skip", dict(base, multiscale_upsample=True)))
    fwd = lambda: model({"images": x})["flows"]  # noqa: E731
    with torch.no_grad():
        if args.config is not None:
            name, kw = configs[args.config]
            patch.accelerate(model, **kw)
            for _ in range(1 + args.calls):
                fwd()
            torch.cuda.synchronize()
            print(f"{family} ({origin}) {name}: {args.calls} forwards", flush=True)
            return
        outs, times = {}, {name: [] for name, _ in configs}
        for name, kw in configs:      # outputs first
            patch.accelerate(model, **kw)
            outs[name] = fwd().float().clone()
            assert bool(torch.isfinite(outs[name]).all()), name
        names = [n for n, _ in configs]
        epe = float((outs[names[1]] - outs[names[0]]).norm(dim=2).mean())
        same = float((outs[names[2]] - outs[names[1]]).abs().max())
        skip = model.__dict__.get(patch._SKIP)
        print(f"{family} ({origin}): option on against off mean EPE {epe:.2e}; max |skip - every iteration| {same:.1e} px; "
              f"last forward: {skip.block_calls} block calls, {skip.masks_skipped} masks skipped, {skip.scratch_answers} scratch answers, "
              f"{model.__dict__['upsample_flow'].calls} served upsample calls in all", flush=True)
        assert same <= 1e-4 * float(outs[names[1]].abs().max()), same      # (bit for bit in tests/test_gpu_ms_upsample.py; a whole reference
        #  forward does not repeat its own bits from run to run on this stack)
        for _ in range(args.rounds):
            for name, kw in configs:
                patch.accelerate(model, **kw)
                fwd()
                times[name].append(timed(torch, fwd, 1))
    t0 = statistics.median(times[names[0]])
    for name in names:
        m = statistics.median(times[name])
        print(f"| {family} ({origin}) {x.shape[3]}x{x.shape[4]} b1 | {name} | {m / 1e3:8.2f} [{(max(times[name]) - min(times[name])) / 1e3:6.2f}] | "
              f"{1e6 / m:.2f} | {m / t0:.3f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, help="kernel | block:<family> | forward:<family> (default: all, each in a child process)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--config", type=int, choices=[0, 1, 2], default=None, help="a forward step: run --calls forwards of one configuration only")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        kind, _, key = args.step.partition(":")
        {"kernel": lambda: step_kernel(args), "block": lambda: step_block(args, key), "forward": lambda: step_forward(args, key)}[kind]()
        return
    lines = []
    for step in ["kernel"] + [f"block:{f}" for f in FAMILIES] + [f"forward:{f}" for f in FAMILIES]:
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
