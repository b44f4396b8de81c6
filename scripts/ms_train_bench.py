#!/usr/bin/env python3
"""`accelerate(model, multiscale_train=True)` — training the multi-scale refinement loops on the kernels: the measurement DESIGN.md K18
still lacks (its table rows, `--out`, are what a profile of the option is to be written from).

    python scripts/ms_train_bench.py [--out table.md]                 # every step below, each in a child process of its own
    python scripts/ms_train_bench.py --step upsample                  # one step, in this process
    python scripts/ms_train_bench.py --step step:ms_raft --config 1 --calls 2      # one side alone, for a kernel trace

Steps:
  upsample         `train.convex_upsample2` forward + backward (`pfk_convex_upsample2_f32` + `pfk_convex_upsample2_bwd_f32`) against
                   the model method's torch autograd on the same tensors, at 1x28x64, 1x56x128, 1x112x256 and 8x56x128
  lookup           `pfk_corr_lookup_coords_bwd_f32` against the backward of `F.grid_sample` with respect to its grid (the level maps
                   do not require grad), two levels of radius 4, at the same grids
  step:<style>     one training step (forward, `train.sequence_loss`, backward) of the stand-in loop with the training order
                   (tests/ms_train_model.py) at 256 x 384, batch 2: `accelerate(model)` (option off: the parent's behaviour) against
                   `accelerate(model, multiscale_train=True)`
Whole reference models in training are not measured: the reference is not on the GPU machine.
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

STEP_LIMIT = 300         # seconds per child
GRIDS = ((1, 28, 64), (1, 56, 128), (1, 112, 256), (8, 56, 128))
STYLES = {"ms_raft": (4, 6, 5, 10), "ccmr": (8, 10, 15)}


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


def step_upsample(args):
    import torch
    import ptlflow_amd
    from ms_loop_model import MsLoopModel
    from ptlflow_amd import train
    ptlflow_amd.load_native()
    g = torch.Generator().manual_seed(3)
    for B, H, W in GRIDS:
        flow = (torch.randn(B, 2, H, W, generator=g) * 3).cuda().requires_grad_()
        rows = torch.randn(B * H * W, 36, generator=g).cuda().requires_grad_()
        mask = rows.view(B, H, W, 36).permute(0, 3, 1, 2)       # the update block's mask view: pixel-major rows seen as NCHW
        go = torch.randn(B, 2, 2 * H, 2 * W, generator=g).cuda()

        def torch_side():
            return torch.autograd.grad(MsLoopModel.upsample_flow(None, flow, mask, scale=2), (flow, rows), go)

        def kernel_side():
            return torch.autograd.grad(train.convex_upsample2(flow, rows), (flow, rows), go)

        want, got = torch_side(), kernel_side()
        err = max(float((a - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(got, want))
        assert err <= 1e-4, (B, H, W, err)
        t = alternate(torch, {"torch": torch_side, "kernel": kernel_side}, args.rounds, args.reps)
        ratio = statistics.median(t["torch"]) / statistics.median(t["kernel"])
        print(f"| upsample x2 fwd + bwd | {B}x{H}x{W} | {med(t['torch'])} | {med(t['kernel'])} | {ratio:.2f} | {err:.1e} |", flush=True)


def step_lookup(args):
    import torch
    import torch.nn.functional as F
    import ptlflow_amd
    ptlflow_amd.load_native()
    L, r = 2, 4
    n = 2 * r + 1
    g = torch.Generator().manual_seed(4)
    for B, H, W in GRIDS:
        M = B * H * W
        levels = [torch.empty(M, H >> l, W >> l, device="cuda").normal_() for l in range(L)]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        coords = (torch.stack([xs, ys]).expand(B, 2, H, W) + torch.randn(B, 2, H, W, generator=g) * 2).contiguous().cuda()
        go = torch.randn(M, L * n * n, generator=g).cuda()
        off = torch.linspace(-r, r, n, device="cuda")
        window = torch.stack(torch.meshgrid(off, off, indexing="ij"), dim=-1).view(1, n, n, 2)
        centre = coords.permute(0, 2, 3, 1).reshape(M, 1, 1, 2)
        grids, outs, gos = [], [], []
        for l, lvl in enumerate(levels):        # raft/corr.py:45-52 per level; the forward is outside the timed region
            hl, wl = lvl.shape[-2:]
            pts = centre / 2 ** l + window
            grid = torch.stack([2 * pts[..., 0] / (wl - 1) - 1, 2 * pts[..., 1] / (hl - 1) - 1], dim=-1).requires_grad_()
            grids.append(grid)
            outs.append(F.grid_sample(lvl[:, None], grid, align_corners=True))
            gos.append(go[:, l * n * n:(l + 1) * n * n].reshape(M, 1, n, n))
        gc = torch.empty_like(coords)

        def torch_side():
            return [torch.autograd.grad(o, gr, gg, retain_graph=True)[0] for o, gr, gg in zip(outs, grids, gos)]

        def kernel_side():
            torch.ops.pfk.corr_lookup_coords_bwd(levels, coords, r, go, gc)

        # d(coords) = sum over levels and taps of d(grid) * 2 / (size - 1) / 2^l
        want = torch.zeros(M, 2, device="cuda")
        for l, (dg, lvl) in enumerate(zip(torch_side(), levels)):
            hl, wl = lvl.shape[-2:]
            want += dg.sum((1, 2)) * torch.tensor([2.0 / (wl - 1), 2.0 / (hl - 1)], device="cuda") / 2 ** l
        kernel_side()
        got = gc.permute(0, 2, 3, 1).reshape(M, 2)
        bad = float(((got - want).abs() > 1e-3 * want.abs().max()).float().mean())      # (a sample point within rounding of an integer may floor differently)
        assert bad <= 1e-3, (B, H, W, bad)
        t = alternate(torch, {"torch": torch_side, "kernel": kernel_side}, args.rounds, args.reps)
        ratio = statistics.median(t["torch"]) / statistics.median(t["kernel"])
        print(f"| lookup coords grad L2 r4 | {B}x{H}x{W} | {med(t['torch'])} | {med(t['kernel'])} | {ratio:.2f} | {bad:.1e} |", flush=True)
        del levels, outs, grids


def step_model(style, multiscale_train):
    import torch
    from ms_train_model import MsTrainModel
    from ptlflow_amd import patch
    torch.manual_seed(7)
    model = MsTrainModel(style, STYLES[style]).train().cuda()
    return patch.accelerate(model, multiscale_train=multiscale_train)


def step_step(args, style):
    import torch
    from ptlflow_amd import train
    g = torch.Generator().manual_seed(3)
    images = torch.rand(2, 2, 3, 256, 384, generator=g).cuda()
    gt = (torch.randn(2, 2, 256, 384, generator=g) * 2).cuda()
    valid = torch.ones(2, 1, 256, 384).cuda()

    def one(model):
        model.zero_grad(set_to_none=True)
        loss = train.sequence_loss(model({"images": images})["flow_preds"], gt, valid)
        loss.backward()
        return loss

    if args.config is not None:
        model = step_model(style, bool(args.config))
        for _ in range(1 + args.calls):
            one(model)
        torch.cuda.synchronize()
        print(f"{style} multiscale_train={bool(args.config)}: {args.calls} steps after one warm-up step; "
              f"block train_calls {model.update_block.train_calls}, seam train_calls {model.__dict__['upsample_flow'].train_calls}", flush=True)
        return
    models = {"off": step_model(style, False), "on": step_model(style, True)}
    losses = {k: float(one(m)) for k, m in models.items()}
    assert abs(losses["on"] - losses["off"]) <= 1e-3 * abs(losses["off"]), losses
    on = models["on"]
    print(f"{style} {STYLES[style]}: loss off {losses['off']:.5f} on {losses['on']:.5f}; option on: {on.update_block.train_calls} block calls and "
          f"{on.__dict__['upsample_flow'].train_calls} scale-2 upsamplings on the kernels in one step", flush=True)
    t = alternate(torch, {k: (lambda m=m: one(m)) for k, m in models.items()}, args.rounds, 1)
    a, b = statistics.median(t["off"]), statistics.median(t["on"])
    print(f"| {style} {STYLES[style]} 256x384 b2 | {a / 1e3:8.2f} [{(max(t['off']) - min(t['off'])) / 1e3:6.2f}] | "
          f"{b / 1e3:8.2f} [{(max(t['on']) - min(t['on'])) / 1e3:6.2f}] | {a / b:.3f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, help="upsample | lookup | step:<style> (default: all, each in a child process)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--config", type=int, choices=[0, 1], default=None, help="a step:<style> step: run --calls steps of one side only (0 off, 1 on)")
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        kind, _, key = args.step.partition(":")
        {"upsample": lambda: step_upsample(args), "lookup": lambda: step_lookup(args), "step": lambda: step_step(args, key)}[kind]()
        return
    lines = []
    for step in ["upsample", "lookup"] + [f"step:{s}" for s in STYLES]:
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
