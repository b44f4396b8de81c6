#!/usr/bin/env python3
"""CCMR's `external_aggregate` step of one update-block call — from the motion features in the update engine's rows to the filled
aggregate slot — with `ccmr_aggregator` off (the aggregator module in torch between two layout changes: the parent's code) and on
(the kernels of ptlflow_amd/xcit.py), on the torch stand-in tests/xcit_model.py: the measurement behind DESIGN.md K14.

    python scripts/xcit_aggregator_bench.py [--grids 1x28x64 ...] [--reps 20] [--rounds 9] [--out table.md]
    python scripts/xcit_aggregator_bench.py --side on --grids 1x56x128 --calls 30        # one side alone, for a kernel trace

Per grid the two sides alternate; each figure is the median of `--rounds` timings of `--reps` calls (device events), with max - min
in brackets.  `step` is the steady-state call (the scale's attention map cached), `prepare` the once-per-(forward, scale) part of the
kernel path (x0, qk, the map, the fold), `iteration` one whole `PfkUpdateBlock` call with the option off / on, and `share` the off
step over the off iteration.  Before timing, the two sides' outputs are compared on the same inputs."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import ptlflow_amd  # noqa: E402
from ptlflow_amd.raft import _param_tree  # noqa: E402
from ptlflow_amd.synth import synth_state_dict, update_block_shapes  # noqa: E402
from ptlflow_amd.update import PfkUpdateBlock, ccmr_spec  # noqa: E402
from xcit_model import XCiT, randomize, register  # noqa: E402

CORR = 162


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


def make_block():
    register()
    spec = ccmr_spec(CORR)
    holder = _param_tree(update_block_shapes(spec))
    holder.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in holder.state_dict().items()}, seed=29))
    holder.add_module("aggregator", torch.nn.ModuleList([randomize(XCiT(separate=True), 61)]))
    ub = PfkUpdateBlock(holder, spec).cuda().eval()
    for p in ub.parameters():
        p.requires_grad_(False)
    return ub


class Case:
    """one grid: the block's engine bound to it, motion features in its rows, and the two sides of the step as callables"""

    def __init__(self, ub, B, H, W):
        g = torch.Generator().manual_seed(B * 1000 + H)
        rnd = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
        self.ub, self.B, self.H, self.W = ub, B, H, W
        self.net, self.inp, self.ctx = torch.tanh(rnd(B, 128, H, W)), torch.relu(rnd(B, 128, H, W)), rnd(B, 128, H, W)
        self.flow = rnd(B, 2, H, W) * 2
        padded = torch.zeros(B * H * W, (CORR + 3) // 4 * 4, device="cuda")      # the rows a ptlflow_amd CorrBlock hands the block
        padded[:, :CORR] = rnd(B * H * W, CORR)
        self.corr = padded[:, :CORR].view(B, H, W, CORR).permute(0, 3, 1, 2)
        self.corr._pfk_padded_pm = padded
        ub.set_ccmr_aggregator(True)
        self.n = self.net
        self.iteration(False)                                                     # binds the engine, fills the motion features
        self.iteration(True)
        self.eng = ub._engine
        self.module = ub._ref[0].aggregator[0]
        self.agg = ub._aggregator_engine(0, self.eng, (self.net, self.ctx), False)
        assert self.agg is not None and ub.aggregator_calls > 0

    def off(self):
        eng, (B, H, W) = self.eng, (self.B, self.H, self.W)
        mf = eng.motion_view.unflatten(0, (B, H, W)).permute(0, 3, 1, 2)
        mfg = self.module(self.ctx, mf)
        eng.ops.nchw_to_pm(mfg.float().contiguous(), eng.aggregate_view)

    def on(self, refresh=False):
        self.agg.run(self.ctx, self.eng.motion_view, self.eng.aggregate_view, self.B, self.H, self.W, refresh=refresh)

    def iteration(self, option):
        """one loop iteration (`net` is the block's own buffer from the previous call; the first call of a case starts the forward)"""
        self.ub.ccmr_aggregator = option          # (the attribute alone: `set_ccmr_aggregator(False)` would drop the engines)
        self.n, _m, _d = self.ub(self.n, self.inp, self.corr, self.flow, self.ctx, level_index=0)


def med(ts):
    return f"{statistics.median(ts):8.1f} [{max(ts) - min(ts):6.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["1x28x64", "1x56x128", "1x112x256", "8x28x64", "8x56x128", "8x112x256"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--side", choices=["off", "on"], default=None, help="run --calls steps of one side only (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ptlflow_amd.load_native()
    ub = make_block()
    lines = ["| grid | pixels | step off (us) | step on (us) | off / on | prepare (us) | iteration off (us) | iteration on (us) | share of the off iteration |",
             "|---|---|---|---|---|---|---|---|---|"]
    with torch.no_grad():
        for grid in args.grids:
            B, H, W = map(int, grid.split("x"))
            c = Case(ub, B, H, W)
            if args.side:
                fn = c.off if args.side == "off" else c.on
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                print(f"{grid}: {args.calls} steps of side {args.side}", flush=True)
                continue
            c.off()
            want = c.eng.aggregate_view.clone()
            c.on(refresh=True)
            got = c.eng.aggregate_view
            err, scale = float((got - want).abs().max()), float(want.abs().max())
            assert err <= 5e-4 * scale, (grid, err, scale)
            t_off, t_on, t_prep, i_off, i_on = [], [], [], [], []
            for _ in range(args.rounds):      # alternating, so that a drift of the clocks hits both alike
                t_off.append(timed(c.off, args.reps))
                t_on.append(timed(c.on, args.reps))
                t_prep.append(timed(lambda: c.on(True), args.reps) - t_on[-1])
                i_off.append(timed(lambda: c.iteration(False), args.reps))
                i_on.append(timed(lambda: c.iteration(True), args.reps))
            row = (f"| {grid} | {B * H * W} | {med(t_off)} | {med(t_on)} | {statistics.median(t_off) / statistics.median(t_on):.2f} | {med(t_prep)} | "
                   f"{med(i_off)} | {med(i_on)} | {statistics.median(t_off) / statistics.median(i_off):.2f} |")
            print(row + f"   (max |on - off| {err:.2e} of {scale:.2e})", flush=True)
            lines.append(row)
    if args.out and not args.side:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
