#!/usr/bin/env python3
"""Host cost of one `ConvPath.conv` call against a stand-in `ops` that does nothing: the op called directly (what `UpdateEngine._conv`
did before conv_path.py), through the launcher with every argument named, and through it positionally.  CPU only; microseconds per call,
best of five rounds.  Then the host side of 32 update-block iterations of `UpdateEngine` (motion encoder, GRU, heads) on the
CPU with the whole library replaced by no-ops: milliseconds, the fastest of 60 rounds of ten (profiles/r23_a_conv_paths.md §7).  The
second part runs unchanged in a tree from before conv_path.py."""
import os
import sys
import timeit

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Ops:
    def conv2d(self, *a):
        pass


try:
    from ptlflow_amd.conv_path import FP32
except ImportError:      # a tree from before the module: the second part only
    FP32 = None
ops, s, w, b, o = Ops(), [0], 1, 2, 3


def direct():
    ops.conv2d(s, 1, 2, 3, 1, 5, w, b, 8, 0, True, 1.0, o, None, None, None, None, None, 1, False, 0, 0)


def positional():
    FP32.conv(ops, s, 1, 2, 3, 1, 5, w, b, 8, o, 0, True, 1.0, None, None, None, None, None, None, 1, False, 0, 0)


def named():
    FP32.conv(ops, srcs=s, B=1, H=2, W=3, kh=1, kw=5, weight=w, bias=b, cout=8, out=o, epi=0, relu=True, scale=1.0, h=None, h_b16=None,
              z=None, rh=None, workspace=None, residual=None, cout_active=0, cout_split=0)


for f in (direct, positional, named) if FP32 is not None else ():
    print(f"{f.__name__:10s} {min(timeit.repeat(f, number=200000, repeat=5)) / 200000 * 1e6:.2f} us")


class NoOps:
    def __init__(self, real):
        self.real = real

    def __getattr__(self, name):
        return getattr(self.real, name) if name.endswith(("_bytes", "fault_offset")) else (lambda *a, **k: None)


import torch  # noqa: E402
from ptlflow_amd import update as U  # noqa: E402
from ptlflow_amd.synth import synth_update_block_params  # noqa: E402

for precision in ("fp32", "bf16"):
    spec = U.basic_spec()
    eng = U.UpdateEngine(synth_update_block_params(spec, 11), spec, torch.device("cpu"), precision)
    eng.ops = NoOps(eng.ops)
    eng.bind(1, 6, 8)
    corr = eng.lookup_out if eng.lookup_out is not None else torch.zeros(48, 324)
    c0, c1 = torch.zeros(1, 2, 6, 8), torch.zeros(1, 2, 6, 8)

    def forward():
        for _ in range(32):
            eng.motion_and_gru(corr, grouped=eng.can_group)
            eng.heads(c0, c1, None, want_mask=False)

    print(f"{precision}: 32 iterations {min(timeit.repeat(forward, number=10, repeat=60)) / 10 * 1e3:.3f} ms")
