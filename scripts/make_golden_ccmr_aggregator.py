"""Writes tests/golden/ccmr_aggregator.pt from the reference's OWN motion aggregator (ptlflow/models/ccmr/xcit.py `XCiT`, imported
unmodified through oracle/ref_loader.py, which stubs timm; build container only, CPU):

    python scripts/make_golden_ccmr_aggregator.py

A reference `XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=True)` (ccmr/update.py:132-134) gets seeded,
non-trivial parameters (tests/xcit_model.py `randomize`: gamma in [0.2, 1], temperature in [0.5, 2.5], non-unit norm weights,
non-zero biases) and runs twice at B = 2 on a 7 x 10 grid: the same `global_context`, two different `motion_features`.  Stored:

    state_dict                     the parameters: fp32 values on the bfloat16 grid, stored as bfloat16 (exact; `.float()` gives them back)
    global_context, motion_features [2 x]   likewise — half the bytes, so that the fixture stays below 1 MiB
    out [2 x]                      the fp32 forwards
    out64 [2 x]                    the same module in float64
    A, x1, x2                      of the first call: the attention map [B, 8, 16, 16] and the tokens [B, N, 128] behind the attention
                                   branch and behind the local patch interaction (forward hooks on attn_drop / norm3 / norm2)
"""
from __future__ import annotations

import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_loader  # noqa: E402
from xcit_model import randomize  # noqa: E402

SEED = 2511
B, H, W = 2, 7, 10
OUT = os.path.join(ROOT, "tests", "golden", "ccmr_aggregator.pt")


def main() -> None:
    ref_loader.load()
    assert ref_loader.ensure_family("ccmr")
    XCiT = ref_loader.ref_module("ptlflow.models.ccmr.xcit").XCiT
    torch.manual_seed(SEED)
    model = randomize(XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=True), SEED).eval()
    grid = lambda t: t.to(torch.bfloat16).float()  # noqa: E731  (the nearest value that bfloat16 holds exactly)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(grid(p))
    g = torch.Generator().manual_seed(SEED + 1)
    gc = grid(torch.randn(B, 128, H, W, generator=g))
    mfs = [grid(torch.randn(B, 128, H, W, generator=g) * s) for s in (1.0, 1.7)]
    blk = model.blocks[0]
    seen = {}

    def keep(name, t):      # the intermediates of the FIRST call stay; a hook returns None (anything else would replace the tensor)
        seen.setdefault(name, t.detach().clone())

    hooks = [blk.attn.attn_drop.register_forward_hook(lambda m, i, o: keep("A", o)),
             blk.norm3.register_forward_pre_hook(lambda m, i: keep("x1", i[0])),
             blk.norm2.register_forward_pre_hook(lambda m, i: keep("x2", i[0]))]
    with torch.no_grad():
        outs = [model(gc, mf) for mf in mfs]
        for h in hooks:
            h.remove()
        model64 = copy.deepcopy(model).double()
        outs64 = [model64(gc.double(), mf.double()) for mf in mfs]
    b16 = lambda t: t.to(torch.bfloat16)  # noqa: E731
    assert all(torch.equal(b16(v).float(), v) for v in list(model.state_dict().values()) + [gc] + mfs)
    golden = {"state_dict": {k: b16(v) for k, v in model.state_dict().items()}, "global_context": b16(gc),
              "motion_features": [b16(m) for m in mfs],
              "out": outs, "out64": outs64, "A": seen["A"], "x1": seen["x1"], "x2": seen["x2"], "shape": (B, H, W), "seed": SEED}
    torch.save(golden, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; relL2(fp32, fp64) = "
          + ", ".join(f"{float((o.double() - o64).norm() / o64.norm()):.2e}" for o, o64 in zip(outs, outs64)))


if __name__ == "__main__":
    main()
