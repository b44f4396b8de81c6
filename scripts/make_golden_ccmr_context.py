"""Writes tests/golden/ccmr_context.pt from the reference's OWN context grouping module (ptlflow/models/ccmr/xcit.py `XCiT` with
``separate=False``, as ccmr/ccmr.py:93-99 builds `model.xcit[i]`; imported unmodified through oracle/ref_loader.py, which stubs timm;
build container only, CPU):

    python scripts/make_golden_ccmr_context.py

A reference `XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=False)` gets seeded, non-trivial parameters
(tests/xcit_model.py `randomize`) and runs at B = 2 on a 7 x 10 grid.  Stored:

    state_dict        the parameters: fp32 values on the bfloat16 grid, stored as bfloat16 (exact; `.float()` gives them back)
    inp               likewise
    out, out64        the fp32 forward and the same module in float64
    A, x1, x2         the attention map [B, 8, 16, 16] and the tokens [B, N, 128] behind the attention branch and behind the local
                      patch interaction (forward hooks on attn_drop / norm3 / norm2)
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

SEED = 2817
B, H, W = 2, 7, 10
OUT = os.path.join(ROOT, "tests", "golden", "ccmr_context.pt")


def main() -> None:
    ref_loader.load()
    assert ref_loader.ensure_family("ccmr")
    XCiT = ref_loader.ref_module("ptlflow.models.ccmr.xcit").XCiT
    torch.manual_seed(SEED)
    model = randomize(XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=False), SEED).eval()
    grid = lambda t: t.to(torch.bfloat16).float()  # noqa: E731  (the nearest value that bfloat16 holds exactly)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(grid(p))
    g = torch.Generator().manual_seed(SEED + 1)
    inp = grid(torch.relu(torch.randn(B, 128, H, W, generator=g) * 1.3))      # the loop hands over relu(context features)
    blk = model.blocks[0]
    seen = {}

    def keep(name, t):      # a hook returns None (anything else would replace the tensor)
        seen.setdefault(name, t.detach().clone())

    hooks = [blk.attn.attn_drop.register_forward_hook(lambda m, i, o: keep("A", o)),
             blk.norm3.register_forward_pre_hook(lambda m, i: keep("x1", i[0])),
             blk.norm2.register_forward_pre_hook(lambda m, i: keep("x2", i[0]))]
    with torch.no_grad():
        out = model(inp)
        for h in hooks:
            h.remove()
        out64 = copy.deepcopy(model).double()(inp.double())
    b16 = lambda t: t.to(torch.bfloat16)  # noqa: E731
    assert all(torch.equal(b16(v).float(), v) for v in list(model.state_dict().values()) + [inp])
    golden = {"state_dict": {k: b16(v) for k, v in model.state_dict().items()}, "inp": b16(inp), "out": out, "out64": out64,
              "A": seen["A"], "x1": seen["x1"], "x2": seen["x2"], "shape": (B, H, W), "seed": SEED}
    torch.save(golden, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; relL2(fp32, fp64) = {float((out.double() - out64).norm() / out64.norm()):.2e}")


if __name__ == "__main__":
    main()
