"""Writes tests/golden/ms_train.pt from the reference's OWN MS-RAFT+ pieces (ptlflow/models/ms_raft_plus: `update.BasicUpdateBlock`,
`ms_raft_plus.MSRAFTPlus.upsample_flow`, `corr.CorrBlock`, imported unmodified through oracle/ref_loader.py; build container only, CPU):

    python scripts/make_ms_train_golden.py

Two scales (8 x 12 and 16 x 24: 32 x 48 at 1/4 and 1/2) of the loop's TRAINING order — detach, carry over with the coarse scale's last
mask, look up, update, upsample (tests/ms_train_model.py `two_scales`) — on seeded inputs and weights (`golden_inputs`), fp32.  Recorded:
the seed, checksums of the inputs, the loss, both predictions, the gradients of the small inputs and of the small parameters in
full, and the gradient norm of every parameter and of the large inputs.  Data only: no weights (2.9 M floats would not fit a
committed file) — both sides regenerate them from the seed.
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_loader  # noqa: E402

SEED = 2901
FULL_INPUTS = ("f1a", "f2a", "net_a", "inp_a", "f1b", "f2b")
FULL_LIMIT = 10000       # parameters up to this many elements are recorded in full


def main() -> None:
    import ms_train_model as T
    ref_loader.load()
    update = ref_loader.ref_module("ptlflow.models.ms_raft_plus.update")
    corr = ref_loader.ref_module("ptlflow.models.ms_raft_plus.corr")
    loop = ref_loader.ref_module("ptlflow.models.ms_raft_plus.ms_raft_plus")
    x = T.golden_inputs(SEED)
    block = update.BasicUpdateBlock(2 * 81, scale=2).train()
    block.load_state_dict(x["weights"], strict=True)
    upsample_flow = lambda flow, mask, scale: loop.MSRAFTPlus.upsample_flow(None, flow, mask, scale=scale)      # reads nothing of `self`
    leaves = {k: x[k].clone().requires_grad_() for k in T.GOLDEN_LEAVES}
    out = T.two_scales(block, upsample_flow, lambda a, b: corr.CorrBlock(a, b, num_levels=2, radius=4), dict(leaves, start=x["start"]))
    loss = T.golden_loss(out, SEED)
    gin = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()), retain_graph=True)))
    loss.backward()
    named = dict(block.named_parameters())
    gd = {
        "seed": SEED,
        "checksums": T.checksums(x),
        "loss": float(loss),
        "out": {k: v.detach().clone() for k, v in out.items()},
        "grad_in": {k: gin[k].clone() for k in FULL_INPUTS},
        "grad_in_norm": {k: float(v.double().norm()) for k, v in gin.items() if k not in FULL_INPUTS},
        "grad_full": {k: p.grad.clone() for k, p in named.items() if p.numel() <= FULL_LIMIT},
        "grad_norm": {k: float(p.grad.double().norm()) for k, p in named.items()},
    }
    path = os.path.join(ROOT, "tests", "golden", "ms_train.pt")
    torch.save(gd, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; loss {gd['loss']:.6f}; "
          f"|d/dmask.2.weight| {gd['grad_norm']['mask.2.weight']:.4e}; full gradients: {sorted(gd['grad_full'])}")


if __name__ == "__main__":
    main()
