"""Writes tests/golden/sea_raft_update_grad.pt from the reference's OWN SEA-RAFT modules (imported unmodified through
oracle/ref_loader.py; build container only):

    python scripts/make_sea_raft_train_golden.py

The backward of one refinement step in float64.  A reference `SEARAFT` is built, its `update_block`, `flow_head` and `upsample_weight`
get the seeded weights of tests/golden/sea_raft_update.pt's recipe (`seeded_params(..., 2024)`, widened to float64) and its inputs
(B = 1, 7 x 8, 324 correlation channels; drawn in fp32, widened; all four require grad), and

    net_out = update_block(net, inp, corr, flow)
    loss    = sum(net_out * R_n) + sum(flow_head(net_out) * R_f) + sum(0.25 * upsample_weight(net_out) * R_w)

with seeded normal cotangents R (drawn in fp32).  Stored, tensors only: the inputs and cotangents (fp32), the four input gradients in
full (`grad.net` ...), the full gradients of `refine.{0,1}.{dwconv.weight, dwconv.bias, norm.weight, norm.bias, gamma}` (`full.<name>`)
and, for every other parameter, its gradient's L2 norm (`norm.<name>`) and its dot product with a seeded +-1 tensor (`dot.<name>`; the
signs are drawn for EVERY parameter in name-sorted order, `sign_tensors`).  `step_gradients` is the recipe itself on any three modules:
tests/test_sea_train_cpu.py runs it on the torch stand-in (tests/sea_seam_model.py) and pins that one's backward to this file.
"""
from __future__ import annotations

import os
import sys
from typing import Dict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 2024
B, H, W = 1, 7, 8
OUT = os.path.join(ROOT, "tests", "golden", "sea_raft_update_grad.pt")
PARTS = ("update_block", "flow_head", "upsample_weight")
FULL_SUFFIXES = ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "gamma")


def inputs() -> Dict[str, torch.Tensor]:
    """the inputs of sea_raft_update.pt's recipe and the cotangents, fp32"""
    g = torch.Generator().manual_seed(SEED + 1)
    d = {"net": torch.tanh(torch.randn(B, 128, H, W, generator=g)), "inp": torch.relu(torch.randn(B, 128, H, W, generator=g)),
         "corr": torch.randn(B, 324, H, W, generator=g), "flow": torch.randn(B, 2, H, W, generator=g) * 2}
    g = torch.Generator().manual_seed(SEED + 2)
    d.update({"R_n": torch.randn(B, 128, H, W, generator=g), "R_f": torch.randn(B, 6, H, W, generator=g),
              "R_w": torch.randn(B, 576, H, W, generator=g)})
    return d


def sign_tensors(shapes: Dict[str, tuple]) -> Dict[str, torch.Tensor]:
    """one +-1 tensor per parameter, drawn in name-sorted order"""
    g = torch.Generator().manual_seed(SEED + 3)
    return {n: (torch.randint(0, 2, tuple(shapes[n]), generator=g) * 2 - 1).double() for n in sorted(shapes)}


def is_full(name: str) -> bool:
    return ".refine." in name and name.endswith(FULL_SUFFIXES)


def step_gradients(update_block, flow_head, upsample_weight, data: Dict[str, torch.Tensor], dtype=torch.float64, device="cpu"):
    """(input gradients {net, inp, corr, flow}, parameter gradients {"update_block.<name>" ...}) of the loss above"""
    x = {k: data[k].to(device=device, dtype=dtype).requires_grad_(True) for k in ("net", "inp", "corr", "flow")}
    R = {k: data[k].to(device=device, dtype=dtype) for k in ("R_n", "R_f", "R_w")}
    named = {f"{part}.{n}": p for part, m in zip(PARTS, (update_block, flow_head, upsample_weight)) for n, p in m.named_parameters()}
    net_out = update_block(x["net"], x["inp"], x["corr"], x["flow"])
    loss = (net_out * R["R_n"]).sum() + (flow_head(net_out) * R["R_f"]).sum() + (0.25 * upsample_weight(net_out) * R["R_w"]).sum()
    grads = torch.autograd.grad(loss, list(x.values()) + list(named.values()))
    return dict(zip(x, grads[:4])), dict(zip(named, grads[4:]))


def summarise(data, gin, gpar) -> Dict[str, torch.Tensor]:
    out = {k: v.contiguous().clone() for k, v in data.items()}      # (clones: a view would be saved with its whole storage)
    out.update({f"grad.{k}": v.detach().contiguous().clone() for k, v in gin.items()})
    signs = sign_tensors({k: tuple(v.shape) for k, v in gpar.items()})
    for name in sorted(gpar):
        g = gpar[name].detach().double().cpu()
        if is_full(name):
            out[f"full.{name}"] = g.contiguous().clone()
        else:
            out[f"norm.{name}"] = g.norm()
            out[f"dot.{name}"] = (g * signs[name]).sum()
    return out


def make() -> Dict[str, torch.Tensor]:
    from oracle import ref_loader
    from sea_seam_model import seeded_params
    mod = ref_loader.ref_module("ptlflow.models.sea_raft.sea_raft")
    torch.manual_seed(0)
    model = mod.SEARAFT(block_dims=[64, 128, 256], iters=4).eval()
    keys = {k: tuple(v.shape) for k, v in model.state_dict().items() if k.split(".")[0] in PARTS}
    model.load_state_dict(seeded_params(keys, SEED), strict=False)
    parts = [getattr(model, p).double() for p in PARTS]
    data = inputs()
    return summarise(data, *step_gradients(*parts, data))


if __name__ == "__main__":
    fixture = make()
    torch.save(fixture, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e6:.2f} MB, {len(fixture)} tensors)")
