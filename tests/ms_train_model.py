"""TEST INFRASTRUCTURE.  `MsLoopModel` (tests/ms_loop_model.py) with the TRAINING order of the two reference loops
(ms_raft_plus/ms_raft_plus.py:197-202, ccmr/ccmr.py:194-204): a block call first detaches the position and only then, at the first
call of every scale but the coarsest, carries the estimate over with `upsample_flow(..., mask, scale=2)` on the previous scale's last
mask.  So the first lookup of a finer scale, and the displacement its block call reads, depend on that mask: its head receives a
gradient through the lookup's COORDINATES and through the block's flow input.  The stock stand-in carries over first and detaches
after (eval drops the graph anyway), so it has neither."""
from __future__ import annotations

from typing import Optional

import torch

import ms_loop_model
from ms_loop_model import Estimate, MsLoopModel


class MsTrainModel(MsLoopModel):
    def _open_scale(self, est: Optional[Estimate], like: torch.Tensor) -> Estimate:
        if est is not None:
            est.position = est.position.detach()            # the detach comes first ...
        new = super()._open_scale(est, like)                # ... then the carry-over, which keeps its graph
        new.carried = est is not None
        return new

    def _refine(self, est: Estimate, lookup, state, scale: int) -> None:
        if est.carried:
            est.carried = False                             # the position was detached before it was carried over
        else:
            est.position = est.position.detach()
        args = (state["hidden"], state["context"], lookup(est.position), est.displacement())
        if self.style == "ccmr":
            state["hidden"], est.mask, step = self.update_block(*args, state["global"], level_index=scale)
        else:
            state["hidden"], est.mask, step = self.update_block(*args)
        est.position = est.position + step


# The inherited `forward` calls the `get_corr_block` global of the stand-in's own module, which is the one seam B1 must rebind:
# `accelerate` finds it through the class's module.  (The parent is registered as a multi-scale loop; `accelerate` reads the MRO.)
MsTrainModel.__module__ = ms_loop_model.__name__


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/ms_train.pt: two scales of the training order on one update block, written by scripts/make_ms_train_golden.py with the
# reference's own block, `upsample_flow` and `CorrBlock`, replayed by tests/test_gpu_ms_train.py through the seams.  The recording
# holds a seed, not the 2.9 M weights: inputs and weights come from `golden_inputs` on both sides (checksums are recorded).
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN_LEAVES = ("f1a", "f2a", "net_a", "inp_a", "f1b", "f2b", "net_b", "inp_b")


def golden_inputs(seed: int) -> dict:
    """feature maps (32 channels), hidden state and context of a 8 x 12 and a 16 x 24 grid (32 x 48 at 1/4 and 1/2), a displacement to
    start from, and the update block's weights by name"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    x = {}
    for tag, (h, w) in (("a", (8, 12)), ("b", (16, 24))):
        x["f1" + tag], x["f2" + tag] = r(1, 32, h, w), r(1, 32, h, w)
        x["net_" + tag], x["inp_" + tag] = torch.tanh(r(1, 128, h, w)), torch.relu(r(1, 128, h, w))
    x["start"] = 1.5 * r(1, 2, 8, 12)
    x["weights"] = {}
    for name, p in ms_loop_model.MsUpdateBlock().state_dict().items():
        scale = (1.0 / p[0].numel()) ** 0.5 if name.endswith("weight") else 0.1
        x["weights"][name] = scale * r(*p.shape)
    return x


def checksums(x: dict) -> dict:
    out = {k: float(v.double().abs().sum()) for k, v in x.items() if torch.is_tensor(v)}
    out["weights"] = float(sum(v.double().abs().sum() for v in x["weights"].values()))
    return out


def two_scales(block, upsample_flow, corr_block, t: dict) -> dict:
    """ms_raft_plus.py:185-209 for two scales with one block call each: `corr_block(fmap1, fmap2)` builds a lookup"""
    grid = lambda like: ms_loop_model.pixel_grid(like.shape[0], like.shape[2], like.shape[3], like)
    out = {}
    coords0 = grid(t["f1a"])
    coords1 = (coords0 + t["start"]).detach()
    corr = corr_block(t["f1a"], t["f2a"])(coords1)
    _, up_mask, delta = block(t["net_a"], t["inp_a"], corr, coords1 - coords0)
    coords1 = coords1 + delta
    out["flow_up_a"] = upsample_flow(coords1 - coords0, up_mask, scale=2)
    coords1 = coords1.detach()                                       # the detach ...
    coords1 = upsample_flow(coords1, up_mask, scale=2)               # ... then the carry-over by the coarse scale's mask
    coords0 = grid(t["f1b"])
    corr = corr_block(t["f1b"], t["f2b"])(coords1)
    _, up_mask, delta = block(t["net_b"], t["inp_b"], corr, coords1 - coords0)
    coords1 = coords1 + delta
    out["flow_up_b"] = upsample_flow(coords1 - coords0, up_mask, scale=2)
    return out


def golden_loss(out: dict, seed: int) -> torch.Tensor:
    """a seeded linear functional of both predictions"""
    g = torch.Generator().manual_seed(seed + 1)
    loss = 0.0
    for k in ("flow_up_a", "flow_up_b"):
        loss = loss + (out[k] * torch.randn(out[k].shape, generator=g).to(out[k].device)).mean()
    return loss
