"""Writes tests/golden/ms_upsample.pt and tests/golden/ms_loop_trace.json from the reference's OWN multi-scale models
(ptlflow/models/ccmr/ccmr.py `CCMR`, ptlflow/models/ms_raft_plus/ms_raft_plus.py `MSRAFTPlus`, imported unmodified through
oracle/ref_loader.py; build container only, CPU):

    python scripts/make_golden_ms_upsample.py

ms_upsample.pt     `upsample_flow(flow, mask, scale=2)` of both classes on small seeded inputs: per case flow [B, 2, H, W], mask
                   [B, 36, H, W] and the fp32 output [B, 2, 2H, 2W]; one case has logits spread over +-60 (a saturated softmax).
ms_loop_trace.json what the eval forward of `CCMR()` and `MSRAFTPlus()` at 128 x 160 calls, in order, with a counting stub in place
                   of `update_block` and `upsample_flow`: per model `iters` and a list of names, "update_block HxW" /
                   "upsample_flow HxW" (the grid of the call's `net` / `flow`).  The schedule of `patch._MultiScaleSkip` is driven
                   by this list in tests/test_ms_upsample_cpu.py, and the stand-in loop (tests/ms_loop_model.py) is checked against it.
"""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402

SEED = 2701
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = {"ccmr": ("ptlflow.models.ccmr.ccmr", "CCMR"), "ms_raft_plus": ("ptlflow.models.ms_raft_plus.ms_raft_plus", "MSRAFTPlus")}
CASES = (("random", (2, 5, 7), 1.0), ("saturated", (1, 3, 9), 60.0))


def upsample_cases() -> dict:
    g = torch.Generator().manual_seed(SEED)
    cases = {}
    for name, (B, H, W), spread in CASES:
        flow = torch.randn(B, 2, H, W, generator=g) * 3
        mask = torch.randn(B, 36, H, W, generator=g) * spread
        case = {"flow": flow, "mask": mask}
        for key, (module, cls) in MODELS.items():
            method = getattr(ref_loader.ref_module(module), cls).upsample_flow      # reads nothing of `self`
            with torch.no_grad():
                case[key] = method(None, flow, mask, scale=2)
        assert torch.equal(case["ccmr"], case["ms_raft_plus"])
        cases[name] = case
    return cases


def loop_trace(module: str, cls: str) -> dict:
    torch.manual_seed(SEED)
    model = getattr(ref_loader.ref_module(module), cls)(alternate_corr=False).eval()
    names = []

    def block(net, inp, corr, flow, *a, **k):
        names.append(f"update_block {net.shape[2]}x{net.shape[3]}")
        B, _, H, W = net.shape
        return net, net.new_zeros(B, 36, H, W), net.new_zeros(B, 2, H, W)

    def upsample_flow(flow, mask, scale=8):
        assert scale == 2 and mask.shape[1] == 36 and mask.shape[2:] == flow.shape[2:]
        names.append(f"upsample_flow {flow.shape[2]}x{flow.shape[3]}")
        B, _, H, W = flow.shape
        return flow.new_zeros(B, 2, 2 * H, 2 * W)

    model.update_block.forward = block
    model.upsample_flow = upsample_flow
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        out = model({"images": torch.rand(1, 2, 3, 128, 160, generator=g)})
    assert set(out) == {"flows", "flow_small"}
    return {"iters": [int(n) for n in model.iters], "calls": names}


def main() -> None:
    ref_loader.load()
    cases = upsample_cases()
    out = os.path.join(GOLDEN, "ms_upsample.pt")
    torch.save({"seed": SEED, "cases": cases}, out)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")
    trace = {key: loop_trace(module, cls) for key, (module, cls) in MODELS.items()}
    out = os.path.join(GOLDEN, "ms_loop_trace.json")
    with open(out, "w") as fh:
        json.dump(trace, fh, indent=0)
        fh.write("\n")
    print(f"wrote {out}: " + ", ".join(f"{k}: iters {v['iters']}, {len(v['calls'])} calls" for k, v in trace.items()))


if __name__ == "__main__":
    main()
