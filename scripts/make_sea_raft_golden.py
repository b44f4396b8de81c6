"""Writes tests/golden/sea_raft_update.pt from the reference's OWN SEA-RAFT modules (imported unmodified through
oracle/ref_loader.py; build container only):

    python scripts/make_sea_raft_golden.py

A reference `SEARAFT` is built, its `update_block`, `flow_head`, `upsample_weight` get seeded weights (tests/sea_seam_model.py
`seeded_params`: every parameter in name-sorted order from one seed, the layer scale gamma at O(1)) and one refinement step runs
at B = 1 on a 7 x 8 grid with 324 correlation channels (small: the fixture stays a few hundred KB;
the kernels are checked on large grids by their own tests):

    net_out = update_block(net, inp, corr, flow)                    sea_raft/update.py:49-54
    flow_update = flow_head(net_out); weight_update = 0.25 * upsample_weight(net_out)
    flow_8x = flow + flow_update[:, :2]; info_8x = flow_update[:, 2:]
    up_flow, up_info = upsample_data(flow_8x, info_8x, weight_update)  sea_raft.py:147-163

Inputs and outputs are stored, weights are not (tests/test_gpu_sea_raft.py regenerates them from the seed).

    python scripts/make_sea_raft_golden.py --autocast

runs the same step under torch.autocast("cpu", dtype=torch.bfloat16) and writes tests/golden/sea_raft_update_autocast.pt: the
reference's own reduced-precision semantics (bf16 convolutions / Linear layers, fp32 LayerNorm, the dtype promotions of its cats and
sums), which tests/test_sea_raft_bf16.py pins the torch restatement to.

    python scripts/make_sea_raft_golden.py --encoder

writes tests/golden/sea_raft_encoder.pt from the reference's own `ResNetFPN` (sea_raft/extractor.py): `resnet18` with 3 and with 6 input
channels and `resnet34` with 3, parameters and running statistics from tests/sea_full_model.py `seeded_encoder_params` (seed
ENC_SEED + variant index), one 3-channel and one 6-channel 64 x 96 input, each output in fp32 and under
torch.autocast("cpu", dtype=torch.bfloat16).  Inputs and outputs only; the tests regenerate the weights from the seed.
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_loader  # noqa: E402
from sea_seam_model import seeded_params  # noqa: E402

SEED = 2024
B, H, W = 1, 7, 8
OUT = os.path.join(ROOT, "tests", "golden", "sea_raft_update.pt")
OUT_AUTOCAST = os.path.join(ROOT, "tests", "golden", "sea_raft_update_autocast.pt")
OUT_ENCODER = os.path.join(ROOT, "tests", "golden", "sea_raft_encoder.pt")
ENC_SEED = 4100
ENC_VARIANTS = (("resnet18", 3), ("resnet18", 6), ("resnet34", 3))       # (pretrain, input_dim); seed = ENC_SEED + index


def main(autocast: bool = False) -> None:
    mod = ref_loader.ref_module("ptlflow.models.sea_raft.sea_raft")
    torch.manual_seed(0)
    model = mod.SEARAFT(block_dims=[64, 128, 256], iters=4).eval()
    keys = {k: tuple(v.shape) for k, v in model.state_dict().items()
            if k.split(".")[0] in ("update_block", "flow_head", "upsample_weight")}
    model.load_state_dict(seeded_params(keys, SEED), strict=False)
    g = torch.Generator().manual_seed(SEED + 1)
    net = torch.tanh(torch.randn(B, 128, H, W, generator=g))
    inp = torch.relu(torch.randn(B, 128, H, W, generator=g))
    corr = torch.randn(B, 324, H, W, generator=g)
    flow = torch.randn(B, 2, H, W, generator=g) * 2
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        net_out = model.update_block(net, inp, corr, flow)
        flow_update = model.flow_head(net_out)
        weight_update = 0.25 * model.upsample_weight(net_out)
        flow_8x = flow + flow_update[:, :2]
        info_8x = flow_update[:, 2:]
        up_flow, up_info = model.upsample_data(flow_8x, info_8x, weight_update)
    data = {"seed": SEED, "net": net, "inp": inp, "corr": corr, "flow": flow, "net_out": net_out, "flow_update": flow_update,
            "weight_update": weight_update, "flow_8x": flow_8x, "info_8x": info_8x.contiguous(), "up_flow": up_flow,
            "up_info": up_info}
    data = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in data.items()}
    out = OUT_AUTOCAST if autocast else OUT
    if autocast:
        data["autocast"] = "cpu/bfloat16"
    torch.save(data, out)
    print(f"wrote {out} ({os.path.getsize(out) / 1e6:.2f} MB)")


def encoder() -> None:
    from sea_full_model import seeded_encoder_params
    ext = ref_loader.ref_module("ptlflow.models.sea_raft.extractor")
    g = torch.Generator().manual_seed(ENC_SEED - 1)
    data = {"seed": ENC_SEED, "variants": [list(v) for v in ENC_VARIANTS], "x3": torch.rand(1, 3, 64, 96, generator=g) * 2 - 1,
            "x6": torch.rand(1, 6, 64, 96, generator=g) * 2 - 1}
    for i, (pretrain, cin) in enumerate(ENC_VARIANTS):
        enc = ext.ResNetFPN(block_dims=[64, 128, 256], initial_dim=64, pretrain=pretrain, input_dim=cin, output_dim=256).eval()
        enc.load_state_dict(seeded_encoder_params({k: tuple(v.shape) for k, v in enc.state_dict().items()}, ENC_SEED + i), strict=True)
        x = data[f"x{cin}"]
        with torch.no_grad():
            data[f"{pretrain}_{cin}"] = enc(x).contiguous()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                data[f"{pretrain}_{cin}_autocast"] = enc(x).contiguous()     # bf16, as the module returns it
    torch.save(data, OUT_ENCODER)
    print(f"wrote {OUT_ENCODER} ({os.path.getsize(OUT_ENCODER) / 1e6:.2f} MB)")


if __name__ == "__main__":
    if "--encoder" in sys.argv[1:]:
        encoder()
    else:
        main("--autocast" in sys.argv[1:])
