"""The reference's OWN `SEARAFT` class with `accelerate(model, sea_raft_update=..., sea_raft_encoders=...)`: its `ResNetFPN` encoders,
`init_conv`, update block, heads and `upsample_data` all on the kernels, held to the model's own CPU fp32 forward (the gates of
tests/test_gpu_reference_models.py::test_sea_raft_whole_model).  The class comes from oracle/ref_loader.py (the reference tree or the
archive staged by `build()`)."""
import pytest
import torch

from oracle import raft_oracle as O
from oracle import ref_loader

pytestmark = [pytest.mark.gpu, pytest.mark.reference,
              pytest.mark.skipif(not ref_loader.reference_available(),
                                 reason="no reference: run `python -c 'import __graft_entry__ as g; g.build()'` where "
                                        "the reference tree exists; it stages oracle/_ref/ for the GPU box")]


def test_sea_raft_whole_model_with_both_options(gpu):
    from ptlflow_amd import patch
    S = ref_loader.ref_module("ptlflow.models.sea_raft.sea_raft")
    torch.manual_seed(1234)
    model = S.SEARAFT(block_dims=[64, 128, 256]).eval()      # (a list: extractor.py:32-33 scales it in place)
    iters = model.iters
    H, W = 436, 1024
    x = O.smooth_pair(1, H, W, seed=11)
    with torch.no_grad():
        ref = model({"images": x.clone()})["flows"]
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ref_bf = model({"images": x.clone()})["flows"].float()
    gap = O.epe(ref_bf[:, 0], ref[:, 0])[0]
    model.to(gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        stock_bf = model({"images": x.to(gpu)})["flows"].float().cpu()
    gap_stock = O.epe(stock_bf[:, 0], ref[:, 0])[0]
    keys = list(model.state_dict())
    patch.accelerate(model, sea_raft_update=True, sea_raft_encoders=True)
    try:
        names = [type(getattr(model, a)).__name__ for a in ("fnet", "cnet", "init_conv", "update_block")]
        assert names == ["PfkResNetEncoder", "PfkResNetEncoder", "PfkInitConv", "PfkSeaRaftUpdateBlock"], names
        assert sorted(model.state_dict()) == sorted(keys)
        with torch.no_grad():
            got = model({"images": x.to(gpu)})["flows"].float().cpu()
        counts = (model.fnet.calls, model.cnet.calls, model.init_conv.calls, model.update_block.calls, model.flow_head.calls,
                  model.upsample_weight.calls, model.upsample_data.calls)
        assert counts == (2, 1, 1, iters, iters + 1, iters + 1, iters + 1), counts
        patch.accelerate(model, sea_raft_update="bf16", sea_raft_encoders="bf16")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            got_bf = model({"images": x.to(gpu)})["flows"].float().cpu()
        assert (model.fnet.calls, model.cnet.calls, model.init_conv.calls) == (4, 2, 2)
    finally:
        patch.restore(model)
        model.cpu()
    assert type(model.fnet).__name__ == "ResNetFPN" and list(model.state_dict()) == keys
    mean, mx = O.epe(got[:, 0], ref[:, 0])
    mean_bf, _ = O.epe(got_bf[:, 0], ref[:, 0])
    print(f"SEARAFT 436x1024, both options: fp32 EPE vs its own CPU forward mean {mean:.3e} max {mx:.3e}; bf16 kernels under autocast "
          f"vs CPU fp32 {mean_bf:.3e} (stock PyTorch-ROCm autocast {gap_stock:.3e}, CPU autocast {gap:.3e})")
    assert mean <= 1e-3
    # bf16: no further from the fp32 forward than twice what bf16 autocast costs this model without the kernels (GPU or CPU)
    assert gap > 0
    assert mean_bf <= 2.0 * max(gap, gap_stock) + 1e-3
