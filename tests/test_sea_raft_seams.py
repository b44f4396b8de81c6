"""SEA-RAFT seams on CPU: the torch restatement (tests/sea_seam_model.py) against the reference's own modules, the dispatch of
`accelerate(model, sea_raft_update=True)` on a live reference SEARAFT, the CPU fallback, the C ABI additions and the golden weights."""
import ctypes
import os

import pytest
import torch

from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _native():
    try:
        import ptlflow_amd
        ptlflow_amd.load_native()
    except Exception as e:  # libs not built in this checkout
        pytest.skip(f"native libs unavailable: {e}")


def _ref_model(iters=2):
    mod = ref_loader.ref_module("ptlflow.models.sea_raft.sea_raft")
    torch.manual_seed(0)
    return mod.SEARAFT(block_dims=[64, 128, 256], iters=iters).eval(), mod


def _seed_heads(model, seed):
    from sea_seam_model import seeded_params
    keys = {k: tuple(v.shape) for k, v in model.state_dict().items() if k.split(".")[0] in ("update_block", "flow_head", "upsample_weight")}
    model.load_state_dict(seeded_params(keys, seed), strict=False)
    return keys


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference tree")
@pytest.mark.parametrize("seed", [0, 2024])
def test_restatement_equals_reference(seed):
    from sea_seam_model import SeaRaftLoop, load_seeded
    ref, _ = _ref_model()
    keys = _seed_heads(ref, seed)
    mine = load_seeded(SeaRaftLoop(), seed).eval()
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == keys
    g = torch.Generator().manual_seed(seed + 1)
    net = torch.tanh(torch.randn(1, 128, 9, 13, generator=g))
    inp = torch.relu(torch.randn(1, 128, 9, 13, generator=g))
    corr = torch.randn(1, 324, 9, 13, generator=g)
    flow = torch.randn(1, 2, 9, 13, generator=g)
    with torch.no_grad():
        a = ref.update_block(net, inp, corr, flow)
        b = mine.update_block(net, inp, corr, flow)
        assert torch.equal(a, b)
        assert torch.equal(ref.flow_head(a), mine.flow_head(b))
        wa, wb = 0.25 * ref.upsample_weight(a), 0.25 * mine.upsample_weight(b)
        assert torch.equal(wa, wb)
        fa = ref.flow_head(a)
        assert all(torch.equal(x, y) for x, y in zip(ref.upsample_data(flow + fa[:, :2], fa[:, 2:], wa),
                                                      mine.upsample_data(flow + fa[:, :2], fa[:, 2:], wa)))


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference tree")
def test_accelerate_wraps_searaft_and_restores():
    _native()
    from ptlflow_amd import patch
    from ptlflow_amd.sea_update import PfkSeaRaftUpdateBlock, _SeaHeadSeam, _UpsampleDataSeam
    model, mod = _ref_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ub, fh, uw = model.update_block, model.flow_head, model.upsample_weight
    orig = mod.get_corr_block
    patch.accelerate(model, sea_raft_update=True)
    try:
        assert isinstance(model.update_block, PfkSeaRaftUpdateBlock) and model.update_block._ref[0] is ub
        assert isinstance(model.flow_head, _SeaHeadSeam) and isinstance(model.upsample_weight, _SeaHeadSeam)
        assert isinstance(model.__dict__["upsample_data"], _UpsampleDataSeam)
        assert model.update_block.spec.corr_channels == 324 and model.update_block.num_blocks == 2
        assert mod.get_corr_block.channels_last is True and mod.get_corr_block.pyramid == "bilinear_f2"
        after = model.state_dict()
        assert list(after) == list(sd) and all(torch.equal(after[k], sd[k]) for k in sd)
        assert model.flow_head[0] is fh[0] and model.upsample_weight[2] is uw[2]
    finally:
        patch.restore(model)
    assert model.update_block is ub and model.flow_head is fh and model.upsample_weight is uw
    assert "upsample_data" not in model.__dict__ and mod.get_corr_block is orig


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference tree")
def test_default_accelerate_leaves_searaft_alone():
    _native()
    from ptlflow_amd import patch
    model, _ = _ref_model()
    ub, fh = model.update_block, model.flow_head
    patch.accelerate(model)
    try:
        assert model.update_block is ub and model.flow_head is fh and "upsample_data" not in model.__dict__
    finally:
        patch.restore(model)


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference tree")
def test_cpu_forward_with_option_equals_unpatched():
    _native()
    from oracle import raft_oracle as O
    from ptlflow_amd import patch
    model, _ = _ref_model(iters=2)
    _seed_heads(model, 5)
    x = O.smooth_pair(1, 128, 192, seed=3)
    with torch.no_grad():
        before = model({"images": x.clone()})
        patch.accelerate(model, sea_raft_update=True)
        try:
            after = model({"images": x.clone()})
        finally:
            patch.restore(model)
    assert torch.equal(before["flows"], after["flows"]) and torch.equal(before["flow_small"], after["flow_small"])


def test_restatement_dispatch_cpu_fallback():
    """the torch restatement registers itself; on CPU tensors every seam is the original module"""
    _native()
    from ptlflow_amd import patch
    from sea_seam_model import SeaRaftLoop, load_seeded
    model = load_seeded(SeaRaftLoop(iters=2), 3).eval()
    g = torch.Generator().manual_seed(1)
    x = [torch.tanh(torch.randn(1, 128, 16, 24, generator=g)), torch.relu(torch.randn(1, 128, 16, 24, generator=g)),
         torch.randn(1, 256, 16, 24, generator=g), torch.randn(1, 256, 16, 24, generator=g)]
    with torch.no_grad():
        want = model(*x)
        patch.accelerate(model, sea_raft_update=True)
        try:
            assert type(model.update_block).__name__ == "PfkSeaRaftUpdateBlock"
            got = model(*x)
            assert model.update_block.calls == 0 and model.flow_head.calls == 0 and model.upsample_data.calls == 0
        finally:
            patch.restore(model)
    assert all(torch.equal(got[k], want[k]) for k in ("flows", "info", "flow_small"))


def test_new_symbols_declared_and_exported():
    _native()
    import ptlflow_amd
    src = open(os.path.join(ROOT, "include", "pfk.h")).read()
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    for sym in ("pfk_dwconv_layernorm_f32", "pfk_convex_upsample_info_pm_f32"):
        assert f"int {sym}(" in src and hasattr(lib, sym)
    assert "PFK_EPI_LINEAR_GELU = 3" in src and "#define PFK_ABI_VERSION 7" in src
    assert lib.pfk_abi_version() == 7
    # argument checks run before anything touches the device
    assert lib.pfk_dwconv_layernorm_f32(None, 384, None, None, None, None, ctypes.c_float(1e-6), None, 384, 1, 4, 4, 384, 7, None) < 0
    assert lib.pfk_convex_upsample_info_pm_f32(None, 2, None, 4, 4, None, 576, None, None, 1, 4, 4, None) < 0
    for name in ("dwconv_layernorm", "convex_upsample_info_pm"):
        assert hasattr(torch.ops.pfk, name)


def test_golden_weights_deterministic():
    from sea_seam_model import SeaRaftLoop, seeded_params
    shapes = {k: tuple(v.shape) for k, v in SeaRaftLoop().state_dict().items()}
    a, b = seeded_params(shapes, 2024), seeded_params(dict(reversed(list(shapes.items()))), 2024)
    assert list(a) == sorted(shapes) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(0.5 <= float(v.min()) and float(v.max()) <= 1.5 for k, v in a.items() if k.endswith("gamma"))
    gd = torch.load(os.path.join(ROOT, "tests", "golden", "sea_raft_update.pt"))
    assert gd["seed"] == 2024 and tuple(gd["corr"].shape) == (1, 324, 7, 8)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sea_raft_update.pt")) <= 512 * 1024
