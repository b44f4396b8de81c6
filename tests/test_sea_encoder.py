"""SEA-RAFT's ResNet encoders without a GPU: the stand-in of tests/sea_full_model.py is the reference's ResNetFPN (where the reference
exists) and reproduces the committed reference outputs, the matcher, `accelerate(model, sea_raft_encoders=...)` dispatch and `restore`,
the CPU fall-through and the C ABI additions."""
import ctypes
import os

import pytest
import torch

import ptlflow_amd
import sea_full_model as M
from ptlflow_amd import patch
from ptlflow_amd.sea_encoder import PfkInitConv, PfkResNetEncoder, block_table, match_resnet_fpn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sea_raft_encoder.pt")
ENC_SEED = 4100          # scripts/make_sea_raft_golden.py
VARIANTS = (("resnet18", 3), ("resnet18", 6), ("resnet34", 3))


def _encoder(pretrain, cin, seed, **kw):
    return M.load_seeded_encoder(M.ResNetFPN(pretrain=pretrain, input_dim=cin, **kw), seed).eval()


# ------------------------------------------------------------------------------------------------------------- the stand-in
@pytest.mark.parametrize("variant", range(3))
def test_stand_in_reproduces_the_golden(variant):
    """fp32: within fp32 rounding of the reference's output (same operations; the thread count may change a summation order);
    autocast: the same bf16 values up to one bf16 ulp of the output's scale"""
    pretrain, cin = VARIANTS[variant]
    gold = torch.load(GOLDEN)
    assert os.path.getsize(GOLDEN) <= 1024 * 1024
    assert gold["seed"] == ENC_SEED and [tuple(v) for v in gold["variants"]] == list(VARIANTS)
    enc = _encoder(pretrain, cin, ENC_SEED + variant)
    x, want = gold[f"x{cin}"], gold[f"{pretrain}_{cin}"]
    with torch.no_grad():
        got = enc(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            got_ac = enc(x)
    scale = float(want.abs().max())
    assert got.shape == want.shape == (1, 256, 8, 12)
    assert float((got - want).abs().max()) <= 1e-5 * scale
    want_ac = gold[f"{pretrain}_{cin}_autocast"]
    assert got_ac.dtype == want_ac.dtype == torch.bfloat16
    assert float((got_ac.float() - want_ac.float()).abs().max()) <= 2 ** -6 * scale
    assert float((want_ac.float() - want).abs().max()) > 0


@pytest.mark.reference
@pytest.mark.parametrize("variant", range(3))
def test_stand_in_is_the_reference_module(variant):
    from oracle import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("no reference tree and no staged archive")
    ext = ref_loader.ref_module("ptlflow.models.sea_raft.extractor")
    pretrain, cin = VARIANTS[variant]
    ref = ext.ResNetFPN(block_dims=[64, 128, 256], initial_dim=64, pretrain=pretrain, input_dim=cin, output_dim=256).eval()
    mine = _encoder(pretrain, cin, 9 + variant)
    ref.load_state_dict(mine.state_dict(), strict=True)
    x = torch.randn(2, cin, 64, 96, generator=torch.Generator().manual_seed(variant))
    with torch.no_grad():
        assert torch.equal(ref(x), mine(x))
    assert match_resnet_fpn(ref), "the matcher refuses the reference's own module"


def test_seeding_keeps_the_two_names_of_bn3_equal():
    enc = _encoder("resnet18", 3, 1)
    sd = enc.state_dict()
    both = [k for k in sd if ".downsample.1." in k]
    assert len(both) == 2 * 5                      # layer2.0 and layer3.0: weight, bias, running_mean, running_var, num_batches_tracked
    for k in both:
        assert torch.equal(sd[k], sd[k.replace(".downsample.1.", ".bn3.")])
    assert all(float(v.min()) > 0 for k, v in sd.items() if k.endswith("running_var"))


# ------------------------------------------------------------------------------------------------------------- the matcher
@pytest.mark.parametrize("pretrain,cin", [("resnet18", 3), ("resnet18", 6), ("resnet34", 3), ("resnet34", 6)])
def test_matcher_accepts_the_stand_in(pretrain, cin):
    enc = _encoder(pretrain, cin, 2)
    assert patch.match_resnet_encoder(enc)
    table = block_table({k: tuple(v.shape) for k, v in enc.state_dict().items()})
    assert len(table) == sum(M.N_BLOCKS[pretrain])
    # a downsample path on a stride and on a width change, nowhere else
    assert [t[4] for t in table] == [t[3] != 1 or t[1] != t[2] for t in table]
    assert [t[0] for t in table if t[4]] == ["layer2.0", "layer3.0"]


def test_matcher_accepts_a_width_change_at_stride_one():
    """layer1 at another width than the stem's: a downsample path without a stride (layer.py:136)"""
    enc = M.ResNetFPN(block_dims=(128, 128, 256))
    table = block_table({k: tuple(v.shape) for k, v in enc.state_dict().items()})
    assert table[0] == ("layer1.0", 64, 128, 1, True)
    assert patch.match_resnet_encoder(enc)


def test_matcher_refusals():
    assert not patch.match_resnet_encoder(M.ResNetFPN(block_dims=(64, 96, 256)))           # a width the kernels' K chunks do not take
    assert not patch.match_resnet_encoder(M.ResNetFPN(initial_dim=32))                     # a stem the stem kernel is not built for
    assert not patch.match_resnet_encoder(M.ResNetFPN(input_dim=4))
    assert not patch.match_resnet_encoder(M.ResNetFPN(norm_layer=lambda c: torch.nn.GroupNorm(8, c)))
    assert not patch.match_resnet_encoder(M.ResNetFPN(norm_layer=torch.nn.InstanceNorm2d))
    enc = M.ResNetFPN()
    del enc.layer2[0].bn3                                                                  # the alias gone: `downsample.1` alone
    assert "layer2.0.downsample.1.weight" in enc.state_dict() and "layer2.0.bn3.weight" not in enc.state_dict()
    assert not patch.match_resnet_encoder(enc)
    enc = M.ResNetFPN()
    enc.layer2[0].bn3 = torch.nn.BatchNorm2d(128)                                          # both names, two different norms
    assert not patch.match_resnet_encoder(enc)
    enc = M.ResNetFPN()
    enc.final_conv = torch.nn.Conv2d(256, 256, 3, padding=1)
    assert not patch.match_resnet_encoder(enc)

    class Other(torch.nn.Module):                                                          # the right state_dict, an unregistered class
        def __init__(self):
            super().__init__()
            for name, child in M.ResNetFPN().named_children():
                self.add_module(name, child)

    assert match_resnet_fpn(Other()) and not patch.match_resnet_encoder(Other())


# ------------------------------------------------------------------------------------------------------------- dispatch
def test_default_accelerate_leaves_the_encoders_alone():
    model = M.seeded_full(0)
    before = (model.fnet, model.cnet, model.init_conv)
    keys = list(model.state_dict())
    for kw in ({}, {"sea_raft_update": True}, {"sea_raft_encoders": False}, {"sea_raft_encoders": None}):
        patch.accelerate(model, **kw)
        try:
            assert (model.fnet, model.cnet, model.init_conv) == before
            assert not getattr(model.update_block, "adopt_first_net", False)
        finally:
            patch.restore(model)
    assert list(model.state_dict()) == keys


@pytest.mark.parametrize("value,precision", [(True, "fp32"), ("fp32", "fp32"), ("bf16", "bf16")])
def test_accelerate_wraps_and_restore_unwraps(value, precision):
    model = M.seeded_full(0)
    before = (model.fnet, model.cnet, model.init_conv)
    keys, n_params = list(model.state_dict()), len(list(model.parameters()))
    patch.accelerate(model, sea_raft_encoders=value)
    assert isinstance(model.fnet, PfkResNetEncoder) and isinstance(model.cnet, PfkResNetEncoder) and isinstance(model.init_conv, PfkInitConv)
    assert (model.fnet.precision, model.cnet.precision, model.init_conv.precision) == (precision,) * 3
    assert sorted(model.state_dict()) == sorted(keys) and len(list(model.parameters())) == n_params
    assert model.init_conv.weight is before[2].weight and model.cnet.conv1 is before[1].conv1
    assert type(model.update_block).__name__ == "BasicUpdateBlock"          # the other option was not asked for
    patch.restore(model)
    assert (model.fnet, model.cnet, model.init_conv) == before and list(model.state_dict()) == keys


def test_switching_and_the_iteration_zero_heads():
    model = M.seeded_full(0)
    patch.accelerate(model, sea_raft_encoders=True)
    wrapped = (model.fnet, model.cnet, model.init_conv)
    patch.accelerate(model, sea_raft_encoders="bf16")                        # a second call switches, it does not wrap twice
    assert (model.fnet, model.cnet, model.init_conv) == wrapped
    assert (model.fnet.precision, model.cnet.precision, model.init_conv.precision) == ("bf16",) * 3
    patch.accelerate(model)                                                  # the default call does not take it away
    assert model.fnet is wrapped[0] and model.fnet.precision == "bf16"
    patch.accelerate(model, sea_raft_update=True)                            # the loop option later: the heads serve iteration 0 too
    assert model.update_block.adopt_first_net is True
    patch.restore(model)
    assert type(model.fnet).__name__ == "ResNetFPN" and type(model.update_block).__name__ == "BasicUpdateBlock"
    patch.accelerate(model, sea_raft_update=True)
    assert model.update_block.adopt_first_net is False
    patch.restore(model)


@pytest.mark.parametrize("value", ["fp16", "bf16x3", 1.5, "true"])
def test_value_errors(value):
    model = M.seeded_full(0)
    with pytest.raises(ValueError, match="sea_raft_encoders"):
        patch.accelerate(model, sea_raft_encoders=value)
    assert type(model.fnet).__name__ == "ResNetFPN"


def test_partial_models():
    """only what matches is wrapped: another cnet keeps init_conv a Conv2d; a model without encoders is left as it is"""
    model = M.seeded_full(0)
    model.cnet = M.ResNetFPN(input_dim=6, norm_layer=lambda c: torch.nn.GroupNorm(8, c))
    patch.accelerate(model, sea_raft_encoders=True)
    assert isinstance(model.fnet, PfkResNetEncoder) and type(model.cnet).__name__ == "ResNetFPN" and type(model.init_conv) is torch.nn.Conv2d
    patch.restore(model)
    model = M.seeded_full(0)
    model.init_conv = torch.nn.Conv2d(256, 256, 3, padding=1, bias=False)
    patch.accelerate(model, sea_raft_encoders=True)
    assert isinstance(model.cnet, PfkResNetEncoder) and type(model.init_conv) is torch.nn.Conv2d
    patch.restore(model)


def test_cpu_forward_is_the_wrapped_modules():
    model = M.seeded_full(3, iters=2)
    x = M.smooth_images(1, 128, 192, seed=1)
    with torch.no_grad():
        want = model(*x)
    patch.accelerate(model, sea_raft_update=True, sea_raft_encoders=True)
    try:
        with torch.no_grad():
            got = model(*x)
        assert (model.fnet.calls, model.cnet.calls, model.init_conv.calls, model.flow_head.calls) == (0, 0, 0, 0)
    finally:
        patch.restore(model)
    assert torch.isfinite(want["flows"]).all()
    for k in ("flows", "info", "flow_small"):
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    if not ptlflow_amd.LIBPFK_PATH.exists():
        from ptlflow_amd import _build
        _build.build_all()
    return ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))


def test_stem2_symbols_validate_their_arguments_without_a_gpu(lib):
    LL, I, P = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)
    for name in ("pfk_conv_stem2_f32", "pfk_conv_stem2_b16"):
        fn = getattr(lib, name)
        fn.argtypes = [P, LL, P, LL, P, P, P, I, I, I, I, I, I, I, P]
        fn.restype = I

        def call(a=p, sa=3 * 16 * 16, b=None, sb=0, w=p, out=p, out_ld=64, B=1, H=16, W=16, cin=3, cout=64):
            return fn(a, sa, b, sb, w, None, out, out_ld, B, H, W, cin, cout, 1, None)

        assert call(a=None) == -1 and call(w=None) == -1 and call(out=None) == -1
        assert call(B=0) == -1 and call(H=0) == -1 and call(out_ld=63) == -1
        assert call(cin=6) == -1                                   # six channels need the second image
        assert call(b=p, sb=3 * 16 * 16, cin=3) == -1              # and two images are six channels
        assert call(cin=4) == -1
        assert call(sa=3 * 16 * 16 - 1) == -1                      # images may not overlap
        assert call(b=p, sb=10, cin=6) == -1
        assert call(cout=32, out_ld=64) == -3 and call(cout=48) == -3     # PFK_ERR_UNSUPPORTED: the caller keeps the module
        assert call(w=ctypes.cast(ctypes.addressof(buf) + 4, P)) == -2    # PFK_ERR_ALIGNMENT
    assert lib.pfk_abi_version() == 7


def test_winograd_residual_symbol_refuses_without_a_gpu(lib):
    assert lib.pfk_conv2d_wino_res_f32(None, None) == -1
    from pfk_ctypes import declared
    assert {"pfk_conv2d_wino_res_f32", "pfk_conv_stem2_f32", "pfk_conv_stem2_b16"} <= set(declared())
