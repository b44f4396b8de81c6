"""SEA-RAFT's bf16 refinement path on CPU: the C ABI additions (declarations, exports, argument checks before any device work), the
`accelerate(model, sea_raft_update="bf16")` opt-in and its dispatch on CPU tensors, and the autocast golden of the reference's own
modules that pins tests/sea_seam_model.py's reduced-precision semantics (the GPU gate of tests/test_gpu_sea_raft_bf16.py uses the
restatement, never the reference)."""
import ctypes
import os

import pytest
import torch

from pfk_ctypes import DescB16 as _DescB16, SrcB16 as _SrcB16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sea_raft_update.pt")
GOLDEN_AUTOCAST = os.path.join(ROOT, "tests", "golden", "sea_raft_update_autocast.pt")
NEW_SYMBOLS = ("pfk_dwconv_layernorm_b16", "pfk_conv2d_gelu_b16", "pfk_convex_upsample_info_pm_b16")
BAD_ARG, ALIGNMENT = -1, -2


@pytest.fixture(scope="module")
def lib():
    try:
        import ptlflow_amd
        ptlflow_amd.load_native()
    except Exception as e:  # libs not built in this checkout
        pytest.skip(f"native libs unavailable: {e}")
    return ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))


def test_symbols_declared_exported_abi_unchanged(lib):
    src = open(os.path.join(ROOT, "include", "pfk.h")).read()
    for sym in NEW_SYMBOLS:
        assert f"int {sym}(" in src and hasattr(lib, sym), sym
    assert "#define PFK_ABI_VERSION 7" in src and lib.pfk_abi_version() == 7
    for name in ("dwconv_layernorm_b16", "conv2d_gelu_b16", "convex_upsample_info_pm_b16"):
        assert hasattr(torch.ops.pfk, name)


def _dw(lib, inp, in_ld, out, out_ld, C=384, k=7, B=1, H=4, W=4):
    w = torch.zeros(512 * 49)
    return lib.pfk_dwconv_layernorm_b16(ctypes.c_void_p(inp), in_ld, ctypes.c_void_p(w.data_ptr()), None,
                                        ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(w.data_ptr()), ctypes.c_float(1e-6),
                                        ctypes.c_void_p(out), out_ld, B, H, W, C, k, None)


def test_dwconv_layernorm_b16_argument_checks(lib):
    a = torch.zeros(16 * 520 + 64, dtype=torch.bfloat16)
    b = torch.zeros(16 * 520 + 64, dtype=torch.bfloat16)
    pa, pb = a.data_ptr(), b.data_ptr()
    assert pa % 16 == 0 and pb % 16 == 0
    assert _dw(lib, 0, 384, pb, 384) == BAD_ARG                       # null input
    assert _dw(lib, pa, 384, pb, 384, k=6) == BAD_ARG                 # even k
    assert _dw(lib, pa, 384, pb, 384, k=9) == BAD_ARG                 # k > 7
    assert _dw(lib, pa, 384, pb, 384, C=4) == BAD_ARG                 # C < 8
    assert _dw(lib, pa, 388, pb, 388, C=388) == ALIGNMENT             # C % 8
    assert _dw(lib, pa, 388, pb, 384, C=384) == ALIGNMENT             # in_ld % 8
    assert _dw(lib, pa, 384, pb, 388, C=384) == ALIGNMENT             # out_ld % 8
    assert _dw(lib, pa + 8, 384, pb, 384) == ALIGNMENT                # input rows not 16-byte aligned
    assert _dw(lib, pa, 384, pb + 8, 384) == ALIGNMENT                # output rows not 16-byte aligned
    assert _dw(lib, pa, 384, pa, 384) == BAD_ARG                      # out overlaps the input rows


def test_conv2d_gelu_b16_argument_checks(lib):
    M, cin, cout = 256, 64, 64
    x = torch.zeros(M, cin, dtype=torch.bfloat16)
    wt = torch.zeros(cout, cin, dtype=torch.bfloat16)
    out = torch.zeros(M, cout, dtype=torch.bfloat16)

    def desc(epilogue=3, relu=0, src_off=0):
        d = _DescB16()
        d.src[0] = _SrcB16(x.data_ptr() + src_off, cin, cin)
        d.num_src, d.B, d.H, d.W, d.kh, d.kw = 1, 1, 1, M, 1, 1
        d.weight, d.cout, d.epilogue, d.relu, d.scale = wt.data_ptr(), cout, epilogue, relu, 1.0
        d.out, d.out_ld, d.out_bf16 = out.data_ptr(), cout, 1
        return d

    assert lib.pfk_conv2d_gelu_b16(None, None) == BAD_ARG
    assert lib.pfk_conv2d_gelu_b16(ctypes.byref(desc(epilogue=0)), None) == BAD_ARG      # LINEAR: not this entry's epilogue
    assert lib.pfk_conv2d_gelu_b16(ctypes.byref(desc(relu=1)), None) == BAD_ARG          # relu together with GELU
    assert lib.pfk_conv2d_gelu_b16(ctypes.byref(desc(src_off=8)), None) == ALIGNMENT     # misaligned source rows
    # pfk_conv2d_b16 keeps refusing the GELU epilogue
    assert lib.pfk_conv2d_b16(ctypes.byref(desc()), None) < 0
    assert float(out.float().abs().sum()) == 0.0


def test_convex_upsample_info_pm_b16_argument_checks(lib):
    M = 16
    flow = torch.zeros(M, 2)
    info = torch.zeros(M, 4)
    mask = torch.zeros(M * 584 + 64, dtype=torch.bfloat16)
    fo, io = torch.zeros(2 * 64 * M), torch.zeros(4 * 64 * M)
    f = lib.pfk_convex_upsample_info_pm_b16

    def call(mask_ptr, mask_ld, n=4, flow_ptr=flow.data_ptr()):
        return f(ctypes.c_void_p(flow_ptr), 2, ctypes.c_void_p(info.data_ptr()), 4, n, ctypes.c_void_p(mask_ptr), mask_ld,
                 ctypes.c_void_p(fo.data_ptr()), ctypes.c_void_p(io.data_ptr()), 1, 4, 4, None)

    assert call(mask.data_ptr(), 576, flow_ptr=0) == BAD_ARG
    assert call(mask.data_ptr(), 576, n=0) == BAD_ARG
    assert call(mask.data_ptr(), 576, n=9) == BAD_ARG
    assert call(mask.data_ptr(), 572) == BAD_ARG                # fewer than 576 logits per row
    assert call(mask.data_ptr(), 580) == ALIGNMENT              # mask_ld % 8
    assert call(mask.data_ptr() + 8, 576) == ALIGNMENT          # rows not 16-byte aligned


# ------------------------------------------------------------------------------------------------------------- public interface
def _loop(seed=3, iters=2):
    from sea_seam_model import SeaRaftLoop, load_seeded
    return load_seeded(SeaRaftLoop(iters=iters), seed).eval()


def _inputs(B=1, H=16, W=24):
    g = torch.Generator().manual_seed(1)
    return [torch.tanh(torch.randn(B, 128, H, W, generator=g)), torch.relu(torch.randn(B, 128, H, W, generator=g)),
            torch.randn(B, 256, H, W, generator=g), torch.randn(B, 256, H, W, generator=g)]


def test_bf16_option_on_cpu_equals_unpatched(lib):
    from ptlflow_amd import patch
    model = _loop()
    x = _inputs()
    with torch.no_grad():
        want = model(*x)
        patch.accelerate(model, sea_raft_update="bf16")
        try:
            ub = model.update_block
            assert type(ub).__name__ == "PfkSeaRaftUpdateBlock" and ub.precision == "bf16"
            assert model.upsample_data.precision == "bf16"
            got = model(*x)
            assert ub.calls == 0 and model.flow_head.calls == 0 and model.upsample_weight.calls == 0 and model.upsample_data.calls == 0
        finally:
            patch.restore(model)
    assert all(torch.equal(got[k], want[k]) for k in ("flows", "info", "flow_small"))


@pytest.mark.parametrize("value", ["fp16", "bf16x3", "BF16", 1])
def test_other_values_raise(lib, value):
    from ptlflow_amd import patch
    model = _loop()
    ub = model.update_block
    with pytest.raises(ValueError):
        patch.accelerate(model, sea_raft_update=value)
    assert model.update_block is ub and "upsample_data" not in model.__dict__


def test_second_accelerate_switches_precision(lib):
    from ptlflow_amd import patch
    model = _loop()
    patch.accelerate(model, sea_raft_update=True)
    try:
        ub = model.update_block
        assert ub.precision == "fp32" and model.upsample_data.precision == "fp32"
        patch.accelerate(model, sea_raft_update="bf16")
        assert model.update_block is ub and ub.precision == "bf16" and model.upsample_data.precision == "bf16"
        assert ub._engine is None
        patch.accelerate(model, sea_raft_update="fp32")
        assert ub.precision == "fp32" and model.upsample_data.precision == "fp32"
    finally:
        patch.restore(model)


# ------------------------------------------------------------------------------------------------------------- autocast golden
def test_autocast_golden_matches_restatement():
    """tests/golden/sea_raft_update_autocast.pt: the reference's own update_block / heads / upsample_data under CPU bf16 autocast
    (scripts/make_sea_raft_golden.py --autocast); the restatement reproduces it bit for bit"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    assert os.path.getsize(GOLDEN_AUTOCAST) <= 512 * 1024
    gd = torch.load(GOLDEN_AUTOCAST)
    fp = torch.load(GOLDEN)
    assert gd["autocast"] == "cpu/bfloat16" and gd["seed"] == fp["seed"]
    for k in ("net", "inp", "corr", "flow"):
        assert torch.equal(gd[k], fp[k]), k          # the same seeded step as the fp32 golden
    model = load_seeded(SeaRaftLoop(), gd["seed"]).eval()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        net_out = model.update_block(gd["net"], gd["inp"], gd["corr"], gd["flow"])
        flow_update = model.flow_head(net_out)
        weight_update = 0.25 * model.upsample_weight(net_out)
        flow_8x = gd["flow"] + flow_update[:, :2]
        info_8x = flow_update[:, 2:]
        up_flow, up_info = model.upsample_data(flow_8x, info_8x, weight_update)
    got = {"net_out": net_out, "flow_update": flow_update, "weight_update": weight_update, "flow_8x": flow_8x, "info_8x": info_8x,
           "up_flow": up_flow, "up_info": up_info}
    for k, v in got.items():
        assert v.dtype == gd[k].dtype and torch.equal(v, gd[k]), k
    # and it is a reduced-precision result: not the fp32 golden
    assert gd["net_out"].dtype == torch.bfloat16 and not torch.equal(gd["net_out"].float(), fp["net_out"])
