"""CCMR's per-scale context grouping `model.xcit[i]` on the kernels (K17, `accelerate(model, ccmr_context=True)`), the parts that need
no GPU: the C ABI of the new entries (declared, exported, ABI version unchanged, arguments validated before the device is touched), the
matcher, the fold algebra of the one-input block in float64, the fixture recorded from the reference
(tests/golden/ccmr_context.pt, scripts/make_golden_ccmr_context.py) against the stand-in, the positional rows, and `accelerate` /
`restore` on a CPU model."""
import copy
import ctypes
import os
import re

import pytest
import torch

import ptlflow_amd
from ccmr_context_refs import attention_map64, context_loop_model, load_golden, plain_layernorm64, rows_of, standin, token_rows64
from op_gate import OP_TOL, close, rel
from ptlflow_amd import patch, xcit
from xcit_model import XCiT, _xca, randomize
from xcit_refs import block_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pfk_xcit_tokens_f32", "pfk_xcit_tokens_pm_f32", "pfk_xca_fold_f32")
BAD_ARG, ALIGNMENT, UNSUPPORTED = -1, -2, -3
LL, VP, I, FL = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_float


@pytest.fixture(scope="module")
def golden():
    return load_golden()


# ---------------------------------------------------------------------------------------------------------------------
# the option: this test fails on the parent commit, where `ccmr_context` is a TypeError
# ---------------------------------------------------------------------------------------------------------------------
def test_accelerate_takes_the_option():
    import inspect
    assert inspect.signature(patch.accelerate).parameters["ccmr_context"].default is False
    assert "ccmr_context" in patch.accelerate.__doc__
    assert patch.register_xcit_context is xcit.register_xcit_context
    model = patch.accelerate(context_loop_model(), ccmr_context=True)
    assert all(isinstance(m, xcit.PfkXcitContext) for m in model.xcit)
    patch.restore(model)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not ptlflow_amd.LIBPFK_PATH.exists():
        from ptlflow_amd import _build
        _build.build_all()
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    sig = {
        # (in, pos, eps, x0, x0_ld, xh, xh_ld, B, C, H, W, stream)
        "pfk_xcit_tokens_f32": (I, [VP, VP, FL, VP, LL, VP, LL, I, I, I, I, VP]),
        # (in, in_ld, pos, eps, x0, x0_ld, xh, xh_ld, B, C, H, W, stream)
        "pfk_xcit_tokens_pm_f32": (I, [VP, LL, VP, FL, VP, LL, VP, LL, I, I, I, I, VP]),
        # (A, wv, bv, wp, bp, M, c, B, heads, dh, stream)
        "pfk_xca_fold_f32": (I, [VP, VP, VP, VP, VP, VP, VP, I, I, I, VP]),
    }
    for n, (res, args) in sig.items():
        getattr(lib, n).restype, getattr(lib, n).argtypes = res, args
    return lib


def test_header_declares_and_library_exports_the_new_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfk.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/pfk.h does not declare {n}"
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    assert lib.pfk_abi_version() == 7
    assert "#define PFK_ABI_VERSION 7" in src
    ptlflow_amd.load_native()
    for n in ("xcit_tokens", "xcit_tokens_pm", "xca_fold"):
        assert hasattr(torch.ops.pfk, n), n


# every call below is refused before a launch: the pointers are never dereferenced
A, Bp, Cp, Dp, Ep, Fp, Gp = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000


def test_tokens_validates_without_a_gpu(lib):
    def f(inp=A, pos=Ep, eps=1e-6, x0=Bp, x0_ld=128, xh=Cp, xh_ld=128, B=2, C=128, H=7, W=10):
        return lib.pfk_xcit_tokens_f32(inp, pos, eps, x0, x0_ld, xh, xh_ld, B, C, H, W, None)
    assert f(inp=None) == BAD_ARG and f(x0=None) == BAD_ARG and f(xh=None) == BAD_ARG
    assert f(B=0) == BAD_ARG and f(H=0) == BAD_ARG and f(W=0) == BAD_ARG and f(B=-1) == BAD_ARG and f(C=0) == BAD_ARG
    assert f(x0_ld=124) == BAD_ARG and f(xh_ld=124) == BAD_ARG and f(eps=-1.0) == BAD_ARG
    assert f(C=64) == UNSUPPORTED and f(C=256, x0_ld=256, xh_ld=256) == UNSUPPORTED
    assert f(C=126) == ALIGNMENT and f(x0_ld=130) == ALIGNMENT and f(xh_ld=130) == ALIGNMENT
    assert f(x0=Bp + 4) == ALIGNMENT and f(xh=Cp + 8) == ALIGNMENT and f(pos=Ep + 4) == ALIGNMENT
    assert f(xh=Bp) == BAD_ARG and f(x0=A) == BAD_ARG and f(xh=A + 64) == BAD_ARG and f(x0=Ep) == BAD_ARG      # nothing overlaps
    # pos is optional; 132 and 160 are row strides like any other

    def g(inp=A, in_ld=128, pos=Ep, eps=1e-6, x0=Bp, x0_ld=128, xh=Cp, xh_ld=128, B=2, C=128, H=7, W=10):
        return lib.pfk_xcit_tokens_pm_f32(inp, in_ld, pos, eps, x0, x0_ld, xh, xh_ld, B, C, H, W, None)
    assert g(inp=None) == BAD_ARG and g(x0=None) == BAD_ARG and g(xh=None) == BAD_ARG and g(in_ld=124) == BAD_ARG
    assert g(B=0) == BAD_ARG and g(H=0) == BAD_ARG and g(W=0) == BAD_ARG and g(x0_ld=124) == BAD_ARG and g(xh_ld=124) == BAD_ARG
    assert g(C=64, in_ld=64) == UNSUPPORTED
    assert g(in_ld=130) == ALIGNMENT and g(inp=A + 4) == ALIGNMENT and g(x0_ld=130) == ALIGNMENT
    assert g(x0=A) == BAD_ARG and g(xh=Bp) == BAD_ARG


def test_xca_fold_validates_without_a_gpu(lib):
    def f(a=A, wv=Bp, bv=Cp, wp=Dp, bp=Ep, M=Fp, c=Gp, B=2, heads=8, dh=16):
        return lib.pfk_xca_fold_f32(a, wv, bv, wp, bp, M, c, B, heads, dh, None)
    for k in ("a", "wv", "bv", "wp", "bp", "M", "c"):
        assert f(**{k: None}) == BAD_ARG, k
    assert f(B=0) == BAD_ARG and f(heads=0) == BAD_ARG and f(dh=0) == BAD_ARG
    assert f(heads=4, dh=32) == UNSUPPORTED and f(heads=8, dh=8) == UNSUPPORTED and f(heads=16, dh=16) == UNSUPPORTED
    for k, v in (("a", A), ("wv", Bp), ("bv", Cp), ("wp", Dp), ("bp", Ep), ("M", Fp), ("c", Gp)):
        assert f(**{k: v + 4}) == ALIGNMENT, k
    assert f(M=A) == BAD_ARG and f(c=Bp) == BAD_ARG and f(c=Fp + 64) == BAD_ARG and f(M=Dp) == BAD_ARG      # outputs overlap nothing


# ---------------------------------------------------------------------------------------------------------------------
# the matcher
# ---------------------------------------------------------------------------------------------------------------------
def test_matcher_accepts_the_standin_and_refuses_everything_else(golden):
    ok = standin(golden)
    assert xcit.match_xcit_context(ok) and not xcit.match_xcit_aggregator(ok)
    assert xcit.match_xcit_context(randomize(XCiT(separate=False, use_pos=False)).eval())
    assert {k: tuple(v.shape) for k, v in ok.state_dict().items()} == xcit.xcit_shapes(separate=False)
    sh = xcit.xcit_shapes(separate=False)
    assert sh["blocks.0.attn.qkv.weight"] == (384, 128) and sh["blocks.0.attn.qkv.bias"] == (384,)
    assert not any("to_qk" in k or "to_v" in k for k in sh)
    assert not xcit.match_xcit_context(XCiT(separate=True))
    assert not xcit.match_xcit_context(XCiT(depth=2, separate=False))
    assert not xcit.match_xcit_context(XCiT(num_heads=4, separate=False))
    assert not xcit.match_xcit_context(XCiT(separate=False, eps=1e-5))
    assert not xcit.match_xcit_context(XCiT(separate=False, qkv_bias=False))
    assert not xcit.match_xcit_context(XCiT(separate=False, mlp_ratio=4))
    assert not xcit.match_xcit_context(XCiT(separate=False).half())
    one = XCiT(separate=False)
    one.blocks[0].norm2.half()                                    # a single non-fp32 parameter
    assert not xcit.match_xcit_context(one)
    gn = XCiT(separate=False)
    gn.blocks[0].local_mp.bn = torch.nn.GroupNorm(4, 128)
    assert not xcit.match_xcit_context(gn)
    # the aggregator's matcher is what it was
    assert xcit.match_xcit_aggregator(XCiT(separate=True)) and xcit.xcit_shapes() == xcit.xcit_shapes(separate=True)
    # the class is the caller's to check: the reference's class is served, the stand-in's once registered
    assert xcit.served_context(type("XCiT", (torch.nn.Module,), {"__module__": "ptlflow.models.ccmr.xcit"})())
    assert not xcit.served_context(torch.nn.Identity())


# ---------------------------------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_pos", [True, False])
def test_fold_from_the_qkv_split_is_the_attention_branch_in_float64(use_pos):
    B, H, W = 2, 5, 7
    m = randomize(XCiT(separate=False, use_pos=use_pos), 17).double().eval()
    inp = torch.randn(B, 128, H, W, generator=torch.Generator().manual_seed(19), dtype=torch.float64)
    with torch.no_grad():
        m(inp)
        x0 = token_rows64(m, inp)
        M, c = xcit.fold_attention(attention_map64(m, x0), xcit.split_qkv(block_params(m)))
        x1 = x0 + plain_layernorm64(x0) @ M.transpose(1, 2) + c[:, None, :]
    r = rel(x1, m.blocks[0].last["x1"])
    print(f"fold (use_pos={use_pos}): relL2 {r:.2e}")
    assert r <= 1e-12
    assert not torch.allclose(M[0], M[1])


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
def test_standin_reproduces_the_golden_outputs(golden):
    m = standin(golden)
    seen = {}
    blk = m.blocks[0]
    h = blk.attn.register_forward_pre_hook(lambda _m, i: seen.setdefault("ln1", i[0].detach().clone()))
    with torch.no_grad():
        got = m(golden["inp"])
        h.remove()
        close(got, golden["out"])
        assert rel(got, golden["out64"]) <= OP_TOL
        B, N, Cc = seen["ln1"].shape
        q, k, v = blk.attn.qkv(seen["ln1"]).reshape(B, N, 3, 8, Cc // 8).permute(2, 0, 3, 4, 1)
        close(_xca(q, k, v, blk.attn.temperature)[1], golden["A"])
        close(blk.last["x1"], golden["x1"])
        close(blk.last["x2"], golden["x2"])
    assert tuple(golden["shape"]) == (2, 7, 10) and os.path.getsize(os.path.join(ROOT, "tests", "golden", "ccmr_context.pt")) < 1 << 20
    for t in list(golden["state_dict"].values()) + [golden["inp"]]:
        assert torch.equal(t.to(torch.bfloat16).float(), t)          # parameters and input on the bfloat16 grid


# ---------------------------------------------------------------------------------------------------------------------
# the positional rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 7, 10), (3, 4, 6), (8, 28, 64)])
def test_one_images_positional_rows_are_every_images(golden, B, H, W):
    eng = xcit.XcitContextEngine(standin(golden), torch.device("cpu"))
    one = eng.pos_rows(H, W)
    every = eng._pos_rows(B, H, W).reshape(B, H * W, 128)
    assert one.shape == (H * W, 128) and one.dtype == torch.float32
    for b in range(B):
        assert torch.equal(every[b].view(torch.int32), one.view(torch.int32)), f"image {b}"
    # and they are the module's own encoding
    with torch.no_grad():
        want = eng.module.pos_embeder(B, H, W, torch.float32).permute(0, 2, 3, 1).reshape(B, H * W, 128)
    assert torch.equal(want, every)
    eng.pack()
    assert eng._pos == {}                                          # dropped on repack


# ---------------------------------------------------------------------------------------------------------------------
# accelerate / restore on a CPU model
# ---------------------------------------------------------------------------------------------------------------------
def _images(seed=5):
    return torch.rand(1, 2, 3, 64, 96, generator=torch.Generator().manual_seed(seed))


def test_accelerate_on_a_cpu_model_installs_wrappers_that_fall_back():
    model = context_loop_model((1, 2, 1))
    mods = list(model.xcit)
    keys = list(model.state_dict().keys())
    x = _images()
    with torch.no_grad():
        want = model({"images": x})
    patch.accelerate(model, ccmr_context=True, update_block=False)      # (the update block's wrapper has no CPU path)
    assert all(isinstance(m, xcit.PfkXcitContext) for m in model.xcit)
    assert [m._ref[0] for m in model.xcit] == mods
    assert list(model.state_dict().keys()) == keys
    with torch.no_grad():
        got = model({"images": x})
    assert [(m.engine_calls, m.fallback_calls) for m in model.xcit] == [(0, 1)] * 3
    for k in ("flows", "flow_small"):
        assert torch.equal(got[k], want[k]), k
    inp = torch.relu(torch.randn(2, 128, 4, 6, generator=torch.Generator().manual_seed(3)))
    with torch.no_grad():
        for m, ref in zip(model.xcit, mods):
            assert torch.equal(m(inp), ref(inp))
    assert all(m.fallback_calls == 2 and m._engine is None for m in model.xcit)
    # .train() / .eval() reach the module the wrapper calls
    model.train()
    with torch.no_grad():
        model.xcit[0](inp)
    assert mods[0].training
    model.eval()
    # a second call switches it
    patch.accelerate(model, ccmr_context=False)
    assert list(model.xcit) == mods and list(model.state_dict().keys()) == keys
    patch.accelerate(model, ccmr_context=True)
    assert all(isinstance(m, xcit.PfkXcitContext) for m in model.xcit)
    patch.accelerate(model, ccmr_context=True)                    # and a third installs nothing twice
    assert [m._ref[0] for m in model.xcit] == mods
    patch.restore(model)
    assert list(model.xcit) == mods and list(model.state_dict().keys()) == keys
    # the default leaves the modules alone
    patch.accelerate(model)
    assert list(model.xcit) == mods
    patch.restore(model)


def test_one_module_that_does_not_match_means_no_wrapper_at_all():
    model = context_loop_model((1, 2, 1))
    model.xcit[1].blocks[0].local_mp.bn = torch.nn.GroupNorm(4, 128)
    mods = list(model.xcit)
    patch.accelerate(model, ccmr_context=True)
    assert list(model.xcit) == mods
    patch.restore(model)
    # a class nobody registered is not served either, whatever its state_dict says
    class Other(XCiT):
        pass
    other = context_loop_model((1, 2, 1))
    other.xcit[2] = randomize(Other(separate=False), 5).eval()
    mods = list(other.xcit)
    patch.accelerate(other, ccmr_context=True)
    assert list(other.xcit) == mods
    patch.restore(other)
    # a model without `xcit` (or with the stand-in's gates) takes the option and gets nothing
    from ms_loop_model import MsLoopModel
    plain = MsLoopModel("ccmr", (1, 2, 1)).eval()
    gates = list(plain.xcit)
    patch.accelerate(plain, ccmr_context=True)
    assert list(plain.xcit) == gates
    patch.restore(plain)
    patch.restore(patch.accelerate(MsLoopModel("ms_raft", (1, 2, 1)).eval(), ccmr_context=True))


def test_deepcopy_of_a_wrapped_model_keeps_working():
    model = patch.accelerate(context_loop_model((1, 2, 1)), ccmr_context=True)
    twin = copy.deepcopy(model)
    inp = torch.relu(torch.randn(1, 128, 3, 5, generator=torch.Generator().manual_seed(9)))
    with torch.no_grad():
        assert torch.equal(twin.xcit[0](inp), model.xcit[0](inp))
    patch.restore(model)
