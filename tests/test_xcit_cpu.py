"""CCMR's XCiT motion aggregator on the kernels (K14), the parts that need no GPU: the torch stand-in tests/xcit_model.py against the
fixture recorded from the reference (tests/golden/ccmr_aggregator.pt, scripts/make_golden_ccmr_aggregator.py), the host algebra
`xcit.fold_attention` in float64, the matcher, and the C ABI of the new entries (declared, exported, ABI version unchanged,
arguments validated before the device is touched)."""
import ctypes
import os
import re

import pytest
import torch

import ptlflow_amd
from oracle import ref_loader
from op_gate import OP_TOL, close, rel
from ptlflow_amd import xcit
from xcit_model import XCiT, randomize
from xcit_refs import block_params, layernorm_ref, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pfk_layernorm_rows_f32", "pfk_xca_map_f32", "pfk_xca_map_workspace_bytes", "pfk_xcit_lpi1_f32", "pfk_xcit_lpi2_f32",
       "pfk_xcit_lpi_workspace_bytes")
BAD_ARG, ALIGNMENT, UNSUPPORTED = -1, -2, -3
LL, VP, I, FL = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_float


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def standin(golden, dtype=torch.float32):
    m = XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=True).to(dtype).eval()
    m.load_state_dict({k: v.to(dtype) for k, v in golden["state_dict"].items()})
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the stand-in is the reference's module
# ---------------------------------------------------------------------------------------------------------------------
def test_standin_reproduces_the_golden_outputs(golden):
    m = standin(golden)
    with torch.no_grad():
        for mf, out, out64 in zip(golden["motion_features"], golden["out"], golden["out64"]):
            got = m(golden["global_context"], mf)
            close(got, out)
            assert rel(got, out64) <= OP_TOL
        m(golden["global_context"], golden["motion_features"][0])
        close(m.blocks[0].attn.last_attn, golden["A"])
        close(m.blocks[0].last["x1"], golden["x1"])
        close(m.blocks[0].last["x2"], golden["x2"])
    assert not torch.equal(golden["out"][0], golden["out"][1])


def test_standin_has_the_references_state_dict():
    if not ref_loader.reference_available() or not ref_loader.ensure_family("ccmr"):
        pytest.skip("no reference tree on this machine")
    ref = ref_loader.ref_module("ptlflow.models.ccmr.xcit").XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=True)
    mine = XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=True)
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}  # noqa: E731
    assert shapes(mine) == shapes(ref) == xcit.xcit_shapes()
    assert xcit.match_xcit_aggregator(ref.eval())


# ---------------------------------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------------------------------
def test_fold_attention_gives_the_golden_x1_in_float64(golden):
    B, H, W = golden["shape"]
    m = standin(golden, torch.float64)
    with torch.no_grad():
        x0 = golden["global_context"].double().flatten(2).transpose(1, 2)
        x0 = x0 + m.pos_embeder(B, H, W, torch.float64).reshape(B, -1, H * W).permute(0, 2, 1)
        M, c = xcit.fold_attention(golden["A"].double(), block_params(m))
        assert M.shape == (B, 128, 128) and c.shape == (B, 128) and M.dtype == torch.float64 and M.device.type == "cpu"
        xh = layernorm_ref(golden["motion_features"][0].double().flatten(2).transpose(1, 2))
        x1 = x0 + xh @ M.transpose(1, 2) + c[:, None, :]
    r = rel(x1, golden["x1"])
    print(f"fold: relL2 {r:.2e}")
    assert r <= OP_TOL
    assert not torch.allclose(M[0], M[1])          # the map, hence the fold, is per image


# ---------------------------------------------------------------------------------------------------------------------
# the matcher
# ---------------------------------------------------------------------------------------------------------------------
def test_matcher_accepts_the_standin_and_refuses_everything_else(golden):
    ok = standin(golden)
    assert xcit.match_xcit_aggregator(ok)
    assert xcit.match_xcit_aggregator(randomize(XCiT(separate=True, use_pos=False)).eval())
    assert not xcit.match_xcit_aggregator(XCiT(depth=2, separate=False))
    assert not xcit.match_xcit_aggregator(XCiT(depth=1, separate=False))
    two = XCiT(separate=True)
    two.blocks.append(XCiT(separate=True).blocks[0])
    assert not xcit.match_xcit_aggregator(two)
    assert not xcit.match_xcit_aggregator(XCiT(num_heads=4, separate=True))
    assert not xcit.match_xcit_aggregator(XCiT(separate=True, eps=1e-5))
    assert not xcit.match_xcit_aggregator(XCiT(separate=True, mlp_ratio=4))
    assert not xcit.match_xcit_aggregator(XCiT(separate=True, qkv_bias=False))
    assert not xcit.match_xcit_aggregator(XCiT(separate=True).half())
    gn = XCiT(separate=True)
    gn.blocks[0].local_mp.bn = torch.nn.GroupNorm(4, 128)
    assert not xcit.match_xcit_aggregator(gn)
    # the class is the caller's to check: served only once registered
    assert not xcit.served(ok)
    assert xcit.served(type("XCiT", (torch.nn.Module,), {"__module__": "ptlflow.models.ccmr.xcit"})())


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
        # (in, in_ld, weight, bias, eps, out, out_ld, M, C, stream)
        "pfk_layernorm_rows_f32": (I, [VP, LL, VP, VP, FL, VP, LL, LL, I, VP]),
        "pfk_xca_map_workspace_bytes": (LL, [I, LL, I, I]),
        # (qk, qk_ld, temperature, A, ws, ws_bytes, B, N, heads, dh, stream)
        "pfk_xca_map_f32": (I, [VP, LL, VP, VP, VP, LL, I, LL, I, I, VP]),
        "pfk_xcit_lpi_workspace_bytes": (LL, [I, I, I]),
        # (x, x_ld, ln_w, ln_b, ln_eps, dw_w, dw_b, u, u_ld, ws, ws_bytes, B, H, W, C, stream)
        "pfk_xcit_lpi1_f32": (I, [VP, LL, VP, VP, FL, VP, VP, VP, LL, VP, LL, I, I, I, I, VP]),
        # (u, u_ld, gn_w, gn_b, gn_eps, groups, dw_w, dw_b, gamma, x, x_ld, x2, x2_ld, ln_w, ln_b, ln_eps, t, t_ld, ws, ws_bytes, B, H, W, C, stream)
        "pfk_xcit_lpi2_f32": (I, [VP, LL, VP, VP, FL, I, VP, VP, VP, VP, LL, VP, LL, VP, VP, FL, VP, LL, VP, LL, I, I, I, I, VP]),
    }
    for n, (res, args) in sig.items():
        getattr(lib, n).restype, getattr(lib, n).argtypes = res, args
    return lib


def test_header_declares_and_library_exports_the_new_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfk.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/pfk.h does not declare {n}"
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    for n in sorted(set(re.findall(r"\b(pfk_[a-z0-9_]+)\s*\(", src))):
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    assert lib.pfk_abi_version() == 7
    assert "#define PFK_ABI_VERSION 7" in src
    ptlflow_amd.load_native()
    for n in ("layernorm_rows", "xca_map", "xcit_lpi_workspace_bytes", "xcit_lpi1", "xcit_lpi2"):
        assert hasattr(torch.ops.pfk, n), n


# every call below is refused before a launch: the pointers are never dereferenced
A, Bp, Cp, Dp, Ep, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x700000
BIG = 1 << 40


def test_layernorm_rows_validates_without_a_gpu(lib):
    def f(inp=A, in_ld=128, w=Ep, b=Ep, eps=1e-6, out=Bp, out_ld=128, M=8, C=128):
        return lib.pfk_layernorm_rows_f32(inp, in_ld, w, b, eps, out, out_ld, M, C, None)
    assert f(inp=None) == BAD_ARG and f(out=None) == BAD_ARG and f(M=0) == BAD_ARG and f(C=0) == BAD_ARG
    assert f(in_ld=124) == BAD_ARG and f(out_ld=124) == BAD_ARG and f(eps=-1.0) == BAD_ARG
    assert f(C=6, in_ld=8, out_ld=8) == ALIGNMENT and f(in_ld=130) == ALIGNMENT and f(out_ld=130) == ALIGNMENT
    assert f(inp=A + 4) == ALIGNMENT and f(out=Bp + 8) == ALIGNMENT and f(w=Ep + 4) == ALIGNMENT and f(b=Ep + 4) == ALIGNMENT
    assert f(C=516, in_ld=516, out_ld=516) == UNSUPPORTED
    assert f(out=A + 64) == BAD_ARG and f(out=A, out_ld=132) == BAD_ARG          # partial overlap; in place needs the same ld


def test_xca_map_validates_without_a_gpu(lib):
    def f(qk=A, qk_ld=256, temp=Ep, out=Bp, ws=WS, ws_bytes=BIG, B=2, N=70, heads=8, dh=16):
        return lib.pfk_xca_map_f32(qk, qk_ld, temp, out, ws, ws_bytes, B, N, heads, dh, None)
    assert f(qk=None) == BAD_ARG and f(temp=None) == BAD_ARG and f(out=None) == BAD_ARG and f(ws=None) == BAD_ARG
    assert f(B=0) == BAD_ARG and f(N=0) == BAD_ARG and f(heads=0) == BAD_ARG and f(dh=0) == BAD_ARG and f(qk_ld=252) == BAD_ARG
    assert f(heads=4, dh=32) == UNSUPPORTED and f(heads=16, dh=8) == UNSUPPORTED and f(heads=8, dh=8) == UNSUPPORTED
    assert f(qk_ld=258) == ALIGNMENT and f(qk=A + 4) == ALIGNMENT and f(out=Bp + 4) == ALIGNMENT and f(ws=WS + 8) == ALIGNMENT
    need = lib.pfk_xca_map_workspace_bytes(2, 70, 8, 16)
    assert need == 2 * 1 * (2048 + 256) * 4          # per image and 256-token chunk: the Gram and both squared norms
    assert f(ws_bytes=need - 1) == BAD_ARG
    assert lib.pfk_xca_map_workspace_bytes(1, 28 * 64, 8, 16) == 7 * 2304 * 4          # one partial per 256 tokens
    assert lib.pfk_xca_map_workspace_bytes(1, 70, 4, 32) == UNSUPPORTED and lib.pfk_xca_map_workspace_bytes(0, 70, 8, 16) == BAD_ARG
    assert f(out=A) == BAD_ARG and f(ws=A) == BAD_ARG and f(ws=Bp, ws_bytes=need) == BAD_ARG      # nothing overlaps


def test_lpi_entries_validate_without_a_gpu(lib):
    need = lib.pfk_xcit_lpi_workspace_bytes(2, 7, 10)
    assert need == 2 * (2 * 2) * 16 * 8 + 2 * 16 * 4          # a double partial per block, group and moment + mean | rstd per image
    assert lib.pfk_xcit_lpi_workspace_bytes(0, 7, 10) == BAD_ARG

    def f1(x=A, x_ld=128, lw=Ep, lb=Ep, dw=Ep, db=Ep, u=Bp, u_ld=128, ws=WS, ws_bytes=BIG, B=2, H=7, W=10, C=128):
        return lib.pfk_xcit_lpi1_f32(x, x_ld, lw, lb, 1e-6, dw, db, u, u_ld, ws, ws_bytes, B, H, W, C, None)
    assert f1(x=None) == BAD_ARG and f1(lw=None) == BAD_ARG and f1(lb=None) == BAD_ARG and f1(dw=None) == BAD_ARG
    assert f1(db=None) == BAD_ARG and f1(u=None) == BAD_ARG and f1(ws=None) == BAD_ARG
    assert f1(B=0) == BAD_ARG and f1(H=0) == BAD_ARG and f1(W=0) == BAD_ARG and f1(C=0) == BAD_ARG
    assert f1(x_ld=124) == BAD_ARG and f1(u_ld=124) == BAD_ARG and f1(ws_bytes=need - 1) == BAD_ARG
    assert f1(C=64, x_ld=64, u_ld=64) == UNSUPPORTED and f1(C=256, x_ld=256, u_ld=256) == UNSUPPORTED
    assert f1(C=126) == ALIGNMENT and f1(x_ld=130) == ALIGNMENT and f1(u_ld=130) == ALIGNMENT
    assert f1(x=A + 4) == ALIGNMENT and f1(u=Bp + 8) == ALIGNMENT and f1(ws=WS + 8) == ALIGNMENT and f1(lw=Ep + 4) == ALIGNMENT
    assert f1(u=A) == BAD_ARG and f1(u=A + 128 * 4 * 16) == BAD_ARG and f1(ws=A, ws_bytes=need) == BAD_ARG     # the halo is read: out of place

    def f2(u=A, u_ld=128, gw=Ep, gb=Ep, groups=8, dw=Ep, db=Ep, gm=Ep, x=Bp, x_ld=128, x2=Cp, x2_ld=128, lw=Ep, lb=Ep, t=Dp, t_ld=128,
           ws=WS, ws_bytes=BIG, B=2, H=7, W=10, C=128):
        return lib.pfk_xcit_lpi2_f32(u, u_ld, gw, gb, 1e-5, groups, dw, db, gm, x, x_ld, x2, x2_ld, lw, lb, 1e-6, t, t_ld, ws, ws_bytes,
                                     B, H, W, C, None)
    assert f2(u=None) == BAD_ARG and f2(gw=None) == BAD_ARG and f2(gb=None) == BAD_ARG and f2(dw=None) == BAD_ARG
    assert f2(db=None) == BAD_ARG and f2(gm=None) == BAD_ARG and f2(x=None) == BAD_ARG and f2(x2=None) == BAD_ARG
    assert f2(t=None) == BAD_ARG and f2(ws=None) == BAD_ARG and f2(groups=0) == BAD_ARG
    assert f2(B=0) == BAD_ARG and f2(H=0) == BAD_ARG and f2(W=0) == BAD_ARG and f2(C=0) == BAD_ARG
    assert f2(u_ld=124) == BAD_ARG and f2(x_ld=124) == BAD_ARG and f2(x2_ld=124) == BAD_ARG and f2(t_ld=124) == BAD_ARG
    assert f2(ws_bytes=need - 1) == BAD_ARG
    assert f2(groups=4) == UNSUPPORTED and f2(groups=16) == UNSUPPORTED
    assert f2(C=64, u_ld=64, x_ld=64, x2_ld=64, t_ld=64) == UNSUPPORTED
    assert f2(u_ld=130) == ALIGNMENT and f2(x_ld=130) == ALIGNMENT and f2(x2_ld=130) == ALIGNMENT and f2(t_ld=130) == ALIGNMENT
    assert f2(u=A + 4) == ALIGNMENT and f2(x=Bp + 4) == ALIGNMENT and f2(x2=Cp + 8) == ALIGNMENT and f2(t=Dp + 4) == ALIGNMENT
    assert f2(gm=Ep + 4) == ALIGNMENT and f2(lw=Ep + 8) == ALIGNMENT and f2(ws=WS + 4) == ALIGNMENT
    assert f2(x2=A) == BAD_ARG and f2(t=A) == BAD_ARG and f2(t=Cp) == BAD_ARG and f2(x2=Bp) == BAD_ARG and f2(t=Bp) == BAD_ARG
    assert f2(ws=Cp, ws_bytes=need) == BAD_ARG


def test_accelerate_takes_the_option_and_builds_no_engine_without_it():
    import inspect
    from ptlflow_amd import patch
    assert inspect.signature(patch.accelerate).parameters["ccmr_aggregator"].default is False
    assert "ccmr_aggregator" in patch.accelerate.__doc__
    assert patch.register_xcit_aggregator is xcit.register_xcit_aggregator
