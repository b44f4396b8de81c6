"""Training SEA-RAFT's ConvNeXt block on bf16 rows (K12f), the parts that need no GPU: the C ABI of the five `_b16` entries (declared,
exported, ABI version unchanged, arguments validated before the device is touched, in tests/test_sea_train_cpu.py's pattern) and how
`accelerate` routes `train_precision` to the SEA-RAFT seams."""
import ctypes
import os
import re

import pytest
import torch

import ptlflow_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pfk_dwconv_layernorm_train_b16", "pfk_layernorm_bwd_b16", "pfk_dwconv_bwd_b16", "pfk_gelu_b16", "pfk_gelu_bwd_b16")
OPS = ("dwconv_layernorm_train_b16", "layernorm_bwd_b16", "dwconv_bwd_b16", "gelu_b16", "gelu_bwd_b16")
BAD_ARG, ALIGNMENT = -1, -2
LL, VP, I, FL = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_float


@pytest.fixture(scope="module")
def lib():
    if not ptlflow_amd.LIBPFK_PATH.exists():
        from ptlflow_amd import _build
        _build.build_all()
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    sig = {
        # (in, in_ld, dw_w, dw_b, ln_w, ln_b, eps, out, out_ld, xhat, xhat_ld, rstd, B, H, W, C, k, stream)
        "pfk_dwconv_layernorm_train_b16": (I, [VP, I, VP, VP, VP, VP, FL, VP, I, VP, I, VP, I, I, I, I, I, VP]),
        # (xhat, xhat_ld, rstd, ln_w, dy, dy_ld, du, du_ld, dgamma, dbeta, ws, ws_bytes, M, C, stream)
        "pfk_layernorm_bwd_b16": (I, [VP, I, VP, VP, VP, I, VP, I, VP, VP, VP, LL, LL, I, VP]),
        "pfk_layernorm_bwd_workspace_bytes": (LL, [LL, I]),
        # (in, in_ld, du, du_ld, dw_w, dx, dx_ld, dweight, dbias, ws, ws_bytes, B, H, W, C, k, stream)
        "pfk_dwconv_bwd_b16": (I, [VP, I, VP, I, VP, VP, I, VP, VP, VP, LL, I, I, I, I, I, VP]),
        "pfk_dwconv_bwd_workspace_bytes": (LL, [I, I, I, I, I]),
        "pfk_gelu_b16": (I, [VP, LL, VP, LL, LL, I, VP]),
        "pfk_gelu_bwd_b16": (I, [VP, LL, VP, LL, VP, LL, LL, I, VP]),
    }
    for n in sig:
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    for n, (res, args) in sig.items():
        getattr(lib, n).restype, getattr(lib, n).argtypes = res, args
    return lib


def test_header_declares_and_library_exports_the_b16_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfk.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/pfk.h does not declare {n}"
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    assert lib.pfk_abi_version() == 7
    assert "#define PFK_ABI_VERSION 7" in src
    ptlflow_amd.load_native()
    for n in OPS:
        assert hasattr(torch.ops.pfk, n), n


# every call below is refused before a launch: the pointers are never dereferenced.  bf16 rows: C % 8, ld % 8, 16-byte aligned
A, Bp, Cp, Dp, Ep, Fp, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
BIG = 1 << 40


def test_train_forward_validates_without_a_gpu(lib):
    def f(in_ld=384, out_ld=384, xhat_ld=384, C=384, k=7, inp=A, out=Bp, xhat=Cp, rstd=Dp, lw=Ep):
        return lib.pfk_dwconv_layernorm_train_b16(inp, in_ld, Ep, Ep, lw, Ep, 1e-6, out, out_ld, xhat, xhat_ld, rstd, 1, 4, 8, C, k, None)
    assert f(C=0) == BAD_ARG and f(C=4, in_ld=8, out_ld=8, xhat_ld=8) == BAD_ARG and f(C=520, in_ld=520, out_ld=520, xhat_ld=520) == BAD_ARG
    assert f(k=9) == BAD_ARG and f(k=4) == BAD_ARG and f(k=0) == BAD_ARG
    assert f(in_ld=376) == BAD_ARG and f(out_ld=376) == BAD_ARG and f(xhat_ld=376) == BAD_ARG
    assert f(xhat=None) == BAD_ARG and f(rstd=None) == BAD_ARG and f(inp=None) == BAD_ARG and f(out=None) == BAD_ARG and f(lw=None) == BAD_ARG
    assert f(C=12, in_ld=16, out_ld=16, xhat_ld=16) == ALIGNMENT                                    # C % 8
    assert f(in_ld=388) == ALIGNMENT and f(out_ld=388) == ALIGNMENT and f(xhat_ld=388) == ALIGNMENT  # ld % 8 (a legal fp32 stride)
    assert f(inp=A + 8) == ALIGNMENT and f(out=Bp + 8) == ALIGNMENT and f(xhat=Cp + 8) == ALIGNMENT and f(rstd=Dp + 2) == ALIGNMENT
    assert f(out=A) == BAD_ARG and f(xhat=A) == BAD_ARG and f(xhat=Bp) == BAD_ARG                    # outputs over the input / each other
    assert f(rstd=A) == BAD_ARG and f(rstd=Bp + 64) == BAD_ARG and f(rstd=Cp) == BAD_ARG


def test_layernorm_bwd_validates_without_a_gpu(lib):
    def f(xhat_ld=384, dy_ld=384, du_ld=384, C=384, M=32, xhat=A, dy=Bp, du=Cp, ws=WS, ws_bytes=BIG, dg=Dp, rstd=Ep):
        return lib.pfk_layernorm_bwd_b16(xhat, xhat_ld, rstd, Ep, dy, dy_ld, du, du_ld, dg, Fp, ws, ws_bytes, M, C, None)
    assert f(C=0) == BAD_ARG and f(C=520, xhat_ld=520, dy_ld=520, du_ld=520) == BAD_ARG and f(M=0) == BAD_ARG
    assert f(C=12, xhat_ld=16, dy_ld=16, du_ld=16) == BAD_ARG and f(C=4, xhat_ld=8, dy_ld=8, du_ld=8) == BAD_ARG      # C % 8, C < 8
    assert f(xhat_ld=376) == BAD_ARG and f(dy_ld=376) == BAD_ARG and f(du_ld=376) == BAD_ARG
    assert f(xhat=None) == BAD_ARG and f(dy=None) == BAD_ARG and f(du=None) == BAD_ARG and f(rstd=None) == BAD_ARG
    assert f(dg=None) == BAD_ARG and f(ws=None) == BAD_ARG
    assert f(ws_bytes=lib.pfk_layernorm_bwd_workspace_bytes(32, 384) - 1) == BAD_ARG
    assert f(xhat_ld=388) == ALIGNMENT and f(dy_ld=388) == ALIGNMENT and f(du_ld=388) == ALIGNMENT
    assert f(xhat=A + 8) == ALIGNMENT and f(dy=Bp + 8) == ALIGNMENT and f(du=Cp + 4) == ALIGNMENT and f(ws=WS + 4) == ALIGNMENT
    assert f(du=Bp) == BAD_ARG and f(du=A) == BAD_ARG                                      # out of place only
    assert f(du=Bp + 31 * 384 * 2) == BAD_ARG and f(du=A - 31 * 384 * 2) == BAD_ARG        # the last / first row only


def test_dwconv_bwd_validates_without_a_gpu(lib):
    def f(in_ld=384, du_ld=384, dx_ld=384, C=384, k=7, inp=A, du=Bp, dx=Cp, ws=WS, ws_bytes=BIG, dw=Dp, w=Ep):
        return lib.pfk_dwconv_bwd_b16(inp, in_ld, du, du_ld, w, dx, dx_ld, dw, Fp, ws, ws_bytes, 1, 4, 8, C, k, None)
    assert f(C=0) == BAD_ARG and f(C=520, in_ld=520, du_ld=520, dx_ld=520) == BAD_ARG
    assert f(C=12, in_ld=16, du_ld=16, dx_ld=16) == BAD_ARG and f(C=4, in_ld=8, du_ld=8, dx_ld=8) == BAD_ARG
    assert f(k=9) == BAD_ARG and f(k=2) == BAD_ARG and f(k=0) == BAD_ARG
    assert f(in_ld=376) == BAD_ARG and f(du_ld=376) == BAD_ARG and f(dx_ld=376) == BAD_ARG
    assert f(inp=None) == BAD_ARG and f(du=None) == BAD_ARG and f(dx=None) == BAD_ARG and f(w=None) == BAD_ARG
    assert f(dw=None) == BAD_ARG and f(ws=None) == BAD_ARG
    assert f(ws_bytes=lib.pfk_dwconv_bwd_workspace_bytes(1, 4, 8, 384, 7) - 1) == BAD_ARG
    assert f(in_ld=388) == ALIGNMENT and f(du_ld=388) == ALIGNMENT and f(dx_ld=388) == ALIGNMENT
    assert f(inp=A + 8) == ALIGNMENT and f(du=Bp + 4) == ALIGNMENT and f(dx=Cp + 8) == ALIGNMENT and f(ws=WS + 8) == ALIGNMENT
    assert f(dx=Bp) == BAD_ARG and f(dx=A) == BAD_ARG and f(dx=A + 31 * 384 * 2) == BAD_ARG


def test_gelu_validates_without_a_gpu(lib):
    fw, bw = lib.pfk_gelu_b16, lib.pfk_gelu_bwd_b16
    assert fw(None, 512, Bp, 512, 8, 512, None) == BAD_ARG and fw(A, 512, None, 512, 8, 512, None) == BAD_ARG
    assert fw(A, 512, Bp, 512, 8, 508, None) == BAD_ARG and fw(A, 512, Bp, 512, 8, 4, None) == BAD_ARG        # C % 8, C < 8
    assert fw(A, 504, Bp, 512, 8, 512, None) == BAD_ARG and fw(A, 512, Bp, 504, 8, 512, None) == BAD_ARG
    assert fw(A, 512, Bp, 512, 0, 512, None) == BAD_ARG and fw(A, 512, A, 512, 8, 512, None) == BAD_ARG
    assert fw(A + 8, 512, Bp, 512, 8, 512, None) == ALIGNMENT and fw(A, 516, Bp, 512, 8, 512, None) == ALIGNMENT
    assert fw(A, 512, Bp + 8, 512, 8, 512, None) == ALIGNMENT and fw(A, 512, Bp, 516, 8, 512, None) == ALIGNMENT
    assert bw(A, 512, None, 512, Cp, 512, 8, 512, None) == BAD_ARG and bw(A, 512, Bp, 504, Cp, 512, 8, 512, None) == BAD_ARG
    assert bw(None, 512, Bp, 512, Cp, 512, 8, 512, None) == BAD_ARG and bw(A, 512, Bp, 512, None, 512, 8, 512, None) == BAD_ARG
    assert bw(A, 512, Bp, 512, Bp, 512, 8, 512, None) == BAD_ARG and bw(A, 512, Bp, 512, A, 512, 8, 512, None) == BAD_ARG
    assert bw(A, 512, Bp, 512, Cp + 8, 512, 8, 512, None) == ALIGNMENT and bw(A, 512, Bp, 516, Cp, 512, 8, 512, None) == ALIGNMENT


def test_accelerate_routes_train_precision_to_the_sea_seams():
    from sea_seam_model import SeaRaftLoop
    from ptlflow_amd import patch
    model = SeaRaftLoop(iters=1)
    with pytest.raises(ValueError):                                          # the pinned refusal: the inference precision is not the way in
        patch.accelerate(model, sea_raft_update="bf16", sea_raft_train=True)
    with pytest.raises(ValueError):
        patch.accelerate(model, sea_raft_update="bf16", sea_raft_train=True, train_precision="bf16")
    with pytest.raises(ValueError):                                          # an unknown value, refused before anything was installed
        patch.accelerate(model, sea_raft_update=True, sea_raft_train=True, train_precision="fp16")
    assert type(model.update_block).__name__ == "BasicUpdateBlock"
    try:
        patch.accelerate(model, sea_raft_update=True, sea_raft_train=True)
        ub = model.update_block
        assert ub.sea_train and ub.train_precision == "fp32"                 # the default
        patch.accelerate(model, sea_raft_update=True, sea_raft_train=True, train_upsample=True, train_precision="bf16")
        assert model.update_block is ub and ub.sea_train and ub.train_precision == "bf16"
        assert ub.precision == "fp32"                                        # independent of the inference precision
        patch.accelerate(model, sea_raft_update="fp32", sea_raft_train=True, train_precision="fp32")      # a second call switches it
        assert ub.train_precision == "fp32" and ub.sea_train
        patch.accelerate(model, sea_raft_update=True, sea_raft_train=True, train_precision="bf16")
        with pytest.raises(ValueError):
            patch.accelerate(model, sea_raft_update=True, sea_raft_train=True, train_precision="half")
        assert ub.train_precision == "bf16"                                  # a refused call changes nothing
        assert ub.train_calls == 0 and model.flow_head.train_calls == 0 and model.upsample_weight.train_calls == 0
    finally:
        patch.restore(model)
    assert type(model.update_block).__name__ == "BasicUpdateBlock" and not hasattr(model.update_block, "train_precision")


def test_row_nodes_refuse_what_the_b16_kernels_do_not_cover():
    """argument errors of the Python faces are raised before any kernel is reached"""
    from ptlflow_amd.train_sea import dwconv_layernorm_pm, gelu_pm
    x = torch.zeros(8, 12)
    w = torch.zeros(12, 1, 7, 7)
    with pytest.raises(ValueError):
        dwconv_layernorm_pm(x, w, None, torch.ones(12), torch.zeros(12), 1, 2, 4, precision="bf16")       # C % 8
    with pytest.raises(ValueError):
        gelu_pm(x, "bf16")
    with pytest.raises(ValueError):
        gelu_pm(torch.zeros(8, 16), "fp16")
