"""Training SEA-RAFT's ConvNeXt block on the kernels (K12d), the parts that need no GPU: the C ABI of the new entries (declared,
exported, ABI version unchanged, arguments validated before the device is touched), `accelerate`'s argument errors, the formulas of
include/pfk.h restated in float64 torch against autograd, and the gradient fixture tests/golden/sea_raft_update_grad.pt (the
reference's own backward, scripts/make_sea_raft_train_golden.py) against the torch stand-in tests/sea_seam_model.py."""
import ctypes
import importlib.util
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import ptlflow_amd
from oracle import ref_loader
from op_gate import rel
from op_refs import dwconv_bwd_ref, gelu_bwd_ref, layernorm_bwd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sea_raft_update_grad.pt")
NEW = ("pfk_dwconv_layernorm_train_f32", "pfk_layernorm_bwd_f32", "pfk_layernorm_bwd_workspace_bytes", "pfk_dwconv_bwd_f32",
       "pfk_dwconv_bwd_workspace_bytes", "pfk_gelu_f32", "pfk_gelu_bwd_f32")
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
        "pfk_dwconv_layernorm_train_f32": (I, [VP, I, VP, VP, VP, VP, FL, VP, I, VP, I, VP, I, I, I, I, I, VP]),
        # (xhat, xhat_ld, rstd, ln_w, dy, dy_ld, du, du_ld, dgamma, dbeta, ws, ws_bytes, M, C, stream)
        "pfk_layernorm_bwd_f32": (I, [VP, I, VP, VP, VP, I, VP, I, VP, VP, VP, LL, LL, I, VP]),
        "pfk_layernorm_bwd_workspace_bytes": (LL, [LL, I]),
        # (in, in_ld, du, du_ld, dw_w, dx, dx_ld, dweight, dbias, ws, ws_bytes, B, H, W, C, k, stream)
        "pfk_dwconv_bwd_f32": (I, [VP, I, VP, I, VP, VP, I, VP, VP, VP, LL, I, I, I, I, I, VP]),
        "pfk_dwconv_bwd_workspace_bytes": (LL, [I, I, I, I, I]),
        "pfk_gelu_f32": (I, [VP, LL, VP, LL, LL, I, VP]),
        "pfk_gelu_bwd_f32": (I, [VP, LL, VP, LL, VP, LL, LL, I, VP]),
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
    for n in ("dwconv_layernorm_train", "layernorm_bwd", "dwconv_bwd", "gelu", "gelu_bwd"):
        assert hasattr(torch.ops.pfk, n), n


# every call below is refused before a launch: the pointers are never dereferenced
A, Bp, Cp, Dp, Ep, Fp, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
BIG = 1 << 40


def test_train_forward_validates_without_a_gpu(lib):
    def f(in_ld=384, out_ld=384, xhat_ld=384, C=384, k=7, inp=A, out=Bp, xhat=Cp, rstd=Dp):
        return lib.pfk_dwconv_layernorm_train_f32(inp, in_ld, Ep, Ep, Ep, Ep, 1e-6, out, out_ld, xhat, xhat_ld, rstd, 1, 4, 8, C, k, None)
    assert f(C=0) == BAD_ARG and f(C=516) == BAD_ARG and f(k=9) == BAD_ARG and f(k=4) == BAD_ARG
    assert f(in_ld=380) == BAD_ARG and f(out_ld=380) == BAD_ARG and f(xhat_ld=380) == BAD_ARG
    assert f(xhat=None) == BAD_ARG and f(rstd=None) == BAD_ARG and f(inp=None) == BAD_ARG
    assert f(C=6, in_ld=8, out_ld=8, xhat_ld=8) == ALIGNMENT and f(in_ld=386) == ALIGNMENT and f(inp=A + 4) == ALIGNMENT
    assert f(out=A) == BAD_ARG and f(xhat=A) == BAD_ARG and f(xhat=Bp) == BAD_ARG          # outputs over the input / each other


def test_layernorm_bwd_validates_without_a_gpu(lib):
    def f(xhat_ld=384, dy_ld=384, du_ld=384, C=384, M=32, xhat=A, dy=Bp, du=Cp, ws=WS, ws_bytes=BIG, dg=Dp):
        return lib.pfk_layernorm_bwd_f32(xhat, xhat_ld, Ep, Ep, dy, dy_ld, du, du_ld, dg, Fp, ws, ws_bytes, M, C, None)
    assert f(C=0) == BAD_ARG and f(C=516) == BAD_ARG and f(C=6, xhat_ld=8, dy_ld=8, du_ld=8) == BAD_ARG and f(M=0) == BAD_ARG
    assert f(xhat_ld=380) == BAD_ARG and f(dy_ld=380) == BAD_ARG and f(du_ld=380) == BAD_ARG
    assert f(dg=None) == BAD_ARG and f(ws=None) == BAD_ARG
    assert f(ws_bytes=lib.pfk_layernorm_bwd_workspace_bytes(32, 384) - 1) == BAD_ARG
    assert f(xhat_ld=386) == ALIGNMENT and f(dy=Bp + 8) == ALIGNMENT and f(du_ld=390) == ALIGNMENT and f(ws=WS + 4) == ALIGNMENT
    assert f(du=Bp) == BAD_ARG and f(du=A) == BAD_ARG                                      # out of place only
    assert lib.pfk_layernorm_bwd_workspace_bytes(32, 384) == 8 * 2 * 384 * 4                # one partial per block of four rows
    assert lib.pfk_layernorm_bwd_workspace_bytes(1 << 20, 384) == 1024 * 2 * 384 * 4        # ... at most 1024 blocks


def test_dwconv_bwd_validates_without_a_gpu(lib):
    def f(in_ld=384, du_ld=384, dx_ld=384, C=384, k=7, inp=A, du=Bp, dx=Cp, ws=WS, ws_bytes=BIG, dw=Dp):
        return lib.pfk_dwconv_bwd_f32(inp, in_ld, du, du_ld, Ep, dx, dx_ld, dw, Fp, ws, ws_bytes, 1, 4, 8, C, k, None)
    assert f(C=0) == BAD_ARG and f(C=516) == BAD_ARG and f(C=6, in_ld=8, du_ld=8, dx_ld=8) == BAD_ARG
    assert f(k=9) == BAD_ARG and f(k=2) == BAD_ARG and f(k=0) == BAD_ARG
    assert f(in_ld=380) == BAD_ARG and f(du_ld=380) == BAD_ARG and f(dx_ld=380) == BAD_ARG
    assert f(dw=None) == BAD_ARG and f(ws=None) == BAD_ARG
    assert f(ws_bytes=lib.pfk_dwconv_bwd_workspace_bytes(1, 4, 8, 384, 7) - 1) == BAD_ARG
    assert f(in_ld=386) == ALIGNMENT and f(du=Bp + 4) == ALIGNMENT and f(dx_ld=390) == ALIGNMENT and f(ws=WS + 8) == ALIGNMENT
    assert f(dx=Bp) == BAD_ARG and f(dx=A) == BAD_ARG
    assert lib.pfk_dwconv_bwd_workspace_bytes(1, 4, 8, 384, 7) == 1 * 384 * 50 * 4          # one tile: one slice
    assert lib.pfk_dwconv_bwd_workspace_bytes(8, 55, 128, 384, 7) == 64 * 384 * 50 * 4      # tens of blocks, not M / 32


def test_gelu_validates_without_a_gpu(lib):
    fw, bw = lib.pfk_gelu_f32, lib.pfk_gelu_bwd_f32
    assert fw(None, 512, Bp, 512, 8, 512, None) == BAD_ARG and fw(A, 512, None, 512, 8, 512, None) == BAD_ARG
    assert fw(A, 512, Bp, 512, 8, 510, None) == BAD_ARG and fw(A, 508, Bp, 512, 8, 512, None) == BAD_ARG
    assert fw(A, 512, Bp, 512, 0, 512, None) == BAD_ARG and fw(A, 512, A, 512, 8, 512, None) == BAD_ARG
    assert fw(A + 4, 512, Bp, 512, 8, 512, None) == ALIGNMENT and fw(A, 514, Bp, 512, 8, 512, None) == ALIGNMENT
    assert bw(A, 512, None, 512, Cp, 512, 8, 512, None) == BAD_ARG and bw(A, 512, Bp, 508, Cp, 512, 8, 512, None) == BAD_ARG
    assert bw(A, 512, Bp, 512, Bp, 512, 8, 512, None) == BAD_ARG and bw(A, 512, Bp, 512, Cp + 8, 512, 8, 512, None) == ALIGNMENT


def test_accelerate_argument_errors():
    from sea_seam_model import SeaRaftLoop
    from ptlflow_amd import patch
    model = SeaRaftLoop(iters=1)
    for upd in (False, None, "bf16"):
        with pytest.raises(ValueError):
            patch.accelerate(model, sea_raft_update=upd, sea_raft_train=True)
    assert type(model.update_block).__name__ == "BasicUpdateBlock"          # refused before anything was installed
    try:
        for upd in (True, "fp32"):
            patch.accelerate(model, sea_raft_update=upd, sea_raft_train=True)
            ub = model.update_block
            assert ub.sea_train and ub.train_calls == 0 and model.flow_head.train_calls == 0 and model.upsample_weight.train_calls == 0
        patch.accelerate(model, sea_raft_update=True)                        # the default switches it off again
        assert not model.update_block.sea_train
    finally:
        patch.restore(model)
    assert type(model.update_block).__name__ == "BasicUpdateBlock" and not hasattr(model.flow_head, "train_calls")


# ---------------------------------------------------------------------------------------------------------------------
# the formulas of include/pfk.h in float64 against autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,k,zero", [(2, 5, 6, 8, 7, False), (1, 9, 11, 12, 3, False), (2, 4, 7, 16, 5, True), (1, 1, 5, 8, 7, True)])
def test_formulas_equal_autograd(B, H, W, C, k, zero):
    g = torch.Generator().manual_seed(B * 100 + H * 10 + k)
    dbl = torch.float64
    x = torch.randn(B, C, H, W, generator=g, dtype=dbl, requires_grad=True)
    w = torch.randn(C, 1, k, k, generator=g, dtype=dbl, requires_grad=True)
    b = torch.randn(C, generator=g, dtype=dbl, requires_grad=True)
    gamma = (1 + 0.3 * torch.randn(C, generator=g, dtype=dbl))
    if zero:
        gamma[3] = 0.0           # a LayerNorm weight of exactly zero: x^ is saved, not (out - beta) / gamma
    gamma.requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=dbl, requires_grad=True)
    dy = torch.randn(B, H, W, C, generator=g, dtype=dbl)
    u = F.conv2d(x, w, b, padding=k // 2, groups=C).permute(0, 2, 3, 1)
    out = F.layer_norm(u, (C,), gamma, beta, 1e-6)
    want = torch.autograd.grad((out * dy).sum(), [x, w, b, gamma, beta])
    with torch.no_grad():
        ud = u.reshape(-1, C)
        mean, var = ud.mean(1, keepdim=True), ud.var(1, unbiased=False, keepdim=True)
        rstd = (var + 1e-6).rsqrt()[:, 0]
        xhat = (ud - mean) * rstd[:, None]
        du, dgamma, dbeta = layernorm_bwd_ref(xhat, rstd, gamma, dy.reshape(-1, C))
        x_pm = x.permute(0, 2, 3, 1).reshape(-1, C)
        dx, dw, db = dwconv_bwd_ref(x_pm, du, w.view(C, k, k), B, H, W)
    got = [dx.view(B, H, W, C).permute(0, 3, 1, 2), dw.view(C, 1, k, k), db, dgamma, dbeta]
    for name, a, bb in zip(("dx", "dweight", "dbias", "dgamma", "dbeta"), got, want):
        assert rel(a, bb) <= 1e-12, (name, rel(a, bb))


def test_gelu_formula_equals_autograd():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4000, generator=g, dtype=torch.float64) * 3, torch.tensor([0.0, -0.0, 30.0, -30.0, 1e3, -1e3], dtype=torch.float64)])
    x.requires_grad_(True)
    dy = torch.randn(x.shape, generator=g, dtype=torch.float64)
    y = F.gelu(x)
    (want,) = torch.autograd.grad((y * dy).sum(), x)
    with torch.no_grad():
        assert rel(0.5 * x * (1 + torch.erf(x / math.sqrt(2))), y) <= 1e-12
        got = gelu_bwd_ref(x, dy)
    assert rel(got, want) <= 1e-12
    assert bool(torch.isfinite(got).all()) and float(got[-1]) == 0.0 and float(got[-2]) == float(dy[-2])


# ---------------------------------------------------------------------------------------------------------------------
# the gradient fixture
# ---------------------------------------------------------------------------------------------------------------------
def _script():
    spec = importlib.util.spec_from_file_location("make_sea_raft_train_golden", os.path.join(ROOT, "scripts", "make_sea_raft_train_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_holds_what_it_should():
    gd = torch.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1_000_000
    assert all(torch.is_tensor(v) for v in gd.values())
    S = _script()
    want = S.inputs()
    for k, v in want.items():
        assert gd[k].dtype == torch.float32 and torch.equal(gd[k], v), k
    for k in ("net", "inp", "corr", "flow"):
        assert gd["grad." + k].dtype == torch.float64 and gd["grad." + k].shape == gd[k].shape
    full = sorted(k for k in gd if k.startswith("full."))
    assert full == sorted(f"full.update_block.refine.{i}.{s}" for i in (0, 1) for s in S.FULL_SUFFIXES)
    norms = {k[5:] for k in gd if k.startswith("norm.")}
    assert norms == {k[4:] for k in gd if k.startswith("dot.")} and len(norms) == 10 + 2 * 6 + 8


def test_stand_in_backward_equals_the_fixture():
    """tests/sea_seam_model.py in float64 against the reference's own backward, every entry, 1e-9 relative"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    S = _script()
    gd = torch.load(GOLDEN)
    model = load_seeded(SeaRaftLoop(), S.SEED).double()
    gin, gpar = S.step_gradients(model.update_block, model.flow_head, model.upsample_weight, gd)
    got = S.summarise({k: gd[k] for k in S.inputs()}, gin, gpar)
    assert sorted(got) == sorted(gd)
    for k in sorted(gd):
        a, b = got[k].double(), gd[k].double()
        assert float((a - b).norm()) <= 1e-9 * float(b.norm()), (k, float((a - b).norm()), float(b.norm()))


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference tree")
def test_fixture_regenerates_bit_identically():
    gd = torch.load(GOLDEN)
    again = _script().make()
    assert sorted(again) == sorted(gd)
    for k in gd:
        assert again[k].dtype == gd[k].dtype and torch.equal(again[k], gd[k]), k
