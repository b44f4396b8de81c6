"""CPU side of the encoder's fused instance norms (tests/test_gpu_encoder_norm_fusion.py holds the kernels): the new entry points are
declared in include/pfk.h and exported by libpfk.so, the ABI version did not move, and bad arguments are refused on the host before
any device call (fake, never dereferenced pointers)."""
import ctypes
import os
import re

import pytest

import pfk_ctypes
from pfk_ctypes import Desc as _Desc, Src as _Src

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pfk_conv2d_wino_norm_f32", "pfk_conv2d_wino_stats_f32", "pfk_conv_wino_stats_workspace_bytes", "pfk_norm_apply_res_f32")
BAD_ARG, ALIGNMENT, UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    lib = pfk_ctypes.lib()
    lib.pfk_conv_wino_stats_workspace_bytes.restype = ctypes.c_longlong
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.pfk_conv2d_wino_norm_f32.argtypes = [P, P, P, I, P]
    lib.pfk_conv2d_wino_stats_f32.argtypes = [P, P, P, I, ctypes.c_float, P, P, P, ctypes.c_longlong, P]
    lib.pfk_norm_apply_res_f32.argtypes = [P, I, P, P, P, I, P, P, I, P, I, I, I, I, I, I, P]
    return lib


def desc(**kw):
    d = _Desc()
    d.src[0] = _Src(0x10000, 64, 64)
    d.num_src, d.B, d.H, d.W, d.kh, d.kw = 1, 2, 6, 8, 3, 3
    d.weight, d.cout, d.epilogue, d.relu, d.scale = 0x20000, 64, 0, 0, 1.0
    d.out, d.out_ld = 0x30000, 64
    for k, v in kw.items():
        setattr(d, k, v)
    return d


MEAN, RSTD, OMEAN, ORSTD, WS = 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


def test_new_symbols_declared_and_exported(lib):
    src = open(os.path.join(ROOT, "include", "pfk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pfk_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert not [s for s in declared if not hasattr(lib, s)]


def test_abi_version_did_not_move(lib):
    assert lib.pfk_abi_version() == 7
    assert re.search(r"#define\s+PFK_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "pfk.h")).read())


def test_stats_workspace_size(lib):
    f = lib.pfk_conv_wino_stats_workspace_bytes
    assert f(2, 6, 8, 64) == 2 * 2 * 1 * 64 * 8                    # 12 tiles per image: one block each
    assert f(2, 18, 26, 64) == 2 * 2 * 4 * 64 * 8                  # 117 tiles: 4 blocks
    assert f(16, 218, 512, 64) == 2 * 16 * 872 * 64 * 8            # more parts per image than a statistics pass ever has (256)
    assert f(0, 6, 8, 64) == BAD_ARG and f(1, 6, 8, 0) == BAD_ARG


def test_norm_form_refusals(lib):
    f = lib.pfk_conv2d_wino_norm_f32
    assert f(None, MEAN, RSTD, 1, None) == BAD_ARG
    assert f(ctypes.byref(desc()), None, RSTD, 1, None) == BAD_ARG
    assert f(ctypes.byref(desc()), MEAN, None, 1, None) == BAD_ARG
    d = desc()
    d.src[0] = _Src(0x10000, 64, 40)                               # cin not a multiple of 32
    assert f(ctypes.byref(d), MEAN, RSTD, 1, None) == UNSUPPORTED
    assert f(ctypes.byref(desc(residual=0x90000, residual_ld=64)), MEAN, RSTD, 1, None) == UNSUPPORTED
    assert f(ctypes.byref(desc()), MEAN + 2, RSTD, 1, None) == ALIGNMENT
    assert f(ctypes.byref(desc(out=None)), MEAN, RSTD, 1, None) == BAD_ARG


def test_stats_form_refusals(lib):
    f = lib.pfk_conv2d_wino_stats_f32
    need = lib.pfk_conv_wino_stats_workspace_bytes(2, 6, 8, 64)

    def call(d, im=MEAN, ir=RSTD, om=OMEAN, orr=ORSTD, ws=WS, nbytes=need):
        return f(ctypes.byref(d), im, ir, 1, 1e-5, om, orr, ws, nbytes, None)
    assert f(None, MEAN, RSTD, 1, 1e-5, OMEAN, ORSTD, WS, need, None) == BAD_ARG
    assert call(desc(), im=None) == BAD_ARG and call(desc(), ir=None) == BAD_ARG      # one of the pair missing
    assert call(desc(), om=None) == BAD_ARG and call(desc(), orr=None) == BAD_ARG
    assert call(desc(), ws=None) == BAD_ARG
    assert call(desc(), nbytes=need - 1) == BAD_ARG                                   # a short workspace
    assert call(desc(), ws=WS + 4) == ALIGNMENT
    assert call(desc(residual=0x90000, residual_ld=64)) == BAD_ARG                    # the statistics form has no residual
    assert call(desc(relu_after_residual=1)) == BAD_ARG
    d = desc()
    d.src[0] = _Src(0x10000, 64, 40)
    assert call(d) == UNSUPPORTED
    assert call(desc(cout=128, out_ld=128, cout_active=64), nbytes=2 * need) == UNSUPPORTED


def test_apply_res_refusals(lib):
    f = lib.pfk_norm_apply_res_f32
    X, RES, OUT = 0x10000, 0x20000, 0x30000

    def call(x=X, mean=MEAN, rstd=RSTD, res=RES, rm=OMEAN, rr=ORSTD, out=OUT, C=64, res_ld=64):
        return f(x, 64, mean, rstd, res, res_ld, rm, rr, 1, out, 64, 2, 48, C, 1, 1, None)
    for kw in (dict(x=None), dict(mean=None), dict(rstd=None), dict(res=None), dict(rm=None), dict(rr=None), dict(out=None),
               dict(res_ld=32), dict(C=0)):
        assert call(**kw) == BAD_ARG, kw
    assert call(C=62) == ALIGNMENT and call(res=RES + 4) == ALIGNMENT and call(rm=OMEAN + 4) == ALIGNMENT
