"""Training GMA on the kernels (K12c), the parts that need no GPU: the C ABI of `pfk_softmax_rows_bwd_*` and
`pfk_transpose_pack_*` (declared, exported, ABI version unchanged, arguments validated before the device is touched) and the
public interface's argument checks."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import ptlflow_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pfk_softmax_rows_bwd_f32", "pfk_softmax_rows_bwd_bf16", "pfk_transpose_pack_f32", "pfk_transpose_pack_b16")
OK, BAD_ARG, ALIGNMENT = 0, -1, -2
LL, VP, I = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    if not ptlflow_amd.LIBPFK_PATH.exists():
        from ptlflow_amd import _build
        _build.build_all()
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    for n in NEW[:2]:          # (p, ld_p, dp, ld_dp, ds, ld_out, rows, cols, stream)
        getattr(lib, n).restype = I
        getattr(lib, n).argtypes = [VP, LL, VP, LL, VP, LL, LL, I, VP]
    for n in NEW[2:]:          # (in, ld_in, outT, out, ld_out, B, N, stream)
        getattr(lib, n).restype = I
        getattr(lib, n).argtypes = [VP, LL, VP, VP, LL, I, I, VP]
    return lib


def test_header_declares_and_library_exports_the_new_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfk.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/pfk.h does not declare {n}"
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    assert lib.pfk_abi_version() == 7
    assert "#define PFK_ABI_VERSION 7" in src


# every call below is refused before a launch: the pointers are never dereferenced
P, DP, DS = 0x10000, 0x20000, 0x30000


@pytest.mark.parametrize("name", NEW[:2])
def test_softmax_rows_bwd_validates_without_a_gpu(lib, name):
    f = getattr(lib, name)
    assert f(None, 144, DP, 144, DS, 144, 8, 140, None) == BAD_ARG
    assert f(P, 144, None, 144, DS, 144, 8, 140, None) == BAD_ARG
    assert f(P, 144, DP, 144, None, 144, 8, 140, None) == BAD_ARG
    assert f(P, 136, DP, 144, DS, 144, 8, 140, None) == BAD_ARG          # cols > ld of p
    assert f(P, 144, DP, 136, DS, 144, 8, 140, None) == BAD_ARG          # ... of dp
    assert f(P, 144, DP, 144, DS, 136, 8, 140, None) == BAD_ARG          # ... of the output
    assert f(P, 144, DP, 144, DS, 144, 0, 140, None) == BAD_ARG
    assert f(P, 144, DP, 144, DS, 144, 8, 0, None) == BAD_ARG


def test_softmax_rows_bwd_alignment_and_in_place_rules(lib):
    b16, f32 = lib.pfk_softmax_rows_bwd_bf16, lib.pfk_softmax_rows_bwd_f32
    assert b16(P, 144, DP + 2, 144, DS, 144, 8, 140, None) == ALIGNMENT      # bf16 rows off a 16-byte boundary
    assert b16(P, 144, DP, 142, DS, 144, 8, 140, None) == ALIGNMENT          # row stride not a multiple of 8 elements
    assert f32(P, 144, DS, 148, DS, 144, 8, 140, None) == BAD_ARG            # in place needs one row stride
    assert b16(P, 144, DS, 144, DS, 144, 8, 140, None) == BAD_ARG            # in place is fp32 only


@pytest.mark.parametrize("name", NEW[2:])
def test_transpose_pack_validates_without_a_gpu(lib, name):
    f = getattr(lib, name)
    A, T, C = 0x10000, 0x20000, 0x30000
    assert f(None, 144, T, C, 144, 2, 140, None) == BAD_ARG
    assert f(A, 144, None, C, 144, 2, 140, None) == BAD_ARG
    assert f(A, 136, T, C, 144, 2, 140, None) == BAD_ARG                 # N > ld_in
    assert f(A, 144, T, C, 136, 2, 140, None) == BAD_ARG                 # N > ld_out
    assert f(A, 144, T, C, 144, 0, 140, None) == BAD_ARG
    assert f(A, 144, T, C, 144, 2, 0, None) == BAD_ARG
    assert f(A, 144, T, T, 144, 2, 140, None) == BAD_ARG                 # the two outputs must differ
    assert f(A, 144, A, None, 144, 2, 140, None) == BAD_ARG              # no in-place transpose


def test_transpose_pack_b16_alignment(lib):
    f = lib.pfk_transpose_pack_b16
    A, T, C = 0x10000, 0x20000, 0x30000
    assert f(A, 144, T + 8, C, 144, 2, 140, None) == ALIGNMENT
    assert f(A, 144, T, C + 2, 144, 2, 140, None) == ALIGNMENT
    assert f(A, 144, T, C, 140, 2, 140, None) == ALIGNMENT               # bf16 row stride not a multiple of 8


def test_update_block_train_pm_no_longer_refuses_gma():
    import ptlflow_amd.train as TR
    src = inspect.getsource(TR.update_block_train_pm)
    assert "does not cover GMA" not in src and "_AttnMatmul" in src and "torch.bmm" not in src
    assert "attention" in inspect.signature(TR.update_block_train).parameters
    for n in ("_AttnMatmul", "_AttentionMap", "_AttnFlush", "pack_attention", "attention_map_train"):
        assert hasattr(TR, n), n


def test_precision_values_are_still_checked():
    from ptlflow_amd.raft import GMA
    from ptlflow_amd.train import check_precision, pack_attention, update_block_train_pm
    from ptlflow_amd.update import gma_spec
    with pytest.raises(ValueError):
        check_precision("fp16")
    t = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        update_block_train_pm({}, gma_spec(), t, t, t, t, 1, 2, 2, precision="fp16", attention=torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError):          # a GMA block needs its map, in either precision
        update_block_train_pm({}, gma_spec(), t, t, t, t, 1, 2, 2, precision="fp32")
    with pytest.raises(ValueError):
        GMA(iters=1, train_precision="fp16")
    assert GMA(iters=1, train_precision="bf16").train_precision == "bf16" and GMA(iters=1).train_precision == "fp32"
    with pytest.raises(ValueError):          # several heads are outside the packed state
        pack_attention(torch.zeros(1, 2, 4, 4), 1, 2, 2)
