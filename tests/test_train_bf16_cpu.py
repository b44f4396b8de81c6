"""bf16 training of the update block (K12b), the parts that need no GPU: the C ABI of `pfk_conv_wgrad_unpacked_b16` (declared,
exported, ABI version unchanged, arguments validated before the device is touched), the data-gradient weight pack in K8b's K
order, and the public interface's argument checks."""
import ctypes
import os
import re

import pytest
import torch

import pfk_ctypes
from pfk_ctypes import DescB16 as Desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pfk_conv_wgrad_unpacked_b16", "pfk_conv_wgrad_unpacked_b16_workspace_bytes", "pfk_debug_set_wgrad_b16")
BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    lib = pfk_ctypes.lib()
    lib.pfk_conv_wgrad_unpacked_b16_workspace_bytes.restype = ctypes.c_longlong
    lib.pfk_conv_wgrad_unpacked_b16_workspace_bytes.argtypes = [ctypes.POINTER(Desc), ctypes.c_int]
    lib.pfk_conv_wgrad_unpacked_b16.restype = ctypes.c_int
    lib.pfk_conv_wgrad_unpacked_b16.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_longlong, ctypes.c_void_p]
    return lib


def test_header_declares_and_library_exports_the_new_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfk.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/pfk.h does not declare {n}"
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    assert lib.pfk_abi_version() == 7
    assert "#define PFK_ABI_VERSION 7" in src


def _desc(stride=1, ld=64, channels=64, kh=3, kw=3, cout=64):
    d = Desc()
    d.src[0].ptr, d.src[0].ld, d.src[0].channels = 0x1000, ld, channels      # never dereferenced: every call below is refused first
    d.num_src, d.B, d.H, d.W, d.kh, d.kw, d.cout, d.stride = 1, 1, 8, 8, kh, kw, cout, stride
    return d


def _call(lib, d, dw=0x2000, ws=0x3000, ws_bytes=None, dy_ld=64):
    real = (ctypes.c_int * 3)(d.src[0].channels, 0, 0)
    if ws_bytes is None:
        ws_bytes = lib.pfk_conv_wgrad_unpacked_b16_workspace_bytes(ctypes.byref(d), 1)
    return lib.pfk_conv_wgrad_unpacked_b16(ctypes.byref(d), real, 0x4000, dy_ld, d.cout, dw, 0x5000, 0, ws, ws_bytes, None)


def test_entry_point_validates_without_a_gpu(lib):
    good = _desc()
    need = lib.pfk_conv_wgrad_unpacked_b16_workspace_bytes(ctypes.byref(good), 1)
    assert need >= 64 * (9 * 64 + 32) * 4          # at least one fp32 slice [cout][ktot + the bias chunk]
    assert _call(lib, _desc(stride=2), ws_bytes=need) == BAD_ARG
    assert _call(lib, _desc(ld=68), ws_bytes=need) == BAD_ARG                 # ld % 8 != 0
    assert _call(lib, good, dy_ld=68) == BAD_ARG                              # dy_ld % 8 != 0
    assert _call(lib, good, dw=None) == BAD_ARG
    assert _call(lib, good, ws=None) == BAD_ARG
    assert _call(lib, good, ws_bytes=need - 1) == BAD_ARG
    assert _call(lib, _desc(kh=7, kw=7), ws_bytes=1 << 30) == BAD_ARG          # outside 1x1, 3x3, 1x5, 5x1
    assert _call(lib, _desc(cout=4), ws_bytes=1 << 30, dy_ld=8) == BAD_ARG     # dy channels below 8
    assert lib.pfk_conv_wgrad_unpacked_b16(None, None, None, 0, 0, None, None, 0, None, 0, None) == BAD_ARG
    assert lib.pfk_conv_wgrad_unpacked_b16_workspace_bytes(None, 0) == 0
    # byte offsets >= 2^31 are refused (PFK_ERR_UNSUPPORTED = -3), as the other launchers do
    big = _desc()
    big.B, big.H, big.W = 16, 1024, 1024
    assert _call(lib, big, ws_bytes=1 << 40) == -3


@pytest.mark.parametrize("kh,kw", [(3, 3), (1, 5), (5, 1), (1, 1)])
def test_dgrad_pack_is_the_flipped_transposed_slice(kh, kw):
    """`dgrad_weight_b16` -> bf16 [n_buf, taps * 64-padded dY channels]; K8b's documented K order is: each tap (ky major), the
    source's channels padded to a multiple of 64.  Unpacked in that order it must equal W[:, slice] with in / out swapped and
    the taps flipped — the weight of the transposed convolution — rounded to bf16, with zero rows for the padding channels."""
    from ptlflow_amd.train import dgrad_weight_b16
    g = torch.Generator().manual_seed(2)
    cout, cin, first, n, n_buf, dy_ch = 40, 50, 12, 30, 32, 40
    w = torch.randn(cout, cin, kh, kw, generator=g)
    pk = dgrad_weight_b16(w, (first, n, n_buf), dy_ch)
    assert pk.dtype == torch.bfloat16 and pk.shape == (n_buf, kh * kw * 64)
    un = pk.float().view(n_buf, kh, kw, 64)
    want = w[:, first:first + n].to(torch.bfloat16).float()            # [cout, n, kh, kw]
    for ky in range(kh):
        for kx in range(kw):
            assert torch.equal(un[:n, ky, kx, :cout], want[:, :, kh - 1 - ky, kw - 1 - kx].t())
    assert bool((un[n:] == 0).all()) and bool((un[..., cout:] == 0).all())


def test_train_precision_values_are_checked():
    from ptlflow_amd.patch import accelerate
    from ptlflow_amd.raft import RAFT
    with pytest.raises(ValueError):
        RAFT(train_precision="fp16")
    assert RAFT(iters=1, train_precision="bf16").train_precision == "bf16"
    assert RAFT(iters=1).train_precision == "fp32"
    with pytest.raises(ValueError):
        accelerate(torch.nn.Linear(2, 2), train_precision="fp16")


def test_bf16_refuses_the_aggregate_branch_and_unknown_values():
    from ptlflow_amd.train import update_block_train_pm
    from ptlflow_amd.update import gma_spec
    t = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        update_block_train_pm({}, gma_spec(), t, t, t, t, 1, 2, 2, precision="bf16")
    with pytest.raises(ValueError):
        update_block_train_pm({}, gma_spec(), t, t, t, t, 1, 2, 2, precision="fp16")
