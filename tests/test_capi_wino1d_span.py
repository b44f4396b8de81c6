"""`pfk_conv1d_wino_f32`'s gate epilogues address the context term, h, z and r*h with 32-bit byte offsets through buffer descriptors
sized to the last pixel's last column, so the launcher refuses any of these spans from 2 GB on with PFK_ERR_UNSUPPORTED, as it does
for the sources.  The check is an argument check: it is reached through the C API with a span that is large on paper only
(B * H * W * h_ld), no allocation of that size and no GPU.

No descriptor here can reach a launch: the weight pointer is deliberately not 16-byte aligned, and that check comes behind the span
checks — a descriptor whose spans fit answers PFK_ERR_ALIGNMENT, one whose span does not fit answers PFK_ERR_UNSUPPORTED before it."""
import ctypes

import pytest

import pfk_ctypes
from pfk_ctypes import EPI_GRU_Q, EPI_GRU_ZR, PFK_ERR_ALIGNMENT, PFK_ERR_UNSUPPORTED, Desc, Src


@pytest.fixture(scope="module")
def lib():
    lib = pfk_ctypes.lib()
    lib.pfk_conv1d_wino_f32.argtypes = [ctypes.POINTER(Desc), ctypes.c_void_p]
    lib.pfk_conv1d_wino_f32.restype = ctypes.c_int
    return lib


B, H, W, CH = 2, 64, 64, 128      # M = 8192
M = B * H * W
A16 = 0x10000                     # a 16-byte aligned address that is never read


def desc(epilogue, kh, kw, h_ld=384, residual=True, residual_ld=None):
    cout = 2 * CH if epilogue == EPI_GRU_ZR else CH
    d = Desc()
    d.src[0] = Src(A16, 384, CH)
    d.src[1] = Src(A16 + 1024, 384, CH)
    d.num_src, d.B, d.H, d.W, d.kh, d.kw = 2, B, H, W, kh, kw
    d.weight = A16 + 4            # not 16-byte aligned: PFK_ERR_ALIGNMENT behind every other argument check, never a launch
    d.cout, d.epilogue, d.scale = cout, epilogue, 1.0
    d.h, d.h_ld, d.aux_z, d.aux_rh = A16, h_ld, A16, A16
    if residual:
        d.residual, d.residual_ld = A16, residual_ld or cout
    return d


@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
@pytest.mark.parametrize("epilogue", [EPI_GRU_ZR, EPI_GRU_Q])
def test_gate_spans_of_2gb_are_refused(lib, epilogue, kh, kw):
    call = lambda d: lib.pfk_conv1d_wino_f32(ctypes.byref(d), None)      # noqa: E731
    assert call(desc(epilogue, kh, kw)) == PFK_ERR_ALIGNMENT, "the control descriptor must pass every span check"
    # h: ((M - 1) * h_ld + Ch) * 4 bytes; `fits` is the largest row stride (a multiple of 4) that stays below 2 GB
    fits = (0x7fffffff // 4 - CH) // (M - 1) // 4 * 4
    assert ((M - 1) * fits + CH) * 4 < 0x7fffffff <= ((M - 1) * (fits + 4) + CH) * 4
    assert call(desc(epilogue, kh, kw, h_ld=fits)) == PFK_ERR_ALIGNMENT
    assert call(desc(epilogue, kh, kw, h_ld=fits + 4)) == PFK_ERR_UNSUPPORTED
    assert call(desc(epilogue, kh, kw, h_ld=1 << 20)) == PFK_ERR_UNSUPPORTED      # 32 GB on paper
    # the context term: ((M - 1) * residual_ld + cout) * 4 bytes
    assert call(desc(epilogue, kh, kw, residual_ld=1 << 20)) == PFK_ERR_UNSUPPORTED
    assert call(desc(epilogue, kh, kw, residual=False)) == PFK_ERR_ALIGNMENT


def test_z_span_of_2gb_is_refused(lib):
    """z and r*h are dense [M][Ch] rows: M * Ch * 4 bytes.  The sources' own check (M * ld * 4) passes with 8-channel sources."""
    d = desc(EPI_GRU_Q, 1, 5)
    d.B, d.H, d.W = 1, 4096, 1024     # M = 2^22, Ch = 128: 2 GB
    d.src[0] = Src(A16, 8, 8)
    d.src[1] = Src(A16, 8, 8)
    d.h_ld = CH
    d.residual = None
    assert lib.pfk_conv1d_wino_f32(ctypes.byref(d), None) == PFK_ERR_UNSUPPORTED
    d.H = 4095
    assert lib.pfk_conv1d_wino_f32(ctypes.byref(d), None) == PFK_ERR_ALIGNMENT
