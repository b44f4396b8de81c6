"""Host side of the Winograd F(2x2,3x3) convolution (no GPU): the weight transform of packing.pack_wino_weight against a float64
restatement, the F(2x2,3x3) algorithm on that layout against a direct fp64 convolution, and the C ABI's argument checks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pfk_ctypes
from pfk_ctypes import Desc as _Desc, Src as _Src
from ptlflow_amd.packing import pack_wino_weight, wino_slot

G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def _unpack(flat, cin, cout):
    """flat [ceil(cout/64)][cin/8][16][64][8 slots] -> U [16][cout][cin] (include/pfk.h)"""
    ncb = (cout + 63) // 64
    u = flat.double().view(ncb, cin // 8, 16, 64, 8)
    slot = wino_slot(torch.arange(64).view(64, 1), torch.arange(8).view(1, 8))
    u = torch.gather(u, 4, slot.view(1, 1, 1, 64, 8).expand_as(u))          # [cb][ks][xi][nl][cc]
    return u.permute(2, 0, 3, 1, 4).reshape(16, ncb * 64, cin)


@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 126), (128, 512), (96, 70)])
def test_weight_transform_matches_float64(cin, cout):
    torch.manual_seed(0)
    w = torch.randn(cout, cin, 3, 3)
    flat = pack_wino_weight(w)
    assert flat.dtype == torch.float32 and flat.is_contiguous()
    ncb = (cout + 63) // 64
    assert flat.numel() == 16 * cin * ncb * 64
    U = _unpack(flat, cin, cout)
    assert bool((U[:, cout:] == 0).all()), "pad columns must be zero"
    # restatement: one 4x4 matrix G g G^T per (co, c), in float64, rounded to fp32 once
    for co in range(0, cout, max(1, cout // 7)):
        for c in range(0, cin, max(1, cin // 5)):
            u = (G @ w[co, c].double() @ G.T).float().double().reshape(16)
            assert torch.equal(U[:, co, c], u), (co, c)


def test_slots_are_a_permutation_per_row():
    for nl in range(64):
        s = wino_slot(torch.tensor(nl), torch.arange(8))
        assert sorted(s.tolist()) == list(range(8))
        # the MFMA lane k of sub-step s reads the slot pair (2k ^ key, 2k ^ key + 1) = channels (k, k + 4)
        for k in range(4):
            assert int(s[k]) % 2 == 0 and int(s[k + 4]) == int(s[k]) + 1


@pytest.mark.parametrize("B,H,W,cin,cout", [(1, 5, 7, 32, 70), (2, 1, 1, 32, 64), (1, 4, 3, 64, 128)])
def test_f2x2_3x3_on_the_packed_layout_is_the_convolution(B, H, W, cin, cout):
    """the algorithm the kernel runs — 4x4 patches from one pixel up-left of each 2x2 tile (zero outside the image), B^T d B,
    16 channel sums against U, A^T m A — on the packed weight equals the fp64 convolution to fp32 rounding of U"""
    torch.manual_seed(1)
    x = torch.randn(B, cin, H, W, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, dtype=torch.float64)
    ref = F.conv2d(x, w, padding=1)
    U = _unpack(pack_wino_weight(w.float()), cin, cout)[:, :cout]
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x, (1, 2 * tw - W + 1, 1, 2 * th - H + 1))
    out = torch.zeros(B, cout, 2 * th, 2 * tw, dtype=torch.float64)
    for ty in range(th):
        for tx in range(tw):
            d = xp[:, :, 2 * ty: 2 * ty + 4, 2 * tx: 2 * tx + 4]
            V = (BT @ d @ BT.T).reshape(B, cin, 16)
            m = torch.einsum("bcx,xoc->bxo", V, U).reshape(B, 4, 4, cout)
            out[:, :, 2 * ty: 2 * ty + 2, 2 * tx: 2 * tx + 2] = torch.einsum("ia,bajo,kj->boik", AT, m, AT)
    err = (out[:, :, :H, :W] - ref).abs().max().item()
    assert err <= 1e-5 * (1 + ref.abs().max().item()), err


@pytest.fixture(scope="module")
def lib():
    return pfk_ctypes.lib()


def test_weight_size_helper(lib):
    lib.pfk_conv_wino_weight_floats.restype = ctypes.c_longlong
    assert lib.pfk_conv_wino_weight_floats(128, 512) == 16 * 128 * 512
    assert lib.pfk_conv_wino_weight_floats(256, 126) == 16 * 256 * 128
    assert lib.pfk_conv_wino_weight_floats(48, 64) == -1
    assert lib.pfk_conv_wino_weight_floats(0, 64) == -1


def test_argument_validation_without_gpu(lib):
    """every refusal happens on the host before any device call (fake, never dereferenced pointers)"""
    BAD_ARG, ALIGNMENT, UNSUPPORTED = -1, -2, -3
    assert lib.pfk_conv2d_wino_f32(None, None) == BAD_ARG

    def desc(**kw):
        d = _Desc()
        d.src[0] = _Src(0x10000, 64, 64)
        d.num_src, d.B, d.H, d.W, d.kh, d.kw = 1, 1, 6, 8, 3, 3
        d.weight, d.cout, d.epilogue, d.relu, d.scale = 0x20000, 64, 0, 1, 1.0
        d.out, d.out_ld = 0x30000, 64
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw in [dict(kh=1, kw=1), dict(stride=2), dict(epilogue=1), dict(epilogue=3), dict(num_src=2), dict(residual=0x40000),
               dict(relu_after_residual=1), dict(cout=128, out_ld=128, cout_active=96)]:
        assert lib.pfk_conv2d_wino_f32(ctypes.byref(desc(**kw)), None) == UNSUPPORTED, kw
    d = desc()
    d.src[0] = _Src(0x10000, 64, 36)
    assert lib.pfk_conv2d_wino_f32(ctypes.byref(d), None) == UNSUPPORTED
    for kw in [dict(weight=None), dict(out=None), dict(B=0), dict(cout=0), dict(out_ld=32)]:
        assert lib.pfk_conv2d_wino_f32(ctypes.byref(desc(**kw)), None) == BAD_ARG, kw
    assert lib.pfk_conv2d_wino_f32(ctypes.byref(desc(weight=0x20004)), None) == ALIGNMENT
    d = desc(B=1 << 12, H=1 << 10, W=1 << 8)                 # 2^30 pixels x 64 channels: past 32-bit byte offsets
    assert lib.pfk_conv2d_wino_f32(ctypes.byref(d), None) == UNSUPPORTED
