"""Weight re-layout for the implicit-GEMM kernels (one-off host glue, pure tensor reshapes).

A PyTorch conv weight ``[cout, cin, kh, kw]`` becomes the K-contiguous matrix ``[cout, ktot]`` that
``pfk_conv2d_f32`` reads as its B operand (include/pfk.h): for every input *segment* (a channel
range of the reference's ``torch.cat`` operand that lives in its own pixel-major buffer slice), for
every tap (ky major, kx minor), the segment's channels zero-padded to a multiple of 32.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn.functional as F


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def pack_conv_weight(weight: torch.Tensor, segments: Sequence[Tuple[int, int, int]], kpad: int = 32) -> torch.Tensor:
    """``segments`` = [(first_channel, n_channels, n_channels_in_buffer)], in source order.
    ``kpad`` = channels per K-step of the kernel that will read it (32: fp32 MFMA, 64: split-bf16 MFMA).

    ``n_channels_in_buffer`` >= ``n_channels`` is how many channels the kernel is told the source
    has (a multiple of 4; extra ones are zero padding in the buffer and get zero weights here)."""
    cout, cin, kh, kw = weight.shape
    parts = []
    for first, n, n_buf in segments:
        assert first + n <= cin and n_buf >= n and n_buf % 4 == 0
        w = weight[:, first:first + n].permute(0, 2, 3, 1)  # [cout, kh, kw, n]
        w = F.pad(w, (0, round_up(n_buf, kpad) - n))
        parts.append(w.reshape(cout, -1))
    return torch.cat(parts, dim=1).contiguous()


# Winograd F(2x2,3x3) weight transform (Lavin & Gray 2016): U = G g G^T
WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def wino_slot(nl: torch.Tensor, cc: torch.Tensor) -> torch.Tensor:
    """LDS slot of channel ``cc`` (0..7 of a K-step) in row ``nl`` of `pfk_conv2d_wino_f32`'s operand images (include/pfk.h)."""
    return ((cc & 3) * 2 + (cc >> 2)) ^ (((nl >> 2) & 3) * 2)


def pack_wino_weight(weight: torch.Tensor) -> torch.Tensor:
    """``[cout, cin, 3, 3]`` -> the flat transformed weight of ``pfk_conv2d_wino_f32``: U = G g G^T in float64 on the host,
    rounded to fp32 once, laid out ``[ceil(cout/64)][cin/8][16][64][8]`` (column block, K-step, component 4*row + col, column,
    slot — include/pfk.h), pad columns zero.  Returned on ``weight``'s device."""
    cout, cin, kh, kw = weight.shape
    assert kh == 3 and kw == 3 and cin % 32 == 0
    G = torch.tensor(WINO_G, dtype=torch.float64)
    g = weight.detach().to(device="cpu", dtype=torch.float64)
    U = torch.einsum("au,ocuv,bv->aboc", G, g, G).reshape(16, cout, cin).to(torch.float32)   # [xi][co][c]
    ncb = (cout + 63) // 64
    U = F.pad(U, (0, 0, 0, ncb * 64 - cout)).reshape(16, ncb, 64, cin // 8, 8)           # [xi][cb][nl][ks][cc]
    nl = torch.arange(64).view(64, 1)
    cc = torch.arange(8).view(1, 8)
    slot = wino_slot(nl, cc).view(1, 1, 64, 1, 8).expand_as(U)
    out = torch.empty_like(U).scatter_(4, slot, U)
    return out.permute(1, 3, 0, 2, 4).contiguous().reshape(-1).to(weight.device)


# Winograd F(4,5) weight transform, points 0, +-1, +-2, +-1/2, inf (correlation order of the 5 taps): U = G g
WINO1D_G = ((-1.0, 0.0, 0.0, 0.0, 0.0),
            (-2 / 9, -2 / 9, -2 / 9, -2 / 9, -2 / 9),
            (-2 / 9, 2 / 9, -2 / 9, 2 / 9, -2 / 9),
            (1 / 90, 1 / 45, 2 / 45, 4 / 45, 8 / 45),
            (1 / 90, -1 / 45, 2 / 45, -4 / 45, 8 / 45),
            (32 / 45, 16 / 45, 8 / 45, 4 / 45, 2 / 45),
            (32 / 45, -16 / 45, 8 / 45, -4 / 45, 2 / 45),
            (0.0, 0.0, 0.0, 0.0, 1.0))


def pack_wino1d_weight(weight: torch.Tensor, segments: Sequence[Tuple[int, int, int]], dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``[cout, cin, 1, 5]`` or ``[cout, cin, 5, 1]`` -> the flat transformed weight of ``pfk_conv1d_wino_f32``: U = G g in float64 on
    the host, rounded to fp32 once.  ``segments`` as in `pack_conv_weight` — one per source of the launch, in K order, with the
    source's channel count in its buffer (a multiple of 8; pad channels get zero U).  Layout
    ``[ceil(cout/128)][ktot/8][8][128][8]`` (column block, K-step, component, column, slot — include/pfk.h), pad columns zero.
    Returned on ``weight``'s device.  ``dtype=torch.float64`` keeps U unrounded (tests of the layout; the kernel reads float32)."""
    cout, cin, kh, kw = weight.shape
    assert (kh, kw) in ((1, 5), (5, 1))
    G = torch.tensor(WINO1D_G, dtype=torch.float64)
    g = weight.detach().to(device="cpu", dtype=torch.float64).reshape(cout, cin, 5)
    parts = []
    for first, n, n_buf in segments:
        assert first + n <= cin and n_buf >= n and n_buf % 8 == 0
        parts.append(F.pad(torch.einsum("xk,ock->xoc", G, g[:, first:first + n]), (0, n_buf - n)))
    U = torch.cat(parts, dim=2).to(dtype)                                                # [xi][co][k]
    ktot = U.shape[2]
    ncb = (cout + 127) // 128
    U = F.pad(U, (0, 0, 0, ncb * 128 - cout)).reshape(8, ncb, 128, ktot // 8, 8)          # [xi][cb][nl][ks][cc]
    nl = torch.arange(128).view(128, 1)
    cc = torch.arange(8).view(1, 8)
    slot = wino_slot(nl, cc).view(1, 1, 128, 1, 8).expand_as(U)
    out = torch.empty_like(U).scatter_(4, slot, U)
    return out.permute(1, 3, 0, 2, 4).contiguous().reshape(-1).to(weight.device)


def split_bf16_planes(packed: torch.Tensor, nsplit: int) -> torch.Tensor:
    """fp32 ``[cout, ktot]`` -> bf16 ``[nsplit, cout, ktot]`` with plane 0 = bf16(w), plane 1 = bf16(w - plane 0), ...
    (round to nearest even; every residual is exact in fp32) — the weight operand of ``pfk_conv2d_bf16s``."""
    assert 1 <= nsplit <= 3 and packed.dtype == torch.float32
    planes, r = [], packed
    for _ in range(nsplit):
        p = r.to(torch.bfloat16)
        planes.append(p)
        r = r - p.to(torch.float32)
    return torch.stack(planes, 0).contiguous()


def pack_conv_operand(weight: torch.Tensor, segments: Sequence[Tuple[int, int, int]], b16: bool, nsplit: int) -> torch.Tensor:
    """The weight operand of the direct convolution kernel an engine's precision selects (the tensor's dtype picks the kernel in
    torch.ops.pfk.conv2d): ``b16`` (K8b, `pfk_conv2d_b16`) one bf16 matrix ``[cout, ktot]`` in 64-channel K chunks, rounded once;
    else fp32 ``[cout, ktot]`` in 32-channel chunks (`pfk_conv2d_f32`) or, ``nsplit`` > 0, its bf16 planes (`pfk_conv2d_bf16s`)."""
    if b16:
        return pack_conv_weight(weight, segments, kpad=64).to(torch.bfloat16).contiguous()
    packed = pack_conv_weight(weight, segments)
    return packed if nsplit == 0 else split_bf16_planes(packed, nsplit)


def pack_cin2_weight(weight: torch.Tensor) -> torch.Tensor:
    """[cout, 2, k, k] -> [k*k, 2, cout] for pfk_conv_cin2_f32."""
    cout, cin, kh, kw = weight.shape
    assert cin == 2 and kh == kw
    return weight.permute(2, 3, 1, 0).reshape(kh * kw, 2, cout).contiguous()


def pack_flow_head_weight(weight: torch.Tensor, cin_buf: int = 0) -> torch.Tensor:
    """[2, cin, 3, 3] -> [9, 2, cin_buf] for pfk_flow_delta_f32."""
    cout, cin, kh, kw = weight.shape
    assert cout == 2 and kh == 3 and kw == 3
    w = weight.permute(2, 3, 0, 1).reshape(9, 2, cin)
    if cin_buf > cin:
        w = F.pad(w, (0, cin_buf - cin))
    return w.contiguous()


def mask_upsample_perm(device=None) -> Tuple["torch.Tensor", "torch.Tensor"]:
    """Row order of `pfk_mask_upsample_f32`'s weight / bias (include/pfk.h): 640 rows = [quarter (4)][tile j (5)][32 columns c], row
    `q*160 + j*32 + c` = mask channel `k*64 + s` with tap `k = 2j + (c >> 4)` and sub-pixel `s = q*16 + (c & 15)`; the rows with
    `k == 9` (tile 4, c >= 16) are zero.  Returns `(index [640] into the 576 channels, valid [640] bool)`."""
    q = torch.arange(4, device=device).view(4, 1, 1)
    j = torch.arange(5, device=device).view(1, 5, 1)
    c = torch.arange(32, device=device).view(1, 1, 32)
    k = 2 * j + (c >> 4)
    s = q * 16 + (c & 15)
    valid = (k < 9).expand(4, 5, 32).reshape(-1)
    idx = (k.clamp(max=8) * 64 + s).expand(4, 5, 32).reshape(-1)
    return idx, valid


def permute_mask_head(weight_packed: "torch.Tensor", bias: "torch.Tensor") -> Tuple["torch.Tensor", "torch.Tensor"]:
    """[576, ktot] packed 1x1 weight and [576] bias of the mask head's second convolution -> the [640, ktot] / [640] operands of
    `pfk_mask_upsample_f32`."""
    idx, valid = mask_upsample_perm(weight_packed.device)
    w = weight_packed[idx] * valid[:, None].to(weight_packed.dtype)
    b = bias[idx] * valid.to(bias.dtype)
    return w.contiguous(), b.contiguous()
