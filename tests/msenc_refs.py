"""TEST INFRASTRUCTURE.  Float64 references of the K15 row kernels (ptlflow_amd/csrc/pfk_msenc.hip) with, next to each, the float64
sum of magnitudes that tests/op_gate.py's per-element bound is written on, and the loaders of the fixtures recorded from the
reference's encoders (tests/golden/ms_encoders*.pt, scripts/make_golden_ms_encoders.py).

    GroupNorm    y = x * scale + shift,  scale = rstd_g gamma_c,  shift = beta_c - mean_g rstd_g gamma_c      mag = |x| |scale| + |shift|
                 The kernel hands out fp32 scale / shift; y is formed from them in float64.  scale and shift are rounded once each
                 (2 u mag); the bound allows k = 6.
    affine apply relu?(x * scale + shift) (+ residual, relu?)                                                   mag = |x scale| + |shift| (+ |residual|)
    resize       the 4-tap bilinear sum (weights >= 0)                                                          mag = the same resize of |x|
"""
import os

import torch
import torch.nn.functional as F

GN_EPS = 1e-5
GROUP = 8
GN_CHUNK_ROWS = 256      # pixels of an image per partial-sum block of pfk_groupnorm_stats_f32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def groupnorm_ref(x, gamma, beta, eps=GN_EPS, group=GROUP):
    """x [B, HW, C] float64, gamma / beta [C] -> (scale [B, C], shift [B, C], y [B, HW, C], mag [B, HW, C]), all float64"""
    B, HW, C = x.shape
    xg = x.reshape(B, HW, C // group, group)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))          # two-pass: no cancellation in the reference
    rstd = 1.0 / torch.sqrt(var + eps)
    g, b = gamma.double(), beta.double()
    scale = rstd.repeat_interleave(group, 1) * g
    shift = b - mean.repeat_interleave(group, 1) * scale
    y = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, HW, C) * g + b
    mag = x.abs() * scale.abs()[:, None, :] + shift.abs()[:, None, :]
    return scale, shift, y, mag


def affine_apply_ref(x, scale, shift, relu, residual=None, relu_after=False):
    """x [B, HW, C], scale / shift [B, C], residual [B, HW, C] or None, float64 -> (out, mag)"""
    v = x * scale[:, None, :] + shift[:, None, :]
    mag = (x * scale[:, None, :]).abs() + shift.abs()[:, None, :]
    if relu:
        v = v.clamp_min(0)
    if residual is not None:
        v = residual + v
        mag = mag + residual.abs()
        if relu_after:
            v = v.clamp_min(0)
    return v, mag


def resize_ref(x, size):
    """x [B, C, H, W] float64 -> (TF.resize's tensor path: bilinear, align_corners=False, antialias on; the same resize of |x|)"""
    kw = dict(size=tuple(size), mode="bilinear", align_corners=False, antialias=True)
    return F.interpolate(x, **kw), F.interpolate(x.abs(), **kw)


def load_golden():
    """{"input": [2, 3, 32, 48] float64, "encoders": {key: {"seed", "shapes", "checksums", "levels"}}}"""
    return torch.load(os.path.join(GOLDEN, "ms_encoders.pt"))


def load_golden_levels(key):
    """the recorded pyramid of encoder `key`, coarse to fine, float32"""
    return torch.load(os.path.join(GOLDEN, f"ms_encoders_{key}.pt"))
