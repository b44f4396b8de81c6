"""float64 reference formulas and input builders that more than one test file uses.  The comparisons are in tests/op_gate.py."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import raft_oracle as O


# ---------------------------------------------------------------------------------------------------------------------
# the ConvNeXt block's backward formulas of include/pfk.h (tests/test_sea_train_cpu.py holds them against autograd)
# ---------------------------------------------------------------------------------------------------------------------
def layernorm_bwd_ref(xhat, rstd, gamma, dy):
    """(b): rows [M, C]"""
    g = dy * gamma
    du = rstd[:, None] * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    return du, (dy * xhat).sum(0), dy.sum(0)


def dwconv_bwd_ref(x, du, w, B, H, W):
    """(c): rows [M, C], w [C, k, k]; shifts written out tap by tap, zero outside the image, never across images"""
    C, k = w.shape[0], w.shape[-1]
    R = k // 2
    xi, di = x.view(B, H, W, C), du.view(B, H, W, C)
    xp, dp = F.pad(xi, (0, 0, R, R, R, R)), F.pad(di, (0, 0, R, R, R, R))
    dx = torch.zeros_like(xi)
    dw = torch.zeros_like(w)
    for ky in range(k):
        for kx in range(k):
            # du[(y - ky + R, x - kx + R)] = dp[y - ky + 2R, x - kx + 2R];  in[(y + ky - R, x + kx - R)] = xp[y + ky, x + kx]
            dx = dx + w[:, ky, kx] * dp[:, 2 * R - ky:2 * R - ky + H, 2 * R - kx:2 * R - kx + W]
            dw[:, ky, kx] = (di * xp[:, ky:ky + H, kx:kx + W]).sum((0, 1, 2))
    return dx.reshape(-1, C), dw, du.sum(0)


def gelu_bwd_ref(x, dy):
    """(d)"""
    return dy * (0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi))


# ---------------------------------------------------------------------------------------------------------------------
# the ConvGRU gate epilogues, restated on what a launch consumed
# ---------------------------------------------------------------------------------------------------------------------
def conv64(srcs, reals, weight, bias, res, b, h, w, kh, kw):
    """fp64 'same' convolution of pixel-major rows: cat(src[:, :real]) x weight [cout, sum(reals), kh, kw] + bias + res, [M, cout]"""
    x = torch.cat([s.cpu()[:, :r].double() for s, r in zip(srcs, reals)], 1)
    x = x.reshape(b, h, w, -1).permute(0, 3, 1, 2)
    v = F.conv2d(x, weight.double(), padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1).reshape(b * h * w, -1)
    if bias is not None:
        v = v + bias.double().cpu()
    if res is not None:
        v = v + res.double().cpu()
    return v


def ref_zr(srcs, reals, weight, bias, res, h_rows, shape, k):
    """z = sigmoid(v[:, :Ch]), r*h = sigmoid(v[:, Ch:]) * h, v = conv + bias + residual (K8b: h is the bf16 twin)"""
    v = conv64(srcs, reals, weight, bias, res, *shape, *k)
    Ch = v.shape[1] // 2
    return torch.sigmoid(v[:, :Ch]), torch.sigmoid(v[:, Ch:]) * h_rows.double().cpu()


def ref_q(srcs, reals, weight, bias, res, z_rows, h_rows, shape, k):
    """h' = (1 - z) h + z tanh(conv + bias + residual), on the z the z|r launch stored and the fp32 h"""
    v = conv64(srcs, reals, weight, bias, res, *shape, *k)
    z, h = z_rows.double().cpu(), h_rows.double().cpu()
    return (1 - z) * h + z * torch.tanh(v)


# ---------------------------------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------------------------------
def coords_cases(B, h, w):
    """(name, [B, 2, h, w] lookup coordinates): integer, fractional, half-pixel, far outside, on the edges, non-finite"""
    g = torch.Generator().manual_seed(7)
    c0 = O.coords_grid(B, h, w)
    yield "integer", c0
    yield "fractional", c0 + torch.rand(B, 2, h, w, generator=g) * 16 - 8
    yield "half", c0 + 0.5
    yield "out_of_bounds", c0 + torch.randn(B, 2, h, w, generator=g) * 80
    edge = c0.clone()
    edge[:, 0] = torch.where(edge[:, 0] < w / 2, -0.25, w - 0.75)
    edge[:, 1] = torch.where(edge[:, 1] < h / 2, -1.0, float(h - 1))
    yield "edges", edge
    bad = c0.clone()
    bad[:, 0, 0, 0] = float("nan")
    bad[:, 1, 0, 1] = float("inf")
    bad[:, 0, 1, 0] = -float("inf")
    bad[:, 0, 1, 1] = 3.0e9
    bad[:, 1, 1, 2] = -2.5e7
    yield "nonfinite", bad


@functools.lru_cache(maxsize=None)
def convex_case(B, H, W, logit_scale):
    """fp32 inputs of the convex-upsampling backward, its float64 gradients and their sums of magnitudes; once per case"""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W + int(logit_scale))
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    mask = torch.randn(B, 576, H, W, generator=g) * logit_scale
    go = torch.randn(B, 2, 8 * H, 8 * W, generator=g)
    f64, m64, g64 = flow.double().requires_grad_(), mask.double().requires_grad_(), go.double()
    out = O.convex_upsample(f64, m64)
    gflow, gmask = torch.autograd.grad((out * g64).sum(), (f64, m64), retain_graph=True)
    (gflow_mag,) = torch.autograd.grad((out * g64.abs()).sum(), f64)        # the softmax weights are >= 0: sum of 8 w |g|
    # magnitudes of dmask[k] = w_k (dw_k - sum_j w_j dw_j), dw_k = g_x v_x,k + g_y v_y,k
    with torch.no_grad():
        m = m64.view(B, 1, 9, 8, 8, H, W)
        wgt = torch.softmax(m, dim=2)[:, 0]                                                          # [B, 9, 8, 8, H, W]
        spread = (m.amax(2) - m.amin(2))[:, 0]                                                       # [B, 8, 8, H, W]
        up = F.unfold(8 * f64, [3, 3], padding=1).view(B, 2, 9, 1, 1, H, W).abs()
        gsub = g64.view(B, 2, H, 8, W, 8).permute(0, 1, 3, 5, 2, 4).abs()                            # [B, 2, sy, sx, H, W]
        T = (gsub[:, :, None] * up).sum(1)                                                           # [B, 9, 8, 8, H, W]
        gmask_mag = wgt * (T + (wgt * T).sum(1, keepdim=True))
    pm = lambda t: t.reshape(B, 576, H, W).permute(0, 2, 3, 1).reshape(B * H * W, 576)
    # K: a softmax weight is off by at most (2 spread + 19) units of 2^-24 relative — the rounded differences m_k - max in the
    # numerator and in the denominator (spread each), expf within 2 ulp twice (4 + 4), nine additions, the reciprocal, the product;
    # dmask then has its weight, dw_k (3 roundings), the dot (each term a weight, a dw, a product; nine additions), the subtraction
    # and the last product: at most 2 (2 spread + 19) + 15 on the magnitudes above.
    k_w = 2 * spread + 19
    k_mask = pm((2 * k_w + 15)[:, None].expand(B, 9, 8, 8, H, W))
    return {"flow": flow, "mask": mask, "go": go, "gflow": gflow, "gflow_mag": gflow_mag, "gmask": pm(gmask), "gmask_mag": pm(gmask_mag),
            "k_mask": k_mask, "k_flow": 9 * 64 + float(k_w.max()) + 2}
