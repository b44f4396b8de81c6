"""TEST INFRASTRUCTURE.  A torch-only stand-in for CCMR's motion aggregator, the XCiT block of ptlflow/models/ccmr/xcit.py, with the
reference's state_dict names and shapes — for machines without the reference tree (and without timm), in the same category as
tests/seam_model.py.  Written from the description of the module, not from its text:

    tokens x = rows(x_nchw) [+ pos],  v = rows(x_v)                              pos: a Fourier encoding of the pixel grid, projected 64 -> dim
    x = x + gamma1 * proj(A @ to_v(norm1(v)))        A = softmax_j(temperature * normalize(q) normalize(k)^T), q | k = to_qk(norm1(x)),
                                                     per head over the head's 16 channels, the norms over the tokens (`separate`)
      (not `separate`: q | k | v = qkv(norm1(x)), one input)
    x = x + gamma3 * conv2(GroupNorm8(GELU(conv1(norm3(x)))))                     depthwise 3x3 convolutions on the H x W grid
    x = x + gamma2 * fc2(GELU(fc1(norm2(x))))

DropPath is the identity in eval and the dropouts have p = 0.  tests/test_xcit_cpu.py pins it to outputs recorded from the reference
(tests/golden/ccmr_aggregator.pt) and, where the reference is available, to its state_dict names and shapes.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class PositionalEncodingFourier(nn.Module):
    """sin / cos of the normalised (y, x) pixel position at 32 frequencies each, then a 1x1 projection to `dim` channels"""

    def __init__(self, hidden_dim: int = 32, dim: int = 128, temperature: float = 10000.0):
        super().__init__()
        self.token_projection = nn.Conv2d(hidden_dim * 2, dim, kernel_size=1)
        self.scale = 2 * math.pi
        self.temperature = temperature
        self.hidden_dim = hidden_dim
        self.dim = dim

    def forward(self, B: int, H: int, W: int, dtype=torch.float32):
        dev = self.token_projection.weight.device
        eps = 1e-6
        y = torch.arange(1, H + 1, dtype=dtype, device=dev)
        x = torch.arange(1, W + 1, dtype=dtype, device=dev)
        y = (y / (y[-1:] + eps) * self.scale)[None, :, None].expand(B, H, W)
        x = (x / (x[-1:] + eps) * self.scale)[None, None, :].expand(B, H, W)
        k = torch.arange(self.hidden_dim, dtype=dtype, device=dev)
        freq = self.temperature ** (2 * torch.div(k, 2, rounding_mode="floor") / self.hidden_dim)

        def enc(p):
            p = p[:, :, :, None] / freq
            return torch.stack((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=4).flatten(3)

        pos = torch.cat((enc(y), enc(x)), dim=3).permute(0, 3, 1, 2)
        return self.token_projection(pos)


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class LPI(nn.Module):
    """local patch interaction: two depthwise 3x3 convolutions with GELU and GroupNorm(8) in between"""

    def __init__(self, dim: int):
        super().__init__()
        self.conv1 = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.act = nn.GELU()
        self.bn = nn.GroupNorm(num_groups=8, num_channels=dim)
        self.conv2 = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)

    def forward(self, x, H: int, W: int):
        B, N, C = x.shape
        x = x.permute(0, 2, 1).reshape(B, C, H, W)
        x = self.conv2(self.bn(self.act(self.conv1(x))))
        return x.reshape(B, C, N).permute(0, 2, 1)


def _xca(q, k, v, temperature):
    """q, k, v [B, heads, dh, N] -> [B, N, heads * dh]"""
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * temperature).softmax(dim=-1)
    out = attn @ v
    B, h, d, N = out.shape
    return out.permute(0, 3, 1, 2).reshape(B, N, h * d), attn


class XCA(nn.Module):
    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = True):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 4, 1)
        return self.proj(_xca(q, k, v, self.temperature)[0])


class XCA_separate(nn.Module):
    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = True):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.to_qk = nn.Linear(dim, dim * 2, bias=qkv_bias)
        self.to_v = nn.Linear(dim, dim, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.last_attn = None      # the map of the last call (tests)

    def forward(self, x_qk, x_v):
        B, N, C = x_qk.shape
        h = self.num_heads
        q, k = self.to_qk(x_qk).reshape(B, N, 2, h, C // h).permute(2, 0, 3, 4, 1)
        v = self.to_v(x_v).reshape(B, N, h, C // h).permute(0, 2, 3, 1)
        out, self.last_attn = _xca(q, k, v, self.temperature)
        return self.proj(out)


class XCABlock(nn.Module):
    def __init__(self, dim: int, num_heads: int = 8, mlp_ratio: float = 1, qkv_bias: bool = True, separate: bool = False,
                 eta: float = 1.0, eps: float = 1e-6):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.separate = separate
        self.attn = XCA_separate(dim, num_heads, qkv_bias) if separate else XCA(dim, num_heads, qkv_bias)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.norm3 = nn.LayerNorm(dim, eps=eps)
        self.local_mp = LPI(dim)
        self.gamma1 = nn.Parameter(eta * torch.ones(dim))
        self.gamma2 = nn.Parameter(eta * torch.ones(dim))
        self.gamma3 = nn.Parameter(eta * torch.ones(dim))
        self.last = {}             # x1, x2 of the last call (tests)

    def forward(self, x, H: int, W: int, x_v=None):
        if self.separate:
            x = x + self.gamma1 * self.attn(self.norm1(x), self.norm1(x_v))
        else:
            x = x + self.gamma1 * self.attn(self.norm1(x))
        x1 = x
        x = x + self.gamma3 * self.local_mp(self.norm3(x), H, W)
        self.last = {"x1": x1, "x2": x}
        return x + self.gamma2 * self.mlp(self.norm2(x))


class XCiT(nn.Module):
    """`forward(x, x_v)` on NCHW tensors; with `separate` the queries and keys come from `x` (+ the positional encoding), the values
    from `x_v`, and there is one block whatever `depth` says"""

    def __init__(self, embed_dim: int = 128, depth: int = 1, num_heads: int = 8, mlp_ratio: float = 1, qkv_bias: bool = True,
                 use_pos: bool = True, eta: float = 1.0, separate: bool = False, eps: float = 1e-6):
        super().__init__()
        self.embed_dim = embed_dim
        self.separate = separate
        if separate:
            depth = 1
        self.blocks = nn.ModuleList([XCABlock(embed_dim, num_heads, mlp_ratio, qkv_bias, separate, eta, eps) for _ in range(depth)])
        self.pos_embeder = PositionalEncodingFourier(dim=embed_dim)
        self.use_pos = use_pos

    def forward(self, x, x_v=None):
        B, C, H, W = x.shape
        x = x.flatten(2).transpose(1, 2)
        if self.use_pos:
            x = x + self.pos_embeder(B, H, W, x.dtype).reshape(B, -1, x.shape[1]).permute(0, 2, 1)
        if self.separate:
            x_v = x_v.flatten(2).transpose(1, 2)
        for blk in self.blocks:
            x = blk(x, H, W, x_v=x_v) if self.separate else blk(x, H, W)
        return x.permute(0, 2, 1).reshape(B, -1, H, W)


def randomize(model: nn.Module, seed: int = 0) -> nn.Module:
    """seeded, non-trivial parameters: gamma in [0.2, 1], temperature in [0.5, 2.5], non-unit norm weights, non-zero biases,
    weights at a scale that keeps the activations O(1)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo  # noqa: E731
    with torch.no_grad():
        for name, p in model.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if leaf.startswith("gamma"):
                v = u(p.shape, 0.2, 1.0)
            elif leaf == "temperature":
                v = u(p.shape, 0.5, 2.5)
            elif leaf == "bias":
                v = u(p.shape, -0.3, 0.3)
            elif p.dim() == 1:                          # norm weights
                v = u(p.shape, 0.5, 1.5)
            else:                                       # linear / convolution weights: uniform, variance 1 / fan_in
                fan_in = p[0].numel()
                v = u(p.shape, -1.0, 1.0) * math.sqrt(3.0 / fan_in)
            p.copy_(v.to(p.dtype))
    return model


# the model's own (module, class) key for `PfkUpdateBlock`, as INTEGRATION.md documents for further families
def register() -> None:
    from ptlflow_amd.xcit import register_xcit_aggregator
    register_xcit_aggregator(XCiT.__module__, "XCiT")
