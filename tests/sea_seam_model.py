"""TEST INFRASTRUCTURE: a torch-only SEA-RAFT refinement loop laid out like ptlflow's (ptlflow/models/sea_raft), written for this
project against torch only, so the SEA-RAFT seams (`patch.accelerate(model, sea_raft_update=True)`, ptlflow_amd/sea_update.py)
can be exercised where neither the reference tree nor its staged archive exists.

* `BasicUpdateBlock` has the reference's module names and parameter shapes (sea_raft/update.py:18-54, layer.py:44-99):
  `encoder.convc1 ... encoder.conv`, `refine.{i}.dwconv / norm / pwconv1 / pwconv2 / gamma / final`;
* `SeaRaftLoop` holds `update_block`, `flow_head`, `upsample_weight` (sea_raft.py:114-126) and `upsample_data` (:147-163) and runs
  the loop of sea_raft.py:190-236 from `net`, `context` and the two feature maps (no ResNet-FPN encoders): `get_corr_block` is a
  global of this module (the B1 hook rebinds it) building the torch correlation block of tests/seam_model.py.

The block registers itself with `patch` at import (bottom of the file).  `seeded_params` draws every parameter in name-sorted order
from one seed, with the layer scale `gamma` at O(1) (the reference's 1e-6 init would hide the ConvNeXt branch).
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from seam_model import TorchCorrBlock


def get_corr_block(fmap1, fmap2, num_levels: int = 4, radius: int = 4, alternate_corr: bool = False):
    """The module global `patch.accelerate` rebinds (sea_raft.py:10 binds the family's own)."""
    return TorchCorrBlock(fmap1, fmap2, num_levels=num_levels, radius=radius)


class BasicMotionEncoder(nn.Module):
    def __init__(self, corr_channels: int, dim: int = 128):
        super().__init__()
        self.convc1 = nn.Conv2d(corr_channels, 2 * dim, 1)
        self.convc2 = nn.Conv2d(2 * dim, dim + dim // 2, 3, padding=1)
        self.convf1 = nn.Conv2d(2, dim, 7, padding=3)
        self.convf2 = nn.Conv2d(dim, dim // 2, 3, padding=1)
        self.conv = nn.Conv2d(2 * dim, dim - 2, 3, padding=1)

    def forward(self, flow, corr):
        c = F.relu(self.convc2(F.relu(self.convc1(corr))))
        f = F.relu(self.convf2(F.relu(self.convf1(flow))))
        return torch.cat([F.relu(self.conv(torch.cat([c, f], 1))), flow], 1)


class LayerNorm(nn.Module):
    """channels-last LayerNorm with `weight` / `bias` parameters (layer.py:86-99)"""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))
        self.eps = eps

    def forward(self, x):
        return F.layer_norm(x, (x.shape[-1],), self.weight, self.bias, self.eps)


class ConvNextBlock(nn.Module):
    def __init__(self, dim: int, out_dim: int, layer_scale: float = 1e-6):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = LayerNorm(dim)
        self.pwconv1 = nn.Linear(dim, 4 * out_dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * out_dim, dim)
        self.gamma = nn.Parameter(torch.full((dim,), layer_scale))
        self.final = nn.Conv2d(dim, out_dim, 1)

    def forward(self, x):
        y = self.norm(self.dwconv(x).permute(0, 2, 3, 1))
        y = self.gamma * self.pwconv2(self.act(self.pwconv1(y)))
        return self.final(x + y.permute(0, 3, 1, 2))


class BasicUpdateBlock(nn.Module):
    def __init__(self, corr_channels: int = 324, num_blocks: int = 2, hdim: int = 128, cdim: int = 128):
        super().__init__()
        self.encoder = BasicMotionEncoder(corr_channels, cdim)
        self.refine = nn.ModuleList([ConvNextBlock(2 * cdim + hdim, hdim) for _ in range(num_blocks)])

    def forward(self, net, inp, corr, flow):
        x = torch.cat([inp, self.encoder(flow, corr)], 1)
        for blk in self.refine:
            net = blk(torch.cat([net, x], 1))
        return net


def coords_grid(b: int, h: int, w: int, device=None) -> torch.Tensor:
    y, x = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32), torch.arange(w, device=device, dtype=torch.float32),
                          indexing="ij")
    return torch.stack([x, y], 0)[None].repeat(b, 1, 1, 1)


def upsample_data_torch(flow, info, mask):
    """SEARAFT.upsample_data restated: softmax over the 9 taps, convex combination of the 3x3 neighbourhoods, pixel shuffle"""
    N, C, H, W = info.shape
    m = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), dim=2)
    f = F.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    i = F.unfold(info, [3, 3], padding=1).view(N, C, 9, 1, 1, H, W)
    f = torch.sum(m * f, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)
    i = torch.sum(m * i, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, C, 8 * H, 8 * W)
    return f, i


class SeaRaftLoop(nn.Module):
    def __init__(self, iters: int = 4, corr_levels: int = 4, corr_radius: int = 4, num_blocks: int = 2, dim: int = 128):
        super().__init__()
        self.iters, self.corr_levels, self.corr_radius = iters, corr_levels, corr_radius
        self.upsample_weight = nn.Sequential(nn.Conv2d(dim, 2 * dim, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(2 * dim, 576, 1))
        self.flow_head = nn.Sequential(nn.Conv2d(dim, 2 * dim, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(2 * dim, 6, 3, padding=1))
        self.update_block = BasicUpdateBlock(corr_levels * (2 * corr_radius + 1) ** 2, num_blocks, dim, dim)

    def upsample_data(self, flow, info, mask):
        return upsample_data_torch(flow, info, mask)

    def forward(self, net, context, fmap1, fmap2, iters=None):
        iters = self.iters if iters is None else iters
        N, _, H, W = net.shape
        flow_update = self.flow_head(net)
        weight_update = 0.25 * self.upsample_weight(net)
        flow_8x, info_8x = flow_update[:, :2], flow_update[:, 2:]
        flow_up, info_up = self.upsample_data(flow_8x, info_8x, weight_update)
        flows, infos = [flow_up], [info_up]
        corr_fn = get_corr_block(fmap1=fmap1, fmap2=fmap2, num_levels=self.corr_levels, radius=self.corr_radius)
        for _ in range(iters):
            flow_8x = flow_8x.detach()
            coords2 = (coords_grid(N, H, W, device=net.device) + flow_8x).detach()
            corr = corr_fn(coords2)
            net = self.update_block(net, context, corr, flow_8x)
            flow_update = self.flow_head(net)
            weight_update = 0.25 * self.upsample_weight(net)
            flow_8x = flow_8x + flow_update[:, :2]
            info_8x = flow_update[:, 2:]
            flow_up, info_up = self.upsample_data(flow_8x, info_8x, weight_update)
            flows.append(flow_up)
            infos.append(info_up)
        return {"flows": flow_up[:, None], "info": info_up, "flow_small": flow_8x, "flow_preds": flows, "info_preds": infos}


def seeded_params(named_shapes: Dict[str, tuple], seed: int = 0) -> Dict[str, torch.Tensor]:
    """One tensor per parameter, drawn in name-sorted order from `seed`: weights ~ N(0, 1/fan_in), biases ~ 0.1 N(0, 1), LayerNorm
    weights 1 + 0.1 N(0, 1), the layer scale `gamma` ~ U(0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(named_shapes):
        shape = tuple(named_shapes[name])
        if name.endswith("gamma"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("norm.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            t = torch.randn(shape, generator=g) / max(fan_in, 1) ** 0.5
        out[name] = t
    return out


def load_seeded(module: nn.Module, seed: int = 0) -> nn.Module:
    sd = module.state_dict()
    P = seeded_params({k: tuple(v.shape) for k, v in sd.items()}, seed)
    module.load_state_dict(P, strict=True)
    return module


def _register() -> None:
    from ptlflow_amd import patch
    patch.register_sea_raft_update_block(__name__, "BasicUpdateBlock")


_register()
