"""TEST INFRASTRUCTURE: a torch-only SEA-RAFT from the images on, laid out like ptlflow's (ptlflow/models/sea_raft), written for this
project against torch only, so `patch.accelerate(model, sea_raft_encoders=...)` (ptlflow_amd/sea_encoder.py) can be exercised where
neither the reference tree nor its staged archive exists.

* `BasicBlock` / `ResNetFPN` have the reference's module names and parameter shapes (sea_raft/layer.py:126-150, extractor.py:6-116):
  `conv1 / bn1`, `layer{1,2,3}.{j}.conv1 / conv2 / bn1 / bn2`, and for a block that changes stride or width `bn3` AND `downsample.0 /
  downsample.1` — the norm is registered under both names, so the state_dict carries both key sets for one tensor; `final_conv`.
* `SeaRaftFull` adds `cnet`, `fnet` and `init_conv` to tests/sea_seam_model.py's `SeaRaftLoop` and restates sea_raft.py's `forward`
  (:186-236) from the two images on (no image normalisation / padding: the caller hands in sizes divisible by 8).  `get_corr_block`
  is a global of THIS module (the B1 hook rebinds the global of the model class's module).

`seeded_encoder_params` draws every tensor in name-sorted order from one seed: convolution weights ~ N(0, 1 / fan_in) (with the
reference's Kaiming fan-out initialisation the ResNet-34 output reaches 1e4, which makes absolute gates meaningless), biases and running
means ~ 0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1), running variances ~ U(0.5, 1.5); `downsample.1.*` repeats `bn3.*`.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn as nn

import sea_seam_model
from seam_model import TorchCorrBlock
from sea_seam_model import SeaRaftLoop, coords_grid

N_BLOCKS = {"resnet18": (2, 2, 2), "resnet34": (3, 4, 6)}


def get_corr_block(fmap1, fmap2, num_levels: int = 4, radius: int = 4, alternate_corr: bool = False):
    """The module global `patch.accelerate` rebinds (sea_raft.py:10 binds the family's own)."""
    return TorchCorrBlock(fmap1, fmap2, num_levels=num_levels, radius=radius)


class BasicBlock(nn.Module):
    def __init__(self, in_planes: int, planes: int, stride: int = 1, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, stride=stride, padding=1)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1)
        self.bn1 = norm_layer(planes)
        self.bn2 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or in_planes != planes:
            self.bn3 = norm_layer(planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride), self.bn3)

    def forward(self, x):
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class ResNetFPN(nn.Module):
    def __init__(self, block_dims: Sequence[int] = (64, 128, 256), initial_dim: int = 64, pretrain: str = "resnet18", input_dim: int = 3,
                 output_dim: int = 256, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.input_dim = input_dim
        self.conv1 = nn.Conv2d(input_dim, initial_dim, 7, stride=2, padding=3)
        self.bn1 = norm_layer(initial_dim)
        self.relu = nn.ReLU(inplace=True)
        cin = initial_dim
        for i, (dim, stride, n) in enumerate(zip(block_dims, (1, 2, 2), N_BLOCKS[pretrain]), start=1):
            blocks = [BasicBlock(cin, dim, stride, norm_layer)] + [BasicBlock(dim, dim, 1, norm_layer) for _ in range(n - 1)]
            setattr(self, f"layer{i}", nn.Sequential(*blocks))
            cin = dim
        self.final_conv = nn.Conv2d(cin, output_dim, 1)

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        x = self.layer3(self.layer2(self.layer1(x)))
        return self.final_conv(x)


class SeaRaftFull(SeaRaftLoop):
    def __init__(self, iters: int = 4, pretrain: str = "resnet18", dim: int = 128, **kw):
        super().__init__(iters=iters, dim=dim, **kw)
        self.dim = dim
        self.cnet = ResNetFPN(pretrain=pretrain, input_dim=6, output_dim=2 * dim)
        self.init_conv = nn.Conv2d(2 * dim, 2 * dim, 3, padding=1)
        self.fnet = ResNetFPN(pretrain=pretrain, input_dim=3, output_dim=2 * dim)

    def forward(self, image1, image2, iters=None):
        iters = self.iters if iters is None else iters
        cnet = self.init_conv(self.cnet(torch.cat([image1, image2], dim=1)))
        net, context = torch.split(cnet, [self.dim, self.dim], dim=1)
        flow_update = self.flow_head(net)
        weight_update = 0.25 * self.upsample_weight(net)
        flow_8x, info_8x = flow_update[:, :2], flow_update[:, 2:]
        flow_up, info_up = self.upsample_data(flow_8x, info_8x, weight_update)
        flows, infos = [flow_up], [info_up]
        if iters > 0:
            fmap1, fmap2 = self.fnet(image1), self.fnet(image2)
            corr_fn = get_corr_block(fmap1=fmap1, fmap2=fmap2, num_levels=self.corr_levels, radius=self.corr_radius)
        for _ in range(iters):
            N, _c, H, W = flow_8x.shape
            flow_8x = flow_8x.detach()
            coords2 = (coords_grid(N, H, W, device=image1.device) + flow_8x).detach()
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


def seeded_encoder_params(named_shapes: Dict[str, tuple], seed: int = 0) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for name in sorted(named_shapes):
        shape = tuple(named_shapes[name])
        leaf = name.rsplit(".", 1)[-1]
        if ".downsample.1." in name:
            continue                                     # the second name of bn3, filled below
        if leaf == "num_batches_tracked":
            t = torch.zeros(shape, dtype=torch.long)
        elif leaf == "running_var":
            t = 0.5 + torch.rand(shape, generator=g)
        elif leaf in ("running_mean", "bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)   # a norm's weight
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            t = torch.randn(shape, generator=g) / fan_in ** 0.5
        out[name] = t
    for name in named_shapes:
        if ".downsample.1." in name:
            out[name] = out[name.replace(".downsample.1.", ".bn3.")].clone()
    return out


def load_seeded_encoder(enc: nn.Module, seed: int = 0) -> nn.Module:
    sd = enc.state_dict()
    enc.load_state_dict(seeded_encoder_params({k: tuple(v.shape) for k, v in sd.items()}, seed), strict=True)
    return enc


def seeded_full(seed: int = 0, iters: int = 4, pretrain: str = "resnet18") -> SeaRaftFull:
    """every part seeded: the loop's modules by sea_seam_model.seeded_params, the encoders by seeded_encoder_params, eval mode"""
    model = SeaRaftFull(iters=iters, pretrain=pretrain)
    for i, name in enumerate(("update_block", "flow_head", "upsample_weight", "init_conv")):
        sea_seam_model.load_seeded(getattr(model, name), seed + i)
    load_seeded_encoder(model.cnet, seed + 10)
    load_seeded_encoder(model.fnet, seed + 11)
    # the magnitudes tests/test_gpu_sea_raft.py's loop inputs have (features ~0.3, net and context ~1): with unit-variance features
    # the seeded loop's flow runs away within a few iterations and an end-point gate says nothing
    with torch.no_grad():
        for conv, k in ((model.fnet.final_conv, 0.05), (model.init_conv, 0.2)):
            conv.weight.mul_(k)
            conv.bias.mul_(k)
    return model.eval()


def smooth_images(B: int, H: int, W: int, seed: int = 0):
    """two frames in [-1, 1]: a smooth random texture and its shift by a few pixels plus a little noise"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, 3, H // 8 + 2, W // 8 + 2, generator=g)
    big = torch.nn.functional.interpolate(low, size=(H + 16, W + 16), mode="bicubic", align_corners=False).clamp(-1, 1)
    im1 = big[:, :, 8:8 + H, 8:8 + W]
    im2 = big[:, :, 6:6 + H, 5:5 + W] + 0.01 * torch.randn(B, 3, H, W, generator=g)
    return im1.contiguous(), im2.contiguous()


def _register() -> None:
    from ptlflow_amd import patch
    patch.register_resnet_encoder(__name__, "ResNetFPN")


_register()
