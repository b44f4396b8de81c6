"""TEST INFRASTRUCTURE.  A torch-only stand-in for the six multi-scale GroupNorm encoders — `fnet` / `cnet` of CCMR, CCMR+
(ptlflow/models/ccmr/extractor.py) and MS-RAFT+ (ptlflow/models/ms_raft_plus/extractor.py) — with the reference's state_dict names and
arithmetic, for machines without the reference tree; in the same category as tests/xcit_model.py.  Written from the description of
the modules, not from their text:

    x  = relu(GN(conv1_7x7/2(img)))                                     64 channels at 1/2 resolution
    e1 = layer1(x), e2 = layer2(e1), e3 = layer3(e2)                    pairs of residual blocks: 64, 96 (/2), 128 (/2)
    e4 = conv2_1x1(layer4(e3))                                          160 (/2), then `out_dim` channels at 1/16
    u2 = [after2](up_layer2(cat(resize(e4 -> e3's size), e3)))          the bottom-up path: bilinear resize (antialias on, which for
    u1 = [after1](up_layer1(cat(resize(u2 -> e2's size), e2)))          upsizing is plain bilinear), the coarser map IN FRONT of the
    u0 = [after0](up_layer0(cat(resize(u1 -> e1's size), e1)))          skip, two blocks, and for CCMR a 1x1 convolution
    returns [e4, u2, u1(, u0)]; a feature encoder is fed a pair of images and returns every level as the pair's two halves

A residual block is relu(GN(conv3x3(.)))) twice, added to its input (through a 1x1 stride-2 convolution + GN where it strides) and
relu'd — except where the block changes the width without striding (the first block of an up level): there it returns the branch alone.
Every GroupNorm has 8 channels per group.  tests/test_msenc_cpu.py pins the stand-in to outputs recorded from the reference's classes
(tests/golden/ms_encoders*.pt, scripts/make_golden_ms_encoders.py).

Also here: the seeded parameter recipe (`recipe_state_dict`) and `MsModel`, the smallest model that carries `fnet` / `cnet`.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

GROUP = 8


def _norm(norm_fn: str, planes: int, group: int):
    if norm_fn == "group":
        return nn.GroupNorm(planes // group, planes)
    if norm_fn == "batch":
        return nn.BatchNorm2d(planes)
    if norm_fn == "instance":
        return nn.InstanceNorm2d(planes)
    raise ValueError(norm_fn)


class ResidualBlock(nn.Module):
    def __init__(self, in_planes: int, planes: int, norm_fn: str = "group", stride: int = 1, group: int = GROUP):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = _norm(norm_fn, planes, group)
        self.norm2 = _norm(norm_fn, planes, group)
        self.downsample = None
        if stride != 1:
            self.norm3 = _norm(norm_fn, planes, group)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return y if x.shape[1] != y.shape[1] else self.relu(x + y)


class MultiScaleEncoder(nn.Module):
    """`planes`: the widths of up_layer2, up_layer1(, up_layer0); `after`: the output widths of the 1x1 convolutions behind them or None;
    `model_type`: the attribute the CCMR classes carry ("CCMR": two up levels, "CCMR+": three), None for MS-RAFT+'s"""
    split_pairs = False

    def __init__(self, out_dim: int, planes: Sequence[int], after: Optional[Sequence[int]] = None, model_type: Optional[str] = None,
                 norm_fn: str = "group", group: int = GROUP):
        super().__init__()
        self.norm_fn = norm_fn
        if model_type is not None:
            self.model_type = model_type
        self.norm1 = _norm(norm_fn, 64, group)
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)

        def pair(cin, cout, stride):
            return nn.Sequential(ResidualBlock(cin, cout, norm_fn, stride, group), ResidualBlock(cout, cout, norm_fn, 1, group))

        self.layer1, self.layer2, self.layer3, self.layer4 = pair(64, 64, 1), pair(64, 96, 2), pair(96, 128, 2), pair(128, 160, 2)
        self.conv2 = nn.Conv2d(160, out_dim, 1)
        coarse = out_dim
        self.levels = []
        for i, (n, skip) in enumerate(((2, 128), (1, 96), (0, 64))[:len(planes)]):
            setattr(self, f"up_layer{n}", pair(coarse + skip, planes[i], 1))
            coarse = planes[i]
            if after is not None:
                setattr(self, f"after_up_layer{n}_conv", nn.Conv2d(planes[i], after[i], 1))
                coarse = after[i]
            self.levels.append(n)

    def forward(self, x):
        is_list = isinstance(x, (tuple, list))
        if is_list:
            batch_dim = x[0].shape[0]
            x = torch.cat(list(x), dim=0)
        x = self.relu1(self.norm1(self.conv1(x)))
        skips = {}
        for i in (1, 2, 3):
            x = getattr(self, f"layer{i}")(x)
            skips[i] = x
        x = self.conv2(self.layer4(x))
        outs = [x]
        for n in self.levels:
            skip = skips[n + 1]
            x = F.interpolate(x, size=skip.shape[-2:], mode="bilinear", align_corners=False, antialias=True)
            x = getattr(self, f"up_layer{n}")(torch.cat((x, skip), dim=1))
            after = getattr(self, f"after_up_layer{n}_conv", None)
            if after is not None:
                x = after(x)
            outs.append(x)
        if self.split_pairs:
            return [torch.split(o, [batch_dim, batch_dim], dim=0) for o in outs]
        return outs


class MsFeatureEncoder(MultiScaleEncoder):
    split_pairs = True


class MsContextEncoder(MultiScaleEncoder):
    pass


# key -> (stand-in class, constructor arguments, (reference module, class, constructor arguments))
ENCODERS: Dict[str, Tuple[type, dict, Tuple[str, str, dict]]] = {
    "ccmr_fnet": (MsFeatureEncoder, dict(out_dim=160, planes=(128, 96), after=(128, 96), model_type="CCMR"),
                  ("ptlflow.models.ccmr.extractor", "BasicEncoder_resconv", dict(output_dim=256, norm_fn="group", model_type="CCMR"))),
    "ccmr_cnet": (MsContextEncoder, dict(out_dim=256, planes=(128, 96), after=(256, 256), model_type="CCMR"),
                  ("ptlflow.models.ccmr.extractor", "Basic_Context_Encoder_resconv", dict(output_dim=256, norm_fn="group", model_type="CCMR"))),
    "ccmrp_fnet": (MsFeatureEncoder, dict(out_dim=160, planes=(128, 96, 64), after=(128, 96, 64), model_type="CCMR+"),
                   ("ptlflow.models.ccmr.extractor", "BasicEncoder_resconv", dict(output_dim=256, norm_fn="group", model_type="CCMR+"))),
    "ccmrp_cnet": (MsContextEncoder, dict(out_dim=256, planes=(128, 96, 64), after=(256, 256, 256), model_type="CCMR+"),
                   ("ptlflow.models.ccmr.extractor", "Basic_Context_Encoder_resconv", dict(output_dim=256, norm_fn="group", model_type="CCMR+"))),
    "msraft_fnet": (MsFeatureEncoder, dict(out_dim=256, planes=(128, 96, 64)),
                    ("ptlflow.models.ms_raft_plus.extractor", "BasicEncoder", dict(output_dim=256, norm_fn="group"))),
    "msraft_cnet": (MsContextEncoder, dict(out_dim=256, planes=(256, 256, 256)),
                    ("ptlflow.models.ms_raft_plus.extractor", "Basic_Context_Encoder", dict(output_dim=256, norm_fn="group"))),
}
SEEDS = {k: 2600 + i for i, k in enumerate(ENCODERS)}


def make(key: str, **overrides) -> MultiScaleEncoder:
    cls, kw, _ref = ENCODERS[key]
    return cls(**{**kw, **overrides})


def recipe_state_dict(shapes: Dict[str, tuple], seed: int, dtype: torch.dtype = torch.float32) -> Dict[str, torch.Tensor]:
    """Seeded parameters for the state_dict `shapes`, drawn in float64 on the CPU and cast: convolution weights randn * sqrt(2 /
    fan_in), convolution biases 0.1 randn, GroupNorm gamma = 1 + 0.3 randn and beta = 0.2 randn (the default 1 / 0 would hide an
    affine bug).  Every tensor has a generator of its own, seeded by its NAME, so the values do not depend on the order in which a
    module registers its parameters; `downsample.1` is `norm3` under another name and draws the same values."""
    sd = {}
    for name, shape in shapes.items():
        canon = name.replace("downsample.1.", "norm3.")
        g = torch.Generator().manual_seed(seed * 1000003 + zlib.crc32(canon.encode()))
        r = torch.randn(tuple(shape), generator=g, dtype=torch.float64)
        is_norm = any(part.startswith("norm") for part in canon.split("."))
        if len(shape) == 4:
            v = r * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif is_norm:
            v = 1.0 + 0.3 * r if canon.endswith(".weight") else 0.2 * r
        else:
            v = 0.1 * r
        sd[name] = v.to(dtype)
    return sd


def randomize(module: nn.Module, seed: int) -> nn.Module:
    """`module` with the recipe's parameters, in its own dtype"""
    sd = module.state_dict()
    dtype = next(iter(sd.values())).dtype
    module.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed, dtype), strict=True)
    return module


def golden_input(seed: int = 2599) -> torch.Tensor:
    """[2, 3, 32, 48] float64: the pair the feature encoders are fed; the context encoders get its first image"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 32, 48, generator=g, dtype=torch.float64)


class MsModel(nn.Module):
    """the smallest model with the seams `accelerate(..., multiscale_encoders=True)` patches: `fnet` on the pair, `cnet` on image 1"""

    def __init__(self, family: str = "ccmrp", seed: int = 77):
        super().__init__()
        self.fnet = randomize(make(f"{family}_fnet"), seed)
        self.cnet = randomize(make(f"{family}_cnet"), seed + 1)

    def forward(self, image1, image2):
        return self.fnet([image1, image2]), self.cnet(image1)


def register() -> None:
    """make `accelerate` serve the stand-in classes"""
    from ptlflow_amd.ms_encoder import register_multiscale_encoder
    register_multiscale_encoder(MsFeatureEncoder.__module__, "MsFeatureEncoder", True)
    register_multiscale_encoder(MsContextEncoder.__module__, "MsContextEncoder", False)
