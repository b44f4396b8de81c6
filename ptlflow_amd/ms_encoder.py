"""The multi-scale GroupNorm encoders — ``fnet`` / ``cnet`` of CCMR, CCMR+ (ptlflow/models/ccmr/extractor.py) and MS-RAFT+
(ptlflow/models/ms_raft_plus/extractor.py) — on pixel-major fp32 rows: eval only, fp32 only, opt-in with
``accelerate(model, multiscale_encoders=True)``.

All six share one skeleton.  Top-down: RAFT's 7x7/2 stem and pairs of 3x3 ``ResidualBlock``s at widths 64 / 96 / 128 down to 1/8
resolution, continued to 160 channels at 1/16 and a 1x1 ``conv2``.  Bottom-up, per level (``up_layer2``, ``up_layer1``, and
``up_layer0`` except for plain CCMR): the coarser output resized bilinearly to the skip's size, concatenated IN FRONT of the skip
(``layer3`` / ``layer2`` / ``layer1``'s output), two more blocks — the first without a residual, its ``in_planes`` differ from its
``planes`` — and, for CCMR, a 1x1 ``after_up_layer{n}_conv``.  Every norm is a GroupNorm with 8 channels per group.

``describe_multiscale_encoder`` reads that skeleton off a module as data (or refuses it), ``MultiScaleEncoderEngine`` is
``EncoderEngine`` (encoder.py: pack loop, `_conv`, `_conv3`, the Winograd rule) with this description as its block table and

* GroupNorm (+ relu, + residual add + relu)   -> ``pfk_groupnorm_stats_f32`` + ``pfk_affine_apply_f32``, in place
* resize to the skip's size                  -> ``pfk_resize_bilinear_pm_f32``
* the concatenation                          -> never materialised: conv1 of the level's first block reads [resized, skip] as two
                                                sources of ``pfk_conv2d_f32``, its weight packed with two segments in `cat` order
* stride-1 3x3 convolutions of a square width 64 / 96 / 128 -> Winograd under encoder.py's ``WINO_MIN_PIXELS``; 160, 256 and every
                                                two-source or strided convolution stay on the direct kernel
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from ._seam import WrappedModule, eligible
from .encoder import EPS, EncoderEngine, _out

GROUP = 8          # channels per group of every GroupNorm in the six encoders
# state_dict names in EncoderEngine's form: (the stem's norm, a block's (conv, norm) pairs, the norm of its downsample path, the output conv)
_NAMES = ("norm1", (("conv1", "norm1"), ("conv2", "norm2")), "downsample.1", "conv2")
# up level n concatenates with the output of layer n + 1
_UP_LEVELS = (2, 1, 0)

# (module of the class, class name) -> the forward splits every level into the pair's two halves (the fnets do, the cnets do not);
# extendable with `register_multiscale_encoder`
_MS_CLASSES: Dict[Tuple[str, str], bool] = {
    ("ptlflow.models.ccmr.extractor", "BasicEncoder_resconv"): True,
    ("ptlflow.models.ccmr.extractor", "Basic_Context_Encoder_resconv"): False,
    ("ptlflow.models.ms_raft_plus.extractor", "BasicEncoder"): True,
    ("ptlflow.models.ms_raft_plus.extractor", "Basic_Context_Encoder"): False,
}


def register_multiscale_encoder(module: str, cls: str, split_pairs: bool) -> None:
    """Serve the class `cls` of `module` as well (an instance must still pass `describe_multiscale_encoder`).  `split_pairs`: its
    forward hands every level back as the two halves of the batch (a feature encoder fed an image pair)."""
    _MS_CLASSES[(module, cls)] = bool(split_pairs)


def served(module: torch.nn.Module) -> bool:
    return (type(module).__module__, type(module).__name__) in _MS_CLASSES


def _is_conv(m, cin: int, cout: int, k: int, stride: int) -> bool:
    return (type(m) is torch.nn.Conv2d and m.in_channels == cin and m.out_channels == cout and m.kernel_size == (k, k)
            and m.stride == (stride, stride) and m.padding == (k // 2, k // 2) and m.dilation == (1, 1) and m.groups == 1
            and m.padding_mode == "zeros" and m.bias is not None)


def _is_gn(m, channels: int) -> bool:
    return (type(m) is torch.nn.GroupNorm and m.num_channels == channels and m.num_groups * GROUP == channels and m.eps == EPS
            and m.affine)


def _describe_block(blk, name: str, cin: int, cout: int, stride: int, norms: List[str]) -> bool:
    """one ResidualBlock: conv1 3x3 (stride), conv2 3x3, GroupNorms, and for stride 2 `downsample` = (1x1 stride-2 conv, norm3)"""
    if not (_is_conv(getattr(blk, "conv1", None), cin, cout, 3, stride) and _is_conv(getattr(blk, "conv2", None), cout, cout, 3, 1)
            and _is_gn(getattr(blk, "norm1", None), cout) and _is_gn(getattr(blk, "norm2", None), cout)
            and type(getattr(blk, "relu", None)) is torch.nn.ReLU):
        return False
    norms += [f"{name}.norm1", f"{name}.norm2"]
    ds = getattr(blk, "downsample", None)
    if stride == 1:
        return ds is None and not hasattr(blk, "norm3")
    if not (type(ds) is torch.nn.Sequential and len(ds) == 2 and _is_conv(ds[0], cin, cout, 1, stride) and ds[0].padding == (0, 0)
            and _is_gn(ds[1], cout) and ds[1] is getattr(blk, "norm3", None)):
        return False
    norms += [f"{name}.norm3", f"{name}.downsample.1"]       # one module under two names
    return True


def describe_multiscale_encoder(module: torch.nn.Module) -> Optional[dict]:
    """The skeleton of the module docstring read off `module`, or None where anything differs from what the engine computes: a
    convolution's kernel, stride, padding or groups, ``norm_fn != "group"``, a norm that is not an affine GroupNorm of 8 channels per
    group with eps 1e-5, a parameter that is not fp32, a state_dict entry the engine would not consume.  The class is the caller's to
    check (`served`).  Keys: ``blocks`` ((name, cin, cout, stride, has_downsample) of the down AND up blocks, `EncoderEngine`'s table),
    ``out_dim``, ``ups`` ((level, name, coarse channels, skip channels, planes, the after-conv's name or None and its
    output channels) coarse to fine), ``norms`` (the GroupNorms' state_dict prefixes), ``names`` (every state_dict key consumed)."""
    if getattr(module, "norm_fn", None) != "group":
        return None
    norms: List[str] = ["norm1"]
    convs: List[str] = ["conv1", "conv2"]
    stem = getattr(module, "conv1", None)
    if not (_is_conv(stem, 3, 64, 7, 2) and _is_gn(getattr(module, "norm1", None), 64)):
        return None
    blocks = []
    cin = 64
    widths = {}
    for i, stride in ((1, 1), (2, 2), (3, 2), (4, 2)):
        layer = getattr(module, f"layer{i}", None)
        if type(layer) is not torch.nn.Sequential or len(layer) != 2:
            return None
        cout = getattr(getattr(layer[0], "conv1", None), "out_channels", None)
        if not isinstance(cout, int):
            return None
        for j, (ci, st) in enumerate(((cin, stride), (cout, 1))):
            name = f"layer{i}.{j}"
            if not _describe_block(layer[j], name, ci, cout, st, norms):
                return None
            blocks.append((name, ci, cout, st, st != 1))
            convs += [f"{name}.conv1", f"{name}.conv2"] + ([f"{name}.downsample.0"] if st != 1 else [])
        widths[i] = cin = cout
    if (widths[1], widths[2], widths[3], widths[4]) != (64, 96, 128, 160):
        return None
    out = getattr(module, "conv2", None)
    if type(out) is not torch.nn.Conv2d or not _is_conv(out, 160, out.out_channels, 1, 1):
        return None
    ups = []
    coarse = out.out_channels
    # plain CCMR (`model_type`, an attribute of the CCMR classes only) stops at 1/4 resolution: its forward runs no `up_layer0`;
    # every other encoder has all three levels
    model_type = getattr(module, "model_type", "CCMR+")
    if model_type not in ("CCMR", "CCMR+") or (getattr(module, "up_layer0", None) is not None) != (model_type == "CCMR+"):
        return None
    for n in _UP_LEVELS if model_type == "CCMR+" else _UP_LEVELS[:2]:
        layer = getattr(module, f"up_layer{n}", None)
        if type(layer) is not torch.nn.Sequential or len(layer) != 2:
            return None
        planes = getattr(getattr(layer[0], "conv1", None), "out_channels", None)
        skip = widths[n + 1]
        if not isinstance(planes, int) or planes == coarse + skip:
            return None          # (equal widths would give the first block a residual the engine does not add)
        name = f"up_layer{n}"
        if not (_describe_block(layer[0], f"{name}.0", coarse + skip, planes, 1, norms)
                and _describe_block(layer[1], f"{name}.1", planes, planes, 1, norms)):
            return None
        blocks += [(f"{name}.0", coarse + skip, planes, 1, False), (f"{name}.1", planes, planes, 1, False)]
        convs += [f"{name}.{j}.{c}" for j in (0, 1) for c in ("conv1", "conv2")]
        after = getattr(module, f"after_up_layer{n}_conv", None)
        after_name, level_out = None, planes
        if after is not None:
            if type(after) is not torch.nn.Conv2d or not _is_conv(after, planes, after.out_channels, 1, 1):
                return None
            after_name, level_out = f"after_up_layer{n}_conv", after.out_channels
            convs.append(after_name)
        ups.append((n, name, coarse, skip, planes, after_name, level_out))
        coarse = level_out
    names = {f"{c}.{k}" for c in convs for k in ("weight", "bias")} | {f"{g}.{k}" for g in norms for k in ("weight", "bias")}
    sd = module.state_dict()
    if set(sd) != names or any(v.dtype != torch.float32 for v in sd.values()):
        return None
    return {"blocks": tuple(blocks), "out_dim": out.out_channels, "ups": tuple(ups), "norms": tuple(norms),
            "names": names}


class MultiScaleEncoderEngine(EncoderEngine):
    """Packed weights of one described encoder; `engine(img)` maps ``img`` [B, 3, H, W] fp32 to the list the reference returns, coarse
    to fine ([B, C_l, H_l, W_l], channels-last views of their row buffers).  `EncoderEngine` with the description's block table (the
    up blocks included), GroupNorm in place of the instance norm and the bottom-up path."""

    NORMS = ("group",)

    def __init__(self, params: Dict[str, torch.Tensor], desc: dict, device: torch.device):
        self.desc = desc
        self._two_source = {f"{name}.0.conv1": (coarse, skip) for _n, name, coarse, skip, _p, _a, _o in desc["ups"]}
        # `_max_batch`: the widest buffer of a forward in floats per half-resolution pixel.  Level l (0 = half resolution; a stride-2
        # block goes one down, up level n runs at level n) has 4^-l of the pixels: 256 for MS-RAFT+'s `cnet` (`up_layer0`), else 128
        wide, lvl = [desc["out_dim"] / 64], 0
        for name, _cin, cout, stride, _ds in desc["blocks"]:
            lvl = int(name[len("up_layer")]) if name.startswith("up_layer") else lvl + (stride == 2)
            wide.append(cout / 4 ** lvl)
        wide += [out / 4 ** n for n, _name, _c, _s, _p, _a, out in desc["ups"]]
        self.widest_row = max(128, math.ceil(max(wide)))
        super().__init__(params, "group", device, "fp32", blocks=desc["blocks"], names=_NAMES)

    # ------------------------------------------------------------------ weights
    def _segments(self, key: str, cin: int):
        if key in self._two_source:      # cat((resized coarse, skip), dim=1): two buffers, in that order
            coarse, skip = self._two_source[key]
            assert coarse + skip == cin
            return [(0, coarse, coarse), (coarse, skip, skip)]
        return super()._segments(key, cin)

    def pack(self, P: Dict[str, torch.Tensor]) -> None:
        super().pack(P)      # the stem, every block's convolutions (down and up) and `conv2`
        f32 = lambda t: t.detach().to(device=self.device, dtype=torch.float32).contiguous()  # noqa: E731
        for _n, _name, _c, _s, _planes, after, _o in self.desc["ups"]:
            if after is not None:
                self._put(self.w, after, *self._fold(P, after, None))
        for g in self.desc["norms"]:
            self.w[g + ".g"], self.w[g + ".beta"] = f32(P[g + ".weight"]), f32(P[g + ".bias"])

    # ------------------------------------------------------------------ kernels
    def _gn(self, x, B, HW, norm: str, relu: bool, residual=None):
        """GroupNorm `norm` (+ relu, + residual add + relu) in place on the pixel-major buffer x"""
        C = x.shape[1]
        scale = torch.empty(B * C, device=self.device, dtype=torch.float32)
        shift = torch.empty(B * C, device=self.device, dtype=torch.float32)
        self.ops.groupnorm_stats(x, B, HW, GROUP, self.w[norm + ".g"], self.w[norm + ".beta"], EPS, scale, shift,
                                 self._workspace(self.ops.groupnorm_workspace_bytes(B, HW, C)))
        self.ops.affine_apply(x, scale, shift, residual, x, B, HW, relu, residual is not None)
        return x

    def _conv2src(self, a, b, B, H, W, key, cout):
        out = torch.empty(B * H * W, cout, device=self.device, dtype=torch.float32)
        self.path.conv(self.ops, srcs=[a, b], B=B, H=H, W=W, kh=3, kw=3, weight=self.w[key + ".w"], bias=self.w[key + ".b"], cout=cout,
                       out=out)
        return out

    def _block(self, x, B, H, W, name, cout, stride, ds, skip=None):
        """ResidualBlock.forward (ccmr/extractor.py:50-59): y = relu(norm2(conv2(relu(norm1(conv1(x)))))); relu(x' + y) with x' the
        downsample path of a strided block — or y alone where the block changes the width without one (an up level's first block,
        which reads `x` and `skip` as the two halves of the reference's concatenation)"""
        Ho, Wo = _out(H, stride), _out(W, stride)
        if skip is not None:
            y = self._conv2src(x, skip, B, H, W, f"{name}.conv1", cout)
        elif stride == 1:
            y = self._conv3(x, B, H, W, f"{name}.conv1", cout)
        else:
            y = self._conv(x, B, H, W, 3, f"{name}.conv1", cout, stride)
        y = self._gn(y, B, Ho * Wo, f"{name}.norm1", relu=True)
        y = self._conv3(y, B, Ho, Wo, f"{name}.conv2", cout)
        if ds:
            x = self._gn(self._conv(x, B, H, W, 1, f"{name}.ds", cout, stride), B, Ho * Wo, f"{name}.norm3", relu=False)
        elif skip is not None or x.shape[1] != cout:
            x = None
        return self._gn(y, B, Ho * Wo, f"{name}.norm2", relu=True, residual=x)

    def _resize(self, x, B, Hi, Wi, Ho, Wo):
        out = torch.empty(B * Ho * Wo, x.shape[1], device=self.device, dtype=torch.float32)
        self.ops.resize_bilinear_pm(x, out, B, Hi, Wi, Ho, Wo)
        return out

    @torch.no_grad()
    def __call__(self, img: torch.Tensor) -> List[torch.Tensor]:
        """``img`` [B, 3, H, W] fp32 -> [enc_out4, up2_out, up1_out(, up0_out)], each [B, C, h, w] with channels-last strides"""
        if not img.is_cuda:
            raise RuntimeError(f"{type(self).__name__} needs GPU tensors (no CPU fallback)")
        if img.dim() != 4 or img.shape[1] != self.input_dim:
            raise ValueError(f"expected [B, {self.input_dim}, H, W], got {tuple(img.shape)}")
        img = img.float().contiguous()
        B, _, H, W = img.shape
        h, w = _out(H, 2), _out(W, 2)
        max_b = self._max_batch(h, w)
        if B > max_b:
            parts = [self(img[i:i + max_b]) for i in range(0, B, max_b)]
            return [torch.cat(level, 0) for level in zip(*parts)]
        x = torch.empty(B * h * w, self.stem_dim, device=self.device, dtype=torch.float32)
        self.ops.conv_stem(img, self.w["stem.w"], self.w["stem.b"], x, False)
        x = self._gn(x, B, h * w, "norm1", relu=True)
        skips = {}       # layer index -> (rows, h, w)
        table = iter(self.blocks)
        for layer in (1, 2, 3, 4):
            for _ in range(2):
                name, _cin, cout, stride, ds = next(table)
                x = self._block(x, B, h, w, name, cout, stride, ds)
                h, w = _out(h, stride), _out(w, stride)
            skips[layer] = (x, h, w)
        x = self._conv(x, B, h, w, 1, "out", self.out_dim, fp32_out=True)
        outs = [(x, h, w)]
        for n, _name, _coarse, _skipc, planes, after, level_out in self.desc["ups"]:
            skip, hs, ws = skips[n + 1]
            x = self._resize(x, B, h, w, hs, ws)
            h, w = hs, ws
            name, _cin, cout, stride, ds = next(table)
            x = self._block(x, B, h, w, name, cout, stride, ds, skip=skip)
            name, _cin, cout, stride, ds = next(table)
            x = self._block(x, B, h, w, name, cout, stride, ds)
            if after is not None:
                x = self._conv(x, B, h, w, 1, after, level_out, fp32_out=True)
            outs.append((x, h, w))
        return [r.view(B, hh, ww, r.shape[1]).permute(0, 3, 1, 2) for r, hh, ww in outs]


class PfkMultiScaleEncoder(WrappedModule):
    """Drop-in for ``model.fnet`` / ``model.cnet`` of a live CCMR / CCMR+ / MS-RAFT+ model: the reference's ``forward(x)`` contract (a
    tensor, or a list of two images that is batched; the feature encoders hand every level back split into the pair), the same
    parameters — the reference sub-modules are re-registered under their own names, so state_dict keys are unchanged.  Eval-mode calls
    outside grad mode and autocast on fp32 GPU tensors with fp32 parameters go to `MultiScaleEncoderEngine` (``engine_calls``); every
    other call runs the reference module (``fallback_calls``)."""

    def __init__(self, ref: torch.nn.Module, desc: dict, split_pairs: bool):
        super().__init__(ref)
        self.desc = desc
        self.split_pairs = split_pairs
        self.engine_calls = 0
        self.fallback_calls = 0

    def _get_engine(self, device) -> MultiScaleEncoderEngine:
        ref = self._ref[0]
        return self._engine_for(device, list(ref.parameters()), lambda: MultiScaleEncoderEngine(ref.state_dict(), self.desc, device))

    def forward(self, x):
        ref = self._ref[0]
        is_list = isinstance(x, (tuple, list))
        probe = x[0] if is_list else x
        ref.training = self.training   # .train() / .eval() reach this wrapper and the shared children, not `ref` itself
        tensors = tuple(x) if is_list else (x,)
        params = list(ref.parameters())
        if (self.training or not all(torch.is_tensor(t) and t.dim() == 4 for t in tensors)
                or not eligible(tensors, params, dtypes=(torch.float32,), autocast=False)
                or any(p.dtype != torch.float32 or p.device != probe.device for p in params)
                or (self.split_pairs and not (is_list and len(x) == 2 and x[0].shape[0] == x[1].shape[0]))):
            self.fallback_calls += 1
            return ref(x)
        self.engine_calls += 1
        batch_dim = probe.shape[0]
        outs = self._get_engine(probe.device)(torch.cat(list(x), dim=0) if is_list else x)
        if self.split_pairs:
            return [torch.split(o, [batch_dim, batch_dim], dim=0) for o in outs]
        return outs
