"""SEA-RAFT's ResNet encoders and `init_conv` on libpfk kernels.

Reference: ptlflow/models/sea_raft/extractor.py:6-116 (``ResNetFPN``: 7x7/2 stem + BatchNorm + relu, three stages of ``BasicBlock``s at
1/2, 1/4, 1/8 resolution — two each for ``resnet18``, 3 / 4 / 6 for ``resnet34`` — and a 1x1 ``final_conv``) and layer.py:126-150
(``BasicBlock``: ``relu(x' + relu(bn2(conv2(relu(bn1(conv1(x)))))))`` with ``x' = bn3(conv1x1(x))`` when the block changes the stride
or the width).  ``fnet`` reads one image; ``cnet`` reads ``cat([image1, image2], 1)`` (sea_raft.py:187).

``ResNetFPNEngine`` is ``EncoderEngine`` (encoder.py: its pack loop, Winograd rule, block and forward) constructed with the block table
read from the state_dict, ResNetFPN's state_dict names, 3 or 6 input channels and this module's ``WINO_MIN_PIXELS``; its own are the
stem launch and the per-layer batch bound.  ``ConvEngine`` (`init_conv`) is that engine's one stride-1 3x3 convolution.  The eval-mode
BatchNorms are folded into the convolutions (`EncoderEngine._fold`), activations stay pixel-major between the kernels:

* stem, 3 or 6 input channels        -> ``pfk_conv_stem2_f32`` / ``_b16`` (reads the two 3-channel halves of the input in place)
* 3x3 / 1x1, stride 1 / 2            -> ``pfk_conv2d_f32`` or ``pfk_conv2d_b16`` (bias, relu, residual add and the block's last relu
                                         in the epilogue)
* fp32, 3x3 stride 1, large launches -> Winograd F(2x2,3x3): ``pfk_conv2d_wino_f32`` (a block's conv1, `init_conv`) and
                                         ``pfk_conv2d_wino_res_f32`` (conv2: + residual, relu), by `WINO_MIN_PIXELS`

``precision="bf16"`` is the K8b path of the other engines: bf16 rows between the layers, fp32 rows out of ``final_conv``.  BatchNorm is
folded in fp32 and the folded weight rounded to bf16 once; autocast rounds the convolution's output to bf16 and then applies the norm,
so one rounding sits elsewhere.

``BasicBlock`` registers the norm of its downsample path twice, as ``bn3`` and as ``downsample.1`` (layer.py:139-142): the state_dict
holds both key sets for one tensor.  `resnet_fpn_shapes` expects both; the engine folds ``bn3`` once.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from ._seam import WrappedModule, eligible, pixel_rows
from .conv_path import PRECISIONS, check_precision
from .encoder import EncoderEngine, _out

STEM_DIM = 64              # the width pfk_conv_stem2 is built for (every shipped `initial_dim`)
# Winograd rule of the fp32 engine: width -> the fewest pixels (B * H * W of the launch) at which `pfk_conv2d_wino_f32` /
# `pfk_conv2d_wino_res_f32` measured faster than `pfk_conv2d_f32` (scripts/wino_res_bench.py, table in DESIGN.md §SEA-RAFT); a width
# that is not listed never takes Winograd
WINO_MIN_PIXELS: Dict[int, int] = {64: 220 * 512, 128: 110 * 256, 256: 55 * 128}     # one 440 x 1024 frame: all it was measured on
# precision -> (input dtypes, cuda autocast) the encoder seams serve (`_seam.eligible`)
ACCEPTS = {"fp32": ((torch.float32,), False), "bf16": ((torch.float32,), torch.bfloat16)}
# state_dict names (`encoder._NAMES`): the stem's norm, a block's (conv, norm) pairs, the norm of its downsample path, the output convolution
_NAMES = ("bn1", (("conv1", "bn1"), ("conv2", "bn2")), "bn3", "final_conv")


def block_table(shapes: Dict[str, tuple]) -> Optional[List[Tuple[str, int, int, int, bool]]]:
    """(name, cin, cout, stride, has_downsample) of every BasicBlock, read from state_dict shapes; None when they are not a ResNetFPN's.
    Stage i has stride 1 (layer1) or 2; a block has a downsample path when ``stride != 1 or cin != cout`` (layer.py:136)."""
    stem = shapes.get("conv1.weight")
    if stem is None or len(stem) != 4:
        return None
    cin = stem[0]
    table = []
    for i, stride in ((1, 1), (2, 2), (3, 2)):
        n = len({k.split(".")[1] for k in shapes if k.startswith(f"layer{i}.")})
        w = shapes.get(f"layer{i}.0.conv1.weight")
        if n < 1 or w is None or len(w) != 4:
            return None
        dim = w[0]
        for j in range(n):
            s = stride if j == 0 else 1
            table.append((f"layer{i}.{j}", cin, dim, s, s != 1 or cin != dim))
            cin = dim
    return table


def resnet_fpn_shapes(input_dim: int, initial_dim: int, table, out_dim: int) -> Dict[str, tuple]:
    """state_dict names / shapes of ResNetFPN with BatchNorm2d for a block table (extractor.py:35-56, layer.py:127-142)."""
    sh: Dict[str, tuple] = {}

    def conv(name, co, ci, k):
        sh[name + ".weight"] = (co, ci, k, k)
        sh[name + ".bias"] = (co,)

    def norm(name, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            sh[f"{name}.{k}"] = (c,)
        sh[name + ".num_batches_tracked"] = ()

    conv("conv1", initial_dim, input_dim, 7)
    norm("bn1", initial_dim)
    for name, cin, cout, _stride, ds in table:
        conv(name + ".conv1", cout, cin, 3)
        conv(name + ".conv2", cout, cout, 3)
        norm(name + ".bn1", cout)
        norm(name + ".bn2", cout)
        if ds:
            norm(name + ".bn3", cout)
            conv(name + ".downsample.0", cout, cin, 1)
            norm(name + ".downsample.1", cout)
    conv("final_conv", out_dim, table[-1][2], 1)
    return sh


def match_resnet_fpn(enc: torch.nn.Module) -> bool:
    """`enc`'s state_dict is exactly a ResNetFPN's with eval-foldable BatchNorm2d layers, 3 or 6 input channels, a 64-wide stem and
    stage widths the convolution kernels take on both precisions (multiples of 64).  The class is checked by the caller."""
    sd = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    table = block_table(sd)
    stem, fin = sd.get("conv1.weight"), sd.get("final_conv.weight")
    if table is None or fin is None or len(fin) != 4:
        return False
    if stem[1] not in (3, 6) or stem[0] != STEM_DIM or any(cout % 64 for _n, _ci, cout, _s, _d in table):
        return False
    if sd != resnet_fpn_shapes(stem[1], stem[0], table, fin[0]):
        return False
    norms = [m for m in enc.modules() if isinstance(m, torch.nn.modules.batchnorm._NormBase)]
    if not norms or any(type(m) is not torch.nn.BatchNorm2d or not m.track_running_stats or m.eps != 1e-5 for m in norms):
        return False
    for name, _ci, _co, _s, ds in table:
        blk = enc.get_submodule(name)
        if ds and blk.downsample[1] is not blk.bn3:      # two registrations of ONE norm (layer.py:139-142)
            return False
    return True


class ResNetFPNEngine(EncoderEngine):
    """Packed weights of one ResNetFPN; `engine(x)` maps ``x`` [B, 3 or 6, H, W] fp32 to [B, out_dim, H/8, W/8] (channels-last)."""

    def __init__(self, params: Dict[str, torch.Tensor], device: torch.device, precision: str = "fp32"):
        self.precision = check_precision(precision, PRECISIONS)
        shapes = {k: tuple(v.shape) for k, v in params.items()}
        table = block_table(shapes)
        if table is None:
            raise ValueError("not a ResNetFPN state_dict")
        stem = shapes["conv1.weight"]
        if stem[0] != STEM_DIM or stem[1] not in (3, 6) or stem[2:] != (7, 7):
            raise ValueError("stem must be Conv2d(3 or 6, 64, 7, stride=2, padding=3)")
        super().__init__(params, "batch", device, precision, blocks=table, names=_NAMES, input_dim=stem[1],
                         wino_min_pixels=WINO_MIN_PIXELS)

    def _max_batch(self, H1: int, W1: int) -> int:
        """images per pass that keep every activation matrix under `max_matrix_bytes` (32-bit byte offsets in the conv kernels)"""
        per_image, h, w = H1 * W1 * self.stem_dim * 4, H1, W1
        for _name, _cin, cout, stride, _ds in self.blocks:
            h, w = _out(h, stride), _out(w, stride)
            per_image = max(per_image, h * w * cout * 4)
        return max(1, self.max_matrix_bytes // per_image)

    def _stem(self, img: torch.Tensor, x: torch.Tensor) -> None:
        # the 6-channel input is read as its two 3-channel halves, in place (batch stride 6 H W)
        self.ops.conv_stem2(img[:, :3], img[:, 3:] if self.input_dim == 6 else None, self.w["stem.w"], self.w["stem.b"], x, True)


class ConvEngine(EncoderEngine):
    """One bias-only 3x3 stride-1 convolution on pixel-major rows (SEA-RAFT's `init_conv`, sea_raft.py:112), packed and launched as the
    encoder's own convolutions are (`_put`, `_conv3`: the encoder's Winograd rule and `winograd` switch)."""

    def __init__(self, params: Dict[str, torch.Tensor], device: torch.device, precision: str = "fp32"):
        self.precision = precision
        super().__init__(params, "none", device, precision, wino_min_pixels=WINO_MIN_PIXELS)

    def pack(self, P: Dict[str, torch.Tensor]) -> None:
        w, b = self._fold(P, "conv", None)
        self.out_dim = w.shape[0]
        self.w = {}
        self._put(self.w, "conv", w, b, wino=True)

    @torch.no_grad()
    def __call__(self, rows: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        if self.path.b16 and rows.dtype != torch.bfloat16:
            rows = rows.to(torch.bfloat16)        # what autocast does to the convolution's input
        y = self._conv3(rows, B, H, W, "conv", self.out_dim, relu=False, fp32_out=True)
        return y.view(B, H, W, self.out_dim).permute(0, 3, 1, 2)


def _accepts(precision: str, x, params, bf16_rows: bool = False) -> bool:
    """the engine of `precision` serves a call on `x` with `params` (fp32, same device); `bf16_rows`: a bf16 `x` is fine on the bf16 path"""
    params = list(params)
    dtypes, autocast = ACCEPTS[precision]
    if bf16_rows and precision == "bf16":
        dtypes = (torch.float32, torch.bfloat16)
    return torch.is_tensor(x) and x.dim() == 4 and eligible((x,), params, dtypes, autocast) and \
        all(p.dtype == torch.float32 and p.device == x.device for p in params)


class PfkResNetEncoder(WrappedModule):
    """Drop-in for SEA-RAFT's ``model.fnet`` / ``model.cnet`` (``ResNetFPN``): same ``forward(x)``, same parameters — the reference
    sub-modules stay registered under their own names.  Eval-mode fp32 GPU inference goes to ``ResNetFPNEngine`` (counted in `calls`);
    training mode, gradient graphs, CPU tensors, half tensors and autocast the precision does not serve stay on the reference module."""

    def __init__(self, ref: torch.nn.Module, precision: str = "fp32"):
        super().__init__(ref)
        self.precision = precision
        self.calls = 0
        self._last_out: Optional[torch.Tensor] = None
        self._last_version = -1

    def set_precision(self, precision: str) -> None:
        if check_precision(precision, PRECISIONS) != self.precision:
            self.precision = precision
            self._engine, self._versions, self._last_out = None, None, None

    def owns(self, x: torch.Tensor) -> bool:
        """`x` is the tensor this encoder handed out last, untouched since"""
        return x is self._last_out and x._version == self._last_version

    def _get_engine(self, device) -> ResNetFPNEngine:
        ref = self._ref[0]
        return self._engine_for(device, [*ref.parameters(), *ref.buffers()],
                                lambda: ResNetFPNEngine(ref.state_dict(), device, self.precision))

    def forward(self, x):
        ref = self._ref[0]
        ref.training = self.training   # .train() / .eval() reach this wrapper and the shared children, not `ref` itself
        if self.training or not _accepts(self.precision, x, ref.parameters()):
            self._last_out = None
            return ref(x)
        y = self._get_engine(x.device)(x)
        if torch.is_autocast_enabled("cuda"):
            y = y.to(torch.bfloat16)   # what the module's last convolution returns inside cuda bf16 autocast
        self.calls += 1
        self._last_out, self._last_version = y, y._version
        return y


class PfkInitConv(WrappedModule):
    """Drop-in for SEA-RAFT's ``model.init_conv`` (3x3, 256 -> 256, no activation, sea_raft.py:112,188): called with the tensor
    ``model.cnet`` (a `PfkResNetEncoder`) just handed out it runs on the kernels from that tensor's pixel-major rows, any other input
    goes to the wrapped ``Conv2d``.  The convolution's own parameters are registered here under their names (`weight`, `bias`)."""

    def __init__(self, ref: torch.nn.Conv2d, encoder: PfkResNetEncoder, precision: str = "fp32"):
        super().__init__(ref)
        self.weight, self.bias = ref.weight, ref.bias
        self._encoder = [encoder]
        self.precision = precision
        self.calls = 0

    def set_precision(self, precision: str) -> None:
        if precision != self.precision:
            self.precision = precision
            self._engine, self._versions = None, None

    def forward(self, x):
        ref, enc = self._ref[0], self._encoder[0]
        ref.training = self.training
        rows = None
        if not self.training and torch.is_tensor(x) and enc.owns(x) and x.shape[1] == ref.in_channels \
                and _accepts(self.precision, x, ref.parameters(), bf16_rows=True):
            rows = pixel_rows(x, x.dtype, align=8, dense=True)
        if rows is None:
            return ref(x)
        B, _, H, W = x.shape
        eng = self._engine_for(x.device, [ref.weight, ref.bias],
                               lambda: ConvEngine({"conv.weight": ref.weight, "conv.bias": ref.bias}, x.device, self.precision))
        y = eng(rows, B, H, W)
        if torch.is_autocast_enabled("cuda"):
            y = y.to(torch.bfloat16)
        self.calls += 1
        return y


def match_init_conv(conv: torch.nn.Module, channels: int) -> bool:
    return type(conv) is torch.nn.Conv2d and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and \
        conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros" and conv.bias is not None and \
        conv.in_channels == channels and conv.out_channels == channels and channels % 64 == 0
