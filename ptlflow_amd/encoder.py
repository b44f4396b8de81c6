"""BasicEncoder / SmallEncoder (the feature / context networks) on libpfk kernels — SURVEY.md §8 f3.

Reference: ptlflow/models/raft/extractor.py:122-194 (``BasicEncoder``: 7x7/2 stem, three pairs of ``ResidualBlock``s at
1/2, 1/4, 1/8 resolution, 1x1 output conv; ``norm_fn`` = ``instance`` for fnet, ``batch`` for cnet; gma/ and the other
RAFT descendants reuse it) and :197-267 (``SmallEncoder`` of raft_small: the same skeleton at widths 32/64/96 with
``BottleneckBlock``s — 1x1 -> 3x3 (stride) -> 1x1, :62-119).  ``EncoderEngine`` is the one engine body of these and of SEA-RAFT's
ResNetFPN (sea_encoder.py) and, subclassed, of the multi-scale GroupNorm encoders (ms_encoder.py): pack loop, Winograd rule, block
and forward are written once; an encoder is its block table, its state_dict names, its stem launch and its module's
``WINO_MIN_PIXELS``.  Activations stay pixel-major ``[B*H*W, C]`` between kernels:

* stem                     -> ``pfk_conv_stem_f32`` (reads the NCHW image)
* 3x3 / 1x1, stride 1 / 2  -> ``pfk_conv2d_f32`` or ``pfk_conv2d_bf16s`` (implicit GEMM; bias, relu, residual add and the
  block's final relu fused in the epilogue)
* fp32, 3x3 stride 1, large launches of BasicEncoder -> Winograd F(2x2,3x3): ``pfk_conv2d_wino_f32`` (in front of an instance
  norm, and a folded-BatchNorm block's conv1) and ``pfk_conv2d_wino_res_f32`` (its conv2: + residual, relu), by ``WINO_MIN_PIXELS``
* InstanceNorm             -> ``pfk_instnorm_stats_f32`` + ``pfk_norm_apply_f32`` (norm + relu + residual + relu)
* InstanceNorm around a Winograd launch of the fp32 engine (``fuse_norms``) -> no pass of its own: the norm in front of the
  convolution is applied to its taps on load and the statistics of the norm behind it are summed in its epilogue
  (``pfk_conv2d_wino_stats_f32``); the block's last apply normalises a raw residual (the stem's output, the downsample path) in
  flight (``pfk_norm_apply_res_f32``).  Same bits as the separate passes
* BatchNorm (eval)         -> folded into the convolution's weights and bias at pack time (no kernel)

The tensor handed back is an NCHW-shaped channels-last view of the last pixel-major buffer, which ``CorrBlock`` and
``UpdateEngine.load_state`` consume without a transpose.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import load_native
from ._seam import WrappedModule, eligible
from .conv_path import resolve
from .packing import pack_wino_weight

# (name, cin, cout, stride, has_downsample) of the six residual blocks, extractor.py:150-153
_BLOCKS = (("layer1.0", 64, 64, 1, False), ("layer1.1", 64, 64, 1, False), ("layer2.0", 64, 96, 2, True), ("layer2.1", 96, 96, 1, False),
           ("layer3.0", 96, 128, 2, True), ("layer3.1", 128, 128, 1, False))
# the six bottleneck blocks of SmallEncoder, extractor.py:216-219
_SMALL_BLOCKS = (("layer1.0", 32, 32, 1, False), ("layer1.1", 32, 32, 1, False), ("layer2.0", 32, 64, 2, True), ("layer2.1", 64, 64, 1, False),
                 ("layer3.0", 64, 96, 2, True), ("layer3.1", 96, 96, 1, False))
# state_dict names: (the stem's norm, a block's (conv, norm) pairs, the norm of its downsample path, the output convolution)
_NAMES = ("norm1", (("conv1", "norm1"), ("conv2", "norm2")), "downsample.1", "conv2")
_SMALL_NAMES = ("norm1", (("conv1", "norm1"), ("conv2", "norm2"), ("conv3", "norm3")), "downsample.1", "conv2")
EPS = 1e-5
# Winograd rule of the fp32 BasicEncoder engine: width -> the fewest pixels (B * H * W of the launch) at which `pfk_conv2d_wino_f32` /
# `pfk_conv2d_wino_res_f32` measured faster than `pfk_conv2d_f32` in both forms (scripts/wino_res_bench.py --encoder raft, table in
# DESIGN.md §3 K9–K11, profiles/r08_a_winograd_lds_dma.md; re-measured with the row-walk epilogue, profiles/r14_a_wino_epilogue.md §2:
# every entry wins by more — 64 at one image 1.76x / 1.73x, 96 1.98x / 1.99x, 128 at two 1.62x / 1.58x — and 128 at one image, 1.06x,
# stays below the line); a width or a size that was not measured keeps the direct kernel
WINO_MIN_PIXELS: Dict[int, int] = {64: 218 * 512, 96: 109 * 256, 128: 2 * 55 * 128}     # 436 x 1024 frames: all it was measured on
# `fuse_norms`, a Winograd conv1 behind an already normalised input (nothing to fold on load): width -> the fewest pixels at which
# the statistics out of its epilogue measured faster than the statistics pass behind the plain launch (scripts/enc_norm_fusion_bench.py,
# profiles/r16_a_encoder_norms.md §2).  The epilogue leaves one partial row per 32 tiles, and at width 64 the fixed-order reduction
# over an image's 880 rows outweighs the pass at two images (+5.6 us) and not at sixteen (-22.5 us); 96 and 128 win at both.  With
# a norm to fold on load the fused launch won at every width and size measured.
STATS_ONLY_MIN_PIXELS: Dict[int, int] = {64: 16 * 218 * 512}


def _out(n: int, s: int) -> int:
    return (n - 1) // s + 1


class EncoderEngine:
    """Packed weights of one encoder; `engine(img)` maps ``img`` [B, input_dim, H, W] fp32 to [B, out_dim, H/8, W/8] (channels-last).
    What differs between BasicEncoder, SmallEncoder and SEA-RAFT's ResNetFPN (sea_encoder.py) is data: the block table, the state_dict
    names, the stem's input channels and the Winograd threshold table — the module's own dict object, read at call time."""

    NORMS = ("instance", "batch", "none")      # the `norm_fn`s this engine body implements (ms_encoder.py: "group")
    widest_row = 128      # floats of the widest activation row at half resolution (32 for the small encoder; same bound)

    def __init__(self, params: Dict[str, torch.Tensor], norm: str, device: torch.device, conv_precision: str = "fp32",
                 small: bool = False, *, blocks=None, names=None, input_dim: int = 3, wino_min_pixels: Optional[Dict[int, int]] = None):
        load_native()
        self.small = small
        self.blocks = blocks if blocks is not None else (_SMALL_BLOCKS if small else _BLOCKS)
        self.names = names if names is not None else (_SMALL_NAMES if small else _NAMES)
        self.input_dim = input_dim
        self.wino_min_pixels = WINO_MIN_PIXELS if wino_min_pixels is None else wino_min_pixels
        if norm not in self.NORMS:
            raise ValueError(norm)
        # "bf16": K8b (`pfk_conv2d_b16`, UpdateEngine's docstring) — bf16 activation storage between the layers, instance norms
        # included (statistics and normalisation in fp32 arithmetic on the bf16 rows, as F.instance_norm under autocast)
        self.path = resolve(conv_precision)
        self.ops = torch.ops.pfk
        self.norm = norm
        self.device = device
        self._ws: Optional[torch.Tensor] = None
        self.winograd = True       # False: the direct kernel everywhere (A/B timing, tests); "always": Winograd wherever its weight exists
        self.fuse_norms = True     # False: every instance norm as its own statistics and apply launches (A/B timing, tests)
        self.max_matrix_bytes = 2 ** 31 - 1   # 32-bit byte offsets in the convolution kernels
        self.pack(params)

    # ------------------------------------------------------------------ weights
    def _fold(self, P, conv: str, norm_name: Optional[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """conv weight / bias with eval-mode BatchNorm folded in (extractor.py:138-139: y = (x - mean)/sqrt(var+eps)*g + b)."""
        dev = self.device
        w = P[conv + ".weight"].detach().to(device=dev, dtype=torch.float32)
        b = P[conv + ".bias"].detach().to(device=dev, dtype=torch.float32)
        if self.norm == "batch" and norm_name is not None:
            g, beta, mean, var = (P[f"{norm_name}.{k}"].detach().to(device=dev, dtype=torch.float32)
                                  for k in ("weight", "bias", "running_mean", "running_var"))
            scale = g / torch.sqrt(var + EPS)
            w = w * scale[:, None, None, None]
            b = (b - mean) * scale + beta
        return w, b.contiguous()

    def _put(self, W, key: str, w: torch.Tensor, b: torch.Tensor, wino: bool = False) -> None:
        """the (folded) convolution under `key`: the direct kernel's operand and the bias; `wino` (a stride-1 3x3 convolution): on the
        fp32 engine of a non-small encoder, square and of a width in the threshold table, also the transformed weight of the Winograd
        kernels `_use_wino` may select"""
        cin = w.shape[1]
        W[key + ".w"], W[key + ".b"] = self.path.pack(w, self._segments(key, cin)), b
        if wino and self.path.fp32_tiles and not self.small and cin == w.shape[0] and cin in self.wino_min_pixels:
            W[key + ".ww"] = pack_wino_weight(w.cpu()).to(self.device)

    def _segments(self, key: str, cin: int):
        """the sources of the convolution under `key`, as `packing.pack_conv_weight` takes them: one buffer of `cin` channels"""
        return [(0, cin, cin)]

    def pack(self, P: Dict[str, torch.Tensor]) -> None:
        W: Dict[str, torch.Tensor] = {}
        stem_norm, convs, ds_norm, out_conv = self.names
        w, b = self._fold(P, "conv1", stem_norm)
        assert w.shape[1:] == (self.input_dim, 7, 7), "stem must be Conv2d(input_dim, C, 7, stride=2, padding=3)"
        W["stem.w"] = w.permute(2, 3, 1, 0).reshape(49, self.input_dim, w.shape[0]).contiguous()
        W["stem.b"] = b
        for name, _cin, _cout, stride, ds in self.blocks:
            for conv, nrm in convs:
                self._put(W, f"{name}.{conv}", *self._fold(P, f"{name}.{conv}", f"{name}.{nrm}"), wino=conv == "conv2" or stride == 1)
            if ds:
                self._put(W, f"{name}.ds", *self._fold(P, f"{name}.downsample.0", f"{name}.{ds_norm}"))
        w, b = self._fold(P, out_conv, None)
        self._put(W, "out", w, b)
        self.out_dim = w.shape[0]
        self.stem_dim = W["stem.b"].numel()
        self.w = W

    # ------------------------------------------------------------------ kernels
    def _conv(self, x, B, H, W, k, key, cout, stride=1, relu=False, residual=None, relu2=False, fp32_out=None):
        M = B * _out(H, stride) * _out(W, stride)
        # bf16 rows out on K8b, also in front of an instance norm: under the reference's autocast switch a convolution returns a
        # 16-bit tensor and F.instance_norm (fp32 arithmetic) reads that — statistics and normalisation of the rounded values
        # (half the bytes of the three passes over the largest activations of the forward); fp32 only for the network's output
        out = torch.empty(M, cout, device=self.device, dtype=torch.float32 if fp32_out else self.path.dtype)
        self.path.conv(self.ops, srcs=[x], B=B, H=H, W=W, kh=k, kw=k, weight=self.w[key + ".w"], bias=self.w[key + ".b"], cout=cout,
                       out=out, relu=relu, residual=residual, stride=stride, relu2=relu2)
        return out

    def _use_wino(self, key: str, cout: int, pixels: int) -> bool:
        """Winograd F(2x2,3x3) for this stride-1 3x3 convolution: its transformed weight exists (`_put`) and the launch is at least as
        large as the smallest one measured faster than `pfk_conv2d_f32` at this width.  Launch shape only: B * H * W of the launch.
        A chunked forward (`max_matrix_bytes`) therefore has the whole-batch forward's bits only where every chunk falls on the same
        side of the threshold as the whole batch (one image at 55 x 128 and width 128 is below it, two are not)."""
        if not self.winograd or (key + ".ww") not in self.w:
            return False
        return self.winograd == "always" or pixels >= self.wino_min_pixels[cout]

    def _conv3(self, x, B, H, W, key, cout, relu=False, residual=None, fp32_out=None):
        """a stride-1 3x3 convolution: plain (in front of an instance norm, `init_conv`), + relu (conv1), or + relu, + residual, relu
        (conv2)"""
        if not self._use_wino(key, cout, B * H * W):
            return self._conv(x, B, H, W, 3, key, cout, relu=relu, residual=residual, relu2=residual is not None, fp32_out=fp32_out)
        out = torch.empty(B * H * W, cout, device=self.device, dtype=torch.float32)
        if residual is None:
            self.ops.conv2d_wino(x, B, H, W, self.w[key + ".ww"], self.w[key + ".b"], cout, relu, 1.0, out, 0)
        else:
            self.ops.conv2d_wino_res(x, B, H, W, self.w[key + ".ww"], self.w[key + ".b"], cout, relu, 1.0, out, residual, True)
        return out

    def _workspace(self, need: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=self.device, dtype=torch.uint8)
        return self._ws

    def _stats(self, x, B, HW):
        """(mean, rstd) [B*C] of the instance norm over the fp32 pixel-major buffer x, by the statistics pass"""
        C = x.shape[1]
        mean = torch.empty(B * C, device=self.device, dtype=torch.float32)
        rstd = torch.empty(B * C, device=self.device, dtype=torch.float32)
        self.ops.instnorm_stats(x, B, HW, EPS, mean, rstd, self._workspace(self.ops.instnorm_workspace_bytes(B, C)))
        return mean, rstd

    def _wino_stats(self, x, xst, B, H, W, key, cout):
        """a Winograd convolution in front of an instance norm -> (raw output, its (mean, rstd)), the statistics out of the epilogue;
        `xst` = (mean, rstd, relu): x is the raw output of the convolution before, normalised on load"""
        out = torch.empty(B * H * W, cout, device=self.device, dtype=torch.float32)
        mean = torch.empty(B * cout, device=self.device, dtype=torch.float32)
        rstd = torch.empty(B * cout, device=self.device, dtype=torch.float32)
        im, ir, irelu = xst if xst is not None else (None, None, False)
        self.ops.conv2d_wino_stats(x, B, H, W, self.w[key + ".ww"], self.w[key + ".b"], cout, out, im, ir, irelu, EPS, mean, rstd,
                                   self._workspace(self.ops.conv_wino_stats_workspace_bytes(B, H, W, cout)))
        return out, (mean, rstd)

    def _block_fused(self, x, xst, B, H, W, name, cout, stride, ds):
        """`_block` of the fp32 instance-norm engine with the norm passes folded into the Winograd launches around them.  A raw
        buffer travels with its statistics: `xst` = (mean, rstd, relu) where x is the raw stem output (layer1.0), else None.  A
        convolution on the direct kernel keeps its separate passes, and every step rounds as they do: `_block`'s bits."""
        Ho, Wo = _out(H, stride), _out(W, stride)
        k1, k2 = f"{name}.conv1", f"{name}.conv2"
        if stride == 1 and self._use_wino(k1, cout, B * H * W) and (xst is not None or B * H * W >= STATS_ONLY_MIN_PIXELS.get(cout, 0)):
            y, yst = self._wino_stats(x, xst, B, H, W, k1, cout)
        else:
            assert xst is None
            y = self._conv3(x, B, H, W, k1, cout) if stride == 1 else self._conv(x, B, H, W, 3, k1, cout, stride)
            yst = self._stats(y, B, Ho * Wo)
        if self._use_wino(k2, cout, B * Ho * Wo):
            z, zst = self._wino_stats(y, (*yst, True), B, Ho, Wo, k2, cout)
        else:
            self.ops.norm_apply(y, *yst, None, y, B, Ho * Wo, True, False)
            z = self._conv3(y, B, Ho, Wo, k2, cout)
            zst = self._stats(z, B, Ho * Wo)
        if ds:
            x = self._conv(x, B, H, W, 1, f"{name}.ds", cout, stride)
            xst = (*self._stats(x, B, Ho * Wo), False)
        if xst is None:
            self.ops.norm_apply(z, *zst, x, z, B, Ho * Wo, True, True)
        else:
            self.ops.norm_apply_res(z, *zst, x, *xst, z, B, Ho * Wo, True, True)
        return z

    def _inorm(self, x, B, HW, relu, residual=None, relu2=False):
        """InstanceNorm2d (+relu, + residual add + relu) in place on the pixel-major buffer x — fp32 rows, or the bf16 rows of the K8b
        path (only the stem, a VALU / fp32-MFMA kernel, hands over fp32 rows there: those are normalised into a fresh bf16 buffer)."""
        C = x.shape[1]
        mean = torch.empty(B * C, device=self.device, dtype=torch.float32)
        rstd = torch.empty(B * C, device=self.device, dtype=torch.float32)
        self.ops.instnorm_stats(x, B, HW, EPS, mean, rstd, self._workspace(self.ops.instnorm_workspace_bytes(B, C)))
        out = torch.empty(x.shape[0], C, device=self.device, dtype=torch.bfloat16) if (self.path.b16 and x.dtype != torch.bfloat16) else x
        self.ops.norm_apply(x, mean, rstd, residual, out, B, HW, relu, relu2)      # (bf16 rows: in place, like the fp32 path)
        return out

    def _bottleneck(self, x, B, H, W, name, cout, stride, ds):
        """BottleneckBlock.forward (extractor.py:110-119): relu(norm(1x1)) -> relu(norm(3x3, stride)) -> relu(norm(1x1)); relu(x + y)."""
        Ho, Wo = _out(H, stride), _out(W, stride)
        mid = cout // 4
        if self.norm == "instance":
            y = self._inorm(self._conv(x, B, H, W, 1, f"{name}.conv1", mid), B, H * W, relu=True)
            y = self._inorm(self._conv(y, B, H, W, 3, f"{name}.conv2", mid, stride), B, Ho * Wo, relu=True)
            y = self._conv(y, B, Ho, Wo, 1, f"{name}.conv3", cout)
            if ds:
                x = self._inorm(self._conv(x, B, H, W, 1, f"{name}.ds", cout, stride), B, Ho * Wo, relu=False)
            return self._inorm(y, B, Ho * Wo, relu=True, residual=x, relu2=True)
        y = self._conv(x, B, H, W, 1, f"{name}.conv1", mid, relu=True)
        y = self._conv(y, B, H, W, 3, f"{name}.conv2", mid, stride, relu=True)
        if ds:
            x = self._conv(x, B, H, W, 1, f"{name}.ds", cout, stride)
        return self._conv(y, B, Ho, Wo, 1, f"{name}.conv3", cout, relu=True, residual=x, relu2=True)

    def _block(self, x, B, H, W, name, cout, stride, ds):
        """ResidualBlock.forward (extractor.py:52-59) / SEA-RAFT's BasicBlock.forward (sea_raft/layer.py:144-150): relu(x' + relu(norm2(
        conv2(relu(norm1(conv1(x))))))) with x' the downsample path where the table has one"""
        if self.small:
            return self._bottleneck(x, B, H, W, name, cout, stride, ds)
        Ho, Wo = _out(H, stride), _out(W, stride)
        act = self.norm != "instance"   # "batch" (folded) and "none": relu straight in the epilogue
        if stride == 1:
            y = self._conv3(x, B, H, W, f"{name}.conv1", cout, relu=act)
        else:
            y = self._conv(x, B, H, W, 3, f"{name}.conv1", cout, stride, relu=act)
        if act:
            if ds:
                x = self._conv(x, B, H, W, 1, f"{name}.ds", cout, stride)
            return self._conv3(y, B, Ho, Wo, f"{name}.conv2", cout, relu=True, residual=x)
        y = self._inorm(y, B, Ho * Wo, relu=True)
        y = self._conv3(y, B, Ho, Wo, f"{name}.conv2", cout)
        if ds:
            x = self._inorm(self._conv(x, B, H, W, 1, f"{name}.ds", cout, stride), B, Ho * Wo, relu=False)
        return self._inorm(y, B, Ho * Wo, relu=True, residual=x, relu2=True)

    def _max_batch(self, H1: int, W1: int) -> int:
        """images per pass that keep every activation matrix under `max_matrix_bytes` (32-bit byte offsets in the conv kernels); the
        widest activation row: `widest_row` floats at half resolution"""
        return max(1, self.max_matrix_bytes // (H1 * W1 * self.widest_row * 4))

    def _stem(self, img: torch.Tensor, x: torch.Tensor) -> None:
        self.ops.conv_stem(img, self.w["stem.w"], self.w["stem.b"], x, self.norm != "instance")

    @torch.no_grad()
    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        """``img`` [B, input_dim, H, W] fp32 (already normalised / padded) -> [B, out_dim, H/8, W/8] (channels-last strides)."""
        if not img.is_cuda:
            raise RuntimeError(f"{type(self).__name__} needs GPU tensors (no CPU fallback)")
        if img.dim() != 4 or img.shape[1] != self.input_dim:
            raise ValueError(f"expected [B, {self.input_dim}, H, W], got {tuple(img.shape)}")
        img = img.float().contiguous()
        B, _, H, W = img.shape
        H1, W1 = _out(H, 2), _out(W, 2)
        max_b = self._max_batch(H1, W1)
        if B > max_b:
            return torch.cat([self(img[i:i + max_b]) for i in range(0, B, max_b)], 0)
        # K8b: the MFMA stem kernels round to bf16 themselves (widths 32 / 64), also in front of an instance norm (`_conv`'s note)
        stem_b16 = self.path.b16 and self.stem_dim in (32, 64)
        x = torch.empty(B * H1 * W1, self.stem_dim, device=self.device, dtype=torch.bfloat16 if stem_b16 else torch.float32)
        self._stem(img, x)
        # the norm passes folded into the Winograd launches: the fp32 BasicEncoder / ResNet engines with instance norm
        fused = self.fuse_norms and self.norm == "instance" and self.path.fp32_tiles and not self.small
        xst = None
        name0, _, cout0, stride0, _ = self.blocks[0]
        if fused and stride0 == 1 and self._use_wino(f"{name0}.conv1", cout0, B * H1 * W1):
            xst = (*self._stats(x, B, H1 * W1), True)      # the stem's output stays raw: the first block normalises it on load
        elif self.norm == "instance":
            x = self._inorm(x, B, H1 * W1, relu=True)
        elif self.path.b16 and not stem_b16:
            x = x.to(torch.bfloat16)
        h, w = H1, W1
        for name, _cin, cout, stride, ds in self.blocks:
            if fused:
                x, xst = self._block_fused(x, xst, B, h, w, name, cout, stride, ds), None
            else:
                x = self._block(x, B, h, w, name, cout, stride, ds)
            h, w = _out(h, stride), _out(w, stride)
        y = self._conv(x, B, h, w, 1, "out", self.out_dim, fp32_out=True)
        return y.view(B, h, w, self.out_dim).permute(0, 3, 1, 2)


class PfkEncoder(WrappedModule):
    """Drop-in for ``model.fnet`` / ``model.cnet`` of a live ptlflow model (``BasicEncoder``, raft/extractor.py:122-194):
    same ``forward(x)`` contract (a tensor, or a list of two images that is batched and split again, :172-193), same
    parameters — the reference sub-modules are re-registered under their own names, so state_dict keys, checkpoints and
    optimizers are untouched.  GPU inference goes to ``EncoderEngine``; training mode, gradient graphs, CPU tensors and
    GroupNorm stay on the reference's own code."""

    def __init__(self, ref: torch.nn.Module, conv_precision: str = "fp32", small: bool = False):
        super().__init__(ref)
        self.small = small
        self.norm_fn = ref.norm_fn
        self.conv_precision = conv_precision

    def _get_engine(self, device) -> EncoderEngine:
        ref = self._ref[0]
        return self._engine_for(device, [*ref.parameters(), *ref.buffers()],
                                lambda: EncoderEngine(ref.state_dict(), self.norm_fn, device, self.conv_precision, self.small))

    def forward(self, x):
        ref = self._ref[0]
        is_list = isinstance(x, (tuple, list))
        probe = x[0] if is_list else x
        ref.training = self.training   # .train() / .eval() reach this wrapper and the shared children, not `ref` itself
        if self.training or not eligible((probe,), ref.parameters()) or self.norm_fn not in ("instance", "batch", "none"):
            return ref(x)
        if is_list:
            batch_dim = x[0].shape[0]
            x = torch.cat(list(x), dim=0)
        y = self._get_engine(x.device)(x)
        if probe.dtype != torch.float32 and probe.is_floating_point():
            y = y.to(probe.dtype)      # a half / bf16 model (`model.half()`, validate.py:243-244) gets its features in its own dtype
        if is_list:
            y = torch.split(y, [batch_dim, batch_dim], dim=0)
        return y
