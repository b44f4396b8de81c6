"""Training path of SEA-RAFT's refinement on libpfk kernels (K12d), fp32, in train.py's idiom: pixel-major rows
``[M = B*H*W, C]``, every dense convolution a ``conv_pm`` (forward, data and weight gradient on the implicit-GEMM kernels), and the
two things of the ConvNeXt block (ptlflow/models/sea_raft/layer.py:41-83) that are no dense convolution as autograd nodes of
their own:

* ``dwconv_layernorm_pm``   depthwise k x k + LayerNorm: forward ``pfk_dwconv_layernorm_train_f32`` (the inference kernel's bits, plus
  the normalised value x^ and rstd), backward ``pfk_layernorm_bwd_f32`` then ``pfk_dwconv_bwd_f32``
* ``gelu_pm``               the exact GELU on rows with its pre-activation saved: ``pfk_gelu_f32`` / ``pfk_gelu_bwd_f32``

``convnext_block_train_pm`` chains them: dwconv+LN -> pwconv1 (a 1x1 ``conv_pm``) -> GELU -> pwconv2 with the layer scale folded into
its weight (``gamma[:, None] * W2``, ``gamma * b2``: formed in torch on the parameters, so autograd delivers dW2, db2 and dgamma from
the one weight gradient; the rounding the inference path documents) -> ``+ x`` -> ``final``.
``sea_update_block_train_pm`` is sea_raft/update.py:49-54 (RAFT's motion encoder, then the blocks), ``sea_heads_train_pm`` the heads of
sea_raft.py:106-117, ``upsample_data_train`` the convex upsampling of flow and info (sea_raft.py:147-163: the inference kernel forward,
``pfk_convex_upsample_info_bwd_pm_f32`` backward; K12e).  Saved per block and iteration: x^ [M, 384] and rstd [M] here, the LayerNorm output, the GELU's input and output
[M, 512] and the residual sum [M, 384] as the operands of the convolutions that read them (the block input is the concatenation the
caller holds anyway).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import load_native
from ._seam import pixel_rows
from .train import _KERNELS, _nchw, _pm, conv_pm, packs_for

LN_EPS = 1e-6              # sea_raft/layer.py:57


def _rows(t: torch.Tensor) -> torch.Tensor:
    """fp32 rows the row kernels read: unit channel stride, 16-byte aligned rows"""
    t = t.float()
    if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


class _DwconvLayerNorm(torch.autograd.Function):
    """out [M, C] = LayerNorm_C(dwconv_kxk(x) + b) * ln_weight + ln_bias on pixel-major rows (C % 4 == 0, C <= 512, k odd <= 7)."""

    @staticmethod
    def forward(ctx, x, dw_weight, dw_bias, ln_weight, ln_bias, B: int, H: int, W: int, eps: float):
        ops = torch.ops.pfk
        x = _rows(x)
        M, C = x.shape
        k = dw_weight.shape[-1]
        w = dw_weight.detach().float().reshape(C, k * k).contiguous()
        lw = ln_weight.detach().float().contiguous()
        out, xhat = torch.empty(M, C, device=x.device), torch.empty(M, C, device=x.device)
        rstd = torch.empty(M, device=x.device)
        ops.dwconv_layernorm_train(x, w, None if dw_bias is None else dw_bias.detach().float().contiguous(), lw,
                                   ln_bias.detach().float().contiguous(), eps, out, xhat, rstd, B, H, W, k)
        ctx.geom = (B, H, W, k)
        ctx.has_bias = dw_bias is not None
        ctx.wshape = tuple(dw_weight.shape)
        ctx.save_for_backward(x, xhat, rstd, w, lw)
        return out

    @staticmethod
    def backward(ctx, dy):
        ops = torch.ops.pfk
        x, xhat, rstd, w, lw = ctx.saved_tensors
        B, H, W, k = ctx.geom
        M, C = x.shape
        dev = x.device
        dy = _rows(dy)
        du = torch.empty(M, C, device=dev)
        dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ops.layernorm_bwd(xhat, rstd, lw, dy, du, dgamma, dbeta)
        dx = torch.empty(M, C, device=dev)
        dw = torch.empty(C, k * k, device=dev)
        db = torch.empty(C, device=dev) if ctx.has_bias else None
        ops.dwconv_bwd(x, du, w, dx, dw, db, B, H, W, k)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dw.view(ctx.wshape) if need[1] else None, db if ctx.has_bias and need[2] else None,
                dgamma if need[3] else None, dbeta if need[4] else None, None, None, None, None)


def dwconv_layernorm_pm(x: torch.Tensor, dw_weight: torch.Tensor, dw_bias: Optional[torch.Tensor], ln_weight: torch.Tensor,
                        ln_bias: torch.Tensor, B: int, H: int, W: int, eps: float = LN_EPS) -> torch.Tensor:
    """ConvNextBlock.dwconv + .norm, differentiable: ``x`` [B*H*W, C] fp32 rows, ``dw_weight`` [C, 1, k, k] (PyTorch's layout; its
    gradient comes back in it), ``dw_bias`` [C] or None, LayerNorm ``ln_weight`` / ``ln_bias`` [C]."""
    load_native()
    if x.dim() != 2 or x.shape[0] != B * H * W:
        raise ValueError(f"dwconv_layernorm_pm: x must be [B*H*W, C] rows, got {tuple(x.shape)} for {(B, H, W)}")
    C, k = x.shape[1], dw_weight.shape[-1]
    if C % 4 or not 4 <= C <= 512 or k % 2 == 0 or k > 7 or dw_weight.numel() != C * k * k:
        raise ValueError(f"dwconv_layernorm_pm covers C % 4 == 0, 4 <= C <= 512 and odd k <= 7, got C = {C}, weight {tuple(dw_weight.shape)}")
    return _DwconvLayerNorm.apply(x, dw_weight, dw_bias, ln_weight, ln_bias, B, H, W, float(eps))


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _rows(x)
        y = torch.empty(x.shape, device=x.device)
        torch.ops.pfk.gelu(x, y)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty(x.shape, device=x.device)
        torch.ops.pfk.gelu_bwd(x, _rows(dy), dx)
        return dx


def gelu_pm(x: torch.Tensor) -> torch.Tensor:
    """nn.GELU() on fp32 rows [M, C] (C % 4 == 0), differentiable; saves its input."""
    load_native()
    if x.dim() != 2 or x.shape[1] % 4:
        raise ValueError(f"gelu_pm: rows [M, C] with C % 4 == 0, got {tuple(x.shape)}")
    return _Gelu.apply(x)


def convnext_block_train_pm(P: Dict[str, torch.Tensor], prefix: str, x: torch.Tensor, B: int, H: int, W: int,
                            cache: Optional[dict] = None, accumulate_wgrad: bool = False) -> torch.Tensor:
    """ConvNextBlock.forward (layer.py:69-83) on rows: ``x`` [M, dim] -> [M, out_dim].  ``P[prefix + ...]``: the block's parameters
    (``prefix`` e.g. "refine.0."; without a ``gamma`` the layer scale is 1).  ``cache`` / ``accumulate_wgrad``: as in
    `train.update_block_train_pm` — with a step-scoped cache the folded pwconv2 weight is formed once per step and the recurrent
    calls add their weight gradients into one buffer per convolution."""
    acc = accumulate_wgrad and cache is not None
    p = prefix
    y = dwconv_layernorm_pm(x, P[p + "dwconv.weight"], P.get(p + "dwconv.bias"), P[p + "norm.weight"], P[p + "norm.bias"], B, H, W)
    w1 = P[p + "pwconv1.weight"]
    y = conv_pm([y], w1[:, :, None, None], P.get(p + "pwconv1.bias"), B, H, W, False, None, packs_for(cache, p + "pwconv1", [w1], acc))
    y = gelu_pm(y)
    w2, b2, gamma = P[p + "pwconv2.weight"], P.get(p + "pwconv2.bias"), P.get(p + "gamma")
    packs = packs_for(cache, p + "pwconv2", [t for t in (w2, b2, gamma) if t is not None], acc)
    folded = packs.extra.get("folded") if acc else None      # (only a step-scoped entry may keep tensors with a graph)
    if folded is None:
        if gamma is None:
            folded = (w2[:, :, None, None], b2)
        else:
            folded = ((gamma[:, None] * w2)[:, :, None, None], None if b2 is None else gamma * b2)
        if acc:
            packs.extra["folded"] = folded
    y = conv_pm([y], folded[0], folded[1], B, H, W, False, None, packs)
    wf = P[p + "final.weight"]
    return conv_pm([x + y], wf, P.get(p + "final.bias"), B, H, W, False, None, packs_for(cache, p + "final", [wf], acc))


def sea_update_block_train_pm(P: Dict[str, torch.Tensor], spec, h, i, c, f, B: int, H: int, W: int, num_blocks: int,
                              cache: Optional[dict] = None, accumulate_wgrad: bool = False) -> torch.Tensor:
    """sea_raft/update.py:49-54 on rows: ``h`` [M, 128], ``i`` [M, 128], ``c`` [M, corr channels], ``f`` [M, 2] -> ``h'`` [M, 128].
    The motion encoder as `train.update_block_train_pm` builds it (fp32); ``x = cat([h, i, motion, f])`` has 384 channels and each
    block's output replaces ``h``."""
    acc = accumulate_wgrad and cache is not None
    k = _KERNELS["fp32"]

    def conv(srcs, name, real=None):
        w = P[name + ".weight"]
        return conv_pm(srcs, w, P.get(name + ".bias"), B, H, W, True, real, packs_for(cache, name, [w], acc))

    cor = conv([k.pad(c)], "encoder.convc1", [c.shape[1]])
    if spec.c2:
        cor = conv([cor], "encoder.convc2")
    flo = conv([conv([k.pad(f)], "encoder.convf1", [2])], "encoder.convf2")
    motion = conv([cor, flo], "encoder.conv")
    rest = torch.cat([i.float(), motion, f.float()], 1)
    for b in range(num_blocks):
        h = convnext_block_train_pm(P, f"refine.{b}.", torch.cat([h.float(), rest], 1), B, H, W, cache, accumulate_wgrad)
    return h


def sea_head_train_pm(P: Dict[str, torch.Tensor], name: str, h: torch.Tensor, B: int, H: int, W: int,
                      cache: Optional[dict] = None, accumulate_wgrad: bool = False) -> torch.Tensor:
    """One head (``name`` = "flow_head" | "upsample_weight", sea_raft.py:106-117): 3x3 + relu, then the head's second convolution."""
    acc = accumulate_wgrad and cache is not None
    w0, w2 = P[name + ".0.weight"], P[name + ".2.weight"]
    y = conv_pm([h], w0, P.get(name + ".0.bias"), B, H, W, True, None, packs_for(cache, name + ".0", [w0], acc))
    return conv_pm([y], w2, P.get(name + ".2.bias"), B, H, W, False, None, packs_for(cache, name + ".2", [w2], acc))


def sea_heads_train_pm(P: Dict[str, torch.Tensor], h: torch.Tensor, B: int, H: int, W: int, cache: Optional[dict] = None,
                       accumulate_wgrad: bool = False):
    """``(flow_head(h) [M, 6], upsample_weight(h) [M, 576])`` — delta flow (2) | info (4), and the mask logits before the loop's 0.25."""
    return (sea_head_train_pm(P, "flow_head", h, B, H, W, cache, accumulate_wgrad),
            sea_head_train_pm(P, "upsample_weight", h, B, H, W, cache, accumulate_wgrad))


# ---- NCHW faces: what the seams call from the model's own loop (`PfkSeaRaftUpdateBlock`, `_SeaHeadSeam`) ----------------------------
def sea_update_block_train(P: Dict[str, torch.Tensor], spec, net, inp, corr, flow, num_blocks: int, cache: Optional[dict] = None):
    B, _, H, W = net.shape
    h = sea_update_block_train_pm(P, spec, _pm(net), _pm(inp), _pm(corr), _pm(flow), B, H, W, num_blocks, cache)
    return _nchw(h, B, H, W)


def sea_head_train(P: Dict[str, torch.Tensor], name: str, net, cache: Optional[dict] = None):
    B, _, H, W = net.shape
    return _nchw(sea_head_train_pm(P, name, _pm(net), B, H, W, cache), B, H, W)


# ---- convex upsampling of flow + info (sea_raft.py:147-163) ----------------------------------------------------------------------------
def _upsample_rows(t: torch.Tensor, align: int = 1) -> torch.Tensor:
    """the pixel-major rows of an NCHW fp32 tensor: a view where the strides allow (`pixel_rows`), else one contiguous copy"""
    r = pixel_rows(t, torch.float32, align)
    return r if r is not None else t.permute(0, 2, 3, 1).contiguous().view(-1, t.shape[1])


class _UpsampleData(torch.autograd.Function):
    """flow [B, 2, H, W], info [B, n, H, W] (n <= 8), mask [B, 576, H, W] (already x 0.25), fp32 -> (flow_up [B, 2, 8H, 8W], info_up
    [B, n, 8H, 8W]): `pfk_convex_upsample_info_pm_f32` forward (the inference seam's bits), `pfk_convex_upsample_info_bwd_pm_f32`
    backward.  The flow and info gradients are the columns 0..1 and 2.. of ONE [M, 2 + n] buffer, handed back as NCHW views of it
    (what `flow_head`'s backward reads as its channels-last output gradient)."""

    @staticmethod
    def forward(ctx, flow, info, mask):
        B, _, H, W = flow.shape
        n = info.shape[1]
        f, i, m = _upsample_rows(flow), _upsample_rows(info), _upsample_rows(mask, 4)
        flow_up = torch.empty(B, 2, 8 * H, 8 * W, device=flow.device, dtype=torch.float32)
        info_up = torch.empty(B, n, 8 * H, 8 * W, device=flow.device, dtype=torch.float32)
        torch.ops.pfk.convex_upsample_info_pm(f, i, m, flow_up, info_up)
        ctx.save_for_backward(f, i, m)
        ctx.geom = (B, H, W, n)
        ctx.set_materialize_grads(False)      # an output without a gradient arrives as None: the kernel's NULL, not a zero tensor
        return flow_up, info_up

    @staticmethod
    def backward(ctx, g_flow, g_info):
        f, i, m = ctx.saved_tensors
        B, H, W, n = ctx.geom
        M, dev = B * H * W, m.device
        if g_flow is None:
            g_flow = torch.zeros(B, 2, 8 * H, 8 * W, device=dev, dtype=torch.float32)
        g_flow = g_flow.float().contiguous()
        g_info = None if g_info is None else g_info.float().contiguous()
        gmask = torch.empty(M, 576, device=dev, dtype=torch.float32)
        gfi = torch.empty(M, 2 + n, device=dev, dtype=torch.float32)
        torch.ops.pfk.convex_upsample_info_bwd(f, i, m, g_flow, g_info, gmask, gfi[:, :2], gfi[:, 2:])
        need = ctx.needs_input_grad
        return (_nchw(gfi[:, :2], B, H, W) if need[0] else None, _nchw(gfi[:, 2:], B, H, W) if need[1] else None,
                _nchw(gmask, B, H, W) if need[2] else None)


def upsample_data_train(flow: torch.Tensor, info: torch.Tensor, mask: torch.Tensor):
    """SEARAFT.upsample_data (sea_raft.py:147-163), differentiable in all three arguments: NCHW fp32 GPU tensors (channel slices of a
    channels-last buffer are read in place) -> ``(flow_up, info_up)``.  An output that receives no gradient counts as a zero one."""
    load_native()
    if not (flow.dim() == 4 and info.dim() == 4 and mask.dim() == 4 and flow.shape[1] == 2 and 1 <= info.shape[1] <= 8
            and mask.shape[1] == 576 and info.shape[0] == flow.shape[0] == mask.shape[0]
            and info.shape[2:] == flow.shape[2:] == mask.shape[2:]):
        raise ValueError(f"upsample_data_train: flow [B, 2, H, W], info [B, 1..8, H, W], mask [B, 576, H, W], got "
                         f"{tuple(flow.shape)}, {tuple(info.shape)}, {tuple(mask.shape)}")
    if not all(t.is_cuda and t.dtype == torch.float32 for t in (flow, info, mask)):
        raise ValueError("upsample_data_train: fp32 GPU tensors")
    return _UpsampleData.apply(flow, info, mask)
