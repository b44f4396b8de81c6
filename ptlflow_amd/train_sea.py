"""Training path of SEA-RAFT's refinement on libpfk kernels (K12d; bf16: K12f), in train.py's idiom: pixel-major rows
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

``precision="bf16"`` (K12f): what the reference trains under ``torch.autocast(bfloat16)``.  Every dense convolution is a
``conv_pm(precision="bf16")`` (``encoder.convf1``, 49 taps, keeps the fp32 kernels with a cast at its boundary, as in train.py) and the
two row nodes run on the ``_b16`` entries: bf16 rows in and out, fp32 arithmetic, one rounding at each store.  The block input
``cat([h, inp, motion, flow])`` is bf16 rows (``inp`` is cast once per forward, `_context_rows`), ``h`` stays bf16 between the blocks,
and everything listed above is saved in bf16 — half the bytes — apart from the fp32 rstd [M].  The last block's ``final`` and each
head's second convolution hand their fp32 accumulators on (``out_fp32``): the loop gets fp32 ``net``, flow / info and mask logits, and
`upsample_data_train` runs on them unchanged.  Parameters, parameter gradients and every accumulator are fp32; the layer-scale fold
is formed in torch on the fp32 parameters and packed to bf16 afterwards.  The block input's gradient is the bf16 sum of the depthwise
backward's bf16 dx and the residual branch's.  What differs between the precisions sits in `_RowKernels`; the rest is written once.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import load_native
from ._seam import pixel_rows
from .conv_path import BF16_ROWS, FP32, ConvPath
from .train import _KERNELS, _nchw, _pm, check_precision, conv_pm, packs_for

LN_EPS = 1e-6              # sea_raft/layer.py:57


class _RowKernels:
    """What the two precisions of the row nodes (`_DwconvLayerNorm`, `_Gelu`) differ in: the element type of the rows and its channel
    quantum (16 bytes), both the conv path's, and the entries' suffix."""

    def __init__(self, path: ConvPath, suffix: str):
        self.dtype, self.quantum, self.suffix = path.dtype, path.quantum, suffix

    def rows(self, t: torch.Tensor) -> torch.Tensor:
        """rows the row kernels read: the element type, unit channel stride, 16-byte aligned rows"""
        t = t if t.dtype == self.dtype else t.to(self.dtype)
        if t.stride(1) != 1 or t.stride(0) % self.quantum or t.data_ptr() % 16:
            t = t.contiguous()
        return t

    def empty(self, like: torch.Tensor, *shape: int) -> torch.Tensor:
        return torch.empty(*shape, device=like.device, dtype=self.dtype)

    def op(self, name: str):
        return getattr(torch.ops.pfk, name + self.suffix)


_ROWS = {"fp32": _RowKernels(FP32, ""), "bf16": _RowKernels(BF16_ROWS, "_b16")}


class _DwconvLayerNorm(torch.autograd.Function):
    """out [M, C] = LayerNorm_C(dwconv_kxk(x) + b) * ln_weight + ln_bias on pixel-major rows (C % 4 == 0, C <= 512, k odd <= 7).
    ``precision="bf16"``: x, out, the saved x^ and both activation gradients are bf16 rows (C % 8 == 0); an fp32 x is rounded here and
    gets its gradient back in fp32."""

    @staticmethod
    def forward(ctx, x, dw_weight, dw_bias, ln_weight, ln_bias, B: int, H: int, W: int, eps: float, precision: str = "fp32"):
        rk = _ROWS[precision]
        ctx.x_dtype = x.dtype
        x = rk.rows(x)
        M, C = x.shape
        k = dw_weight.shape[-1]
        w = dw_weight.detach().float().reshape(C, k * k).contiguous()
        lw = ln_weight.detach().float().contiguous()
        out, xhat = rk.empty(x, M, C), rk.empty(x, M, C)
        rstd = torch.empty(M, device=x.device)
        rk.op("dwconv_layernorm_train")(x, w, None if dw_bias is None else dw_bias.detach().float().contiguous(), lw,
                                        ln_bias.detach().float().contiguous(), eps, out, xhat, rstd, B, H, W, k)
        ctx.rk = rk
        ctx.geom = (B, H, W, k)
        ctx.has_bias = dw_bias is not None
        ctx.wshape = tuple(dw_weight.shape)
        ctx.save_for_backward(x, xhat, rstd, w, lw)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, xhat, rstd, w, lw = ctx.saved_tensors
        rk = ctx.rk
        B, H, W, k = ctx.geom
        M, C = x.shape
        dev = x.device
        dy = rk.rows(dy)
        du = rk.empty(x, M, C)
        dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
        rk.op("layernorm_bwd")(xhat, rstd, lw, dy, du, dgamma, dbeta)
        dx = rk.empty(x, M, C)
        dw = torch.empty(C, k * k, device=dev)
        db = torch.empty(C, device=dev) if ctx.has_bias else None
        rk.op("dwconv_bwd")(x, du, w, dx, dw, db, B, H, W, k)
        need = ctx.needs_input_grad
        return (dx.to(ctx.x_dtype) if need[0] else None, dw.view(ctx.wshape) if need[1] else None,
                db if ctx.has_bias and need[2] else None, dgamma if need[3] else None, dbeta if need[4] else None,
                None, None, None, None, None)


def dwconv_layernorm_pm(x: torch.Tensor, dw_weight: torch.Tensor, dw_bias: Optional[torch.Tensor], ln_weight: torch.Tensor,
                        ln_bias: torch.Tensor, B: int, H: int, W: int, eps: float = LN_EPS, precision: str = "fp32") -> torch.Tensor:
    """ConvNextBlock.dwconv + .norm, differentiable: ``x`` [B*H*W, C] fp32 rows, ``dw_weight`` [C, 1, k, k] (PyTorch's layout; its
    gradient comes back in it), ``dw_bias`` [C] or None, LayerNorm ``ln_weight`` / ``ln_bias`` [C].  ``precision="bf16"``: bf16 rows
    out (``x`` bf16 or fp32 rows, C % 8 == 0); the parameters and their gradients stay fp32."""
    load_native()
    q = _ROWS[check_precision(precision)].quantum
    if x.dim() != 2 or x.shape[0] != B * H * W:
        raise ValueError(f"dwconv_layernorm_pm: x must be [B*H*W, C] rows, got {tuple(x.shape)} for {(B, H, W)}")
    C, k = x.shape[1], dw_weight.shape[-1]
    if C % q or not q <= C <= 512 or k % 2 == 0 or k > 7 or dw_weight.numel() != C * k * k:
        raise ValueError(f"dwconv_layernorm_pm({precision}) covers C % {q} == 0, {q} <= C <= 512 and odd k <= 7, got C = {C}, "
                         f"weight {tuple(dw_weight.shape)}")
    return _DwconvLayerNorm.apply(x, dw_weight, dw_bias, ln_weight, ln_bias, B, H, W, float(eps), precision)


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, precision: str = "fp32"):
        rk = _ROWS[precision]
        ctx.rk, ctx.x_dtype = rk, x.dtype
        x = rk.rows(x)
        y = rk.empty(x, *x.shape)
        rk.op("gelu")(x, y)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        rk = ctx.rk
        dx = rk.empty(x, *x.shape)
        rk.op("gelu_bwd")(x, rk.rows(dy), dx)
        return dx.to(ctx.x_dtype), None


def gelu_pm(x: torch.Tensor, precision: str = "fp32") -> torch.Tensor:
    """nn.GELU() on rows [M, C], differentiable; saves its input.  fp32 rows (C % 4 == 0), or with ``precision="bf16"`` bf16 rows in
    and out (C % 8 == 0; an fp32 ``x`` is rounded first), the formula evaluated in fp32."""
    load_native()
    q = _ROWS[check_precision(precision)].quantum
    if x.dim() != 2 or x.shape[1] % q:
        raise ValueError(f"gelu_pm({precision}): rows [M, C] with C % {q} == 0, got {tuple(x.shape)}")
    return _Gelu.apply(x, precision)


def convnext_block_train_pm(P: Dict[str, torch.Tensor], prefix: str, x: torch.Tensor, B: int, H: int, W: int,
                            cache: Optional[dict] = None, accumulate_wgrad: bool = False, precision: str = "fp32",
                            out_fp32: bool = False) -> torch.Tensor:
    """ConvNextBlock.forward (layer.py:69-83) on rows: ``x`` [M, dim] -> [M, out_dim].  ``P[prefix + ...]``: the block's parameters
    (``prefix`` e.g. "refine.0."; without a ``gamma`` the layer scale is 1).  ``cache`` / ``accumulate_wgrad``: as in
    `train.update_block_train_pm` — with a step-scoped cache the folded pwconv2 weight is formed once per step and the recurrent
    calls add their weight gradients into one buffer per convolution.  ``precision="bf16"``: bf16 rows throughout (module docstring;
    ``x`` bf16 or fp32 rows), bf16 rows out, or with ``out_fp32`` ``final``'s fp32 accumulators."""
    acc = accumulate_wgrad and cache is not None
    p = prefix
    x = x.to(_ROWS[check_precision(precision)].dtype)

    def conv(srcs, w, b, name, params, out32=False):
        return conv_pm(srcs, w, b, B, H, W, False, None, packs_for(cache, p + name, params, acc), 1, precision, out32)

    y = dwconv_layernorm_pm(x, P[p + "dwconv.weight"], P.get(p + "dwconv.bias"), P[p + "norm.weight"], P[p + "norm.bias"], B, H, W,
                            precision=precision)
    w1 = P[p + "pwconv1.weight"]
    y = conv([y], w1[:, :, None, None], P.get(p + "pwconv1.bias"), "pwconv1", [w1])
    y = gelu_pm(y, precision)
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
    y = conv_pm([y], folded[0], folded[1], B, H, W, False, None, packs, 1, precision)
    wf = P[p + "final.weight"]
    return conv([x + y], wf, P.get(p + "final.bias"), "final", [wf], out_fp32)


def _context_rows(i: torch.Tensor, k, cache: Optional[dict], owner: Optional[torch.Tensor]) -> torch.Tensor:
    """The context rows in the operand dtype of ``k``.  bf16: `inp` is the same tensor in every iteration, so with a cache and the
    caller's tensor ``owner`` to know it by, it is rounded ONCE per forward and every iteration's concatenation reads that copy (its
    gradient is summed in fp32 by the one cast's backward).  The entry goes when ``owner`` dies (`train._attention_state`'s rule)."""
    if i.dtype == k.dtype:
        return i
    if cache is None or owner is None or k.dtype == torch.float32:
        return i.to(k.dtype)
    import weakref
    ent = cache.get("inp_rows")
    if ent is not None and ent[0]() is owner and ent[1] == owner._version:
        return ent[2]
    cache.pop("inp_rows", None)

    def gone(ref, cache=cache):
        if cache.get("inp_rows", (None,))[0] is ref:
            del cache["inp_rows"]

    r = i.to(k.dtype)
    cache["inp_rows"] = (weakref.ref(owner, gone), owner._version, r)
    return r


def sea_update_block_train_pm(P: Dict[str, torch.Tensor], spec, h, i, c, f, B: int, H: int, W: int, num_blocks: int,
                              cache: Optional[dict] = None, accumulate_wgrad: bool = False, precision: str = "fp32",
                              context_owner: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sea_raft/update.py:49-54 on rows: ``h`` [M, 128], ``i`` [M, 128], ``c`` [M, corr channels], ``f`` [M, 2] -> ``h'`` [M, 128] fp32.
    The motion encoder as `train.update_block_train_pm` builds it; ``x = cat([h, i, motion, f])`` has 384 channels and each
    block's output replaces ``h``.  ``precision="bf16"``: module docstring; ``context_owner``: the caller's tensor that ``i`` was
    made from (`_context_rows`)."""
    acc = accumulate_wgrad and cache is not None
    k = _KERNELS[check_precision(precision)]

    def conv(srcs, name, real=None, prec=precision):
        w = P[name + ".weight"]
        return conv_pm(srcs, w, P.get(name + ".bias"), B, H, W, True, real, packs_for(cache, name, [w], acc), 1, prec)

    cor = conv([k.pad(c)], "encoder.convc1", [c.shape[1]])
    if spec.c2:
        cor = conv([cor], "encoder.convc2")
    # 7x7: outside pfk_conv2d_b16's 32 taps, fp32 in either mode
    flo = conv([conv([_KERNELS["fp32"].pad(f)], "encoder.convf1", [2], "fp32")], "encoder.convf2")
    motion = conv([cor, flo], "encoder.conv")
    rest = torch.cat([_context_rows(i, k, cache, context_owner), motion, f.to(k.dtype)], 1)
    for b in range(num_blocks):
        h = convnext_block_train_pm(P, f"refine.{b}.", torch.cat([h.to(k.dtype), rest], 1), B, H, W, cache, accumulate_wgrad, precision,
                                    out_fp32=b == num_blocks - 1)
    return h


def sea_head_train_pm(P: Dict[str, torch.Tensor], name: str, h: torch.Tensor, B: int, H: int, W: int,
                      cache: Optional[dict] = None, accumulate_wgrad: bool = False, precision: str = "fp32") -> torch.Tensor:
    """One head (``name`` = "flow_head" | "upsample_weight", sea_raft.py:106-117): 3x3 + relu, then the head's second convolution.
    fp32 rows out in either precision (bf16: the second convolution's fp32 accumulators)."""
    acc = accumulate_wgrad and cache is not None
    w0, w2 = P[name + ".0.weight"], P[name + ".2.weight"]
    y = conv_pm([h], w0, P.get(name + ".0.bias"), B, H, W, True, None, packs_for(cache, name + ".0", [w0], acc), 1, precision)
    return conv_pm([y], w2, P.get(name + ".2.bias"), B, H, W, False, None, packs_for(cache, name + ".2", [w2], acc), 1, precision,
                   precision == "bf16")


def sea_heads_train_pm(P: Dict[str, torch.Tensor], h: torch.Tensor, B: int, H: int, W: int, cache: Optional[dict] = None,
                       accumulate_wgrad: bool = False, precision: str = "fp32"):
    """``(flow_head(h) [M, 6], upsample_weight(h) [M, 576])`` — delta flow (2) | info (4), and the mask logits before the loop's 0.25."""
    return (sea_head_train_pm(P, "flow_head", h, B, H, W, cache, accumulate_wgrad, precision),
            sea_head_train_pm(P, "upsample_weight", h, B, H, W, cache, accumulate_wgrad, precision))


# ---- NCHW faces: what the seams call from the model's own loop (`PfkSeaRaftUpdateBlock`, `_SeaHeadSeam`) ----------------------------
def sea_update_block_train(P: Dict[str, torch.Tensor], spec, net, inp, corr, flow, num_blocks: int, cache: Optional[dict] = None,
                           precision: str = "fp32"):
    B, _, H, W = net.shape
    h = sea_update_block_train_pm(P, spec, _pm(net), _pm(inp), _pm(corr), _pm(flow), B, H, W, num_blocks, cache, precision=precision,
                                  context_owner=inp)
    return _nchw(h, B, H, W)


def sea_head_train(P: Dict[str, torch.Tensor], name: str, net, cache: Optional[dict] = None, precision: str = "fp32"):
    B, _, H, W = net.shape
    return _nchw(sea_head_train_pm(P, name, _pm(net), B, H, W, cache, precision=precision), B, H, W)


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
