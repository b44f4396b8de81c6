"""Training path of the update block on libpfk kernels — SURVEY.md §8 f4 (first half).

The inference path fuses gates and concatenations into convolution epilogues and keeps its state in place, which autograd
cannot see.  For training the update block (ptlflow/models/raft/update.py:6-153) is re-composed from ONE differentiable
primitive, ``conv_pm`` — a "same" convolution over pixel-major ``[B*H*W, C]`` tensors whose forward, data gradient and weight
gradient all run on matrix-core implicit-GEMM kernels — plus one fused autograd node per GRU pass (``_GruPass``: gate
arithmetic and its derivatives in four small fp32 kernels, ``pfk_gru_*``).  Both nodes are written once, against a `_Kernels`
object per precision: ``"fp32"``, or ``"bf16"`` (K12b) — what the reference trains under ``torch.autocast(bfloat16)``.

* forward   ``out = conv(srcs, W) + b`` (relu fused)               -> ``pfk_conv2d_f32`` | ``pfk_conv2d_b16`` LINEAR, bf16 rows out
  (the saved activations are the operand rows: bf16 ones in bf16)
* dgrad     ``dX_s = conv(dY, flip(W_s)^T)``  — a convolution again -> the forward's kernel with a re-packed weight slice
  (K chunks of 32 fp32 | 64 bf16 channels); bf16 rounds the gradient to bf16 first
* wgrad     ``dW[:, c, ky, kx] = sum_p dY[p, :] * X[p + tap, c]``  -> ``pfk_conv_wgrad_unpacked_f32`` | ``_b16``: the transposed
  product with the PIXEL as reduction index on the same matrix cores, read straight from the pixel-major tensors (tap
  padding by out-of-range buffer offsets, operands fetched from LDS "transposed": conflict-free ``ds_read_b32`` |
  ``ds_read_b64_tr_b16`` feeding ``v_mfma_f32_32x32x16_bf16``), pixel range cut into slices that are summed in a fixed order
  (deterministic); fp32 dW / db in PyTorch's layouts, the bias gradient being one more K chunk; step-scoped accumulation
  (`ConvPacks.acc`, `_Flush`) in both
* dbias     without a weight gradient: column sums (torch).
* GRU pass  the pre-activations are fp32 rows and the gate arithmetic is fp32 in both; bf16: ``h`` stays fp32 with a bf16 copy as
  the convolutions' operand, ``r * h`` is rounded to bf16.

Every MIOpen convolution of the update block's forward and backward is gone; the encoders, the correlation volume and
the lookup have their own nodes (train_encoder.py, corr.py).

Hidden state, coordinates, flow, loss, every parameter, every parameter gradient and every accumulator stay fp32 in either
precision.  Layers outside ``pfk_conv2d_b16``'s envelope keep the fp32 kernels, with a cast at their boundary:

* ``encoder.convf1`` (7x7 = 49 taps; K8b takes at most 32).

No other layer of the basic / small / GMA update block is refused; a strided convolution is (the update block has none).

GMA (K12c) — the attention map and its per-iteration use, in both precisions, with no torch matmul or softmax:

* ``_AttentionMap``   once per step, fp32: ``to_qk`` as a ``conv_pm``, ``P = softmax_rows(scale q k^T)`` on K1 (``pfk_corr_volume_f32``) +
  ``pfk_softmax_rows_f32``; backward ``pfk_softmax_rows_bwd_f32`` then ``pfk_corr_volume_bwd_f32`` per pair for dq, dk
* ``pack_attention``  once per step: P and P^T as zero-padded GEMM operands, fp32 or bf16, one pass of ``pfk_transpose_pack_*``
* ``_AttnMatmul``     once per iteration: ``agg = P v`` and ``dV = P^T dAgg`` on the convolution GEMMs (``pfk_conv2d_f32`` per pair /
  one batched ``pfk_conv2d_b16``) with ``v^T`` / ``dAgg^T`` as the K-contiguous weight; the map's gradient ``dAgg v^T`` is K1 with scale 1 —
  per use, or with a step sink (``_AttnFlush``) ONE product over the concatenated K = T*C of all uses of the step.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import conv_path, load_native
from .conv_path import PRECISIONS  # noqa: F401  (re-exported: tests and the seams import it from here)
from .packing import round_up


def _segments(srcs: Sequence[torch.Tensor], real: Sequence[int]) -> List[Tuple[int, int, int]]:
    segs, first = [], 0
    for s, n in zip(srcs, real):
        segs.append((first, n, s.shape[1]))
        first += n
    return segs


class _Geometry:
    """Input grid (B, H, W), kernel and stride of one convolution; the output grid is (Ho, Wo) = ((H-1)//stride + 1, ...).
    ``precision``: "fp32" | "bf16" | "bf16-f32out" — which kernels the `_ConvPM` node of this convolution runs on."""
    __slots__ = ("B", "H", "W", "kh", "kw", "stride", "precision")

    def __init__(self, B, H, W, kh, kw, stride=1, precision="fp32"):
        self.B, self.H, self.W, self.kh, self.kw, self.stride, self.precision = B, H, W, kh, kw, stride, precision

    @property
    def Ho(self):
        return (self.H - 1) // self.stride + 1

    @property
    def Wo(self):
        return (self.W - 1) // self.stride + 1


def _workspace(device) -> torch.Tensor:
    ws = _workspace.cache.get(device)
    if ws is None:
        ws = torch.zeros(torch.ops.pfk.conv_workspace_bytes(), device=device, dtype=torch.uint8)
        _workspace.cache[device] = ws
    return ws


_workspace.cache = {}


class ConvPacks:
    """Packed forms of one convolution weight, built lazily and reused for as long as the parameter versions in ``key`` do
    not change — i.e. for all recurrent iterations of a training step.  ``packed``: {(precision, "fwd") | (precision, "dgrad",
    source): operand}, so an entry used under both precisions keeps both forms apart.

    ``acc``: gradient accumulators of a step-scoped entry (`packs_for(..., accumulate=True)`): the weight-gradient launches of
    all recurrent uses add into ONE buffer per parameter (`pfk_conv_wgrad_unpacked_f32(accumulate=1)`) and a `_Flush` node
    hands the total to autograd once — instead of every use returning its own gradient and the engine adding them (eleven
    small additions per parameter and step at 12 iterations)."""
    __slots__ = ("key", "packed", "accumulate", "acc", "alias", "extra")

    def __init__(self, key=None, accumulate=False):
        self.key, self.packed = key, {}
        self.accumulate = accumulate
        self.acc = None          # {position among the parameters given to _Flush: accumulator}, None before the first use
        self.alias = None        # the parameters as seen by the uses of this step (outputs of _Flush)
        self.extra = {}          # per-step derived tensors (the z|r weight concatenation)


def packs_for(cache: Optional[dict], name: str, params: Sequence[torch.Tensor], accumulate: bool = False) -> ConvPacks:
    """``accumulate=True`` only for a ``cache`` that lives for ONE forward / backward (the mirror's training forward creates a
    fresh dict per step): the accumulators belong to that step's graph."""
    key = tuple((p.data_ptr(), p._version) for p in params)
    if cache is None:
        return ConvPacks(key)
    entry = cache.get(name)
    if entry is None or entry.key != key:
        entry = cache[name] = ConvPacks(key, accumulate)
    return entry


class _Flush(torch.autograd.Function):
    """Identity on a group of parameters whose uses accumulate their gradients in ``packs.acc`` (and return None): this node
    sits between the parameters and ALL their uses, so the engine runs its backward after the last use — whatever the order,
    however many uses — and it hands the totals on.  (Uses that never ran simply did not contribute; nothing is counted.)"""

    @staticmethod
    def forward(ctx, packs, *params):
        ctx.set_materialize_grads(False)
        ctx.packs = packs
        return tuple(p.view_as(p) for p in params)

    @staticmethod
    def backward(ctx, *grads):
        packs = ctx.packs
        acc, packs.acc = packs.acc, None
        # break the cycle ConvPacks -> alias (this node's outputs) -> grad_fn -> ctx -> ConvPacks, and drop the step's
        # accumulators: a later backward through the same graph returns its gradients the ordinary way (g below)
        packs.alias = None
        packs.extra.pop("dwzr", None)
        packs.extra.pop("dbzr", None)
        out = []
        for i, g in enumerate(grads):          # accumulated total, plus whatever a use returned the ordinary way
            a = None if acc is None else acc.get(i)
            out.append(a if g is None else (g if a is None else a + g))
        return (None, *out)


def step_params(packs: ConvPacks, *params):
    """The parameters as the uses of this step see them: aliases behind one `_Flush` node (accumulating entries) or themselves."""
    if not packs.accumulate or not any(p is not None and p.requires_grad for p in params) or not torch.is_grad_enabled():
        return params
    if packs.alias is None:
        real = [p for p in params if p is not None]
        out = iter(_Flush.apply(packs, *real))
        packs.alias = tuple(None if p is None else next(out) for p in params)
    return packs.alias


BF16 = torch.bfloat16


def check_precision(precision: str, what: str = "precision") -> str:
    return conv_path.check_precision(precision, PRECISIONS, what)


def _rows_b16(s: torch.Tensor) -> torch.Tensor:
    """bf16 rows with unit channel stride and a row stride that is a multiple of 8 (what the b16 kernels read)."""
    s = s if s.dtype == BF16 else s.to(BF16)
    if s.stride(1) != 1 or s.stride(0) % 8 or s.data_ptr() % 16:
        s = s.contiguous()
    return s


class _Kernels:
    """What the two training precisions differ in — everything else of `_ConvPM` and `_GruPass` is written once.  Name, operand
    dtype, channel quantum, the packed weight and the forward launch are the conv path's (conv_path.py); the autograd-only parts are
    here.  This is the fp32 instance: fp32 operands, channel counts in multiples of 4, packed weights in K chunks of 32 channels,
    outputs as wide as the weight, any odd kernel and stride."""
    path, pads_cout = conv_path.FP32, False
    workspace = staticmethod(_workspace)      # the stream-K scratch of the forward kernel

    name = property(lambda self: self.path.name)
    dtype = property(lambda self: self.path.dtype)
    quantum = property(lambda self: self.path.quantum)
    pack = property(lambda self: self.path.pack)

    def check(self, g: _Geometry, srcs) -> None:
        """Refuses what the kernels do not cover."""

    def rows(self, t: torch.Tensor) -> torch.Tensor:
        """``t`` (of the operand dtype already, or any dtype in bf16) in the layout the kernels read."""
        return t.contiguous() if t.stride(1) != 1 else t

    def operand(self, t: torch.Tensor) -> torch.Tensor:
        """``t`` in the operand dtype: ``t`` itself where it is contiguous fp32 | its rounding to bf16."""
        return t.float().contiguous()

    def pad(self, x: torch.Tensor) -> torch.Tensor:
        """Channels zero-padded to the quantum."""
        c = x.shape[1]
        return x if c % self.quantum == 0 else F.pad(x, (0, round_up(c, self.quantum) - c))

    def cout_buf(self, cout: int) -> int:
        """Width of the output rows (and of the bias and the forward weight's rows) the forward kernel is given."""
        return round_up(cout, self.quantum) if self.pads_cout else cout

    def conv(self, srcs, g: _Geometry, wpack, bias, cout: int, relu: bool, out, residual=None, stride: int = 1) -> None:
        self.path.conv(torch.ops.pfk, srcs=list(srcs), B=g.B, H=g.H, W=g.W, kh=g.kh, kw=g.kw, weight=wpack, bias=bias, cout=cout,
                       out=out, relu=relu, workspace=self.workspace(out.device), residual=residual, stride=stride)

    def wgrad(self, srcs, dY, g: _Geometry, dW, db, reals, accumulate: bool) -> None:
        torch.ops.pfk.conv_wgrad_unpacked(list(srcs), dY, g.B, g.H, g.W, g.kh, g.kw, dW, db, reals, g.stride, accumulate)


class _KernelsB16(_Kernels):
    """bf16 operands on ``pfk_conv2d_b16`` / ``pfk_conv_wgrad_unpacked_b16``: channel counts in multiples of 8, K chunks of 64
    channels, output rows padded to 8 channels (a 2-channel head); stride 1 and at most 32 taps."""
    path, pads_cout = conv_path.BF16_ROWS, True
    rows = staticmethod(_rows_b16)
    workspace = staticmethod(lambda device: None)

    def check(self, g, srcs):
        if g.stride != 1:
            raise ValueError("conv_pm(precision='bf16') covers stride 1 only")
        if g.kh * g.kw > 32:
            raise ValueError("conv_pm(precision='bf16'): pfk_conv2d_b16 takes at most 32 taps; keep this layer on precision='fp32'")
        assert all(s.shape[1] % 8 == 0 for s in srcs), "bf16 sources need channel counts that are multiples of 8"

    def operand(self, t):
        return t.to(BF16)

    def wgrad(self, srcs, dY, g, dW, db, reals, accumulate):
        torch.ops.pfk.conv_wgrad_unpacked_b16(list(srcs), dY, g.B, g.H, g.W, g.kh, g.kw, dW, db, reals, accumulate)


_KERNELS = {"fp32": _Kernels(), "bf16": _KernelsB16()}
# `_Geometry.precision` -> (kernels, dtype of the forward's output rows); "bf16-f32out": the fp32 accumulators as they are
_NODE = {"fp32": (_KERNELS["fp32"], torch.float32), "bf16": (_KERNELS["bf16"], BF16), "bf16-f32out": (_KERNELS["bf16"], torch.float32)}


def _fwd_pack(packs: ConvPacks, k: _Kernels, weight: torch.Tensor, segs) -> torch.Tensor:
    """The forward kernel's weight [cout_buf, ktot]; rows past cout (a 2-channel head padded to 8) are zero."""
    key = (k.name, "fwd")
    if key not in packs.packed:
        w = weight.detach().float()
        extra = k.cout_buf(w.shape[0]) - w.shape[0]
        if extra:
            w = F.pad(w, (0, 0, 0, 0, 0, 0, 0, extra))
        packs.packed[key] = k.pack(w, segs)
    return packs.packed[key]


def _dgrad_weight(k: _Kernels, weight: torch.Tensor, seg, dy_channels: int) -> torch.Tensor:
    """Packed weight of the data-gradient convolution w.r.t. one source: W[:, seg] with in / out swapped and the taps flipped,
    [n_buf, taps * round_up(dy_channels, kpad)] in the forward kernel's K order (tap major, then dY's channels)."""
    first, n, n_buf = seg
    cout = weight.shape[0]
    wt = weight.detach().float()[:, first:first + n].permute(1, 0, 2, 3).flip(2, 3)        # [n, cout, kh, kw]
    if n_buf > n:
        wt = F.pad(wt, (0, 0, 0, 0, 0, 0, 0, n_buf - n))                                   # padded channels: zero gradient
    return k.pack(wt.contiguous(), [(0, cout, dy_channels)])


def dgrad_weight_b16(weight: torch.Tensor, seg, dy_channels: int) -> torch.Tensor:
    """`_dgrad_weight` for K8b: bf16 [n_buf, taps * round_up(dy_channels, 64)]."""
    return _dgrad_weight(_KERNELS["bf16"], weight, seg, dy_channels)


def _dgrad_pack(packs: ConvPacks, k: _Kernels, i: int, weight: torch.Tensor, seg, dy_channels: int) -> torch.Tensor:
    key = (k.name, "dgrad", i)
    if key not in packs.packed:
        packs.packed[key] = _dgrad_weight(k, weight, seg, dy_channels)
    return packs.packed[key]


class _ConvPM(torch.autograd.Function):
    """out[M, cout] = relu?(conv(cat(srcs), weight) + bias) on pixel-major tensors; srcs[i] is [M, C_i] with C_i % 4 == 0
    (bf16: % 8; ``real[i]`` <= C_i real channels, the rest zero padding).  ``g.precision``:

    "fp32"         fp32 sources (taken as they are), fp32 out
    "bf16"         bf16 or fp32 sources (fp32 ones are rounded here: the cast at an fp32 layer's boundary), bf16 rows out
    "bf16-f32out"  the same with the fp32 accumulators as they are (the heads' last layers)"""

    @staticmethod
    def forward(ctx, weight, bias, g: _Geometry, relu: bool, real: Tuple[int, ...], packs: ConvPacks, *srcs):
        k, out_dtype = _NODE[g.precision]
        k.check(g, srcs)
        ctx.src_dtypes = tuple(s.dtype for s in srcs)
        srcs = [k.rows(s) for s in srcs]
        cout = weight.shape[0]
        cout_buf = k.cout_buf(cout)
        buf = torch.empty(g.B * g.Ho * g.Wo, cout_buf, device=srcs[0].device, dtype=out_dtype)
        b = None
        if bias is not None:
            b = bias.detach().float().contiguous()
            b = b if cout_buf == cout else F.pad(b, (0, cout_buf - cout))
        k.conv(srcs, g, _fwd_pack(packs, k, weight, _segments(srcs, real)), b, cout_buf, relu, buf, stride=g.stride)
        out = buf if cout_buf == cout else buf[:, :cout]
        ctx.g, ctx.relu, ctx.real, ctx.has_bias, ctx.packs = g, relu, real, bias is not None, packs
        ctx.save_for_backward(weight, out if relu else None, *srcs)
        return out

    @staticmethod
    def backward(ctx, dY):
        weight, out, *srcs = ctx.saved_tensors
        g, real, packs = ctx.g, ctx.real, ctx.packs
        k = _NODE[g.precision][0]
        cout = weight.shape[0]
        M = g.B * g.H * g.W
        dev = dY.device
        dY = k.operand(dY)          # bf16: what autocast's backward hands the convolution, the gradient of a 16-bit output
        if ctx.relu:
            dY = torch.ops.aten.threshold_backward(dY, out.to(k.dtype), 0.0)     # dY * (out > 0) in one kernel (what torch's relu backward runs)
        need = ctx.needs_input_grad      # (weight, bias, g, relu, real, packs, *srcs)
        dW = db = None
        dsrcs: List[Optional[torch.Tensor]] = [None] * len(srcs)
        # channels of dY padded to the quantum for its role as a convolution source (flow head: cout = 2)
        dY_src = k.rows(k.pad(dY))
        segs = _segments(srcs, real)
        # ---- dgrad: dX_s = conv(dY, W_s^T flipped); for a strided convolution the gradient is first spread over the input grid
        # (zeros between the samples: the transposed convolution written as a stride-1 one)
        dY_in = dY_src
        if g.stride != 1 and any(need[6:]):
            dY_in = torch.zeros(g.B, g.H, g.W, dY_src.shape[1], device=dev, dtype=dY_src.dtype)
            dY_in[:, ::g.stride, ::g.stride] = dY_src.view(g.B, g.Ho, g.Wo, -1)
            dY_in = dY_in.view(M, -1)
        for i, seg in enumerate(segs):
            if not need[6 + i]:
                continue
            dx = torch.empty(M, seg[2], device=dev, dtype=ctx.src_dtypes[i])     # the source's dtype: fp32, or in bf16 also bf16 rows
            k.conv([dY_in], g, _dgrad_pack(packs, k, i, weight, seg, dY_src.shape[1]), None, seg[2], False, dx)
            dsrcs[i] = dx
        # ---- wgrad: one launch + a deterministic slice reduction straight from the pixel-major tensors; the reduction writes
        # PyTorch's [cout, cin, kh, kw] / [cout] layouts directly, the bias gradient being one more K chunk whose A operand is
        # a column of ones
        want_b = ctx.has_bias and need[1]
        if need[0]:
            # a step-scoped entry adds into the parameter's accumulators (allocated by the first use) and `_Flush` returns the
            # totals once (weight, [bias]); any other returns its own
            accumulate = packs.accumulate and packs.alias is not None
            first = not accumulate or packs.acc is None
            bufs = packs.acc
            if first:
                bufs = {0: torch.empty(weight.shape, device=dev, dtype=torch.float32)}
                if want_b:
                    bufs[1] = torch.empty(cout, device=dev, dtype=torch.float32)
                if accumulate:
                    packs.acc = bufs
            k.wgrad(srcs, dY_src, g, bufs[0], bufs.get(1), [n for _, n, _ in segs], not first)
            if not accumulate:
                dW, db = bufs[0].to(weight.dtype), bufs.get(1)
        elif want_b:
            db = dY.float().sum(0)          # the unpadded gradient's column sums, in fp32
        return (dW, db, None, None, None, None, *dsrcs)


def _unpack_wgrad(packed: torch.Tensor, weight_shape, segs, g: _Geometry) -> torch.Tensor:
    """packed [cout(+pad), ktot] (the forward weight's layout) -> PyTorch layout [cout, cin, kh, kw]."""
    cout = weight_shape[0]
    taps = g.kh * g.kw
    dW = torch.empty(weight_shape, device=packed.device, dtype=torch.float32)
    k0 = 0
    for first, n, n_buf in segs:
        cpad = round_up(n_buf, 32)
        blk = packed[:cout, k0:k0 + taps * cpad].view(cout, g.kh, g.kw, cpad)[..., :n]
        dW[:, first:first + n] = blk.permute(0, 3, 1, 2)
        k0 += taps * cpad
    return dW


class _GruPass(torch.autograd.Function):
    """One ConvGRU / SepConvGRU pass (raft/update.py:24-32, 58-73) as a single autograd node:
        z, r = sigmoid(conv([h, x], Wz|Wr));  q = tanh(conv([r*h, x], Wq));  h' = (1 - z) h + z q
    two convolutions + two fused gate kernels forward; backward = two gate-derivative kernels, four data-gradient
    convolutions (the second pair accumulates into the first pair's results through the epilogue's residual input) and two
    weight-gradient launches."""

    @staticmethod
    def forward(ctx, h, x, wz, wr, wq, bz, br, bq, g: _Geometry, x_real: int, pk_zr: ConvPacks, pk_q: ConvPacks,
                pzr: Optional[torch.Tensor] = None, pq: Optional[torch.Tensor] = None, precision: str = "fp32"):
        """``pzr`` [M, 2C] / ``pq`` [M, C]: additive terms of the z|r and q pre-activations — the loop-invariant context part of
        the gate convolutions, computed once per step by the caller (`update_block_train_pm`); ``x`` / the weights then cover
        the remaining input channels only.  Their gradient is the pre-activation gradient itself.

        ``precision="bf16"``: ``x`` is bf16 rows (``Cx % 8 == 0``), ``h`` fp32; the four convolutions and the two weight
        gradients run on bf16 operands, everything between them in fp32 (module docstring)."""
        ops = torch.ops.pfk
        ctx.precision = precision
        k = _KERNELS[precision]
        k.check(g, [h, x])
        h = h.float().contiguous()
        x = k.rows(k.operand(x))
        M, C = h.shape
        dev = h.device
        if "wzr" not in pk_zr.extra:      # once per (parameter version): the z and r convolutions run as one
            pk_zr.extra["wzr"] = torch.cat([wz.detach(), wr.detach()], 0).float()
            pk_zr.extra["bzr"] = torch.cat([bz.detach(), br.detach()], 0).float().contiguous()
        wzr, bzr = pk_zr.extra["wzr"], pk_zr.extra["bzr"]
        segs = [(0, C, C), (C, x_real, x.shape[1])]
        hb = k.operand(h)                  # the convolutions' operand; the state itself stays fp32

        def res(p):                        # the epilogue's residual input takes the operand dtype or fp32
            return None if p is None else (p.detach() if p.dtype == k.dtype else p.detach().float()).contiguous()

        a_zr = torch.empty(M, 2 * C, device=dev, dtype=torch.float32)       # fp32 pre-activations: the accumulators, unrounded
        k.conv([hb, x], g, _fwd_pack(pk_zr, k, wzr, segs), bzr, 2 * C, False, a_zr, res(pzr))
        z, r, rh = (torch.empty(M, C, device=dev, dtype=torch.float32) for _ in range(3))
        ops.gru_gates_zr(a_zr, h, z, r, rh)
        rh = k.operand(rh)
        a_q = torch.empty(M, C, device=dev, dtype=torch.float32)
        k.conv([rh, x], g, _fwd_pack(pk_q, k, wq, segs), bq.detach().float().contiguous(), C, False, a_q, res(pq))
        q, hn = torch.empty_like(a_q), torch.empty_like(a_q)
        ops.gru_gates_q(a_q, z, h, q, hn)
        ctx.g, ctx.x_real, ctx.pk_zr, ctx.pk_q, ctx.wzr = g, x_real, pk_zr, pk_q, wzr
        ctx.has_p = (pzr is not None, pq is not None)
        ctx.p_dtypes = (None if pzr is None else pzr.dtype, None if pq is None else pq.dtype)
        ctx.save_for_backward(h, x, z, r, q, rh, wq)      # r*h as the operand it was; h's operand form is derived again in backward
        return hn

    @staticmethod
    def backward(ctx, dhn):
        ops = torch.ops.pfk
        h, x, z, r, q, rh, wq = ctx.saved_tensors
        k, g, x_real, pk_zr, pk_q, wzr = _KERNELS[ctx.precision], ctx.g, ctx.x_real, ctx.pk_zr, ctx.pk_q, ctx.wzr
        M, C = h.shape
        Cx = x.shape[1]
        dev = h.device
        segs = [(0, C, C), (C, x_real, Cx)]
        dhn = dhn.float()
        if dhn.stride(1) != 1:
            dhn = dhn.contiguous()
        da_q = torch.empty(M, C, device=dev, dtype=torch.float32)
        da_zr = torch.empty(M, 2 * C, device=dev, dtype=torch.float32)
        dh = torch.empty(M, C, device=dev, dtype=torch.float32)
        ops.gru_backward_q(dhn, z, q, h, da_q, da_zr, dh)

        def dgrad(dy, packs, weight, i, n_out, residual=None):
            out = torch.empty(M, n_out, device=dev, dtype=torch.float32)
            k.conv([dy], g, _dgrad_pack(packs, k, i, weight, segs[i], dy.shape[1]), None, n_out, False, out, residual)
            return out

        dy_q = k.operand(da_q)             # each pre-activation gradient in operand form once: both dgrads and the wgrad read it
        d_rh = dgrad(dy_q, pk_q, wq, 0, C)
        dx = dgrad(dy_q, pk_q, wq, 1, Cx)
        ops.gru_backward_zr(d_rh, h, r, da_zr, dh)
        dy_zr = k.operand(da_zr)
        dh = dgrad(dy_zr, pk_zr, wzr, 0, C, residual=dh)          # + dh through the epilogue's fp32 residual input
        dx = dgrad(dy_zr, pk_zr, wzr, 1, Cx, residual=dx).to(x.dtype)
        hb = k.operand(h)
        reals = [n for _, n, _ in segs]
        gp = (None if not ctx.has_p[0] else da_zr.to(ctx.p_dtypes[0]), None if not ctx.has_p[1] else da_q.to(ctx.p_dtypes[1]))
        # step-scoped entries: every pass of every iteration adds into one buffer per parameter (allocated by the first) and
        # `_Flush` returns the totals; any other returns its own
        accumulate = pk_zr.accumulate and pk_zr.alias is not None and pk_q.alias is not None
        first = not accumulate or pk_q.acc is None
        if first:
            dwq, dbq = torch.empty(wq.shape, device=dev, dtype=torch.float32), torch.empty(C, device=dev, dtype=torch.float32)
            dwzr, dbzr = torch.empty(wzr.shape, device=dev, dtype=torch.float32), torch.empty(2 * C, device=dev, dtype=torch.float32)
            if accumulate:
                pk_q.acc = {0: dwq, 1: dbq}
                pk_zr.extra["dwzr"], pk_zr.extra["dbzr"] = dwzr, dbzr
                pk_zr.acc = {0: dwzr[:C], 1: dwzr[C:], 2: dbzr[:C], 3: dbzr[C:]}      # (wz, wr, bz, br) as given to _Flush
        else:
            dwq, dbq, dwzr, dbzr = pk_q.acc[0], pk_q.acc[1], pk_zr.extra["dwzr"], pk_zr.extra["dbzr"]
        k.wgrad([rh, x], dy_q, g, dwq, dbq, reals, not first)
        k.wgrad([hb, x], dy_zr, g, dwzr, dbzr, reals, not first)
        gw = (None,) * 6 if accumulate else (dwzr[:C], dwzr[C:], dwq, dbzr[:C], dbzr[C:], dbq)
        return (dh, dx, *gw, None, None, None, None, gp[0], gp[1], None)


def conv_pm(srcs: Sequence[torch.Tensor], weight: torch.Tensor, bias: Optional[torch.Tensor], B: int, H: int, W: int,
            relu: bool = False, real: Optional[Sequence[int]] = None, packs: Optional[ConvPacks] = None,
            stride: int = 1, precision: str = "fp32", out_fp32: bool = False) -> torch.Tensor:
    """Differentiable convolution (odd kernel, padding k//2, stride s: PyTorch's Conv2d(k, stride=s, padding=k//2)) of the
    channel-concatenation of ``srcs`` (pixel-major ``[B*H*W, C_i]``, ``C_i % 4 == 0``) with a PyTorch-layout weight
    ``[cout, sum(real), kh, kw]``; returns ``[B*Ho*Wo, cout]``.  ``packs``: a ``ConvPacks`` from ``packs_for`` to reuse the
    packed weights across calls.

    ``precision="bf16"``: the node on the bf16 matrix cores (module docstring) — stride 1, at most 32 taps, ``C_i % 8 == 0``;
    sources may be bf16 or fp32 rows (their gradient comes back in their dtype), the result is bf16 rows, or with ``out_fp32``
    the fp32 accumulators unrounded (the incoming gradient is rounded to bf16 either way); weight / bias gradients are fp32."""
    load_native()
    check_precision(precision)
    real = tuple(int(s.shape[1]) for s in srcs) if real is None else tuple(real)
    assert sum(real) == weight.shape[1], (real, tuple(weight.shape))
    if precision == "bf16" and out_fp32:
        precision = "bf16-f32out"
    g = _Geometry(B, H, W, weight.shape[2], weight.shape[3], int(stride), precision)
    packs = packs if packs is not None else ConvPacks()
    weight, bias = step_params(packs, weight, bias)
    return _ConvPM.apply(weight, bias, g, relu, real, packs, *srcs)


# --------------------------------------------------------------------------------------------------------------------
# GMA (K12c): the attention map and its per-iteration use `attn @ v` (gma_utils.py:50-78, 100-113)
# --------------------------------------------------------------------------------------------------------------------
class AttnState:
    """The attention map of one forward, packed for the GEMMs of `_AttnMatmul` (built once per step by `pack_attention`):

    ``P``  [B][N][ld]  the map, the A operand of ``agg = P @ v``       — fp32 (ld = N rounded up to 4) or bf16 (to 8)
    ``PT`` [B][N][ld]  its transpose, the A operand of ``dV = P^T @ dAgg``
    both with zero pad columns, written in one pass by `pfk_transpose_pack_*`.  ``map``: with a step sink, the map's alias behind
    an `_AttnFlush` node — what the uses of the step hang on in the autograd graph; None otherwise: the state holds no reference to
    the caller's tensor (a cache that outlives the step must not keep the map and its graph alive), the uses take it directly."""
    __slots__ = ("map", "B", "H", "W", "N", "ld", "path", "P", "PT", "wt", "sink", "uses", "dcat", "vcat", "__weakref__")

    @property
    def dtype(self):
        return self.path.dtype

    def target(self, attention: torch.Tensor) -> torch.Tensor:
        """The tensor a use passes to `_AttnMatmul` as the receiver of the map's gradient."""
        return self.map if self.sink and self.map is not None else attention


def pack_attention(attention: torch.Tensor, B: int, H: int, W: int, precision: str = "fp32", sink: bool = False) -> AttnState:
    """``attention`` [B, 1, N, N] (one head) -> `AttnState`.  ``sink`` (a step-scoped caller only, like ``accumulate_wgrad``): the
    uses of this step leave their part of the map's gradient in two [B][N][T*C] buffers and an `_AttnFlush` node between the
    map and all its uses writes the N x N gradient once."""
    N = H * W
    if attention.dim() != 4 or tuple(attention.shape) != (B, 1, N, N):
        raise ValueError(f"attention must be [B, 1, N, N] = {(B, 1, N, N)} (one head), got {tuple(attention.shape)}")
    load_native()
    st = AttnState()
    st.B, st.H, st.W, st.N, st.path = B, H, W, N, _KERNELS[check_precision(precision)].path
    st.ld = round_up(N, st.path.quantum)
    a = attention.detach().float().reshape(B, N, N)
    if a.stride(2) != 1 or a.stride(0) != N * a.stride(1):
        a = a.contiguous()
    st.PT = torch.empty(B, N, st.ld, device=a.device, dtype=st.dtype)
    if not st.path.b16 and st.ld == N and a.is_contiguous():
        st.P = a                                  # already a legal operand: only the transpose is written
        torch.ops.pfk.transpose_pack(a, st.PT, None)
    else:
        st.P = torch.empty_like(st.PT)
        torch.ops.pfk.transpose_pack(a, st.PT, st.P)
    st.wt, st.uses, st.dcat, st.vcat = {}, 0, None, None
    st.sink = bool(sink) and attention.requires_grad and torch.is_grad_enabled()
    st.map = _AttnFlush.apply(st, attention) if st.sink else None
    return st


def _attn_gemm(st: AttnState, A: torch.Tensor, x: torch.Tensor, out: torch.Tensor) -> None:
    """out[b] = A[b] @ x[b] for A = st.P or st.PT ([B][N][ld]), x / out pixel-major rows [B*N, C]: the 1x1 "convolution" of
    `UpdateEngine._aggregate` with x[b]^T as its K-contiguous weight — fp32 on pfk_conv2d_f32 (grouped over the pairs), bf16
    as ONE batched pfk_conv2d_b16."""
    ops = torch.ops.pfk
    B, N, C = st.B, st.N, x.shape[1]
    wt = st.wt.get(C)
    if wt is None:       # pad columns stay zero; the columns below N are rewritten by every use (same stream: no hazard)
        wt = st.wt[C] = torch.zeros(B, C, round_up(st.ld, st.path.kchunk), device=x.device, dtype=st.dtype)
    gemm = dict(B=1, H=st.H, W=st.W, kh=1, kw=1, bias=None, cout=C)
    if st.path.b16:
        wt[:, :, :N].copy_(x.view(B, N, C).transpose(1, 2))
        st.path.conv(ops, srcs=[A], weight=wt, out=out.view(B, N, C), **gemm)
        return
    ops.pm_to_cm(x, wt)
    if B == 1:
        st.path.conv(ops, srcs=[A[0]], weight=wt[0], out=out, workspace=_workspace(x.device), **gemm)
        return
    none = x.new_empty(0)
    for b0 in range(0, B, 4):      # up to four pairs' tiles resident together (`UpdateEngine._aggregate`)
        bs = range(b0, min(B, b0 + 4))
        ops.conv2d_group([A[b] for b in bs], 1, st.H, st.W, [1] * len(bs), [wt[b] for b in bs], [none] * len(bs), [0] * len(bs),
                         [1.0] * len(bs), [out[b * N:(b + 1) * N] for b in bs], [])


def _outer_k1(a: torch.Tensor, b: torch.Tensor, B: int, N: int) -> torch.Tensor:
    """K1 with scale 1 on pixel-major rows [B*N, D]: [B, 1, N, N] fp32 = a[b] @ b[b]^T (bf16 rows: the bf16 K1, then widened)."""
    D = a.shape[1]
    out = torch.empty(B, N, N, device=a.device, dtype=a.dtype)
    (torch.ops.pfk.corr_volume_bf16 if a.dtype == BF16 else torch.ops.pfk.corr_volume)(a.view(B, N, D), b.view(B, N, D), 1.0, out)
    return out.float().view(B, 1, N, N)


class _AttnFlush(torch.autograd.Function):
    """Identity on the attention map, between the map and ALL its uses of one step (the `_Flush` pattern): the uses return no
    gradient for the map but leave dAgg_t and v_t in slot t of ``st.dcat`` / ``st.vcat`` [B][N][T*C]; the engine runs this node after
    the last of them and ONE K1 with K = T*C writes  dP = sum_t dAgg_t v_t^T.  A use that never ran backward left its slot zero.
    The node holds the state WEAKLY (the uses and the step's cache hold it): AttnState -> map (this node's output) -> grad_fn -> ctx
    is then no cycle, and a forward whose backward never runs frees P and P^T with the step like any other tensor."""

    @staticmethod
    def forward(ctx, st, amap):
        import weakref
        ctx.set_materialize_grads(False)
        ctx.st = weakref.ref(st)
        return amap.view_as(amap)

    @staticmethod
    def backward(ctx, g):
        st = ctx.st()
        if st is None:       # no use is alive: nothing was left in the sink
            return None, g
        dcat, vcat, st.dcat, st.vcat = st.dcat, st.vcat, None, None
        st.map = None        # the sink is closed: a later backward through the same graph gets its gradients the ordinary way
        if dcat is not None:
            total = _outer_k1(dcat.view(st.B * st.N, -1), vcat.view(st.B * st.N, -1), st.B, st.N)
            g = total if g is None else total + g
        return None, g


class _AttnMatmul(torch.autograd.Function):
    """agg [M, C] fp32 = P[b] @ v[b] per pair (gma_utils.py:108, `torch.einsum('b h i j, b h j d -> b h i d')` with one head).
    ``amap``: the tensor the map's gradient goes to (`AttnState.target`); ``v`` [M, C] fp32 or bf16 rows, C % 32 == 0.
    bf16: P, P^T, v and the incoming gradient are bf16 operands (what autocast hands a 16-bit matmul), accumulation fp32."""

    @staticmethod
    def forward(ctx, amap, v, st: AttnState):
        if v.shape[1] % 32:
            raise ValueError(f"_AttnMatmul: the value width must be a multiple of 32, got {v.shape[1]}")
        v = _rows_b16(v) if st.path.b16 else v.float().contiguous()
        out = torch.empty(v.shape[0], v.shape[1], device=v.device, dtype=torch.float32)
        _attn_gemm(st, st.P, v, out)
        ctx.st, ctx.slot = st, st.uses
        st.uses += 1
        ctx.save_for_backward(v)
        return out

    @staticmethod
    def backward(ctx, dAgg):
        (v,), st = ctx.saved_tensors, ctx.st
        M, C = v.shape
        d = _rows_b16(dAgg.to(BF16)) if st.path.b16 else dAgg.float().contiguous()
        dV = None
        if ctx.needs_input_grad[1]:
            dV = torch.empty(M, C, device=v.device, dtype=v.dtype)
            _attn_gemm(st, st.PT, d, dV)
        gmap = None
        if ctx.needs_input_grad[0]:
            if st.sink and st.map is not None and st.dcat is None:      # first use to run backward: every use of the step is known
                st.dcat = torch.zeros(M, st.uses * C, device=v.device, dtype=v.dtype)
                st.vcat = torch.zeros(M, st.uses * C, device=v.device, dtype=v.dtype)
            if st.dcat is not None and (ctx.slot + 1) * C <= st.dcat.shape[1]:
                st.dcat[:, ctx.slot * C:(ctx.slot + 1) * C] = d
                st.vcat[:, ctx.slot * C:(ctx.slot + 1) * C] = v
            else:
                gmap = _outer_k1(d, v, st.B, st.N)
        return gmap, dV, None


class _AttentionMap(torch.autograd.Function):
    """GMA's attention map, content only, one head (gma_utils.py:55-78): P [B, 1, N, N] = softmax_rows(scale * q k^T) from
    ``qk`` [B*N, 2d] pixel-major (q | k: `to_qk` as a `conv_pm`, whose own node gives the weight and input gradients).
    Forward: K1 + `pfk_softmax_rows_f32`; backward: `pfk_softmax_rows_bwd_f32` into rows padded to 4 floats (zero pad columns),
    then `pfk_corr_volume_bwd_f32` per pair for dq and dk.  fp32 in either training precision."""

    @staticmethod
    def forward(ctx, qk, B: int, N: int, scale: float):
        ops = torch.ops.pfk
        d = qk.shape[1] // 2
        q, k = qk[:, :d].float().contiguous(), qk[:, d:].float().contiguous()
        attn = torch.empty(B, N, N, device=qk.device, dtype=torch.float32)
        ops.corr_volume(q.view(B, N, d), k.view(B, N, d), float(scale), attn)
        ops.softmax_rows(attn)
        ctx.scale = float(scale)
        ctx.save_for_backward(q, k, attn)
        return attn.view(B, 1, N, N)

    @staticmethod
    def backward(ctx, dP):
        ops = torch.ops.pfk
        q, k, attn = ctx.saved_tensors
        B, N, _ = attn.shape
        d = q.shape[1]
        ldc = round_up(N, 4)
        dS = torch.empty(B * N, ldc, device=q.device, dtype=torch.float32)
        ops.softmax_rows_bwd(attn.view(B * N, N), dP.float().reshape(B * N, N), dS)
        kcm = torch.zeros(B, d, round_up(ldc, 32), device=q.device, dtype=torch.float32)
        ops.pm_to_cm(k, kcm)
        dq = torch.empty(B, N, d, device=q.device, dtype=torch.float32)
        dk = torch.empty(B, ldc, round_up(d, 32), device=q.device, dtype=torch.float32)
        ops.corr_volume_bwd(dS.view(B, N, ldc), N, q.view(B, N, d), kcm, ctx.scale, dq, False, dk)
        return torch.cat([dq.view(B * N, d), dk[:, :N, :d].reshape(B * N, d)], 1), None, None, None


def attention_map_train(inp_pm: torch.Tensor, to_qk_weight: torch.Tensor, B: int, H: int, W: int, scale: float,
                        packs: Optional[ConvPacks] = None) -> torch.Tensor:
    """`Attention.forward` for one head on the kernels, differentiable: ``inp_pm`` [B*H*W, C] fp32 rows (C % 32 == 0),
    ``to_qk_weight`` [2d, C, 1, 1] -> [B, 1, N, N]."""
    if to_qk_weight.shape[0] % 64 or inp_pm.shape[1] % 32:
        raise ValueError("attention_map_train covers one head with widths that are multiples of 32")
    qk = conv_pm([inp_pm], to_qk_weight, None, B, H, W, False, None, packs)
    return _AttentionMap.apply(qk, B, H * W, scale)


# --------------------------------------------------------------------------------------------------------------------
# The update block as a differentiable composition (raft/update.py:94-153)
# --------------------------------------------------------------------------------------------------------------------
def _pm(x: torch.Tensor) -> torch.Tensor:
    B, C, H, W = x.shape
    return x.float().permute(0, 2, 3, 1).reshape(B * H * W, C)


def _nchw(x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    return x.view(B, H, W, x.shape[1]).permute(0, 3, 1, 2)


def _context_terms(P: Dict[str, torch.Tensor], spec, i: torch.Tensor, B: int, H: int, W: int, cache: dict, owner: torch.Tensor,
                   acc: bool, precision: str = "fp32"):
    """The loop-invariant part of the GRU (raft/update.py:60-71 / :27-30): the gate convolutions run over cat([h, inp, motion])
    and `inp` — the context features — is the same tensor in every iteration, so conv(W[:, inp slice], inp) is computed ONCE per
    training step (forward, data and weight gradient alike: autograd sums the twelve pre-activation gradients and runs one
    backward convolution) and the per-iteration nodes work on W without that slice.  Returns, per GRU pass,
    (wz_rest, wr_rest, wq_rest, pzr, pq); cached in `cache` for as long as `owner` (the caller's context tensor) is the same
    object at the same version — a new forward brings a new one."""
    import weakref
    ent = cache.get("ctx")
    if ent is not None and ent[0]() is owner and ent[1] == owner._version:
        return ent[2]
    Ch, Ci = spec.hidden, spec.context
    out = {}
    for kh, kw, sfx in spec.gru_passes:
        ws = [P[f"gru.conv{k}{sfx}.weight"] for k in "zrq"]
        rest = [torch.cat([w[:, :Ch], w[:, Ch + Ci:]], 1).contiguous() for w in ws]       # autograd routes the gradients back
        wc = [w[:, Ch:Ch + Ci].contiguous() for w in ws]
        wzr_c = torch.cat([wc[0], wc[1]], 0)
        # (bf16: the terms stay fp32 — they are added to the fp32 pre-activations through the epilogue's residual input)
        pzr = conv_pm([i], wzr_c, None, B, H, W, False, None, packs_for(cache, "zrc" + sfx, [wzr_c], acc), 1, precision, True)
        pq = conv_pm([i], wc[2], None, B, H, W, False, None, packs_for(cache, "qc" + sfx, [wc[2]], acc), 1, precision, True)
        out[sfx] = (rest[0], rest[1], rest[2], pzr, pq)
    cache["ctx"] = (weakref.ref(owner), owner._version, out)
    return out


def _attention_state(attention: torch.Tensor, B: int, H: int, W: int, cache: Optional[dict], acc: bool, precision: str) -> AttnState:
    """The packed attention map of this step: built once and kept in `cache` for as long as `attention` is the same object at
    the same version (`_context_terms`' rule).  A step-scoped cache (`acc`) also gets the step sink for the map's gradient.
    A cache that outlives the step (the seam's) must not pin a step's N x N buffers: without a sink the state holds no reference to
    the map, the entry goes when the caller's tensor dies, and a stale entry is dropped BEFORE the new pack allocates.  (The
    autograd nodes of a step still hold their state until that step's graph is freed.)"""
    import weakref
    if cache is None:
        return pack_attention(attention, B, H, W, precision, sink=False)
    ent = cache.get("attn")
    if ent is not None and ent[0]() is attention and ent[1] == attention._version and ent[2] == precision:
        return ent[3]
    cache.pop("attn", None)
    del ent

    def gone(ref, cache=cache):
        if cache.get("attn", (None,))[0] is ref:
            del cache["attn"]

    st = pack_attention(attention, B, H, W, precision, sink=acc)
    cache["attn"] = (weakref.ref(attention, gone), attention._version, precision, st)
    return st


def update_block_train_pm(P: Dict[str, torch.Tensor], spec, h, i, c, f, B: int, H: int, W: int, cache: Optional[dict] = None,
                          accumulate_wgrad: bool = False, attention: Optional[torch.Tensor] = None, hoist_context: bool = True,
                          context_owner: Optional[torch.Tensor] = None, precision: str = "fp32", aggregator=None,
                          global_context: Optional[torch.Tensor] = None):
    """BasicUpdateBlock.forward / SmallUpdateBlock.forward (update.py:144-153 / :122-128) with every convolution on
    ``conv_pm``, on pixel-major tensors: ``h`` [M, Ch], ``i`` [M, Ci], ``c`` [M, corr channels], ``f`` [M, 2] ->
    ``(h', mask [M, 576] | None, delta [M, 2])``.  ``P``: the block's named parameters; ``cache``: a dict that keeps the packed
    weights between the recurrent calls of one training step.  ``accumulate_wgrad`` (only with a ``cache`` that is created per
    step): the recurrent calls add their weight gradients into one buffer per parameter (`ConvPacks.acc`, `_Flush`).
    ``precision="bf16"``: the convolutions on the bf16 matrix cores (module docstring); inputs and outputs stay fp32 rows.
    ``attention`` (GMA, `spec.aggregate`): the map [B, 1, N, N] of this forward, fp32; its gradient flows back to it.
    ``aggregator`` / ``global_context`` (CCMR, `spec.external_aggregate`, ccmr/update.py:152-163): the caller's module of this scale
    and its first argument.  It stays torch autograd: it runs on the NCHW view of the motion features and its result fills the
    second motion slot of the GRU input, where GMA's branch puts `mf + gamma * attn @ v`.  The mask is [M, `spec.mask_channels`]."""
    acc = accumulate_wgrad and cache is not None
    k = _KERNELS[check_precision(precision)]
    b16 = k.dtype == BF16
    if spec.external_aggregate and aggregator is None:
        raise ValueError("update_block_train_pm: a block with an external aggregate slot needs the scale's aggregator module")
    if spec.aggregate and not spec.external_aggregate and attention is None:
        raise ValueError("update_block_train_pm: a block with GMA's aggregate branch needs the attention map [B, 1, N, N]")

    def conv(srcs, name, relu=False, real=None, prec=precision, out_fp32=False):
        w = P[name + ".weight"]
        return conv_pm(srcs, w, P.get(name + ".bias"), B, H, W, relu, real, packs_for(cache, name, [w], acc), 1, prec, out_fp32)

    # motion encoder (update.py:104-112 / :85-91)
    cor = conv([k.pad(c)], "encoder.convc1", True, [c.shape[1]])
    if spec.c2:
        cor = conv([cor], "encoder.convc2", True)
    flo = conv([_KERNELS["fp32"].pad(f)], "encoder.convf1", True, [2], "fp32")      # 7x7: outside pfk_conv2d_b16's 32 taps, fp32 in either mode
    flo = conv([flo], "encoder.convf2", True)
    out = conv([cor, flo], "encoder.conv", True)
    # x = [inp | motion features (encoder out | flow) | zero pad to a multiple of 4] in ONE concatenation (update.py:112 + :146);
    # with the context term hoisted (`_context_terms`, needs a cache to live in) `inp` stays out of it
    # (step-scoped caches only — `accumulate_wgrad`, the mirror's training forward: a cache that outlives the step would hand the
    #  next forward derived tensors whose autograd graph the previous backward has already freed)
    hoist = hoist_context and acc
    ctx_terms = (_context_terms(P, spec, i, B, H, W, cache, i if context_owner is None else context_owner, acc, precision)
                 if hoist else None)
    x_real = spec.x_channels - (spec.context if hoist else 0)
    parts = [out, f] if hoist else [i, out, f]
    if spec.external_aggregate:
        mf = torch.cat([out.float(), f], 1)
        mfg = _pm(aggregator(global_context, _nchw(mf, B, H, W)))
        parts = [mf, mfg] if hoist else [i, mf, mfg]
    elif spec.aggregate:
        mf = torch.cat([out, f], 1)
        v = conv([mf], "aggregator.to_v")                                        # 1x1, no bias
        att = _attention_state(attention, B, H, W, cache, acc, precision)       # packed once per step (P and P^T, fp32 or bf16)
        agg = _AttnMatmul.apply(att.target(attention), v, att)                                 # fp32 rows in either precision
        parts = [mf, mf + P["aggregator.gamma"] * agg] if hoist else [i, mf, mf + P["aggregator.gamma"] * agg]
    if x_real % k.quantum:
        zkey = ("zpad", i.shape[0], round_up(x_real, k.quantum) - x_real, i.device)
        z = cache.get(zkey) if cache is not None else None
        if z is None:
            z = torch.zeros(i.shape[0], round_up(x_real, k.quantum) - x_real, device=i.device, dtype=torch.float32)
            if cache is not None:
                cache[zkey] = z
        parts.append(z)
    x = torch.cat([t.to(k.dtype) for t in parts], 1)
    # GRU passes (update.py:58-73 / :24-32): one fused autograd node per pass (z and r share a convolution)
    for kh, kw, sfx in spec.gru_passes:
        names = [f"gru.conv{k}{sfx}" for k in "zrq"]
        wz, wr, wq = (P[n + ".weight"] for n in names)
        bz, br, bq = (P[n + ".bias"] for n in names)
        pzr = pq = None
        if hoist:
            wz, wr, wq, pzr, pq = ctx_terms[sfx]      # the weights without their context slice; that slice's products, once per step
        pk_zr = packs_for(cache, "zr" + sfx, [wz, wr, bz, br], acc)      # the cached z|r concatenation includes the biases
        pk_q = packs_for(cache, "q" + sfx, [wq], acc)
        wz, wr, bz, br = step_params(pk_zr, wz, wr, bz, br)
        wq, bq = step_params(pk_q, wq, bq)
        h = _GruPass.apply(h, x, wz, wr, wq, bz, br, bq, _Geometry(B, H, W, kh, kw), x_real, pk_zr, pk_q, pzr, pq, precision)
    # heads (update.py:6-14, 138-142, 152); bf16: the last layers hand their fp32 accumulators on (flow and mask stay fp32)
    delta = conv([conv([h], "flow_head.conv1", True)], "flow_head.conv2", out_fp32=b16)
    mask = None
    if spec.has_mask:
        mask = 0.25 * conv([conv([h], "mask.0", True)], "mask.2", out_fp32=b16)
    return h, mask, delta


def update_block_train(P: Dict[str, torch.Tensor], spec, net, inp, corr, flow, cache: Optional[dict] = None,
                       precision: str = "fp32", attention: Optional[torch.Tensor] = None, aggregator=None,
                       global_context: Optional[torch.Tensor] = None):
    """NCHW face of `update_block_train_pm` (what `PfkUpdateBlock` calls from the reference's loop):
    NCHW in, NCHW out: ``(net, mask | None, delta_flow)``; ``attention``: GMA's map [B, 1, N, N]; ``aggregator`` /
    ``global_context``: CCMR's module of this scale and its first argument."""
    B, _, H, W = net.shape
    h, mask, delta = update_block_train_pm(P, spec, _pm(net), _pm(inp), _pm(corr), _pm(flow), B, H, W, cache, context_owner=inp,
                                           precision=precision, attention=attention, aggregator=aggregator,
                                           global_context=global_context)
    return _nchw(h, B, H, W), (None if mask is None else _nchw(mask, B, H, W)), _nchw(delta, B, H, W)


# --------------------------------------------------------------------------------------------------------------------
# Convex upsampling (raft/raft.py:112-123) and the sequence loss (raft/raft.py:20-45) for the training step
# --------------------------------------------------------------------------------------------------------------------
class _ConvexUpsample(torch.autograd.Function):
    """flow [B,2,H,W] (NCHW), mask pixel-major [B*H*W, 576] (already x0.25) -> [B,2,8H,8W]; forward and both gradients on
    libpfk (`pfk_convex_upsample_f32`, `pfk_convex_upsample_bwd_f32`)."""

    @staticmethod
    def forward(ctx, flow, mask):
        flow = flow.float().contiguous()
        mask = mask.float()
        if mask.stride(1) != 1:
            mask = mask.contiguous()
        B, _, H, W = flow.shape
        out = torch.empty(B, 2, 8 * H, 8 * W, device=flow.device, dtype=torch.float32)
        torch.ops.pfk.convex_upsample(flow, mask, out)
        ctx.save_for_backward(flow, mask)
        return out

    @staticmethod
    def backward(ctx, g):
        flow, mask = ctx.saved_tensors
        gmask = torch.empty(mask.shape[0], 576, device=mask.device, dtype=torch.float32)
        gflow = torch.empty_like(flow)
        torch.ops.pfk.convex_upsample_bwd(flow, mask, g.float().contiguous(), gmask, gflow)
        return gflow, gmask


def convex_upsample(flow: torch.Tensor, mask_pm: torch.Tensor) -> torch.Tensor:
    load_native()
    return _ConvexUpsample.apply(flow, mask_pm)


class _ConvexUpsample2(torch.autograd.Function):
    """`upsample_flow(flow, mask, scale=2)` of the multi-scale loops (ccmr/ccmr.py:128-139, ms_raft_plus/ms_raft_plus.py:133-144):
    flow [B,2,H,W] (NCHW), mask pixel-major [B*H*W, 36] (already x0.25; any row stride) -> [B,2,2H,2W]; forward and both gradients
    on libpfk (`pfk_convex_upsample2_f32`, `pfk_convex_upsample2_bwd_f32`)."""

    @staticmethod
    def forward(ctx, flow, mask):
        flow = flow.float().contiguous()
        mask = mask.float()
        if mask.stride(1) != 1:
            mask = mask.contiguous()
        B, _, H, W = flow.shape
        out = torch.empty(B, 2, 2 * H, 2 * W, device=flow.device, dtype=torch.float32)
        torch.ops.pfk.convex_upsample2(flow, mask, out)
        ctx.save_for_backward(flow, mask)
        return out

    @staticmethod
    def backward(ctx, g):
        flow, mask = ctx.saved_tensors
        gmask = torch.empty(mask.shape[0], 36, device=mask.device, dtype=torch.float32)
        gflow = torch.empty_like(flow)
        torch.ops.pfk.convex_upsample2_bwd(flow, mask, g.float().contiguous(), gmask, gflow)
        return gflow, gmask


def convex_upsample2(flow: torch.Tensor, mask_pm: torch.Tensor) -> torch.Tensor:
    load_native()
    return _ConvexUpsample2.apply(flow, mask_pm)


def sequence_loss(flow_preds: Sequence[torch.Tensor], flow_gt: torch.Tensor, valid: torch.Tensor, gamma: float = 0.8,
                  max_flow: float = 400.0) -> torch.Tensor:
    """SequenceLoss.forward (raft/raft.py:31-45): gamma-weighted L1 over the prediction sequence; pixels that are invalid
    or whose ground-truth displacement is >= max_flow are excluded by zeroing (the mean still runs over all pixels, as in
    the reference).  ``flow_gt`` [B,2,H,W], ``valid`` [B,1,H,W]."""
    n = len(flow_preds)
    mag = torch.sum(flow_gt ** 2, dim=1, keepdim=True).sqrt()
    keep = (valid >= 0.5) & (mag < max_flow)
    loss = 0.0
    for k, pred in enumerate(flow_preds):
        loss = loss + gamma ** (n - k - 1) * (keep * (pred - flow_gt).abs()).mean()
    return loss
