"""CCMR's motion aggregator — ``XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=True)``, one per scale
(ptlflow/models/ccmr/xcit.py, ccmr/update.py:132-163) — on pixel-major fp32 rows: eval only, fp32 only, opt-in with
``accelerate(model, ccmr_aggregator=True)``.

The block computes, on tokens x0 = rows(global_context) + pos and v = rows(motion_features):

    x1  = x0 + gamma1 * proj(A @ to_v(LN1(v)))          A = the 8 x (16 x 16) cross-covariance map of to_qk(LN1(x0))
    x2  = x1 + gamma3 * conv2(GN(GELU(conv1(LN3(x1)))))  two depthwise 3x3 convolutions around a GroupNorm(8)
    out = x2 + gamma2 * fc2(GELU(fc1(LN2(x2))))

x0 and A depend on `global_context` only, which is one tensor for all iterations of a scale (ccmr.py:191-208), and everything
between LN1(v) and `proj` is linear: the attention branch is ONE 128 -> 128 GEMM per image, x1 = x0 + xh M_b^T + c_b with
xh = LayerNorm(v) without affine and (`fold_attention`)

    M_b = diag(gamma1) W_proj blockdiag(A_b) W_v diag(ln1.weight),   c_b = gamma1 * (W_proj blockdiag(A_b) (W_v ln1.bias + b_v) + b_proj).

`XcitAggregatorEngine.prepare` does the per-scale part once (x0, qk, `pfk_xca_map_f32`, the fold); `run` is then, per iteration,

    xh  = LayerNorm(mf)                         pfk_layernorm_rows_f32
    x1  = x0 + xh M_b^T + c_b                   pfk_conv2d_group_f32, one problem per image, residual x0
    u   = GELU(dw3x3(LN3(x1)) + b1)             pfk_xcit_lpi1_f32 (+ GroupNorm partial sums)
    x2, t = ..., LN2(x2)                        pfk_xcit_lpi2_f32 (two launches: the statistics finished first)
    g   = GELU(fc1(t))                          pfk_conv2d_f32, PFK_EPI_LINEAR_GELU
    out = x2 + (gamma2 fc2)(g)                  pfk_conv2d_f32, residual x2, straight into the update engine's aggregate slot

reading the update engine's `motion_view` and writing its `aggregate_view`: no NCHW round trip, no torch op per iteration.

CCMR's per-scale context grouping ``model.xcit[i](inp)`` (ccmr/ccmr.py:191) is the same block with ``separate=False``: one input,
q | k | v = qkv(LN1(x0)).  The fold applies unchanged with W_qk = qkv.weight[:256] and W_v = qkv.weight[256:] (`split_qkv`), and xh is
LayerNorm(x0) itself; `XcitContextEngine` (opt-in with ``accelerate(model, ccmr_context=True)``) runs it once per scale
with `pfk_xcit_tokens_f32` in front, `pfk_xca_fold_f32` for the fold and the same tail, behind the drop-in `PfkXcitContext`.
"""
from __future__ import annotations

import copy
from typing import Dict, Optional, Tuple

import torch

from . import load_native
from ._seam import WrappedModule, eligible, pixel_rows
from .conv_path import EPI_LINEAR, EPI_LINEAR_GELU

DIM, HEADS, HEAD_DIM, GROUPS = 128, 8, 16, 8
LN_EPS, GN_EPS = 1e-6, 1e-5
POS_HIDDEN = 32

# (module of the class, class name) of the aggregators `PfkUpdateBlock` may serve; extendable with `register_xcit_aggregator`
_XCIT_CLASSES = {("ptlflow.models.ccmr.xcit", "XCiT")}


def register_xcit_aggregator(module: str, cls: str = "XCiT") -> None:
    """Serve the class `cls` of `module` as well (it must still pass `match_xcit_aggregator`)."""
    _XCIT_CLASSES.add((module, cls))


def served(module: torch.nn.Module) -> bool:
    return (type(module).__module__, type(module).__name__) in _XCIT_CLASSES


# (module of the class, class name) of the context grouping modules `model.xcit[i]` that `PfkXcitContext` may serve;
# extendable with `register_xcit_context`
_CONTEXT_CLASSES = {("ptlflow.models.ccmr.xcit", "XCiT")}


def register_xcit_context(module: str, cls: str = "XCiT") -> None:
    """Serve the class `cls` of `module` as a context grouping module as well (it must still pass `match_xcit_context`)."""
    _CONTEXT_CLASSES.add((module, cls))


def served_context(module: torch.nn.Module) -> bool:
    return (type(module).__module__, type(module).__name__) in _CONTEXT_CLASSES


def xcit_shapes(separate: bool = True) -> Dict[str, tuple]:
    """state_dict names / shapes of XCiT(128, depth 1, 8 heads, mlp_ratio 1, qkv_bias, separate) (xcit.py:242-373): `separate` has
    `attn.to_qk` and `attn.to_v`, the one-input form `attn.qkv` (384 x 128 with bias)"""
    sh: Dict[str, tuple] = {}

    def vec(name, c=DIM):
        sh[name + ".weight"] = (c,)
        sh[name + ".bias"] = (c,)

    def lin(name, co, ci=DIM):
        sh[name + ".weight"] = (co, ci)
        sh[name + ".bias"] = (co,)

    b = "blocks.0."
    for n in ("norm1", "norm2", "norm3", "local_mp.bn"):
        vec(b + n)
    sh[b + "attn.temperature"] = (HEADS, 1, 1)
    if separate:
        lin(b + "attn.to_qk", 2 * DIM)
        lin(b + "attn.to_v", DIM)
    else:
        lin(b + "attn.qkv", 3 * DIM)
    lin(b + "attn.proj", DIM)
    lin(b + "mlp.fc1", DIM)
    lin(b + "mlp.fc2", DIM)
    for n in ("conv1", "conv2"):
        sh[b + f"local_mp.{n}.weight"] = (DIM, 1, 3, 3)
        sh[b + f"local_mp.{n}.bias"] = (DIM,)
    for n in ("gamma1", "gamma2", "gamma3"):
        sh[b + n] = (DIM,)
    sh["pos_embeder.token_projection.weight"] = (DIM, 2 * POS_HIDDEN, 1, 1)
    sh["pos_embeder.token_projection.bias"] = (DIM,)
    return sh


def match_xcit_aggregator(module: torch.nn.Module) -> bool:
    """`module` computes exactly what the engine implements: the state_dict of `xcit_shapes` in fp32, `separate`, one block, 8 heads
    (temperature (8, 1, 1)), LayerNorms with eps 1e-6, GroupNorm(8, 128), depthwise 3x3 convolutions, exact GELUs.  The class is the
    caller's to check (`served`)."""
    return _match_xcit(module, True)


def match_xcit_context(module: torch.nn.Module) -> bool:
    """The same for the one-input form `XcitContextEngine` implements: not `separate` (`attn.qkv` 384 x 128 with bias, no `to_qk` /
    `to_v`), everything else as `match_xcit_aggregator`.  The class is the caller's to check (`served_context`)."""
    return _match_xcit(module, False)


def _match_xcit(module: torch.nn.Module, separate: bool) -> bool:
    sd = module.state_dict()
    if {k: tuple(v.shape) for k, v in sd.items()} != xcit_shapes(separate):
        return False
    if any(v.dtype != torch.float32 for v in sd.values()):
        return False
    blocks = getattr(module, "blocks", None)
    says = lambda m: hasattr(m, "separate") and bool(m.separate) is separate  # noqa: E731
    if not says(module) or blocks is None or len(blocks) != 1 or not hasattr(module, "use_pos"):
        return False
    blk = blocks[0]
    if not says(blk) or getattr(blk.attn, "num_heads", None) != HEADS:
        return False
    for n in ("norm1", "norm2", "norm3"):
        ln = getattr(blk, n)
        if type(ln) is not torch.nn.LayerNorm or tuple(ln.normalized_shape) != (DIM,) or ln.eps != LN_EPS:
            return False
    lpi = blk.local_mp
    gn = lpi.bn
    if type(gn) is not torch.nn.GroupNorm or gn.num_groups != GROUPS or gn.num_channels != DIM or gn.eps != GN_EPS:
        return False
    for conv in (lpi.conv1, lpi.conv2):
        if type(conv) is not torch.nn.Conv2d or conv.groups != DIM or conv.stride != (1, 1) or conv.padding != (1, 1) \
                or conv.dilation != (1, 1) or conv.padding_mode != "zeros":
            return False
    for act in (lpi.act, blk.mlp.act):
        if type(act) is not torch.nn.GELU or getattr(act, "approximate", "none") != "none":
            return False
    pe = module.pos_embeder
    return getattr(pe, "hidden_dim", None) == POS_HIDDEN and callable(pe)


def fold_attention(A: torch.Tensor, P: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The attention branch of the block as one affine map per image (module docstring): `A` [B, 8, 16, 16], `P` the block's
    parameters under their state_dict names without the ``blocks.0.`` prefix (`norm1.weight`, `attn.to_v.weight`, `gamma1`, ...).
    Returns M [B, 128, 128] and c [B, 128] with  gamma1 * attn(x_qk, x_v) = LayerNorm(x_v, no affine) @ M_b^T + c_b,  in `A`'s dtype
    on `A`'s device (CPU tensors included)."""
    p = {k: P[k].detach().to(device=A.device, dtype=A.dtype) for k in
         ("norm1.weight", "norm1.bias", "attn.to_v.weight", "attn.to_v.bias", "attn.proj.weight", "attn.proj.bias", "gamma1")}
    B = A.shape[0]
    # blockdiag(A_b) @ X for X [128, n]: head h mixes its own 16 rows
    def mix(X):
        return torch.matmul(A, X.reshape(-1, HEADS, HEAD_DIM, X.shape[-1])).reshape(B, DIM, X.shape[-1])
    wv = p["attn.to_v.weight"] * p["norm1.weight"][None, :]                     # W_v diag(ln1.weight)
    bv = (p["attn.to_v.weight"] @ p["norm1.bias"] + p["attn.to_v.bias"])[:, None]  # W_v ln1.bias + b_v
    wp = p["gamma1"][:, None] * p["attn.proj.weight"]                            # diag(gamma1) W_proj
    M = torch.matmul(wp, mix(wv[None]))
    c = torch.matmul(wp, mix(bv[None]))[:, :, 0] + p["gamma1"] * p["attn.proj.bias"]
    return M.contiguous(), c.contiguous()


def split_qkv(P: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The parameters of a one-input block (`attn.qkv`, rows q | k | v, row head * 16 + d within each: xcit.py:167-170) under the names
    of the `separate` form, so that `fold_attention` and the aggregator's algebra read them: `attn.to_qk` = rows [0, 256), `attn.to_v`
    = rows [256, 384).  The other entries are passed through."""
    out = {k: v for k, v in P.items() if not k.startswith("attn.qkv.")}
    out["attn.to_qk.weight"], out["attn.to_v.weight"] = P["attn.qkv.weight"][:2 * DIM], P["attn.qkv.weight"][2 * DIM:]
    out["attn.to_qk.bias"], out["attn.to_v.bias"] = P["attn.qkv.bias"][:2 * DIM], P["attn.qkv.bias"][2 * DIM:]
    return out


class _XcitEngine:
    """What the two engines share: the packed weights of the block's tail, the work buffers of the bound (B, H, W), the module's
    positional encoding, the attention branch as one GEMM per image and the launches behind it."""

    def __init__(self, module: torch.nn.Module, device: torch.device):
        load_native()
        self.ops = torch.ops.pfk
        self.module = module
        self.device = device
        self._shape: Optional[Tuple[int, int, int]] = None
        self.pack()

    # ------------------------------------------------------------------ weights
    def _pack_common(self, qk_w: str, qk_b: str) -> Dict[str, torch.Tensor]:
        blk = self.module.blocks[0]
        P = {k: v.detach().to(device=self.device, dtype=torch.float32).contiguous() for k, v in blk.state_dict().items()}
        self.P = P
        w: Dict[str, torch.Tensor] = {}
        # 1x1 "convolutions" over 128 channels: the packed weight [cout][ktot = 128] is the Linear weight itself
        w["qk.w"], w["qk.b"] = P[qk_w], P[qk_b]
        w["fc1.w"], w["fc1.b"] = P["mlp.fc1.weight"], P["mlp.fc1.bias"]
        w["fc2.w"] = (P["gamma2"][:, None] * P["mlp.fc2.weight"]).contiguous()      # gamma2 folded into fc2
        w["fc2.b"] = (P["gamma2"] * P["mlp.fc2.bias"]).contiguous()
        for i in ("1", "2"):
            w[f"dw{i}.w"] = P[f"local_mp.conv{i}.weight"].reshape(DIM, 9).contiguous()
            w[f"dw{i}.b"] = P[f"local_mp.conv{i}.bias"]
        w["temperature"] = P["attn.temperature"].reshape(HEADS).contiguous()
        self.w = w
        self._pos_module = copy.deepcopy(self.module.pos_embeder).to(device="cpu", dtype=torch.float32)
        self._pos: Dict[tuple, torch.Tensor] = {}
        return w

    # ------------------------------------------------------------------ buffers
    def _bind_common(self, B: int, H: int, W: int) -> bool:
        """the buffers of (B, H, W); False when they are bound already"""
        if self._shape == (B, H, W):
            return False
        M = B * H * W
        z = lambda c: torch.zeros(M, c, device=self.device, dtype=torch.float32)  # noqa: E731
        self.x0, self.xh, self.x1, self.u, self.x2, self.t, self.g = (z(DIM) for _ in range(7))
        self.qk = z(2 * DIM)
        self.A = torch.zeros(B, HEADS, HEAD_DIM, HEAD_DIM, device=self.device, dtype=torch.float32)
        self.lpi_ws = torch.zeros(self.ops.xcit_lpi_workspace_bytes(B, H, W), device=self.device, dtype=torch.uint8)
        self.workspace = torch.zeros(self.ops.conv_workspace_bytes(), device=self.device, dtype=torch.uint8)      # stream-K scratch
        self._shape = (B, H, W)
        return True

    def _pos_rows(self, B: int, H: int, W: int) -> torch.Tensor:
        """the module's own positional encoding as rows [B*H*W, 128]: a function of the shape (and of parameters: `pack` drops it)"""
        pos = self._pos.get((B, H, W))
        if pos is None:
            # on a CPU copy of the module's encoder: torch's first GPU convolution of a shape in a process may take another algorithm
            # than its later ones (2e-7 apart, measured), and the engine's results must not depend on what ran before it
            with torch.no_grad():
                pos = self._pos_module(B, H, W, torch.float32)
            pos = pos.permute(0, 2, 3, 1).reshape(B * H * W, DIM).contiguous().to(self.device)
            self._pos[(B, H, W)] = pos
        return pos

    def _linear(self, src, key: str, cout: int, out, epi=EPI_LINEAR, residual=None) -> None:
        B, H, W = self._shape
        self.ops.conv2d([src], B, H, W, 1, 1, self.w[key + ".w"], self.w[key + ".b"], cout, epi, False, 1.0, out, None, None, None,
                        self.workspace, residual, 1, False, 0, 0)

    # ------------------------------------------------------------------ launches
    def _attention_branch(self) -> None:
        """x1 = x0 + xh M_b^T + c_b: the images' GEMMs are independent, up to four problems per grouped launch"""
        B, H, W = self._shape
        N = H * W
        for b0 in range(0, B, 4):
            rows = [slice(b * N, (b + 1) * N) for b in range(b0, min(B, b0 + 4))]
            n = len(rows)
            self.ops.conv2d_group([self.xh[r] for r in rows], 1, H, W, [1] * n, [self.M[b0 + i] for i in range(n)],
                                  [self.c[b0 + i] for i in range(n)], [0] * n, [1.0] * n, [self.x1[r] for r in rows],
                                  [self.x0[r] for r in rows])

    def _tail(self, out: torch.Tensor) -> None:
        """everything behind x1: the local patch interaction (x2, t = LN2(x2)) and the MLP with its residual into the rows `out`"""
        B, H, W = self._shape
        ops, P, w = self.ops, self.P, self.w
        ops.xcit_lpi1(self.x1, P["norm3.weight"], P["norm3.bias"], LN_EPS, w["dw1.w"], w["dw1.b"], self.u, self.lpi_ws, B, H, W)
        ops.xcit_lpi2(self.u, P["local_mp.bn.weight"], P["local_mp.bn.bias"], GN_EPS, GROUPS, w["dw2.w"], w["dw2.b"], P["gamma3"],
                      self.x1, self.x2, P["norm2.weight"], P["norm2.bias"], LN_EPS, self.t, self.lpi_ws, B, H, W)
        self._linear(self.t, "fc1", DIM, self.g, epi=EPI_LINEAR_GELU)
        self._linear(self.g, "fc2", DIM, out, residual=self.x2)


class XcitAggregatorEngine(_XcitEngine):
    """One matched aggregator on the kernels: its packed weights, the work buffers of the bound (B, H, W), the per-scale cache
    (x0, the folded attention branch; keyed by the `global_context` object and its `_version`) and the launches."""

    def __init__(self, module: torch.nn.Module, device: torch.device):
        self.prepared = 0          # per-scale preparations so far (tests: the cached map is reused)
        super().__init__(module, device)

    def pack(self) -> None:
        self._pack_common("attn.to_qk.weight", "attn.to_qk.bias")
        self._gc_ref, self._gc_version = None, -1

    def bind(self, B: int, H: int, W: int) -> None:
        if self._bind_common(B, H, W):
            self._gc_ref, self._gc_version = None, -1

    # ------------------------------------------------------------------ once per (forward, scale)
    def prepare(self, global_context: torch.Tensor) -> None:
        """x0 = rows(global_context) [+ pos], the attention map of to_qk(LN1(x0)) and the folded branch (M, c)"""
        B, H, W = self._shape
        ops, P = self.ops, self.P
        gc = global_context
        if gc.is_contiguous():
            ops.nchw_to_pm(gc, self.x0)
        else:
            self.x0.view(B, H, W, DIM).copy_(gc.permute(0, 2, 3, 1))
        if self.module.use_pos:
            self.x0 += self._pos_rows(B, H, W)
        ops.layernorm_rows(self.x0, P["norm1.weight"], P["norm1.bias"], LN_EPS, self.t)
        self._linear(self.t, "qk", 2 * DIM, self.qk)
        ops.xca_map(self.qk, self.w["temperature"], self.A, B, H * W)
        self.M, self.c = fold_attention(self.A, P)
        self.prepared += 1

    # ------------------------------------------------------------------ one call
    def run(self, global_context: torch.Tensor, motion: torch.Tensor, out: torch.Tensor, B: int, H: int, W: int,
            refresh: bool = False) -> None:
        """aggregator(global_context, motion_features) on rows: `motion` [B*H*W, 128] view in, `out` [B*H*W, 128] view out.
        `refresh`: the caller knows a new forward began (the per-scale cache is rebuilt whatever the tensor's identity says)."""
        self.bind(B, H, W)
        gc = global_context
        if refresh or gc is not self._gc_ref or gc._version != self._gc_version:
            self.prepare(gc)
            self._gc_ref, self._gc_version = gc, gc._version      # a strong reference: the address cannot be recycled while cached
        self.ops.layernorm_rows(motion, None, None, LN_EPS, self.xh)
        self._attention_branch()
        self._tail(out)


class XcitContextEngine(_XcitEngine):
    """One matched context grouping module (`model.xcit[i]`: the block with one input) on the kernels.  `engine(inp)`
    maps ``inp`` [B, 128, H, W] fp32 — NCHW-contiguous, or dense channels-last as the multi-scale encoder engine hands it out — to a
    fresh contiguous [B, 128, H, W]:

        x0, xh = rows(inp) + pos, LayerNorm(x0)     pfk_xcit_tokens_f32 (pfk_xcit_tokens_pm_f32 for channels-last input)
        qk  = xh (W_qk diag(ln1.w))^T + ...         pfk_conv2d_f32: LN1's affine folded into the packed weight
        A   = the 8 x (16 x 16) map                 pfk_xca_map_f32
        M, c                                        pfk_xca_fold_f32
        x1  = x0 + xh M_b^T + c_b                   pfk_conv2d_group_f32
        ... the aggregator's tail (`_tail`) ...     into rows, then pfk_pm_to_nchw_f32
    """

    def pack(self) -> None:
        w = self._pack_common("attn.qkv.weight", "attn.qkv.bias")
        P = self.P
        ln_w, ln_b = P["norm1.weight"], P["norm1.bias"]
        w_qk, w_v = P["attn.qkv.weight"][:2 * DIM], P["attn.qkv.weight"][2 * DIM:]
        b_qk, b_v = P["attn.qkv.bias"][:2 * DIM], P["attn.qkv.bias"][2 * DIM:]
        # LN1's affine folded into both consumers of the normalised rows: one un-affine xh feeds the qk GEMM and the folded branch
        w["qk.w"] = (w_qk * ln_w[None, :]).contiguous()
        w["qk.b"] = (w_qk @ ln_b + b_qk).contiguous()
        w["v.w"] = (w_v * ln_w[None, :]).contiguous()
        w["v.b"] = (w_v @ ln_b + b_v).contiguous()
        w["proj.w"] = (P["gamma1"][:, None] * P["attn.proj.weight"]).contiguous()
        w["proj.b"] = (P["gamma1"] * P["attn.proj.bias"]).contiguous()

    def bind(self, B: int, H: int, W: int) -> None:
        if self._bind_common(B, H, W):
            self.M = torch.zeros(B, DIM, DIM, device=self.device, dtype=torch.float32)
            self.c = torch.zeros(B, DIM, device=self.device, dtype=torch.float32)
            self.o = torch.zeros(B * H * W, DIM, device=self.device, dtype=torch.float32)

    def pos_rows(self, H: int, W: int) -> torch.Tensor:
        """one image's rows [H*W, 128] of the positional encoding: the mask is all zeros, so every image of a batch gets the same"""
        return self._pos_rows(1, H, W)

    @torch.no_grad()
    def __call__(self, inp: torch.Tensor) -> torch.Tensor:
        B, C, H, W = inp.shape
        if C != DIM or inp.dtype != torch.float32 or not inp.is_cuda:
            raise ValueError(f"{type(self).__name__}: expected a CUDA fp32 [B, {DIM}, H, W] tensor, got {tuple(inp.shape)} {inp.dtype}")
        self.bind(B, H, W)
        ops, w = self.ops, self.w
        pos = self.pos_rows(H, W) if self.module.use_pos else None
        if inp.is_contiguous():
            ops.xcit_tokens(inp, pos, LN_EPS, self.x0, self.xh)
        else:
            rows = pixel_rows(inp, torch.float32, align=4)
            if rows is None:
                raise ValueError(f"{type(self).__name__}: the input is neither NCHW-contiguous nor channels-last rows")
            ops.xcit_tokens_pm(rows, pos, LN_EPS, self.x0, self.xh, B, H, W)
        self._linear(self.xh, "qk", 2 * DIM, self.qk)
        ops.xca_map(self.qk, w["temperature"], self.A, B, H * W)
        ops.xca_fold(self.A, w["v.w"], w["v.b"], w["proj.w"], w["proj.b"], self.M, self.c)
        self._attention_branch()
        self._tail(self.o)
        out = torch.empty(B, DIM, H, W, device=self.device, dtype=torch.float32)
        ops.pm_to_nchw(self.o, out)
        return out


def servable_layout(inp: torch.Tensor) -> bool:
    """`XcitContextEngine` reads `inp` without a copy: NCHW-contiguous, or pixel-major rows (channels-last strides, 16-byte aligned)"""
    return inp.is_contiguous() or pixel_rows(inp, torch.float32, align=4) is not None


class PfkXcitContext(WrappedModule):
    """Drop-in for ``model.xcit[i]`` of a live CCMR / CCMR+ model (``accelerate(model, ccmr_context=True)``): the reference's
    ``forward(x)`` contract and the same parameters — the reference sub-modules are re-registered under their own names, so state_dict
    keys are unchanged.  An eval-mode call ``module(x)`` outside grad mode and autocast on an fp32 GPU tensor [B, 128, H, W] in a layout
    the engine reads (`servable_layout`) with fp32 parameters goes to `XcitContextEngine` (``engine_calls``); every other call runs the
    reference module (``fallback_calls``)."""

    def __init__(self, ref: torch.nn.Module):
        super().__init__(ref)
        self.engine_calls = 0
        self.fallback_calls = 0

    def _get_engine(self, device) -> XcitContextEngine:
        ref = self._ref[0]
        return self._engine_for(device, list(ref.parameters()), lambda: XcitContextEngine(ref, device), lambda e: e.pack())

    def forward(self, *args, **kwargs):
        ref = self._ref[0]
        ref.training = self.training   # .train() / .eval() reach this wrapper and the shared children, not `ref` itself
        x = args[0] if len(args) == 1 and not kwargs else None
        params = list(ref.parameters())
        if (x is None or self.training or not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != DIM or x.numel() == 0
                or not eligible((x,), params, dtypes=(torch.float32,), autocast=False)
                or any(p.dtype != torch.float32 or p.device != x.device for p in params) or not servable_layout(x)):
            self.fallback_calls += 1
            return ref(*args, **kwargs)
        self.engine_calls += 1
        return self._get_engine(x.device)(x)


