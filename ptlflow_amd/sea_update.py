"""SEA-RAFT's refinement loop on gfx950 kernels: the update block (ptlflow/models/sea_raft/update.py:18-54, the ConvNeXt blocks of
layer.py:44-83), the flow / upsample-weight heads (sea_raft.py:114-126) and `upsample_data` (sea_raft.py:147-163).

`SeaUpdateEngine` is an `UpdateEngine` without GRU passes.  Its `hx` buffer is RAFT's `[h (128) | inp (128) | motion (126) | flow (2)]`
and that is exactly the ConvNeXt block input `cat([net, cat([context, motion_features])])` (update.py:50-53): 384 channels.  Per
iteration, after the caller's lookup:

    motion encoder                       UpdateEngine.motion / motion_grouped    -> hx[:, 256:382]
    per ConvNeXt block i (2):
      dwconv 7x7 + LayerNorm             pfk_dwconv_layernorm_f32  (hx)          -> ln   [M, 384]
      pwconv1 + GELU                     pfk_conv2d_f32, PFK_EPI_LINEAR_GELU     -> mid  [M, 512]
      gamma * pwconv2 + input            pfk_conv2d_f32, LINEAR + residual hx    -> res  [M, 384]   (gamma folded into W2, b2)
      final 1x1 384 -> 128               pfk_conv2d_f32                          -> hx[:, :128]
    flow_head[0] | upsample_weight[0]    UpdateEngine.heads_conv1 (one GEMM, relu) -> fm [M, 512]
    flow_head[2] 3x3 256 -> 6            pfk_conv2d_f32, cout 6                  -> fo   [M, 8]
    upsample_weight[2] 1x1 256 -> 576    UpdateEngine._conv                       -> mask [M, 576]
    upsample_data                        pfk_convex_upsample_info_pm_f32          -> flow_up, info_up

Layer scale: `gamma * (x @ W2^T + b2)` is computed as `x @ (gamma W2)^T + gamma b2`, one rounding moved.

`precision="bf16"` runs the same chain on the K8b path (`UpdateEngine`'s `b16`: bf16 activation rows, bf16 weights in 64-channel K
chunks, fp32 accumulation): the motion encoder writes the bf16 twin `hxb`, and per block

      dwconv 7x7 + LayerNorm             pfk_dwconv_layernorm_b16  (hxb)         -> ln   bf16 [M, 384]
      pwconv1 + GELU                     pfk_conv2d_gelu_b16                     -> mid  bf16 [M, 512]
      gamma * pwconv2 + input            pfk_conv2d_b16, LINEAR + residual hxb   -> res  bf16 [M, 384]
      final 1x1 384 -> 128               pfk_conv2d_b16                          -> hxb[:, :128]

The net state lives in hxb only (bf16, as the `final` convolution's output under autocast).  The heads read hxb; `fo` stays fp32
[M, 8], the mask logits are bf16 [M, 576] in the plain channel order, upsampled by pfk_convex_upsample_info_pm_b16.  gamma is folded
into W2 in fp32 and rounded to bf16 once: `bf16(gamma W2)` against autocast's `gamma * bf16(x W2^T)`, one weight rounding apart.

The seams (`accelerate(model, sea_raft_update=True)`, patch.py) hand the model's own loop (sea_raft.py:217-236) views of these
buffers, the way `PfkUpdateBlock` does for RAFT: `update_block(net, context, corr, flow) -> net` is the engine's h slice, and
`flow_head(net)` / `upsample_weight(net)` recognise that very object and run the heads from it.  Everything the kernels do not
implement — CPU tensors, gradient graphs, other dtypes, autocast — is passed to the wrapped modules unchanged.

`accelerate(model, sea_raft_update=True, sea_raft_train=True)` (opt-in, fp32): calls that carry a gradient graph — CUDA fp32, grad mode
on, an input or a parameter that requires grad, no autocast — run on the differentiable composition of train_sea.py (K12d) instead
of the wrapped modules, and are counted in `train_calls`.  `train_precision="bf16"` (`PfkSeaRaftUpdateBlock.train_precision`, K12f) runs
that composition on bf16 rows; the calls it takes and the fp32 tensors it hands back are the same.  With `train_upsample=True` on top, `upsample_data` in such a graph runs
`train_sea.upsample_data_train` (the inference kernel forward, `pfk_convex_upsample_info_bwd_pm_f32` backward; K12e) instead of the
model's own method, counted in the seam's `train_calls`; without it, it stays the model's method.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ._seam import ProbedMethodSeam, WrappedModule, carries_grad, eligible, pixel_rows
from .conv_path import EPI_LINEAR, EPI_LINEAR_GELU, PRECISIONS, check_precision
from .update import UpdateEngine, UpdateSpec, corr_rows

LN_EPS = 1e-6              # sea_raft/layer.py:57 (LayerNorm(dim, eps=1e-6))


def sea_spec(corr_channels: int = 324) -> UpdateSpec:
    """SEA-RAFT's BasicUpdateBlock at cdim = hdim = 128 (sea_raft/update.py:39-47): RAFT's motion encoder, no GRU, heads of
    sea_raft.py:114-126 (both hidden convolutions 128 -> 256, mask 576)."""
    return UpdateSpec(128, 128, corr_channels, 256, 192, 128, 64, 126, (), 256, True)


def sea_block_shapes(corr_channels: int, num_blocks: int) -> Dict[str, tuple]:
    """state_dict names / shapes of sea_raft/update.py:BasicUpdateBlock (cdim = hdim = 128, ConvNextBlock(384, 128))."""
    sh: Dict[str, tuple] = {}

    def conv(name, co, ci, k):
        sh[name + ".weight"] = (co, ci, k, k)
        sh[name + ".bias"] = (co,)

    conv("encoder.convc1", 256, corr_channels, 1)
    conv("encoder.convc2", 192, 256, 3)
    conv("encoder.convf1", 128, 2, 7)
    conv("encoder.convf2", 64, 128, 3)
    conv("encoder.conv", 126, 256, 3)
    for i in range(num_blocks):
        p = f"refine.{i}."
        sh[p + "dwconv.weight"] = (384, 1, 7, 7)
        sh[p + "dwconv.bias"] = (384,)
        sh[p + "norm.weight"] = (384,)
        sh[p + "norm.bias"] = (384,)
        sh[p + "pwconv1.weight"] = (512, 384)
        sh[p + "pwconv1.bias"] = (512,)
        sh[p + "pwconv2.weight"] = (384, 512)
        sh[p + "pwconv2.bias"] = (384,)
        sh[p + "gamma"] = (384,)
        conv(p + "final", 128, 384, 1)
    return sh


HEAD_SHAPES = {
    "flow_head": {"0.weight": (256, 128, 3, 3), "0.bias": (256,), "2.weight": (6, 256, 3, 3), "2.bias": (6,)},
    "upsample_weight": {"0.weight": (256, 128, 3, 3), "0.bias": (256,), "2.weight": (576, 256, 1, 1), "2.bias": (576,)},
}


class SeaUpdateEngine(UpdateEngine):
    """Packed weights and pixel-major buffers of SEA-RAFT's refinement (module docstring).  `params`: the update block's parameters
    (`encoder.*`, `refine.{i}.*`) and the heads' as `flow_head.{0,2}.*`, `upsample_weight.{0,2}.*`.
    `precision`: "fp32" or "bf16" (the K8b path, module docstring)."""

    def __init__(self, params: Dict[str, torch.Tensor], spec: UpdateSpec, device: torch.device, num_blocks: int = 2,
                 precision: str = "fp32"):
        self.num_blocks = int(num_blocks)
        self.precision = check_precision(precision, PRECISIONS)
        super().__init__(params, spec, device, precision)

    # ------------------------------------------------------------------ weights
    def pack(self, P: Dict[str, torch.Tensor]) -> None:
        # the motion encoder, the fused flow_head[0] | upsample_weight[0] GEMM (`fm`) and the 576-channel mask conv (`mk`) are RAFT's:
        # packed by UpdateEngine under its names
        alias = {"flow_head.conv1.": "flow_head.0.", "mask.0.": "upsample_weight.0.", "mask.2.": "upsample_weight.2."}
        Q = {k: v for k, v in P.items() if k.startswith("encoder.")}
        for dst, src in alias.items():
            for t in ("weight", "bias"):
                Q[dst + t] = P[src + t]
        super().pack(Q)
        dev = self.device

        def g(name):
            return P[name].detach().to(device=dev, dtype=torch.float32)

        pk = self.path.pack            # (bf16: rounded once from the fp32, gamma-folded weight)
        C = self.spec.hx_channels
        w = self.w
        for i in range(self.num_blocks):
            p = f"refine.{i}."
            w[f"dw{i}.w"] = g(p + "dwconv.weight").reshape(C, -1).contiguous()
            w[f"dw{i}.b"] = g(p + "dwconv.bias").contiguous()
            w[f"ln{i}.w"] = g(p + "norm.weight").contiguous()
            w[f"ln{i}.b"] = g(p + "norm.bias").contiguous()
            w1 = g(p + "pwconv1.weight")
            w[f"p1{i}.w"] = pk(w1[:, :, None, None], [(0, C, C)])
            w[f"p1{i}.b"] = g(p + "pwconv1.bias").contiguous()
            gamma = g(p + "gamma") if (p + "gamma") in P else torch.ones(C, device=dev)
            w2 = g(p + "pwconv2.weight")
            w[f"p2{i}.w"] = pk((gamma[:, None] * w2)[:, :, None, None], [(0, w2.shape[1], w2.shape[1])])
            w[f"p2{i}.b"] = (gamma * g(p + "pwconv2.bias")).contiguous()
            w[f"fi{i}.w"] = pk(g(p + "final.weight"), [(0, C, C)])
            w[f"fi{i}.b"] = g(p + "final.bias").contiguous()
            self._real_cin.update({f"p1{i}": C, f"p2{i}": w2.shape[1], f"fi{i}": C})
        w["fo.w"] = pk(g("flow_head.2.weight"), [(0, self.spec.fh_hidden, self.spec.fh_hidden)])
        w["fo.b"] = g("flow_head.2.bias").contiguous()
        self._real_cin["fo"] = self.spec.fh_hidden
        self.mid_channels = int(P["refine.0.pwconv1.weight"].shape[0]) if self.num_blocks else 0

    # ------------------------------------------------------------------ buffers
    def bind(self, B: int, H: int, W: int) -> None:
        if self._shape == (B, H, W):
            return
        super().bind(B, H, W)
        M, dev = B * H * W, self.device
        C = self.spec.hx_channels
        dt = self.path.dtype
        self.ln = torch.zeros(M, C, device=dev, dtype=dt)
        self.mid = torch.zeros(M, self.mid_channels, device=dev, dtype=dt)
        self.res = torch.zeros(M, C, device=dev, dtype=dt)
        self.fo = torch.zeros(M, 8, device=dev, dtype=torch.float32)      # flow_head output: delta (2) | info (4) | pad

    # ------------------------------------------------------------------ one iteration
    def refine(self) -> None:
        """`for blk in self.refine: net = blk(cat([net, inp]))` (update.py:52-53) on hx: each block's `final` writes the new net
        into hx[:, :128], which the next block (and the heads) read."""
        B, H, W = self._shape
        C = self.spec.hx_channels
        if self.path.b16:
            for i in range(self.num_blocks):
                self.ops.dwconv_layernorm_b16(self.hxb, self.w[f"dw{i}.w"], self.w[f"dw{i}.b"], self.w[f"ln{i}.w"], self.w[f"ln{i}.b"],
                                              LN_EPS, self.ln, B, H, W, 7)
                self.ops.conv2d_gelu_b16([self.ln], B, H, W, 1, 1, self.w[f"p1{i}.w"], self.w[f"p1{i}.b"], self.mid_channels, 1.0,
                                         self.mid)
                self._conv([self.mid], 1, 1, f"p2{i}", C, relu=False, out=self.res, residual=self.hxb)
                self._conv([self.res], 1, 1, f"fi{i}", self.spec.hidden, relu=False, out=self.hxb[:, : self.spec.hidden])
            return
        for i in range(self.num_blocks):
            self.ops.dwconv_layernorm(self.hx, self.w[f"dw{i}.w"], self.w[f"dw{i}.b"], self.w[f"ln{i}.w"], self.w[f"ln{i}.b"], LN_EPS,
                                      self.ln, B, H, W, 7)
            self._conv([self.ln], 1, 1, f"p1{i}", self.mid_channels, relu=False, out=self.mid, epi=EPI_LINEAR_GELU)
            self._conv([self.mid], 1, 1, f"p2{i}", C, relu=False, out=self.res, residual=self.hx)
            self._conv([self.res], 1, 1, f"fi{i}", self.spec.hidden, relu=False, out=self.hx[:, : self.spec.hidden])

    def update(self, corr_pm: torch.Tensor) -> None:
        """update.py:49-54: motion encoder into hx, then the ConvNeXt blocks; `flow` must already be in hx."""
        if self.wants_grouped_motion:
            self.motion_grouped(corr_pm)       # convc1 | convf2 as one grouped launch (same bits as motion())
        else:
            self.motion(corr_pm)
        self.refine()

    def stage(self, net: Optional[torch.Tensor], inp: Optional[torch.Tensor], flow: torch.Tensor, corr: torch.Tensor) -> torch.Tensor:
        """The block's NCHW inputs into the state: `net` and `inp` (None: staged already) into their slices of hx, or of hxb on the
        bf16 path, `flow` into hx's flow slice (mirrored into hxb).  `corr`: the lookup's fp32 rows on the fp32 path, read as
        they are; NCHW on the bf16 path, copied into corr16.  Returns the rows `update` reads."""
        s = self.spec
        if self.path.b16:
            def put(src, dst):         # any float NCHW -> the [M, C] rows `dst`, converting the dtype
                self.nchw_view(dst).copy_(src.permute(0, 2, 3, 1))
        else:
            def put(src, dst):
                self.ops.nchw_to_pm(src.contiguous(), dst)
        if net is not None:
            self.stage_net(net)
        if inp is not None:
            put(inp, self.act[:, s.hidden: s.hidden + s.context])
        if flow.dtype == torch.float32:
            self.ops.nchw_to_pm(flow.contiguous(), self.flow_view)
        else:
            put(flow, self.flow_view)
        self.flow_changed()            # bf16: the fp32 flow (convf1's input) mirrored into hxb (the ConvNeXt blocks' input)
        if not self.path.b16:
            return corr
        put(corr, self.corr16[:, : s.corr_channels])
        return self.corr16

    def stage_net(self, net: torch.Tensor) -> None:
        """`net` (any float NCHW) into the h slice of hx, or of hxb on the bf16 path"""
        dst = self.act[:, : self.spec.hidden]
        if self.path.b16:
            self.nchw_view(dst).copy_(net.permute(0, 2, 3, 1))
        else:
            self.ops.nchw_to_pm(net.contiguous(), dst)

    def flow_head_out(self) -> None:
        """flow_head[2] (3x3, 256 -> 6) on the flow-head half of fm -> fo[:, :6]: delta flow (2) | info (4)"""
        self._conv([self.fm[:, : self.spec.fh_hidden]], 3, 3, "fo", 6, relu=False, out=self.fo[:, :6])

    def mask_logits(self, scale: float = 1.0) -> None:
        """upsample_weight[2] (1x1, 256 -> 576) on the mask half of fm, times `scale` -> mask"""
        self._conv([self.fm[:, self.spec.fh_hidden:]], 1, 1, "mk", self.spec.mask_channels, relu=False, scale=scale, out=self.mask,
                   epi=EPI_LINEAR)

    def upsample(self, flow_pm: torch.Tensor, info_pm: torch.Tensor, mask_pm: torch.Tensor, flow_up: torch.Tensor,
                 info_up: torch.Tensor) -> None:
        """upsample_data (sea_raft.py:147-163) on pixel-major rows; mask_pm already scaled by 0.25"""
        self.ops.convex_upsample_info_pm(flow_pm, info_pm, mask_pm, flow_up, info_up)

    def fo_nchw(self) -> torch.Tensor:
        B, H, W = self._shape
        return self.fo[:, :6].unflatten(0, (B, H, W)).permute(0, 3, 1, 2)

    def net_nchw(self) -> torch.Tensor:
        """the net state as NCHW with channels-last strides: a view of hx's h slice, or of hxb's on the bf16 path"""
        if not self.path.b16:
            return super().net_nchw()
        B, H, W = self._shape
        return self.hxb[:, : self.spec.hidden].unflatten(0, (B, H, W)).permute(0, 3, 1, 2)

    def mask_nchw_raw(self) -> torch.Tensor:
        """the mask logits as NCHW with channels-last strides, in the buffer's own dtype (bf16 on the bf16 path)"""
        B, H, W = self._shape
        return self.mask.view(B, H, W, self.spec.mask_channels).permute(0, 3, 1, 2)


# precision -> (activation dtypes, cuda autocast) the seams serve: the kernels' inputs (`_seam.eligible`)
SEA_ACCEPTS = {"fp32": ((torch.float32,), False), "bf16": ((torch.float32, torch.bfloat16), torch.bfloat16)}


class PfkSeaRaftUpdateBlock(WrappedModule):
    """Drop-in for SEA-RAFT's ``model.update_block``: ``forward(net, inp, corr, flow) -> net`` NCHW (sea_raft/update.py:49-54), a
    view of the engine's h slice with channels-last strides, overwritten by the next call (the reference loop rebinds `net` every
    iteration, sea_raft.py:223).  Keeps the wrapped sub-modules (`encoder`, `refine`): state_dict keys, checkpoints and optimizers
    are unchanged.  The heads' parameters are read through `_heads` (not registered here: they stay the model's own children)."""

    def __init__(self, ref_block: torch.nn.Module, num_blocks: int, corr_channels: int, precision: str = "fp32"):
        super().__init__(ref_block)
        self.precision = check_precision(precision, PRECISIONS)
        self.spec = sea_spec(corr_channels)
        self.num_blocks = num_blocks
        self._heads: Dict[str, torch.nn.Module] = {}   # "flow_head" / "upsample_weight" -> the model's modules (set by patch)
        self._inp_ref, self._inp_version = None, -1
        self._last_out, self._last_version = None, -1
        self._fm_for = None        # the `net` object whose flow_head[0] | upsample_weight[0] activation `fm` holds
        self._out_b16 = False      # bf16 path: the handed-out net is a bf16 view (an autocast loop), else an fp32 copy
        self.calls = 0             # kernel-path calls (tests count them)
        self._adopted = None           # the net `adopt` staged last
        self.adopt_first_net = False   # the heads also serve the iteration-0 net (`adopt`); set with `accelerate(sea_raft_encoders=)`
        self.sea_train = False         # `accelerate(sea_raft_train=True)`: gradient-graph calls run on train_sea.py
        # "fp32" | "bf16": precision of that training path (`accelerate(train_precision=)`), independent of the inference `precision`
        self.train_precision = "fp32"
        self.train_calls = 0           # calls served by the training path
        self._train_cache: dict = {}   # its packed weights, keyed by parameter versions (`PfkUpdateBlock._train_cache`'s rules)

    def trains(self, tensors, params) -> bool:
        """the training path (train_sea.py) serves a call on `tensors`: opted in, CUDA fp32 throughout, grad mode on with something
        that requires grad, outside autocast"""
        if not (self.sea_train and self.precision == "fp32" and torch.is_grad_enabled() and not torch.is_autocast_enabled("cuda")):
            return False
        t0 = tensors[0]
        if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == t0.device for t in tensors):
            return False
        if not all(p.dtype == torch.float32 and p.device == t0.device for p in params):
            return False
        return any(t.requires_grad for t in tensors) or any(p.requires_grad for p in params)

    def _all_params(self) -> Dict[str, torch.nn.Parameter]:
        P = dict(self.named_parameters())
        for name, mod in self._heads.items():
            P.update({f"{name}.{k}": v for k, v in mod.named_parameters()})
        return P

    def _get_engine(self, device) -> SeaUpdateEngine:
        if self._engine is not None and self._engine.precision != self.precision:
            self._engine = None
        P = self._all_params()
        return self._engine_for(device, P.values(), lambda: SeaUpdateEngine(P, self.spec, device, self.num_blocks, self.precision),
                                lambda eng: eng.pack(P))

    def owns(self, x: torch.Tensor) -> bool:
        """`x` is the net this block handed out last, untouched since"""
        return x is self._last_out and x._version == self._last_version

    def accepts(self, tensors, params) -> bool:
        """the engine of this precision implements a call on `tensors` (SEA_ACCEPTS), with `params` fp32 on the same device"""
        return eligible(tensors, params, *SEA_ACCEPTS[self.precision]) and \
            all(p.dtype == torch.float32 and p.device == tensors[0].device for p in params)

    def set_precision(self, precision: str) -> None:
        """switch the kernel path (a second `accelerate` with another `sea_raft_update`): the engine is rebuilt on the next call"""
        if check_precision(precision, PRECISIONS) != self.precision:
            self.precision = precision
            self._engine, self._versions = None, None
            self._inp_ref, self._inp_version = None, -1
            self._last_out, self._last_version, self._fm_for = None, -1, None

    def _params(self):
        return list(self.parameters()) + [p for m in self._heads.values() for p in m.parameters()]

    def adopt(self, net: torch.Tensor) -> bool:
        """Iteration 0 (sea_raft.py:189-197): the heads run on `net` before the block was ever called — the split of `init_conv`'s
        output.  Stage it into the engine and treat it as handed out by this block, so the heads serve it from the engine's state and
        the loop's first `forward(net, ...)` finds it staged already.  Only with `adopt_first_net` (`accelerate(sea_raft_encoders=)`)."""
        s = self.spec
        if not (self.adopt_first_net and net.dim() == 4 and net.shape[1] == s.hidden
                and self.accepts((net,), self._params())):
            return False
        B, _, H, W = net.shape
        with torch.no_grad():
            eng = self._get_engine(net.device)
            eng.bind(B, H, W)
            eng.watch_faults()
            eng.stage_net(net)
        self._out_b16 = eng.b16 and (net.dtype == torch.bfloat16 or torch.is_autocast_enabled("cuda"))
        self._last_out, self._last_version, self._fm_for = net, net._version, None
        self._adopted = net
        return True

    def forward(self, net, inp, corr, flow):
        s = self.spec
        if (self.sea_train and all(torch.is_tensor(t) and t.dim() == 4 for t in (net, inp, corr, flow))
                and corr.shape[1] == s.corr_channels and net.shape[1] == s.hidden and inp.shape[1] == s.context and flow.shape[1] == 2
                and all(t.shape[0] == net.shape[0] and t.shape[2:] == net.shape[2:] for t in (inp, corr, flow))
                and self.trains((net, inp, corr, flow), list(self.parameters()))):
            from .train_sea import sea_update_block_train
            self._last_out, self._fm_for = None, None
            self.train_calls += 1
            return sea_update_block_train(dict(self.named_parameters()), s, net, inp, corr, flow, self.num_blocks, self._train_cache,
                                          self.train_precision)
        ok = (torch.is_tensor(corr) and net.dim() == 4 and corr.dim() == 4 and self.accepts((net, inp, corr, flow), self._params())
              and corr.shape[1] == s.corr_channels and net.shape[1] == s.hidden and inp.shape[1] == s.context)
        if self.precision == "fp32":
            # the fp32 engine reads the lookup's own rows (what ptlflow_amd.CorrBlock hands out); anything else is the module's
            corr_pm = corr_rows(corr) if ok else None
            ok = corr_pm is not None
        else:
            # the bf16 engine copies the lookup into its bf16 rows: any NCHW layout of the block's shapes
            corr_pm = corr
            ok = ok and flow.dim() == 4 and flow.shape[1] == 2 and \
                all(t.shape[0] == net.shape[0] and t.shape[2:] == net.shape[2:] for t in (inp, corr, flow))
        if not ok:
            # the wrapped module, on the NCHW tensor the family's own correlation block would have handed it (the B1 hook's
            # channel view holds the same values; a dense copy keeps the module's convolutions on their usual layout)
            self._last_out, self._fm_for = None, None
            return self._ref[0](net, inp, corr.contiguous() if torch.is_tensor(corr) else corr, flow)
        B, _, H, W = net.shape
        with torch.no_grad():
            eng = self._get_engine(net.device)
            eng.bind(B, H, W)
            new_forward = not self.owns(net)
            if new_forward:
                eng.watch_faults()
            new_inp = new_forward or inp is not self._inp_ref or inp._version != self._inp_version
            if new_inp:
                self._inp_ref, self._inp_version = inp, inp._version
            eng.update(eng.stage(net if new_forward else None, inp if new_inp else None, flow, corr_pm))
            out = eng.net_nchw()
            if eng.b16:
                # bf16 out where the model's own block would return bf16: a bf16 net, or any net inside cuda bf16 autocast
                self._out_b16 = net.dtype == torch.bfloat16 or torch.is_autocast_enabled("cuda")
                if not self._out_b16:
                    out = out.float()
        self.calls += 1
        self._last_out, self._last_version, self._fm_for = out, out._version, None
        return out

    def heads_fm(self, net: torch.Tensor) -> SeaUpdateEngine:
        """flow_head[0] | upsample_weight[0] (+ relu) from the engine's h, once per handed-out net"""
        eng = self._engine
        if self._fm_for is not net:
            with torch.no_grad():
                eng.heads_conv1(True)
            self._fm_for = net
        return eng


class _SeaHeadSeam(WrappedModule):
    """Wraps ``model.flow_head`` / ``model.upsample_weight`` (sea_raft.py:114-126), keeping their children 0 / 1 / 2.  Called with the
    net view the update block just handed out, it runs from the engine's pixel-major state; any other input (the `init_conv` split
    before the loop, sea_raft.py:191-197, CPU, half, autocast, gradient graphs) goes to the original module."""

    def __init__(self, ref: torch.nn.Module, block: PfkSeaRaftUpdateBlock, kind: str):
        super().__init__(ref)
        self._block = [block]
        self.kind = kind
        self.calls = 0
        self.train_calls = 0           # calls served by the training path (`accelerate(sea_raft_train=True)`)

    def __getitem__(self, i):          # model.flow_head[0] etc. keep working (nn.Sequential indexing)
        return list(self._modules.values())[i]

    def __len__(self):
        return len(self._modules)

    def forward(self, x):
        blk = self._block[0]
        if (blk.sea_train and torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == blk.spec.hidden
                and blk.trains((x,), list(self.parameters()))):
            # any [B, 128, H, W] net with a gradient graph, the iteration-0 split of `init_conv` included
            from .train_sea import sea_head_train
            self.train_calls += 1
            P = {f"{self.kind}.{k}": v for k, v in self.named_parameters()}
            return sea_head_train(P, self.kind, x, blk._train_cache, blk.train_precision)
        if not (torch.is_tensor(x) and (blk.owns(x) or blk.adopt(x)) and blk.accepts((x,), list(self.parameters()))):
            return self._ref[0](x)
        eng = blk.heads_fm(x)
        with torch.no_grad():
            if self.kind == "flow_head":
                eng.flow_head_out()
                out = eng.fo_nchw()            # fp32 on both paths
                if blk._adopted is x:
                    # iteration 0: the loop keeps this flow (`flow_8x = flow_update[:, :2]`, sea_raft.py:193) across the next
                    # flow_head call, which overwrites the engine's buffer; later iterations add it to a tensor of their own
                    out = out.clone()
            else:
                eng.mask_logits(1.0)
                # bf16 logits: a view for an autocast loop, an fp32 copy for an fp32 one
                out = eng.mask_nchw_raw() if eng.b16 and blk._out_b16 else eng.mask_nchw()
        self.calls += 1
        return out


def _rows(t: torch.Tensor, dtype: torch.dtype, align: int = 1) -> torch.Tensor:
    """`pixel_rows` of `t`, else one contiguous copy of them"""
    r = pixel_rows(t, dtype, align)
    return r if r is not None else t.permute(0, 2, 3, 1).clone(memory_format=torch.contiguous_format).view(-1, t.shape[1])


class _UpsampleDataSeam(ProbedMethodSeam):
    """`model.upsample_data(flow, info, mask)` (sea_raft.py:147-163) shadowed on the instance by `pfk_convex_upsample_info_pm_f32`
    behind the behaviour probe (`ProbedMethodSeam`, like seam B5's; a bf16 mask has a probe of its own, `ok16`).  Pixel-major rows
    are read without a copy where the strides allow (the channels-last `0.25 * upsample_weight(net)` and the info slice of
    `flow_head(net)`).  A call that carries a gradient graph goes to the model's own method, or — `train_upsample`, fp32 seams only:
    three CUDA fp32 tensors, grad mode on, something requiring grad, outside autocast, the probe passed — to
    `train_sea.upsample_data_train` (`train_calls`)."""

    refusal = "ptlflow_amd: this model's upsample_data is not SEA-RAFT's; it keeps the model's own method"

    def __init__(self, original, precision: str = "fp32"):
        super().__init__(original)
        self.precision = precision     # "bf16": also bf16 tensors and cuda bf16 autocast; bf16 masks on their own kernel
        self.ok16 = None               # the probe of the bf16-mask kernel
        self.train_upsample = False    # `accelerate(train_upsample=True)`: gradient-graph calls run `train_sea.upsample_data_train`
        self.train_calls = 0           # calls served by it

    @staticmethod
    def _kernel(flow, info, mask):
        B, _, H, W = flow.shape
        n = info.shape[1]
        flow_up = torch.empty(B, 2, 8 * H, 8 * W, device=flow.device, dtype=torch.float32)
        info_up = torch.empty(B, n, 8 * H, 8 * W, device=flow.device, dtype=torch.float32)
        flow, info = flow.float(), info.float()        # (bf16 flow / info of an autocast loop: fp32 rows, exact)
        f32 = torch.float32
        if mask.dtype == torch.bfloat16:
            torch.ops.pfk.convex_upsample_info_pm_b16(_rows(flow, f32), _rows(info, f32), _rows(mask, torch.bfloat16, 8), flow_up, info_up)
        else:
            torch.ops.pfk.convex_upsample_info_pm(_rows(flow, f32), _rows(info, f32), _rows(mask, f32, 4), flow_up, info_up)
        return flow_up, info_up

    def _probe_args(self, device, mask_dtype):
        """a small random input; a bf16 mask is given to the method as its exact fp32 value (the kernel's softmax runs in fp32)"""
        g = torch.Generator().manual_seed(7)
        flow = (torch.randn(2, 2, 5, 7, generator=g) * 3).to(device)
        info = torch.randn(2, 4, 5, 7, generator=g).to(device)
        mask = torch.randn(2, 576, 5, 7, generator=g).to(device=device, dtype=mask_dtype)
        return (flow, info, mask.float()), (flow, info, mask)

    def _probe_context(self):
        return torch.autocast("cuda", enabled=False)

    def __call__(self, *args, **kwargs):
        if kwargs or len(args) != 3 or not all(torch.is_tensor(a) for a in args):
            return self.original(*args, **kwargs)
        flow, info, mask = args
        shapes = (flow.dim() == 4 and flow.shape[1] == 2 and info.dim() == 4
                  and 1 <= info.shape[1] <= 8 and mask.dim() == 4 and mask.shape[1] == 576
                  and info.shape[0] == flow.shape[0] == mask.shape[0]
                  and info.shape[2:] == flow.shape[2:] == mask.shape[2:])
        if (self.train_upsample and self.precision == "fp32" and shapes and carries_grad(args)
                and self._verdict("ok", flow.device, torch.float32)):
            from .train_sea import upsample_data_train
            self.train_calls += 1
            return upsample_data_train(flow, info, mask)
        ok = shapes and eligible(args, (), *SEA_ACCEPTS[self.precision])
        if not (ok and self._verdict("ok16" if mask.dtype == torch.bfloat16 else "ok", flow.device, mask.dtype)):
            return self.original(flow, info, mask)
        self.calls += 1
        return self._kernel(flow, info, mask)
