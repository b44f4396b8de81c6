"""Drop-in shim for a *live* ptlflow model (a machine that has ptlflow + lightning installed).

    import ptlflow, ptlflow_amd.patch
    model = ptlflow.get_model("raft", ckpt_path="things").eval().cuda()
    ptlflow_amd.patch.accelerate(model)          # <- the only new line
    out = model({"images": images})              # validate.py / infer.py / model_benchmark.py unchanged

What gets replaced:
* seam B1 — every model family binds ``get_corr_block`` by name into its own model module at import
  (`from .corr import get_corr_block`, raft.py:10, gma.py:11, sea_raft.py:10, ccmr.py:10, ms_raft_plus.py:12), so the
  patch target is the *model module's* global, not `corr.py`;
* seam B3 — ``model.update_block`` is wrapped by `PfkUpdateBlock`, which keeps the original sub-modules
  (state_dict keys, checkpoints and optimizers are untouched) and only overrides ``forward``;
* seam B4 — ``model.fnet`` / ``model.cnet`` (`BasicEncoder`) are wrapped by `PfkEncoder` the same way;
* SEA-RAFT only, opt-in — ``accelerate(model, sea_raft_update=...)`` (update block, heads, ``upsample_data``; sea_update.py) and
  ``accelerate(model, sea_raft_encoders=...)`` (``ResNetFPN`` ``fnet`` / ``cnet`` and ``init_conv``; sea_encoder.py);
* seam B5 — ``model.upsample_flow`` (raft.py:112-123, a method the loop calls every iteration) is shadowed on the instance by
  the convex-upsampling kernel after a behaviour probe (`_UpsampleSeam`).  ``accelerate(model, train_upsample=True)``: this seam and
  SEA-RAFT's ``upsample_data`` also serve the calls that carry a gradient graph (forward and backward on the kernels).

Dispatch is by *implementation identity*, never by class name alone: about two dozen ptlflow families call their block
``BasicUpdateBlock`` with different layers and ``forward`` signatures (sea_raft/update.py:39-54 is a ConvNeXt stack that
returns one tensor; ccmr/update.py:152 takes six arguments).  A block is wrapped only when
  (1) its class comes from a module whose source was checked to be the RAFT/GMA implementation (`_UPDATE_BLOCKS`,
      `_ENCODERS` below — extendable with `register_update_block` / `register_encoder`), AND
  (2) its ``state_dict`` names and shapes are exactly those of the `UpdateSpec` / `BasicEncoder` the kernels implement.
Everything else is left untouched and keeps running the reference's own code; the B1 hook (which only depends on the
`get_corr_block` contract the five families share) is still installed for it.

Nothing in ptlflow is edited or copied; `restore(model)` undoes the patch.
"""
from __future__ import annotations

import contextvars
import importlib
import sys
from typing import Callable, Dict, Optional, Tuple

import torch

from . import load_native
from ._seam import ProbedMethodSeam, WrappedModule, carries_grad, eligible, pixel_rows
from .conv_path import PRECISIONS, check_precision
from .corr import get_corr_block as _pfk_get_corr_block
from .encoder import PfkEncoder
from .ms_encoder import _MS_CLASSES, PfkMultiScaleEncoder, describe_multiscale_encoder, served as _ms_encoder_served
from .ms_encoder import register_multiscale_encoder  # noqa: F401  (next to the other register_* hooks)
from .sea_encoder import PfkInitConv, PfkResNetEncoder, match_init_conv, match_resnet_fpn
from .sea_update import HEAD_SHAPES, PfkSeaRaftUpdateBlock, _SeaHeadSeam, _UpsampleDataSeam, sea_block_shapes
from .update import PfkUpdateBlock, UpdateSpec, basic_spec, ccmr_spec, gma_spec, ms_raft_plus_spec, small_spec
from .xcit import PfkXcitContext, match_xcit_context, served_context
from .xcit import register_xcit_aggregator  # noqa: F401  (the hook for further aggregator classes, next to the other register_* calls)
from .xcit import register_xcit_context  # noqa: F401  (likewise for the context grouping modules `model.xcit[i]`)

_ORIG = "_pfk_original_get_corr_block"

# (module of the class, class name) -> spec factory(corr_channels); raft/update.py:115-142, gma/update.py:127-160
_UPDATE_BLOCKS: Dict[Tuple[str, str], Callable[[int], UpdateSpec]] = {
    ("ptlflow.models.raft.update", "BasicUpdateBlock"): lambda cc: _with_corr_channels(basic_spec(), cc),
    ("ptlflow.models.raft.update", "SmallUpdateBlock"): lambda cc: _with_corr_channels(small_spec(), cc),
    ("ptlflow.models.gma.update", "GMAUpdateBlock"): lambda cc: _with_corr_channels(gma_spec(), cc),
    # ccmr/update.py:110-168: RAFT's encoder / SepConvGRU(512) / heads around an XCiT aggregator that stays the reference's module
    ("ptlflow.models.ccmr.update", "BasicUpdateBlock"): lambda cc: ccmr_spec(cc),
    # ms_raft_plus/update.py:119-153 (stack_coords=False): RAFT's block with a x2 mask head
    ("ptlflow.models.ms_raft_plus.update", "BasicUpdateBlock"): lambda cc: ms_raft_plus_spec(cc),
    # lcv/update.py is raft/update.py reformatted (LCV-RAFT swaps the cost volume for a learnable one, lcv/corr_lcv.py, and
    # keeps RAFT's encoders, update block and loop: lcv_raft.py:143-179)
    ("ptlflow.models.lcv.update", "BasicUpdateBlock"): lambda cc: _with_corr_channels(basic_spec(), cc),
    ("ptlflow.models.lcv.update", "SmallUpdateBlock"): lambda cc: _with_corr_channels(small_spec(), cc),
    # llaflow/update.py: RAFT's block (`llaflow_raft`) and GMA's with heads = 1 (`llaflow`; llaflow/gma.py's Aggregate is
    # gma/gma_utils.py's), around the family's own cost volume (llaflow/corr.py, built directly: no B1 there)
    ("ptlflow.models.llaflow.update", "BasicUpdateBlock"): lambda cc: _with_corr_channels(basic_spec(), cc),
    ("ptlflow.models.llaflow.update", "GMAUpdateBlock"): lambda cc: _with_corr_channels(gma_spec(), cc),
}
# parameters of a matched block that belong to a sub-module the wrapper keeps calling as is (not part of the shape check)
_FOREIGN_PREFIX = {("ptlflow.models.ccmr.update", "BasicUpdateBlock"): "aggregator."}
# (module, class) of the BasicEncoder implementations that are raft/extractor.py:122-194 verbatim
_ENCODERS = {
    ("ptlflow.models.raft.extractor", "BasicEncoder"),
    ("ptlflow.models.raft.extractor", "SmallEncoder"),     # raft_small: bottleneck blocks, extractor.py:197-267
    ("ptlflow.models.gma.extractor", "BasicEncoder"),
    ("ptlflow.models.lcv.extractor", "BasicEncoder"),       # lcv/extractor.py == raft/extractor.py, byte for byte
    ("ptlflow.models.lcv.extractor", "SmallEncoder"),
    ("ptlflow.models.llaflow.extractor", "BasicEncoder"),   # likewise identical to raft/extractor.py
}
# families whose CorrBlock pyramid is not the avg-pool one (sea_raft/corr.py:71-84)
_PYRAMID = {"ptlflow.models.sea_raft.sea_raft": "bilinear_f2"}


# (module of the class, class name) of SEA-RAFT update blocks (sea_raft/update.py:39-54: RAFT's motion encoder + ConvNeXt blocks,
# `forward(net, inp, corr, flow) -> net`); installed only with `accelerate(model, sea_raft_update=True)` (extendable with
# `register_sea_raft_update_block`), and only when the state_dict names / shapes are exactly sea_update.sea_block_shapes
_SEA_UPDATE_BLOCKS = {("ptlflow.models.sea_raft.update", "BasicUpdateBlock")}


def register_sea_raft_update_block(module: str, cls: str = "BasicUpdateBlock") -> None:
    """Declare another module's block to be SEA-RAFT's BasicUpdateBlock (the shape check still applies)."""
    _SEA_UPDATE_BLOCKS.add((module, cls))


def match_sea_raft(model: torch.nn.Module) -> Optional[Tuple[int, int]]:
    """(corr_channels, num_blocks) when `model.update_block`, `model.flow_head` and `model.upsample_weight` are provably SEA-RAFT's
    (sea_raft/update.py:39-54, sea_raft.py:114-126 at dim = 128), else None."""
    block = getattr(model, "update_block", None)
    if block is None or (type(block).__module__, type(block).__name__) not in _SEA_UPDATE_BLOCKS:
        return None
    sd = {k: tuple(v.shape) for k, v in block.state_dict().items()}
    w = sd.get("encoder.convc1.weight")
    if w is None or len(w) != 4:
        return None
    nb = len({k.split(".")[1] for k in sd if k.startswith("refine.")})
    if nb < 1 or sd != sea_block_shapes(int(w[1]), nb):
        return None
    for attr, want in HEAD_SHAPES.items():
        head = getattr(model, attr, None)
        if not isinstance(head, torch.nn.Sequential) or len(head) != 3 or not isinstance(head[1], torch.nn.ReLU):
            return None
        if {k: tuple(v.shape) for k, v in head.state_dict().items()} != want:
            return None
    return int(w[1]), nb


def _sea_precision(sea_raft_update, option: str = "sea_raft_update") -> Optional[str]:
    """`accelerate`'s `sea_raft_update` / `sea_raft_encoders` -> the SEA seams' precision, None = not installed"""
    if sea_raft_update is False or sea_raft_update is None:
        return None
    if sea_raft_update is True:
        return "fp32"
    return check_precision(sea_raft_update, PRECISIONS, option, "False, True, 'fp32' or 'bf16'")


# (module of the class, class name) of SEA-RAFT's ResNet encoders (sea_raft/extractor.py:6-116); wrapped only with
# `accelerate(model, sea_raft_encoders=...)` and only when the state_dict is exactly sea_encoder.resnet_fpn_shapes
_RESNET_ENCODERS = {("ptlflow.models.sea_raft.extractor", "ResNetFPN")}


def register_resnet_encoder(module: str, cls: str = "ResNetFPN") -> None:
    """Declare another module's class to be SEA-RAFT's ResNetFPN (the state_dict check still applies)."""
    _RESNET_ENCODERS.add((module, cls))


def match_resnet_encoder(enc: torch.nn.Module) -> bool:
    return (type(enc).__module__, type(enc).__name__) in _RESNET_ENCODERS and match_resnet_fpn(enc)


def _install_sea_encoders(model: torch.nn.Module, precision: str) -> bool:
    """SEA-RAFT's `fnet` / `cnet` (ResNetFPN) and, behind a wrapped `cnet`, `init_conv` (sea_encoder.py); True when any is installed.
    Installed wrappers of another precision are switched to this one (their engines are rebuilt on the next call)."""
    for attr in ("fnet", "cnet"):
        enc = getattr(model, attr, None)
        if isinstance(enc, PfkResNetEncoder):
            enc.set_precision(precision)
        elif enc is not None and match_resnet_encoder(enc):
            setattr(model, attr, PfkResNetEncoder(enc, precision))
    cnet, conv = getattr(model, "cnet", None), getattr(model, "init_conv", None)
    if isinstance(conv, PfkInitConv):
        conv.set_precision(precision)
    elif isinstance(cnet, PfkResNetEncoder) and conv is not None and match_init_conv(conv, cnet.final_conv.out_channels):
        model.init_conv = PfkInitConv(conv, cnet, precision)
    return any(isinstance(getattr(model, a, None), PfkResNetEncoder) for a in ("fnet", "cnet"))


def _install_sea_raft(model: torch.nn.Module, precision: str = "fp32") -> bool:
    """SEA-RAFT's update block, heads and `upsample_data` (sea_update.py); True when installed (or already there).  Installed seams
    of another precision are switched to this one (the block's engine is rebuilt on its next call)."""
    if isinstance(getattr(model, "update_block", None), PfkSeaRaftUpdateBlock):
        model.update_block.set_precision(precision)
        seam = model.__dict__.get("upsample_data")
        if isinstance(seam, _UpsampleDataSeam):
            seam.precision = precision
        return True
    m = match_sea_raft(model)
    if m is None:
        return False
    block = PfkSeaRaftUpdateBlock(model.update_block, num_blocks=m[1], corr_channels=m[0], precision=precision)
    block._heads = {"flow_head": model.flow_head, "upsample_weight": model.upsample_weight}
    model.update_block = block
    model.flow_head = _SeaHeadSeam(model.flow_head, block, "flow_head")
    model.upsample_weight = _SeaHeadSeam(model.upsample_weight, block, "upsample_weight")
    if callable(getattr(model, "upsample_data", None)) and not isinstance(model.__dict__.get("upsample_data"), _UpsampleDataSeam):
        _shadow(model, upsample_data=_UpsampleDataSeam(model.upsample_data, precision))
    return True


def _upsample_seam_expected(model: torch.nn.Module, upsample: bool, sea_precision: Optional[str]) -> bool:
    """an upsampling seam is installed on `model`, or `accelerate` with these options installs one"""
    d = getattr(model, "__dict__", {})
    if isinstance(d.get("upsample_flow"), _UpsampleSeam) or isinstance(d.get("upsample_data"), _UpsampleDataSeam):
        return True
    if upsample and callable(getattr(model, "upsample_flow", None)):
        return True
    return sea_precision is not None and callable(getattr(model, "upsample_data", None)) and match_sea_raft(model) is not None


def _shadow(obj, **seams) -> None:
    """Shadow methods of the instance `obj`: an instance attribute wins over the class's method (nn.Module's `__call__` looks
    `forward` up on the instance too).  Each seam keeps the method it replaces."""
    obj.__dict__.update(seams)


def _unshadow(obj, kind: type, name: str, *also: str) -> None:
    """Undo `_shadow` where `obj.name` is a `kind` seam: drop it and the names shadowed together with it."""
    d = getattr(obj, "__dict__", {})
    if isinstance(d.get(name), kind):
        for n in (name, *also):
            d.pop(n, None)


def _with_corr_channels(spec: UpdateSpec, corr_channels: int) -> UpdateSpec:
    from dataclasses import replace
    return replace(spec, corr_channels=corr_channels)


def register_update_block(module: str, cls: str, factory: Callable[[int], UpdateSpec], foreign_prefix: Optional[str] = None) -> None:
    """Declare another family's update block to be one of the three implementations above (shape check still applies).
    `foreign_prefix`: parameters under it belong to a sub-module the wrapper keeps calling as is (CCMR's `aggregator.`)."""
    _UPDATE_BLOCKS[(module, cls)] = factory
    if foreign_prefix:
        _FOREIGN_PREFIX[(module, cls)] = foreign_prefix


def register_encoder(module: str, cls: str = "BasicEncoder") -> None:
    _ENCODERS.add((module, cls))


def match_update_block(block: torch.nn.Module) -> Optional[UpdateSpec]:
    """The `UpdateSpec` this block implements, or None when it is not (provably) one of ours."""
    from .synth import update_block_shapes
    factory = _UPDATE_BLOCKS.get((type(block).__module__, type(block).__name__))
    if factory is None:
        return None
    foreign = _FOREIGN_PREFIX.get((type(block).__module__, type(block).__name__))
    sd = {k: tuple(v.shape) for k, v in block.state_dict().items() if not (foreign and k.startswith(foreign))}
    w = sd.get("encoder.convc1.weight")
    if w is None or len(w) != 4:
        return None
    spec = factory(int(w[1]))
    mk = sd.get("mask.2.weight")
    if mk is not None and spec.has_mask and mk[0] != spec.mask_channels and len(mk) == 4:
        from dataclasses import replace
        spec = replace(spec, mask_channels=int(mk[0]))      # 9 * scale^2: the upsampling factor is the model's choice
    want = update_block_shapes(spec)
    # GMA registers its unused relative-position tables nowhere under update_block; any extra or missing key is a mismatch
    return spec if sd == want else None


def _basic_encoder_shapes(out_dim: int, norm_fn: str, small: bool = False) -> Dict[str, tuple]:
    """state_dict names/shapes of BasicEncoder (raft/extractor.py:122-170) / SmallEncoder (:197-236) for norm_fn in
    {instance, batch, none}."""
    sh: Dict[str, tuple] = {}

    def conv(name, co, ci, k):
        sh[name + ".weight"] = (co, ci, k, k)
        sh[name + ".bias"] = (co,)

    def norm(name, c):
        if norm_fn == "batch":
            sh[name + ".weight"] = (c,)
            sh[name + ".bias"] = (c,)
            sh[name + ".running_mean"] = (c,)
            sh[name + ".running_var"] = (c,)
            sh[name + ".num_batches_tracked"] = ()

    dims = (32, 32, 64, 96) if small else (64, 64, 96, 128)
    conv("conv1", dims[0], 3, 7)
    norm("norm1", dims[0])
    cin = dims[0]
    for i, (dim, stride) in enumerate(zip(dims[1:], (1, 2, 2)), start=1):
        for j, (ci, s) in enumerate(((cin, stride), (dim, 1))):
            p = f"layer{i}.{j}"
            if small:    # BottleneckBlock: 1x1 -> 3x3 -> 1x1 at a quarter of the width, norm4 on the downsample path
                conv(p + ".conv1", dim // 4, ci, 1)
                conv(p + ".conv2", dim // 4, dim // 4, 3)
                conv(p + ".conv3", dim, dim // 4, 1)
                norm(p + ".norm1", dim // 4)
                norm(p + ".norm2", dim // 4)
                norm(p + ".norm3", dim)
                extra = ".norm4"
            else:
                conv(p + ".conv1", dim, ci, 3)
                conv(p + ".conv2", dim, dim, 3)
                norm(p + ".norm1", dim)
                norm(p + ".norm2", dim)
                extra = ".norm3"
            if s != 1:
                norm(p + extra, dim)
                conv(p + ".downsample.0", dim, ci, 1)
                norm(p + ".downsample.1", dim)
        cin = dim
    conv("conv2", out_dim, dims[3], 1)
    return sh


def match_encoder(enc: torch.nn.Module) -> bool:
    if (type(enc).__module__, type(enc).__name__) not in _ENCODERS:
        return False
    norm_fn = getattr(enc, "norm_fn", None)
    if norm_fn not in ("instance", "batch", "none") or getattr(enc, "dropout", None) is not None:
        return False
    sd = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    out = sd.get("conv2.weight")
    return out is not None and sd == _basic_encoder_shapes(out[0], norm_fn, type(enc).__name__ == "SmallEncoder")


def _supported_envelope(fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int, radius: int) -> bool:
    """What `CorrBlock` (K1-K3) was built for; anything else stays on the reference implementation."""
    if fmap1.dim() != 4 or fmap2.dim() != 4 or fmap1.shape[0] != fmap2.shape[0] or fmap1.shape[1] != fmap2.shape[1]:
        return False
    B, D, h, w = fmap1.shape
    h2, w2 = fmap2.shape[-2:]
    if not (1 <= radius <= 4 and 1 <= num_levels <= 8 and D % 32 == 0):
        return False
    if fmap1.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        return False
    # kernels address one batch element's feature matrix / one source with 32-bit byte offsets
    return max(h * w, h2 * w2) * D * 4 < 2 ** 31 - 1 and B * h * w * num_levels * (2 * radius + 1) ** 2 * 4 < 2 ** 31 - 1


# the accelerated model instance whose forward is running publishes its lookup layout here (None: no such forward on this context)
_LAYOUT: "contextvars.ContextVar[Optional[bool]]" = contextvars.ContextVar("pfk_lookup_channels_last", default=None)
# ... and whether its lookups return a coordinate gradient (`accelerate(model, multiscale_train=True)`)
_COORDS_GRAD: "contextvars.ContextVar[bool]" = contextvars.ContextVar("pfk_lookup_coords_grad", default=False)
_LAYOUT_HOOKS = "_pfk_layout_hooks"


def _bracket_forward_with_layout(model: torch.nn.Module, channels_last: bool, coords_grad: bool = False) -> None:
    """forward pre-hook / hook pair on the INSTANCE: sets `_LAYOUT` and `_COORDS_GRAD` for the duration of its forward (re-entrant:
    a token stack)."""
    state = model.__dict__.get(_LAYOUT_HOOKS)
    if state is not None:
        state["channels_last"], state["coords_grad"] = channels_last, coords_grad
        return
    state = {"channels_last": channels_last, "coords_grad": coords_grad, "tokens": []}

    def pre(_m, _args, _kwargs=None):
        state["tokens"].append((_LAYOUT.set(state["channels_last"]), _COORDS_GRAD.set(state["coords_grad"])))

    def post(_m, _args, _out):
        if state["tokens"]:
            layout, coords_grad = state["tokens"].pop()
            _COORDS_GRAD.reset(coords_grad)
            _LAYOUT.reset(layout)

    state["handles"] = (model.register_forward_pre_hook(pre), model.register_forward_hook(post, always_call=True))
    model.__dict__[_LAYOUT_HOOKS] = state


def _make_corr_hook(module_name: str, original):
    pyramid = _PYRAMID.get(module_name, "avgpool")

    def get_corr_block(fmap1, fmap2, num_levels: int = 4, radius: int = 4, alternate_corr: bool = False, **kw):
        # GPU tensors inside the kernels' envelope go to libpfk (inference and — with gradients flowing to the feature maps
        # through `pfk_corr_lookup_bwd_f32` / `pfk_corr_volume_bwd_f32` — training); CPU tensors, alternate_corr, other
        # shapes stay on the reference's own implementation.
        if fmap1.is_cuda and not alternate_corr and not kw and _supported_envelope(fmap1, fmap2, num_levels, radius):
            # layout per model INSTANCE (several instances of one family module may be accelerated with different `update_block=`
            # settings): `accelerate` brackets the instance's forward with hooks that publish its setting in a context variable
            # (`_LAYOUT`); a caller outside such a forward gets the hook's default, set by the last `accelerate` on this module
            cl = _LAYOUT.get()
            if cl is None:
                cl = get_corr_block.channels_last
            return _pfk_get_corr_block(fmap1, fmap2, num_levels=num_levels, radius=radius, pyramid=pyramid, channels_last=cl,
                                       coords_grad=_COORDS_GRAD.get())
        return original(fmap1=fmap1, fmap2=fmap2, num_levels=num_levels, radius=radius, alternate_corr=alternate_corr, **kw)

    get_corr_block.pyramid = pyramid
    # layout of the lookups handed back: a channels-last view for this package's own update block (no transpose), plain NCHW
    # for a model whose update block stays torch code (set by `accelerate`, see CorrBlock.__init__)
    get_corr_block.channels_last = True
    return get_corr_block


class _UpsampleSeam(ProbedMethodSeam):
    """Seam B5 — `model.upsample_flow(flow, mask)` (raft.py:112-123; the same method in gma.py:130-141, ccmr.py:128-139):
    8x convex upsampling, called once per iteration by the reference's loop, in the reference five torch kernels over a
    [B, 576, h, w] mask (softmax, unfold, multiply, sum, permute-copy).  The replacement is `pfk_convex_upsample_f32`, behind
    the behaviour probe of `ProbedMethodSeam` (a family whose `upsample_flow` does something else — another scale, a different
    neighbourhood — keeps its own code).  CPU tensors, other mask widths and dtypes always take the original; so do gradient
    graphs, unless `train_upsample` is set (`accelerate(model, train_upsample=True)`): then the plain call on two CUDA fp32 tensors
    with grad mode on, something requiring grad and no autocast runs `train.convex_upsample` (`pfk_convex_upsample_f32` forward,
    `pfk_convex_upsample_bwd_f32` backward) and is counted in `train_calls`.  The dead-work skip is never active in grad mode.

    `multiscale` (`accelerate(model, multiscale_upsample=True)`): the seam also serves `upsample_flow(flow, mask, scale=2)` /
    `(flow, mask, 2)` of the multi-scale families (ccmr/ccmr.py:196,213, ms_raft_plus/ms_raft_plus.py:199,209) with
    `pfk_convex_upsample2_f32` — CUDA fp32 tensors, a 36-channel mask, an eval-mode model, no gradient graph, no autocast, behind a
    probe of its own (`ok2`: `original(flow, mask, scale=2)` against the kernel; separate from `ok`).  Every other scale, extra
    arguments, CPU tensors and gradient graphs go to the model's method as before.  Served calls count in `calls`.

    `multiscale_train` (`accelerate(model, multiscale_train=True)`, independent of `multiscale`): a `scale=2` call of either shape that
    carries a gradient graph — CUDA fp32 tensors, a 36-channel mask, grad mode on with something requiring grad, no autocast, the
    `ok2` probe passed — runs `train.convex_upsample2` (`pfk_convex_upsample2_f32` forward, `pfk_convex_upsample2_bwd_f32` backward)
    and is counted in `train_calls`."""

    refusal = "ptlflow_amd: this model's upsample_flow is not RAFT's 8x convex upsampling; seam B5 keeps the model's own method"

    def __init__(self, original):
        super().__init__(original)
        self.skip = None        # `_DeadWorkSkip` shared with seam B3 (accelerate(..., skip_dead_upsample=True)), else None
        self.train_upsample = False    # `accelerate(train_upsample=True)`: gradient-graph calls run `train.convex_upsample`
        self.train_calls = 0           # calls served by it
        self.multiscale = False        # `accelerate(multiscale_upsample=True)`: `scale=2` calls run `pfk_convex_upsample2_f32`
        self.multiscale_train = False  # `accelerate(multiscale_train=True)`: `scale=2` calls with a gradient graph run `train.convex_upsample2`
        self.ok2 = None                # the x2 probe's verdict (None = not probed yet)

    @staticmethod
    def _kernel2(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        B, _, H, W = flow.shape
        rows = pixel_rows(mask, torch.float32)      # PfkUpdateBlock's mask: a view, no copy
        if rows is None:      # (`.contiguous()`: a plain NCHW mask of one image reshapes to a VIEW with channel stride H * W)
            rows = mask.permute(0, 2, 3, 1).contiguous().view(B * H * W, 36)
        out = torch.empty(B, 2, 2 * H, 2 * W, device=flow.device, dtype=torch.float32)
        torch.ops.pfk.convex_upsample2(flow.contiguous(), rows, out)
        return out

    refusal2 = ("ptlflow_amd: this model's upsample_flow(flow, mask, scale=2) is not the x2 convex upsampling of the multi-scale "
                "families; seam B5 keeps the model's own method for scale=2 calls")

    def _refusal(self, *key):
        return self.refusal2 if key == (2,) else self.refusal

    def _probe_pair(self, *key):
        if key == (2,):
            return (lambda flow, mask: self.original(flow, mask, scale=2)), self._kernel2
        return super()._probe_pair(*key)

    @staticmethod
    def _scale2_call(args, kwargs):
        """(flow, mask) of a call shaped `(flow, mask, scale=2)` or `(flow, mask, 2)`, else None"""
        if len(args) == 3 and not kwargs:
            scale = args[2]
        elif len(args) == 2 and set(kwargs) == {"scale"}:
            scale = kwargs["scale"]
        else:
            return None
        if type(scale) is not int or scale != 2 or not (torch.is_tensor(args[0]) and torch.is_tensor(args[1])):
            return None
        return args[0], args[1]

    def _serve2(self, flow: torch.Tensor, mask: torch.Tensor):
        """the x2 upsampling of a served call, or None: the call is the model's own method's"""
        skip = self.skip if isinstance(self.skip, _MultiScaleSkip) else None
        if skip is not None and skip.upsample_is_dead():
            # the block call before this one left its mask out: the answer never falls through to `original` on that stale view
            if skip.first_upsample_since_block() and not torch.is_grad_enabled():
                self.calls += 1
                return skip.scratch(flow)
            skip.recover()      # a second reader of a mask the schedule held for dead: compute it after all, skip nothing more
        shapes = flow.dim() == 4 and flow.shape[1] == 2 and mask.dim() == 4 and mask.shape[1] == 36 \
            and flow.shape[0] == mask.shape[0] and flow.shape[2:] == mask.shape[2:]
        model = getattr(self.original, "__self__", None)
        if not shapes or getattr(model, "training", False) or not eligible((flow, mask), dtypes=(torch.float32,), autocast=False) \
                or not self._verdict("ok2", flow.device, 2):
            return None
        self.calls += 1
        return self._kernel2(flow, mask)

    @staticmethod
    def _kernel(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        B, _, H, W = flow.shape
        pm = mask.permute(0, 2, 3, 1)
        pm = pm.reshape(B * H * W, 576) if pm.is_contiguous() else pm.contiguous().view(B * H * W, 576)   # PfkUpdateBlock's mask: a view
        out = torch.empty(B, 2, 8 * H, 8 * W, device=flow.device, dtype=torch.float32)
        torch.ops.pfk.convex_upsample(flow.contiguous(), pm, out)
        return out

    def _probe_args(self, device, scale: int = 8):
        g = torch.Generator().manual_seed(5)
        flow = (torch.randn(2, 2, 5, 7, generator=g) * 3).to(device)
        mask = torch.randn(2, 9 * scale * scale, 5, 7, generator=g).to(device)
        return (flow, mask), (flow, mask)

    def _train2(self, flow: torch.Tensor, mask: torch.Tensor):
        """the x2 upsampling of a call that carries a gradient graph (`multiscale_train`), or None"""
        shapes = flow.dim() == 4 and flow.shape[1] == 2 and mask.dim() == 4 and mask.shape[1] == 36 \
            and flow.shape[0] == mask.shape[0] and flow.shape[2:] == mask.shape[2:]
        if not shapes or not carries_grad((flow, mask)) or not self._verdict("ok2", flow.device, 2):
            return None
        from .train import convex_upsample2
        self.train_calls += 1
        rows = pixel_rows(mask, torch.float32)      # PfkUpdateBlock's training mask: a view
        if rows is None:
            rows = mask.permute(0, 2, 3, 1).reshape(-1, 36)
        return convex_upsample2(flow, rows)

    def __call__(self, *args, **kwargs):
        if self.multiscale or self.multiscale_train:
            fm = self._scale2_call(args, kwargs)
            out = None
            if fm is not None and self.multiscale_train:
                out = self._train2(*fm)
            if out is None and fm is not None and self.multiscale:
                out = self._serve2(*fm)
            if out is not None:
                return out
        # Other families give `upsample_flow` more arguments — ccmr.py:213 / ms_raft_plus.py:199 pass `scale=`, dip a `rate`,
        # rapidflow / dpflow a `factor`, gmflow (feature, bilinear, upsample_factor): anything but the plain two-tensor
        # positional call is the model's own business and goes to its own method exactly as it was written.
        if kwargs or len(args) != 2 or not (torch.is_tensor(args[0]) and torch.is_tensor(args[1])):
            return self.original(*args, **kwargs)
        flow, mask = args
        shapes = mask.dim() == 4 and mask.shape[1] == 576 and flow.dim() == 4 and flow.shape[1] == 2
        if self.train_upsample and shapes and flow.shape[0] == mask.shape[0] and flow.shape[2:] == mask.shape[2:] \
                and carries_grad(args) and self._verdict("ok", flow.device):
            from .train import convex_upsample
            self.train_calls += 1
            rows = pixel_rows(mask, torch.float32)      # PfkUpdateBlock's training mask: a view
            if rows is None:
                rows = mask.permute(0, 2, 3, 1).reshape(-1, 576)
            return convex_upsample(flow, rows)
        if not (shapes and eligible(args, dtypes=(torch.float32,)) and self._verdict("ok", flow.device)):
            return self.original(flow, mask)
        self.calls += 1
        if isinstance(self.skip, _DeadWorkSkip):      # (a `_MultiScaleSkip` schedules the `scale=2` calls above only)
            if self.skip.upsample_is_dead():
                return self.skip.scratch(flow)      # a non-final iteration's prediction: eval drops it (raft/raft.py:186-192)
            eng = self.skip.take_deferred(mask)
            if eng is not None:
                # seam B3 left mask conv2 to this call: raft/update.py:152 + raft/raft.py:112-123 as ONE kernel on the mask head's
                # hidden activation (K13, bit-identical to the pair); the flow goes pixel-major into the engine's flow slice, which
                # the next block call rewrites from its own `flow` argument anyway
                B, _, H, W = flow.shape
                out = torch.empty(B, 2, 8 * H, 8 * W, device=flow.device, dtype=torch.float32)
                torch.ops.pfk.nchw_to_pm(flow.contiguous(), eng.flow_view)
                eng.mask_upsample(out)
                return out
        return self._kernel(flow, mask)


# (module, class) of correlation MODULES whose volume is a bilinear form of the two feature maps: lcv/corr_lcv.py:19-50
_BILINEAR_VOLUMES = {("ptlflow.models.lcv.corr_lcv", "LearnableCorrBlock")}


class _VolumeToken:
    """What the adapted `compute_cost_volume` hands the caller's loop in place of the list of pyramid levels."""

    def __init__(self, block):
        self.block = block


class _LearnableVolumeSeam:
    """Seam B1 for LCV-RAFT's learnable cost volume (lcv/corr_lcv.py, called from lcv_raft.py:147,167).

    The volume is `(fmap1ᵀ W) fmap2 / √D` with `W = Pᵀ D P` rebuilt from the module's parameters on every call (:20-31), its
    pyramid and radius-r lookup are RAFT's (:44-49, :52-76).  So it IS `CorrBlock(W-transformed fmap1, fmap2)`: the transform is
    one `[B·N, D] x [D, D]` product, K1-K3 do the rest.  Both methods of the module instance are shadowed (the module object,
    its parameters and state_dict keys stay): `compute_cost_volume` returns a token, `forward(token, coords)` looks up.

    Left to the module's own code: CPU tensors, gradient graphs (W is learnable), shapes outside the kernels' envelope, and
    maps so small that the module stops pooling (`min(h, w) <= 2r + 1` at some level: it then repeats a level where RAFT's
    block keeps halving)."""

    def __init__(self, module: torch.nn.Module):
        self.module = module
        self.compute_original = module.compute_cost_volume
        self.forward_original = module.forward
        self.channels_last = True

    def eligible(self, fmap1: torch.Tensor, fmap2: torch.Tensor) -> bool:
        m = self.module
        if not (fmap1.is_cuda and fmap1.dim() == 4 and fmap1.shape == fmap2.shape):
            return False
        if torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad or any(p.requires_grad for p in m.parameters())):
            return False
        h, w = fmap1.shape[-2:]
        if any(min(h >> i, w >> i) <= 2 * m.radius + 1 for i in range(m.num_levels - 1)):
            return False
        return _supported_envelope(fmap1, fmap2, m.num_levels, m.radius)

    def compute_cost_volume(self, fmap1, fmap2):
        if not self.eligible(fmap1, fmap2):
            return self.compute_original(fmap1, fmap2)
        B, D, h, w = fmap1.shape
        # W by the module's own arithmetic: its method on a one-pixel crop (:20-31 run in full, the volume part on 1 x 1 maps)
        self.compute_original(fmap1[:, :, :1, :1].contiguous(), fmap2[:, :, :1, :1].contiguous())
        f1w = torch.matmul(fmap1.float().flatten(2).transpose(1, 2), self.module.W.float())       # [B, N, D]: already pixel-major
        block = _pfk_get_corr_block(f1w.view(B, h, w, D).permute(0, 3, 1, 2), fmap2.float(), num_levels=self.module.num_levels,
                                    radius=self.module.radius, channels_last=self.channels_last)
        return _VolumeToken(block)

    def forward(self, corr_pyramid, coords):
        if isinstance(corr_pyramid, _VolumeToken):
            return corr_pyramid.block(coords)
        return self.forward_original(corr_pyramid, coords)


_VOLUME_SEAM = "_pfk_learnable_volume_seam"


# (module, class) whose `forward` was checked to return, in eval mode, only the LAST iteration's upsampled flow: the loop runs
# `range(self.iters)`, `up_mask` is consumed by `self.upsample_flow` alone, and the intermediate `flow_up` tensors go into a list
# that eval drops (raft/raft.py:169-192, gma/gma.py:189-215).  Only for these the dead mask-head + upsampling work may be skipped.
_LAST_FLOW_ONLY_FORWARDS = {
    ("ptlflow.models.raft.raft", "RAFT"),
    ("ptlflow.models.gma.gma", "GMA"),
}


def register_last_flow_only_forward(module: str, cls: str) -> None:
    """Declare that `module.cls.forward` (and `upsample_flow`) is a loop of that kind — checked by whoever registers it."""
    _LAST_FLOW_ONLY_FORWARDS.add((module, cls))
_SKIP = "_pfk_dead_work_skip"


def _defining_class(model: torch.nn.Module, attr: str):
    for cls in type(model).__mro__:
        if attr in cls.__dict__:
            return cls
    return None


class _DeadWorkSkip:
    """§8 f2 at the seams (opt-in: `accelerate(model, skip_dead_upsample=True)`).  In eval the reference's loop computes the mask
    head and the 8x convex upsampling on every iteration and returns the last one only (raft/raft.py:180-192).  This object is shared
    by seam B3 (`PfkUpdateBlock`) and seam B5 (`_UpsampleSeam`): the block counts its calls since the forward began and, knowing
    `model.iters`, computes the mask half of fh|mask conv1 and mask conv2 on the final call only; `upsample_flow` returns a
    never-handed-out scratch tensor before it.  Active per forward only when the model is in eval mode, no gradient graph is
    recorded and `model.iters` is a positive int; any call at or beyond `iters - 1` computes everything."""

    def __init__(self, model: torch.nn.Module, skip_dead: bool = True, fuse: bool = True):
        import weakref
        self._model = weakref.ref(model)
        self.skip_dead = skip_dead   # False: every iteration keeps its mask head + upsampling (only the fused kernel is wanted)
        self.fuse = fuse             # live iterations: mask conv2 + softmax + upsampling as ONE kernel inside `upsample_flow` (K13)
        self.active = False
        self.iters = 0
        self.call = 0           # index of the update-block call in flight (0-based) within the current forward
        self._dead_now = False  # the call in flight is a non-final one: its mask / upsampled flow are never read
        self._scratch = None
        self._deferred = None   # (engine, data_ptr of the mask view handed out) of a live call whose mask conv2 was left to seam B5

    def begin_forward(self, fp32: bool = True, device=None, grid=None) -> None:
        """`fp32` = the state tensors of this forward are float32 (`device`, `grid`: read by `_MultiScaleSkip` only).  A half / bf16 model (`model.half()`, validate.py:243-244) gets
        its tensors back as fresh casts, so the block cannot tell the calls of one forward apart by storage: nothing is skipped
        for it (the counter used to restart on every call and the final mask was never computed)."""
        m = self._model()
        it = getattr(m, "iters", None) if m is not None else None
        self.active = bool(fp32 and m is not None and not m.training and not torch.is_grad_enabled()
                           and isinstance(it, int) and not isinstance(it, bool) and it >= 1)
        self.iters = it if self.active else 0
        self.call = 0
        self._dead_now = False
        self._deferred = None

    def next_call(self) -> bool:
        """Called by the block per call (after `begin_forward` on the first); True when this call's mask is dead."""
        dead = self.skip_dead and self.active and not torch.is_grad_enabled() and self.call < self.iters - 1
        self._dead_now = dead
        self.call += 1
        self._deferred = None
        return dead

    def may_defer(self) -> bool:
        """A live call of an armed forward may leave mask conv2 to `upsample_flow` (the fused kernel): same conditions as skipping."""
        m = self._model()
        return bool(self.fuse and self.active and not self._dead_now and m is not None and not m.training and not torch.is_grad_enabled())

    def defer(self, engine, mask_view: torch.Tensor) -> None:
        self._deferred = (engine, mask_view.data_ptr())

    def take_deferred(self, mask: torch.Tensor):
        """The engine whose mask conv2 is pending, if `mask` is the (unfilled) view the block handed out for this very call."""
        d, self._deferred = self._deferred, None
        if d is not None and torch.is_tensor(mask) and mask.data_ptr() == d[1]:
            return d[0]
        return None

    def upsample_is_dead(self) -> bool:
        m = self._model()
        return bool(self.active and self._dead_now and m is not None and not m.training and not torch.is_grad_enabled())

    def scratch(self, flow: torch.Tensor) -> torch.Tensor:
        B, _, H, W = flow.shape
        shape = (B, 2, 8 * H, 8 * W)
        if self._scratch is None or tuple(self._scratch.shape) != shape or self._scratch.device != flow.device:
            self._scratch = torch.zeros(shape, device=flow.device, dtype=torch.float32)
        return self._scratch


# (module, class) whose `forward` was checked to be a multi-scale loop of this kind (ccmr/ccmr.py:179-230,
# ms_raft_plus/ms_raft_plus.py:183-226): scale `index` runs `self.iters[index]` block calls on a `net` made fresh per scale; every
# block call is followed by one `self.upsample_flow(..., up_mask, scale=2)` whose result goes through `upflow2` /
# `postprocess_predictions` into a list that eval drops (only the last `flow_up` is returned, as `flows` and `flow_small`); the first
# iteration of a scale `index >= 1` calls `self.upsample_flow(..., up_mask, scale=2)` once more BEFORE its block call, on the previous
# scale's last mask; `up_mask` has no other reader.  So within a scale only the last block call's mask is live.
_MULTISCALE_LOOPS = {
    ("ptlflow.models.ccmr.ccmr", "CCMR"),                      # CCMRPlus inherits forward and upsample_flow
    ("ptlflow.models.ms_raft_plus.ms_raft_plus", "MSRAFTPlus"),
}


def register_multiscale_loop(module: str, cls: str) -> None:
    """Declare that `module.cls.forward` (and `upsample_flow`) is a multi-scale loop of that kind — checked by whoever registers it."""
    _MULTISCALE_LOOPS.add((module, cls))


def _iters_list_ok(it) -> bool:
    return isinstance(it, (list, tuple)) and len(it) > 0 and all(type(n) is int and n >= 1 for n in it)


class _MultiScaleSkip:
    """The dead-work skip for a per-scale iteration list (`accelerate(model, multiscale_upsample=True)`), shared by
    seam B3 and seam B5 as `_DeadWorkSkip` is.  A forward pre-hook on the model (`start_forward`) restarts the count and re-reads
    `model.iters`; every `begin_forward` from the block (a fresh `net`) moves to the next scale.  Within scale k the mask is live
    on block call `iters[k] - 1` only; an `upsample_flow(scale=2)` call is dead exactly when the block call before it was.

    Armed per forward, at its first block call, only when: eval mode, grad mode off, no autocast, fp32 state, `model.iters` a
    list / tuple of positive ints (no bools), and the x2 probe's verdict is True (probed there, outside stream capture; never on
    `ok2 is None`).  Disarmed for the rest of the forward — everything is computed — when the bookkeeping does not add up: a scale
    that began before the previous one had exactly `iters[k]` calls, a grid that is not twice the previous scale's, more scales
    than `len(iters)`, more calls than `iters[k]`, a block call without a pre-hook before it.  Re-armed only by the next pre-hook.

    Counters, per forward: `block_calls`, `masks_skipped`, `scratch_answers`."""

    skip_dead = True
    fuse = False      # no fused mask-conv2 + upsampling form for 36 channels

    def __init__(self, model: torch.nn.Module, seam: "_UpsampleSeam"):
        import weakref
        self._model = weakref.ref(model)
        self._seam = weakref.ref(seam)
        self._hook = self._end_hook = None
        self._scratch = {}
        self._reset()

    def _reset(self) -> None:
        self.iters = ()
        self.armed = False
        self._pending = False     # a pre-hook fired and the forward's first block call has not asked yet
        self.scale = -1
        self.call = 0             # block calls of the scale in flight
        self._grid = None
        self._dead_now = False
        self._ups_since_block = 0
        self._grad = True         # grad mode where the forward began (the block runs its kernels under no_grad: it cannot tell)
        self.block_calls = self.masks_skipped = self.scratch_answers = 0

    # ---- the model's forward pre-hook
    def start_forward(self, module=None, args=None):
        self._reset()
        m = self._model()
        it = getattr(m, "iters", None) if m is not None else None
        if _iters_list_ok(it):
            self.iters = tuple(it)
        self._pending = True
        self._grad = torch.is_grad_enabled()

    def end_forward(self, module=None, args=None, output=None):
        """the model's forward is over (or died): nothing is dead outside a forward — a direct `model.upsample_flow(..., scale=2)`
        from user code never gets the scratch tensor"""
        self.armed = False
        self._pending = False
        self._dead_now = False

    def install(self, model: torch.nn.Module) -> None:
        self._hook = model.register_forward_pre_hook(self.start_forward)
        self._end_hook = model.register_forward_hook(self.end_forward, always_call=True)

    def remove(self) -> None:
        for h in (self._hook, self._end_hook):
            if h is not None:
                h.remove()
        self._hook = self._end_hook = None

    def _conditions(self) -> bool:
        m = self._model()
        return bool(m is not None and not m.training and not self._grad and not torch.is_autocast_enabled("cuda"))

    # ---- seam B3
    def begin_forward(self, fp32: bool = True, device=None, grid=None) -> None:
        """a block call on a fresh `net`: the next scale begins (`grid` = its (H, W))"""
        if self._pending:
            self._pending = False
            seam = self._seam()
            self.armed = bool(fp32 and self.iters and self._conditions() and seam is not None and seam.multiscale
                              and device is not None and seam._verdict("ok2", device, 2) is True)
        elif self.armed:
            g = self._grid
            if self.call != self.iters[self.scale] or self.scale + 1 >= len(self.iters) or not fp32 \
                    or g is None or grid is None or tuple(grid) != (2 * g[0], 2 * g[1]):
                self.armed = False
        self.scale += 1
        self.call = 0
        self._grid = tuple(grid) if grid is not None else None

    def next_call(self) -> bool:
        """per block call (after `begin_forward` on a scale's first); True when this call's mask is dead"""
        self._pending = False       # a block call that did not begin a scale: this forward stays unarmed
        dead = False
        if self.armed:
            if not self._conditions() or self.scale < 0 or self.call >= self.iters[self.scale]:
                self.armed = False
            else:
                dead = self.call < self.iters[self.scale] - 1
        self.call += 1
        self.block_calls += 1
        self.masks_skipped += int(dead)
        self._dead_now = dead
        self._ups_since_block = 0
        return dead

    def may_defer(self) -> bool:
        return False

    def defer(self, engine, mask_view) -> None:
        pass

    def take_deferred(self, mask):
        return None

    # ---- seam B5
    def upsample_is_dead(self) -> bool:
        return self._dead_now

    def first_upsample_since_block(self) -> bool:
        self._ups_since_block += 1
        return self._ups_since_block == 1

    def recover(self) -> None:
        """The mask of the block call before was left out and has a reader after all (a scale that ended early): compute it from
        the block's state, which that call left complete, and skip nothing more in this forward."""
        m = self._model()
        self.armed = False
        self._dead_now = False
        m.update_block.fill_mask()

    def scratch(self, flow: torch.Tensor) -> torch.Tensor:
        B, _, H, W = flow.shape
        key = (B, 2, 2 * H, 2 * W, flow.device)
        if key not in self._scratch:
            self._scratch[key] = torch.zeros(key[:4], device=flow.device, dtype=torch.float32)
        self.scratch_answers += 1
        return self._scratch[key]


def _multiscale_skip_for(model: torch.nn.Module, warn: bool = True):
    """The multi-scale skip state, or None (with a warning saying why, when the caller asked for the skip explicitly)."""
    import warnings
    why = None
    fwd, ups = _defining_class(model, "forward"), _defining_class(model, "upsample_flow")
    it = getattr(model, "iters", None)
    seam = model.__dict__.get("upsample_flow")
    block = getattr(model, "update_block", None)
    if fwd is None or (fwd.__module__, fwd.__name__) not in _MULTISCALE_LOOPS:
        why = (f"`forward` is defined by {getattr(fwd, '__module__', '?')}.{getattr(fwd, '__name__', '?')}, not by one of the multi-scale "
               "loops checked to return only the last prediction in eval")
    elif ups is None or (ups.__module__, ups.__name__) not in _MULTISCALE_LOOPS:
        why = "`upsample_flow` is overridden"
    elif not _iters_list_ok(it):
        why = f"`model.iters` is not a non-empty list of positive ints ({it!r})"
    elif model.training:
        why = "the model is in train mode (every prediction enters the loss)"
    elif not (isinstance(block, PfkUpdateBlock) and block.spec.has_mask and block.spec.mask_channels == 36
              and isinstance(seam, _UpsampleSeam)):
        why = "seams B3 (an update block with a x2 mask head) and B5 are not both installed"
    if why is not None:
        if warn:
            warnings.warn(f"ptlflow_amd: skip_dead_upsample refused, every iteration keeps its mask head + upsampling: {why}",
                          RuntimeWarning, stacklevel=3)
        return None
    return _MultiScaleSkip(model, seam)


def _drop_skip(model: torch.nn.Module) -> None:
    skip = model.__dict__.pop(_SKIP, None)
    if skip is None:
        return
    if isinstance(skip, _MultiScaleSkip):
        skip.remove()
    if isinstance(getattr(model, "update_block", None), PfkUpdateBlock):
        model.update_block._skip = None
    seam = model.__dict__.get("upsample_flow")
    if isinstance(seam, _UpsampleSeam):
        seam.skip = None


def _dead_work_skip_for(model: torch.nn.Module, warn: bool = True, skip_dead: bool = True, fuse: bool = True):
    """The shared skip state, or None (with a warning saying why, when the caller asked for it explicitly) when skipping is not
    provably output-preserving for this model."""
    import warnings
    why = None
    fwd, ups = _defining_class(model, "forward"), _defining_class(model, "upsample_flow")
    it = getattr(model, "iters", None)
    if fwd is None or (fwd.__module__, fwd.__name__) not in _LAST_FLOW_ONLY_FORWARDS:
        why = (f"`forward` is defined by {getattr(fwd, '__module__', '?')}.{getattr(fwd, '__name__', '?')}, not by one of the loops checked "
               "to return only the last prediction in eval")
    elif ups is None or (ups.__module__, ups.__name__) not in _LAST_FLOW_ONLY_FORWARDS:
        why = "`upsample_flow` is overridden"
    elif not isinstance(it, int) or isinstance(it, bool) or it < 1:
        why = f"`model.iters` is not a positive int attribute ({it!r})"
    elif model.training:
        why = "the model is in train mode (every prediction enters the loss)"
    elif not (isinstance(model.update_block, PfkUpdateBlock) and model.update_block.spec.has_mask
              and isinstance(model.__dict__.get("upsample_flow"), _UpsampleSeam)):
        why = "seams B3 (a mask-head update block) and B5 are not both installed"
    if why is not None:
        if warn:
            warnings.warn(f"ptlflow_amd: skip_dead_upsample refused, every iteration keeps its mask head + upsampling: {why}",
                          RuntimeWarning, stacklevel=3)
        return None
    return _DeadWorkSkip(model, skip_dead=skip_dead, fuse=fuse)


def _set_ccmr_context(model: torch.nn.Module, on: bool) -> None:
    """`model.xcit[i]` -> `PfkXcitContext` (all elements or none), or back to the reference modules"""
    mods = getattr(model, "xcit", None)
    if not isinstance(mods, torch.nn.ModuleList) or len(mods) == 0:
        return
    for i, m in enumerate(mods):
        if isinstance(m, PfkXcitContext) and not on:
            mods[i] = m._ref[0]
    if on and all(isinstance(m, PfkXcitContext) or (served_context(m) and match_xcit_context(m)) for m in mods):
        for i, m in enumerate(mods):
            if not isinstance(m, PfkXcitContext):
                mods[i] = PfkXcitContext(m)


def accelerate(model: torch.nn.Module, corr: bool = True, update_block: bool = True,
               conv_precision: str = "fp32", encoders: bool = True, upsample: bool = True,
               skip_dead_upsample: Optional[bool] = None, fuse_mask_upsample: Optional[bool] = None,
               sea_raft_update=False, sea_raft_encoders=False, train_precision: str = "fp32",
               sea_raft_train: bool = False, train_upsample: bool = False, ccmr_aggregator: bool = False,
               multiscale_encoders: bool = False, multiscale_upsample: bool = False, ccmr_context: bool = False,
               multiscale_train: bool = False) -> torch.nn.Module:
    """Patch seams B1/B3/B4 (+ B5, the model's `upsample_flow` method) of a ptlflow model instance in place and return it.

    ``conv_precision``: "fp32" (default, the parity path) or a split-bf16 mode of the convolutions
    ("bf16x6", "bf16x3", "bf16"), see ``UpdateEngine``.
    ``skip_dead_upsample`` (eval + no_grad + float32 forwards only): compute the mask head and the convex upsampling on the LAST
    iteration only — the reference's loop computes them 32 times and returns the last (raft/raft.py:180-192) — and run that
    last one as the fused mask-conv2 + softmax + upsampling kernel inside `upsample_flow` (K13).  `flows` stays bit-identical.
    ``None`` (default): ON wherever it is provably output-preserving — the model's `forward` and `upsample_flow` are those of
    the loops checked to drop the intermediate predictions (`raft.RAFT`, `gma.GMA`), `model.iters` is a positive int and the
    model is in eval mode when it is accelerated — silently off otherwise; ``True``: the same, with a warning saying why when it
    is refused; ``False`` (opt-out): every iteration keeps its mask head and upsampling, as the reference (the fused kernel
    still serves them where the same checks pass; ``fuse_mask_upsample=False`` keeps the two separate launches).  Re-armed per
    forward: train mode, a gradient graph, a half / bf16 model or a changed `iters` are honoured (`_DeadWorkSkip`).
    ``sea_raft_update`` (default False): on a SEA-RAFT model, also replace its update block (motion encoder + ConvNeXt blocks), its
    `flow_head` / `upsample_weight` heads and its `upsample_data` by the kernels of sea_update.py (fp32 inference; anything else
    keeps the model's modules).  Off by default: plain `accelerate(model)` leaves SEA-RAFT's block to torch as before.
    ``sea_raft_update="bf16"``: the same seams on the bf16 matrix-core path (K8b, bf16 activation rows): they serve fp32 and bf16
    GPU tensors with autocast off or cuda autocast to bfloat16 (an autocast loop gets bf16 `net` / mask views back, an fp32 loop
    fp32 ones; `flow_head` returns fp32).  ``True`` and ``"fp32"`` are today's fp32 path; any other value raises ValueError.  A
    second call with another value switches the installed seams.  ``conv_precision`` is not read by the SEA seams.
    ``sea_raft_encoders`` (default False; the same values and switching rules): on a SEA-RAFT model, replace its ``ResNetFPN`` encoders
    `fnet` / `cnet` (BatchNorm folded, stem for the 3- and the 6-channel input) and `init_conv` by the kernels of sea_encoder.py.
    They serve eval-mode fp32 GPU inference ("bf16": also inside cuda autocast to bfloat16); anything else keeps the model's modules.
    ``train_precision`` ("fp32" default | "bf16"; anything else raises ValueError): precision of the update block's NATIVE TRAINING
    path, the calls that carry a gradient graph (`PfkUpdateBlock.train_precision`).  "bf16" runs its convolutions — forward, data
    and weight gradients — on the bf16 matrix cores (ptlflow_amd/train.py), as the reference does under
    torch.autocast(bfloat16); hidden state, flow and parameter gradients stay fp32.  The conditions of the fp32 training path
    apply unchanged (576 mask channels, no external aggregate).  GMA's update block trains natively in both precisions: its
    `attention` argument goes through to `train._AttnMatmul` and its gradient flows back to the caller's map.
    On a SEA-RAFT model with ``sea_raft_train=True`` it is the precision of that training path (`PfkSeaRaftUpdateBlock.train_precision`,
    ptlflow_amd/train_sea.py): "bf16" runs the update block and both heads on bf16 rows — the dense convolutions on the
    bf16 matrix cores, the depthwise convolution + LayerNorm and the GELU, forward and backward, on the `_b16` row kernels — and hands
    fp32 `net`, flow / info and mask logits back, so ``train_upsample`` keeps working unchanged.  It is independent of the inference
    precision: the spelling is ``accelerate(model, sea_raft_update=True, sea_raft_train=True, train_precision="bf16")``.
    A second call with another value switches it.
    ``sea_raft_train`` (default False; needs ``sea_raft_update=True`` or ``"fp32"``, anything else raises ValueError): the SEA-RAFT
    seams also serve the calls that carry a gradient graph — CUDA fp32 tensors, grad mode on, an input or a parameter that requires
    grad, outside autocast — on the native training path of ptlflow_amd/train_sea.py: the update block (motion
    encoder and ConvNeXt blocks) and the `flow_head` / `upsample_weight` heads on any such ``[B, 128, H, W]`` input, forward and
    backward, counted in each wrapper's ``train_calls``, in fp32 or with ``train_precision="bf16"`` on bf16 rows (``sea_raft_update="bf16"``
    with ``sea_raft_train=True`` stays refused).  `upsample_data` in a gradient graph stays the model's own method unless
    ``train_upsample`` is set.  Off: such calls reach the model's own modules, as before.
    ``train_upsample`` (default False): the upsampling seams — B5 (`upsample_flow`) and SEA-RAFT's `upsample_data` — also serve the
    plain positional call on CUDA fp32 tensors that carries a gradient graph (grad mode on, something requiring grad, outside
    autocast, the behaviour probe passed): forward on the inference kernel, backward on `pfk_convex_upsample_bwd_f32` /
    `pfk_convex_upsample_info_bwd_pm_f32`, counted in the seam's ``train_calls``.  Everything else, and every
    gradient graph while it is off, goes to the model's own method.  Raises ValueError when the model gets neither seam, and on a
    SEA-RAFT model unless ``sea_raft_update`` is True or "fp32".  A second call with another value switches the installed seams.
    ``ccmr_aggregator`` (default False): on a CCMR model, the update block also runs the scales' XCiT motion aggregators
    (``update_block.aggregator[i]``, ccmr/xcit.py) on the kernels of xcit.py instead of calling the modules in torch:
    the attention branch folded into one GEMM per image once per (forward, scale), seven launches per iteration on the update engine's
    own rows.  It serves eval-mode calls outside grad mode and autocast on fp32 GPU tensors with ``conv_precision="fp32"``, and only
    when every aggregator is a served class (`register_xcit_aggregator`) that passes `xcit.match_xcit_aggregator`; every other call
    runs the modules as before.  Served calls are counted in ``update_block.aggregator_calls``.  A second call with another value
    switches the path.
    ``multiscale_encoders`` (default False): on a CCMR, CCMR+ or MS-RAFT+ model, replace the multi-scale GroupNorm encoders `fnet` /
    `cnet` (ccmr/extractor.py, ms_raft_plus/extractor.py) by the kernels of ms_encoder.py: GroupNorm, the bilinear
    resize and the concatenating convolutions of the bottom-up path on pixel-major rows.  Installed on an encoder only when it is a
    served class (`register_multiscale_encoder`) that `ms_encoder.describe_multiscale_encoder` accepts.  The wrapper serves eval-mode
    calls outside grad mode and autocast on fp32 GPU tensors with fp32 parameters (``engine_calls``); every other call runs the
    reference module (``fallback_calls``).  ``conv_precision`` is not read.  A second call with another value switches the path.
    ``multiscale_upsample`` (default False): on a CCMR, CCMR+ or MS-RAFT+ model, seam B5 also serves the loop's
    `upsample_flow(flow, mask, scale=2)` calls with the x2 convex-upsampling kernel — CUDA fp32 tensors with a
    36-channel mask, eval mode, no gradient graph, no autocast, after a behaviour probe of its own; every other call reaches the
    model's method as before.  With it, ``skip_dead_upsample`` (``None`` or ``True``) extends to these models' per-scale iteration
    lists: within scale k the mask head runs on block call ``iters[k] - 1`` only and the `upsample_flow` calls after a dead block
    call return a scratch tensor; `flows` and `flow_small` stay bit-identical to ``skip_dead_upsample=False``.  It needs `forward`
    and `upsample_flow` of a loop checked by reading it (`register_multiscale_loop`), ``model.iters`` a non-empty list of positive
    ints, eval mode and both seams; ``True`` warns with the reason when it is refused.  Re-armed per forward by a forward pre-hook
    on the model (train mode, grad mode, a bf16 model or a changed ``iters`` are honoured); any inconsistency in the loop's call
    pattern turns it off for the rest of that forward.  The intermediate `up_mask` / `flow_up` tensors are not valid in eval while it
    is active.  Counters: ``model.update_block._skip.block_calls / masks_skipped / scratch_answers``.  A second call with another
    value switches it; `restore` removes the hook and the state.
    ``ccmr_context`` (default False): on a CCMR or CCMR+ model, replace the per-scale context grouping modules ``model.xcit[i]``
    (ccmr/ccmr.py:191: the XCiT block with one input) by `xcit.PfkXcitContext`: the NCHW input to token rows and
    LayerNorm in one kernel, the attention branch folded into one GEMM per image by `pfk_xca_fold_f32`, then the aggregator's tail;
    ten launches per call.  Installed only when EVERY element of ``model.xcit`` is a served class (`register_xcit_context`) that passes
    `xcit.match_xcit_context`.  A wrapper serves eval-mode calls outside grad mode and autocast on an fp32 GPU tensor [B, 128, H, W]
    (NCHW-contiguous or dense channels-last) with fp32 parameters (``engine_calls``); every other call runs the reference module
    (``fallback_calls``).  With it and the three options above every module a CCMR forward calls has a kernel path, and the forward
    repeats its bits.  ``conv_precision`` is not read.  A second call with another value switches it; `restore` undoes it.
    ``multiscale_train`` (default False; fp32 only: with ``train_precision="bf16"`` it raises ValueError): a training step of a
    CCMR, CCMR+ or MS-RAFT+ refinement loop on the kernels.  (1) The update block's native training path also takes
    these models' blocks — a 36-channel mask, and CCMR's external aggregate slot, whose per-scale `aggregator` module stays torch
    autograd on the NCHW view of the motion features — for fp32 CUDA calls outside autocast with ``conv_precision="fp32"``; served
    calls count in ``update_block.train_calls``.  (2) Seam B5 serves `upsample_flow(flow, mask, scale=2)` / `(flow, mask, 2)` calls
    that carry a gradient graph with `train.convex_upsample2` (backward: `pfk_convex_upsample2_bwd_f32`), behind the ``ok2`` probe,
    counted in the seam's ``train_calls``.  (3) The lookups of seam B1 return the gradient of their coordinates
    (`pfk_corr_lookup_coords_bwd_f32`): these loops rebuild `coords1` from `upsample_flow(..., up_mask, scale=2)` after the detach
    at the first iteration of every scale but the coarsest, so the previous scale's last mask receives a gradient through the
    lookup — which an accelerated model drops (returns zero for) while the option is off.  Under the option a lookup block built
    in grad mode keeps the row-major fp32 pyramid whether or not the feature maps require grad.  The on-demand (`alternate_corr`)
    block has no coordinate gradient, as in the reference.  Independent of ``multiscale_upsample``, whose skip is never armed in
    grad mode.  Off: every such call takes the reference's autograd, as before.  A second call with another value switches it;
    `restore` undoes it."""
    check_precision(train_precision, PRECISIONS, "train_precision")
    if multiscale_train and train_precision != "fp32":
        raise ValueError(f"multiscale_train=True is fp32 only (its training kernels are fp32), got train_precision={train_precision!r}")
    sea_precision = _sea_precision(sea_raft_update)
    if sea_raft_train and sea_precision != "fp32":
        raise ValueError(f"sea_raft_train=True needs sea_raft_update=True or 'fp32' (the training path sits behind the fp32 seams; "
                         f"its own precision is train_precision), got {sea_raft_update!r}")
    sea_enc_precision = _sea_precision(sea_raft_encoders, "sea_raft_encoders")
    if train_upsample:
        if (isinstance(getattr(model, "update_block", None), PfkSeaRaftUpdateBlock) or match_sea_raft(model) is not None) \
                and sea_precision != "fp32":
            raise ValueError(f"train_upsample=True needs sea_raft_update=True or 'fp32' on a SEA-RAFT model (the training path is fp32), "
                             f"got {sea_raft_update!r}")
        if not _upsample_seam_expected(model, upsample, sea_precision):
            raise ValueError("train_upsample=True: this model gets neither seam B5 (`upsample_flow`) nor SEA-RAFT's `upsample_data` seam")
    load_native()
    mod_name = type(model).__module__
    # registered classes (`class raft(RAFT)`) live in the same module as the implementation
    mod = sys.modules.get(mod_name) or importlib.import_module(mod_name)
    if corr and hasattr(mod, "get_corr_block") and not hasattr(mod, _ORIG):
        setattr(mod, _ORIG, mod.get_corr_block)
        mod.get_corr_block = _make_corr_hook(mod_name, getattr(mod, _ORIG))
    if update_block and hasattr(model, "update_block") and not isinstance(model.update_block, PfkUpdateBlock):
        spec = match_update_block(model.update_block)
        if spec is not None:
            model.update_block = PfkUpdateBlock(model.update_block, spec, conv_precision)
    if update_block and isinstance(getattr(model, "update_block", None), PfkUpdateBlock):
        model.update_block.train_precision = train_precision
        model.update_block.multiscale_train = bool(multiscale_train)
        model.update_block.set_ccmr_aggregator(ccmr_aggregator)
    sea = sea_precision is not None and _install_sea_raft(model, sea_precision)
    if sea:
        model.update_block.sea_train = bool(sea_raft_train)
        model.update_block.train_precision = train_precision
    if sea_enc_precision is not None:
        _install_sea_encoders(model, sea_enc_precision)
    if isinstance(getattr(model, "update_block", None), PfkSeaRaftUpdateBlock):
        # with both options the heads serve the iteration-0 prediction too (the split of `init_conv`'s output, sea_raft.py:189-197)
        model.update_block.adopt_first_net = isinstance(getattr(model, "init_conv", None), PfkInitConv)
    hook = getattr(mod, "get_corr_block", None)
    if corr and hasattr(mod, _ORIG) and hasattr(hook, "channels_last"):      # (default for callers that are not a model's forward)
        hook.channels_last = sea or isinstance(getattr(model, "update_block", None), PfkUpdateBlock)
        _bracket_forward_with_layout(model, hook.channels_last, bool(multiscale_train))
    cb = getattr(model, "corr_block", None)
    if corr and isinstance(cb, torch.nn.Module) and (type(cb).__module__, type(cb).__name__) in _BILINEAR_VOLUMES \
            and not isinstance(cb.__dict__.get(_VOLUME_SEAM), _LearnableVolumeSeam):
        seam = _LearnableVolumeSeam(cb)
        seam.channels_last = isinstance(getattr(model, "update_block", None), PfkUpdateBlock)
        _shadow(cb, **{_VOLUME_SEAM: seam, "compute_cost_volume": seam.compute_cost_volume, "forward": seam.forward})
    if encoders:
        # seam B4: the BasicEncoder feature / context networks (raft, gma: `self.fnet`, `self.cnet`)
        for attr in ("fnet", "cnet"):
            enc = getattr(model, attr, None)
            if enc is not None and not isinstance(enc, PfkEncoder) and match_encoder(enc):
                setattr(model, attr, PfkEncoder(enc, conv_precision, small=type(enc).__name__ == "SmallEncoder"))
    for attr in ("fnet", "cnet"):
        enc = getattr(model, attr, None)
        if isinstance(enc, PfkMultiScaleEncoder) and not multiscale_encoders:
            setattr(model, attr, enc._ref[0])
        elif multiscale_encoders and isinstance(enc, torch.nn.Module) and _ms_encoder_served(enc):
            desc = describe_multiscale_encoder(enc)
            if desc is not None:
                setattr(model, attr, PfkMultiScaleEncoder(enc, desc, _MS_CLASSES[(type(enc).__module__, type(enc).__name__)]))
    _set_ccmr_context(model, bool(ccmr_context))
    if upsample and callable(getattr(model, "upsample_flow", None)) and not isinstance(model.__dict__.get("upsample_flow"), _UpsampleSeam):
        _shadow(model, upsample_flow=_UpsampleSeam(model.upsample_flow))
    seam5 =model.__dict__.get("upsample_flow")
    if isinstance(seam5, _UpsampleSeam):
        seam5.multiscale = bool(multiscale_upsample)
        seam5.multiscale_train = bool(multiscale_train)
    # a model of a multi-scale family (a subclass included: `_multiscale_skip_for` says why it is refused) takes the per-scale skip
    ms_loop = bool(multiscale_upsample) and any((c.__module__, c.__name__) in _MULTISCALE_LOOPS for c in type(model).__mro__)
    if isinstance(model.__dict__.get(_SKIP), _MultiScaleSkip) and (not ms_loop or skip_dead_upsample is False):
        _drop_skip(model)
    if ms_loop and _SKIP not in model.__dict__ and skip_dead_upsample is not False:
        skip = _multiscale_skip_for(model, warn=skip_dead_upsample is True)
        if skip is not None:
            skip.install(model)
            model.__dict__[_SKIP] = skip
            model.update_block._skip = skip
            seam5.skip = skip
    both = isinstance(getattr(model, "update_block", None), PfkUpdateBlock) and isinstance(model.__dict__.get("upsample_flow"), _UpsampleSeam)
    if not ms_loop and _SKIP not in model.__dict__ and (skip_dead_upsample is True or both) \
            and not (skip_dead_upsample is False and fuse_mask_upsample is False):
        skip = _dead_work_skip_for(model, warn=skip_dead_upsample is True, skip_dead=skip_dead_upsample is not False,
                                   fuse=fuse_mask_upsample is not False)
        if skip is not None:
            model.__dict__[_SKIP] = skip
            model.update_block._skip = skip
            model.__dict__["upsample_flow"].skip = skip
    for name, kind in (("upsample_flow", _UpsampleSeam), ("upsample_data", _UpsampleDataSeam)):
        if isinstance(model.__dict__.get(name), kind):
            model.__dict__[name].train_upsample = bool(train_upsample)
    return model


def restore(model: torch.nn.Module) -> torch.nn.Module:
    _unshadow(model, _UpsampleDataSeam, "upsample_data")
    state = model.__dict__.pop(_LAYOUT_HOOKS, None)
    if state is not None:
        for h in state["handles"]:
            h.remove()
    _drop_skip(model)
    _unshadow(model, _UpsampleSeam, "upsample_flow")
    mod = sys.modules.get(type(model).__module__)
    if mod is not None and hasattr(mod, _ORIG):
        mod.get_corr_block = getattr(mod, _ORIG)
        delattr(mod, _ORIG)
    _unshadow(getattr(model, "corr_block", None), _LearnableVolumeSeam, _VOLUME_SEAM, "compute_cost_volume", "forward")
    for name, child in list(model._modules.items()):      # update_block, fnet / cnet, SEA-RAFT's heads
        if isinstance(child, WrappedModule):
            setattr(model, name, child._ref[0])
    _set_ccmr_context(model, False)
    return model
