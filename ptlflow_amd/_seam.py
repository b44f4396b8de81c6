"""The seam layer shared by the drop-in module wrappers (update.py, sea_update.py, encoder.py) and the method seams of patch.py:
adopting a wrapped module and keeping its engine current, the probe-then-dispatch method seam, pixel-major row views of NCHW
tensors and the eligibility rule of the kernel paths.  Imports torch only, so every one of those modules can import it."""
from __future__ import annotations

import contextlib
import warnings
from typing import Optional

import torch


class EngineSlot:
    """One engine and the versions of the tensors it was packed from: what `WrappedModule` keeps for its own module, and what a
    wrapper keeps for each further module it serves (`PfkUpdateBlock`'s XCiT aggregators, one per scale)."""
    _engine = None
    _versions = None

    def _engine_for(self, device, tensors, build, repack=None):
        """`_engine`, made by `build()` when there is none for `device`.  When a tensor of `tensors` (parameters, buffers) changed
        since (its `(data_ptr, _version)`), `repack(engine)` refreshes the engine in place; without `repack` it is rebuilt."""
        v = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._engine is None or self._engine.device != device or (v != self._versions and repack is None):
            self._engine = build()
        elif v != self._versions:
            repack(self._engine)
        self._versions = v
        return self._engine


class WrappedModule(torch.nn.Module, EngineSlot):
    """A drop-in for the model's sub-module `ref`: `ref`'s children are re-registered under their own names (state_dict keys,
    checkpoints and optimizers are unchanged) and `ref` itself is kept in a list (not registered twice in the module tree)."""

    def __init__(self, ref: torch.nn.Module):
        super().__init__()
        for name, child in ref.named_children():
            self.add_module(name, child)
        self._ref = [ref]
        self.training = ref.training
        self._engine = None
        self._versions = None


def eligible(tensors, params=(), dtypes=None, autocast=None) -> bool:
    """A kernel path may serve a call on `tensors`: GPU tensors on one device, of `dtypes` (None: any), no gradient graph through
    them or `params`.  `autocast`: False = cuda autocast must be off, a dtype = off or cuda autocast to that dtype, None = not read."""
    t0 = tensors[0]
    if not t0.is_cuda:
        return False
    if autocast is not None and torch.is_autocast_enabled("cuda") and (autocast is False or torch.get_autocast_dtype("cuda") != autocast):
        return False
    for t in tensors:
        if not torch.is_tensor(t) or (dtypes is not None and t.dtype not in dtypes) or t.device != t0.device:
            return False
    return not (torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in params)))


def carries_grad(tensors, params=()) -> bool:
    """A native fp32 training path may serve a call on `tensors` (the rule of `PfkSeaRaftUpdateBlock.trains`): CUDA fp32 tensors on
    one device, grad mode on with a tensor or a parameter that requires grad, outside cuda autocast."""
    if not torch.is_grad_enabled() or torch.is_autocast_enabled("cuda"):
        return False
    t0 = tensors[0]
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == t0.device for t in tensors):
        return False
    if not all(p.dtype == torch.float32 and p.device == t0.device for p in params):
        return False
    return any(t.requires_grad for t in tensors) or any(p.requires_grad for p in params)


def pixel_rows(t: torch.Tensor, dtype: torch.dtype, align: int = 1, dense: bool = False) -> Optional[torch.Tensor]:
    """The [B*H*W, C] pixel-major rows of the NCHW tensor `t` as a view, or None: `t` must be of `dtype`, its pixels one row stride
    apart with unit channel stride (channels-last strides, or a channel slice of such a buffer; `dense`: no slice), and the data
    pointer and the row stride multiples of `align` elements."""
    if t.dtype != dtype:
        return None
    B, C, H, W = t.shape
    pm = t.permute(0, 2, 3, 1)
    if not (pm.is_contiguous() if dense else
            (H == 1 or pm.stride(1) == W * pm.stride(2)) and (B == 1 or pm.stride(0) == H * W * pm.stride(2))):
        return None
    r = pm.view(B * H * W, C)
    if r.stride(1) != 1 or r.data_ptr() % (align * r.element_size()) or r.stride(0) % align:
        return None
    return r


class ProbedMethodSeam:
    """A method of a model instance (`original`) shadowed by a kernel (`_kernel`), dispatched by BEHAVIOUR, not by name: on the
    first eligible call the method and the kernel run on a small seeded random input (`_probe_args`) and the kernel serves from
    then on only if they agree to 1e-5, so a family whose method does something else keeps its own code.  The verdict is
    cached (`ok`: None = not probed yet); during stream capture nothing is probed (the probe copies host data) and the call
    takes the original.  Subclasses decide which calls are eligible and count the ones the kernel serves in `calls`."""

    refusal = "ptlflow_amd: this model's method is not the one the kernel implements; it keeps the model's own method"

    def __init__(self, original):
        self.original = original
        self.ok = None
        self.calls = 0

    def _probe_context(self):
        """the context the method runs in during the probe"""
        return contextlib.nullcontext()

    def _probe_pair(self, *key):
        return self.original, self._kernel

    def _refusal(self, *key):
        """the warning of a failed probe"""
        return self.refusal

    def _verdict(self, attr: str, device, *key) -> bool:
        """the probe's verdict cached in `attr`, probing on first use (`key`: what `_probe_args` varies on)"""
        ok = getattr(self, attr)
        if ok is None:
            if torch.cuda.is_current_stream_capturing():
                return False
            ok = self._probe(device, *key)
            setattr(self, attr, ok)
        return ok

    def _probe(self, device, *key) -> bool:
        """`_probe_args(device, *key)` -> (the method's arguments, the kernel's); True when their outputs agree in shape and to
        1e-5 of the largest magnitude.  `_probe_pair(*key)` names the two sides: (`original`, `_kernel`) unless a seam that serves
        more than one form of the call says otherwise."""
        want_args, got_args = self._probe_args(device, *key)
        try:
            original, kernel = self._probe_pair(*key)
            with torch.no_grad(), self._probe_context():
                want = original(*want_args)
            got = kernel(*got_args)
            if torch.is_tensor(got):
                want, got = (want,), (got,)
            ok = len(want) == len(got) and all(
                torch.is_tensor(a) and tuple(a.shape) == tuple(b.shape)
                and float((a.float() - b).abs().max()) <= 1e-5 * max(1.0, float(a.float().abs().max())) for a, b in zip(want, got))
        except Exception:
            ok = False
        if not ok:
            warnings.warn(self._refusal(*key), RuntimeWarning, stacklevel=4)
        return ok
