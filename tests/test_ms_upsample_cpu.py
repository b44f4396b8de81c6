"""`accelerate(model, multiscale_upsample=True)` without a GPU: the C entry point of the x2 convex upsampling (declared, exported,
argument checks), and the per-scale dead-work schedule (`patch._MultiScaleSkip`) driven by a call trace instead of kernels.

The trace (tests/golden/ms_loop_trace.json, scripts/make_golden_ms_upsample.py) is what the reference's own `CCMR()` and
`MSRAFTPlus()` eval forwards call, in order, with a counting stub in place of `update_block` and `upsample_flow`."""
import ctypes
import json
import os
import warnings

import pytest
import torch

import pfk_ctypes
from pfk_ctypes import PFK_ERR_BAD_ARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = json.load(open(os.path.join(ROOT, "tests", "golden", "ms_loop_trace.json")))


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbol():
    assert "pfk_convex_upsample2_f32" in pfk_ctypes.declared()
    lib = pfk_ctypes.lib()
    assert hasattr(lib, "pfk_convex_upsample2_f32")
    assert lib.pfk_abi_version() == 7            # an addition only


def test_bad_arguments_answer_status_codes():
    lib = pfk_ctypes.lib()
    f = lib.pfk_convex_upsample2_f32
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    P = 4096                                      # a made-up, aligned address: every case below is refused before a launch
    ok = dict(flow=P, flow_ld=0, mask=P, mask_ld=36, out=P, B=1, H=2, W=3)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["flow"], a["flow_ld"], a["mask"], a["mask_ld"], a["out"], a["B"], a["H"], a["W"], None)

    for kw in (dict(flow=None), dict(mask=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-1), dict(mask_ld=35), dict(mask_ld=0),
               dict(flow_ld=1), dict(flow_ld=-2)):
        assert call(**kw) == PFK_ERR_BAD_ARG, kw
    if not torch.cuda.is_available():            # (with a device an accepted case would launch on the made-up addresses)
        for kw in (dict(), dict(mask_ld=37), dict(mask_ld=40, flow_ld=2), dict(out=P + 4)):
            assert call(**kw) == pfk_ctypes.PFK_ERR_LAUNCH, kw      # accepted: no alignment is required, odd strides included


# ---------------------------------------------------------------------------------------------------------------------
# the schedule, driven by the recorded trace
# ---------------------------------------------------------------------------------------------------------------------
class _Block:
    filled = 0

    def fill_mask(self):
        self.filled += 1


class _Model(torch.nn.Module):
    def __init__(self, iters):
        super().__init__()
        self.iters = iters
        self.update_block = _Block()
        self.eval()


class _Seam:
    """what the schedule reads of seam B5: the option and the x2 probe's verdict"""

    def __init__(self, ok2=True):
        self.multiscale, self.ok2, self.probes = True, ok2, 0

    def _verdict(self, attr, device, *key):
        assert attr == "ok2" and key == (2,)
        self.probes += 1
        return False if self.ok2 is None else self.ok2      # None: "not probed, stream capture" answers False without a verdict


def _skip(iters, ok2=True):
    from ptlflow_amd.patch import _MultiScaleSkip
    model, seam = _Model(iters), _Seam(ok2)
    skip = _MultiScaleSkip(model, seam)
    skip._keep = (model, seam)      # the schedule holds weak references only
    return skip, model


def drive(skip, calls, fp32=True, hook=True):
    """feed `calls` ("update_block HxW" / "upsample_flow HxW") to the schedule as the two seams do, under no_grad; returns per call
    "live" / "dead" (block calls) and "kernel" / "scratch" (upsample calls).  A block call on another grid than the one before is a
    fresh `net`: a new scale."""
    out, grid = [], None
    with torch.no_grad():
        if hook:
            skip.start_forward()
        for name in calls:
            kind, size = name.split()
            hw = tuple(int(n) for n in size.split("x"))
            if kind == "update_block":
                if hw != grid:
                    skip.begin_forward(fp32=fp32, device=torch.device("cpu"), grid=hw)
                    grid = hw
                out.append("dead" if skip.next_call() else "live")
            else:
                if skip.upsample_is_dead():      # (the order of `_UpsampleSeam._serve2`)
                    if skip.first_upsample_since_block():
                        out.append("scratch")
                        continue
                    skip.recover()
                out.append("kernel")
    return out


def expected(iters, calls):
    """live exactly the last block call of each scale and the upsample calls after it"""
    want, scale, n, live = [], -1, 0, True
    grid = None
    for name in calls:
        kind, size = name.split()
        if kind == "update_block":
            if size != grid:
                scale, n, grid = scale + 1, 0, size
            n += 1
            live = n == iters[scale]
            want.append("live" if live else "dead")
        else:
            want.append("kernel" if live else "scratch")
    return want


@pytest.mark.parametrize("family", sorted(TRACE))
def test_schedule_on_the_reference_trace(family):
    iters, calls = TRACE[family]["iters"], TRACE[family]["calls"]
    blocks = [c for c in calls if c.startswith("update_block")]
    assert len(blocks) == sum(iters) and len(calls) - len(blocks) == sum(iters) + len(iters) - 1
    skip, _m = _skip(list(iters))
    got = drive(skip, calls)
    assert got == expected(iters, calls)
    assert got.count("live") == len(iters) and got.count("kernel") == 2 * len(iters) - 1
    assert skip.armed and skip.block_calls == sum(iters) and skip.masks_skipped == sum(iters) - len(iters)
    # a second forward re-arms from the pre-hook and gives the same schedule
    assert drive(skip, calls) == got


def test_stand_in_loops_call_what_the_reference_calls():
    """tests/ms_loop_model.py against the recorded trace: the same sequence of block and upsample calls for the same `iters`"""
    from ms_loop_model import MsLoopModel
    for family, style in (("ccmr", "ccmr"), ("ms_raft_plus", "ms_raft")):
        iters = TRACE[family]["iters"]
        model = MsLoopModel(style, iters).eval()
        names = []

        def block(net, inp, corr, flow, *a, **k):
            names.append("update_block")
            B, _, H, W = net.shape
            return net, net.new_zeros(B, 36, H, W), net.new_zeros(B, 2, H, W)

        def upsample_flow(flow, mask, scale=8):
            assert scale == 2
            names.append("upsample_flow")
            return flow.new_zeros(flow.shape[0], 2, 2 * flow.shape[2], 2 * flow.shape[3])

        model.update_block.forward = block
        model.upsample_flow = upsample_flow
        with torch.no_grad():
            out = model({"images": torch.rand(1, 2, 3, 64, 96)})
        assert set(out) == {"flows", "flow_small"}
        assert names == [c.split()[0] for c in TRACE[family]["calls"]], family


def _calls(iters, h=4, w=6):
    """the loops' call pattern for `iters`"""
    calls = []
    for k, n in enumerate(iters):
        size = f"{h << k}x{w << k}"
        for i in range(n):
            if k >= 1 and i == 0:
                calls.append(f"upsample_flow {h << (k - 1)}x{w << (k - 1)}")
            calls += [f"update_block {size}", f"upsample_flow {size}"]
    return calls


def test_counters_and_one_iteration_scales():
    skip, _m = _skip([2, 3, 2])
    got = drive(skip, _calls((2, 3, 2)))
    assert (skip.block_calls, skip.masks_skipped) == (7, 4)
    assert got.count("scratch") == 4 and got.count("kernel") == 5
    skip, _m = _skip((1, 2, 1, 2))
    got = drive(skip, _calls((1, 2, 1, 2)))
    assert got == expected((1, 2, 1, 2), _calls((1, 2, 1, 2))) and got[0] == "live" and skip.masks_skipped == 2


def test_a_changed_iters_is_read_at_the_next_forward():
    skip, model = _skip([2, 3, 2])
    drive(skip, _calls((2, 3, 2)))
    model.iters = [1, 1, 3]
    got = drive(skip, _calls((1, 1, 3)))
    assert got == expected((1, 1, 3), _calls((1, 1, 3))) and skip.masks_skipped == 2


def _all_computed(got):
    return "dead" not in got and "scratch" not in got


def test_not_armed_without_its_conditions():
    calls = _calls((2, 3, 2))
    skip, model = _skip([2, 3, 2])
    assert _all_computed(drive(skip, calls, fp32=False)) and not skip.armed                  # a bf16 model
    model.train()
    assert _all_computed(drive(skip, calls)) and not skip.armed
    model.eval()
    assert _all_computed(drive(skip, calls, hook=False)) and not skip.armed                  # no pre-hook, nothing to count from
    assert "dead" in drive(skip, calls)
    with torch.enable_grad():
        skip.start_forward()
        skip.begin_forward(fp32=True, device=torch.device("cpu"), grid=(4, 6))
        assert skip.next_call() is False and not skip.armed
    for iters in (7, [], [2, 0, 1], [2, True, 1], [2.0, 1], None):
        skip, _m = _skip(iters)
        assert _all_computed(drive(skip, calls)) and not skip.armed, iters
    for ok2 in (False, None):                                                               # refused probe; no verdict yet (capture)
        skip, _m = _skip([2, 3, 2], ok2=ok2)
        assert _all_computed(drive(skip, calls)) and not skip.armed and skip._keep[1].probes == 1


def test_inconsistent_bookkeeping_disarms_for_the_rest_of_the_forward():
    # a scale that begins before the previous one had its iters[k] calls
    skip, model = _skip([2, 3, 2])
    got = drive(skip, _calls((2, 2, 2)))
    # ... its first `upsample_flow` is the SECOND reader of a dead call's mask: never a scratch answer, the mask is computed after all
    assert got[:10] == ["dead", "scratch", "live", "kernel", "kernel", "dead", "scratch", "dead", "scratch", "kernel"]
    assert model.update_block.filled == 1 and _all_computed(got[10:]) and not skip.armed
    # a grid that is not twice the previous scale's
    skip, _m = _skip([2, 3, 2])
    calls = _calls((2,)) + ["upsample_flow 4x6"] + ["update_block 8x13", "upsample_flow 8x13"] * 3
    got = drive(skip, calls)
    assert _all_computed(got[5:]) and not skip.armed
    # more scales than len(iters)
    skip, _m = _skip([1, 1])
    got = drive(skip, _calls((1, 1, 2)))
    assert _all_computed(got) and not skip.armed
    # more block calls in a scale than iters[k]
    skip, _m = _skip([2, 1])
    got = drive(skip, ["update_block 4x6", "upsample_flow 4x6"] * 4)
    assert got[:4] == ["dead", "scratch", "live", "kernel"] and _all_computed(got[4:]) and not skip.armed
    # the next pre-hook re-arms
    assert "dead" in drive(skip, _calls((2, 1))) and skip.armed


def test_nothing_is_dead_outside_a_forward():
    """a forward that died on a dead block call: its post-hook (always called) clears the state, so a direct `upsample_flow` from user
    code is never answered with the scratch tensor"""
    skip, _m = _skip([2, 3, 2])
    got = drive(skip, _calls((2, 3, 2))[:1])
    assert got == ["dead"] and skip.upsample_is_dead()
    skip.end_forward()
    assert not skip.upsample_is_dead() and not skip.armed
    assert drive(skip, _calls((2, 3, 2))) == expected((2, 3, 2), _calls((2, 3, 2)))      # the next forward arms again


# ---------------------------------------------------------------------------------------------------------------------
# acceptance and refusal on the reference's classes
# ---------------------------------------------------------------------------------------------------------------------
def _attempt(model, **kw):
    from ptlflow_amd import patch
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        patch.accelerate(model, multiscale_upsample=True, skip_dead_upsample=True, **kw)
    try:
        skip = model.__dict__.get(patch._SKIP)
        hooks = skip is not None and skip._hook is not None and skip._hook.id in model._forward_pre_hooks
        return skip, hooks, [str(x.message) for x in w if "skip_dead_upsample refused" in str(x.message)]
    finally:
        patch.restore(model)
        assert patch._SKIP not in model.__dict__ and "upsample_flow" not in model.__dict__


@pytest.mark.reference
def test_accepted_and_refused_on_the_reference_classes():
    from oracle import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("needs the reference tree")
    import ptlflow_amd
    from ptlflow_amd import patch
    ptlflow_amd.load_native()
    C = ref_loader.ref_module("ptlflow.models.ccmr.ccmr")
    M = ref_loader.ref_module("ptlflow.models.ms_raft_plus.ms_raft_plus")
    for cls in (C.CCMR, C.CCMRPlus, M.MSRAFTPlus):
        torch.manual_seed(7)
        model = cls().eval()
        before = len(model._forward_pre_hooks)
        skip, hooks, warned = _attempt(model)
        assert isinstance(skip, patch._MultiScaleSkip) and not warned and hooks, cls.__name__
        assert len(model._forward_pre_hooks) == before                          # restore() removed the pre-hook
        # skip_dead_upsample=False keeps every iteration's mask head and upsampling (on the kernel): no schedule object
        patch.accelerate(model, multiscale_upsample=True, skip_dead_upsample=False)
        assert patch._SKIP not in model.__dict__ and model.__dict__["upsample_flow"].multiscale
        # ... and a second call switches
        patch.accelerate(model, multiscale_upsample=True)
        assert isinstance(model.__dict__.get(patch._SKIP), patch._MultiScaleSkip)
        patch.accelerate(model)
        assert patch._SKIP not in model.__dict__ and not model.__dict__["upsample_flow"].multiscale
        patch.restore(model)

    class OwnForward(C.CCMR):
        def forward(self, inputs):
            return super().forward(inputs)

    class OwnUpsample(M.MSRAFTPlus):
        def upsample_flow(self, flow, mask, scale=8):
            return super().upsample_flow(flow, mask, scale=scale)

    torch.manual_seed(7)
    skip, _h, warned = _attempt(OwnForward().eval())
    assert skip is None and len(warned) == 1 and "forward" in warned[0]
    skip, _h, warned = _attempt(OwnUpsample().eval())
    assert skip is None and len(warned) == 1 and "upsample_flow" in warned[0]
    skip, _h, warned = _attempt(C.CCMR().train())
    assert skip is None and len(warned) == 1 and "train mode" in warned[0]
    for iters in (12, [], [8, 0, 15], [8, True, 15]):
        model = C.CCMR().eval()
        model.iters = iters
        skip, _h, warned = _attempt(model)
        assert skip is None and len(warned) == 1 and "iters" in warned[0], iters
    # without the option the multi-scale classes are refused as before
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model = patch.accelerate(C.CCMR().eval(), skip_dead_upsample=True)
    assert patch._SKIP not in model.__dict__ and any("skip_dead_upsample refused" in str(x.message) for x in w)
    patch.restore(model)


def test_seam_on_cpu_tensors_reaches_the_original_without_a_probe():
    from ptlflow_amd.patch import _UpsampleSeam
    calls = []

    def original(flow, mask, scale=8):
        calls.append(scale)
        return flow * scale

    seam = _UpsampleSeam(original)
    seam.multiscale = True
    f, m = torch.ones(1, 2, 3, 4), torch.zeros(1, 36, 3, 4)
    assert torch.equal(seam(f, m, scale=2), f * 2) and torch.equal(seam(f, m, 2), f * 2) and torch.equal(seam(f, m, scale=4), f * 4)
    assert calls == [2, 2, 4] and seam.ok is None and seam.ok2 is None and seam.calls == 0
