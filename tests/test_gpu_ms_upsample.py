"""`accelerate(model, multiscale_upsample=True)` on the GPU: the x2 convex-upsampling kernel against float64 on its
own inputs and against outputs recorded from the reference's `upsample_flow(scale=2)`; seam B5's dispatch of `scale=2` calls; and
the per-scale dead-work skip on the stand-in loops of tests/ms_loop_model.py (and on the reference's own classes where the staged
reference is present): skip on against `skip_dead_upsample=False` bit for bit, option on against option off within BLOCK_TOL."""
import copy
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

from op_gate import BLOCK_TOL, GUARD, OP_TOL, SENTINEL, close, pm, rel, scale_close

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ms_upsample.pt")
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
def ref64(flow, mask):
    """softmax over the nine taps of mask [N, 36 = 9 x 2 x 2, H, W], convex combination of the zero-padded 3x3 neighbourhood of
    2 * flow, sub-pixels interleaved to [N, 2, 2H, 2W]; float64"""
    N, _, H, W = flow.shape
    w = torch.softmax(mask.double().view(N, 1, 9, 2, 2, H, W), dim=2)
    nb = F.unfold(2 * flow.double(), [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    return (w * nb).sum(dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 2 * H, 2 * W)


def out_buffer(shape, gpu, shift=0):
    """a contiguous output in the middle of a sentinel-filled flat buffer (`shift` floats off its 256-byte alignment)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD + shift,), SENTINEL, device=gpu)
    return flat, flat[GUARD + shift: GUARD + shift + n].view(shape)


def guards_kept(flat, out, shift=0):
    n = out.numel()
    return bool((flat[:GUARD + shift] == SENTINEL).all()) and bool((flat[GUARD + shift + n:] == SENTINEL).all())


def run(flow, mask, gpu, mask_ld=36, mask_off=0, flow_pm=False, shift=0):
    """the kernel on mask rows of stride `mask_ld` starting `mask_off` floats into their buffer (NaN everywhere else), the flow NCHW or
    as a two-column slice of NaN-filled pixel-major rows, the output between sentinels"""
    B, _, H, W = flow.shape
    M = B * H * W
    buf = torch.full((M, mask_ld + mask_off), NAN, device=gpu)[:, mask_off:] if mask_off else torch.full((M, mask_ld), NAN, device=gpu)
    rows = buf[:, :36]
    rows.copy_(pm(mask, gpu))
    flat, out = out_buffer((B, 2, 2 * H, 2 * W), gpu, shift)
    if flow_pm:
        fbuf = torch.full((M, 7), NAN, device=gpu)
        fbuf[:, 3:5] = pm(flow, gpu)
        torch.ops.pfk.convex_upsample2_pm(fbuf[:, 3:5], rows, out)
    else:
        torch.ops.pfk.convex_upsample2(flow.to(gpu), rows, out)
    torch.cuda.synchronize()
    assert guards_kept(flat, out, shift), "memory around the output was written"
    return out


def inputs(B, H, W, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 2, H, W, generator=g) * 3, torch.randn(B, 36, H, W, generator=g) * spread


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 7), (1, 3, 65), (3, 4, 6)])
def test_kernel_against_float64(gpu, B, H, W):
    """1x3x65: a row longer than a wave's 32-pixel group, ragged; 3x4x6: a group that spans images"""
    flow, mask = inputs(B, H, W, 100 + H)
    want = ref64(flow, mask)
    out = run(flow, mask, gpu)
    r = rel(out, want)
    print(f"{B}x{H}x{W}: relL2 {r:.2e}")
    assert r <= OP_TOL
    close(out, want, rtol=1e-5, atol=1e-5)
    assert torch.equal(run(flow, mask, gpu), out), "a second run gave other bits"
    # every layout of the same values gives the same bits: padded rows (the pad columns hold NaN), a row view into a wider buffer on
    # an 8-byte and on a 4-byte boundary, an odd row stride, an output off its 8-byte alignment, pixel-major flow from a slice
    for what, kw in (("mask_ld 40", dict(mask_ld=40)), ("view at +10 of 64", dict(mask_ld=54, mask_off=10)),
                     ("view at +5 of 48", dict(mask_ld=43, mask_off=5)), ("mask_ld 37", dict(mask_ld=37)), ("out + 4 bytes", dict(shift=1)),
                     ("pixel-major flow", dict(flow_pm=True)), ("pixel-major flow, mask_ld 40", dict(flow_pm=True, mask_ld=40))):
        assert torch.equal(run(flow, mask, gpu, **kw), out), what


def test_kernel_saturated_and_infinite_logits(gpu):
    flow, mask = inputs(2, 5, 7, 7, spread=60.0)
    out = run(flow, mask, gpu)
    assert rel(out, ref64(flow, mask)) <= OP_TOL
    close(out, ref64(flow, mask), rtol=1e-5, atol=1e-5)
    # -inf in eight of the nine taps: the ninth has weight one, the output is exactly 2 * that neighbour (zero outside the image)
    for keep in (0, 4, 8):
        m = torch.full((2, 9, 4, 5, 7), float("-inf"))
        m[:, keep] = mask.view(2, 9, 4, 5, 7)[:, keep]
        m = m.view(2, 36, 5, 7)
        out = run(flow, m, gpu)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out.cpu(), ref64(flow, m).float()), f"tap {keep}"


def test_kernel_keeps_images_apart(gpu):
    """NaN flow and NaN logits in image 1 never reach image 0"""
    flow, mask = inputs(2, 4, 6, 9)
    clean = run(flow, mask, gpu)
    flow[1], mask[1] = NAN, NAN
    for kw in (dict(), dict(flow_pm=True)):
        out = run(flow, mask, gpu, **kw)
        assert torch.equal(out[0], clean[0]) and bool(torch.isnan(out[1]).all())


def test_kernel_against_the_reference_recording(gpu):
    """tests/golden/ms_upsample.pt: `CCMR.upsample_flow` / `MSRAFTPlus.upsample_flow` at scale=2 (scripts/make_golden_ms_upsample.py)"""
    gold = torch.load(GOLDEN)
    assert set(gold["cases"]) == {"random", "saturated"}
    for name, case in gold["cases"].items():
        out = run(case["flow"], case["mask"], gpu)
        for key in ("ccmr", "ms_raft_plus"):
            close(out, case[key], rtol=1e-5, atol=1e-5)
            assert rel(out, case[key]) <= OP_TOL, (name, key)


def test_binding_refuses_wrong_views(gpu):
    flow, mask = inputs(2, 5, 7, 3)
    rows, out = pm(mask, gpu), torch.empty(2, 2, 10, 14, device=gpu)
    for bad in (lambda: torch.ops.pfk.convex_upsample2(flow.to(gpu), rows[:, :35], out),
                lambda: torch.ops.pfk.convex_upsample2(flow.to(gpu), rows[:-1], out),
                lambda: torch.ops.pfk.convex_upsample2(flow.to(gpu), rows, torch.empty(2, 2, 10, 15, device=gpu)),
                lambda: torch.ops.pfk.convex_upsample2(flow[:, :, :4].to(gpu), rows, out),
                lambda: torch.ops.pfk.convex_upsample2_pm(pm(flow, gpu)[:, :1], rows, out),
                lambda: torch.ops.pfk.convex_upsample2(flow.to(gpu), rows.bfloat16(), out)):
        with pytest.raises(RuntimeError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------
# seam B5
# ---------------------------------------------------------------------------------------------------------------------
class _Host(torch.nn.Module):
    """a model with the loops' `upsample_flow(flow, mask, scale=8)` that counts the calls reaching it"""

    def __init__(self):
        super().__init__()
        self.reached = []

    def upsample_flow(self, flow, mask, scale=8):
        from ms_loop_model import MsLoopModel
        self.reached.append(scale)
        return MsLoopModel.upsample_flow(self, flow, mask, scale=scale)


def _seam(host, on=True):
    from ptlflow_amd.patch import _UpsampleSeam
    seam = _UpsampleSeam(host.upsample_flow)
    seam.multiscale = on
    return seam


def test_seam_serves_scale_2(gpu):
    host = _Host().eval()
    seam = _seam(host)
    flow, mask = (t.to(gpu) for t in inputs(2, 5, 7, 21))
    want = ref64(flow.cpu(), mask.cpu())
    with torch.no_grad():
        a = seam(flow, mask, scale=2)
        assert seam.ok2 is True and seam.ok is None and host.reached == [2]       # the x2 probe alone ran, once, on the method
        b = seam(flow, mask, 2)
    assert seam.calls == 2 and host.reached == [2]
    assert torch.equal(a, b)
    close(a, want, rtol=1e-5, atol=1e-5)
    # the update block's own view: channels-last strides, served without a copy, same bits
    view = pm(mask).to(gpu).view(2, 5, 7, 36).permute(0, 3, 1, 2)
    with torch.no_grad():
        assert torch.equal(seam(flow, view, scale=2), a)
    assert seam.calls == 3 and host.reached == [2]
    # a plain NCHW mask of ONE image (its pixel-major reshape would be a view with strided channels: the seam must copy)
    f1, m1 = (t.to(gpu) for t in inputs(1, 5, 7, 24))
    with torch.no_grad():
        close(seam(f1, m1, scale=2), ref64(f1.cpu(), m1.cpu()), rtol=1e-5, atol=1e-5)
    assert seam.calls == 4 and host.reached == [2]


def test_seam_leaves_everything_else_to_the_model(gpu):
    host = _Host().eval()
    seam = _seam(host)
    flow, mask = (t.to(gpu) for t in inputs(2, 5, 7, 22))
    g = torch.Generator().manual_seed(1)
    mask4, mask8 = torch.randn(2, 144, 5, 7, generator=g).to(gpu), torch.randn(2, 576, 5, 7, generator=g).to(gpu)
    with torch.no_grad():
        seam(flow, mask, scale=2)
        host.reached.clear()
        n = seam.calls
        assert seam(flow, mask4, scale=4).shape == (2, 2, 20, 28)
        assert seam(flow, mask8, scale=8).shape == (2, 2, 40, 56)
        assert seam(flow.cpu(), mask.cpu(), scale=2).device.type == "cpu"
        with pytest.raises(RuntimeError):
            seam(flow, mask[:, :35], scale=2)                                     # a 35-channel mask: the method's own error
        assert host.reached == [4, 8, 2, 2] and seam.calls == n
    host.reached.clear()
    leaf = flow.clone().requires_grad_()
    out = seam(leaf, mask, scale=2)                                               # a gradient graph
    assert out.requires_grad and host.reached == [2] and seam.calls == n
    host.train()
    with torch.no_grad():
        seam(flow, mask, scale=2)                                                 # train mode
        host.eval()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            seam(flow, mask, scale=2)                                             # autocast
    assert host.reached == [2, 2, 2] and seam.calls == n
    off = _seam(host, on=False)                                                   # the option off: today's path, no probe
    host.reached.clear()
    with torch.no_grad():
        off(flow, mask, scale=2)
        off(flow, mask, 2)
    assert host.reached == [2, 2] and off.ok2 is None and off.calls == 0


def test_seam_probe_refuses_another_method(gpu):
    class Other(torch.nn.Module):
        def upsample_flow(self, flow, mask, scale=8):
            return scale * F.interpolate(flow, scale_factor=scale, mode="bilinear", align_corners=True)

    host = Other().eval()
    seam = _seam(host)
    flow, mask = (t.to(gpu) for t in inputs(2, 5, 7, 23))
    with warnings.catch_warnings(record=True) as w, torch.no_grad():
        warnings.simplefilter("always")
        out = seam(flow, mask, scale=2)
        seam(flow, mask, scale=2)
    assert seam.ok2 is False and seam.calls == 0
    assert torch.equal(out, host.upsample_flow(flow, mask, scale=2))
    said = [str(x.message) for x in w if "upsample_flow" in str(x.message)]
    assert len(said) == 1 and "scale=2" in said[0] and "8x" not in said[0]      # the x2 verdict's own message


# ---------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------
CASES = [("ccmr", (2, 3, 2)), ("ccmr", (1, 2, 1, 2)), ("ms_raft", (2, 3, 2)), ("ms_raft", (1, 2, 1, 2))]
_RUNS = {}


def images(gpu, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, 2, 3, 64, 96, generator=g).to(gpu)


# Every configuration runs the encoders on the kernels (`multiscale_encoders=True`): the stock torch encoders do not repeat their own
# bits on this GPU (the same module on the same input twice: feature maps 5e-6 apart, the every-iteration flow 2e-5 apart from run
# to run, measured), and a bit-for-bit comparison needs a substrate that does.
ENC = dict(multiscale_encoders=True)


def fresh(style, iters, gpu):
    from ms_loop_model import MsLoopModel
    model = MsLoopModel(style, iters).eval().to(gpu)
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def forward(model, x):
    with torch.no_grad():
        out = model({"images": x})
    return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}


def runs(style, iters, gpu):
    """one forward per configuration, computed once per (style, iters) and shared: option off, option on with every iteration's mask
    head and upsampling, option on with the skip (and its counters)"""
    key = (style, iters)
    if key not in _RUNS:
        from ptlflow_amd import patch
        x = images(gpu)
        res = {}
        for name, kw in (("off", {}), ("every", dict(multiscale_upsample=True, skip_dead_upsample=False)),
                         ("skip", dict(multiscale_upsample=True))):
            model = patch.accelerate(fresh(style, iters, gpu), **ENC, **kw)
            res[name] = forward(model, x)
            seam, skip = model.__dict__["upsample_flow"], model.__dict__.get(patch._SKIP)
            res[name + " calls"] = seam.calls
            if skip is not None:
                res[name + " counters"] = (skip.block_calls, skip.masks_skipped, skip.scratch_answers)
            patch.restore(model)
        _RUNS[key] = res
    return _RUNS[key]


@pytest.mark.parametrize("style,iters", CASES)
def test_loop_skip_is_bit_identical_and_option_is_close(gpu, style, iters):
    r = runs(style, iters, gpu)
    for k in ("flows", "flow_small"):
        assert bool(torch.isfinite(r["every"][k]).all()) and float(r["every"][k].abs().max()) > 1e-3
        assert torch.equal(r["skip"][k], r["every"][k]), f"{k}: the skip changed the result"
        scale_close(r["every"][k], r["off"][k], f"{style} {iters} {k}: option on against off", BLOCK_TOL)
    n, s = sum(iters), len(iters)
    assert r["off calls"] == 0 and "off counters" not in r and "every counters" not in r
    assert r["every calls"] == n + s - 1 and r["skip calls"] == n + s - 1
    assert r["skip counters"] == (n, n - s, n - s)


def test_loop_counters(gpu):
    r = runs("ccmr", (2, 3, 2), gpu)
    assert r["skip counters"] == (7, 4, 4) and r["skip calls"] == 9


@pytest.mark.parametrize("style", ["ccmr", "ms_raft"])
def test_loop_skips_nothing_outside_its_conditions(gpu, style):
    from ptlflow_amd import patch
    iters = (2, 3, 2)
    x = images(gpu)
    model = patch.accelerate(fresh(style, iters, gpu), multiscale_upsample=True, **ENC)
    skip, seam = model.__dict__[patch._SKIP], model.__dict__["upsample_flow"]
    want = runs(style, iters, gpu)["every"]
    # grad mode on (nothing requires grad: the kernels still serve)
    out = model({"images": x})
    assert (skip.block_calls, skip.masks_skipped, skip.scratch_answers) == (7, 0, 0)
    scale_close(out["flows"], want["flows"], "grad mode on", BLOCK_TOL)      # (the encoders run in torch there: close, not equal)
    # train mode: every prediction is returned
    model.train()
    with torch.no_grad():
        out = model({"images": x})
    assert (skip.masks_skipped, skip.scratch_answers) == (0, 0) and len(out["flow_preds"]) == 7
    model.eval()
    # armed again by the next forward's pre-hook
    out = forward(model, x)
    assert skip.masks_skipped == 4 and torch.equal(out["flows"], want["flows"])
    # a bf16 model (last: the cast rounds the parameters)
    n = seam.calls
    model.bfloat16()
    with torch.no_grad():
        out = model({"images": x.bfloat16()})
    assert (skip.block_calls, skip.masks_skipped, skip.scratch_answers) == (7, 0, 0) and seam.calls == n
    assert bool(torch.isfinite(out["flows"]).all())
    patch.restore(model)


def test_loop_honours_a_changed_iters(gpu):
    from ptlflow_amd import patch
    x = images(gpu)
    model = patch.accelerate(fresh("ms_raft", (2, 3, 2), gpu), multiscale_upsample=True, **ENC)
    skip = model.__dict__[patch._SKIP]
    forward(model, x)
    model.iters = [1, 2, 1]
    got = forward(model, x)
    assert (skip.block_calls, skip.masks_skipped, skip.scratch_answers) == (4, 1, 1)
    patch.restore(model)
    every = patch.accelerate(fresh("ms_raft", (1, 2, 1), gpu), multiscale_upsample=True, skip_dead_upsample=False, **ENC)
    want = forward(every, x)
    assert torch.equal(got["flows"], want["flows"]) and torch.equal(got["flow_small"], want["flow_small"])


def test_loop_recovers_from_an_aborted_forward(gpu):
    """a forward that dies in the middle of a scale leaves no state behind: the next one gives a fresh model's bits"""
    from ptlflow_amd import patch
    x = images(gpu)
    model = patch.accelerate(fresh("ccmr", (2, 3, 2), gpu), multiscale_upsample=True, **ENC)
    seen = []

    class Abort(Exception):
        pass

    def hook(_m, _args, _out):
        seen.append(1)
        if len(seen) == 4:          # the second call of scale 1: a dead one
            raise Abort()

    h = model.update_block.register_forward_hook(hook)
    with pytest.raises(Abort), torch.no_grad():
        model({"images": x})
    h.remove()
    got = forward(model, x)
    want = runs("ccmr", (2, 3, 2), gpu)["skip"]
    assert torch.equal(got["flows"], want["flows"]) and torch.equal(got["flow_small"], want["flow_small"])
    skip = model.__dict__[patch._SKIP]
    assert (skip.block_calls, skip.masks_skipped, skip.scratch_answers) == (7, 4, 4)


@pytest.mark.parametrize("style,size,iters,short,at", [("ccmr", (64, 96), (2, 3, 2), 1, 2), ("ms_raft", (64, 96), (1, 3, 2), 1, 2),
                                                       ("ms_raft", (448, 1024), (1, 1, 3, 1), 2, 2)])
def test_loop_scale_that_ends_early_gets_its_mask_after_all(gpu, style, size, iters, short, at):
    """`model.iters[short]` shrinks to `at` in mid-forward, after the schedule read it: scale `short` ends on a call the schedule held
    for dead, and the next scale's first `upsample_flow` is a second reader of that call's mask.  The block computes it after all
    (`PfkUpdateBlock.fill_mask`) and nothing more is skipped: the forward equals the every-iteration forward with the counts the loop
    really ran, bit for bit.  Once at small grids and once where the early scale has 112 x 256 = 28 672 pixels (from
    `SMALL_GRID_PIXELS` up the update engine's launches take their large-grid forms, fh|mask conv1 the Winograd kernel)."""
    from ptlflow_amd import patch
    from ptlflow_amd.update import SMALL_GRID_PIXELS
    g = torch.Generator().manual_seed(8)
    B = 2 if size == (64, 96) else 1
    x = torch.rand(B, 2, 3, *size, generator=g).to(gpu)
    ran = list(iters)
    ran[short] = at
    every = patch.accelerate(fresh(style, ran, gpu), multiscale_upsample=True, skip_dead_upsample=False, **ENC)
    want = forward(every, x)
    model = patch.accelerate(fresh(style, iters, gpu), multiscale_upsample=True, **ENC)
    skip = model.__dict__[patch._SKIP]
    fills, grids = [], []
    fill = model.update_block.fill_mask
    model.update_block.fill_mask = lambda: (fills.append(1), fill())[1]

    def shrink(_m, args, _out):
        grids.append(args[0].shape[0] * args[0].shape[2] * args[0].shape[3])
        model.iters[short] = at          # (the loop reads iters[k] when scale k begins; the schedule read it at the pre-hook)

    h = model.update_block.register_forward_hook(shrink)
    got = forward(model, x)
    h.remove()
    assert len(fills) == 1 and len(grids) == sum(ran) and not skip.armed
    early = grids[sum(ran[:short])]
    assert (early >= SMALL_GRID_PIXELS) == (size != (64, 96)), early
    assert skip.masks_skipped == sum(n - 1 for n in ran[:short]) + at and skip.scratch_answers == skip.masks_skipped
    for k in ("flows", "flow_small"):
        assert torch.equal(got[k], want[k]), f"{k}: the recovered mask changed the result"
    # a direct call outside a forward is computed, never the scratch
    flow, mask = (t.to(gpu) for t in inputs(1, 5, 7, 2))
    with torch.no_grad():
        close(model.upsample_flow(flow, mask, scale=2), ref64(flow.cpu(), mask.cpu()), rtol=1e-5, atol=1e-5)
    patch.restore(model)


def test_restore_removes_hook_and_state(gpu):
    from ptlflow_amd import patch
    from ptlflow_amd.update import PfkUpdateBlock
    model = fresh("ccmr", (2, 3, 2), gpu)
    before = len(model._forward_pre_hooks)
    patch.accelerate(model, multiscale_upsample=True)
    skip = model.__dict__[patch._SKIP]
    assert isinstance(skip, patch._MultiScaleSkip) and skip._hook.id in model._forward_pre_hooks
    assert model.update_block._skip is skip and model.__dict__["upsample_flow"].skip is skip
    patch.restore(model)
    assert patch._SKIP not in model.__dict__ and "upsample_flow" not in model.__dict__ and skip._hook is None
    assert len(model._forward_pre_hooks) == before and not isinstance(model.update_block, PfkUpdateBlock)
    x = images(gpu)
    assert forward(model, x)["flows"].shape == (2, 1, 2, 64, 96)          # the plain torch model again


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own classes (staged reference only)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ccmr", "ms_raft_plus"])
def test_reference_models(gpu, family):
    from oracle import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("no reference: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference tree exists; it stages "
                    "oracle/_ref/ for the GPU box")
    from ptlflow_amd import patch
    if family == "ccmr":
        M = ref_loader.ref_module("ptlflow.models.ccmr.ccmr")
        make, iters, kw = (lambda: M.CCMR(iters=[2, 2, 2])), (2, 2, 2), dict(ccmr_aggregator=True, **ENC)
    else:
        M = ref_loader.ref_module("ptlflow.models.ms_raft_plus.ms_raft_plus")
        make, iters, kw = (lambda: M.MSRAFTPlus(iters=(1, 2, 1, 2))), (1, 2, 1, 2), dict(ENC)
    torch.manual_seed(1234)
    base = make().eval()
    g = torch.Generator().manual_seed(6)
    x = torch.rand(1, 2, 3, 128, 192, generator=g).to(gpu)
    res = {}
    # CCMR's per-scale self-attention `model.xcit[i]` stays the reference's torch module, and on this GPU its fp32 forward does not repeat
    # its own bits (the same module on bit-identical inputs twice: outputs 9.5e-7 and 1.4e-6 apart, measured; the whole every-iteration
    # forward then differs by 5e-6 from run to run).  So, as tests/test_gpu_xcit.py does for the aggregators, the modules' outputs of the
    # every-iteration run are recorded, and in the run with the skip each call must arrive with bit-identical inputs and gets the
    # recorded output back: everything the option itself does must then be equal bit for bit.
    tape = {"mode": None, "calls": [], "at": 0}

    def replay(_m, inputs, output):
        if tape["mode"] == "every":
            tape["calls"].append(([t.clone() for t in inputs], output.clone()))
        elif tape["mode"] == "skip":
            want_in, want_out = tape["calls"][tape["at"]]
            tape["at"] += 1
            assert all(torch.equal(a, b) for a, b in zip(inputs, want_in)), "a context module's inputs differ from the every-iteration run's"
            return want_out.clone()
        return None

    for name, opts in (("off", {}), ("every", dict(multiscale_upsample=True, skip_dead_upsample=False)), ("skip", dict(multiscale_upsample=True))):
        model = patch.accelerate(copy.deepcopy(base).to(gpu), **kw, **opts)
        handles = [m.register_forward_hook(replay) for m in getattr(model, "xcit", [])]
        tape["mode"] = name
        res[name] = forward(model, x)
        for h in handles:
            h.remove()
        if name == "skip":
            skip = model.__dict__[patch._SKIP]
            n, s = sum(iters), len(iters)
            assert (skip.block_calls, skip.masks_skipped, skip.scratch_answers) == (n, n - s, n - s)
            assert model.__dict__["upsample_flow"].calls == n + s - 1
        patch.restore(model)
    assert tape["at"] == len(tape["calls"]) == (len(iters) if family == "ccmr" else 0)
    for k in ("flows", "flow_small"):
        assert torch.equal(res["skip"][k], res["every"][k]), f"{k}: the skip changed the result"
        scale_close(res["every"][k], res["off"][k], f"{family} {k}: option on against off", BLOCK_TOL)
