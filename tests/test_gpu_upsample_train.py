"""Training through the upsampling seams (K12e): the backward of SEA-RAFT's `upsample_data` (`pfk_convex_upsample_info_bwd_pm_f32`), the
autograd node on it (`train_sea.upsample_data_train`) and `accelerate(model, train_upsample=True)` on seam B5 and on `upsample_data`.

Kernel gates: 1-4 of tests/op_gate.py's docstring, with its harness.  The reference is float64 autograd through
`sea_seam_model.upsample_data_torch` on the kernel's own fp32 inputs.  The per-element bounds are `convex_case`'s derivation with
C = 2 + n_info channels in place of 2: a softmax weight is off by at most k_w = 2 spread + 19 units of 2^-24 relative; dw_k = sum_c g_c
v_c,k has C products and C - 1 additions, 2C - 1 roundings where the two-channel kernel has 3, so
    K_mask = 2 (2 spread + 19) + 12 + (2C - 1)          (C = 2: the existing 15)
on the magnitudes w_k (T_k + sum_j w_j T_j), T_k = sum_c |g_c| |v_c,k|, and
    K_flow = 9 * 64 + max(2 spread + 19) + 2
on the float64 gradient of the same loss with |g| in place of g (the weights are >= 0), for the flow and the info rows alike.
Nodes and seams: 5e-4 of each tensor's scale (`scale_close`, `BLOCK_TOL`) against the torch stand-ins in float64.

Measured on an MI355X, worst over the cases of each test (relative L2 | error as a fraction of the per-element bound):
  test_info_bwd_kernel               grad_mask 1.2e-7 | 0.131 (logits x 40: 4.1e-7 | 0.196)     grad_flow 1.4e-7 | 0.001     grad_info 1.2e-7 | 0.001
  test_agrees_with_raft_reference    grad_mask 9.5e-8 | 0.128 (logits x 40: 3.5e-7 | 0.211)     grad_flow 1.0e-7 | 0.001
and as a fraction of each tensor's scale: test_upsample_data_node <= 1.7e-7; test_sea_raft_loop_trains_through_upsample_data <= 4.3e-6
(d/dfmap1; parameters <= 2.6e-6); test_raft_loop_trains_through_upsample_flow <= 2.4e-6 on the gradients that have a scale, the
structurally zero biases <= 3.2e-7 of their convolution's weight gradient; two flag-off instances differ by up to 7.3e-6 (flow_small),
and so does one instance run twice (no step of this model in train mode is bit-reproducible).
"""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

from sea_seam_model import upsample_data_torch
from op_gate import BLOCK_TOL, FLOOR, SENTINEL, Rows, gates, pm, scale_close
from op_refs import convex_case

pytestmark = pytest.mark.gpu

# (B, H, W, logit_scale, n_info): H = 1 | W = 1 | M = 234 (no multiple of 4; a batch boundary the neighbourhoods must not cross) |
# a saturated softmax | n_info = 1, 8 (the maximum), 0
CASES = [(2, 1, 5, 1.0, 4), (1, 6, 1, 1.0, 4), (2, 9, 13, 1.0, 4), (2, 9, 13, 40.0, 4), (2, 3, 5, 1.0, 1), (2, 3, 5, 1.0, 8), (2, 3, 5, 1.0, 0)]


@functools.lru_cache(maxsize=None)
def info_case(B, H, W, logit_scale, n):
    """fp32 inputs, the float64 gradients of sum(flow_up * gf) + sum(info_up * gi) and their magnitudes, pixel-major; once per case"""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + n + int(logit_scale))
    C = 2 + n
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    info = torch.randn(B, n, H, W, generator=g)
    mask = torch.randn(B, 576, H, W, generator=g) * logit_scale
    gf = torch.randn(B, 2, 8 * H, 8 * W, generator=g)
    gi = torch.randn(B, n, 8 * H, 8 * W, generator=g)
    f64, m64 = flow.double().requires_grad_(), mask.double().requires_grad_()
    # without info channels the stand-in still wants an info tensor: one zero channel with a zero gradient, which changes no gradient
    i64 = (info.double() if n else torch.zeros(B, 1, H, W, dtype=torch.float64)).requires_grad_()
    gi64 = gi.double() if n else torch.zeros(B, 1, 8 * H, 8 * W, dtype=torch.float64)
    fu, iu = upsample_data_torch(f64, i64, m64)
    gflow, ginfo, gmask = torch.autograd.grad((fu * gf.double()).sum() + (iu * gi64).sum(), (f64, i64, m64), retain_graph=True)
    gflow_mag, ginfo_mag = torch.autograd.grad((fu * gf.double().abs()).sum() + (iu * gi64.abs()).sum(), (f64, i64))
    with torch.no_grad():
        m = m64.view(B, 1, 9, 8, 8, H, W)
        wgt = torch.softmax(m, dim=2)[:, 0]                                                          # [B, 9, 8, 8, H, W]
        spread = (m.amax(2) - m.amin(2))[:, 0]                                                       # [B, 8, 8, H, W]
        v = torch.cat([F.unfold(8 * f64, [3, 3], padding=1).view(B, 2, 9, H, W), F.unfold(i64, [3, 3], padding=1).view(B, -1, 9, H, W)], 1)
        gsub = torch.cat([gf.double(), gi64], 1).view(B, -1, H, 8, W, 8).permute(0, 1, 3, 5, 2, 4).abs()   # [B, C, sy, sx, H, W]
        T = (gsub[:, :, None] * v.abs()[:, :, :, None, None]).sum(1)                                 # [B, 9, 8, 8, H, W]
        gmask_mag = wgt * (T + (wgt * T).sum(1, keepdim=True))
    pm576 = lambda t: pm(t.reshape(B, 576, H, W))
    k_w = 2 * spread + 19
    k_mask = pm576((2 * k_w + 12 + (2 * C - 1))[:, None].expand(B, 9, 8, 8, H, W))
    return {"flow": flow, "info": info, "mask": mask, "gf": gf, "gi": gi, "gmask": pm576(gmask), "gmask_mag": pm576(gmask_mag),
            "gflow": pm(gflow), "gflow_mag": pm(gflow_mag), "ginfo": pm(ginfo)[:, :n], "ginfo_mag": pm(ginfo_mag)[:, :n],
            "k_mask": k_mask, "k_flow": 9 * 64 + float(k_w.max()) + 2}


class InfoRun:
    """one case on the GPU: flow_ld = 4 and info_ld = n + 4 with NaN pads, mask_ld = 580; `run` on fresh sentinel-filled outputs with
    grad_mask_ld = 584 and the gradient rows in ONE [M, 8 + 4] buffer (columns 0..1 and 2..2+n; n <= 6) or in two of their own"""

    def __init__(self, gpu, B, H, W, logit_scale, n):
        self.gpu, self.n, self.M = gpu, n, B * H * W
        self.c = c = info_case(B, H, W, logit_scale, n)
        self.flow = Rows(self.M, 2, gpu, pm(c["flow"]), pad=2)
        self.info = Rows(self.M, n, gpu, pm(c["info"]), pad=4)
        self.mask = Rows(self.M, 576, gpu, pm(c["mask"]))
        self.gf, self.gi = c["gf"].to(gpu), c["gi"].to(gpu)
        assert (self.flow.ld, self.info.ld, self.mask.ld) == (4, n + 4, 580)

    def run(self, shared, grad_info_up="given"):
        M, n, gpu = self.M, self.n, self.gpu
        gmask = Rows(M, 576, gpu, pad=8)
        assert gmask.ld == 584
        if shared:
            bufs = (Rows(M, 8, gpu, pad=4),)
            gflow, ginfo = bufs[0].full[:, :2], bufs[0].full[:, 2:2 + n]
        else:
            bufs = (Rows(M, 2, gpu, pad=2), Rows(M, n, gpu, pad=4))
            gflow, ginfo = bufs[0].rows, bufs[1].rows
        gi = self.gi if isinstance(grad_info_up, str) else grad_info_up
        torch.ops.pfk.convex_upsample_info_bwd(self.flow.rows, self.info.rows, self.mask.rows, self.gf, gi, gmask.rows, gflow, ginfo)
        torch.cuda.synchronize()
        return gmask, bufs, gflow, ginfo

    def untouched(self, gmask, bufs, shared, what):
        gmask.check_untouched(what + " grad_mask")
        if shared:
            b = bufs[0]
            assert bool((b.flat[self.M * b.ld:] == SENTINEL).all()), f"{what}: memory past the shared gradient buffer was written"
            assert bool((b.full[:, 2 + self.n:] == SENTINEL).all()), f"{what}: columns >= {2 + self.n} of the shared gradient buffer were written"
        else:
            bufs[0].check_untouched(what + " grad_flow"), bufs[1].check_untouched(what + " grad_info")


@pytest.mark.parametrize("B,H,W,logit_scale,n", CASES)
def test_info_bwd_kernel(gpu, B, H, W, logit_scale, n):
    r = InfoRun(gpu, B, H, W, logit_scale, n)
    c, shared = r.c, n <= 6
    gmask, bufs, gflow, ginfo = r.run(shared)
    what = f"convex_upsample_info_bwd {(B, H, W)} x{logit_scale:g} n_info {n}"
    r.untouched(gmask, bufs, shared, what)
    gates(what + " grad_mask", gmask.rows, c["gmask"], c["gmask_mag"], c["k_mask"], floor=FLOOR)
    gates(what + " grad_flow", gflow, c["gflow"], c["gflow_mag"], c["k_flow"], floor=FLOOR)
    if n:
        gates(what + " grad_info", ginfo, c["ginfo"], c["ginfo_mag"], c["k_flow"], floor=FLOOR)
    gmask2, bufs2, _, _ = r.run(shared)
    assert torch.equal(gmask2.flat, gmask.flat) and all(torch.equal(a.flat, b.flat) for a, b in zip(bufs2, bufs)), "a second run gives other bits"
    if shared:       # rows of their own: the same bits, nothing written around them
        gmask3, bufs3, gflow3, ginfo3 = r.run(False)
        r.untouched(gmask3, bufs3, False, what + " (own rows)")
        assert torch.equal(gmask3.flat, gmask.flat) and torch.equal(gflow3, gflow) and torch.equal(ginfo3, ginfo)


def test_info_bwd_without_info_gradient(gpu):
    """grad_info_up = None is a zero gradient"""
    r = InfoRun(gpu, 2, 9, 13, 1.0, 4)
    gmask, bufs, _, _ = r.run(True, grad_info_up=None)
    gmask0, bufs0, _, _ = r.run(True, grad_info_up=torch.zeros_like(r.gi))
    r.untouched(gmask, bufs, True, "grad_info_up = None")
    assert torch.equal(gmask.flat, gmask0.flat) and torch.equal(bufs[0].flat, bufs0[0].flat)
    given, _, _, _ = r.run(True)
    assert not torch.equal(gmask.flat, given.flat), "the info gradient does not reach grad_mask"


@pytest.mark.parametrize("logit_scale", [1.0, 40.0])
def test_agrees_with_raft_reference(gpu, logit_scale):
    """n_info = 0 against the float64 reference and bounds that hold `pfk_convex_upsample_bwd_f32` (test_convex_upsample_bwd)"""
    B, H, W = 2, 9, 13
    c, M = convex_case(B, H, W, logit_scale), B * H * W
    flow = Rows(M, 2, gpu, pm(c["flow"]), pad=2)
    none = Rows(M, 0, gpu, torch.empty(M, 0), pad=4)
    mask = Rows(M, 576, gpu, pm(c["mask"]))
    gmask, gflow, ginfo = Rows(M, 576, gpu, pad=8), Rows(M, 2, gpu, pad=2), Rows(M, 0, gpu, pad=4)
    torch.ops.pfk.convex_upsample_info_bwd(flow.rows, none.rows, mask.rows, c["go"].to(gpu), None, gmask.rows, gflow.rows, ginfo.rows)
    torch.cuda.synchronize()
    gmask.check_untouched("grad_mask"), gflow.check_untouched("grad_flow")
    assert bool((ginfo.flat == SENTINEL).all()), "n_info = 0 but the info gradient buffer was written"
    what = f"convex_upsample_info_bwd n_info 0 x{logit_scale:g} vs RAFT's reference"
    gates(what + " grad_mask", gmask.rows, c["gmask"], c["gmask_mag"], c["k_mask"], floor=FLOOR)
    gates(what + " grad_flow", gflow.rows, pm(c["gflow"]), pm(c["gflow_mag"]), c["k_flow"], floor=FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# the autograd node
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_on", ["both", "flow", "info"])
def test_upsample_data_node(gpu, loss_on):
    """flow / info as channel slices of one channels-last [1, 6, 7, 8] tensor and a channels-last mask, the way the loop passes them"""
    from ptlflow_amd.train_sea import upsample_data_train
    g = torch.Generator().manual_seed(17)
    B, H, W = 1, 7, 8
    fo, mk = torch.randn(B, H, W, 6, generator=g) * 2, torch.randn(B, H, W, 576, generator=g)
    R = (torch.randn(B, 2, 8 * H, 8 * W, generator=g), torch.randn(B, 4, 8 * H, 8 * W, generator=g))
    use = (loss_on != "info", loss_on != "flow")

    def run(fo_leaf, mk_leaf, fn, to):
        o = fo_leaf.permute(0, 3, 1, 2)
        outs = fn(o[:, :2], o[:, 2:], mk_leaf.permute(0, 3, 1, 2))
        sum((out * to(r)).sum() for out, r, u in zip(outs, R, use) if u).backward()
        return outs

    fo64, mk64 = fo.double().requires_grad_(), mk.double().requires_grad_()
    want = run(fo64, mk64, upsample_data_torch, lambda t: t.double())
    fog, mkg = fo.to(gpu).requires_grad_(), mk.to(gpu).requires_grad_()
    got = run(fog, mkg, upsample_data_train, lambda t: t.to(gpu))
    flow_up, info_up = torch.empty_like(got[0]), torch.empty_like(got[1])
    with torch.no_grad():
        torch.ops.pfk.convex_upsample_info_pm(fog.view(-1, 6)[:, :2], fog.view(-1, 6)[:, 2:], mkg.view(-1, 576), flow_up, info_up)
    assert torch.equal(got[0], flow_up) and torch.equal(got[1], info_up), "the node's forward is not the inference kernel's bits"
    scale_close(got[0], want[0], "flow_up"), scale_close(got[1], want[1], "info_up")
    assert fog.grad.shape == fo.shape and mkg.grad.shape == mk.shape
    scale_close(fog.grad[..., :2], fo64.grad[..., :2], f"loss on {loss_on}: d/dflow")
    scale_close(fog.grad[..., 2:], fo64.grad[..., 2:], f"loss on {loss_on}: d/dinfo")
    scale_close(mkg.grad, mk64.grad, f"loss on {loss_on}: d/dmask")


# ---------------------------------------------------------------------------------------------------------------------
# the seams, end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_sea_raft_loop_trains_through_upsample_data(gpu):
    """tests/test_gpu_sea_train.py::test_training_loop_through_the_seam's inputs, seeds and loss, with `train_upsample=True` on top:
    every parameter's gradient and the feature maps' against the stand-in's CPU float64 run; all three upsamplings on the node"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    from ptlflow_amd import patch
    g = torch.Generator().manual_seed(5)
    B, H, W = 1, 16, 24
    x = [torch.tanh(torch.randn(B, 128, H, W, generator=g)), torch.relu(torch.randn(B, 128, H, W, generator=g)),
         torch.randn(B, 256, H, W, generator=g) * 0.3, torch.randn(B, 256, H, W, generator=g) * 0.3]
    R = {"flows": torch.randn(B, 1, 2, 8 * H, 8 * W, generator=g), "info": torch.randn(B, 4, 8 * H, 8 * W, generator=g),
         "flow_small": torch.randn(B, 2, H, W, generator=g)}

    def run(model, xs, to):
        out = model(*xs)
        sum(((out[k] * to(R[k])).sum() for k in R)).backward()

    ref = load_seeded(SeaRaftLoop(iters=2), 2).double().train()
    xr = [t.double() for t in x]
    xr[2].requires_grad_(True), xr[3].requires_grad_(True)
    run(ref, xr, lambda t: t.double())

    model = load_seeded(SeaRaftLoop(iters=2), 2).to(gpu).train()
    patch.accelerate(model, sea_raft_update=True, sea_raft_train=True, train_upsample=True)
    try:
        xg = [t.to(gpu) for t in x]
        xg[2].requires_grad_(True), xg[3].requires_grad_(True)
        run(model, xg, lambda t: t.to(gpu))
        assert model.upsample_data.train_calls == 3 and model.upsample_data.calls == 0
        assert (model.update_block.train_calls, model.flow_head.train_calls, model.upsample_weight.train_calls) == (2, 3, 3)
        want, got = dict(ref.named_parameters()), dict(model.named_parameters())
        assert sorted(got) == sorted(want)
        for name, p in got.items():
            assert p.grad is not None, name
            scale_close(p.grad, want[name].grad, name)
        scale_close(xg[2].grad, xr[2].grad, "d/dfmap1")
        scale_close(xg[3].grad, xr[3].grad, "d/dfmap2")
    finally:
        patch.restore(model)
    assert "upsample_data" not in model.__dict__ and not hasattr(model.upsample_data, "train_calls")


ZERO_BY_NORM = re.compile(r"^(fnet|cnet)\.(conv1|layer\d+\.\d+\.(conv\d|downsample\.0))\.bias$")


def _raft_pair(gpu, **flag):
    """two SeamRAFT(iters=2).train() with the same weights: accelerate(model, **flag) and plain accelerate(model).  Two pyramid levels:
    a 6 x 9 grid has no third and fourth one"""
    from seam_model import SeamRAFT
    from ptlflow_amd import patch
    torch.manual_seed(4)
    a, b = SeamRAFT(iters=2, corr_levels=2).to(gpu).train(), SeamRAFT(iters=2, corr_levels=2).to(gpu).train()
    b.load_state_dict(a.state_dict())
    patch.accelerate(a, **flag)
    patch.accelerate(b)
    return a, b


def _raft_step(model, images, R):
    """forward with a gradient graph (the stand-in's `forward` is wrapped in no_grad for its eval callers) and one backward"""
    model.zero_grad(set_to_none=True)
    out = type(model).forward.__wrapped__(model, {"images": images})
    ((out["flows"] * R[0]).sum() + (out["flow_small"] * R[1]).sum()).backward()
    return out, {k: p.grad for k, p in model.named_parameters() if p.grad is not None}


def _raft_inputs(gpu):
    g = torch.Generator().manual_seed(6)
    H, W = 48, 72                                             # a 6 x 9 grid
    images = torch.rand(1, 2, 3, H, W, generator=g).to(gpu)
    return images, (torch.randn(1, 1, 2, H, W, generator=g).to(gpu), torch.randn(1, 2, H // 8, W // 8, generator=g).to(gpu))


def test_raft_loop_trains_through_upsample_flow(gpu):
    from ptlflow_amd import patch
    a, b = _raft_pair(gpu, train_upsample=True)
    try:
        images, R = _raft_inputs(gpu)
        out_a, grads_a = _raft_step(a, images, R)
        out_b, grads_b = _raft_step(b, images, R)
        assert a.upsample_flow.train_calls == 2 and a.upsample_flow.calls == 0
        assert b.upsample_flow.train_calls == 0 and b.upsample_flow.calls == 0
        scale_close(out_a["flows"], out_b["flows"], "flows")
        assert sorted(grads_a) == sorted(grads_b) and any(k.startswith("update_block.mask.") for k in grads_a)
        for k in grads_a:
            if ZERO_BY_NORM.match(k):
                # a convolution bias in front of an instance / batch normalisation: its true gradient is zero, and both runs hold the
                # rounding noise of the sum over pixels — which has no scale of its own, so it is held to the scale of the same
                # convolution's weight gradient (a sum over the same output gradients)
                scale = float(grads_b[k[:-len("bias")] + "weight"].abs().max())
                err = float((grads_a[k] - grads_b[k]).abs().max())
                print(f"{k}: max err {err:.3e} of the weight gradient's scale {scale:.3e}")
                assert err <= BLOCK_TOL * scale, f"{k}: max err {err:.3e} vs the weight gradient's scale {scale:.3e}"
            else:
                scale_close(grads_a[k], grads_b[k], k)
    finally:
        patch.restore(a), patch.restore(b)
    assert not hasattr(a.upsample_flow, "train_calls")


def test_flag_off_changes_nothing(gpu):
    """`train_upsample=False` is plain `accelerate`: the same bits, no call on the nodes, gradient calls on the model's own methods"""
    from seam_model import convex_upsample_torch
    from sea_seam_model import SeaRaftLoop, load_seeded
    from ptlflow_amd import patch
    a, b = _raft_pair(gpu, train_upsample=False)
    try:
        images, R = _raft_inputs(gpu)
        out_a, grads_a = _raft_step(a, images, R)
        out_b, grads_b = _raft_step(b, images, R)
        for m in (a, b):
            assert m.upsample_flow.train_upsample is False and m.upsample_flow.train_calls == 0 and m.upsample_flow.calls == 0
        # (a training step of this model is not bit-reproducible, flag or no flag: the same instance run twice on the same input
        # gives other bits in `flows` and in every gradient, so whole steps are held to the block gate and the seam itself is
        # compared bit for bit below)
        scale_close(out_a["flows"], out_b["flows"], "flows"), scale_close(out_a["flow_small"], out_b["flow_small"], "flow_small")
        assert sorted(grads_a) == sorted(grads_b)
        g = torch.Generator().manual_seed(8)
        flow = (torch.randn(1, 2, 6, 9, generator=g) * 3).to(gpu).requires_grad_()
        mask = torch.randn(1, 576, 6, 9, generator=g).to(gpu).requires_grad_()
        for m in (a, b):      # a gradient call is the model's own method: its bits, its graph
            up = m.upsample_flow(flow, mask)
            assert torch.equal(up, convex_upsample_torch(flow, mask)) and type(up.grad_fn).__name__ != "_ConvexUpsampleBackward"
            assert m.upsample_flow.train_calls == 0 and m.upsample_flow.calls == 0
        # switched on by a second call, off again by a third
        patch.accelerate(a, train_upsample=True)
        up = a.upsample_flow(flow, mask)
        assert a.upsample_flow.train_calls == 1 and up.requires_grad
        scale_close(up, convex_upsample_torch(flow, mask), "upsample_flow on the node")
        patch.accelerate(a)
        assert a.upsample_flow.train_upsample is False
        # extra arguments, autocast and no_grad never reach the node
        patch.accelerate(a, train_upsample=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            a.upsample_flow(flow, mask)
        with torch.no_grad():
            a.upsample_flow(flow, mask)
        assert a.upsample_flow.train_calls == 1
    finally:
        patch.restore(a), patch.restore(b)
    sea = load_seeded(SeaRaftLoop(iters=1), 3).to(gpu).train()
    patch.accelerate(sea, sea_raft_update=True, sea_raft_train=True)
    try:
        info = torch.randn(1, 4, 6, 9, generator=g).to(gpu).requires_grad_()
        got = sea.upsample_data(flow, info, mask)
        assert sea.upsample_data.train_calls == 0 and sea.upsample_data.calls == 0
        assert all(torch.equal(u, v) for u, v in zip(got, upsample_data_torch(flow, info, mask)))
    finally:
        patch.restore(sea)
