"""`pfk_convex_upsample2_bwd_f32` — the backward of `upsample_flow(flow, mask, scale=2)` — under gates 1-4 of
tests/op_gate.py, its autograd node (`train.convex_upsample2`) and seam B5 under `accelerate(model, multiscale_train=True)`.

Reference: float64 autograd through `ms_loop_model.MsLoopModel.upsample_flow(scale=2)` on the kernel's own fp32 inputs.

Per-element bounds: `op_refs.convex_case`'s derivation with S = 2.  A softmax weight is off by at most k_w = 2 spread + 19 units of
2^-24 relative (the rounded differences m_k - max in the numerator and in the denominator, expf within 2 ulp twice, nine additions,
the reciprocal, the product).
  grad_mask   w_k (dw_k - sum_j w_j dw_j): its weight, dw_k (3 roundings), the dot (each term a weight, a dw, a product; nine
              additions), the subtraction and the last product:  K = 2 k_w + 15  on  w_k (T_k + sum_j w_j T_j),
              T_k = |g_x| |v_x,k| + |g_y| |v_y,k|.  (Unchanged from the x8 kernel: the expression is per sub-pixel.)
  grad_flow   a flow pixel receives at most 9 neighbours x 4 sub-pixels = 36 products 2 w g, where the x8 kernel sums 9 x 64:
              K = 9 * 4 + max k_w + 2  on  sum 2 w |g|.  At logit scale 1 the spread stays below ~8: K <= ~73; at scale 40 it is
              data-dependent (spread up to ~300) and computed next to the reference.
Where the magnitudes are 0 the element is an exact zero.

Cases (B, H, W, logit scale): (2,1,5,1), (1,6,1,1), (2,9,13,1) (M = 234: not a multiple of a wave's 32 pixels, and an image boundary
the neighbourhoods must not cross), (2,9,13,40) (a saturated softmax), (1,3,65,1) (a row longer than one wave's 32 pixels).  Every
case runs in three layouts: mask rows of stride 36 / 37 / 40 inside NaN-filled buffers, grad_mask rows of stride 38 / 37 / 40 (the
last one float off 8-byte alignment), flow and grad_flow as NCHW or as rows.

Measured on an MI355X, worst over the cases (relative L2 | error as a fraction of the per-element bound):
  test_kernel              grad_mask 9.2e-8 | 0.106 (logits x 40: 3.5e-7 | 0.211)     grad_flow 9.5e-8 | 0.034
                           (the three layouts of a case give the same figures: they give the same bits)
  test_autograd_node       grad_mask 9.2e-8 | 0.106     grad_flow 9.5e-8 | 0.026
  test_seam_b5_...         against the model's method in float64: forward 1.2e-7, grad_flow 9.2e-8, grad_mask 8.1e-8 of the scale
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from op_gate import BLOCK_TOL, FLOOR, Rows, flat_out, gates, leaf, nchw, scale_close, tail_kept

pytestmark = pytest.mark.gpu

CASES = [(2, 1, 5, 1.0), (1, 6, 1, 1.0), (2, 9, 13, 1.0), (2, 9, 13, 40.0), (1, 3, 65, 1.0)]
# name: (mask pad, grad_mask lead, grad_mask pad, flow as rows, grad_flow as rows)
LAYOUTS = {
    "ld36_nchw": (0, 0, 2, False, False),      # 8-byte accesses: mask_ld 36, grad_mask_ld 38
    "ld37_rows": (1, 0, 1, True, True),        # odd strides: the 4-byte twin
    "ld40_mixed": (4, 1, 3, True, False),      # even strides, grad_mask one float off 8-byte alignment: the 4-byte twin again
}


def model_method(flow, mask):
    from ms_loop_model import MsLoopModel
    return MsLoopModel.upsample_flow(None, flow, mask, scale=2)       # (the method reads nothing of the model)


@functools.lru_cache(maxsize=None)
def case(B, H, W, logit_scale):
    """fp32 inputs, the float64 gradients of the model's method and their sums of magnitudes; once per case"""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W + int(logit_scale))
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    mask = torch.randn(B, 36, H, W, generator=g) * logit_scale
    go = torch.randn(B, 2, 2 * H, 2 * W, generator=g)
    f64, m64, g64 = flow.double().requires_grad_(), mask.double().requires_grad_(), go.double()
    out = model_method(f64, m64)
    gflow, gmask = torch.autograd.grad((out * g64).sum(), (f64, m64), retain_graph=True)
    (gflow_mag,) = torch.autograd.grad((out * g64.abs()).sum(), f64)        # the softmax weights are >= 0: sum of 2 w |g|
    with torch.no_grad():
        m = m64.view(B, 1, 9, 2, 2, H, W)
        wgt = torch.softmax(m, dim=2)[:, 0]                                                          # [B, 9, 2, 2, H, W]
        spread = (m.amax(2) - m.amin(2))[:, 0]                                                       # [B, 2, 2, H, W]
        up = F.unfold(2 * f64, [3, 3], padding=1).view(B, 2, 9, 1, 1, H, W).abs()
        gsub = g64.view(B, 2, H, 2, W, 2).permute(0, 1, 3, 5, 2, 4).abs()                            # [B, 2, sy, sx, H, W]
        T = (gsub[:, :, None] * up).sum(1)                                                           # [B, 9, 2, 2, H, W]
        gmask_mag = wgt * (T + (wgt * T).sum(1, keepdim=True))
    rows = lambda t: t.reshape(B, 36, H, W).permute(0, 2, 3, 1).reshape(B * H * W, 36)
    k_w = 2 * spread + 19
    return {"flow": flow, "mask": mask, "go": go, "gflow": gflow.detach(), "gflow_mag": gflow_mag, "gmask": rows(gmask.detach()),
            "gmask_mag": rows(gmask_mag), "k_mask": rows((2 * k_w + 15)[:, None].expand(B, 9, 2, 2, H, W)),
            "k_flow": 9 * 4 + float(k_w.max()) + 2}


def launch(c, gpu, layout):
    """one launch in `layout` on fresh outputs -> (grad_mask Rows, the buffer behind grad_flow, grad_flow as NCHW)"""
    mpad, glead, gpad, flow_rows, gflow_rows = LAYOUTS[layout]
    B, _, H, W = c["flow"].shape
    M = B * H * W
    mask = Rows(M, 36, gpu, rows36(c["mask"]), pad=mpad, nan_tail=True)
    assert mask.ld == 36 + mpad
    flow = Rows(M, 2, gpu, rows36(c["flow"]), pad=2).rows if flow_rows else c["flow"].to(gpu)      # rows: flow_ld = 4, NaN in columns 2..3
    gmask = Rows(M, 36, gpu, pad=gpad, lead=glead)
    if gflow_rows:
        gf = Rows(M, 2, gpu, pad=2)
        guard, gflow = gf, gf.rows
    else:
        guard, gflow = flat_out((B, 2, H, W), gpu)
    torch.ops.pfk.convex_upsample2_bwd(flow, mask.rows, c["go"].to(gpu), gmask.rows, gflow)
    torch.cuda.synchronize()
    gmask.check_untouched("grad_mask")
    if gflow_rows:
        guard.check_untouched("grad_flow")
        return gmask, guard.flat, nchw(gflow, B, H, W)
    assert tail_kept(guard), "memory past grad_flow was written"
    return gmask, guard, gflow


def rows36(t):
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B,H,W,logit_scale", CASES)
def test_kernel(gpu, B, H, W, logit_scale, layout):
    c = case(B, H, W, logit_scale)
    gmask, flat, gflow = launch(c, gpu, layout)
    what = f"convex_upsample2_bwd {(B, H, W)} x{logit_scale:g} {layout}"
    gates(what + " grad_mask", gmask.rows, c["gmask"], c["gmask_mag"], c["k_mask"], floor=FLOOR)
    gates(what + " grad_flow", gflow, c["gflow"], c["gflow_mag"], c["k_flow"], floor=FLOOR)
    gmask2, flat2, _ = launch(c, gpu, layout)
    assert torch.equal(gmask2.flat, gmask.flat) and torch.equal(flat2, flat), "a second run gives other bits"


def test_layouts_give_the_same_bits(gpu):
    """8-byte and 4-byte accesses, NCHW and rows: one arithmetic"""
    c = case(2, 9, 13, 1.0)
    res = [launch(c, gpu, layout) for layout in LAYOUTS]
    for gmask, _, gflow in res[1:]:
        assert torch.equal(gmask.rows, res[0][0].rows) and torch.equal(gflow, res[0][2])


@pytest.mark.parametrize("keep", [0, 4, 8])
def test_minus_infinity_in_eight_taps(gpu, keep):
    """-inf in eight of the nine taps: the mask gradient is exactly zero (the one weight is exactly 1, the others exactly 0), and the
    flow gradient lands on neighbour `keep` alone: 2 x the sum of the pixel's four sub-pixel gradients, shifted"""
    B, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(keep)
    d = {"flow": torch.randn(B, 2, H, W, generator=g), "go": torch.randn(B, 2, 2 * H, 2 * W, generator=g)}
    mask = torch.full((B, 9, 4, H, W), float("-inf"))
    mask[:, keep] = torch.randn(B, 4, H, W, generator=g)
    d["mask"] = mask.view(B, 36, H, W)
    for layout in LAYOUTS:
        gmask, _, gflow = launch(d, gpu, layout)
        assert bool((gmask.rows == 0).all()), "a mask gradient that is not exactly zero"
        dy, dx = keep // 3 - 1, keep % 3 - 1
        ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))             # pixels whose neighbour is inside
        yd, xd = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
        want, mag = torch.zeros(B, 2, H, W, dtype=torch.float64), torch.zeros(B, 2, H, W, dtype=torch.float64)
        want[:, :, yd, xd] = (2 * 4 * F.avg_pool2d(d["go"].double(), 2))[:, :, ys, xs]               # 2 x the sum of a pixel's four sub-pixels
        mag[:, :, yd, xd] = (2 * 4 * F.avg_pool2d(d["go"].double().abs(), 2))[:, :, ys, xs]
        got = gflow.double().cpu()
        assert bool((got[mag == 0] == 0).all())
        assert bool(((got - want).abs() <= 4 * 2.0 ** -24 * mag).all())                              # three additions (the doubling is exact)


def test_autograd_node(gpu):
    """`train.convex_upsample2` under `torch.autograd.grad`: the forward is the inference kernel's, both gradients pass the gates"""
    from ptlflow_amd import train
    B, H, W, s = 2, 9, 13, 1.0
    c = case(B, H, W, s)
    flow, rows = leaf(c["flow"].to(gpu), torch.float32), leaf(rows36(c["mask"]).to(gpu), torch.float32)
    out = train.convex_upsample2(flow, rows)
    ref = torch.empty_like(out)
    torch.ops.pfk.convex_upsample2(flow.detach(), rows.detach(), ref)
    assert torch.equal(out, ref)
    gflow, gmask = torch.autograd.grad(out, (flow, rows), c["go"].to(gpu))
    gates("node grad_mask", gmask, c["gmask"], c["gmask_mag"], c["k_mask"], floor=FLOOR)
    gates("node grad_flow", gflow, c["gflow"], c["gflow_mag"], c["k_flow"], floor=FLOOR)
    # a mask handed in as the NCHW view of wider rows (the update block's training mask)
    wide = torch.zeros(B * H * W, 40, device=gpu)
    wide[:, :36] = rows.detach()
    wide.requires_grad_()
    out2 = train.convex_upsample2(flow, wide[:, :36])
    assert torch.equal(out2, ref)
    (gwide,) = torch.autograd.grad(out2, wide, c["go"].to(gpu))
    assert torch.equal(gwide[:, :36], gmask) and bool((gwide[:, 36:] == 0).all())


def test_seam_b5_serves_gradient_graphs(gpu):
    """`accelerate(model, multiscale_train=True)`: `upsample_flow(flow, mask, scale=2)` / `(flow, mask, 2)` with a gradient graph run
    the node and count in `train_calls`; the gradients are the model's own method's in float64 within BLOCK_TOL.  Without the option
    the call is the model's method's."""
    from ms_loop_model import MsLoopModel
    from ptlflow_amd import patch
    model = MsLoopModel("ms_raft", (1, 1, 1)).train().to(gpu)
    B, H, W = 2, 9, 13
    c = case(B, H, W, 1.0)
    go = c["go"].to(gpu)

    def grads(call):
        flow, mask = leaf(c["flow"].to(gpu), torch.float32), leaf(c["mask"].to(gpu), torch.float32)
        out = call(flow, mask)
        return out, torch.autograd.grad(out, (flow, mask), go)

    patch.accelerate(model, multiscale_train=True)
    seam = model.__dict__["upsample_flow"]
    assert seam.multiscale_train and not seam.multiscale and seam.train_calls == 0
    out_kw, (gf_kw, gm_kw) = grads(lambda f, m: model.upsample_flow(f, m, scale=2))
    assert seam.train_calls == 1 and seam.ok2 is True
    out_pos, (gf_pos, gm_pos) = grads(lambda f, m: model.upsample_flow(f, m, 2))
    assert seam.train_calls == 2 and seam.calls == 0
    assert torch.equal(out_kw, out_pos) and torch.equal(gf_kw, gf_pos) and torch.equal(gm_kw, gm_pos)
    f64, m64 = leaf(c["flow"], torch.float64), leaf(c["mask"], torch.float64)
    want = model_method(f64, m64)
    wf, wm = torch.autograd.grad(want, (f64, m64), c["go"].double())
    scale_close(out_kw, want, "seam B5 x2 forward", BLOCK_TOL)
    scale_close(gf_kw, wf, "seam B5 x2 grad_flow", BLOCK_TOL)
    scale_close(gm_kw, wm, "seam B5 x2 grad_mask", BLOCK_TOL)
    # not served: no gradient graph, autocast, another scale, a 35-channel mask
    with torch.no_grad():
        model.upsample_flow(c["flow"].to(gpu), c["mask"].to(gpu), scale=2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        grads(lambda f, m: model.upsample_flow(f, m, scale=2))
    g8 = torch.randn(B, 576, H, W, device=gpu, requires_grad=True)
    model.upsample_flow(c["flow"].to(gpu), g8, scale=8)
    assert seam.train_calls == 2
    # the option off again: the same seam object stops serving
    patch.accelerate(model, multiscale_train=False)
    grads(lambda f, m: model.upsample_flow(f, m, scale=2))
    assert seam.train_calls == 2
    patch.restore(model)
    assert "upsample_flow" not in model.__dict__
