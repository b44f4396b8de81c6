"""K12b, `torch.ops.pfk.conv_wgrad_unpacked_b16` (pfk_wgrad_b16.hip): the weight / bias gradient of a "same" convolution on
bf16 operands — transposed LDS reads feeding v_mfma_f32_32x32x16_bf16 — against the float64 product of the SAME bf16-rounded
operands.  Operands are drawn in fp32 and rounded to bf16, so every product is exact in fp32 and only the accumulation order
differs from the reference: the gate is the one of the fp32 weight gradient (tests/test_gpu_train.py), 2e-4 of the tensor's
largest magnitude.

Shapes are the smallest at which the kernel can go wrong: fewer pixels than one 64-pixel K-step; a K-step that straddles two
images (a tap must not read across the border) with a tail that is no multiple of 16; two sources with padding channels that
must produce no column; a padded 1x1 source; a forced split of the pixel range (deterministic, twice the same bits); the widest
and the narrowest cout."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel_close(a, b, tol=2e-4, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = float(b.abs().max()) + 1e-12
    err = float((a - b).abs().max())
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _case(B, H, W, kh, kw, reals, bufs, cout_real, cout_buf, seed=3):
    """bf16 pixel-major operands (padding channels filled with NON-zero junk where the buffer is wider than the real channels:
    they must get no column) and the float64 reference gradients of the same rounded values."""
    g = torch.Generator().manual_seed(seed)
    M = B * H * W
    xs = [torch.randn(M, cb, generator=g).bfloat16() for cb in bufs]
    dy = torch.randn(M, cout_buf, generator=g).bfloat16()
    x64 = torch.cat([x[:, :r].double() for x, r in zip(xs, reals)], 1).view(B, H, W, -1).permute(0, 3, 1, 2)
    dy64 = dy[:, :cout_real].double().view(B, H, W, cout_real).permute(0, 3, 1, 2)
    w = torch.zeros(cout_real, sum(reals), kh, kw, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout_real, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w, b, padding=(kh // 2, kw // 2)).backward(dy64)
    return xs, dy, w.grad, b.grad


def _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout_real, with_bias=True, accumulate=False, into=None):
    if into is None:
        dw = torch.full((cout_real, sum(reals), kh, kw), float("nan"), device=gpu)
        db = torch.full((cout_real,), float("nan"), device=gpu) if with_bias else None
    else:
        dw, db = into
    torch.ops.pfk.conv_wgrad_unpacked_b16([x.to(gpu) for x in xs], dy.to(gpu), B, H, W, kh, kw, dw, db, list(reals), accumulate)
    return dw, db


CASES = [
    # B, H, W, kh, kw, real channels, buffer channels, cout real, cout buffer
    pytest.param(1, 5, 7, 3, 3, (8,), (8,), 8, 8, id="35px-below-one-kstep"),
    pytest.param(2, 9, 13, 1, 1, (72,), (72,), 96, 96, id="1x1-two-images"),
    pytest.param(2, 9, 13, 3, 3, (72,), (72,), 96, 96, id="3x3-two-images"),
    pytest.param(2, 9, 13, 1, 5, (72,), (72,), 96, 96, id="1x5-two-images"),
    pytest.param(2, 9, 13, 5, 1, (72,), (72,), 96, 96, id="5x1-two-images"),
    pytest.param(1, 8, 20, 1, 5, (128, 126), (128, 128), 256, 256, id="gru-zr-two-sources-padded"),
    pytest.param(1, 8, 12, 1, 1, (324,), (328,), 256, 256, id="convc1-padded"),
    pytest.param(1, 8, 12, 1, 1, (256,), (256,), 576, 576, id="mask-576"),
    pytest.param(1, 8, 12, 3, 3, (256,), (256,), 2, 8, id="flow-head-cout2"),
]


@pytest.mark.parametrize("B,H,W,kh,kw,reals,bufs,cout_real,cout_buf", CASES)
def test_wgrad_b16_against_float64(gpu, B, H, W, kh, kw, reals, bufs, cout_real, cout_buf):
    xs, dy, dw_ref, db_ref = _case(B, H, W, kh, kw, reals, bufs, cout_real, cout_buf)
    dw, db = _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout_real)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())      # every element written
    rel_close(dw, dw_ref, what="dw")
    rel_close(db, db_ref, what="db")


def test_wgrad_b16_slices_are_deterministic(gpu):
    """The pixel range forced into 3 slices (pfk_debug_set_wgrad_b16): same result as the reference, twice the same bits, and
    the same gate as one slice."""
    B, H, W, kh, kw, reals, cout = 2, 24, 40, 3, 3, (128,), 64
    xs, dy, dw_ref, db_ref = _case(B, H, W, kh, kw, reals, reals, cout, cout, seed=5)
    ops = torch.ops.pfk
    try:
        ops.debug_set_wgrad_b16(3)
        dw1, db1 = _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout)
        dw2, db2 = _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout)
        ops.debug_set_wgrad_b16(1)
        dw3, db3 = _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout)
    finally:
        ops.debug_set_wgrad_b16(0)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    rel_close(dw1, dw_ref, what="dw (3 slices)")
    rel_close(db1, db_ref, what="db (3 slices)")
    rel_close(dw3, dw_ref, what="dw (1 slice)")
    assert not torch.equal(dw1, dw3), "the forced split did not change the summation order: the knob had no effect"


def test_wgrad_b16_accumulate_and_no_bias(gpu):
    B, H, W, kh, kw, reals, cout = 2, 9, 13, 3, 3, (72,), 96
    xs, dy, dw_ref, db_ref = _case(B, H, W, kh, kw, reals, reals, cout, cout, seed=9)
    dw1, db1 = _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout)
    dw2, db2 = _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout, accumulate=True, into=(dw1.clone(), db1.clone()))
    assert torch.equal(dw2, dw1 + dw1) and torch.equal(db2, db1 + db1)
    dw3, none = _run(gpu, B, H, W, kh, kw, reals, xs, dy, cout, with_bias=False)
    assert none is None
    rel_close(dw3, dw_ref, what="dw without db")


def test_wgrad_b16_refuses_what_it_does_not_cover(gpu):
    ops = torch.ops.pfk
    x = torch.zeros(24, 16, device=gpu, dtype=torch.bfloat16)
    dy = torch.zeros(24, 8, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):                      # 7x7: outside the scope of kernels
        ops.conv_wgrad_unpacked_b16([x], dy, 1, 4, 6, 7, 7, torch.empty(8, 16, 7, 7, device=gpu), None, [16], False)
    with pytest.raises(RuntimeError):                      # fp32 source
        ops.conv_wgrad_unpacked_b16([x.float()], dy, 1, 4, 6, 1, 1, torch.empty(8, 16, 1, 1, device=gpu), None, [16], False)
    with pytest.raises(RuntimeError):                      # 12 channels: not a multiple of 8
        ops.conv_wgrad_unpacked_b16([x[:, :12]], dy, 1, 4, 6, 1, 1, torch.empty(8, 12, 1, 1, device=gpu), None, [12], False)
