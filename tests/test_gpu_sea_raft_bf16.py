"""SEA-RAFT's refinement on the bf16 matrix-core path (`accelerate(model, sea_raft_update="bf16")`, ptlflow_amd/sea_update.py): the
three bf16 kernels against fp64 restatements of their bf16 operands, the whole loop of tests/sea_seam_model.py under cuda bf16
autocast and as an fp32 loop (gated against the CPU-autocast gap, the convention of test_gpu_bf16_gate.py), the fallbacks, and the
bf16 `bilinear_f2` correlation against the oracle."""
import math

import pytest
import torch
import torch.nn.functional as F

from op_gate import ulp_bf16, within_ulp

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- dwconv + LayerNorm
@pytest.mark.parametrize("B,H,W", [(1, 55, 128), (2, 55, 128), (1, 7, 9), (1, 13, 5)])
@pytest.mark.parametrize("C", [64, 384])
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("pad", [0, 24])
def test_dwconv_layernorm_b16(gpu, B, H, W, C, k, pad):
    g = torch.Generator().manual_seed(B * 7 + H * 1000 + W + C + k + pad)
    x = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16)
    w = torch.randn(C, 1, k, k, generator=g) / k
    b = 0.1 * torch.randn(C, generator=g)
    lw = 1 + 0.1 * torch.randn(C, generator=g)
    lb = 0.1 * torch.randn(C, generator=g)
    y = F.conv2d(x.double(), w.double(), b.double(), padding=k // 2, groups=C).permute(0, 2, 3, 1)
    ref = F.layer_norm(y, (C,), lw.double(), lb.double(), 1e-6).reshape(-1, C)
    M = B * H * W
    # in_ld = C, or a slice of a wider row (like the update engine's hxb); the output rows padded too
    buf = torch.zeros(M, C + pad, device=gpu, dtype=torch.bfloat16)
    inp = buf[:, 8: 8 + C] if pad else buf
    inp.copy_(x.permute(0, 2, 3, 1).reshape(M, C).to(gpu))
    out_buf = torch.full((M, C + pad), float("nan"), device=gpu, dtype=torch.bfloat16)
    out = out_buf[:, :C]
    torch.ops.pfk.dwconv_layernorm_b16(inp, w.to(gpu).reshape(C, k * k).contiguous(), b.to(gpu), lw.to(gpu), lb.to(gpu), 1e-6, out,
                                       B, H, W, k)
    torch.cuda.synchronize()
    within_ulp(out.cpu(), ref, 2.0 ** -16)
    if pad:
        assert bool(torch.isnan(out_buf[:, C:].float()).all()), "wrote past the C channels of its rows"


# ------------------------------------------------------------------------------------------------------------- K8b + GELU
@pytest.mark.parametrize("M,cin,cout", [(7040, 384, 512), (56320, 384, 512), (1000, 384, 512), (4000, 512, 384)])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_conv2d_gelu_b16(gpu, M, cin, cout, out_dtype):
    from ptlflow_amd.packing import pack_conv_weight
    g = torch.Generator().manual_seed(M + cin + (out_dtype == torch.float32))
    x = torch.randn(M, cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(torch.bfloat16)
    b = torch.randn(cout, generator=g)
    ref = F.gelu(F.linear(x.double(), w.double(), b.double()))
    wp = pack_conv_weight(w.float()[:, :, None, None], [(0, cin, cin)], kpad=64).to(torch.bfloat16).to(gpu)
    out = torch.full((M, cout), float("nan"), device=gpu, dtype=out_dtype)
    torch.ops.pfk.conv2d_gelu_b16([x.to(gpu)], 1, 1, M, 1, 1, wp, b.to(gpu), cout, 1.0, out)
    torch.cuda.synchronize()
    got = out.double().cpu()
    if out_dtype == torch.bfloat16:      # the rounding of the output (half an ulp) and fp32 accumulation
        lim = 0.5 * ulp_bf16(ref) + 1e-5 * (1 + ref.abs())
    else:
        lim = 2e-5 * (1 + ref.abs())
    err = (got - ref).abs()
    assert bool((err <= lim).all()), f"max err {float(err.max()):.3e}, worst ratio {float((err / lim).max()):.2f}"


def test_conv2d_gelu_b16_residual(gpu):
    """GELU, scale, then the residual, as LINEAR: fp32 and bf16 residual rows"""
    from ptlflow_amd.packing import pack_conv_weight
    M, cin, cout = 3000, 128, 256
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(torch.bfloat16)
    b = torch.randn(cout, generator=g)
    r = torch.randn(M, cout, generator=g)
    wp = pack_conv_weight(w.float()[:, :, None, None], [(0, cin, cin)], kpad=64).to(torch.bfloat16).to(gpu)
    for res in (r, r.to(torch.bfloat16)):
        ref = res.double() + 0.5 * F.gelu(F.linear(x.double(), w.double(), b.double()))
        out = torch.full((M, cout), float("nan"), device=gpu)
        torch.ops.pfk.conv2d_gelu_b16([x.to(gpu)], 1, 1, M, 1, 1, wp, b.to(gpu), cout, 0.5, out, res.to(gpu))
        torch.cuda.synchronize()
        torch.testing.assert_close(out.double().cpu(), ref, rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------------------- info upsampling
@pytest.mark.parametrize("B,H,W", [(2, 55, 128), (1, 13, 17)])
def test_convex_upsample_info_b16(gpu, B, H, W):
    from sea_seam_model import upsample_data_torch
    g = torch.Generator().manual_seed(B * 100 + H + 1)
    M = B * H * W
    fo = torch.randn(M, 8, generator=g) * 3
    mask = (torch.randn(M, 576, generator=g) * 2).to(torch.bfloat16)
    fo_d, mask_d = fo.to(gpu), mask.to(gpu)
    flow_up = torch.empty(B, 2, 8 * H, 8 * W, device=gpu)
    info_up = torch.empty(B, 4, 8 * H, 8 * W, device=gpu)
    torch.ops.pfk.convex_upsample_info_pm_b16(fo_d[:, :2], fo_d[:, 2:6], mask_d, flow_up, info_up)
    want = torch.empty_like(flow_up)
    torch.ops.pfk.convex_upsample_pm(fo_d[:, :2], mask_d, want)
    torch.cuda.synchronize()
    assert torch.equal(flow_up, want)
    nchw = lambda t: t.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    _, ri = upsample_data_torch(nchw(fo[:, :2].double()), nchw(fo[:, 2:6].double()), nchw(mask.double()))
    torch.testing.assert_close(info_up.double().cpu(), ri, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------- whole loop
def _seeded_loop(seed, iters=4):
    from sea_seam_model import SeaRaftLoop, load_seeded
    return load_seeded(SeaRaftLoop(iters=iters), seed).eval()


def _loop_inputs(B, H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(B, 128, H, W, generator=g))
    ctx = torch.relu(torch.randn(B, 128, H, W, generator=g))
    f1 = torch.randn(B, 256, H, W, generator=g) * 0.3
    f2 = torch.roll(f1, shifts=(1, 2), dims=(2, 3)) + 0.1 * torch.randn(B, 256, H, W, generator=g)
    return net, ctx, f1, f2


def _epe(a, b):
    return float((a.float().cpu() - b.float().cpu()).norm(dim=1).mean())


def _mad(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().mean())


@pytest.mark.parametrize("B,H,W", [(1, 55, 128), (2, 16, 24)])
@pytest.mark.parametrize("mode", ["autocast", "fp32"])
def test_whole_loop_bf16(gpu, B, H, W, mode):
    from ptlflow_amd import patch
    iters = 4
    x = _loop_inputs(B, H, W)
    cpu = _seeded_loop(11, iters)
    with torch.no_grad():
        ref = cpu(*x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ref_ac = cpu(*x)
    gap_flow = _epe(ref_ac["flows"][:, 0], ref["flows"][:, 0])
    gap_info = _mad(ref_ac["info"], ref["info"])
    assert gap_flow > 0 and gap_info > 0

    model = _seeded_loop(11, iters).to(gpu)
    patch.accelerate(model, sea_raft_update="bf16")
    dtypes = {"update_block": [], "flow_head": [], "upsample_weight": []}
    hooks = [getattr(model, k).register_forward_hook(lambda m, i, o, k=k: dtypes[k].append(o.dtype)) for k in dtypes]
    try:
        ub = model.update_block
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "autocast"):
            out = model(*[t.to(gpu) for t in x])
        torch.cuda.synchronize()
        assert (ub.calls, model.flow_head.calls, model.upsample_weight.calls) == (iters, iters, iters)
        assert model.upsample_data.calls == iters + 1          # (the loop's first upsampling, before the iterations, too)
        want = torch.bfloat16 if mode == "autocast" else torch.float32
        assert dtypes["update_block"][-iters:] == [want] * iters
        assert dtypes["upsample_weight"][-iters:] == [want] * iters
        assert dtypes["flow_head"][-iters:] == [torch.float32] * iters
        assert out["flows"].dtype == torch.float32 and out["info"].dtype == torch.float32
        e_flow = _epe(out["flows"][:, 0], ref["flows"][:, 0])
        e_info = _mad(out["info"], ref["info"])
        assert math.isfinite(e_flow) and math.isfinite(e_info)
        assert e_flow <= 2 * gap_flow, f"flow EPE {e_flow:.3e} vs the autocast gap {gap_flow:.3e}"
        assert e_info <= 2 * gap_info, f"info error {e_info:.3e} vs the autocast gap {gap_info:.3e}"
    finally:
        for h in hooks:
            h.remove()
        patch.restore(model)


# ------------------------------------------------------------------------------------------------------------- fallbacks
def _run(model, x, mode):
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        if mode == "fp16_autocast":
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return model(*x)
        if mode == "half":
            with torch.no_grad():
                return model(*[t.half() for t in x])
        return model(*x)          # "grad": parameters require grad, grad mode on: a gradient graph


@pytest.mark.parametrize("mode", ["fp16_autocast", "half", "grad"])
def test_bf16_fallbacks_are_the_original_modules(gpu, mode):
    from ptlflow_amd import patch
    B, H, W = 1, 16, 24
    x = [t.to(gpu) for t in _loop_inputs(B, H, W, seed=5)]
    model = _seeded_loop(2, iters=2).to(gpu)
    if mode == "half":
        model = model.half()
    patch.accelerate(model)
    try:
        want = _run(model, x, mode)
    finally:
        patch.restore(model)
    patch.accelerate(model, sea_raft_update="bf16")
    try:
        got = _run(model, x, mode)
        assert model.update_block.calls == 0 and model.flow_head.calls == 0 and model.upsample_weight.calls == 0
        assert model.upsample_data.calls == 0
    finally:
        patch.restore(model)
    for k in ("flows", "info", "flow_small"):
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------- bf16 correlation
def test_bilinear_f2_bf16_volume_against_oracle(gpu):
    """CorrBlock(pyramid="bilinear_f2", volume_dtype=bf16) at 55 x 128, D = 256: each level within one bf16 ulp of the oracle's
    GEMM on the bf16-rounded operands (fmap1, and fmap2 halved in fp32 then rounded, as the block feeds K1); the oracle's lookup on
    the GPU's own bf16 pyramid is the kernel's lookup, bit for bit"""
    from oracle import raft_oracle as O
    from ptlflow_amd.corr import CorrBlock
    B, D, h, w, L, r = 1, 256, 55, 128, 4, 4
    g = torch.Generator().manual_seed(8)
    f1 = torch.randn(B, D, h, w, generator=g)
    f2 = torch.randn(B, D, h, w, generator=g)
    cb = CorrBlock(f1.to(gpu), f2.to(gpu), num_levels=L, radius=r, pyramid="bilinear_f2", volume_dtype=torch.bfloat16,
                   layout="rowmajor")
    gpu_pyr = [lv.cpu() for lv in cb.corr_pyramid]
    assert all(lv.dtype == torch.bfloat16 for lv in gpu_pyr)
    f1b = f1.to(torch.bfloat16).float()
    # the block's target maps: fmap2 halved in fp32 by its own 2x2 kernel (pinned to the bilinear halving elsewhere), then rounded
    f2_pm = f2.to(gpu).permute(0, 2, 3, 1).reshape(B * h * w, D).contiguous()
    h2, w2 = h, w
    for lvl in range(L):
        if lvl > 0:
            nxt = torch.empty(B * (h2 // 2) * (w2 // 2), D, device=gpu)
            torch.ops.pfk.fmap_pool2x2(f2_pm, nxt, B, h2, w2)
            f2_pm, h2, w2 = nxt, h2 // 2, w2 // 2
        f2l = f2_pm.view(B, h2, w2, D).permute(0, 3, 1, 2).cpu()
        ref = O.sea_correlation_pyramid(f1b, f2l.to(torch.bfloat16).float(), num_levels=1)[0]
        # (two fp32 sums of 256 products, the oracle's and K1's, in different orders: 2^-14 absolute near zero)
        within_ulp(gpu_pyr[lvl].reshape(ref.shape), ref.double(), 2.0 ** -14)
    coords = O.coords_grid(B, h, w) + torch.randn(B, 2, h, w, generator=g) * 6
    pyr32 = [lv.float().reshape(B * h * w, 1, lv.shape[-2], lv.shape[-1]) for lv in gpu_pyr]
    want = O.lookup(pyr32, coords, r)
    got = cb(coords.to(gpu)).float().cpu()
    assert torch.equal(got, want)
