"""SEA-RAFT's refinement on the kernels (ptlflow_amd/sea_update.py): dwconv + LayerNorm, the GELU epilogue, the info-carrying convex
upsampling, the golden replay of the reference's own modules and the whole loop of tests/sea_seam_model.py behind
`accelerate(model, sea_raft_update=True)`."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from pfk_ctypes import Desc as _Desc, DescB16 as _DescB16, Src as _Src, SrcB16 as _SrcB16

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sea_raft_update.pt")


# local, not op_gate.close: the limit is tol * (1 + |ref|), with a shape check and the worst ratio in the message
def _close(got, ref, tol=2e-5):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    lim = tol * (1 + ref.abs())
    assert bool((err <= lim).all()), f"max err {float(err.max()):.3e}, worst ratio {float((err / lim).max()):.2f}"


# ------------------------------------------------------------------------------------------------------------- dwconv + LayerNorm
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(55, 128), (47, 156), (13, 17), (1, 5)])
def test_dwconv_layernorm(gpu, B, H, W):
    C, k = 384, 7
    g = torch.Generator().manual_seed(H * 1000 + W + B)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, k, k, generator=g) / k
    b = 0.1 * torch.randn(C, generator=g)
    lw = 1 + 0.1 * torch.randn(C, generator=g)
    lb = 0.1 * torch.randn(C, generator=g)
    ref = F.layer_norm(F.conv2d(x, w, b, padding=k // 2, groups=C).permute(0, 2, 3, 1), (C,), lw, lb, 1e-6).reshape(-1, C)
    M = B * H * W
    # a strided slice of a wider buffer, like the update engine's hx
    buf = torch.zeros(M, C + 8, device=gpu)
    buf[:, 4:4 + C] = x.permute(0, 2, 3, 1).reshape(M, C).to(gpu)
    out = torch.full((M, C), float("nan"), device=gpu)
    torch.ops.pfk.dwconv_layernorm(buf[:, 4:4 + C], w.to(gpu).contiguous(), b.to(gpu), lw.to(gpu), lb.to(gpu), 1e-6, out, B, H, W, k)
    torch.cuda.synchronize()
    _close(out, ref)


# ------------------------------------------------------------------------------------------------------------- GELU epilogue
@pytest.mark.parametrize("M,cin,cout,ws", [(7040, 384, 512, True), (1000, 384, 512, True), (1000, 384, 512, False),
                                            (56320, 384, 512, True), (7040, 512, 384, False)])
def test_gelu_epilogue(gpu, M, cin, cout, ws):
    from ptlflow_amd.packing import pack_conv_weight
    g = torch.Generator().manual_seed(M + cin)
    x = torch.randn(M, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    ref = F.gelu(F.linear(x, w, b))
    out = torch.full((M, cout), float("nan"), device=gpu)
    workspace = torch.zeros(torch.ops.pfk.conv_workspace_bytes(), device=gpu, dtype=torch.uint8) if ws else None
    wp = pack_conv_weight(w[:, :, None, None], [(0, cin, cin)]).to(gpu)
    torch.ops.pfk.conv2d([x.to(gpu)], 1, 1, M, 1, 1, wp, b.to(gpu), cout, 3, False, 1.0, out, None, None, None, workspace)
    torch.cuda.synchronize()
    _close(out, ref)
    # relu together with the GELU epilogue is a bad argument, not a silent choice
    with pytest.raises(RuntimeError):
        torch.ops.pfk.conv2d([x.to(gpu)], 1, 1, M, 1, 1, wp, b.to(gpu), cout, 3, True, 1.0, out, None, None, None, workspace)


def test_gelu_other_entry_points_refuse(gpu):
    """pfk_conv2d_group_f32, pfk_conv2d_bf16s and pfk_conv2d_b16 do not implement PFK_EPI_LINEAR_GELU: an error status, no launch"""
    import ptlflow_amd
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    M, cin, cout = 256, 64, 64
    x = torch.randn(M, cin, device=gpu)
    wt = torch.randn(cout, cin, device=gpu)
    out = torch.zeros(M, cout, device=gpu)
    d = _Desc()
    d.src[0] = _Src(x.data_ptr(), cin, cin)
    d.num_src, d.B, d.H, d.W, d.kh, d.kw = 1, 1, 1, M, 1, 1
    d.weight, d.cout, d.epilogue, d.relu, d.scale = wt.data_ptr(), cout, 3, 0, 1.0
    d.out, d.out_ld = out.data_ptr(), cout
    planes = torch.zeros(1, cout, cin, device=gpu, dtype=torch.bfloat16)
    assert lib.pfk_conv2d_group_f32(ctypes.byref(d), 1, None) < 0
    assert lib.pfk_conv2d_bf16s(ctypes.byref(d), ctypes.c_void_p(planes.data_ptr()), 1, None) < 0
    xb, wb = x.to(torch.bfloat16), wt.to(torch.bfloat16)
    e = _DescB16()
    e.src[0] = _SrcB16(xb.data_ptr(), cin, cin)
    e.num_src, e.B, e.H, e.W, e.kh, e.kw = 1, 1, 1, M, 1, 1
    e.weight, e.cout, e.epilogue, e.relu, e.scale = wb.data_ptr(), cout, 3, 0, 1.0
    e.out, e.out_ld = out.data_ptr(), cout
    assert lib.pfk_conv2d_b16(ctypes.byref(e), None) < 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0
    # while pfk_conv2d_f32 runs it
    assert lib.pfk_conv2d_f32(ctypes.byref(d), None) == 0
    torch.cuda.synchronize()
    wp = wt.cpu()
    _close(out, F.gelu(x.cpu() @ wp.t()))


# ------------------------------------------------------------------------------------------------------------- info upsampling
@pytest.mark.parametrize("B,H,W", [(2, 55, 128), (1, 13, 17)])
def test_convex_upsample_info(gpu, B, H, W):
    from sea_seam_model import upsample_data_torch
    g = torch.Generator().manual_seed(B * 100 + H)
    M = B * H * W
    fo = torch.randn(M, 8, generator=g) * 3        # delta | info | pad, like the engine's flow-head rows
    mask = torch.randn(M, 576, generator=g) * 2
    fo_d, mask_d = fo.to(gpu), mask.to(gpu)
    flow_up = torch.empty(B, 2, 8 * H, 8 * W, device=gpu)
    info_up = torch.empty(B, 4, 8 * H, 8 * W, device=gpu)
    torch.ops.pfk.convex_upsample_info_pm(fo_d[:, :2], fo_d[:, 2:6], mask_d, flow_up, info_up)
    want = torch.empty_like(flow_up)
    torch.ops.pfk.convex_upsample_pm(fo_d[:, :2], mask_d, want)
    torch.cuda.synchronize()
    assert torch.equal(flow_up, want)
    nchw = lambda t: t.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    rf, ri = upsample_data_torch(nchw(fo[:, :2]), nchw(fo[:, 2:6]), nchw(mask))
    torch.testing.assert_close(info_up.cpu(), ri, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(flow_up.cpu(), rf, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------- golden replay
def _seeded_loop(seed, iters=4):
    from sea_seam_model import SeaRaftLoop, load_seeded
    return load_seeded(SeaRaftLoop(iters=iters), seed).eval()


def test_golden_replay(gpu):
    """The reference's own BasicUpdateBlock, flow_head, 0.25 * upsample_weight and upsample_data (scripts/make_sea_raft_golden.py)
    against the seams on the same seeded weights."""
    from ptlflow_amd import patch
    gd = torch.load(GOLDEN)
    model = _seeded_loop(gd["seed"]).to(gpu)
    patch.accelerate(model, sea_raft_update=True)
    try:
        dev = lambda t: t.to(gpu)  # noqa: E731
        corr = dev(gd["corr"]).contiguous(memory_format=torch.channels_last)     # the channel view the B1 hook hands out
        with torch.no_grad():
            net = model.update_block(dev(gd["net"]), dev(gd["inp"]), corr, dev(gd["flow"]))
            fh = model.flow_head(net)
            wu = 0.25 * model.upsample_weight(net)
            up_flow, up_info = model.upsample_data(dev(gd["flow_8x"]), dev(gd["info_8x"]), dev(gd["weight_update"]))
        torch.cuda.synchronize()
        assert model.update_block.calls == 1 and model.flow_head.calls == 1 and model.upsample_weight.calls == 1
        assert model.upsample_data.calls == 1
        _close(net, gd["net_out"])
        _close(fh, gd["flow_update"])
        _close(wu, gd["weight_update"])
        _close(up_flow, gd["up_flow"])
        _close(up_info, gd["up_info"])
    finally:
        patch.restore(model)


# ------------------------------------------------------------------------------------------------------------- whole loop
H8, W8 = 55, 128       # 436 x 1024 frames


def _loop_inputs(B, seed=3):
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(B, 128, H8, W8, generator=g))
    ctx = torch.relu(torch.randn(B, 128, H8, W8, generator=g))
    f1 = torch.randn(B, 256, H8, W8, generator=g) * 0.3
    f2 = torch.roll(f1, shifts=(1, 2), dims=(2, 3)) + 0.1 * torch.randn(B, 256, H8, W8, generator=g)
    return net, ctx, f1, f2


@pytest.fixture(scope="module")
def cpu_loop():
    model = _seeded_loop(11, iters=12)
    x = _loop_inputs(2)
    with torch.no_grad():
        out = model(*x)
    return x, out


def _epe(a, b):
    return float((a.float().cpu() - b.float()).norm(dim=1).mean())


def test_whole_loop(gpu, cpu_loop):
    import sea_seam_model
    from ptlflow_amd import patch
    x, ref = cpu_loop
    model = _seeded_loop(11, iters=12).to(gpu)
    patch.accelerate(model, sea_raft_update=True)
    hook = sea_seam_model.get_corr_block
    corr_calls = [0]

    def counting(*a, **k):
        corr_calls[0] += 1
        return hook(*a, **k)

    sea_seam_model.get_corr_block = counting
    try:
        ub = model.update_block
        assert type(ub).__name__ == "PfkSeaRaftUpdateBlock"
        runs = [((0, 1), 12), ((0, 1), 4), ((0,), 12), ((1,), 12)]     # the last two: a new input after another (no stale state)
        for rows, iters in runs:
            c0 = (ub.calls, model.flow_head.calls, model.upsample_weight.calls, model.upsample_data.calls, corr_calls[0])
            with torch.no_grad():
                out = model(*[t[list(rows)].to(gpu) for t in x], iters=iters)
            torch.cuda.synchronize()
            c1 = (ub.calls, model.flow_head.calls, model.upsample_weight.calls, model.upsample_data.calls, corr_calls[0])
            assert [b - a for a, b in zip(c0, c1)] == [iters, iters, iters, iters + 1, 1], (c0, c1)
            want_flow = ref["flow_preds"][iters][list(rows)]
            want_info = ref["info_preds"][iters][list(rows)]
            epe = _epe(out["flows"][:, 0], want_flow)
            assert epe <= 1e-3, f"rows {rows} iters {iters}: EPE {epe:.3e}"
            assert float((out["info"].cpu() - want_info).abs().max()) <= 1e-3
    finally:
        sea_seam_model.get_corr_block = hook
        patch.restore(model)
    assert sea_seam_model.get_corr_block is not hook and not isinstance(model.update_block, type(ub))


# ------------------------------------------------------------------------------------------------------------- fallbacks
def _fallback_run(model, x, mode):
    # MIOpen's deterministic mode: the reduced-precision convolutions may otherwise pick split-K solvers whose atomics make two
    # runs of the SAME modules differ in the last bits
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return _fallback_run_inner(model, x, mode)


def _fallback_run_inner(model, x, mode):
    if mode == "autocast":
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model(*x)
    if mode == "half":
        with torch.no_grad():
            return model(*[t.half() for t in x])
    return model(*x)          # "grad": parameters require grad, grad mode on: a gradient graph


@pytest.mark.parametrize("mode", ["autocast", "half", "grad"])
def test_fallbacks_are_the_original_modules(gpu, mode):
    from ptlflow_amd import patch
    g = torch.Generator().manual_seed(5)
    B, H, W = 1, 16, 24
    x = [torch.tanh(torch.randn(B, 128, H, W, generator=g)), torch.relu(torch.randn(B, 128, H, W, generator=g)),
         torch.randn(B, 256, H, W, generator=g) * 0.3, torch.randn(B, 256, H, W, generator=g) * 0.3]
    x = [t.to(gpu) for t in x]
    model = _seeded_loop(2, iters=2).to(gpu)
    if mode == "half":
        model = model.half()
    patch.accelerate(model)                       # the default: SEA-RAFT's modules stay the model's own (seam B1 only)
    try:
        want = _fallback_run(model, x, mode)
        again = _fallback_run(model, x, mode)
    finally:
        patch.restore(model)
    assert all(torch.equal(again[k], want[k]) for k in ("flows", "info", "flow_small")), "the unpatched forward is not reproducible"

    patch.accelerate(model, sea_raft_update=True)
    try:
        got = _fallback_run(model, x, mode)
        assert model.update_block.calls == 0 and model.flow_head.calls == 0 and model.upsample_weight.calls == 0
        assert model.upsample_data.calls == 0
    finally:
        patch.restore(model)
    for k in ("flows", "info", "flow_small"):
        assert torch.equal(got[k], want[k]), k
