"""SEA-RAFT's ResNet encoders on the kernels (`accelerate(model, sea_raft_encoders=...)`, ptlflow_amd/sea_encoder.py) on the GPU.

Gates.  Single kernels: the project's stem gates of tests/test_gpu_encoder.py::test_stem — |err| <= 2e-5 (1 + |ref|) for fp32 rows,
2^-8 relative (+ 2e-5) for bf16 rows — against an fp64 `F.conv2d`.  The whole fp32 encoder: 2e-4 relative plus 2e-4 max|ref| absolute, the
gate of `test_basic_encoder` (the fp32 module itself is 7e-7 max|ref| from fp64, so the gate leaves room for kernel rounding only).
bf16 paths: mean and max error against fp64 / the fp32 CPU forward at most twice the error of the CPU forward under
torch.autocast(bfloat16) (the construction of tests/test_gpu_bf16_gate.py), which must be > 0.  Whole forward, fp32: flow EPE <= 1e-3 px
mean and info within 1e-3 of the model's own CPU fp32 forward, the gates of tests/test_gpu_sea_raft.py::test_whole_loop.

The frames are 440 x 1024: what SEA-RAFT's input padder makes of 436 x 1024 (sea_raft.py:166-175; the stand-in does not pad)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from op_gate import close, unpm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sea_raft_encoder.pt")
ENC_SEED = 4100          # scripts/make_sea_raft_golden.py
VARIANTS = (("resnet18", 3), ("resnet18", 6), ("resnet34", 3))


# ------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,relu", [(1, 37, 70, True), (2, 24, 64, False), (3, 65, 131, True), (1, 7, 5, False), (9, 234, 440, True)])
@pytest.mark.parametrize("source", ["one", "halves", "two"])
def test_stem2(gpu, source, B, H, W, relu, out_dtype):
    """Conv2d(3 or 6, 64, 7, stride 2, padding 3): one image pointer, the two channel halves of one [B, 6, H, W] tensor read in place
    (batch stride 6 H W), two separate images.  9 x 234 x 440: 945 tiles, two rounds of the persistent walk (256 workgroups of two
    groups: 512 tiles a round), the second one partial; tests/test_gpu_encoder_gate.py::test_stem_three_rounds reaches a third."""
    cin = 3 if source == "one" else 6
    torch.manual_seed(B * 1000 + H + cin)
    x = torch.randn(B, cin, H, W)
    wt = torch.randn(64, cin, 7, 7) / math.sqrt(49 * cin)
    bias = torch.randn(64) * 0.1
    ref = F.conv2d(x.double(), wt.double(), bias.double(), stride=2, padding=3).float()
    if relu:
        ref = F.relu(ref)
    Ho, Wo = ref.shape[-2:]
    xg = x.to(gpu)
    if source == "one":
        a, b = xg, None
    elif source == "halves":
        a, b = xg[:, :3], xg[:, 3:]
    else:
        a, b = xg[:, :3].contiguous(), xg[:, 3:].contiguous()
    out = torch.full((B * Ho * Wo, 68), 7.0, device=gpu, dtype=out_dtype)
    w = wt.permute(2, 3, 1, 0).reshape(49, cin, 64).contiguous().to(gpu)
    torch.ops.pfk.conv_stem2(a, b, w, bias.to(gpu), out[:, :64], relu)
    again = torch.full_like(out, 7.0)
    torch.ops.pfk.conv_stem2(a, b, w, bias.to(gpu), again[:, :64], relu)
    if out_dtype == torch.bfloat16:   # one rounding of the fp32 result
        close(unpm(out[:, :64], B, Ho, Wo), ref, rtol=2 ** -8, atol=2e-5)
    else:
        close(unpm(out[:, :64], B, Ho, Wo), ref)
    assert bool((out[:, 64:] == 7.0).all()), "the kernel wrote beyond column cout"
    assert torch.equal(out, again), "two runs differ"
    if source == "one":               # the 3-channel stem the other encoders use: the same gate
        old = torch.empty(B * Ho * Wo, 64, device=gpu, dtype=out_dtype)
        torch.ops.pfk.conv_stem(xg, w, bias.to(gpu), old, relu)
        close(out[:, :64], old, rtol=2 ** -8 if out_dtype == torch.bfloat16 else 2e-5)


def test_stem2_refuses_other_widths(gpu):
    x = torch.randn(1, 3, 16, 24, device=gpu)
    for cout in (32, 48):
        w = torch.randn(49, 3, cout, device=gpu)
        with pytest.raises(RuntimeError, match="conv_stem2"):
            torch.ops.pfk.conv_stem2(x, None, w, None, torch.empty(8 * 12, cout, device=gpu), True)


# ------------------------------------------------------------------------------------------------------------- winograd
RATIO = 4.0      # tests/test_gpu_winograd.py: Winograd's max error <= 4 x the direct kernel's + 1e-6


@pytest.mark.parametrize("relu,relu2", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("C,B,H,W", [(64, 1, 220, 512), (128, 2, 110, 256), (256, 3, 55, 128), (64, 1, 55, 128), (256, 1, 109, 255)])
def test_winograd_residual_entry(gpu, C, B, H, W, relu, relu2):
    """pfk_conv2d_wino_res_f32 on the encoder's widths and grids (and an odd one): relu?(conv + bias), + residual, relu? against fp64;
    the error at most 4 x the direct kernel's; two runs give the same bits"""
    from ptlflow_amd.packing import pack_conv_weight, pack_wino_weight
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g)
    wt = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    bias = torch.randn(C, generator=g) * 0.1
    res = torch.randn(B, C, H, W, generator=g)
    ref = F.conv2d(x.to(gpu).double(), wt.to(gpu).double(), bias.to(gpu).double(), padding=1)
    if relu:
        ref = F.relu(ref)
    ref = res.to(gpu).double() + ref
    if relu2:
        ref = F.relu(ref)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, C)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(gpu)      # noqa: E731
    xr, rr, b = rows(x), rows(res), bias.to(gpu)
    M = B * H * W
    out_w, again, out_d = (torch.full((M, C + 4), 7.0, device=gpu) for _ in range(3))
    ww = pack_wino_weight(wt).to(gpu)
    torch.ops.pfk.conv2d_wino_res(xr, B, H, W, ww, b, C, relu, 1.0, out_w[:, :C], rr, relu2)
    torch.ops.pfk.conv2d_wino_res(xr, B, H, W, ww, b, C, relu, 1.0, again[:, :C], rr, relu2)
    wd = pack_conv_weight(wt, [(0, C, C)]).to(gpu)
    torch.ops.pfk.conv2d([xr], B, H, W, 3, 3, wd, b, C, 0, relu, 1.0, out_d[:, :C], None, None, None, None, rr, 1, relu2)
    torch.cuda.synchronize()
    ew = float((out_w[:, :C].double() - ref).abs().max())
    ed = float((out_d[:, :C].double() - ref).abs().max())
    print(f"C {C} {B}x{H}x{W} relu {relu} relu2 {relu2}: wino max err {ew:.3e}, direct {ed:.3e}")
    assert ew <= RATIO * ed + 1e-6, f"wino max err {ew:.3e} vs direct {ed:.3e}"
    assert torch.equal(out_w, again), "two runs differ"
    assert bool((out_w[:, C:] == 7.0).all())


def test_plain_winograd_entry_still_refuses_a_residual(gpu):
    x = torch.randn(48, 64, device=gpu)
    w = torch.randn(16 * 64 * 64, device=gpu)
    out = torch.zeros(48, 64, device=gpu)
    with pytest.raises(RuntimeError, match="conv2d_wino_res"):       # and the new one wants its residual's shape
        torch.ops.pfk.conv2d_wino_res(x, 1, 6, 8, w, None, 64, True, 1.0, out, torch.zeros(48, 32, device=gpu), True)
    import ctypes
    import ptlflow_amd
    from pfk_ctypes import EPI_LINEAR, Desc, Src
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    d = Desc()
    d.src[0] = Src(x.data_ptr(), 64, 64)
    d.num_src, d.B, d.H, d.W, d.kh, d.kw = 1, 1, 6, 8, 3, 3
    d.weight, d.cout, d.epilogue, d.relu, d.scale = w.data_ptr(), 64, EPI_LINEAR, 1, 1.0
    d.out, d.out_ld = out.data_ptr(), 64
    assert lib.pfk_conv2d_wino_res_f32(ctypes.byref(d), None) == -1           # no residual: PFK_ERR_BAD_ARG
    d.residual, d.residual_ld = out.data_ptr(), 64
    assert lib.pfk_conv2d_wino_f32(ctypes.byref(d), None) == -3               # PFK_ERR_UNSUPPORTED, as before
    d.cout_active = 64 * 0 + 32
    assert lib.pfk_conv2d_wino_res_f32(ctypes.byref(d), None) == -3
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0, "a refused launch wrote its output"


# ------------------------------------------------------------------------------------------------------------- engine
def _encoder(pretrain, cin, seed):
    import sea_full_model as M
    return M.load_seeded_encoder(M.ResNetFPN(pretrain=pretrain, input_dim=cin), seed).eval()


def _fp64(enc, x):
    import copy
    with torch.no_grad():
        return copy.deepcopy(enc).double()(x.double())


def _errs(a, ref64):
    e = (a.double().cpu() - ref64).abs()
    return float(e.mean()), float(e.max())


@pytest.mark.parametrize("winograd", [True, "always", False])
@pytest.mark.parametrize("variant", range(3))
def test_engine_fp32(gpu, variant, winograd):
    """ResNetFPNEngine against the module in fp64 and against the reference's own output (the golden), and at an odd size, batch 2;
    with the engine's own Winograd rule (these sizes are below it), Winograd on every stride-1 3x3 convolution, and none"""
    from ptlflow_amd.sea_encoder import ResNetFPNEngine
    pretrain, cin = VARIANTS[variant]
    gold = torch.load(GOLDEN)
    enc = _encoder(pretrain, cin, ENC_SEED + variant)
    eng = ResNetFPNEngine(enc.state_dict(), gpu, "fp32")
    eng.winograd = winograd
    assert sum(k.endswith(".ww") for k in eng.w) == 2 * len(eng.blocks) - 2      # all but the two stride-2 conv1
    g = torch.Generator().manual_seed(variant)
    for x, want in ((gold[f"x{cin}"], gold[f"{pretrain}_{cin}"]), (torch.rand(2, cin, 136, 200, generator=g) * 2 - 1, None)):
        ref = _fp64(enc, x)
        got = eng(x.to(gpu))
        torch.cuda.synchronize()
        assert got.shape == ref.shape and got.dtype == torch.float32
        assert got.permute(0, 2, 3, 1).is_contiguous(), "the output is not the channels-last view CorrBlock takes"
        scale = float(ref.abs().max())
        err = (got.double().cpu() - ref).abs()
        print(f"{pretrain} cin {cin} {tuple(x.shape)}: max err {float(err.max()):.3e}, max |ref| {scale:.3e}")
        assert bool((err <= 2e-4 * ref.abs() + 2e-4 * scale).all()), f"max err {float(err.max()):.3e} at scale {scale:.3e}"
        if want is not None:
            err = (got.cpu() - want).abs()
            assert bool((err <= 2e-4 * want.abs() + 2e-4 * scale).all()), f"against the golden: max err {float(err.max()):.3e}"


@pytest.mark.parametrize("variant", range(3))
def test_engine_bf16(gpu, variant):
    from ptlflow_amd.sea_encoder import ResNetFPNEngine
    pretrain, cin = VARIANTS[variant]
    gold = torch.load(GOLDEN)
    enc = _encoder(pretrain, cin, ENC_SEED + variant)
    x = gold[f"x{cin}"]
    ref = _fp64(enc, x)
    gap_mean, gap_max = _errs(gold[f"{pretrain}_{cin}_autocast"], ref)
    got = ResNetFPNEngine(enc.state_dict(), gpu, "bf16")(x.to(gpu))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32
    mean, mx = _errs(got, ref)
    print(f"{pretrain} cin {cin}: bf16 engine mean {mean:.3e} max {mx:.3e} | autocast-CPU gap mean {gap_mean:.3e} max {gap_max:.3e}")
    assert gap_mean > 0 and gap_max > 0
    assert math.isfinite(mean) and mean <= 2 * gap_mean and mx <= 2 * gap_max


# ------------------------------------------------------------------------------------------------------------- whole forward
SIZES = {"frame": (1, 440, 1024), "odd": (2, 136, 200)}
_CPU = {}


def _cpu_forward(size, autocast=False):
    """the stand-in's own CPU forward, 12 iterations (prediction 4 of it is the 4-iteration forward's), once per process"""
    import sea_full_model as M
    key = (size, autocast)
    if key not in _CPU:
        B, H, W = SIZES[size]
        x = M.smooth_images(B, H, W, seed=7)
        model = M.seeded_full(21, iters=12)
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            out = model(*x)
        _CPU[key] = (x, {"flow_preds": [t.float() for t in out["flow_preds"]], "info_preds": [t.float() for t in out["info_preds"]]})
    return _CPU[key]


def _epe(a, b):
    return float((a.float().cpu() - b.float()).norm(dim=1).mean())


def _counters(model, corr_calls):
    return (model.fnet.calls, model.cnet.calls, model.init_conv.calls, model.update_block.calls, model.flow_head.calls,
            model.upsample_weight.calls, model.upsample_data.calls, corr_calls[0])


def _count_corr(M, corr_calls):
    hook = M.get_corr_block

    def counting(*a, **k):
        corr_calls[0] += 1
        return hook(*a, **k)

    M.get_corr_block = counting
    return hook


@pytest.mark.parametrize("size", ["frame", "odd"])
def test_whole_forward(gpu, size):
    import sea_full_model as M
    from ptlflow_amd import patch
    x, ref = _cpu_forward(size)
    model = M.seeded_full(21, iters=12).to(gpu)
    patch.accelerate(model, sea_raft_update=True, sea_raft_encoders=True)
    corr_calls = [0]
    hook = _count_corr(M, corr_calls)
    try:
        assert type(model.fnet).__name__ == type(model.cnet).__name__ == "PfkResNetEncoder" and type(model.init_conv).__name__ == "PfkInitConv"
        for iters in (12, 4):
            c0 = _counters(model, corr_calls)
            with torch.no_grad():
                out = model(*[t.to(gpu) for t in x], iters=iters)
            torch.cuda.synchronize()
            delta = [b - a for a, b in zip(c0, _counters(model, corr_calls))]
            # fnet twice, cnet, init_conv, the block `iters` times, every one of the iters + 1 predictions' heads and upsampling
            assert delta == [2, 1, 1, iters, iters + 1, iters + 1, iters + 1, 1], delta
            epe = _epe(out["flows"][:, 0], ref["flow_preds"][iters])
            info = float((out["info"].cpu() - ref["info_preds"][iters]).abs().max())
            print(f"{size} iters {iters}: EPE {epe:.3e}, info max err {info:.3e}, max |flow| {float(ref['flow_preds'][iters].abs().max()):.1f}")
            assert epe <= 1e-3, f"iters {iters}: EPE {epe:.3e}"
            assert info <= 1e-3, f"iters {iters}: info {info:.3e}"
            epe0 = _epe(out["flow_preds"][0], ref["flow_preds"][0])
            assert epe0 <= 1e-3, f"the iteration-0 prediction: EPE {epe0:.3e}"
    finally:
        M.get_corr_block = hook
        patch.restore(model)
    assert type(model.fnet).__name__ == "ResNetFPN" and type(model.init_conv).__name__ == "Conv2d"


@pytest.mark.parametrize("mode", ["autocast", "fp32"])
@pytest.mark.parametrize("size", ["frame", "odd"])
def test_whole_forward_bf16(gpu, size, mode):
    import sea_full_model as M
    from ptlflow_amd import patch
    iters = 4
    x, ref = _cpu_forward(size)
    _, ref_ac = _cpu_forward(size, autocast=True)
    gap_flow = _epe(ref_ac["flow_preds"][iters], ref["flow_preds"][iters])
    gap_info = float((ref_ac["info_preds"][iters] - ref["info_preds"][iters]).abs().mean())
    assert gap_flow > 0 and gap_info > 0
    model = M.seeded_full(21, iters=iters).to(gpu)
    patch.accelerate(model, sea_raft_update="bf16", sea_raft_encoders="bf16")
    corr_calls = [0]
    hook = _count_corr(M, corr_calls)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "autocast"):
            out = model(*[t.to(gpu) for t in x])
        torch.cuda.synchronize()
        assert _counters(model, corr_calls) == (2, 1, 1, iters, iters + 1, iters + 1, iters + 1, 1)
        e_flow = _epe(out["flows"][:, 0], ref["flow_preds"][iters])
        e_info = float((out["info"].float().cpu() - ref["info_preds"][iters]).abs().mean())
        print(f"{size} {mode}: flow EPE {e_flow:.3e} (autocast-CPU gap {gap_flow:.3e}), info {e_info:.3e} (gap {gap_info:.3e})")
        assert math.isfinite(e_flow) and math.isfinite(e_info)
        assert e_flow <= 2 * gap_flow, f"flow EPE {e_flow:.3e} vs the autocast gap {gap_flow:.3e}"
        assert e_info <= 2 * gap_info, f"info error {e_info:.3e} vs the autocast gap {gap_info:.3e}"
    finally:
        M.get_corr_block = hook
        patch.restore(model)


# ------------------------------------------------------------------------------------------------------------- fallbacks
def _run(model, x, mode):
    # MIOpen's deterministic mode: two runs of the SAME modules may otherwise differ in the last bits
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        if mode == "half":
            with torch.no_grad():
                return model(*[t.half() for t in x])
        if mode == "fp16_autocast":
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return model(*x)
        return model(*x)          # "grad": parameters require grad, grad mode on; "train": train mode


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["train", "grad", "half", "fp16_autocast", "cpu"])
def test_fallbacks_are_the_original_modules(gpu, mode, precision):
    import sea_full_model as M
    from ptlflow_amd import patch
    x = M.smooth_images(1, 128, 192, seed=3)
    model = M.seeded_full(5, iters=2)
    dev = torch.device("cpu") if mode == "cpu" else gpu
    model = model.to(dev)
    x = [t.to(dev) for t in x]
    if mode == "half":
        model = model.half()
    if mode == "train":
        model.train()          # BatchNorm on batch statistics (and updating the running ones: both runs start from a copy)
    import copy
    state = copy.deepcopy(model.state_dict())
    patch.accelerate(model)                       # the default: the encoders stay the model's own
    try:
        assert type(model.fnet).__name__ == "ResNetFPN"
        want = _run(model, x, mode)
    finally:
        patch.restore(model)
    model.load_state_dict(state)
    patch.accelerate(model, sea_raft_encoders=precision)
    try:
        got = _run(model, x, mode)
        assert (model.fnet.calls, model.cnet.calls, model.init_conv.calls) == (0, 0, 0)
    finally:
        patch.restore(model)
    for k in ("flows", "info", "flow_small"):
        assert torch.equal(got[k], want[k]), k
