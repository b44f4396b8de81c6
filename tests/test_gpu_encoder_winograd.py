"""BasicEncoder's stride-1 3x3 convolutions on the Winograd F(2x2,3x3) kernels (`EncoderEngine.winograd`, `encoder.WINO_MIN_PIXELS`).

Kernel level: `pfk_conv2d_wino_f32` / `pfk_conv2d_wino_res_f32` at the widths and epilogues the engine launches (64, 96 -- padded to 128
columns --, 128; plain in front of an instance norm, + relu, + relu + residual + relu) against an fp64 convolution.  Gate, as in
test_gpu_winograd.py: the Winograd kernel's max |error| is at most 4x the direct kernel's (`pfk_conv2d_f32`) on the same inputs.

Engine level: Winograd on against off, an instance-norm, a folded-BatchNorm and a norm-free encoder, at a size the rule takes at every
width and one it takes at none;
every output against the CPU oracle with test_basic_encoder's tolerance (2e-4 of the output's scale)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import raft_oracle as O
from op_gate import pm, unpm

pytestmark = pytest.mark.gpu

EPI_LINEAR = 0
RATIO = 4.0


@pytest.mark.parametrize("form", ["plain", "relu", "res"])
@pytest.mark.parametrize("B,H,W,C", [(1, 218, 512, 64), (2, 109, 256, 96), (2, 55, 128, 128), (3, 27, 35, 96), (1, 33, 47, 64)])
def test_kernels_at_encoder_shapes(gpu, B, H, W, C, form):
    from ptlflow_amd.packing import pack_conv_weight, pack_wino_weight
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, H, W, generator=g)
    wt = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9)
    bias = torch.randn(C, generator=g)
    res = torch.randn(B, C, H, W, generator=g)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    if form != "plain":
        ref = F.relu(ref)
    if form == "res":
        ref = F.relu(res.double() + ref)
    ops = torch.ops.pfk
    src, r = pm(x, "cuda"), pm(res, "cuda")
    ow = torch.zeros(B * H * W, C, device=gpu)
    od = torch.zeros(B * H * W, C, device=gpu)
    ww, wd = pack_wino_weight(wt).cuda(), pack_conv_weight(wt, [(0, C, C)]).cuda()
    if form == "res":
        ops.conv2d_wino_res(src, B, H, W, ww, bias.cuda(), C, True, 1.0, ow, r, True)
        ops.conv2d([src], B, H, W, 3, 3, wd, bias.cuda(), C, EPI_LINEAR, True, 1.0, od, None, None, None, None, r, 1, True)
    else:
        ops.conv2d_wino(src, B, H, W, ww, bias.cuda(), C, form == "relu", 1.0, ow, 0)
        ops.conv2d([src], B, H, W, 3, 3, wd, bias.cuda(), C, EPI_LINEAR, form == "relu", 1.0, od, None, None, None)
    ew = (unpm(ow, B, H, W).double() - ref).abs().max().item()
    ed = (unpm(od, B, H, W).double() - ref).abs().max().item()
    print(f"B{B} {H}x{W} C{C} {form}: wino max err {ew:.3e}, direct {ed:.3e}, ratio {ew / max(ed, 1e-30):.2f}")
    assert ew <= RATIO * ed + 1e-6, f"wino max err {ew:.3e} vs direct {ed:.3e}"


def _encoder_params(kind, out_dim, seed):
    from ptlflow_amd.raft import Encoder
    from ptlflow_amd.synth import synth_state_dict
    own = Encoder(out_dim, kind, False).state_dict()
    shapes = {"fnet." + k: tuple(v.shape) for k, v in own.items()}      # "fnet." prefix: the encoder init statistics
    return {k[len("fnet."):]: v for k, v in synth_state_dict(shapes, seed).items()}


def _wino_launches(eng, B, H, W):
    """the stride-1 3x3 convolutions of a B x H x W forward that `_use_wino` sends to Winograd"""
    taken = []
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for name, _cin, cout, stride, _ds in eng.blocks:
        if stride == 1 and eng._use_wino(f"{name}.conv1", cout, B * h * w):
            taken.append(f"{name}.conv1")
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
        if eng._use_wino(f"{name}.conv2", cout, B * h * w):
            taken.append(f"{name}.conv2")
    return taken


@pytest.mark.parametrize("kind", ["instance", "batch", "none"])
@pytest.mark.parametrize("B,H,W,takes", [(2, 436, 1024, True), (2, 64, 96, False)])
def test_engine_winograd_on_off(gpu, kind, B, H, W, takes):
    from ptlflow_amd.encoder import EncoderEngine
    P = _encoder_params(kind, 256, seed=17)
    x = (O.smooth_pair(B, H, W, seed=9)[:, 0] - 0.5) * 2.0
    ref = O.encoder(P, x, kind)
    eng = EncoderEngine(P, kind, gpu)
    assert eng.winograd is True
    taken = _wino_launches(eng, B, H, W)
    assert bool(taken) == takes
    if takes:       # two 436 x 1024 frames reach the threshold of every width: layer1 (64), layer2 (96) and layer3 (128) all launch it
        assert {k.split(".")[0] for k in taken} == {"layer1", "layer2", "layer3"}
    on = eng(x.cuda()).cpu()
    eng.winograd = False
    assert _wino_launches(eng, B, H, W) == []
    off = eng(x.cuda()).cpu()
    scale = float(ref.abs().max())
    for name, out in (("winograd", on), ("direct", off)):
        err = (out - ref).abs()
        print(f"{kind} {B}x{H}x{W} {name}: max err {err.max().item():.3e} (ref max {scale:.3e})")
        assert bool((err <= 2e-4 * scale + 2e-4 * ref.abs()).all()), f"{name}: max err {err.max().item():.3e} (ref max {scale:.3e})"
    if takes:
        assert not torch.equal(on, off), "the Winograd path was not taken"
    else:
        assert torch.equal(on, off), "a launch below the thresholds took another kernel"


def test_other_engines_pack_no_winograd_weight(gpu):
    """bf16, split-bf16 and the small encoder are untouched: no transformed weight, no Winograd launch"""
    from ptlflow_amd.encoder import EncoderEngine
    from ptlflow_amd.raft import Encoder
    from ptlflow_amd.synth import synth_state_dict
    P = _encoder_params("batch", 256, seed=17)
    for precision in ("bf16", "bf16x3"):
        assert not any(k.endswith(".ww") for k in EncoderEngine(P, "batch", gpu, precision).w)
    own = Encoder(128, "instance", True).state_dict()
    Ps = {k[len("fnet."):]: v for k, v in synth_state_dict({"fnet." + k: tuple(v.shape) for k, v in own.items()}, 3).items()}
    assert not any(k.endswith(".ww") for k in EncoderEngine(Ps, "instance", gpu, "fp32", small=True).w)
