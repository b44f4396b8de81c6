"""The instance norms of the fp32 feature encoder folded into the Winograd launches around them.

* `conv2d_wino_norm` (`pfk_conv2d_wino_norm_f32`): the norm in front of the convolution applied to the taps on load.  Held to the bits
  of `norm_apply` followed by `conv2d_wino` on the same data.
* `conv2d_wino_stats` (`pfk_conv2d_wino_stats_f32`): mean / rstd of the norm behind the convolution out of its epilogue.  The output is
  held to the bits of the plain launch (the tile list is laid out per image here, another mapping of tiles to blocks), mean / rstd to
  float64 statistics of that output at the gate of `test_gpu_encoder.py::test_instance_norm` (rtol 1e-5, atol 1e-6), and a second
  launch to the first one's bits.  How many values differ from `instnorm_stats` (another order of the double sums) is printed.
* `norm_apply_res` (`pfk_norm_apply_res_f32`): the block's last apply with a raw residual normalised in flight, held to the bits of
  the two `norm_apply` launches.
* `EncoderEngine.fuse_norms`: True against False, whole batch and one-image chunks, with every Winograd threshold patched to 0.

Shapes, the smallest at which the paths can go wrong:
  A  2 x 5x7    64 -> 64   12 tiles per image: one block spans both images (its threads read two images' statistics); odd H and W
  B  3 x 9x13   96 -> 96   35 tiles per image: several blocks hold an image boundary; 32 pad columns in the second column block
  C  2 x 18x26  64 -> 64   117 tiles per image: more than one block per image, not a multiple of 32
Input channels carry offsets of several units, so a padding tap that was normalised instead of left at zero shows.
"""
import contextlib
import functools

import pytest
import torch

from op_gate import close

pytestmark = pytest.mark.gpu

EPS = 1e-5
SHAPES = {"A": (2, 5, 7, 64), "B": (3, 9, 13, 96), "C": (2, 18, 26, 64)}


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """raw rows [B*H*W, C] with per-channel offsets and spreads, a 3x3 weight (transformed) and a bias; CPU generator, fixed seed"""
    from ptlflow_amd.packing import pack_wino_weight
    B, H, W, C = SHAPES[shape]
    g = torch.Generator().manual_seed(160 + C + H)
    x = torch.randn(B * H * W, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + (torch.rand(C, generator=g) * 10 - 5)
    w = torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5
    bias = torch.randn(C, generator=g)
    return x, pack_wino_weight(w), bias


def _stats(ops, x, B, HW):
    C = x.shape[1]
    mean, rstd = torch.empty(B * C, device=x.device), torch.empty(B * C, device=x.device)
    ws = torch.empty(ops.instnorm_workspace_bytes(B, C), device=x.device, dtype=torch.uint8)
    ops.instnorm_stats(x, B, HW, EPS, mean, rstd, ws)
    return mean, rstd


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_normalise_on_load(gpu, shape, relu):
    ops = torch.ops.pfk
    B, H, W, C = SHAPES[shape]
    x, ww, bias = (t.to(gpu) for t in _inputs(shape))
    mean, rstd = _stats(ops, x, B, H * W)
    xn = torch.empty_like(x)
    ops.norm_apply(x, mean, rstd, None, xn, B, H * W, relu, False)
    ref, got = torch.empty(B * H * W, C, device=gpu), torch.full((B * H * W, C), float("nan"), device=gpu)
    ops.conv2d_wino(xn, B, H, W, ww, bias, C, False, 1.0, ref, 0)
    ops.conv2d_wino_norm(x, B, H, W, ww, bias, C, False, 1.0, got, mean, rstd, relu)
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} values differ, max {(got - ref).abs().max().item():.3e}"


@pytest.mark.parametrize("shape,norm,big_mean", [("A", False, False), ("A", True, True), ("B", True, False), ("B", False, True),
                                                 ("C", True, False), ("C", False, False)])
def test_statistics_in_the_epilogue(gpu, shape, norm, big_mean):
    ops = torch.ops.pfk
    B, H, W, C = SHAPES[shape]
    x, ww, bias = (t.to(gpu) for t in _inputs(shape))
    M = B * H * W
    ref = torch.empty(M, C, device=gpu)
    im, ir = _stats(ops, x, B, H * W) if norm else (None, None)

    def plain():
        if norm:
            ops.conv2d_wino_norm(x, B, H, W, ww, bias, C, False, 1.0, ref, im, ir, True)
        else:
            ops.conv2d_wino(x, B, H, W, ww, bias, C, False, 1.0, ref, 0)
    plain()
    if big_mean:                 # channel 3 gets a mean of 10^4 times its spread through the bias
        bias = bias.clone()
        bias[3] += 1.0e4 * ref[:, 3].std() - ref[:, 3].mean()
        plain()
    need = ops.conv_wino_stats_workspace_bytes(B, H, W, C)
    assert need == 2 * B * -(-(((H + 1) // 2) * ((W + 1) // 2)) // 32) * C * 8
    runs = []
    for fill in (0xFF, 0x00):        # the workspace needs no clearing: NaN patterns, then zeros
        ws = torch.full((need,), fill, device=gpu, dtype=torch.uint8)
        out = torch.full((M, C), float("nan"), device=gpu)
        mean, rstd = torch.full((B * C,), float("nan"), device=gpu), torch.full((B * C,), float("nan"), device=gpu)
        ops.conv2d_wino_stats(x, B, H, W, ww, bias, C, out, im, ir, True, EPS, mean, rstd, ws)
        runs.append((out, mean, rstd))
    out, mean, rstd = runs[0]
    assert torch.equal(out, ref), f"{(out != ref).sum().item()} of {ref.numel()} output values differ from the plain launch"
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "a second launch gave other bits"
    o64 = ref.double().view(B, H * W, C)
    if big_mean:
        m, s = o64[:, :, 3].mean(), o64[:, :, 3].std()
        assert abs(m) > 9e3 * s, (m, s)
    close(mean.view(B, C), o64.mean(dim=1), rtol=1e-5, atol=1e-6, dtype=torch.float64)
    close(rstd.view(B, C), 1.0 / torch.sqrt(o64.var(dim=1, unbiased=False) + EPS), rtol=1e-5, atol=1e-6, dtype=torch.float64)
    pm, pr = _stats(ops, ref, B, H * W)
    print(f"[{shape} norm={norm} big_mean={big_mean}] values that differ from instnorm_stats: mean {(pm != mean).sum().item()}, "
          f"rstd {(pr != rstd).sum().item()} of {B * C}")


@pytest.mark.parametrize("relu,res_relu,relu2", [(True, True, True), (True, False, True), (False, False, False), (False, True, True)])
def test_apply_with_normalised_residual(gpu, relu, res_relu, relu2):
    ops = torch.ops.pfk
    B, H, W, C = SHAPES["B"]
    HW = H * W
    x = _inputs("B")[0].to(gpu)
    res = (_inputs("B")[0].flip(0) * 0.7 + 1.5).contiguous().to(gpu)
    m, r = _stats(ops, x, B, HW)
    rm, rr = _stats(ops, res, B, HW)
    resn, ref = torch.empty_like(res), torch.empty_like(x)
    ops.norm_apply(res, rm, rr, None, resn, B, HW, res_relu, False)
    ops.norm_apply(x, m, r, resn, ref, B, HW, relu, relu2)
    got = x.clone()
    ops.norm_apply_res(got, m, r, res, rm, rr, res_relu, got, B, HW, relu, relu2)      # in place, as the engine calls it
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} values differ"


@contextlib.contextmanager
def _zero_thresholds(table):
    saved = dict(table)
    for k in table:
        table[k] = 0
    try:
        yield
    finally:
        table.update(saved)


@pytest.mark.parametrize("one_image_chunks", [False, True])
def test_engine_fuse_norms(gpu, one_image_chunks):
    """2 x 3 x 72 x 104 (grids 36x52, 18x26, 9x13) with every Winograd threshold at 0, as tests/test_gpu_engine_bits.py runs it"""
    from ptlflow_amd import encoder as E
    from ptlflow_amd.raft import Encoder
    from ptlflow_amd.synth import synth_state_dict
    shapes = {"fnet." + k: tuple(v.shape) for k, v in Encoder(256, "instance", False).state_dict().items()}
    P = {k[len("fnet."):]: v for k, v in synth_state_dict(shapes, 21).items()}
    eng = E.EncoderEngine(P, "instance", gpu, "fp32")
    assert eng.fuse_norms is True
    if one_image_chunks:
        eng.max_matrix_bytes = 36 * 52 * 128 * 4
    img = (torch.rand(2, 3, 72, 104, generator=torch.Generator().manual_seed(103)) * 2 - 1).to(gpu)
    with _zero_thresholds(E.WINO_MIN_PIXELS):
        eng.fuse_norms = False
        ref = eng(img).clone()
        eng.fuse_norms = True
        separate = eng._inorm

        def refuse(*a, **k):
            raise AssertionError("a separate norm pass in the fused forward")
        eng._inorm = refuse            # every norm of this forward has a Winograd neighbour or goes through _stats / norm_apply
        try:
            got = eng(img).clone()
        finally:
            eng._inorm = separate
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} values differ, max {(got - ref).abs().max().item():.3e}"
