"""Parity of the split-bf16 convolution path (pfk_conv2d_bf16s, include/pfk.h) against the same oracle as the fp32 path.

nsplit = number of bf16 planes per operand; kept product terms a_i*b_j with i + j < nsplit:
  * nsplit 3 ("bf16x6"): fp32-grade — held to the fp32 kernels' tolerance (2e-5) and to the headline EPE gate (1e-3 px);
  * nsplit 2 ("bf16x3"): ~2^-17 relative product error — 2e-4 on single convolutions;
  * nsplit 1 ("bf16"):   plain bf16 operands, fp32 accumulate (what the reference computes under bf16 autocast) — the
    bound is the operand rounding itself, 2^-8 relative per product; and EXACT-grade (fp32 tolerance) when the operands
    are bf16-representable, which pins the indexing / padding / epilogue logic independently of rounding.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import raft_oracle as O
from op_gate import close, pm, unpm

pytestmark = pytest.mark.gpu

EPI_LINEAR, EPI_GRU_ZR, EPI_GRU_Q = 0, 1, 2
TOL = {3: 2e-5, 2: 2e-4, 1: 4e-2}


def planes(weight, segs, nsplit):
    from ptlflow_amd.packing import pack_conv_weight, split_bf16_planes
    return split_bf16_planes(pack_conv_weight(weight, segs), nsplit).cuda()


CASES = [
    (1, 12, 20, 64, 96, 3, 3, True),
    (2, 9, 7, 324, 256, 1, 1, True),      # convc1: 324 channels -> 6 K-steps of 64, the last one 4 channels wide
    (1, 17, 33, 128, 126, 3, 3, True),    # cout not a multiple of 64
    (1, 11, 19, 36, 40, 5, 1, False),     # a single partial K-step per tap
    (1, 55, 128, 128, 64, 3, 3, True),
]


@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("B,H,W,cin,cout,kh,kw,relu", CASES)
def test_split_conv_linear(gpu, nsplit, B, H, W, cin, cout, kh, kw, relu):
    torch.manual_seed(3)
    x = torch.randn(B, cin, H, W)
    wt = torch.randn(cout, cin, kh, kw) / math.sqrt(cin * kh * kw)
    bias = torch.randn(cout)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=(kh // 2, kw // 2))
    if relu:
        ref = F.relu(ref)
    ref = (ref * 0.25).float()
    M = B * H * W
    buf = torch.full((M, cout + 12), 5.0, device=gpu)
    out = buf[:, 4:4 + cout]
    torch.ops.pfk.conv2d([pm(x, "cuda")], B, H, W, kh, kw, planes(wt, [(0, cin, cin)], nsplit), bias.cuda(), cout, EPI_LINEAR, relu,
                         0.25, out, None, None, None)
    close(unpm(out, B, H, W), ref, rtol=TOL[nsplit], atol=TOL[nsplit])
    assert bool((buf[:, :4] == 5.0).all()) and bool((buf[:, 4 + cout:] == 5.0).all()), "wrote outside its channel slice"


@pytest.mark.parametrize("B,H,W,cin,cout,kh,kw,relu", CASES)
def test_plain_bf16_is_exact_on_bf16_operands(gpu, B, H, W, cin, cout, kh, kw, relu):
    """bf16-representable operands: products are exact in fp32, only the accumulation order differs."""
    torch.manual_seed(4)
    x = torch.randn(B, cin, H, W).bfloat16().float()
    wt = (torch.randn(cout, cin, kh, kw) / math.sqrt(cin * kh * kw)).bfloat16().float()
    bias = torch.randn(cout)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=(kh // 2, kw // 2)).float()
    if relu:
        ref = F.relu(ref)
    out = torch.zeros(B * H * W, cout, device=gpu)
    torch.ops.pfk.conv2d([pm(x, "cuda")], B, H, W, kh, kw, planes(wt, [(0, cin, cin)], 1), bias.cuda(), cout, EPI_LINEAR, relu, 1.0,
                         out, None, None, None)
    close(unpm(out, B, H, W), ref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("nsplit", [2, 3])
def test_split_conv_multi_source(gpu, nsplit):
    torch.manual_seed(5)
    B, H, W = 1, 14, 18
    ca, cb, cc, cout = 96, 148, 32, 128
    a, b, c = torch.randn(B, ca, H, W), torch.randn(B, cb, H, W), torch.randn(B, cc, H, W)
    b[:, 146:] = 0
    wt = torch.randn(cout, ca + 146 + cc, 3, 3) / 40
    bias = torch.randn(cout)
    ref = F.conv2d(torch.cat([a, b[:, :146], c], 1).double(), wt.double(), bias.double(), padding=1).float()
    wide = torch.zeros(B * H * W, 300, device=gpu)
    wide[:, 100:248] = pm(b, "cuda")
    w = planes(wt, [(0, ca, ca), (ca, 146, 148), (ca + 146, cc, cc)], nsplit)
    out = torch.zeros(B * H * W, cout, device=gpu)
    torch.ops.pfk.conv2d([pm(a, "cuda"), wide[:, 100:248], pm(c, "cuda")], B, H, W, 3, 3, w, bias.cuda(), cout, EPI_LINEAR, False, 1.0,
                         out, None, None, None)
    close(unpm(out, B, H, W), ref, rtol=TOL[nsplit], atol=TOL[nsplit])


@pytest.mark.parametrize("B,H,W,Ch,Cx,passes", [
    (1, 12, 16, 128, 256, ((1, 5, "1"), (5, 1, "2"))),
    (2, 10, 14, 96, 148, ((3, 3, ""),)),
])
def test_split_gru_bf16x6(gpu, B, H, W, Ch, Cx, passes):
    torch.manual_seed(6)
    P = {}
    for kh, kw, sfx in passes:
        for k in "zrq":
            P[f"gru.conv{k}{sfx}.weight"] = torch.randn(Ch, Ch + Cx, kh, kw) / math.sqrt((Ch + Cx) * kh * kw)
            P[f"gru.conv{k}{sfx}.bias"] = torch.randn(Ch) * 0.1
    h = torch.tanh(torch.randn(B, Ch, H, W))
    x = torch.randn(B, Cx, H, W)
    ref = O.sepconv_gru(P, h, x) if len(passes) == 2 else O.conv_gru(P, h, x)
    M = B * H * W
    hx = torch.cat([pm(h, "cuda"), pm(x, "cuda")], 1).contiguous()
    z = torch.zeros(M, Ch, device=gpu)
    rh = torch.zeros(M, Ch, device=gpu)
    for kh, kw, sfx in passes:
        wzr = planes(torch.cat([P[f"gru.convz{sfx}.weight"], P[f"gru.convr{sfx}.weight"]], 0), [(0, Ch + Cx, Ch + Cx)], 3)
        bzr = torch.cat([P[f"gru.convz{sfx}.bias"], P[f"gru.convr{sfx}.bias"]]).cuda()
        wq = planes(P[f"gru.convq{sfx}.weight"], [(0, Ch, Ch), (Ch, Cx, Cx)], 3)
        bq = P[f"gru.convq{sfx}.bias"].cuda()
        torch.ops.pfk.conv2d([hx], B, H, W, kh, kw, wzr, bzr, 2 * Ch, EPI_GRU_ZR, False, 1.0, None, hx[:, :Ch], z, rh)
        torch.ops.pfk.conv2d([rh, hx[:, Ch:]], B, H, W, kh, kw, wq, bq, Ch, EPI_GRU_Q, False, 1.0, None, hx[:, :Ch], z, None)
    close(unpm(hx[:, :Ch], B, H, W), ref, rtol=2e-5, atol=3e-5)


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 74, 75, 76, 84, 85, 86])
def test_split_conv_every_tile_configuration(gpu, tile):
    """The tile configurations of the split kernel forced one by one (`debug_set_tile(100 + t)`: 64x64, 128x64, 128x128 with
    four waves, 128x128 / 256x128 / 128x256 with eight waves) through the linear cases (ragged M, cout 40 / 96 / 126, partial
    K-steps) at 1, 2 and 3 planes and through both fused GRU epilogues.  On the eight-wave tiles (4-6) three planes stage their
    weight planes by LDS-DMA (round 4, the default); 70 + t forces the register-staged path of the same tile, 80 + t the DMA path
    for two planes as well."""
    torch.ops.pfk.debug_set_tile(100 + tile)
    try:
        for nsplit in (1, 2, 3):
            for case in CASES:
                test_split_conv_linear(gpu, nsplit, *case)
            if nsplit > 1:
                test_split_conv_multi_source(gpu, nsplit)
        for case in CASES:
            test_plain_bf16_is_exact_on_bf16_operands(gpu, *case)
        test_split_gru_bf16x6(gpu, 1, 12, 16, 128, 256, ((1, 5, "1"), (5, 1, "2")))
        test_split_gru_bf16x6(gpu, 2, 10, 14, 96, 148, ((3, 3, ""),))
    finally:
        torch.ops.pfk.debug_set_tile(100)


@pytest.mark.parametrize("nsplit", [2, 3])
def test_split_conv_tail_split(gpu, nsplit):
    """A grid of 2.15 rounds of one-block-per-CU tiles (275 row tiles x 2 column tiles of 128x256): `launch_bf` gives the two whole
    rounds to the big tiles and rows 32768.. to the eight-wave 128x128 tile in a second launch.  Checked against float64 on the
    first image (first launch only) and on the last one (which holds the split row), and against the un-split launch."""
    torch.manual_seed(17)
    B, H, W, cin, cout = 5, 55, 128, 64, 512
    x = torch.randn(B, cin, H, W)
    wt = torch.randn(cout, cin, 3, 3) / math.sqrt(cin * 9)
    bias = torch.randn(cout)
    w = planes(wt, [(0, cin, cin)], nsplit)
    xp = pm(x, "cuda")
    outs = []
    for knob in (100, 190):                    # heuristic with / without the tail split
        torch.ops.pfk.debug_set_tile(knob)
        try:
            out = torch.zeros(B * H * W, cout, device=gpu)
            torch.ops.pfk.conv2d([xp], B, H, W, 3, 3, w, bias.cuda(), cout, EPI_LINEAR, True, 1.0, out, None, None, None)
            outs.append(out)
        finally:
            torch.ops.pfk.debug_set_tile(100)
    for b in (0, B - 1):
        ref = F.relu(F.conv2d(x[b:b + 1].double(), wt.double(), bias.double(), padding=1)).float()
        got = unpm(outs[0][b * H * W:(b + 1) * H * W], 1, H, W)
        close(got, ref, rtol=TOL[nsplit], atol=TOL[nsplit])
    # the two schedules differ only in the term order of the 2^-16 products on the rows that changed kernel
    assert (outs[0] - outs[1]).abs().max().item() <= TOL[nsplit]
    assert torch.equal(outs[0][:32768], outs[1][:32768]), "the rows of the whole rounds run the same kernel either way"


def _epe(precisions, H, W, iters, small=False, seed=1234):
    from ptlflow_amd.raft import RAFT
    base = RAFT(small=small, iters=iters).load_synthetic(seed).eval()
    P = {k: v.clone() for k, v in base.state_dict().items()}
    x = O.smooth_pair(1, H, W, seed)
    from _cpu_cache import cpu_forward
    ref = cpu_forward("raft", P, x, iters, small=small, key=("synthetic", seed, "smooth", seed))
    res = {}
    for prec in precisions:
        model = RAFT(small=small, iters=iters, conv_precision=prec).eval()
        model.load_state_dict(P)
        out = model.cuda()({"images": x.cuda()})
        torch.cuda.synchronize()
        res[prec] = O.epe(out["flows"][:, 0].cpu(), ref["flows"][:, 0])
    return res


@pytest.mark.parametrize("small", [False, True])
def test_raft_bf16x6_meets_fp32_gate(gpu, small):
    mean, mx = _epe(["bf16x6"], 184, 320, 12, small=small)["bf16x6"]
    print(f"bf16x6 EPE mean {mean:.3e} max {mx:.3e}")
    assert mean <= 1e-3 and mx <= 1e-2


def test_raft_headline_split_modes(gpu):
    """BASELINE.json configs[1] (436x1024, 32 iterations): EPE of each split mode against the fp32 CPU oracle.
    bf16x6 is held to the north-star gate; bf16x3 / bf16 are reduced-precision modes and only bounded loosely."""
    res = _epe(["bf16x6", "bf16x3", "bf16"], 436, 1024, 32)
    for p, (mean, mx) in res.items():
        print(f"headline EPE {p}: mean {mean:.3e} max {mx:.3e}")
    assert res["bf16x6"][0] <= 1e-3 and res["bf16x6"][1] <= 1e-2
    assert res["bf16x3"][0] <= 2e-2
    # plain bf16 (config 3) has its own gate: tests/test_gpu_bf16_gate.py


def test_gma_split_modes(gpu):
    """BASELINE.json configs[2] (gma, shared CorrBlock / GRU path): C_in = 512 SepConvGRU, to_v conv and both encoders on the
    split kernels; bf16x6 inside the fp32 gate, plain bf16 (what bf16 autocast computes in its convolutions) loosely bounded."""
    from ptlflow_amd.raft import GMA
    base = GMA(iters=6).load_synthetic(77).eval()
    P = {k: v.clone() for k, v in base.state_dict().items()}
    x = O.smooth_pair(1, 184, 248, seed=9)
    ref = O.gma_forward(P, x, iters=6)
    res = {}
    for prec in ("bf16x6", "bf16x3", "bf16"):
        m = GMA(iters=6, conv_precision=prec).eval()
        m.load_state_dict(P)
        out = m.cuda()({"images": x.cuda()})
        res[prec] = O.epe(out["flows"][:, 0].cpu(), ref["flows"][:, 0])
        print(f"gma {prec}: EPE mean {res[prec][0]:.3e} max {res[prec][1]:.3e}")
    assert res["bf16x6"][0] <= 1e-3 and res["bf16x6"][1] <= 1e-2
    assert res["bf16x3"][0] <= 1e-2
    # plain bf16 (config 3) has its own gate: tests/test_gpu_bf16_gate.py


def test_kitti_shape_split(gpu):
    """BASELINE.json configs[3] shape (1242x375 -> 47x156 grid, 7332 pixels per image: partial 128-row tiles), batch 2."""
    res = _epe(["bf16x6", "bf16x3"], 375, 1242, 4)
    assert res["bf16x6"][0] <= 1e-3 and res["bf16x6"][1] <= 1e-2
    assert res["bf16x3"][0] <= 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# bf16x6 as an fp32-GRADE mode: its error against a float64 oracle next to the fp32 kernel's own error on the same inputs
# (VERDICT round 1, item 4).  fp32 products are exact and accumulated in fp32; bf16x6 keeps the six product terms down to
# 2^-24 of |a||b| and accumulates them in fp32 too, so both sit at a few 1e-7 of the output scale.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,cin,cout,kh,kw", [
    (1, 55, 128, 128, 512, 3, 3),      # fh | mask conv1 (the roofline launch)
    (1, 55, 128, 384, 256, 1, 5),      # z | r conv of the SepConvGRU
    (2, 23, 40, 324, 256, 1, 1),       # convc1
])
def test_bf16x6_error_next_to_fp32_kernel_vs_float64(gpu, B, H, W, cin, cout, kh, kw):
    from ptlflow_amd.packing import pack_conv_weight
    torch.manual_seed(21)
    x = torch.randn(B, cin, H, W)
    wt = torch.randn(cout, cin, kh, kw) / math.sqrt(cin * kh * kw)
    bias = torch.randn(cout)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=(kh // 2, kw // 2))
    scale = float(ref.abs().max())
    M = B * H * W
    errs = {}
    for name, weight in (("fp32", pack_conv_weight(wt, [(0, cin, cin)]).cuda()), ("bf16x6", planes(wt, [(0, cin, cin)], 3))):
        out = torch.empty(M, cout, device=gpu)
        torch.ops.pfk.conv2d([pm(x, "cuda")], B, H, W, kh, kw, weight, bias.cuda(), cout, EPI_LINEAR, False, 1.0, out, None, None, None)
        d = (unpm(out, B, H, W).double().cpu() - ref).abs()
        errs[name] = (float(d.max()) / scale, float(d.pow(2).mean().sqrt()) / scale)
    print(f"conv {cin}->{cout} {kh}x{kw}: max / rms error over scale  fp32 {errs['fp32'][0]:.2e} / {errs['fp32'][1]:.2e}   "
          f"bf16x6 {errs['bf16x6'][0]:.2e} / {errs['bf16x6'][1]:.2e}")
    assert errs["fp32"][0] <= 2e-6 and errs["bf16x6"][0] <= 2e-6                       # both fp32-grade in absolute terms
    assert errs["bf16x6"][1] <= 3.0 * errs["fp32"][1] + 1e-9, "bf16x6 rms error is not in the fp32 kernel's class"


def test_bf16x6_forward_error_next_to_fp32_vs_float64(gpu):
    """End to end: EPE against the FLOAT64 oracle forward of the fp32 kernels and of bf16x6 on the same weights / frames."""
    from ptlflow_amd.raft import RAFT
    base = RAFT(iters=8).load_synthetic(31)
    P = {k: v.clone() for k, v in base.state_dict().items()}
    x = O.smooth_pair(1, 184, 320, 4)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    ref = O.raft_forward(P64, x.double(), iters=8)["flows"][:, 0]
    epe = {}
    for prec in ("fp32", "bf16x6"):
        model = RAFT(iters=8, conv_precision=prec).eval()
        model.load_state_dict(P)
        out = model.cuda()({"images": x.cuda()})["flows"][:, 0].double().cpu()
        epe[prec] = O.epe(out, ref)
    print(f"EPE vs float64 oracle: fp32 kernels mean {epe['fp32'][0]:.3e} max {epe['fp32'][1]:.3e}; "
          f"bf16x6 mean {epe['bf16x6'][0]:.3e} max {epe['bf16x6'][1]:.3e}")
    assert epe["fp32"][0] <= 1e-3 and epe["bf16x6"][0] <= 1e-3
    assert epe["bf16x6"][0] <= 2.0 * epe["fp32"][0] + 1e-7
