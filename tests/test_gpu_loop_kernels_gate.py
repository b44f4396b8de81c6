"""The small direct kernels that every RAFT, GMA and SEA-RAFT forward runs once per refinement iteration (and that are the forward of the
training nodes), held to the fp64 op gate of tests/op_gate.py: pfk_misc.hip's conv_cin2 (generic, tiled and MFMA kernels, fp32 and
bf16 rows out), flow_delta (4 and 8 pixels per wave, fp32 and bf16 rows in), flow_from_coords, upflow8, the three layout changes and
softmax_rows, and the five forward x8 convex-upsampling kernels of pfk_upsample.hip.  tests/test_gpu_kernels.py compares them with
torch's fp32 result within 2e-5 + 2e-5 |ref|; this file compares with float64 ON THE KERNEL'S OWN INPUTS (tests/op_refs.py).

Every launch: input rows are slices of wider rows with NaN in the lead and pad columns and behind the last row, dense inputs sit
between NaN guards (`guarded`); outputs are sentinel-filled and every column, row and tail the launch must not write is checked
afterwards; the launch is repeated on fresh buffers and must give the same bits; gates 1 and 2 (relative L2 <= OP_TOL, per-element
|err| <= k 2^-24 mag [+ FLOOR]) on what it wrote.  A `keep` mask excludes only the elements that NaN isolation says must be NaN, and
those are asserted to be NaN.  Inputs come from seeded CPU generators.

Bounds (none of them measured):
 conv_cin2      mag = |bias| + sum |x| |w| over n = 2 k k products, k = n + 2; relu is 1-Lipschitz and where mag is 0 the output is an
                exact zero.  bf16 rows: the rounding of the fp32 launch bit for bit, and the bound with the bf16 rounding on top.
 flow_delta     mag = |bias| + sum |x| |w| over 9 cin products, k = 9 cin + 2 (any summation order: lanes, butterfly).  The coordinate
                update is exact: coords1 += delta and flow = coords1 - coords0 are single fp32 operations, compared bit for bit.
 upsampling     w_k = softmax over nine logits, out = sum_k w_k v_k with v = 8 flow (exact) or info.  A weight is off by at most
                k_w = 2 spread + 19 units of 2^-24 relative (op_refs.convex_case: the two rounded differences m_k - max, expf within 2
                ulp in the numerator and in the denominator, nine additions, the reciprocal, the product); the combination adds the
                rounding of the product w_k v_k and of nine additions, one to spare: |err| <= (k_w + 11) 2^-24 sum_k w_k |v_k| + FLOOR.
                FLOOR because a weight can underflow in fp32 (expf(-104) is 0) and its whole term is then lost: without it the fp32
                restatement misses the bound by orders of magnitude at scale 60 (tests/test_op_gate_cpu.py shows it).
 upflow8        the kernel's fp32 index arithmetic restated (scale = (in - 1) / (out - 1), src = scale dst, i0 = trunc, lambda1 = src -
                i0, i1 = i0 + (i0 < in - 1)), then the blend in float64: mag = 8 sum ly lx |v|, k = 8 (the difference c1 - c0, 1 -
                lambda twice, two levels of products and additions: at most 7 roundings on a term's path).
 softmax_rows   k = 2 spread_row + cols + 19 on p itself, + FLOOR.
 layout changes and flow_from_coords are exact.
tests/test_op_gate_cpu.py holds each reference against an independent restatement, shows that torch's fp32 arithmetic and an fp32
restatement in the kernel's own operation order pass these bounds (upsampling <= 0.5, upflow8 <= 0.7, softmax <= 0.3 of them), and
that swapped weight planes, a wrap into the neighbouring image, dropped channels >= 256, a row taken from image b - 1, transposed taps,
swapped sub-pixels, a misplaced factor 8, a missing max subtraction, align_corners=False, an unclamped i1 and a normaliser over ld
all fail them.

What the shapes reach (restated and asserted in `test_cases_reach_what_they_claim`):
 conv_cin2  (2, 3, 21) two images shorter than the 7x7 halo, a last 16-pixel tile of 5 pixels whose second 8-pixel half is empty;
            (1, 1, 1); (2, 9, 33); cout 130 = a second trip of the tiled kernel's channel loop with two channels; k = 1, 9 the generic
            kernel.  MFMA kernel (debug_set_cin2_valu(2)): those, (1, 5, 33) = 2 x 2 tiles with a one-row and a one-column tail, and
            (2, 5, 4163) = 524 tiles on a grid capped at 512 blocks: twelve blocks walk to a second tile.
 flow_delta cin 4 (one lane holds channels), 36, 128 (half the lanes), 260 and 512 (a second trip of the lane loop; 260 with one lane);
            4 pixels per wave below B H ceil(W / 8) = 4096 and 8 from there: (2, 1024, 9) 2 waves per row, the second with 1 pixel;
            (4, 1024, 5) one wave of 5 pixels.  bf16 rows start 8 bytes, not 16, into their buffer.
 upsampling (1, 1, 1), (2, 1, 5), (1, 6, 1), (2, 5, 7) = 70 pixels: 17.5 waves of four pixels; logits of scale 1, 40 and 60.

Measured on an MI355X, the worst over the cases of each kernel (relative L2 | error as a fraction of the per-element bound).  Records,
not thresholds: the thresholds are OP_TOL and a ratio of 1.
  conv_cin2 generic                          2.0e-7 | 0.395
  conv_cin2 tiled                            1.7e-7 | 0.193        bf16 rows  2.5e-3 | 0.995
  conv_cin2 mfma                             1.6e-7 | 0.057        bf16 rows  1.7e-3 | 0.993
  flow_delta                                 1.7e-7 | 0.034        bf16 rows in  1.7e-7 | 0.032
  convex_upsample, _pm (4 and 1 pixels per wave), _info_pm       8.6e-8 | 0.359   (one arithmetic core: the same bits, the same record)
  convex_upsample_pm_b16                     8.8e-8 | 0.119
  convex_upsample_info_pm_b16                8.8e-8 | 0.133
  upflow8                                    5.1e-8 | 0.364
  softmax_rows, contiguous and ld > cols     8.1e-8 | 0.234
Nothing failed: no kernel was changed.  A bf16 ratio near 1 is the half-ulp rounding itself.  The small ratios of flow_delta and of the
MFMA cin2 kernel are those of a worst-case bound on a long sum (36 to 4608 and 98 products of random sign, whose rounding errors
mostly cancel; the generic kernel's 0.395 is its k = 1 case, two products); the bound is the one any correct summation order meets, and
the CPU mutations show that it still separates a dropped channel block, a swapped weight plane and a row from the wrong image from a
correct result.  The upsampling kernels sit at 0.36 where the fp32 restatement on the CPU sits below 0.5.
The module's 133 cases take 5.4 s on an MI355X run alone (pytest's wall time); the slowest are the 524-tile cin2 grid at cout 128
(1.2 s: 5.3 M outputs gated in float64 on the CPU, four launches) and the 8-pixel flow_delta grids at cin 260 (0.45 s and 0.22 s).
"""
import contextlib
import ctypes
import math
from collections import defaultdict

import pytest
import torch

import op_refs as R
import pfk_ctypes
from op_gate import FLOOR, SENTINEL, Rows, flat_out, gates, gates_b16, guarded, nchw, pm, record, same_bits, tail_kept

pytestmark = pytest.mark.gpu
F32, B16 = torch.float32, torch.bfloat16
NAN, GPU = float("nan"), "cuda"
WORST = defaultdict(list)          # kernel -> [(relative L2, ratio to the bound)] over the module: `note` prints the running worst


def note(kernel, result):
    WORST[kernel].append(result)
    record(kernel, WORST[kernel])


def zeroed(nan, *ts):
    return [torch.where(nan, torch.zeros((), dtype=t.dtype), t) for t in ts]


def nan_exactly(what, got, nan):
    assert torch.equal(torch.isnan(got), nan), f"{what}: {int((torch.isnan(got) != nan).sum())} elements are NaN where they must not be, or not NaN where they must"


def untouched(flat):
    return bool((flat == SENTINEL).all())


def test_cases_reach_what_they_claim():
    tiled = lambda B, H, W: (B * H * math.ceil(W / 16), W - (math.ceil(W / 16) - 1) * 16)          # noqa: E731  (blocks, pixels of the last)
    assert tiled(2, 3, 21) == (12, 5) and 3 < 7 and tiled(2, 9, 33) == (54, 1) and 130 - 128 == 2
    mfma = lambda B, H, W: (B * math.ceil(H / 4) * math.ceil(W / 32), H % 4, W % 32)                # noqa: E731
    assert mfma(1, 5, 33) == (4, 1, 1) and mfma(2, 5, 4163)[0] == 524 > 512 and 2 * 5 * 4163 == 41630
    assert all(mfma(*g)[0] < 256 for g in R.CIN2_MFMA_GRIDS[:-1]), "below 256 tiles only the knob reaches the MFMA kernel"
    assert not any(pixels_per_wave(*g) == 8 for g in R.FLOW_DELTA_GRIDS4) and all(pixels_per_wave(*g) == 8 for g in R.FLOW_DELTA_GRIDS8)
    assert 2 * 1024 * math.ceil(9 / 8) == 4096 and 4 * 1024 * math.ceil(5 / 8) == 4096
    assert [c > 256 for c in (4, 36, 128, 260, 512)] == [False, False, False, True, True] and 260 - 256 == 4
    assert 2 * 5 * 7 % 16 != 0 and 577 % 4 != 0 and 584 % 4 == 0 and 592 % 8 == 0


# ---------------------------------------------------------------------------------------------------------------------
# 1. conv_cin2
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def cin2_knob(v):
    torch.ops.pfk.debug_set_cin2_valu(v)
    try:
        yield
    finally:
        torch.ops.pfk.debug_set_cin2_valu(0)


def cin2_buffers(c, dtype):
    """the flow as a 2-column slice at lead 1 of 5-wide NaN rows, the weight and bias between NaN guards, and a maker of outputs: a
    channel slice at lead 1 of wider sentinel rows"""
    B, H, W = c["grid"]
    inp = Rows(B * H * W, 2, GPU, c["rows"], pad=2, lead=1, nan_tail=True)
    assert inp.ld == 5 and inp.rows.stride() == (5, 1)
    bias = None if c["bias"] is None else guarded(c["bias"], GPU)
    return inp, guarded(c["packed"], GPU), bias, lambda: Rows(B * H * W, c["cout"], GPU, pad=3, dtype=dtype, lead=1)


def cin2_launch(what, c, dtype, knob):
    """the launch twice on fresh outputs: guards, the same bits; returns the [M, cout] rows on the CPU"""
    inp, w, bias, make = cin2_buffers(c, dtype)
    outs = []
    for _ in range(2):
        o = make()
        with cin2_knob(knob):
            torch.ops.pfk.conv_cin2(inp.rows, w, bias, o.rows, *c["grid"], c["k"], c["relu"])
        torch.cuda.synchronize()
        o.check_untouched(what)
        outs.append(o)
    assert same_bits(outs[0].flat, outs[1].flat), f"{what}: a second run gives other bits"
    return outs[0].rows.cpu()


def cin2_gate(what, got, c, twin=None):
    nan = c["nan"]
    nan_exactly(what, got.float(), nan)
    g, ref, mag = zeroed(nan, got, c["ref"], c["mag"])
    if got.dtype == B16:
        return gates_b16(what, g, zeroed(nan, twin)[0], ref, mag, c["K"])
    return gates(what, g, ref, mag, c["K"], keep=~nan)


def cin2_both(what, c, knob):
    """fp32 and bf16 rows out of one case on one kernel: [(result, rows)]"""
    f = cin2_launch(what, c, F32, knob)
    h = cin2_launch(what + " bf16", c, B16, knob)
    return f, h, [cin2_gate(what, f, c), cin2_gate(what + " bf16", h, c, f)]


@pytest.mark.parametrize("cout", [1, 64, 130])
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("grid", R.CIN2_GRIDS, ids=str)
def test_cin2_tiled(gpu, grid, k, cout):
    relu = (k, cout) not in ((3, 64), (5, 130), (7, 1))
    c = R.cin2_case(*grid, k, cout, relu, (grid, k, cout) != ((2, 9, 33), 5, 64))
    _, _, res = cin2_both(f"cin2 tiled {grid} k{k} cout{cout}", c, 1)
    note("conv_cin2 tiled", res[0])
    note("conv_cin2 tiled bf16", res[1])


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("grid", R.CIN2_GRIDS, ids=str)
def test_cin2_generic(gpu, grid, k):
    c = R.cin2_case(*grid, k, 5, k == 9)
    what = f"cin2 generic {grid} k{k}"
    note("conv_cin2 generic", cin2_gate(what, cin2_launch(what, c, F32, 0), c))
    # it has no bf16 form: the call raises and writes nothing
    inp, w, bias, make = cin2_buffers(c, B16)
    o = make()
    with pytest.raises(RuntimeError, match="unsupported"):
        torch.ops.pfk.conv_cin2(inp.rows, w, bias, o.rows, *grid, k, True)
    torch.cuda.synchronize()
    assert untouched(o.flat), f"{what}: a refused call wrote its output"


@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("grid", R.CIN2_MFMA_GRIDS, ids=str)
def test_cin2_mfma(gpu, grid, cout):
    c = R.cin2_case(*grid, 7, cout, cout == 64 or grid != (1, 5, 33))
    what = f"cin2 mfma {grid} cout{cout}"
    f, h, res = cin2_both(what, c, 2)
    note("conv_cin2 mfma", res[0])
    note("conv_cin2 mfma bf16", res[1])
    assert same_bits(f, cin2_launch(what + " (tiled)", c, F32, 1)), f"{what}: other bits than the tiled kernel"
    assert same_bits(h, cin2_launch(what + " (tiled) bf16", c, B16, 1)), f"{what}: other bf16 bits than the tiled kernel"


@pytest.mark.parametrize("kernel,k,cout,knob", [("tiled", 7, 64, 1), ("tiled", 3, 130, 1), ("generic", 9, 5, 0), ("mfma", 7, 64, 2), ("mfma", 7, 128, 2)])
def test_cin2_nan_reaches_its_window_only(gpu, kernel, k, cout, knob):
    """one NaN flow pixel of image 1, next to the 16- and 32-pixel tile edge at x = 32: exactly the outputs whose k x k window covers
    it are NaN; everything else, image 0 included, passes the gates"""
    c = R.cin2_case(2, 9, 33, k, cout, True, True, (2, 31))
    assert bool(c["nan"].any()) and not bool(c["nan"][:9 * 33].any())
    what = f"cin2 {kernel} NaN k{k} cout{cout}"
    f = cin2_launch(what, c, F32, knob)
    note(f"conv_cin2 {kernel}", cin2_gate(what, f, c))
    if kernel != "generic":
        note(f"conv_cin2 {kernel} bf16", cin2_gate(what + " bf16", cin2_launch(what + " bf16", c, B16, knob), c, f))


# ---------------------------------------------------------------------------------------------------------------------
# 2. flow_delta, flow_from_coords
# ---------------------------------------------------------------------------------------------------------------------
def pixels_per_wave(B, H, W):
    """flow_delta_launch's rule: 8 pixels per wave once that still gives B H ceil(W / 8) >= 4096 waves, 4 below"""
    return 8 if B * H * math.ceil(W / 8) >= 4096 else 4


def fd_launch(what, c, x=None, delta=True, flow=True, flow16=None, in_pad=4):
    """the launch twice on fresh buffers: input rows at lead 4 (16 bytes into the buffer in fp32, 8 in bf16) of rows with ld = cin + 4
    + `in_pad`, weight / bias / coords0 between NaN guards, coords1 (updated in place) and delta_out at the head of sentinel-tailed
    buffers, the two flow outputs as 2-column slices at lead 1 of 5-wide sentinel rows.  Returns the outputs on the CPU."""
    B, H, W = c["grid"]
    M = B * H * W
    x = c["x"] if x is None else x
    b16 = x.dtype == B16
    flow16 = b16 if flow16 is None else flow16
    inp = Rows(M, x.shape[1], GPU, x, pad=in_pad, dtype=x.dtype, lead=4, nan_tail=True)
    assert inp.rows.data_ptr() % 16 == (8 if b16 else 0) and inp.ld > x.shape[1]
    w, bias, c0 = guarded(c["packed"][:, :, :x.shape[1]].contiguous(), GPU), guarded(c["bias"], GPU), guarded(c["c0"], GPU)
    runs = []
    for _ in range(2):
        c1flat, c1 = flat_out((B, 2, H, W), GPU)
        c1.copy_(c["c1"])
        dflat, d = flat_out((B, 2, H, W), GPU)
        fo, f16 = Rows(M, 2, GPU, pad=2, lead=1), Rows(M, 2, GPU, pad=2, lead=1, dtype=B16)
        before = c1flat.clone()
        try:
            torch.ops.pfk.flow_delta(inp.rows, w, bias, c0, c1, d if delta else None, fo.rows if flow else None, f16.rows if flow16 else None)
        except RuntimeError:
            torch.cuda.synchronize()
            assert same_bits(c1flat, before) and untouched(dflat) and untouched(fo.flat) and untouched(f16.flat), f"{what}: a refused call wrote"
            raise
        torch.cuda.synchronize()
        assert tail_kept(c1flat) and tail_kept(dflat), f"{what}: memory behind coords1 / delta_out was written"
        fo.check_untouched(what + " flow_out")
        f16.check_untouched(what + " flow_out_b16")
        assert delta or untouched(dflat), f"{what}: delta_out = None, yet written"
        assert flow or untouched(fo.flat), f"{what}: flow_out = None, yet written"
        assert flow16 or untouched(f16.flat), f"{what}: flow_out_b16 = None, yet written"
        runs.append({"c1": c1flat, "delta": dflat, "flow": fo.flat, "flow16": f16.flat})
    for key in runs[0]:
        assert same_bits(runs[0][key], runs[1][key]), f"{what}: a second run gives other bits in {key}"
    return {"c1": c1.cpu(), "delta": d.cpu(), "flow": nchw(fo.rows.cpu(), B, H, W), "flow16": nchw(f16.rows.cpu(), B, H, W)}


def fd_check(what, c, out):
    """gates on delta_out; the coordinate update bit for bit in fp32 on the CPU (NaN where delta is NaN)"""
    nan = c["nan"]
    d = out["delta"]
    nan_exactly(what, d, nan)
    res = gates(what, *zeroed(nan, d, c["ref"], c["mag"]), c["K"], keep=~nan)
    c1 = c["c1"] + d
    flow = c1 - c["c0"]
    for name, got, want in (("coords1", out["c1"], c1), ("flow_out", out["flow"], flow)):
        nan_exactly(f"{what} {name}", got, nan)
        assert torch.equal(*zeroed(nan, got, want)), f"{what}: {name} is not the single fp32 operation on delta_out"
    if c["x"].dtype == B16:
        nan_exactly(f"{what} flow_out_b16", out["flow16"].float(), nan)
        assert torch.equal(*zeroed(nan, out["flow16"], flow.to(B16))), f"{what}: flow_out_b16 is not flow_out rounded"
    return res


def fd_case_both(what, grid, cin, nan_corners=False):
    """the fp32 case, the bf16 case, and the fp32 launch on the widened bf16 rows: the same delta bits"""
    c = R.flow_delta_case(*grid, cin, F32, nan_corners)
    note("flow_delta", fd_check(what, c, fd_launch(what, c)))
    h = R.flow_delta_case(*grid, cin, B16, nan_corners)
    out = fd_launch(what + " bf16", h)
    note("flow_delta bf16 rows", fd_check(what + " bf16", h, out))
    wide = fd_launch(what + " widened", h, x=h["x"].float())
    assert same_bits(wide["delta"], out["delta"]), f"{what}: bf16 rows and the same values as fp32 rows give other delta bits"


@pytest.mark.parametrize("cin", [4, 36, 128, 260, 512])
@pytest.mark.parametrize("grid", R.FLOW_DELTA_GRIDS4, ids=str)
def test_flow_delta_4_pixels(gpu, grid, cin):
    assert pixels_per_wave(*grid) == 4
    fd_case_both(f"flow_delta {grid} cin{cin}", grid, cin)


@pytest.mark.parametrize("cin", [8, 260])
@pytest.mark.parametrize("grid", R.FLOW_DELTA_GRIDS8, ids=str)
def test_flow_delta_8_pixels(gpu, grid, cin):
    assert pixels_per_wave(*grid) == 8
    fd_case_both(f"flow_delta {grid} cin{cin}", grid, cin)


@pytest.mark.parametrize("dtype", [F32, B16], ids=["f32", "b16"])
def test_flow_delta_optional_outputs(gpu, dtype):
    c = R.flow_delta_case(1, 3, 9, 36, dtype)
    what = f"flow_delta optional {dtype}"
    full = fd_launch(what, c)
    fd_check(what, c, full)
    for off in ("delta", "flow") + (("flow16",) if dtype == B16 else ()):
        out = fd_launch(f"{what} without {off}", c, **{off: False})
        for key in full:
            if key != off and (key != "flow16" or dtype == B16):
                assert same_bits(out[key], full[key]), f"{what}: without {off}, {key} has other bits"
    if dtype == F32:
        with pytest.raises(RuntimeError, match="bfloat16 input"):
            fd_launch(what + " b16 twin of fp32 rows", c, flow16=True)


@pytest.mark.parametrize("grid,cin", [((2, 2, 5), 36), ((2, 1, 3), 260), ((2, 1024, 9), 8)], ids=str)
def test_flow_delta_nan_reaches_its_neighbours_only(gpu, grid, cin):
    """NaN input rows at the four corner pixels of image 1: only their 3x3 neighbours' deltas are NaN — the clamped addresses of the
    zero padding hold NaN there and stay out, and the row above image 1 is padding, not image 0's last row (image 0 is clean)"""
    c = R.flow_delta_case(*grid, cin, F32, True)
    assert bool(c["nan"][1].any()) and not bool(c["nan"][0].any())
    fd_case_both(f"flow_delta NaN {grid} cin{cin}", grid, cin, True)


def test_flow_delta_refusals(gpu):
    c = R.flow_delta_case(1, 3, 9, 36, F32)
    with pytest.raises(RuntimeError, match="alignment"):          # cin % 4 != 0
        fd_launch("flow_delta cin 34", c, x=c["x"][:, :34].contiguous(), in_pad=2)
    with pytest.raises(RuntimeError, match="alignment"):          # ld % 4 != 0
        fd_launch("flow_delta ld 43", c, in_pad=3)
    h = R.flow_delta_case(1, 3, 9, 36, B16)
    with pytest.raises(RuntimeError, match="alignment"):
        fd_launch("flow_delta bf16 ld 42", h, in_pad=2)


@pytest.mark.parametrize("grid", R.FLOW_DELTA_GRIDS4 + R.FLOW_DELTA_GRIDS8, ids=str)
def test_flow_from_coords(gpu, grid):
    B, H, W = grid
    c = R.flow_delta_case(*grid, 8 if pixels_per_wave(*grid) == 8 else 4)
    c0, c1 = guarded(c["c0"], GPU), guarded(c["c1"], GPU)
    outs = []
    for _ in range(2):
        o = Rows(B * H * W, 2, GPU, pad=2, lead=1)
        torch.ops.pfk.flow_from_coords(c0, c1, o.rows)
        torch.cuda.synchronize()
        o.check_untouched("flow_from_coords")
        outs.append(o)
    assert same_bits(outs[0].flat, outs[1].flat)
    assert torch.equal(nchw(outs[0].rows.cpu(), B, H, W), c["c1"] - c["c0"])
    o = Rows(B * H * W, 1, GPU, pad=2, lead=1)
    with pytest.raises(RuntimeError):
        torch.ops.pfk.flow_from_coords(c0, c1, o.rows)
    torch.cuda.synchronize()
    assert untouched(o.flat)


# ---------------------------------------------------------------------------------------------------------------------
# 3. forward x8 convex upsampling
# ---------------------------------------------------------------------------------------------------------------------
def up_launch(what, kind, grid, flow, mask, info=None, n_info=0, mask_lead=None, mask_pad=None):
    """One of the five kernels twice on fresh outputs.  kind: "nchw" (convex_upsample), "pm" (convex_upsample_pm, four pixels per wave;
    a bf16 mask: its bf16 kernel), "pm1" (mask_ld = 577: one pixel per wave), "info" (convex_upsample_info_pm / _b16, `n_info` channels).
    The mask rows are a slice of wider NaN rows, the pixel-major flow / info 2- / n-column slices at lead 1, the NCHW flow between
    guards; the outputs lead sentinel-tailed buffers.  Returns [B, 2 + n_info, 8H, 8W] on the CPU."""
    B, H, W = grid
    M = B * H * W
    b16 = mask.dtype == B16
    lead, pad = (0, 1) if kind == "pm1" else (8, 8) if b16 else (4, 4)
    lead, pad = lead if mask_lead is None else mask_lead, pad if mask_pad is None else mask_pad
    m = Rows(M, 576, GPU, pm(mask), pad=pad, dtype=mask.dtype, lead=lead, nan_tail=True)
    f = guarded(flow, GPU) if kind == "nchw" else Rows(M, 2, GPU, pm(flow), pad=2, lead=1, nan_tail=True).rows
    i = Rows(M, n_info, GPU, pm(info[:, :n_info]), pad=3, lead=1, nan_tail=True).rows if kind == "info" else None
    runs = []
    for _ in range(2):
        oflat, out = flat_out((B, 2, 8 * H, 8 * W), GPU)
        iflat, iout = flat_out((B, n_info, 8 * H, 8 * W), GPU)
        try:
            if kind == "nchw":
                torch.ops.pfk.convex_upsample(f, m.rows, out)
            elif kind == "info":
                (torch.ops.pfk.convex_upsample_info_pm_b16 if b16 else torch.ops.pfk.convex_upsample_info_pm)(f, i, m.rows, out, iout)
            else:
                torch.ops.pfk.convex_upsample_pm(f, m.rows, out)
        except RuntimeError:
            torch.cuda.synchronize()
            assert untouched(oflat) and untouched(iflat), f"{what}: a refused call wrote"
            raise
        torch.cuda.synchronize()
        assert tail_kept(oflat) and tail_kept(iflat), f"{what}: memory behind an output was written"
        assert kind == "info" or untouched(iflat)
        runs.append((oflat, iflat))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), f"{what}: a second run gives other bits"
    return torch.cat([out, iout], 1).cpu()


def up_gate(what, got, ref, mag, k, keep=None):
    C = got.shape[1]
    return gates(what, got, ref[:, :C], mag[:, :C], k[:, :C], floor=FLOOR, keep=keep)


def up_all(what, grid, flow, mask, info, ref, mag, k, check):
    """every kernel that takes `mask`'s type on one set of inputs; `check(what, kernel name, got)` judges each; the header's bit
    equalities: NCHW flow = pixel-major flow, four pixels per wave = one, the info kernels' flow = the plain kernel's"""
    b16 = mask.dtype == B16
    plain = up_launch(what + " pm", "pm", grid, flow, mask)
    check(what + " pm", "convex_upsample_pm_b16" if b16 else "convex_upsample_pm", plain)
    if b16:
        wide = up_launch(what + " widened", "pm", grid, flow, mask.float())
        assert same_bits(wide, plain), f"{what}: bf16 logits and the same values as fp32 logits give other bits"
    else:
        got = up_launch(what + " nchw", "nchw", grid, flow, mask)
        check(what + " nchw", "convex_upsample", got)
        assert same_bits(got, plain), f"{what}: NCHW flow and pixel-major flow give other bits"
        got = up_launch(what + " pm1", "pm1", grid, flow, mask)
        check(what + " pm1", "convex_upsample_pm (one pixel per wave)", got)
        assert same_bits(got, plain), f"{what}: one pixel per wave and four give other bits"
    for n in (1, 4, 8):
        got = up_launch(f"{what} info{n}", "info", grid, flow, mask, info, n)
        check(f"{what} info{n}", "convex_upsample_info_pm_b16" if b16 else "convex_upsample_info_pm", got)
        assert same_bits(got[:, :2].contiguous(), plain), f"{what}: the info kernel's flow has other bits than the plain kernel's"


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
@pytest.mark.parametrize("scale", R.UP_SCALES)
@pytest.mark.parametrize("grid", R.UP_GRIDS, ids=str)
def test_convex_forward(gpu, grid, scale, b16):
    c = R.convex_fwd_case(*grid, scale, b16)
    up_all(f"up {grid} x{scale:g}", grid, c["flow"], c["mask"], c["info"], c["ref"], c["mag"], c["k"],
           lambda what, kernel, got: note(kernel, up_gate(what, got, c["ref"], c["mag"], c["k"])))


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
@pytest.mark.parametrize("grid", [(2, 1, 5), (2, 5, 7)], ids=str)
def test_convex_forward_zero_flow_gives_exact_zeros(gpu, grid, b16):
    c = R.convex_fwd_case(*grid, 1.0, b16, 0)
    assert bool((c["mag"][0, :2] == 0).all()) and bool((c["mag"][1] > 0).all())

    def check(what, kernel, got):
        assert bool((got[0, :2] == 0).all()), f"{what}: image 0 has no flow, its upsampled flow must be exact zeros"
        note(kernel, up_gate(what, got, c["ref"], c["mag"], c["k"]))

    up_all(f"up zero image {grid}", grid, c["flow"], c["mask"], c["info"], c["ref"], c["mag"], c["k"], check)


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
@pytest.mark.parametrize("keep", [0, 4, 8])
def test_convex_forward_infinite_logits(gpu, keep, b16):
    """-inf in eight of the nine taps: the ninth has weight one, the output is exactly 8 x that neighbour's flow (its info), zero
    outside the image, and finite"""
    grid = (2, 5, 7)
    c = R.convex_fwd_case(*grid, 1.0, b16)
    m = torch.full((2, 9, 64, 5, 7), float("-inf"), dtype=c["mask"].dtype)
    m[:, keep] = c["mask"].view(2, 9, 64, 5, 7)[:, keep]
    m = m.view(2, 576, 5, 7)
    ref, mag, k = R.convex_fwd64(c["flow"], m.float(), c["info"])
    assert bool((k == 30).all()) and bool((ref == 0).any()) == (keep != 4)

    def check(what, kernel, got):
        assert bool(torch.isfinite(got).all()) and torch.equal(got, ref[:, :got.shape[1]].float()), f"{what}: not exactly the neighbour"
        note(kernel, up_gate(what, got, ref, mag, k))

    up_all(f"up -inf but tap {keep}", grid, c["flow"], m, c["info"], ref, mag, k, check)


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
def test_convex_forward_keeps_images_apart(gpu, b16):
    """NaN flow, info and logits in image 1: image 0 keeps the bits of the clean run, image 1 is NaN everywhere"""
    grid = (2, 5, 7)
    c = R.convex_fwd_case(*grid, 1.0, b16)
    flow, mask, info = c["flow"].clone(), c["mask"].clone(), c["info"].clone()
    flow[1], mask[1], info[1] = NAN, NAN, NAN
    clean = {}
    launch = lambda what: what.split()[-1]          # noqa: E731   `up_all` names a launch "<what> pm", "<what> nchw", "<what> info4", ...
    up_all("up clean", grid, c["flow"], c["mask"], c["info"], c["ref"], c["mag"], c["k"], lambda what, kernel, got: clean.setdefault(launch(what), got))
    keep = torch.zeros(2, 10, 40, 56, dtype=torch.bool)
    keep[0] = True

    def check(what, kernel, got):
        assert bool(torch.isnan(got[1]).all()), f"{what}: image 1 is not NaN everywhere"
        assert same_bits(got[0].contiguous(), clean[launch(what)][0].contiguous()), f"{what}: image 1's NaN changed image 0"
        z = torch.where(torch.isnan(got), torch.zeros(()), got)
        note(kernel, up_gate(what, z, *zeroed(~keep, c["ref"], c["mag"], c["k"]), keep=keep[:, :got.shape[1]]))

    up_all("up NaN image 1", grid, flow, mask, info, c["ref"], c["mag"], c["k"], check)


def test_convex_forward_refusals(gpu):
    grid = (2, 5, 7)
    c = R.convex_fwd_case(*grid, 1.0, False)
    h = R.convex_fwd_case(*grid, 1.0, True)
    with pytest.raises(RuntimeError, match="alignment"):           # bf16 mask rows 4 bytes into their buffer
        up_launch("up bf16 mask at +4 bytes", "pm", grid, h["flow"], h["mask"], mask_lead=2, mask_pad=2)
    with pytest.raises(RuntimeError, match="alignment"):           # the info kernels have no one-pixel-per-wave form
        up_launch("up info ld 577", "info", grid, c["flow"], c["mask"], c["info"], 4, mask_lead=0, mask_pad=1)
    with pytest.raises(RuntimeError, match="alignment"):
        up_launch("up info bf16 ld 580", "info", grid, h["flow"], h["mask"], h["info"], 4, mask_lead=0, mask_pad=4)


# ---------------------------------------------------------------------------------------------------------------------
# 4. upflow8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", R.UPFLOW_GRIDS, ids=str)
def test_upflow8(gpu, grid):
    B, H, W = grid
    c = R.upflow8_case(*grid)
    c0, c1 = guarded(c["c0"], GPU), guarded(c["c1"], GPU)
    flats = []
    for _ in range(2):
        flat, out = flat_out((B, 2, 8 * H, 8 * W), GPU)
        torch.ops.pfk.upflow8(c0, c1, out)
        torch.cuda.synchronize()
        assert tail_kept(flat), f"upflow8 {grid}: memory behind the output was written"
        flats.append(flat)
    assert same_bits(flats[0], flats[1]), f"upflow8 {grid}: a second run gives other bits"
    note("upflow8", gates(f"upflow8 {grid}", out.cpu(), c["ref"], c["mag"], c["K"]))
    flat, out = flat_out((B, 2, 8 * H, 8 * W + 8), GPU)
    with pytest.raises(RuntimeError):
        torch.ops.pfk.upflow8(c0, c1, out)
    torch.cuda.synchronize()
    assert untouched(flat)


# ---------------------------------------------------------------------------------------------------------------------
# 5. layout changes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.LAYOUT_SHAPES, ids=str)
def test_layout_changes_are_exact_copies(gpu, shape):
    B, C, H, W = shape
    M, N = B * H * W, H * W
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(C * 100 + W))
    rows = pm(x)
    # nchw_to_pm into a channel slice at lead 1
    dense = guarded(x, GPU)
    outs = []
    for _ in range(2):
        o = Rows(M, C, GPU, pad=3, lead=1)
        torch.ops.pfk.nchw_to_pm(dense, o.rows)
        torch.cuda.synchronize()
        o.check_untouched("nchw_to_pm")
        outs.append(o)
    assert same_bits(outs[0].flat, outs[1].flat) and torch.equal(outs[0].rows.cpu(), rows)
    # pm_to_nchw from such a slice
    inp = Rows(M, C, GPU, rows, pad=3, lead=1, nan_tail=True)
    flats = []
    for _ in range(2):
        flat, out = flat_out(shape, GPU)
        torch.ops.pfk.pm_to_nchw(inp.rows, out)
        torch.cuda.synchronize()
        assert tail_kept(flat), "pm_to_nchw: memory behind the output was written"
        flats.append(flat)
    assert same_bits(flats[0], flats[1]) and torch.equal(out.cpu(), x)
    # pm_to_cm into [B, C, Npad], Npad > N: include/pfk.h — the pad columns [N, out_ld) are not written
    for npad in (N + 5, N + 1):
        flats = []
        for _ in range(2):
            flat, out = flat_out((B, C, npad), GPU)
            torch.ops.pfk.pm_to_cm(inp.rows, out)
            torch.cuda.synchronize()
            assert tail_kept(flat), "pm_to_cm: memory behind the output was written"
            assert bool((out[:, :, N:] == SENTINEL).all()), "pm_to_cm: pad columns were written"
            flats.append(flat)
        assert same_bits(flats[0], flats[1]) and torch.equal(out[:, :, :N].cpu(), x.reshape(B, C, N))
    # refusals: an output of C + 1 channels
    for bad in (lambda o: torch.ops.pfk.nchw_to_pm(dense, o[:M * (C + 1)].view(M, C + 1)),
                lambda o: torch.ops.pfk.pm_to_nchw(inp.rows, o[:M * (C + 1)].view(B, C + 1, H, W)),
                lambda o: torch.ops.pfk.pm_to_cm(inp.rows, o[:B * (C + 1) * (N + 1)].view(B, C + 1, N + 1))):
        o = torch.full((B * (C + 1) * (N + 1) + 8,), SENTINEL, device=GPU)
        with pytest.raises(RuntimeError):
            bad(o)
        torch.cuda.synchronize()
        assert untouched(o)


# ---------------------------------------------------------------------------------------------------------------------
# 6. softmax_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax_rows(gpu, cols, scale):
    c = R.softmax_rows_case(cols, scale)
    rows = R.SOFTMAX_ROWS
    what = f"softmax_rows {cols} x{scale:g}"
    # in place on contiguous rows, through the binding
    flats = []
    for _ in range(2):
        flat, x = flat_out((rows, cols), GPU)
        x.copy_(c["x"])
        torch.ops.pfk.softmax_rows(x)
        torch.cuda.synchronize()
        assert tail_kept(flat), f"{what}: memory behind the rows was written"
        flats.append(flat)
    assert same_bits(flats[0], flats[1]), f"{what}: a second run gives other bits"
    dense = x.cpu()
    note("softmax_rows", gates(what, dense, c["ref"], c["mag"], c["k"], floor=FLOOR))
    if cols >= 3:
        assert int((dense[3] == 0).sum()) == cols - 2, f"{what}: a -inf logit has a weight"
    # ld > cols through the C ABI: the pad columns hold NaN before the launch and after it
    lib = pfk_ctypes.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda r, ld: lib.pfk_softmax_rows_f32(ctypes.c_void_p(r.rows.data_ptr()), ctypes.c_longlong(rows), ctypes.c_int(cols),          # noqa: E731
                                                  ctypes.c_longlong(ld), stream)
    wides = []
    for _ in range(2):
        r = Rows(rows, cols, GPU, c["x"], pad=3, lead=0)
        assert call(r, r.ld) == pfk_ctypes.PFK_OK
        torch.cuda.synchronize()
        assert bool(torch.isnan(r.full[:, cols:]).all()), f"{what}: pad columns were written"
        assert bool((r.flat[rows * r.ld:] == SENTINEL).all()), f"{what}: memory behind the last row was written"
        wides.append(r)
    assert same_bits(wides[0].flat, wides[1].flat), f"{what}: a second run gives other bits (ld > cols)"
    wide = wides[0].rows.cpu()
    note("softmax_rows ld > cols", gates(what + " ld > cols", wide, c["ref"], c["mag"], c["k"], floor=FLOOR))
    assert same_bits(wide.contiguous(), dense), f"{what}: the row stride changed the bits"
    # ld < cols is refused and nothing is written
    if cols > 1:
        r = Rows(rows, cols, GPU, c["x"], pad=3, lead=0)
        before = r.flat.clone()
        assert call(r, cols - 1) == pfk_ctypes.PFK_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert same_bits(r.flat, before)
