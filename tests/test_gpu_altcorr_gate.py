"""The on-demand correlation kernels (ptlflow_amd/csrc/pfk_altcorr.hip) held to the fp64 op gate: the per-pixel kernel, the
window-sharing MFMA kernel on 8x4 / 8x8 patches, the overflow kernel, the plan kernel with its launch-wide 5/8 gate, the bf16
variant of each, and the atomics-based backward.  Every forward case runs with each kernel forced (`debug_set_altcorr` 1, 2, 3, 4)
on fp32 and on bf16 maps.

Gates (tests/op_gate.py's `gates`, `OP_TOL`, `SENTINEL`, `rel`, `guarded`):
 1. relative L2 <= 5e-6 against float64 on the CPU ON THE KERNEL'S OWN INPUTS (for bf16 maps: the bf16-rounded values), over the
    cells whose float64 reference is finite.  Forward reference: `oracle.raft_oracle.alt_corr_forward` on `.double()` copies —
    `floor(x)` and `x - floor(x)` of an fp32 value are exact in both precisions, so the tap positions are the kernel's and
    everything after them is float64.  Backward reference: float64 autograd through the same function.
 2. a per-element bound that needs no measurement, K * 2^-24 * mag, where `mag` is the same function on |f1|, |f2| (and
    |corr_grad|): the bilinear weights are >= 0, so that is the exact sum of the magnitudes of an element's terms.
      forward, K = C + 10:   a tap is a C-term dot product: every term passes one rounding of its product and at most C - 1 of the
                             running sum (fused or not, butterfly or MFMA: any order)                              <= C
                             `1 - dx` and `1 - dy`                                                               + 2
                             two multiplications per weighted tap, `s * ey * ex`                                  + 2
                             the four-term sum                                                                   + 3
                             = C + 7 to first order; + 3 for the (1 + 2^-24)^(C + 7) - 1 second-order terms (C <= 512).
      backward, K = n + 12:  n = the number of in-map taps that reach the element, counted by an integer scatter in the test (per
                             fmap1 pixel for `fmap1_grad`, per fmap2 cell for `fmap2_grad`): n roundings of the running sum (the
                             fused multiply-add of `fmap1_grad`, the atomic add of `fmap2_grad` — in any order).  The 12: the folded
                             tap weight `gs` is a four-term sum (+ 3) of `g * w_y * w_x` (+ 2) with `w = 1 - d` rounded once each
                             (+ 2), then the product `gs * f` where it is not fused (+ 1): 8 to first order, 4 to spare for the
                             second-order terms and for the op's addition of the per-set results when N > 1.
    Where `mag == 0` the element must be an exact zero.  Where the float64 reference is NaN the kernel must be NaN and nowhere else;
    those cells are the only ones left out of the numeric comparison.
 3. every input is a contiguous 16-byte-aligned view in the middle of a NaN-filled flat buffer (bf16 NaN for bf16 maps) with 64
    elements of guard on each side: a read outside a map poisons the result.  The C entry points (`ctypes`) write into
    sentinel-filled buffers whose 64-float tail must survive; the workspace of the plan kernel likewise.
 4. a second forward run gives the same bits; so does `fmap1_grad`.  `fmap2_grad` is accumulated with atomics in a free order:
    two runs must agree within the bound of 2.

Non-finite coordinates.  Forward: a NaN or infinite coordinate makes the fraction NaN and the whole window NaN (as in the oracle and
in the reference extension); a finite coordinate beyond the kernel's 1e9 cut has fraction 0 and reaches no tap: exact zeros.
Backward: such a pixel reaches no tap — its `fmap1_grad` row is exactly 0 and it adds nothing to `fmap2_grad`; the reference is
built with those coordinates replaced by (-1e6, -1e6).  The reference extension (correlation_kernel.cu:181-237) does not define this
case: it converts `floor(x)` to int unchecked (undefined for NaN / inf / 1e12 in C++; in practice 0 or a saturated value) and adds
`g * f2` with g = NaN unconditionally (:225), which leaves NaN in that pixel's `fmap1_grad` row and, where the converted tap lands in
the map, in `fmap2_grad`.  Nothing there contradicts the tighter contract pinned here.

`patch_boxes()` restates `patch_box()` / `patch_takes_gemm()` of the kernel file in Python, so that the box-size and 5/8-gate cases
assert the counts they were built for before the kernel runs.

Per test — what is gated (K = C + 10 on every forward output, n + 12 on every gradient) and, measured on an MI355X, the worst over its
cases of relative L2 | error as a fraction of the per-element bound (fp32 maps; bf16 maps).  Records, not thresholds: the thresholds
are `OP_TOL` and a ratio of 1.
  test_forward_channel_radius         C in {4, 20, 68, 132, 512} x r in {1..4} (twelve), 2 x 11 x 13 on 7 x 8, kernels 1-4
                                      4.1e-7 | 0.283; 1.8e-7 | 0.173
  test_forward_integer_coordinates    identity, half-resolution and shifted integer grids, r = 1 and 4, kernels 1-4
                                      8.7e-8 | 0.113; 3.2e-8 | 0.052
  test_forward_nonfinite_coordinates  NaN in x / in y, +-inf, +-9.9e8, 1e9, +-2^31, +-1e12, a block at (-30, 2.5), a block of NaN, kernels 1-4
                                      9.8e-8 | 0.093; 6.0e-8 | 0.061
  test_forward_box_sizes              8x4 and 8x8 patches with boxes of 1, 32, 33, 512, 513 points (asserted), kernels 1-4
                                      7.3e-8 | 0.147; 5.4e-8 | 0.110
  test_forward_tiny_maps              fmap2 1x1, 1x2, 2x1 under 5x13; fmap1 1x1, 3x5, 1x9, kernels 1-4
                                      1.2e-7 | 0.166; 5.8e-8 | 0.177
  test_forward_heuristic_gate         mode 0 at 256 patches: all qualify, 49 (noise), 160, 159 (asserted); 255 patches
                                      7.5e-8 | 0.211; 5.4e-8 | 0.191
  test_forward_coordinate_sets        N = 3 through the op, mode 0 and kernels 1-4                    9.3e-8 | 0.092; 5.7e-8 | 0.052
  test_forward_c_entry                `pfk_altcorr_forward_f32` / `_bf16`, workspace and NULL, output and workspace tails
                                      7.5e-8 | 0.147; 5.0e-8 | 0.130
  test_seam_half_maps                 the fp32 result behind `altcorr.forward` for fp16 / bf16 maps   7.6e-8 | 0.085; its rounding exact
  test_backward_channel_radius        C in {4, 68, 132, 512} x r in {1, 3, 4} (eight), 2 x 9 x 11 on 7 x 8; n1 <= 56, n2 <= 95
                                      fmap1_grad 8.8e-8 | 0.169     fmap2_grad 1.7e-7 | 0.186
  test_backward_contention            2 x 3 under 12 x 20: n2 = 240 on every cell                     6.4e-8 | 0.131     2.6e-7 | 0.004
  test_backward_borders, _c_entry     r = 1, both images leave fmap2 cells untouched (exact zeros)    6.7e-8 | 0.148     1.2e-7 | 0.107
  test_backward_integer_coordinates                                                                   7.0e-8 | 0.081     1.4e-7 | 0.063
  test_backward_nonfinite_coordinates seven pixels with NaN / +-inf / +-1e12: rows of exact zeros     8.1e-8 | 0.114     1.4e-7 | 0.036
  test_backward_coordinate_sets       N = 2, summed by the op                                         9.3e-8 | 0.020     1.4e-7 | 0.021
"""
import ctypes
import functools

import pytest
import torch

from oracle import raft_oracle as O
from op_gate import OP_TOL, SENTINEL, U, flat_out, gates, guarded, rel, tail_kept

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
MODES = (1, 2, 3, 4)                    # per-pixel | window-sharing 8x4 | 8x8 | the overflow kernel on every patch
DTYPES = (torch.float32, torch.bfloat16)
WS_NP_MAX = 512


# ---------------------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------------------
def grid_xy(B, H, W):
    """[B, 1, H, W, 2] (x, y): the identity coordinate field of an H x W map"""
    return O.coords_grid(B, H, W).permute(0, 2, 3, 1)[:, None].contiguous()


def maps(g, B, H1, W1, H2, W2, C, dtype):
    """feature maps as the kernel gets them (fp32 values; for bf16 the bf16-rounded ones)"""
    f1, f2 = torch.randn(B, H1, W1, C, generator=g), torch.randn(B, H2, W2, C, generator=g)
    return (f1, f2) if dtype == torch.float32 else (f1.bfloat16().float(), f2.bfloat16().float())


def fwd_reference(f1, f2, coords, r):
    """float64 forward on the kernel's own inputs and the exact sum of magnitudes (NaN exactly where the result is NaN)"""
    c = coords.double()
    ref = O.alt_corr_forward(f1.double(), f2.double(), c, r)
    mag = O.alt_corr_forward(f1.double().abs(), f2.double().abs(), c, r)
    assert torch.equal(torch.isnan(ref), torch.isnan(mag)) and not bool(torch.isinf(ref).any())
    return ref, mag


def check_fwd(what, got, ref, mag, C):
    """the NaN pattern, then gates 1 and 2 on every other cell with K = C + 10 (module docstring)"""
    got = got.detach().double().cpu().reshape(ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), \
        f"{what}: NaN pattern differs in {int((torch.isnan(got) != nan).sum())} cells ({int(nan.sum())} expected)"
    zero = torch.zeros((), dtype=torch.float64)
    return gates(what, torch.where(nan, zero, got), torch.where(nan, zero, ref), torch.where(nan, zero, mag), C + 10, keep=~nan)


def op_forward(gpu, f1, f2, coords, r, mode, dtype):
    """`torch.ops.pfk.altcorr_forward` on guarded inputs with one kernel forced; two runs, the same bits"""
    a, b, c = guarded(f1.to(dtype), gpu), guarded(f2.to(dtype), gpu), guarded(coords, gpu)
    torch.ops.pfk.debug_set_altcorr(mode)
    try:
        out = torch.ops.pfk.altcorr_forward(a, b, c, r)
        again = torch.ops.pfk.altcorr_forward(a, b, c, r)
        torch.cuda.synchronize()
    finally:
        torch.ops.pfk.debug_set_altcorr(0)
    assert out.dtype == torch.float32 and tuple(out.shape) == (f1.shape[0], coords.shape[1], (2 * r + 1) ** 2, f1.shape[1], f1.shape[2])
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), f"mode {mode}: a second run gives other bits"
    return out


def forward_all(gpu, what, f1, f2, coords, r, dtype, ref, mag, modes=MODES):
    C = f1.shape[3]
    return [check_fwd(f"{what} {str(dtype)[6:]} mode {m}", op_forward(gpu, f1, f2, coords, r, m, dtype), ref, mag, C) for m in modes]


def patch_boxes(coords, tpy, H2, W2, r):
    """`patch_box()` of pfk_altcorr.hip restated: coords [B, H1, W1, 2] fp32 -> the (w, h) of every 8 x tpy patch's clipped bounding
    box, [B, tiles_y, tiles_x, 2].  A patch takes the GEMM when w * h <= WS_NP_MAX (`patch_takes_gemm`)."""
    assert coords.dtype == torch.float32
    B, H1, W1, _ = coords.shape
    n, big = 2 * r + 2, 1 << 30
    ty, tx = -(-H1 // tpy), -(-W1 // 8)
    fx, fy = torch.floor(coords[..., 0]), torch.floor(coords[..., 1])
    okx, oky = fx.abs() < 1.0e9, fy.abs() < 1.0e9                 # false for NaN and +-inf, like fabsf(fx) < 1.0e9f
    x0 = torch.where(okx, fx, torch.zeros_like(fx)).long() - r
    y0 = torch.where(oky, fy, torch.zeros_like(fy)).long() - r
    use = okx & oky & (x0 < W2) & (y0 < H2) & (x0 + n > 0) & (y0 + n > 0)

    def tiles(v, fill, red):
        full = torch.full((B, ty * tpy, tx * 8), fill, dtype=torch.long)
        full[:, :H1, :W1] = torch.where(use, v, torch.full_like(v, fill))
        return red(red(full.view(B, ty, tpy, tx, 8), 4).values, 2).values

    lo_x, hi_x = tiles(x0.clamp_min(0), big, torch.min), tiles((x0 + n).clamp_max(W2), -big, torch.max)
    lo_y, hi_y = tiles(y0.clamp_min(0), big, torch.min), tiles((y0 + n).clamp_max(H2), -big, torch.max)
    some = (hi_x > lo_x) & (hi_y > lo_y)
    zero = torch.zeros_like(lo_x)
    return torch.stack([torch.where(some, hi_x - lo_x, zero), torch.where(some, hi_y - lo_y, zero)], -1)


def box_points(coords, tpy, H2, W2, r):
    b = patch_boxes(coords, tpy, H2, W2, r)
    return b[..., 0] * b[..., 1]


# ---------------------------------------------------------------------------------------------------------------------
# forward 1: channel and radius edges
# ---------------------------------------------------------------------------------------------------------------------
# C = 4: one float4 on lane 0 of each tap group, one quarter of a K step | 20: a K step of 16 and one of 4 | 68, 132: one / two full
# 64-channel register chunks and one lane of the next | 512: MAX_C4
CHANNEL_RADIUS = [(4, 1), (4, 4), (20, 2), (20, 3), (68, 1), (68, 2), (68, 4), (132, 1), (132, 3), (132, 4), (512, 2), (512, 4)]


@functools.lru_cache(maxsize=None)
def channel_case(C, r, dtype):
    g = torch.Generator().manual_seed(1000 * C + r)
    B, H1, W1, H2, W2 = 2, 11, 13, 7, 8                                   # ragged patch grid both ways; fmap2 of another size
    f1, f2 = maps(g, B, H1, W1, H2, W2, C, dtype)
    coords = grid_xy(B, H1, W1) * (W2 / W1) + torch.randn(B, 1, H1, W1, 2, generator=g) * 1.5    # windows over every border
    return (f1, f2, coords) + fwd_reference(f1, f2, coords, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("C,r", CHANNEL_RADIUS)
def test_forward_channel_radius(gpu, C, r, dtype):
    f1, f2, coords, ref, mag = channel_case(C, r, dtype)
    forward_all(gpu, f"fwd C={C} r={r}", f1, f2, coords, r, dtype, ref, mag)


# ---------------------------------------------------------------------------------------------------------------------
# forward 2: integer coordinates
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_case(field, r, dtype):
    g = torch.Generator().manual_seed(77 + r)
    B, H1, W1, C = 2, 11, 13, 20
    if field == "identity":               # every dx = dy = 0: the first refinement iteration of every model
        H2, W2, coords = H1, W1, grid_xy(B, H1, W1)
    elif field == "half":                 # the second pyramid level: every fraction 0 or 0.5
        H2, W2, coords = 6, 7, grid_xy(B, H1, W1) / 2
    else:                                 # integer shift on a smaller map: windows hang over all four borders, some miss the map
        H2, W2, coords = 7, 8, grid_xy(B, H1, W1) + torch.tensor([-3.0, -2.0])
    assert bool((coords * 2 == torch.floor(coords * 2)).all())
    f1, f2 = maps(g, B, H1, W1, H2, W2, C, dtype)
    return (f1, f2, coords.contiguous()) + fwd_reference(f1, f2, coords, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("field", ["identity", "half", "shifted"])
def test_forward_integer_coordinates(gpu, field, r, dtype):
    f1, f2, coords, ref, mag = integer_case(field, r, dtype)
    forward_all(gpu, f"fwd integer {field} r={r}", f1, f2, coords, r, dtype, ref, mag)


# ---------------------------------------------------------------------------------------------------------------------
# forward 3: non-finite and extreme coordinates
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nonfinite_case(dtype):
    g = torch.Generator().manual_seed(5)
    B, H1, W1, H2, W2, C, r = 1, 12, 24, 9, 10, 20, 3
    f1, f2 = maps(g, B, H1, W1, H2, W2, C, dtype)
    coords = grid_xy(B, H1, W1) * (W2 / W1) + torch.randn(B, 1, H1, W1, 2, generator=g)
    c = coords[0, 0]
    c[0, 0, 0] = NAN                                   # NaN in x only
    c[0, 2, 1] = NAN                                   # NaN in y only
    c[1, 1] = torch.tensor([INF, 3.5])
    c[1, 3] = torch.tensor([2.5, -INF])
    c[2, 0] = torch.tensor([9.9e8, 1.5])               # finite, below the kernel's 1e9 cut: the window origin is computed in int
    c[2, 2] = torch.tensor([1.5, -9.9e8])
    c[2, 5] = torch.tensor([9.9e8, -9.9e8])
    c[3, 1] = torch.tensor([1.0e9, 2.5])               # at the cut and above it: no tap, fraction 0
    c[3, 3] = torch.tensor([2.5, 2.0 ** 31])
    c[3, 5] = torch.tensor([1.0e12, -1.0e12])
    c[8, 3] = torch.tensor([-2.0 ** 31, 4.25])
    c[0:8, 8:16] = torch.tensor([-30.0, 2.5])          # an 8 x 8 block (two 8x4 patches, one 8x8 patch) left of the map: NP == 0
    c[0:8, 16:24] = NAN                                # and one of NaN
    c[9, 20] = INF
    for tpy in (4, 8):
        np_ = box_points(c[None], tpy, H2, W2, r)[0]
        assert int(np_[0, 1]) == 0 and int(np_[0, 2]) == 0 and int(np_[8 // tpy - 1, 1]) == 0 and int(np_[0, 0]) > 0
    ref, mag = fwd_reference(f1, f2, coords, r)
    # the contract per pixel: NaN / inf -> a window of NaN; beyond the cut or off the map -> a window of exact zeros
    for y, x in ((0, 0), (0, 2), (1, 1), (1, 3), (0, 16), (7, 23), (9, 20)):
        assert bool(torch.isnan(ref[0, 0, :, y, x]).all())
    for y, x in ((2, 0), (2, 2), (2, 5), (3, 1), (3, 3), (3, 5), (8, 3), (0, 8), (7, 15)):
        assert bool((mag[0, 0, :, y, x] == 0).all())
    return f1, f2, coords, ref, mag, r


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_forward_nonfinite_coordinates(gpu, dtype):
    f1, f2, coords, ref, mag, r = nonfinite_case(dtype)
    forward_all(gpu, "fwd non-finite", f1, f2, coords, r, dtype, ref, mag)


# ---------------------------------------------------------------------------------------------------------------------
# forward 4: box-size edges
# ---------------------------------------------------------------------------------------------------------------------
BOX_POINTS = (1, 32, 33, 512, 513)       # one point | three idle waves | the second column block holds one point | 16 full column
                                         # blocks (32 x 16) | one more than WS_NP_MAX (27 x 19): the overflow kernel


@functools.lru_cache(maxsize=None)
def box_case(tpy, dtype):
    """one row of 8 x tpy patches whose clipped boxes have exactly BOX_POINTS points, and a ragged sixth patch"""
    g = torch.Generator().manual_seed(40 + tpy)
    B, H1, W1, H2, W2, C, r = 1, tpy, 44, 24, 40, 8, 4
    n = 2 * r + 2                                                          # 10: a window of floor fx covers columns fx - 4 .. fx + 5
    i = torch.arange(tpy * 8).view(tpy, 8)
    zero = torch.zeros_like(i)
    fx, fy = torch.zeros(H1, W1, dtype=torch.long), torch.zeros(H1, W1, dtype=torch.long)
    # 1 = 1 x 1: only column 0 / row 0 of the window in the map:                      fx - r + n = 1
    fx[:, 0:8], fy[:, 0:8] = zero + (1 - n + r), zero + (1 - n + r)
    # 32 = 8 x 4: columns 0..7 and rows 0..3 in the map:                              fx - r + n = 8, fy - r + n = 4
    fx[:, 8:16], fy[:, 8:16] = zero + (8 - n + r), zero + (4 - n + r)
    # 33 = 11 x 3: two floors one apart inside the map, rows 0..2
    fx[:, 16:24], fy[:, 16:24] = 10 + i % 2, zero + (3 - n + r)
    # 512 = 32 x 16: floors 22 apart in x and 6 apart in y, inside the map
    fx[:, 24:32], fy[:, 24:32] = 5 + 11 * (i % 3), 6 + 3 * (i % 3)
    # 513 = 27 x 19: 17 apart in x, 9 apart in y
    fx[:, 32:40], fy[:, 32:40] = 5 + 17 * (i % 2), 6 + 9 * (i % 2)
    fx[:, 40:44], fy[:, 40:44] = 20 + i[:, :4] % 8, 10 + i[:, :4] // 8
    frac = torch.rand(H1, W1, 2, generator=g) * 0.875 + 0.0625
    coords = (torch.stack([fx, fy], -1).float() + frac)[None, None].contiguous()
    assert torch.equal(torch.floor(coords[0, 0]).long(), torch.stack([fx, fy], -1))
    f1, f2 = maps(g, B, H1, W1, H2, W2, C, dtype)
    return (f1, f2, coords) + fwd_reference(f1, f2, coords, r) + (r, H2, W2)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("tpy", [4, 8])
def test_forward_box_sizes(gpu, tpy, dtype):
    f1, f2, coords, ref, mag, r, H2, W2 = box_case(tpy, dtype)
    boxes = patch_boxes(coords[:, 0], tpy, H2, W2, r)[0, 0]
    points = [int(w * h) for w, h in boxes[:5]]
    assert points == list(BOX_POINTS), points
    assert [tuple(b.tolist()) for b in boxes[:5]] == [(1, 1), (8, 4), (11, 3), (32, 16), (27, 19)]
    assert [p <= WS_NP_MAX for p in points] == [True, True, True, True, False]       # patch_takes_gemm
    assert 0 < int(boxes[5, 0] * boxes[5, 1]) <= WS_NP_MAX
    forward_all(gpu, f"fwd boxes 8x{tpy}", f1, f2, coords, r, dtype, ref, mag)


# ---------------------------------------------------------------------------------------------------------------------
# forward 5: tiny maps
# ---------------------------------------------------------------------------------------------------------------------
TINY = [(5, 13, 1, 1), (5, 13, 1, 2), (5, 13, 2, 1), (1, 1, 7, 8), (3, 5, 7, 8), (1, 9, 7, 8)]        # H1, W1, H2, W2


@functools.lru_cache(maxsize=None)
def tiny_case(H1, W1, H2, W2, dtype):
    g = torch.Generator().manual_seed(H1 * 1000 + W1 * 100 + H2 * 10 + W2)
    B, C, r = 2, 20, 4
    f1, f2 = maps(g, B, H1, W1, H2, W2, C, dtype)
    centre = torch.tensor([(W2 - 1) / 2, (H2 - 1) / 2])
    coords = centre + torch.randn(B, 1, H1, W1, 2, generator=g) * 2.5          # around the map, some windows past it
    coords[0, 0, 0, 0] = torch.floor(centre)                                    # one integer coordinate
    return (f1, f2, coords.contiguous()) + fwd_reference(f1, f2, coords, r) + (r,)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("H1,W1,H2,W2", TINY)
def test_forward_tiny_maps(gpu, H1, W1, H2, W2, dtype):
    f1, f2, coords, ref, mag, r = tiny_case(H1, W1, H2, W2, dtype)
    assert float(mag.nan_to_num().max()) > 0
    forward_all(gpu, f"fwd tiny {H1}x{W1} on {H2}x{W2}", f1, f2, coords, r, dtype, ref, mag)


# ---------------------------------------------------------------------------------------------------------------------
# forward 6: the heuristic (mode 0): plan kernel and the 5/8 gate
# ---------------------------------------------------------------------------------------------------------------------
GATE_GRID = (4, 32, 64)                 # B * ceil(H1 / 4) * ceil(W1 / 8) = 256: the smallest grid the heuristic hands to the plan kernel
GATE_C, GATE_R = 8, 3


def spoiled_field(B, H, W, n_spoiled):
    """the identity field plus a constant fraction, with one pixel of each of the first `n_spoiled` patches of the order below sent
    (+-32, +-16) away inside the map: that patch's box overflows"""
    coords = grid_xy(B, H, W) + torch.tensor([0.25, 0.625])
    ty, tx = H // 4, W // 8
    order = [p for k in range(8) for p in range(B * ty * tx) if p % 8 == k]
    for p in order[:n_spoiled]:
        b, t = divmod(p, ty * tx)
        y, x = (t // tx) * 4 + 1, (t % tx) * 8 + 3
        coords[b, 0, y, x, 0] += 32.0 if x < W // 2 else -32.0
        coords[b, 0, y, x, 1] += 16.0 if y < H // 2 else -16.0
    return coords.contiguous()


@functools.lru_cache(maxsize=None)
def gate_case(field, dtype):
    g = torch.Generator().manual_seed(sum(map(ord, field)))
    B, H, W = (3, 18, 130) if field == "255_patches" else GATE_GRID
    npatch = B * -(-H // 4) * -(-W // 8)
    if field == "smooth":
        low = torch.nn.functional.interpolate(torch.randn(B, 2, 3, 4, generator=g) * 2, size=(H, W), mode="bicubic", align_corners=True)
        coords = grid_xy(B, H, W) + low.permute(0, 2, 3, 1)[:, None]
    elif field == "noise":
        coords = grid_xy(B, H, W) + torch.randn(B, 1, H, W, 2, generator=g) * 6
    elif field == "255_patches":
        coords = grid_xy(B, H, W) + torch.randn(B, 1, H, W, 2, generator=g) * 0.6
    else:
        coords = spoiled_field(B, H, W, npatch - int(field))
    coords = coords.contiguous()
    qualify = int((box_points(coords[:, 0], 4, H, W, GATE_R) <= WS_NP_MAX).sum())
    f1, f2 = maps(g, B, H, W, H, W, GATE_C, dtype)
    return (f1, f2, coords) + fwd_reference(f1, f2, coords, GATE_R) + (npatch, qualify)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("field", ["smooth", "noise", "160", "159", "255_patches"])
def test_forward_heuristic_gate(gpu, field, dtype):
    """mode 0 on both sides of `8 s >= 5 npatch` and of the size rule.  Which pass ran cannot be observed; the output must be right:
    gate on (all patches; 160 of 256 with 96 overflow patches beside the GEMM patches), gate off (159 of 256; iid noise)."""
    f1, f2, coords, ref, mag, npatch, qualify = gate_case(field, dtype)
    if field == "255_patches":
        assert npatch == 255
    else:
        assert npatch == 256
        if field == "smooth":
            assert qualify == npatch
        elif field == "noise":
            assert 8 * qualify < 5 * npatch
        else:
            assert qualify == int(field) and (8 * qualify >= 5 * npatch) == (field == "160")
    forward_all(gpu, f"fwd heuristic {field}", f1, f2, coords, GATE_R, dtype, ref, mag, modes=(0,))


# ---------------------------------------------------------------------------------------------------------------------
# forward 7: several coordinate sets through the op
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sets_case(dtype):
    g = torch.Generator().manual_seed(3)
    B, H1, W1, H2, W2, C, r, N = 2, 9, 11, 7, 8, 20, 2, 3
    f1, f2 = maps(g, B, H1, W1, H2, W2, C, dtype)
    coords = (grid_xy(B, H1, W1) * 0.7 + torch.randn(B, N, H1, W1, 2, generator=g) * 2).contiguous()
    return (f1, f2, coords) + fwd_reference(f1, f2, coords, r) + (r,)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_forward_coordinate_sets(gpu, dtype):
    """N = 3: one workspace shared by the launches, per-set output copies"""
    f1, f2, coords, ref, mag, r = sets_case(dtype)
    forward_all(gpu, "fwd N=3", f1, f2, coords, r, dtype, ref, mag, modes=(0,) + MODES)


# ---------------------------------------------------------------------------------------------------------------------
# forward 8 / backward sentinel case: the C entry points through ctypes
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capi():
    import ptlflow_amd
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    p, i = ctypes.c_void_p, ctypes.c_int
    for fn in (lib.pfk_altcorr_forward_f32, lib.pfk_altcorr_forward_bf16):
        fn.argtypes, fn.restype = [p, p, p, p] + [i] * 7 + [p, p], i
    lib.pfk_altcorr_backward_f32.argtypes, lib.pfk_altcorr_backward_f32.restype = [p] * 6 + [i] * 7 + [p], i
    lib.pfk_altcorr_workspace_bytes.argtypes, lib.pfk_altcorr_workspace_bytes.restype = [i, i, i], ctypes.c_longlong
    return lib


@pytest.mark.parametrize("with_workspace", [True, False], ids=("workspace", "null"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_forward_c_entry(gpu, dtype, with_workspace):
    """`pfk_altcorr_forward_f32` / `_bf16` as INTEGRATION.md's stub calls the library, on the 160-of-256 field (GEMM and overflow
    patches in one launch): the output inside a sentinel buffer, with the plan kernel's workspace (inside one too) and with NULL"""
    lib = capi()
    f1, f2, coords, ref, mag, npatch, qualify = gate_case("160", dtype)
    assert 0 < qualify < npatch
    B, H, W, C = f1.shape
    a, b, c = guarded(f1.to(dtype), gpu), guarded(f2.to(dtype), gpu), guarded(coords, gpu)
    nws = lib.pfk_altcorr_workspace_bytes(B, H, W) // 4
    assert nws == npatch // 8
    fn = lib.pfk_altcorr_forward_f32 if dtype == torch.float32 else lib.pfk_altcorr_forward_bf16
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        flat, out = flat_out((B, (2 * GATE_R + 1) ** 2, H, W), gpu)
        ws = torch.full((nws + 64,), 0x5a5a5a5a, dtype=torch.int32, device=gpu)
        st = fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), out.data_ptr(), B, H, W, H, W, C, GATE_R,
                ctypes.c_void_p(ws.data_ptr()) if with_workspace else None, stream)
        torch.cuda.synchronize()
        assert st == 0, f"status {st}"
        assert tail_kept(flat), "memory past the output was written"
        assert bool((ws[nws:] == 0x5a5a5a5a).all()), "memory past the workspace was written"
        if with_workspace:
            assert int(ws[:nws].sum()) == qualify, "the plan kernel's counts differ from patch_boxes()"
        else:
            assert bool((ws == 0x5a5a5a5a).all())
        assert bool((out != SENTINEL).all()), "output cells were left unwritten"
        runs.append(out)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "a second run gives other bits"
    check_fwd(f"fwd C entry {str(dtype)[6:]} ws={int(with_workspace)}", runs[0], ref, mag, C)


# ---------------------------------------------------------------------------------------------------------------------
# the Python seam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=("f16", "bf16"))
def test_seam_half_maps(gpu, dtype):
    """`altcorr.forward` returns the maps' dtype.  fp16 maps: the fp32 kernel on the up-cast maps, then one fp16 rounding; bf16 maps:
    the bf16 kernel, then one bf16 rounding.  The fp32 result behind the seam takes the full gate, the seam's result must be its
    rounding bit for bit and, stated per element, lie within the bound plus half a unit of the narrow format."""
    import ptlflow_amd.altcorr as altcorr
    g = torch.Generator().manual_seed(16)
    B, H1, W1, H2, W2, C, r = 2, 9, 11, 7, 8, 20, 3
    f1, f2 = torch.randn(B, H1, W1, C, generator=g).to(dtype), torch.randn(B, H2, W2, C, generator=g).to(dtype)
    coords = (grid_xy(B, H1, W1) * 0.7 + torch.randn(B, 1, H1, W1, 2, generator=g) * 2).contiguous()
    ref, mag = fwd_reference(f1.float(), f2.float(), coords, r)
    kernel_dtype = torch.bfloat16 if dtype == torch.bfloat16 else torch.float32
    a, b, c = guarded(f1.to(kernel_dtype), gpu), guarded(f2.to(kernel_dtype), gpu), guarded(coords, gpu)
    wide = torch.ops.pfk.altcorr_forward(a, b, c, r)
    check_fwd(f"seam {str(dtype)[6:]} fp32 result", wide, ref, mag, C)
    (got,) = altcorr.forward(f1.to(gpu), f2.to(gpu), c, r)
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape)
    assert torch.equal(got.view(torch.int16), wide.to(dtype).view(torch.int16)), "the seam's result is not the kernel's, rounded once"
    eps, tiny = (2.0 ** -11, 2.0 ** -25) if dtype == torch.float16 else (2.0 ** -8, 0.0)     # half a unit: relative | fp16 subnormals
    bound = (C + 10) * U * mag
    bound = bound + eps * (ref.abs() + bound) + tiny
    assert bool(((got.double().cpu() - ref).abs() <= bound).all())
    assert rel(got, ref) <= OP_TOL + eps                 # the rounding moves every element by at most eps of itself


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def finite_far(coords):
    """coordinates the backward treats as reaching no tap (NaN, +-inf, beyond the cut) replaced by (-1e6, -1e6)"""
    bad = (~(torch.floor(coords).abs() < 1.0e9)).any(-1, keepdim=True)
    return torch.where(bad, torch.full_like(coords, -1.0e6), coords), bad[..., 0]


def tap_counts(coords, r, B, H2, W2):
    """the number of in-map taps per fmap1 pixel and per fmap2 cell, by an integer scatter (summed over the coordinate sets)"""
    n = 2 * r + 2
    N, H1, W1 = coords.shape[1:4]
    fl = torch.floor(coords.double()).long()                            # finite: finite_far() ran first
    off = torch.arange(n)
    xx = (fl[..., 0] - r)[..., None, None] + off[None, :]               # [B, N, H1, W1, 1, n]
    yy = (fl[..., 1] - r)[..., None, None] + off[:, None]               # [B, N, H1, W1, n, 1]
    ok = (xx >= 0) & (xx < W2) & (yy >= 0) & (yy < H2)                  # [B, N, H1, W1, n, n]
    n1 = ok.sum((1, 4, 5))                                              # [B, H1, W1]
    cell = (torch.arange(B).view(B, 1, 1, 1, 1, 1) * H2 + yy.clamp(0, H2 - 1)) * W2 + xx.clamp(0, W2 - 1)
    n2 = torch.zeros(B * H2 * W2, dtype=torch.long).index_add_(0, cell[ok], torch.ones(int(ok.sum()), dtype=torch.long))
    return n1, n2.view(B, H2, W2)


def bwd_reference(f1, f2, coords, grad, r):
    """float64 autograd through the oracle's forward: gradients, their sums of magnitudes, the term counts per element"""
    B, H2, W2 = f2.shape[:3]
    c, bad = finite_far(coords)
    res = []
    for absolute in (False, True):
        a, b, go = f1.double(), f2.double(), grad.double()
        if absolute:
            a, b, go = a.abs(), b.abs(), go.abs()
        a.requires_grad_(), b.requires_grad_()
        O.alt_corr_forward(a, b, c.double(), r).backward(go)
        res += [a.grad, b.grad]
    n1, n2 = tap_counts(c, r, B, H2, W2)
    C = f1.shape[3]
    return {"g1": res[0], "g2": res[1], "m1": res[2], "m2": res[3], "bad": bad.any(1),
            "n1": n1[..., None].expand(-1, -1, -1, C).double(), "n2": n2[..., None].expand(-1, -1, -1, C).double()}


def check_bwd(what, ref, g1, g2, again1, again2):
    r1 = gates(what + " fmap1_grad", g1, ref["g1"], ref["m1"], ref["n1"] + 12)
    r2 = gates(what + " fmap2_grad", g2, ref["g2"], ref["m2"], ref["n2"] + 12)
    assert bool((g1.cpu()[ref["n1"] == 0] == 0).all()) and bool((g2.cpu()[ref["n2"] == 0] == 0).all()), \
        f"{what}: an element no in-map tap reaches is not an exact zero"
    assert torch.equal(g1.view(torch.int32), again1.view(torch.int32)), f"{what}: fmap1_grad of a second run has other bits"
    diff = (g2.double().cpu() - again2.double().cpu()).abs()
    assert bool((diff <= (ref["n2"] + 12) * U * ref["m2"]).all()), f"{what}: fmap2_grad of two runs differs by more than the bound"
    return r1, r2


def op_backward(gpu, what, f1, f2, coords, grad, r, ref):
    a, b, c, go = (guarded(t, gpu) for t in (f1, f2, coords, grad))
    g1, g2, gc = torch.ops.pfk.altcorr_backward(a, b, c, go, r)
    h1, h2, _ = torch.ops.pfk.altcorr_backward(a, b, c, go, r)
    torch.cuda.synchronize()
    assert tuple(gc.shape) == tuple(coords.shape) and gc.dtype == torch.float32 and bool((gc == 0).all())
    assert g1.shape == f1.shape and g2.shape == f2.shape
    return check_bwd(what, ref, g1, g2, h1, h2)


# C = 4 | 68, 132: register chunks i >= 1 | 512: all eight
BWD_CHANNEL_RADIUS = [(4, 1), (4, 4), (68, 1), (68, 3), (132, 3), (132, 4), (512, 1), (512, 4)]


@functools.lru_cache(maxsize=None)
def bwd_case(name, C=20, r=3):
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 1000 * C + r)
    B, H1, W1, H2, W2, N = 2, 9, 11, 7, 8, 1
    if name == "contention":            # a map much coarser than fmap1, every window over it: hundreds of atomics per cell
        H1, W1, H2, W2 = 12, 20, 2, 3
    elif name == "sets":
        N = 2
    f1, f2 = torch.randn(B, H1, W1, C, generator=g), torch.randn(B, H2, W2, C, generator=g)
    coords = grid_xy(B, H1, W1) * (W2 / W1) + torch.randn(B, N, H1, W1, 2, generator=g) * 1.5
    if name == "contention":
        coords = torch.rand(B, N, H1, W1, 2, generator=g) * torch.tensor([W2 - 1.0, H2 - 1.0])     # confined to the map
    elif name == "borders":             # r = 1; image 0: windows over the top and left borders, the far rows / columns of fmap2
        # never reached; image 1: over the bottom and right borders, the near ones never reached; one 8x4 patch entirely outside
        coords = grid_xy(B, H1, W1) * 0.4 + torch.rand(B, N, H1, W1, 2, generator=g)
        coords[0] -= 2.0
        coords[1] += 4.0
        coords[:, :, 0:4, 0:8] = torch.tensor([-30.0, 2.5])
    elif name == "integer":             # the folded tap weights are exact zeros
        coords = torch.round(coords)
        coords[1] = grid_xy(1, H1, W1)[0] / 2
    elif name == "nonfinite":
        c = coords[0, 0]
        c[0, 0, 0] = NAN
        c[0, 1, 1] = NAN
        c[1, 2] = torch.tensor([INF, 3.5])
        c[2, 3] = torch.tensor([2.5, -INF])
        c[3, 4] = torch.tensor([1.0e12, 2.5])
        c[4, 5] = torch.tensor([2.5, -1.0e12])
        c[5, 6] = NAN
    coords = coords.contiguous()
    grad = torch.randn(B, N, (2 * r + 1) ** 2, H1, W1, generator=g)
    return f1, f2, coords, grad, bwd_reference(f1, f2, coords, grad, r)


@pytest.mark.parametrize("C,r", BWD_CHANNEL_RADIUS)
def test_backward_channel_radius(gpu, C, r):
    f1, f2, coords, grad, ref = bwd_case("plain", C, r)
    op_backward(gpu, f"bwd C={C} r={r}", f1, f2, coords, grad, r, ref)


def test_backward_contention(gpu):
    f1, f2, coords, grad, ref = bwd_case("contention")
    assert int(ref["n2"].min()) >= 200
    op_backward(gpu, "bwd contention", f1, f2, coords, grad, 3, ref)


def test_backward_borders(gpu):
    """windows over every border and a patch entirely outside; fmap2 cells no in-map tap reaches are exact zeros"""
    f1, f2, coords, grad, ref = bwd_case("borders", 20, 1)
    assert bool((ref["n1"][:, 0:4, 0:8] == 0).all())
    for b in range(2):
        assert bool((ref["n2"][b] == 0).any()) and bool((ref["n2"][b] > 0).any())
    op_backward(gpu, "bwd borders", f1, f2, coords, grad, 1, ref)


def test_backward_integer_coordinates(gpu):
    f1, f2, coords, grad, ref = bwd_case("integer")
    op_backward(gpu, "bwd integer", f1, f2, coords, grad, 3, ref)


def test_backward_nonfinite_coordinates(gpu):
    """A pixel whose coordinate is NaN, +-inf or beyond the 1e9 cut reaches no tap: its `fmap1_grad` row is exactly 0, it adds nothing
    to `fmap2_grad`, everything stays finite (`gates` asserts that).  The reference extension leaves this case undefined and in
    practice writes NaN (module docstring); the float64 reference here has those coordinates at (-1e6, -1e6)."""
    f1, f2, coords, grad, ref = bwd_case("nonfinite")
    bad = ref["bad"]
    assert int(bad.sum()) == 7 and bool((ref["n1"][bad] == 0).all())
    a, b, c, go = (guarded(t, gpu) for t in (f1, f2, coords, grad))
    g1, g2, _ = torch.ops.pfk.altcorr_backward(a, b, c, go, 3)
    assert bool((g1.cpu()[bad] == 0).all())
    op_backward(gpu, "bwd non-finite", f1, f2, coords, grad, 3, ref)


def test_backward_coordinate_sets(gpu):
    """N = 2, summed by the op; `coords_grad` all zeros with `coords`' shape (checked in `op_backward`)"""
    f1, f2, coords, grad, ref = bwd_case("sets")
    assert coords.shape[1] == 2
    op_backward(gpu, "bwd N=2", f1, f2, coords, grad, 3, ref)


def test_backward_c_entry(gpu):
    """`pfk_altcorr_backward_f32` through ctypes: both gradients inside sentinel-filled buffers whose tails must survive, every
    element of both overwritten"""
    lib = capi()
    f1, f2, coords, grad, ref = bwd_case("borders", 20, 1)
    (B, H1, W1, C), (H2, W2) = f1.shape, f2.shape[1:3]
    a, b, c, go = (guarded(t, gpu) for t in (f1, f2, coords, grad))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        flat1, g1 = flat_out(tuple(f1.shape), gpu)
        flat2, g2 = flat_out(tuple(f2.shape), gpu)
        st = lib.pfk_altcorr_backward_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), go.data_ptr(), g1.data_ptr(), g2.data_ptr(),
                                          B, H1, W1, H2, W2, C, 1, stream)
        torch.cuda.synchronize()
        assert st == 0, f"status {st}"
        assert tail_kept(flat1) and tail_kept(flat2), "memory past a gradient was written"
        assert bool((g1 != SENTINEL).all()) and bool((g2 != SENTINEL).all()), "gradient elements were left unwritten"
        runs += [g1, g2]
    check_bwd("bwd C entry", ref, *runs)
