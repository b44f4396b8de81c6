"""The encoder kernels of ptlflow_amd/csrc/pfk_encoder.hip held to the fp64 op gate, kernel by kernel: the 7x7/2 stem (VALU, MFMA, the
two-image `stem2`), the stem weight gradient, the instance-norm statistics on fp32 and bf16 rows, `norm_apply` in its four
instantiations, `norm_apply_res` and the norm backward — all twelve C entry points, through `torch.ops.pfk`.

Gates on every kernel output (tests/op_gate.py's `gates`, `gates_b16`, `Rows`, `OP_TOL`, `SENTINEL`):
 1. relative L2 <= 5e-6 against float64 on the CPU ON THE KERNEL'S OWN INPUTS (bf16 rows: the bf16 values; `mean` / `rstd` of the
    apply and backward kernels: the fp32 tensors the kernel gets).  A bf16 OUTPUT cannot meet 5e-6 (one rounding to 8 significand bits
    is 2^-9 on average); it must instead be, bit for bit, the round-to-nearest-even bf16 of the fp32 output of the same kernel body on
    the same (widened) inputs — which is itself under gate 1 — and it gets gate 2.
 2. a per-element bound that needs no measurement, K * 2^-24 * (sum of the magnitudes of the element's terms), the magnitudes computed
    in float64 next to the reference; where they are 0 the output must be an exact zero.  K, counted from the kernel text (u = 2^-24):
      stem, fp32 out      K = n + 2, n = 49 cin + 1 terms (the products and the bias): n roundings of the running sum whatever the
                          order (fused multiply-adds, MFMA K-steps, the second image's pass), + 2 to spare; on sum |x w| + |b|.
                          The relu is 1-Lipschitz.
      stem, bf16 out      the same times (1 + 2^-8), plus 2^-8 |ref|: one round-to-nearest to 8 significand bits is 2^-8 relative at
                          worst (1 + 2^-8 lies half-way between the bf16 values 1 and 1 + 2^-7), not 2^-9.
      stem wgrad dw, db   K = n + 2, n = B Ho Wo, on sum_p |dy img| / sum_p |dy|: any order of the sum (eight pixels per thread, tiles
                          per block, four waves, up to 512 partials) stays inside it; taps in the zero padding contribute 0.
      stats mean          u |ref| + (HW + 2) 2^-53 mean|x|: one rounding to float of a double sum.  (2 u |ref| would assume that the
                          double sum's error is small next to |mean|, which a cancelling mean does not promise.)
      stats rstd          relative u + 4 * 2^-53 + (1.5 HW + 3) 2^-53 (sum x^2 / HW) / (var + eps): the double sum of x^2 carries
                          HW 2^-53 of itself, mean^2 twice that of the double sum of x (2 |m| d m, |m| mean|x| <= mean x^2), the
                          subtraction 2^-53: (3 HW + 2) 2^-53 of mean x^2 on var, halved by the square root; the addition of eps,
                          the square root and the division 2.5 * 2^-53; the rounding to float u.  The reference takes
                          float32(eps) widened to double, as the kernel does, and a two-pass float64 variance.
      norm_apply          K = 3 on |(x - m) r| + |residual|: the subtraction, the product, the addition; bf16 out as for the stem;
                          bf16 rows widen exactly.
      norm_apply_res      K = 5 on |(x - m) r| + |(res - rm) rr|: two roundings on each side and the addition.
      norm_bwd sum_g      K = 2 on sum |g|;  sum_gxhat  K = 4 on sum |g xhat| (xhat is formed in fp32 with two roundings, one more to
                          float);  dx  K = 6 on rstd (|g| + |s1| / HW + |xhat| sum |g xhat| / HW) — xhat twice (in s2 and as the
                          factor), each with two roundings, and the rounding to float — plus the double-precision sums'
                          (HW + 4) 2^-53 of rstd (sum |g| / HW + |xhat| sum |g xhat| / HW).  The relu mask of the reference is
                          `x > mean` on the fp32 values: the sign of fl(fl(x - mean) * rstd) is exact.
 3. NaN in every input column between `C` and `ld`, the images in the middle of NaN-filled buffers; outputs inside sentinel-filled
    buffers whose pad columns and whose 64 elements past the last row must keep the sentinel; the statistics workspace exactly
    `instnorm_workspace_bytes(B, C)` long with guard bytes behind it, filled with NaN patterns for one run and zeros for the other.
 4. a second run into fresh buffers gives the same bits.

What the shapes reach is restated in Python and asserted: `in_chunks` (256, 204, 146 and 32 chunks), the tile counts of the persistent
stems (1029 tiles: three rounds of 512) and of the weight gradient (1102 tiles on 512 blocks; 4 tiles on 4 blocks).  (32, 74, 516) is
the one norm shape at which `instnorm_partial_kernel` enters its two-row main loop (3 rows per chunk, one row per iteration).

The statistics tensor carries, besides the four channel families, four constant channels of 1e6 .. 4e6: the double sums of their
squares round, E[x^2] - mean^2 comes out at -1e-4 .. -4e-3 instead of 0, and only the clamp keeps `rstd` a number.
`onepass_variance_of_constant` restates the kernels' summation order for such a channel (it predicted exactly the cases that
failed without the clamp on the MI355X) and the test asserts at which shapes the clamp receives less than -eps.  Those four channels
are held to `0 < rstd <= 1 / sqrt(eps)` and left out of the numeric gates of `rstd`.

Found by this module: a NaN in a channel left `rstd` FINITE — `var > 0. ? var : 0.` turned the NaN variance into 0, so `rstd` was
1 / sqrt(eps) = 316.2 next to a NaN `mean` (an `inf` likewise: inf - inf).  The clamp is now `var < 0. ? 0. : var`, the same bits for
every finite input.

`norm_apply_res` against the two `norm_apply` launches it replaces: tests/test_gpu_encoder_norm_fusion.py holds that at 3 x 9x13 x 96
with dense rows; here it is held at every shape below, with padded rows and all eight flag combinations.
`norm_bwd`'s `dx`: ptlflow_amd/train_encoder.py allocates it with `empty_like(x)` — it aliases nothing, and that is what is tested.

Measured on an MI355X, worst over the cases of each test (relative L2 | error as a fraction of the per-element bound).  Records, not
thresholds: the thresholds are `OP_TOL` and a ratio of 1.  A ratio near 1 where K is 1 to 3 is one rounding at its worst (half an ulp),
not a kernel at its limit; the bf16 relative L2 is the rounding to bf16 itself.
  test_stem_valu                            2.2e-7 | 0.040
  test_stem_mfma                            fp32 2.1e-7 | 0.030     bf16 1.9e-3 | 0.987, every value the rounding of the fp32 one
  test_stem2                                fp32 2.9e-7 | 0.030     bf16 1.8e-3 | 0.987, likewise
  test_stem_three_rounds                    fp32 2.3e-7 | 0.034     bf16 1.7e-3 | 0.989, likewise
  test_stem_wgrad                           dw 1.5e-7 | 0.439     db 1.4e-6 | 0.248
  test_stem_wgrad_persistent_walk           dw 4.3e-7 | 0.001     db 4.9e-7 | 0.000
  test_stem_wgrad_fewer_tiles_than_blocks   dw 4.6e-8 | 0.150     db 4.9e-8 | 0.076
  test_instnorm_stats                       fp32 rows: mean 2.4e-11 | 0.999   rstd 4.2e-8 | 0.995     bf16 rows: 2.4e-11 | 0.974   4.2e-8 | 0.995
  test_norm_apply                           3.3e-8 | 0.919
  test_norm_apply_b16                       1.9e-3 | 0.996, every value the rounding of the fp32 twin's
  test_norm_apply_res                       4.3e-8 | 0.543, the bits of the two launches everywhere
  test_norm_bwd                             sum_g 2.8e-8 | 0.499     sum_gxhat 3.6e-7 | 0.505     dx 2.8e-8 | 0.348
Before the clamp was changed, all sixteen cases of test_instnorm_stats failed on "non-finite rstd at [], expected [[0, 0], [0, 1]]"
and its like: `mean` NaN / inf, `rstd` 316.2.
The module's 148 cases take 4 s on an MI355X (pytest's wall time, the float64 references included); the slowest case 0.3 s.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from op_gate import SENTINEL, Rows, flat_out, gates, gates_b16, guarded, record, same_bits, tail_kept

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
F32, B16 = torch.float32, torch.bfloat16
D = 2.0 ** -29                               # 2^-53 in units of 2^-24
EPS = 1e-5
EPS_D = float(torch.tensor(EPS, dtype=F32))  # what the kernels add to the variance: float32(eps), widened


# ---------------------------------------------------------------------------------------------------------------------
# stem forward
# ---------------------------------------------------------------------------------------------------------------------
# (1, 1): one tap inside the image | (2, 2) | (7, 5) | Wo = 65: three column tiles, the last holding one pixel | Ho = 9: one row into
# a second row tile of the MFMA kernels
EDGE = [(2, 1, 1), (2, 2, 2), (2, 7, 5), (2, 16, 130), (2, 17, 129)]
ROUNDS3 = (3, 5481, 5)                      # Ho = 2741, Wo = 3: 343 x 1 tiles per image
FLAGS = [(relu, bias) for relu in (True, False) for bias in (True, False)]


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def mfma_tiles(B, H, W):
    """the tile list of conv_stem_mfma_kernel / conv_stem2_mfma_kernel: 8 x 32 output pixels per tile"""
    Ho, Wo = out_hw(H, W)
    return B * ((Wo + 31) // 32) * ((Ho + 7) // 8)


def row_tiles(B, H, W):
    """the tile list of conv_stem_kernel / conv_stem_wgrad_kernel: 32 pixels of one output row per tile"""
    Ho, Wo = out_hw(H, W)
    return B * Ho * ((Wo + 31) // 32)


@functools.lru_cache(maxsize=None)
def stem_case(B, H, W, cin, cout):
    """fp32 inputs, the float64 convolution without its bias and the sum of the magnitudes of its terms, pixel-major"""
    g = torch.Generator().manual_seed(B * 7919 + H * 131 + W * 17 + cin * 5 + cout)
    x = torch.randn(B, cin, H, W, generator=g)
    wt = torch.randn(cout, cin, 7, 7, generator=g) / math.sqrt(49 * cin)
    bias = torch.randn(cout, generator=g) * 0.3
    pm = lambda t: t.permute(0, 2, 3, 1).reshape(-1, cout)
    return {"x": x, "w": wt.permute(2, 3, 1, 0).reshape(49, cin, cout).contiguous(), "bias": bias, "k": 49 * cin + 1 + 2,
            "pre": pm(F.conv2d(x.double(), wt.double(), None, stride=2, padding=3)),
            "mag": pm(F.conv2d(x.double().abs(), wt.double().abs(), None, stride=2, padding=3))}


def check_stem(what, launch, c, gpu, flags=FLAGS, b16=False):
    """gates 1-4 on `launch(bias, relu, dtype) -> Rows` for every (relu, bias) of `flags`; bf16 rows against their fp32 twin"""
    r32, r16 = [], []
    for relu, with_bias in flags:
        b64 = c["bias"].double() if with_bias else torch.zeros_like(c["bias"]).double()
        ref, mag = c["pre"] + b64, c["mag"] + b64.abs()
        ref = ref.clamp_min(0) if relu else ref
        bias = c["bias"].to(gpu) if with_bias else None
        tag = f"{what} relu={int(relu)} bias={int(with_bias)}"
        out = launch(bias, relu, F32)
        torch.cuda.synchronize()
        out.check_untouched(tag)
        r32.append(gates(tag, out.rows, ref, mag, c["k"]))
        assert torch.equal(launch(bias, relu, F32).flat, out.flat), f"{tag}: a second run gives other bits"
        if b16:
            o16 = launch(bias, relu, B16)
            o16.check_untouched(tag + " bf16")
            r16.append(gates_b16(tag + " bf16", o16.rows, out.rows, ref, mag, c["k"]))
            assert torch.equal(launch(bias, relu, B16).flat, o16.flat), f"{tag} bf16: a second run gives other bits"
    return r32, r16


def stem_launcher(c, gpu, B, H, W, cout):
    Ho, Wo = out_hw(H, W)
    xg, w = guarded(c["x"], gpu), c["w"].to(gpu)

    def launch(bias, relu, dtype):
        out = Rows(B * Ho * Wo, cout, gpu, dtype=dtype)
        torch.ops.pfk.conv_stem(xg, w, bias, out.rows, relu)
        return out
    return launch


@pytest.mark.parametrize("cout", [1, 48, 65, 100, 32, 64])      # the `c += 64` loop and its tail; 32 and 64 forced off the MFMA kernel
@pytest.mark.parametrize("B,H,W", EDGE)
def test_stem_valu(gpu, B, H, W, cout):
    c = stem_case(B, H, W, 3, cout)
    torch.ops.pfk.debug_set_stem_valu(1 if cout in (32, 64) else 0)
    try:
        r32, _ = check_stem(f"stem VALU {(B, H, W)} cout {cout}", stem_launcher(c, gpu, B, H, W, cout), c, gpu)
    finally:
        torch.ops.pfk.debug_set_stem_valu(0)
    record("test_stem_valu", r32)


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("B,H,W", EDGE)
def test_stem_mfma(gpu, B, H, W, cout):
    c = stem_case(B, H, W, 3, cout)
    r32, r16 = check_stem(f"stem MFMA {(B, H, W)} cout {cout}", stem_launcher(c, gpu, B, H, W, cout), c, gpu, b16=True)
    record("test_stem_mfma fp32", r32), record("test_stem_mfma bf16", r16)


SOURCES = ("one", "one_strided", "halves", "two")


def stem2_launcher(source, gpu, B, H, W):
    """one: a dense [B, 3, H, W] | one_strided: the second half of a [B, 6, H, W] tensor whose first half is NaN, read in place |
    halves: both halves of one [B, 6, H, W] tensor in place | two: two separate images"""
    c = stem_case(B, H, W, 3 if source.startswith("one") else 6, 64)
    Ho, Wo = out_hw(H, W)
    w = c["w"].to(gpu)
    if source == "one":
        a, b = guarded(c["x"], gpu), None
    elif source == "one_strided":
        x6 = guarded(torch.cat([torch.full_like(c["x"], NAN), c["x"]], 1), gpu)
        a, b = x6[:, 3:], None
    elif source == "halves":
        x6 = guarded(c["x"], gpu)
        a, b = x6[:, :3], x6[:, 3:]
    else:
        a, b = guarded(c["x"][:, :3].contiguous(), gpu), guarded(c["x"][:, 3:].contiguous(), gpu)

    def launch(bias, relu, dtype):
        out = Rows(B * Ho * Wo, 64, gpu, dtype=dtype)
        torch.ops.pfk.conv_stem2(a, b, w, bias, out.rows, relu)
        return out
    return c, launch


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("B,H,W", EDGE)
def test_stem2(gpu, B, H, W, source):
    """the float64 reference convolves the split input: a value of the other half (NaN for `one_strided`) in the result shows"""
    c, launch = stem2_launcher(source, gpu, B, H, W)
    r32, r16 = check_stem(f"stem2 {source} {(B, H, W)}", launch, c, gpu, b16=True)
    record("test_stem2 fp32", r32), record("test_stem2 bf16", r16)


@pytest.mark.parametrize("kernel", ["mfma64", "mfma32", "stem2_one", "stem2_halves", "stem2_two"])
def test_stem_three_rounds(gpu, kernel):
    """1029 tiles: `conv_stem_mfma_kernel` walks them with 512 blocks, `conv_stem2_mfma_kernel` with 256 workgroups of two groups.
    Either way a third round, in which the patch double buffer returns to buffer 0, and an odd count."""
    B, H, W = ROUNDS3
    tiles = mfma_tiles(B, H, W)
    assert tiles == 1029 and 2 * 512 < tiles < 3 * 512
    if kernel.startswith("mfma"):
        cout = int(kernel[4:])
        c = stem_case(B, H, W, 3, cout)
        launch = stem_launcher(c, gpu, B, H, W, cout)
    else:
        c, launch = stem2_launcher(kernel[6:], gpu, B, H, W)
    r32, r16 = check_stem(f"three rounds {kernel}", launch, c, gpu, flags=[(True, True)], b16=True)
    record("test_stem_three_rounds fp32", r32), record("test_stem_three_rounds bf16", r16)


# ---------------------------------------------------------------------------------------------------------------------
# stem weight gradient
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stem_wgrad_case(B, H, W, cout):
    g = torch.Generator().manual_seed(B * 7919 + H * 131 + W * 17 + cout + 1)
    Ho, Wo = out_hw(H, W)
    x = torch.randn(B, 3, H, W, generator=g)
    dy = torch.randn(B * Ho * Wo, cout, generator=g)
    gy = dy.double().view(B, Ho, Wo, cout).permute(0, 3, 1, 2).contiguous()
    packed = lambda t: t.permute(2, 3, 1, 0).reshape(49, 3, cout)                # the kernel's dw[(ky * 7 + kx) * 3 + ci][c]
    dw = torch.nn.grad.conv2d_weight(x.double(), (cout, 3, 7, 7), gy, stride=2, padding=3)
    dw_mag = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, 3, 7, 7), gy.abs(), stride=2, padding=3)
    return {"x": x, "dy": dy, "dw": packed(dw), "dw_mag": packed(dw_mag), "db": dy.double().sum(0), "db_mag": dy.double().abs().sum(0)}


def check_stem_wgrad(gpu, B, H, W, cout):
    c = stem_wgrad_case(B, H, W, cout)
    Ho, Wo = out_hw(H, W)
    n = B * Ho * Wo
    xg, dy = guarded(c["x"], gpu), Rows(n, cout, gpu, c["dy"])

    def run():
        fw, dw = flat_out((49, 3, cout), gpu)
        fb, db = flat_out((cout,), gpu)
        torch.ops.pfk.conv_stem_wgrad(xg, dy.rows, dw, db)
        return fw, dw, fb, db

    fw, dw, fb, db = run()
    torch.cuda.synchronize()
    what = f"stem wgrad {(B, H, W)} cout {cout}"
    assert tail_kept(fw) and tail_kept(fb), f"{what}: memory past an output was written"
    res = (gates(what + " dw", dw, c["dw"], c["dw_mag"], n + 2), gates(what + " db", db, c["db"], c["db_mag"], n + 2))
    fw2, _, fb2, _ = run()
    assert torch.equal(fw2, fw) and torch.equal(fb2, fb), f"{what}: a second run gives other bits"
    return res


@pytest.mark.parametrize("cout", [1, 32, 48, 64])
@pytest.mark.parametrize("B,H,W", EDGE)
def test_stem_wgrad(gpu, B, H, W, cout):
    """(1, 1): every tap but the centre one lies in the padding — 146 exact zeros per channel"""
    dw, db = check_stem_wgrad(gpu, B, H, W, cout)
    record("test_stem_wgrad dw", [dw]), record("test_stem_wgrad db", [db])


@pytest.mark.parametrize("cout", [64, 48])
def test_stem_wgrad_persistent_walk(gpu, cout):
    """1102 tiles on 512 blocks: blocks 0..77 take three tiles, the others two — the barrier at the loop top, the accumulators
    carried across tiles, `tile += gridDim.x`"""
    B, H, W = 2, 1101, 5
    assert row_tiles(B, H, W) == 1102 and 2 * 512 < row_tiles(B, H, W) < 3 * 512
    dw, db = check_stem_wgrad(gpu, B, H, W, cout)
    record("test_stem_wgrad_persistent_walk dw", [dw]), record("test_stem_wgrad_persistent_walk db", [db])


def test_stem_wgrad_fewer_tiles_than_blocks(gpu):
    """4 tiles: 4 blocks, and the reduce kernel adds 4 partials, not 512"""
    B, H, W = 1, 7, 5
    assert row_tiles(B, H, W) == 4
    dw, db = check_stem_wgrad(gpu, B, H, W, 64)
    record("test_stem_wgrad_fewer_tiles_than_blocks dw", [dw]), record("test_stem_wgrad_fewer_tiles_than_blocks db", [db])


def test_stem_wgrad_refuses_cout_65(gpu):
    x, dy = torch.randn(1, 3, 7, 5, device=gpu), torch.randn(4 * 3, 65, device=gpu)
    _, dw = flat_out((49, 3, 65), gpu)
    _, db = flat_out((65,), gpu)
    with pytest.raises(RuntimeError, match="conv_stem_wgrad"):
        torch.ops.pfk.conv_stem_wgrad(x, dy, dw, db)
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# instance norm: statistics, apply, backward
# ---------------------------------------------------------------------------------------------------------------------
# (B, HW, C):  HW = 1, tpr = 1 | rows = 1, most chunks empty | 2 rows per chunk, 129 chunks used | 204 chunks | 146 chunks, tpr = 129:
# 127 idle threads, one row per iteration | 32 chunks, tpr = 256 | 13 rows per chunk on 16 row slots | the two-row main loop, its tail
# row, a chunk of two rows and seven empty chunks
NORM_SHAPES = [(1, 1, 4), (1, 31, 24), (1, 257, 96), (5, 209, 64), (7, 33, 516), (40, 9, 1024), (2, 3264, 64), (32, 74, 516)]
CHUNKS = {1: 256, 2: 256, 5: 204, 7: 146, 32: 32, 40: 32}
HUGE = torch.tensor([1039342.5625, 3947263.25, 1732050.75, 3702701.5])      # fp32 values; chosen with onepass_variance_of_constant
BELOW_ZERO = {(5, 209, 64), (7, 33, 516), (2, 3264, 64), (32, 74, 516)}      # where one of them comes out below -eps


def in_chunks(B):
    """pfk_encoder.hip's in_chunks: partial-sum chunks per image"""
    return max(32, min(256, 1024 // max(B, 1)))


def onepass_variance_of_constant(v, B, HW, C):
    """E[x^2] - mean^2 of a channel that is `v` everywhere, with the double sums in the order of instnorm_partial_kernel and
    chunk_reduce_kernel (Python floats are doubles; v * v is exact for an fp32 v): what the clamp in front of `rstd` receives"""
    nch, tpr = in_chunks(B), C // 4
    rpi, rows, sq = 256 // tpr, (HW + in_chunks(B) - 1) // in_chunks(B), v * v
    parts = []
    for chunk in range(nch):
        r0, r1 = chunk * rows, min(HW, chunk * rows + rows)
        tot = None
        for rr in range(rpi):                      # a thread: two accumulator sets, the tail row into the first
            acc, r = [[0.0, 0.0], [0.0, 0.0]], r0 + rr
            while r + rpi < r1:
                acc = [[acc[0][0] + v, acc[0][1] + sq], [acc[1][0] + v, acc[1][1] + sq]]
                r += 2 * rpi
            if r < r1:
                acc[0] = [acc[0][0] + v, acc[0][1] + sq]
            mine = [acc[0][0] + acc[1][0], acc[0][1] + acc[1][1]]
            tot = mine if tot is None else [tot[0] + mine[0], tot[1] + mine[1]]
        parts.append(tot)
    fin = []
    for a in (0, 1):                               # sixteen slices of the chunk list, two accumulators each, a fixed tree over them
        red = []
        for sl in range(16):
            s0, s1, k = 0.0, 0.0, sl
            while k + 16 < nch:
                s0, s1, k = s0 + parts[k][a], s1 + parts[k + 16][a], k + 32
            if k < nch:
                s0 += parts[k][a]
            red.append(s0 + s1)
        s = 0.0
        for k in range(0, 16, 4):
            s += (red[k] + red[k + 1]) + (red[k + 2] + red[k + 3])
        fin.append(s)
    m = fin[0] / HW
    return fin[1] / HW - m * m                     # the sums of v are exact: m is v, and m * m is exact, fused or not


def stats64(x64):
    """mean, two-pass biased variance, rstd and E[x^2] of [B, HW, C] float64"""
    mean = x64.mean(1)
    var = ((x64 - mean[:, None]) ** 2).mean(1)
    return mean, var, 1.0 / torch.sqrt(var + EPS_D), (x64 * x64).mean(1)


@functools.lru_cache(maxsize=None)
def norm_case(B, HW, C):
    """x [B, HW, C] with the channel families  c % 4 == 0: 0.7 + 2 N(0, 1) | 1: 300 + N(0, 1) | 2: constant 3.25 | 3: 1e-3 N(0, 1);
    a residual, an incoming gradient 0.8 + N(0, 1), and fp32 statistics: the float64 ones rounded once (a constant channel's mean is
    the constant, and with HW = 1 every mean is its x)"""
    g = torch.Generator().manual_seed(B * 100003 + HW * 101 + C)
    fam = torch.arange(C) % 4
    z = torch.randn(B, HW, C, generator=g)
    x = torch.where(fam == 0, 0.7 + 2 * z, torch.where(fam == 1, 300 + z, torch.where(fam == 2, torch.full_like(z, 3.25), 1e-3 * z)))
    res = torch.randn(B, HW, C, generator=g) * 0.7 + 0.3
    res = torch.where(fam == 1, 300 + res, res)
    dy = 0.8 + torch.randn(B, HW, C, generator=g)
    c = {"x": x, "res": res, "dy": dy, "fam": fam}
    for name, t in (("x", x), ("x16", x.to(B16)), ("res", res)):
        mean, _, rstd, _ = stats64(t.double())
        c[name + "_mean"], c[name + "_rstd"] = mean.float().reshape(-1), rstd.float().reshape(-1)
    assert torch.equal(c["x_mean"].view(B, C)[:, fam == 2], torch.full((B, int((fam == 2).sum())), 3.25))
    return c


def test_chunk_counts():
    assert [in_chunks(B) for B, _, _ in NORM_SHAPES] == [256, 256, 256, 204, 146, 32, 256, 32]
    assert all(in_chunks(B) == n for B, n in CHUNKS.items())


@pytest.mark.parametrize("dtype", [F32, B16], ids=["f32", "b16"])
@pytest.mark.parametrize("B,HW,C", NORM_SHAPES)
def test_instnorm_stats(gpu, B, HW, C, dtype):
    """the four families, four huge constant channels where C >= 24, one NaN and one +inf: exactly their (image, channel) entries of
    `mean` and `rstd` are not finite (a wrong image or channel index shows), every other entry stays inside its bound"""
    ops = torch.ops.pfk
    c = norm_case(B, HW, C)
    x = c["x"].clone()
    huge = torch.zeros(B, C, dtype=torch.bool)
    if C >= 24:
        x[:, :, C - 4:] = HUGE
        huge[:, C - 4:] = True
        if dtype == F32:                           # (bf16 squares have 16 bits: their sums are exact)
            lowest = min(onepass_variance_of_constant(float(v), B, HW, C) for v in HUGE)
            assert (lowest < -EPS) == ((B, HW, C) in BELOW_ZERO), f"the clamp receives {lowest:.3e} at best"
    bad = torch.zeros(B, C, dtype=torch.bool)
    (b_nan, c_nan), (b_inf, c_inf) = (B - 1, 4 % C), (B // 2, 1)
    x[b_nan, HW - 1, c_nan], x[b_inf, HW // 2, c_inf] = NAN, INF
    bad[b_nan, c_nan] = bad[b_inf, c_inf] = True
    x = x.to(dtype)
    rows = Rows(B * HW, C, gpu, x.view(B * HW, C).to(gpu), dtype=dtype)
    need = ops.instnorm_workspace_bytes(B, C)
    assert need == (2 * B * in_chunks(B) * C + 2 * B * C) * 8

    def run(fill):
        ws = torch.full((need + 256,), 0xA5, device=gpu, dtype=torch.uint8)
        ws[:need] = fill
        fm, mean = flat_out((B * C,), gpu)
        fr, rstd = flat_out((B * C,), gpu)
        ops.instnorm_stats(rows.rows, B, HW, EPS, mean, rstd, ws[:need])
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()), "bytes past the workspace were written"
        assert tail_kept(fm) and tail_kept(fr), "memory past mean / rstd was written"
        return fm, mean, fr, rstd

    fm, mean, fr, rstd = run(0xFF)
    what = f"stats {(B, HW, C)} {'bf16' if dtype == B16 else 'fp32'}"
    mean, rstd = mean.cpu().view(B, C), rstd.cpu().view(B, C)
    assert torch.equal(~torch.isfinite(mean), bad), f"{what}: non-finite means at {(~torch.isfinite(mean)).nonzero().tolist()}, expected {bad.nonzero().tolist()}"
    assert torch.equal(~torch.isfinite(rstd), bad), f"{what}: non-finite rstd at {(~torch.isfinite(rstd)).nonzero().tolist()}, expected {bad.nonzero().tolist()}"
    x64 = x.double()
    m64, v64, r64, q64 = stats64(x64)
    absmean = x64.abs().mean(1)
    mean, rstd = mean.masked_fill(bad, 0.0), rstd.masked_fill(bad, 0.0)
    res_m = gates(what + " mean", mean, m64, m64.abs() + (HW + 2) * D * absmean, 1, keep=~bad)
    res_r = gates(what + " rstd", rstd, r64, r64 * (1 + D * (4 + (1.5 * HW + 3) * q64 / (v64 + EPS_D))), 1, keep=~(bad | huge))
    # the constant channels, exactly (on the CPU): mean 3.25 and rstd = float(1 / sqrt(double(float32(eps))))
    const = (c["fam"] == 2)[None].expand(B, C) & ~huge & ~bad
    top = torch.tensor(1.0 / math.sqrt(EPS_D), dtype=torch.float64).float()
    assert bool((mean[const] == 3.25).all()) and bool((rstd[const] == top).all()), f"{what}: a constant channel's statistics are not exact"
    if HW == 1:
        assert bool((rstd[~bad] == top).all()) and torch.equal(mean[~bad], x.float().view(B, C)[~bad]), f"{what}: HW = 1 is not exact"
    # the huge constant channels: the clamp's business
    assert bool(((rstd[huge & ~bad] > 0) & (rstd[huge & ~bad] <= top)).all()), f"{what}: rstd of a huge constant channel outside (0, 1 / sqrt(eps)]"
    fm2, _, fr2, _ = run(0x00)
    assert torch.equal(fm2.view(torch.int32), fm.view(torch.int32)) and torch.equal(fr2.view(torch.int32), fr.view(torch.int32)), \
        f"{what}: a second run on a zeroed workspace gives other bits"
    record(f"test_instnorm_stats {'bf16' if dtype == B16 else 'fp32'} mean", [res_m])
    record(f"test_instnorm_stats {'bf16' if dtype == B16 else 'fp32'} rstd", [res_r])


@pytest.mark.parametrize("C", [1028, 6])
def test_instnorm_stats_refuses(gpu, C):
    ops = torch.ops.pfk
    x = torch.randn(2 * 5, C, device=gpu)
    mean, rstd = torch.empty(2 * C, device=gpu), torch.empty(2 * C, device=gpu)
    ws = torch.empty(ops.instnorm_workspace_bytes(2, 1024), device=gpu, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="instnorm_stats"):
        ops.instnorm_stats(x, 2, 5, EPS, mean, rstd, ws)


def per_pixel(t, B, HW, C):
    """[B*C] statistics as float64 [B*HW, C]"""
    return t.double().view(B, 1, C).expand(B, HW, C).reshape(B * HW, C)


@pytest.mark.parametrize("B,HW,C", NORM_SHAPES)
def test_norm_apply(gpu, B, HW, C):
    """fp32 rows: no residual, an fp32 residual, in place (as the encoders call it).  Row strides C + 4 (x), C + 8 (residual),
    C + 12 (out).  The constant channels and HW = 1 have x == mean: exact zeros in front of the residual."""
    ops = torch.ops.pfk
    c = norm_case(B, HW, C)
    M = B * HW
    x, res = c["x"].view(M, C), c["res"].view(M, C)
    mean, rstd = c["x_mean"].to(gpu), c["x_rstd"].to(gpu)
    y = (x.double() - per_pixel(c["x_mean"], B, HW, C)) * per_pixel(c["x_rstd"], B, HW, C)
    assert not bool(y[:, c["fam"] == 2].any()) and (HW > 1 or not bool(y.any()))
    xr, rr = Rows(M, C, gpu, x.to(gpu)), Rows(M, C, gpu, res.to(gpu), pad=8)
    results = []
    for relu in (True, False):
        y1 = y.clamp_min(0) if relu else y
        for with_res, relu2 in ((False, False), (True, False), (True, True)):
            ref = y1 + res.double() if with_res else y1
            ref = ref.clamp_min(0) if relu2 else ref
            mag = y.abs() + res.double().abs() if with_res else y.abs()
            what = f"norm_apply {(B, HW, C)} relu={int(relu)} res={int(with_res)} relu2={int(relu2)}"

            def run(inplace=False):
                out = Rows(M, C, gpu, x.to(gpu)) if inplace else Rows(M, C, gpu, pad=12)
                ops.norm_apply(xr.rows if not inplace else out.rows, mean, rstd, rr.rows if with_res else None, out.rows, B, HW, relu, relu2)
                return out

            out = run()
            torch.cuda.synchronize()
            out.check_untouched(what)
            results.append(gates(what, out.rows, ref, mag, 3))
            assert same_bits(run().flat, out.flat), f"{what}: a second run gives other bits"
            inp = run(inplace=True)
            assert same_bits(inp.rows.contiguous(), out.rows.contiguous()), f"{what}: in place gives other bits"
            assert bool(torch.isnan(inp.full[:, C:]).all()) and tail_kept(inp.flat), f"{what}: in place wrote outside its rows"
    record("test_norm_apply", results)


@pytest.mark.parametrize("B,HW,C", NORM_SHAPES)
def test_norm_apply_b16(gpu, B, HW, C):
    """the three bf16 instantiations: fp32 rows -> bf16, bf16 rows -> bf16 (also in place), either with a bf16 residual.  The fp32
    twin is `norm_apply` on the widened rows and the widened residual."""
    ops = torch.ops.pfk
    c = norm_case(B, HW, C)
    M = B * HW
    res16 = c["res"].view(M, C).to(B16)
    results = []
    for x_dtype in (F32, B16):
        x = c["x"].view(M, C).to(x_dtype)
        key = "x16" if x_dtype == B16 else "x"
        mean, rstd = c[key + "_mean"].to(gpu), c[key + "_rstd"].to(gpu)
        y = (x.double() - per_pixel(c[key + "_mean"], B, HW, C)) * per_pixel(c[key + "_rstd"], B, HW, C)
        xr, xw = Rows(M, C, gpu, x.to(gpu), dtype=x_dtype), Rows(M, C, gpu, x.float().to(gpu))
        rr, rw = Rows(M, C, gpu, res16.to(gpu), pad=8, dtype=B16), Rows(M, C, gpu, res16.float().to(gpu), pad=8)
        for relu in (True, False):
            y1 = y.clamp_min(0) if relu else y
            for with_res, relu2 in ((False, False), (True, False), (True, True)):
                ref = y1 + res16.double() if with_res else y1
                ref = ref.clamp_min(0) if relu2 else ref
                mag = y.abs() + res16.double().abs() if with_res else y.abs()
                what = f"norm_apply_b16 {(B, HW, C)} x={'bf16' if x_dtype == B16 else 'fp32'} relu={int(relu)} res={int(with_res)} relu2={int(relu2)}"
                twin = Rows(M, C, gpu, pad=12)
                ops.norm_apply(xw.rows, mean, rstd, rw.rows if with_res else None, twin.rows, B, HW, relu, relu2)

                def run(inplace=False):
                    out = Rows(M, C, gpu, x.to(gpu), dtype=B16) if inplace else Rows(M, C, gpu, pad=12, dtype=B16)
                    ops.norm_apply(xr.rows if not inplace else out.rows, mean, rstd, rr.rows if with_res else None, out.rows, B, HW, relu, relu2)
                    return out

                out = run()
                torch.cuda.synchronize()
                out.check_untouched(what)
                gates(what + " (fp32 twin)", twin.rows, ref, mag, 3)
                results.append(gates_b16(what, out.rows, twin.rows, ref, mag, 3))
                assert same_bits(run().flat, out.flat), f"{what}: a second run gives other bits"
                if x_dtype == B16:
                    inp = run(inplace=True)
                    assert same_bits(inp.rows.contiguous(), out.rows.contiguous()), f"{what}: in place gives other bits"
                    assert bool(torch.isnan(inp.full[:, C:]).all()) and tail_kept(inp.flat), f"{what}: in place wrote outside its rows"
    record("test_norm_apply_b16", results)


@pytest.mark.parametrize("B,HW,C", NORM_SHAPES)
def test_norm_apply_res(gpu, B, HW, C):
    """the fused launch: gates 1-4, the bits of the two `norm_apply` launches it replaces, and in place (out is x, as the engine
    calls it), for all eight flag combinations"""
    ops = torch.ops.pfk
    c = norm_case(B, HW, C)
    M = B * HW
    x, res = c["x"].view(M, C), c["res"].view(M, C)
    st = [c[k].to(gpu) for k in ("x_mean", "x_rstd", "res_mean", "res_rstd")]
    y = (x.double() - per_pixel(c["x_mean"], B, HW, C)) * per_pixel(c["x_rstd"], B, HW, C)
    z = (res.double() - per_pixel(c["res_mean"], B, HW, C)) * per_pixel(c["res_rstd"], B, HW, C)
    xr, rr = Rows(M, C, gpu, x.to(gpu)), Rows(M, C, gpu, res.to(gpu), pad=8)
    results = []
    for relu in (True, False):
        for res_relu in (True, False):
            for relu2 in (True, False):
                ref = (y.clamp_min(0) if relu else y) + (z.clamp_min(0) if res_relu else z)
                ref = ref.clamp_min(0) if relu2 else ref
                what = f"norm_apply_res {(B, HW, C)} relu={int(relu)} res_relu={int(res_relu)} relu2={int(relu2)}"

                def run(inplace=False):
                    out = Rows(M, C, gpu, x.to(gpu)) if inplace else Rows(M, C, gpu, pad=12)
                    ops.norm_apply_res(xr.rows if not inplace else out.rows, st[0], st[1], rr.rows, st[2], st[3], res_relu, out.rows, B, HW, relu, relu2)
                    return out

                out = run()
                torch.cuda.synchronize()
                out.check_untouched(what)
                results.append(gates(what, out.rows, ref, y.abs() + z.abs(), 5))
                assert same_bits(run().flat, out.flat), f"{what}: a second run gives other bits"
                resn, two = Rows(M, C, gpu, pad=8), Rows(M, C, gpu, pad=12)
                ops.norm_apply(rr.rows, st[2], st[3], None, resn.rows, B, HW, res_relu, False)
                ops.norm_apply(xr.rows, st[0], st[1], resn.rows, two.rows, B, HW, relu, relu2)
                assert same_bits(two.flat, out.flat), f"{what}: {int((two.rows != out.rows).sum())} values differ from the two norm_apply launches"
                inp = run(inplace=True)
                assert same_bits(inp.rows.contiguous(), out.rows.contiguous()), f"{what}: in place gives other bits"
                assert bool(torch.isnan(inp.full[:, C:]).all()) and tail_kept(inp.flat), f"{what}: in place wrote outside its rows"
    record("test_norm_apply_res", results)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,HW,C", NORM_SHAPES)
def test_norm_bwd(gpu, B, HW, C, relu):
    """g = 0.8 + N(0, 1): dominated by its mean, dx is what is left of a cancellation.  The constant channels have x == mean: under
    relu their mask is closed (`>`, not `>=`), so sum_g, sum_gxhat and dx are exact zeros there.  HW = 1: dx is exactly 0."""
    c = norm_case(B, HW, C)
    M = B * HW
    x, dy = c["x"].view(M, C), c["dy"].view(M, C)
    mean, rstd = c["x_mean"].to(gpu), c["x_rstd"].to(gpu)
    xr, gr = Rows(M, C, gpu, x.to(gpu)), Rows(M, C, gpu, dy.to(gpu), pad=8)

    def run():
        dx = Rows(M, C, gpu, pad=12)                    # train_encoder.py: dx = empty_like(x), no aliasing
        f1, s1 = flat_out((B * C,), gpu)
        f2, s2 = flat_out((B * C,), gpu)
        torch.ops.pfk.norm_bwd(xr.rows, gr.rows, mean, rstd, dx.rows, s1, s2, B, HW, relu)
        return dx, f1, s1, f2, s2

    dx, f1, s1, f2, s2 = run()
    torch.cuda.synchronize()
    what = f"norm_bwd {(B, HW, C)} relu={int(relu)}"
    dx.check_untouched(what)
    assert tail_kept(f1) and tail_kept(f2), f"{what}: memory past sum_g / sum_gxhat was written"
    r64 = per_pixel(c["x_rstd"], B, HW, C)
    xh = (x.double() - per_pixel(c["x_mean"], B, HW, C)) * r64
    g = dy.double()
    if relu:
        g = g * (c["x"] > c["x_mean"].view(B, 1, C)).view(M, C)             # compared on the fp32 values
    img = lambda t: t.view(B, HW, C)
    t1, a1 = img(g).sum(1), img(g).abs().sum(1)                            # [B, C]
    t2, a2 = img(g * xh).sum(1), img(g * xh).abs().sum(1)
    px = lambda t: t[:, None].expand(B, HW, C).reshape(M, C)
    ref = r64 * (g - px(t1) / HW - xh * px(t2) / HW)
    mag = r64 * (g.abs() + px(t1).abs() / HW + xh.abs() * px(a2) / HW) + r64 * (HW + 4) * D / 6 * (px(a1) / HW + xh.abs() * px(a2) / HW)
    res = {"sum_g": gates(what + " sum_g", s1, t1.reshape(-1), a1.reshape(-1), 2),
           "sum_gxhat": gates(what + " sum_gxhat", s2, t2.reshape(-1), a2.reshape(-1), 4),
           "dx": gates(what + " dx", dx.rows, ref, mag, 6)}
    if relu:
        assert not bool(a1[:, c["fam"] == 2].any()), "the reference mask lets a constant channel through"
    if HW == 1:
        assert not bool(dx.rows.any()), f"{what}: HW = 1 must give dx exactly 0"
    dx2, g1, _, g2, _ = run()
    assert torch.equal(dx2.flat, dx.flat) and torch.equal(g1, f1) and torch.equal(g2, f2), f"{what}: a second run gives other bits"
    for k, v in res.items():
        record(f"test_norm_bwd {k}", [v])
