"""tests/op_gate.py held to its own contract on the CPU: every comparison on a result that passes AND on results built to fail, so
that a wrong `keep` mask, a bound multiplied into zero or a guard that is not there cannot make the GPU gates pass silently."""
import math

import pytest
import torch
import torch.nn.functional as F

import op_refs
from op_gate import (FLOOR, GUARD, OP_TOL, SENTINEL, SK_BLOCKS, SK_FLAG_BYTES, U, Rows, arm, close, close32, flat_out, gates, gates_b16,
                     guarded, rel, scale_close, tail_kept, ulp_bf16, within_ulp, ws_regions)

CPU = torch.device("cpu")
F32, B16, F64 = torch.float32, torch.bfloat16, torch.float64
ROWS = 64


def products(n):
    """fp32 factors of ROWS sums of n products; the float64 sums and the sums of magnitudes"""
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(ROWS, n, generator=g), torch.randn(ROWS, n, generator=g)
    exact = a.double() * b.double()
    return a * b, exact.sum(1), exact.abs().sum(1)


def left_to_right(p):
    s = torch.zeros(p.shape[0])
    for j in range(p.shape[1]):
        s = s + p[:, j]
    return s


def pairwise(p):
    if p.shape[1] == 1:
        return p[:, 0]
    h = p.shape[1] // 2
    return pairwise(p[:, :h]) + pairwise(p[:, h:])


def bf16_next(t, steps=1):
    """the bf16 value `steps` ulps further from zero"""
    return (t.view(torch.int16) + steps).view(B16)


# ---------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("order", [left_to_right, pairwise])
def test_gates_pass_on_any_correct_fp32_summation(n, order):
    p, ref, mag = products(n)
    r, ratio = gates(f"{order.__name__} {n}", order(p), ref, mag, n + 2)
    assert r == rel(order(p), ref) and 0.0 <= ratio <= 1.0


def test_gates_fail_on_one_element_outside_its_bound():
    n = 7
    p, ref, mag = products(n)
    got = left_to_right(p).double()
    got[5] = ref[5] + 2 * (n + 2) * U * mag[5]
    with pytest.raises(AssertionError, match=r"per-element error 2\.000 x the bound"):
        gates("s", got, ref, mag, n + 2)
    got[5] = ref[5] + 0.5 * (n + 2) * U * mag[5]
    gates("s", got, ref, mag, n + 2)


def test_gates_fail_on_relative_l2_under_a_loose_bound():
    p, ref, mag = products(7)
    with pytest.raises(AssertionError, match="relative L2 1.0"):
        gates("s", ref * (1 + 1e-5), ref, mag, 1e6)
    assert rel(ref * (1 + 1e-5), ref) > OP_TOL


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_gates_fail_on_a_non_finite_value(bad):
    p, ref, mag = products(7)
    got = left_to_right(p)
    got[0] = bad
    with pytest.raises(AssertionError, match="1 non-finite values"):
        gates("s", got, ref, mag, 9)
    keep = torch.ones(ROWS, dtype=torch.bool)
    keep[0] = False
    with pytest.raises(AssertionError, match="non-finite"):        # finiteness is asked of every element, kept or not
        gates("s", got, ref, mag, 9, keep=keep)


def test_gates_exact_zero_contract():
    p, ref, mag = products(7)
    got, ref, mag = left_to_right(p), ref.clone(), mag.clone()
    ref[3] = mag[3] = 0.0
    got[3] = 1e-45
    assert float(got[3]) != 0.0
    with pytest.raises(AssertionError, match="1 elements that are exact zeros by contract are not"):
        gates("s", got, ref, mag, 9)
    got[3] = -0.0
    gates("s", got, ref, mag, 9)
    # an absolute floor admits an underflow-sized error there, and nothing larger
    got[3] = 1e-38
    with pytest.raises(AssertionError, match="exact zeros"):
        gates("s", got, ref, mag, 9)
    _, ratio = gates("s", got, ref, mag, 9, floor=FLOOR)
    assert ratio <= 1.0
    got[3] = 1e-34
    with pytest.raises(AssertionError, match="x the bound"):
        gates("s", got, ref, mag, 9, floor=FLOOR)


def test_gates_keep_masks_values_and_a_tensor_k_alike():
    n = 7
    p, ref, mag = products(n)
    got = left_to_right(p)
    got[11] += 1.0
    keep = torch.ones(ROWS, dtype=torch.bool)
    keep[11] = False
    k = torch.full((ROWS,), float(n + 2))
    k[11] = 0.0                                    # would make element 11 an "exact zero" if it took part
    for kk in (n + 2, k):
        with pytest.raises(AssertionError):
            gates("s", got, ref, mag, kk)
        r, ratio = gates("s", got, ref, mag, kk, keep=keep)
        assert ratio <= 1.0 and r == rel(got[keep], ref[keep])
    # the mask is applied to k as to the values: a k that is tight only for the excluded element does not leak to its neighbours
    k = torch.full((ROWS,), float(n + 2))
    k[11] = 1e-9
    gates("s", got, ref, mag, k, keep=keep)
    wrong = keep.roll(1)
    with pytest.raises(AssertionError):
        gates("s", got, ref, mag, k, keep=wrong)


def test_gates_refuse_other_shapes():
    p, ref, mag = products(7)
    with pytest.raises(AssertionError, match="shapes"):
        gates("s", left_to_right(p)[:-1], ref, mag, 9)


def test_gates_b16():
    n = 7
    p, ref, mag = products(n)
    twin = left_to_right(p)
    r, ratio = gates_b16("b", twin.to(B16), twin, ref, mag, n + 2)
    assert ratio <= 1.0 and r > OP_TOL               # a bf16 result is far outside the fp32 gate 1: the twin stands in for it
    off = twin.to(B16)
    off[9] = bf16_next(off[9])
    with pytest.raises(AssertionError, match="1 of 64 values are not the bf16 rounding"):
        gates_b16("b", off, twin, ref, mag, n + 2)
    with pytest.raises(AssertionError):              # an fp32 "bf16 output"
        gates_b16("b", twin, twin, ref, mag, n + 2)
    wrong = (ref * 1.5).float()                      # the rounding of a twin that is itself wrong: gate 2 catches it
    with pytest.raises(AssertionError, match="x the bound"):
        gates_b16("b", wrong.to(B16), wrong, ref, mag, n + 2)


# ---------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, B16])
@pytest.mark.parametrize("pad", [4, 8])
def test_rows(dtype, pad):
    M, C = 5, 12
    g = torch.Generator().manual_seed(1)
    values = torch.randn(M, C, generator=g).to(dtype)
    inp = Rows(M, C, CPU, values, pad=pad, dtype=dtype)
    assert inp.rows.dtype == dtype and inp.ld == C + pad and inp.rows.stride() == (C + pad, 1) and torch.equal(inp.rows, values)
    assert bool(torch.isnan(inp.full[:, C:]).all()), "input pads are NaN"
    assert bool((inp.flat[M * inp.ld:] == SENTINEL).all()) and inp.flat.numel() == M * inp.ld + GUARD
    with pytest.raises(AssertionError):
        Rows(M, C, CPU, values.to(F64), pad=pad, dtype=dtype)

    def out():
        r = Rows(M, C, CPU, pad=pad, dtype=dtype)
        assert bool((r.flat == SENTINEL).all()), "an output is the sentinel everywhere"
        return r

    r = out()
    r.rows.copy_(values)
    r.rows[M - 1, C - 1] = 3.0
    r.check_untouched("out")
    for col in (C, C + pad - 1):
        r = out()
        r.full[2, col] = 1.0
        with pytest.raises(AssertionError, match="out: pad columns of the output were written"):
            r.check_untouched("out")
    for at in (M * (C + pad), M * (C + pad) + GUARD - 1):
        r = out()
        r.flat[at] = 1.0
        with pytest.raises(AssertionError, match="out: memory past the last row was written"):
            r.check_untouched("out")


@pytest.mark.parametrize("lead", [1, 2, 4])
def test_rows_as_a_slice_of_wider_rows(lead):
    M, C, pad = 5, 12, 3
    values = torch.randn(M, C, generator=torch.Generator().manual_seed(1))
    inp = Rows(M, C, CPU, values, pad=pad, lead=lead, nan_tail=True)
    assert inp.ld == lead + C + pad and inp.rows.stride() == (inp.ld, 1) and inp.rows.storage_offset() == lead and torch.equal(inp.rows, values)
    assert bool(torch.isnan(inp.full[:, :lead]).all()) and bool(torch.isnan(inp.full[:, lead + C:]).all())
    assert bool(torch.isnan(inp.flat[M * inp.ld:]).all()), "nan_tail: NaN behind the last row"
    r = Rows(M, C, CPU, pad=pad, lead=lead)
    r.rows.copy_(values)
    r.check_untouched("out")
    r.full[3, lead - 1] = 1.0
    with pytest.raises(AssertionError, match="out: columns in front of the output slice were written"):
        r.check_untouched("out")
    r = Rows(M, C, CPU, pad=pad, lead=lead)
    r.full[0, lead + C] = 1.0
    with pytest.raises(AssertionError, match="out: pad columns of the output were written"):
        r.check_untouched("out")
    flat, view = flat_out((3, 4), CPU, B16)
    assert flat.dtype == B16 and view.dtype == B16 and tail_kept(flat)


def test_sentinel_is_a_bf16_value():
    assert float(torch.tensor(SENTINEL).to(B16)) == SENTINEL == 3 * 2.0 ** 12


def test_flat_out_and_tail_kept():
    for shape in ((3, 5), (7,), (2, 3, 4)):
        n = math.prod(shape)
        flat, view = flat_out(shape, CPU)
        assert view.shape == shape and view.is_contiguous() and view.data_ptr() == flat.data_ptr() and flat.numel() == n + GUARD
        assert bool((flat == SENTINEL).all()) and tail_kept(flat)
        view.fill_(1.0)
        assert tail_kept(flat)
        for at in (n, n + GUARD - 1):
            flat, _ = flat_out(shape, CPU)
            flat[at] = 0.0
            assert not tail_kept(flat)


@pytest.mark.parametrize("dtype", [F32, B16])
@pytest.mark.parametrize("shape", [(2, 3, 7, 6), (5,), (1, 9, 9, 3)])
def test_guarded(dtype, shape):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(2)).to(dtype)
    v = guarded(t, CPU)
    assert v.dtype == dtype and torch.equal(v, t) and v.is_contiguous() and v.data_ptr() % 16 == 0
    whole = torch.empty(0, dtype=dtype).set_(v.untyped_storage())
    first, n = v.storage_offset(), v.numel()
    assert first >= 64 and whole.numel() - first - n >= 64
    assert bool(torch.isnan(whole[:first]).all()) and bool(torch.isnan(whole[first + n:]).all()), "the guards are NaN on both sides"
    with pytest.raises(AssertionError):
        guarded(t.double(), CPU)


# ---------------------------------------------------------------------------------------------------------------------
# the other comparisons
# ---------------------------------------------------------------------------------------------------------------------
def test_within_ulp():
    g = torch.Generator().manual_seed(3)
    r16 = (torch.randn(500, generator=g) * 4).to(B16)
    mantissa = r16.view(torch.int16) & 0x7F
    r16 = r16[(mantissa > 0) & (mantissa < 0x7F)]                                # both neighbours in the same binade
    ref = r16.double() + 0.25 * ulp_bf16(r16)                                     # rounds to r16
    assert r16.numel() > 400 and torch.equal(ref.to(B16), r16)
    assert within_ulp(r16, ref, 0.0) == 0.0
    for steps in (1, -1):
        assert within_ulp(bf16_next(r16, steps), ref, 0.0) == 1.0
        with pytest.raises(AssertionError, match=f"{r16.numel()} of {r16.numel()} over"):
            within_ulp(bf16_next(r16, 2 * steps), ref, 0.0)
    one = torch.tensor([1.0], dtype=F64)
    assert float(ulp_bf16(one)) == 2.0 ** -7
    assert within_ulp(bf16_next(one.to(B16)), one, 0.0, "z") == 1.0
    with pytest.raises(AssertionError, match="z: 1 of 1 over one bf16 ulp, worst ratio 2.00"):
        within_ulp(bf16_next(one.to(B16), 2), one, 0.0, "z")
    with pytest.raises(AssertionError, match="^1 of 1 over, worst ratio 2.00"):
        within_ulp(bf16_next(one.to(B16), 2), one, 0.0)
    # near zero the floor is the limit: 1e-6 against 0 is ~130 ulps of 1e-6
    tiny, zero = torch.tensor([1e-6], dtype=F64), torch.zeros(1, dtype=B16)
    with pytest.raises(AssertionError):
        within_ulp(zero, tiny, 0.0)
    assert within_ulp(zero, tiny, 2.0 ** -16) < 1.0
    with pytest.raises(AssertionError):
        within_ulp(zero, tiny * 100, 2.0 ** -16)


def test_close_at_the_limit():
    ref = torch.tensor([1.0, -2.0])                                               # limits 0.5 + 0.25 |ref| = 0.75, 1.0: exact in fp32
    at = torch.tensor([1.75, -3.0])
    close(at, ref, rtol=0.25, atol=0.5)
    close(2 * ref - at, ref, rtol=0.25, atol=0.5)
    for i in range(2):
        above = at.clone()
        above[i] = torch.nextafter(at[i], at[i] * 2)
        with pytest.raises(AssertionError, match="max err"):
            close(above, ref, rtol=0.25, atol=0.5)
    # float32 is the default; float64 sees an excess that the float32 conversion rounds away
    above = at.double() + torch.tensor([2.0 ** -40, 0.0], dtype=F64)
    close(above, ref, rtol=0.25, atol=0.5)
    with pytest.raises(AssertionError, match="max excess"):
        close(above, ref, rtol=0.25, atol=0.5, dtype=F64)
    close(at.double(), ref, rtol=0.25, atol=0.5, dtype=F64)
    with pytest.raises(AssertionError):
        close(torch.tensor([1.0 + 5e-5]), torch.tensor([1.0]))                    # the defaults: 2e-5 + 2e-5 |ref|


def test_close32_at_the_limit():
    ref = torch.tensor([0.0, 1.0, -3.0], dtype=F64)
    lim = 3e-5 + 2e-5 * ref.abs()
    at = ref + lim * torch.tensor([1.0, 0.5, -0.5], dtype=F64)                  # 0 + 3e-5 is exact; the others are well inside
    assert close32(at, ref, "h") == 1.0
    assert close32(ref.float(), ref, "h") == 0.0
    above = at.clone()
    above[0] = torch.nextafter(at[0], torch.tensor(1.0, dtype=F64))
    with pytest.raises(AssertionError, match=r"h: 1 of 3 outside 3e-5 \+ 2e-5\|ref\|"):
        close32(above, ref, "h")


def test_rel():
    x = torch.randn(6, 5, generator=torch.Generator().manual_seed(4))
    assert rel(x, x.clone()) == 0.0 and rel(x.to(B16), x.to(B16).double()) == 0.0
    z = torch.zeros(6, 5)
    assert rel(z, z) == 0.0 and math.isfinite(rel(x, z)) and rel(x, z) > 1e300
    assert rel(2 * x, x) == pytest.approx(1.0, rel=1e-12) and rel(x.double() * (1 + 1e-6), x) == pytest.approx(1e-6, rel=1e-6)


def test_scale_close_at_the_limit():
    ref = torch.tensor([1.0, -4.0], dtype=F64)                                   # scale 4 (+ 1e-12): the limit at tol 0.25 is 1 + 2.5e-13
    scale_close(ref + torch.tensor([1.0, 0.0], dtype=F64), ref, "t", tol=0.25)
    scale_close(ref.float(), ref, "t", tol=0.0)
    with pytest.raises(AssertionError, match="t: max err 1.000e\\+00 vs scale 4.000e\\+00"):
        scale_close(ref + torch.tensor([1.0 + 1e-9, 0.0], dtype=F64), ref, "t", tol=0.25)
    with pytest.raises(AssertionError):
        scale_close(ref * (1 + 1e-3), ref, "t")                                   # the default: BLOCK_TOL = 5e-4 of the scale
    scale_close(ref * (1 + 4e-4), ref, "t")


# ---------------------------------------------------------------------------------------------------------------------
# the LINEAR and volume references of tests/op_refs.py
# ---------------------------------------------------------------------------------------------------------------------
def test_gates_b16_without_a_twin():
    n = 7
    p, ref, mag = products(n)
    got = left_to_right(p).to(B16)
    r, ratio = gates_b16("b", got, None, ref, mag, n + 2)
    assert ratio <= 1.0 and r <= 2.0 ** -8 * (1 + 1e-3)
    off = got.clone()
    off[9] = bf16_next(off[9], 2)                    # two bf16 ulps off: outside half an ulp + the fp32 bound
    with pytest.raises(AssertionError, match="x the bound"):
        gates_b16("b", off, None, ref, mag, n + 2)
    with pytest.raises(AssertionError):
        gates_b16("b", got.float(), None, ref, mag, n + 2)
    with pytest.raises(AssertionError, match="shapes"):
        gates_b16("b", got[:-1], None, ref, mag, n + 2)


def test_ws_regions_and_arm():
    ws = torch.zeros(SK_BLOCKS * (64 * 64 * 4 + SK_FLAG_BYTES), dtype=torch.uint8)     # pfk_gemm.hip SK_WS_BYTES
    part, flags = ws_regions(ws)
    assert part.numel() == SK_BLOCKS * 64 * 64 * 4 and flags.numel() == SK_BLOCKS * SK_FLAG_BYTES
    arm(ws)
    assert bool((part == 0xFF).all()) and not bool(flags.any())
    assert bool(torch.isnan(part.view(F32)).all()), "an armed partial reads as NaN"


def linear_restated(c):
    """`linear_case`'s formula once more, independently: explicit loops over sources, taps and output pixels in float64"""
    (B, H, W), (Bo, Ho, Wo), (kh, kw), s = c["grid"], c["out_grid"], c["k"], c["stride"]
    out = torch.zeros(c["M"], c["cout"], dtype=F64)
    w64, first = c["w"].double(), 0
    for x, real in zip(c["xs"], c["reals"]):
        img = x[:, :real].double().reshape(B, H, W, real)
        for ky in range(kh):
            for kx in range(kw):
                wt = w64[:, first:first + real, ky, kx]                              # [cout, real]
                for b in range(B):
                    for yo in range(Ho):
                        for xo in range(Wo):
                            y, xx = yo * s + ky - kh // 2, xo * s + kx - kw // 2
                            if 0 <= y < H and 0 <= xx < W:
                                out[(b * Ho + yo) * Wo + xo] += wt @ img[b, y, xx]
        first += real
    if c["bias"] is not None:
        out = out + c["bias"].double()
    out = torch.where(out < 0, torch.zeros_like(out), out) if c["act"] == "relu" else out
    out = out * c["scale"]
    if c["residual"] is not None:
        out = c["residual"].double() + out
    return torch.where(out < 0, torch.zeros_like(out), out) if c["relu2"] else out


def test_linear_case_equals_its_restatement(monkeypatch):
    """(a) a tiny shape with stride 2, two sources (one with pad channels), a residual, a scale and relu2"""
    monkeypatch.setitem(op_refs.LINEAR_CASES, "tiny_s2", ((2, 5, 6), (3, 3), 2, [(8, 8), (6, 8)], 12, "relu", 0.37, True, True, True))
    c = op_refs.linear_case("tiny_s2")
    assert c["out_grid"] == (2, 3, 3) and c["M"] == 18 and c["K"] == 9 * 14 + 1 + 4 and c["steps"] == 18
    assert c["packed"].shape == (12, 9 * 64) and c["scale"] == float(torch.tensor(0.37, dtype=F32))
    want = linear_restated(c)
    assert float((c["ref"] - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert bool((c["ref"] == 0).any()) and bool((c["mag"] > 0).all())
    # the pad channels of the second source take no part
    assert bool((c["packed"].view(12, 2, 9, 32)[:, 1, :, 6:] == 0).all())


@pytest.mark.parametrize("name", list(op_refs.LINEAR_CASES))
def test_torch_fp32_passes_the_linear_gates(name):
    """(b) the reference alone stays inside the gates: torch's fp32 CPU convolution of the same op"""
    c = op_refs.linear_case(name)
    got = op_refs.linear_torch32(c)
    if c["act"] == "gelu":
        assert rel(got, c["ref"]) <= OP_TOL
    else:
        gates(name, got, c["ref"], c["mag"], c["K"])


@pytest.mark.parametrize("case", op_refs.VOLUMES_F32 + op_refs.VOLUMES_B16, ids=str)
def test_torch_fp32_passes_the_volume_gates(case):
    b16 = case in op_refs.VOLUMES_B16
    c = op_refs.volume_case(*case, B16 if b16 else F32)
    got = op_refs.volume_torch32(c)
    if b16:
        gates_b16(str(case), got, None, c["ref"], c["mag"], c["K"])
    else:
        gates(str(case), got, c["ref"], c["mag"], c["K"])


def fails(what, got, c, b16=False):
    with pytest.raises(AssertionError, match="x the bound|relative L2"):
        (gates_b16(what, got, None, c["ref"], c["mag"], c["K"]) if b16 else gates(what, got, c["ref"], c["mag"], c["K"]))


def test_linear_mutations_fail_a_gate():
    """(c) each of these is a correct fp32 output with one thing wrong"""
    c = op_refs.linear_case("res_block")
    good = op_refs.linear_torch32(c)
    gates("res_block", good, c["ref"], c["mag"], c["K"])
    B, H, W = c["grid"]
    # one tap (ky, kx) = (1, 0) dropped at the border pixel (1, 5, W - 1) — the residual keeps the output away from relu2's zero
    p = (1 * H + 5) * W + (W - 1)
    tap = c["w"][:, :, 1, 0] @ c["xs"][0][p - 1]
    pre32 = F.relu(c["pre"].float()[p])
    got = good.clone()
    got[p] = F.relu(c["residual"][p] + F.relu(c["pre"].float()[p] - tap))
    assert not torch.equal(got[p], F.relu(c["residual"][p] + pre32))
    fails("tap dropped", got, c)
    # relu2 omitted
    fails("relu2 omitted", c["residual"] + F.relu(c["pre"].float()), c)
    # one output row of image 1 taken from image 0
    got = good.clone()
    got[H * W + 3 * W: H * W + 4 * W] = good[3 * W: 4 * W]
    fails("row of the other image", got, c)
    # the residual added before the scale
    c = op_refs.linear_case("res_scaled")
    gates("res_scaled", op_refs.linear_torch32(c), c["ref"], c["mag"], c["K"])
    fails("residual before the scale", (c["residual"] + F.relu(c["pre"].float())) * c["scale"], c)


def test_volume_mutations_fail_a_gate():
    # batch 1 written with stride N1 * N2 - 1
    for case, dt in (((2, 117, 130, 64), F32), ((2, 130, 117, 40), B16)):
        c = op_refs.volume_case(*case, dt)
        good = op_refs.volume_torch32(c)
        n = case[1] * case[2]
        flat = torch.zeros(2 * n, dtype=dt)
        flat[:n] = good[0].reshape(-1)
        flat[n - 1: 2 * n - 1] = good[1].reshape(-1)
        flat[n - 1] = good[0].reshape(-1)[-1]          # (the last element of batch 0 written after batch 1's first)
        fails("batch stride", flat.view(good.shape), c, dt == B16)
    # the last partial K chunk dropped: 36 = 32 + 4 channels of the fp32 kernel, 72 = 64 + 8 of the bf16 one
    c = op_refs.volume_case(2, 150, 140, 36, F32)
    fails("partial chunk", op_refs.volume_torch32(c, 32), c)
    c = op_refs.volume_case(1, 257, 264, 72, B16)
    fails("partial chunk bf16", op_refs.volume_torch32(c, 64), c, True)


# ---------------------------------------------------------------------------------------------------------------------
# the refinement loop's small direct kernels (tests/test_gpu_loop_kernels_gate.py): each reference against an independent restatement,
# torch's fp32 arithmetic inside the gates (the bounds are conditions, not measurements), and fp32 results with one thing wrong outside
# ---------------------------------------------------------------------------------------------------------------------
def same64(got, want, what):
    assert got.shape == want.shape, what
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-30), what


def tall(x):
    """[B, C, H, W] as ONE image of B H rows: what a kernel sees that walks from an image into its neighbour instead of padding"""
    B, C, H, W = x.shape
    return x.permute(1, 0, 2, 3).reshape(1, C, B * H, W)


def untall(x, B):
    _, C, BH, W = x.shape
    return x.view(C, B, BH // B, W).permute(1, 0, 2, 3)


CIN2_CPU = [(g, k, cout) for g in op_refs.CIN2_GRIDS for k, cout in ((3, 130), (5, 1), (7, 64), (1, 5), (9, 5))] + \
           [((1, 5, 33), 7, 128), ((2, 5, 4163), 7, 64)]


@pytest.mark.parametrize("grid,k,cout", CIN2_CPU, ids=str)
def test_cin2_reference_and_torch_fp32(grid, k, cout):
    c = op_refs.cin2_case(*grid, k, cout)
    assert c["packed"].shape == (k * k, 2, cout) and c["K"] == 2 * k * k + 2 and not bool(c["nan"].any())
    want = op_refs._rows_of(F.relu(F.conv2d(c["flow"].double(), c["w"].double(), c["bias"].double(), padding=k // 2)))
    same64(c["ref"], want, "cin2 reference")
    assert bool((c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all())
    gates(f"cin2 {grid} k{k} cout{cout}", op_refs.cin2_torch32(c), c["ref"], c["mag"], c["K"])


def test_cin2_nan_reaches_its_window_only():
    B, H, W, k = 2, 9, 33, 7
    c = op_refs.cin2_case(B, H, W, k, 64, nan_at=(2, 31))
    nan = c["nan"].view(B, H, W, 64)
    assert torch.equal(torch.isnan(c["ref"]), c["nan"]) and torch.equal(torch.isnan(c["mag"]), c["nan"])
    assert not bool(nan[0].any()) and bool(nan[1, :6, 28:33].all()) and int(nan[..., 0].sum()) == 6 * 5
    clean = op_refs.cin2_case(B, H, W, k, 64)
    assert torch.equal(c["ref"][~c["nan"]], clean["ref"][~c["nan"]])


def test_cin2_mutations_fail_a_gate():
    c = op_refs.cin2_case(2, 3, 21, 7, 64)
    gates("cin2", op_refs.cin2_torch32(c), c["ref"], c["mag"], c["K"])
    with pytest.raises(AssertionError, match="x the bound|relative L2"):
        gates("x / y weight planes swapped", op_refs.cin2_torch32(c, w=c["w"][:, [1, 0]]), c["ref"], c["mag"], c["K"])
    wrapped = untall(F.relu(F.conv2d(tall(c["flow"]), c["w"], c["bias"], padding=3)), 2)
    with pytest.raises(AssertionError, match="x the bound|relative L2"):
        gates("wraps into the neighbouring image", op_refs._rows_of(wrapped), c["ref"], c["mag"], c["K"])


FLOW_DELTA_CPU = [(g, cin, F32) for g in op_refs.FLOW_DELTA_GRIDS4 for cin in (4, 36, 128, 260, 512)] + \
                 [(g, cin, F32) for g in op_refs.FLOW_DELTA_GRIDS8 for cin in (8, 260)] + [((2, 2, 5), 260, B16), ((4, 1024, 5), 8, B16)]


@pytest.mark.parametrize("grid,cin,dtype", FLOW_DELTA_CPU, ids=str)
def test_flow_delta_reference_and_torch_fp32(grid, cin, dtype):
    c = op_refs.flow_delta_case(*grid, cin, dtype)
    B, H, W = grid
    assert c["x"].dtype == dtype and c["packed"].shape == (9, 2, cin) and c["K"] == 9 * cin + 2
    want = F.conv2d(op_refs._images_of(c["x"].double(), B, H, W), c["w"].double(), c["bias"].double(), padding=1)
    same64(c["ref"], want, "flow_delta reference")
    gates(f"flow_delta {grid} cin{cin}", op_refs.flow_delta_torch32(c), c["ref"], c["mag"], c["K"])


def test_flow_delta_nan_corners_reach_their_neighbours_only():
    for grid in op_refs.FLOW_DELTA_GRIDS4[:2]:
        B, H, W = grid
        c = op_refs.flow_delta_case(*grid, 36, F32, nan_corners=True)
        assert torch.equal(torch.isnan(c["ref"]), c["nan"]) and not bool(c["nan"][0].any())
        want = torch.zeros(H, W, dtype=torch.bool)
        for y in range(H):
            for x in range(W):
                want[y, x] = min(y, H - 1 - y) <= 1 and min(x, W - 1 - x) <= 1
        assert torch.equal(c["nan"][1, 0], want) and torch.equal(c["nan"][1, 1], want)


def test_flow_delta_mutations_fail_a_gate():
    c = op_refs.flow_delta_case(2, 2, 5, 260)
    gates("flow_delta", op_refs.flow_delta_torch32(c), c["ref"], c["mag"], c["K"])
    with pytest.raises(AssertionError, match="x the bound|relative L2"):
        gates("channels >= 256 dropped", op_refs.flow_delta_torch32(c, c["x"][:, :256]), c["ref"], c["mag"], c["K"])
    # the row above y = 0 of image b > 0 read from image b - 1's last row (zeros above image 0)
    x = op_refs._images_of(c["x"], 2, 2, 5)
    xp = F.pad(x, (1, 1, 1, 1))
    xp[1:, :, 0, 1:-1] = x[:-1, :, -1, :]
    got = F.conv2d(xp, c["w"], c["bias"])
    assert torch.equal(got[0], op_refs.flow_delta_torch32(c)[0])
    with pytest.raises(AssertionError, match="x the bound|relative L2"):
        gates("image b - 1's last row above y = 0", got, c["ref"], c["mag"], c["K"])


def up_restated(flow, mask, info, dtype, tap=lambda dy, dx: 3 * dy + dx, swap_s=False, flow_factor=8.0, info_factor=1.0, sub_max=True):
    """pfk_upsample.h operation by operation in `dtype`: max in tap order, exp(m - max), the sum in tap order, one reciprocal, e * inv;
    then sum_k w_k v_k in tap order, a multiply and an add.  The keyword arguments are the mutations."""
    B, _, H, W = flow.shape
    m = mask.to(dtype).view(B, 9, 8, 8, H, W)
    if swap_s:
        m = m.transpose(2, 3)
    e = torch.exp(m - m.amax(1, keepdim=True)) if sub_max else torch.exp(m)
    s = e[:, 0]
    for k in range(1, 9):
        s = s + e[:, k]
    w = e * (1.0 / s)[:, None]
    v = torch.cat([flow_factor * flow.to(dtype), info_factor * info.to(dtype)], 1)
    vp = F.pad(v, (1, 1, 1, 1))
    out = torch.zeros(B, v.shape[1], 8, 8, H, W, dtype=dtype)
    for dy in range(3):
        for dx in range(3):
            out = out + w[:, tap(dy, dx)][:, None] * vp[:, :, dy:dy + H, dx:dx + W][:, :, None, None]
    return out.permute(0, 1, 4, 2, 5, 3).reshape(B, v.shape[1], 8 * H, 8 * W)


@pytest.mark.parametrize("scale", op_refs.UP_SCALES)
@pytest.mark.parametrize("grid", op_refs.UP_GRIDS, ids=str)
@pytest.mark.parametrize("b16", [False, True])
def test_convex_forward_reference_and_fp32(grid, scale, b16):
    c = op_refs.convex_fwd_case(*grid, scale, b16)
    assert c["mask"].dtype == (B16 if b16 else F32) and c["ref"].shape == (grid[0], 10, 8 * grid[1], 8 * grid[2])
    same64(c["ref"], up_restated(c["flow"], c["mask"], c["info"], F64), "convex forward reference")
    assert float(c["k"].min()) >= 30.0 and bool((c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all())
    what = f"convex forward {grid} x{scale}"
    _, q = gates(what + " (the kernel's order)", up_restated(c["flow"], c["mask"], c["info"], F32), c["ref"], c["mag"], c["k"], floor=FLOOR)
    assert q <= 0.5
    from oracle import raft_oracle as O
    _, q = gates(what + " (torch.softmax)", O.convex_upsample(c["flow"], c["mask"].float()), c["ref"][:, :2], c["mag"][:, :2], c["k"][:, :2], floor=FLOOR)
    assert q <= 0.5


def test_convex_forward_needs_the_floor():
    """at saturated logits a weight underflows in fp32 and its term is lost whole: only the absolute floor admits that"""
    c = op_refs.convex_fwd_case(2, 5, 7, 60.0)
    with pytest.raises(AssertionError, match="x the bound"):
        gates("no floor", up_restated(c["flow"], c["mask"], c["info"], F32), c["ref"], c["mag"], c["k"])


def test_convex_forward_zero_image_and_infinite_logits():
    c = op_refs.convex_fwd_case(2, 5, 7, 1.0, False, 0)
    assert bool((c["ref"][0, :2] == 0).all()) and bool((c["mag"][0, :2] == 0).all()) and bool((c["mag"][1] > 0).all()) and bool((c["mag"][0, 2:] > 0).all())
    flow, info = c["flow"], c["info"]
    for keep in (0, 4, 8):
        m = torch.full((2, 9, 64, 5, 7), float("-inf"))
        m[:, keep] = c["mask"].view(2, 9, 64, 5, 7)[:, keep]
        ref, mag, k = op_refs.convex_fwd64(flow, m.view(2, 576, 5, 7), info)
        dy, dx = keep // 3 - 1, keep % 3 - 1
        nb = F.pad(torch.cat([8 * flow, info], 1), (1, 1, 1, 1))[:, :, 1 + dy:6 + dy, 1 + dx:8 + dx]
        assert torch.equal(ref, nb.double().repeat_interleave(8, 2).repeat_interleave(8, 3)), keep
        assert bool((k == 30).all()) and torch.equal(mag, ref.abs())


def test_convex_forward_mutations_fail_a_gate():
    c = op_refs.convex_fwd_case(2, 5, 7, 1.0)
    args = (c["flow"], c["mask"], c["info"], F32)
    gates("convex forward", up_restated(*args), c["ref"], c["mag"], c["k"], floor=FLOOR)
    for what, kw in (("taps transposed", dict(tap=lambda dy, dx: 3 * dx + dy)), ("sy and sx swapped", dict(swap_s=True)),
                     ("factor 8 on the info", dict(info_factor=8.0)), ("no factor 8 on the flow", dict(flow_factor=1.0))):
        with pytest.raises(AssertionError, match="x the bound|relative L2"):
            gates(what, up_restated(*args, **kw), c["ref"], c["mag"], c["k"], floor=FLOOR)
    # without the max subtraction expf overflows at scale 60: inf / inf
    c = op_refs.convex_fwd_case(2, 5, 7, 60.0)
    gates("convex forward x60", up_restated(c["flow"], c["mask"], c["info"], F32), c["ref"], c["mag"], c["k"], floor=FLOOR)
    with pytest.raises(AssertionError, match="non-finite|x the bound|relative L2"):
        gates("no max subtraction", up_restated(c["flow"], c["mask"], c["info"], F32, sub_max=False), c["ref"], c["mag"], c["k"], floor=FLOOR)


def upflow8_restated(c, clamp=True):
    """the kernel thread by thread in fp32, reading c1 - c0 from a flat array with NaN behind its last element (`clamp=False`: i1 =
    i0 + 1 whatever i0: the read past a row or past the array)"""
    B, H, W = c["grid"]
    flat = torch.cat([(c["c1"] - c["c0"]).reshape(-1), torch.full((W + 2,), float("nan"))])
    y0, y1, ly = op_refs.upflow8_axis(H)
    x0, x1, lx = op_refs.upflow8_axis(W)
    if not clamp:
        y1, x1 = y0 + 1, x0 + 1
    ly1, lx1 = ly[:, None], lx[None, :]
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1
    out = torch.empty(B * 2, 8 * H, 8 * W)
    for p in range(B * 2):
        at = lambda yi, xi: flat[p * H * W + yi[:, None] * W + xi[None, :]]        # noqa: E731
        out[p] = 8.0 * (ly0 * (lx0 * at(y0, x0) + lx1 * at(y0, x1)) + ly1 * (lx0 * at(y1, x0) + lx1 * at(y1, x1)))
    return out.view(B, 2, 8 * H, 8 * W)


@pytest.mark.parametrize("grid", op_refs.UPFLOW_GRIDS, ids=str)
def test_upflow8_reference_and_torch_fp32(grid):
    c = op_refs.upflow8_case(*grid)
    B, H, W = grid
    # the reference pixel by pixel
    v = c["c1"].double() - c["c0"].double()
    (y0, y1, ly), (x0, x1, lx) = op_refs.upflow8_axis(H), op_refs.upflow8_axis(W)
    want = torch.empty(B, 2, 8 * H, 8 * W, dtype=F64)
    for yo in range(8 * H):
        for xo in range(8 * W):
            a, b = float(ly[yo]), float(lx[xo])
            want[:, :, yo, xo] = 8 * ((1 - a) * ((1 - b) * v[:, :, y0[yo], x0[xo]] + b * v[:, :, y0[yo], x1[xo]]) +
                                      a * ((1 - b) * v[:, :, y1[yo], x0[xo]] + b * v[:, :, y1[yo], x1[xo]]))
    same64(c["ref"], want, "upflow8 reference")
    assert int(y1.max()) == H - 1 and int(x1.max()) == W - 1 and float(ly.min()) >= 0 and float(lx.max()) < 1
    _, q = gates(f"upflow8 {grid} (the kernel's order)", upflow8_restated(c), c["ref"], c["mag"], c["K"])
    assert q <= 0.7
    torch32 = 8 * F.interpolate(c["c1"] - c["c0"], size=(8 * H, 8 * W), mode="bilinear", align_corners=True)
    _, q = gates(f"upflow8 {grid} (F.interpolate)", torch32, c["ref"], c["mag"], c["K"])
    assert q <= 0.7


def test_upflow8_mutations_fail_a_gate():
    c = op_refs.upflow8_case(2, 9, 13)
    wrong = 8 * F.interpolate(c["c1"] - c["c0"], size=(72, 104), mode="bilinear", align_corners=False)
    with pytest.raises(AssertionError, match="x the bound|relative L2"):
        gates("align_corners=False", wrong, c["ref"], c["mag"], c["K"])
    # i1 unclamped: at the last row / column lambda1 is 0 and the product with the element read past the end still is not
    for grid in ((2, 9, 13), (1, 1, 5), (2, 6, 1)):
        c = op_refs.upflow8_case(*grid)
        with pytest.raises(AssertionError, match="non-finite|x the bound|relative L2"):
            gates("i1 unclamped", upflow8_restated(c, clamp=False), c["ref"], c["mag"], c["K"])


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("cols", op_refs.SOFTMAX_COLS)
def test_softmax_rows_reference_and_torch_fp32(cols, scale):
    c = op_refs.softmax_rows_case(cols, scale)
    want = torch.empty(op_refs.SOFTMAX_ROWS, cols, dtype=F64)
    for r in range(op_refs.SOFTMAX_ROWS):
        row = [float(t) for t in c["x"][r]]
        top = max(row)
        e = [math.exp(t - top) for t in row]
        want[r] = torch.tensor([t / math.fsum(e) for t in e], dtype=F64)
    same64(c["ref"], want, "softmax_rows reference")
    if cols >= 3:
        assert int((c["ref"][3] == 0).sum()) == cols - 2 and int(torch.isinf(c["x"]).sum()) == cols - 2
    _, q = gates(f"softmax_rows {cols} x{scale}", torch.softmax(c["x"], 1), c["ref"], c["mag"], c["k"], floor=FLOOR)
    assert q <= 0.3


def test_softmax_rows_mutation_fails_a_gate():
    c = op_refs.softmax_rows_case(140, 1.0)
    wide = F.pad(c["x"], (0, 4))                     # ld = cols + 4, zeros in the pad columns
    with pytest.raises(AssertionError, match="x the bound|relative L2"):
        gates("normalised over ld", torch.softmax(wide, 1)[:, :140], c["ref"], c["mag"], c["k"], floor=FLOOR)
