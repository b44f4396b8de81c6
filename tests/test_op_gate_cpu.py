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
