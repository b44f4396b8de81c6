"""The measuring instrument of the kernel tests: comparisons against a float64 reference and guarded buffers.  No domain knowledge —
reference formulas and input builders are in tests/op_refs.py.  tests/test_op_gate_cpu.py runs all of it on the CPU.

The fp64 op gate.  A kernel output is compared with float64 arithmetic on the CPU ON THE KERNEL'S OWN INPUTS:
 1. `rel`: relative L2 <= `OP_TOL`;
 2. `gates`: gate 1 and a per-element bound that needs no measurement.  An element that sums n products must satisfy
        |got - ref| <= (n + 2) * 2^-24 * sum_i |term_i|
    with the sum of magnitudes computed in float64 next to the reference: any correct fp32 summation, in any order, satisfies it.
    Where the magnitudes are 0 the element is an exact zero and is compared with `==`.  `gates_b16` is the same for a bf16 output that
    has an fp32 twin;
 3. `Rows`, `flat_out` / `tail_kept`, `guarded`: NaN where an input must not be read, a sentinel where an output must not be written;
 4. a second run on fresh output buffers gives the same bits (`same_bits`, or `torch.equal` on `.flat`).
`arm` / `ws_after` put the stream-K workspace of pfk_conv2d_f32 under the same kind of guard: partial tiles read before they are
written are NaN, and the flag region must be zero again after every launch.
Blocks and seams are compared with `scale_close` (`BLOCK_TOL` of each tensor's scale); 16-bit training with `within_2x_cpu_autocast`."""
import math

import torch

from ptlflow_amd.packing import round_up  # noqa: F401  (the tests' one `round_up`)

OP_TOL = 5e-6
BLOCK_TOL = 5e-4
AUTOCAST_FACTOR = 2.0
SENTINEL = 12288.0           # 3 * 2^12: exact in bf16, and nothing a gated kernel computes
U = 2.0 ** -24               # unit roundoff of float32
U16 = 2.0 ** -8              # unit roundoff of bfloat16
FLOOR = 1e-35                # absolute floor of a bound whose terms can underflow in fp32
GUARD = 64                   # elements of guard around `guarded`, behind `flat_out` and behind `Rows`


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def pm(x, device=None):
    """NCHW -> contiguous pixel-major rows [B * H * W, C] (C = 0 included), on `device` if one is given"""
    B, C, H, W = x.shape
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()
    return rows if device is None else rows.to(device)


def nchw(rows, B, H, W):
    """pixel-major rows [B * H * W, C] (any row stride) -> NCHW, a view where the strides allow one"""
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def unpm(rows, B, H, W):
    """`nchw` on the CPU"""
    return nchw(rows, B, H, W).cpu()


def leaf(t, dtype):
    """A fresh leaf: `.to()` of the same dtype returns the tensor itself, and requires_grad_() would then mark the shared input."""
    return t.detach().clone().to(dtype).requires_grad_()


# ---------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    """relative L2 error of `a` against `b`, in float64 on the CPU"""
    b = b.detach().double().cpu()
    return float((a.detach().double().cpu() - b).norm() / b.norm().clamp_min(1e-300))


def scale_close(a, b, what, tol=BLOCK_TOL):
    """max |a - b| <= tol * max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = float(b.abs().max()) + 1e-12
    err = float((a - b).abs().max())
    print(f"{what}: max err {err:.3e} of scale {scale:.3e} ({err / scale:.2e})")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def close(a, b, rtol=2e-5, atol=2e-5, dtype=torch.float32):
    """|a - b| <= atol + rtol |b|, both converted to `dtype` first (float32: the comparison is made in the kernels' own precision)"""
    a, b = a.to(dtype).cpu(), b.to(dtype).cpu()
    err, tol = (a - b).abs(), atol + rtol * b.abs()
    assert bool((err <= tol).all()), (f"max err {err.max().item():.3e} (ref max {b.abs().max().item():.3e})" if dtype == torch.float32 else
                                      f"max excess {(err - tol).max().item():.3e}, max err {err.max().item():.3e}")


def close32(got, ref, what):
    """|got - ref| <= 3e-5 + 2e-5 |ref| in float64 (the gate of the GRU epilogues); returns the worst err / limit"""
    err = (got.double().cpu() - ref).abs()
    lim = 3e-5 + 2e-5 * ref.abs()
    ratio = float((err / lim).max())
    assert bool((err <= lim).all()), f"{what}: {int((err > lim).sum())} of {err.numel()} outside 3e-5 + 2e-5|ref|, worst ratio {ratio:.2f}"
    return ratio


def ulp_bf16(v):
    """one bf16 ulp at |v| (normal range; 2^-133 below it)"""
    a = v.abs().double().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def within_ulp(got, ref, floor, what=None):
    """|got - bf16(ref)| <= 1 bf16 ulp of ref + `floor`: the absolute error of the fp32 arithmetic before the rounding, which is
    more than an ulp only for results within ~1e-5 of zero (torch's own fp32 forms miss a plain one-ulp bound there as well).
    `ref` is on the CPU; returns the worst err / limit."""
    err = (got.double().cpu() - ref.to(torch.bfloat16).double()).abs()
    lim = ulp_bf16(ref) + floor
    ratio = float((err / lim).max())
    over = f"{int((err > lim).sum())} of {err.numel()} over"
    assert bool((err <= lim).all()), f"{over}, worst ratio {ratio:.2f}" if what is None else f"{what}: {over} one bf16 ulp, worst ratio {ratio:.2f}"
    return ratio


def bits(t):
    """a float32 / bfloat16 tensor as integers of its width: equality of these is equality of bits (-0.0 != 0.0, NaN == NaN)"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def gates(what, got, ref, mag, k, floor=0.0, keep=None):
    """gates 1 and 2 on one output: `mag` the float64 sum of magnitudes per element, `k` the factor in front of 2^-24 (a number or
    a tensor), `keep` a mask of the elements that take part (default: all).  Returns (relative L2, worst ratio to the bound)."""
    got = got.detach().double().cpu()
    ref, mag = ref.detach().double(), mag.detach().double()
    assert got.shape == ref.shape == mag.shape, f"{what}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(mag.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    if keep is not None:
        got, ref, mag = got[keep], ref[keep], mag[keep]
        k = k[keep] if torch.is_tensor(k) else k
    bound = k * U * mag + floor
    err = (got - ref).abs()
    zero = bound == 0
    assert bool((got[zero] == 0).all()), f"{what}: {int((got[zero] != 0).sum())} elements that are exact zeros by contract are not"
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    r = rel(got, ref)
    print(f"{what}: relL2 {r:.2e}  worst |err| / bound {ratio:.3f}")
    assert r <= OP_TOL, f"{what}: relative L2 {r:.3e}"
    assert ratio <= 1.0, f"{what}: per-element error {ratio:.3f} x the bound"
    return r, ratio


def gates_b16(what, got, twin, ref, mag, k):
    """a bf16 output: the rounding of its fp32 twin bit for bit (in place of gate 1: the twin passed it) and gate 2 with the bf16
    rounding on top of the fp32 bound, k * 2^-24 * mag * (1 + 2^-8) + 2^-8 |ref|.  `twin=None` (a kernel without an fp32 form of the
    same body): gate 2 alone — it implies a relative L2 of at most 2^-8 (1 + eps), so bf16 needs no threshold of its own."""
    assert got.dtype == torch.bfloat16 and (twin is None or twin.dtype == torch.float32)
    if twin is not None:
        same = got == twin.to(torch.bfloat16)
        assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} values are not the bf16 rounding of the fp32 kernel's"
    got, ref, mag = got.detach().double().cpu(), ref.detach().double(), mag.detach().double()
    assert got.shape == ref.shape == mag.shape, f"{what}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(mag.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    bound = k * U * mag * (1 + U16) + U16 * ref.abs()
    err, zero = (got - ref).abs(), bound == 0
    assert bool((got[zero] == 0).all()), f"{what}: elements that are exact zeros by contract are not"
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    r = rel(got, ref)
    print(f"{what}: relL2 {r:.2e}  worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: per-element error {ratio:.3f} x the bound"
    return r, ratio


def record(name, results):
    """one line per output kind for a module docstring: the worst of `results` [(relative L2, ratio to the bound), ...]"""
    if results:
        print(f"RECORD {name}: {max(r for r, _ in results):.1e} | {max(q for _, q in results):.3f}")


def within_2x_cpu_autocast(got, ref64, cpu16, expect=None):
    """16-bit training: for every tensor the L2 error against float64 is at most `AUTOCAST_FACTOR` x the error of the same torch ops
    on the CPU under ``torch.autocast("cpu", bfloat16)``.  got / ref64 / cpu16: {name: tensor}; every name of ref64 must be in `got`
    (nothing skipped).  A tensor whose true value is numerically zero is measured against 1e-3 of the largest scale in the group."""
    assert set(got) == set(ref64) == set(cpu16), (sorted(set(ref64) ^ set(got)), sorted(set(ref64) ^ set(cpu16)))
    if expect is not None:
        assert set(expect) <= set(got), sorted(set(expect) - set(got))
    scale_all = max(float(v.abs().max()) for v in ref64.values())
    rows = []
    for n, ref in ref64.items():
        ref = ref.detach().double().cpu()
        g, c = got[n], cpu16[n]
        assert g is not None and c is not None, f"{n}: no value"
        g, c = g.detach().double().cpu(), c.detach().double().cpu()
        assert g.shape == ref.shape == c.shape, (n, g.shape, ref.shape, c.shape)
        assert bool(torch.isfinite(g).all()), f"{n}: not finite"
        den = max(float(ref.norm()), 1e-3 * scale_all * ref.numel() ** 0.5)
        e_gpu, e_cpu = float((g - ref).norm()) / den, float((c - ref).norm()) / den
        rows.append((e_gpu / max(e_cpu, 1e-30), n, e_gpu, e_cpu))
    rows.sort(reverse=True)
    for r in rows:
        print("   ratio %.2f  %-40s  L2 err %.3e  (CPU autocast %.3e)" % r)
    bad = [r for r in rows if r[2] > AUTOCAST_FACTOR * r[3]]
    assert not bad, "worse than %.0fx CPU autocast: " % AUTOCAST_FACTOR + ", ".join("%s %.2e vs %.2e" % (r[1], r[2], r[3]) for r in bad)


# ---------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
class Rows:
    """[M, C] rows of `dtype` inside a flat buffer with row stride lead + C + pad and 64 elements past the last row; the rows start
    `lead` columns into the wide rows (a channel slice; lead = 1 or 2: a view that is not 16-byte aligned).  Inputs (`values` given):
    NaN in the lead and pad columns, which must not be read (`nan_tail`: behind the last row too); outputs: the sentinel everywhere
    (lead and pad columns and the tail must keep it)."""

    def __init__(self, M, C, device, values=None, pad=4, dtype=torch.float32, lead=0, nan_tail=False):
        self.M, self.C, self.ld, self.lead = M, C, lead + C + pad, lead
        self.flat = torch.full((M * self.ld + GUARD,), SENTINEL, device=device, dtype=dtype)
        self.full = self.flat[:M * self.ld].view(M, self.ld)
        self.rows = self.full[:, lead:lead + C]
        if values is not None:
            assert values.dtype == dtype
            (self.flat if nan_tail else self.full).fill_(float("nan"))
            self.rows.copy_(values)

    def check_untouched(self, what):
        assert bool((self.flat[self.M * self.ld:] == SENTINEL).all()), f"{what}: memory past the last row was written"
        assert bool((self.full[:, self.lead + self.C:] == SENTINEL).all()), f"{what}: pad columns of the output were written"
        assert bool((self.full[:, :self.lead] == SENTINEL).all()), f"{what}: columns in front of the output slice were written"


def flat_out(shape, device, dtype=torch.float32):
    """a contiguous output of `shape` at the start of a sentinel-filled flat buffer with 64 more elements behind it"""
    n = math.prod(shape)
    flat = torch.full((n + GUARD,), SENTINEL, device=device, dtype=dtype)
    return flat, flat[:n].view(shape)


def tail_kept(flat):
    return bool((flat[flat.numel() - GUARD:] == SENTINEL).all())


def guarded(t, device):
    """`t` as a contiguous 16-byte-aligned view in the middle of a NaN-filled flat buffer, >= 64 elements of guard on each side"""
    assert t.dtype in (torch.float32, torch.bfloat16)
    n = t.numel()
    flat = torch.full((n + 2 * GUARD + 8,), float("nan"), dtype=t.dtype, device=device)
    view = flat[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + n:]).all())
    return view


# ---------------------------------------------------------------------------------------------------------------------
# the stream-K workspace of pfk_conv2d_f32 (cfg 9): 768 partial tiles of 64 x 64 floats, then one 64-byte flag slot per block
# ---------------------------------------------------------------------------------------------------------------------
SK_BLOCKS, SK_FLAG_BYTES = 768, 64


def ws_regions(ws):
    """(partials, flags) of a uint8 workspace of `pfk_conv_workspace_bytes()` bytes"""
    flags = ws.numel() - SK_BLOCKS * SK_FLAG_BYTES
    return ws[:flags], ws[flags:]


def arm(ws):
    """0xFF over the partials (a partial read before it is written shows up as NaN); the flags stay zero"""
    ws_regions(ws)[0].fill_(0xFF)


def ws_after(ws, split_expected, what):
    """after a launch on an armed workspace: no fix-up timed out, the flag region is zero again, and partial tiles were written if and
    only if `split_expected` (None: either); returns whether they were"""
    part, flags = ws_regions(ws)
    off = torch.ops.pfk.conv_workspace_fault_offset()
    assert int(ws[off: off + 4].view(torch.int32).item()) == 0, f"{what}: stream-K fix-up timed out"
    assert not bool(flags.any()), f"{what}: the flag region is not zero after the launch"
    touched = bool((part != 0xFF).any())
    if split_expected is not None:
        if split_expected:
            assert touched, f"{what}: no partial tile was written: the launch did not run split stream-K tiles"
        else:
            assert not touched, f"{what}: partial tiles were written: the launch ran stream-K, not a tile grid"
    return touched
