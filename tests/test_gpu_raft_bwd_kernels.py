"""RAFT's older backward kernels held to the fp64 op gate, kernel by kernel: the fp32 weight gradient (`pfk_conv_wgrad_f32`,
`pfk_conv_wgrad_unpacked_f32`), the correlation volume and lookup backward (`pfk_corr_volume_bwd_f32`, `pfk_corr_lookup_bwd_f32`),
the convex-upsampling backward (`pfk_convex_upsample_bwd_f32`) and the GRU gate kernels (`pfk_gru_gates_*`, `pfk_gru_backward_*`).
Until now they were reached only through `conv_pm`, `CorrBlock` autograd or whole training steps.

Gates on every kernel output (tests/op_gate.py's harness: `gates`, `Rows`, `flat_out`, `SENTINEL`):
 1. relative L2 <= 5e-6 against float64 on the CPU ON THE KERNEL'S OWN fp32 INPUTS;
 2. a per-element bound that needs no measurement.  An element that sums n products must satisfy
        |got - ref| <= (n + 2) * 2^-24 * sum_i |term_i|
    with the sum of magnitudes computed in float64 next to the reference: any correct fp32 summation, in any order, satisfies it
    (n roundings of the running sum and one of each product are <= (n + 1) units of 2^-24 of the magnitudes; the + 2 leaves room for
    a scale factor and an accumulate).  Where the magnitudes are 0 the element is an exact zero and is compared with `==`.  Outputs
    that are short expressions rather than sums (GRU gates, the mask gradient) get a bound of the same form, K * 2^-24 * the
    magnitudes of the expression's terms, with K counted from the expression (written next to each) and an absolute floor of 1e-35
    for fp32 underflow;
 3. NaN in every column of an input between `channels` and `ld`; outputs inside sentinel-filled buffers whose pad columns and whose
    64 floats past the last row must keep the sentinel;
 4. a second run on fresh output buffers gives the same bits.

Lookup backward: the reference is float64 autograd through `oracle.raft_oracle.lookup` on a float64 pyramid with the kernel's own
fp32 coordinates, so the tap positions come out of grid_sample's fp32 round trip — which is part of the operation (the forward is
bit-exact on it) — and everything after them is float64.  A cell receives at most 2 x 2 taps per call; two calls: n = 8.

Planner values in the comments of `WGRAD` were worked out from `pick_cb` / `pick_splits` of ptlflow_amd/csrc/pfk_wgrad.hip.

Measured on an MI355X, worst over the cases of each test (relative L2 | error as a fraction of the per-element bound):
  test_wgrad, test_wgrad_forced_tile_height, test_wgrad_unpacked_entry
                                 packed / dw 4.2e-7 | 0.014 (the single slice; <= 0.003 with slices)     db 9.9e-7 | 0.001
  test_corr_volume_bwd           df1 2.3e-7 | 0.108     df2 4.7e-7 | 0.026
  test_corr_lookup_bwd           every level of every family <= 7.0e-8 | 0.286; the 1-pixel levels exactly 0
  test_convex_upsample_bwd       grad_mask 9.5e-8 | 0.128 (logits x 40: 3.5e-7 | 0.211)     grad_flow 1.1e-7 | 0.001
  test_gru_gate_kernels          z, r, rh, q, h_new <= 4.5e-8 | 0.275     da_q, da_z, da_r, dh <= 5.6e-8 | 0.475
The 1 x 2 and 1 x 39 levels are what made the lookup backward drop the taps whose round-trip coordinate is not finite: their NaN
weights used to reach patch rows / columns 0 and 1, which lie inside the map when the scaled coordinate is 4..5 pixels past the edge.
"""
import functools
import math

import pytest
import torch

from oracle import raft_oracle as O
from op_gate import FLOOR, SENTINEL, Rows, flat_out, gates, tail_kept
from op_refs import convex_case, coords_cases

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
# name: (B, H, W, real channels, buffer channels, kh, kw, cout, with_bias, stride)
WGRAD = {
    # M = 1058: two slices of 544 pixels, the boundary 15 pixels into image 1, a 2-pixel tail K-step; 36 chunks with the bias chunk
    "1x5_two_sources": (2, 23, 23, (36, 146), (36, 148), 1, 5, 132, True, 1),
    # 19 chunks (odd: a dead chunk in the last group under CB = 2, chunks % 4 != 0 under CB = 1); cout 40 / 4: tall tiles mostly masked
    "3x3_cout40": (2, 23, 23, (36,), (36,), 3, 3, 40, True, 1),
    "3x3_cout4": (2, 23, 23, (36,), (36,), 3, 3, 4, True, 1),
    "3x3_three_slices": (3, 23, 23, (36,), (36,), 3, 3, 40, True, 1),                 # M = 1587
    # M = 32769, one tile: 64 slices of 544 pixels, slices 61..63 empty
    "1x1_empty_slices": (1, 99, 331, (4,), (4,), 1, 1, 4, True, 1),
    # M = 288: one slice, written straight to the output (the packed entry gets a NULL workspace)
    "3x3_single_slice": (2, 12, 12, (64,), (64,), 3, 3, 96, False, 1),
    "5x1_three_sources": (2, 23, 23, (36, 62, 4), (36, 64, 4), 5, 1, 64, True, 1),
    "7x7_cin2": (2, 23, 23, (2,), (4,), 7, 7, 64, True, 1),
    "3x3_stride2": (2, 45, 47, (36,), (36,), 3, 3, 40, True, 2),                      # Ho, Wo = 23, 24: M = 1104
    "1x1_stride2": (2, 45, 47, (36,), (36,), 1, 1, 40, True, 2),
}
KNOB_CASES = ("1x5_two_sources", "3x3_cout40", "3x3_cout4")


@functools.lru_cache(maxsize=None)
def wgrad_case(name):
    """fp32 inputs and the float64 weight / bias gradient over the BUFFER channels (the zero channels between `real` and `buffer`
    included), with the sums of magnitudes, in PyTorch's layout; computed once per case"""
    from ptlflow_amd.packing import pack_conv_weight
    B, H, W, reals, bufs, kh, kw, cout, with_bias, sd = WGRAD[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Ho, Wo = (H - 1) // sd + 1, (W - 1) // sd + 1
    M, Mo = B * H * W, B * Ho * Wo
    xs = []
    for r, b in zip(reals, bufs):
        x = torch.randn(M, b, generator=g)
        x[:, r:] = 0.0
        xs.append(x)
    dy = torch.randn(Mo, cout, generator=g)
    x64 = torch.cat([x.double().view(B, H, W, -1).permute(0, 3, 1, 2) for x in xs], 1).contiguous()
    gy64 = dy.double().view(B, Ho, Wo, cout).permute(0, 3, 1, 2).contiguous()
    shape, pad = (cout, sum(bufs), kh, kw), (kh // 2, kw // 2)
    dw = torch.nn.grad.conv2d_weight(x64, shape, gy64, stride=sd, padding=pad)
    dw_mag = torch.nn.grad.conv2d_weight(x64.abs(), shape, gy64.abs(), stride=sd, padding=pad)
    db, db_mag = dy.double().sum(0), dy.double().abs().sum(0)
    buf_segs, real_segs, real_idx, fb, fr = [], [], [], 0, 0
    for r, b in zip(reals, bufs):
        buf_segs.append((fb, b, b))
        real_segs.append((fr, r, b))
        real_idx += list(range(fb, fb + r))
        fb, fr = fb + b, fr + r

    def packed(w, bias):
        p = pack_conv_weight(w, buf_segs)
        if not with_bias:
            return p
        col = torch.zeros(cout, 32, dtype=torch.float64)
        col[:, 0] = bias
        return torch.cat([p, col], 1)

    return {"xs": xs, "dy": dy, "M": M, "Mo": Mo, "packed": packed(dw, db), "packed_mag": packed(dw_mag, db_mag),
            "dw": dw[:, real_idx], "dw_mag": dw_mag[:, real_idx], "db": db, "db_mag": db_mag, "real_segs": real_segs,
            "ktot": sum(kh * kw * ((b + 31) // 32 * 32) for b in bufs)}


class WgradRun:
    """the inputs of one case on the GPU (NaN pads) and the two entries on fresh sentinel-filled outputs"""

    def __init__(self, gpu, name):
        self.gpu, self.c = gpu, wgrad_case(name)
        self.B, self.H, self.W, self.reals, self.bufs, self.kh, self.kw, self.cout, self.with_bias, self.sd = WGRAD[name]
        self.srcs = [Rows(self.c["M"], b, gpu, x) for b, x in zip(self.bufs, self.c["xs"])]
        self.dy = Rows(self.c["Mo"], self.cout, gpu, self.c["dy"])

    def packed(self, with_bias=None):
        with_bias = self.with_bias if with_bias is None else with_bias
        flat, out = flat_out((self.cout, self.c["ktot"] + (32 if with_bias else 0)), self.gpu)
        torch.ops.pfk.conv_wgrad([s.rows for s in self.srcs], self.dy.rows, self.B, self.H, self.W, self.kh, self.kw, out, with_bias, self.sd)
        return flat, out

    def unpacked(self, with_bias=None, cout_real=None, accumulate=False, init=None):
        with_bias = self.with_bias if with_bias is None else with_bias
        cout_real = self.cout if cout_real is None else cout_real
        fw, dw = flat_out((cout_real, sum(self.reals), self.kh, self.kw), self.gpu)
        fb, db = flat_out((cout_real,), self.gpu)
        if init is not None:
            dw.copy_(init[0]), db.copy_(init[1])
        torch.ops.pfk.conv_wgrad_unpacked([s.rows for s in self.srcs], self.dy.rows, self.B, self.H, self.W, self.kh, self.kw, dw,
                                          db if with_bias else None, list(self.reals), self.sd, accumulate)
        return fw, dw, fb, db

    def unpack_on_host(self, pk):
        from ptlflow_amd.train import _Geometry, _unpack_wgrad
        shape = (self.cout, sum(self.reals), self.kh, self.kw)
        return _unpack_wgrad(pk, shape, self.c["real_segs"], _Geometry(self.B, self.H, self.W, self.kh, self.kw, self.sd))


def _check_wgrad(gpu, name, what):
    run = WgradRun(gpu, name)
    c, ktot, n = run.c, run.c["ktot"], run.c["Mo"]
    flat, pk = run.packed()
    fw, dw, fb, db = run.unpacked()
    torch.cuda.synchronize()
    assert tail_kept(flat) and tail_kept(fw) and tail_kept(fb), f"{what}: memory past an output was written"
    # the packed layout: channel-pad columns and the 31 columns after the bias column are exact zeros
    layout = torch.ones(ktot + (32 if run.with_bias else 0), dtype=torch.bool)
    k0 = 0
    for b in run.bufs:
        cpad = (b + 31) // 32 * 32
        layout[k0:k0 + run.kh * run.kw * cpad].view(-1, cpad)[:, :b] = False
        k0 += run.kh * run.kw * cpad
    if run.with_bias:
        layout[ktot] = False
    assert bool((pk.cpu()[:, layout] == 0).all()), f"{what}: pad columns of the packed gradient are not zero"
    res = [gates(f"wgrad {what} packed", pk, c["packed"], c["packed_mag"], n + 2)]
    # the unpacked entry runs the same plan: the same bits
    assert torch.equal(run.unpack_on_host(pk), dw), f"{what}: unpacked entry differs from the packed result unpacked on the host"
    res.append(gates(f"wgrad {what} dw", dw, c["dw"], c["dw_mag"], n + 2))
    if run.with_bias:
        assert torch.equal(pk[:, ktot], db), f"{what}: db differs from the packed bias column"
        res.append(gates(f"wgrad {what} db", db, c["db"], c["db_mag"], n + 2))
    else:
        assert bool((db == SENTINEL).all()), f"{what}: db = None but the bias buffer was written"
    flat2, _ = run.packed()
    fw2, _, fb2, _ = run.unpacked()
    assert torch.equal(flat2, flat) and torch.equal(fw2, fw) and torch.equal(fb2, fb), f"{what}: a second run gives other bits"
    return res


@pytest.mark.parametrize("name", list(WGRAD))
def test_wgrad(gpu, name):
    _check_wgrad(gpu, name, name)


@pytest.mark.parametrize("variant", [1, 2, 4])
@pytest.mark.parametrize("name", KNOB_CASES)
def test_wgrad_forced_tile_height(gpu, name, variant):
    """every tile height on every `cout`, not only the one `pick_cb` selects for it"""
    torch.ops.pfk.debug_set_wgrad(variant)
    try:
        _check_wgrad(gpu, name, f"{name} CB={variant}")
    finally:
        torch.ops.pfk.debug_set_wgrad(0)


def test_wgrad_unpacked_entry(gpu):
    """`accumulate`, `db = None` and `cout_real < cout` of the unpacked entry, on two slices"""
    run = WgradRun(gpu, "3x3_cout40")
    c = run.c
    fw, dw, fb, db = run.unpacked()
    # accumulate onto non-zero dw / db: old + plain, bit for bit
    g = torch.Generator().manual_seed(8)
    old = (torch.randn(dw.shape, generator=g).to(gpu), torch.randn(db.shape, generator=g).to(gpu))
    fwa, dwa, fba, dba = run.unpacked(accumulate=True, init=old)
    torch.cuda.synchronize()
    assert torch.equal(dwa, old[0] + dw) and torch.equal(dba, old[1] + db)
    assert tail_kept(fwa) and tail_kept(fba)
    # db = None: the plan without the bias chunk — the packed entry's bits without a bias column, nothing written to a bias buffer
    fwn, dwn, fbn, dbn = run.unpacked(with_bias=False)
    _, pkn = run.packed(with_bias=False)
    torch.cuda.synchronize()
    assert bool((fbn == SENTINEL).all()), "db = None but the bias buffer was written"
    assert tail_kept(fwn) and torch.equal(run.unpack_on_host(pkn), dwn)
    gates("wgrad db=None dw", dwn, c["dw"], c["dw_mag"], c["Mo"] + 2)
    # cout_real < d->cout: the first rows of the full result, nothing behind them
    fwc, dwc, fbc, dbc = run.unpacked(cout_real=38)
    torch.cuda.synchronize()
    assert torch.equal(dwc, dw[:38]) and torch.equal(dbc, db[:38]) and tail_kept(fwc) and tail_kept(fbc)


# ---------------------------------------------------------------------------------------------------------------------
# correlation volume backward
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def volume_case(B, N1, N2, D):
    g = torch.Generator().manual_seed(N1 + N2 + D)
    ldc, Dpad = (N2 + 3) // 4 * 4, (D + 31) // 32 * 32
    dC = torch.zeros(B, N1, ldc)
    dC[..., :N2] = torch.randn(B, N1, N2, generator=g)
    f1, f2, old = (torch.randn(B, n, D, generator=g) for n in (N1, N2, N1))
    scale = float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32))          # the fp32 value the kernel receives
    c64, a64, b64 = dC[..., :N2].double(), f1.double(), f2.double()
    df1, df1_mag = scale * c64 @ b64, scale * c64.abs() @ b64.abs()
    df2, df2_mag = torch.zeros(B, ldc, Dpad, dtype=torch.float64), torch.zeros(B, ldc, Dpad, dtype=torch.float64)
    df2[:, :N2, :D] = scale * c64.transpose(1, 2) @ a64
    df2_mag[:, :N2, :D] = scale * c64.abs().transpose(1, 2) @ a64.abs()
    return {"dC": dC, "f1": f1, "f2": f2, "old": old, "scale": scale, "df1": df1, "df1_mag": df1_mag, "df2": df2, "df2_mag": df2_mag}


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,N1,N2,D", [(2, 140, 35, 36), (1, 1426, 165, 64)])      # N1 != N2; the second has two pixel slices
def test_corr_volume_bwd(gpu, B, N1, N2, D, accumulate):
    ops = torch.ops.pfk
    c = volume_case(B, N1, N2, D)
    ldc, Dpad = c["dC"].shape[2], c["df2"].shape[2]
    dC, f1 = c["dC"].to(gpu), c["f1"].to(gpu)
    f2 = Rows(B * N2, D, gpu, c["f2"].reshape(B * N2, D))
    f2cm = torch.zeros(B, D, (ldc + 31) // 32 * 32, device=gpu)
    ops.pm_to_cm(f2.rows, f2cm)

    def run():
        flat1, df1 = flat_out((B, N1, D), gpu)
        flat2, df2 = flat_out((B, ldc, Dpad), gpu)
        if accumulate:
            df1.copy_(c["old"])
        ops.corr_volume_bwd(dC, N2, f1, f2cm, c["scale"], df1, accumulate, df2)
        return flat1, df1, flat2, df2

    flat1, df1, flat2, df2 = run()
    torch.cuda.synchronize()
    assert tail_kept(flat1) and tail_kept(flat2), "memory past an output was written"
    assert bool((df2[:, N2:] == 0).all()) and bool((df2[:, :, D:] == 0).all()), "df2 rows >= N2 / columns >= D are not zero"
    ref1 = c["df1"] + c["old"].double() if accumulate else c["df1"]
    mag1 = c["df1_mag"] + c["old"].double().abs() if accumulate else c["df1_mag"]
    what = f"volume_bwd {(B, N1, N2, D)} acc={int(accumulate)}"
    gates(what + " df1", df1, ref1, mag1, N2 + 2)
    gates(what + " df2", df2, c["df2"], c["df2_mag"], N1 + 2)
    again = run()
    assert torch.equal(again[0], flat1) and torch.equal(again[2], flat2), "a second run gives other bits"


# ---------------------------------------------------------------------------------------------------------------------
# lookup backward
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("integer", "fractional", "half", "out_of_bounds", "edges", "nonfinite")
# the last level of the first is 1 x 2 | odd maps, the width with the most round-trip index flips, a 1 x 39 level | radius 1
LOOKUP_SHAPES = [(1, 8, 16, 4, 4), (2, 5, 156, 3, 4), (1, 9, 12, 3, 1)]


def _level_sizes(h, w, L):
    sizes = []
    for _ in range(L):
        sizes.append((h, w))
        h, w = h // 2, w // 2
    return sizes


@functools.lru_cache(maxsize=None)
def lookup_case(B, h, w, L, r):
    """per coordinate family: the coordinates and, per level, the float64 gradient of two lookups with the two `grad_out`s and its
    sum of magnitudes (the weights are >= 0, so that is the same gradient for |grad_out|)"""
    g = torch.Generator().manual_seed(h * 1000 + w + r)
    N, n = h * w, 2 * r + 1
    assert [name for name, _ in coords_cases(B, h, w)] == list(FAMILIES)
    pyr = [torch.randn(B * N, 1, a, b, generator=g, dtype=torch.float64).requires_grad_() for a, b in _level_sizes(h, w, L)]
    gos = [torch.randn(B, L * n * n, h, w, generator=g) for _ in range(2)]
    fams = {}
    for name, coords in coords_cases(B, h, w):
        out = O.lookup(pyr, coords, r)
        ref = torch.autograd.grad((out * (gos[0].double() + gos[1].double())).sum(), pyr, retain_graph=True)
        mag = torch.autograd.grad((out * (gos[0].double().abs() + gos[1].double().abs())).sum(), pyr)
        fams[name] = (coords, [t.reshape(B * N, -1) for t in ref], [t.reshape(B * N, -1) for t in mag])
    return gos, fams


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,h,w,L,r", LOOKUP_SHAPES)
def test_corr_lookup_bwd(gpu, B, h, w, L, r, family):
    gos, fams = lookup_case(B, h, w, L, r)
    coords, ref, mag = fams[family]
    sizes = _level_sizes(h, w, L)
    M, n = B * h * w, 2 * r + 1
    cg = coords.to(gpu)
    gout = [Rows(M, L * n * n, gpu, go.permute(0, 2, 3, 1).reshape(M, L * n * n), pad=(-L * n * n) % 4 + 4) for go in gos]

    def run():
        bufs = [Rows(M, a * b, gpu, pad=(-a * b) % 4 + 4) for a, b in sizes]
        for buf in bufs:
            buf.full.zero_()                          # the entry accumulates: the caller zeroes the buffers
        for go in gout:
            torch.ops.pfk.corr_lookup_bwd([buf.rows for buf in bufs], [s[0] for s in sizes], [s[1] for s in sizes], cg, r, go.rows)
        return bufs

    bufs = run()
    torch.cuda.synchronize()
    for buf, (a, b), want, m in zip(bufs, sizes, ref, mag):
        what = f"lookup_bwd {(B, h, w, L, r)} {family} level {a}x{b}"
        assert bool((buf.flat[M * buf.ld:] == SENTINEL).all()), f"{what}: memory past the last row was written"
        assert bool((buf.full[:, a * b:] == 0).all()), f"{what}: the pad columns do not stay zero"
        assert bool(torch.isfinite(want).all())
        if a == 1 or b == 1:
            assert not bool(want.any()), "grid_sample's backward gives a 1-pixel level exactly 0"
        gates(what, buf.rows, want, m, 8 + 2)
    for b2, b1 in zip(run(), bufs):
        assert torch.equal(b2.flat, b1.flat), "a second run gives other bits"


# ---------------------------------------------------------------------------------------------------------------------
# convex upsampling backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "pixel_major"])
@pytest.mark.parametrize("B,H,W,logit_scale", [(2, 1, 5, 1.0), (1, 6, 1, 1.0), (2, 9, 13, 1.0), (2, 9, 13, 40.0)])
def test_convex_upsample_bwd(gpu, B, H, W, logit_scale, layout):
    """H = 1 / W = 1, both flow layouts, mask_ld = 580 and grad_mask_ld = 584, logits x 40 (a saturated softmax)"""
    c = convex_case(B, H, W, logit_scale)
    M = B * H * W
    mask = Rows(M, 576, gpu, c["mask"].permute(0, 2, 3, 1).reshape(M, 576))
    go = c["go"].to(gpu)
    if layout == "nchw":
        flow = c["flow"].to(gpu)
    else:
        flow = Rows(M, 2, gpu, c["flow"].permute(0, 2, 3, 1).reshape(M, 2), pad=2).rows          # flow_ld = 4, NaN in columns 2..3
    assert mask.ld == 580

    def run():
        gmask = Rows(M, 576, gpu, pad=8)
        flat, gflow = flat_out((B, 2, H, W), gpu)
        torch.ops.pfk.convex_upsample_bwd(flow, mask.rows, go, gmask.rows, gflow)
        return gmask, flat, gflow

    gmask, flat, gflow = run()
    torch.cuda.synchronize()
    assert gmask.ld == 584
    gmask.check_untouched("grad_mask")
    assert tail_kept(flat), "memory past grad_flow was written"
    what = f"convex_upsample_bwd {(B, H, W)} x{logit_scale:g} {layout}"
    gates(what + " grad_mask", gmask.rows, c["gmask"], c["gmask_mag"], c["k_mask"], floor=FLOOR)
    gates(what + " grad_flow", gflow, c["gflow"], c["gflow_mag"], c["k_flow"], floor=FLOOR)
    gmask2, flat2, _ = run()
    assert torch.equal(gmask2.flat, gmask.flat) and torch.equal(flat2, flat), "a second run gives other bits"


# ---------------------------------------------------------------------------------------------------------------------
# GRU gate kernels (include/pfk.h: gates_zr, gates_q, backward_q, backward_zr)
# ---------------------------------------------------------------------------------------------------------------------
SPECIAL = torch.tensor([100.0, -100.0, 1e30, -1e30])      # saturated pre-activations in row 0, columns 0..3


@functools.lru_cache(maxsize=None)
def gru_case(M, C):
    g = torch.Generator().manual_seed(M * 7 + C)
    d = {k: torch.randn(M, C, generator=g) for k in ("h", "a_q", "dh_new", "d_rh")}
    d["a_zr"] = torch.randn(M, 2 * C, generator=g) * 2
    d["a_zr"][0, :4], d["a_zr"][0, C:C + 4], d["a_q"][0, :4] = SPECIAL, SPECIAL, SPECIAL
    d["h"] = torch.tanh(d["h"])
    # inputs of the later kernels: the float64 gates rounded to fp32, exactly saturated where the pre-activation is
    for k, v in (("z", torch.sigmoid(d["a_zr"][:, :C].double())), ("r", torch.sigmoid(d["a_zr"][:, C:].double())), ("q", torch.tanh(d["a_q"].double()))):
        d[k] = v.float()
    d["z"][0, :4], d["r"][0, :4], d["q"][0, :4] = torch.tensor([1.0, 0, 1, 0]), torch.tensor([1.0, 0, 1, 0]), torch.tensor([1.0, -1, 1, -1])
    keep = torch.ones(M, C, dtype=torch.bool)
    keep[0, :4] = False
    d["keep"] = keep
    return d


@pytest.mark.parametrize("M,C", [(3, 4), (37, 36), (2 * 13 * 17, 128)])      # the minimum C | a partial block, ragged | several blocks
def test_gru_gate_kernels(gpu, M, C):
    """row stride h_ld = dh_new_ld = C + 8 with NaN pads; one row of pre-activations +-100, +-1e30: gates exactly 0 / +-1, derivatives
    exactly 0.  K per output, counted from the formulas of include/pfk.h with expf / tanhf within 2 / 5 ulp and every operation rounded
    once:  z, r 8 (expf 4, the addition, the division, slack 2);  rh 10;  q 10;  h_new 12 on |(1-z) h| + |z q|;  da_q 6 on
    |g z| (1 + q^2);  da_z 6 on |g| (|q| + |h|) z (1 + z);  dh 3 on |g| (1 + z);  da_r 6 on |d_rh h r| (1 + r);  dh += 3 on |dh| + |d_rh r|."""
    ops = torch.ops.pfk
    d = gru_case(M, C)
    keep = d["keep"]
    h, dh_new = Rows(M, C, gpu, d["h"], pad=8), Rows(M, C, gpu, d["dh_new"], pad=8)
    dev = {k: d[k].to(gpu) for k in ("a_zr", "a_q", "z", "r", "q", "d_rh")}
    D = {k: v.double() for k, v in d.items() if k != "keep"}
    one = torch.tensor([1.0, 0.0, 1.0, 0.0])

    def run():
        o = {k: flat_out((M, C), gpu) for k in ("z", "r", "rh", "q", "h_new", "da_q", "dh")}
        o["da_zr"] = flat_out((M, 2 * C), gpu)
        ops.gru_gates_zr(dev["a_zr"], h.rows, o["z"][1], o["r"][1], o["rh"][1])
        ops.gru_gates_q(dev["a_q"], dev["z"], h.rows, o["q"][1], o["h_new"][1])
        ops.gru_backward_q(dh_new.rows, dev["z"], dev["q"], h.rows, o["da_q"][1], o["da_zr"][1], o["dh"][1])
        torch.cuda.synchronize()
        half = o["da_zr"][1].clone()
        dh1 = o["dh"][1].clone()
        ops.gru_backward_zr(dev["d_rh"], h.rows, dev["r"], o["da_zr"][1], o["dh"][1])
        torch.cuda.synchronize()
        return o, half, dh1

    o, half, dh1 = run()
    for k, (flat, _) in o.items():
        assert tail_kept(flat), f"{k}: memory past the last row was written"
    assert bool((half[:, C:] == SENTINEL).all()), "backward_q wrote the r half of da_zr"
    assert torch.equal(half[:, :C], o["da_zr"][1][:, :C]), "backward_zr wrote the z half of da_zr"
    got = {k: v[1].cpu() for k, v in o.items()}
    # the saturated row
    assert torch.equal(got["z"][0, :4], one) and torch.equal(got["r"][0, :4], one), "saturated sigmoid is not exactly 0 / 1"
    assert torch.equal(got["rh"][0, :4], one * d["h"][0, :4]) and torch.equal(got["q"][0, :4], 2 * one - 1)
    assert torch.equal(got["h_new"][0, :4], (1 - d["z"][0, :4]) * d["h"][0, :4] + d["z"][0, :4] * (2 * one - 1))
    for k in ("da_q", "da_zr"):
        assert bool((got[k][0, :4] == 0).all()) and bool((got[k][0, C:C + 4] == 0).all() if k == "da_zr" else True), f"{k}: saturated gates must give exactly 0"
    z, r, q, hh, g, drh = D["z"], D["r"], D["q"], D["h"], D["dh_new"], D["d_rh"]
    zr, rr, qr = torch.sigmoid(D["a_zr"][:, :C]), torch.sigmoid(D["a_zr"][:, C:]), torch.tanh(D["a_q"])
    what = f"gru {(M, C)} "
    gates(what + "z", got["z"], zr, zr, 8, FLOOR, keep)
    gates(what + "r", got["r"], rr, rr, 8, FLOOR, keep)
    gates(what + "rh", got["rh"], rr * hh, (rr * hh).abs(), 10, FLOOR, keep)
    gates(what + "q", got["q"], qr, qr.abs(), 10, FLOOR, keep)
    gates(what + "h_new", got["h_new"], (1 - z) * hh + z * qr, ((1 - z) * hh).abs() + (z * qr).abs(), 12, FLOOR, keep)
    gates(what + "da_q", got["da_q"], g * z * (1 - q * q), (g * z).abs() * (1 + q * q), 6, FLOOR)
    gates(what + "da_z", got["da_zr"][:, :C], g * (q - hh) * z * (1 - z), g.abs() * (q.abs() + hh.abs()) * z * (1 + z), 6, FLOOR)
    gates(what + "dh (backward_q)", dh1, g * (1 - z), g.abs() * (1 + z), 3, FLOOR)
    gates(what + "da_r", got["da_zr"][:, C:], drh * hh * r * (1 - r), (drh * hh * r).abs() * (1 + r), 6, FLOOR)
    old = dh1.double().cpu()                   # backward_zr adds into the dh that backward_q left: its own fp32 input
    gates(what + "dh (backward_zr)", got["dh"], old + drh * r, old.abs() + (drh * r).abs(), 3, FLOOR)
    o2, _, _ = run()
    for k in o:
        assert torch.equal(o2[k][0], o[k][0]), f"{k}: a second run gives other bits"
