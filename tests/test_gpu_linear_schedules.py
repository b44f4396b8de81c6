"""The fp32 implicit-GEMM convolution with its LINEAR epilogue (pfk_conv2d_f32, pfk_conv2d_group_f32; ptlflow_amd/csrc/pfk_gemm.hip) on
every schedule of `launch()`'s switch, held to the fp64 op gate of tests/op_gate.py.

Every launch is restated in float64 on exactly what it consumes (tests/op_refs.py::linear_case: sources cut to their real channels,
the float32 scale widened, stride and 'same' padding) as
    out = relu2?( residual + scale * act(sum x w + bias) )
and gets
 1. relative L2 <= OP_TOL = 5e-6;
 2. |err| <= K * 2^-24 * mag, mag = |scale| (sum |x| |w| + |bias|) + |residual|, K = n + 4, n = kh kw sum(real) + [bias]: n roundings
    of the running sum in any order (stream-K partials included), one for the scale, one for the residual add, two to spare; relu is
    1-Lipschitz.  PFK_EPI_LINEAR_GELU gets gate 1 only: `gelu_erf` evaluates erff, whose own error is not derivable from the
    magnitudes of the terms;
 3. guards: the sources in `Rows` with NaN between the view width and the row stride and behind the last row (the columns between
    `real` and the view width ARE read, against zero weights: they hold finite garbage); the packed weight and the bias in the middle
    of NaN-filled buffers; the output in sentinel-filled rows whose lead and pad columns and whose 64 floats behind the last row must
    keep the sentinel; the residual buffer unchanged;
 4. a second run into fresh output rows gives the same bits.

Schedules.  `launch()` returns for a LINEAR launch (M rows, cout columns, `steps` K-steps of 32 channels, blocks64 = ceil(M / 64) *
ceil(cout / 64)): 11 where cout >= 2048 and M >= 2048; 9 (stream-K) with a workspace where 256 < blocks64 < 1024 fills its last round
of 256 below 0.92 with steps >= 24 and blocks64 * steps >= 80 * 256, or where blocks64 <= 64 and steps >= 128; else 10 from
blocks64 >= 768, 0 where steps < 16 and blocks64 < 256, else 4; then 15 where cout == 96 and M >= 128 * 256 (not over 9), and 11 over
10 where cout >= 256 is a multiple of 128 with ceil(M / 64) * (cout / 128) >= 1536 and steps >= 8: SELECTED = (0, 4, 10, 11, 15, 9).
OTHERS are the tiles the switch still holds.  Every schedule is forced (pfk_debug_set_tile); cfg 9 gets an armed workspace, must
leave the flag region zero and report no timed-out fix-up, and must have written partial tiles exactly where `sk_splits` — the
launcher's split restated — says a block boundary falls inside a tile.  More than one K-step is not enough for that: `down_1x1_s2`
has 6 tiles x 2 K-steps, which the launcher gives to 2 blocks of 3 whole tiles each, and its workspace must stay untouched; every
other case splits (`test_which_cases_split`).

Grids: 2 x 11 x 13, M = 286 = 4 * 64 + 30 = 2 * 128 + 30 with the image boundary (pixel 143) inside a tile; the strided cases
3 x 13 x 15 -> 7 x 8, M = 168 = 128 + 40.  Cases (op_refs.LINEAR_CASES): `motion` 3x3, sources 64/64 + 146/148 + 2/4 -> 126, relu,
dense [M, 126] rows (scalar stores) | `mask_head` 1x1 256 -> 576, x 0.25, the slice [:, 4:580] of 588-wide rows | `res_block` 3x3
96 -> 96 (the 128 x 96 tile's exact width), relu, residual in wider rows, relu2 | `down_s2` 3x3 stride 2 64 -> 96, relu, residual,
relu2 | `down_1x1_s2` | `sep_1x5`, `sep_5x1` (no bias) 128 + 128 -> 128 | `k7` 7x7 3/4 -> 40 | `convc1` 1x1 324 -> 256 (the last
chunk holds 4 channels) | `res_scaled` 3x3 48 -> 72, relu, x 0.37, residual: a residual AND a scale, which none of the others has.

Equal bits across schedules are asserted where the source promises them: pfk_gemm.hip, the comment above `cfg = 15` in `launch()`
("Same K order per output element: same bits"), and tests/test_gpu_conv_pp.py's TILES loop (cfgs 10-13 against cfg 4).  The base is
cfg 4.  For every other schedule the comparison is only printed.

Alignment fall-backs: `gemm_vec_flags` (pfk_gemm.h) turns the float4 accesses of `out`, `residual` and `bias` into scalar ones; all
eight combinations on `res_block` and `motion_res` (motion with a residual) must give the all-aligned launch's bits.
`cout_active` / `cout_split`: the active half carries the full launch's bits, the other half keeps the sentinel.
pfk_conv2d_group_f32: its three instantiations (the rule that picks one is restated in `group_kind` and asserted) against the gates
and, bit for bit, against the single launches.

Measured on an MI355X, worst over the cases of each test (relative L2 | error as a fraction of the per-element bound).  Records, not
thresholds: the thresholds are OP_TOL and a ratio of 1.
  test_linear_selected_schedules     7.3e-7 | 0.051     cfgs 10, 11, 15: the bits of cfg 4 on all ten cases, as promised; cfg 0 too
                                                        (not promised); cfg 9 differs on nine cases and agrees on `down_1x1_s2`,
                                                        the one it does not split
  test_linear_other_schedules        7.3e-7 | 0.005     cfgs 12, 13: the bits of cfg 4, as promised; 1, 2, 3, 5, 6, 7, 14 too; cfg 8
                                                        (two groups, in-block split K) differs
  test_linear_alignment_fallbacks    4.1e-7 | 0.005     all 2 x 6 x 7 unaligned launches: the aligned launch's bits
  test_linear_cout_active            5.6e-7 | 0.003
  test_linear_gelu                   7.9e-7 | -         (gate 1 only)
  test_group                         padded 1.9e-7 | 0.016     swizzled 6.4e-8 | 0.107     wide 4.6e-7 | 0.002
The ratios are small because K counts one rounding per term (about 1300 for `motion`) where a sum of random terms loses about
sqrt(n) of them; tests/test_op_gate_cpu.py shows that one dropped tap, a residual added before the scale, an omitted relu2 or a row
of the other image each fail the gates all the same.  Nothing failed: no kernel was changed.
The module's 115 cases take 2.5 s on an MI355X run alone (pytest's wall time, the float64 references included); the slowest case
0.14 s (the first one: the library's first launch), every other at most 0.06 s.
"""
import functools
import math

import pytest
import torch

from op_gate import OP_TOL, SENTINEL, Rows, arm, gates, guarded, record, rel, same_bits, ws_after
from op_refs import LINEAR_CASES, linear_case

pytestmark = pytest.mark.gpu

EPI_LINEAR, EPI_LINEAR_GELU = 0, 3
SELECTED = (0, 4, 10, 11, 15, 9)
OTHERS = (1, 2, 3, 5, 6, 7, 8, 12, 13, 14)
SAME_AS_4 = (10, 11, 12, 13, 15)     # test_gpu_conv_pp.py TILES; pfk_gemm.hip launch(), above `cfg = 15`
EVERY = ("motion", "mask_head", "res_block", "down_s2", "down_1x1_s2", "sep_1x5", "sep_5x1", "k7", "convc1", "res_scaled")
# where a case's output / residual rows lie in their wide rows: (lead, pad); default (0, 4)
OUT_AT = {"motion": (0, 0), "mask_head": (4, 8)}
RES_AT = {"res_block": (4, 4)}
assert set(EVERY) <= set(LINEAR_CASES) and sorted(SELECTED + OTHERS) == list(range(16))


@functools.lru_cache(maxsize=None)
def device_inputs(name, gpu):
    """sources with NaN pad columns and NaN behind the last row, packed weight and bias between NaN guards; shared, read-only"""
    c = linear_case(name)
    srcs = [Rows(c["M_in"], width, gpu, values=x, nan_tail=True) for x, (_, width) in zip(c["xs"], c["sources"])]
    return srcs, guarded(c["packed"], gpu), (guarded(c["bias"], gpu) if c["bias"] is not None else None)


@functools.lru_cache(maxsize=None)
def residual_rows(name, gpu, lead, pad):
    c = linear_case(name)
    r = Rows(c["M"], c["cout"], gpu, values=c["residual"], lead=lead, pad=pad, nan_tail=True)
    return r, r.flat.clone()


@functools.lru_cache(maxsize=None)
def off_by_one_bias(name, gpu):
    """the bias as buf[1: 1 + cout] of a 16-byte aligned NaN-filled buffer"""
    b = linear_case(name)["bias"]
    buf = torch.full((b.numel() + 72,), float("nan"), device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = buf[1: 1 + b.numel()]
    view.copy_(b)
    return view


def sk_splits(c):
    """whether the forced stream-K launch hands a partial tile from block to block — `launch_sk` and `conv_gemm_sk_kernel` restated:
    U = tiles * steps units over G blocks (512, or U / 6 where that leaves a block fewer than 6 units), block k owning the units
    [k U / G, (k + 1) U / G); one group of blocks below 64 tiles.  A tile is split where a block boundary is no tile boundary."""
    tiles, steps = math.ceil(c["M"] / 64) * math.ceil(c["cout"] / 64), c["steps"]
    units = tiles * steps
    blocks = 512 if units // 512 >= 6 else max(units // 6, 1)
    assert tiles < 64, "from 64 tiles up the stream-K launch cuts the tile list into one range per XCD first"
    return any((k * units // blocks) % steps for k in range(1, blocks))


def run(name, gpu, cfg, out_at=None, res_at=None, bias_off=False, active=0, split=0):
    """one forced launch into fresh sentinel rows, with its guard checks; returns the output `Rows`"""
    c = linear_case(name)
    srcs, packed, bias = device_inputs(name, gpu)
    if bias_off:
        bias = off_by_one_bias(name, gpu)
    lead, pad = out_at or OUT_AT.get(name, (0, 4))
    out = Rows(c["M"], c["cout"], gpu, lead=lead, pad=pad)
    res = res0 = None
    if c["residual"] is not None:
        res, res0 = residual_rows(name, gpu, *(res_at or RES_AT.get(name, (0, 4))))
    ws = None
    if cfg == 9:
        ws = torch.zeros(torch.ops.pfk.conv_workspace_bytes(), device=gpu, dtype=torch.uint8)
        arm(ws)
    what = f"{name} cfg {cfg}"
    torch.ops.pfk.debug_set_tile(cfg)
    try:
        torch.ops.pfk.conv2d([s.rows for s in srcs], *c["grid"], *c["k"], packed, bias, c["cout"],
                             EPI_LINEAR_GELU if c["act"] == "gelu" else EPI_LINEAR, c["relu"], c["scale"], out.rows, None, None, None, ws,
                             None if res is None else res.rows, c["stride"], c["relu2"], active, split)
    finally:
        torch.ops.pfk.debug_set_tile(-1)
    torch.cuda.synchronize()
    if ws is not None:
        ws_after(ws, None if active else sk_splits(c), what)     # (which of a partial launch's tiles are split is not restated)
    out.check_untouched(what)
    if res is not None:
        assert same_bits(res.flat, res0), f"{what}: the residual buffer was written"
    return out


def check(name, gpu, cfg, **kw):
    """gates 1-4 on one forced launch: (output Rows, (relative L2, ratio to the bound))"""
    c = linear_case(name)
    what = f"{name} cfg {cfg}"
    out = run(name, gpu, cfg, **kw)
    if c["act"] == "gelu":
        assert bool(torch.isfinite(out.rows).all()), f"{what}: non-finite values"
        r = rel(out.rows, c["ref"])
        print(f"{what}: relL2 {r:.2e}")
        assert r <= OP_TOL, f"{what}: relative L2 {r:.3e}"
        result = (r, 0.0)
    else:
        result = gates(what, out.rows, c["ref"], c["mag"], c["K"])
    assert same_bits(run(name, gpu, cfg, **kw).flat, out.flat), f"{what}: a second run gives other bits"
    return out, result


@functools.lru_cache(maxsize=None)
def base_bits(name, gpu):
    """cfg 4's output, the base of the equal-bits promises"""
    return run(name, gpu, 4).rows.clone()


def against_base(name, gpu, cfg, out):
    same = same_bits(out.rows, base_bits(name, gpu))
    if cfg in SAME_AS_4:
        assert same, f"{name}: cfg {cfg} differs from cfg 4, whose K order per output element it shares"
    else:
        print(f"{name}: cfg {cfg} {'has' if same else 'has not'} the bits of cfg 4")


def test_which_cases_split():
    on_cfg9 = EVERY + ("motion_res", "gelu_motion", "gelu_res", "active")
    assert {n for n in on_cfg9 if not sk_splits(linear_case(n))} == {"down_1x1_s2"}
    assert all(linear_case(n)["steps"] > 1 for n in on_cfg9)


@pytest.mark.parametrize("name", EVERY)
@pytest.mark.parametrize("cfg", SELECTED)
def test_linear_selected_schedules(gpu, cfg, name):
    out, result = check(name, gpu, cfg)
    against_base(name, gpu, cfg, out)
    record("test_linear_selected_schedules", [result])


@pytest.mark.parametrize("name", ("motion", "res_block"))
@pytest.mark.parametrize("cfg", OTHERS)
def test_linear_other_schedules(gpu, cfg, name):
    out, result = check(name, gpu, cfg)
    against_base(name, gpu, cfg, out)
    record("test_linear_other_schedules", [result])


# (lead, pad) of aligned and unaligned rows: res_block, cout 96: a view 1 / 2 floats into 100-wide rows; motion_res, cout 126: an odd
# row stride (127) / a view 1 float into 128-wide rows
ALIGNED = {"res_block": ((0, 4), (4, 4)), "motion_res": ((0, 2), (0, 2))}
UNALIGNED = {"res_block": ((1, 3), (2, 2)), "motion_res": ((0, 1), (1, 1))}


@pytest.mark.parametrize("name", ("res_block", "motion_res"))
@pytest.mark.parametrize("cfg", SELECTED)
def test_linear_alignment_fallbacks(gpu, cfg, name):
    """all eight combinations of aligned / unaligned out, residual and bias: the all-aligned launch's bits, and its guards"""
    (out_a, res_a), (out_u, res_u) = ALIGNED[name], UNALIGNED[name]
    base, result = check(name, gpu, cfg, out_at=out_a, res_at=res_a)
    assert base.rows.data_ptr() % 16 == 0 and base.ld % 4 == 0
    for bits in range(1, 8):
        uo, ur, ub = bits & 1, bits & 2, bits & 4
        out = run(name, gpu, cfg, out_at=out_u if uo else out_a, res_at=res_u if ur else res_a, bias_off=bool(ub))
        assert not uo or out.rows.data_ptr() % 16 != 0 or out.ld % 4 != 0
        assert same_bits(out.rows, base.rows), f"{name} cfg {cfg}: unaligned out={bool(uo)} residual={bool(ur)} bias={bool(ub)} gives other bits"
    record("test_linear_alignment_fallbacks", [result])


@pytest.mark.parametrize("cfg", SELECTED)
def test_linear_cout_active(gpu, cfg):
    """3x3 128 -> 128 with cout_active 64 (and cout_split 64, the stream-K tile order of the fused heads)"""
    c = linear_case("active")
    results = []
    for split in (0, 64):
        full, result = check("active", gpu, cfg, split=split)
        half = run("active", gpu, cfg, active=64, split=split)
        assert same_bits(half.rows[:, :64], full.rows[:, :64]), f"cfg {cfg} split {split}: the active half differs from the full launch"
        assert bool((half.rows[:, 64:] == SENTINEL).all()), f"cfg {cfg} split {split}: the inactive half was written"
        results += [result, gates(f"active half cfg {cfg}", half.rows[:, :64], c["ref"][:, :64], c["mag"][:, :64], c["K"])]
    record("test_linear_cout_active", results)


@pytest.mark.parametrize("name", ("gelu_motion", "gelu_res"))
@pytest.mark.parametrize("cfg", SELECTED)
def test_linear_gelu(gpu, cfg, name):
    _, result = check(name, gpu, cfg)
    record("test_linear_gelu", [result])


# ---------------------------------------------------------------------------------------------------------------------
# pfk_conv2d_group_f32
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = {"padded": ("g_c1", "g_k3", "g_mask"), "swizzled": ("g_sw0", "g_sw1"), "wide": ("g_wide0", "g_wide1")}


def group_kind(cases):
    """pfk_conv2d_group_f32's choice: 64 x 128 tiles where every cout is a multiple of 128 and every K >= 2048; else 64 x 64 tiles on
    the swizzled layout from 768 tiles up, on the padded one below"""
    wide = all(c["cout"] % 128 == 0 and c["packed"].shape[1] >= 64 * 32 for c in cases)
    bn = 128 if wide else 64
    total = sum(math.ceil(c["M"] / 64) * math.ceil(c["cout"] / bn) for c in cases)
    return ("wide" if wide else "swizzled" if total >= 3 * 256 else "padded"), total


def test_group_kinds():
    kinds = {k: group_kind([linear_case(n) for n in names]) for k, names in GROUPS.items()}
    assert kinds == {"padded": ("padded", 75), "swizzled": ("swizzled", 780), "wide": ("wide", 9)}, kinds


@pytest.mark.parametrize("kind", list(GROUPS))
def test_group(gpu, kind):
    names = GROUPS[kind]
    cases = [linear_case(n) for n in names]
    assert group_kind(cases)[0] == kind and len({c["grid"] for c in cases}) == 1
    assert all(c["k"][0] == c["k"][1] and c["stride"] == 1 and len(c["sources"]) == 1 and not c["relu2"] for c in cases)
    ins = [device_inputs(n, gpu) for n in names]
    res = [residual_rows(n, gpu, 4, 4) for n in names]
    empty = torch.empty(0, device=gpu)

    def launch():
        outs = [Rows(c["M"], c["cout"], gpu, lead=4, pad=8) for c in cases]
        torch.ops.pfk.conv2d_group([i[0][0].rows for i in ins], *cases[0]["grid"], [c["k"][0] for c in cases], [i[1] for i in ins],
                                   [empty if i[2] is None else i[2] for i in ins], [int(c["relu"]) for c in cases],
                                   [c["scale"] for c in cases], [o.rows for o in outs], [r.rows for r, _ in res])
        torch.cuda.synchronize()
        return outs

    outs, again = launch(), launch()
    results = []
    for n, c, o, o2, (r, r0) in zip(names, cases, outs, again, res):
        o.check_untouched(n)
        assert same_bits(r.flat, r0), f"{n}: the residual buffer was written"
        results.append(gates(f"group {kind} {n}", o.rows, c["ref"], c["mag"], c["K"]))
        assert same_bits(o.flat, o2.flat), f"{n}: a second run gives other bits"
        assert same_bits(o.rows, run(n, gpu, -1).rows), f"{n}: the grouped launch differs from the single launch"
    record(f"test_group {kind}", results)
