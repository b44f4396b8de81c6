"""CCMR's per-scale context grouping `model.xcit[i]` on the kernels (K17, ptlflow_amd/csrc/pfk_xcit.hip, ptlflow_amd/xcit.py) on the GPU.

The two new kernels against float64 on their own inputs (instruments of tests/op_gate.py): `pfk_xcit_tokens_f32` — x0 bit for bit (one
correctly rounded add has one answer), xh within OP_TOL and `close32`, row strides 128 / 132 / 160 into NaN-filled rows between
sentinels, NaN-guarded inputs, a NaN image that stays in its image, an input on which a one-pass variance fails — and
`pfk_xca_fold_f32` against `xcit.fold_attention` in float64 and the closed form of an identity map.  Then `XcitContextEngine` against
the stand-in in float64 under the gate of tests/test_gpu_xcit.py's engine test (`scale_close`, BLOCK_TOL), the fixture replay, the
wrapper's dispatch, and the multi-scale loop with every option on: close to the option off, and the same bits twice."""
import copy

import pytest
import torch

from ccmr_context_refs import aggregator_registered, context_loop_model, load_golden, standin
from op_gate import BLOCK_TOL, GUARD, OP_TOL, SENTINEL, close32, flat_out, guarded, rel, same_bits, scale_close, tail_kept
from xcit_model import XCiT, randomize
from xcit_refs import C, LN_EPS, block_params, layernorm_ref

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1, 1), (2, 5, 7), (1, 3, 65), (3, 4, 6), (1, 9, 33)]      # 3x65: a row wider than a wave; 9x33 = 297 tokens: two xca_map chunks
ids = lambda g: "x".join(map(str, g))  # noqa: E731
OFFSET = 24.0     # the common per-row offset of `offset_input` (see test_offset_input_separates_the_two_variance_forms)


def plain_input(B, H, W, seed):
    """[B, C, H, W] fp32: every image at its own scale and offset, so that a read from the neighbouring image moves the result"""
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
    for b in range(B):
        x[b] = x[b] * (1.0 + 0.5 * b) + 0.3 * b
    return x


def offset_input(B, H, W, seed):
    """unit noise on a common per-row (per-pixel) offset in [OFFSET, OFFSET + 3]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g) + (OFFSET + 3 * torch.rand(B, 1, H, W, generator=g))


def pos_values(H, W, seed):
    return torch.randn(H * W, C, generator=torch.Generator().manual_seed(seed)) * 0.7


class OutRows:
    """[M, C] output rows with row stride `ld` in a flat buffer: NaN in the rows' region (the pad columns must keep it), the sentinel
    in 64 elements on both sides"""

    def __init__(self, M, ld, device):
        self.flat = torch.full((2 * GUARD + M * ld,), SENTINEL, device=device, dtype=torch.float32)
        self.full = self.flat[GUARD:GUARD + M * ld].view(M, ld)
        self.full.fill_(float("nan"))
        self.rows = self.full[:, :C]

    def check(self, what):
        assert tail_kept(self.flat) and bool((self.flat[:GUARD] == SENTINEL).all()), f"{what}: memory beside the rows was written"
        assert bool(torch.isnan(self.full[:, C:]).all()), f"{what}: pad columns were written"
        assert bool(torch.isfinite(self.rows).all()), f"{what}: rows left unwritten (or not finite)"


def run_tokens(gpu, x, pos, B, H, W, ld=C, layout="nchw"):
    """the kernel on NaN-guarded inputs; `layout` "pm": the same values as channels-last rows through pfk_xcit_tokens_pm_f32"""
    x0, xh = OutRows(B * H * W, ld, gpu), OutRows(B * H * W, ld, gpu)
    p = None if pos is None else guarded(pos, gpu)
    if layout == "nchw":
        torch.ops.pfk.xcit_tokens(guarded(x, gpu), p, LN_EPS, x0.rows, xh.rows)
    else:
        rows = guarded(x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous(), gpu)
        torch.ops.pfk.xcit_tokens_pm(rows, p, LN_EPS, x0.rows, xh.rows, B, H, W)
    x0.check(f"xcit_tokens x0 ld {ld}")
    xh.check(f"xcit_tokens xh ld {ld}")
    return x0, xh


def check_tokens(what, x0, xh, x, pos, B, H, W):
    want0 = x.permute(0, 2, 3, 1).reshape(B, H * W, C)
    if pos is not None:
        want0 = want0 + pos[None]                               # fp32: one correctly rounded add
    got0 = x0.rows.cpu()
    assert same_bits(got0, want0.reshape(-1, C).contiguous()), f"{what}: x0 is not rows(in) + pos bit for bit"
    ref = layernorm_ref(got0.double())
    close32(xh.rows.cpu(), ref, what)
    r = rel(xh.rows, ref)
    print(f"{what}: xh relL2 {r:.2e}")
    assert r <= OP_TOL, f"{what}: relative L2 {r:.3e}"
    return r


# ---------------------------------------------------------------------------------------------------------------------
# pfk_xcit_tokens_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=ids)
@pytest.mark.parametrize("layout", ["nchw", "pm"])
def test_tokens(gpu, grid, layout):
    B, H, W = grid
    x, pos = plain_input(B, H, W, 11), pos_values(H, W, 13)
    for ld in (128, 132, 160):
        x0, xh = run_tokens(gpu, x, pos, B, H, W, ld, layout)
        check_tokens(f"tokens {layout} {grid} ld {ld}", x0, xh, x, pos, B, H, W)
        again0, againh = run_tokens(gpu, x, pos, B, H, W, ld, layout)
        assert same_bits(again0.rows, x0.rows) and same_bits(againh.rows, xh.rows)          # a second run: the same bits
    n0, nh = run_tokens(gpu, x, None, B, H, W, 132, layout)                                   # pos absent
    check_tokens(f"tokens {layout} {grid} without pos", n0, nh, x, None, B, H, W)
    assert B * H * W == 1 or not same_bits(n0.rows, x0.rows)


def test_tokens_both_layouts_give_the_same_bits(gpu):
    B, H, W = 2, 5, 7
    x, pos = plain_input(B, H, W, 17), pos_values(H, W, 19)
    a0, ah = run_tokens(gpu, x, pos, B, H, W, 128, "nchw")
    b0, bh = run_tokens(gpu, x, pos, B, H, W, 128, "pm")
    assert same_bits(a0.rows, b0.rows) and same_bits(ah.rows, bh.rows)


@pytest.mark.parametrize("layout", ["nchw", "pm"])
def test_tokens_nan_image_stays_in_its_image(gpu, layout):
    B, H, W = 2, 5, 7                                             # 35 pixels: both images inside one 64-pixel tile's reach
    x, pos = plain_input(B, H, W, 23), pos_values(H, W, 29)
    clean0, cleanh = run_tokens(gpu, x, pos, B, H, W, 132, layout)
    bad = x.clone()
    bad[1] = float("nan")
    x0 = OutRows(B * H * W, 132, gpu)
    xh = OutRows(B * H * W, 132, gpu)
    if layout == "nchw":
        torch.ops.pfk.xcit_tokens(guarded(bad, gpu), guarded(pos, gpu), LN_EPS, x0.rows, xh.rows)
    else:
        torch.ops.pfk.xcit_tokens_pm(guarded(bad.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), gpu), guarded(pos, gpu), LN_EPS, x0.rows,
                                     xh.rows, B, H, W)
    N = H * W
    assert same_bits(x0.rows[:N], clean0.rows[:N]) and same_bits(xh.rows[:N], cleanh.rows[:N])
    assert bool(torch.isnan(x0.rows[N:]).all()) and bool(torch.isnan(xh.rows[N:]).all())


def _two_pass_fp32(x):
    m = x.mean(-1, keepdim=True)
    d = x - m
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + LN_EPS)


def _one_pass_fp32(x):
    m = x.mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(((x * x).mean(-1, keepdim=True) - m * m).clamp_min(0) + LN_EPS)


def test_offset_input_separates_the_two_variance_forms():
    """On the CPU, in fp32: on unit noise around a common per-row offset of 24 .. 27 the variance about the mean (two passes) stays
    inside OP_TOL (measured 1.3e-6: the mean's rounding, linear in the offset) and E[x^2] - mean^2 does not (3.8e-5: quadratic).  The
    offset is fixed here, before the kernel sees the input."""
    rows = offset_input(1, 9, 33, 31).permute(0, 2, 3, 1).reshape(-1, C)
    ref = layernorm_ref(rows.double())
    two, one = rel(_two_pass_fp32(rows), ref), rel(_one_pass_fp32(rows), ref)
    print(f"offset {OFFSET}: two-pass relL2 {two:.2e}, one-pass {one:.2e}")
    assert two <= OP_TOL / 2 and one > 4 * OP_TOL


@pytest.mark.parametrize("layout", ["nchw", "pm"])
def test_tokens_variance_is_taken_about_the_mean(gpu, layout):
    B, H, W = 1, 9, 33
    x = offset_input(B, H, W, 31)
    x0, xh = run_tokens(gpu, x, None, B, H, W, 128, layout)
    check_tokens(f"tokens {layout} on an offset of {OFFSET}", x0, xh, x, None, B, H, W)


def test_tokens_binding_refuses_wrong_views(gpu):
    x = plain_input(2, 3, 4, 37).to(gpu)
    M = 2 * 3 * 4
    ok = lambda: torch.zeros(M, C, device=gpu)  # noqa: E731
    with pytest.raises(RuntimeError):
        torch.ops.pfk.xcit_tokens(x.permute(0, 1, 3, 2), None, LN_EPS, ok(), ok())                   # not contiguous
    with pytest.raises(RuntimeError):
        torch.ops.pfk.xcit_tokens(x, None, LN_EPS, torch.zeros(M - 1, C, device=gpu), ok())          # a row short
    with pytest.raises(RuntimeError):
        torch.ops.pfk.xcit_tokens(x, torch.zeros(3 * 4 - 1, C, device=gpu), LN_EPS, ok(), ok())      # pos too small
    with pytest.raises(RuntimeError):
        torch.ops.pfk.xcit_tokens(x[:, :64].contiguous(), None, LN_EPS, torch.zeros(M, 64, device=gpu), torch.zeros(M, 64, device=gpu))
    buf = ok()
    with pytest.raises(RuntimeError):
        torch.ops.pfk.xcit_tokens(x, None, LN_EPS, buf, buf)                                         # the outputs overlap


# ---------------------------------------------------------------------------------------------------------------------
# pfk_xca_fold_f32
# ---------------------------------------------------------------------------------------------------------------------
def fold_setup(gpu, seed):
    from ptlflow_amd.xcit import XcitContextEngine
    model = randomize(XCiT(separate=False), seed).eval()
    eng = XcitContextEngine(copy.deepcopy(model).to(gpu), gpu)
    return model, eng


def run_fold(gpu, eng, A):
    B = A.shape[0]
    mflat, M = flat_out((B, C, C), gpu)
    cflat, c = flat_out((B, C), gpu)
    w = eng.w
    torch.ops.pfk.xca_fold(guarded(A, gpu), w["v.w"], w["v.b"], w["proj.w"], w["proj.b"], M, c)
    assert tail_kept(mflat) and tail_kept(cflat)
    return mflat, cflat, M, c


@pytest.mark.parametrize("B", [1, 3])
def test_xca_fold_against_fold_attention_in_float64(gpu, B):
    from ptlflow_amd.xcit import fold_attention, split_qkv
    model, eng = fold_setup(gpu, 41)
    A = torch.softmax(torch.randn(B, 8, 16, 16, generator=torch.Generator().manual_seed(43)) * 2.0, -1)
    m1, c1, M, c = run_fold(gpu, eng, A)
    m2, c2, _, _ = run_fold(gpu, eng, A)
    assert torch.equal(m1, m2) and torch.equal(c1, c2)                                        # a second run: the same bits
    M64, c64 = fold_attention(A.double(), split_qkv(block_params(model)))
    rm, rc = rel(M, M64), rel(c, c64)
    print(f"xca_fold B={B}: relL2 M {rm:.2e}  c {rc:.2e}")
    assert rm <= OP_TOL and rc <= OP_TOL
    close32(M.cpu(), M64, "xca_fold M")
    close32(c.cpu(), c64, "xca_fold c")
    assert B == 1 or float((M[0] - M[-1]).abs().max()) > 1e-3                                  # per image


def test_xca_fold_of_the_identity_map_is_the_closed_form(gpu):
    _, eng = fold_setup(gpu, 47)
    B = 2
    A = torch.eye(16).expand(B, 8, 16, 16).contiguous()
    _, _, M, c = run_fold(gpu, eng, A)
    w = {k: v.double().cpu() for k, v in eng.w.items()}
    M64 = w["proj.w"] @ w["v.w"]                                                              # diag(gamma1) W_proj W_v'
    c64 = w["proj.w"] @ w["v.b"] + w["proj.b"]
    assert torch.equal(M[0], M[1]) and torch.equal(c[0], c[1])
    assert rel(M[0], M64) <= OP_TOL and rel(c[0], c64) <= OP_TOL
    close32(M[0].cpu(), M64, "xca_fold identity M")
    close32(c[0].cpu(), c64, "xca_fold identity c")


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS + [(5, 4, 6)], ids=ids)             # 5x4x6: past the four-image group of the grouped GEMM
@pytest.mark.parametrize("use_pos", [True, False], ids=["pos", "nopos"])
def test_engine_against_the_standin_in_float64(gpu, grid, use_pos):
    from ptlflow_amd.xcit import XcitContextEngine
    B, H, W = grid
    model = randomize(XCiT(separate=False, use_pos=use_pos), 53).eval()
    m64 = copy.deepcopy(model).double()
    eng = XcitContextEngine(copy.deepcopy(model).to(gpu), gpu)
    results = []
    with torch.no_grad():
        for i in range(2):
            inp = torch.relu(plain_input(B, H, W, 59 + i))
            ref, cpu32 = m64(inp.double()), model(inp)
            got = eng(inp.to(gpu))
            assert got.shape == (B, C, H, W) and got.is_contiguous() and got.dtype == torch.float32
            scale_close(got, ref, f"context engine {grid} call {i}")
            results.append((rel(got, ref), rel(cpu32, ref)))
            cl = eng(inp.to(gpu).contiguous(memory_format=torch.channels_last))              # the channels-last load path
            assert same_bits(cl, got) and cl.data_ptr() != got.data_ptr()                    # the same bits, a fresh tensor
    print(f"RECORD context engine {ids(grid)} use_pos={use_pos}: relL2 to fp64 {max(r for r, _ in results):.1e} | torch fp32 on the CPU "
          f"{max(c for _, c in results):.1e}")


def test_golden_replay(gpu):
    from ptlflow_amd.xcit import XcitContextEngine, match_xcit_context
    gold = load_golden()
    B, H, W = gold["shape"]
    model = standin(gold)
    assert match_xcit_context(model)
    eng = XcitContextEngine(model.to(gpu), gpu)
    with torch.no_grad():
        got = eng(gold["inp"].to(gpu))
        scale_close(got, gold["out"], "golden out")
        scale_close(got, gold["out64"], "golden out64")
        scale_close(eng.A.cpu(), gold["A"], "golden A")
        scale_close(eng.x1.cpu().reshape(B, H * W, C), gold["x1"], "golden x1")
        scale_close(eng.x2.cpu().reshape(B, H * W, C), gold["x2"], "golden x2")
        # a parameter changed in place: `pack` again, as the `_engine_for` idiom of the wrapper does on a new version
        model.blocks[0].gamma2.mul_(2.0)
        eng.pack()
        scale_close(eng(gold["inp"].to(gpu)), copy.deepcopy(model).cpu().double()(gold["inp"].double()), "after a repack")


# ---------------------------------------------------------------------------------------------------------------------
# the wrapper
# ---------------------------------------------------------------------------------------------------------------------
def test_wrapper_serves_and_falls_back(gpu):
    from ptlflow_amd.xcit import PfkXcitContext
    ref = randomize(XCiT(separate=False), 61).to(gpu).eval()
    for p in ref.parameters():
        p.requires_grad_(False)
    wrap = PfkXcitContext(ref)
    assert list(wrap.state_dict().keys()) == list(ref.state_dict().keys())
    x = torch.relu(plain_input(2, 5, 7, 67)).to(gpu)
    with torch.no_grad():
        want = ref(x)
        got = wrap(x)
    assert (wrap.engine_calls, wrap.fallback_calls) == (1, 0)
    scale_close(got, want, "wrapper, served")
    with torch.no_grad():
        assert same_bits(wrap(x.contiguous(memory_format=torch.channels_last)), got)           # channels-last rows are served too
    assert (wrap.engine_calls, wrap.fallback_calls) == (2, 0)

    # Every other call is the module's: the wrapper hands back the very tensor the module returned for that call (a forward hook on
    # the module sees it), so "equals the module's" holds bit for bit although the module in torch does not repeat its own bits
    # from call to call on the GPU; a second call of the module itself is compared as closely as the precision in use allows.
    seen = []

    def falls_back(what, w, m, call, tol=1e-5):
        handle = m.register_forward_hook(lambda _m, _i, o: seen.append(o))
        e, f = w.engine_calls, w.fallback_calls
        out = call(w)
        handle.remove()
        assert (w.engine_calls, w.fallback_calls) == (e, f + 1), what
        assert out is seen[-1], f"{what}: the wrapper did not return the module's own output"
        scale_close(out.detach().float(), call(m).detach().float(), f"wrapper fallback: {what}", tol)

    def no_grad(t):
        def call(m):
            with torch.no_grad():
                return m(t)
        return call

    def autocast(m):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return m(x)

    wrap.train()
    falls_back("train mode", wrap, ref, no_grad(x))
    assert ref.training
    wrap.eval()
    ref.eval()
    ref.blocks[0].gamma1.requires_grad_(True)
    falls_back("grad mode with a parameter requiring grad", wrap, ref, lambda m: m(x))
    ref.blocks[0].gamma1.requires_grad_(False)
    falls_back("cuda autocast", wrap, ref, autocast, tol=2e-2)             # (bf16 matmuls on both sides)
    half = copy.deepcopy(ref).half()
    hwrap = PfkXcitContext(half)
    falls_back("an fp16 input", hwrap, half, no_grad(x.half()), tol=1e-2)
    assert hwrap.engine_calls == 0
    wide = torch.relu(plain_input(2, 5, 14, 71)).to(gpu)
    assert not wide[..., ::2].is_contiguous()
    falls_back("a non-contiguous input", wrap, ref, no_grad(wide[..., ::2]))
    with torch.no_grad():
        assert same_bits(wrap(x), got)                                # and the served path repeats its bits
    assert wrap.engine_calls == 3


def test_wrapper_rebuilds_on_a_parameter_version_change(gpu):
    from ptlflow_amd.xcit import PfkXcitContext
    ref = randomize(XCiT(separate=False), 73).to(gpu).eval()
    for p in ref.parameters():
        p.requires_grad_(False)
    wrap = PfkXcitContext(ref)
    x = torch.relu(plain_input(1, 4, 6, 79)).to(gpu)
    with torch.no_grad():
        a = wrap(x)
        ref.blocks[0].gamma2.mul_(2.0)
        b = wrap(x)
        scale_close(b, copy.deepcopy(ref).double()(x.double()), "after an in-place parameter change")
    assert not torch.equal(a, b) and wrap.engine_calls == 2


# ---------------------------------------------------------------------------------------------------------------------
# the loop: every multi-scale option on
# ---------------------------------------------------------------------------------------------------------------------
OPTS = dict(multiscale_encoders=True, multiscale_upsample=True, ccmr_aggregator=True)
_LOOP = {}


def loop_runs(gpu):
    """three forwards, computed once: the three options without `ccmr_context`, and two forwards of one model with it"""
    if not _LOOP:
        from ptlflow_amd import patch
        iters = (2, 3, 2)
        x = torch.rand(2, 2, 3, 64, 96, generator=torch.Generator().manual_seed(5)).to(gpu)

        def make(**kw):
            model = context_loop_model(iters, aggregators=True).to(gpu)
            for p in model.parameters():
                p.requires_grad_(False)
            return patch.accelerate(model, **OPTS, **kw)

        def forward(model):
            with torch.no_grad():
                out = model({"images": x})
            return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}

        with aggregator_registered():
            off, on = make(), make(ccmr_context=True)
        _LOOP["off"] = forward(off)
        _LOOP["off aggregator_calls"] = off.update_block.aggregator_calls
        _LOOP["off wrapped"] = [type(m).__name__ for m in off.xcit]
        _LOOP["on"] = forward(on)
        _LOOP["on counters"] = [(m.engine_calls, m.fallback_calls) for m in on.xcit]
        _LOOP["on aggregator_calls"] = on.update_block.aggregator_calls
        _LOOP["again"] = forward(on)
        _LOOP["again counters"] = [(m.engine_calls, m.fallback_calls) for m in on.xcit]
        _LOOP["iters"] = iters
        patch.restore(on)
        _LOOP["restored"] = [type(m).__name__ for m in on.xcit]
        patch.restore(off)
    return _LOOP


def test_loop_serves_every_scale_and_leaves_the_aggregator_alone(gpu):
    r = loop_runs(gpu)
    n = len(r["iters"])
    assert r["off wrapped"] == ["XCiT"] * n and r["restored"] == ["XCiT"] * n
    assert r["on counters"] == [(1, 0)] * n                                   # engine_calls == num_scales per forward
    assert r["again counters"] == [(2, 0)] * n
    assert r["on aggregator_calls"] == r["off aggregator_calls"] == sum(r["iters"])


def test_loop_option_on_is_close_to_option_off(gpu):
    r = loop_runs(gpu)
    for k in ("flows", "flow_small"):
        assert bool(torch.isfinite(r["on"][k]).all()) and float(r["on"][k].abs().max()) > 1e-3
        scale_close(r["on"][k], r["off"][k], f"{k}: ccmr_context on against off", BLOCK_TOL)


def test_loop_repeats_its_bits_without_a_replay_hook(gpu):
    r = loop_runs(gpu)
    for k in ("flows", "flow_small"):
        assert same_bits(r["again"][k], r["on"][k]), f"{k}: two forwards of the all-options model differ"

