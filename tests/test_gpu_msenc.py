"""The multi-scale GroupNorm encoders on the kernels (K15, ptlflow_amd/csrc/pfk_msenc.hip, ptlflow_amd/ms_encoder.py) on the GPU.

Per kernel, against float64 on the kernel's own inputs (tests/msenc_refs.py; instruments of tests/op_gate.py): the per-element bound
through `gates`, NaN where an input must not be read (pad columns, the neighbouring image), sentinels where an output must not be
written, the same bits on a second run on fresh buffers.  Then the engine against the stand-in (tests/msenc_model.py) in float64 for
all six encoders, the fixture recorded from the reference's classes, and the `accelerate(model, multiscale_encoders=True)` seam.

`pfk_groupnorm_stats_f32` hands out the fp32 pair (scale, shift), so the gate has two parts.  (1) y = x * scale + shift, formed in
float64 from the kernel's pair, stays within 6 * 2^-24 * (|x| |scale| + |shift|) of float64 GroupNorm at every element of the input.
(2) Relative L2 <= OP_TOL holds for the kernel's OUTPUTS, scale and shift, against their float64 values.  It cannot be asked of y:
with a group mean of 100 and a deviation of 0.1, shift is about -1000 and its own fp32 rounding (up to 3e-5) is 1e-5 of y's scale
whatever the kernel does; the same for HW = 1, where rstd = 1 / sqrt(eps) = 316.  y's relative L2 is printed.  A single-precision
E[x^2] - mean^2 loses all of var = 0.01 next to E[x^2] = 10000 (one fp32 ulp there is 1e-3) and fails both parts.

Engine gate, per pyramid level: relative L2 to the stand-in's float64 forward <= max(4 * e_ref, OP_TOL), e_ref the stand-in's own
torch-fp32 CPU forward against the same float64 forward (the factor 4: other summation orders, Winograd's larger constant).
"""
import copy
import functools

import pytest
import torch

from msenc_model import ENCODERS, SEEDS, MsModel, make, randomize, register
from msenc_refs import GN_CHUNK_ROWS, GN_EPS, affine_apply_ref, groupnorm_ref, load_golden, load_golden_levels, resize_ref
from op_gate import BLOCK_TOL, OP_TOL, SENTINEL, Rows, flat_out, gates, rel, same_bits, scale_close, tail_kept

pytestmark = pytest.mark.gpu

KEYS = sorted(ENCODERS)


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------
# pfk_groupnorm_stats_f32
# ---------------------------------------------------------------------------------------------------------------------
def gn_input(case, B, C, seed):
    """[B, HW, C] fp32.  hw1: one pixel, constant per group (variance exactly 0); 7x9; chunks: 2 * 256 + 88 pixels, three reduction
    chunks of GN_CHUNK_ROWS with a ragged last one; offset: mean 100, standard deviation 0.1 per group"""
    assert GN_CHUNK_ROWS == 256
    if case == "hw1":
        return randn(seed, B, 1, C // 8, 1).expand(B, 1, C // 8, 8).reshape(B, 1, C).contiguous()
    HW = {"7x9": 63, "chunks": 2 * GN_CHUNK_ROWS + 88, "offset": 2 * GN_CHUNK_ROWS + 88}[case]
    x = randn(seed, B, HW, C)
    if case == "offset":
        return 100.0 + 0.1 * x
    for b in range(B):       # every image and every group at its own scale and offset
        x[b] = x[b] * (1.0 + 0.5 * b) + 0.3 * b
    return x * (1.0 + 0.1 * (torch.arange(C) // 8)) + 0.05 * (torch.arange(C) // 8)


@pytest.mark.parametrize("case", ["hw1", "7x9", "chunks", "offset"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [64, 96, 160, 256])
def test_groupnorm_stats(gpu, C, B, case):
    x = gn_input(case, B, C, 11 + C + B)
    HW = x.shape[1]
    gamma, beta = 1.0 + 0.3 * randn(3, C), 0.2 * randn(4, C)
    src = Rows(B * HW, C, gpu, x.reshape(B * HW, C).to(gpu))          # ld = C + 4, NaN in the pad columns
    outs = []
    for _ in range(2):
        fs, scale = flat_out((B * C,), gpu)
        ft, shift = flat_out((B * C,), gpu)
        ws = torch.empty(torch.ops.pfk.groupnorm_workspace_bytes(B, HW, C), dtype=torch.uint8, device=gpu)
        torch.ops.pfk.groupnorm_stats(src.rows, B, HW, 8, gamma.to(gpu), beta.to(gpu), GN_EPS, scale, shift, ws)
        assert tail_kept(fs) and tail_kept(ft)
        outs.append((fs, ft))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    scale = outs[0][0][:B * C].view(B, C).double().cpu()
    shift = outs[0][1][:B * C].view(B, C).double().cpu()
    rs, rt, y, mag = groupnorm_ref(x.double(), gamma, beta)
    got = x.double() * scale[:, None, :] + shift[:, None, :]
    print(f"groupnorm_stats C={C} B={B} {case}: relL2 of y {rel(got, y):.2e}")
    err, bound = (got - y).abs(), 6 * 2.0 ** -24 * mag
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bound).all()), f"y: worst |err| / bound {float((err / bound).max()):.3f}"
    r_scale, r_shift = rel(scale, rs), rel(shift, rt)
    print(f"   scale relL2 {r_scale:.2e}  shift relL2 {r_shift:.2e}  worst |err| / bound {float((err / bound).max()):.3f}")
    assert r_scale <= OP_TOL and r_shift <= OP_TOL
    if case == "hw1":      # variance exactly 0: rstd = 1 / sqrt(eps)
        assert float((scale / (gamma.double() / GN_EPS ** 0.5) - 1).abs().max()) <= 2.0 ** -23


def test_groupnorm_stats_refuses_another_group_size(gpu):
    x = randn(1, 10, 64).to(gpu)
    out = lambda: torch.empty(64, device=gpu)  # noqa: E731
    ws = torch.empty(torch.ops.pfk.groupnorm_workspace_bytes(1, 10, 64), dtype=torch.uint8, device=gpu)
    for gs in (4, 16):
        with pytest.raises(RuntimeError, match="groupnorm_stats"):
            torch.ops.pfk.groupnorm_stats(x, 1, 10, gs, out(), out(), GN_EPS, out(), out(), ws)


# ---------------------------------------------------------------------------------------------------------------------
# pfk_affine_apply_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("residual", [None, "add", "add-relu"])
def test_affine_apply(gpu, relu, residual):
    B, HW, C = 2, 35, 160
    x, res = randn(21, B, HW, C) * 2, randn(22, B, HW, C)
    scale, shift = 1.0 + 0.5 * randn(23, B, C), randn(24, B, C)
    for t in (x, res, scale, shift):
        t[1] = float("nan")                                            # image 1: whatever image 0 reads of it shows
    xs = Rows(B * HW, C, gpu, x.reshape(-1, C).to(gpu), pad=4)        # three distinct row strides
    rs = Rows(B * HW, C, gpu, res.reshape(-1, C).to(gpu), pad=8)
    r_rows = rs.rows if residual else None
    sc, sh = scale.reshape(-1).to(gpu), shift.reshape(-1).to(gpu)
    outs = []
    for _ in range(2):
        out = Rows(B * HW, C, gpu, pad=12)
        torch.ops.pfk.affine_apply(xs.rows, sc, sh, r_rows, out.rows, B, HW, relu, residual == "add-relu")
        out.check_untouched("affine_apply")
        outs.append(out)
    assert same_bits(outs[0].flat, outs[1].flat)                       # (bits: image 1 is NaN)
    got = outs[0].rows.cpu().reshape(B, HW, C)
    ref, mag = affine_apply_ref(x[:1].double(), scale[:1].double(), shift[:1].double(), relu, res[:1].double() if residual else None,
                                residual == "add-relu")
    gates(f"affine_apply relu={relu} residual={residual}", got[:1], ref, mag, 5)       # (n + 2) of the three terms
    assert bool(torch.isnan(got[1]).all())
    inplace = Rows(B * HW, C, gpu, x.reshape(-1, C).to(gpu), pad=4)
    inplace.full[:, C:] = 7.0
    torch.ops.pfk.affine_apply(inplace.rows, sc, sh, r_rows, inplace.rows, B, HW, relu, residual == "add-relu")
    assert torch.equal(inplace.rows[:HW], outs[0].rows[:HW]) and bool((inplace.full[:, C:] == 7.0).all())
    assert bool((inplace.flat[B * HW * inplace.ld:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# pfk_resize_bilinear_pm_f32
# ---------------------------------------------------------------------------------------------------------------------
SIZES = [((7, 9), (14, 18)), ((7, 9), (13, 17)), ((5, 6), (10, 11)), ((1, 2), (2, 3)), ((4, 5), (4, 5))]


@pytest.mark.parametrize("C", [96, 128, 160, 256])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize(gpu, sizes, C):
    (Hi, Wi), (Ho, Wo) = sizes
    B = 2
    x = randn(31 + C, B, C, Hi, Wi)
    x[1] = float("nan")                                                # a tap that crosses into the next image shows in image 0
    src = Rows(B * Hi * Wi, C, gpu, x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(gpu), pad=4)
    outs = []
    for _ in range(2):
        out = Rows(B * Ho * Wo, C, gpu, pad=8)
        torch.ops.pfk.resize_bilinear_pm(src.rows, out.rows, B, Hi, Wi, Ho, Wo)
        out.check_untouched("resize_bilinear_pm")
        outs.append(out)
    assert same_bits(outs[0].flat, outs[1].flat)                       # (bits: image 1 is NaN)
    got = outs[0].rows.cpu().reshape(B, Ho, Wo, C).permute(0, 3, 1, 2)
    ref, mag = resize_ref(x[:1].double(), (Ho, Wo))
    gates(f"resize {sizes} C={C}", got[:1], ref, mag, 6)              # (n + 2) of the four taps
    assert bool(torch.isnan(got[1]).all())
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(got[:1], x[:1])


def test_resize_refuses_downsizing(gpu):
    src, out = torch.zeros(2 * 7 * 9, 96, device=gpu), torch.zeros(2 * 6 * 9, 96, device=gpu)
    with pytest.raises(RuntimeError, match="resize_bilinear_pm"):
        torch.ops.pfk.resize_bilinear_pm(src, out, 2, 7, 9, 6, 9)
    with pytest.raises(RuntimeError, match="resize_bilinear_pm"):
        torch.ops.pfk.resize_bilinear_pm(src, torch.zeros(2 * 7 * 8, 96, device=gpu), 2, 7, 9, 7, 8)


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
INPUTS = {"64x96": (2, 3, 64, 96), "52x76": (2, 3, 52, 76)}      # 52x76: non-integer resize ratios, 4x5 -> 7x10 -> 13x19 -> 26x38


def flat_levels(outs, split):
    return [torch.cat(list(o), 0) if split else o for o in outs]


@functools.lru_cache(maxsize=None)
def standin_forwards(key, size):
    """(the randomised stand-in, its input, its float64 forward, e_ref per level = its own fp32 CPU forward against that)"""
    m = randomize(make(key), SEEDS[key]).eval()
    x = randn(41, *INPUTS[size])
    feed = (lambda t: [t[0:1], t[1:2]]) if m.split_pairs else (lambda t: t)
    with torch.no_grad():
        ref = flat_levels(copy.deepcopy(m).double()(feed(x.double())), m.split_pairs)
        cpu = flat_levels(m(feed(x)), m.split_pairs)
    return m, x, ref, [rel(c, r) for c, r in zip(cpu, ref)]


def engine_for(m, gpu, winograd):
    from ptlflow_amd.ms_encoder import MultiScaleEncoderEngine, describe_multiscale_encoder
    desc = describe_multiscale_encoder(m)
    assert desc is not None
    eng = MultiScaleEncoderEngine(m.state_dict(), desc, gpu)
    eng.winograd = winograd
    return eng


def level_gate(what, outs, ref, e_ref):
    assert len(outs) == len(ref)
    for i, (o, r, e) in enumerate(zip(outs, ref, e_ref)):
        assert tuple(o.shape) == tuple(r.shape)
        got = rel(o, r)
        print(f"RECORD {what} level {i} {tuple(r.shape)}: engine relL2 {got:.2e} | torch fp32 on the CPU (e_ref) {e:.2e}")
        assert bool(torch.isfinite(o).all())
        assert got <= max(4 * e, OP_TOL), f"{what} level {i}: relative L2 {got:.3e}, e_ref {e:.3e}"


@pytest.mark.parametrize("winograd", [False, "always"], ids=["direct", "winograd"])
@pytest.mark.parametrize("size", sorted(INPUTS))
@pytest.mark.parametrize("key", KEYS)
def test_engine_against_the_standin_in_float64(gpu, key, size, winograd):
    m, x, ref, e_ref = standin_forwards(key, size)
    eng = engine_for(m, gpu, winograd)
    outs = eng(x.to(gpu))
    level_gate(f"{key} {size} {'winograd' if winograd else 'direct'}", outs, ref, e_ref)
    again = eng(x.to(gpu))
    assert all(torch.equal(a, b) for a, b in zip(outs, again))          # the same bits on a second run
    assert all(o.permute(0, 2, 3, 1).is_contiguous() for o in outs)     # channels-last views of the row buffers
    if winograd:
        assert any(k.endswith(".ww") for k in eng.w)
        assert not any(k.endswith(".ww") and ("layer4" in k or k.startswith("up_layer") and ".0.conv1" in k) for k in eng.w)


@pytest.mark.parametrize("key", KEYS)
def test_engine_on_the_fixture(gpu, key):
    gold = load_golden()
    rec = gold["encoders"][key]
    m = randomize(make(key), rec["seed"]).eval()
    x = gold["input"].float()
    x = x if m.split_pairs else x[0:1]
    ref = [lv.double() for lv in load_golden_levels(key)]
    with torch.no_grad():
        cpu = flat_levels(m([x[0:1], x[1:2]] if m.split_pairs else x), m.split_pairs)
    e_ref = [rel(c, r) for c, r in zip(cpu, ref)]
    for winograd in (False, "always"):
        level_gate(f"fixture {key} {'winograd' if winograd else 'direct'}", engine_for(m, gpu, winograd)(x.to(gpu)), ref, e_ref)


def test_engine_chunked_forward(gpu):
    m, x, _ref, _e = standin_forwards("msraft_cnet", "52x76")
    eng = engine_for(m, gpu, False)
    assert eng.widest_row == 256                                        # MS-RAFT+'s cnet: 256 floats at half resolution
    assert engine_for(standin_forwards("ccmr_fnet", "52x76")[0], gpu, False).widest_row == 128
    whole = eng(x.to(gpu))
    eng.max_matrix_bytes = 26 * 38 * 256 * 4                            # one image's widest buffer: the two images split
    assert eng._max_batch(26, 38) == 1
    parts = eng(x.to(gpu))
    for i, (a, b) in enumerate(zip(parts, whole)):
        scale_close(a, b, f"chunked level {i}")


# ---------------------------------------------------------------------------------------------------------------------
# the seam
# ---------------------------------------------------------------------------------------------------------------------
def structure(out):
    return [(type(o), [tuple(t.shape) for t in o]) if isinstance(o, (tuple, list)) else tuple(o.shape) for o in out]


@pytest.mark.parametrize("family", ["ccmr", "ccmrp", "msraft"])
def test_seam_option_on_against_off(gpu, family):
    from ptlflow_amd import patch
    from ptlflow_amd.ms_encoder import PfkMultiScaleEncoder
    register()
    model = MsModel(family).to(gpu).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    keys = list(model.state_dict())
    a, b = randn(51, 2, 3, 52, 76).to(gpu), randn(52, 2, 3, 52, 76).to(gpu)
    with torch.no_grad():
        off_f, off_c = model(a, b)
    patch.accelerate(model, multiscale_encoders=True)
    assert isinstance(model.fnet, PfkMultiScaleEncoder) and isinstance(model.cnet, PfkMultiScaleEncoder)
    assert list(model.state_dict()) == keys
    with torch.no_grad():
        on_f, on_c = model(a, b)
        model(a, b)
    assert (model.fnet.engine_calls, model.cnet.engine_calls, model.fnet.fallback_calls, model.cnet.fallback_calls) == (2, 2, 0, 0)
    assert structure(on_f) == structure(off_f) and structure(on_c) == structure(off_c)
    for i, (x, y) in enumerate(zip(on_f, off_f)):
        for j in (0, 1):
            scale_close(x[j], y[j], f"{family} fnet level {i} image {j + 1}", BLOCK_TOL)
    for i, (x, y) in enumerate(zip(on_c, off_c)):
        scale_close(x, y, f"{family} cnet level {i}", BLOCK_TOL)
    patch.restore(model)
    assert not isinstance(model.fnet, PfkMultiScaleEncoder) and list(model.state_dict()) == keys


def test_seam_falls_back(gpu):
    """grad mode, train mode, autocast and a .half() input reach the reference module — its `forward` is replaced by a recorder here,
    so that what is tested is the dispatch (torch would tune every convolution of the module once more per mode and dtype)"""
    from ptlflow_amd import patch
    register()
    model = MsModel("ccmr").to(gpu).eval()
    patch.accelerate(model, multiscale_encoders=True)
    seen = []
    for enc in (model.fnet, model.cnet):
        ref = enc._ref[0]
        ref.forward = lambda x, ref=ref: seen.append((ref, x)) or "the reference module's answer"
    fallback = ("the reference module's answer",) * 2
    a, b = randn(53, 1, 3, 32, 48).to(gpu), randn(54, 1, 3, 32, 48).to(gpu)
    counts = lambda: (model.fnet.engine_calls, model.fnet.fallback_calls, model.cnet.engine_calls, model.cnet.fallback_calls)  # noqa: E731
    assert model(a, b) == fallback                                      # grad mode with parameters that require grad
    assert counts() == (0, 1, 0, 1) and len(seen) == 2
    assert seen[0][0] is model.fnet._ref[0] and seen[0][1][0] is a and seen[0][1][1] is b and seen[1][1] is a
    for p in model.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        served = model(a, b)
    assert counts() == (1, 1, 1, 1) and len(seen) == 2 and torch.is_tensor(served[1][0])
    model.train()
    with torch.no_grad():
        assert model(a, b) == fallback
    assert counts() == (1, 2, 1, 2) and model.fnet._ref[0].training
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert model(a, b) == fallback
    assert counts() == (1, 3, 1, 3)
    with torch.no_grad():
        again = model(a, b)
        assert model(a.half(), b.half()) == fallback                    # a .half() input
    assert counts() == (2, 4, 2, 4) and len(seen) == 8
    assert all(torch.equal(x, y) for x, y in zip(again[1], served[1]))
