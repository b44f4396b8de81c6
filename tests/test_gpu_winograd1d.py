"""`pfk_conv1d_wino_f32` (torch.ops.pfk.conv2d_wino1d): the SepConvGRU's 1x5 / 5x1 gate convolutions as 1-D Winograd F(4,5).

Every result is compared against float64 restated on what the launch consumed (`ref_zr` / `ref_q` of tests/op_refs.py).
Gates: the gate epilogues' own — z, r*h, h inside 3e-5 + 2e-5 |ref| — and for LINEAR |err| <= 2e-5 (1 + |ref|).  A gate relative to
the direct kernel's error is deliberately not used: F(4,5)'s pre-activation error is 6 to 8 times the direct form's while staying
at 6e-6 absolute (tests/test_wino1d_packing.py measures it on the CPU)."""
import math

import pytest
import torch

from op_gate import close32
from op_refs import conv64, ref_q, ref_zr

pytestmark = pytest.mark.gpu

EPI_LINEAR, EPI_GRU_ZR, EPI_GRU_Q = 0, 1, 2
WIDTHS = {"sepconv_1x5": ("raft", 1, 5), "sepconv_5x1": ("raft", 5, 1), "gma_1x5": ("gma", 1, 5), "gma_5x1": ("gma", 5, 1)}
B, H, W = 2, 23, 31          # M = 1426: no multiple of a block's 128 outputs, partial tiles in both orientations (31 = 7*4 + 3, 23 = 5*4 + 3)
SENTINEL = 7.0               # no gate output can take it: sigmoid < 1, |r * h| < 1
PAD_ROWS = 64


def _spec(model):
    from ptlflow_amd.update import basic_spec, gma_spec
    return {"raft": basic_spec, "gma": gma_spec}[model]()


# ---------------------------------------------------------------------------------------------------------------- the gate epilogues
@pytest.mark.parametrize("with_ctx", [True, False], ids=["ctx", "noctx"])
@pytest.mark.parametrize("wset", list(WIDTHS))
def test_gates_ragged(gpu, wset, with_ctx):
    """z|r, then q on what z|r stored, on the engine's widths and slices: h = act[:, :Ch], motion = act[:, Ch + Ci:]"""
    from ptlflow_amd.packing import pack_wino1d_weight
    model, kh, kw = WIDTHS[wset]
    spec = _spec(model)
    Ch, Ci, row = spec.hidden, spec.context, spec.hx_channels
    real, width = spec.x_channels - Ci, row - Ch - Ci
    M, shape, k, reals = B * H * W, (B, H, W), (kh, kw), [Ch, real]
    g = torch.Generator().manual_seed(41)
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    K = Ch + real
    wzr, wq = rnd(2 * Ch, K, kh, kw) / math.sqrt(K * 5), rnd(Ch, K, kh, kw) / math.sqrt(K * 5)
    bzr, bq = (rnd(2 * Ch) * 0.1).cuda(), (rnd(Ch) * 0.1).cuda()
    act = rnd(M, row)
    act[:, :Ch] = torch.tanh(rnd(M, Ch))
    act = act.cuda()
    segs = [(0, Ch, Ch), (Ch, real, width)]
    pzr, pq = pack_wino1d_weight(wzr, segs).cuda(), pack_wino1d_weight(wq, segs).cuda()
    ctx, bufs = {"zr": None, "q": None}, {}
    if with_ctx:      # context rows inside wider rows (residual_ld != cout) with sentinel neighbours
        for name, cout in (("zr", 2 * Ch), ("q", Ch)):
            bufs[name] = torch.full((M, cout + 16), SENTINEL, device="cuda")
            bufs[name][:, 8: 8 + cout] = (rnd(M, cout) * 0.5).cuda()
            ctx[name] = bufs[name][:, 8: 8 + cout]
    bufs0 = {n: b.clone() for n, b in bufs.items()}
    z = torch.full((M + PAD_ROWS, Ch), SENTINEL, device="cuda")
    rh = torch.full((M + PAD_ROWS, Ch), SENTINEL, device="cuda")
    act0 = act.clone()
    motion = act[:, Ch + Ci:]
    torch.ops.pfk.conv2d_wino1d([act[:, :Ch], motion], B, H, W, kh, kw, pzr, bzr, 2 * Ch, EPI_GRU_ZR, False, 1.0, None, act[:, :Ch], z, rh,
                                ctx["zr"])
    torch.cuda.synchronize()
    assert torch.equal(act, act0), "z|r wrote into the [h | context | motion] rows"
    assert bool((z[M:] == SENTINEL).all()) and bool((rh[M:] == SENTINEL).all()), "z|r wrote rows past M"
    z_ref, rh_ref = ref_zr([act0[:, :Ch], act0[:, Ch + Ci:]], reals, wzr, bzr, ctx["zr"], act0[:, :Ch], shape, k)
    rz, rr = close32(z[:M], z_ref, "z"), close32(rh[:M], rh_ref, "r*h")
    z1, rh1 = z.clone(), rh.clone()
    # the same launch again (the gate epilogues' own store path: parked in LDS, walked as rows): identical bits
    z.fill_(SENTINEL), rh.fill_(SENTINEL)
    torch.ops.pfk.conv2d_wino1d([act[:, :Ch], motion], B, H, W, kh, kw, pzr, bzr, 2 * Ch, EPI_GRU_ZR, False, 1.0, None, act[:, :Ch], z, rh,
                                ctx["zr"])
    torch.cuda.synchronize()
    assert torch.equal(z, z1) and torch.equal(rh, rh1), "the same z|r launch gave other bits"
    torch.ops.pfk.conv2d_wino1d([rh[:M], motion], B, H, W, kh, kw, pq, bq, Ch, EPI_GRU_Q, False, 1.0, None, act[:, :Ch], z, None, ctx["q"])
    torch.cuda.synchronize()
    assert torch.equal(act[:, Ch:], act0[:, Ch:]), "q wrote outside h"
    assert torch.equal(z, z1) and torch.equal(rh, rh1), "q wrote into z / r*h"
    h_ref = ref_q([rh1[:M], act0[:, Ch + Ci:]], reals, wq, bq, ctx["q"], z1[:M], act0[:, :Ch], shape, k)
    rq = close32(act[:, :Ch], h_ref, "h")
    h1 = act[:, :Ch].clone()
    act[:, :Ch] = act0[:, :Ch]      # q updates h in place: the same launch again from the same h
    torch.ops.pfk.conv2d_wino1d([rh[:M], motion], B, H, W, kh, kw, pq, bq, Ch, EPI_GRU_Q, False, 1.0, None, act[:, :Ch], z, None, ctx["q"])
    torch.cuda.synchronize()
    assert torch.equal(act[:, :Ch], h1), "the same q launch gave other bits"
    for n in bufs:
        assert torch.equal(bufs[n], bufs0[n]), "wrote into the context rows or their neighbours"
    print(f"[ratio] wino1d {wset} {'ctx' if with_ctx else 'noctx'} z={rz:.3f} rh={rr:.3f} h={rq:.3f}")


# ---------------------------------------------------------------------------------------------------------------- LINEAR
def _linear(b, h, w, kh, kw, cin, cout, relu=False, scale=1.0, seed=0, src_ld=None, src_off=0, twice=False):
    """one LINEAR launch into a sentinel-framed out buffer; returns the worst err / (2e-5 (1 + |ref|))"""
    from ptlflow_amd.packing import pack_wino1d_weight
    M = b * h * w
    g = torch.Generator().manual_seed(seed)
    wt = torch.randn(cout, cin, kh, kw, generator=g) / math.sqrt(cin * 5)
    bias = (torch.randn(cout, generator=g) * 0.1).cuda()
    buf = torch.randn(M, src_ld or cin, generator=g).cuda()
    src = buf[:, src_off: src_off + cin]
    ww = pack_wino1d_weight(wt, [(0, cin, cin)]).cuda()
    ncol = (cout + 127) // 128 * 128 + 16
    frame = torch.full((M + PAD_ROWS, ncol), SENTINEL, device="cuda")
    out = frame[:M, :cout]
    buf0 = buf.clone()
    torch.ops.pfk.conv2d_wino1d([src], b, h, w, kh, kw, ww, bias, cout, EPI_LINEAR, relu, scale, out)
    torch.cuda.synchronize()
    assert torch.equal(buf, buf0), "wrote into its source"
    assert bool((frame[M:] == SENTINEL).all()), "wrote rows past M"
    assert bool((frame[:, cout:] == SENTINEL).all()), "wrote columns past cout"
    v = conv64([src], [cin], wt, bias, None, b, h, w, kh, kw)
    if relu:
        v = torch.relu(v)
    v = v * scale
    err = (out.double().cpu() - v).abs()
    lim = 2e-5 * (1 + v.abs())
    assert bool((err <= lim).all()), f"{int((err > lim).sum())} of {err.numel()} outside 2e-5 (1 + |ref|), worst {float((err / lim).max()):.2f}"
    if twice:
        first = frame.clone()
        frame.fill_(SENTINEL)
        torch.ops.pfk.conv2d_wino1d([src], b, h, w, kh, kw, ww, bias, cout, EPI_LINEAR, relu, scale, out)
        torch.cuda.synchronize()
        assert torch.equal(frame, first), "the same launch gave other bits"
    return float((err / lim).max())


@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (1, 4), (1, 5), (3, 1), (4, 4), (5, 9), (7, 2)])
def test_linear_tiny_and_odd_grids(gpu, h, w, kh, kw):
    _linear(1, h, w, kh, kw, 32, 128, seed=h * 16 + w)


@pytest.mark.parametrize("relu,scale", [(False, 1.0), (True, 0.25), (False, -2.0)])
def test_linear_relu_scale(gpu, relu, scale):
    _linear(2, 9, 13, 1, 5, 64, 128, relu=relu, scale=scale, seed=3)
    _linear(2, 9, 13, 5, 1, 64, 128, relu=relu, scale=scale, seed=4)


@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
def test_linear_strided_source_slice_and_cout_126(gpu, kh, kw):
    """a channel slice of wider rows as the source; cout 126: the two pad columns of the block are not written; twice: same bits"""
    _linear(2, 23, 31, kh, kw, 40, 126, src_ld=72, src_off=24, seed=5, twice=True)


def test_refused_arguments_raise_and_write_nothing(gpu):
    from ptlflow_amd.packing import pack_wino1d_weight
    M = 2 * 5 * 6
    src = torch.randn(M, 32, device="cuda")
    wt = torch.randn(128, 32, 1, 5)
    ww = pack_wino1d_weight(wt, [(0, 32, 32)]).cuda()
    out = torch.full((M, 128), SENTINEL, device="cuda")
    op = torch.ops.pfk.conv2d_wino1d
    with pytest.raises(RuntimeError):       # 3x3 is the 2-D kernel's
        op([src], 2, 5, 6, 3, 3, ww, None, 128, EPI_LINEAR, False, 1.0, out)
    with pytest.raises(RuntimeError):       # channels not a multiple of 8
        op([src[:, :28]], 2, 5, 6, 1, 5, ww, None, 128, EPI_LINEAR, False, 1.0, out)
    with pytest.raises(RuntimeError):       # a weight of another size
        op([src], 2, 5, 6, 1, 5, ww[:-8], None, 128, EPI_LINEAR, False, 1.0, out)
    with pytest.raises(RuntimeError):       # rows of another grid
        op([src], 2, 5, 7, 1, 5, ww, None, 128, EPI_LINEAR, False, 1.0, out)
    with pytest.raises(RuntimeError):       # a gate epilogue without its state
        op([src], 2, 5, 6, 1, 5, ww, None, 128, EPI_GRU_Q, False, 1.0, None, None, None)
    with pytest.raises(RuntimeError):       # LINEAR without out
        op([src], 2, 5, 6, 1, 5, ww, None, 128, EPI_LINEAR, False, 1.0, None)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- engine
def test_engine_rule(gpu):
    """UpdateEngine (fp32, raft) bound at the smallest production grid at or above WINO1D_MIN_PIXELS: gru() through the F(4,5)
    launches agrees with the direct kernels inside the gate, and `winograd=False` is the direct path bit for bit."""
    from ptlflow_amd import update
    from ptlflow_amd.synth import synth_update_block_params
    from ptlflow_amd.update import UpdateEngine
    spec = _spec("raft")
    h, w = 55, 128
    b = -(-update.WINO1D_MIN_PIXELS // (h * w))
    assert b * h * w >= update.WINO1D_MIN_PIXELS > 20480
    P = synth_update_block_params(spec, seed=17)
    eng = UpdateEngine(P, spec, gpu)
    eng.bind(b, h, w)
    Ch, Ci, real = spec.hidden, spec.context, spec.x_channels - spec.context
    g = torch.Generator().manual_seed(29)
    net = torch.tanh(torch.randn(b, Ch, h, w, generator=g)).to(gpu)
    inp = torch.relu(torch.randn(b, Ci, h, w, generator=g)).to(gpu)
    motion = torch.randn(b * h * w, real, generator=g).to(gpu)

    def run(winograd, spy=None):
        eng.winograd = winograd
        eng.load_state(net, inp)
        eng.hx[:, Ch + Ci: Ch + Ci + real] = motion
        if spy is not None:
            orig = eng.ops
            eng.ops = spy(orig)
        try:
            eng.gru()
        finally:
            if spy is not None:
                eng.ops = orig
        torch.cuda.synchronize()
        return eng.hx[:, :Ch].clone()

    class Count:
        def __init__(self, ops):
            self._ops, self.names = ops, names
        def __getattr__(self, name):
            self.names.append(name)
            return getattr(self._ops, name)

    names = []
    h_w = run(True, Count)
    assert names == ["conv2d_wino1d"] * 4, names
    names.clear()
    h_d = run(False, Count)
    assert names == ["conv2d"] * 4, names
    # the direct path restated without the engine's rule: the same four launches through torch.ops.pfk.conv2d
    eng.load_state(net, inp)
    eng.hx[:, Ch + Ci: Ch + Ci + real] = motion
    rest = eng.hx[:, Ch + Ci:]
    for kh, kw, sfx in spec.gru_passes:
        torch.ops.pfk.conv2d([eng.hx[:, :Ch], rest], b, h, w, kh, kw, eng.w[f"zr{sfx}.w"], None, 2 * Ch, EPI_GRU_ZR, False, 1.0, None,
                             eng.h_view, eng.zbuf, eng.rh, eng.workspace, eng.ctx["zr" + sfx])
        torch.ops.pfk.conv2d([eng.rh, rest], b, h, w, kh, kw, eng.w[f"q{sfx}.w"], None, Ch, EPI_GRU_Q, False, 1.0, None,
                             eng.h_view, eng.zbuf, None, eng.workspace, eng.ctx["q" + sfx])
    torch.cuda.synchronize()
    assert torch.equal(eng.hx[:, :Ch], h_d), "winograd=False is not the direct path"
    r = close32(h_w, h_d.double().cpu(), "h through F(4,5) against h through the direct kernels")
    print(f"[engine] batch {b}: worst |h_winograd - h_direct| / (3e-5 + 2e-5 |h|) = {r:.3f}")
