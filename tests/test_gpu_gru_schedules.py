"""The ConvGRU gate epilogues (PFK_EPI_GRU_ZR / PFK_EPI_GRU_Q, include/pfk.h) on every schedule the two conv launchers can pick for
them, against fp64.

Each launch is restated in float64 on exactly what it consumed — its sources, packed weight, bias, h and context rows, and for q the z
and r*h the z|r launch itself stored — so every launch is judged on its own: a rounding flip in z|r can neither excuse nor hide an
error in q.
  fp32 (pfk_conv2d_f32)  z, r*h, h: |err| <= 3e-5 + 2e-5 |ref|  (the gate of test_gpu_kernels.py::test_gru)
  K8b  (pfk_conv2d_b16)  z, r*h (bf16): within one bf16 ulp of the fp64 value + 2^-16;  h (fp32): 3e-5 + 2e-5 |ref|;
                         the h twin: bf16(h) bit for bit
Every launch must also leave alone what is not its output: the other columns of the [h | context | motion] rows h is a slice of,
sentinel rows past M in z / r*h, the context rows and their neighbours.

  1. The forced-schedule matrix (F32_CFGS, B16_CFGS) on a ragged shape (M = 1426 is no multiple of 64, 128 or 256) over the three
     width sets the engine launches (WIDTHS), with and without the context term; K8b's q with and without the h twin; K8b's LINEAR
     epilogue with fp32 / bf16 residual rows on the same tiles.
  2. The engine's own z|r and q launches (UpdateEngine.gru) at the shapes bench and users run, on the launchers' heuristic.  The
     schedule each launch is meant to take is in the case id; on the fp32 path the workspace shows it: a stream-K launch writes
     partial tiles into it, a tile grid never touches it."""
import math

import pytest
import torch

from op_gate import arm, close32, within_ulp, ws_after
from op_refs import conv64, ref_q, ref_zr

pytestmark = pytest.mark.gpu

EPI_LINEAR, EPI_GRU_ZR, EPI_GRU_Q = 0, 1, 2
BF = torch.bfloat16

# every schedule the launchers can return for the gate epilogues (pfk_gemm.hip::launch, pfk_gemm_b16.hip::launch_b16)
F32_CFGS = (0, 4, 10, 11, 9)      # 9 = stream-K, forced with a zero-filled pfk_conv_workspace_bytes() workspace
F32_LINEAR_ONLY = (14, 15)        # the 128x96 tiles: LINEAR only, must refuse a gate epilogue
B16_CFGS = (1, 2, 3, 4, 6, 8, 9)
B16_NO_Q = (6,)                   # 256x256: z|r and LINEAR only, must refuse q
# width sets: update-block spec, GRU pass (kh, kw).  Widths and slices are the engine's: h = act[:, :Ch], the motion source =
# act[:, Ch + Ci:] (motion features [| aggregated ones] | pad), with Ci the context columns the hoisted launches skip
WIDTHS = {
    "sepconv_1x5": ("raft", 1, 5),     # SepConvGRU, Ch 128, 128 motion channels
    "sepconv_5x1": ("raft", 5, 1),
    "convgru_3x3": ("small", 3, 3),    # raft_small's ConvGRU, Ch 96: 82 motion channels in an 84 (fp32) / 88 (bf16) wide slice
    "gma_1x5": ("gma", 1, 5),          # GMA: [h | motion | aggregate], 256 channels behind the context
}
B, H, W = 2, 23, 31
SENTINEL = 7.0      # no gate output can take it: sigmoid < 1, |r * h| < 1
PAD_ROWS = 64


def _spec(model):
    from ptlflow_amd.update import basic_spec, gma_spec, small_spec
    return {"raft": basic_spec, "small": small_spec, "gma": gma_spec}[model]()


def _widths(spec, b16):
    """Ch, Ci, real motion channels, motion slice width, act row width"""
    from ptlflow_amd.packing import round_up
    row = round_up(spec.hidden + spec.x_channels, 8) if b16 else spec.hx_channels
    Ch, Ci = spec.hidden, spec.context
    return Ch, Ci, spec.x_channels - Ci, row - Ch - Ci, row


def _report(tag, **ratios):
    print(f"[ratio] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


# ---------------------------------------------------------------------------------------------------------------- 1. forced schedules
def _inputs(wset, b16, with_ctx, seed):
    from ptlflow_amd.packing import pack_conv_weight
    model, kh, kw = WIDTHS[wset]
    Ch, Ci, real, width, row = _widths(_spec(model), b16)
    M = B * H * W
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    K = Ch + real
    t = {"Ch": Ch, "Ci": Ci, "real": real, "k": (kh, kw), "M": M}
    t["wzr"], t["wq"] = rnd(2 * Ch, K, kh, kw) / math.sqrt(K * kh * kw), rnd(Ch, K, kh, kw) / math.sqrt(K * kh * kw)
    t["bzr"], t["bq"] = rnd(2 * Ch) * 0.1, rnd(Ch) * 0.1
    # [h | context | motion | pad] rows: everything but h is finite garbage the launches must neither write nor let into a result
    # through the pad columns (their packed weights are zero)
    act = rnd(M, row)
    act[:, :Ch] = torch.tanh(rnd(M, Ch))
    ctx_zr, ctx_q = rnd(M, 2 * Ch) * 0.5, rnd(M, Ch) * 0.5
    segs = [(0, Ch, Ch), (Ch, real, width)]
    if b16:
        t["wzr"], t["wq"] = t["wzr"].to(BF).float(), t["wq"].to(BF).float()
        t["pzr"] = pack_conv_weight(t["wzr"], segs, kpad=64).to(BF).cuda()
        t["pq"] = pack_conv_weight(t["wq"], segs, kpad=64).to(BF).cuda()
        t["hx32"] = rnd(M, _widths(_spec(model), False)[4]).cuda()      # the engine's fp32 hx: h is its first Ch columns
        t["hx32"][:, :Ch] = act[:, :Ch].cuda()
        t["act"] = act.to(BF).cuda()                                      # its bf16 twin: the convolutions' operand
        ctx_zr, ctx_q = ctx_zr.to(BF), ctx_q.to(BF)
    else:
        t["pzr"], t["pq"] = pack_conv_weight(t["wzr"], segs).cuda(), pack_conv_weight(t["wq"], segs).cuda()
        t["act"] = act.cuda()
    dt = BF if b16 else torch.float32
    # context rows inside wider rows (residual_ld != cout) with sentinel neighbours
    t["ctx_zr"] = t["ctx_q"] = None
    if with_ctx:
        for name, c, cout in (("ctx_zr", ctx_zr, 2 * Ch), ("ctx_q", ctx_q, Ch)):
            buf = torch.full((M, cout + 16), SENTINEL, device="cuda", dtype=dt)
            buf[:, 8: 8 + cout] = c.cuda()
            t[name + "_buf"], t[name] = buf, buf[:, 8: 8 + cout]
    # z / r*h with sentinel rows past M
    t["z"] = torch.full((M + PAD_ROWS, Ch), SENTINEL, device="cuda", dtype=dt)
    t["rh"] = torch.full((M + PAD_ROWS, Ch), SENTINEL, device="cuda", dtype=dt)
    return t


def _pad_rows_untouched(t):
    M = t["M"]
    for n in ("z", "rh"):
        assert bool((t[n][M:] == SENTINEL).all()), f"wrote {n} rows past M"


def _run_f32(t, epi, cfg):
    Ch = t["Ch"]
    act = t["act"]
    motion = act[:, Ch + t["Ci"]:]
    ws = None
    if cfg == 9:
        ws = torch.zeros(torch.ops.pfk.conv_workspace_bytes(), device="cuda", dtype=torch.uint8)
        arm(ws)
    if epi == EPI_GRU_ZR:
        args = ([act[:, :Ch], motion], t["pzr"], t["bzr"], 2 * Ch, t["z"], t["rh"], t["ctx_zr"])
    else:
        args = ([t["rh"][: t["M"]], motion], t["pq"], t["bq"], Ch, t["z"], None, t["ctx_q"])
    srcs, wpk, bias, cout, z, rh, res = args
    torch.ops.pfk.debug_set_tile(cfg)
    try:
        torch.ops.pfk.conv2d(srcs, B, H, W, *t["k"], wpk, bias.cuda(), cout, epi, False, 1.0, None,
                             act[:, :Ch], z, rh, ws, res)
    finally:
        torch.ops.pfk.debug_set_tile(-1)
    if ws is not None:
        ws_after(ws, True, f"cfg 9 epilogue {epi}")


@pytest.mark.parametrize("with_ctx", [True, False], ids=["ctx", "noctx"])
@pytest.mark.parametrize("wset", list(WIDTHS))
@pytest.mark.parametrize("cfg", F32_CFGS)
def test_f32_gates_every_schedule(gpu, cfg, wset, with_ctx):
    t = _inputs(wset, False, with_ctx, seed=100 + cfg)
    Ch, M, reals, shape = t["Ch"], t["M"], [t["Ch"], t["real"]], (B, H, W)
    act0, ctx0 = t["act"].clone(), [t[n].clone() for n in ("ctx_zr_buf", "ctx_q_buf") if n in t]
    _run_f32(t, EPI_GRU_ZR, cfg)
    torch.cuda.synchronize()
    assert torch.equal(t["act"], act0), "z|r wrote into the [h | context | motion] rows"
    _pad_rows_untouched(t)
    zr_in = [act0[:, :Ch], act0[:, Ch + t["Ci"]:]]
    z_ref, rh_ref = ref_zr(zr_in, reals, t["wzr"], t["bzr"], t["ctx_zr"], act0[:, :Ch], shape, t["k"])
    rz = close32(t["z"][:M], z_ref, "z")
    rr = close32(t["rh"][:M], rh_ref, "r*h")
    z1, rh1 = t["z"].clone(), t["rh"].clone()
    _run_f32(t, EPI_GRU_Q, cfg)
    torch.cuda.synchronize()
    assert torch.equal(t["act"][:, Ch:], act0[:, Ch:]), "q wrote outside h"
    assert torch.equal(t["z"], z1) and torch.equal(t["rh"], rh1), "q wrote into z / r*h"
    q_in = [rh1[:M], act0[:, Ch + t["Ci"]:]]
    h_ref = ref_q(q_in, reals, t["wq"], t["bq"], t["ctx_q"], z1[:M], act0[:, :Ch], shape, t["k"])
    rq = close32(t["act"][:, :Ch], h_ref, "h")
    if with_ctx:
        assert torch.equal(t["ctx_zr_buf"], ctx0[0]) and torch.equal(t["ctx_q_buf"], ctx0[1]), "wrote into the context rows"
    _report(f"f32 cfg {cfg} {wset}", z=rz, rh=rr, h=rq)


@pytest.mark.parametrize("cfg", F32_LINEAR_ONLY)
@pytest.mark.parametrize("epi", [EPI_GRU_ZR, EPI_GRU_Q], ids=["zr", "q"])
def test_f32_linear_only_tiles_refuse_the_gates(gpu, cfg, epi):
    t = _inputs("sepconv_1x5", False, True, seed=7)
    act0, z0, rh0 = t["act"].clone(), t["z"].clone(), t["rh"].clone()
    with pytest.raises(RuntimeError):
        _run_f32(t, epi, cfg)
    torch.cuda.synchronize()
    assert torch.equal(t["act"], act0) and torch.equal(t["z"], z0) and torch.equal(t["rh"], rh0), "a refused launch wrote"


def _run_b16(t, epi, cfg, with_twin=True):
    Ch = t["Ch"]
    act = t["act"]
    motion = act[:, Ch + t["Ci"]:]
    torch.ops.pfk.debug_set_b16(cfg)
    try:
        if epi == EPI_GRU_ZR:
            torch.ops.pfk.conv2d_b16([act[:, :Ch], motion], B, H, W, *t["k"], t["pzr"], t["bzr"].cuda(), 2 * Ch, EPI_GRU_ZR, False, 1.0,
                                     None, None, act[:, :Ch], t["z"], t["rh"], t["ctx_zr"])
        else:
            torch.ops.pfk.conv2d_b16([t["rh"][: t["M"]], motion], B, H, W, *t["k"], t["pq"], t["bq"].cuda(), Ch, EPI_GRU_Q, False, 1.0,
                                     None, t["hx32"][:, :Ch], act[:, :Ch] if with_twin else None, t["z"], None, t["ctx_q"])
    finally:
        torch.ops.pfk.debug_set_b16(0)


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "notwin"])
@pytest.mark.parametrize("with_ctx", [True, False], ids=["ctx", "noctx"])
@pytest.mark.parametrize("wset", list(WIDTHS))
@pytest.mark.parametrize("cfg", B16_CFGS)
def test_b16_gates_every_schedule(gpu, cfg, wset, with_ctx, twin):
    t = _inputs(wset, True, with_ctx, seed=200 + cfg)
    Ch, M, reals, shape = t["Ch"], t["M"], [t["Ch"], t["real"]], (B, H, W)
    act0, hx0 = t["act"].clone(), t["hx32"].clone()
    ctx0 = [t[n].clone() for n in ("ctx_zr_buf", "ctx_q_buf") if n in t]
    _run_b16(t, EPI_GRU_ZR, cfg)
    torch.cuda.synchronize()
    assert torch.equal(t["act"], act0) and torch.equal(t["hx32"], hx0), "z|r wrote into the [h | context | motion] rows"
    _pad_rows_untouched(t)
    zr_in = [act0[:, :Ch], act0[:, Ch + t["Ci"]:]]
    z_ref, rh_ref = ref_zr(zr_in, reals, t["wzr"], t["bzr"], t["ctx_zr"], act0[:, :Ch], shape, t["k"])
    rz = within_ulp(t["z"][:M], z_ref, 2.0 ** -16, "z")
    rr = within_ulp(t["rh"][:M], rh_ref, 2.0 ** -16, "r*h")
    z1, rh1 = t["z"].clone(), t["rh"].clone()
    if cfg in B16_NO_Q:
        with pytest.raises(RuntimeError):
            _run_b16(t, EPI_GRU_Q, cfg, twin)
        torch.cuda.synchronize()
        assert torch.equal(t["hx32"], hx0) and torch.equal(t["act"], act0), "a refused q launch wrote h or its twin"
        _report(f"b16 cfg {cfg} {wset}", z=rz, rh=rr)
        return
    _run_b16(t, EPI_GRU_Q, cfg, twin)
    torch.cuda.synchronize()
    assert torch.equal(t["hx32"][:, Ch:], hx0[:, Ch:]) and torch.equal(t["act"][:, Ch:], act0[:, Ch:]), "q wrote outside h"
    assert torch.equal(t["z"], z1) and torch.equal(t["rh"], rh1), "q wrote into z / r*h"
    q_in = [rh1[:M], act0[:, Ch + t["Ci"]:]]
    h_ref = ref_q(q_in, reals, t["wq"], t["bq"], t["ctx_q"], z1[:M], hx0[:, :Ch], shape, t["k"])
    rq = close32(t["hx32"][:, :Ch], h_ref, "h")
    if twin:
        assert torch.equal(t["act"][:, :Ch], t["hx32"][:, :Ch].to(BF)), "the h twin is not bf16(h)"
    else:
        assert torch.equal(t["act"][:, :Ch], act0[:, :Ch]), "q without a twin wrote one"
    if with_ctx:
        assert torch.equal(t["ctx_zr_buf"], ctx0[0]) and torch.equal(t["ctx_q_buf"], ctx0[1]), "wrote into the context rows"
    _report(f"b16 cfg {cfg} {wset}", z=rz, rh=rr, h=rq)


@pytest.mark.parametrize("relu2", [False, True], ids=["", "relu2"])
@pytest.mark.parametrize("res_dtype", [torch.float32, BF], ids=["res32", "res16"])
@pytest.mark.parametrize("wset", list(WIDTHS))
@pytest.mark.parametrize("cfg", B16_CFGS)
def test_b16_linear_residual_every_schedule(gpu, cfg, wset, res_dtype, relu2):
    """K8b LINEAR with residual rows on the same tiles: out = [relu](residual + scale * relu(conv + bias)), written in the residual's
    precision (bf16 rows: 4-column stores, not the 16-byte form of residual-free launches)"""
    t = _inputs(wset, True, False, seed=300 + cfg)
    Ch, M, reals, shape = t["Ch"], t["M"], [t["Ch"], t["real"]], (B, H, W)
    cout = 2 * Ch
    g = torch.Generator().manual_seed(cfg)
    res = torch.randn(M, cout, generator=g).to(res_dtype)
    rbuf = torch.full((M, cout + 16), SENTINEL, device="cuda", dtype=res_dtype)
    rbuf[:, 8: 8 + cout] = res.cuda()
    obuf = torch.full((M + PAD_ROWS, cout + 16), SENTINEL, device="cuda", dtype=res_dtype)
    rbuf0, act0 = rbuf.clone(), t["act"].clone()
    torch.ops.pfk.debug_set_b16(cfg)
    try:
        torch.ops.pfk.conv2d_b16([t["act"][:, :Ch], t["act"][:, Ch + t["Ci"]:]], B, H, W, *t["k"], t["pzr"], t["bzr"].cuda(), cout,
                                 EPI_LINEAR, True, 0.5, obuf[:M, 8: 8 + cout], None, None, None, None, rbuf[:, 8: 8 + cout], 1, relu2)
    finally:
        torch.ops.pfk.debug_set_b16(0)
    torch.cuda.synchronize()
    v = conv64([act0[:, :Ch], act0[:, Ch + t["Ci"]:]], reals, t["wzr"], t["bzr"], None, *shape, *t["k"])
    ref = res.double() + 0.5 * v.clamp_min(0)
    if relu2:
        ref = ref.clamp_min(0)
    got = obuf[:M, 8: 8 + cout]
    r = within_ulp(got, ref, 2.0 ** -16, "out") if res_dtype == BF else close32(got, ref, "out")
    assert bool((obuf[M:] == SENTINEL).all()) and bool((obuf[:, :8] == SENTINEL).all()) and bool((obuf[:, 8 + cout:] == SENTINEL).all()), \
        "wrote outside its [M, cout] view"
    assert torch.equal(rbuf, rbuf0) and torch.equal(t["act"], act0), "wrote into an input"
    _report(f"b16 cfg {cfg} {wset} linear", out=r)


# ---------------------------------------------------------------------------------------------------------------- 2. production sites
# path, model, B, H, W, expected schedule of the z|r and the q launches ("sk" = stream-K)
PRODUCTION = [
    ("f32", "raft", 1, 55, 128, "cfg4", "cfg4"),
    ("f32", "raft", 8, 55, 128, "cfg11", "cfg10"),
    ("f32", "gma", 1, 55, 128, "sk", "cfg4"),          # z|r: 440 tiles x 60 K-steps
    ("f32", "raft", 1, 128, 160, "cfg10", "sk"),       # q: 640 tiles x 40 K-steps
    ("b16", "raft", 1, 55, 128, "cfg4", "cfg4"),
    ("b16", "raft", 8, 55, 128, "cfg6", "cfg1"),
    ("b16", "gma", 4, 55, 128, "cfg6", "cfg4"),
    ("b16", "raft", 8, 47, 156, "cfg6", "cfg1"),       # KITTI's grid: the last 256-row tile is partial
    ("b16", "small", 8, 55, 128, "cfg6", "cfg1"),      # z|r: 192 outputs (64 pad columns in the 256x256 tile), q: 96
]


@pytest.mark.parametrize("path,model,b,h,w,zr_sched,q_sched", PRODUCTION,
                         ids=[f"{p[0]}-{p[1]}-{p[3]}x{p[4]}x{p[2]}-zr_{p[5]}-q_{p[6]}" for p in PRODUCTION])
def test_engine_gate_launches(gpu, path, model, b, h, w, zr_sched, q_sched):
    """UpdateEngine.gru() at a production shape: every z|r and q launch it makes (both SepConvGRU passes), each checked on its own
    inputs as it happens — the engine's buffers, packed weights, context rows and stream-K workspace."""
    from ptlflow_amd.synth import synth_update_block_params
    from ptlflow_amd.update import UpdateEngine
    b16 = path == "b16"
    spec = _spec(model)
    P = synth_update_block_params(spec, seed=17)
    eng = UpdateEngine(P, spec, gpu, conv_precision="bf16" if b16 else "fp32")
    eng.bind(b, h, w)
    Ch, Ci, real, _, _ = _widths(spec, b16)
    M = b * h * w
    g = torch.Generator().manual_seed(23)
    net = torch.tanh(torch.randn(b, Ch, h, w, generator=g))
    inp = torch.relu(torch.randn(b, Ci, h, w, generator=g))
    eng.load_state(net.to(gpu), inp.to(gpu))          # h, inp -> hx (+ the bf16 twin), the context terms
    motion = torch.randn(M, real, generator=g).to(gpu)
    eng.hx[:, Ch + Ci: Ch + Ci + real] = motion
    if b16:
        eng.hxb[:, Ch + Ci: Ch + Ci + real] = motion.to(BF)
    shape, tag = (b, h, w), f"{path} {model} b{b} {h}x{w}"
    rnd = (lambda x: x.to(BF).float()) if b16 else (lambda x: x)
    orig = eng._conv
    seen = []

    def weight(key):
        sfx = key[2:] if key.startswith("zr") else key[1:]
        wt = torch.cat([P[f"gru.convz{sfx}.weight"], P[f"gru.convr{sfx}.weight"]], 0) if key.startswith("zr") else P[f"gru.convq{sfx}.weight"]
        return rnd(torch.cat([wt[:, :Ch], wt[:, Ch + Ci: Ch + Ci + real]], 1).float())

    def launch(srcs, kh, kw, key, cout, epi=EPI_LINEAR, h=None, z=None, rh=None, residual=None, **kw_):
        if epi == EPI_LINEAR:
            return orig(srcs, kh, kw, key, cout, epi=epi, h=h, z=z, rh=rh, residual=residual, **kw_)
        sched = zr_sched if epi == EPI_GRU_ZR else q_sched
        ins = [s.clone() for s in srcs]
        hx0, hxb0 = eng.hx.clone(), (eng.hxb.clone() if b16 else None)
        z0, rh0, res0 = eng.zbuf.clone(), eng.rh.clone(), (residual.clone() if residual is not None else None)
        if not b16:
            arm(eng.workspace)
        orig(srcs, kh, kw, key, cout, epi=epi, h=h, z=z, rh=rh, residual=residual, **kw_)
        torch.cuda.synchronize()
        what = f"{key} ({sched})"
        if not b16:
            ws_after(eng.workspace, sched == "sk", what)
        if residual is not None:
            assert torch.equal(residual, res0), f"{what} wrote into its context rows"
        bias = eng.w.get(key + ".b")
        if epi == EPI_GRU_ZR:
            assert torch.equal(eng.hx, hx0) and (not b16 or torch.equal(eng.hxb, hxb0)), f"{what} wrote into the hx rows"
            z_ref, rh_ref = ref_zr(ins, [Ch, real], weight(key), bias, res0, (hxb0 if b16 else hx0)[:, :Ch], shape, (kh, kw))
            check = (lambda got, ref, what: within_ulp(got, ref, 2.0 ** -16, what)) if b16 else close32
            _report(f"{tag} {what}", z=check(eng.zbuf, z_ref, f"{what} z"), rh=check(eng.rh, rh_ref, f"{what} r*h"))
        else:
            assert torch.equal(eng.hx[:, Ch:], hx0[:, Ch:]), f"{what} wrote outside h"
            assert torch.equal(eng.zbuf, z0) and torch.equal(eng.rh, rh0), f"{what} wrote into z / r*h"
            h_ref = ref_q(ins, [Ch, real], weight(key), bias, res0, z0, hx0[:, :Ch], shape, (kh, kw))
            _report(f"{tag} {what}", h=close32(eng.hx[:, :Ch], h_ref, f"{what} h"))
            if b16:
                assert torch.equal(eng.hxb[:, Ch:], hxb0[:, Ch:]), f"{what} wrote outside the h twin"
                assert torch.equal(eng.hxb[:, :Ch], eng.hx[:, :Ch].to(BF)), f"{what}: the h twin is not bf16(h)"
        seen.append(key)

    eng._conv = launch
    eng.gru()
    assert seen == [k + s for _, _, s in spec.gru_passes for k in ("zr", "q")]
