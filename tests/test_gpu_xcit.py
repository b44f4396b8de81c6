"""CCMR's XCiT motion aggregator on the kernels (K14, ptlflow_amd/csrc/pfk_xcit.hip, ptlflow_amd/xcit.py) on the GPU.

Per kernel, against float64 on the kernel's own inputs (tests/xcit_refs.py; instruments of tests/op_gate.py): relative L2 <= OP_TOL,
the per-element bounds of xcit_refs' docstring through `gates` for the depthwise sums, `close32` for the normalised and softmax
outputs, NaN pad columns in, sentinels out, the same bits on a second run.  Every input has different content in neighbouring
images, values at every border and corner and (more than one pixel) an all-zero row.  Then the engine against the stand-in in float64,
the golden replay, and `PfkUpdateBlock` with the option on against the option off."""
import copy

import pytest
import torch

from op_gate import BLOCK_TOL, OP_TOL, Rows, close32, flat_out, gates, record, rel, same_bits, scale_close, tail_kept
from xcit_model import XCiT, randomize, register
from xcit_refs import C, GN_EPS, LN_EPS, groupnorm_stats, layernorm_ref, load_golden, lpi1_ref, lpi2_ref, rows64, xca_map_ref

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1, 1), (1, 2, 2), (2, 1, 7), (2, 3, 5), (3, 9, 17), (5, 4, 6), (1, 28, 64)]      # (5,4,6): past the 4-image group;
ENGINE_GRIDS = [(2, 3, 5), (5, 4, 6), (1, 28, 64)]                                             # (1,28,64): CCMR's coarsest scale at 448 x 1024
ids = lambda g: "x".join(map(str, g))  # noqa: E731


def grid_values(B, H, W, Cc, seed, scale=1.0):
    """[B*H*W, Cc] fp32: each image at its own scale and offset, +-2.5 on the border pixels and +-4 in the corners (so a tap that
    wraps around a row, crosses into the next image or reads padding as data moves the result), one all-zero row (M > 1)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cc, generator=g) * scale
    for b in range(B):
        x[b] = x[b] * (1.0 + 0.5 * b) + 0.3 * b
    sign = torch.where(torch.arange(Cc) % 2 == 0, 1.0, -1.0)
    for sl in ((slice(None), 0), (slice(None), H - 1), (slice(None), slice(None), 0), (slice(None), slice(None), W - 1)):
        x[sl] += 2.5 * sign
    for yy in (0, H - 1):
        for xx in (0, W - 1):
            x[:, yy, xx] -= 4.0 * sign
    x = x.reshape(B * H * W, Cc)
    if x.shape[0] > 1:
        x[x.shape[0] // 2] = 0.0
    return x.contiguous()


def vec(seed, lo, hi, n=C):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


# ---------------------------------------------------------------------------------------------------------------------
# pfk_layernorm_rows_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,Cc", [(g, C) for g in GRIDS] + [((2, 3, 5), 4), ((2, 3, 5), 132), ((2, 3, 5), 512)],
                         ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
def test_layernorm_rows(gpu, grid, Cc, affine):
    B, H, W = grid
    M = B * H * W
    x = grid_values(B, H, W, Cc, 11)
    w, b = (vec(1, 0.5, 1.5, Cc), vec(2, -0.3, 0.3, Cc)) if affine else (None, None)
    src = Rows(M, Cc, gpu, x.to(gpu))
    dev = lambda t: None if t is None else t.to(gpu)  # noqa: E731
    outs = []
    for _ in range(2):
        out = Rows(M, Cc, gpu)
        torch.ops.pfk.layernorm_rows(src.rows, dev(w), dev(b), LN_EPS, out.rows)
        out.check_untouched("layernorm_rows")
        outs.append(out)
    assert torch.equal(outs[0].flat, outs[1].flat)
    got = outs[0].rows.cpu()
    ref = layernorm_ref(x.double(), w, b)
    close32(got, ref, "layernorm_rows")
    assert rel(got, ref) <= OP_TOL
    if M > 1:      # the all-zero row: exactly the bias, or exactly 0
        assert torch.equal(got[M // 2], b if affine else torch.zeros(Cc))
    inplace = Rows(M, Cc, gpu, x.to(gpu))
    inplace.full[:, Cc:] = 7.0
    torch.ops.pfk.layernorm_rows(inplace.rows, dev(w), dev(b), LN_EPS, inplace.rows)
    assert torch.equal(inplace.rows, outs[0].rows) and bool((inplace.full[:, Cc:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# pfk_xca_map_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS + [(2, 20, 30)], ids=ids)       # 600 tokens: three chunks, the last one partial
def test_xca_map(gpu, grid):
    B, H, W = grid
    N = H * W
    qk = grid_values(B, H, W, 2 * C, 23, scale=0.7)
    temp = vec(3, 0.5, 2.5, 8)
    src = Rows(B * N, 2 * C, gpu, qk.to(gpu))
    outs = []
    for _ in range(2):
        flat, A = flat_out((B, 8, 16, 16), gpu)
        torch.ops.pfk.xca_map(src.rows, temp.reshape(8, 1, 1).to(gpu), A, B, N)
        assert tail_kept(flat)
        outs.append(flat)
    assert torch.equal(outs[0], outs[1])
    got = outs[0][:B * 2048].view(B, 8, 16, 16).cpu()
    ref = xca_map_ref(qk.double().reshape(B, N, 2 * C), temp)
    close32(got, ref, "xca_map")
    r = rel(got, ref)
    print(f"xca_map {grid}: relL2 {r:.2e}")
    assert r <= OP_TOL
    assert float((got.double().sum(-1) - 1).abs().max()) <= 4 * 2.0 ** -24 * 16
    assert float((got[0] - got[-1]).abs().max()) > 1e-3 or B == 1          # the map is per image


# ---------------------------------------------------------------------------------------------------------------------
# pfk_xcit_lpi1_f32 / pfk_xcit_lpi2_f32
# ---------------------------------------------------------------------------------------------------------------------
def lpi_params(seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *shape: torch.rand(*shape, generator=g) * (hi - lo) + lo  # noqa: E731
    return dict(ln3_w=u(0.5, 1.5, C), ln3_b=u(-0.3, 0.3, C), dw1_w=u(-0.4, 0.4, C, 9), dw1_b=u(-0.3, 0.3, C), gn_w=u(0.5, 1.5, C),
                gn_b=u(-0.3, 0.3, C), dw2_w=u(-0.4, 0.4, C, 9), dw2_b=u(-0.3, 0.3, C), gamma=u(0.2, 1.0, C), ln2_w=u(0.5, 1.5, C),
                ln2_b=u(-0.3, 0.3, C))


def run_lpi1(gpu, src, P, B, H, W):
    out = Rows(B * H * W, C, gpu)
    ws = torch.zeros(torch.ops.pfk.xcit_lpi_workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    torch.ops.pfk.xcit_lpi1(src.rows, P["ln3_w"], P["ln3_b"], LN_EPS, P["dw1_w"], P["dw1_b"], out.rows, ws, B, H, W)
    out.check_untouched("xcit_lpi1")
    return out, ws


@pytest.mark.parametrize("grid", GRIDS, ids=ids)
def test_lpi1(gpu, grid):
    B, H, W = grid
    x = grid_values(B, H, W, C, 31)
    P = lpi_params(5)
    G = {k: v.to(gpu) for k, v in P.items()}
    src = Rows(B * H * W, C, gpu, x.to(gpu))
    (o1, ws1), (o2, ws2) = run_lpi1(gpu, src, G, B, H, W), run_lpi1(gpu, src, G, B, H, W)
    assert torch.equal(o1.flat, o2.flat) and torch.equal(ws1, ws2)
    ref, bound = lpi1_ref(x.double().reshape(B, H, W, C), P["ln3_w"], P["ln3_b"], P["dw1_w"], P["dw1_b"])
    res = gates(f"lpi1 {grid}", rows64(o1.rows, B, H, W), ref, bound, 1)
    record("xcit_lpi1", [res])


@pytest.mark.parametrize("grid", GRIDS, ids=ids)
@pytest.mark.parametrize("affine", [True, False], ids=["ln2-affine", "ln2-plain"])
def test_lpi2_and_groupnorm(gpu, grid, affine):
    B, H, W = grid
    M = B * H * W
    x = grid_values(B, H, W, C, 37)
    P = lpi_params(7)
    G = {k: v.to(gpu) for k, v in P.items()}
    src = Rows(M, C, gpu, x.to(gpu))
    u, ws = run_lpi1(gpu, src, G, B, H, W)
    u_in = Rows(M, C, gpu, u.rows.clone())                    # the u the GPU produced, NaN in its pad columns
    lw, lb = (G["ln2_w"], G["ln2_b"]) if affine else (None, None)
    outs = []
    for _ in range(2):
        x2, t = Rows(M, C, gpu), Rows(M, C, gpu)
        torch.ops.pfk.xcit_lpi2(u_in.rows, G["gn_w"], G["gn_b"], GN_EPS, 8, G["dw2_w"], G["dw2_b"], G["gamma"], src.rows, x2.rows, lw, lb,
                                LN_EPS, t.rows, ws, B, H, W)
        x2.check_untouched("xcit_lpi2 x2")
        t.check_untouched("xcit_lpi2 t")
        outs.append((x2, t))
    assert torch.equal(outs[0][0].flat, outs[1][0].flat) and torch.equal(outs[0][1].flat, outs[1][1].flat)
    assert same_bits(u_in.rows, u.rows)
    u64 = rows64(u.rows, B, H, W)
    # the statistics the kernel finished (mean | rstd per image and group, behind the partials) against float64 on the same u
    mean, rstd = groupnorm_stats(u64)
    stats = ws[ws.numel() - B * 16 * 4:].view(torch.float32).view(B, 8, 2).double().cpu()
    assert float((stats[:, :, 0] - mean[:, 0, 0, ::16]).abs().max()) <= 2.0 ** -23 * float(mean.abs().max()) + 1e-12
    assert float((stats[:, :, 1] / rstd[:, 0, 0, ::16] - 1).abs().max()) <= 2.0 ** -22
    ref, bound = lpi2_ref(u64, P["gn_w"], P["gn_b"], P["dw2_w"], P["dw2_b"], P["gamma"], x.double().reshape(B, H, W, C))
    res = gates(f"lpi2 {grid}", rows64(outs[0][0].rows, B, H, W), ref, bound, 1)
    record("xcit_lpi2", [res])
    # t = LN2 of the x2 the kernel wrote
    x2_64 = outs[0][0].rows.double().cpu()
    tref = layernorm_ref(x2_64, P["ln2_w"] if affine else None, P["ln2_b"] if affine else None)
    close32(outs[0][1].rows.cpu(), tref, "lpi2 t")
    assert rel(outs[0][1].rows, tref) <= OP_TOL


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
def engine_call(eng, gc, mf, B, H, W, gpu, **kw):
    """one `run` on guarded rows: NaN beside the motion rows, sentinels around the output; returns NCHW on the CPU"""
    src = Rows(B * H * W, C, gpu, mf.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(gpu))
    out = Rows(B * H * W, C, gpu)
    eng.run(gc, src.rows, out.rows, B, H, W, **kw)
    out.check_untouched("XcitAggregatorEngine.run")
    return out.rows.cpu().reshape(B, H, W, C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("grid", ENGINE_GRIDS, ids=ids)
def test_engine_against_the_standin_in_float64(gpu, grid):
    from ptlflow_amd.xcit import XcitAggregatorEngine
    B, H, W = grid
    model = randomize(XCiT(separate=True), 41).eval()
    m64 = copy.deepcopy(model).double()
    eng = XcitAggregatorEngine(copy.deepcopy(model).to(gpu), gpu)
    g = torch.Generator().manual_seed(43)
    gcs = [torch.randn(B, C, H, W, generator=g) for _ in range(2)]
    mfs = [grid_values(B, H, W, C, 47 + i).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous() for i in range(4)]
    gc = gcs[0].to(gpu)
    results = []

    def check(what, got, gc_cpu, mf, prepared):
        with torch.no_grad():
            ref, cpu32 = m64(gc_cpu.double(), mf.double()), model(gc_cpu, mf)
        scale_close(got, ref, f"engine {grid} {what}")
        assert eng.prepared == prepared, (what, eng.prepared)
        results.append((rel(got, ref), rel(cpu32, ref)))

    with torch.no_grad():
        check("first call", engine_call(eng, gc, mfs[0], B, H, W, gpu), gcs[0], mfs[0], 1)
        check("cached map", engine_call(eng, gc, mfs[1], B, H, W, gpu), gcs[0], mfs[1], 1)
        gc.mul_(0.5)                                                   # in place: the same object, another _version
        check("mutated in place", engine_call(eng, gc, mfs[2], B, H, W, gpu), gcs[0] * 0.5, mfs[2], 2)
        fresh = gcs[1].to(gpu).contiguous(memory_format=torch.channels_last)      # (and not NCHW-contiguous: the other load path)
        check("fresh tensor", engine_call(eng, fresh, mfs[3], B, H, W, gpu), gcs[1], mfs[3], 3)
        check("refresh", engine_call(eng, fresh, mfs[0], B, H, W, gpu, refresh=True), gcs[1], mfs[0], 4)
    print(f"RECORD xcit engine {ids(grid)}: relL2 to fp64 {max(r for r, _ in results):.1e} | torch fp32 on the CPU "
          f"{max(c for _, c in results):.1e}")


def test_engine_without_positional_encoding(gpu):
    from ptlflow_amd.xcit import XcitAggregatorEngine
    B, H, W = 2, 3, 5
    model = randomize(XCiT(separate=True, use_pos=False), 53).eval()
    eng = XcitAggregatorEngine(copy.deepcopy(model).to(gpu), gpu)
    g = torch.Generator().manual_seed(59)
    gc, mf = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    with torch.no_grad():
        scale_close(engine_call(eng, gc.to(gpu), mf, B, H, W, gpu), copy.deepcopy(model).double()(gc.double(), mf.double()), "use_pos=False")


def test_golden_replay(gpu):
    from ptlflow_amd.xcit import XcitAggregatorEngine, match_xcit_aggregator
    gold = load_golden()
    B, H, W = gold["shape"]
    model = XCiT(separate=True).eval()
    model.load_state_dict(gold["state_dict"])
    assert match_xcit_aggregator(model)
    eng = XcitAggregatorEngine(model.to(gpu), gpu)
    gc = gold["global_context"].to(gpu)
    with torch.no_grad():
        for i, mf in enumerate(gold["motion_features"]):
            got = engine_call(eng, gc, mf, B, H, W, gpu)
            scale_close(got, gold["out"][i], f"golden out[{i}]")
            scale_close(got, gold["out64"][i], f"golden out64[{i}]")
            if i == 0:
                scale_close(eng.A.cpu(), gold["A"], "golden A")
                scale_close(eng.x1.cpu().reshape(B, H * W, C), gold["x1"], "golden x1")
                scale_close(eng.x2.cpu().reshape(B, H * W, C), gold["x2"], "golden x2")
    assert eng.prepared == 1
    # a parameter changed in place: `pack` again, as the `_engine_for` idiom of the wrappers does on a new version
    with torch.no_grad():
        model.blocks[0].gamma2.mul_(2.0)
    eng.pack()
    cpu = copy.deepcopy(model).cpu().double()
    with torch.no_grad():
        scale_close(engine_call(eng, gc, gold["motion_features"][0], B, H, W, gpu),
                    cpu(gold["global_context"].double(), gold["motion_features"][0].double()), "after a repack")


# ---------------------------------------------------------------------------------------------------------------------
# the update block, option on against option off
# ---------------------------------------------------------------------------------------------------------------------
LEVELS = ((2, 5, 6), (2, 9, 12))


def make_block(gpu):
    from ptlflow_amd.raft import _param_tree
    from ptlflow_amd.synth import synth_state_dict, update_block_shapes
    from ptlflow_amd.update import PfkUpdateBlock, ccmr_spec
    register()
    spec = ccmr_spec(162)
    holder = _param_tree(update_block_shapes(spec))
    holder.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in holder.state_dict().items()}, seed=29))
    holder.add_module("aggregator", torch.nn.ModuleList([randomize(XCiT(separate=True), 61 + i) for i in range(2)]))
    ub = PfkUpdateBlock(holder, spec).to(gpu).eval()
    for p in ub.parameters():
        p.requires_grad_(False)
    return ub


def drive(ub, gpu, seed=8):
    """the coarse-to-fine loop's calls: two levels of different size, three iterations each; every output cloned"""
    g = torch.Generator().manual_seed(seed)
    outs = []
    for level, (B, h, w) in enumerate(LEVELS):
        n = torch.tanh(torch.randn(B, 128, h, w, generator=g)).to(gpu)
        inp = torch.relu(torch.randn(B, 128, h, w, generator=g)).to(gpu)
        ctx = torch.randn(B, 128, h, w, generator=g).to(gpu)
        for _ in range(3):
            corr = torch.randn(B, 162, h, w, generator=g).to(gpu)
            flow = (torch.randn(B, 2, h, w, generator=g) * 2).to(gpu)
            n, m, d = ub(n, inp, corr, flow, ctx, level_index=level)
            outs.append((n.clone(), m.clone(), d.clone()))
    return outs


def test_block_option_on_against_off(gpu):
    ub = make_block(gpu)
    with torch.no_grad():
        off = drive(ub, gpu)
        assert ub.aggregator_calls == 0 and ub._agg_slots == {}          # without the option: no aggregator engine
        ub.set_ccmr_aggregator(True)
        on = drive(ub, gpu)
    assert ub.aggregator_calls == 6 and sorted(ub._agg_slots) == [0, 1]
    assert all(slot._engine.prepared == 1 for slot in ub._agg_slots.values())      # once per (forward, scale)
    for i, (a, b) in enumerate(zip(on, off)):
        for name, x, y in zip(("net", "mask", "delta"), a, b):
            scale_close(x, y, f"call {i} {name}")
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(on, off))                # another path did run

    # The option-off path calls the aggregator MODULES in torch, and on this GPU their fp32 forward does not repeat its own bits at
    # the smaller level (the same module on the same tensors, 2 x 5 x 6: outputs 1e-6 apart from call to call; measured, the
    # block's outputs then differ by 3e-7 between two option-off runs).  So the modules' outputs of the option-off run are recorded
    # and, in the option-on run, each call must arrive with bit-identical inputs and gets the recorded output back: everything
    # the block itself does must then be equal bit for bit.
    tape = {"mode": None, "calls": [], "at": 0}

    def hook(_m, inputs, output):
        if tape["mode"] == "record":
            tape["calls"].append(([t.clone() for t in inputs], output.clone()))
        elif tape["mode"] == "replay":
            want_in, want_out = tape["calls"][tape["at"]]
            tape["at"] += 1
            assert all(torch.equal(a, b) for a, b in zip(inputs, want_in)), "the module's inputs differ from the option-off run's"
            return want_out.clone()
        return None

    handles = [m.register_forward_hook(hook) for m in ub._ref[0].aggregator]

    def same_as_off(what, ctx):
        """under `ctx` the option-on block serves nothing: the modules are called as in the option-off block, and the outputs are equal"""
        with ctx():
            ub.set_ccmr_aggregator(False)
            tape.update(mode="record", calls=[], at=0)
            want = drive(ub, gpu)
            ub.set_ccmr_aggregator(True)
            before = ub.aggregator_calls
            tape.update(mode="replay")
            got = drive(ub, gpu)
            tape.update(mode=None)
        assert ub.aggregator_calls == before and len(tape["calls"]) == 6 and tape["at"] == 6, what
        assert all(torch.equal(x, y) for a, b in zip(got, want) for x, y in zip(a, b)), what

    class Autocast:
        def __enter__(self):
            self.ctx = [torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16)]
            for c in self.ctx:
                c.__enter__()

        def __exit__(self, *exc):
            for c in reversed(self.ctx):
                c.__exit__(*exc)

    same_as_off("autocast", Autocast)
    same_as_off("grad enabled", torch.enable_grad)
    ub.train()
    same_as_off("train()", torch.no_grad)
    ub.eval()
    for h in handles:
        h.remove()
    with torch.no_grad():
        ub.set_ccmr_aggregator(True)
        before = ub.aggregator_calls
        again = drive(ub, gpu)
    assert ub.aggregator_calls == before + 6
    assert all(torch.equal(x, y) for a, b in zip(again, on) for x, y in zip(a, b))      # and the served path repeats its bits


def test_block_refuses_what_the_engine_does_not_implement(gpu):
    from ptlflow_amd.update import PfkUpdateBlock
    ub = make_block(gpu)
    ub._ref[0].aggregator[1].blocks[0].local_mp.bn = torch.nn.GroupNorm(4, 128).to(gpu)      # one aggregator that does not match
    ub.set_ccmr_aggregator(True)
    with torch.no_grad():
        drive(ub, gpu)
    assert ub.aggregator_calls == 0 and ub._agg_slots == {}
    half = PfkUpdateBlock(ub._ref[0], ub.spec, "bf16x3").to(gpu).eval()                         # not the fp32 convolution path
    half._ref[0].aggregator[1].blocks[0].local_mp.bn = torch.nn.GroupNorm(8, 128).to(gpu)
    half.set_ccmr_aggregator(True)
    with torch.no_grad():
        drive(half, gpu)
    assert half._agg_ok and half.aggregator_calls == 0
