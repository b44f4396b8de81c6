"""The epilogue of the 2-D Winograd kernel (`pfk_conv2d_wino_f32`, `pfk_conv2d_wino_res_f32`): tile coordinates from a per-block
table, rows parked in LDS and written as 16-byte pieces, a dword path for misaligned rows and the ragged last column block.

Every case is held to
* the bits of the kernel before that epilogue: sha256 of the whole output buffer (sentinel columns and guard rows included) against
  tests/golden/wino_epilogue_bits.json, recorded once on the GPU from the commit that file names;
* nothing written outside the launch's pixels and channels;
* the fp64 gate of test_gpu_winograd.py: max |error| <= 4x the direct kernel's + 1e-6, both against an fp64 convolution
  (residual form: relu2(res + scale * relu(conv + bias))).

Shapes (cin a multiple of 32), the smallest at which the paths can go wrong:
  A  B3 5x7 32->126    odd H and W; 12 tiles per image: block 0 holds tiles of three images, block 1 is 4 tiles and 28 empty;
                       126 columns: dense rows are not 16-byte aligned, and the last column block has 2 pad columns
  B  B1 2x2 32->64     one tile
  C  B2 13x17 64->192  source = a channel slice of a wider buffer, output = a channel slice (row stride 256, offset 32: 16-byte
                       pieces; offset 30: the dword path) of a taller buffer
  D  B2 64x130 32->512 and its cout_active=256 launch: 1040 blocks of tiles x 8 (4) column blocks, a ragged last tile group
  E  A and C with a residual in a wider buffer, relu / second relu on and off, scale 1 and 0.25
"""
import functools
import hashlib
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from op_gate import pm, unpm

pytestmark = pytest.mark.gpu

EPI_LINEAR = 0
RATIO = 4.0
SENTINEL = 7.0
GUARD = 2          # rows behind the last pixel
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_epilogue_bits.json")

SHAPES = {
    "A": dict(B=3, H=5, W=7, cin=32, cout=126),
    "B": dict(B=1, H=2, W=2, cin=32, cout=64),
    "C": dict(B=2, H=13, W=17, cin=64, cout=192),
    "D": dict(B=2, H=64, W=130, cin=32, cout=512),
}
# name -> shape, relu, scale, placement of source / output / residual, form
PLAIN = {
    "A": dict(shape="A", relu=True, scale=1.0),
    "B": dict(shape="B", relu=False, scale=0.25),
    "C_off32": dict(shape="C", relu=True, scale=1.0, src_off=12, src_ld=104, out_ld=256, out_off=32),
    "C_off30": dict(shape="C", relu=True, scale=1.0, src_off=12, src_ld=104, out_ld=256, out_off=30),
    "D": dict(shape="D", relu=True, scale=1.0),
    "D_active256": dict(shape="D", relu=True, scale=1.0, cout_active=256),
}
RES_FORMS = {"relu_relu2_s1": (True, True, 1.0), "plain_s025": (False, False, 0.25), "relu_s025": (True, False, 0.25),
             "relu2_s1": (False, True, 1.0)}
RES = {}
for _f, (_relu, _relu2, _scale) in RES_FORMS.items():
    RES[f"EA_{_f}"] = dict(shape="A", relu=_relu, relu2=_relu2, scale=_scale, res_ld=130, res_off=2)
    RES[f"EC_{_f}"] = dict(shape="C", relu=_relu, relu2=_relu2, scale=_scale, src_off=12, src_ld=104, out_ld=256, out_off=32,
                           res_ld=200, res_off=4)
# the output rows take 16-byte pieces, the residual's rows do not
RES["EC_resoff3"] = dict(shape="C", relu=True, relu2=True, scale=0.25, src_off=12, src_ld=104, out_ld=256, out_off=32, res_ld=200,
                         res_off=3)
CASES = {**PLAIN, **RES}


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed=3):
    """x, weight, bias as `_case` of test_gpu_winograd.py makes them, then a residual; CPU generator, fixed seed"""
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(s["B"], s["cin"], s["H"], s["W"], generator=g)
    wt = torch.randn(s["cout"], s["cin"], 3, 3, generator=g) / math.sqrt(s["cin"] * 9)
    bias = torch.randn(s["cout"], generator=g)
    res = torch.randn(s["B"], s["cout"], s["H"], s["W"], generator=g)
    return x, wt, bias, res


@functools.lru_cache(maxsize=None)
def _conv64(shape):
    x, wt, bias, _ = _inputs(shape)
    return F.conv2d(x.double(), wt.double(), bias.double(), padding=1)


@functools.lru_cache(maxsize=None)
def _weights(shape):
    from ptlflow_amd.packing import pack_conv_weight, pack_wino_weight
    _, wt, _, _ = _inputs(shape)
    cin = wt.shape[1]
    return pack_wino_weight(wt).cuda(), pack_conv_weight(wt, [(0, cin, cin)]).cuda()


def _ref64(name):
    c = CASES[name]
    r = _conv64(c["shape"])
    if c["relu"]:
        r = F.relu(r)
    r = r * c["scale"]
    if "res_ld" in c:
        r = _inputs(c["shape"])[3].double() + r
        if c["relu2"]:
            r = F.relu(r)
    return r


def _place(rows, ld, off, fill, extra_rows=0):
    """`rows` as the channel slice [off, off + C) of a [M + extra_rows, ld] buffer filled with `fill`: (buffer, view)"""
    M, C = rows.shape
    buf = torch.full((M + extra_rows, ld), fill, device="cuda")
    view = buf[:M, off:off + C]
    view.copy_(rows)
    return buf, view


def run_case(name, x=None):
    """Launch case `name` (on other images `x` of its shape, if given): the whole output buffer, its written view, the active columns"""
    c = CASES[name]
    s = SHAPES[c["shape"]]
    x0, wt, bias, res = _inputs(c["shape"])
    x = x0 if x is None else x
    B, H, W, cin, cout = x.shape[0], s["H"], s["W"], s["cin"], s["cout"]
    M = B * H * W
    ww, _ = _weights(c["shape"])
    _, src = _place(pm(x).cuda(), c.get("src_ld", cin), c.get("src_off", 0), 1.5)
    out_ld, out_off = c.get("out_ld", cout), c.get("out_off", 0)
    buf = torch.full((M + GUARD, out_ld), SENTINEL, device="cuda")
    out = buf[:M, out_off:out_off + cout]
    active = c.get("cout_active", 0)
    if "res_ld" in c:
        _, r = _place(pm(res[:B]).cuda(), c["res_ld"], c["res_off"], 3.0)
        torch.ops.pfk.conv2d_wino_res(src, B, H, W, ww, bias.cuda(), cout, c["relu"], c["scale"], out, r, c["relu2"])
    else:
        torch.ops.pfk.conv2d_wino(src, B, H, W, ww, bias.cuda(), cout, c["relu"], c["scale"], out, active)
    torch.cuda.synchronize()
    return buf, out, (active or cout)


def _direct(name):
    c = CASES[name]
    s = SHAPES[c["shape"]]
    x, _, bias, res = _inputs(c["shape"])
    B, H, W, cout = s["B"], s["H"], s["W"], s["cout"]
    _, wd = _weights(c["shape"])
    out = torch.zeros(B * H * W, cout, device="cuda")
    r = pm(res).cuda() if "res_ld" in c else None
    torch.ops.pfk.conv2d([pm(x).cuda()], B, H, W, 3, 3, wd, bias.cuda(), cout, EPI_LINEAR, c["relu"], c["scale"], out, None, None, None,
                         None, r, 1, bool(c.get("relu2", False)))
    return out


def digest(buf):
    return hashlib.sha256(buf.cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_bounds_and_fp64_gate(gpu, name):
    c = CASES[name]
    s = SHAPES[c["shape"]]
    B, H, W, cout = s["B"], s["H"], s["W"], s["cout"]
    M = B * H * W
    buf, out, active = run_case(name)
    # nothing else written: sentinel columns, the channels a cout_active launch leaves out, the guard rows
    off = c.get("out_off", 0)
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[:M, off:off + active] = False
    assert bool((buf[outside] == SENTINEL).all()), "wrote outside its pixels or channels"
    assert not bool((out[:, :active] == SENTINEL).any()), "left an output unwritten"
    # fp64 gate
    ref = _ref64(name)[:, :active]
    ew = (unpm(out[:, :active], B, H, W).double() - ref).abs().max().item()
    ed = (unpm(_direct(name)[:, :active], B, H, W).double() - ref).abs().max().item()
    print(f"{name}: wino max err {ew:.3e}, direct {ed:.3e}, ratio {ew / max(ed, 1e-30):.2f}")
    assert ew <= RATIO * ed + 1e-6, f"wino max err {ew:.3e} vs direct {ed:.3e}"
    # the bits of the kernel before the lean epilogue
    golden = json.load(open(GOLDEN))
    got = digest(buf)
    print(f"{name}: sha256 {got}")
    assert got == golden["sha256"][name], f"{name}: output bits differ from commit {golden['parent_commit']}"


def test_position_independence(gpu):
    """image 0 of A alone and as the second of a batch of two (its 12 tiles start at tile 12 of block 0): bit-equal rows.  (The
    residual form adds residual b to image b, so there image 0 is compared as the first of the pair.)"""
    x = _inputs("A")[0]
    px = SHAPES["A"]["H"] * SHAPES["A"]["W"]
    for name in ("A", "EA_relu_relu2_s1"):
        _, alone, _ = run_case(name, x[0:1])
        _, first_of_pair, _ = run_case(name, torch.cat([x[0:1], x[1:2]]))
        assert torch.equal(first_of_pair[:px], alone)
        if name == "A":
            _, pair, _ = run_case(name, torch.cat([x[1:2], x[0:1]]))
            assert torch.equal(pair[px:], alone), "rows depend on the tile's place in its block"


@pytest.mark.parametrize("b,h,w", [(8, 55, 128), (3, 5, 7)])
def test_engine_f2_call_site(gpu, monkeypatch, b, h, w):
    """`f2` (convf2, 3x3, 128 -> 64) at the engine's call site (`motion_flow`: convf1 into `flo1`, then `f2` into its slice of `corflo`)
    at the benchmark's grid, which the rule sends to Winograd, and at a ragged grid with the floor lowered: the Winograd launch is
    taken, `winograd=False` is the direct launch, and both are held to the fp64 gate on the `flo1` the engine produced."""
    from ptlflow_amd import update
    from ptlflow_amd.synth import synth_update_block_params
    from ptlflow_amd.update import UpdateEngine, basic_spec
    spec = basic_spec()
    if b * h * w < update.WINO_F2_MIN_PIXELS:
        monkeypatch.setattr(update, "WINO_F2_MIN_PIXELS", 0)
    else:
        assert b * h * w >= update.WINO_F2_MIN_PIXELS >= 28160        # nothing unmeasured takes Winograd
    P = synth_update_block_params(spec, seed=17)
    eng = UpdateEngine(P, spec, gpu)
    eng.bind(b, h, w)
    M = b * h * w
    eng.flow_view.copy_(torch.randn(M, 2, generator=torch.Generator().manual_seed(31)).to(gpu) * 3.0)
    cor_c = spec.c2 if spec.c2 else spec.c1
    names = []

    class Count:
        def __init__(self, ops):
            self._ops = ops

        def __getattr__(self, name):
            names.append(name)
            return getattr(self._ops, name)

    def run(winograd):
        eng.winograd = winograd
        eng.corflo.fill_(SENTINEL)
        names.clear()
        orig, eng.ops = eng.ops, Count(eng.ops)
        try:
            eng.motion_flow()
        finally:
            eng.ops = orig
        torch.cuda.synchronize()
        return eng.corflo.clone()

    cw = run(True)
    assert names == ["conv_cin2", "conv2d_wino"], names
    cd = run(False)
    assert names == ["conv_cin2", "conv2d"], names
    for c in (cw, cd):
        assert bool((c[:, :cor_c] == SENTINEL).all()) and bool((c[:, cor_c + spec.f2:] == SENTINEL).all()), "wrote outside f2's slice"
    x = unpm(eng.flo1[:M], b, h, w).double()
    ref = F.relu(F.conv2d(x, P["encoder.convf2.weight"].double().cpu(), P["encoder.convf2.bias"].double().cpu(), padding=1))
    ew = (unpm(cw[:M, cor_c: cor_c + spec.f2], b, h, w).double() - ref).abs().max().item()
    ed = (unpm(cd[:M, cor_c: cor_c + spec.f2], b, h, w).double() - ref).abs().max().item()
    print(f"f2 at {b}x{h}x{w}: wino max err {ew:.3e}, direct {ed:.3e}, ratio {ew / max(ed, 1e-30):.2f}")
    assert ew <= RATIO * ed + 1e-6, f"wino max err {ew:.3e} vs direct {ed:.3e}"


def test_f2_leaves_the_grouped_launch_where_it_takes_winograd(gpu, monkeypatch):
    """With the floor lowered so that `f2` takes Winograd on a small grid, the grouped schedule (`motion_grouped`: f2 taken out of
    the grouped launch) and the one-launch-per-convolution schedule give the same bits, and both differ from the direct `f2`."""
    from oracle import raft_oracle as O
    from ptlflow_amd import update
    from ptlflow_amd.raft import RAFT
    x = O.smooth_pair(2, 184, 320, seed=1).cuda()

    def forward(grouped):
        m = RAFT(iters=3).load_synthetic(5).eval().cuda()
        m.group_launches = grouped
        out = m({"images": x})
        torch.cuda.synchronize()
        return out["flows"].clone()

    direct = forward(False)
    monkeypatch.setattr(update, "WINO_F2_MIN_PIXELS", 0)
    single, grouped = forward(False), forward(True)
    assert torch.equal(single, grouped)
    assert not torch.equal(single, direct), "f2 did not take the Winograd kernel"


def test_deterministic(gpu):
    a, _, _ = run_case("D")
    b, _, _ = run_case("D")
    assert torch.equal(a, b)
    half, _, _ = run_case("D_active256")
    assert torch.equal(half[:, :256], a[:, :256]), "the cout_active launch does not have the full launch's bits"
