"""The torch binding (ptlflow_amd/csrc/pfk_torch.cpp) is where a tensor becomes the pointer, stride and extents a kernel trusts.
Every case below hands one op one bad argument — too few elements, too few columns, a non-unit channel stride, or a 1-D tensor where
rows are expected — and asserts a RuntimeError that names the op and the argument, raised before anything was launched: after one
synchronize the sentinel-filled outputs still hold the sentinel.  Each op first makes one valid call at the same shape, so the table
cannot pass by rejecting everything.

Every bad argument is a view cut out of a full-size allocation (`buf[:M - 1]`, `buf[:, :C - 4]`, `buf.t()`, `buf.reshape(-1)`): a
kernel that ran anyway would stay inside allocated memory.  CPU tensors, other GPUs and undersized allocations are not cases here:
every pointer comes from a helper of pfk_torch_views.h that checks the op's device (tests/test_capi.py holds the source to that).

Shapes: B, H, W = 1, 2, 3 (M = 6), C = 8 for the gate kernels, cout = 64 for the GRU epilogues (Ch = 32 for z|r, 64 for q)."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W = 1, 2, 3
M = B * H * W
C = 8
SENTINEL = -7.5
BF = torch.bfloat16
EPI_GRU_ZR, EPI_GRU_Q = 1, 2

few = lambda t: t[:M - 1]                 # noqa: E731  one row short
narrow = lambda t: t[:, :-4]              # noqa: E731  four columns short (and, for a dense tensor, no longer contiguous)
strided = lambda t: t.t()                 # noqa: E731  channel stride != 1
flat = lambda t: t.reshape(-1)            # noqa: E731  1-D where rows are expected (the operands here are contiguous or [M, C] slices)
short = lambda t: t.reshape(-1)[:-1]      # noqa: E731  one element short


def rnd(*shape, dtype=torch.float32):
    return torch.randn(*shape, device="cuda").to(dtype)


def sentinel(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, device="cuda", dtype=dtype)


def gru_gates_zr():
    args = dict(a_zr=rnd(M, 2 * C), h=rnd(M, C + 8)[:, :C], z=sentinel(M, C), r=sentinel(M, C), rh=sentinel(M, C))
    return args, ["z", "r", "rh"], [("a_zr", few), ("h", flat), ("z", few), ("r", narrow), ("rh", short)]


def gru_gates_q():
    args = dict(a_q=rnd(M, C), z=rnd(M, C), h=rnd(M, C + 8)[:, :C], q=sentinel(M, C), h_new=sentinel(M, C))
    return args, ["q", "h_new"], [("a_q", few), ("z", few), ("h", flat), ("q", narrow), ("h_new", short)]


def gru_backward_q():
    args = dict(dh_new=rnd(M, C + 8)[:, :C], z=rnd(M, C), q=rnd(M, C), h=rnd(M, C + 8)[:, :C], da_q=sentinel(M, C),
                da_zr=sentinel(M, 2 * C), dh=sentinel(M, C))
    return args, ["da_q", "da_zr", "dh"], [("dh_new", few), ("dh_new", strided), ("z", few), ("q", narrow), ("da_q", few), ("da_zr", few),
                                           ("dh", short)]


def gru_backward_zr():
    args = dict(d_rh=rnd(M, C), h=rnd(M, C + 8)[:, :C], r=rnd(M, C), da_zr=sentinel(M, 2 * C), dh=sentinel(M, C))
    return args, ["da_zr", "dh"], [("d_rh", few), ("r", narrow), ("da_zr", few), ("dh", short)]


def _conv_gru(epi, b16):
    """a 1x1 gate convolution over one [M, Ch] source with cout = 64; the state is the first Ch columns of a wider buffer"""
    from ptlflow_amd.packing import pack_conv_weight
    cout = 64
    Ch = cout // 2 if epi == EPI_GRU_ZR else cout
    dt = BF if b16 else torch.float32
    hx = torch.tanh(rnd(M, Ch + 8))
    packed = pack_conv_weight(torch.randn(cout, Ch, 1, 1) / 8, [(0, Ch, Ch)], kpad=64 if b16 else 32).to(dt).cuda()
    args = dict(srcs=[rnd(M, Ch, dtype=dt)], B=B, H=H, W=W, kh=1, kw=1, weight=packed, bias=rnd(cout), cout=cout, epilogue=epi, relu=False,
                scale=1.0, out=None, h=hx[:, :Ch])
    if b16:      # z|r reads the bf16 twin of h only; q updates the fp32 state and mirrors it
        args["h_b16"] = hx.to(BF)[:, :Ch]
        if epi == EPI_GRU_ZR:
            args["h"] = None
    if epi == EPI_GRU_ZR:
        args.update(aux_z=sentinel(M, Ch, dtype=dt), aux_rh=sentinel(M, Ch, dtype=dt))
        state = "h_b16" if b16 else "h"
        return args, ["aux_z", "aux_rh"], [(state, narrow), (state, flat), ("aux_z", few), ("aux_rh", short), ("bias", short)]
    args.update(aux_z=torch.sigmoid(rnd(M, Ch)).to(dt), aux_rh=None)
    return args, ["h"] + (["h_b16"] if b16 else []), [("h", narrow), ("h", strided), ("aux_z", few), ("bias", short)]


def flow_from_coords():
    args = dict(coords0=rnd(B, 2, H, W), coords1=rnd(B, 2, H, W), flow_out=sentinel(M, 4)[:, 1:3])
    return args, ["flow_out"], [("flow_out", few), ("flow_out", flat), ("coords1", short)]


def flow_delta():
    cin = 128
    args = dict(inp=rnd(M, cin + 8)[:, :cin], weight=rnd(9 * 2 * cin) / 48, bias=rnd(2), coords0=rnd(B, 2, H, W), coords1=sentinel(B, 2, H, W),
                delta_out=sentinel(B, 2, H, W), flow_out=sentinel(M, 4)[:, :2])
    return args, ["coords1", "delta_out", "flow_out"], [("inp", few), ("weight", short), ("coords1", short), ("delta_out", short),
                                                        ("flow_out", few), ("flow_out", strided)]


def convex_upsample():
    args = dict(flow=rnd(B, 2, H, W), mask=rnd(M, 580)[:, :576], out=sentinel(B, 2, 8 * H, 8 * W))
    return args, ["out"], [("mask", narrow), ("mask", few), ("out", short)]


def nchw_to_pm():
    args = dict(inp=rnd(B, C, H, W), out=sentinel(M, C + 8)[:, :C])
    return args, ["out"], [("out", narrow), ("out", few), ("inp", short)]


def pm_to_nchw():
    args = dict(inp=rnd(M, C + 8)[:, :C], out=sentinel(B, C, H, W))
    return args, ["out"], [("inp", few), ("inp", narrow), ("out", short)]


def pm_to_cm():
    args = dict(inp=rnd(M, C + 8)[:, :C], out=sentinel(B, C, 32))
    return args, ["out"], [("inp", narrow), ("inp", strided), ("out", lambda t: t[:, :, :M - 1])]


def conv_cin2():
    from ptlflow_amd.packing import pack_cin2_weight
    cout = 64
    args = dict(inp=rnd(M, 8)[:, 4:6], weight=pack_cin2_weight(torch.randn(cout, 2, 7, 7) / 8).cuda(), bias=rnd(cout), out=sentinel(M, cout + 8)[:, :cout],
                B=B, H=H, W=W, k=7, relu=True)
    return args, ["out"], [("inp", few), ("weight", short), ("bias", short), ("out", few)]


CASES = {
    "gru_gates_zr": gru_gates_zr, "gru_gates_q": gru_gates_q, "gru_backward_q": gru_backward_q, "gru_backward_zr": gru_backward_zr,
    "conv2d/zr": lambda: _conv_gru(EPI_GRU_ZR, False), "conv2d/q": lambda: _conv_gru(EPI_GRU_Q, False),
    "conv2d_b16/zr": lambda: _conv_gru(EPI_GRU_ZR, True), "conv2d_b16/q": lambda: _conv_gru(EPI_GRU_Q, True),
    "flow_from_coords": flow_from_coords, "flow_delta": flow_delta, "convex_upsample": convex_upsample, "nchw_to_pm": nchw_to_pm,
    "pm_to_nchw": pm_to_nchw, "pm_to_cm": pm_to_cm, "conv_cin2": conv_cin2,
}


@pytest.mark.parametrize("case", list(CASES))
def test_bad_argument_is_refused_before_any_launch(gpu, case):
    op = case.split("/")[0]
    fn = getattr(torch.ops.pfk, op)
    torch.manual_seed(len(case))
    args, outs, bad = CASES[case]()
    fn(**args)                                  # the valid call
    torch.cuda.synchronize()
    assert any(bool((args[n] != SENTINEL).any()) for n in outs), "the valid call wrote nothing"
    for n in outs:
        args[n].fill_(SENTINEL)
    for name, cut in bad:
        with pytest.raises(RuntimeError) as e:
            fn(**dict(args, **{name: cut(args[name])}))
        assert re.search(rf"{op}: {name}\b", str(e.value)), f"{case}: bad `{name}` was refused without naming it: {str(e.value)[:200]}"
    torch.cuda.synchronize()
    for n in outs:
        assert bool((args[n] == SENTINEL).all()), f"{case}: `{n}` was written by a refused call"
