"""Host side of the 1-D Winograd F(4,5) convolution (no GPU): the weight transform of packing.pack_wino1d_weight against a plain
restatement, the F(4,5) algorithm on that layout against a direct fp64 convolution, an fp32 emulation of the kernel's arithmetic on
the inputs of test_gpu_gru_schedules.py::test_engine_gate_launches held to that test's gate, and the C ABI's argument checks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import pfk_ctypes
from pfk_ctypes import Desc as _Desc, Src as _Src
from ptlflow_amd.packing import WINO1D_G, pack_wino1d_weight, wino_slot

G = torch.tensor(WINO1D_G, dtype=torch.float64)
BT = torch.tensor([[-1, 0, 21 / 4, 0, -21 / 4, 0, 1, 0],
                   [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0],
                   [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
                   [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0],
                   [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0],
                   [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0],
                   [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0],
                   [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 1, 1, 1, 0],
                   [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0],
                   [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0],
                   [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 1]], dtype=torch.float64)


def _unpack(flat, ktot, cout):
    """flat [ceil(cout/128)][ktot/8][8][128][8 slots] -> U [8][cout padded][ktot] (include/pfk.h)"""
    ncb = (cout + 127) // 128
    u = flat.double().view(ncb, ktot // 8, 8, 128, 8)
    slot = wino_slot(torch.arange(128).view(128, 1), torch.arange(8).view(1, 8))
    u = torch.gather(u, 4, slot.view(1, 1, 1, 128, 8).expand_as(u))          # [cb][ks][xi][nl][cc]
    return u.permute(2, 0, 3, 1, 4).reshape(8, ncb * 128, ktot)


def test_transform_matrices_are_the_convolution():
    """sum_x A^T[i, x] * G[x, k] * B^T[x, j] = [j == i + k]: the three matrices compute y_i = sum_k d[i + k] g[k] exactly"""
    T = torch.einsum("ix,xk,xj->ikj", AT, G, BT)
    want = torch.zeros(4, 5, 8, dtype=torch.float64)
    for i in range(4):
        for k in range(5):
            want[i, k, i + k] = 1
    assert (T - want).abs().max().item() < 1e-14
    assert torch.equal(BT.float().double(), BT) and torch.equal(AT.float().double(), AT)      # exact in fp32


@pytest.mark.parametrize("shape", [(1, 5), (5, 1)])
@pytest.mark.parametrize("cout,segments,cin", [(128, [(0, 32, 32)], 32), (126, [(0, 16, 16), (40, 22, 24)], 64),
                                               (256, [(0, 128, 128), (256, 128, 128)], 384), (300, [(8, 8, 16)], 16)])
def test_weight_layout_matches_restatement(shape, cout, segments, cin):
    torch.manual_seed(0)
    w = torch.randn(cout, cin, *shape)
    flat = pack_wino1d_weight(w, segments)
    ktot = sum(s[2] for s in segments)
    ncb = (cout + 127) // 128
    assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() == 8 * ktot * ncb * 128
    U = _unpack(flat, ktot, cout)
    assert bool((U[:, cout:] == 0).all()), "pad columns must be zero"
    k0 = 0
    for first, n, n_buf in segments:
        assert bool((U[:, :, k0 + n: k0 + n_buf] == 0).all()), "pad channels must be zero"
        for co in range(0, cout, max(1, cout // 7)):
            for c in range(0, n, max(1, n // 5)):
                # float64, rounded to fp32 once (one fp32 ulp: the float64 sums may be taken in another order)
                u = (G @ w[co, first + c].double().reshape(5)).float().double()
                assert bool(((U[:, co, k0 + c] - u).abs() <= 2.0 ** -23 * u.abs()).all()), (co, c)
        k0 += n_buf
    # the flat order itself: element [cb][ks][xi][nl][slot]
    v = flat.view(ncb, ktot // 8, 8, 128, 8)
    for cb, ks, xi, nl, cc in [(0, 0, 0, 0, 0), (ncb - 1, ktot // 8 - 1, 7, 127, 7), (0, ktot // 8 - 1, 3, 77, 5), (ncb - 1, 0, 6, 13, 2)]:
        slot = ((cc & 3) * 2 + (cc >> 2)) ^ (((nl >> 2) & 3) * 2)
        assert float(v[cb, ks, xi, nl, slot]) == float(U[xi, cb * 128 + nl, ks * 8 + cc])


def f45(x, U, vert, dtype):
    """The algorithm the kernel runs, in `dtype`: x [B, K, H, W], U [8][cout][K] -> [B, cout, H, W].  8 input pixels from 2 in front
    of each tile of 4 outputs along the convolution axis (zero outside the image), B^T d term by term with the shared even / odd
    parts, one channel sum per component against U, A^T m term by term."""
    if vert:
        return f45(x.transpose(2, 3), U, False, dtype).transpose(2, 3)
    B, K, H, W = x.shape
    nt = (W + 3) // 4
    d = F.pad(x.to(dtype), (2, 4 * nt + 2 - W)).unfold(3, 8, 4)          # [B, K, H, nt, 8]
    d = [d[..., j] for j in range(8)]
    e12, o12 = d[2] - 4.25 * d[4] + d[6], d[1] - 4.25 * d[3] + d[5]
    e34, o34 = 0.25 * d[2] - 1.25 * d[4] + d[6], 0.5 * d[1] - 2.5 * d[3] + 2.0 * d[5]
    e56, o56 = 4.0 * d[2] - 5.0 * d[4] + d[6], 2.0 * d[1] - 2.5 * d[3] + 0.5 * d[5]
    V = [(d[6] - d[0]) + 5.25 * (d[2] - d[4]), e12 + o12, e12 - o12, e34 + o34, e34 - o34, e56 + o56, e56 - o56,
         (d[7] - d[1]) + 5.25 * (d[3] - d[5])]
    m = [torch.einsum("bkhn,ok->bohn", V[i], U[i].to(dtype)) for i in range(8)]
    p12, q12, p34, q34, p56, q56 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4], m[5] + m[6], m[5] - m[6]
    y = [m[0] + p12 + p34 + p56, q12 + 2.0 * q34 + 0.5 * q56, p12 + 4.0 * p34 + 0.25 * p56, q12 + 8.0 * q34 + 0.125 * q56 + m[7]]
    return torch.stack(y, 4).reshape(B, -1, H, 4 * nt)[..., :W]


@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 9), (1, 7, 2), (1, 4, 4)])
def test_f45_on_the_packed_layout_is_the_convolution(kh, kw, B, H, W):
    """two segments, the second padded in its buffer"""
    torch.manual_seed(1)
    cin, cout, segs = 48, 70, [(0, 16, 16), (24, 21, 24)]
    w = torch.randn(cout, cin, kh, kw, dtype=torch.float64)
    x = torch.randn(B, 40, H, W, dtype=torch.float64)
    x[:, 37:] = 5.0        # pad channels of the second buffer: garbage that zero U must keep out
    ref = F.conv2d(torch.cat([x[:, :16], x[:, 16:37]], 1), torch.cat([w[:, 0:16], w[:, 24:45]], 1), padding=(kh // 2, kw // 2))
    # U unrounded, through the packed layout: exact
    U64 = _unpack(pack_wino1d_weight(w, segs, dtype=torch.float64), 40, cout)[:, :cout]
    got64 = f45(x, U64, kh == 5, torch.float64)
    assert (got64 - ref).abs().max().item() <= 1e-12 * (1 + ref.abs().max().item())
    # U as the kernel reads it (rounded to fp32 once): 2^-24 per entry of U, through |B^T| (row sums <= 21.25) and |A^T| (<= 8 per
    # component, 8 components) over the 37 channels
    U32 = _unpack(pack_wino1d_weight(w, segs), 40, cout)[:, :cout]
    got = f45(x, U32, kh == 5, torch.float64)
    worst = 8 * 8 * 37 * 2.0 ** -24 * 21.25 * float(x[:, :37].abs().max()) * float(U64.abs().max())
    assert (got - ref).abs().max().item() <= worst


def _gate(got, ref, what):
    err = (got.double() - ref).abs()
    lim = 3e-5 + 2e-5 * ref.abs()
    ratio = float((err / lim).max())
    assert bool((err <= lim).all()), f"{what}: worst err / (3e-5 + 2e-5|ref|) = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("model", ["raft", "gma"])
def test_fp32_emulation_meets_the_engine_gate(model):
    """What `pfk_conv1d_wino_f32` computes — U rounded once, B^T / A^T term by term in fp32, an fp32 channel sum per component — on
    the inputs of test_engine_gate_launches' raft / gma cases (seed 17 parameters, tanh h, relu context, randn motion) at 2x55x128:
    every z, r*h and h of both SepConvGRU passes inside that test's gate, each launch against fp64 restated on what it consumed."""
    from ptlflow_amd.synth import synth_update_block_params
    from ptlflow_amd.update import basic_spec, gma_spec
    spec = {"raft": basic_spec, "gma": gma_spec}[model]()
    P = synth_update_block_params(spec, seed=17)
    b, hh, ww = 2, 55, 128
    Ch, Ci, real = spec.hidden, spec.context, spec.x_channels - spec.context
    g = torch.Generator().manual_seed(23)
    h = torch.tanh(torch.randn(b, Ch, hh, ww, generator=g))
    inp = torch.relu(torch.randn(b, Ci, hh, ww, generator=g))
    motion = torch.randn(b * hh * ww, real, generator=g).reshape(b, hh, ww, real).permute(0, 3, 1, 2).contiguous()
    worst = 0.0
    for kh, kw, sfx in spec.gru_passes:
        pad = (kh // 2, kw // 2)
        wz, wr, wq = (P[f"gru.conv{k}{sfx}.weight"].float() for k in "zrq")
        bz, br, bq = (P[f"gru.conv{k}{sfx}.bias"].float() for k in "zrq")
        wzr, bzr = torch.cat([wz, wr], 0), torch.cat([bz, br])
        rest = [(0, Ch, Ch), (Ch + Ci, real, real)]
        cut = lambda wt: torch.cat([wt[:, :Ch], wt[:, Ch + Ci: Ch + Ci + real]], 1)      # noqa: E731
        # the loop-invariant context rows as `prepare_context` stores them (fp32)
        ctx_zr = F.conv2d(inp, wzr[:, Ch: Ch + Ci], bzr, padding=pad)
        ctx_q = F.conv2d(inp, wq[:, Ch: Ch + Ci], bq, padding=pad)
        Uzr = _unpack(pack_wino1d_weight(wzr, rest), Ch + real, 2 * Ch)[:, : 2 * Ch].float()
        Uq = _unpack(pack_wino1d_weight(wq, rest), Ch + real, Ch)[:, :Ch].float()
        # z | r
        x = torch.cat([h, motion], 1)
        v = f45(x, Uzr, kh == 5, torch.float32) + ctx_zr
        z, rh = torch.sigmoid(v[:, :Ch]), torch.sigmoid(v[:, Ch:]) * h
        v64 = F.conv2d(x.double(), cut(wzr).double(), padding=pad) + ctx_zr.double()
        worst = max(worst, _gate(z, torch.sigmoid(v64[:, :Ch]), f"z{sfx}"), _gate(rh, torch.sigmoid(v64[:, Ch:]) * h.double(), f"rh{sfx}"))
        # q on what z | r stored
        x = torch.cat([rh, motion], 1)
        v = f45(x, Uq, kh == 5, torch.float32) + ctx_q
        hn = (1 - z) * h + z * torch.tanh(v)
        v64 = F.conv2d(x.double(), cut(wq).double(), padding=pad) + ctx_q.double()
        worst = max(worst, _gate(hn, (1 - z.double()) * h.double() + z.double() * torch.tanh(v64), f"h{sfx}"))
        h = hn
    print(f"[ratio] {model} F(4,5) fp32 emulation, worst err / limit {worst:.3f}")
    assert worst <= 0.5, "the GPU gate must be reachable with a margin"


@pytest.fixture(scope="module")
def lib():
    return pfk_ctypes.lib()


def test_weight_size_helper(lib):
    lib.pfk_conv_wino1d_weight_floats.restype = ctypes.c_longlong
    assert lib.pfk_conv_wino1d_weight_floats(256, 256) == 8 * 256 * 256
    assert lib.pfk_conv_wino1d_weight_floats(40, 126) == 8 * 40 * 128
    assert lib.pfk_conv_wino1d_weight_floats(36, 64) == -1
    assert lib.pfk_conv_wino1d_weight_floats(0, 64) == -1
    assert lib.pfk_abi_version() == 7


def test_argument_validation_without_gpu(lib):
    """every refusal happens on the host before any device call (fake, never dereferenced pointers)"""
    BAD_ARG, ALIGNMENT, UNSUPPORTED = -1, -2, -3
    f = lib.pfk_conv1d_wino_f32
    assert f(None, None) == BAD_ARG

    def desc(epi=0, **kw):
        d = _Desc()
        d.src[0] = _Src(0x10000, 64, 32)
        d.src[1] = _Src(0x10080, 64, 32)
        d.num_src, d.B, d.H, d.W, d.kh, d.kw = 2, 1, 6, 8, 1, 5
        d.weight, d.cout, d.epilogue, d.relu, d.scale = 0x20000, 64, epi, 0, 1.0
        if epi == 0:
            d.out, d.out_ld = 0x30000, 64
        else:
            d.h, d.h_ld, d.aux_z, d.aux_rh = 0x40000, 64, 0x50000, 0x60000
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw in [dict(kh=3, kw=3), dict(kh=1, kw=1), dict(kh=5, kw=5), dict(kh=1, kw=3), dict(stride=2), dict(epilogue=3), dict(num_src=3), dict(num_src=0),
               dict(residual=0x70000, residual_ld=64), dict(relu_after_residual=1), dict(cout=128, out_ld=128, cout_active=64)]:
        assert f(ctypes.byref(desc(**kw)), None) == UNSUPPORTED, kw
    d = desc()
    d.src[1] = _Src(0x10080, 64, 36)                         # channels not a multiple of 8
    assert f(ctypes.byref(d), None) == UNSUPPORTED
    d = desc(B=1 << 12, H=1 << 10, W=1 << 8)                 # 2^30 pixels x 64 floats: past 32-bit byte offsets
    assert f(ctypes.byref(d), None) == UNSUPPORTED
    for kw in [dict(weight=None), dict(out=None), dict(B=0), dict(cout=0), dict(out_ld=32)]:
        assert f(ctypes.byref(desc(**kw)), None) == BAD_ARG, kw
    d = desc()
    d.src[0] = _Src(None, 64, 32)
    assert f(ctypes.byref(d), None) == BAD_ARG
    d = desc()
    d.src[0] = _Src(0x10000, 16, 32)                         # ld < channels
    assert f(ctypes.byref(d), None) == BAD_ARG
    for epi in (1, 2):
        for kw in [dict(h=None), dict(aux_z=None), dict(h_ld=16), dict(residual=0x70000, residual_ld=32)]:
            assert f(ctypes.byref(desc(epi, **kw)), None) == BAD_ARG, (epi, kw)
    assert f(ctypes.byref(desc(1, aux_rh=None)), None) == BAD_ARG
    assert f(ctypes.byref(desc(1, cout=63)), None) == BAD_ARG
    assert f(ctypes.byref(desc(weight=0x20004)), None) == ALIGNMENT
    assert f(ctypes.byref(desc(out=0x30002)), None) == ALIGNMENT
    assert f(ctypes.byref(desc(2, residual=0x70001, residual_ld=64)), None) == ALIGNMENT
    d = desc()
    d.src[0] = _Src(0x10001, 64, 32)
    assert f(ctypes.byref(d), None) == ALIGNMENT
