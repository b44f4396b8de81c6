"""pfk_conv2d_wino_f32 (Winograd F(2x2,3x3), torch.ops.pfk.conv2d_wino) against an fp64 CPU convolution, and the engine's use of it
for the update block's `fm`, `c2` and `cv` convolutions.

Error gate: the Winograd kernel's max |error| vs fp64 is at most 4x the direct kernel's (`pfk_conv2d_f32`) on the same inputs."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import raft_oracle as O
from pfk_ctypes import Desc as _Desc, Src as _Src
from op_gate import pm, unpm

pytestmark = pytest.mark.gpu

EPI_LINEAR = 0
RATIO = 4.0


def _case(B, H, W, cin, cout, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    bias = torch.randn(cout, generator=g)
    return x, wt, bias


def _ref64(x, wt, bias, relu, scale):
    r = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    if relu:
        r = F.relu(r)
    return r * scale


def _wino(src, B, H, W, wt, bias, cout, relu, scale, out=None, cout_active=0):
    from ptlflow_amd.packing import pack_wino_weight
    if out is None:
        out = torch.zeros(B * H * W, cout, device=src.device)
    torch.ops.pfk.conv2d_wino(src, B, H, W, pack_wino_weight(wt).cuda(), bias.cuda(), cout, relu, scale, out, cout_active)
    return out


def _direct(src, B, H, W, wt, bias, cout, relu, scale):
    from ptlflow_amd.packing import pack_conv_weight
    cin = wt.shape[1]
    out = torch.zeros(B * H * W, cout, device=src.device)
    torch.ops.pfk.conv2d([src], B, H, W, 3, 3, pack_conv_weight(wt, [(0, cin, cin)]).cuda(), bias.cuda(), cout, EPI_LINEAR, relu,
                         scale, out, None, None, None)
    return out


def _check(B, H, W, cin, cout, relu, scale):
    x, wt, bias = _case(B, H, W, cin, cout)
    src = pm(x, "cuda")
    ref = _ref64(x, wt, bias, relu, scale)
    ew = (unpm(_wino(src, B, H, W, wt, bias, cout, relu, scale), B, H, W).double() - ref).abs().max().item()
    ed = (unpm(_direct(src, B, H, W, wt, bias, cout, relu, scale), B, H, W).double() - ref).abs().max().item()
    print(f"B{B} {H}x{W} {cin}->{cout}: wino max err {ew:.3e}, direct {ed:.3e}, ratio {ew / max(ed, 1e-30):.2f}")
    assert ew <= RATIO * ed + 1e-6, f"wino max err {ew:.3e} vs direct {ed:.3e}"
    return ew, ed


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("cin,cout", [(128, 512), (256, 192), (256, 126)])
def test_update_block_shapes(gpu, B, cin, cout):
    """fm (128 -> 512), c2 (256 -> 192), cv (256 -> 126) at 55x128"""
    _check(B, 55, 128, cin, cout, True, 1.0)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 3), (3, 5), (5, 1), (5, 5), (2, 2), (3, 3)])
def test_tiny_and_odd(gpu, H, W):
    _check(2, H, W, 32, 126, False, 0.25)
    _check(1, H, W, 64, 64, True, 1.0)


@pytest.mark.parametrize("relu,scale", [(False, 1.0), (True, 0.25), (False, -2.0)])
def test_epilogue(gpu, relu, scale):
    _check(1, 13, 17, 96, 128, relu, scale)


def test_strided_source_and_channel_slice(gpu):
    """source = a channel slice of a wider buffer (row stride != cin), output = a channel slice: nothing outside it is written"""
    B, H, W, cin, cout = 2, 11, 21, 64, 126
    x, wt, bias = _case(B, H, W, cin, cout)
    M = B * H * W
    wide = torch.randn(M, cin + 40, device=gpu)
    wide[:, 12:12 + cin] = pm(x, "cuda")
    buf = torch.full((M, cout + 12), 5.0, device=gpu)
    out = buf[:, 4:4 + cout]
    _wino(wide[:, 12:12 + cin], B, H, W, wt, bias, cout, True, 1.0, out=out)
    dense = _wino(pm(x, "cuda"), B, H, W, wt, bias, cout, True, 1.0)
    assert torch.equal(out, dense)
    assert bool((buf[:, :4] == 5.0).all()) and bool((buf[:, 4 + cout:] == 5.0).all()), "wrote outside its channel slice"
    ed = (unpm(_direct(pm(x, "cuda"), B, H, W, wt, bias, cout, True, 1.0), B, H, W).double() - _ref64(x, wt, bias, True, 1.0)).abs().max()
    ew = (unpm(out, B, H, W).double() - _ref64(x, wt, bias, True, 1.0)).abs().max()
    assert ew <= RATIO * ed + 1e-6


@pytest.mark.parametrize("B", [1, 8])
def test_cout_active_has_the_full_launch_bits(gpu, B):
    H, W, cin, cout = 55, 128, 128, 512
    x, wt, bias = _case(B, H, W, cin, cout)
    src = pm(x, "cuda")
    full = _wino(src, B, H, W, wt, bias, cout, True, 1.0)
    half = torch.full_like(full, 7.0)
    _wino(src, B, H, W, wt, bias, cout, True, 1.0, out=half, cout_active=256)
    assert torch.equal(half[:, :256], full[:, :256])
    assert bool((half[:, 256:] == 7.0).all()), "cout_active launch wrote past its channels"


def test_deterministic(gpu):
    B, H, W, cin, cout = 8, 55, 128, 256, 192
    x, wt, bias = _case(B, H, W, cin, cout)
    src = pm(x, "cuda")
    a = _wino(src, B, H, W, wt, bias, cout, True, 1.0)
    for _ in range(3):
        assert torch.equal(_wino(src, B, H, W, wt, bias, cout, True, 1.0), a)


def test_unsupported_arguments_return_the_error_status(gpu):
    import ptlflow_amd
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    B, H, W, cin, cout = 1, 6, 8, 64, 64
    M = B * H * W
    x = torch.randn(M, cin, device=gpu)
    w = torch.randn(int(lib.pfk_conv_wino_weight_floats(cin, cout)), device=gpu)
    out = torch.zeros(M, cout, device=gpu)

    def desc(**kw):
        d = _Desc()
        d.src[0] = _Src(x.data_ptr(), cin, cin)
        d.num_src, d.B, d.H, d.W, d.kh, d.kw = 1, B, H, W, 3, 3
        d.weight, d.cout, d.epilogue, d.relu, d.scale = w.data_ptr(), cout, EPI_LINEAR, 1, 1.0
        d.out, d.out_ld = out.data_ptr(), cout
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    UNSUPPORTED = -3
    cases = [desc(kh=1, kw=1), desc(kh=5, kw=5), desc(stride=2), desc(epilogue=1), desc(num_src=2),
             desc(residual=out.data_ptr(), residual_ld=cout), desc(relu_after_residual=1), desc(cout_active=32),
             desc(epilogue=3, relu=0)]
    d = desc()
    d.src[0] = _Src(x.data_ptr(), cin, 48)        # channels % 32 != 0
    cases.append(d)
    for d in cases:
        assert lib.pfk_conv2d_wino_f32(ctypes.byref(d), None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0, "a refused launch wrote its output"
    with pytest.raises(RuntimeError):
        torch.ops.pfk.conv2d_wino(x[:, :48], B, H, W, w, None, cout, True, 1.0, out, 0)
    assert lib.pfk_conv2d_wino_f32(ctypes.byref(desc()), None) == 0
    torch.cuda.synchronize()


def _forward(winograd, H, W, B, iters, seed=1234):
    from ptlflow_amd.raft import RAFT
    model = RAFT(small=False, iters=iters).load_synthetic(seed).eval()
    P = {k: v.clone() for k, v in model.state_dict().items()}
    x = O.smooth_pair(B, H, W, seed)
    model = model.cuda()
    xg = x.cuda()
    model.engine(xg.device).winograd = winograd
    out = model({"images": xg})
    torch.cuda.synchronize()
    return out, P, x


@pytest.mark.parametrize("B", [1, 2])
def test_engine_paths(gpu, B):
    """winograd=False is the direct path bit for bit (a fresh model and the same inputs give the same flows twice); with the
    Winograd path (batch 1: fm only; batch 2: fm, c2, cv) the EPE against the CPU oracle stays inside the gate of
    tests/test_gpu_model.py"""
    from ptlflow_amd.update import WINO_MIN_WORK
    H, W, iters = 436, 1024, 12
    px = ((H + 7) // 8) * ((W + 7) // 8)
    assert px * 3 < WINO_MIN_WORK <= px * 8 and 2 * px * 2 >= WINO_MIN_WORK
    off_a, P, x = _forward(False, H, W, B, iters)
    off_b, _, _ = _forward(False, H, W, B, iters)
    assert torch.equal(off_a["flows"], off_b["flows"])
    on, _, _ = _forward(True, H, W, B, iters)
    from _cpu_cache import cpu_forward
    ref = cpu_forward("raft", P, x, iters, small=False, key=("synthetic", 1234, "smooth", 1234, B))
    mean, mx = O.epe(on["flows"][:, 0].cpu(), ref["flows"][:, 0])
    mean_d, mx_d = O.epe(off_a["flows"][:, 0].cpu(), ref["flows"][:, 0])
    print(f"EPE vs CPU oracle: winograd mean {mean:.3e} max {mx:.3e}; direct mean {mean_d:.3e} max {mx_d:.3e}")
    assert mean <= 1e-3 and mx <= 1e-2, f"EPE mean {mean:.2e} max {mx:.2e}"
    assert not torch.equal(on["flows"], off_a["flows"]), "the Winograd path was not taken"
