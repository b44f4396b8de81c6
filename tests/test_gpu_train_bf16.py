"""precision="bf16" of the training nodes (ptlflow_amd/train.py, K12b): `conv_pm`, `_GruPass` and three chained calls of
`update_block_train_pm` against float64 autograd on the CPU.

The yardstick is the reference's own arithmetic in 16 bits, not the code under test: the SAME torch ops on the CPU under
``torch.autocast("cpu", bfloat16)`` (what the reference trains with).  For every output and every gradient tensor the L2-relative
error against float64 must be at most 2x the error of that autocast run on the same tensor — the factor of the bf16 inference
gates (test_gpu_bf16_gate.py, test_gpu_sea_raft_bf16.py).  Denominators are floored as `compare_gradients` does
(test_gpu_train_step.py): a tensor whose true value is numerically zero is measured against 1e-3 of the largest scale in its group."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import raft_oracle as O
from op_gate import leaf, nchw, pm, within_2x_cpu_autocast

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("kh,kw,cins,bufs,cout,relu", [
    (3, 3, (72,), (72,), 96, True),
    (1, 5, (64, 38), (64, 40), 96, False),        # two sources, the second with 2 padding channels
])
def test_conv_pm_bf16(gpu, kh, kw, cins, bufs, cout, relu):
    from ptlflow_amd.train import conv_pm
    torch.manual_seed(7)
    B, H, W = 2, 9, 13
    M = B * H * W
    xs = [torch.randn(B, c, H, W) for c in cins]
    w = torch.randn(cout, sum(cins), kh, kw) / math.sqrt(sum(cins) * kh * kw)
    b = torch.randn(cout) * 0.1
    gout = torch.randn(B, cout, H, W)

    def cpu(dtype, autocast):
        lx = [leaf(x, dtype) for x in xs]
        lw, lb = leaf(w, dtype), leaf(b, dtype)
        with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
            y = F.conv2d(torch.cat(lx, 1), lw, lb, padding=(kh // 2, kw // 2))
            y = F.relu(y) if relu else y
        y.backward(gout.to(y.dtype))
        out = {"out": y, "dW": lw.grad, "db": lb.grad}
        out.update({f"dx{i}": x.grad for i, x in enumerate(lx)})
        return out

    ref64, cpu16 = cpu(torch.float64, False), cpu(torch.float32, True)
    srcs = [F.pad(pm(x), (0, cb - c)).to(gpu).requires_grad_() for x, c, cb in zip(xs, cins, bufs)]
    wg, bg = w.to(gpu).requires_grad_(), b.to(gpu).requires_grad_()
    out = conv_pm(srcs, wg, bg, B, H, W, relu, list(cins), precision="bf16")
    assert out.dtype == torch.bfloat16 and out.shape == (M, cout)
    out.backward(pm(gout).to(gpu).to(out.dtype))
    assert wg.grad.dtype == torch.float32 and bg.grad.dtype == torch.float32
    got = {"out": nchw(out, B, H, W), "dW": wg.grad, "db": bg.grad}
    for i, (s, c) in enumerate(zip(srcs, cins)):
        assert s.grad.dtype == torch.float32 and bool((s.grad[:, c:] == 0).all()), "gradient in a padding channel"
        got[f"dx{i}"] = nchw(s.grad[:, :c], B, H, W)
    within_2x_cpu_autocast(got, ref64, cpu16)


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
def test_gru_pass_bf16(gpu, kh, kw):
    from ptlflow_amd.train import ConvPacks, _Geometry, _GruPass
    torch.manual_seed(11)
    B, H, W, C, xr, xbuf = 1, 8, 20, 128, 130, 136
    h = torch.tanh(torch.randn(B, C, H, W))
    x = torch.randn(B, xr, H, W)
    P = {}
    for k in "zrq":
        P[k + ".weight"] = torch.randn(C, C + xr, kh, kw) / math.sqrt((C + xr) * kh * kw)
        P[k + ".bias"] = torch.randn(C) * 0.1
    gout = torch.randn(B, C, H, W)

    def cpu(dtype, autocast):
        L = {k: leaf(v, dtype) for k, v in P.items()}
        lh, lx = leaf(h, dtype), leaf(x, dtype)
        with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
            hn = O._gru_pass(L, lh, lx, "z", "r", "q", (kh // 2, kw // 2))
        hn.backward(gout.to(hn.dtype))
        out = {"h'": hn, "dh": lh.grad, "dx": lx.grad}
        out.update({"d" + k: v.grad for k, v in L.items()})
        return out

    ref64, cpu16 = cpu(torch.float64, False), cpu(torch.float32, True)
    G = {k: v.to(gpu).requires_grad_() for k, v in P.items()}
    hg = pm(h).to(gpu).requires_grad_()
    xg = F.pad(pm(x), (0, xbuf - xr)).to(gpu).requires_grad_()
    hn = _GruPass.apply(hg, xg.to(torch.bfloat16), G["z.weight"], G["r.weight"], G["q.weight"], G["z.bias"], G["r.bias"], G["q.bias"],
                        _Geometry(B, H, W, kh, kw), xr, ConvPacks(), ConvPacks(), None, None, "bf16")
    assert hn.dtype == torch.float32
    hn.backward(pm(gout).to(gpu))
    assert bool((xg.grad[:, xr:] == 0).all()), "gradient in a padding channel"
    got = {"h'": nchw(hn, B, H, W), "dh": nchw(hg.grad, B, H, W), "dx": nchw(xg.grad[:, :xr], B, H, W)}
    for k, v in G.items():
        assert v.grad is not None and v.grad.dtype == torch.float32, k
        got["d" + k] = v.grad
    within_2x_cpu_autocast(got, ref64, cpu16, expect=["d" + k for k in P])


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_update_block_three_chained_calls_bf16(gpu):
    """h fed back, flow += delta, the step-scoped weight-gradient accumulation (and with it the hoisted context term) on —
    against `oracle.raft_oracle.basic_update_block` chained the same way."""
    from ptlflow_amd.raft import _param_tree
    from ptlflow_amd.synth import synth_state_dict, update_block_shapes
    from ptlflow_amd.train import update_block_train_pm
    from ptlflow_amd.update import basic_spec
    spec = basic_spec()
    holder = _param_tree(update_block_shapes(spec))
    P = synth_state_dict({k: tuple(v.shape) for k, v in holder.state_dict().items()}, seed=19)
    g = torch.Generator().manual_seed(4)
    B, H, W, K = 1, 8, 12, 3
    net = torch.tanh(torch.randn(B, spec.hidden, H, W, generator=g))
    inp = torch.relu(torch.randn(B, spec.context, H, W, generator=g))
    corrs = [torch.randn(B, spec.corr_channels, H, W, generator=g) for _ in range(K)]
    flow0 = torch.randn(B, 2, H, W, generator=g) * 2
    wn, wd, wm = (torch.randn(B, c, H, W, generator=g) for c in (spec.hidden, 2, 576))

    def cpu(dtype, autocast):
        L = {k: leaf(v, dtype) for k, v in P.items()}
        n, i = leaf(net, dtype), leaf(inp, dtype)
        cs = [leaf(c, dtype) for c in corrs]
        h, flow, loss, outs = n, flow0.to(dtype), 0.0, {}
        for k in range(K):
            with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
                h, m, d = O.basic_update_block(L, h, i, cs[k], flow)
            flow = flow + d
            loss = loss + (k + 1) * ((h * wn.to(h)).sum() + (d * wd.to(d)).sum() + (m * wm.to(m)).sum())
            outs.update({f"net{k}": h, f"mask{k}": m, f"delta{k}": d})
        loss.backward()
        outs.update({"d/dnet": n.grad, "d/dinp": i.grad})
        outs.update({f"d/dcorr{k}": c.grad for k, c in enumerate(cs)})
        outs.update({"d/d" + k: v.grad for k, v in L.items()})
        return outs

    ref64, cpu16 = cpu(torch.float64, False), cpu(torch.float32, True)

    L = {k: v.to(gpu).requires_grad_() for k, v in P.items()}
    n, i = pm(net).to(gpu).requires_grad_(), pm(inp).to(gpu).requires_grad_()
    cs = [pm(c).to(gpu).requires_grad_() for c in corrs]
    h, flow, loss, got, cache = n, pm(flow0).to(gpu), 0.0, {}, {}
    wng, wdg, wmg = (pm(t).to(gpu) for t in (wn, wd, wm))
    for k in range(K):
        h, m, d = update_block_train_pm(L, spec, h, i, cs[k], flow, B, H, W, cache, accumulate_wgrad=True, precision="bf16")
        assert h.dtype == m.dtype == d.dtype == torch.float32
        flow = flow + d
        loss = loss + (k + 1) * ((h * wng).sum() + (d * wdg).sum() + (m * wmg).sum())
        got.update({f"net{k}": nchw(h, B, H, W), f"mask{k}": nchw(m, B, H, W), f"delta{k}": nchw(d, B, H, W)})
    loss.backward()
    got.update({"d/dnet": nchw(n.grad, B, H, W), "d/dinp": nchw(i.grad, B, H, W)})
    got.update({f"d/dcorr{k}": nchw(c.grad, B, H, W) for k, c in enumerate(cs)})
    for k, v in L.items():
        assert v.grad is not None and v.grad.dtype == torch.float32, k
        got["d/d" + k] = v.grad
    within_2x_cpu_autocast(got, ref64, cpu16, expect=["d/d" + k for k in holder.state_dict()])


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_bf16_accumulating_and_plain_paths_agree(gpu):
    """Three recurrent uses of one weight: the step-scoped accumulation (`ConvPacks.acc` + `_Flush`, the kernel's accumulate flag)
    hands autograd the same totals as the per-use gradients it replaces (fp32 sums of the same fp32 terms in another order)."""
    from ptlflow_amd.train import conv_pm, packs_for
    g = torch.Generator().manual_seed(4)
    B, H, W, cin, cout = 2, 11, 17, 40, 48
    M = B * H * W
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(gpu)
    b = (torch.randn(cout, generator=g) * 0.1).to(gpu)
    xs = [torch.randn(M, cin, generator=g).to(gpu) for _ in range(3)]

    def grads(accumulate):
        wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        cache = {}
        loss = 0.0
        for k, xi in enumerate(xs):
            y = conv_pm([xi], wp, bp, B, H, W, relu=True, packs=packs_for(cache, "c", [wp], accumulate), precision="bf16")
            loss = loss + (k + 1) * y.float().square().mean()
        loss.backward()
        return wp.grad, bp.grad

    (gw0, gb0), (gw1, gb1) = grads(False), grads(True)
    assert float(gw0.abs().max()) > 0
    assert float((gw1 - gw0).abs().max()) <= 1e-6 * float(gw0.abs().max()) and float((gb1 - gb0).abs().max()) <= 1e-6 * float(gb0.abs().max())


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_one_conv_packs_under_both_precisions(gpu):
    """One `ConvPacks` entry used under fp32, then bf16, then fp32 again keeps each precision's packed weights (forward and data
    gradient) apart: every output and gradient is bit-identical to the same call with a `ConvPacks` of its own — the node that
    tests (a) and (d) above hold against float64 and CPU autocast."""
    from ptlflow_amd.train import ConvPacks, conv_pm
    g = torch.Generator().manual_seed(23)
    B, H, W, cin, cout = 1, 8, 12, 40, 48
    M = B * H * W
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(gpu)
    b = (torch.randn(cout, generator=g) * 0.1).to(gpu)
    x = torch.randn(M, cin, generator=g).to(gpu)               # fp32 rows: the bf16 node casts them
    gout = torch.randn(M, cout, generator=g).to(gpu)

    def run(precision, packs):
        wp, bp, xp = (t.clone().requires_grad_() for t in (w, b, x))
        out = conv_pm([xp], wp, bp, B, H, W, relu=True, packs=packs, precision=precision)
        out.backward(gout.to(out.dtype))
        return {"out": out.detach(), "dW": wp.grad, "db": bp.grad, "dx": xp.grad}

    shared = ConvPacks()
    for precision in ("fp32", "bf16", "fp32"):
        got, want = run(precision, shared), run(precision, ConvPacks())
        for name, t in want.items():
            assert t is not None and bool(t.isfinite().all()) and float(t.float().abs().max()) > 0, (precision, name)
            assert got[name].dtype == t.dtype and torch.equal(got[name], t), f"{precision}: {name} differs with the shared ConvPacks"
    assert {k[0] for k in shared.packed} == {"fp32", "bf16"}
