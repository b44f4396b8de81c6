"""Training SEA-RAFT's ConvNeXt block and heads on bf16 rows (K12f): the five `_b16` entries (`pfk_dwconv_layernorm_train_b16`,
`pfk_layernorm_bwd_b16`, `pfk_dwconv_bwd_b16`, `pfk_gelu_b16` / `pfk_gelu_bwd_b16`), the two autograd nodes on them, the compositions of
ptlflow_amd/train_sea.py with ``precision="bf16"`` and the seam
``accelerate(model, sea_raft_update=True, sea_raft_train=True, train_precision="bf16")``.

Gates.
* Kernels: the reference is float64 on each kernel's OWN inputs (bf16 values, fp32 parameters).  bf16 outputs: `within_ulp` of
  tests/op_gate.py with a 2^-16 floor, |got - bf16(ref)| <= 1 bf16 ulp + floor; fp32 outputs (rstd, dgamma, dbeta,
  dweight, dbias): the project's op gate, relative L2 <= 5e-6; `out` `torch.equal` to `ops.dwconv_layernorm_b16`.  The harness is
  tests/op_gate.py's on bf16 buffers: NaN in the pad columns of the inputs, a sentinel in the pad columns of the outputs
  and past the last row, the same bits on a second run.
* Nodes, compositions and the whole loop: `within_2x_cpu_autocast` of tests/op_gate.py — for every output and
  gradient tensor the L2-relative error against float64 is at most 2x the error of the same torch modules (tests/sea_seam_model.py)
  on the CPU under ``torch.autocast("cpu", bfloat16)``, nothing skipped.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from op_gate import OP_TOL, SENTINEL, Rows, leaf, nchw, pm, rel, within_2x_cpu_autocast, within_ulp
from op_refs import dwconv_bwd_ref, gelu_bwd_ref, layernorm_bwd_ref

pytestmark = pytest.mark.gpu
ULP_FLOOR = 2.0 ** -16
BF = torch.bfloat16

# (B, H, W, C): smaller than a tile and than the 7x7 halo, two images | ragged tiles both ways, image boundary | exact tiles, a 32 + 8
# channel chunk | minimum size | maximum C
SHAPES = [(2, 1, 5, 384), (2, 13, 17, 384), (1, 8, 16, 40), (1, 4, 8, 8), (1, 9, 33, 512)]
CASES = [(*s, 7) for s in SHAPES] + [(2, 13, 17, 384, 3)]


def ulp_ok(got, ref, what):
    try:
        within_ulp(got.detach().cpu(), ref, ULP_FLOOR)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


@functools.lru_cache(maxsize=None)
def case(B, H, W, C, k):
    """bf16 inputs of the three kernels and their float64 references, computed once per shape on the CPU.  Each kernel's reference is
    float64 arithmetic on that kernel's own inputs: bf16 x, dy; x^ and du are the float64 values rounded to bf16, rstd to fp32."""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W + C + k)
    M = B * H * W
    d = {"x": torch.randn(M, C, generator=g).to(BF), "w": torch.randn(C, k * k, generator=g) / k, "b": 0.1 * torch.randn(C, generator=g),
         "gamma": 1 + 0.2 * torch.randn(C, generator=g), "beta": 0.1 * torch.randn(C, generator=g),
         "dy": torch.randn(M, C, generator=g).to(BF)}
    d["gamma"][C // 2] = 0.0           # a LayerNorm weight of exactly zero
    x64 = d["x"].double().view(B, H, W, C).permute(0, 3, 1, 2)
    u = F.conv2d(x64, d["w"].double().view(C, 1, k, k), d["b"].double(), padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(M, C)
    mean, var = u.mean(1, keepdim=True), u.var(1, unbiased=False, keepdim=True)
    rstd = (var + 1e-6).rsqrt()
    xhat = (u - mean) * rstd
    d["xhat_ref"], d["rstd_ref"] = xhat, rstd[:, 0]
    d["out_ref"] = xhat * d["gamma"].double() + d["beta"].double()
    d["xhat"], d["rstd"] = xhat.to(BF), rstd[:, 0].float()
    d["du_ref"], d["dgamma_ref"], d["dbeta_ref"] = layernorm_bwd_ref(d["xhat"].double(), d["rstd"].double(), d["gamma"].double(), d["dy"].double())
    d["du"] = d["du_ref"].to(BF)
    dx, dw, db = dwconv_bwd_ref(d["x"].double(), d["du"].double(), d["w"].double().view(C, k, k), B, H, W)
    d["dx_ref"], d["dw_ref"], d["db_ref"] = dx, dw.reshape(C, k * k), db
    return d


# ---------------------------------------------------------------------------------------------------------------------
# (a) pfk_dwconv_layernorm_train_b16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,k", CASES)
def test_dwconv_layernorm_train_b16(gpu, B, H, W, C, k):
    ops = torch.ops.pfk
    d = case(B, H, W, C, k)
    M = B * H * W
    x = Rows(M, C, gpu, d["x"], pad=8, dtype=BF)
    par = [d[n].to(gpu) for n in ("w", "b", "gamma", "beta")]

    def run():
        out, xhat = Rows(M, C, gpu, pad=16, dtype=BF), Rows(M, C, gpu, pad=24, dtype=BF)
        rstd = torch.full((M + 64,), SENTINEL, device=gpu)
        ops.dwconv_layernorm_train_b16(x.rows, *par, 1e-6, out.rows, xhat.rows, rstd[:M], B, H, W, k)
        return out, xhat, rstd

    out, xhat, rstd = run()
    want = torch.empty(M, C, device=gpu, dtype=BF)
    ops.dwconv_layernorm_b16(x.rows, *par, 1e-6, want, B, H, W, k)
    torch.cuda.synchronize()
    out.check_untouched("out"), xhat.check_untouched("xhat")
    assert bool((rstd[M:] == SENTINEL).all()), "rstd: memory past the last pixel was written"
    assert torch.equal(out.rows, want), "out differs from pfk_dwconv_layernorm_b16's bits"
    e = rel(rstd[:M], d["rstd_ref"])
    print("dwconv_layernorm_train_b16 %s k %d: relL2 out %.2e xhat %.2e rstd %.2e" %
          ((B, H, W, C), k, rel(out.rows, d["out_ref"]), rel(xhat.rows, d["xhat_ref"]), e))
    ulp_ok(out.rows, d["out_ref"], "out")
    ulp_ok(xhat.rows, d["xhat_ref"], "xhat")
    assert e <= OP_TOL
    # x^ is saved as such: the channel whose LayerNorm weight is zero has it too
    assert float(xhat.rows[:, C // 2].float().abs().max()) > 0
    out2, xhat2, rstd2 = run()
    assert torch.equal(out2.flat, out.flat) and torch.equal(xhat2.flat, xhat.flat) and torch.equal(rstd2, rstd)


# ---------------------------------------------------------------------------------------------------------------------
# (b) pfk_layernorm_bwd_b16
# ---------------------------------------------------------------------------------------------------------------------
def _run_layernorm_bwd(gpu, xhat, rstd, gamma, dy, refs, what):
    ops = torch.ops.pfk
    M, C = xhat.shape
    xh, dyr = Rows(M, C, gpu, xhat, pad=8, dtype=BF), Rows(M, C, gpu, dy, pad=24, dtype=BF)
    rs, gm = rstd.to(gpu), gamma.to(gpu)

    def run():
        du = Rows(M, C, gpu, pad=16, dtype=BF)
        vec = torch.full((2 * C + 64,), SENTINEL, device=gpu)
        ops.layernorm_bwd_b16(xh.rows, rs, gm, dyr.rows, du.rows, vec[:C], vec[C:2 * C])
        return du, vec

    du, vec = run()
    torch.cuda.synchronize()
    du.check_untouched("du")
    assert bool((vec[2 * C:] == SENTINEL).all())
    e = (rel(vec[:C], refs[1]), rel(vec[C:2 * C], refs[2]))
    print("layernorm_bwd_b16 %s: relL2 du %.2e dgamma %.2e dbeta %.2e" % (what, rel(du.rows, refs[0]), *e))
    ulp_ok(du.rows, refs[0], "du")
    assert max(e) <= OP_TOL
    du2, vec2 = run()
    assert torch.equal(du2.flat, du.flat) and torch.equal(vec2, vec)


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_layernorm_bwd_b16(gpu, B, H, W, C):
    d = case(B, H, W, C, 7)
    _run_layernorm_bwd(gpu, d["xhat"], d["rstd"], d["gamma"], d["dy"], (d["du_ref"], d["dgamma_ref"], d["dbeta_ref"]), (B, H, W, C))


def test_layernorm_bwd_b16_one_row(gpu):
    g = torch.Generator().manual_seed(9)
    C = 384
    xhat, dy = torch.randn(1, C, generator=g), torch.randn(1, C, generator=g).to(BF)
    xhat = ((xhat - xhat.mean()) / xhat.std(unbiased=False)).to(BF)
    rstd, gamma = torch.tensor([0.7]), 1 + 0.2 * torch.randn(C, generator=g)
    gamma[17] = 0.0
    _run_layernorm_bwd(gpu, xhat, rstd, gamma, dy, layernorm_bwd_ref(xhat.double(), rstd.double(), gamma.double(), dy.double()), "M = 1")


# ---------------------------------------------------------------------------------------------------------------------
# (c) pfk_dwconv_bwd_b16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,k", CASES)
def test_dwconv_bwd_b16(gpu, B, H, W, C, k):
    ops = torch.ops.pfk
    d = case(B, H, W, C, k)
    M = B * H * W
    x, du = Rows(M, C, gpu, d["x"], pad=8, dtype=BF), Rows(M, C, gpu, d["du"], pad=16, dtype=BF)
    w = d["w"].to(gpu)

    def run():
        dx = Rows(M, C, gpu, pad=24, dtype=BF)
        vec = torch.full((C * k * k + C + 64,), SENTINEL, device=gpu)
        ops.dwconv_bwd_b16(x.rows, du.rows, w, dx.rows, vec[:C * k * k], vec[C * k * k:C * k * k + C], B, H, W, k)
        return dx, vec

    dx, vec = run()
    torch.cuda.synchronize()
    dx.check_untouched("dx")
    assert bool((vec[C * k * k + C:] == SENTINEL).all())
    e = (rel(vec[:C * k * k].view(C, k * k), d["dw_ref"]), rel(vec[C * k * k:C * k * k + C], d["db_ref"]))
    print("dwconv_bwd_b16 %s k %d: relL2 dx %.2e dweight %.2e dbias %.2e" % ((B, H, W, C), k, rel(dx.rows, d["dx_ref"]), *e))
    ulp_ok(dx.rows, d["dx_ref"], "dx")
    assert max(e) <= OP_TOL
    dx2, vec2 = run()
    assert torch.equal(dx2.flat, dx.flat) and torch.equal(vec2, vec)
    # dbias is optional
    nb = torch.full((C * k * k + 64,), SENTINEL, device=gpu)
    dx3 = Rows(M, C, gpu, pad=24, dtype=BF)
    ops.dwconv_bwd_b16(x.rows, du.rows, w, dx3.rows, nb[:C * k * k], None, B, H, W, k)
    assert torch.equal(dx3.flat, dx.flat) and torch.equal(nb[:C * k * k], vec[:C * k * k]) and bool((nb[C * k * k:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# (d) pfk_gelu_b16 / pfk_gelu_bwd_b16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(2 * 13 * 17, 512), (3, 8), (37, 40)])
def test_gelu_rows_b16(gpu, M, C):
    ops = torch.ops.pfk
    g = torch.Generator().manual_seed(M + C)
    x, dy = (torch.randn(M, C, generator=g) * 2.5).to(BF), torch.randn(M, C, generator=g).to(BF)
    special = torch.tensor([30.0, -30.0, 1e30, -1e30]).to(BF)     # large |x|: y = x or 0, dx = dy or 0, never NaN
    x[0, :4] = special
    xr, dyr = Rows(M, C, gpu, x, pad=8, dtype=BF), Rows(M, C, gpu, dy, pad=16, dtype=BF)

    def run():
        y, dx = Rows(M, C, gpu, pad=8, dtype=BF), Rows(M, C, gpu, pad=24, dtype=BF)
        ops.gelu_b16(xr.rows, y.rows)
        ops.gelu_bwd_b16(xr.rows, dyr.rows, dx.rows)
        return y, dx

    y, dx = run()
    torch.cuda.synchronize()
    y.check_untouched("y"), dx.check_untouched("dx")
    assert bool(torch.isfinite(y.rows.float()).all()) and bool(torch.isfinite(dx.rows.float()).all())
    keep = torch.tensor([1.0, 0.0, 1.0, 0.0])
    assert torch.equal(y.rows[0, :4].float().cpu(), special.float() * keep)
    assert torch.equal(dx.rows[0, :4].float().cpu(), dy[0, :4].float() * keep)
    x64, dy64 = x.double(), dy.double()
    print("gelu rows b16 %dx%d: relL2 y %.2e dx %.2e" % (M, C, rel(y.rows, F.gelu(x64)), rel(dx.rows, gelu_bwd_ref(x64, dy64))))
    ulp_ok(y.rows, F.gelu(x64), "y")
    ulp_ok(dx.rows, gelu_bwd_ref(x64, dy64), "dx")
    y2, dx2 = run()
    assert torch.equal(y2.flat, y.flat) and torch.equal(dx2.flat, dx.flat)


# ---------------------------------------------------------------------------------------------------------------------
# nodes and compositions: 2x CPU autocast on every tensor
# ---------------------------------------------------------------------------------------------------------------------
BB, BH, BW = 2, 13, 17


def _seeded_block():
    from sea_seam_model import ConvNextBlock, seeded_params
    blk = ConvNextBlock(384, 128)
    blk.load_state_dict(seeded_params({k: tuple(v.shape) for k, v in blk.state_dict().items()}, 5))
    return blk


def _cpu_runs(run):
    """(float64, CPU autocast) results of `run(dtype, autocast)`"""
    return run(torch.float64, False), run(torch.float32, True)


def _block_copy(blk, dtype):
    import copy
    m = copy.deepcopy(blk).to(dtype)
    for p in m.parameters():
        p.grad = None
    return m


def test_dwconv_layernorm_node_bf16(gpu):
    """`ConvNextBlock.dwconv` + `.norm` against `dwconv_layernorm_pm(precision="bf16")`: fp32 rows in (rounded by the node), bf16 out"""
    from ptlflow_amd.train_sea import dwconv_layernorm_pm
    blk = _seeded_block()
    g = torch.Generator().manual_seed(6)
    x, R = torch.randn(BB, 384, BH, BW, generator=g), torch.randn(BB, BH, BW, 384, generator=g)
    names = ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias")

    def cpu(dtype, autocast):
        m, xl = _block_copy(blk, dtype), leaf(x, dtype)
        with torch.autocast("cpu", BF, enabled=autocast):
            y = m.norm(m.dwconv(xl).permute(0, 2, 3, 1))
        y.backward(R.to(y.dtype))
        P = dict(m.named_parameters())
        return {"out": y.detach().permute(0, 3, 1, 2), "d/dx": xl.grad, **{"d/d" + n: P[n].grad for n in names}}

    ref64, cpu16 = _cpu_runs(cpu)
    P = {n: p.detach().to(gpu).requires_grad_() for n, p in blk.named_parameters() if n in names}
    xg = pm(x, gpu).requires_grad_()
    out = dwconv_layernorm_pm(xg, *(P[n] for n in names), BB, BH, BW, precision="bf16")
    assert out.dtype == BF
    out.backward(R.reshape(-1, 384).to(gpu).to(BF))
    assert xg.grad.dtype == torch.float32 and all(p.grad.dtype == torch.float32 for p in P.values())
    assert P["dwconv.weight"].grad.shape == (384, 1, 7, 7)
    within_2x_cpu_autocast({"out": nchw(out, BB, BH, BW), "d/dx": nchw(xg.grad, BB, BH, BW), **{"d/d" + n: P[n].grad for n in names}}, ref64, cpu16)


def test_gelu_node_bf16(gpu):
    """`gelu_pm(precision="bf16")` where the block has it: behind pwconv1, whose bf16 output is what nn.GELU() sees under autocast
    (on an fp32 tensor autocast leaves GELU in fp32 and there is no 16-bit arithmetic to compare with)"""
    from ptlflow_amd.train import conv_pm
    from ptlflow_amd.train_sea import gelu_pm
    blk = _seeded_block()
    g = torch.Generator().manual_seed(3)
    M = BB * BH * BW
    x, R = torch.randn(M, 384, generator=g), torch.randn(M, 512, generator=g)

    def cpu(dtype, autocast):
        m, xl = _block_copy(blk, dtype), leaf(x, dtype)
        with torch.autocast("cpu", BF, enabled=autocast):
            y = m.act(m.pwconv1(xl))
        y.backward(R.to(y.dtype))
        return {"y": y.detach(), "d/dx": xl.grad, "d/dpwconv1.weight": m.pwconv1.weight.grad, "d/dpwconv1.bias": m.pwconv1.bias.grad}

    ref64, cpu16 = _cpu_runs(cpu)
    w, b = (p.detach().to(gpu).requires_grad_() for p in (blk.pwconv1.weight, blk.pwconv1.bias))
    xg = x.to(gpu).requires_grad_()
    a = conv_pm([xg], w[:, :, None, None], b, BB, BH, BW, precision="bf16")
    y = gelu_pm(a, "bf16")
    assert a.dtype == BF and y.dtype == BF
    y.backward(R.to(gpu).to(BF))
    within_2x_cpu_autocast({"y": y, "d/dx": xg.grad, "d/dpwconv1.weight": w.grad, "d/dpwconv1.bias": b.grad}, ref64, cpu16)


def test_convnext_block_bf16(gpu):
    from ptlflow_amd.train_sea import convnext_block_train_pm
    blk = _seeded_block()
    g = torch.Generator().manual_seed(6)
    x, R = torch.randn(BB, 384, BH, BW, generator=g), torch.randn(BB, 128, BH, BW, generator=g)

    def cpu(dtype, autocast):
        m, xl = _block_copy(blk, dtype), leaf(x, dtype)
        with torch.autocast("cpu", BF, enabled=autocast):
            y = m(xl)
        (y * R.to(dtype)).sum().backward()
        return {"out": y.detach(), "d/dx": xl.grad, **{"d/d" + n: p.grad for n, p in m.named_parameters()}}

    ref64, cpu16 = _cpu_runs(cpu)
    for out_fp32 in (True, False):
        P = {"b." + n: p.detach().to(gpu).requires_grad_() for n, p in blk.named_parameters()}
        xg = pm(x, gpu).requires_grad_()
        out = convnext_block_train_pm(P, "b.", xg, BB, BH, BW, precision="bf16", out_fp32=out_fp32)
        assert out.dtype == (torch.float32 if out_fp32 else BF)
        (out * pm(R, gpu)).sum().backward()
        assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in P.values())
        print(f"convnext block, out_fp32={out_fp32}")
        within_2x_cpu_autocast({"out": nchw(out, BB, BH, BW), "d/dx": nchw(xg.grad, BB, BH, BW), **{"d/d" + n[2:]: p.grad for n, p in P.items()}}, ref64, cpu16)


PARTS = ("update_block", "flow_head", "upsample_weight")


@functools.lru_cache(maxsize=None)
def chained_reference():
    """the stand-in at (2, 13, 17), two chained update-block calls and both heads: inputs, and the float64 and CPU-autocast results"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    model = load_seeded(SeaRaftLoop(), 31)
    g = torch.Generator().manual_seed(32)
    x = {"net": torch.tanh(torch.randn(BB, 128, BH, BW, generator=g)), "inp": torch.relu(torch.randn(BB, 128, BH, BW, generator=g)),
         "corr": torch.randn(BB, 324, BH, BW, generator=g), "flow": torch.randn(BB, 2, BH, BW, generator=g) * 2}
    R = [torch.randn(BB, c, BH, BW, generator=g) for c in (128, 6, 576)]
    parts = PARTS

    def cpu(dtype, autocast):
        m = _block_copy(model, dtype)
        net = leaf(x["net"], dtype)
        inp, corr, flow = (x[k].to(dtype) for k in ("inp", "corr", "flow"))
        with torch.autocast("cpu", BF, enabled=autocast):
            h = m.update_block(m.update_block(net, inp, corr, flow), inp, corr, flow)
            fh, uw = m.flow_head(h), m.upsample_weight(h)
        ((h * R[0].to(dtype)).sum() + (fh * R[1].to(dtype)).sum() + (0.25 * uw * R[2].to(dtype)).sum()).backward()
        out = {"h": h.detach(), "flow_head": fh.detach(), "upsample_weight": uw.detach(), "d/dnet": net.grad}
        out.update({f"d/d{part}.{n}": p.grad for part in parts for n, p in getattr(m, part).named_parameters()})
        return out

    ref64, cpu16 = _cpu_runs(cpu)
    return model, x, R, ref64, cpu16


def test_two_chained_update_blocks_and_heads_bf16(gpu):
    """two chained `sea_update_block_train` calls (h fed back, one cache: `inp` is cast once) plus both heads at B = 2, 13 x 17: h, both
    heads, d/dnet and all 40 parameter gradients"""
    from ptlflow_amd.sea_update import sea_spec
    from ptlflow_amd.train_sea import sea_head_train, sea_update_block_train
    model, x, R, ref64, cpu16 = chained_reference()
    parts = PARTS
    assert len(ref64) == 44
    P = {part: {n: p.detach().to(gpu).requires_grad_() for n, p in getattr(model, part).named_parameters()} for part in parts}
    net = x["net"].to(gpu).requires_grad_()
    inp, corr, flow = (x[k].to(gpu) for k in ("inp", "corr", "flow"))
    cache, spec = {}, sea_spec(324)
    h = sea_update_block_train(P["update_block"], spec, net, inp, corr, flow, 2, cache, "bf16")
    assert "inp_rows" in cache
    cast = cache["inp_rows"][2]
    h = sea_update_block_train(P["update_block"], spec, h, inp, corr, flow, 2, cache, "bf16")
    assert cache["inp_rows"][2] is cast, "the context rows were cast again for the second call of the same forward"
    fh, uw = (sea_head_train({f"{n}.{k}": v for k, v in P[n].items()}, n, h, cache, "bf16") for n in parts[1:])
    assert h.dtype == fh.dtype == uw.dtype == torch.float32
    Rg = [r.to(gpu) for r in R]
    ((h * Rg[0]).sum() + (fh * Rg[1]).sum() + (0.25 * uw * Rg[2]).sum()).backward()
    got = {"h": h, "flow_head": fh, "upsample_weight": uw, "d/dnet": net.grad}
    for part in parts:
        for n, p in P[part].items():
            assert p.grad is not None and p.grad.dtype == torch.float32, (part, n)
            got[f"d/d{part}.{n}"] = p.grad
    within_2x_cpu_autocast(got, ref64, cpu16, expect=[k for k in ref64 if k.startswith("d/d")])


# ---------------------------------------------------------------------------------------------------------------------
# the seam
# ---------------------------------------------------------------------------------------------------------------------
def test_seam_block_call_train_precision(gpu):
    """`accelerate(..., sea_raft_train=True, train_precision="bf16")`: a call of the update block and of each head that carries a gradient
    graph runs the bf16 composition; a second `accelerate` switches back and the fp32 path is then bit-identical to a model that never
    left it"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    from ptlflow_amd import patch
    from ptlflow_amd.sea_update import PfkSeaRaftUpdateBlock
    models = [load_seeded(SeaRaftLoop(iters=2), 11).to(gpu).train() for _ in range(3)]
    a, a2, b = models
    g = torch.Generator().manual_seed(3)
    B, H, W = 1, 10, 14
    net = torch.tanh(torch.randn(B, 128, H, W, generator=g)).to(gpu)
    inp = torch.relu(torch.randn(B, 128, H, W, generator=g)).to(gpu)
    corr = torch.randn(B, 324, H, W, generator=g).to(gpu)
    flow = (torch.randn(B, 2, H, W, generator=g) * 2).to(gpu)

    def step(m):
        m.zero_grad(set_to_none=True)
        n = net.clone().requires_grad_()
        calls = (m.update_block.train_calls, m.flow_head.train_calls, m.upsample_weight.train_calls)
        h = m.update_block(n, inp, corr, flow)
        fh, uw = m.flow_head(h), m.upsample_weight(h)
        assert (m.update_block.train_calls, m.flow_head.train_calls, m.upsample_weight.train_calls) == tuple(c + 1 for c in calls)
        assert (m.update_block.calls, m.flow_head.calls, m.upsample_weight.calls) == (0, 0, 0)
        (h.square().mean() + fh.square().mean() + uw.square().mean()).backward()
        grads = {k: p.grad.clone() for k, p in m.named_parameters()}
        return (h.detach().clone(), fh.detach().clone(), uw.detach().clone(), n.grad.clone()), grads

    try:
        for m in (a, a2):
            patch.accelerate(m, sea_raft_update=True, sea_raft_train=True, train_upsample=True)
        patch.accelerate(b, sea_raft_update=True, sea_raft_train=True, train_upsample=True, train_precision="bf16")
        assert isinstance(b.update_block, PfkSeaRaftUpdateBlock) and b.update_block.train_precision == "bf16"
        assert a.update_block.train_precision == "fp32"
        outs_b16, grads_b16 = step(b)
        assert len(grads_b16) == len(list(b.parameters())) == 40
        for k, gr in grads_b16.items():
            assert gr.dtype == torch.float32 and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, k
        assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in outs_b16)
        outs_a, grads_a = step(a)
        outs_a2, grads_a2 = step(a2)
        # like with like: two fp32 instances agree bit for bit on this call
        assert all(torch.equal(u, v) for u, v in zip(outs_a, outs_a2)) and all(torch.equal(grads_a[k], grads_a2[k]) for k in grads_a)
        for name, u, v in zip(("net", "flow_head", "upsample_weight"), outs_b16, outs_a):
            assert not torch.equal(u, v), f"{name}: the bf16 path computed fp32's bits: it did not run"
            assert float((u - v).abs().max()) < 0.05 * float(v.abs().max()), name       # bf16 operands: close to the fp32 path
        patch.accelerate(b, sea_raft_update=True, sea_raft_train=True, train_upsample=True, train_precision="fp32")      # switch back
        assert b.update_block.train_precision == "fp32"
        outs_b, grads_b = step(b)
        assert all(torch.equal(u, v) for u, v in zip(outs_a, outs_b))
        assert all(torch.equal(grads_a[k], grads_b[k]) for k in grads_a)
    finally:
        for m in models:
            patch.restore(m)


def _autocast_forward(mod):
    """`mod.forward` inside torch.autocast("cpu", bfloat16): autocast around this module only"""
    inner = mod.forward

    def forward(*args, **kwargs):
        with torch.autocast("cpu", BF):
            return inner(*args, **kwargs)

    mod.forward = forward


def _loop_inputs():
    g = torch.Generator().manual_seed(5)
    B, H, W = 1, 16, 24
    x = [torch.tanh(torch.randn(B, 128, H, W, generator=g)), torch.relu(torch.randn(B, 128, H, W, generator=g)),
         torch.randn(B, 256, H, W, generator=g) * 0.3, torch.randn(B, 256, H, W, generator=g) * 0.3]
    R = {"flows": torch.randn(B, 1, 2, 8 * H, 8 * W, generator=g), "info": torch.randn(B, 4, 8 * H, 8 * W, generator=g),
         "flow_small": torch.randn(B, 2, H, W, generator=g)}
    return x, R


def _loop_run(model, xs, to):
    """forward + backward of the loop: the three outputs, the feature maps' gradients and every parameter's"""
    R = _loop_inputs()[1]
    xs = [t.detach().clone() for t in xs]
    xs[2].requires_grad_(True), xs[3].requires_grad_(True)
    out = model(*xs)
    sum(((out[k] * to(R[k])).sum() for k in R)).backward()
    res = {k: out[k].detach() for k in R}
    res.update({"d/dfmap1": xs[2].grad, "d/dfmap2": xs[3].grad})
    res.update({"d/d" + n: p.grad for n, p in model.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def loop_reference():
    from sea_seam_model import SeaRaftLoop, load_seeded
    x = _loop_inputs()[0]
    ref = load_seeded(SeaRaftLoop(iters=2), 2).double().train()
    ref64 = _loop_run(ref, [t.double() for t in x], lambda t: t.double())
    ac = load_seeded(SeaRaftLoop(iters=2), 2).train()
    for part in PARTS:
        _autocast_forward(getattr(ac, part))
    return ref64, _loop_run(ac, x, lambda t: t)


def test_training_loop_through_the_seam_bf16(gpu):
    """SeaRaftLoop(iters=2).train() at B = 1, 16 x 24 with a fixed linear loss over flows, info and flow_small: the three outputs, every
    parameter's gradient and the feature maps' against the stand-in's CPU float64 run; the CPU-autocast run enters autocast around
    `update_block`, `flow_head` and `upsample_weight` only"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    from ptlflow_amd import patch
    x, R = _loop_inputs()
    ref64, cpu16 = loop_reference()
    model = load_seeded(SeaRaftLoop(iters=2), 2).to(gpu).train()
    patch.accelerate(model, sea_raft_update=True, sea_raft_train=True, train_upsample=True, train_precision="bf16")
    try:
        ub, fh, uw = model.update_block, model.flow_head, model.upsample_weight
        got = _loop_run(model, [t.to(gpu) for t in x], lambda t: t.to(gpu))
        assert (ub.train_calls, fh.train_calls, uw.train_calls) == (2, 3, 3) and (ub.calls, fh.calls, uw.calls) == (0, 0, 0)
        assert model.upsample_data.train_calls == 3
        assert all(got[k].dtype == torch.float32 for k in R)
        assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in model.parameters())
        within_2x_cpu_autocast(got, ref64, cpu16, expect=["d/d" + n for n, _ in model.named_parameters()])
    finally:
        patch.restore(model)
