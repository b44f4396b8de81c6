"""Training SEA-RAFT's ConvNeXt block and heads on the kernels (K12d): the four new entries (`pfk_dwconv_layernorm_train_f32`,
`pfk_layernorm_bwd_f32`, `pfk_dwconv_bwd_f32`, `pfk_gelu_f32` / `pfk_gelu_bwd_f32`), the two autograd nodes on them, the block
compositions of ptlflow_amd/train_sea.py and the seam `accelerate(model, sea_raft_update=True, sea_raft_train=True)`.

Gates.  Kernels and nodes: relative L2 <= 5e-6 against float64 torch on the CPU ON THE KERNEL'S OWN INPUTS (the project's fp32 op gate);
the train forward's `out` must be `torch.equal` to `ops.dwconv_layernorm`.  Blocks and seam: 5e-4 of each tensor's scale against the
torch stand-in (tests/sea_seam_model.py) in float64 (tests/test_gpu_train.py::test_update_block_training_step's gate).  The kernel tests
use tests/op_gate.py's harness: NaN in the pad columns of the inputs, a sentinel in the pad columns of the outputs and past
the last row, the same bits on a second run.

Measured on an MI355X: every kernel and node output <= 1.7e-7 (dweight <= 1.3e-7, dgamma <= 1.7e-7: no weight-gradient reduction needed
another gate); blocks, fixture replay and the loop <= 4.3e-6 of scale."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from op_gate import BLOCK_TOL, OP_TOL, SENTINEL, Rows, nchw, pm, rel, scale_close
from op_refs import dwconv_bwd_ref, gelu_bwd_ref, layernorm_bwd_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sea_raft_update_grad.pt")

# (B, H, W, C): smaller than a tile and than the 7x7 halo, two images | ragged tiles both ways, image boundary | exact tiles, a 32 + 4
# channel chunk | minimum size | maximum C
SHAPES = [(2, 1, 5, 384), (2, 13, 17, 384), (1, 8, 16, 36), (1, 4, 8, 4), (1, 9, 33, 512)]
CASES = [(*s, 7) for s in SHAPES] + [(2, 13, 17, 384, 3)]


@functools.lru_cache(maxsize=None)
def case(B, H, W, C, k):
    """fp32 inputs of the three kernels and their float64 references, computed once per shape on the CPU.  Each kernel's reference
    is float64 arithmetic on that kernel's own fp32 inputs (x^, rstd and du are the rounded float64 values)."""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W + C + k)
    M = B * H * W
    d = {"x": torch.randn(M, C, generator=g), "w": torch.randn(C, k * k, generator=g) / k, "b": 0.1 * torch.randn(C, generator=g),
         "gamma": 1 + 0.2 * torch.randn(C, generator=g), "beta": 0.1 * torch.randn(C, generator=g), "dy": torch.randn(M, C, generator=g)}
    d["gamma"][C // 2] = 0.0           # a LayerNorm weight of exactly zero
    x64 = d["x"].double().view(B, H, W, C).permute(0, 3, 1, 2)
    u = F.conv2d(x64, d["w"].double().view(C, 1, k, k), d["b"].double(), padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(M, C)
    mean, var = u.mean(1, keepdim=True), u.var(1, unbiased=False, keepdim=True)
    rstd = (var + 1e-6).rsqrt()
    xhat = (u - mean) * rstd
    d["xhat_ref"], d["rstd_ref"] = xhat, rstd[:, 0]
    d["out_ref"] = xhat * d["gamma"].double() + d["beta"].double()
    d["xhat"], d["rstd"] = xhat.float(), rstd[:, 0].float()
    d["du_ref"], d["dgamma_ref"], d["dbeta_ref"] = layernorm_bwd_ref(d["xhat"].double(), d["rstd"].double(), d["gamma"].double(), d["dy"].double())
    d["du"] = d["du_ref"].float()
    dx, dw, db = dwconv_bwd_ref(d["x"].double(), d["du"].double(), d["w"].double().view(C, k, k), B, H, W)
    d["dx_ref"], d["dw_ref"], d["db_ref"] = dx, dw.reshape(C, k * k), db
    return d


# ---------------------------------------------------------------------------------------------------------------------
# (a) pfk_dwconv_layernorm_train_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,k", CASES)
def test_dwconv_layernorm_train(gpu, B, H, W, C, k):
    ops = torch.ops.pfk
    d = case(B, H, W, C, k)
    M = B * H * W
    x = Rows(M, C, gpu, d["x"])
    par = [d[n].to(gpu) for n in ("w", "b", "gamma", "beta")]

    def run():
        out, xhat = Rows(M, C, gpu), Rows(M, C, gpu, pad=8)
        rstd = torch.full((M + 64,), SENTINEL, device=gpu)
        ops.dwconv_layernorm_train(x.rows, *par, 1e-6, out.rows, xhat.rows, rstd[:M], B, H, W, k)
        return out, xhat, rstd

    out, xhat, rstd = run()
    want = torch.empty(M, C, device=gpu)
    ops.dwconv_layernorm(x.rows, *par, 1e-6, want, B, H, W, k)
    torch.cuda.synchronize()
    out.check_untouched("out"), xhat.check_untouched("xhat")
    assert bool((rstd[M:] == SENTINEL).all()), "rstd: memory past the last pixel was written"
    assert torch.equal(out.rows, want), "out differs from pfk_dwconv_layernorm_f32's bits"
    e = (rel(out.rows, d["out_ref"]), rel(xhat.rows, d["xhat_ref"]), rel(rstd[:M], d["rstd_ref"]))
    print("dwconv_layernorm_train %s k %d: relL2 out %.2e xhat %.2e rstd %.2e" % ((B, H, W, C), k, *e))
    assert max(e) <= OP_TOL
    # x^ is saved as such: the channel whose LayerNorm weight is zero has it too
    assert rel(xhat.rows[:, C // 2], d["xhat_ref"][:, C // 2]) <= OP_TOL * 10 and float(xhat.rows[:, C // 2].abs().max()) > 0
    out2, xhat2, rstd2 = run()
    assert torch.equal(out2.flat, out.flat) and torch.equal(xhat2.flat, xhat.flat) and torch.equal(rstd2, rstd)


# ---------------------------------------------------------------------------------------------------------------------
# (b) pfk_layernorm_bwd_f32
# ---------------------------------------------------------------------------------------------------------------------
def _run_layernorm_bwd(gpu, xhat, rstd, gamma, dy, refs, what):
    ops = torch.ops.pfk
    M, C = xhat.shape
    xh, dyr = Rows(M, C, gpu, xhat), Rows(M, C, gpu, dy, pad=12)
    rs, gm = rstd.to(gpu), gamma.to(gpu)

    def run():
        du = Rows(M, C, gpu, pad=8)
        vec = torch.full((2 * C + 64,), SENTINEL, device=gpu)
        ops.layernorm_bwd(xh.rows, rs, gm, dyr.rows, du.rows, vec[:C], vec[C:2 * C])
        return du, vec

    du, vec = run()
    torch.cuda.synchronize()
    du.check_untouched("du")
    assert bool((vec[2 * C:] == SENTINEL).all())
    e = (rel(du.rows, refs[0]), rel(vec[:C], refs[1]), rel(vec[C:2 * C], refs[2]))
    print("layernorm_bwd %s: relL2 du %.2e dgamma %.2e dbeta %.2e" % (what, *e))
    assert max(e) <= OP_TOL
    du2, vec2 = run()
    assert torch.equal(du2.flat, du.flat) and torch.equal(vec2, vec)


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_layernorm_bwd(gpu, B, H, W, C):
    d = case(B, H, W, C, 7)
    _run_layernorm_bwd(gpu, d["xhat"], d["rstd"], d["gamma"], d["dy"], (d["du_ref"], d["dgamma_ref"], d["dbeta_ref"]), (B, H, W, C))


def test_layernorm_bwd_one_row(gpu):
    g = torch.Generator().manual_seed(9)
    C = 384
    xhat, dy = torch.randn(1, C, generator=g), torch.randn(1, C, generator=g)
    xhat = (xhat - xhat.mean()) / xhat.std(unbiased=False)
    rstd, gamma = torch.tensor([0.7]), 1 + 0.2 * torch.randn(C, generator=g)
    gamma[17] = 0.0
    _run_layernorm_bwd(gpu, xhat, rstd, gamma, dy, layernorm_bwd_ref(xhat.double(), rstd.double(), gamma.double(), dy.double()), "M = 1")


# ---------------------------------------------------------------------------------------------------------------------
# (c) pfk_dwconv_bwd_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,k", CASES)
def test_dwconv_bwd(gpu, B, H, W, C, k):
    ops = torch.ops.pfk
    d = case(B, H, W, C, k)
    M = B * H * W
    x, du = Rows(M, C, gpu, d["x"]), Rows(M, C, gpu, d["du"], pad=8)
    w = d["w"].to(gpu)

    def run():
        dx = Rows(M, C, gpu, pad=12)
        vec = torch.full((C * k * k + C + 64,), SENTINEL, device=gpu)
        ops.dwconv_bwd(x.rows, du.rows, w, dx.rows, vec[:C * k * k], vec[C * k * k:C * k * k + C], B, H, W, k)
        return dx, vec

    dx, vec = run()
    torch.cuda.synchronize()
    dx.check_untouched("dx")
    assert bool((vec[C * k * k + C:] == SENTINEL).all())
    e = (rel(dx.rows, d["dx_ref"]), rel(vec[:C * k * k].view(C, k * k), d["dw_ref"]), rel(vec[C * k * k:C * k * k + C], d["db_ref"]))
    print("dwconv_bwd %s k %d: relL2 dx %.2e dweight %.2e dbias %.2e" % ((B, H, W, C), k, *e))
    assert max(e) <= OP_TOL
    dx2, vec2 = run()
    assert torch.equal(dx2.flat, dx.flat) and torch.equal(vec2, vec)


# ---------------------------------------------------------------------------------------------------------------------
# (d) pfk_gelu_f32 / pfk_gelu_bwd_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(2 * 13 * 17, 512), (3, 4), (37, 36)])
def test_gelu_rows(gpu, M, C):
    ops = torch.ops.pfk
    g = torch.Generator().manual_seed(M + C)
    x, dy = torch.randn(M, C, generator=g) * 2.5, torch.randn(M, C, generator=g)
    special = torch.tensor([30.0, -30.0, 1e30, -1e30])            # large |x|: y = x or 0, dx = dy or 0, never NaN
    x[0, :4] = special
    xr, dyr = Rows(M, C, gpu, x), Rows(M, C, gpu, dy, pad=8)

    def run():
        y, dx = Rows(M, C, gpu), Rows(M, C, gpu, pad=12)
        ops.gelu(xr.rows, y.rows)
        ops.gelu_bwd(xr.rows, dyr.rows, dx.rows)
        return y, dx

    y, dx = run()
    torch.cuda.synchronize()
    y.check_untouched("y"), dx.check_untouched("dx")
    assert torch.equal(y.rows[0, :4].cpu(), special * torch.tensor([1.0, 0.0, 1.0, 0.0]))
    assert torch.equal(dx.rows[0, :4].cpu(), dy[0, :4] * torch.tensor([1.0, 0.0, 1.0, 0.0]))
    keep = torch.ones(M, C, dtype=torch.bool)
    keep[0, :4] = False
    x64, dy64 = x.double(), dy.double()
    e = (rel(y.rows.cpu()[keep], F.gelu(x64)[keep]), rel(dx.rows.cpu()[keep], gelu_bwd_ref(x64, dy64)[keep]))
    print("gelu rows %dx%d: relL2 y %.2e dx %.2e" % (M, C, *e))
    assert max(e) <= OP_TOL
    y2, dx2 = run()
    assert torch.equal(y2.flat, y.flat) and torch.equal(dx2.flat, dx.flat)


# ---------------------------------------------------------------------------------------------------------------------
# the two nodes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,k", [(2, 13, 17, 384, 7), (1, 8, 16, 36, 5), (2, 1, 5, 384, 7)])
def test_dwconv_layernorm_node(gpu, B, H, W, C, k):
    from ptlflow_amd.train_sea import dwconv_layernorm_pm
    d = case(B, H, W, C, 7)
    g = torch.Generator().manual_seed(k)
    w = torch.randn(C, 1, k, k, generator=g) / k
    names = ("x", "w", "b", "gamma", "beta")
    vals = [d["x"], w, d["b"], d["gamma"], d["beta"]]
    ref = [v.double().requires_grad_(True) for v in vals]
    u = F.conv2d(ref[0].view(B, H, W, C).permute(0, 3, 1, 2), ref[1], ref[2], padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    out_ref = F.layer_norm(u, (C,), ref[3], ref[4], 1e-6)
    want = torch.autograd.grad((out_ref * d["dy"].double()).sum(), ref)
    got_in = [v.to(gpu).requires_grad_(True) for v in vals]
    out = dwconv_layernorm_pm(*got_in, B, H, W)
    got = torch.autograd.grad((out * d["dy"].to(gpu)).sum(), got_in)
    errs = {"out": rel(out, out_ref), **{"d" + n: rel(a, b) for n, a, b in zip(names, got, want)}}
    print("dwconv_layernorm_pm %s k %d: " % ((B, H, W, C), k) + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert got[1].shape == w.shape and max(errs.values()) <= OP_TOL


def test_gelu_node(gpu):
    from ptlflow_amd.train_sea import gelu_pm
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(221, 512, generator=g) * 2, torch.randn(221, 512, generator=g)
    r = x.double().requires_grad_(True)
    (want,) = torch.autograd.grad((F.gelu(r) * dy.double()).sum(), r)
    xg = x.to(gpu).requires_grad_(True)
    y = gelu_pm(xg)
    (got,) = torch.autograd.grad((y * dy.to(gpu)).sum(), xg)
    assert rel(y, F.gelu(x.double())) <= OP_TOL and rel(got, want) <= OP_TOL


# ---------------------------------------------------------------------------------------------------------------------
# blocks against the stand-in in float64
# ---------------------------------------------------------------------------------------------------------------------
BB, BH, BW = 2, 13, 17


@functools.lru_cache(maxsize=None)
def block_reference():
    """the stand-in's update block and heads in float64 on the CPU at (2, 13, 17): inputs, outputs, every gradient"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    model = load_seeded(SeaRaftLoop(), 31).double()
    g = torch.Generator().manual_seed(32)
    x = {"net": torch.tanh(torch.randn(BB, 128, BH, BW, generator=g)), "inp": torch.relu(torch.randn(BB, 128, BH, BW, generator=g)),
         "corr": torch.randn(BB, 324, BH, BW, generator=g), "flow": torch.randn(BB, 2, BH, BW, generator=g) * 2}
    R = [torch.randn(BB, c, BH, BW, generator=g) for c in (128, 6, 576)]
    xin = {k: v.double().requires_grad_(True) for k, v in x.items()}
    named = {f"{part}.{n}": p for part in ("update_block", "flow_head", "upsample_weight") for n, p in getattr(model, part).named_parameters()}
    h = model.update_block(*xin.values())
    fh, uw = model.flow_head(h), model.upsample_weight(h)
    loss = (h * R[0].double()).sum() + (fh * R[1].double()).sum() + (0.25 * uw * R[2].double()).sum()
    grads = torch.autograd.grad(loss, list(xin.values()) + list(named.values()))
    params = {k: v.detach().float() for k, v in named.items()}
    return {"x": x, "R": R, "params": params, "out": (h.detach(), fh.detach(), uw.detach()),
            "gin": dict(zip(xin, grads[:4])), "gpar": dict(zip(named, grads[4:]))}


def _block_run(gpu, ref, cache, accumulate, calls=1):
    """`calls` recurrent uses of update block + heads on the same inputs (the loss is the sum over the calls)"""
    from ptlflow_amd.sea_update import sea_spec
    from ptlflow_amd.train_sea import sea_heads_train_pm, sea_update_block_train_pm
    P = {k: v.to(gpu).requires_grad_(True) for k, v in ref["params"].items()}
    Pu = {k[len("update_block."):]: v for k, v in P.items() if k.startswith("update_block.")}
    Ph = {k: v for k, v in P.items() if not k.startswith("update_block.")}
    xin = {k: pm(v, gpu).requires_grad_(True) for k, v in ref["x"].items()}
    R = [pm(r, gpu) for r in ref["R"]]
    loss, outs = 0.0, None
    for _ in range(calls):
        h = sea_update_block_train_pm(Pu, sea_spec(324), xin["net"], xin["inp"], xin["corr"], xin["flow"], BB, BH, BW, 2, cache, accumulate)
        fh, uw = sea_heads_train_pm(Ph, h, BB, BH, BW, cache, accumulate)
        loss = loss + (h * R[0]).sum() + (fh * R[1]).sum() + (0.25 * uw * R[2]).sum()
        outs = (h, fh, uw)
    grads = torch.autograd.grad(loss, list(xin.values()) + list(P.values()))
    return outs, dict(zip(xin, grads[:4])), dict(zip(P, grads[4:]))


def test_update_block_and_heads(gpu):
    ref = block_reference()
    outs, gin, gpar = _block_run(gpu, ref, {}, False)
    for name, a, b in zip(("net", "flow_head", "upsample_weight"), outs, ref["out"]):
        scale_close(nchw(a, BB, BH, BW), b, name)
    for k in gin:
        scale_close(nchw(gin[k], BB, BH, BW), ref["gin"][k], "d/d" + k)
    for k in gpar:
        scale_close(gpar[k], ref["gpar"][k], k)


def test_recurrent_calls_accumulate(gpu):
    """two recurrent calls with a step cache and `accumulate_wgrad=True` against the sum of the two calls' gradients"""
    ref = block_reference()
    _, gin1, gpar1 = _block_run(gpu, ref, None, False)
    _, gin2, gpar2 = _block_run(gpu, ref, {}, True, calls=2)
    for k in gin1:
        scale_close(gin2[k], 2 * gin1[k], "d/d" + k, 1e-5)
    for k in gpar1:
        scale_close(gpar2[k], 2 * gpar1[k], k, 1e-5)
        scale_close(gpar2[k], 2 * ref["gpar"][k], k + " (float64)")


def test_convnext_block(gpu):
    from sea_seam_model import ConvNextBlock, seeded_params
    from ptlflow_amd.train_sea import convnext_block_train_pm
    blk = ConvNextBlock(384, 128)
    blk.load_state_dict(seeded_params({k: tuple(v.shape) for k, v in blk.state_dict().items()}, 5))
    g = torch.Generator().manual_seed(6)
    x, R = torch.randn(BB, 384, BH, BW, generator=g), torch.randn(BB, 128, BH, BW, generator=g)
    P32 = {k: v.detach().clone() for k, v in blk.named_parameters()}
    blk = blk.double()
    xr = x.double().requires_grad_(True)
    out_ref = blk(xr)
    want = torch.autograd.grad((out_ref * R.double()).sum(), [xr] + list(blk.parameters()))
    P = {"b." + k: v.to(gpu).requires_grad_(True) for k, v in P32.items()}
    xg = pm(x, gpu).requires_grad_(True)
    out = convnext_block_train_pm(P, "b.", xg, BB, BH, BW)
    got = torch.autograd.grad((out * pm(R, gpu)).sum(), [xg] + list(P.values()))
    scale_close(nchw(out, BB, BH, BW), out_ref, "out")
    scale_close(nchw(got[0], BB, BH, BW), want[0], "d/dx")
    for name, a, b in zip(P32, got[1:], want[1:]):
        scale_close(a, b, name)
    # a block without gamma behaves as gamma = 1
    P1 = {k: (torch.ones_like(v) if k.endswith("gamma") else v.detach()) for k, v in P.items()}
    P0 = {k: v for k, v in P1.items() if not k.endswith("gamma")}
    with torch.no_grad():
        assert torch.equal(convnext_block_train_pm(P0, "b.", xg, BB, BH, BW), convnext_block_train_pm(P1, "b.", xg, BB, BH, BW))


# ---------------------------------------------------------------------------------------------------------------------
# the seam
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_replay_through_the_seam(gpu):
    """the reference's own backward (scripts/make_sea_raft_train_golden.py) against accelerate(..., sea_raft_train=True)"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    from ptlflow_amd import patch
    gd = torch.load(GOLDEN)
    model = load_seeded(SeaRaftLoop(), 2024).to(gpu).train()
    patch.accelerate(model, sea_raft_update=True, sea_raft_train=True)
    try:
        x = {k: gd[k].to(gpu).requires_grad_(True) for k in ("net", "inp", "corr", "flow")}
        net_out = model.update_block(x["net"], x["inp"], x["corr"], x["flow"])
        fh, uw = model.flow_head(net_out), model.upsample_weight(net_out)
        assert net_out.shape == (1, 128, 7, 8) and fh.shape == (1, 6, 7, 8) and uw.shape == (1, 576, 7, 8) and net_out.dtype == torch.float32
        loss = (net_out * gd["R_n"].to(gpu)).sum() + (fh * gd["R_f"].to(gpu)).sum() + (0.25 * uw * gd["R_w"].to(gpu)).sum()
        loss.backward()
        assert (model.update_block.train_calls, model.flow_head.train_calls, model.upsample_weight.train_calls) == (1, 1, 1)
        assert model.update_block.calls == 0 and model.flow_head.calls == 0 and model.upsample_weight.calls == 0
        for k, v in x.items():
            scale_close(v.grad, gd["grad." + k], "d/d" + k)
        named = dict(model.named_parameters())
        for k in sorted(gd):
            if k.startswith("full."):
                scale_close(named[k[5:]].grad, gd[k], k)
            elif k.startswith("norm."):
                assert named[k[5:]].grad is not None and abs(float(named[k[5:]].grad.double().norm()) - float(gd[k])) <= BLOCK_TOL * float(gd[k]), k
    finally:
        patch.restore(model)


def test_training_loop_through_the_seam(gpu):
    """SeaRaftLoop(iters=2).train() at B = 1, 16 x 24 with a fixed linear loss over flows, info and flow_small: every parameter's
    gradient and the feature maps' against the stand-in's CPU float64 run"""
    from sea_seam_model import SeaRaftLoop, load_seeded
    from ptlflow_amd import patch
    from ptlflow_amd.sea_update import PfkSeaRaftUpdateBlock, _SeaHeadSeam
    g = torch.Generator().manual_seed(5)
    B, H, W = 1, 16, 24
    x = [torch.tanh(torch.randn(B, 128, H, W, generator=g)), torch.relu(torch.randn(B, 128, H, W, generator=g)),
         torch.randn(B, 256, H, W, generator=g) * 0.3, torch.randn(B, 256, H, W, generator=g) * 0.3]
    R = {"flows": torch.randn(B, 1, 2, 8 * H, 8 * W, generator=g), "info": torch.randn(B, 4, 8 * H, 8 * W, generator=g),
         "flow_small": torch.randn(B, 2, H, W, generator=g)}

    def run(model, xs, to):
        out = model(*xs)
        sum(((out[k] * to(R[k])).sum() for k in R)).backward()

    ref = load_seeded(SeaRaftLoop(iters=2), 2).double().train()
    xr = [t.double() for t in x]
    xr[2].requires_grad_(True), xr[3].requires_grad_(True)
    run(ref, xr, lambda t: t.double())

    model = load_seeded(SeaRaftLoop(iters=2), 2).to(gpu).train()
    patch.accelerate(model, sea_raft_update=True, sea_raft_train=True)
    try:
        ub, fh, uw = model.update_block, model.flow_head, model.upsample_weight
        assert isinstance(ub, PfkSeaRaftUpdateBlock) and isinstance(fh, _SeaHeadSeam)
        xg = [t.to(gpu) for t in x]
        xg[2].requires_grad_(True), xg[3].requires_grad_(True)
        run(model, xg, lambda t: t.to(gpu))
        assert (ub.train_calls, fh.train_calls, uw.train_calls) == (2, 3, 3)
        assert (ub.calls, fh.calls, uw.calls) == (0, 0, 0)
        want = dict(ref.named_parameters())
        got = dict(model.named_parameters())
        assert sorted(got) == sorted(want)
        for name, p in got.items():
            assert p.grad is not None, name
            scale_close(p.grad, want[name].grad, name)
        scale_close(xg[2].grad, xr[2].grad, "d/dfmap1")
        scale_close(xg[3].grad, xr[3].grad, "d/dfmap2")
    finally:
        patch.restore(model)
    assert not isinstance(model.update_block, PfkSeaRaftUpdateBlock) and not isinstance(model.flow_head, _SeaHeadSeam)
    assert not hasattr(model.update_block, "train_calls") and not hasattr(model.flow_head, "train_calls")
    assert not hasattr(model.upsample_weight, "train_calls")
