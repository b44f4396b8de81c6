"""Training GMA on the kernels (K12c): the softmax backward and the transposed pack, the autograd nodes of the attention map and
of its per-iteration use (`_AttentionMap`, `_AttnMatmul`, the step sink `_AttnFlush`) in fp32 and bf16, one whole training step of
the mirror in either precision, and the drop-in seam (`PfkUpdateBlock` with GMA's five-argument forward).

Gates.  fp32 ops: relative L2 <= 5e-6 against float64 arithmetic ON THE NODE'S OWN INPUTS (the op-level gate of
tests/test_gpu_train_step.py).  bf16: the rule of tests/test_gpu_train_step_bf16.py — the error against float64 must be within 2x the
error of the oracle's same computation under ``torch.autocast("cpu", bfloat16)``, per tensor, L2.  Block-level fp32 comparison of the
seam: 5e-4 of each tensor's scale (tests/test_gpu_train.py::test_update_block_training_step)."""
import functools

import pytest
import torch

from oracle import raft_oracle as O
from op_gate import OP_TOL, SENTINEL, bits, rel, round_up

pytestmark = pytest.mark.gpu
FACTOR = 2.0
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# 1. pfk_softmax_rows_bwd_{f32,bf16}
# ---------------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [(2 * 140, 140, 140), (2 * 140, 140, 144), (64, 396, 396), (8, 713, 716), (4, 1, 4)]


def _softmax_inputs(rows, cols, ld, gpu):
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    p = torch.full((rows, ld), float("nan"))              # pad columns of the inputs must not be read
    p[:, :cols] = torch.softmax(torch.randn(rows, cols, generator=g) * 3, dim=-1)
    dp = torch.full((rows, ld), float("nan"))
    dp[:, :cols] = torch.randn(rows, cols, generator=g)
    return p.to(gpu), dp.to(gpu)


def _softmax_ref(p, dp, cols):
    p64, d64 = p[:, :cols].double().cpu(), dp[:, :cols].double().cpu()
    return p64 * (d64 - (d64 * p64).sum(-1, keepdim=True))


def _check_softmax_out(flat, rows, cols, ld, ref):
    out = flat[:rows * ld].view(rows, ld)
    assert bool((flat[rows * ld:] == SENTINEL).all()), "memory past the last row was written"
    assert bool((out[:, cols:] == 0).all()), "pad columns of the output must be zero"
    if cols == 1:
        assert bool((out[:, :1] == 0).all()), "one column: the gradient is exactly zero"
        return 0.0
    return rel(out[:, :cols], ref)


@pytest.mark.parametrize("rows,cols,ld", SOFTMAX_CASES)
def test_softmax_rows_bwd(gpu, rows, cols, ld):
    ops = torch.ops.pfk
    p, dp = _softmax_inputs(rows, cols, ld, gpu)
    ref = _softmax_ref(p, dp, cols)
    # fp32, out of place
    flat = torch.full((rows * ld + 64,), SENTINEL, device=gpu)
    ops.softmax_rows_bwd(p[:, :cols], dp[:, :cols], flat[:rows * ld].view(rows, ld))
    e_out = _check_softmax_out(flat, rows, cols, ld, ref)
    # fp32, in place: dS over dP
    flat2 = torch.full((rows * ld + 64,), SENTINEL, device=gpu)
    buf = flat2[:rows * ld].view(rows, ld)
    buf.copy_(dp)
    ops.softmax_rows_bwd(p[:, :cols], buf[:, :cols], buf)
    e_in = _check_softmax_out(flat2, rows, cols, ld, ref)
    assert torch.equal(flat[:rows * ld], flat2[:rows * ld]), "in place and out of place differ"
    # bf16 dP with its own row stride; the reference is float64 on the bf16 values
    ldb = round_up(cols, 8)
    dpb = torch.full((rows, ldb), float("nan"), device=gpu, dtype=BF16)
    dpb[:, :cols] = dp[:, :cols].to(BF16)
    flat3 = torch.full((rows * ld + 64,), SENTINEL, device=gpu)
    ops.softmax_rows_bwd(p[:, :cols], dpb[:, :cols], flat3[:rows * ld].view(rows, ld))
    e_b16 = _check_softmax_out(flat3, rows, cols, ld, _softmax_ref(p, dpb.float(), cols))
    print("softmax_rows_bwd %dx%d ld %d: relL2 out of place %.2e, in place %.2e, bf16 dP %.2e" % (rows, cols, ld, e_out, e_in, e_b16))
    assert max(e_out, e_in, e_b16) <= OP_TOL
    # deterministic: the same bits on a second run
    again = torch.empty(rows, ld, device=gpu)
    ops.softmax_rows_bwd(p[:, :cols], dp[:, :cols], again)
    assert torch.equal(again.flatten(), flat[:rows * ld])


# ---------------------------------------------------------------------------------------------------------------------
# 2. pfk_transpose_pack_{f32,b16}
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,ld_in,extra", [(2, 128, 128, 0), (2, 140, 145, 0), (2, 140, 140, 64), (2, 396, 396, 0), (1, 713, 713, 0)])
def test_transpose_pack(gpu, B, N, ld_in, extra):
    ops = torch.ops.pfk
    g = torch.Generator().manual_seed(N)
    buf = torch.randn(B, N, ld_in, generator=g)
    x = buf[:, :, :N]
    # signed zero, a denormal, and exact ties of the bf16 rounding (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6, and negated)
    special = torch.tensor([-0.0, 0.0, 1e-40, -1e-40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8),
                            3.3895314e38, 2.0 ** -126])
    x[:, 0, :special.numel()] = special
    x[:, N - 1, N - special.numel():] = special
    x[:, 5:5 + special.numel(), N - 1] = special[None]
    xt = x.transpose(1, 2).contiguous()
    xg = buf.to(gpu)[:, :, :N]
    for dtype, align in ((torch.float32, 4), (BF16, 8)):
        ld = round_up(N, align) + extra
        n = B * N * ld
        want_t, want = xt.to(dtype), x.contiguous().to(dtype)
        for with_out in (True, False):
            flat_t = torch.full((n + 64,), SENTINEL, device=gpu, dtype=dtype)
            flat_o = torch.full((n + 64,), SENTINEL, device=gpu, dtype=dtype)
            outT, out = flat_t[:n].view(B, N, ld), flat_o[:n].view(B, N, ld)
            ops.transpose_pack(xg, outT, out if with_out else None)
            assert torch.equal(bits(outT[:, :, :N].cpu().contiguous()), bits(want_t)), (dtype, "outT")
            assert bool((outT[:, :, N:] == 0).all()), "pad columns of outT must be zero"
            assert bool((flat_t[n:] == SENTINEL).all())
            if with_out:
                assert torch.equal(bits(out[:, :, :N].cpu().contiguous()), bits(want)), (dtype, "out")
                assert bool((out[:, :, N:] == 0).all()), "pad columns of out must be zero"
            else:
                assert bool((flat_o == SENTINEL).all()), "out was written although none was given"
            assert bool((flat_o[n:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3 / 4. _AttnMatmul (and the step sink), fp32 and bf16
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = [(10, 14), (8, 16), (18, 22)]        # N = 140 (no multiple of 8), 128 (exact), 396 (two 256-row tiles)
T_USES = 3


@functools.lru_cache(maxsize=None)
def _matmul_case(H, W):
    """Inputs and the float64 / CPU-autocast results, computed once per shape and shared by the fp32 and bf16 tests."""
    B, C, N = 2, 128, H * W
    g = torch.Generator().manual_seed(H * 100 + W)
    P = torch.softmax(torch.randn(B, 1, N, N, generator=g) * 2, dim=-1)
    vs = [torch.randn(B * N, C, generator=g) for _ in range(T_USES)]
    gos = [torch.randn(B * N, C, generator=g) for _ in range(T_USES)]

    def run(dtype, autocast):
        p = P.clone().to(dtype).requires_grad_(True)
        res = {"out": [], "dP": [], "dV": []}
        for t in range(T_USES):
            v = vs[t].clone().to(dtype).requires_grad_(True)
            with torch.autocast("cpu", BF16, enabled=autocast):      # a 16-bit matmul: bf16 operands, bf16 result, bf16 gradients
                o = torch.matmul(p[:, 0], v.view(B, N, C))
            o = o.to(dtype).reshape(B * N, C)
            dp, dv = torch.autograd.grad((o * gos[t].to(dtype)).sum(), [p, v])
            res["out"].append(o.detach()), res["dP"].append(dp), res["dV"].append(dv)
        return res

    return {"B": B, "C": C, "N": N, "P": P, "v": vs, "go": gos, "f64": run(torch.float64, False), "ac": run(torch.float32, True)}


def _run_matmul(gpu, case, H, W, precision, sink, uses=(0, 1, 2), in_loss=(0, 1, 2)):
    """The node on the GPU: forward of `uses`, loss over `in_loss`; returns (outs, dP, dVs)."""
    from ptlflow_amd.train import _AttnMatmul, pack_attention
    B = case["B"]
    p = case["P"].to(gpu).requires_grad_(True)
    v = {t: case["v"][t].to(gpu).requires_grad_(True) for t in uses}
    st = pack_attention(p, B, H, W, precision, sink=sink)
    outs = {t: _AttnMatmul.apply(st.target(p), v[t], st) for t in uses}
    for o in outs.values():
        assert o.dtype == torch.float32 and bool(torch.isfinite(o).all())
    sum((outs[t] * case["go"][t].to(gpu)).sum() for t in in_loss).backward()
    assert p.grad is not None and p.grad.dtype == torch.float32 and tuple(p.grad.shape) == tuple(p.shape)
    return outs, p.grad, {t: v[t].grad for t in uses}


@pytest.mark.parametrize("H,W", GRIDS)
def test_attn_matmul_fp32(gpu, H, W):
    case = _matmul_case(H, W)
    ref = case["f64"]
    outs, dP, dV = _run_matmul(gpu, case, H, W, "fp32", sink=False, uses=(0,), in_loss=(0,))
    errs = {"out": rel(outs[0], ref["out"][0]), "dV": rel(dV[0], ref["dV"][0]), "dP": rel(dP, ref["dP"][0])}
    # the step sink: T uses, the N x N gradient written once
    outs, dP, dV = _run_matmul(gpu, case, H, W, "fp32", sink=True)
    errs["sink dP"] = rel(dP, sum(ref["dP"]))
    errs["sink dV"] = max(rel(dV[t], ref["dV"][t]) for t in range(T_USES))
    errs["sink out"] = max(rel(outs[t], ref["out"][t]) for t in range(T_USES))
    # the middle use does not reach the loss: its slot stays zero
    _, dP, dV = _run_matmul(gpu, case, H, W, "fp32", sink=True, in_loss=(0, 2))
    errs["sink dP without the middle use"] = rel(dP, ref["dP"][0] + ref["dP"][2])
    assert dV[1] is None
    print("_AttnMatmul fp32 %dx%d: " % (H, W) + ", ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) <= OP_TOL, errs


def _within_autocast(rows):
    """rows: (name, got, float64 reference, CPU autocast result) -> assert ||got - ref|| <= 2 ||autocast - ref|| per tensor."""
    bad = []
    for name, got, ref, ac in rows:
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), name
        ref = ref.double()
        e_gpu, e_cpu = float((got.double().cpu() - ref).norm()), float((ac.double() - ref).norm())
        den = max(float(ref.norm()), 1e-300)
        print("   %-40s L2 err %.3e  (CPU autocast %.3e)  ratio %.2f" % (name, e_gpu / den, e_cpu / den, e_gpu / max(e_cpu, 1e-300)))
        if e_gpu > FACTOR * e_cpu:
            bad.append("%s %.3e vs %.3e" % (name, e_gpu / den, e_cpu / den))
    assert not bad, "worse than 2x CPU autocast: " + ", ".join(bad[:8])


@pytest.mark.parametrize("H,W", GRIDS)
def test_attn_matmul_bf16(gpu, H, W):
    case = _matmul_case(H, W)
    ref, ac = case["f64"], case["ac"]
    outs, dP, dV = _run_matmul(gpu, case, H, W, "bf16", sink=False, uses=(0,), in_loss=(0,))
    rows = [("out", outs[0].detach(), ref["out"][0], ac["out"][0]), ("dV", dV[0], ref["dV"][0], ac["dV"][0]),
            ("dP", dP, ref["dP"][0], ac["dP"][0])]
    outs, dP, dV = _run_matmul(gpu, case, H, W, "bf16", sink=True)
    rows.append(("sink dP (3 uses, one product)", dP, sum(ref["dP"]), sum(ac["dP"])))
    rows += [("sink dV %d" % t, dV[t], ref["dV"][t], ac["dV"][t]) for t in range(T_USES)]
    _, dP, dV = _run_matmul(gpu, case, H, W, "bf16", sink=True, in_loss=(0, 2))
    rows.append(("sink dP without the middle use", dP, ref["dP"][0] + ref["dP"][2], ac["dP"][0] + ac["dP"][2]))
    assert dV[1] is None
    _within_autocast(rows)


# ---------------------------------------------------------------------------------------------------------------------
# 5. _AttentionMap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(18, 22), (10, 14), (23, 31)])      # N = 396; 140 and 713: N % 32 != 0 / N % 4 != 0, padded rows
def test_attention_map(gpu, H, W):
    from ptlflow_amd.train import attention_map_train
    B, C = 2, 128
    N = H * W
    g = torch.Generator().manual_seed(11)
    inp = torch.relu(torch.randn(B, C, H, W, generator=g))
    wqk = torch.randn(2 * C, C, 1, 1, generator=g) * 0.1
    dP = torch.randn(B, 1, N, N, generator=g)
    w64, i64 = wqk.double().requires_grad_(True), inp.double().requires_grad_(True)
    ref = O.gma_attention({"att.to_qk.weight": w64}, i64, heads=1)
    gw, gi = torch.autograd.grad(ref, [w64, i64], dP.double())
    w = wqk.to(gpu).requires_grad_(True)
    ipm = inp.permute(0, 2, 3, 1).reshape(B * N, C).to(gpu).requires_grad_(True)
    P = attention_map_train(ipm, w, B, H, W, C ** -0.5)
    assert tuple(P.shape) == (B, 1, N, N) and P.dtype == torch.float32
    err = (P.detach().double().cpu() - ref.detach()).abs()
    assert bool((err <= 2e-5 * (1 + ref.detach().abs())).all()), float(err.max())
    P.backward(dP.to(gpu))
    e_w, e_i = rel(w.grad, gw), rel(ipm.grad.view(B, H, W, C).permute(0, 3, 1, 2), gi)
    print("_AttentionMap: max |P - ref| %.2e, d to_qk.weight relL2 %.2e, d inp relL2 %.2e" % (float(err.max()), e_w, e_i))
    assert max(e_w, e_i) <= OP_TOL


# ---------------------------------------------------------------------------------------------------------------------
# 6 / 7. whole training steps of the mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_train_step_gma_bf16(gpu, monkeypatch):
    """`test_train_step_raft_bf16` restated for GMA: loss and every parameter's gradient within 2x of what the float32 oracle with
    ``torch.autocast`` around `O.gma_update_block` ONLY loses against float64; `att.pos_emb.*` has no gradient on either side.

    On the parent commit this fails with `update_block_train_pm`'s ValueError for the aggregate branch."""
    from ptlflow_amd.raft import GMA
    from ptlflow_amd.train import sequence_loss
    B, H, W, iters = 1, 184, 248, 3
    model = GMA(iters=iters, train_precision="bf16").load_synthetic(21)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(9)                      # inputs as test_gpu_train_step._run
    x = torch.rand(B, 2, 3, H, W, generator=g)
    gt = torch.randn(B, 2, H, W, generator=g) * 4
    valid = (torch.rand(B, 1, H, W, generator=g) > 0.1).float()
    gt[0, :, :8, :8] = 500.0
    names = [n for n, _ in model.named_parameters()]
    alias = {n: n.replace(".norm3.", ".downsample.1.") for n in names}     # see test_gpu_train_step._run
    alias = {n: (a if a in sd else n) for n, a in alias.items()}

    def oracle_grads(dtype):
        leaves = {a: sd[a].to(dtype).requires_grad_(True) for a in set(alias.values())}
        P = {k: leaves.get(k, v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        preds = O.raft_forward_train(P, x.to(dtype), iters=iters, gma=True)
        loss = O.sequence_loss(preds, gt.to(dtype), valid.to(dtype))
        keys = sorted(leaves)
        return loss, dict(zip(keys, torch.autograd.grad(loss, [leaves[k] for k in keys], allow_unused=True)))

    loss64, g64 = oracle_grads(torch.float64)
    block = O.gma_update_block

    def block_autocast(*a, **k):
        with torch.autocast("cpu", BF16):
            net, mask, delta = block(*a, **k)
        return net.float(), mask.float(), delta.float()

    monkeypatch.setattr(O, "gma_update_block", block_autocast)
    loss16, g16 = oracle_grads(torch.float32)
    monkeypatch.setattr(O, "gma_update_block", block)

    model = model.to(gpu).train()
    out = model({"images": x.to(gpu)})
    assert len(out["flow_preds"]) == iters
    loss = sequence_loss(out["flow_preds"], gt.to(gpu), valid.to(gpu))
    loss.backward()

    e_gpu, e_cpu = abs(loss.item() - loss64.item()), abs(loss16.item() - loss64.item())
    print("loss %.6f (float64 %.6f, CPU autocast %.6f): err %.3e vs %.3e" % (loss.item(), loss64.item(), loss16.item(), e_gpu, e_cpu))
    scale_all = max(float(v.abs().max()) for v in g64.values() if v is not None)
    rows, compared = [], 0
    for n, p in model.named_parameters():
        ref, c = g64[alias[n]], g16[alias[n]]
        if n.startswith("att.pos_emb."):
            assert ref is None and c is None and p.grad is None, f"{n}: unused in content-only attention"
            continue
        assert ref is not None and c is not None and p.grad is not None, f"{n}: no gradient"
        assert p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        ref, c, gp = ref.double(), c.double(), p.grad.double().cpu()
        den = max(float(ref.norm()), 1e-3 * scale_all * ref.numel() ** 0.5)
        rows.append((float((gp - ref).norm()) / den / max(float((c - ref).norm()) / den, 1e-30), n, float((gp - ref).norm()) / den,
                     float((c - ref).norm()) / den))
        compared += 1
    assert {"att.to_qk.weight", "update_block.aggregator.to_v.weight", "update_block.aggregator.gamma"} <= {r[1] for r in rows}
    assert compared > 100, compared
    rows.sort(reverse=True)
    for r in rows[:12]:
        print("   ratio %.2f  %-44s  L2 err %.3e  (CPU autocast %.3e)" % r)
    for r in rows:
        if r[1].startswith(("att.", "update_block.aggregator.")):
            print("   ratio %.2f  %-44s  L2 err %.3e  (CPU autocast %.3e)" % r)
    assert e_gpu <= FACTOR * e_cpu, f"loss error {e_gpu:.3e} vs CPU autocast {e_cpu:.3e}"
    bad = [r for r in rows if r[2] > FACTOR * r[3]]
    assert not bad, "worse than 2x CPU autocast: " + ", ".join("%s %.2e vs %.2e" % (r[1], r[2], r[3]) for r in bad[:8])


def test_train_step_gma_fp32_no_foreign_matrix_work(gpu, monkeypatch):
    """A GMA training step of the mirror with torch's matrix products and softmax made to raise: forward and backward complete on
    the project's own kernels.  (The numeric gate of this path is tests/test_gpu_train_step.py::test_train_step_gma.)

    On the parent commit this fails in `torch.bmm` (the aggregate) — and before that in `_Attention.forward`."""
    import ptlflow_amd.raft as R
    from ptlflow_amd.train import sequence_loss

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called in a GMA training step")
        return f

    B, H, W = 1, 184, 248
    model = R.GMA(iters=2).load_synthetic(21).to(gpu).train()
    g = torch.Generator().manual_seed(9)
    x = torch.rand(B, 2, 3, H, W, generator=g).to(gpu)
    gt = (torch.randn(B, 2, H, W, generator=g) * 4).to(gpu)
    valid = torch.ones(B, 1, H, W, device=gpu)
    monkeypatch.setattr(torch, "bmm", refuse("torch.bmm"))
    monkeypatch.setattr(torch, "matmul", refuse("torch.matmul"))
    monkeypatch.setattr(torch, "softmax", refuse("torch.softmax"))
    monkeypatch.setattr(torch.Tensor, "softmax", refuse("Tensor.softmax"))
    monkeypatch.setattr(R._Attention, "forward", refuse("_Attention.forward"))
    out = model({"images": x})
    sequence_loss(out["flow_preds"], gt, valid).backward()
    monkeypatch.undo()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if n.startswith("att.pos_emb."):
            assert p.grad is None, n
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert float(model.att.to_qk.weight.grad.abs().max()) > 0 and float(model.update_block.aggregator.to_v.weight.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8 / 9. the drop-in seam: PfkUpdateBlock with GMA's forward(net, inp, corr, flow, attention)
# ---------------------------------------------------------------------------------------------------------------------
def _seam_loss(h, mask, delta):
    return h.square().mean() + mask.square().mean() + delta.square().mean()


@functools.lru_cache(maxsize=None)
def _seam_case(zero_gamma):
    """Weights (seed 19, as test_gma_update_block_dropin), inputs, float64 gradients and the CPU-autocast ones — shared."""
    from ptlflow_amd.raft import _param_tree
    from ptlflow_amd.synth import synth_state_dict, update_block_shapes
    from ptlflow_amd.update import gma_spec
    spec = gma_spec()
    holder = _param_tree(update_block_shapes(spec))
    P = synth_state_dict({k: tuple(v.shape) for k, v in holder.state_dict().items()}, seed=19)
    if zero_gamma:
        P["aggregator.gamma"] = torch.zeros_like(P["aggregator.gamma"])      # the reference's initial value (gma_utils.py:98)
    g = torch.Generator().manual_seed(5)
    B, h, w = 2, 10, 14
    net = torch.tanh(torch.randn(B, 128, h, w, generator=g))
    inp = torch.relu(torch.randn(B, 128, h, w, generator=g))
    corr = torch.randn(B, 324, h, w, generator=g)
    flow = torch.randn(B, 2, h, w, generator=g) * 2
    attn = torch.softmax(torch.randn(B, 1, h * w, h * w, generator=g), dim=-1)

    def grads(dtype, autocast):
        Pd = {k: v.clone().to(dtype).requires_grad_(True) for k, v in P.items()}
        n, a = net.clone().to(dtype).requires_grad_(True), attn.clone().to(dtype).requires_grad_(True)
        with torch.autocast("cpu", BF16, enabled=autocast):
            outs = O.gma_update_block(Pd, n, inp.to(dtype), corr.to(dtype), flow.to(dtype), a)
        _seam_loss(*(o.to(dtype) for o in outs)).backward()
        out = {k: v.grad for k, v in Pd.items()}
        out["d net"], out["d attention"] = n.grad, a.grad
        return out

    return {"spec": spec, "P": P, "inputs": (net, inp, corr, flow, attn), "f64": grads(torch.float64, False),
            "ac": grads(torch.float32, True)}


def _seam_block(case, gpu):
    from ptlflow_amd.raft import _param_tree
    from ptlflow_amd.synth import update_block_shapes
    from ptlflow_amd.update import PfkUpdateBlock
    holder = _param_tree(update_block_shapes(case["spec"]))       # a parameter holder: it has no forward of its own
    holder.load_state_dict(case["P"])
    return PfkUpdateBlock(holder, case["spec"]).to(gpu).train()


def _seam_step(ub, case, gpu):
    ub.zero_grad(set_to_none=True)
    net, inp, corr, flow, attn = (t.to(gpu) for t in case["inputs"])
    net, attn = net.requires_grad_(True), attn.requires_grad_(True)
    outs = ub(net, inp, corr, flow, attn)
    _seam_loss(*outs).backward()
    got = {k: p.grad for k, p in ub.named_parameters()}
    assert all(v is not None for v in got.values()) and len(got) == len(case["P"])
    got["d net"], got["d attention"] = net.grad, attn.grad
    return [o.detach().clone() for o in outs], {k: v.clone() for k, v in got.items()}


def test_seam_gma_fp32(gpu):
    """A GMA block with a gradient graph takes the native path (on the parent commit it falls through to the holder, which has
    no forward): every block parameter, `net` and `attention` against float64 autograd through `O.gma_update_block`, 5e-4 of each
    tensor's scale (the block-level gate of tests/test_gpu_train.py::test_update_block_training_step)."""
    case = _seam_case(False)
    _, got = _seam_step(_seam_block(case, gpu), case, gpu)
    for k, ref in case["f64"].items():
        a, b = got[k].double().cpu(), ref
        scale, err = float(b.abs().max()) + 1e-12, float((a - b).abs().max())
        assert err <= 5e-4 * scale, f"{k}: max err {err:.3e} vs scale {scale:.3e}"
    assert float(got["d attention"].abs().max()) > 0 and tuple(got["d attention"].shape) == tuple(case["inputs"][4].shape)


def test_seam_gma_bf16_and_back(gpu):
    """`train_precision="bf16"` under the 2x autocast rule; switching back to "fp32" gives the bits of a block that never left it."""
    case = _seam_case(False)
    a, b = _seam_block(case, gpu), _seam_block(case, gpu)
    b.train_precision = "bf16"
    outs16, got16 = _seam_step(b, case, gpu)
    _within_autocast([(k, got16[k], case["f64"][k], case["ac"][k]) for k in case["f64"]])
    outs_a, got_a = _seam_step(a, case, gpu)
    assert not torch.equal(outs16[0], outs_a[0]), "the bf16 path computed fp32's bits: it did not run"
    b.train_precision = "fp32"
    outs_b, got_b = _seam_step(b, case, gpu)
    assert all(torch.equal(u, v) for u, v in zip(outs_a, outs_b))
    assert all(torch.equal(got_a[k], got_b[k]) for k in got_a)


def test_seam_gma_native_backward_off_uses_the_wrapped_module(gpu):
    from ptlflow_amd.raft import _param_tree
    from ptlflow_amd.synth import update_block_shapes
    from ptlflow_amd.update import PfkUpdateBlock
    case = _seam_case(False)

    class TorchBlock(torch.nn.Module):          # GMAUpdateBlock on torch ops, the holder's parameters under the same names
        def __init__(self, holder):
            super().__init__()
            for name, child in holder.named_children():
                self.add_module(name, child)
            self.calls = 0

        def forward(self, net, inp, corr, flow, attention):
            self.calls += 1
            return O.gma_update_block(dict(self.named_parameters()), net, inp, corr, flow, attention)

    holder = _param_tree(update_block_shapes(case["spec"]))
    holder.load_state_dict(case["P"])
    ref = TorchBlock(holder)
    ub = PfkUpdateBlock(ref, case["spec"]).to(gpu).train()
    ub.native_backward = False
    _, got = _seam_step(ub, case, gpu)
    assert ref.calls == 1
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    ub.native_backward = True
    _seam_step(ub, case, gpu)
    assert ref.calls == 1, "the native path must not call the wrapped module"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_seam_gma_gamma_zero(gpu, precision):
    """gamma == 0, the reference's initial value: the step runs, gamma's own gradient is right, and nothing flows into `to_v` or
    the attention map (their gradients are exactly zero)."""
    case = _seam_case(True)
    ub = _seam_block(case, gpu)
    ub.train_precision = precision
    _, got = _seam_step(ub, case, gpu)
    k = "aggregator.gamma"
    assert float(case["f64"][k].abs().max()) > 0
    if precision == "fp32":
        err, scale = float((got[k].double().cpu() - case["f64"][k]).abs().max()), float(case["f64"][k].abs().max())
        assert err <= 5e-4 * scale, (err, scale)
    else:
        _within_autocast([(k, got[k], case["f64"][k], case["ac"][k])])
    assert float(got["aggregator.to_v.weight"].abs().max()) == 0.0
    assert float(got["d attention"].abs().max()) == 0.0
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
