"""`RAFT(train_precision="bf16")`: one end-to-end training step of the mirror with the update block on the bf16 matrix cores
(K12b) against float64 autograd through the CPU oracle's training forward — and the drop-in seam, `accelerate(model,
train_precision="bf16")`.

Yardstick: the same oracle in fp32 with ``torch.autocast("cpu", bfloat16)`` entered around `O.basic_update_block` ONLY (encoders,
volume, lookup and upsampling stay fp32 there as they do here) — the reference's own 16-bit arithmetic.  The loss and every
parameter's gradient must be within 2x of that run's gap to float64 (L2-relative per tensor, denominators floored as
`compare_gradients` does)."""
import pytest
import torch

from oracle import raft_oracle as O

pytestmark = pytest.mark.gpu
FACTOR = 2.0


def test_train_step_raft_bf16(gpu, monkeypatch):
    from ptlflow_amd.raft import RAFT
    from ptlflow_amd.train import sequence_loss
    B, H, W, iters = 1, 184, 248, 3
    model = RAFT(iters=iters, train_precision="bf16").load_synthetic(21)
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
        preds = O.raft_forward_train(P, x.to(dtype), iters=iters)
        loss = O.sequence_loss(preds, gt.to(dtype), valid.to(dtype))
        keys = sorted(leaves)
        return loss, dict(zip(keys, torch.autograd.grad(loss, [leaves[k] for k in keys], allow_unused=True)))

    loss64, g64 = oracle_grads(torch.float64)
    block = O.basic_update_block

    def block_autocast(*a, **k):
        with torch.autocast("cpu", torch.bfloat16):
            net, mask, delta = block(*a, **k)
        return net.float(), mask.float(), delta.float()

    monkeypatch.setattr(O, "basic_update_block", block_autocast)
    loss16, g16 = oracle_grads(torch.float32)
    monkeypatch.setattr(O, "basic_update_block", block)

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
        assert ref is not None and c is not None and p.grad is not None, f"{n}: no gradient"
        assert p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        ref, c, gp = ref.double(), c.double(), p.grad.double().cpu()
        den = max(float(ref.norm()), 1e-3 * scale_all * ref.numel() ** 0.5)
        rows.append((float((gp - ref).norm()) / den / max(float((c - ref).norm()) / den, 1e-30), n, float((gp - ref).norm()) / den,
                     float((c - ref).norm()) / den))
        compared += 1
    assert compared == len(names) and compared > 100, compared
    rows.sort(reverse=True)
    for r in rows[:12]:
        print("   ratio %.2f  %-44s  L2 err %.3e  (CPU autocast %.3e)" % r)
    assert e_gpu <= FACTOR * e_cpu, f"loss error {e_gpu:.3e} vs CPU autocast {e_cpu:.3e}"
    bad = [r for r in rows if r[2] > FACTOR * r[3]]
    assert not bad, "worse than 2x CPU autocast: " + ", ".join("%s %.2e vs %.2e" % (r[1], r[2], r[3]) for r in bad[:8])


def test_seam_train_precision(gpu):
    """`accelerate(model, train_precision="bf16")` on the torch-only caller (tests/seam_model.py): a call of the wrapped update
    block that carries a gradient graph runs the bf16 composition and every parameter of the block gets a finite gradient;
    a second `accelerate` call switches back, and the fp32 path is then bit-identical to a model that never left it."""
    from seam_model import SeamRAFT
    from ptlflow_amd import patch
    from ptlflow_amd.update import PfkUpdateBlock
    a, b = SeamRAFT(iters=2).to(gpu).train(), SeamRAFT(iters=2).to(gpu).train()
    b.load_state_dict(a.state_dict())
    patch.accelerate(a)
    patch.accelerate(b, train_precision="bf16")
    assert isinstance(b.update_block, PfkUpdateBlock) and b.update_block.train_precision == "bf16"
    assert a.update_block.train_precision == "fp32"
    g = torch.Generator().manual_seed(3)
    B, H, W = 1, 10, 14
    net = torch.tanh(torch.randn(B, 128, H, W, generator=g)).to(gpu)
    inp = torch.relu(torch.randn(B, 128, H, W, generator=g)).to(gpu)
    corr = torch.randn(B, 324, H, W, generator=g).to(gpu)
    flow = (torch.randn(B, 2, H, W, generator=g) * 2).to(gpu)

    def step(m):
        m.zero_grad(set_to_none=True)
        n = net.clone().requires_grad_()
        h, mask, delta = m.update_block(n, inp, corr, flow)
        (h.square().mean() + mask.square().mean() + delta.square().mean()).backward()
        grads = {k: p.grad.clone() for k, p in m.update_block.named_parameters()}
        return (h.detach().clone(), mask.detach().clone(), delta.detach().clone(), n.grad.clone()), grads

    outs_b16, grads_b16 = step(b)
    for k, gr in grads_b16.items():
        assert gr.dtype == torch.float32 and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, k
    assert len(grads_b16) == len(list(b.update_block.parameters())) and all(bool(torch.isfinite(t).all()) for t in outs_b16)
    outs_a, grads_a = step(a)
    assert not torch.equal(outs_b16[0], outs_a[0]), "the bf16 path computed fp32's bits: it did not run"
    # bf16 operands: close to the fp32 path, not equal to it
    assert float((outs_b16[0] - outs_a[0]).abs().max()) < 0.05 * float(outs_a[0].abs().max())
    patch.accelerate(b, train_precision="fp32")            # switch back
    assert b.update_block.train_precision == "fp32"
    outs_b, grads_b = step(b)
    assert all(torch.equal(u, v) for u, v in zip(outs_a, outs_b))
    assert all(torch.equal(grads_a[k], grads_b[k]) for k in grads_a)
    with pytest.raises(ValueError):
        patch.accelerate(b, train_precision="fp16")
