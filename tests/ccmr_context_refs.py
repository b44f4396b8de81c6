"""TEST INFRASTRUCTURE of the CCMR context-grouping tests (K17: tests/test_ccmr_context_cpu.py, tests/test_gpu_ccmr_context.py): the
loader of tests/golden/ccmr_context.pt, the stand-in module with the fixture's parameters, the float64 pieces of the one-input block
(token rows, attention map) and the multi-scale loop stand-in with `XCiT(separate=False)` context modules.  The instruments are
tests/op_gate.py's, the block formulas tests/xcit_refs.py's."""
import contextlib
import os

import torch

import xcit_model
from xcit_model import XCiT, randomize
from xcit_refs import C, layernorm_ref, xca_map_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ccmr_context.pt")


def load_golden():
    """the fixture with its bfloat16-stored tensors (exact fp32 values on the bfloat16 grid) back in float32"""
    g = torch.load(GOLDEN, map_location="cpu")
    g["state_dict"] = {k: v.float() for k, v in g["state_dict"].items()}
    g["inp"] = g["inp"].float()
    return g


def standin(golden, dtype=torch.float32):
    m = XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1, separate=False).to(dtype).eval()
    m.load_state_dict({k: v.to(dtype) for k, v in golden["state_dict"].items()})
    return m


def rows_of(x):
    """NCHW -> [B, H*W, C] token rows, as the module flattens them"""
    return x.flatten(2).transpose(1, 2)


def token_rows64(model64, inp):
    """x0 [B, N, C] float64 of the float64 stand-in `model64`: rows(inp) + its positional encoding (if it uses one)"""
    B, _, H, W = inp.shape
    x0 = rows_of(inp.double())
    if model64.use_pos:
        x0 = x0 + model64.pos_embeder(B, H, W, torch.float64).reshape(B, -1, H * W).permute(0, 2, 1)
    return x0


def attention_map64(model64, x0):
    """A [B, 8, 16, 16] float64 of the one-input block on the token rows x0: q | k = the first 256 columns of qkv(norm1(x0))"""
    blk = model64.blocks[0]
    qkv = blk.attn.qkv(blk.norm1(x0))
    return xca_map_ref(qkv[:, :, :2 * C], blk.attn.temperature.reshape(-1))


def plain_layernorm64(x0):
    return layernorm_ref(x0)


def register() -> None:
    """the stand-in's own (module, class) key as a context module (K17), as INTEGRATION.md documents for further families"""
    from ptlflow_amd.xcit import register_xcit_context
    register_xcit_context(XCiT.__module__, "XCiT")


@contextlib.contextmanager
def aggregator_registered():
    """the stand-in registered as an aggregator class (K14) too, for the duration: tests/test_xcit_cpu.py checks that nobody has
    registered it, so the registry is left as it was found"""
    from ptlflow_amd import xcit
    key = (XCiT.__module__, "XCiT")
    was = key in xcit._XCIT_CLASSES
    xcit_model.register()
    try:
        yield
    finally:
        if not was:
            xcit._XCIT_CLASSES.discard(key)


def context_loop_model(iters=(2, 3, 2), seed=31, aggregators=False):
    """`MsLoopModel` in its CCMR form with `xcit` replaced by stand-in `XCiT(separate=False)` modules (and, `aggregators`, the update
    block's per-scale gates by `XCiT(separate=True)`: accelerate it inside `aggregator_registered()`)"""
    from ms_loop_model import MsLoopModel
    register()
    model = MsLoopModel("ccmr", iters, seed)
    n = len(iters)
    model.xcit = torch.nn.ModuleList([randomize(XCiT(separate=False), 71 + i) for i in range(n)])
    if aggregators:
        model.update_block.aggregator = torch.nn.ModuleList([randomize(XCiT(separate=True), 83 + i) for i in range(n)])
    return model.eval()
