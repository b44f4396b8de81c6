"""The encoder engines' outputs are held to the bits of the commit that tests/golden/engine_bits.json names: sha256 of the output's
fp32 bytes, recorded once on the MI355X from that commit.  The engines' launches are plain tile grids (no stream-K workspace) and the
instance-norm statistics a fixed-order chunked reduction, so the bits are reproducible.

Images are 2 x C x 72 x 104 in [-1, 1]: half / quarter / eighth grids 36 x 52, 18 x 26, 9 x 13 — the smallest frame with a stride-2
block on an even and on an odd grid; the odd last grid runs the Winograd kernels' row and column masks.  Every fp32 case runs under
two rules: the shipped `WINO_MIN_PIXELS` (at this size every launch is the direct kernel) and every entry of the engine's table
patched to 0 (every stride-1 3x3 convolution of the non-small engines on Winograd: plain, relu and residual form).

`python tests/test_gpu_engine_bits.py COMMIT [OUT.json]` records the file from the tree it runs in (every case twice; a digest that
differs between the two runs is refused).  It uses only what exists on both sides of the comparison: the constructors,
`eng.winograd`, `eng.max_matrix_bytes`, `eng(img)` and the two `WINO_MIN_PIXELS` dicts."""
import contextlib
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_bits.json")
B, H, W = 2, 72, 104
ENC_SEED = 4100          # tests/test_gpu_sea_encoder.py
VARIANTS = (("resnet18", 3), ("resnet18", 6), ("resnet34", 3))


def digest(t: torch.Tensor) -> str:
    torch.cuda.synchronize()
    return hashlib.sha256(t.float().cpu().contiguous().numpy().tobytes()).hexdigest()


def image(cin: int) -> torch.Tensor:
    return torch.rand(B, cin, H, W, generator=torch.Generator().manual_seed(100 + cin)) * 2 - 1


@contextlib.contextmanager
def thresholds(table, zero: bool):
    saved = dict(table)
    if zero:
        for k in table:
            table[k] = 0
    try:
        yield
    finally:
        table.update(saved)


# ------------------------------------------------------------------------------------------------------------- the engines
def run_encoder(kind, small, precision, zero=False, one_image_chunks=False):
    from ptlflow_amd import encoder as E
    from ptlflow_amd.raft import Encoder
    from ptlflow_amd.synth import synth_state_dict
    own = Encoder(128 if small else 256, kind, small).state_dict()
    shapes = {"fnet." + k: tuple(v.shape) for k, v in own.items()}      # "fnet." prefix: the encoder init statistics
    P = {k[len("fnet."):]: v for k, v in synth_state_dict(shapes, 21).items()}
    eng = E.EncoderEngine(P, kind, torch.device("cuda:0"), precision, small=small)
    if one_image_chunks:
        eng.max_matrix_bytes = 36 * 52 * 128 * 4
    with thresholds(E.WINO_MIN_PIXELS, zero):
        return digest(eng(image(3).cuda()))


def run_resnet(variant, precision, zero=False, winograd=True):
    import sea_full_model as M
    from ptlflow_amd import sea_encoder as S
    pretrain, cin = VARIANTS[variant]
    enc = M.load_seeded_encoder(M.ResNetFPN(pretrain=pretrain, input_dim=cin), ENC_SEED + variant).eval()
    eng = S.ResNetFPNEngine(enc.state_dict(), torch.device("cuda:0"), precision)
    eng.winograd = winograd
    with thresholds(S.WINO_MIN_PIXELS, zero):
        return digest(eng(image(cin).cuda()))


def run_conv(precision, zero=False, winograd=True):
    from ptlflow_amd import sea_encoder as S
    from ptlflow_amd.synth import synth_state_dict
    eng = S.ConvEngine(synth_state_dict({"conv.weight": (256, 256, 3, 3), "conv.bias": (256,)}, 22), torch.device("cuda:0"), precision)
    eng.winograd = winograd
    rows = (torch.rand(B * 9 * 13, 256, generator=torch.Generator().manual_seed(23)) * 2 - 1).cuda()
    with thresholds(S.WINO_MIN_PIXELS, zero):
        return digest(eng(rows, B, 9, 13))


CASES = {}
for _name, _kind, _small in (("instance", "instance", False), ("batch", "batch", False), ("none", "none", False),
                             ("small-instance", "instance", True), ("small-none", "none", True)):
    for _rule in ("shipped", "zero"):
        CASES[f"encoder/{_name}/fp32/{_rule}"] = functools.partial(run_encoder, _kind, _small, "fp32", _rule == "zero")
for _rule in ("shipped", "zero"):
    CASES[f"encoder/instance/fp32/one-image-chunks/{_rule}"] = functools.partial(run_encoder, "instance", False, "fp32", _rule == "zero", True)
    CASES[f"conv/fp32/{_rule}"] = functools.partial(run_conv, "fp32", _rule == "zero")
    for _v, (_pre, _cin) in enumerate(VARIANTS):
        CASES[f"resnet/{_pre}-{_cin}ch/fp32/{_rule}"] = functools.partial(run_resnet, _v, "fp32", _rule == "zero")
CASES["encoder/instance/bf16"] = functools.partial(run_encoder, "instance", False, "bf16")
CASES["encoder/batch/bf16"] = functools.partial(run_encoder, "batch", False, "bf16")
CASES["encoder/instance/bf16x3"] = functools.partial(run_encoder, "instance", False, "bf16x3")
CASES["conv/bf16"] = functools.partial(run_conv, "bf16")
for _v, (_pre, _cin) in enumerate(VARIANTS):
    CASES[f"resnet/{_pre}-{_cin}ch/bf16"] = functools.partial(run_resnet, _v, "bf16")


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_bits(gpu, name):
    g = golden()
    assert sorted(g["sha256"]) == sorted(CASES)
    assert CASES[name]() == g["sha256"][name], f"{name}: output bits differ from commit {g['parent_commit']}"


def test_patched_rule_takes_winograd():
    """the zero-threshold digests are another kernel's: they differ from the shipped rule's wherever a transformed weight exists, and
    agree on the small encoder, which has none"""
    g = golden()["sha256"]
    for name in g:
        if name.endswith("/zero"):
            assert (g[name] == g[name[:-4] + "shipped"]) == name.startswith("encoder/small-"), name


@pytest.mark.parametrize("variant", range(3))
def test_resnet_always_is_the_patched_rule(gpu, variant):
    pretrain, cin = VARIANTS[variant]
    assert run_resnet(variant, "fp32", winograd="always") == golden()["sha256"][f"resnet/{pretrain}-{cin}ch/fp32/zero"]


def test_conv_engine_winograd_off_is_the_direct_kernel(gpu):
    """`ConvEngine.winograd = False` selects the direct kernel, whatever the threshold table says"""
    assert run_conv("fp32", zero=True, winograd=False) == golden()["sha256"]["conv/fp32/shipped"]


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import ptlflow_amd
    ptlflow_amd.load_native()
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    recorded = {}
    for name in sorted(CASES):
        first, second = CASES[name](), CASES[name]()
        if first != second:
            sys.exit(f"{name}: two runs differ ({first} / {second}); nothing written")
        recorded[name] = first
        print(name, first, flush=True)
    with open(out, "w") as f:
        json.dump({"parent_commit": commit, "sha256": recorded}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(recorded)} digests from {commit} -> {out}")
