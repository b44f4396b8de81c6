"""The packed weight tables of every engine (`engine.w`: `.w` / `.b` / `.ww` / `.w1d` ...) are held to the bits of the commit that
tests/golden/engine_pack_bits.json names: sha256 over the sorted (key, dtype, shape, bytes) of the dict, engines built on the CPU from
`synth.synth_state_dict`.  Packing is host code (reshapes, the BatchNorm fold, the fp64 Winograd transforms, bf16 rounding), so the
digests need the built library (the constructors load it) but no GPU.

`python tests/test_engine_pack_bits.py` records the file from the tree it runs in."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_pack_bits.json")
CPU = torch.device("cpu")


def digest(w) -> str:
    h = hashlib.sha256()
    for key in sorted(w):
        t = w[key]
        if t is None:
            h.update(f"{key}|None;".encode())
            continue
        h.update(f"{key}|{t.dtype}|{tuple(t.shape)}|".encode())
        h.update(t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
        h.update(b";")
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------- the engines
def _update(spec_name, precision, hoist=True):
    from ptlflow_amd import update as U
    from ptlflow_amd.synth import synth_update_block_params
    spec = {"basic": U.basic_spec, "small": U.small_spec, "gma": U.gma_spec, "ccmr": lambda: U.ccmr_spec(324)}[spec_name]()
    return U.UpdateEngine(synth_update_block_params(spec, 11), spec, CPU, precision, hoist_context=hoist)


def _sea_update(precision):
    from ptlflow_amd import sea_update as S
    from ptlflow_amd.synth import synth_state_dict
    shapes = dict(S.sea_block_shapes(324, 2))
    for head, sh in S.HEAD_SHAPES.items():
        shapes.update({f"{head}.{k}": v for k, v in sh.items()})
    return S.SeaUpdateEngine(synth_state_dict(shapes, 12), S.sea_spec(324), CPU, 2, precision)


def _encoder(kind, small, precision):
    from ptlflow_amd.encoder import EncoderEngine
    from ptlflow_amd.raft import Encoder
    from ptlflow_amd.synth import synth_state_dict
    own = Encoder(128 if small else 256, kind, small).state_dict()
    shapes = {"fnet." + k: tuple(v.shape) for k, v in own.items()}      # "fnet." prefix: the encoder init statistics
    P = {k[len("fnet."):]: v for k, v in synth_state_dict(shapes, 13).items()}
    return EncoderEngine(P, kind, CPU, precision, small=small)


def _resnet_table(counts):
    table, cin = [], 64
    for i, (dim, stride, n) in enumerate(zip((64, 128, 256), (1, 2, 2), counts), start=1):
        for j in range(n):
            s = stride if j == 0 else 1
            table.append((f"layer{i}.{j}", cin, dim, s, s != 1 or cin != dim))
            cin = dim
    return table


def _resnet(counts, input_dim, precision):
    from ptlflow_amd.sea_encoder import ResNetFPNEngine, resnet_fpn_shapes
    from ptlflow_amd.synth import synth_state_dict
    shapes = {"fnet." + k: v for k, v in resnet_fpn_shapes(input_dim, 64, _resnet_table(counts), 256).items()}
    P = {k[len("fnet."):]: v for k, v in synth_state_dict(shapes, 14).items()}
    return ResNetFPNEngine(P, CPU, precision)


def _conv(precision):
    from ptlflow_amd.sea_encoder import ConvEngine
    from ptlflow_amd.synth import synth_state_dict
    return ConvEngine(synth_state_dict({"conv.weight": (256, 256, 3, 3), "conv.bias": (256,)}, 15), CPU, precision)


CASES = {}
for _p in ("fp32", "bf16", "bf16x3"):
    for _s in ("basic", "small", "gma", "ccmr"):
        CASES[f"update/{_s}/{_p}"] = functools.partial(_update, _s, _p)
    CASES[f"update/basic-unhoisted/{_p}"] = functools.partial(_update, "basic", _p, False)
for _p in ("fp32", "bf16"):
    CASES[f"sea_update/{_p}"] = functools.partial(_sea_update, _p)
    for _name, _kind, _small in (("instance", "instance", False), ("batch", "batch", False), ("small-instance", "instance", True)):
        CASES[f"encoder/{_name}/{_p}"] = functools.partial(_encoder, _kind, _small, _p)
    CASES[f"resnet/222-6ch/{_p}"] = functools.partial(_resnet, (2, 2, 2), 6, _p)
    CASES[f"resnet/346-3ch/{_p}"] = functools.partial(_resnet, (3, 4, 6), 3, _p)
    CASES[f"conv/256/{_p}"] = functools.partial(_conv, _p)
CASES["encoder/instance/bf16x3"] = functools.partial(_encoder, "instance", False, "bf16x3")


@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_table_bits(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden["sha256"]) == sorted(CASES)
    got = digest(CASES[name]().w)
    assert got == golden["sha256"][name], f"{name}: the packed table differs from commit {golden['parent_commit']}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    commit = sys.argv[1]
    with open(GOLDEN, "w") as f:
        json.dump({"parent_commit": commit, "sha256": {k: digest(CASES[k]().w) for k in sorted(CASES)}}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} digests from {commit}")
