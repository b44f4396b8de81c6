"""ptlflow_amd/conv_path.py: the precision names resolve to the three paths, CCMR's exception included, and every option refuses an
unknown name with the words it used before the module existed."""
import pytest
import torch

from ptlflow_amd import conv_path as C


def test_paths_and_their_facts():
    facts = lambda p: (p.planes, p.dtype, p.quantum, p.element_bytes, p.kchunk, p.fp32_tiles, p.b16)  # noqa: E731
    assert facts(C.resolve("fp32")) == (0, torch.float32, 4, 4.0, 32, True, False)
    assert facts(C.resolve("bf16")) == (0, torch.bfloat16, 8, 2.0, 64, False, True)
    assert facts(C.resolve("bf16x3")) == (2, torch.float32, 4, 4.0, 32, False, False)
    assert facts(C.resolve("bf16x6")) == (3, torch.float32, 4, 4.0, 32, False, False)
    # CCMR on "bf16": the split kernel with one plane, fp32 rows; every other name is what it is without the exception
    assert facts(C.resolve("bf16", external_aggregate=True)) == (1, torch.float32, 4, 4.0, 32, False, False)
    for name in ("fp32", "bf16x3", "bf16x6"):
        assert C.resolve(name, external_aggregate=True) is C.resolve(name)
    assert C.resolve("fp32").segment(126) == [(0, 126, 128)] and C.resolve("bf16").segment(324) == [(0, 324, 328)]


def test_pack_is_pack_conv_operand():
    from ptlflow_amd.packing import pack_conv_operand
    w = torch.randn(8, 12, 3, 3, generator=torch.Generator().manual_seed(3))
    for name, ext in (("fp32", False), ("bf16", False), ("bf16", True), ("bf16x3", False), ("bf16x6", False)):
        p = C.resolve(name, ext)
        got, want = p.pack(w, p.segment(12)), pack_conv_operand(w, p.segment(12), p.b16, p.planes)
        assert got.dtype == want.dtype and torch.equal(got, want)
        assert got.shape[-1] == 9 * p.kchunk


def test_refusals_word_for_word():
    from ptlflow_amd.patch import _sea_precision
    from ptlflow_amd.train import check_precision
    with pytest.raises(ValueError) as e:
        C.resolve("fp16")
    assert str(e.value) == "conv_precision must be one of ['bf16', 'bf16x3', 'bf16x6', 'fp32'], got 'fp16'"
    with pytest.raises(ValueError) as e:
        check_precision("fp16")
    assert str(e.value) == "precision must be one of ('fp32', 'bf16'), got 'fp16'"
    with pytest.raises(ValueError) as e:
        check_precision("bf16x3", "train_precision")
    assert str(e.value) == "train_precision must be one of ('fp32', 'bf16'), got 'bf16x3'"
    with pytest.raises(ValueError) as e:
        _sea_precision("bf16x3", "sea_raft_encoders")
    assert str(e.value) == "sea_raft_encoders must be False, True, 'fp32' or 'bf16', got 'bf16x3'"
    assert [_sea_precision(v) for v in (False, None, True, "fp32", "bf16")] == [None, None, "fp32", "fp32", "bf16"]
    with pytest.raises(ValueError):
        _sea_precision(1)


def test_launcher_orders_the_arguments_each_op_wants():
    calls = []

    class Ops:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a))

    kw = dict(srcs=["s"], B=1, H=2, W=3, kh=1, kw=5, weight="w", bias="b", cout=8, out="o", epi=C.EPI_GRU_ZR, relu=True, scale=0.5,
              h="h", h_b16="hb", z="z", rh="rh", workspace="ws", residual="r", cout_active=4, cout_split=4)
    C.resolve("fp32").conv(Ops(), **kw)
    C.resolve("bf16").conv(Ops(), **kw)
    C.resolve("bf16").conv(Ops(), **dict(kw, epi=C.EPI_GRU_Q))
    C.resolve("bf16").conv(Ops(), **dict(kw, epi=C.EPI_LINEAR))
    # `UpdateEngine._conv` passes the same arguments positionally, in the signature's order
    C.resolve("fp32").conv(Ops(), ["s"], 1, 2, 3, 1, 5, "w", "b", 8, "o", C.EPI_GRU_ZR, True, 0.5, "h", "hb", "z", "rh", "ws", "r", 1, False, 4, 4)
    assert calls.pop() == calls[0]
    head = (["s"], 1, 2, 3, 1, 5, "w", "b", 8)
    assert calls[0] == ("conv2d", (*head, 1, True, 0.5, "o", "h", "z", "rh", "ws", "r", 1, False, 4, 4))
    # bf16 rows: z|r reads h from the twin only, q also gets the fp32 h, a linear launch neither; no workspace, no cout_active
    assert calls[1] == ("conv2d_b16", (*head, 1, True, 0.5, "o", None, "hb", "z", "rh", "r", 1, False))
    assert calls[2] == ("conv2d_b16", (*head, 2, True, 0.5, "o", "h", "hb", "z", "rh", "r", 1, False))
    assert calls[3] == ("conv2d_b16", (*head, 0, True, 0.5, "o", None, None, "z", "rh", "r", 1, False))
