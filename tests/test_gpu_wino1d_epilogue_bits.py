"""The gate epilogues of `pfk_conv1d_wino_f32` (GRU_ZR, GRU_Q) are held to the bits of the commit that
tests/golden/wino1d_epilogue_bits.json names: sha256 of the WHOLE buffers after a z|r launch and the q launch chained onto it —
z, r*h (with their sentinel rows past M), the [h | context | motion] rows and the context buffers (with their sentinel columns) —
recorded once on the MI355X from that commit, never from the code under test.  Nothing in the kernel depends on the grid or on timing,
so the bits are reproducible.

Cases, each in both orientations (1x5, 5x1), the smallest at which the epilogue can go wrong:
  ragged           2 x 23 x 31       partial tiles both ways, more than one block
  short-tile       1 x 1 x 3         one tile shorter than 4 outputs; vertically L = 1
  one-tile         1 x 5 x 4         exactly one full tile per row; vertically 4 + 1
  mid-image        3 x 9 x 13        108 / 117 tiles: a block that ends mid-image, images that change inside a block, ragged last block
  gma              1 x 7 x 10        gma widths: K = 384, the second source has another row stride
  hidden96         1 x 7 x 10        hidden 96, motion 64: cout 192 / 96, a column block with columns past cout, z | r boundary in a wave
  ragged-noctx     2 x 23 x 31       no context term (`residual` null)
  ragged-widectx   2 x 23 x 31       the context rows inside wider sentinel rows (`residual_ld` != cout)

The same runs are compared with float64 restated on what the launches consumed (the helpers of tests/test_gpu_winograd1d.py) under the
project's gate, 3e-5 + 2e-5 |ref| for z, r*h and h; the sentinels must be untouched and a repeated launch must give equal bits.

`python tests/test_gpu_wino1d_epilogue_bits.py COMMIT [OUT.json]` records the file from the tree it runs in (every case twice; a
digest that differs between the two runs is refused).  It uses only `torch.ops.pfk.conv2d_wino1d` and `pack_wino1d_weight`, which
exist on both sides of the comparison."""
import functools
import hashlib
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino1d_epilogue_bits.json")
EPI_GRU_ZR, EPI_GRU_Q = 1, 2
SENTINEL = 7.0               # no gate output can take it: sigmoid < 1, |r * h| < 1, |h| < 1
PAD_ROWS = 64

# name: (B, H, W, hidden, context, real motion channels, motion slice width, context term: "dense" / "wide" / None)
SHAPES = {
    "ragged": (2, 23, 31, 128, 128, 128, 128, "dense"),
    "short-tile": (1, 1, 3, 128, 128, 128, 128, "dense"),
    "one-tile": (1, 5, 4, 128, 128, 128, 128, "dense"),
    "mid-image": (3, 9, 13, 128, 128, 128, 128, "dense"),
    "gma": (1, 7, 10, 128, 128, 256, 256, "dense"),
    "hidden96": (1, 7, 10, 96, 32, 64, 64, "dense"),
    "ragged-noctx": (2, 23, 31, 128, 128, 128, 128, None),
    "ragged-widectx": (2, 23, 31, 128, 128, 128, 128, "wide"),
}
CASES = [f"{name}/{kh}x{kw}" for name in SHAPES for kh, kw in ((1, 5), (5, 1))]


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def launch_pair(case):
    """z|r (twice), then q (twice) on what z|r stored; returns every buffer on the CPU, before and after"""
    from ptlflow_amd.packing import pack_wino1d_weight
    name, k = case.split("/")
    kh, kw = map(int, k.split("x"))
    B, H, W, Ch, Ci, real, width, ctx_kind = SHAPES[name]
    M, row, K = B * H * W, Ch + Ci + width, Ch + real
    g = torch.Generator().manual_seed(1800 + CASES.index(case))
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    wzr, wq = rnd(2 * Ch, K, kh, kw) / math.sqrt(K * 5), rnd(Ch, K, kh, kw) / math.sqrt(K * 5)
    bzr, bq = rnd(2 * Ch) * 0.1, rnd(Ch) * 0.1
    act = rnd(M, row)
    act[:, :Ch] = torch.tanh(rnd(M, Ch))
    act = act.cuda()
    segs = [(0, Ch, Ch), (Ch, real, width)]
    pzr, pq = pack_wino1d_weight(wzr, segs).cuda(), pack_wino1d_weight(wq, segs).cuda()
    ctx, bufs = {"zr": None, "q": None}, {}
    if ctx_kind is not None:
        pad, off = (16, 8) if ctx_kind == "wide" else (0, 0)
        for n, cout in (("zr", 2 * Ch), ("q", Ch)):
            bufs[n] = torch.full((M, cout + pad), SENTINEL, device="cuda")
            bufs[n][:, off: off + cout] = (rnd(M, cout) * 0.5).cuda()
            ctx[n] = bufs[n][:, off: off + cout]
    z = torch.full((M + PAD_ROWS, Ch), SENTINEL, device="cuda")
    rh = torch.full((M + PAD_ROWS, Ch), SENTINEL, device="cuda")
    r = dict(M=M, Ch=Ch, Ci=Ci, real=real, shape=(B, H, W), k=(kh, kw), wzr=wzr, wq=wq, bzr=bzr, bq=bq, act0=act.cpu(),
             bufs0={n: b.cpu() for n, b in bufs.items()}, ctx0={n: (None if c is None else c.cpu()) for n, c in ctx.items()})
    op, h, motion = torch.ops.pfk.conv2d_wino1d, act[:, :Ch], act[:, Ch + Ci:]

    def zr():
        op([h, motion], B, H, W, kh, kw, pzr, bzr.cuda(), 2 * Ch, EPI_GRU_ZR, False, 1.0, None, h, z, rh, ctx["zr"])
        torch.cuda.synchronize()

    def q():
        op([rh[:M], motion], B, H, W, kh, kw, pq, bq.cuda(), Ch, EPI_GRU_Q, False, 1.0, None, h, z, None, ctx["q"])
        torch.cuda.synchronize()

    zr()
    r["act_zr"], r["z"], r["rh"] = act.cpu(), z.cpu(), rh.cpu()
    z.fill_(SENTINEL), rh.fill_(SENTINEL)
    zr()
    r["zr_again"] = torch.equal(z.cpu(), r["z"]) and torch.equal(rh.cpu(), r["rh"])
    q()
    r["act_q"], r["z_q"], r["rh_q"] = act.cpu(), z.cpu(), rh.cpu()
    r["bufs"] = {n: b.cpu() for n, b in bufs.items()}
    act[:, :Ch] = r["act0"][:, :Ch].cuda()      # q updates h in place: the same launch again from the same h
    q()
    r["q_again"] = torch.equal(act.cpu(), r["act_q"])
    return r


run = functools.lru_cache(maxsize=None)(launch_pair)


def digests(r):
    d = {"z": sha(r["z_q"]), "rh": sha(r["rh_q"]), "rows": sha(r["act_q"])}
    d.update({"ctx_" + n: sha(b) for n, b in r["bufs"].items()})
    return d


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES)
def test_epilogue_bits(gpu, case):
    g = golden()
    assert sorted(g["sha256"]) == sorted(CASES)
    assert digests(run(case)) == g["sha256"][case], f"{case}: buffers differ from commit {g['parent_commit']}"


@pytest.mark.parametrize("case", CASES)
def test_fp64_gate_sentinels_and_repeat(gpu, case):
    from op_gate import close32
    from op_refs import ref_q, ref_zr
    r = run(case)
    M, Ch, Ci, real, a0 = r["M"], r["Ch"], r["Ci"], r["real"], r["act0"]
    reals = [Ch, real]
    assert torch.equal(r["act_zr"], a0), "z|r wrote into the [h | context | motion] rows"
    assert bool((r["z"][M:] == SENTINEL).all()) and bool((r["rh"][M:] == SENTINEL).all()), "z|r wrote rows past M"
    assert r["zr_again"], "the same z|r launch gave other bits"
    z_ref, rh_ref = ref_zr([a0[:, :Ch], a0[:, Ch + Ci:]], reals, r["wzr"], r["bzr"], r["ctx0"]["zr"], a0[:, :Ch], r["shape"], r["k"])
    rz, rr = close32(r["z"][:M], z_ref, "z"), close32(r["rh"][:M], rh_ref, "r*h")
    assert torch.equal(r["act_q"][:, Ch:], a0[:, Ch:]), "q wrote outside h"
    assert torch.equal(r["z_q"], r["z"]) and torch.equal(r["rh_q"], r["rh"]), "q wrote into z / r*h"
    assert r["q_again"], "the same q launch gave other bits"
    for n, b in r["bufs"].items():
        assert torch.equal(b, r["bufs0"][n]), "wrote into the context rows or their neighbours"
    h_ref = ref_q([r["rh"][:M], a0[:, Ch + Ci:]], reals, r["wq"], r["bq"], r["ctx0"]["q"], r["z"][:M], a0[:, :Ch], r["shape"], r["k"])
    rq = close32(r["act_q"][:, :Ch], h_ref, "h")
    print(f"[ratio] wino1d epilogue {case} z={rz:.3f} rh={rr:.3f} h={rq:.3f}")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import ptlflow_amd
    ptlflow_amd.load_native()
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    recorded = {}
    for case in CASES:
        first, second = digests(launch_pair(case)), digests(launch_pair(case))
        if first != second:
            sys.exit(f"{case}: two runs differ ({first} / {second}); nothing written")
        recorded[case] = first
        print(case, first["rows"], flush=True)
    with open(out, "w") as f:
        json.dump({"parent_commit": commit, "sha256": recorded}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(recorded)} cases from {commit} -> {out}")
