"""The convex-upsampling kernels' outputs are held to the bits of the commit that tests/golden/upsample_bits.json names: sha256 of
every output's bytes, recorded once on the MI355X from that commit.  All of them sum in a fixed order (no atomics), so the bits are
reproducible.  The arithmetic of every kernel here is written once, in csrc/pfk_upsample.h; this file is what "unchanged" means for it.

Grids (B, H, W): (2, 5, 7) — M = 70, no multiple of 4 or 16, below the fused kernels' 128-pixel tile, every pixel near a border — and
(1, 11, 13) — M = 143, one full and one partial fused tile.  Flow randn * 4, mask logits randn * 3, seeded CPU generators.

`python tests/test_gpu_upsample_bits.py COMMIT [OUT.json]` records the file from the tree it runs in (every case twice; a digest that
differs between the two runs is refused).  It uses only `torch.ops.pfk.*` calls that exist on both sides of the comparison."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upsample_bits.json")
GRIDS = ((2, 5, 7), (1, 11, 13))
DEV = "cuda:0"


def digest(*tensors) -> str:
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def inputs(B, H, W):
    """CPU tensors, made once per grid and never written: flow [M, 2], info [M, 8], mask logits [M, 576], the upsampled gradients"""
    g = torch.Generator().manual_seed(1700 + 100 * B + 10 * H + W)
    M = B * H * W
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"flow": r(M, 2) * 4, "info": r(M, 8), "mask": r(M, 576) * 3,
            "gflow_up": r(B, 2, 8 * H, 8 * W), "ginfo_up": r(B, 8, 8 * H, 8 * W),
            "x": r(M, 64), "wt": r(576, 64, 1, 1) / 8, "bias": r(576) * 0.1}


def wide(t: torch.Tensor, ld: int, first: int = 0) -> torch.Tensor:
    """`t` [M, n] as columns first .. first + n of a zero [M, ld] buffer on the GPU"""
    buf = torch.zeros(t.shape[0], ld, dtype=t.dtype, device=DEV)
    buf[:, first:first + t.shape[1]] = t.to(DEV)
    return buf[:, first:first + t.shape[1]]


# local, not op_gate's: this file also runs as a recording script, before the repository root is on sys.path
def nchw(t: torch.Tensor, B, H, W) -> torch.Tensor:
    return t.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def up(B, n, H, W) -> torch.Tensor:
    return torch.full((B, n, 8 * H, 8 * W), 7.0, device=DEV)


# ------------------------------------------------------------------------------------------------------------- forward
def fwd_plain(grid, form):
    B, H, W = grid
    c = inputs(*grid)
    out = up(B, 2, H, W)
    if form == "nchw":
        torch.ops.pfk.convex_upsample(nchw(c["flow"], B, H, W).to(DEV), c["mask"].to(DEV), out)
    elif form == "pm":
        torch.ops.pfk.convex_upsample_pm(wide(c["flow"], 8, 4), c["mask"].to(DEV), out)
    elif form == "pm-ld577":             # mask rows that are not 16-byte aligned: one pixel per wave
        torch.ops.pfk.convex_upsample_pm(wide(c["flow"], 8, 4), wide(c["mask"], 577), out)
    else:
        torch.ops.pfk.convex_upsample_pm(wide(c["flow"], 8, 4), c["mask"].to(DEV, torch.bfloat16), out)
    return digest(out)


def fwd_info(grid, n, b16):
    B, H, W = grid
    c = inputs(*grid)
    fi = wide(torch.cat([c["flow"], c["info"][:, :n]], 1), 12)
    flow_up, info_up = up(B, 2, H, W), up(B, n, H, W)
    if b16:
        torch.ops.pfk.convex_upsample_info_pm_b16(fi[:, :2], fi[:, 2:], c["mask"].to(DEV, torch.bfloat16), flow_up, info_up)
    else:
        torch.ops.pfk.convex_upsample_info_pm(fi[:, :2], fi[:, 2:], c["mask"].to(DEV), flow_up, info_up)
    return digest(flow_up, info_up)


def fwd_fused(grid, b16):
    from ptlflow_amd.packing import pack_conv_weight, permute_mask_head
    B, H, W = grid
    c = inputs(*grid)
    wp, bp = permute_mask_head(pack_conv_weight(c["wt"], [(0, 64, 64)], 64 if b16 else 32), c["bias"])
    dt = torch.bfloat16 if b16 else torch.float32
    out = up(B, 2, H, W)
    torch.ops.pfk.mask_upsample(wide(c["x"].to(dt), 128, 64), wp.to(DEV, dt), bp.to(DEV), 0.25, wide(c["flow"], 8, 4), out)
    return digest(out)


# ------------------------------------------------------------------------------------------------------------- backward
def bwd_plain(grid, form):
    B, H, W = grid
    c = inputs(*grid)
    flow = nchw(c["flow"], B, H, W).to(DEV) if form == "nchw" else wide(c["flow"], 4)
    gmask = torch.full((B * H * W, 576), 7.0, device=DEV)
    gflow = torch.full((B, 2, H, W), 7.0, device=DEV)
    torch.ops.pfk.convex_upsample_bwd(flow, c["mask"].to(DEV), c["gflow_up"].to(DEV), gmask, gflow)
    return digest(gmask, gflow)


def bwd_info(grid, n, with_ginfo=True):
    B, H, W = grid
    c = inputs(*grid)
    M = B * H * W
    fi = wide(torch.cat([c["flow"], c["info"][:, :n]], 1), 12)
    gi = c["ginfo_up"][:, :n].contiguous().to(DEV) if with_ginfo else None
    gmask = torch.full((M, 576), 7.0, device=DEV)
    grad = torch.full((M, 12), 7.0, device=DEV)       # grad_flow | grad_info, slices of one buffer like the training node's
    torch.ops.pfk.convex_upsample_info_bwd(fi[:, :2], fi[:, 2:], c["mask"].to(DEV), c["gflow_up"].to(DEV), gi, gmask,
                                           grad[:, :2], grad[:, 2:2 + n])
    return digest(gmask, grad[:, :2], grad[:, 2:2 + n])


CASES = {}
for _g in GRIDS:
    _t = "%dx%dx%d" % _g
    for _form in ("nchw", "pm", "pm-ld577", "pm-bf16"):
        CASES[f"fwd/{_form}/{_t}"] = functools.partial(fwd_plain, _g, _form)
    for _n in (1, 4, 8):
        CASES[f"fwd/info{_n}/fp32/{_t}"] = functools.partial(fwd_info, _g, _n, False)
        CASES[f"fwd/info{_n}/bf16/{_t}"] = functools.partial(fwd_info, _g, _n, True)
    CASES[f"fwd/fused/fp32/{_t}"] = functools.partial(fwd_fused, _g, False)
    CASES[f"fwd/fused/bf16/{_t}"] = functools.partial(fwd_fused, _g, True)
    for _form in ("nchw", "pm"):
        CASES[f"bwd/{_form}/{_t}"] = functools.partial(bwd_plain, _g, _form)
    for _n in (0, 4, 8):
        CASES[f"bwd/info{_n}/{_t}"] = functools.partial(bwd_info, _g, _n)
    CASES[f"bwd/info4/no-grad-info/{_t}"] = functools.partial(bwd_info, _g, 4, False)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_bits(gpu, name):
    g = golden()
    assert sorted(g["sha256"]) == sorted(CASES)
    assert CASES[name]() == g["sha256"][name], f"{name}: output bits differ from commit {g['parent_commit']}"


def test_the_kernels_the_cases_name_differ():
    """the recorded digests tell the inputs apart: a bf16 mask, a dropped grad_info_up and another n_info each change the bits, and
    the three fp32 forms of the plain forward (NCHW flow, pixel-major flow, one pixel per wave) are one result"""
    g = golden()["sha256"]
    for grid in GRIDS:
        t = "%dx%dx%d" % grid
        assert g[f"fwd/nchw/{t}"] == g[f"fwd/pm/{t}"] == g[f"fwd/pm-ld577/{t}"] != g[f"fwd/pm-bf16/{t}"]
        assert g[f"bwd/nchw/{t}"] == g[f"bwd/pm/{t}"]
        assert g[f"bwd/info4/{t}"] != g[f"bwd/info4/no-grad-info/{t}"]
        assert len({g[f"fwd/info{n}/fp32/{t}"] for n in (1, 4, 8)}) == 3


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
