"""`pfk_corr_lookup_coords_bwd_f32` — the coordinate gradient of the pyramid lookup — under gates 1-4 of
tests/op_gate.py, and `corr._LookupFn` with and without ``coords_grad``.

Reference: float64 autograd through `seam_model.TorchCorrBlock` on the same fp32 feature maps and coordinates.  The block's fp32
level maps (torch, CPU) are the kernel's input and, widened to float64, the reference's: the comparison is on the kernel's own inputs.

The formula (include/pfk.h), per source pixel:  grad_x = sum over the n = L (2r+1)^2 taps of
    g * 2^-l * [(v10 - v00)(1 - wy) + (v11 - v01) wy]            (grad_y: x and y exchanged)
Bound, by the harness's rules, per element |got - ref| <= 2^-24 * (K * A + P):
  A   the same sum with absolute values, sum |g| 2^-l [(|v10| + |v00|)(1 - wy) + (|v11| + |v01|) wy];
  K   n + 8: a term carries seven roundings on its magnitudes (two differences, 1 - wy, two products, their sum, the product with
      g; g * 2^-l and wy = iy - floor(iy) are exact), a sum of n terms in any order n - 1 more, + 2 as everywhere: 170 (L = 2, r = 4),
      332 (L = 4, r = 4), 204 (L = 4, r = 3);
  P   the sample point itself is fp32 arithmetic that the float64 reference does not share: x/2^l + i - r is rounded once
      (2^-24 |p|), then pfk_lookup.h's round trip 2p / (S - 1) - 1 + 1, times (S - 1)/2 adds at most 2^-24 (4 |p| + |p - (S-1)/2|):
      |d wy| <= 2^-24 (6 |p_y| + (H_l - 1)/2) in all, and the term moves by at most |g| 2^-l (|v00| + |v01| + |v10| + |v11|) |d wy|.
      P is the sum of that over the taps (for grad_y: |d wx| with p_x and W_l).
The gradient jumps where a sample point is an integer, so the inputs are built with the fractional part of x / 2^l and y / 2^l in
[2^-8, 1 - 2^-8] at every level, which the test asserts before it compares: a stated condition on the inputs, not a tolerance.  (The
position error above is below 2^-24 * 6000 = 3.6e-4 < 2^-8 for every coordinate used here: kernel and reference floor alike.)

Measured on an MI355X, worst over grids and families (relative L2 | error as a fraction of the per-element bound):
  5 x 7, L = 2, r = 4       1.7e-7 | 0.014        (K A is 0.84 of the bound, the position term P the rest)
  16 x 24, L = 4, r = 4     4.7e-7 | 0.018        (0.73)
  16 x 24, L = 4, r = 3     5.5e-7 | 0.048        (0.63)
  far outside               exactly 0 at every grid
"""
import functools

import pytest
import torch

from op_gate import Rows, flat_out, gates, leaf, same_bits, tail_kept
from seam_model import TorchCorrBlock

pytestmark = pytest.mark.gpu

B = 2
GRIDS = {"5x7_L2_r4": (5, 7, 2, 4), "16x24_L4_r4": (16, 24, 4, 4), "16x24_L4_r3": (16, 24, 4, 3)}
FAMILIES = ("noise", "borders", "far")
LO, HI = 2.0 ** -8, 1 - 2.0 ** -8


def grid_of(h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys]).expand(B, 2, h, w).contiguous()


def off_integers(c, L):
    """True where the fractional part of c / 2^l lies in [2^-8, 1 - 2^-8] for every level l < L"""
    ok = torch.ones_like(c, dtype=torch.bool)
    for l in range(L):
        f = c.double() / 2 ** l
        f = f - f.floor()
        ok &= (f >= LO) & (f <= HI)
    return ok


def coords_family(name, h, w, L, seed):
    g = torch.Generator().manual_seed(seed)
    base = grid_of(h, w)
    if name == "borders":      # windows that cross each border: the left / right columns and the top / bottom rows of the map
        base[:, 0] = torch.where(base[:, 0] < w / 2, 0.0, float(w - 1))
        base[:, 1] = torch.where(base[:, 1] < h / 2, 0.0, float(h - 1))
    elif name == "far":        # every tap of every level outside the map
        base = base + 200.0
    spread = 2.0 ** 0.5 if name == "noise" else 0.6
    c = base + torch.randn(base.shape, generator=g) * spread
    for _ in range(200):
        bad = ~off_integers(c, L)
        if not bool(bad.any()):
            break
        c = torch.where(bad, base + torch.randn(base.shape, generator=g) * spread, c)
    return c


def taps64(levels, coords, r):
    """per level: the four float64 values around every tap [M, n (x offset), n (y offset)] with zero padding, the fractional parts and
    the sample positions"""
    Bc, _, h, w = coords.shape
    M, n = Bc * h * w, 2 * r + 1
    centre = coords.double().permute(0, 2, 3, 1).reshape(M, 2)
    off = torch.arange(-r, r + 1, dtype=torch.float64)
    out = []
    for l, lvl in enumerate(levels):
        hl, wl = lvl.shape[-2:]
        flat = lvl.double().reshape(M, hl * wl)
        px, py = centre[:, 0:1] / 2 ** l + off, centre[:, 1:2] / 2 ** l + off          # [M, n]
        x0, y0 = px.floor(), py.floor()

        def at(dy, dx):
            yy = (y0.long() + dy)[:, None, :].expand(M, n, n)
            xx = (x0.long() + dx)[:, :, None].expand(M, n, n)
            valid = (yy >= 0) & (yy < hl) & (xx >= 0) & (xx < wl)
            idx = yy.clamp(0, hl - 1) * wl + xx.clamp(0, wl - 1)
            return flat.gather(1, idx.reshape(M, n * n)).view(M, n, n) * valid

        out.append({"v00": at(0, 0), "v10": at(0, 1), "v01": at(1, 0), "v11": at(1, 1), "wx": (px - x0)[:, :, None],
                    "wy": (py - y0)[:, None, :], "px": px[:, :, None], "py": py[:, None, :], "hl": hl, "wl": wl, "inv": 2.0 ** -l})
    return out


@functools.lru_cache(maxsize=None)
def pyramid(grid):
    """the fp32 level maps [M, h_l, w_l] of a 16-channel feature-map pair, and a float64 TorchCorrBlock on exactly those maps"""
    h, w, L, r = GRIDS[grid]
    g = torch.Generator().manual_seed(h * 100 + w + L + r)
    f1, f2 = torch.randn(B, 16, h, w, generator=g), torch.randn(B, 16, h, w, generator=g)
    blk32 = TorchCorrBlock(f1, f2, num_levels=L, radius=r)
    blk64 = TorchCorrBlock(f1.double(), f2.double(), num_levels=L, radius=r)
    blk64.levels = [lv.double() for lv in blk32.levels]
    return [lv[:, 0].contiguous() for lv in blk32.levels], blk64


@functools.lru_cache(maxsize=None)
def case(grid, family):
    h, w, L, r = GRIDS[grid]
    n = 2 * r + 1
    levels, blk64 = pyramid(grid)
    coords = coords_family(family, h, w, L, seed=FAMILIES.index(family) + 10 * h)
    assert bool(off_integers(coords, L).all()), "the inputs must keep every sample point off the integers"
    g = torch.Generator().manual_seed(3)
    go = torch.randn(B * h * w, L * n * n, generator=g)
    c64 = leaf(coords, torch.float64)
    out = blk64(c64)                                                                     # [B, C, h, w]
    go_img = go.double().view(B, h, w, -1).permute(0, 3, 1, 2)
    (ref,) = torch.autograd.grad((out * go_img).sum(), c64)
    # the formula in float64, term by term: the reference again (checked), its sum of magnitudes and the position term
    form, A, P = torch.zeros(B * h * w, 2, dtype=torch.float64), torch.zeros(B * h * w, 2, dtype=torch.float64), torch.zeros(B * h * w, 2, dtype=torch.float64)
    for l, t in enumerate(taps64(levels, coords, r)):
        gl = go[:, l * n * n:(l + 1) * n * n].double().view(-1, n, n) * t["inv"]
        v00, v10, v01, v11, wx, wy = (t[k] for k in ("v00", "v10", "v01", "v11", "wx", "wy"))
        form[:, 0] += (gl * ((v10 - v00) * (1 - wy) + (v11 - v01) * wy)).sum((1, 2))
        form[:, 1] += (gl * ((v01 - v00) * (1 - wx) + (v11 - v10) * wx)).sum((1, 2))
        A[:, 0] += (gl.abs() * ((v10.abs() + v00.abs()) * (1 - wy) + (v11.abs() + v01.abs()) * wy)).sum((1, 2))
        A[:, 1] += (gl.abs() * ((v01.abs() + v00.abs()) * (1 - wx) + (v11.abs() + v10.abs()) * wx)).sum((1, 2))
        four = gl.abs() * (v00.abs() + v01.abs() + v10.abs() + v11.abs())
        P[:, 0] += (four * (6 * t["py"].abs() + (t["hl"] - 1) / 2)).sum((1, 2))
        P[:, 1] += (four * (6 * t["px"].abs() + (t["wl"] - 1) / 2)).sum((1, 2))
    img = lambda rows: rows.view(B, h, w, 2).permute(0, 3, 1, 2)
    assert float((img(form) - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max())), "the test's own formula is not the reference's"
    K = L * n * n + 8
    return {"levels": levels, "coords": coords, "go": go, "ref": ref, "mag": K * img(A) + img(P), "A": img(A)}


def run(levels, coords, go, r, gpu, pad=3):
    """the op on guarded buffers -> (the buffer behind grad_coords, grad_coords)"""
    M, C = go.shape
    g = Rows(M, C, gpu, go, pad=pad, nan_tail=True)
    flat, gc = flat_out(tuple(coords.shape), gpu)
    lv = [x.to(gpu) for x in levels]
    keep = [x.clone() for x in lv]
    torch.ops.pfk.corr_lookup_coords_bwd(lv, coords.to(gpu), r, g.rows, gc)
    torch.cuda.synchronize()
    assert tail_kept(flat), "memory past grad_coords was written"
    assert all(same_bits(a, b) for a, b in zip(lv, keep)), "the level maps were written"
    return flat, gc


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_kernel(gpu, grid, family):
    h, w, L, r = GRIDS[grid]
    c = case(grid, family)
    flat, gc = run(c["levels"], c["coords"], c["go"], r, gpu)
    if family == "far":
        assert float(c["A"].abs().max()) == 0.0 and bool((gc == 0).all()), "far outside the map the gradient is exactly zero"
    else:
        assert float(c["ref"].abs().mean()) > 0.05, "a reference gradient that tests nothing"
    gates(f"lookup coords grad {grid} {family}", gc, c["ref"], c["mag"], 1.0)
    if family != "far":
        share = float(((L * (2 * r + 1) ** 2 + 8) * c["A"]).sum() / c["mag"].sum())
        print(f"   K * A is {share:.2f} of the bound, the position term P the rest")
    flat2, _ = run(c["levels"], c["coords"], c["go"], r, gpu)
    assert torch.equal(flat2, flat), "a second run gives other bits"
    # grad_out rows without padding (ld = C): the same bits
    _, gc3 = run(c["levels"], c["coords"], c["go"], r, gpu, pad=0)
    assert torch.equal(gc3, gc)


def test_non_finite_coordinates_give_exact_zero(gpu):
    """NaN, +-inf and absurd coordinates: exactly 0 for that pixel (both components), everything else as without them; the existing
    backward leaves grad_levels unchanged for the same pixels"""
    grid = "16x24_L4_r4"
    h, w, L, r = GRIDS[grid]
    c = case(grid, "noise")
    bad = c["coords"].clone()
    spots = {(0, 0, 0): float("nan"), (1, 0, 1): float("inf"), (0, 1, 0): -float("inf"), (0, 1, 1): 3.0e9, (1, 1, 2): -2.5e7, (1, 5, 5): 1.0e30}
    for (ch, y, x), v in spots.items():
        bad[:, ch, y, x] = v
    _, good = run(c["levels"], c["coords"], c["go"], r, gpu)
    _, gc = run(c["levels"], bad, c["go"], r, gpu)
    assert bool(torch.isfinite(gc).all())
    hit = torch.zeros(B, 1, h, w, dtype=torch.bool)
    for (_, y, x) in spots:
        hit[:, :, y, x] = True
    hit = hit.expand(B, 2, h, w).to(gpu)
    assert bool((gc[hit] == 0).all()) and torch.equal(gc[~hit], good[~hit])
    # pfk_corr_lookup_bwd_f32 on the same coordinates: the maps of those pixels stay what they were
    sizes = [tuple(lv.shape[-2:]) for lv in c["levels"]]
    glv = [torch.full((B * h * w, (a * b + 3) // 4 * 4), 0.5, device=gpu) for a, b in sizes]
    torch.ops.pfk.corr_lookup_bwd(glv, [s[0] for s in sizes], [s[1] for s in sizes], bad.to(gpu), r, c["go"].to(gpu))
    rows = hit[:, 0].reshape(-1)
    assert all(bool((g[rows] == 0.5).all()) for g in glv)


def test_one_pixel_levels_give_exact_zero(gpu):
    """5 x 7 with three levels: level 2 is 1 x 1 (the round trip divides by zero); 2 x 24 with two: level 1 is 1 x 12.  With a gradient
    on that level alone the result is exactly zero; with one on every level it is the result of the other levels; and the existing
    backward leaves that level's grad_levels unchanged"""
    g = torch.Generator().manual_seed(11)
    for (h, w, L, dead) in ((5, 7, 3, 2), (2, 24, 2, 1), (24, 2, 2, 1)):
        r, n = 4, 9
        f1, f2 = torch.randn(B, 16, h, w, generator=g), torch.randn(B, 16, h, w, generator=g)
        levels = [lv[:, 0].contiguous() for lv in TorchCorrBlock(f1, f2, num_levels=L, radius=r).levels]
        assert 1 in levels[dead].shape[-2:]
        coords = coords_family("noise", h, w, L, seed=h)
        go = torch.randn(B * h * w, L * n * n, generator=g)
        only = torch.zeros_like(go)
        only[:, dead * n * n:(dead + 1) * n * n] = go[:, dead * n * n:(dead + 1) * n * n]
        _, gc = run(levels, coords, only, r, gpu)
        assert bool((gc == 0).all()), f"{h}x{w}: a 1-pixel level contributes"
        _, full = run(levels, coords, go, r, gpu)
        _, rest = run(levels, coords, go - only, r, gpu)
        assert bool(torch.isfinite(full).all()) and torch.equal(full, rest)
        assert float(full.abs().max()) > 0
        # pfk_corr_lookup_bwd_f32 on the same call: the 1-pixel level's gradient maps stay what they were, the others do not
        sizes = [tuple(lv.shape[-2:]) for lv in levels]
        glv = [torch.full((B * h * w, max(4, (a * b + 3) // 4 * 4)), 0.5, device=gpu) for a, b in sizes]
        torch.ops.pfk.corr_lookup_bwd(glv, [s[0] for s in sizes], [s[1] for s in sizes], coords.to(gpu), r, go.to(gpu))
        assert bool((glv[dead] == 0.5).all()), f"{h}x{w}: grad_levels of the 1-pixel level was changed"
        assert all(bool((g != 0.5).any()) and bool(torch.isfinite(g).all()) for l, g in enumerate(glv) if l != dead)


def test_lookup_node(gpu):
    """`corr._LookupFn`: with ``coords_grad=True`` the coordinates get the kernel's gradient (the op on the block's own levels, bit
    for bit) and the feature maps the gradients they always got; with the default the coordinates get none"""
    from ptlflow_amd.corr import CorrBlock
    h, w, L, r = 5, 7, 2, 4
    g = torch.Generator().manual_seed(9)
    f1, f2 = torch.randn(B, 32, h, w, generator=g).to(gpu), torch.randn(B, 32, h, w, generator=g).to(gpu)
    coords = coords_family("noise", h, w, L, seed=1).to(gpu)
    go = torch.randn(B, L * 81, h, w, generator=g).to(gpu)
    res = {}
    for flag in (True, False):
        a, b, c = leaf(f1, torch.float32), leaf(f2, torch.float32), leaf(coords, torch.float32)
        block = CorrBlock(a, b, num_levels=L, radius=r, coords_grad=flag)
        out = block(c)
        res[flag] = (out.detach().clone(), torch.autograd.grad(out, (a, b, c), go, allow_unused=True), [lv.clone() for lv in block._levels])
    out_on, (ga_on, gb_on, gc_on), levels = res[True]
    out_off, (ga_off, gb_off, gc_off), _ = res[False]
    assert gc_off is None, "without coords_grad the lookup returns no coordinate gradient"
    assert torch.equal(out_on, out_off) and torch.equal(ga_on, ga_off) and torch.equal(gb_on, gb_off)
    direct = torch.empty_like(coords)
    rows = go.permute(0, 2, 3, 1).reshape(B * h * w, -1).contiguous()
    torch.ops.pfk.corr_lookup_coords_bwd(levels, coords, r, rows, direct)
    assert torch.equal(gc_on, direct) and float(direct.abs().mean()) > 0.05
    # frozen feature maps: the coordinates alone carry a gradient
    c = leaf(coords, torch.float32)
    out = CorrBlock(f1, f2, num_levels=L, radius=r, coords_grad=True)(c)
    (gc_frozen,) = torch.autograd.grad(out, c, go)
    assert torch.equal(gc_frozen, direct)
