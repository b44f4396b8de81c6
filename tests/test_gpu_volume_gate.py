"""The two all-pairs correlation volumes, pfk_corr_volume_f32 (pfk_gemm.hip: the fp32 implicit GEMM's `launch()` with `batches = B`)
and pfk_corr_volume_bf16 (pfk_corr_bf16.hip), held to the fp64 op gate of tests/op_gate.py.

    out[b, i, j] = scale * <f1[b, i, :], f2[b, j, :]>,  scale = float32(1 / sqrt(D))

against float64 on the kernel's own inputs (tests/op_refs.py::volume_case): ref = scale * sum a b, mag = |scale| sum |a| |b|, K = D + 3
(D roundings of the sum in any order, one for the scale, two to spare).  fp32: gates 1 and 2 (relative L2 <= OP_TOL, |err| <=
K 2^-24 mag).  bf16 (products of bf16 values are exact in fp32; one rounding to bf16 at the end): |err| <= K 2^-24 mag (1 + 2^-8) +
2^-8 |ref|, which implies a relative L2 of at most 2^-8 (1 + eps) — the kernel has no fp32 twin.  Every case: inputs between NaN guards,
the output at the head of a sentinel-filled flat buffer whose tail must keep the sentinel, the same bits on a second run.

What each case reaches is restated in Python (`f32_schedule`, `b16_path`) and asserted.
 fp32, through torch.ops.pfk.corr_volume, forced on cfgs 0, 4, 10, 11 and on the heuristic:
   (2, 117, 130, 64)     N2 = 130: scalar stores and a batch stride that is no multiple of 4 (o_bs = 15210); heuristic: cfg 0
   (2, 132, 120, 128)    N2 = 120: float4 stores; heuristic: cfg 0
   (1, 2050, 2114, 32)   cfg 10: 33 x 34 tiles of 64 x 64, the 16 x 16 supertile walk with a ragged last band and column block
   (2, 2050, 4000, 32)   the heuristic's cfg 11: 33 x 32 tiles of 64 x 128, supertile walk, B = 2
 fp32, through the C ABI: (2, 150, 140, 36) with ld1 = 44 and ld2 = 64 = round_up(D, 32).  f1's pad columns hold NaN.  f2's rows are
   read as packed weight rows, K-step by K-step over all ld2 columns, against f1 channels that the kernel zeroes past D: the pad
   columns of f2 must hold finite values (the contract of include/pfk.h's corr volume: zeros), and zeros is what the test puts there.
 bf16, through torch.ops.pfk.corr_volume_bf16 (128 x 128 tiles, K chunks of 64):
   (2, 130, 117, 40)     odd N2: scalar stores; a partial K chunk
   (2, 132, 132, 64)     N2 % 8 = 4: scalar stores with a batch offset
   (1, 257, 264, 72)     the 16-byte store path, 1.125 chunks, 3 x 3 tiles with ragged last ones
   (1, 40, 9, 8)         one tile, one eighth of a chunk
   (1, 4100, 4230, 8)    33 x 34 tiles: the supertile walk with ragged edges
 bf16, through the C ABI: (2, 70, 133, 40) with ld1 = 48, ld2 = 56 and NaN in the pad columns of both (a chunk's 16-byte pieces past D
   are not loaded).

Measured on an MI355X, worst over the cases of each test (relative L2 | error as a fraction of the per-element bound).  Records, not
thresholds: the thresholds are OP_TOL and a ratio of 1; a bf16 ratio near 1 is the half-ulp rounding itself.
  test_volume_f32_small          2.0e-7 | 0.054
  test_volume_f32_supertiles     1.1e-7 | 0.167
  test_volume_f32_padded_rows    1.1e-7 | 0.094
  test_volume_b16                1.7e-3 | 0.996
  test_volume_b16_padded_rows    1.7e-3 | 0.987
Nothing failed: no kernel was changed.  tests/test_op_gate_cpu.py shows that a batch stride off by one and a dropped partial K chunk
fail these gates, in fp32 and in bf16.
The module's 20 cases take 3.5 s on an MI355X run alone (pytest's wall time, with the start of the process and the float64
references), 2 s inside the suite; the slowest are the two supertile volumes, bf16 (1, 4100, 4230, 8) 0.65 s and fp32
(2, 2050, 4000, 32) 0.57 s (35 and 66 MB of output, gated element by element in float64 on the CPU); every other case is below 0.2 s.
"""
import ctypes
import math

import pytest
import torch

import pfk_ctypes
from op_gate import Rows, flat_out, gates, gates_b16, guarded, record, same_bits, tail_kept
from op_refs import VOLUMES_B16, VOLUMES_F32, volume_case

pytestmark = pytest.mark.gpu
F32, B16 = torch.float32, torch.bfloat16
TILE = {0: (64, 64), 4: (64, 64), 10: (64, 64), 11: (64, 128)}


def f32_schedule(B, N1, N2, D, cfg=-1):
    """(cfg, tiles_m, tiles_n, supertile) of pfk_corr_volume_f32: `launch()` without a workspace and with batches = B, `launch_cfg`"""
    steps = math.ceil(D / 32)
    if cfg < 0:
        blocks64 = math.ceil(N1 / 64) * math.ceil(N2 / 64)
        cfg = 11 if N2 >= 2048 and N1 >= 2048 else 10 if blocks64 >= 768 else 0 if steps < 16 and blocks64 < 256 else 4
    bm, bn = TILE[cfg]
    tm, tn = math.ceil(N1 / bm), math.ceil(N2 / bn)
    return cfg, tm, tn, tm >= 32 and tn >= 32


def b16_path(B, N1, N2, D):
    """(tiles_m, tiles_n, supertile, 16-byte stores, K chunks, channels of the last chunk) of pfk_corr_volume_bf16"""
    tm, tn = math.ceil(N1 / 128), math.ceil(N2 / 128)
    return tm, tn, tm >= 32 and tn >= 32, N2 % 8 == 0, math.ceil(D / 64), D - (math.ceil(D / 64) - 1) * 64


def test_cases_reach_what_they_claim():
    assert f32_schedule(2, 117, 130, 64) == (0, 2, 3, False) and (117 * 130) % 4 != 0 and 130 % 4 != 0
    assert f32_schedule(2, 132, 120, 128) == (0, 3, 2, False) and 120 % 4 == 0 and (132 * 120) % 4 == 0
    assert f32_schedule(1, 2050, 2114, 32, 10) == (10, 33, 34, True) and 33 % 16 != 0 and 34 % 16 != 0
    assert f32_schedule(2, 2050, 4000, 32) == (11, 33, 32, True)
    assert f32_schedule(2, 150, 140, 36) == (0, 3, 3, False)
    assert b16_path(2, 130, 117, 40) == (2, 1, False, False, 1, 40)
    assert b16_path(2, 132, 132, 64) == (2, 2, False, False, 1, 64) and 132 % 8 == 4
    assert b16_path(1, 257, 264, 72) == (3, 3, False, True, 2, 8)
    assert b16_path(1, 40, 9, 8) == (1, 1, False, False, 1, 8)
    assert b16_path(1, 4100, 4230, 8) == (33, 34, True, False, 1, 8)
    assert b16_path(2, 70, 133, 40) == (1, 2, False, False, 1, 40)


def check_volume(what, case, dtype, launch):
    """gates, guards and the second run on `launch(out)` with `out` a [B, N1, N2] view at the head of a sentinel-filled buffer"""
    B, N1, N2, D = case
    c = volume_case(*case, dtype)
    flats = []
    for _ in range(2):
        flat, out = flat_out((B, N1, N2), "cuda", dtype)
        launch(out)
        torch.cuda.synchronize()
        assert tail_kept(flat), f"{what}: memory behind the volume was written"
        flats.append(flat)
    assert same_bits(flats[0], flats[1]), f"{what}: a second run gives other bits"
    got = flats[0][:B * N1 * N2].view(B, N1, N2)
    if dtype == B16:
        return gates_b16(what, got, None, c["ref"], c["mag"], c["K"])
    return gates(what, got, c["ref"], c["mag"], c["K"])


def forced(cfg, fn):
    torch.ops.pfk.debug_set_tile(cfg)
    try:
        fn()
    finally:
        torch.ops.pfk.debug_set_tile(-1)


@pytest.mark.parametrize("cfg", [0, 4, 10, 11, -1], ids=lambda c: "heuristic" if c < 0 else f"cfg{c}")
@pytest.mark.parametrize("case", VOLUMES_F32[:2], ids=str)
def test_volume_f32_small(gpu, case, cfg):
    c = volume_case(*case, F32)
    a, b = guarded(c["a"], gpu), guarded(c["b"], gpu)
    result = check_volume(f"fp32 {case} cfg {cfg}", case, F32, lambda out: forced(cfg, lambda: torch.ops.pfk.corr_volume(a, b, c["scale"], out)))
    record("test_volume_f32_small", [result])


@pytest.mark.parametrize("case,cfg", [(VOLUMES_F32[2], 10), (VOLUMES_F32[3], -1)], ids=["1x2050x2114x32-cfg10", "2x2050x4000x32-heuristic"])
def test_volume_f32_supertiles(gpu, case, cfg):
    assert f32_schedule(*case, cfg)[3], "the case does not reach the supertile walk"
    c = volume_case(*case, F32)
    a, b = guarded(c["a"], gpu), guarded(c["b"], gpu)
    result = check_volume(f"fp32 {case} cfg {cfg}", case, F32, lambda out: forced(cfg, lambda: torch.ops.pfk.corr_volume(a, b, c["scale"], out)))
    record("test_volume_f32_supertiles", [result])


def c_abi(name, f1, ld1, f2, ld2, out, case, scale):
    B, N1, N2, D = case
    fn = getattr(pfk_ctypes.lib(), name)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_void_p]
    status = fn(f1.data_ptr(), ld1, f2.data_ptr(), ld2, out.data_ptr(), B, N1, N2, D, scale, None)     # the null stream: torch's default
    assert status == pfk_ctypes.PFK_OK, f"{name}: status {status}"


def test_volume_f32_padded_rows(gpu):
    """the C ABI with ld > D: f1's pad columns hold NaN; f2's hold zeros — they are read as packed weight rows (module docstring)"""
    case = VOLUMES_F32[4]
    B, N1, N2, D = case
    ld1, ld2 = 44, 64
    c = volume_case(*case, F32)
    f1 = Rows(B * N1, D, gpu, values=c["a"].reshape(B * N1, D), pad=ld1 - D, nan_tail=True)
    f2 = guarded(torch.nn.functional.pad(c["b"], (0, ld2 - D)), gpu)
    torch.cuda.synchronize()
    result = check_volume(f"fp32 {case} ld {ld1}/{ld2}", case, F32,
                          lambda out: c_abi("pfk_corr_volume_f32", f1.rows, ld1, f2, ld2, out, case, c["scale"]))
    record("test_volume_f32_padded_rows", [result])


@pytest.mark.parametrize("case", VOLUMES_B16[:5], ids=str)
def test_volume_b16(gpu, case):
    c = volume_case(*case, B16)
    a, b = guarded(c["a"], gpu), guarded(c["b"], gpu)
    result = check_volume(f"bf16 {case}", case, B16, lambda out: torch.ops.pfk.corr_volume_bf16(a, b, c["scale"], out))
    record("test_volume_b16", [result])


def test_volume_b16_padded_rows(gpu):
    case = VOLUMES_B16[5]
    B, N1, N2, D = case
    ld1, ld2 = 48, 56
    c = volume_case(*case, B16)
    f1 = Rows(B * N1, D, gpu, values=c["a"].reshape(B * N1, D), pad=ld1 - D, dtype=B16, nan_tail=True)
    f2 = Rows(B * N2, D, gpu, values=c["b"].reshape(B * N2, D), pad=ld2 - D, dtype=B16, nan_tail=True)
    torch.cuda.synchronize()
    result = check_volume(f"bf16 {case} ld {ld1}/{ld2}", case, B16,
                          lambda out: c_abi("pfk_corr_volume_bf16", f1.rows, ld1, f2.rows, ld2, out, case, c["scale"]))
    record("test_volume_b16_padded_rows", [result])
