"""The three direct-convolution paths an engine can be on, and the precision names that select them.

    fp32 tiles   `pfk_conv2d_f32`: fp32 rows, fp32 weights in 32-channel K chunks.  The only path with the Winograd twins (F(2x2,3x3),
                 F(4,5)), the grouped launch, `cout_active` / `cout_split`, the fused instance norms and the fp32 fused mask-upsample.
    split bf16   `pfk_conv2d_bf16s`: fp32 rows, the weight cut into 1..3 bf16 planes (same op, the weight's dtype picks the kernel).
    bf16 rows    K8b, `pfk_conv2d_b16`: bf16 activation rows between an engine's own kernels, one bf16 weight in 64-channel K chunks.

`resolve` is the only place a user's precision string becomes a path; an engine holds the result as `self.path` and asks it what it
needs to know (`fp32_tiles`, `b16`, `planes`, `dtype`, `quantum`, ...) instead of re-deriving it.  `ConvPath.conv` is the one launcher
of `torch.ops.pfk.conv2d` / `conv2d_b16`: each op's positional order written once, the callers name the arguments (but one, see there).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from .packing import pack_conv_operand, round_up

EPI_LINEAR, EPI_GRU_ZR, EPI_GRU_Q, EPI_LINEAR_GELU = 0, 1, 2, 3        # enum pfk_epilogue (include/pfk.h)


@dataclass(frozen=True)
class ConvPath:
    name: str
    planes: int               # bf16 planes per weight operand of the split kernel; 0 on the other two paths
    dtype: torch.dtype        # activation rows between an engine's kernels
    quantum: int              # channels per 16-byte row unit: what buffer widths and source channel counts are rounded up to
    element_bytes: float      # of an activation / weight element, for the algorithmic byte counts
    kchunk: int               # channels per K chunk of the packed weight

    @property
    def b16(self) -> bool:
        """bf16 rows: K8b"""
        return self.dtype is torch.bfloat16

    @property
    def fp32_tiles(self) -> bool:
        """the fp32 tile kernels (module docstring: what only they have)"""
        return self.planes == 0 and not self.b16

    def segment(self, c: int) -> List[Tuple[int, int, int]]:
        """the segment list of a convolution with ONE source of `c` channels in a buffer of this path's quantum"""
        return [(0, c, round_up(c, self.quantum))]

    def pack(self, weight: torch.Tensor, segments: Sequence[Tuple[int, int, int]]) -> torch.Tensor:
        """the weight operand of this path's kernel (`packing.pack_conv_operand`)"""
        return pack_conv_operand(weight, segments, self.b16, self.planes)

    def conv(self, ops, srcs, B, H, W, kh, kw, weight, bias, cout, out, epi=EPI_LINEAR, relu=False, scale=1.0, h=None, h_b16=None,
             z=None, rh=None, workspace=None, residual=None, stride=1, relu2=False, cout_active=0, cout_split=0) -> None:
        """One direct convolution on this path through `ops` (the caller's `torch.ops.pfk`, or whatever stands in for it).  `h`: the
        fp32 recurrent state of a GRU epilogue, `h_b16` its bf16 twin.  On bf16 rows z|r reads h from the twin (r * h is rounded to
        bf16 anyway) and q updates the fp32 h and mirrors it; that kernel has no stream-K `workspace` and no `cout_active` /
        `cout_split`.  Callers name the arguments.  The one exception is `UpdateEngine._conv`, about 300 launches per forward, which
        passes them in this order: naming all of them costs 1.1 us a call more than the op called directly, positionally 0.25 us
        (scripts/launcher_call_cost.py), and the enqueue time of a forward showed it (profiles/r23_a_conv_paths.md §7);
        tests/test_conv_path.py holds the positional call to the named one."""
        if self.b16:
            ops.conv2d_b16(srcs, B, H, W, kh, kw, weight, bias, cout, epi, relu, scale, out, h if epi == EPI_GRU_Q else None,
                           h_b16 if epi != EPI_LINEAR else None, z, rh, residual, stride, relu2)
        else:
            ops.conv2d(srcs, B, H, W, kh, kw, weight, bias, cout, epi, relu, scale, out, h, z, rh, workspace, residual, stride, relu2,
                       cout_active, cout_split)


FP32 = ConvPath("fp32", 0, torch.float32, 4, 4.0, 32)
BF16_ROWS = ConvPath("bf16", 0, torch.bfloat16, 8, 2.0, 64)
_SPLIT = {n: ConvPath(f"split-bf16x{n}", n, torch.float32, 4, 4.0, 32) for n in (1, 2, 3)}

# the one definition of the precision names: `conv_precision=` takes all four, everything else ("precision=", `train_precision=`,
# `sea_raft_update=`) the two that are a precision of the reference's own (fp32 and its autocast switch)
_BY_NAME = {"fp32": FP32, "bf16": BF16_ROWS, "bf16x3": _SPLIT[2], "bf16x6": _SPLIT[3]}
CONV_PRECISIONS = sorted(_BY_NAME)
PRECISIONS = ("fp32", "bf16")


def check_precision(value, allowed, what: str = "precision", expected: Optional[str] = None):
    """`value` if it is one of `allowed`, else the ValueError every option of the package raises for a precision it does not know"""
    if value not in allowed:
        raise ValueError(f"{what} must be {expected or f'one of {allowed}'}, got {value!r}")
    return value


def resolve(conv_precision: str, external_aggregate: bool = False) -> ConvPath:
    """The path of an engine built with `conv_precision` (refuses a name that is not in `CONV_PRECISIONS`)."""
    path = _BY_NAME[check_precision(conv_precision, CONV_PRECISIONS, "conv_precision")]
    if path.b16 and external_aggregate:
        # CCMR: the second motion-feature slot is filled by the caller's torch module (an XCiT block), which reads the motion features
        # out of hx — they must stay fp32 rows.  "bf16" there is the split kernel with one plane: bf16 operands, fp32 storage.
        return _SPLIT[1]
    return path
