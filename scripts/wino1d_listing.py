#!/usr/bin/env python3
"""Static figures of the 1-D Winograd kernels from a gfx950 assembly listing of ptlflow_amd/csrc/pfk_wino.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Iptlflow_amd/csrc --cuda-device-only -S ptlflow_amd/csrc/pfk_wino.hip -o wino.s
    python scripts/wino1d_listing.py wino.s

Per instantiation of conv_gemm_wino1d_f32_kernel<VERT, EPI>: instructions in front of the first v_mfma (prologue) and behind the last
one (epilogue), the epilogue's integer multiplies, branches, s_waitcnt, vector-memory loads / stores and LDS writes by kind, and the
resource figures of the kernel descriptor (VGPRs + AGPRs, SGPRs, scratch, LDS)."""
import re
import sys

EPI = {0: "LINEAR", 1: "GRU_ZR", 2: "GRU_Q"}


def main(path):
    txt = open(path).read()
    for m in re.finditer(r"^(_ZN\S*conv_gemm_wino1d_f32_kernelILb([01])ELi(\d)E\S*):[^\n]*\n(.*?)\n\s*s_endpgm", txt, re.S | re.M):
        name, vert, epi, body = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
        ins = [ln.strip().split()[0] for ln in body.split("\n")
               if ln.startswith("\t") and not ln.strip().startswith((".", ";")) and ln.strip()]
        mf = [i for i, op in enumerate(ins) if op.startswith("v_mfma")]
        pro, epl = ins[:mf[0]], ins[mf[-1] + 1:]
        c = lambda pat, seq=epl: sum(1 for op in seq if re.match(pat, op))   # noqa: E731
        meta = txt[txt.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        g = lambda key: re.search(r"\.amdhsa_" + key + r"\s+(\S+)", meta).group(1)   # noqa: E731
        print(f"{'5x1' if vert else '1x5'} {EPI[epi]:7s} prologue {len(pro):4d} epilogue {len(epl):4d} | epilogue: int mul {c(r'v_mul_(lo|hi)_|v_mad_[ui](32|64)|s_mul_'):3d} "
              f"branches {c(r's_cbranch'):3d} s_waitcnt {c(r's_waitcnt'):3d} loads {c(r'(buffer|global)_load'):3d} stores {c(r'(buffer|global)_store'):3d} "
              f"ds_write_b32 {c(r'ds_write_b32'):3d} ds_write2_b32 {c(r'ds_write2'):3d} v_rcp_iflag/cvt (division) {c(r'v_rcp_iflag|v_cvt_f32_u32|v_cvt_u32_f32'):3d} | "
              f"vgpr+agpr {g('next_free_vgpr')} (accum offset {g('accum_offset')}) sgpr {g('next_free_sgpr')} "
              f"scratch {g('private_segment_fixed_size')} LDS {g('group_segment_fixed_size')}")


if __name__ == "__main__":
    main(sys.argv[1])
