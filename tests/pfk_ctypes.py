"""The one ctypes mirror of include/pfk.h's convolution descriptors for the tests that call libpfk.so's C ABI directly.
`tests/test_capi_status_table.py::test_ctypes_mirror_matches_header` compares every size and offset here with the header's."""
import ctypes
import os
import re

PFK_OK, PFK_ERR_BAD_ARG, PFK_ERR_ALIGNMENT, PFK_ERR_UNSUPPORTED, PFK_ERR_LAUNCH, PFK_ERR_DISABLED = 0, -1, -2, -3, -4, -5
EPI_LINEAR, EPI_GRU_ZR, EPI_GRU_Q, EPI_LINEAR_GELU = 0, 1, 2, 3

_P, _I, _F, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


class Src(ctypes.Structure):       # pfk_conv_src
    _fields_ = [("ptr", _P), ("ld", _I), ("channels", _I)]


class Desc(ctypes.Structure):      # pfk_conv_desc
    _fields_ = [("src", Src * 3), ("num_src", _I), ("B", _I), ("H", _I), ("W", _I), ("kh", _I), ("kw", _I), ("weight", _P), ("bias", _P),
                ("cout", _I), ("epilogue", _I), ("relu", _I), ("scale", _F), ("out", _P), ("out_ld", _I), ("out_coff", _I), ("h", _P),
                ("h_ld", _I), ("aux_z", _P), ("aux_rh", _P), ("residual", _P), ("residual_ld", _I), ("stride", _I),
                ("relu_after_residual", _I), ("workspace", _P), ("workspace_bytes", _LL), ("cout_active", _I), ("cout_split", _I)]


class SrcB16(ctypes.Structure):    # pfk_conv_src_b16
    _fields_ = [("ptr", _P), ("ld", _I), ("channels", _I)]


class DescB16(ctypes.Structure):   # pfk_conv_b16_desc
    _fields_ = [("src", SrcB16 * 3), ("num_src", _I), ("B", _I), ("H", _I), ("W", _I), ("kh", _I), ("kw", _I), ("weight", _P),
                ("bias", _P), ("cout", _I), ("epilogue", _I), ("relu", _I), ("scale", _F), ("out", _P), ("out_ld", _I), ("out_coff", _I),
                ("out_bf16", _I), ("h", _P), ("h_ld", _I), ("h_b16", _P), ("h_b16_ld", _I), ("aux_z", _P), ("aux_rh", _P),
                ("residual", _P), ("residual_ld", _I), ("stride", _I), ("relu_after_residual", _I), ("residual_bf16", _I),
                ("batches", _I), ("src_batch_stride", _LL), ("weight_batch_stride", _LL), ("out_batch_stride", _LL),
                ("residual_batch_stride", _LL)]


def declared():
    """every function name include/pfk.h declares (comments stripped)"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pfk_[a-z0-9_]+)\s*\(", src)))


def rocm_clang():
    """the clang that stands next to hipcc, for the small host programs some tests compile; None where there is none"""
    import shutil
    from pathlib import Path
    from ptlflow_amd import _build
    hipcc = shutil.which(_build.HIPCC) or shutil.which("hipcc")
    cands = []
    if hipcc:
        bindir = Path(os.path.realpath(hipcc)).parent
        cands += [bindir / "amdclang", bindir / "clang", bindir.parent / "llvm" / "bin" / "clang", bindir.parent / "lib" / "llvm" / "bin" / "clang"]
    return next((str(c) for c in cands if c.exists()), None)


def lib():
    """libpfk.so through ctypes (built first where the tree has none); torch's HIP runtime is loaded before it, as the product does."""
    import ptlflow_amd
    if not ptlflow_amd.LIBPFK_PATH.exists():
        from ptlflow_amd import _build
        _build.build_all()
    import torch  # noqa: F401
    return ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
