"""`accelerate(model, multiscale_train=True)` without a GPU: the option's argument checks, what it switches and what
`restore` undoes, and the two new entry points in the header and in the library."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

import ms_train_model
from ms_loop_model import MsLoopModel
from ptlflow_amd import patch
from ptlflow_amd.update import PfkUpdateBlock

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("pfk_convex_upsample2_bwd_f32", "pfk_convex_upsample2_bwd_workspace_bytes", "pfk_corr_lookup_coords_bwd_f32")


def test_bf16_is_refused():
    model = MsLoopModel("ms_raft", (1, 1, 1))
    with pytest.raises(ValueError, match="multiscale_train"):
        patch.accelerate(model, multiscale_train=True, train_precision="bf16")
    assert not isinstance(model.update_block, PfkUpdateBlock) and "upsample_flow" not in model.__dict__      # nothing was installed
    patch.accelerate(model, multiscale_train=False, train_precision="bf16")                                    # off: no objection
    patch.restore(model)


def test_default_is_off():
    assert inspect.signature(patch.accelerate).parameters["multiscale_train"].default is False


@pytest.mark.parametrize("style", ["ms_raft", "ccmr"])
def test_option_switches_and_restores(style):
    model = ms_train_model.MsTrainModel(style, (1, 1, 1))
    block = model.update_block
    patch.accelerate(model, multiscale_train=True)
    seam, state = model.__dict__["upsample_flow"], model.__dict__[patch._LAYOUT_HOOKS]
    assert isinstance(model.update_block, PfkUpdateBlock) and model.update_block.multiscale_train
    assert seam.multiscale_train and not seam.multiscale and state["coords_grad"] is True
    assert patch._COORDS_GRAD.get() is False            # published for the duration of a forward only
    patch.accelerate(model, multiscale_train=False)      # a second call switches it
    assert not model.update_block.multiscale_train and not seam.multiscale_train and state["coords_grad"] is False
    assert model.__dict__["upsample_flow"] is seam
    patch.accelerate(model, multiscale_train=True, multiscale_upsample=True)      # independent of the eval option
    assert seam.multiscale_train and seam.multiscale
    patch.restore(model)
    assert model.update_block is block and "upsample_flow" not in model.__dict__ and patch._LAYOUT_HOOKS not in model.__dict__
    import ms_loop_model
    assert not hasattr(ms_loop_model, patch._ORIG)


def test_cpu_calls_keep_the_models_method():
    """the seam serves CUDA tensors only: a CPU call with a gradient graph is the model's own method's, probe not run"""
    model = ms_train_model.MsTrainModel("ms_raft", (1, 1, 1)).train()
    patch.accelerate(model, multiscale_train=True)
    seam = model.__dict__["upsample_flow"]
    flow, mask = torch.randn(1, 2, 3, 4), torch.randn(1, 36, 3, 4, requires_grad=True)
    out = model.upsample_flow(flow, mask, scale=2)
    assert out.requires_grad and seam.train_calls == 0 and seam.ok2 is None
    patch.restore(model)


def test_new_symbols_are_declared_and_exported():
    import ptlflow_amd
    header = (ROOT / "include" / "pfk.h").read_text()
    lib = ctypes.CDLL(str(Path(ptlflow_amd.__file__).resolve().parent / "libpfk.so"))
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/pfk.h"
        assert hasattr(lib, name), f"{name} is not exported by libpfk.so"
    assert "pfk_lookup_coords_bwd_desc" in header
    assert re.search(r"#define\s+PFK_ABI_VERSION\s+7\b", header), "additions only: the ABI version stays 7"
    lib.pfk_convex_upsample2_bwd_workspace_bytes.restype = ctypes.c_longlong
    assert lib.pfk_convex_upsample2_bwd_workspace_bytes(2, 9, 13) == 2 * 9 * 13 * 18 * 4
    assert lib.pfk_convex_upsample2_bwd_workspace_bytes(0, 9, 13) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-logic test on made-up addresses: with a device a case that were wrongly accepted would launch on them")
def test_entry_points_refuse_bad_arguments():
    """host-side checks only, and only without a GPU (tests/test_capi_status_table.py's rule): every case must be refused; one that
    were accepted answers PFK_ERR_LAUNCH here and returns"""
    import ptlflow_amd
    lib = ctypes.CDLL(str(Path(ptlflow_amd.__file__).resolve().parent / "libpfk.so"))
    BAD_ARG = -1
    f = lib.pfk_convex_upsample2_bwd_f32
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    p = 4096        # a made-up, aligned address: only refused calls are made
    need = 2 * 3 * 4 * 18 * 4
    ok = [p, 0, p, 36, p, p, 36, p, 0, p, need, 2, 3, 4, None]
    for at, value in ((0, None), (2, None), (4, None), (5, None), (7, None), (9, None), (3, 35), (6, 35), (1, 1), (1, -2), (8, 1), (8, -2),
                      (10, need - 1), (11, 0), (12, 0), (13, -1)):
        args = list(ok)
        args[at] = value
        assert f(*args) == BAD_ARG, f"argument {at} = {value} was not refused"
    assert lib.pfk_corr_lookup_coords_bwd_f32(None, None) == BAD_ARG
