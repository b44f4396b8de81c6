"""Training through the upsampling seams, the parts that need no GPU: the C ABI additions (`pfk_convex_upsample_info_bwd_pm_f32` and
its workspace query: declared, exported, arguments checked before the device is touched) and the dispatch of
`accelerate(model, train_upsample=True)` on the torch stand-ins (tests/seam_model.py, tests/sea_seam_model.py)."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    try:
        import ptlflow_amd
        ptlflow_amd.load_native()
    except Exception as e:  # libs not built in this checkout
        pytest.skip(f"native libs unavailable: {e}")
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    lib.pfk_convex_upsample_info_bwd_workspace_bytes.restype = ctypes.c_longlong
    lib.pfk_convex_upsample_info_bwd_workspace_bytes.argtypes = [ctypes.c_int] * 4
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.pfk_convex_upsample_info_bwd_pm_f32.restype = ctypes.c_int
    lib.pfk_convex_upsample_info_bwd_pm_f32.argtypes = [P, I, P, I, I, P, I, P, P, P, I, P, I, P, I, P, L, I, I, I, P]
    return lib


def test_symbols_declared_and_exported(lib):
    src = open(os.path.join(ROOT, "include", "pfk.h")).read()
    assert "long long pfk_convex_upsample_info_bwd_workspace_bytes(" in src and hasattr(lib, "pfk_convex_upsample_info_bwd_workspace_bytes")
    assert "int pfk_convex_upsample_info_bwd_pm_f32(" in src and hasattr(lib, "pfk_convex_upsample_info_bwd_pm_f32")
    assert "#define PFK_ABI_VERSION 7" in src and lib.pfk_abi_version() == 7
    assert hasattr(torch.ops.pfk, "convex_upsample_info_bwd")


@pytest.mark.parametrize("B,H,W,n", [(1, 1, 1, 0), (2, 9, 13, 4), (8, 55, 128, 8)])
def test_workspace_bytes(lib, B, H, W, n):
    assert lib.pfk_convex_upsample_info_bwd_workspace_bytes(B, H, W, n) == B * H * W * 9 * (2 + n) * 4


def test_argument_checks(lib):
    """-1 (PFK_ERR_BAD_ARG) before anything touches the device: each NULL pointer in turn, n_info = 9, short rows, a short workspace"""
    f = lib.pfk_convex_upsample_info_bwd_pm_f32
    B, H, W, n = 1, 4, 4, 4
    need = lib.pfk_convex_upsample_info_bwd_workspace_bytes(B, H, W, n)
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: every call below fails its checks
    ptr_args = (0, 2, 5, 7, 9, 11, 13, 15)            # flow, info, mask, grad_flow_up, grad_mask, grad_flow_pm, grad_info_pm, workspace

    def call(**over):
        a = [ptr, 2, ptr, n, n, ptr, 576, ptr, ptr, ptr, 576, ptr, 2, ptr, n, ptr, need, B, H, W, None]
        for k, v in over.items():
            a[int(k[1:])] = v
        return f(*a)

    for i in ptr_args:
        assert call(**{f"a{i}": None}) == -1, f"argument {i} = NULL"
    assert call(a4=9) == -1 and call(a4=-1) == -1                       # n_info
    assert call(a1=1) == -1 and call(a3=3) == -1 and call(a6=575) == -1 and call(a10=575) == -1       # flow_ld, info_ld, mask_ld, grad_mask_ld
    assert call(a12=1) == -1 and call(a14=3) == -1                      # grad_flow_ld, grad_info_ld
    assert call(a16=need - 1) == -1                                     # workspace_bytes
    assert call(a17=0) == -1 and call(a18=0) == -1 and call(a19=0) == -1
    assert call(a6=578) == -2 and call(a10=578) == -2                   # PFK_ERR_ALIGNMENT: row strides that are no multiple of 4


class _NoSeams(torch.nn.Module):
    def forward(self, x):
        return x


def test_needs_a_seam(lib):
    from ptlflow_amd import patch
    model = _NoSeams()
    with pytest.raises(ValueError, match="train_upsample"):
        patch.accelerate(model, train_upsample=True)
    assert not model.__dict__.get("upsample_flow") and not model.__dict__.get("upsample_data")


def test_sea_raft_needs_the_fp32_seams(lib):
    from ptlflow_amd import patch
    from sea_seam_model import SeaRaftLoop
    model = SeaRaftLoop(iters=1)
    ub = model.update_block
    for value in ("bf16", False):
        with pytest.raises(ValueError, match="train_upsample=True needs sea_raft_update=True or 'fp32'"):
            patch.accelerate(model, sea_raft_update=value, train_upsample=True)
        assert model.update_block is ub and "upsample_data" not in model.__dict__, "a refused call must leave the model alone"
    patch.accelerate(model, sea_raft_update=True, train_upsample=True)
    try:
        seam = model.__dict__["upsample_data"]
        assert seam.train_upsample is True and seam.train_calls == 0
        patch.accelerate(model, sea_raft_update=True)                   # a second call switches the installed seam
        assert model.__dict__["upsample_data"] is seam and seam.train_upsample is False
    finally:
        patch.restore(model)


def test_cpu_gradient_calls_take_the_original(lib):
    """CPU tensors with a gradient graph on accelerated models: the model's own methods, bit for bit, and `train_calls` stays 0"""
    from ptlflow_amd import patch
    from seam_model import SeamRAFT, convex_upsample_torch
    from sea_seam_model import SeaRaftLoop, load_seeded, upsample_data_torch
    g = torch.Generator().manual_seed(11)
    flow = (torch.randn(1, 2, 3, 5, generator=g) * 3).requires_grad_(True)
    info = torch.randn(1, 4, 3, 5, generator=g).requires_grad_(True)
    mask = torch.randn(1, 576, 3, 5, generator=g).requires_grad_(True)

    raft = SeamRAFT(iters=1)
    patch.accelerate(raft, train_upsample=True)
    try:
        seam = raft.__dict__["upsample_flow"]
        assert seam.train_upsample is True
        out = raft.upsample_flow(flow, mask)
        assert out.requires_grad and torch.equal(out, convex_upsample_torch(flow, mask))
        assert seam.train_calls == 0 and seam.calls == 0
    finally:
        patch.restore(raft)
    assert not hasattr(raft.upsample_flow, "train_calls")

    sea = load_seeded(SeaRaftLoop(iters=1), 3)
    patch.accelerate(sea, sea_raft_update=True, sea_raft_train=True, train_upsample=True)
    try:
        seam = sea.__dict__["upsample_data"]
        got = sea.upsample_data(flow, info, mask)
        want = upsample_data_torch(flow, info, mask)
        assert all(a.requires_grad and torch.equal(a, b) for a, b in zip(got, want))
        assert seam.train_calls == 0 and seam.calls == 0
    finally:
        patch.restore(sea)
    assert "upsample_data" not in sea.__dict__ and not hasattr(sea.upsample_data, "train_calls")
