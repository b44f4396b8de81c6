"""The multi-scale GroupNorm encoders on the kernels (K15), the parts that need no GPU: the torch stand-in tests/msenc_model.py against
the fixtures recorded from the reference's classes (tests/golden/ms_encoders*.pt, scripts/make_golden_ms_encoders.py), the describer
(`ms_encoder.describe_multiscale_encoder`) on what it must accept and refuse, `accelerate(model, multiscale_encoders=True)` on a CPU
model (the wrapper is installed and every call falls back to the reference module), and the C ABI of the new entries (declared,
exported, ABI version unchanged, arguments validated before the device is touched)."""
import copy
import ctypes
import inspect
import os
import re

import pytest
import torch

import ptlflow_amd
from msenc_model import ENCODERS, SEEDS, MsModel, make, randomize, recipe_state_dict, register
from msenc_refs import load_golden, load_golden_levels
from oracle import ref_loader
from ptlflow_amd import ms_encoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = sorted(ENCODERS)
NEW = ("pfk_groupnorm_workspace_bytes", "pfk_groupnorm_stats_f32", "pfk_affine_apply_f32", "pfk_resize_bilinear_pm_f32")
BAD_ARG, ALIGNMENT, UNSUPPORTED = -1, -2, -3
LL, VP, I, FL = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_float


@pytest.fixture(scope="module")
def golden():
    return load_golden()


# ---------------------------------------------------------------------------------------------------------------------
# the stand-in is the reference's module, the recipe is the one the fixture was recorded with
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_standin_reproduces_the_fixture(golden, key):
    rec = golden["encoders"][key]
    m = make(key).double().eval()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == rec["shapes"], sorted(set(shapes.items()) ^ set(rec["shapes"].items()))
    sd = recipe_state_dict(shapes, rec["seed"], torch.float64)
    for name, (s, a) in rec["checksums"].items():
        got = (float(sd[name].sum()), float(sd[name].abs().sum()))
        assert abs(got[0] - s) <= 1e-12 * max(1.0, a) and abs(got[1] - a) <= 1e-12 * max(1.0, a), \
            f"{key}: the recipe's {name} has (sum, |sum|) {got}, the fixture was recorded with {(s, a)}"
    m.load_state_dict(sd, strict=True)
    x = golden["input"]
    with torch.no_grad():
        outs = m([x[0:1], x[1:2]]) if m.split_pairs else m(x[0:1])
    levels = load_golden_levels(key)
    assert len(outs) == len(levels) == len(rec["levels"])
    for i, (o, want) in enumerate(zip(outs, levels)):
        if m.split_pairs:
            assert isinstance(o, tuple) and len(o) == 2
            o = torch.cat(o, 0)
        assert tuple(o.shape) == tuple(want.shape) == tuple(rec["levels"][i])
        err, scale = float((o - want.double()).abs().max()), float(want.abs().max())
        print(f"{key} level {i}: max err {err:.2e} of scale {scale:.2e}")
        assert err <= 1e-6 * scale, f"{key} level {i}: {err:.3e} vs scale {scale:.3e}"
    assert SEEDS[key] == rec["seed"]


def test_describer_accepts_the_reference_classes_and_consumes_their_state_dict():
    if not ref_loader.reference_available():
        pytest.skip("no reference tree on this machine")
    for key, (_cls, _kw, (mod, name, kw)) in ENCODERS.items():
        ref = getattr(ref_loader.ref_module(mod), name)(**kw).eval()
        assert ms_encoder.served(ref), key
        desc = ms_encoder.describe_multiscale_encoder(ref)
        assert desc is not None, key
        assert desc["names"] == set(ref.state_dict()), key
        mine = ms_encoder.describe_multiscale_encoder(make(key))
        assert {k: mine[k] for k in ("blocks", "ups", "norms", "out_dim", "names")} == \
            {k: desc[k] for k in ("blocks", "ups", "norms", "out_dim", "names")}, key
        assert ms_encoder._MS_CLASSES[(mod, name)] == ENCODERS[key][0].split_pairs


# ---------------------------------------------------------------------------------------------------------------------
# the describer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_describer_reads_the_skeleton(key):
    m = make(key)
    desc = ms_encoder.describe_multiscale_encoder(m)
    assert desc is not None
    assert desc["names"] == set(m.state_dict())
    nup = 2 if key.startswith("ccmr_") else 3
    assert len(desc["ups"]) == nup and len(desc["blocks"]) == 8 + 2 * nup
    assert [b[:4] for b in desc["blocks"][:8]] == [("layer1.0", 64, 64, 1), ("layer1.1", 64, 64, 1), ("layer2.0", 64, 96, 2),
                                                   ("layer2.1", 96, 96, 1), ("layer3.0", 96, 128, 2), ("layer3.1", 128, 128, 1),
                                                   ("layer4.0", 128, 160, 2), ("layer4.1", 160, 160, 1)]
    for (n, name, coarse, skip, planes, after, out), want_n in zip(desc["ups"], (2, 1, 0)):
        assert n == want_n and name == f"up_layer{n}" and skip == {2: 128, 1: 96, 0: 64}[n]
        assert (after is not None) == key.startswith("ccmr")
        first = getattr(m, name)[0].conv1
        assert first.in_channels == coarse + skip and first.out_channels == planes


@pytest.mark.parametrize("key", ["ccmrp_fnet", "msraft_cnet"])
def test_describer_refuses_what_the_engine_does_not_compute(key):
    assert ms_encoder.describe_multiscale_encoder(make(key, norm_fn="instance")) is None
    assert ms_encoder.describe_multiscale_encoder(make(key, norm_fn="batch")) is None
    assert ms_encoder.describe_multiscale_encoder(make(key, group=16)) is None                 # 16 channels per group
    one = make(key)
    one.layer3[1].norm2 = torch.nn.GroupNorm(8, 128)                                             # a single norm of 16 per group
    assert ms_encoder.describe_multiscale_encoder(one) is None
    extra = make(key)
    extra.layer2[0].extra_scale = torch.nn.Parameter(torch.ones(96))                             # a parameter nobody consumes
    assert ms_encoder.describe_multiscale_encoder(extra) is None
    assert ms_encoder.describe_multiscale_encoder(make(key).bfloat16()) is None
    half = make(key)
    half.up_layer1[0].conv1.bfloat16()                                                           # one bf16 parameter
    assert ms_encoder.describe_multiscale_encoder(half) is None
    eps = make(key)
    eps.norm1.eps = 1e-6
    assert ms_encoder.describe_multiscale_encoder(eps) is None
    plain = make(key)
    plain.up_layer2[1].norm1 = torch.nn.GroupNorm(plain.up_layer2[1].norm1.num_groups, plain.up_layer2[1].norm1.num_channels, affine=False)
    assert ms_encoder.describe_multiscale_encoder(plain) is None
    for attr, val in (("stride", (1, 1)), ("padding", (0, 0)), ("groups", 2), ("dilation", (2, 2))):
        odd = make(key)
        setattr(odd.layer2[0].conv1, attr, val)
        assert ms_encoder.describe_multiscale_encoder(odd) is None, attr
    k5 = make(key)
    k5.layer1[1].conv2 = torch.nn.Conv2d(64, 64, 5, padding=2)
    assert ms_encoder.describe_multiscale_encoder(k5) is None
    assert ms_encoder.describe_multiscale_encoder(make(key)) is not None


def test_describer_ties_the_ccmr_model_type_to_the_levels():
    assert ms_encoder.describe_multiscale_encoder(make("ccmr_fnet", model_type="CCMR+")) is None       # CCMR+ without up_layer0
    assert ms_encoder.describe_multiscale_encoder(make("ccmrp_fnet", model_type="CCMR")) is None       # a level the forward never runs
    assert ms_encoder.describe_multiscale_encoder(make("ccmrp_cnet", model_type="other")) is None


# ---------------------------------------------------------------------------------------------------------------------
# the seam, on the CPU: installed, and every call falls back
# ---------------------------------------------------------------------------------------------------------------------
def test_accelerate_installs_the_wrappers_and_a_cpu_call_falls_back():
    from ptlflow_amd import patch
    assert inspect.signature(patch.accelerate).parameters["multiscale_encoders"].default is False
    assert "multiscale_encoders" in patch.accelerate.__doc__
    assert patch.register_multiscale_encoder is ms_encoder.register_multiscale_encoder
    register()
    model = MsModel("ccmrp").eval()
    keys = list(model.state_dict())
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(1, 3, 32, 48, generator=g), torch.randn(1, 3, 32, 48, generator=g)
    with torch.no_grad():
        want_f, want_c = copy.deepcopy(model)(a, b)
    fnet, cnet = model.fnet, model.cnet
    patch.accelerate(model)                                             # option off: nothing installed
    assert model.fnet is fnet and model.cnet is cnet
    patch.accelerate(model, multiscale_encoders=True)
    assert isinstance(model.fnet, ms_encoder.PfkMultiScaleEncoder) and isinstance(model.cnet, ms_encoder.PfkMultiScaleEncoder)
    assert model.fnet.split_pairs and not model.cnet.split_pairs
    assert list(model.state_dict()) == keys
    with torch.no_grad():
        got_f, got_c = model(a, b)
    assert (model.fnet.engine_calls, model.fnet.fallback_calls, model.cnet.engine_calls, model.cnet.fallback_calls) == (0, 1, 0, 1)
    assert len(got_f) == len(want_f) == 4 and len(got_c) == len(want_c) == 4
    for g_pair, w_pair in zip(got_f, want_f):
        assert isinstance(g_pair, tuple) and all(torch.equal(x, y) for x, y in zip(g_pair, w_pair))
    assert all(torch.equal(x, y) for x, y in zip(got_c, want_c))
    patch.accelerate(model, multiscale_encoders=True)                   # a second call wraps nothing twice
    assert model.fnet._ref[0] is fnet
    patch.accelerate(model)                                             # another value switches the path
    assert model.fnet is fnet and model.cnet is cnet
    patch.accelerate(model, multiscale_encoders=True)
    patch.restore(model)
    assert model.fnet is fnet and model.cnet is cnet and list(model.state_dict()) == keys


def test_accelerate_leaves_unserved_and_undescribed_encoders_alone():
    from ptlflow_amd import patch
    register()
    model = MsModel("msraft").eval()
    model.fnet = randomize(make("msraft_fnet", norm_fn="instance"), 3)          # served class, refused description
    cnet = model.cnet

    class Other(type(cnet)):                                                     # described, but not a served class
        pass

    model.cnet = randomize(Other(**ENCODERS["msraft_cnet"][1]), 4)
    fnet, cnet = model.fnet, model.cnet
    patch.accelerate(model, multiscale_encoders=True)
    assert model.fnet is fnet and model.cnet is cnet
    patch.restore(model)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not ptlflow_amd.LIBPFK_PATH.exists():
        from ptlflow_amd import _build
        _build.build_all()
    lib = ctypes.CDLL(str(ptlflow_amd.LIBPFK_PATH))
    sig = {
        "pfk_groupnorm_workspace_bytes": (LL, [I, I, I]),
        # (x, ld, B, HW, C, group_size, gamma, beta, eps, scale, shift, ws, ws_bytes, stream)
        "pfk_groupnorm_stats_f32": (I, [VP, I, I, I, I, I, VP, VP, FL, VP, VP, VP, LL, VP]),
        # (x, x_ld, scale, shift, residual, residual_ld, out, out_ld, B, HW, C, relu, relu_after, stream)
        "pfk_affine_apply_f32": (I, [VP, I, VP, VP, VP, I, VP, I, I, I, I, I, I, VP]),
        # (in, in_ld, out, out_ld, B, Hi, Wi, Ho, Wo, C, stream)
        "pfk_resize_bilinear_pm_f32": (I, [VP, I, VP, I, I, I, I, I, I, I, VP]),
    }
    for n, (res, args) in sig.items():
        getattr(lib, n).restype, getattr(lib, n).argtypes = res, args
    return lib


def test_header_declares_and_library_exports_the_new_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfk.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/pfk.h does not declare {n}"
        assert hasattr(lib, n), f"libpfk.so does not export {n}"
    assert lib.pfk_abi_version() == 7 and "#define PFK_ABI_VERSION 7" in src
    ptlflow_amd.load_native()
    for n in ("groupnorm_workspace_bytes", "groupnorm_stats", "affine_apply", "resize_bilinear_pm"):
        assert hasattr(torch.ops.pfk, n), n
    from ptlflow_amd import _build
    assert "pfk_msenc.hip" in [s for s, _ in _build.HIP_SOURCES]


# every call below is refused before a launch: the pointers are never dereferenced
A, Bp, Cp, Ep, Fp, WS = 0x100000, 0x200000, 0x300000, 0x500000, 0x600000, 0x700000
BIG = 1 << 40


def test_groupnorm_stats_validates_without_a_gpu(lib):
    def f(x=A, ld=64, B=2, HW=63, C=64, gs=8, gamma=Ep, beta=Ep, eps=1e-5, scale=Bp, shift=Cp, ws=WS, ws_bytes=BIG):
        return lib.pfk_groupnorm_stats_f32(x, ld, B, HW, C, gs, gamma, beta, eps, scale, shift, ws, ws_bytes, None)
    assert f(x=None) == BAD_ARG and f(gamma=None) == BAD_ARG and f(beta=None) == BAD_ARG and f(scale=None) == BAD_ARG
    assert f(shift=None) == BAD_ARG and f(ws=None) == BAD_ARG
    assert f(B=0) == BAD_ARG and f(HW=0) == BAD_ARG and f(C=0) == BAD_ARG and f(gs=0) == BAD_ARG and f(ld=60) == BAD_ARG
    assert f(eps=-1.0) == BAD_ARG
    assert f(gs=16) == UNSUPPORTED and f(gs=4) == UNSUPPORTED and f(C=68, ld=68) == UNSUPPORTED and f(C=1032, ld=1032) == UNSUPPORTED
    assert f(ld=66) == ALIGNMENT and f(x=A + 4) == ALIGNMENT and f(ws=WS + 4) == ALIGNMENT and f(gamma=Ep + 2) == ALIGNMENT
    need = lib.pfk_groupnorm_workspace_bytes(2, 600, 64)
    assert need == 2 * 2 * 3 * 8 * 8          # sums and sums of squares, per image, 256-pixel chunk and group, in double
    assert f(HW=600, ws_bytes=need - 1) == BAD_ARG
    assert lib.pfk_groupnorm_workspace_bytes(0, 63, 64) == BAD_ARG and lib.pfk_groupnorm_workspace_bytes(1, 63, 68) == UNSUPPORTED


def test_affine_apply_and_resize_validate_without_a_gpu(lib):
    def f(x=A, x_ld=160, scale=Ep, shift=Fp, res=Cp, res_ld=160, out=Bp, out_ld=160, B=2, HW=35, C=160):
        return lib.pfk_affine_apply_f32(x, x_ld, scale, shift, res, res_ld, out, out_ld, B, HW, C, 1, 1, None)
    assert f(x=None) == BAD_ARG and f(scale=None) == BAD_ARG and f(shift=None) == BAD_ARG and f(out=None) == BAD_ARG
    assert f(B=0) == BAD_ARG and f(HW=0) == BAD_ARG and f(C=0) == BAD_ARG and f(x_ld=156) == BAD_ARG and f(out_ld=156) == BAD_ARG
    assert f(C=158) == ALIGNMENT and f(x_ld=162) == ALIGNMENT and f(out_ld=162) == ALIGNMENT and f(res_ld=162) == ALIGNMENT
    assert f(res_ld=156) == ALIGNMENT and f(x=A + 4) == ALIGNMENT and f(out=Bp + 8) == ALIGNMENT and f(scale=Ep + 4) == ALIGNMENT
    assert f(shift=Fp + 4) == ALIGNMENT and f(res=Cp + 4) == ALIGNMENT

    def r(inp=A, in_ld=96, out=Bp, out_ld=96, B=2, Hi=7, Wi=9, Ho=13, Wo=17, C=96):
        return lib.pfk_resize_bilinear_pm_f32(inp, in_ld, out, out_ld, B, Hi, Wi, Ho, Wo, C, None)
    assert r(inp=None) == BAD_ARG and r(out=None) == BAD_ARG and r(B=0) == BAD_ARG and r(Hi=0) == BAD_ARG and r(Wo=0) == BAD_ARG
    assert r(C=0) == BAD_ARG and r(in_ld=92) == BAD_ARG and r(out_ld=92) == BAD_ARG
    assert r(C=94) == ALIGNMENT and r(in_ld=98) == ALIGNMENT and r(out_ld=98) == ALIGNMENT and r(inp=A + 4) == ALIGNMENT
    assert r(out=Bp + 8) == ALIGNMENT
    assert r(Ho=6) == UNSUPPORTED and r(Wo=8) == UNSUPPORTED and r(Ho=6, Wo=8) == UNSUPPORTED          # downsizing
    assert r(Hi=40000, Ho=40000) == UNSUPPORTED                                                             # 2 * Ho * Hi >= 2^31
