"""The launch sequence of the update engines is held to the commit that tests/golden/engine_launch_transcript.json names.

The engines reach the library only through `self.ops` and their control flow depends on shapes alone, so the sequence can be read
on the CPU: the engines are built on `torch.device("cpu")` (as tests/test_engine_pack_bits.py builds them), `eng.ops` is replaced by
a recorder, and the public methods are driven at B=2, H=6, W=8.  The pure queries (`conv_workspace_bytes`,
`conv_workspace_fault_offset`, `*_workspace_bytes`) go through to the real library; every other op is written down and NOT executed.

A record is the op's name and its arguments as the op's schema binds them (by name, defaults filled in): a tensor (singly or in a list) as dtype, shape, strides and the engine buffer or
`w[...]` entry it is a view of with its storage offset (`tmp`: a fresh temporary; `arg:*`: a tensor of the driver), ints, bools and
None as they are, floats by `repr` (only literals reach a record: `gamma` is set to 0.5).  No tensor VALUE is recorded, so the digest
does not depend on the host's float paths.  The methods that enqueue nothing on the library leave a record of what they decided
instead: `bind` every buffer's dtype and shape, `set_attention` the operand it stored, `flow_changed` / `stage` / `stage_net` (torch
copies on the bf16 path) the views the convolutions and the lookup are pointed at.

Every case runs twice, the second time with `WINO_MIN_WORK`, `WINO_F2_MIN_PIXELS`, `WINO1D_MIN_PIXELS` and `SMALL_GRID_PIXELS` set
to 1: at 96 pixels that takes the Winograd, 1-D Winograd and large-grid side of each rule.  The gma cases run a third time at H=5,
W=6 (N=30, a multiple of neither 4 nor 8: both padding branches of `set_attention`).  The encoders are not here (`EncoderEngine`
refuses CPU tensors): their packed tables and the GPU tests hold them.

`python tests/test_engine_launch_transcript.py <commit>` records the file from the tree it runs in."""
import contextlib
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_transcript.json")
CPU = torch.device("cpu")
B, H, W = 2, 6, 8
THRESHOLDS = ("WINO_MIN_WORK", "WINO_F2_MIN_PIXELS", "WINO1D_MIN_PIXELS", "SMALL_GRID_PIXELS")
QUERIES = ("conv_workspace_bytes", "conv_workspace_fault_offset")


def is_query(name: str) -> bool:
    return name in QUERIES or name.endswith("_workspace_bytes")


class Recorder:
    """Stands in for `eng.ops`: `log` is the transcript, `args` the driver's own tensors by name."""

    def __init__(self, eng, real):
        self.eng, self.real, self.log, self.args = eng, real, [], {}

    def __getattr__(self, name):
        if is_query(name):
            return getattr(self.real, name)
        return functools.partial(self._op, name)

    def _op(self, name, *args, **kwargs):
        """the call as the op's schema binds it: every parameter by name, defaults filled in — a trailing default that is spelled out
        and one that is left out are the same launch"""
        params = getattr(self.real, name).default._schema.arguments
        assert len(args) <= len(params) and not set(kwargs) - {p.name for p in params[len(args):]}, f"{name}: arguments do not bind"
        bound = dict(zip((p.name for p in params), args), **kwargs)
        for p in params:
            if p.name not in bound:
                assert p.has_default_value(), f"{name}: no value for {p.name}"
                bound[p.name] = p.default_value
        owners = self._owners()
        self.log.append([name, {k: self._enc(v, owners) for k, v in bound.items()}])

    def _owners(self):
        """storage address -> the name of the first tensor that owns it: the driver's, then the engine's attributes and dicts by name"""
        named = [("arg:" + k, v) for k, v in self.args.items()]
        for attr in sorted(vars(self.eng)):
            v = vars(self.eng)[attr]
            if torch.is_tensor(v):
                named.append((attr, v))
            elif isinstance(v, dict):
                named += [(f"{attr}[{k!r}]", t) for k, t in sorted(v.items(), key=lambda kv: str(kv[0])) if torch.is_tensor(t)]
        owners = {}
        for name, t in named:
            if t.numel():
                owners.setdefault(t.untyped_storage().data_ptr(), name)
        return owners

    def _enc(self, v, owners):
        if torch.is_tensor(v):
            base = owners.get(v.untyped_storage().data_ptr(), "tmp") if v.numel() else "empty"
            return ["T", str(v.dtype), list(v.shape), list(v.stride()), base, v.storage_offset() if base != "tmp" else 0]
        if isinstance(v, (list, tuple)):
            return [self._enc(x, owners) for x in v]
        if isinstance(v, float):
            return ["F", repr(v)]
        assert v is None or isinstance(v, (bool, int)), f"unexpected argument {type(v)}"
        return v

    def note(self, what, tensors):
        """a record of a method that enqueues nothing: (name, dtype, shape) of what it set"""
        self.log.append(["=" + what, [[k, None if t is None else [str(t.dtype), list(t.shape), list(t.stride())]] for k, t in tensors]])


def _buffers(eng):
    out = []
    for attr in sorted(vars(eng)):
        v = vars(eng)[attr]
        if torch.is_tensor(v):
            out.append((attr, v))
        elif attr != "w" and isinstance(v, dict):
            out += [(f"{attr}[{k!r}]", t) for k, t in sorted(v.items()) if torch.is_tensor(t)]
    return out


class Driver:
    """Calls the engine's methods in the issue's order; `counts` = records each driven method left."""

    def __init__(self, eng):
        self.eng, self.counts = eng, []
        self.rec = eng.ops = Recorder(eng, eng.ops)

    def call(self, name, *args, **kwargs):
        n = len(self.rec.log)
        self.rec.log.append(["#" + name, None])
        getattr(self.eng, name)(*args, **kwargs)
        if name == "bind":
            self.rec.note("buffers", _buffers(self.eng))
        elif name == "set_attention":
            self.rec.note("attn", [("attn", self.eng.attn)])
        elif name in ("flow_changed", "stage", "stage_net"):
            self.rec.note("views", [("act", self.eng.act), ("lookup_out", self.eng.lookup_out)])
        self.counts.append((name, len(self.rec.log) - n - 1))

    def arg(self, name, *shape, dtype=torch.float32):
        t = self.rec.args[name] = torch.zeros(*shape, dtype=dtype)
        return t


def _round_up(x, m):
    return (x + m - 1) // m * m


def drive_update(eng, h, w):
    s, d = eng.spec, Driver(eng)
    M, N = B * h * w, h * w
    d.call("bind", B, h, w)
    d.call("load_state", d.arg("net", B, s.hidden, h, w), d.arg("inp", B, s.context, h, w))
    eng.flow_view.zero_()
    d.call("flow_changed")
    corr = eng.lookup_out if eng.lookup_out is not None else d.arg("corr", M, _round_up(s.corr_channels, 4))
    if s.external_aggregate:
        d.call("motion", corr)
        d.call("gru")
    else:
        if s.aggregate:
            eng.gamma = 0.5
            d.call("set_attention", d.arg("attention", B, 1, N, N))
        d.call("motion_and_gru", corr, grouped=False)
        if eng.can_group:
            d.call("motion_and_gru", corr, grouped=True, prev_mask=s.has_mask)
    c0, c1, delta = d.arg("coords0", B, 2, h, w), d.arg("coords1", B, 2, h, w), d.arg("delta", B, 2, h, w)
    d.call("heads", c0, c1, delta, want_mask=True)
    d.call("heads", c0, c1, delta, want_mask=False)
    if eng.can_fuse_mask_upsample:
        d.call("heads", c0, c1, delta, mask_conv2=False)
        d.call("mask_upsample", d.arg("flow_up", B, 2, 8 * h, 8 * w))
    if s.has_mask:
        d.call("mask_head", side_stream=True)
    return d


def drive_sea(eng, h, w):
    s, d = eng.spec, Driver(eng)
    d.call("bind", B, h, w)
    net, inp, flow = d.arg("net", B, s.hidden, h, w), d.arg("inp", B, s.context, h, w), d.arg("flow", B, 2, h, w)
    # the lookup's result as each path takes it: fp32 rows, read in place | NCHW, copied into the bf16 rows
    corr = d.arg("corr", B, s.corr_channels, h, w) if eng.lookup_out is not None else d.arg("corr", B * h * w, s.corr_channels)
    d.call("stage", net, inp, flow, corr)
    d.call("update", eng.lookup_out if eng.lookup_out is not None else corr)
    d.call("heads_conv1", True)
    d.call("flow_head_out")
    d.call("mask_logits", 1.0)
    d.call("stage_net", net)
    return d


def _update_engine(spec_name, precision, hoist=True):
    from ptlflow_amd import update as U
    from ptlflow_amd.synth import synth_update_block_params
    spec = {"basic": U.basic_spec, "small": U.small_spec, "gma": U.gma_spec, "ccmr": lambda: U.ccmr_spec(324)}[spec_name]()
    return U.UpdateEngine(synth_update_block_params(spec, 11), spec, CPU, precision, hoist_context=hoist)


def _sea_engine(precision):
    from ptlflow_amd import sea_update as S
    from ptlflow_amd.synth import synth_state_dict
    shapes = dict(S.sea_block_shapes(324, 2))
    for head, sh in S.HEAD_SHAPES.items():
        shapes.update({f"{head}.{k}": v for k, v in sh.items()})
    return S.SeaUpdateEngine(synth_state_dict(shapes, 12), S.sea_spec(324), CPU, 2, precision)


# name -> (engine factory, driver, precision, the grids it is driven at)
CASES = {}
for _p in ("fp32", "bf16", "bf16x3"):
    for _s in ("basic", "small", "gma", "ccmr"):
        CASES[f"update/{_s}/{_p}"] = (functools.partial(_update_engine, _s, _p), drive_update, _p,
                                     ((H, W), (5, 6)) if _s == "gma" else ((H, W),))
    CASES[f"update/basic-unhoisted/{_p}"] = (functools.partial(_update_engine, "basic", _p, False), drive_update, _p, ((H, W),))
for _p in ("fp32", "bf16"):
    CASES[f"sea_update/{_p}"] = (functools.partial(_sea_engine, _p), drive_sea, _p, ((H, W),))


@contextlib.contextmanager
def thresholds_at_one():
    from ptlflow_amd import update as U
    saved = {k: getattr(U, k) for k in THRESHOLDS}
    try:
        for k in THRESHOLDS:
            setattr(U, k, 1)
        yield
    finally:
        for k, v in saved.items():
            setattr(U, k, v)


@functools.lru_cache(maxsize=None)
def transcript(name):
    """(passes, counts): every pass's records under its label, and the records each driven method left"""
    make, drive, _precision, grids = CASES[name]
    passes, counts = {}, {}
    for h, w in grids:
        for label, ctx in ((f"{h}x{w}", contextlib.nullcontext()), (f"{h}x{w}/thresholds=1", thresholds_at_one())):
            with ctx:
                d = drive(make(), h, w)
            passes[label], counts[label] = d.rec.log, d.counts
    return passes, counts


def digest(name) -> str:
    return hashlib.sha256(json.dumps(transcript(name)[0], sort_keys=True).encode()).hexdigest()


def _ops(records):
    return {r[0] for r in records}


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_transcript(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden["sha256"]) == sorted(CASES)
    passes, counts = transcript(name)
    for label, per_method in counts.items():
        assert per_method and all(n >= 1 for _m, n in per_method), f"{name} {label}: a driven method left no record: {per_method}"
    assert digest(name) == golden["sha256"][name], f"{name}: the launch sequence differs from commit {golden['parent_commit']}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_winograd_only_on_fp32_past_the_thresholds(name):
    """`conv2d_wino` shows in the fp32 transcripts of the thresholds-at-1 pass and nowhere else; `conv2d_wino1d` in those of them
    whose engine packed the F(4,5) twins (SepConvGRU with the context hoisted)"""
    precision = CASES[name][2]
    for label, records in transcript(name)[0].items():
        past = precision == "fp32" and label.endswith("thresholds=1")
        ops = _ops(records)
        assert ("conv2d_wino" in ops) == past, (name, label)
        has_1d = past and "sea_update" not in name and "small" not in name and "unhoisted" not in name
        assert ("conv2d_wino1d" in ops) == has_1d, (name, label)
        assert "conv2d_wino_res" not in ops and "conv2d_wino_stats" not in ops


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    commit = sys.argv[1]
    with open(GOLDEN, "w") as f:
        json.dump({"parent_commit": commit, "sha256": {k: digest(k) for k in sorted(CASES)}}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} digests from {commit}")
