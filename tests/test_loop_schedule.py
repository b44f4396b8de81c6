"""`ptlflow_amd.raft.loop_schedule`: the one rule that picks `RAFT._iterate`'s schedule, against its specification.

No GPU and no `torch.cuda` call: the rule takes plain values.  The five lines in `_spec` ARE the specification (the rule as the loop
spelled it before it was a function); the named cases below are the rows that carry the project's measured decisions."""
import itertools

import pytest

from ptlflow_amd.raft import loop_schedule
from ptlflow_amd.update import SMALL_GRID_PIXELS as T


def _spec(*, pixels, has_mask, aggregate, alternate_corr, can_fuse, b16, can_group, capturing,
          fork_branches, fuse_mask_upsample, overlap_mask_head, group_launches):
    fork = fork_branches if fork_branches is not None else capturing
    forked = fork and not aggregate and not alternate_corr          # ignores `fuse`: always mask_head + convex_upsample_pm
    fuse = has_mask and can_fuse and (fuse_mask_upsample if fuse_mask_upsample is not None else pixels >= T)
    side = has_mask and overlap_mask_head and pixels >= T and not capturing and not (fuse and b16)
    grouped = not side and not fuse and can_group and not alternate_corr and (group_launches if group_launches is not None else pixels < T)
    if forked:
        return "forked", False
    if grouped:
        return "grouped", False      # (`grouped` implies `not fuse`)
    return ("side" if side else "serial"), bool(fuse)


TRI, BOOL = (None, True, False), (True, False)
FIELDS = ("fork_branches", "fuse_mask_upsample", "group_launches", "overlap_mask_head", "capturing", "has_mask", "aggregate",
          "alternate_corr", "can_fuse", "b16", "can_group", "pixels")


def test_truth_table():
    """every combination of the three tri-state overrides, the eight booleans and the two sides of the threshold: 3^3 * 2^8 * 2 rows"""
    rows = 0
    for values in itertools.product(TRI, TRI, TRI, *([BOOL] * 8), (T - 1, T)):
        kw = dict(zip(FIELDS, values))
        loop, fused = loop_schedule(**kw)
        assert (loop, fused) == _spec(**kw), kw
        assert isinstance(loop, str) and isinstance(fused, bool), kw
        rows += 1
    assert rows == 27 * 256 * 2


def _model(pixels, **kw):
    """RAFT (mask head, materialised volume) on the fp32 engine, eager, every attribute at its default"""
    base = dict(pixels=pixels, has_mask=True, aggregate=False, alternate_corr=False, can_fuse=True, b16=False, can_group=True,
                capturing=False, fork_branches=None, fuse_mask_upsample=None, overlap_mask_head=True, group_launches=None)
    base.update(kw)
    return base


BF16 = dict(b16=True, can_group=False)      # the K8b engine: fused K13b, no grouped launch
GMA = dict(aggregate=True)


@pytest.mark.parametrize("name,kw,want", [
    ("fp32 batch 1 of 436x1024, defaults", _model(55 * 128), ("grouped", False)),
    ("fp32 batch 8, defaults", _model(8 * 55 * 128), ("side", True)),
    ("bf16 batch 8: the `fuse and b16` exclusion", _model(8 * 55 * 128, **BF16), ("serial", True)),
    ("capturing with fork_branches=None", _model(55 * 128, capturing=True), ("forked", False)),
    ("capturing at batch 8", _model(8 * 55 * 128, capturing=True), ("forked", False)),
])
def test_named_cases(name, kw, want):
    assert loop_schedule(**kw) == want, name


@pytest.mark.parametrize("pixels", [55 * 128, 8 * 55 * 128])
@pytest.mark.parametrize("fork_branches", TRI)
def test_gma_is_never_forked(pixels, fork_branches):
    for capturing in BOOL:
        loop, _ = loop_schedule(**_model(pixels, capturing=capturing, fork_branches=fork_branches, **GMA))
        assert loop != "forked"
    assert loop_schedule(**_model(55 * 128, capturing=True, **GMA)) == ("grouped", False)


def test_alternate_corr_is_never_grouped_never_forked():
    for pixels, capturing, fork, group, fuse, overlap in itertools.product((T - 1, T), BOOL, TRI, TRI, TRI, BOOL):
        loop, _ = loop_schedule(**_model(pixels, alternate_corr=True, capturing=capturing, fork_branches=fork, group_launches=group,
                                         fuse_mask_upsample=fuse, overlap_mask_head=overlap))
        assert loop in ("serial", "side"), (pixels, capturing, fork, group, fuse, overlap)


def test_threshold_sides():
    """the defaults flip exactly at the threshold: 28 160 pixels, batch 4 of 436x1024"""
    assert T == 4 * 55 * 128
    assert loop_schedule(**_model(T - 1)) == ("grouped", False) and loop_schedule(**_model(T)) == ("side", True)
