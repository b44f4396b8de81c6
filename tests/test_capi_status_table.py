"""The argument checks of the convolution launchers, pinned case by case: scripts/capi_status_table.py mutates a few valid descriptors
per entry point (every pointer and integer field, then pairs) and tests/golden/capi_status_table.json holds what the library
answered when the table was recorded.  The launchers' host side may be rewritten freely as long as every one of these ~190 000
answers stays what it was — BAD_ARG / ALIGNMENT / UNSUPPORTED in the same order of precedence, and nothing valid refused.

Host logic only, and only without a GPU: the descriptors sit on made-up addresses, so with a device a case that is (rightly or
wrongly) accepted would be a launch on them.  Without one an accepted case answers PFK_ERR_LAUNCH and returns."""
import ctypes
import importlib.util
import json
import subprocess
from pathlib import Path

import pytest
import torch

import pfk_ctypes
from pfk_ctypes import PFK_ERR_ALIGNMENT, PFK_ERR_BAD_ARG, PFK_ERR_LAUNCH, PFK_ERR_UNSUPPORTED

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def table():
    spec = importlib.util.spec_from_file_location("capi_status_table", ROOT / "scripts" / "capi_status_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-logic test: with a device an accepted case would launch on made-up addresses")
def test_capi_status_table(table):
    want = json.loads(table.GOLDEN.read_text())
    got = table.run_all(pfk_ctypes.lib())
    assert set(got) == set(want) == set(table.ENTRIES)
    diff = table.first_difference(got, want)      # compares every case of every (entry point, base); lengths included
    assert diff is None, diff
    for name, per_base in want.items():
        ncases = len(table.case_list(name))
        assert set(per_base) == {b for b, _ in table.bases(name)}
        for base, s in per_base.items():
            assert len(s) == ncases, f"{name} / {base}: {len(s)} recorded answers for {ncases} cases"
            if table.ENTRIES[name][4]:
                continue       # a query answers a size; the launchers below answer a status
            assert s[0] == str(-PFK_ERR_LAUNCH), f"{name} / {base}: the base itself must be accepted, answered '{s[0]}'"
            for code in (PFK_ERR_BAD_ARG, PFK_ERR_ALIGNMENT, PFK_ERR_UNSUPPORTED, PFK_ERR_LAUNCH):
                assert str(-code) in s, f"{name} / {base}: no case answers {code}"
            assert set(s) <= set("1234"), f"{name} / {base}: unexpected answers {sorted(set(s) - set('1234'))}"


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "pfk.h"
#define S(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  S(pfk_conv_src); S(pfk_conv_src_b16); S(pfk_conv_desc); S(pfk_conv_b16_desc);
@FIELDS@  return 0;
}
"""
MIRRORS = {"pfk_conv_src": pfk_ctypes.Src, "pfk_conv_src_b16": pfk_ctypes.SrcB16, "pfk_conv_desc": pfk_ctypes.Desc,
           "pfk_conv_b16_desc": pfk_ctypes.DescB16}


def test_ctypes_mirror_matches_header(tmp_path):
    """sizeof and every offsetof of the four structs, printed by a C program compiled against include/pfk.h"""
    clang = pfk_ctypes.rocm_clang()
    if clang is None:
        pytest.skip("no ROCm clang next to hipcc")
    lines = "".join(f"  O({cname}, {f});\n" for cname, cls in MIRRORS.items() for f, _ in cls._fields_)
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("@FIELDS@", lines))
    exe = tmp_path / "probe"
    subprocess.run([clang, "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for cname, cls in MIRRORS.items():
        want[cname] = str(ctypes.sizeof(cls))
        want.update({f"{cname}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert out == want
    # the header's field lists are the mirrors' too: a field added to pfk.h without its mirror changes sizeof
