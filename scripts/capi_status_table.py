#!/usr/bin/env python3
"""Status-code table of libpfk.so's convolution launchers: what each entry point answers to a grid of mutated descriptors.

    python scripts/capi_status_table.py --write     # record tests/golden/capi_status_table.json from the library in the tree
    python scripts/capi_status_table.py             # compare the library in the tree with the recorded table

For every conv-descriptor entry point a few valid base descriptors (small shapes on made-up aligned addresses, 0x10000 + k * 4096;
an argument check never dereferences them) are mutated one field at a time — every pointer to NULL / +2 / +4 / +8 bytes, every
integer to INTS — and then in PAIRS drawn from PAIR_PTR x PAIR_INT of the same list: the pairs pin the precedence between
PFK_ERR_BAD_ARG, PFK_ERR_ALIGNMENT and PFK_ERR_UNSUPPORTED.  One character per case, in generation order:

    launchers   '0' PFK_OK, '1'..'5' the status -1..-5.  Without a device an accepted descriptor answers '4' (PFK_ERR_LAUNCH) and
                returns cleanly: those cases pin that nothing valid starts being refused.
    queries     '1'..'5' for a negative answer, else a letter: the value mod 52.

ONLY FOR A MACHINE WITHOUT A GPU: with a device an accepted case would be a launch on the made-up addresses.
tests/test_capi_status_table.py runs the comparison; scripts/capi_status_main.cpp replays the same cases under the sanitizers."""
import argparse
import ctypes
import itertools
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from pfk_ctypes import EPI_GRU_Q, EPI_GRU_ZR, EPI_LINEAR, EPI_LINEAR_GELU, Desc, DescB16  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "capi_status_table.json"
P, I, F, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong

INTS = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 31, 33, 64, 1 << 20, 1 << 28]
PTRS = ["null", 2, 4, 8]                    # NULL or + that many bytes
PAIR_INT, PAIR_PTR = [-1, 33, 1 << 20], ["null", 4]
QUERY_PAIR_INT, QUERY_PAIR_PTR = [-1, 1 << 20], ["null"]


def addr(k):
    return 0x10000 + k * 4096


# ---------------------------------------------------------------------------------------------------------------- base descriptors
def base_desc(kind, b16=False, wide=False):
    """kind: lin3 (LINEAR 3x3, three sources), zr15 (GRU_ZR 1x5), q51 (GRU_Q 5x1), lin15 (LINEAR 1x5), wino (one source, 3x3),
    res (wino + residual), gelu (LINEAR_GELU 1x1), wg11 (1x1, the weight gradient's third kernel shape)."""
    d = (DescB16 if b16 else Desc)()
    chans = {"wino": [(128, 136)], "res": [(128, 136)], "zr15": [(128, 136), (64, 64)], "q51": [(128, 136), (64, 64)],
             "lin15": [(128, 136), (64, 64)]}.get(kind, [(128, 136), (64, 64), (8, 8)])
    for i, (c, ld) in enumerate(chans):
        d.src[i].ptr, d.src[i].ld, d.src[i].channels = addr(i), (1 << 20) if (wide and i == 0) else ld, c
    d.num_src, d.B, d.H, d.W = len(chans), 2, 6, 10
    d.kh, d.kw = {"zr15": (1, 5), "lin15": (1, 5), "q51": (5, 1), "gelu": (1, 1), "wg11": (1, 1)}.get(kind, (3, 3))
    d.weight, d.bias, d.scale = addr(3), addr(4), 1.0
    d.epilogue = {"zr15": EPI_GRU_ZR, "q51": EPI_GRU_Q, "gelu": EPI_LINEAR_GELU}.get(kind, EPI_LINEAR)
    d.cout = 128 if kind == "zr15" else 64
    if d.epilogue in (EPI_LINEAR, EPI_LINEAR_GELU):
        d.out, d.out_ld, d.out_coff = addr(5), 72, 8
        if b16:
            d.out_bf16 = 1
        if kind == "res":
            d.residual, d.residual_ld = addr(9), 64
    else:
        d.h, d.h_ld, d.aux_z, d.aux_rh, d.residual, d.residual_ld = addr(6), 136, addr(7), addr(8), addr(9), d.cout
        if b16:
            d.h_b16, d.h_b16_ld = addr(10), 136
    return d


def fields(struct, prefix=""):
    """(path, 'ptr' | 'int') of every pointer and integer field, the three sources' included (floats are not mutated)."""
    out = []
    for name, tp in struct._fields_:
        if name == "src":
            for i in range(3):
                out += [(f"src{i}.{n}", k) for n, k in fields(tp._type_)]
        elif tp is P:
            out.append((prefix + name, "ptr"))
        elif tp in (I, LL):
            out.append((prefix + name, "int"))
    return out


# -------------------------------------------------------------------------------------------------------------------- entry points
# extras: (name, ctype, base value); 'hostints' = a real host array of three ints (the launcher reads it)
WS = ("workspace", P, addr(14)), ("workspace_bytes", LL, 1 << 30)
UNPACKED = (("real_channels", "hostints", (100, 64, 8)), ("dy", P, addr(11)), ("dy_ld", I, 136), ("cout_real", I, 60), ("dw", P, addr(12)),
            ("db", P, addr(13)), ("accumulate", I, 0)) + WS
NORM = ("in_mean", P, addr(11)), ("in_rstd", P, addr(12)), ("in_relu", I, 1)
GATES = ["lin3", "zr15", "q51"]
# name -> (b16 descriptor?, base kinds, extras, restype, query?)
ENTRIES = {
    "pfk_conv2d_f32": (False, GATES + ["gelu"], (), I, False),
    "pfk_conv2d_group_f32": (False, ["lin3"], (("n", I, 2),), I, False),
    "pfk_conv2d_bf16s": (False, GATES, (("weight_planes", P, addr(11)), ("nsplit", I, 2)), I, False),
    "pfk_conv2d_b16": (True, GATES, (), I, False),
    "pfk_conv2d_gelu_b16": (True, ["gelu"], (), I, False),
    "pfk_conv2d_wino_f32": (False, ["wino"], (), I, False),
    "pfk_conv2d_wino_res_f32": (False, ["res"], (), I, False),
    "pfk_conv2d_wino_norm_f32": (False, ["wino"], NORM, I, False),
    "pfk_conv2d_wino_stats_f32": (False, ["wino"], NORM + (("eps", F, 1e-5), ("out_mean", P, addr(13)), ("out_rstd", P, addr(15))) + WS, I, False),
    "pfk_conv1d_wino_f32": (False, ["lin15", "zr15", "q51"], (), I, False),
    "pfk_conv_wgrad_f32": (False, ["lin3", "zr15"], (("dy", P, addr(11)), ("dy_ld", I, 136), ("dw_packed", P, addr(12)), ("with_bias", I, 1)) + WS, I, False),
    "pfk_conv_wgrad_unpacked_f32": (False, ["lin3", "zr15"], UNPACKED, I, False),
    "pfk_conv_wgrad_unpacked_b16": (True, ["lin3", "zr15", "wg11"], UNPACKED, I, False),
    "pfk_conv_ktot": (False, ["lin3"], (), I, True),
    "pfk_conv_ktot_bf16": (False, ["lin3"], (), I, True),
    "pfk_conv_ktot_b16": (True, ["lin3"], (), I, True),
    "pfk_conv_wgrad_workspace_bytes": (False, ["lin3"], (("with_bias", I, 1),), LL, True),
    "pfk_conv_wgrad_unpacked_workspace_bytes": (False, ["lin3"], (("with_bias", I, 1),), LL, True),
    "pfk_conv_wgrad_unpacked_b16_workspace_bytes": (True, ["lin3"], (("with_bias", I, 1),), LL, True),
    # scalar queries: their arguments are read off the (mutated) descriptor
    "pfk_conv_wino_weight_floats": (False, ["wino"], "scalars", LL, True),
    "pfk_conv_wino1d_weight_floats": (False, ["lin15"], "scalars", LL, True),
    "pfk_conv_wino_stats_workspace_bytes": (False, ["wino"], "scalars", LL, True),
}
SCALARS = {
    "pfk_conv_wino_weight_floats": lambda d: (d.src[0].channels, d.cout),
    "pfk_conv_wino1d_weight_floats": lambda d: (ctypes.c_int(d.src[0].channels + d.src[1].channels).value, d.cout),
    "pfk_conv_wino_stats_workspace_bytes": lambda d: (d.B, d.H, d.W, d.cout),
}


def bases(name):
    """(label, descriptor) of an entry point's bases: its kinds, and the first kind once more with src[0].ld = 2^20 ('wide': B * H * W
    * ld passes 2 GB, so the mutations meet the span checks) on a batch that makes the base itself still fit."""
    b16, kinds = ENTRIES[name][0], ENTRIES[name][1]
    out = [(k, base_desc(k, b16)) for k in kinds]
    w = base_desc(kinds[0], b16, wide=True)
    w.B, w.H, w.W = 1, 6, 10      # 60 rows of 2^20 elements: 240 MB on paper; B -> 8 and up no longer fits
    return out if ENTRIES[name][4] else out + [("wide", w)]       # (a query has no span check to meet)


def mutations(name):
    """The single mutations of an entry point, as (label, target, path, kind, value); target 'd' (descriptor) or 'x' (extra)."""
    b16, _, extras, _, query = ENTRIES[name]
    muts = []
    for path, kind in fields(DescB16 if b16 else Desc):
        muts += [(f"{path}={v}", "d", path, kind, v) for v in (PTRS if kind == "ptr" else INTS)]
    for ename, tp, _ in (() if extras == "scalars" else extras):
        if tp == "hostints":
            muts.append((f"{ename}=null", "x", ename, "ptr", "null"))
            muts += [(f"{ename}[{i}]={v}", "x", (ename, i), "elem", v) for i in range(3) for v in (-1, 0, 1 << 20)]
        elif tp is P:
            muts += [(f"{ename}={v}", "x", ename, "ptr", v) for v in PTRS]
        elif tp in (I, LL):
            muts += [(f"{ename}={v}", "x", ename, "int", v) for v in INTS]
    pi, pp = (QUERY_PAIR_INT, QUERY_PAIR_PTR) if query else (PAIR_INT, PAIR_PTR)
    # 33 (off every alignment quantum) only where a quantum applies: row strides and channel counts
    quantum = lambda m: m[2].endswith(("ld", "channels", "cout"))      # noqa: E731
    sub = [m for m in muts if (m[3] == "ptr" and m[4] in pp) or (m[3] == "int" and m[4] in pi and (m[4] != 33 or quantum(m))) or
           (m[3] == "elem" and m[4] == -1)]
    return muts, sub


def case_list(name):
    """[(label, (mutation, ...))]: the unmutated base, every single mutation, every pair of the subsample."""
    muts, sub = mutations(name)
    return [("base", ())] + [(m[0], (m,)) for m in muts] + [(f"{a[0]} & {b[0]}", (a, b)) for a, b in itertools.combinations(sub, 2)]


def _set(obj, path, kind, v):
    if "." in path:
        s, path = path.split(".")
        obj = obj.src[int(s[3:])]
    if kind == "ptr":
        cur = getattr(obj, path) or 0
        setattr(obj, path, None if v == "null" else cur + v)
    else:
        setattr(obj, path, v)


def materialise(name):
    """(base label, base, mutated descriptor, {extra name: value}) of every case of an entry point, in generation order"""
    extras = ENTRIES[name][2]
    cases = case_list(name)
    for blabel, base in bases(name):
        for _, muts in cases:
            d = type(base).from_buffer_copy(base)
            x = {} if extras == "scalars" else {e[0]: (list(e[2]) if e[1] == "hostints" else e[2]) for e in extras}
            for _, target, path, kind, v in muts:
                if target == "d":
                    _set(d, path, kind, v)
                elif kind == "elem":
                    if x[path[0]] is not None:
                        x[path[0]][path[1]] = v
                elif kind == "ptr":
                    x[path] = None if (v == "null" or x[path] is None) else x[path] + v
                else:
                    x[path] = v
            yield blabel, base, d, x


LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def run_entry(lib, name):
    """{base label: string of one character per case}"""
    _, _, extras, restype, query = ENTRIES[name]
    fn = getattr(lib, name)
    fn.restype = restype
    out = {}
    for blabel, base, d, x in materialise(name):
        if extras == "scalars":
            r = fn(*[I(a) for a in SCALARS[name](d)])
        else:
            args = []
            for ename, tp, _ in extras:
                val = x[ename]
                args.append((None if val is None else (I * 3)(*val)) if tp == "hostints" else (P(val) if tp is P else tp(val)))
            if name == "pfk_conv2d_group_f32":       # descs[0] carries the mutations; `n` descriptors are read
                r = fn((Desc * 4)(d, base, base, base), *args, None)
            elif query:
                r = fn(ctypes.byref(d), *args)
            else:
                r = fn(ctypes.byref(d), *args, None)
        c = LETTERS[r % 52] if (query and r >= 0) else (str(-r) if -9 <= r <= 0 else "?")
        out[blabel] = out.get(blabel, "") + c
    return out


def dump(path, want):
    """The cases as text for scripts/capi_status_main.cpp: `entry expected descriptor-bytes-in-hex argument ...` per line; an argument is
    an integer (a pointer's address), a float, or h:a,b,c / h:null for the host array."""
    with open(path, "w") as f:
        for name, (_, _, extras, _, _) in ENTRIES.items():
            pos = {}
            for blabel, base, d, x in materialise(name):
                i = pos[blabel] = pos.get(blabel, -1) + 1
                if extras == "scalars":
                    args = [str(a) for a in SCALARS[name](d)]
                else:
                    args = []
                    for ename, tp, _ in extras:
                        v = x[ename]
                        args.append(("h:null" if v is None else "h:" + ",".join(map(str, v))) if tp == "hostints" else
                                    repr(float(v)) if tp is F else str(v or 0))
                blob = bytes(d) + (bytes(base) * 3 if name == "pfk_conv2d_group_f32" else b"")
                f.write(" ".join([name, want[name][blabel][i], blob.hex(), *args]) + "\n")


def run_all(lib):
    return {name: run_entry(lib, name) for name in ENTRIES}


def first_difference(got, want):
    """None, or a one-line description of the first case whose answer differs from the recorded one."""
    for name in ENTRIES:
        if name not in want:
            return f"{name}: not in the recorded table"
        labels = None
        for blabel, s in got[name].items():
            w = want[name].get(blabel)
            if w is None or len(w) != len(s):
                return f"{name} / {blabel}: {len(s)} cases here, {None if w is None else len(w)} recorded"
            if s != w:
                labels = labels or [c[0] for c in case_list(name)]
                i = next(i for i in range(len(s)) if s[i] != w[i])
                return f"{name} / base {blabel} / case {i} ({labels[i]}): answers '{s[i]}', recorded '{w[i]}'"
    return None


def load_lib():
    from pfk_ctypes import lib
    return lib()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="record the table instead of comparing with it")
    ap.add_argument("--dump", type=Path, metavar="FILE", help="write the recorded cases as text for scripts/capi_status_main.cpp and exit")
    a = ap.parse_args()
    if a.dump:
        dump(a.dump, json.loads(GOLDEN.read_text()))
        return 0
    import torch
    if torch.cuda.is_available():
        sys.exit("a GPU is visible: an accepted case would launch on made-up addresses")
    got = run_all(load_lib())
    n = sum(len(s) for e in got.values() for s in e.values())
    if a.write:
        GOLDEN.write_text(json.dumps(got, indent=0, sort_keys=True) + "\n")
        print(f"{n} cases -> {GOLDEN} ({GOLDEN.stat().st_size} bytes)")
        return 0
    diff = first_difference(got, json.loads(GOLDEN.read_text()))
    print(diff or f"{n} cases answer as recorded")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
