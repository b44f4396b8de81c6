"""The K order of the packed convolution weight, checked on the CPU.  ptlflow_amd/csrc/pfk_conv_k.h is the one definition the
kernels use (conv_k_decode: stream-K seeks; conv_k_advance: every forward stager; chunk_ref: the weight-gradient kernels);
scripts/conv_k_order_main.cpp compiles that header for the host and prints, per case, every K-step as decoded and as reached by
advancing from step 0.  Held here to each other, to pfk_conv_k's count (through the library's pfk_conv_ktot*), to what
packing.pack_conv_weight lays out, and to the inverse that wgrad_reduce_unpack_kernel applies (restated below).  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import pfk_ctypes
from ptlflow_amd.packing import pack_conv_weight

ROOT = Path(__file__).resolve().parent.parent
CHANNELS = (4, 8, 32, 36, 64, 96, 128, 324)
TAPS = ((1, 1), (3, 3), (1, 5), (5, 1), (7, 7))


def _cases():
    """(bk, channels per source, kh, kw): 1, 2 and 3 sources drawn from CHANNELS (multiples of 8 for the 64-channel chunk)"""
    out = []
    for bk in (32, 64):
        ch = [c for c in CHANNELS if bk == 32 or c % 8 == 0]
        n = len(ch)
        tuples = [(c,) for c in ch]
        tuples += [(ch[i], ch[(i + d) % n]) for i in range(n) for d in (1, n // 2)]
        tuples += [(ch[i], ch[(i + 3) % n], ch[(i + 5) % n]) for i in range(n)]
        out += [(bk, t, kh, kw) for t in tuples for kh, kw in TAPS]
    return out


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    """{case: (S rows [steps][11], R rows [steps + 2][7] or None)} from one run of the host program over all cases"""
    clang = pfk_ctypes.rocm_clang()
    if clang is None:
        pytest.skip("no ROCm clang next to hipcc")
    exe = tmp_path_factory.mktemp("conv_k_order") / "conv_k_order"
    subprocess.run([clang, "-x", "c++", "-std=c++17", "-O1", f"-I{ROOT / 'ptlflow_amd' / 'csrc'}", str(ROOT / "scripts" / "conv_k_order_main.cpp"),
                    "-o", str(exe)], check=True)
    cases = _cases()
    text = "".join(f"{bk} {len(ch)} {' '.join(str(c) for c in (ch + (0, 0))[:3])} {kh} {kw}\n" for bk, ch, kh, kw in cases)
    lines = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    out, i = {}, 0
    for case in cases:
        bk, ch, kh, kw = case
        head = lines[i].split()
        assert head[0] == "C" and [int(v) for v in head[1:8]] == [bk, len(ch), *(ch + (0, 0))[:3], kh, kw], lines[i]
        steps = int(head[8])
        s = np.array([ln.split()[1:] for ln in lines[i + 1:i + 1 + steps]], dtype=np.int64)
        assert all(ln[0] == "S" for ln in lines[i + 1:i + 1 + steps])
        i += 1 + steps
        r = None
        if bk == 32:
            assert all(ln[0] == "R" for ln in lines[i:i + steps + 2])
            r = np.array([ln.split()[1:] for ln in lines[i:i + steps + 2]], dtype=np.int64)
            i += steps + 2
        out[case] = (s, r)
    assert i == len(lines)
    return out


def _ktot(bk, ch, kh, kw):
    """pfk_conv_k of the launcher that reads this weight, asked of the library (a query: nothing is launched)"""
    lib = pfk_ctypes.lib()
    d = pfk_ctypes.Desc() if bk == 32 else pfk_ctypes.DescB16()
    d.num_src, d.kh, d.kw = len(ch), kh, kw
    for s, c in enumerate(ch):
        d.src[s].channels = c
    fn = lib.pfk_conv_ktot if bk == 32 else lib.pfk_conv_ktot_b16
    fn.restype = ctypes.c_int
    return fn(ctypes.byref(d))


def _encode(c, ky, kx, kh, kw):
    return 1 + (c * kh + ky) * kw + kx      # never 0: the padding's value


def _packed_row(bk, ch, kh, kw):
    """row 0 of the packed weight whose element [co, c, ky, kx] is _encode(c, ky, kx): exact in fp32 (< 2^24)"""
    cin = sum(ch)
    c, ky, kx = np.meshgrid(np.arange(cin), np.arange(kh), np.arange(kw), indexing="ij")
    w = torch.from_numpy(_encode(c, ky, kx, kh, kw).astype(np.float32))[None]
    first = np.concatenate([[0], np.cumsum(ch)[:-1]])
    return pack_conv_weight(w, [(int(f), n, n) for f, n in zip(first, ch)], kpad=bk)[0].numpy().astype(np.int64), first


def test_case_count(walks):
    assert 200 <= len(walks) <= 400 and len({bk for bk, *_ in walks}) == 2


def test_decode_equals_advance(walks):
    """(a) decode(step) is where advance() arrives from step 0, step by step, and there are pfk_conv_k / chunk steps"""
    for (bk, ch, kh, kw), (s, _) in walks.items():
        assert len(s) * bk == _ktot(bk, ch, kh, kw), (bk, ch, kh, kw)
        assert (s[:, 0] == np.arange(len(s))).all()
        assert (s[:, 1:5] == s[:, 5:9]).all(), (bk, ch, kh, kw, int(np.argmax((s[:, 1:5] != s[:, 5:9]).any(axis=1))))
        assert (s[:, 9] == s[:, 0] * bk).all()                      # kofs
        assert (s[:, 10] == s[:, 2] * kw + s[:, 3]).all()           # the running tap of the bf16 stager
        assert (s[:, 1] < len(ch)).all() and (s[:, 2] < kh).all() and (s[:, 3] < kw).all() and (s[:, 4] % bk == 0).all()


def test_order_is_the_packing(walks):
    """(b) chunk k of the packed row holds the bk channels from c0 of source seg at tap (ky, kx), zeros past the source's channels"""
    for (bk, ch, kh, kw), (s, _) in walks.items():
        row, first = _packed_row(bk, ch, kh, kw)
        assert row.size == len(s) * bk
        seg, ky, kx, c0 = (s[:, j][:, None] for j in (1, 2, 3, 4))
        c = c0 + np.arange(bk)[None]
        want = np.where(c < np.array(ch)[seg], _encode(first[seg] + c, ky, kx, kh, kw), 0)
        assert (row.reshape(len(s), bk) == want).all(), (bk, ch, kh, kw)


def test_chunk_ref_is_decode(walks):
    """(c) the weight-gradient kernels' entry for chunk k: decode(k)'s source and first channel, its tap re-centred; then the bias
    chunk, then dead chunks"""
    for (bk, ch, kh, kw), (s, r) in walks.items():
        if bk != 32:
            continue
        n = len(s)
        assert (r[:, 0] == np.arange(n + 2)).all()
        assert (r[:n, 1] == 100 + s[:, 1]).all() and (r[:n, 2] == s[:, 4]).all(), (ch, kh, kw)
        assert (r[:n, 3] == s[:, 2] - kh // 2).all() and (r[:n, 4] == s[:, 3] - kw // 2).all(), (ch, kh, kw)
        assert (r[:n, 5] == 0).all() and (r[:n, 6] == 1).all()
        assert r[n, 2:].tolist() == [0, 0, 0, 1, 1] and r[n + 1, 2:].tolist() == [0, 0, 0, 0, 0]


def _unpack_destination(k, ch, taps):
    """wgrad_reduce_unpack_kernel's index arithmetic (pfk_wgrad_reduce.h) for the packed columns k (an array) of a row without bias
    chunk: (real, channel of the concatenated input, tap) of the dw element each is added to; real = False for a padding column.
    u.cpad[s] = channels padded to 32, u.nreal[s] = the source's real channels, u.first[s] = the channels in front of source s."""
    cpad = np.array([(c + 31) // 32 * 32 for c in ch])
    first = np.array([sum(ch[:s]) for s in range(len(ch))])
    kk, sg = k.copy(), np.zeros_like(k)
    for _ in range(len(ch) - 1):      # while (sg < u.nseg - 1 && kk >= u.taps * u.cpad[sg]) { kk -= u.taps * u.cpad[sg]; ++sg; }
        move = (sg < len(ch) - 1) & (kk >= taps * cpad[sg])
        kk = kk - np.where(move, taps * cpad[sg], 0)
        sg = sg + move
    tap = kk // cpad[sg]
    c = kk - tap * cpad[sg]
    return c < np.array(ch)[sg], first[sg] + c, tap


def test_unpack_inverts_the_packing(walks):
    """(d) every packed column goes back to the weight element it was packed from; padding columns go nowhere"""
    for (bk, ch, kh, kw) in walks:
        if bk != 32:
            continue
        row, _ = _packed_row(32, ch, kh, kw)
        real, c, tap = _unpack_destination(np.arange(row.size), ch, kh * kw)
        # dw[co][c][ky][kx] lies at dw + (co * cin + c) * taps + tap: tap = ky * kw + kx
        assert (row == np.where(real, _encode(c, tap // kw, tap % kw, kh, kw), 0)).all(), (ch, kh, kw)
