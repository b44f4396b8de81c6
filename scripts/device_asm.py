#!/usr/bin/env python3
"""gfx950 device assembly of every translation unit of libpfk.so, one .s per file, for comparing two trees:

    python scripts/device_asm.py ptlflow_amd/csrc            out/branch  [--variants]
    python scripts/device_asm.py ../parent/ptlflow_amd/csrc  out/parent  [--variants]
    diff -r out/parent out/branch

The file list and each file's flags (-ffp-contract=off, ...) are ptlflow_amd/_build.py's; the csrc directory is an argument, so
the same flags compile a checkout of another commit (its public header is taken from <csrc>/../../include).  -fuse-cuid=none
keeps hipcc from stamping a random __hip_cuid_* symbol into each listing: without it two compilations of one file differ in
exactly those lines.  --variants adds -DPFK_BENCH_VARIANTS to the pfk_gemm* files, as PFK_BENCH_VARIANTS=1 does in the build.
Needs no GPU: a refactor that leaves every kernel alone leaves `diff -r` empty.

--summary writes <file>.summary next to each <file>.s, for a listing that did change: per kernel a digest of its text, its
`.amdhsa_` resource lines (registers, scratch, LDS), the code length where the assembler states it, and how often each mnemonic
occurs.  A kernel whose digest changed while the rest of its block did not was only re-ordered or re-allocated (same instructions,
same resources); `diff` of two .summary files shows which kernels those are.  A tally of every mnemonic, not a search for any."""
import argparse
import hashlib
import re
import subprocess
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ptlflow_amd._build import HIP_FLAGS, HIP_SOURCES, HIPCC  # noqa: E402


def summarize(listing):
    """{kernel: lines} of one .s file: the text between `<kernel>:` and its `.Lfunc_end`, and the kernel's `.amdhsa_kernel` block"""
    lines = listing.splitlines()
    kernels = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    out = {}
    for k in kernels:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(f"{k}:"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[start + 1:end]
        ops = Counter(ln.split()[0] for ln in body if ln.startswith("\t") and not ln.lstrip().startswith((".", ";")))
        d0 = next(i for i in range(start, end) if ".amdhsa_kernel" in lines[i])
        d1 = next(i for i in range(d0, end) if ".end_amdhsa_kernel" in lines[i])
        meta = [ln.strip() for ln in lines[d0 + 1:d1]]
        meta += [ln.strip() for ln in lines[end:end + 40] if ln.startswith("; codeLenInByte")][:1]
        out[k] = ([f"text sha1 {hashlib.sha1(chr(10).join(body).encode()).hexdigest()}"] + meta
                  + [f"{n:7d} {op}" for op, n in sorted(ops.items())] + [f"{sum(ops.values()):7d} instructions"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csrc", type=Path, help="the csrc directory of the tree to compile")
    ap.add_argument("out", type=Path, help="output directory (one <file>.s per translation unit)")
    ap.add_argument("--variants", action="store_true", help="compile the pfk_gemm* files with -DPFK_BENCH_VARIANTS")
    ap.add_argument("--only", nargs="+", metavar="FILE", help="these translation units only (pfk_wino.hip ...)")
    ap.add_argument("--summary", action="store_true", help="also write <file>.summary: per kernel a digest, resources and a mnemonic tally")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    csrc = a.csrc.resolve()
    a.out.mkdir(parents=True, exist_ok=True)
    flags = [f for f in HIP_FLAGS if not f.startswith("-I")] + [f"-I{csrc.parent.parent / 'include'}", f"-I{csrc}"]

    def one(job):
        src, extra = job
        if a.variants and src.startswith("pfk_gemm") and "-DPFK_BENCH_VARIANTS" not in extra:
            extra = extra + ["-DPFK_BENCH_VARIANTS"]
        cmd = [HIPCC, *flags, *extra, "--cuda-device-only", "-fuse-cuid=none", "-S", src, "-o", str((a.out / src).with_suffix(".s").resolve())]
        return src, subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)   # cwd: no tree path reaches the listing

    jobs = [j for j in HIP_SOURCES if not a.only or j[0] in a.only]
    with ThreadPoolExecutor(max_workers=a.j) as pool:
        bad = [(s, r.stderr) for s, r in pool.map(one, jobs) if r.returncode != 0]
    for s, err in bad:
        print(f"{s}: hipcc failed\n{err}", file=sys.stderr)
    if a.summary:
        for src, _ in jobs:
            lst = (a.out / src).with_suffix(".s")
            if lst.exists():
                blocks = summarize(lst.read_text())
                lst.with_suffix(".summary").write_text("".join(f"{k}\n" + "".join(f"  {ln}\n" for ln in v) for k, v in sorted(blocks.items())))
    print(f"{len(jobs) - len(bad)} of {len(jobs)} translation units -> {a.out}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
