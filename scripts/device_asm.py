#!/usr/bin/env python3
"""gfx950 device assembly of every translation unit of libpfk.so, one .s per file, for comparing two trees:

    python scripts/device_asm.py ptlflow_amd/csrc            out/branch  [--variants]
    python scripts/device_asm.py ../parent/ptlflow_amd/csrc  out/parent  [--variants]
    diff -r out/parent out/branch

The file list and each file's flags (-ffp-contract=off, ...) are ptlflow_amd/_build.py's; the csrc directory is an argument, so
the same flags compile a checkout of another commit (its public header is taken from <csrc>/../../include).  -fuse-cuid=none
keeps hipcc from stamping a random __hip_cuid_* symbol into each listing: without it two compilations of one file differ in
exactly those lines.  --variants adds -DPFK_BENCH_VARIANTS to the pfk_gemm* files, as PFK_BENCH_VARIANTS=1 does in the build.
Needs no GPU and does not read the assembly: a refactor that leaves every kernel alone leaves `diff -r` empty."""
import argparse
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ptlflow_amd._build import HIP_FLAGS, HIP_SOURCES, HIPCC  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csrc", type=Path, help="the csrc directory of the tree to compile")
    ap.add_argument("out", type=Path, help="output directory (one <file>.s per translation unit)")
    ap.add_argument("--variants", action="store_true", help="compile the pfk_gemm* files with -DPFK_BENCH_VARIANTS")
    ap.add_argument("--only", nargs="+", metavar="FILE", help="these translation units only (pfk_wino.hip ...)")
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
    print(f"{len(jobs) - len(bad)} of {len(jobs)} translation units -> {a.out}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
