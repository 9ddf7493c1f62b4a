#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  Compares device assembly, kernel by kernel.

    for f in java-sdr_amd/csrc/bpsk*.hip; do      # once per build, with the flags of java-sdr_amd/build.py for that file
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off ... --cuda-device-only -S $f -o DIR/$(basename $f .hip).s
    done
    python tools/kernel_asm_diff.py DIR_BEFORE DIR_AFTER [> profiles/<name>_kernel_digests.txt]

For every kernel symbol (.amdhsa_kernel NAME) of every .s file of a directory: (a) its instruction text from its label to its
.Lfunc_end, comment lines dropped and the numbers of local labels (.LBB<fn>_<k>, .Lfunc_*<n>, .Ltmp<n>) normalised -- they count
the functions of the translation unit, so they move when code around a kernel does; (b) its .amdhsa_kernel ... .end_amdhsa_kernel
block (VGPRs, SGPRs, LDS, scratch, ...).  A kernel may move between files.  Exit status 0: the two sets of symbols are equal
and (a) and (b) are identical for every one.
"""
import glob
import hashlib
import os
import re
import sys

LOCAL = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(\w+?)\d+"), r".Lfunc_\1"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"),
         # the tune-mode units' copies of the __constant__ tables, jsdr::{front,fm,tail}::c_bpsk: one object, jsdr::c_bpsk, before the cut
         (re.compile(r"_ZN4jsdr(?:5front|2fm|4tail)6c_bpskE"), "_ZN4jsdr6c_bpskE")]


def norm(line):
    line = line.split(";", 1)[0].rstrip()  # (a trailing comment carries no code)
    for rx, to in LOCAL:
        line = rx.sub(to, line)
    return line


def kernels(directory):
    """{symbol: (file, sha256 of the code, sha256 of the descriptor block)}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end") and lines[i].endswith(":"))
            code = [norm(ln) for ln in lines[start:end] if not ln.lstrip().startswith(";")]
            code = [ln for ln in code if ln.strip()]
            d0 = next(i for i, ln in enumerate(lines) if ln.strip() == ".amdhsa_kernel " + name)
            d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            desc = [ln.strip() for ln in lines[d0:d1 + 1]]
            if name in out:
                sys.exit(f"{name}: defined in {out[name][0]} and in {os.path.basename(path)}")
            out[name] = (os.path.basename(path), hashlib.sha256("\n".join(code).encode()).hexdigest(),
                         hashlib.sha256("\n".join(desc).encode()).hexdigest(), len(code))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    lost, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [k for k in sorted(set(a) & set(b)) if a[k][1:3] != b[k][1:3]]
    files = sorted({os.path.basename(f) for d in sys.argv[1:3] for f in glob.glob(os.path.join(d, "*.s"))})
    print(f"kernel symbols: {len(a)} before, {len(b)} after; lost {len(lost)}, new {len(new)}, "
          f"code or descriptor differs {len(differ)}")
    for f in files:
        print(f"  {f}: {sum(v[0] == f for v in a.values())} before, {sum(v[0] == f for v in b.values())} after")
    for k in lost:
        print(f"LOST    {k} ({a[k][0]})")
    for k in new:
        print(f"NEW     {k} ({b[k][0]})")
    for k in differ:
        what = ("code " if a[k][1] != b[k][1] else "") + ("descriptor" if a[k][2] != b[k][2] else "")
        print(f"DIFFERS {k}: {what.strip()}")
    print("# symbol  file-before -> file-after  instructions  sha256(code)[:16]  sha256(descriptor)[:16]")
    for k in sorted(set(a) & set(b)):
        print(f"{k}  {a[k][0]} -> {b[k][0]}  {b[k][3]}  {b[k][1][:16]}  {b[k][2][:16]}")
    ok = not (lost or new or differ)
    print("RESULT: " + ("identical" if ok else "NOT identical"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
