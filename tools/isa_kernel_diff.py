#!/usr/bin/env python3
"""Per-kernel comparison of two device ISA texts of one source file (hipcc <the file's Makefile flags> --cuda-device-only -S), for changes
that add template parameters or instances to a translation unit: isa_kernel_diff.py parent.s branch.s [drop-suffix]

A kernel is compared by its instruction text and its code-object metadata (registers, spills, scratch, LDS).  What an added instance
changes in its neighbours without changing their code is normalised away: the function index inside block labels (.LBB<n>_<m>) and the
label padding that follows it.  `drop-suffix` is removed from the mangled names of the branch text first -- a defaulted template parameter
that the parent did not have, e.g. ELi32EEEvNS_10GemmParamsE -> EEEvNS_10GemmParamsE."""
import re
import sys


def kernels(path, drop=None):
    s = open(path).read()
    if drop:
        s = s.replace(drop[0], drop[1])
    body, meta = {}, {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.S | re.M):
        t = re.sub(r"BB\d+_", "BB_", m.group(2))
        t = re.sub(r"\.Lfunc_(begin|end)\d+", ".Lfunc", t)
        body[m.group(1)] = re.sub(r"[ \t]+", " ", t)
    for m in re.finditer(r"\.name:\s+(_Z\w+)\n(.*?)(?=\n  - |\namdhsa)", s, re.S):
        keys = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
        meta[m.group(1)] = {k: v.group(1) for k in keys for v in [re.search(k + r":\s*(\d+)", m.group(0))] if v}
    return body, meta


def main():
    drop = None
    if len(sys.argv) > 3:
        suffix = sys.argv[3]
        drop = (suffix, re.sub(r"^ELi\d+E", "E", suffix))
    a, ma = kernels(sys.argv[1])
    b, mb = kernels(sys.argv[2], drop)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a:
            print("new      ", k, mb.get(k))
        elif k not in b:
            print("gone     ", k)
            bad += 1
        elif a[k] == b[k] and ma.get(k) == mb.get(k):
            print("equal    ", k)
        else:
            print("DIFFERENT", k)
            bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
