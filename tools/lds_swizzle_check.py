#!/usr/bin/env python3
"""CPU enumeration of the LDS bank conflicts of the split GEMM's fragment reads (csrc/gemm_tile.h): 128-byte rows, ds_read_b128, the lane
groups of the hardware's LDS table -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- on the 16 columns of 16 bytes of the
256-byte bank row.  Prints the worst multiplicity per lane group for both lane maps on both swizzles, for the hi (lo = 0) and the lo
(lo = 1) chunk of a k group: 1 = conflict-free."""

GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
GROUPS += [[l + 32 for l in g] for g in GROUPS]


def swz32(r):          # the image of the 32x32x16 instances
    return (r >> 1) & 7


def swz16(r):          # gm_swz16
    return ((r >> 1) & 3) | (((((r & 15) + 4) >> 3) & 1) << 2)


def map32(lane, lo, ks=0):        # row li, chunk 2 (2 ks + hi) + lo
    return lane & 31, 2 * (2 * ks + (lane >> 5)) + lo


def map16(lane, lo, ks=0):        # row c, chunk 2 g + lo
    return lane & 15, 2 * (lane >> 4) + lo


def worst(lane_map, swz, lo):
    out = []
    for grp in GROUPS:
        cols = {}
        for lane in grp:
            r, k = lane_map(lane, lo)
            col = (r & 1) * 8 + (k ^ swz(r))
            cols[col] = cols.get(col, 0) + 1
        out.append(max(cols.values()))
    return out


if __name__ == "__main__":
    for mname, m in (("32x32x16 lane map", map32), ("16x16x32 lane map", map16)):
        for sname, s in (("(r >> 1) & 7", swz32), ("gm_swz16", swz16)):
            print("%s on %-13s lo=0 %s  lo=1 %s" % (mname, sname, worst(m, s, 0), worst(m, s, 1)))
    for r in range(16):
        assert sorted(cp ^ swz16(r) for cp in range(8)) == list(range(8))      # a permutation of the row's chunks: the DMA side fills every one
