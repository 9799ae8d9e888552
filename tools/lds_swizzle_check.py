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


# ---- the transposing read of the pack kernels (csrc/gemm.hip to_hl8_t_kernel, csrc/grad_pack.hip, csrc/half_pack.hip): a lane reads the 8
# rows of row group g at column c of a 128-row x 64-column fp32 tile, one ds_read_b32 per row: banks (dword address) mod 32, conflicts
# among the lanes of a 32-lane half.  The staging stores of half_pack are ds_write_b128: groups of 8 contiguous lanes, banks mod 32.
def padded_at(r, c):              # to_hl8_t_kernel / grad_pack_kernel: tile[128][65]
    return r * 65 + c


def padded_lanes(lane, it):       # unit u = tid + 256 it: g = u % 16, c = u / 16 (wave 0)
    return lane % 16, lane // 16 + 16 * it


def rotated_at(r, c):             # hp_at of half_pack.hip: the columns of a group of 8 rows rotated by 4 per group
    return r * 64 + ((c + 4 * ((r >> 3) & 7)) & 63)


def rotated_lanes(lane, it):      # half_pack_kernel (wave 0): 8 row groups x 4 columns per 32-lane half
    return (lane & 7) + 8 * (lane >> 5), 4 * (4 * it) + ((lane >> 3) & 3)


def worst_transposed_read(at, lanes):
    worst_of = 1
    for it in range(4):
        for e in range(8):
            for half in (range(0, 32), range(32, 64)):
                banks = {}
                for lane in half:
                    g, c = lanes(lane, it)
                    banks.setdefault(at(8 * g + e, c) % 32, set()).add(at(8 * g + e, c))
                worst_of = max(worst_of, max(len(v) for v in banks.values()))
    return worst_of


def worst_staging_store(swap):
    """ds_write_b128 of half_pack's staging: lane k writes the two 16-byte halves of (row k >> 3, column group k & 7); swap: the half
    (g >> 2) first.  Returns the worst number of different addresses on one bank within a group of 8 contiguous lanes."""
    worst_of = 1
    for first in (0, 1):
        for base in range(0, 64, 8):
            banks = {}
            for lane in range(base, base + 8):
                i, g = lane >> 3, lane & 7
                sw = (g >> 2) & 1 if swap else 0
                a = rotated_at(i, 8 * g + 4 * (sw if first == 0 else 1 - sw))
                for d in range(4):
                    banks.setdefault((a + d) % 32, set()).add(a + d)
            worst_of = max(worst_of, max(len(v) for v in banks.values()))
    return worst_of


# ---- csrc/patch_pack.hip on the same rotated tile.  PIXELS staging: a lane holds the 8 rows of row group g at column c (the lanes of
# half_pack's transposing read) and writes them with 8 ds_write_b32: banks mod 32 per 32-lane half.  Row read of PIXELS / GATHER: lane u
# reads the two 16-byte halves of (row u >> 3, column group u & 7) with ds_read_b128, the half ((row >> 1) & 1) first: 64 banks, the four
# lane groups of GROUPS.  GATHER staging: one ds_write_b32 per element in the order the map is walked (k = 2).
def worst_pixels_store():
    return worst_transposed_read(rotated_at, rotated_lanes)          # the same addresses, written instead of read


def worst_row_read(swap):
    worst_of = 1
    for it in range(4):
        for first in (0, 1):
            for grp in GROUPS:
                slots = {}
                for lane in grp:
                    u = lane + 256 * it
                    i, q = u >> 3, u & 7
                    sw = (i >> 1) & 1 if swap else 0
                    a = rotated_at(i, 8 * q + 4 * (sw if first == 0 else 1 - sw))
                    slots.setdefault((a // 4) % 16, set()).add(a)
                worst_of = max(worst_of, max(len(v) for v in slots.values()))
    return worst_of


def worst_gather_store(order, k):
    worst_of = 1
    k2 = k * k
    for base in range(0, 128 * 64, 32):
        banks = {}
        for u in range(base, base + 32):
            if order == 1:
                t = u // k
                r, c = t & 127, (t >> 7) * k + u % k
            else:
                ch = 64 // k2
                t = u // ch
                r, c = u >> 6, (u % ch) * k2 + t % k2
            a = rotated_at(r, c)
            banks.setdefault(a % 32, set()).add(a)
        worst_of = max(worst_of, max(len(v) for v in banks.values()))
    return worst_of


if __name__ == "__main__":
    print("patch_pack: PIXELS staging ds_write_b32 %d-way; row ds_read_b128 halves in order %d-way, half ((row >> 1) & 1) first %d-way; "
          "GATHER staging ds_write_b32, k = 2: NCHW order %d-way, channels-last order %d-way"
          % (worst_pixels_store(), worst_row_read(False), worst_row_read(True), worst_gather_store(1, 2), worst_gather_store(2, 2)))
    assert worst_pixels_store() == 1 and worst_row_read(True) == 1
    print("transposing ds_read_b32: tile[128][65] (to_hl8_t, grad_pack) %d-way, rotated tile (half_pack) %d-way"
          % (worst_transposed_read(padded_at, padded_lanes), worst_transposed_read(rotated_at, rotated_lanes)))
    print("half_pack staging ds_write_b128: halves in order %d-way, half (g >> 2) first %d-way" % (worst_staging_store(False), worst_staging_store(True)))
    assert worst_transposed_read(rotated_at, rotated_lanes) == 1 and worst_staging_store(True) == 1
    for mname, m in (("32x32x16 lane map", map32), ("16x16x32 lane map", map16)):
        for sname, s in (("(r >> 1) & 7", swz32), ("gm_swz16", swz16)):
            print("%s on %-13s lo=0 %s  lo=1 %s" % (mname, sname, worst(m, s, 0), worst(m, s, 1)))
    for r in range(16):
        assert sorted(cp ^ swz16(r) for cp in range(8)) == list(range(8))      # a permutation of the row's chunks: the DMA side fills every one
