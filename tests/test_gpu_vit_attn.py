"""The two ViT attention kernels with the decomposed relative-position bias computed in the kernel (hipie_amd/csrc/vit_attn.hip through
ops.vit_attn_rel, hipie_amd/csrc/vit_attn_split.hip through ops.vit_attn_split) against float64 references, over every launch line a
shipped build can reach.

Launch lines and a test id that reaches each (`launch_line` restates dispatch_va / dispatch_vs and the transposed swap, `lds_bytes`
restates launch_va / launch_sp / launch_vs; test_matrix_covers_every_instantiation enforces this table from the mirror):

  dispatch_va  win14    launch_va<T,HD,1,7,FAST,2,14,0>  kw == 14, kh <= 96       test_rel[win14-7x14-b1h3-hd80-bf16-exact-geometry], [win14-96x14-...]
               narrow   launch_va<T,HD,1,4,FAST,1,0,0>   kw <= 32                 test_rel[narrow-5x3-b1h3-hd64-f16-fast-geometry], [narrow-97x14-...] (the
                                                                                  fall-through from win14), [narrow-160x32-...]
               sp       launch_sp<T,HD,2,FAST,0>         33..64 wide, kh <= 96,   test_rel[sp-16x64-b2h4-hd80-f16-fast-geometry], [sp-32x33-...], [sp-17x61-...],
                                                         N >= 1024                [sp-96x64-...]
               plain64  launch_va<T,HD,2,4,FAST,1,0,0>   33..64 wide otherwise    test_rel[plain64-1x33-b2h4-hd64-f16-fast-geometry], [plain64-31x33-...] (N = 1023),
                                                                                  [plain64-97x40-...], [plain64-160x33-...]
               wide96   launch_va<T,HD,3,8,FAST,1,0,0>   65..96 wide              test_rel[wide96-1x65-b2h4-hd80-bf16-fast-geometry], [wide96-84x96-...]
               every line x {f16, bf16} x {64, 80} x {exact, FAST} (40)           test_rel[<line>-...-<value case>], six value cases each
               refused: kw > 96, kh > 160, hd 96, LDS > 160 KiB                   test_refusals
  dispatch_vs  win14    launch_vs<HD,1,7,2,14>           kw == 14, kh <= 96       test_split[win14-7x14-b1h3-hd64-hl8-lazy-geometry]
               narrow   launch_vs<HD,1,4,1,0>            kw <= 32                 test_split[narrow-160x32-b1h3-hd64-hl8-lazy-geometry]
               w8x2     launch_vs<HD,2,8,1,0>            33..64 wide, kh <= 64    test_split[w8x2-64x64-b1h3-hd64-hl8-lazy-geometry]
               w4x2     launch_vs<HD,2,4,1,0>            33..64 wide, kh > 64     test_split[w4x2-132x40-b3h1-hd80-hl8-lazy-geometry]
               slot96   launch_vs<HD,3,8,1,0,16>         65..96 wide              test_split[slot96-17x70-b1h3-hd80-hl8-lazy-geometry], [slot96-160x65-...]
  transposed   tr-narrow / tr-w4x2 / tr-slot96 (gw > 96, gh <= 96: kh = gw)       test_split[tr-narrow-2x97-...], [tr-narrow-14x128-...] (not win14),
                                                                                  [tr-w4x2-64x128-b1h1-...], [tr-w4x2-33x132-...], [tr-slot96-90x112-...]
               every line x {64, 80}                                              test_split[<line>-...-<value case>]
               refused: both sides > 96, gh > 160, hd 96, LDS > 160 KiB           test_refusals (33x160 is one of them: kh = 160 rows of a 4-wave
                                                                                  two-block instance need 172 KiB; vit_attn_split_ok says no as well)

Not reachable from a shipped build, hence not tested here: HIPIE_VA_MODE (the plain kernel on the sp geometry), HIPIE_VA_ABL (timing
ablations), HIPIE_VA_PRIO and HIPIE_VA_TRANSPOSE (the transposed walk forced on narrower grids) sit behind study_env, which compiles
them out without -DHIPIE_STUDY_KNOBS.  No environment variable is set by this file.

References, float64 on the values the kernel reads.  A problem holds the KERNEL's operands: q' = scale log2(e) q, tables' = R / scale
(tests/test_gpu_kernels.py::_fold_rel).  `ref_vit` unfolds them in float64 and materialises, per (b, h) and chunk of query rows,
    s[i,j] = scale q_i.k_j + q_i.Rh[yi - yj + gh - 1] + q_i.Rw[xi - xj + gw - 1],   softmax over j,   times v.
For ops.vit_attn_rel the 16-bit operands are rounded first, then upcast; for ops.vit_attn_split the reference takes the ORIGINAL fp32
values the HL8 pairs stand for.  `ref_loops` states the same in plain numpy loops over (b, h, i, j) for the tiny edge inputs;
test_references_agree checks the two to 1e-12 on the CPU.  On grids of more than 16 query blocks the reference covers whole 32-query
blocks only (the first two, the last two, eight random ones: the op is independent per query); the whole output must be finite.

Metric: `block_err` = max|got - ref| over a (batch, head, 32-query block) / max|ref| over the same block, the maximum over blocks.  A
32-query block is what a wave owns.  V is scaled per head by 1, 1/8, 8.

Bounds (tests/test_gpu_kernels.py): fp16 exact 1e-3, fp16 FAST 1.5e-3, bf16 8e-3 against float64 on the same rounded operands; split
4e-4 against float64 on the unrounded operands.  No bound comes from a kernel.  Attainability on the CPU: `emu_rel` (fp32 scores of the
rounded operands, P = exp2(s - max) rounded to T, fp32 PV and row sum, output rounded to T) and `emu_split` (three-product logits, P as
an fp16 pair, HL8 output) emulate the format choice only; test_emulation_within_half_bound asserts block_err <= bound / 2 on every case
and re-measures EMULATION_ERR (docs/measurements.md).  For that to hold per block in fp16 -- rounding the output alone costs up to
2^-11 = 4.9e-4 of a block's scale, and rounding P costs about as much again where a handful of keys carry a row (first_max on a 20-wide
grid) -- `settle` makes the last channel of V a constant c per (batch, head): the softmax weights sum to one, so that channel of the
output is c for every query, whatever the logits.  c = 1.9375 x a power of two, between two and four times the largest other |output|
m of the slice: c is the largest |reference| of every block, every other output lies a binade lower and rounds within 2^-12 / 1.9375 =
1.3e-4 of c.  What a block is measured by is therefore at most 4 m of its (batch, head) slice, never another head's magnitude; and a
row sum that is off (a dropped l_run rescale) shows on that channel at full size.

Value cases (one representative geometry per launch line; vit_attn_rel in f16 / bf16 x hd 64 / 80 x exact / FAST).  The inputs use the
thresholds read from the kernels (DEFER = 8 in vit_attn.hip, VS_LAZY = 6 in vit_attn_split.hip; 0 in exact mode, which the same inputs
cross a fortiori); the bounds do not.  Steps between key tiles are q'[0] x k[0] with both factors exact in bf16 and column 0 of the
tables zero, so they survive the rounding; test_value_inputs_have_their_properties asserts each property on the operands as read.
  random        logits of natural size
  stairs_over   every row's maximum rises by threshold + 0.5 from key tile to key tile: the cold path runs at every tile (of the first 17;
                a grid with more stays at that level: fp32 sums of logits beyond 2^8 cost the split bound in the emulation already)
  stairs_under  it rises once, by threshold - 0.5, and stays: the reference point stays put, P reaches ~2^threshold
  late_jump     flat logits, then ONE key of a tile in the second half exceeds the reference by threshold + 0.5 for 5 of a wave's 32 rows;
                the keys before it keep >= 10 % of those rows' mass, so a wrong rescale of O or of the row sum shows
  first_max     the maximum sits in tile 0, every later tile lies more than 150 below it: exp2 gives zero in fp32
  one_hot       per query one key at a pseudo-random position dominates by more than 40 (log2): the output is that key's v row; the
                positions include the first and last slot of a tile, the last key of the walk and the slot next to a tile's padding

Output buffers: `poisoned` frees a NaN-filled block of the output's size before every call through ops.*; test_guarded_output calls the C
entry through ops._call (as tests/test_gpu_grad_scale.py does) with `out` in the middle of a sentinel-filled buffer, 256 rows of guard
on both sides, for one ragged case per launch line.  Batch invariance is bit for bit: a (batch, head) pair is computed by its own
workgroups in the same order whatever the batch; B = 3 cannot switch the batch/head swizzle (3 H % 8 == 0 iff H % 8 == 0), so the
swizzle on / off pair is B = 2 against B = 1 at 4 heads, next to B = 3 against B = 1."""
import collections
import functools
import itertools
import math
import zlib

import numpy as np
import pytest
import torch

torch.set_grad_enabled(False)
DEV = "cuda"
gpu = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
DTS = (F16, BF16)
NAME = {F16: "f16", BF16: "bf16", torch.float32: "hl8"}
LOG2E = 1.4426950408889634
V_SCALE = (1.0, 0.125, 8.0)                 # per head, cycled
OUT_MANTISSA = 1.9375
THRESHOLD = {"rel": 8.0, "split": 6.0}      # DEFER (vit_attn.hip, FAST), VS_LAZY (vit_attn_split.hip): used by the inputs only
VALUES = ("random", "stairs_over", "stairs_under", "late_jump", "first_max", "one_hot")
JUMP_ROWS = (1, 5, 6, 17, 30)               # late_jump: the rows of every 32-query block that jump
STAIRS = 16                                 # stairs_over: steps (the logits stay below 2^8: fp32 sums of larger ones lose the split bound)
ONE_HOT_GAIN = 24.0                         # one_hot: a differing code bit costs 2 x 24 = 48 in log2
LDS_LIMIT = 160 * 1024


def bound(entry, dt, fast):
    if entry == "split":
        return 4e-4
    return 8e-3 if dt == BF16 else 1.5e-3 if fast else 1e-3


# Largest block_err of emu_rel / emu_split against the float64 reference per (entry point, operand type, value case; "geometry" = the
# geometry matrix on random values), measured on the CPU by test_emulation_within_half_bound, which re-measures them: each must stay at or
# below its entry and above half of it; the entries are the measured values plus 1 %.  Half of the bound is 5e-4 (fp16, exact mode),
# 4e-3 (bf16), 2e-4 (split).  An entry of 1e-12 stands for "exact" (one_hot: P is 1 or 0, the output is a v row; what is left is the float64
# reference's own rounding) and is checked from above only.
EMULATION_ERR = {
    ("rel", "f16", "geometry"): 0.000174, ("rel", "bf16", "geometry"): 0.00159, ("rel", "f16", "random"): 0.00016, ("rel", "bf16", "random"): 0.00158,
    ("rel", "f16", "stairs_over"): 0.00022, ("rel", "bf16", "stairs_over"): 0.00196, ("rel", "f16", "stairs_under"): 0.000229, ("rel", "bf16", "stairs_under"): 0.0018,
    ("rel", "f16", "late_jump"): 0.000133, ("rel", "bf16", "late_jump"): 0.00105, ("rel", "f16", "first_max"): 0.000254, ("rel", "bf16", "first_max"): 0.00205,
    ("rel", "f16", "one_hot"): 1e-12, ("rel", "bf16", "one_hot"): 1e-12, ("split", "hl8", "geometry"): 2.42e-05, ("split", "hl8", "random"): 6.96e-06,
    ("split", "hl8", "stairs_over"): 1.33e-05, ("split", "hl8", "stairs_under"): 2.55e-06, ("split", "hl8", "late_jump"): 1.65e-06, ("split", "hl8", "first_max"): 4.97e-07,
    ("split", "hl8", "one_hot"): 3.11e-08,
}


# ------------------------------------------------------------------------------------------------------ mirror of the dispatch
LINES = {"rel": ("win14", "narrow", "sp", "plain64", "wide96"), "split": ("win14", "narrow", "w8x2", "w4x2", "slot96")}
TR_LINES = ("tr-narrow", "tr-w4x2", "tr-slot96")
# line -> (NB, WAVES, R, BHC) of its instantiation
INST = {"rel": {"win14": (1, 7, 2, 0), "narrow": (1, 4, 1, 0), "sp": (2, 8, 1, 0), "plain64": (2, 4, 1, 0), "wide96": (3, 8, 1, 0)},
        "split": {"win14": (1, 7, 2, 0), "narrow": (1, 4, 1, 0), "w8x2": (2, 8, 1, 0), "w4x2": (2, 4, 1, 0), "slot96": (3, 8, 1, 16)}}


def kernel_grid(entry, gh, gw):
    """(kh, kw, transposed) as the kernel sees them: hipie_vit_attn_split walks grids wider than 96 and at most 96 high column by column"""
    if entry == "split" and gw > 96 and gh <= 96:
        return gw, gh, True
    return gh, gw, False


def launch_line(entry, gh, gw, hd, dtype=F16, fast=False):
    """the launch line of hipie_vit_attn_rel (dispatch_va) / hipie_vit_attn_split (dispatch_vs) for a grid, None where the entry refuses
    before it looks at LDS; `fast` selects a template argument of the same line"""
    if hd not in (64, 80) or gh < 1 or gw < 1 or gh > 160 or dtype not in ((F16, BF16) if entry == "rel" else (F16, torch.float32)):
        return None
    kh, kw, tr = kernel_grid(entry, gh, gw)
    if kw == 14 and kh <= 96:
        line = "win14"
    elif kw <= 32:
        line = "narrow"
    elif entry == "rel":
        line = "sp" if (kw <= 64 and kh <= 96 and kh * kw >= 1024) else "plain64" if kw <= 64 else "wide96" if kw <= 96 else None
    else:
        line = "w8x2" if (kw <= 64 and kh <= 64) else "w4x2" if kw <= 64 else "slot96" if kw <= 96 else None
    return None if line is None else ("tr-" + line if tr else line)


def lds_bytes(entry, line, kh, hd):
    """dynamic LDS of launch_va / launch_sp / launch_vs for kh key rows (the kernel's, after the transposed swap)"""
    line = line[3:] if line.startswith("tr-") else line
    NB, WAVES, _, BHC = INST[entry][line]
    KT, DB = 32 * NB, (hd + 31) // 32
    KSTR = hd + 8
    VSTR = DB * 32 if DB * 32 in (96, 32) else DB * 32 + 32
    KBLK, VBLK = (KT * (KSTR // 8) + 63) // 64, (KT * (VSTR // 8) + 63) // 64
    stage = WAVES * 32 * 32 * 4
    if entry == "split":
        return max(2 * (2 * KBLK + 2 * VBLK) * 1024, stage) + (BHC if BHC > 0 else kh) * WAVES * 32 * 4
    if line == "sp":
        return max((3 * KBLK + 2 * VBLK) * 1024, stage) + (kh + 1) * WAVES * 32 * 4
    return max(2 * KT * (KSTR + VSTR) * 2, stage) + kh * WAVES * 32 * 4


def first_over_lds(entry, line, hd):
    """the smallest number of key rows at which the line exceeds 160 KiB of LDS, None if it never does within the rows it is given"""
    most = 96 if line in ("win14", "sp") else 64 if line == "w8x2" else 160
    return next((kh for kh in range(1, most + 1) if lds_bytes(entry, line, kh, hd) > LDS_LIMIT), None)


def key_tiles(entry, gh, gw):
    """per key (memory token index): its key tile and its slot inside the tile in the kernel's walk -> (tiles (N,), slots (N,), ntiles)"""
    line = launch_line(entry, gh, gw, 80)
    j = torch.arange(gh * gw)
    if line.startswith("tr-"):
        return j % gw, j // gw, gw
    R = INST[entry][line][2]
    tiles = (j // gw) // R
    return tiles, j - tiles * R * gw, (gh + R - 1) // R


# --------------------------------------------------------------------------------------------------------------- references
Problem = collections.namedtuple("Problem", "entry q k v th tw gh gw scale")     # q (the kernel's q'), k, v: (B, N, H, hd); th, tw: tables'


def _logits(q, k, th, tw, gh, gw, ii, qk_scale=1.0):
    """qk_scale q_i.k_j + q_i.th[yi - yj + gh - 1] + q_i.tw[xi - xj + gw - 1] for the query rows ii -> (B, H, len(ii), N), in q's type"""
    B, N, H, hd = q.shape
    qi = q[:, ii]
    s = torch.einsum("bihd,bjhd->bhij", qi, k) * qk_scale
    bh = torch.einsum("bihd,rd->bhir", qi, th).gather(3, ((ii // gw)[:, None] - torch.arange(gh)[None, :] + gh - 1).expand(B, H, -1, -1))
    bw = torch.einsum("bihd,rd->bhir", qi, tw).gather(3, ((ii % gw)[:, None] - torch.arange(gw)[None, :] + gw - 1).expand(B, H, -1, -1))
    return (s.view(B, H, len(ii), gh, gw) + bh[..., :, None] + bw[..., None, :]).reshape(B, H, len(ii), N)


def unfolded(p):
    """float64 (q, k, v, Rh, Rw) the kernel's operands stand for: q = q' / (scale log2 e), R = tables' x scale"""
    return p.q.double() / (p.scale * LOG2E), p.k.double(), p.v.double(), p.th.double() * p.scale, p.tw.double() * p.scale


def all_rows(p):
    return torch.arange(p.q.shape[1])


def chunks(p, idx, budget=6000000):
    B, N, H, _ = p.q.shape
    step = max(1, budget // (B * H * N))
    return [idx[s:s + step] for s in range(0, len(idx), step)]


def ref_vit(p, idx=None):
    """float64 reference for the query rows idx (all by default) -> (B, len(idx), H, hd)"""
    q, k, v, Rh, Rw = unfolded(p)
    out = []
    for ii in chunks(p, all_rows(p) if idx is None else idx):
        s = _logits(q, k, Rh, Rw, p.gh, p.gw, ii, p.scale)
        w = torch.exp(s - s.amax(-1, keepdim=True))
        out.append(torch.einsum("bhij,bjhd->bihd", w / w.sum(-1, keepdim=True), v))
    return torch.cat(out, 1)


def ref_loops(p):
    """the formula of the header of vit_attn.hip written out: one loop iteration per (b, h, i, j), numpy float64"""
    q, k, v, Rh, Rw = (t.numpy() for t in unfolded(p))
    B, N, H, hd = q.shape
    out = np.zeros((B, N, H, hd))
    for b, h, i in itertools.product(range(B), range(H), range(N)):
        s = np.zeros(N)
        for j in range(N):
            yi, xi, yj, xj = i // p.gw, i % p.gw, j // p.gw, j % p.gw
            s[j] = p.scale * float(np.dot(q[b, i, h], k[b, j, h])) + float(np.dot(q[b, i, h], Rh[yi - yj + p.gh - 1])) \
                + float(np.dot(q[b, i, h], Rw[xi - xj + p.gw - 1]))
        w = np.exp(s - s.max())
        out[b, i, h] = (w[:, None] * v[b, :, h]).sum(0) / w.sum()
    return torch.from_numpy(out)


def scores2(p, ii):
    """float64 logits in the log2 domain of the operands AS READ (16-bit rounded; for split the fp16 pairs) -> (B, H, len(ii), N)"""
    q, k, th, tw = ((pair(t)[0].double() + pair(t)[1].double()) if p.entry == "split" else t.double() for t in (p.q, p.k, p.th, p.tw))
    return _logits(q, k, th, tw, p.gh, p.gw, ii)


def pair(x):
    """fp32 -> the fp16 pair (hi, lo) of the HL8 layout, as fp32"""
    hi = x.float().clamp(-65504.0, 65504.0).half()
    return hi.float(), (x.float() - hi.float()).half().float()


def emu_rel(p, idx):
    """CPU emulation of vit_attn.hip's format choice (not of its order of operations): fp32 scores from the rounded operands, P = exp2(s -
    max) rounded to the operand type, fp32 PV, division by the fp32 sum of the unrounded P, output rounded to the operand type"""
    dt = p.q.dtype
    q, k, v, th, tw = (t.float() for t in (p.q, p.k, p.v, p.th, p.tw))
    out = []
    for ii in chunks(p, idx):
        s = _logits(q, k, th, tw, p.gh, p.gw, ii)
        w = torch.exp2(s - s.amax(-1, keepdim=True))
        o = torch.einsum("bhij,bjhd->bihd", w.to(dt).float(), v) / w.sum(-1).permute(0, 2, 1)[..., None]
        out.append(o.to(dt).double())
    return torch.cat(out, 1)


def emu_split(p, idx):
    """CPU emulation of vit_attn_split.hip's format choice: every logit term as a_lo.b_hi + a_hi.b_lo + a_hi.b_hi in fp32 from the fp16
    pairs, P = exp2(s - max) as an fp16 pair, O = V_hi.(P_hi + P_lo) + V_lo.P_hi in fp32, fp32 sum of the unrounded P, an HL8 output"""
    (qh, ql), (kh, kl), (vh, vl), (hh, hl), (wh, wl) = (pair(t) for t in (p.q, p.k, p.v, p.th, p.tw))
    out = []
    for ii in chunks(p, idx):
        s = _logits(ql, kh, hh, wh, p.gh, p.gw, ii) + _logits(qh, kl, hl, wl, p.gh, p.gw, ii) + _logits(qh, kh, hh, wh, p.gh, p.gw, ii)
        w = torch.exp2(s - s.amax(-1, keepdim=True))
        ph, pl = pair(w)
        o = torch.einsum("bhij,bjhd->bihd", ph + pl, vh) + torch.einsum("bhij,bjhd->bihd", ph, vl)
        oh, ol = pair(o / w.sum(-1).permute(0, 2, 1)[..., None])
        out.append(oh.double() + ol.double())
    return torch.cat(out, 1)


def block_err(got, want):
    """max over (batch, head, 32-query block) of max|got - want| / max|want| of the block; got, want (B, n, H, hd) with n a run of whole
    blocks (the last one may be ragged).  Non-finite values fail; a block whose reference is all zero must be exactly zero"""
    got, want = got.detach().cpu().double().reshape(want.shape), want.double()
    assert bool(torch.isfinite(got).all()), "non-finite output (an element the kernel did not write reads NaN)"
    B, n, H, hd = want.shape
    npad = -(-n // 32) * 32
    d, r = torch.zeros(B, npad, H, hd, dtype=torch.float64), torch.zeros(B, npad, H, hd, dtype=torch.float64)
    d[:, :n], r[:, :n] = (got - want).abs(), want.abs()
    d, r = d.view(B, npad // 32, 32, H, hd).amax((2, 4)), r.view(B, npad // 32, 32, H, hd).amax((2, 4))
    dead = r == 0
    assert bool((d[dead] == 0).all()), "a block whose reference is all zero must be exactly zero"
    return float((d[~dead] / r[~dead]).max()) if bool((~dead).any()) else 0.0


# ------------------------------------------------------------------------------------------------------------------- inputs
def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def head_scaled(v):
    """(B,N,H,hd) values with the per-head scale 1, 1/8, 8"""
    return v * torch.tensor([V_SCALE[h % 3] for h in range(v.shape[2])]).view(1, 1, -1, 1)


def some_blocks(N, g, n=8):
    """query rows of whole 32-query blocks: all of a grid of up to 16 blocks; else the first two, the last two and n random ones"""
    nb = (N + 31) // 32
    if nb <= 16:
        return torch.arange(N)
    blocks = sorted({0, 1, nb - 2, nb - 1} | {2 + int(b) for b in torch.randperm(nb - 4, generator=g)[:n]})
    return torch.cat([torch.arange(32 * b, min(32 * b + 32, N)) for b in blocks])


def settle(p, idx):
    """-> (problem, float64 reference on idx) with the last channel of V the per-(batch, head) constant c = OUT_MANTISSA x 2^k in [2 m,
    4 m), m the largest other |reference| of the slice (see the module docstring); that channel of the reference is c"""
    want = ref_vit(p, idx)
    m = want[..., :-1].abs().amax((1, 3)).clamp_min(1e-30)                                  # (B, H)
    c = OUT_MANTISSA * torch.exp2(torch.ceil(torch.log2(m / OUT_MANTISSA)) + 1)
    v = p.v.clone()
    v[..., -1] = c[:, None, :].to(v.dtype)
    assert torch.equal(v[..., -1].double(), c[:, None, :].expand(v.shape[:3]))
    want[..., -1] = c[:, None, :]
    return p._replace(v=v), want


Case = collections.namedtuple("Case", "entry line gh gw B H hd dt fast value")


def case_id(c):
    return "%s-%dx%d-b%dh%d-hd%d-%s-%s-%s" % (c.line, c.gh, c.gw, c.B, c.H, c.hd, NAME[c.dt],
                                              "lazy" if c.entry == "split" else "fast" if c.fast else "exact", c.value)


def special_keys(tiles, slots, nt):
    """one_hot: the first slot of tile 0, the last slot of tile 0 (next to the tile's padding when the tile is not full), the first slot of
    the second tile, and the last key of the walk (the last slot of the last tile; next to the padding of a ragged last tile)"""
    def key(t, last):
        cand = torch.nonzero(tiles == t).flatten()
        return int(cand[slots[cand].argmax() if last else slots[cand].argmin()])
    return [key(0, False), key(0, True), key(min(1, nt - 1), False), key(nt - 1, True)]


@functools.lru_cache(maxsize=None)
def _problem(entry, gh, gw, B, H, hd, dt, value):
    g = gen("%s-%dx%d-b%dh%d-hd%d-%s-%s" % (entry, gh, gw, B, H, hd, NAME[dt], value))
    N, scale, thr = gh * gw, hd ** -0.5, THRESHOLD[entry]
    tiles, slots, nt = key_tiles(entry, gh, gw)

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    if value in ("random", "geometry"):
        sd = 0.8 if entry == "rel" else 1.6            # split: |q.k| up to ~25, a single-fp16 q or k would move P by 1e-2
        q, k = rn(B, N, H, hd) * (sd * scale * LOG2E), rn(B, N, H, hd) * sd
        th, tw = rn(2 * gh - 1, hd) * (0.2 / scale), rn(2 * gw - 1, hd) * (0.2 / scale)
    else:
        # small noise of standard deviation ~0.05 (one_hot: ~0.17) in log2 units; the structure sits in exact columns of q' and k
        q, k = rn(B, N, H, hd) * ((0.1 if value == "one_hot" else 0.03) / math.sqrt(hd)), rn(B, N, H, hd)
        th, tw = rn(2 * gh - 1, hd), rn(2 * gw - 1, hd)
        if value == "one_hot":
            L = max(1, (N - 1).bit_length())
            code = ((torch.arange(N)[:, None] >> torch.arange(L)[None, :]) & 1).float() * 2 - 1           # (N, L) of +-1
            pos = torch.randint(0, N, (B, H, N), generator=g)
            sp = torch.tensor(special_keys(tiles, slots, nt))
            pos[:, :, :8], pos[:, :, N - 4:] = sp.repeat(2), sp                   # in the first and in the last (ragged) query block
            k[..., 1:1 + L] = code[None, :, None, :]
            q[..., 1:1 + L] = ONE_HOT_GAIN * code[pos].permute(0, 2, 1, 3)
            th[:, 1:1 + L], tw[:, 1:1 + L] = 0.0, 0.0
        else:
            assert nt >= 4
            th[:, 0], tw[:, 0] = 0.0, 0.0
            if value == "stairs_over":
                a, step = torch.full((N,), thr + 0.5), tiles.clamp_max(STAIRS).float()
            elif value == "stairs_under":
                a, step = torch.full((N,), thr - 0.5), tiles.clamp_max(1).float()
            elif value == "first_max":
                a, step = torch.full((N,), thr + 0.5), -32.0 * tiles.clamp_max(1).float()
            elif value == "late_jump":
                a = torch.isin(torch.arange(N) % 32, torch.tensor(JUMP_ROWS)).float() * (thr + 0.5)
                cand = torch.nonzero(tiles == (3 * nt) // 4).flatten()
                step = torch.zeros(N)
                step[cand[slots[cand].argsort()[len(cand) // 2]]] = 1.0
            else:
                raise ValueError(value)
            q[..., 0], k[..., 0] = a[None, :, None], step[None, :, None]
    v = head_scaled(rn(B, N, H, hd))
    if entry == "rel":
        q, k, v, th, tw = (t.to(dt) for t in (q, k, v, th, tw))
    idx = some_blocks(N, g)
    p, want = settle(Problem(entry, q, k, v, th, tw, gh, gw, scale), idx)
    return p, idx, want


def problem(c):
    """-> (problem, the query rows the reference covers, float64 reference): the same for exact and FAST"""
    return _problem(c.entry, c.gh, c.gw, c.B, c.H, c.hd, c.dt, c.value)


# ---- the matrices ----
REL_GEOMETRY = {
    "win14": ((14, 14), (7, 14), (1, 14), (17, 14), (96, 14)),
    "narrow": ((1, 1), (5, 3), (32, 32), (97, 14), (160, 32)),
    "sp": ((16, 64), (32, 33), (17, 61), (96, 64)),
    "plain64": ((1, 33), (15, 64), (31, 33), (97, 40), (160, 33)),
    "wide96": ((1, 65), (3, 70), (84, 96))}
SPLIT_GEOMETRY = {
    "win14": ((14, 14), (7, 14), (1, 14), (17, 14), (96, 14)),
    "narrow": ((1, 1), (5, 3), (32, 32), (97, 14), (160, 32)),
    "w8x2": ((1, 33), (64, 64), (33, 50)),
    "w4x2": ((65, 33), (132, 40)),
    "slot96": ((1, 65), (17, 70), (160, 65)),
    "tr-narrow": ((2, 97), (14, 128), (32, 160)),
    "tr-w4x2": ((33, 132), (64, 128)),
    "tr-slot96": ((90, 112),)}
# the representative grid of a line for the value cases: small, at least four key tiles, more than one query block
VALUE_GRID = {"rel": {"win14": (14, 14), "narrow": (9, 20), "sp": (26, 40), "plain64": (12, 40), "wide96": (10, 70)},
              "split": {"win14": (14, 14), "narrow": (9, 20), "w8x2": (12, 40), "w4x2": (65, 33), "slot96": (18, 70), "tr-narrow": (5, 97)}}


def _batch_heads(i, N, grid):
    """B, heads of the i-th geometry case of a line: 8 (swizzle on) and 3 (off) alternate on the smaller grids; the large ones keep 3"""
    if grid == (64, 128):
        return 1, 1
    return ((2, 4), (1, 3))[i % 2] if N <= 4400 else ((1, 3), (3, 1))[i % 2]


def _geometry_cases(entry):
    out, n = [], 0
    for line, grids in (REL_GEOMETRY if entry == "rel" else SPLIT_GEOMETRY).items():
        for i, (gh, gw) in enumerate(grids):
            B, H = _batch_heads(i, gh * gw, (gh, gw))
            dt, fast, hd = (DTS[n % 2], n % 4 >= 2, (80, 64)[(n // 4) % 2]) if entry == "rel" else (torch.float32, False, (80, 64)[n % 2])
            out.append(Case(entry, line, gh, gw, B, H, hd, dt, fast, "geometry"))
            n += 1
    return out


def _value_cases(entry):
    out = []
    for line, (gh, gw) in VALUE_GRID[entry].items():
        for hd, value in itertools.product((64, 80), VALUES):
            if entry == "rel":
                out += [Case(entry, line, gh, gw, 1, 3, hd, dt, fast, value) for dt in DTS for fast in (False, True)]
            else:
                out.append(Case(entry, line, gh, gw, 1, 3, hd, torch.float32, False, value))
    return out


REL = _geometry_cases("rel") + _value_cases("rel")
SPLIT = _geometry_cases("split") + _value_cases("split")
# one ragged geometry case per launch line for the guarded output buffer
GUARDED = [next(c for c in REL + SPLIT if (c.entry, c.line, c.gh, c.gw) == key) for key in (
    ("rel", "win14", 7, 14), ("rel", "narrow", 5, 3), ("rel", "sp", 17, 61), ("rel", "plain64", 31, 33), ("rel", "wide96", 3, 70),
    ("split", "win14", 7, 14), ("split", "narrow", 5, 3), ("split", "w8x2", 33, 50), ("split", "w4x2", 65, 33), ("split", "slot96", 17, 70),
    ("split", "tr-narrow", 2, 97), ("split", "tr-w4x2", 33, 132), ("split", "tr-slot96", 90, 112))]


def refusal_cases():
    """(entry, gh, gw, hd, what the message must name): every refusal of the two entry points, the LDS ones taken from the mirror"""
    out = [("rel", 2, 97, 80, "wider than 96"), ("split", 97, 97, 80, "wider than 96"), ("rel", 161, 4, 80, "160 key rows"),
           ("split", 161, 4, 80, "160 key rows"), ("rel", 4, 4, 96, "head_dim"), ("split", 4, 4, 96, "head_dim")]
    for entry, line, gw in (("rel", "wide96", 65), ("split", "w4x2", 33)):
        for hd in (64, 80):
            out.append((entry, first_over_lds(entry, line, hd), gw, hd, "LDS"))
    out += [("split", 33, first_over_lds("split", "w4x2", 80), 80, "LDS"), ("split", 33, 160, 80, "LDS")]        # transposed: kh = gw
    return out


# ---- tiny inputs for the two references ----
def edge_problems():
    g = gen("edges")
    for name, gh, gw in (("plain", 3, 4), ("one_token", 1, 1), ("one_row", 1, 5), ("one_column", 4, 1), ("rect", 2, 3)):
        B, H, hd, N = 2, 2, 4, gh * gw
        q, k = (torch.randn(B, N, H, hd, generator=g).to(BF16) for _ in range(2))
        v = head_scaled(torch.randn(B, N, H, hd, generator=g)).to(BF16)
        th, tw = (torch.randn(2 * n - 1, hd, generator=g).to(BF16) for n in (gh, gw))
        yield name, Problem("rel", q, k, v, th, tw, gh, gw, 0.5)


# -------------------------------------------------------------------------------------- CPU: references, inputs, bounds (no GPU)
def test_references_agree():
    for name, p in edge_problems():
        a, b = ref_vit(p), ref_loops(p)
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
        if name == "one_token":
            assert torch.equal(a, p.v.double())
        # the constant channel of `settle` comes out as the constant, and the other channels do not move
        p2, want = settle(p, all_rows(p))
        c = p2.v[:, :1, :, -1].double()
        assert float((ref_loops(p2)[..., -1] - c).abs().max()) <= 1e-12 * float(c.max()) and torch.equal(want[..., -1], c.expand(want.shape[:3]))
        assert float((ref_loops(p2)[..., :-1] - a[..., :-1]).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
        m = a[..., :-1].abs().amax((1, 3))[:, None, :]
        assert bool((c >= 2 * m).all()) and bool((c < 4 * m).all())


def test_mirror_admits_what_ok_admits():
    """wherever ops.vit_attn_rel_ok / ops.vit_attn_split_ok say yes, the dispatch has a launch line that fits 160 KiB of LDS: what
    modeling/vit.py relies on when it routes without a fallback.  And the LDS limits the mirror finds are the ones the refusals use"""
    from hipie_amd import ops
    for entry, ok in (("rel", ops.vit_attn_rel_ok), ("split", ops.vit_attn_split_ok)):
        for hd, gh, gw in itertools.product((64, 80), range(1, 171), range(1, 171)):
            if ok((gh, gw), hd):
                line = launch_line(entry, gh, gw, hd)
                assert line is not None, (entry, gh, gw, hd)
                assert lds_bytes(entry, line, kernel_grid(entry, gh, gw)[0], hd) <= LDS_LIMIT, (entry, gh, gw, hd, line)
        assert not ok((8, 8), 96) and not ok((161, 8), 80)
    assert (first_over_lds("rel", "wide96", 80), first_over_lds("rel", "wide96", 64)) == (92, 98)
    assert (first_over_lds("split", "w4x2", 80), first_over_lds("split", "w4x2", 64)) == (137, 153)
    assert all(first_over_lds(e, line, hd) is None for e in LINES for line in LINES[e] for hd in (64, 80)
               if (e, line) not in (("rel", "wide96"), ("split", "w4x2")))
    for entry, gh, gw, hd, _ in refusal_cases():
        line = launch_line(entry, gh, gw, hd)
        assert line is None or lds_bytes(entry, line, kernel_grid(entry, gh, gw)[0], hd) > LDS_LIMIT, (entry, gh, gw, hd)
        assert not (ops.vit_attn_rel_ok if entry == "rel" else ops.vit_attn_split_ok)((gh, gw), hd)


def test_matrix_covers_every_instantiation():
    from hipie_amd import ops
    for c in REL + SPLIT:
        assert launch_line(c.entry, c.gh, c.gw, c.hd, c.dt, c.fast) == c.line, case_id(c)
        assert lds_bytes(c.entry, c.line, kernel_grid(c.entry, c.gh, c.gw)[0], c.hd) <= LDS_LIMIT, case_id(c)
        assert (ops.vit_attn_rel_ok if c.entry == "rel" else ops.vit_attn_split_ok)((c.gh, c.gw), c.hd), case_id(c)
    rel = {(c.line, c.dt, c.hd, c.fast) for c in REL}
    assert rel == set(itertools.product(LINES["rel"], DTS, (64, 80), (False, True))) and len(rel) == 40
    for value in VALUES:                      # and each of the 40 on every value case
        assert {(c.line, c.dt, c.hd, c.fast) for c in REL if c.value == value} == rel
    assert {(c.line, c.hd) for c in SPLIT if not c.line.startswith("tr-")} == set(itertools.product(LINES["split"], (64, 80)))
    assert {c.line for c in SPLIT if c.line.startswith("tr-")} == set(TR_LINES)
    for value in VALUES:
        assert {(c.line, c.hd) for c in SPLIT if c.value == value} == set(itertools.product(LINES["split"] + ("tr-narrow",), (64, 80)))
    for cases in (REL, SPLIT):                # per line: the batch/head swizzle on and off (tr-slot96 has one grid)
        for line in {c.line for c in cases} - {"tr-slot96"}:
            assert {c.B * c.H % 8 == 0 for c in cases if c.line == line and c.value == "geometry"} == {True, False}, line
    assert {(c.line, c.gh, c.gw) for c in REL if c.value == "geometry"} == {(ln, a, b) for ln, gs in REL_GEOMETRY.items() for a, b in gs}
    assert {(c.line, c.gh, c.gw) for c in SPLIT if c.value == "geometry"} == {(ln, a, b) for ln, gs in SPLIT_GEOMETRY.items() for a, b in gs}
    assert len({case_id(c) for c in REL + SPLIT}) == len(REL + SPLIT)
    assert {(c.entry, c.line) for c in GUARDED} == {(e, ln) for e in LINES for ln in LINES[e]} | {("split", ln) for ln in TR_LINES}
    # the neighbours the issue names: 31x33 has 1023 tokens and takes plain64 next to 32x33 on sp; 14x128 lands on narrow, not on win14
    assert launch_line("rel", 31, 33, 80) == "plain64" and launch_line("rel", 32, 33, 80) == "sp" and launch_line("split", 14, 128, 80) == "tr-narrow"


def value_problems():
    seen = {}
    for c in REL + SPLIT:
        if c.value != "geometry":
            seen.setdefault((c.entry, c.gh, c.gw, c.B, c.H, c.hd, c.dt, c.value), c)
    return list(seen.values())


def tile_maxima(p, idx, tiles, nt):
    """(B, H, len(idx), ntiles) float64: the row maximum per key tile, log2 domain, of the operands as read"""
    s = scores2(p, idx)
    tm = torch.full(s.shape[:3] + (nt,), -math.inf, dtype=torch.float64)
    return tm.scatter_reduce_(3, tiles.expand_as(s).contiguous(), s, "amax"), s


def test_value_inputs_have_their_properties():
    """each value case has the property its name claims, on the operands as the kernel reads them, for every query row the reference
    covers.  1/16 of slack wherever a threshold is crossed or kept: the sp kernel keeps its reference point on a 1/16 grid"""
    for c in value_problems():
        if c.value == "random":
            continue
        p, idx, _ = problem(c)
        thr, name = THRESHOLD[c.entry], case_id(c)
        tiles, slots, nt = key_tiles(c.entry, c.gh, c.gw)
        tm, s = tile_maxima(p, idx, tiles, nt)
        run = torch.cummax(tm, 3).values
        if c.value == "stairs_over":
            assert float((tm[..., 1:STAIRS + 1] - run[..., :min(STAIRS, nt - 1)]).min()) > thr + 0.0625, name
            assert nt <= STAIRS + 1 or float((tm[..., STAIRS + 1:] - tm[..., STAIRS:STAIRS + 1]).abs().max()) < 1, name
        elif c.value == "stairs_under":
            rise = tm[..., 1:] - tm[..., :1]
            assert thr - 1 < float(rise.min()) and float(rise.max()) < thr - 0.0625, name
        elif c.value == "first_max":
            assert float((tm[..., 1:] - tm[..., :1]).max()) < -150, name
        elif c.value == "late_jump":
            tj = (3 * nt) // 4
            rows = torch.isin(idx % 32, torch.tensor(JUMP_ROWS))
            assert 2 * tj >= nt and 0 < int(rows.sum()) < len(idx)
            assert float((tm[:, :, rows, tj] - run[:, :, rows, tj - 1]).min()) > thr + 0.0625, name
            assert float((tm[:, :, ~rows][..., 1:] - tm[:, :, ~rows][..., :1]).abs().max()) < 1 and float((run[:, :, rows, tj - 1] - tm[:, :, rows, 0]).max()) < 1
            w = torch.exp2(s - s.amax(-1, keepdim=True))
            share = (w * (tiles < tj)).sum(-1) / w.sum(-1)
            assert float(share[:, :, rows].min()) >= 0.10, (name, float(share[:, :, rows].min()))
        elif c.value == "one_hot":
            top = s.topk(2, -1)
            assert float((top.values[..., 0] - top.values[..., 1]).min()) > 40, name
            pos = top.indices[..., 0]
            want_keys = special_keys(tiles, slots, nt)
            assert all(bool((pos == key).any()) for key in want_keys), name
            R, kw = INST[c.entry][c.line.replace("tr-", "")][2], kernel_grid(c.entry, c.gh, c.gw)[1]
            assert int(slots[want_keys[0]]) == 0 and int(slots[want_keys[2]]) == 0 and int(tiles[want_keys[2]]) == 1
            assert int(slots[want_keys[1]]) == R * kw - 1 and int(tiles[want_keys[3]]) == nt - 1
            assert int(slots[want_keys[3]]) == (c.gh * c.gw - (nt - 1) * R * kw if R > 1 else kw) - 1
            assert len(torch.unique(pos)) > min(c.gh * c.gw, len(idx)) // 4


def emulation_groups(entry):
    groups = collections.defaultdict(dict)
    for c in (REL if entry == "rel" else SPLIT):
        groups[entry, NAME[c.dt], c.value].setdefault((c.gh, c.gw, c.B, c.H, c.hd), c)
    return groups


@pytest.mark.parametrize("entry", ["rel", "split"])
def test_emulation_within_half_bound(entry):
    """the bounds are attainable: the format choice alone stays within half of each on every case; and EMULATION_ERR is what it says"""
    for (_, dtn, value), cases in emulation_groups(entry).items():
        worst = 0.0
        for c in cases.values():
            p, idx, want = problem(c)
            e = block_err((emu_rel if entry == "rel" else emu_split)(p, idx), want)
            print("emulation %s: %.3e" % (case_id(c._replace(fast=False)), e))
            assert e <= bound(entry, c.dt, False) / 2, (case_id(c), e)
            worst = max(worst, e)
        print("emulation worst (%r, %r, %r): %.3e" % (entry, dtn, value, worst))
        rec = EMULATION_ERR[entry, dtn, value]
        assert (0.5 * rec if rec > 1e-12 else 0.0) <= worst <= rec, (entry, dtn, value, worst, rec)


# --------------------------------------------------------------------------------------------------------------------- GPU
def poisoned(*shapes_dtypes):
    """free NaN-filled device blocks of the given (shape, dtype): the allocator hands the most recently freed block of a size to the
    next torch.empty of that size, so an element the kernel does not write reads NaN"""
    blocks = [torch.full(shape, math.nan, dtype=dt, device=DEV) for shape, dt in shapes_dtypes]
    del blocks


def operands(p):
    """the device tensors of the entry point: qkv (B, N, 3 H hd) packed as (3, heads, hd), the two tables; HL8 for the split kernel"""
    from hipie_amd import ops
    ts = (torch.stack([p.q, p.k, p.v], 2).flatten(2).contiguous(), p.th.contiguous(), p.tw.contiguous())
    return tuple((ops.hl8_pack(t) if p.entry == "split" else t).to(DEV) for t in ts)


def hl8_planes(t):
    """HL8 (..., 2K) fp16 -> (hi, lo) float64 planes (..., K)"""
    pl = t.double().reshape(*t.shape[:-1], t.shape[-1] // 16, 2, 8)
    return pl[..., 0, :].reshape(*t.shape[:-1], -1), pl[..., 1, :].reshape(*t.shape[:-1], -1)


def check_planes(out):
    """the HL8 plane condition: |lo| <= |hi| 2^-11 + 2^-24"""
    hi, lo = hl8_planes(out.cpu())
    assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -11 + 2.0 ** -24).all())


def run(c, p):
    """-> the whole output (B, N, H, hd) on the host, as float64 for the split kernel (hi + lo) and in the operand type otherwise"""
    from hipie_amd import ops
    B, N, H, hd = p.q.shape
    qkv, th, tw = operands(p)
    if c.entry == "rel":
        poisoned(((B, N, H * hd), c.dt))
        out = ops.vit_attn_rel(qkv, th, tw, (c.gh, c.gw), H, fast=c.fast)
        assert out.dtype == c.dt and out.shape == (B, N, H * hd)
        return out.cpu().view(B, N, H, hd)
    poisoned(((B, N, 2 * H * hd), F16))
    out = ops.vit_attn_split(qkv, th, tw, (c.gh, c.gw), H)
    assert out.dtype == F16 and out.shape == (B, N, 2 * H * hd)
    check_planes(out)
    hi, lo = hl8_planes(out.cpu())
    return (hi + lo).view(B, N, H, hd)


def check(c, got, idx, want):
    assert bool(torch.isfinite(got).all()), "non-finite output (an element the kernel did not write reads NaN)"
    e, b = block_err(got[:, idx], want), bound(c.entry, c.dt, c.fast)
    print("block_err %s: %.3e (bound %.1e)" % (case_id(c), e, b))
    assert e < b, (case_id(c), e)


@gpu
@pytest.mark.parametrize("c", REL, ids=case_id)
def test_rel(c):
    p, idx, want = problem(c)
    check(c, run(c, p), idx, want)


@gpu
@pytest.mark.parametrize("c", SPLIT, ids=case_id)
def test_split(c):
    p, idx, want = problem(c)
    check(c, run(c, p), idx, want)


def call_entry(c, qkv, th, tw, out, B, H, gh=None, gw=None, hd=None):
    from hipie_amd import ops
    gh, gw, hd = gh or c.gh, gw or c.gw, hd or c.hd
    if c.entry == "rel":
        ops._call("hipie_vit_attn_rel", qkv.data_ptr(), th.data_ptr(), tw.data_ptr(), out.data_ptr(), B, gh, gw, H, hd, ops._DT[qkv.dtype],
                  ops.ATTN_FAST if c.fast else 0)
    else:
        ops._call("hipie_vit_attn_split", qkv.data_ptr(), th.data_ptr(), tw.data_ptr(), out.data_ptr(), B, gh, gw, H, hd)


SENTINEL = -7.0                               # exact in fp16 and bf16; compared bit for bit


@gpu
@pytest.mark.parametrize("c", GUARDED, ids=case_id)
def test_guarded_output(c):
    """`out` in the middle of a sentinel-filled buffer, 256 token rows (the largest workgroup's queries) of guard on both sides: every
    row is written (the result meets the bound) and nothing beyond the rows (a ragged last query tile, a transposed store)"""
    p, idx, want = problem(c)
    B, N, H, hd = p.q.shape
    row = H * hd * (2 if c.entry == "split" else 1)
    dt = F16 if c.entry == "split" else c.dt
    guard, n = 256 * row, B * N * row
    assert (guard * 2) % 16 == 0
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=dt, device=DEV)
    out = buf[guard:guard + n]
    call_entry(c, *operands(p), out, B, H)
    torch.cuda.synchronize()
    fill = torch.full((guard,), SENTINEL, dtype=dt).view(torch.int16)
    host = buf.cpu()
    assert torch.equal(host[:guard].view(torch.int16), fill) and torch.equal(host[guard + n:].view(torch.int16), fill)
    res = host[guard:guard + n].view(B, N, row)
    if c.entry == "split":
        hi, lo = hl8_planes(res)
        res = hi + lo
    check(c, res.view(B, N, H, hd), idx, want)


@gpu
def test_refusals():
    """what the entry points refuse is an error with the reason in it (no fall-back), and the output stays untouched"""
    from hipie_amd import ops
    from hipie_amd._lib import HipieLibraryError
    for entry, gh, gw, hd, what in refusal_cases():
        c = Case(entry, None, gh, gw, 1, 1, hd, F16, True, "refusal")
        N, mult = gh * gw, 2 if entry == "split" else 1
        qkv = torch.zeros(1, N, 3 * hd * mult, dtype=F16, device=DEV)
        th, tw = torch.zeros(2 * gh - 1, hd * mult, dtype=F16, device=DEV), torch.zeros(2 * gw - 1, hd * mult, dtype=F16, device=DEV)
        out = torch.full((N * hd * mult,), SENTINEL, dtype=F16, device=DEV)
        with pytest.raises(HipieLibraryError, match=what):
            call_entry(c, qkv, th, tw, out, 1, 1)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), (entry, gh, gw, hd)
        with pytest.raises(HipieLibraryError, match=what):
            (ops.vit_attn_rel if entry == "rel" else ops.vit_attn_split)(qkv.view(1, N, -1), th, tw, (gh, gw), 1)


@gpu
@pytest.mark.parametrize("c", [c for c in GUARDED if c.entry == "split" and c.line in ("win14", "w8x2", "slot96", "tr-w4x2")], ids=case_id)
def test_split_output_is_hl8(c):
    """the output is a well-formed HL8 tensor: the plane condition, and ops.to_hl8 of its own value gives that value back within one lo
    ulp (the value, not the planes: a lo of exactly half an ulp of hi is legal, and re-splitting it may round hi the other way)"""
    from hipie_amd import ops
    p, _, _ = problem(c)
    B, N, H, hd = p.q.shape
    poisoned(((B, N, 2 * H * hd), F16))
    out = ops.vit_attn_split(*operands(p), (c.gh, c.gw), H)
    check_planes(out)
    again = ops.to_hl8(ops.hl8_unpack(out))
    (hi, lo), (hi2, lo2) = hl8_planes(out.cpu()), hl8_planes(again.cpu())
    ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(lo.abs(), lo2.abs()).clamp_min(2.0 ** -14))) - 10)
    assert bool((((hi + lo) - (hi2 + lo2)).abs() <= ulp).all())


@gpu
@pytest.mark.parametrize("B,H", [(3, 3), (2, 4)], ids=["b3h3", "b2h4-swizzle"])
@pytest.mark.parametrize("c", [c for c in GUARDED if c.line in ("win14", "sp", "wide96", "w8x2", "tr-narrow")], ids=case_id)
def test_batch_invariance(c, B, H):
    """each image of a batched call equals the call on that image alone, bit for bit (see the module docstring): B = 3 x 3 heads (no
    swizzle in either call), and B = 2 x 4 heads (swizzle on) against 1 x 4 (off)"""
    g = gen("batch-%s-%d" % (case_id(c), B))
    N, mult = c.gh * c.gw, 2 if c.entry == "split" else 1
    dt = F16 if c.entry == "split" else c.dt
    qkv = (torch.randn(B, N, 3 * H * c.hd * mult, generator=g) * (0.02 if c.entry == "split" else 0.6)).to(dt).to(DEV)
    if c.entry == "split":                    # any fp16 content is a legal HL8 operand; keep the lo planes small beside the hi planes
        qkv.view(B, N, -1, 2, 8)[..., 0, :] *= 40
    th, tw = ((torch.randn(2 * n - 1, c.hd * mult, generator=g) * 0.3).to(dt).to(DEV) for n in (c.gh, c.gw))
    assert (B * H % 8 == 0) != (H % 8 == 0) or B == 3
    outs = []
    for lo_, hi_ in [(0, B)] + [(b, b + 1) for b in range(B)]:
        out = torch.full((hi_ - lo_, N, H * c.hd * mult), math.nan, dtype=dt, device=DEV)
        call_entry(c, qkv[lo_:hi_].contiguous(), th, tw, out, hi_ - lo_, H)
        outs.append(out.cpu())
    assert bool(torch.isfinite(outs[0]).all())
    for b in range(B):
        assert torch.equal(outs[0][b].view(torch.int16), outs[1 + b][0].view(torch.int16)), b
