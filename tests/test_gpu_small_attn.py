"""The small fp32-class attentions (hipie_amd/csrc/attn_f32.hip through ops.attn_f32 / ops.attn_f32_rows, hipie_amd/csrc/attn_split.hip
through ops.attn_split / ops.attn_f32_rows(split=True)) against float64 references, over every launch line.

Launch lines and a test id that reaches each (`launch_line` restates attn_f32_launch / attn_split_launch and the four C entries;
test_matrix_covers_every_line enforces this table from the mirror):

  hipie_attn_f32         attn_f32_kernel<32>    key mask (B, Nk) or none    test_attn[attn_f32-hd32-b2h1-1x197-packed-geometry-random]
                         attn_f32_kernel<64>                                test_attn[attn_f32-hd64-b2h1-1x197-packed-geometry-random]
  hipie_attn_f32_rows    attn_f32_kernel<32>    mask per (row, key)         test_attn[attn_f32_rows-hd32-b3h3-32x31-separate-geometry-random]
                         attn_f32_kernel<64>                                test_attn[attn_f32_rows-hd64-b3h3-32x31-separate-geometry-random]
  hipie_attn_split       attn_split_kernel<32>  key mask (B, Nk) or none    test_attn[attn_split-hd32-b1h2-33x32-batch-geometry-random]
                         attn_split_kernel<64>                              test_attn[attn_split-hd64-b1h2-33x32-batch-geometry-random]
  hipie_attn_split_rows  attn_split_kernel<32>  mask per (row, key)         test_attn[attn_split_rows-hd32-b2h3-130x197-separate-stairs-ones]
                         attn_split_kernel<64>                              test_attn[attn_split_rows-hd64-b2h3-130x197-separate-stairs-ones]
  every line x 11 geometries, x 5 value cases, x 5 mask cases (21 per line, 168 ids)              test_attn[<entry>-hd<hd>-...]
  refused by the C entries: head_dim 16 / 80 / 128, a pointer off a 16-byte boundary, a stride that is no multiple of 4 elements
                                                                            test_refusals
  refused by the op layer before the library (k / v / mask that disagree with q about B, H, hd, Nk): tests/test_small_attn_host.py (CPU)

No environment variable is read by these kernels or set by this file.

References, float64 on the fp32 values the kernel reads.  `ref_attn`: s = scale q.k, -inf where the key (key mask) or the (row, key) pair
(row mask) is not attended, softmax over the keys, times v.  `ref_loops` states the same in plain numpy loops over (b, h, i, j) for the
tiny edge inputs; test_references_agree checks the two to 1e-12 on the CPU.

Masked-row contract: a query row with no attended key gives ZEROS (both kernels: l_run stays 0 and the epilogue multiplies by 0), where
masked_fill(-inf).softmax of the reference model gives NaN.  The product never sends such a row (open_vocab.py never blocks the class
token; BERT's [CLS] is never padding), the kernels' behaviour is pinned here all the same: `all_masked`, and every random row mask with
Nk = 1.  Mask bytes: 0 = blocked, anything else attends (`bytes`).

Metric: `block_err` = max|got - ref| over a (batch, head, 32-query block) / max|ref| over the same block, the maximum over blocks.  A
32-query block is what a wave of attn_split owns (a quarter of a workgroup of attn_f32).  A block whose reference is all zero must be
exactly zero, and so must every single row whose reference is zero (a dead row among the live rows of its block).  V is scaled per head by 1, 1/8, 8, so a head that reads its neighbour's V shows at up to 64 times its own scale.

Bound: 1e-5 for all eight lines, the project's number for both kernels (tests/test_gpu_kernels.py::test_attn_f32_exact).  No bound comes
from a kernel.  Attainability on the CPU: `emu_f32` (fp32 scores in the exp2 domain, fp32 P, fp32 PV) and `emu_split` (three-product
logits of fp16 pairs with hl_split's clamp, P as an fp16 pair, V_hi.(P_hi + P_lo) + V_lo.P_hi) emulate the format choice only;
test_emulation_within_half_bound asserts block_err <= bound / 2 on every case of every matrix and re-measures EMULATION_ERR
(docs/measurements.md).

Geometry cases (random values, a random mask of 70 % attended; the key-mask entries alternate with no mask): Nq x Nk of 1x197, 32x31,
33x32, 127x33, 128x63, 129x64, 257x65, 33x129, 129x1, 1x1, 129x129; (B, H) of (2,1), (3,3), (1,2) in turn (H = 1: the op layer skips its
head-stride check); the layouts turn against them (`batch` meets B = 3 at 128x63 and B = 2 at 257x65; 129x129 is `packed` at B = H = 3,
the qkv of modeling/text.py); layouts `packed` (q, k, v column blocks of one projection output; with Nq != Nk q alone and k, v of one buffer),
`separate` (three buffers of different row strides, v behind a foreign column block), `batch` (rows of padding after every batch item:
a batch stride that is not N x row stride).  The padding is NaN: a tail key that read past Nk would show.

Value cases (B 2, H 3, 130 x 197; no mask / a mask of ones), properties asserted on the operands as read by
test_value_inputs_have_their_properties for both tilings (32 keys in attn_f32, 64 in attn_split):
  random       logits of natural size (|s| up to ~20 in the log2 domain), random mask
  stairs       every row's maximum rises by 3 from one 32-key tile to the next: the rescale runs at every tile of either kernel
  late_jump    flat logits, then ONE key of the last tile exceeds the rest by 6.5 for 5 rows of every 32; the keys before keep >= 10 % of
               those rows' mass, so a wrong rescale of O or of the row sum shows
  first_max    the maximum sits in keys 0..31, every later key lies more than 150 below it: exp2 gives zero
  one_hot      per query one key dominates by more than 40: the output is that key's v row; positions include the first and last slot of
               a tile of either kernel (0, 31, 32, 63, 64) and the last key of the walk, which is the slot next to the tail padding
Mask cases (B 4, H 3, 130 x 197, random values), on the key-mask and the per-row entries:
  prefix_masked  keys [0, 32), [0, 64), [0, 128) blocked per batch item (one, two, four tiles of attn_f32; half, one, two of attn_split),
                 the fourth item sees the LAST key only; per-row: rows 3, 40, 129 of every item see the last key only as well
  tail_masked    only the first 150, 65, 33, 1 keys attended (Nk = 197 is ragged for both tilings)
  holes          every second key (even, odd), every third, every 64th
  all_masked     key mask: item 1 fully blocked; per-row: rows 0, 31, 32, 77, 129 of items 0 and 2 fully blocked among live rows
  bytes          attended bytes are 1, 2 or 255

Range contract of attn_split (measured by emulation, asserted on the kernel):
  small_v   V ~ N(0, 1) x 2^e: the lo halves of V fall into fp16 subnormals as e falls.  SMALL_V_LOG2 is the smallest e at which (and
            above which) emu_split stays within half the bound; the kernel is asserted there, attn_f32 at 2^-20 of it.
  sink      Nk 910, one key holds the maximum with its V scaled by 0.01, the other 909 hold 2^-12 .. 2^-24 of it: the lo half of P has
            an absolute floor of 2^-25 of the largest probability, so the tail's sum is off by up to ~1e-4 of the (small) output.
            `sink_err` measures against max|v| over the attended keys of the head instead of the block's own scale; the emulation stays
            within half the bound under that denominator (SINK_ERR), and attn_f32 meets the plain block metric.

Cross-checks that need no bound: a key mask equals, bit for bit, the same mask expanded to (B, Nq, Nk) through the _rows entry; item b of
a B = 3 call equals the B = 1 call on that item; two calls agree.  attn_split against attn_f32 on the random cases: twice the
emulations' mutual difference (MUTUAL_DIFF).

Output buffers: `poisoned` frees a NaN block of the output's size before every call through ops.*; test_guarded_output calls the C
entries through ops._call with `out` in the middle of a sentinel-filled buffer for one ragged case (129 x 65) per launch line."""
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
F32 = torch.float32
LOG2E = 1.4426950408889634
BOUND = 1e-5
V_SCALE = (1.0, 0.125, 8.0)                 # per head, cycled
VALUES = ("random", "stairs", "late_jump", "first_max", "one_hot")
MASKS = ("prefix_masked", "tail_masked", "holes", "all_masked", "bytes")
JUMP_ROWS = (1, 5, 6, 17, 30)               # late_jump: the rows of every 32-query block that jump
JUMP, STEP = 6.5, 3.0
ONE_HOT_GAIN = 24.0                         # one_hot: a differing code bit costs 2 x 24 = 48 in log2
TILE = {"f32": 32, "split": 64}             # keys per tile (TK in attn_f32.hip, KT in attn_split.hip): used by the inputs' checks only
LAST_KEY_ROWS = (3, 40, 129)
DEAD_ROWS = (0, 31, 32, 77, 129)

# Largest block_err of emu_f32 / emu_split against the float64 reference per (kernel, group of cases), measured on the CPU by
# test_emulation_within_half_bound, which re-measures them: each must stay at or below its entry and above half of it; the entries are
# the measured values plus 1 %.  Half of the bound is 5e-6.  An entry of 1e-12 stands for "exact" (one_hot: P is 1 or 0).
# The emulations are fp32 einsums: another CPU BLAS or vector width may move their last bits and an entry with them.  To re-measure, run
# `pytest tests/test_gpu_small_attn.py -m "not gpu" -s` and read the "emulation worst", "mutual difference", "small_v" and "sink" lines
# (a test stops at its first entry that is off, so repeat after each correction); enter the printed value times 1.01.  What must hold
# whatever the library is `<= BOUND / 2`, which is asserted apart from the table.
EMULATION_ERR = {
    ("f32", "geometry"): 1.51e-06, ("f32", "random"): 1.47e-06, ("f32", "stairs"): 8.67e-07, ("f32", "late_jump"): 3e-07,
    ("f32", "first_max"): 3.94e-07, ("f32", "masks"): 2.09e-06, ("f32", "one_hot"): 1e-12, ("split", "geometry"): 1.45e-06,
    ("split", "random"): 1.4e-06, ("split", "stairs"): 1.3e-06, ("split", "late_jump"): 6.54e-07, ("split", "first_max"): 4.23e-07,
    ("split", "one_hot"): 1.18e-07, ("split", "masks"): 1.91e-06,
}
MUTUAL_DIFF = 2.09e-06                      # largest block_err(emu_split, emu_f32) over the `random` value cases, plus 1 %
SMALL_V_LOG2 = {32: -8, 64: -8}             # hd -> smallest e with emu_split within BOUND / 2 on V ~ N(0, 1) 2^e' for every e' in [e, 0]
# sink, per hd: (emu_split by block_err: beyond the bound, the documented limit; emu_split by sink_err; emu_f32 by block_err), plus 1 %
SINK_ERR = {32: (8.09e-05, 4.68e-07, 1.02e-06), 64: (8.15e-05, 4.54e-07, 1.05e-06)}


# ------------------------------------------------------------------------------------------------------ mirror of the dispatch
ENTRY = {("f32", False): "hipie_attn_f32", ("f32", True): "hipie_attn_f32_rows",
         ("split", False): "hipie_attn_split", ("split", True): "hipie_attn_split_rows"}
KERNEL = {"f32": "attn_f32_kernel", "split": "attn_split_kernel"}
HDS = (32, 64)


def launch_line(kernel, rows, hd):
    """(C entry, kernel instantiation) of attn_f32_launch / attn_split_launch, None where the entry refuses"""
    return (ENTRY[kernel, rows], "%s<%d>" % (KERNEL[kernel], hd)) if hd in HDS else None


LINES = [(kernel, rows, hd) for kernel in ("f32", "split") for rows in (False, True) for hd in HDS]


# --------------------------------------------------------------------------------------------------------------- references
# q (B, Nq, H, hd), k, v (B, Nk, H, hd) fp32; kmask (B, Nk) / qmask (B, Nq, Nk) uint8 or None, at most one of them
Problem = collections.namedtuple("Problem", "q k v kmask qmask scale")


def attended(p):
    """(B, 1 | Nq, Nk) bool, or None without a mask"""
    if p.qmask is not None:
        return p.qmask != 0
    return None if p.kmask is None else (p.kmask != 0)[:, None, :]


def _masked(s, p):
    """s (B, H, Nq, Nk) with -inf where the row may not see the key"""
    a = attended(p)
    return s if a is None else s.masked_fill(~a[:, None], -math.inf)


def _softmax_v(s, v, exp):
    """rows of s with no finite entry give zeros"""
    m = s.amax(-1, keepdim=True)
    w = exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = w.sum(-1)
    o = torch.einsum("bhij,bjhd->bihd", w, v)
    return o / torch.where(l > 0, l, torch.ones_like(l)).permute(0, 2, 1)[..., None]


def ref_attn(p):
    """float64 reference -> (B, Nq, H, hd)"""
    s = torch.einsum("bihd,bjhd->bhij", p.q.double(), p.k.double()) * p.scale
    return _softmax_v(_masked(s, p), p.v.double(), torch.exp)


def ref_loops(p):
    """the same, one loop iteration per (b, h, i, j), numpy float64"""
    q, k, v = (t.double().numpy() for t in (p.q, p.k, p.v))
    B, Nq, H, hd = q.shape
    Nk = k.shape[1]
    out = np.zeros((B, Nq, H, hd))
    for b, h, i in itertools.product(range(B), range(H), range(Nq)):
        keys = [j for j in range(Nk) if (p.kmask is None or p.kmask[b, j] != 0) and (p.qmask is None or p.qmask[b, i, j] != 0)]
        if not keys:
            continue
        s = np.array([p.scale * float(np.dot(q[b, i, h], k[b, j, h])) for j in keys])
        w = np.exp(s - s.max())
        out[b, i, h] = sum(w[n] * v[b, j, h] for n, j in enumerate(keys)) / w.sum()
    return torch.from_numpy(out)


def pair(x):
    """fp32 -> the fp16 pair (hi, lo) of hl_split, as fp32"""
    hi = x.float().clamp(-65504.0, 65504.0).half().float()
    return hi, (x.float().clamp(-65504.0, 65504.0) - hi).half().float()


def q_scaled(p):
    """q as the kernels use it: times the fp32 product scale x log2(e), in fp32"""
    return p.q * float(np.float32(p.scale) * np.float32(LOG2E))


def scores2(p, kernel):
    """float64 logits in the log2 domain of the operands AS READ (attn_split: the fp16 pairs), masked -> (B, H, Nq, Nk)"""
    q, k = q_scaled(p), p.k
    if kernel == "split":
        q, k = sum(pair(q)), sum(pair(k))
    return _masked(torch.einsum("bihd,bjhd->bhij", q.double(), k.double()), p)


def emu_f32(p):
    """CPU emulation of attn_f32.hip's format choice (not of its order of operations): everything in fp32, scores in the exp2 domain"""
    s = _masked(torch.einsum("bihd,bjhd->bhij", q_scaled(p), p.k), p)
    return _softmax_v(s, p.v, torch.exp2).double()


def emu_split(p):
    """CPU emulation of attn_split.hip's format choice: logits q_lo.k_hi + q_hi.k_lo + q_hi.k_hi in fp32 from the fp16 pairs, P = exp2(s -
    max) as an fp16 pair, O = V_hi.(P_hi + P_lo) + V_lo.P_hi in fp32, divided by the fp32 sum of the unrounded P"""
    (qh, ql), (kh, kl), (vh, vl) = pair(q_scaled(p)), pair(p.k), pair(p.v)
    dot = functools.partial(torch.einsum, "bihd,bjhd->bhij")
    s = _masked(dot(ql, kh) + dot(qh, kl) + dot(qh, kh), p)
    m = s.amax(-1, keepdim=True)
    w = torch.exp2(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    ph, pl = pair(w)
    o = torch.einsum("bhij,bjhd->bihd", ph + pl, vh) + torch.einsum("bhij,bjhd->bihd", ph, vl)
    l = w.sum(-1)
    return (o / torch.where(l > 0, l, torch.ones_like(l)).permute(0, 2, 1)[..., None]).double()


EMU = {"f32": emu_f32, "split": emu_split}


def _blocks(x):
    """(B, n, H, hd) of absolute values -> (B, blocks, H) maxima over 32-query blocks"""
    B, n, H, hd = x.shape
    npad = -(-n // 32) * 32
    y = torch.zeros(B, npad, H, hd, dtype=torch.float64)
    y[:, :n] = x
    return y.view(B, npad // 32, 32, H, hd).amax((2, 4))


def block_err(got, want, denom=None):
    """max over (batch, head, 32-query block) of max|got - want| / max|want| of the block (denom (B, H): that value per head instead).
    Non-finite values fail; every (batch, query, head) row whose reference is all zero -- a row with no attended key, also one among live
    rows of its block -- must be exactly zero, and so a block whose reference is all zero"""
    got, want = got.detach().cpu().double().reshape(want.shape), want.double()
    assert bool(torch.isfinite(got).all()), "non-finite output (an element the kernel did not write reads NaN)"
    assert bool((got[(want == 0).all(-1)] == 0).all()), "a row whose reference is all zero (no attended key) must be exactly zero"
    d, r = _blocks((got - want).abs()), _blocks(want.abs())
    dead = r == 0
    assert bool((d[dead] == 0).all()), "a block whose reference is all zero must be exactly zero"
    if denom is not None:
        r = denom.double()[:, None, :].expand_as(r)
    return float((d[~dead] / r[~dead]).max()) if bool((~dead).any()) else 0.0


def sink_denominator(p):
    """(B, H): max|v| over the attended keys of the head (every key of the `sink` input is attended)"""
    return p.v.abs().amax((1, 3))


# ------------------------------------------------------------------------------------------------------------------- inputs
def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def head_scaled(v):
    """(B,N,H,hd) values with the per-head scale 1, 1/8, 8"""
    return v * torch.tensor([V_SCALE[h % 3] for h in range(v.shape[2])]).view(1, 1, -1, 1)


def special_keys(Nk):
    """one_hot: first / last slot of the first tile of either kernel, first slot of the second tile of either, the last key of the walk"""
    return sorted({min(j, Nk - 1) for j in (0, 31, 32, 63, 64, Nk - 1)})


def key_mask_of(name, B, Nk, g):
    """(B, Nk) uint8 of a mask case, None for `none`"""
    j = torch.arange(Nk)
    if name == "none":
        return None
    if name == "ones":
        return torch.ones(B, Nk, dtype=torch.uint8)
    m = (torch.rand(B, Nk, generator=g) < 0.7).to(torch.uint8)
    if name == "prefix_masked":
        assert B == 4 and Nk > 129
        m = torch.stack([j >= 32, j >= 64, j >= 128, j == Nk - 1]).to(torch.uint8)
    elif name == "tail_masked":
        m = torch.stack([j < n for n in (150, 65, 33, 1)][:B]).to(torch.uint8)
    elif name == "holes":
        m = torch.stack([j % 2 == 0, j % 2 == 1, j % 3 == 1, j % 64 == 63][:B]).to(torch.uint8)
    elif name == "all_masked":
        m[1] = 0
    elif name == "bytes":
        m = m * torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (B, Nk), generator=g)]
    else:
        assert name == "random", name
    return m


def row_mask_of(name, B, Nq, Nk, g):
    """(B, Nq, Nk) uint8 of a mask case for the per-row entries"""
    if name == "none":
        name = "ones"
    if name in ("random", "bytes", "all_masked"):
        m = (torch.rand(B, Nq, Nk, generator=g) < 0.7).to(torch.uint8)
        if name == "bytes":
            m = m * torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (B, Nq, Nk), generator=g)]
        if name == "all_masked":
            m[0::2, list(DEAD_ROWS)] = 0
        return m
    m = key_mask_of(name, B, Nk, g)[:, None, :].repeat(1, Nq, 1)
    if name == "prefix_masked":
        m[:, list(LAST_KEY_ROWS)] = 0
        m[:, list(LAST_KEY_ROWS), Nk - 1] = 1
    return m


Case = collections.namedtuple("Case", "kernel rows hd B H Nq Nk layout value mask")


def case_id(c):
    return "%s-hd%d-b%dh%d-%dx%d-%s-%s-%s" % (ENTRY[c.kernel, c.rows][6:], c.hd, c.B, c.H, c.Nq, c.Nk, c.layout, c.value, c.mask)


@functools.lru_cache(maxsize=None)
def _problem(rows, hd, B, H, Nq, Nk, value, mask):
    g = gen("small-attn-%d-hd%d-b%dh%d-%dx%d-%s-%s" % (rows, hd, B, H, Nq, Nk, value, mask))
    scale = hd ** -0.5
    unit = 1.0 / (scale * LOG2E)                       # q = q' x unit gives q' in the log2 domain

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    v = head_scaled(rn(B, Nk, H, hd))
    if value in ("random", "geometry"):
        q, k = rn(B, Nq, H, hd) * 1.6, rn(B, Nk, H, hd) * 1.6          # |q.k| scale log2 e up to ~20
    elif value == "small_v":
        q, k, v = rn(B, Nq, H, hd) * 1.6, rn(B, Nk, H, hd) * 1.6, rn(B, Nk, H, hd)
    else:
        # small noise (standard deviation ~0.03, one_hot ~0.1, in log2 units); the structure sits in exact columns of q' and k: the LAST
        # one, so that a sum over the head dimension in ascending order adds the large term once, after the noise
        q, k = rn(B, Nq, H, hd) * ((0.1 if value == "one_hot" else 0.03) / math.sqrt(hd)), rn(B, Nk, H, hd)
        i, j = torch.arange(Nq), torch.arange(Nk)
        if value == "one_hot":
            L = max(1, (Nk - 1).bit_length())
            code = ((j[:, None] >> torch.arange(L)[None, :]) & 1).float() * 2 - 1                     # (Nk, L) of +-1
            pos = torch.randint(0, Nk, (B, H, Nq), generator=g)
            sp = torch.tensor(special_keys(Nk))
            pos[:, :, :len(sp)], pos[:, :, Nq - len(sp):] = sp, sp          # in the first and in the last (ragged) query block
            k[..., 1:1 + L] = code[None, :, None, :]
            q[..., 1:1 + L] = ONE_HOT_GAIN * code[pos].permute(0, 2, 1, 3)
        elif value == "sink":
            dom = Nk // 2
            step = -(12.0 + 12.0 * torch.rand(Nk, generator=g))
            step[dom] = 0.0
            q[..., -1], k[..., -1] = 1.0, step[None, :, None]
            v[:, dom] *= 0.01
        else:
            if value == "stairs":
                a, step = torch.full((Nq,), STEP), (j // 32).float()
            elif value == "first_max":
                a, step = torch.full((Nq,), JUMP), -32.0 * (j >= 32).float()
            elif value == "late_jump":
                a, step = torch.isin(i % 32, torch.tensor(JUMP_ROWS)).float() * JUMP, (j == Nk - 3).float()
            else:
                raise ValueError(value)
            q[..., -1], k[..., -1] = a[None, :, None], step[None, :, None]
        q = q * unit
    p = Problem(q.float().contiguous(), k.float().contiguous(), v.float().contiguous(),
                None if rows else key_mask_of(mask, B, Nk, g), row_mask_of(mask, B, Nq, Nk, g) if rows else None, scale)
    return p, ref_attn(p)


def problem(c):
    """-> (problem, float64 reference): shared by the two kernels, left unchanged by every test"""
    return _problem(c.rows, c.hd, c.B, c.H, c.Nq, c.Nk, c.value, c.mask)


# ---- the matrices ----
GEOMETRY = ((1, 197), (32, 31), (33, 32), (127, 33), (128, 63), (129, 64), (257, 65), (33, 129), (129, 1), (1, 1), (129, 129))
BATCH_HEADS = ((2, 1), (3, 3), (1, 2))
LAYOUTS = ("packed", "separate", "batch")
VALUE_SHAPE = (2, 3, 130, 197)              # B, H, Nq, Nk of the value cases; the mask cases take B = 4
GUARD_SHAPE = (2, 3, 129, 65)


def _cases(kernel, rows, hd):
    out = []
    for n, (Nq, Nk) in enumerate(GEOMETRY):
        B, H = BATCH_HEADS[n % 3]
        # the layouts turn against (B, H), so that `batch` meets B = 3 and B = 2; 129 x 129 is the product's qkv of one projection output
        layout = "packed" if Nq == Nk > 1 else LAYOUTS[(n // 3 + n) % 3]
        out.append(Case(kernel, rows, hd, B, H, Nq, Nk, layout, "geometry", "random" if rows or n % 2 == 0 else "none"))
    B, H, Nq, Nk = VALUE_SHAPE
    for n, value in enumerate(VALUES):
        out.append(Case(kernel, rows, hd, B, H, Nq, Nk, LAYOUTS[n % 3], value, "random" if value == "random" else "ones" if rows else "none"))
    for n, mask in enumerate(MASKS):
        out.append(Case(kernel, rows, hd, 4, H, Nq, Nk, LAYOUTS[n % 3], "random", mask))
    return out


CASES = [c for line in LINES for c in _cases(*line)]
GUARDED = [Case(kernel, rows, hd, *GUARD_SHAPE, "separate", "geometry", "random") for kernel, rows, hd in LINES]
RANGE = [Case(kernel, rows, hd, 1, 3, 130, 197, "packed", "small_v", "ones" if rows else "none") for kernel, rows, hd in LINES]
SINK = [Case(kernel, rows, hd, 1, 3, 130, 910, "packed", "sink", "ones" if rows else "none") for kernel, rows, hd in LINES]


def group(c):
    return "geometry" if c.value == "geometry" else "masks" if c.mask in MASKS else c.value


# ---- tiny inputs for the two references ----
def edge_problems():
    g = gen("edges")
    for name, B, H, Nq, Nk, mask in (("plain", 2, 2, 3, 5, "none"), ("one_key", 1, 2, 4, 1, "none"), ("key_mask", 2, 2, 3, 7, "random"),
                                     ("row_mask", 2, 1, 5, 4, "rows"), ("dead_item", 2, 2, 3, 4, "all_masked"), ("dead_rows", 2, 2, 3, 4, "dead_rows")):
        q, k = torch.randn(B, Nq, H, 4, generator=g), torch.randn(B, Nk, H, 4, generator=g)
        v = head_scaled(torch.randn(B, Nk, H, 4, generator=g))
        km = qm = None
        if mask in ("rows", "dead_rows"):
            qm = (torch.rand(B, Nq, Nk, generator=g) < 0.6).to(torch.uint8) * 255
            qm[:, 0, 0] = 1
            if mask == "dead_rows":
                qm[:, 1] = 0
        elif mask != "none":
            km = key_mask_of(mask, B, Nk, g)
        yield name, Problem(q, k, v, km, qm, 0.5)


# -------------------------------------------------------------------------------------- CPU: references, inputs, bounds (no GPU)
def test_references_agree():
    for name, p in edge_problems():
        a, b = ref_attn(p), ref_loops(p)
        assert bool(torch.isfinite(a).all()) and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
        if name == "one_key":
            assert float((a - p.v.double().expand_as(a)).abs().max()) <= 1e-12 * float(p.v.abs().max())
        if name == "dead_item":
            assert bool((a[1] == 0).all()) and bool((a[0] != 0).any())
        if name == "dead_rows":
            assert bool((a[:, 1] == 0).all()) and bool((a[:, 0] != 0).any())
        for emu in (emu_f32, emu_split):             # the emulations state the same contract
            assert block_err(emu(p), a) < 1e-5, name


def test_matrix_covers_every_line():
    from hipie_amd import ops
    assert len(LINES) == 8 and len({launch_line(*line) for line in LINES}) == 8
    assert all(launch_line("f32", rows, hd) is None and not ops.attn_f32_ok(hd) for rows in (False, True) for hd in (16, 80, 128))
    assert all(ops.attn_f32_ok(hd) for hd in HDS)
    for line in LINES:
        mine = [c for c in CASES if (c.kernel, c.rows, c.hd) == line]
        assert all(launch_line(c.kernel, c.rows, c.hd) == launch_line(*line) for c in mine)
        assert {(c.Nq, c.Nk) for c in mine if c.value == "geometry"} == set(GEOMETRY)
        assert {c.value for c in mine} == set(VALUES) | {"geometry"} and {c.mask for c in mine} >= set(MASKS)
        geo = [c for c in mine if c.value == "geometry"]
        assert {c.layout for c in geo} == set(LAYOUTS) and {(c.B, c.H) for c in geo} == set(BATCH_HEADS)
        assert any(c.B == 3 and c.H == 3 for c in geo) and any(c.H == 1 for c in geo)
        assert {c.B for c in geo if c.layout == "batch"} >= {2, 3} and any(c.layout == "packed" and c.Nq == c.Nk > 64 and c.H == 3 for c in geo)
        assert any(c.Nq > c.Nk for c in geo) and any(c.Nq < c.Nk for c in geo)
        assert line[1] or {c.mask for c in geo} == {"random", "none"}
        for cases in (GUARDED, RANGE, SINK):
            assert sum((c.kernel, c.rows, c.hd) == line for c in cases) == 1
    assert {c.Nq for c in CASES} >= {1, 32, 33, 127, 128, 129, 257} and {c.Nk for c in CASES} >= {1, 31, 32, 33, 63, 64, 65, 129, 197}
    assert max(c.Nq for c in CASES) <= 257 and max(c.Nk for c in CASES) <= 200
    ids = {case_id(c) for c in CASES}
    assert len(ids) == len(CASES)
    for line in __doc__.split("\n"):                  # the table of the docstring names real cases
        if "test_attn[" in line and "<" not in line.split("test_attn[")[1]:
            assert line.split("test_attn[")[1].split("]")[0] in ids, line
    named = {launch_line(c.kernel, c.rows, c.hd) for c in CASES if "test_attn[%s]" % case_id(c) in __doc__}
    assert named == {launch_line(*line) for line in LINES}


def tile_maxima(s, tile):
    """(B, H, Nq, ntiles): the row maximum per key tile"""
    Nk = s.shape[-1]
    pad = torch.full(s.shape[:3] + (-(-Nk // tile) * tile,), -math.inf, dtype=s.dtype)
    pad[..., :Nk] = s
    return pad.view(*s.shape[:3], -1, tile).amax(-1)


def test_value_inputs_have_their_properties():
    """each value case has the property its name claims, on the operands as either kernel reads them and for either tiling"""
    for c in CASES:
        if c.value in ("random", "geometry"):
            continue
        p, _ = problem(c)
        name, tile = case_id(c), TILE[c.kernel]
        s = scores2(p, c.kernel)
        tm = tile_maxima(s, tile)
        run = torch.cummax(tm, 3).values
        Nk, nt = c.Nk, tm.shape[-1]
        assert nt >= 4 and Nk % 64 != 0
        if c.value == "stairs":
            assert float((tm[..., 1:] - run[..., :-1]).min()) > STEP - 1 and float(s.abs().max()) < 25, name
        elif c.value == "first_max":
            assert float((s[..., 32:].amax(-1) - s[..., :32].amax(-1)).max()) < -150, name
        elif c.value == "late_jump":
            rows = torch.isin(torch.arange(c.Nq) % 32, torch.tensor(JUMP_ROWS))
            assert (Nk - 3) // tile == nt - 1 and 0 < int(rows.sum()) < c.Nq
            assert float((tm[:, :, rows, -1] - run[:, :, rows, -2]).min()) > JUMP - 1, name
            assert float((tm[:, :, ~rows] - tm[:, :, ~rows][..., :1]).abs().max()) < 1 and float((run[:, :, rows, -2] - tm[:, :, rows, 0]).max()) < 1
            w = torch.exp2(s - s.amax(-1, keepdim=True))
            share = w[..., :(nt - 1) * tile].sum(-1) / w.sum(-1)
            assert float(share[:, :, rows].min()) >= 0.10, (name, float(share[:, :, rows].min()))
        elif c.value == "one_hot":
            top = s.topk(2, -1)
            assert float((top.values[..., 0] - top.values[..., 1]).min()) > 40, name
            pos = top.indices[..., 0]
            want_keys = special_keys(Nk)
            assert all(bool((pos == key).any()) for key in want_keys), name
            assert {0, tile - 1, tile, Nk - 1} <= set(want_keys) and Nk - 1 == (nt - 1) * tile + Nk % tile - 1
            assert len(torch.unique(pos)) > min(Nk, c.Nq) // 4
    for c in SINK:
        p, want = problem(c)
        s = scores2(p, c.kernel)
        top = s.topk(2, -1)
        assert bool((top.indices[..., 0] == c.Nk // 2).all()) and 11.5 < float((top.values[..., 0] - top.values[..., 1]).min())
        assert float((s.amax(-1) - s.amin(-1)).max()) < 24.5


def test_mask_inputs_have_their_properties():
    for c in CASES:
        if c.mask not in MASKS:
            continue
        p, want = problem(c)
        a = attended(p).expand(c.B, c.Nq, c.Nk)
        name = case_id(c)
        first = a.int().argmax(-1)                     # the first attended key of every row (0 for a row with none)
        if c.mask == "prefix_masked":
            for b, n in enumerate((32, 64, 128, c.Nk - 1)):
                rows = [i for i in range(c.Nq) if not (c.rows and i in LAST_KEY_ROWS)]
                assert bool((first[b, rows] == n).all()) and not bool(a[b, :, :n].any()), name
            assert bool((a[3].sum(-1) == 1).all()) and bool(a[3, :, -1].all())
            if c.rows:
                assert bool((a[:, list(LAST_KEY_ROWS)].sum(-1) == 1).all()) and bool(a[:, list(LAST_KEY_ROWS), -1].all())
        elif c.mask == "tail_masked":
            assert [int(x) for x in a[:, 0].sum(-1)] == [150, 65, 33, 1] and bool((first == 0).all()) and c.Nk % 32 and c.Nk % 64
        elif c.mask == "holes":
            assert [int(x) for x in a[:, 5].sum(-1)] == [99, 98, 66, 3] and not bool(a[3, :, :63].any())
        elif c.mask == "all_masked":
            dead = a.sum(-1) == 0
            if c.rows:
                assert bool(dead[0::2][:, list(DEAD_ROWS)].all()) and int(dead.sum()) == 2 * len(DEAD_ROWS)
            else:
                assert bool(dead[1].all()) and int(dead.sum()) == c.Nq
            assert bool((want[dead] == 0).all()) and bool((want[~dead].abs().amax((1, 2)) > 0).all()), name
        elif c.mask == "bytes":
            m = p.qmask if c.rows else p.kmask
            assert set(torch.unique(m).tolist()) == {0, 1, 2, 255}
    # every batch item of a B = 3, H = 3 geometry has a mask of its own
    for c in CASES:
        if c.value == "geometry" and c.B == 3 and c.mask == "random" and c.Nk > 8:
            a = attended(problem(c)[0])
            assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]) and not torch.equal(a[0], a[2])


@pytest.mark.parametrize("kernel", ["f32", "split"])
def test_emulation_within_half_bound(kernel):
    """the bound is attainable: the format choice alone stays within half of it on every case; and EMULATION_ERR is what it says"""
    worst = collections.defaultdict(float)
    for c in CASES:
        if c.kernel != kernel:
            continue
        p, want = problem(c)
        e = block_err(EMU[kernel](p), want)
        print("emulation %s: %.3e" % (case_id(c), e))
        assert e <= BOUND / 2, (case_id(c), e)
        worst[group(c)] = max(worst[group(c)], e)
    for grp, e in worst.items():
        print("emulation worst (%r, %r): %.3e" % (kernel, grp, e))
        rec = EMULATION_ERR[kernel, grp]
        assert (0.5 * rec if rec > 1e-12 else 0.0) <= e <= rec, (kernel, grp, e, rec)
    assert set(worst) == {g for k, g in EMULATION_ERR if k == kernel}


def random_value_cases():
    return [c for c in CASES if c.value == "random" and c.mask == "random"]


def test_mutual_difference_of_the_emulations():
    """MUTUAL_DIFF: how far the two format choices lie apart on the random cases; twice that bounds attn_split against attn_f32"""
    worst = 0.0
    for c in random_value_cases():
        if c.kernel == "split":
            p, _ = problem(c)
            worst = max(worst, block_err(emu_split(p), emu_f32(p)))
    print("mutual difference: %.3e" % worst)
    assert 0.5 * MUTUAL_DIFF <= worst <= MUTUAL_DIFF and 2 * MUTUAL_DIFF <= BOUND


def v_scaled(p, e):
    return p._replace(v=p.v * 2.0 ** e)


def small_v_limit(p, want):
    """the smallest e such that emu_split stays within BOUND / 2 on v x 2^e' for every e' in [e, 0]"""
    e = 0
    while e > -40 and block_err(emu_split(v_scaled(p, e - 1)), want * 2.0 ** (e - 1)) <= BOUND / 2:
        e -= 1
    return e


def test_range_contract_by_emulation():
    """small_v: SMALL_V_LOG2 is the measured limit of the split format, and the fp32 format has none 2^-20 below it.  sink: emu_split
    misses the bound per block, meets half of it against max|v| of the attended keys; emu_f32 meets half of it per block"""
    for c in RANGE:
        if c.kernel == "split" and not c.rows:
            p, want = problem(c)
            e = small_v_limit(p, want)
            below = block_err(emu_split(v_scaled(p, e - 1)), want * 2.0 ** (e - 1))
            print("small_v hd %d: limit 2^%d, one below %.3e" % (c.hd, e, below))
            assert e == SMALL_V_LOG2[c.hd] and below > BOUND / 2
            assert block_err(emu_f32(v_scaled(p, e - 20)), want * 2.0 ** (e - 20)) <= BOUND / 2
    for c in SINK:
        if not c.rows:
            p, want = problem(c)
            if c.kernel == "split":
                own, sink = block_err(emu_split(p), want), block_err(emu_split(p), want, sink_denominator(p))
                print("sink hd %d: emu_split %.3e per block, %.3e of max|v|" % (c.hd, own, sink))
                assert 0.5 * SINK_ERR[c.hd][0] <= own <= SINK_ERR[c.hd][0] and own > BOUND
                assert 0.5 * SINK_ERR[c.hd][1] <= sink <= SINK_ERR[c.hd][1] <= BOUND / 2
            else:
                own = block_err(emu_f32(p), want)
                print("sink hd %d: emu_f32 %.3e per block" % (c.hd, own))
                assert 0.5 * SINK_ERR[c.hd][2] <= own <= SINK_ERR[c.hd][2] <= BOUND / 2


# --------------------------------------------------------------------------------------------------------------------- GPU
def poisoned(shape):
    """free a NaN-filled device block of the output's size: the allocator hands the most recently freed block of a size to the next
    torch.empty of that size, so an element the kernel does not write reads NaN.  `call` hands the per-row entries a dense uint8 mask, so
    that no allocation of the op layer comes between this block and `out`; it remains the allocator's habit, not a promise:
    test_guarded_output is the rigorous check of what is written"""
    block = torch.full(shape, math.nan, dtype=F32, device=DEV)
    del block


def _columns(parts, N, pad_cols, pad_rows, lead=0):
    """one NaN-filled device buffer (B, N + pad_rows, (lead + len(parts)) C + pad_cols) with the parts as column blocks behind `lead`
    foreign blocks -> their (B, N, H, hd) views"""
    B, _, H, hd = parts[0].shape
    C = H * hd
    buf = torch.full((B, N + pad_rows, (lead + len(parts)) * C + pad_cols), math.nan, dtype=F32)
    for n, t in enumerate(parts):
        buf[:, :N, (lead + n) * C:(lead + n + 1) * C] = t.reshape(B, N, C)
    buf = buf.to(DEV)
    return [buf[:, :N, (lead + n) * C:(lead + n + 1) * C].view(B, N, H, hd) for n in range(len(parts))]


def operands(p, layout):
    """q, k, v on the device in that layout (see the module docstring)"""
    Nq, Nk = p.q.shape[1], p.k.shape[1]
    if layout == "separate":
        return _columns([p.q], Nq, 4, 0)[0], _columns([p.k], Nk, 8, 0)[0], _columns([p.v], Nk, 12, 0, lead=1)[0]
    pad = {"packed": (0, 0), "batch": (3, 5)}[layout]
    if Nq == Nk:
        return tuple(_columns([p.q, p.k, p.v], Nq, 0, pad[0]))
    return (_columns([p.q], Nq, 0, pad[0])[0],) + tuple(_columns([p.k, p.v], Nk, 0, pad[1]))


def device_mask(c, p):
    """the mask as the product sends it: bool, except where the bytes matter (`call` converts it for the per-row entries)"""
    m = p.qmask if c.rows else p.kmask
    return None if m is None else (m if c.mask == "bytes" else m != 0).to(DEV)


def call(c, q, k, v, scale, mask):
    from hipie_amd import ops
    B, Nq, H, hd = q.shape
    if c.rows:
        mask = mask.to(torch.uint8).contiguous()          # ops.attn_f32_rows would make this copy in front of `out`
    poisoned((B, Nq, H * hd))
    if c.rows:
        out = ops.attn_f32_rows(q, k, v, scale, mask, split=c.kernel == "split")
    else:
        out = (ops.attn_split if c.kernel == "split" else ops.attn_f32)(q, k, v, scale, key_mask=mask)
    assert out.dtype == F32 and out.shape == (B, Nq, H * hd) and out.is_contiguous()
    return out


def run(c, p):
    """-> the output (B, Nq, H, hd) on the host"""
    q, k, v = operands(p, c.layout)
    return call(c, q, k, v, p.scale, device_mask(c, p)).cpu().view(p.q.shape)


def check(c, got, want, denom=None):
    e = block_err(got, want, denom)
    print("block_err %s: %.3e (bound %.1e)" % (case_id(c), e, BOUND))
    assert e < BOUND, (case_id(c), e)


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_attn(c):
    p, want = problem(c)
    check(c, run(c, p), want)


@gpu
@pytest.mark.parametrize("c", RANGE, ids=case_id)
def test_small_v(c):
    """attn_split at the smallest V scale its format carries (SMALL_V_LOG2, from the emulation); attn_f32 2^-20 below it"""
    p, want = problem(c)
    e = SMALL_V_LOG2[c.hd] - (0 if c.kernel == "split" else 20)
    check(c, run(c, v_scaled(p, e)), want * 2.0 ** e)


@gpu
@pytest.mark.parametrize("c", SINK, ids=case_id)
def test_sink(c):
    """one dominant key with a small V over a 909-key tail: attn_split within the bound of max|v| over the attended keys (its P_lo has
    an absolute floor), attn_f32 within the bound of the block's own scale"""
    p, want = problem(c)
    check(c, run(c, p), want, sink_denominator(p) if c.kernel == "split" else None)


@gpu
@pytest.mark.parametrize("c", [c for c in random_value_cases() if c.kernel == "split"], ids=case_id)
def test_split_matches_f32(c):
    """the two kernels on the same operands: within twice the mutual difference of their emulations"""
    p, _ = problem(c)
    a, b = run(c, p), run(c._replace(kernel="f32"), p)
    e = block_err(a, b.double())
    print("attn_split against attn_f32 %s: %.3e (bound %.1e)" % (case_id(c), e, 2 * MUTUAL_DIFF))
    assert e < 2 * MUTUAL_DIFF, (case_id(c), e)


def same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


BITWISE = [c for c in CASES if c.B == 3 and c.H == 3 and (c.Nq, c.Nk) == (129, 129)]


@gpu
@pytest.mark.parametrize("c", [c for c in CASES if not c.rows and c.mask in ("holes", "all_masked", "prefix_masked")], ids=case_id)
def test_key_mask_equals_row_mask(c):
    """a key mask and the same mask expanded to (B, Nq, Nk) through the _rows entry: the same scores, the same bits"""
    p, _ = problem(c)
    q, k, v = operands(p, c.layout)
    km = p.kmask.to(DEV)
    a = call(c, q, k, v, p.scale, km)
    b = call(c._replace(rows=True), q, k, v, p.scale, km[:, None, :].expand(c.B, c.Nq, c.Nk))
    assert bool(torch.isfinite(a).all()) and same_bits(a, b)


@gpu
@pytest.mark.parametrize("c", BITWISE, ids=case_id)
def test_batch_invariance_and_repeat(c):
    """item b of the B = 3 call equals the B = 1 call on that item, and a second call on the same operands equals the first, bit for bit"""
    p, _ = problem(c)
    q, k, v = operands(p, c.layout)
    m = device_mask(c, p)
    whole = call(c, q, k, v, p.scale, m)
    assert bool(torch.isfinite(whole).all()) and same_bits(whole, call(c, q, k, v, p.scale, m))
    for b in range(c.B):
        one = call(c, q[b:b + 1], k[b:b + 1], v[b:b + 1], p.scale, m[b:b + 1])
        assert same_bits(whole[b], one[0]), b


SENTINEL = -7.0
GUARD_ROWS = 128                              # a workgroup's queries


def call_entry(c, q, k, v, mask, out, B, H, Nq, Nk, hd, scale, strides=None):
    from hipie_amd import ops
    strides = strides or (q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1))
    ops._call(ENTRY[c.kernel, c.rows], q.data_ptr(), k.data_ptr(), v.data_ptr(), ops._ptr(mask), out.data_ptr(), B, H, Nq, Nk, hd, *strides, float(scale))


@gpu
@pytest.mark.parametrize("c", GUARDED, ids=case_id)
def test_guarded_output(c):
    """`out` in the middle of a sentinel-filled buffer, a workgroup's 128 rows of guard on both sides: every row is written (the result
    meets the bound) and nothing beyond (the tail queries of the ragged last tile clamp their loads and must not store)"""
    p, want = problem(c)
    B, Nq, H, hd = p.q.shape
    guard, n = GUARD_ROWS * H * hd, B * Nq * H * hd
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=F32, device=DEV)
    q, k, v = operands(p, c.layout)
    m = p.qmask if c.rows else p.kmask
    call_entry(c, q, k, v, m.to(DEV).contiguous(), buf[guard:guard + n], B, H, Nq, p.k.shape[1], hd, p.scale)
    torch.cuda.synchronize()
    host = buf.cpu()
    fill = torch.full((guard,), SENTINEL).view(torch.int32)
    assert torch.equal(host[:guard].view(torch.int32), fill) and torch.equal(host[guard + n:].view(torch.int32), fill)
    check(c, host[guard:guard + n].view(B, Nq, H, hd), want)


@gpu
@pytest.mark.parametrize("kernel,rows", [(k, r) for k in ("f32", "split") for r in (False, True)], ids=lambda x: str(x))
def test_refusals(kernel, rows):
    """what the C entries refuse is an error with the reason in it, nothing is launched and the output stays untouched"""
    from hipie_amd import ops
    from hipie_amd._lib import HipieLibraryError
    c = Case(kernel, rows, 32, 2, 2, 5, 7, "refusal", "refusal", "ones")
    B, H, Nq, Nk = c.B, c.H, c.Nq, c.Nk
    mask = torch.ones(B, Nq, Nk, dtype=torch.uint8, device=DEV) if rows else torch.ones(B, Nk, dtype=torch.uint8, device=DEV)

    def wrapper(q, k, v):
        return call(c, q, k, v, 1.0, mask)
    for hd in (16, 80, 128):
        q, k, v = (torch.zeros(B, n, H, hd, device=DEV) for n in (Nq, Nk, Nk))
        out = torch.full((B, Nq, H * hd), SENTINEL, device=DEV)
        with pytest.raises(HipieLibraryError, match="head_dim"):
            call_entry(c, q, k, v, mask, out, B, H, Nq, Nk, hd, 1.0)
        with pytest.raises(HipieLibraryError, match="head_dim"):
            wrapper(q, k, v)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    hd, C = 32, 64
    q, k, v = (torch.zeros(B, n, H, hd, device=DEV) for n in (Nq, Nk, Nk))
    out = torch.full((B * Nq * C + 4,), SENTINEL, device=DEV)

    def off(N):                                       # a view at a storage offset of one element
        return torch.zeros(B * N * C + 4, device=DEV)[1:1 + B * N * C].view(B, N, H, hd)
    for args in ((off(Nq), k, v, mask, out), (q, off(Nk), v, mask, out), (q, k, off(Nk), mask, out), (q, k, v, mask, out[1:])):
        with pytest.raises(HipieLibraryError, match="16-byte aligned"):
            call_entry(c, *args, B, H, Nq, Nk, hd, 1.0)
    for args in ((off(Nq), k, v), (q, off(Nk), v)):
        with pytest.raises(HipieLibraryError, match="16-byte aligned"):
            wrapper(*args)

    def wide(N):                                      # a row stride of C + 2 elements (N is odd: the batch stride stays a multiple of 4)
        return torch.zeros(B, N + 1, C + 2, device=DEV)[:, :N, :C].view(B, N, H, hd)

    def apart(N):                                     # a batch stride of N C + 2 elements
        return torch.zeros(B, N * C + 2, device=DEV)[:, :N * C].view(B, N, H, hd)
    for make, which in ((wide, 1), (apart, 0)):
        t = make(Nk)
        assert t.stride(which) % 4 == 2 and t.stride(1 - which) % 4 == 0 and t.data_ptr() % 16 == 0
        for args in ((make(Nq), k, v), (q, make(Nk), v), (q, k, make(Nk))):
            with pytest.raises(HipieLibraryError, match="multiples of 4"):
                call_entry(c, *args, mask, out, B, H, Nq, Nk, hd, 1.0)
            with pytest.raises(HipieLibraryError, match="multiples of 4"):
                wrapper(*args)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
