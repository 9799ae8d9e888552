"""The 16-bit flash attention family (hipie_amd/csrc/flash_attn.hip and bi_xattn.hip: ops.flash_attn, ops.vit_attn, ops.vit_attn_fused,
ops.bi_xattn) against float64 references, over every launch line a shipped build can reach.

Launch lines and a test id that reaches each (T = f16_t | bf16_t; every line below runs in both):

  dispatch_hd   case 32 / 64 / 80 / 256                        test_generic[hd32-f16-q130-k128-bh8-none-c0-o16], [hd64-...], [hd80-...], [hd256-f16-q130-k64-...]
                default (head_dim refused)                     test_refusals
  dispatch_nb   FUSEREL  <HD,2,1,4,true,false,false,true>      test_vit_attn_fused[kh1-hd64-f16] .. [kh33-hd80-bf16]
                         any other grid                        tests/test_gpu_kernels.py::test_vit_attention_fused_rejects_other_grids
                bias nb 1 full / ragged                        test_bias[kw32-q37-hd64-f16] / test_bias[kw5-q37-hd64-f16]
                bias nb 2 full / ragged (4 waves)              test_bias[kw64-q130-hd80-bf16] / test_bias[kw40-q130-hd80-bf16], test_vit_attn_entry[40x40]
                bias nb 3 full / ragged                        test_bias[kw96-q130-hd64-f16] / test_bias[kw70-q130-hd64-f16], test_vit_attn_entry[3x70]
                bias nb > 3 (kw > 96 refused)                  test_refusals
                no bias, CLAMP, MASKED                         test_generic[hd64-f16-q130-k191-bh6-holes-cbind-o16]
                no bias, CLAMP, full tiles                     test_generic[hd64-f16-q33-k128-bh6-none-cbind-f32], [hd64-f16-q130-k64-bh6-none-c50000-o16]
                no bias, no clamp, MASKED                      test_generic[hd64-f16-q1-k65-bh8-none-c0-o16] (ragged tail), [hd64-f16-q33-k191-bh8-prefix-c0-f32]
                no bias, no clamp, full tiles                  test_generic[hd64-f16-q130-k128-bh8-none-c0-o16]
                (the same four at every hd and in bf16: test_generic_matrix_covers_every_instantiation)
  xattn_i2t_try return 1 (L <= 64, L > 224: generic kernel)    test_bi_xattn[L20-nv257-f16-holes-o16], [L64-nv255-f16-prefix-o16], [L225-nv257-f16-holes-o16]
                NKB 4 (64 < L <= 128) / NKB 7 (L <= 224)       test_bi_xattn[L65-nv1-f16-last-o16], [L128-nv257-bf16-holes-o16] / [L129-nv255-bf16-prefix-o16],
                                                               [L224-nv520-f16-last-o16]; each L in f16 and bf16 (test_bi_inputs_have_their_properties)
  xattn_t2i_try return 1 (no workspace: same L limits)         the same L = 20, 64, 225 cases
                NKB 4 / NKB 7 + combine                        the same L = 65 .. 224 cases; two splits: [L224-nv520-f16-last-o16]
                a split without tiles (combine guard)          test_bi_xattn_empty_split
  hipie_bi_xattn_ws  out_f32: both directions generic          test_bi_xattn[L129-nv520-bf16-holes-f32]

Not reachable from a shipped build, hence not tested here: the 8-wave (`wide`, BWL) instantiations of dispatch_nb case 2 and the forced
generic / forced split count paths sit behind HIPIE_FA_WAVES, HIPIE_FA_DEFER, HIPIE_XATTN_GENERIC and HIPIE_XT_SP, which study_env
compiles out without -DHIPIE_STUDY_KNOBS.

Files.  This file covers flash_attn.hip and bi_xattn.hip only; vit_attn.hip (vit_attn_rel) and vit_attn_split.hip have their own file
of this kind, tests/test_gpu_vit_attn.py, and so have attn_f32.hip and attn_split.hip, tests/test_gpu_small_attn.py.  Not covered by a
conformance file of this kind yet: the training kernels (attn_train*.hip); their tests are the older ones in tests/test_gpu_kernels.py,
which stay as they are.

References, both in float64 on the values the kernel reads (16-bit operands are rounded first, then upcast).  `ref_attn` is the formula of
the header of flash_attn.hip in torch:  s[i,j] = clamp(scale q_i.k_j, +-clamp) + bias_h[j // kw, i] + bias_w[i, j % kw], masked keys
-inf, softmax over j, a row with no attended key gives zeros.  `ref_loops` states the same in plain numpy loops over (b, h, i, j) and is
used on the tiny exact-edge inputs only; test_references_agree checks the two to 1e-12 on the CPU.  ops.bi_xattn is compared with
oracle.ops.bi_attention_core in float64 wherever a batch item attends a token (its -9e15 fill and second clamp are the model's own
formulation, so "mask = -inf" is checked against it), and with ref_attn for all-masked items and for a clamp other than 50000.
ops.vit_attn_fused is compared with ref_attn fed the decomposed bias built in float64 from the rounded tables and the rounded q.

Metric: util.rel_err per (batch, head) slice, the maximum over slices (`slice_err`).  V is scaled per head by 1, 1/8, 8, so a head that
is wrong by its own magnitude, or reads another head's values, fails although the global metric would pass it.

Bounds (header of tests/test_gpu_kernels.py): fp16 1e-3, bf16 8e-3 against the float64 reference on the same rounded operands, with or
without out_f32 (the rounding of P remains).  No bound comes from the kernel.  That they are attainable is shown on the CPU: `emu_attn`
emulates the format choice (fp32 scores, P = exp(s - max) rounded to the operand type, fp32 PV, division by the fp32 sum, output rounded
unless out_f32) and test_emulation_within_half_bound asserts its slice_err <= bound / 2 on every case of every matrix below;
EMULATION_ERR records the largest value per group (docs/measurements.md).  For that to hold in fp16, where rounding the output alone can
cost 2^-11 = 4.9e-4 of a slice's scale, `settle` places the largest output of every slice at 1.9375 x a power of two.

Output buffers: ops.* allocate them with torch.empty.  `poisoned` frees a NaN-filled block of the same size just before each call, so
that a row the kernel never writes shows as NaN (rel_err refuses it) instead of passing on stale data of an earlier, correct call."""
import collections
import functools
import itertools
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import ops as oo
from util import rel_err

torch.set_grad_enabled(False)
DEV = "cuda"
gpu = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
DTS = (F16, BF16)
TOL = {F16: 1e-3, BF16: 8e-3}
NAME = {F16: "f16", BF16: "bf16"}
V_SCALE = (1.0, 0.125, 8.0)                 # per head, cycled
BIND_SHARE = 0.05                           # a "binding" clamp changes at least this share of the logits

# Largest slice_err of emu_attn against the float64 reference per (group, operand type, out_f32), measured on the CPU by
# test_emulation_within_half_bound (which re-measures them: each must stay at or below its entry and above half of it; the entries are
# the measured values plus 1 %).  Half of the bound is 5e-4 (fp16) / 4e-3 (bf16).
EMULATION_ERR = {
    ("generic", "f16", False): 4.55e-4, ("generic", "f16", True): 2.68e-4, ("generic", "bf16", False): 3.67e-3, ("generic", "bf16", True): 1.85e-3,
    ("deferred_max", "f16", False): 4.56e-4, ("deferred_max", "bf16", False): 3.46e-3,
    ("bias", "f16", False): 3.95e-4, ("bias", "bf16", False): 2.96e-3,
    ("fused", "f16", False): 3.42e-4, ("fused", "bf16", False): 2.82e-3,
    ("bi", "f16", False): 4.22e-4, ("bi", "f16", True): 2.19e-4, ("bi", "bf16", False): 3.17e-3, ("bi", "bf16", True): 1.77e-3,
}


# --------------------------------------------------------------------------------------------------------------- references
def _scores(q, k, scale, key_mask, clamp, bias_h, bias_w, kw, ft):
    """(B,H,Nq,Nk) scores in float type ft; q (B,Nq,H,hd), k (B,Nk,H,hd); bias_h (B*H,kh,Nq), bias_w (B*H,Nq,kw); key_mask (B,Nk)"""
    B, Nq, H, _ = q.shape
    Nk = k.shape[1]
    s = torch.einsum("bihd,bjhd->bhij", q.cpu().to(ft), k.cpu().to(ft)) * scale
    if clamp > 0:
        s = s.clamp(-clamp, clamp)
    if bias_h is not None:
        kh = Nk // kw
        bh = bias_h.cpu().to(ft).view(B, H, kh, Nq).permute(0, 1, 3, 2)
        bw = bias_w.cpu().to(ft).view(B, H, Nq, kw)
        s = (s.view(B, H, Nq, kh, kw) + bh[..., None] + bw[:, :, :, None, :]).reshape(B, H, Nq, Nk)
    if key_mask is not None:
        s = s.masked_fill(~key_mask.cpu().bool()[:, None, None, :], -math.inf)
    return s


def ref_attn(q, k, v, scale, key_mask=None, clamp=0.0, bias_h=None, bias_w=None, kw=None):
    """float64 reference of the attention core -> (B,Nq,H,hd); a query with no attended key gives zeros"""
    s = _scores(q, k, scale, key_mask, clamp, bias_h, bias_w, kw, torch.float64)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    p = torch.where(l > 0, p / l, torch.zeros_like(p))
    return torch.einsum("bhij,bjhd->bihd", p, v.cpu().double())


def ref_loops(q, k, v, scale, key_mask=None, clamp=0.0, bias_h=None, bias_w=None, kw=None):
    """The formula of the header of flash_attn.hip written out: one loop iteration per (b, h, i, j), numpy float64."""
    q, k, v = (t.cpu().double().numpy() for t in (q, k, v))
    B, Nq, H, hd = q.shape
    Nk = k.shape[1]
    out = np.zeros((B, Nq, H, hd))
    for b, h, i in itertools.product(range(B), range(H), range(Nq)):
        s = np.full(Nk, -np.inf)
        for j in range(Nk):
            if key_mask is not None and not bool(key_mask[b, j]):
                continue
            x = scale * float(np.dot(q[b, i, h], k[b, j, h]))
            if clamp > 0:
                x = min(max(x, -clamp), clamp)
            if bias_h is not None:
                x += float(bias_h[b * H + h, j // kw, i]) + float(bias_w[b * H + h, i, j % kw])
            s[j] = x
        if np.isfinite(s).any():
            w = np.exp(s - s.max())
            out[b, i, h] = (w[:, None] * v[b, :, h]).sum(0) / w.sum()
    return torch.from_numpy(out)


def emu_attn(q, k, v, scale, key_mask=None, clamp=0.0, bias_h=None, bias_w=None, kw=None, out_f32=False):
    """CPU emulation of the kernels' format choice (not of their order of operations): fp32 scores, P = exp(s - max) rounded to the
    operand type, fp32 PV, division by the fp32 sum of the unrounded P, output rounded to the operand type unless out_f32"""
    dt = q.dtype
    s = _scores(q, k, float(np.float32(scale)), key_mask, clamp, bias_h, bias_w, kw, torch.float32)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True).permute(0, 2, 1, 3)
    o = torch.einsum("bhij,bjhd->bihd", p.to(dt).float(), v.cpu().float())
    o = torch.where(l > 0, o / l, torch.zeros_like(o))
    return (o if out_f32 else o.to(dt)).double()


def ref_bi(q, k, vv, vl, mask):
    """oracle.ops.bi_attention_core in float64 on (B,N,H,hd) operands -> out_v (B,Nv,H,hd), out_l (B,L,H,hd)"""
    B, Nv, H, hd = q.shape
    L = k.shape[1]

    def split(t):
        return t.cpu().double().transpose(1, 2).reshape(B * H, t.shape[1], hd)
    wv, wl = oo.bi_attention_core(split(q), split(k), split(vv), split(vl), mask.cpu().long())
    return wv.view(B, H, Nv, hd).transpose(1, 2), wl.view(B, H, L, hd).transpose(1, 2)


def slice_err(got, want):
    """max over (batch, head) of rel_err; got (B,N,H*hd) or (B,N,H,hd) from the kernel or the emulation, want (B,N,H,hd) float64"""
    B, N, H, hd = want.shape
    got = got.detach().cpu().double().reshape(B, N, H, hd)
    return max(rel_err(got[b, :, h], want[b, :, h]) for b in range(B) for h in range(H))


# ------------------------------------------------------------------------------------------------------------------- inputs
def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def head_scaled(v):
    """(B,N,H,hd) values with the per-head scale 1, 1/8, 8"""
    return v * torch.tensor([V_SCALE[h % 3] for h in range(v.shape[2])]).view(1, 1, -1, 1)


def key_tile(hd):
    """keys per tile of the no-bias instantiations (dispatch_hd: NBN = 1 at hd 256, else 2)"""
    return 32 if hd == 256 else 64


def make_mask(kind, B, Nk, KT, g):
    if kind == "none":
        return None
    m = torch.zeros(B, Nk, dtype=torch.bool)
    for b in range(B):
        if kind == "prefix":
            m[b, :max(1, Nk - 3 - 5 * b)] = True
        elif kind == "holes":                       # key 0 kept, key 1 dropped, one late key kept: never a prefix
            m[b] = torch.rand(Nk, generator=g) < 0.5
            m[b, 0], m[b, 1], m[b, Nk - 1 - b] = True, False, True
        elif kind == "late":                        # a few keys in tile 0, none in the middle tiles, one in the last tile
            m[b, [b, 3 + b, 7 + 2 * b]] = True
            m[b, Nk - 2 - b] = True
        elif kind == "early":                       # nothing after tile 0
            m[b, :KT] = torch.rand(KT, generator=g) < 0.6
            m[b, 0], m[b, KT - 1 - b] = True, True
        elif kind == "last":                        # a single attended key at position Nk - 1
            m[b, Nk - 1] = True
        elif kind == "all_masked":                  # item 0 a prefix, every later item without an attended key
            m[b, :max(1, Nk - 3)] = (b == 0)
        else:
            raise ValueError(kind)
    return m


def check_mask(kind, m, KT):
    """the property the mask's name claims, per batch item"""
    if kind == "none":
        assert m is None
        return
    for b, row in enumerate(m.tolist()):
        n, Nk = sum(row), len(row)
        last = max((j for j in range(Nk) if row[j]), default=-1)
        if kind == "prefix":
            assert 1 <= n and row == [True] * n + [False] * (Nk - n)
        elif kind == "holes":
            assert row[0] and n >= 2 and last > n - 1                       # an unattended key in front of an attended one
        elif kind == "late":
            nt = (Nk + KT - 1) // KT
            assert nt >= 3 and 1 <= sum(row[:KT]) <= 4 and sum(row[KT:(nt - 1) * KT]) == 0 and sum(row[(nt - 1) * KT:]) == 1
        elif kind == "early":
            assert Nk == 5 * KT and row[0] and last < KT and sum(row[KT:]) == 0 and n < KT
        elif kind == "last":
            assert n == 1 and row[Nk - 1]
        elif kind == "all_masked":
            assert (n > 0) == (b == 0) and len(m) >= 2


def bind_share(q, k, scale, clamp):
    """share of the unclamped float64 logits of the rounded operands that the clamp changes"""
    s = _scores(q, k, scale, None, 0.0, None, None, None, torch.float64)
    return float((s.abs() > clamp).double().mean())


Problem = collections.namedtuple("Problem", "q k v scale key_mask clamp bias_h bias_w kw")
Problem.__new__.__defaults__ = (None, 0.0, None, None, None)
OUT_MANTISSA = 1.9375                          # of the largest |reference| of every (batch, head) slice, see `settle`


def settle(p):
    """-> (problem, float64 reference) with V of every (batch, head) slice rescaled by a factor in (0.96, 1.94] such that the largest
    |reference| of the slice is OUT_MANTISSA x a power of two.  Rounding the output to 16 bit then costs at most 2^-11 / 1.9375 = 2.5e-4
    (fp16) or 2^-9 / 1.9375 = 1.0e-3 (bf16) of the slice's scale, wherever the seed put that maximum; without this the worst slice of a
    case has its maximum just above a power of two and the output rounding alone takes 4.9e-4 of the 5e-4 that test_emulation_within_
    half_bound allows in fp16.  The reference is computed on the rescaled, re-rounded V."""
    m = ref_attn(*p).abs().amax((1, 3))                                                 # (B, H)
    f = torch.where(m > 0, OUT_MANTISSA * torch.exp2(torch.floor(torch.log2(m.clamp_min(1e-300)))) / m.clamp_min(1e-300), torch.ones_like(m))
    p = p._replace(v=(p.v.double() * f[:, None, :, None]).to(p.v.dtype))
    return p, ref_attn(*p)


# ---- generic path: ops.flash_attn without bias ----
GenericCase = collections.namedtuple("GenericCase", "hd dt Nq Nk B H mask clamp out_f32")
CLAMP_BIND = 1.5                               # unit-scale logits: about 13 % lie outside +-1.5
CLAMP_NAME = {0.0: "c0", 50000.0: "c50000", CLAMP_BIND: "cbind"}


def generic_id(c):
    return "hd%d-%s-q%d-k%d-bh%d-%s-%s-%s" % (c.hd, NAME[c.dt], c.Nq, c.Nk, c.B * c.H, c.mask, CLAMP_NAME[c.clamp], "f32" if c.out_f32 else "o16")


def _generic_cases():
    """The axes of the issue, pruned: per (hd, dtype) every (MASKED, CLAMP) instantiation of dispatch_nb; every Nk form (one tile, a
    multiple of the tile without a mask, KT + 1, 3 KT - 1, a multiple with a mask, 5 tiles with an early stop, 1); Nq 1 / 33 / 130;
    B*H 8 (swz) and 6 (no swz, with two query tiles in three of the cases); every mask form; the three clamps; out_f32 both ways."""
    out = []
    for hd, dt in itertools.product((32, 64, 80, 256), DTS):
        KT = key_tile(hd)
        for Nq, Nk, (B, H), mask, clamp, f32 in (
                (130, 2 * KT, (2, 4), "none", 0.0, False),                 # full tiles, no clamp
                (33, 2 * KT, (2, 3), "none", CLAMP_BIND, True),            # full tiles, binding clamp
                (130, KT, (2, 3), "none", 50000.0, False),                 # exactly one tile, the callers' clamp
                (1, KT + 1, (2, 4), "none", 0.0, False),                   # ragged tail of one key, one query
                (130, 3 * KT - 1, (2, 3), "holes", CLAMP_BIND, False),
                (33, 3 * KT - 1, (2, 4), "prefix", 0.0, True),
                (33, 3 * KT, (2, 3), "late", 50000.0, False),
                (130, 5 * KT, (2, 4), "early", 0.0, False),
                (33, 1, (2, 3), "none", 0.0, False),                       # one key: the output is v
                (1, 1, (2, 4), "none", 50000.0, True),
                (130, KT + 1, (2, 3), "holes", 0.0, True)):
            out.append(GenericCase(hd, dt, Nq, Nk, B, H, mask, clamp, f32))
    return out


GENERIC = _generic_cases()


def qkv_unit(g, B, Nq, Nk, H, hd, dt):
    """q, k of unit variance (scale hd**-0.5 then gives unit-scale logits), v head-scaled; rounded to dt"""
    q = torch.randn(B, Nq, H, hd, generator=g).to(dt)
    k = torch.randn(B, Nk, H, hd, generator=g).to(dt)
    v = head_scaled(torch.randn(B, Nk, H, hd, generator=g)).to(dt)
    return q, k, v


@functools.lru_cache(maxsize=None)
def generic_problem(c):
    g = gen(generic_id(c))
    KT = key_tile(c.hd)
    q, k, v = qkv_unit(g, c.B, c.Nq, c.Nk, c.H, c.hd, c.dt)
    mask = make_mask(c.mask, c.B, c.Nk, KT, g)
    p, want = settle(Problem(q, k, v, c.hd ** -0.5, mask, c.clamp))
    if c.mask == "early":                          # the skipped K / V rows: finite, and dominant if they reached the softmax
        big = 6e4 if c.dt == F16 else 1e30
        for t in (p.k, p.v):
            t[:, KT:] = torch.where(torch.randn(t[:, KT:].shape, generator=g) > 0, big, -big).to(c.dt)
        want = ref_attn(*p)
    return p, want


# ---- deferred running max (bf16: kDefer = 8; fp16: the classic running max on the same inputs) ----
DEFER = [(inp, dt) for inp in ("steps", "jump") for dt in DTS]
DEFER_HD, DEFER_TILES = 64, 6


@functools.lru_cache(maxsize=None)
def defer_problem(inp, dt):
    """keys of tile t shifted along one direction so that every row's maximum rises by about 3 (log2 units) per tile -- the bf16 kernel
    then moves its reference point only every third tile; "jump": the last tile rises by 20 more."""
    g = gen("defer-" + inp)
    B, H, Nq, hd, KT = 2, 4, 130, DEFER_HD, key_tile(DEFER_HD)
    Nk = DEFER_TILES * KT
    u = torch.randn(hd, generator=g)
    u = u / u.norm()
    q = torch.randn(B, Nq, H, hd, generator=g) * 0.5
    q = q - (q @ u)[..., None] * u + math.sqrt(hd) * u                    # q.u = sqrt(hd) exactly (before rounding): scale * q.(c u) = c
    k = torch.randn(B, Nk, H, hd, generator=g)
    k = k - (k @ u)[..., None] * u
    rise = 3.0 * math.log(2.0) * torch.arange(DEFER_TILES).repeat_interleave(KT).double()
    if inp == "jump":
        rise[-KT:] += 20.0 * math.log(2.0)
    k = k + rise.float()[None, :, None, None] * u
    v = head_scaled(torch.randn(B, Nk, H, hd, generator=g))
    return settle(Problem(q.to(dt), k.to(dt), v.to(dt), hd ** -0.5))


def tile_max_steps(p, KT):
    """median over (b, h, i) of the rise of the per-tile row maximum from tile t to t + 1, in log2 units -> (ntiles - 1,)"""
    s = _scores(p.q, p.k, p.scale, None, 0.0, None, None, None, torch.float64) * math.log2(math.e)
    tm = s.view(*s.shape[:3], -1, KT).amax(-1)
    return (tm[..., 1:] - tm[..., :-1]).flatten(0, 2).median(0).values


# ---- bias path: ops.flash_attn(bias_h, bias_w) with random fp32 biases, Nq != Nk ----
BiasCase = collections.namedtuple("BiasCase", "kw Nq hd dt")
BIAS = [BiasCase(kw, Nq, hd, dt) for kw in (5, 32, 40, 64, 70, 96) for Nq in (37, 130) for hd in (64, 80) for dt in DTS]
BIAS_KH = 3


def bias_id(c):
    return "kw%d-q%d-hd%d-%s" % (c.kw, c.Nq, c.hd, NAME[c.dt])


@functools.lru_cache(maxsize=None)
def bias_problem(c):
    g = gen(bias_id(c))
    B, H, Nk = 2, 2, BIAS_KH * c.kw
    q, k, v = qkv_unit(g, B, c.Nq, Nk, H, c.hd, c.dt)
    bias_h = torch.randn(B * H, BIAS_KH, c.Nq, generator=g)
    bias_w = torch.randn(B * H, c.Nq, c.kw, generator=g)
    return settle(Problem(q, k, v, c.hd ** -0.5, None, 0.0, bias_h, bias_w, c.kw))


# ---- packed-qkv entry points: ops.vit_attn (bias given) and ops.vit_attn_fused (bias from the tables) ----
def some_queries(N, g, n=200):
    """all queries of a small grid; of a large one the first and the last 64 and n random ones (the op is independent per query)"""
    if N <= 2 * 64 + n:
        return torch.arange(N)
    return torch.cat([torch.arange(64), torch.arange(N - 64, N), torch.randperm(N - 128, generator=g)[:n].sort().values + 64])


def pack_qkv(q, k, v):
    """(B,N,heads,hd) each -> (B, N, 3*heads*hd) packed as (3, heads, hd)"""
    return torch.stack([q, k, v], 2).flatten(2).contiguous()


VIT_ENTRY = [(40, 40), (3, 70)]                # (gh, gw): nb = 2 ragged, nb = 3 ragged; hd 80, bf16


@functools.lru_cache(maxsize=None)
def vit_entry_problem(grid):
    gh, gw = grid
    g = gen("vit-%dx%d" % grid)
    B, heads, hd, N = 1, 2, 80, gh * gw
    q, k, v = qkv_unit(g, B, N, N, heads, hd, BF16)
    rel_h = torch.randn(B * heads, gh, N, generator=g)
    rel_w = torch.randn(B * heads, N, gw, generator=g)
    idx = some_queries(N, g)
    p, want = settle(Problem(q[:, idx], k, v, hd ** -0.5, None, 0.0, rel_h[:, :, idx], rel_w[:, idx], gw))
    return (pack_qkv(q, k, p.v), rel_h, rel_w, heads, idx), p, want


FusedCase = collections.namedtuple("FusedCase", "kh hd dt")
FUSED = [FusedCase(kh, hd, dt) for kh in (1, 2, 32, 33) for hd in (64, 80) for dt in DTS]
FUSED_KW = 64


def fused_id(c):
    return "kh%d-hd%d-%s" % (c.kh, c.hd, NAME[c.dt])


def decomposed_bias(q, th, tw, kh, kw):
    """add_decomposed_rel_pos in float64 from the rounded q (B,N,heads,hd) and tables: bias_h (B*heads,kh,N), bias_w (B*heads,N,kw),
    bias_h[q, ky] = q . Rh[qy - ky + kh - 1], bias_w[q, kx] = q . Rw[qx - kx + kw - 1] (the tables indexed directly)"""
    B, N, heads, hd = q.shape
    Rh = th.double()[torch.arange(kh)[:, None] - torch.arange(kh)[None, :] + kh - 1]
    Rw = tw.double()[torch.arange(kw)[:, None] - torch.arange(kw)[None, :] + kw - 1]
    rq = q.double().reshape(B, kh, kw, heads, hd)
    bias_h = torch.einsum("byxhc,ykc->bhkyx", rq, Rh).reshape(B * heads, kh, N)
    bias_w = torch.einsum("byxhc,xkc->bhyxk", rq, Rw).reshape(B * heads, N, kw)
    return bias_h, bias_w


@functools.lru_cache(maxsize=None)
def fused_problem(c):
    g = gen(fused_id(c))
    B, heads, N = 1, 3, c.kh * FUSED_KW
    q, k = ((torch.randn(B, N, heads, c.hd, generator=g) * 0.7).to(c.dt) for _ in range(2))
    v = head_scaled(torch.randn(B, N, heads, c.hd, generator=g)).to(c.dt)
    th = (torch.randn(2 * c.kh - 1, c.hd, generator=g) * 0.3).to(c.dt)
    tw = (torch.randn(2 * FUSED_KW - 1, c.hd, generator=g) * 0.3).to(c.dt)
    idx = some_queries(N, g)
    bias_h, bias_w = decomposed_bias(q, th, tw, c.kh, FUSED_KW)
    p, want = settle(Problem(q[:, idx], k, v, c.hd ** -0.5, None, 0.0, bias_h[:, :, idx], bias_w[:, idx], FUSED_KW))
    return (pack_qkv(q, k, p.v), th, tw, heads, idx), p, want


# ---- ops.bi_xattn: hd 256, H = 2 ----
BiCase = collections.namedtuple("BiCase", "L Nv dt mask out_f32 B clamp")
BI_L = (20, 64, 65, 128, 129, 224, 225)        # both sides of every boundary of xattn_i2t_try / xattn_t2i_try (64 | 128 | 224)
BI_NV = (1, 255, 257, 520)                     # 520 at B*H = 4: 17 tiles, SP = 2, 9 + 8 tiles, the last one ragged
BI_MASKS = ("prefix", "holes", "last")
BI_H, BI_HD = 2, 256
BI_CLAMP = 8.0


def bi_id(c):
    return "L%d-nv%d-%s-%s-%s%s%s" % (c.L, c.Nv, NAME[c.dt], c.mask, "f32" if c.out_f32 else "o16", "" if c.B == 2 else "-b%d" % c.B,
                                      "" if c.clamp == 50000.0 else "-clamp%g" % c.clamp)


def _bi_cases():
    """every (L, Nv); dtype, mask form and out_f32 rotate over them, then the other dtype of every L at Nv = 257 through the
    specialised kernels (16-bit output), so that each L runs both dtypes there"""
    out = []
    for (iL, L), (iN, Nv) in itertools.product(enumerate(BI_L), enumerate(BI_NV)):
        out.append(BiCase(L, Nv, DTS[(iL + iN) % 2], BI_MASKS[(iL + 2 * iN) % 3], (iL + iN) % 4 == 3, 2, 50000.0))
    for iL, L in enumerate(BI_L):
        out.append(BiCase(L, 257, DTS[(iL + 2 + 1) % 2], BI_MASKS[iL % 3], False, 2, 50000.0))
    return out


BI = _bi_cases()
BI_EMPTY_SPLIT = BiCase(70, 4130, F16, "holes", False, 1, 50000.0)
BI_CLAMPED = [BiCase(L, 257, dt, "holes", False, 2, BI_CLAMP) for L in (100, 20) for dt in DTS]
BI_ALL_MASKED = [BiCase(L, 130, DTS[(i + int(f32)) % 2], "all_masked", f32, 2, 50000.0) for i, L in enumerate((20, 100, 300)) for f32 in (False, True)]


def t2i_split_plan(B, H, Nv):
    """t2i_splits and the tiles_per_split of xattn_t2i_try (bi_xattn.hip) restated: (ntiles, SP, tiles per split)"""
    ntiles = (Nv + 31) // 32
    sp = max(1, min((256 + B * H - 1) // (B * H), 16, ntiles // 8))
    return ntiles, sp, (ntiles + sp - 1) // sp


@functools.lru_cache(maxsize=None)
def bi_problem(c):
    """-> (q, k, vv, vl, mask), the two attention problems (image -> text, text -> image), their float64 references (B,N,H,hd)"""
    g = gen(bi_id(c))
    # logits q.k (scale 1) of unit scale; with the binding clamp of standard deviation 5: about 11 % lie outside +-8
    sd = 0.25 if c.clamp == 50000.0 else math.sqrt(5.0 / 16.0)
    q = (torch.randn(c.B, c.Nv, BI_H, BI_HD, generator=g) * sd).to(c.dt)
    k = (torch.randn(c.B, c.L, BI_H, BI_HD, generator=g) * sd).to(c.dt)
    vv = head_scaled(torch.randn(c.B, c.Nv, BI_H, BI_HD, generator=g)).to(c.dt)
    vl = head_scaled(torch.randn(c.B, c.L, BI_H, BI_HD, generator=g)).to(c.dt)
    mask = make_mask(c.mask, c.B, c.L, 32, g)
    (pv, want_v), (pl, want_l) = settle(Problem(q, k, vl, 1.0, mask, c.clamp)), settle(Problem(k, q, vv, 1.0, None, c.clamp))
    vl, vv = pv.v, pl.v
    if c.clamp == 50000.0 and c.mask != "all_masked":
        want_v, want_l = ref_bi(q, k, vv, vl, mask)
    elif c.mask == "all_masked":               # the item that attends a token: against the oracle, like every other case
        want_v, want_l = want_v.clone(), want_l.clone()
        want_v[:1], want_l[:1] = ref_bi(q[:1], k[:1], vv[:1], vl[:1], mask[:1])
    return (q, k, vv, vl, mask), (pv, pl), (want_v, want_l)


# ---- a batch item with no attended key through ops.flash_attn ----
MaskedCase = collections.namedtuple("MaskedCase", "hd dt out_f32")
ALL_MASKED = [MaskedCase(hd, dt, f32) for hd in (64, 256) for dt in DTS for f32 in (False, True)]


def masked_id(c):
    return "hd%d-%s-%s" % (c.hd, NAME[c.dt], "f32" if c.out_f32 else "o16")


@functools.lru_cache(maxsize=None)
def masked_problem(c):
    g = gen("all-masked-" + masked_id(c))
    KT = key_tile(c.hd)
    q, k, v = qkv_unit(g, 2, 70, 2 * KT + 5, 3, c.hd, c.dt)
    return settle(Problem(q, k, v, c.hd ** -0.5, make_mask("all_masked", 2, 2 * KT + 5, KT, g), 50000.0))


# ---- tiny exact-edge inputs for the two references ----
def edge_problems():
    g = gen("edges")
    B, H, hd = 2, 2, 4

    def qkv(Nq, Nk):
        return (torch.randn(B, Nq, H, hd, generator=g).to(BF16), torch.randn(B, Nk, H, hd, generator=g).to(BF16),
                head_scaled(torch.randn(B, Nk, H, hd, generator=g)).to(BF16))
    yield "plain", Problem(*qkv(5, 7), 0.5)
    yield "one_query_one_key", Problem(*qkv(1, 1), 0.5)
    yield "holes", Problem(*qkv(3, 9), 0.5, make_mask("holes", B, 9, 4, g))
    yield "all_masked_item", Problem(*qkv(3, 9), 0.5, make_mask("all_masked", B, 9, 4, g))
    yield "binding_clamp", Problem(*qkv(4, 6), 1.0, make_mask("prefix", B, 6, 4, g), 0.75)
    yield "bias", Problem(*qkv(5, 6), 0.5, None, 0.0, torch.randn(B * H, 2, 5, generator=g), torch.randn(B * H, 5, 3, generator=g), 3)
    yield "bias_clamp", Problem(*qkv(2, 6), 1.0, None, 0.75, torch.randn(B * H, 3, 2, generator=g), torch.randn(B * H, 2, 2, generator=g), 2)


# -------------------------------------------------------------------------------------- CPU: references, inputs, bounds (no GPU)
def test_references_agree():
    for name, p in edge_problems():
        a, b = ref_attn(*p), ref_loops(*p)
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
        if name == "all_masked_item":
            assert torch.count_nonzero(a[1]) == 0 and torch.count_nonzero(a[0]) > 0
        if name in ("binding_clamp", "bias_clamp"):
            assert bind_share(p.q, p.k, p.scale, p.clamp) >= BIND_SHARE
        if name == "one_query_one_key":
            assert torch.equal(a, p.v.double())


def test_generic_matrix_covers_every_instantiation():
    """per (hd, dtype): both values of MASKED and of CLAMP in dispatch_nb, every Nk form, mask form, clamp, Nq, swz and out_f32"""
    for hd, dt in itertools.product((32, 64, 80, 256), DTS):
        cs = [c for c in GENERIC if (c.hd, c.dt) == (hd, dt)]
        KT = key_tile(hd)
        inst = {(c.mask != "none" or c.Nk % KT != 0, c.clamp > 0) for c in cs}
        assert inst == {(m, cl) for m in (False, True) for cl in (False, True)}
        assert {c.Nk for c in cs} == {1, KT, 2 * KT, KT + 1, 3 * KT - 1, 3 * KT, 5 * KT}
        assert {c.mask for c in cs} == {"none", "prefix", "holes", "late", "early"}
        assert {c.clamp for c in cs} == {0.0, 50000.0, CLAMP_BIND} and {c.Nq for c in cs} == {1, 33, 130}
        assert {c.out_f32 for c in cs} == {False, True}
        assert any(c.B * c.H % 8 == 0 and c.Nq > 128 for c in cs) and any(c.B * c.H % 8 != 0 and c.Nq > 128 for c in cs)
    assert len({generic_id(c) for c in GENERIC}) == len(GENERIC)


def test_generic_inputs_have_their_properties():
    for c in GENERIC:
        p, _ = generic_problem(c)
        check_mask(c.mask, p.key_mask, key_tile(c.hd))
        if c.clamp == CLAMP_BIND:
            assert bind_share(p.q, p.k, p.scale, c.clamp) >= BIND_SHARE, generic_id(c)
        if c.clamp == 50000.0:
            assert bind_share(p.q, p.k, p.scale, c.clamp) == 0.0
        if c.mask == "early":
            KT = key_tile(c.hd)
            for t in (p.k, p.v):
                assert torch.isfinite(t).all() and float(t[:, KT:].abs().min()) >= 6e4 > 100 * float(t[:, :KT].abs().max())


def test_deferred_max_inputs_have_their_properties():
    KT = key_tile(DEFER_HD)
    for inp, dt in DEFER:
        steps = tile_max_steps(defer_problem(inp, dt)[0], KT)
        assert steps.shape == (DEFER_TILES - 1,)
        assert all(2.0 < float(s) < 4.0 for s in steps[:-1]), (inp, steps)          # below kDefer = 8: no move on most tiles
        assert (2.0 < float(steps[-1]) < 4.0) if inp == "steps" else (float(steps[-1]) > 20.0), (inp, steps)


def test_bi_inputs_have_their_properties():
    assert {(c.L, c.Nv) for c in BI} == set(itertools.product(BI_L, BI_NV))
    for L in BI_L:                             # each L: both dtypes through the specialised kernels, every mask form somewhere, out_f32
        assert {c.dt for c in BI if c.L == L and not c.out_f32} == set(DTS)
        assert any(c.out_f32 for c in BI if c.L == L)
    assert {c.mask for c in BI} == set(BI_MASKS)
    for c in BI + [BI_EMPTY_SPLIT] + BI_CLAMPED + BI_ALL_MASKED:
        (q, k, vv, vl, mask), _, _ = bi_problem(c)
        check_mask(c.mask, mask, 32)
        share = bind_share(q, k, 1.0, c.clamp)
        assert (share >= BIND_SHARE) if c.clamp == BI_CLAMP else (share == 0.0), bi_id(c)
    # Nv = 520 at B*H = 4: 17 tiles in 2 splits of 9 and 8, the last tile ragged
    assert t2i_split_plan(2, BI_H, 520) == (17, 2, 9) and 520 % 32 != 0
    # the empty split: Nv = 4130 -> 130 tiles; SP = min(ceil(256 / 2) = 128, 16, 130 // 8 = 16) = 16; ceil(130 / 16) = 9 tiles per
    # split; split 15 would start at tile 135 >= 130: no tiles, and the combine kernel's m == -inf guard runs
    c = BI_EMPTY_SPLIT
    ntiles, sp, per = t2i_split_plan(c.B, BI_H, c.Nv)
    assert (ntiles, sp, per) == (130, 16, 9) and (sp - 1) * per >= ntiles > (sp - 2) * per and 64 < c.L <= 224


def emulation_groups():
    """(group, dtype, out_f32) -> list of (id, problem, reference): every case of every matrix of this file"""
    groups = collections.defaultdict(list)
    for c in GENERIC:
        groups["generic", c.dt, c.out_f32].append((generic_id(c),) + generic_problem(c))
    for inp, dt in DEFER:
        groups["deferred_max", dt, False].append((inp,) + defer_problem(inp, dt))
    for c in BIAS:
        groups["bias", c.dt, False].append((bias_id(c),) + bias_problem(c))
    for grid in VIT_ENTRY:
        groups["bias", BF16, False].append(("vit-%dx%d" % grid,) + vit_entry_problem(grid)[1:])
    for c in FUSED:
        groups["fused", c.dt, False].append((fused_id(c),) + fused_problem(c)[1:])
    for c in BI + [BI_EMPTY_SPLIT] + BI_CLAMPED + BI_ALL_MASKED:
        _, problems, wants = bi_problem(c)
        for side, p, want in zip("vl", problems, wants):
            groups["bi", c.dt, c.out_f32].append((bi_id(c) + "-out_" + side, p, want))
    for c in ALL_MASKED:
        groups["generic", c.dt, c.out_f32].append((masked_id(c),) + masked_problem(c))
    return groups


def emulation_err(p, want, out_f32):
    """slice_err of the emulation; an all-masked item (reference exactly zero) must be exactly zero and is left out of the maximum"""
    got = emu_attn(*p, out_f32=out_f32)
    live = [b for b in range(want.shape[0]) if torch.count_nonzero(want[b]) > 0]
    dead = [b for b in range(want.shape[0]) if b not in live]
    assert torch.count_nonzero(got[dead]) == 0
    return slice_err(got[live], want[live])


@pytest.mark.parametrize("group", ["generic", "deferred_max", "bias", "fused", "bi"])
def test_emulation_within_half_bound(group):
    """the bounds are attainable: the format choice alone stays within half of each on every case; and EMULATION_ERR is what it says"""
    for (grp, dt, f32), items in emulation_groups().items():
        if grp != group:
            continue
        worst = 0.0
        for name, p, want in items:
            e = emulation_err(p, want, f32)
            print("emulation %s %s %s %s: %.3e" % (grp, NAME[dt], "out_f32" if f32 else "rounded", name, e))
            assert e <= TOL[dt] / 2, (name, e)
            worst = max(worst, e)
        print("emulation worst %s %s %s: %.3e" % (grp, NAME[dt], "out_f32" if f32 else "rounded", worst))
        rec = EMULATION_ERR[grp, NAME[dt], f32]
        assert 0.5 * rec <= worst <= rec, (grp, NAME[dt], f32, worst, rec)


# --------------------------------------------------------------------------------------------------------------------- GPU
def poisoned(*shapes_dtypes):
    """free NaN-filled device blocks of the given (shape, dtype): the allocator hands the most recently freed block of a size to the
    next torch.empty of that size, so an element the kernel does not write reads NaN"""
    blocks = [torch.full(shape, math.nan, dtype=dt, device=DEV) for shape, dt in shapes_dtypes]
    del blocks


def run_flash(p, out_f32=False):
    from hipie_amd import ops
    B, Nq, H, hd = p.q.shape
    dev = [None if t is None else t.to(DEV) for t in (p.q, p.k, p.v, p.bias_h, p.bias_w, p.key_mask)]
    poisoned(((B, Nq, H * hd), torch.float32 if out_f32 else p.q.dtype))
    out = ops.flash_attn(dev[0], dev[1], dev[2], p.scale, bias_h=dev[3], bias_w=dev[4], key_mask=dev[5], clamp=p.clamp, out_f32=out_f32)
    assert out.dtype == (torch.float32 if out_f32 else p.q.dtype) and out.shape == (B, Nq, H * hd)
    return out.cpu()


def check(got, want, dt, what=""):
    e = slice_err(got, want)
    print("slice_err %s: %.3e (bound %.0e)" % (what, e, TOL[dt]))
    assert e < TOL[dt], (what, e)


@gpu
@pytest.mark.parametrize("c", GENERIC, ids=generic_id)
def test_generic(c):
    p, want = generic_problem(c)
    got = run_flash(p, c.out_f32)
    check(got, want, c.dt, generic_id(c))
    if c.Nk == 1:                                   # softmax over one key: the output IS v, whatever the query
        assert torch.equal(got.view(c.B, c.Nq, c.H, c.hd).to(c.dt), p.v.expand(c.B, c.Nq, c.H, c.hd))


@gpu
@pytest.mark.parametrize("hd,dt", [(32, F16), (64, BF16), (80, F16), (256, BF16)])
def test_generic_strided_views(hd, dt):
    """q, k, v as strided views of one packed buffer (head_dim contiguous) give the bits of dense copies"""
    from hipie_amd import ops
    KT = key_tile(hd)
    B, H, Nq, Nk = 2, 3, 130, 3 * KT - 1
    g = gen("strided-%d" % hd)
    packed = torch.randn(B, max(Nq, Nk), 3, H, hd, generator=g)
    packed[:, :, 2] = head_scaled(packed[:, :, 2])
    packed = packed.to(dt).to(DEV)
    q, k, v = packed[:, :Nq, 0], packed[:, :Nk, 1], packed[:, :Nk, 2]
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    poisoned(((B, Nq, H * hd), dt))
    a = ops.flash_attn(q, k, v, hd ** -0.5, clamp=50000.0)
    poisoned(((B, Nq, H * hd), dt))
    b = ops.flash_attn(q.contiguous(), k.contiguous(), v.contiguous(), hd ** -0.5, clamp=50000.0)
    assert torch.equal(a, b)
    check(a.cpu(), ref_attn(q, k, v, hd ** -0.5, None, 50000.0), dt, "strided hd%d" % hd)


@gpu
@pytest.mark.parametrize("inp,dt", DEFER, ids=["%s-%s" % (i, NAME[d]) for i, d in DEFER])
def test_deferred_max(inp, dt):
    p, want = defer_problem(inp, dt)
    check(run_flash(p), want, dt, "deferred max %s" % inp)


@gpu
@pytest.mark.parametrize("c", BIAS, ids=bias_id)
def test_bias(c):
    p, want = bias_problem(c)
    check(run_flash(p), want, c.dt, bias_id(c))


@gpu
def test_refusals():
    """kw > 96 with a bias, and a head_dim outside 32 / 64 / 80 / 256, are errors (no fall-back)"""
    from hipie_amd import ops
    q = torch.zeros(1, 8, 1, 64, dtype=F16, device=DEV)
    kv = torch.zeros(1, 97, 1, 64, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match="kw=97"):
        ops.flash_attn(q, kv, kv, 1.0, bias_h=torch.zeros(1, 1, 8, device=DEV), bias_w=torch.zeros(1, 8, 97, device=DEV))
    ops.flash_attn(q, kv[:, :96], kv[:, :96], 1.0, bias_h=torch.zeros(1, 1, 8, device=DEV), bias_w=torch.zeros(1, 8, 96, device=DEV))
    t = torch.zeros(1, 8, 1, 48, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim 48"):
        ops.flash_attn(t, t, t, 1.0)


@gpu
@pytest.mark.parametrize("grid", VIT_ENTRY, ids=["%dx%d" % g for g in VIT_ENTRY])
def test_vit_attn_entry(grid):
    """the packed-qkv entry point on a 40 x 40 grid (nb = 2, ragged) and a 3 x 70 grid (nb = 3, ragged), hd 80, bf16"""
    from hipie_amd import ops
    (qkv, rel_h, rel_w, heads, idx), p, want = vit_entry_problem(grid)
    poisoned((tuple(qkv.shape[:2]) + (qkv.shape[2] // 3,), BF16))
    got = ops.vit_attn(qkv.to(DEV), rel_h.to(DEV), rel_w.to(DEV), grid, heads, p.scale).cpu()
    assert torch.isfinite(got).all()
    check(got[:, idx], want, BF16, "vit_attn %dx%d" % grid)


@gpu
@pytest.mark.parametrize("c", FUSED, ids=fused_id)
def test_vit_attn_fused(c):
    """the bh_all prologue at 1, 2, 32 and 33 key rows (one 32-row block, its boundary, a second block of one row)"""
    from hipie_amd import ops
    (qkv, th, tw, heads, idx), p, want = fused_problem(c)
    assert ops.vit_attn_fused_ok((c.kh, FUSED_KW), c.hd)
    poisoned((tuple(qkv.shape[:2]) + (qkv.shape[2] // 3,), c.dt))
    got = ops.vit_attn_fused(qkv.to(DEV), th.to(DEV), tw.to(DEV), (c.kh, FUSED_KW), heads, p.scale).cpu()
    assert torch.isfinite(got).all()
    check(got[:, idx], want, c.dt, fused_id(c))


def run_bi(c):
    from hipie_amd import ops
    (q, k, vv, vl, mask), _, _ = bi_problem(c)
    odt = torch.float32 if c.out_f32 else c.dt
    poisoned(((c.B, c.Nv, BI_H * BI_HD), odt), ((c.B, c.L, BI_H * BI_HD), odt))
    out_v, out_l = ops.bi_xattn(q.to(DEV), k.to(DEV), vv.to(DEV), vl.to(DEV), mask.to(DEV), clamp=c.clamp, out_f32=c.out_f32)
    assert out_v.dtype == odt and out_l.dtype == odt
    return out_v.cpu(), out_l.cpu()


@gpu
@pytest.mark.parametrize("c", BI + BI_CLAMPED, ids=bi_id)
def test_bi_xattn(c):
    out_v, out_l = run_bi(c)
    want_v, want_l = bi_problem(c)[2]
    check(out_v, want_v, c.dt, bi_id(c) + " out_v")
    check(out_l, want_l, c.dt, bi_id(c) + " out_l")


@gpu
def test_bi_xattn_empty_split():
    """Nv = 4130 at B*H = 2: 130 tiles, 16 splits of 9 tiles, the last split has none (test_bi_inputs_have_their_properties)"""
    c = BI_EMPTY_SPLIT
    out_v, out_l = run_bi(c)
    want_v, want_l = bi_problem(c)[2]
    check(out_v, want_v, c.dt, "empty split out_v")
    check(out_l, want_l, c.dt, "empty split out_l")


@gpu
@pytest.mark.parametrize("c", ALL_MASKED, ids=masked_id)
def test_all_masked_flash_attn(c):
    """a query with no attended key gives zeros: item 1 has no attended key, item 0 a prefix"""
    p, want = masked_problem(c)
    got = run_flash(p, c.out_f32)
    assert torch.isfinite(got).all()
    assert torch.count_nonzero(got[1]) == 0
    check(got[:1], want[:1], c.dt, masked_id(c))


@gpu
@pytest.mark.parametrize("c", BI_ALL_MASKED, ids=bi_id)
def test_all_masked_bi_xattn(c):
    """the same answer from every kernel a text length selects (L 20: generic, 100: specialised, 300: generic): out_v of the item
    without an attended token is zero, its out_l is still the unmasked text -> image softmax"""
    out_v, out_l = run_bi(c)
    want_v, want_l = bi_problem(c)[2]
    assert torch.isfinite(out_v).all() and torch.isfinite(out_l).all()
    assert torch.count_nonzero(out_v[1]) == 0
    check(out_v[:1], want_v[:1], c.dt, bi_id(c) + " out_v")
    check(out_l, want_l, c.dt, bi_id(c) + " out_l")
