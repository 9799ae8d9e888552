"""Host restatement (torch, float64 / fp16) of what csrc/grad_pack.hip computes, shared by tests/test_grad_scale_cpu.py and
tests/test_gpu_grad_scale.py: the scale rule, hl_split, both HL8 layouts, and an emulation of the three-product split GEMM with EXACT
accumulation (float64 holds every fp16 x fp16 product and their sums over these K exactly enough: 22 + 22 bits of product, < 2^9 terms)."""
import struct

import torch

# the cases of the operator tests: dy = g * N(0, 1); (M, N, K) of y = x (M, K) . W (N, K)^T.  The second shape takes the split-K path.
GAINS = (1.0, 2.0 ** -12, 2.0 ** -20, 2.0 ** -30, 2.0 ** 15)
SHAPES = ((300, 96, 160), (1024, 64, 64), (333, 320, 256))
BOUND = 5e-6                      # rel_err bound of test_split_linear_function_forward_and_backward (tests/test_gpu_gemm.py) for these products
PACK_SHAPES = ((40, 32), (300, 96), (257, 320), (1024, 64))
INVARIANCE_EXPONENTS = (-30, -20, -12, 10)
TILE_ROWS = 128                   # kGpRows of csrc/grad_pack.hip: rows of one tile's column sum


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def from_bits(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def scale_rule(amax):
    """(s, 1 / s) for the largest magnitude amax (a python float holding an fp32 value): s = 2^e with amax * 2^e in [2^14, 2^15), e from
    the exponent field with integer arithmetic, clamped to +-126 (both floats normal fp32); amax == 0 or non-finite: (1, 1)"""
    if amax != amax:
        return 1.0, 1.0
    b = bits(abs(amax)) & 0x7FFFFFFF
    field = b >> 23
    if b == 0 or field == 255:
        return 1.0, 1.0
    E = field - 127 if field else (b.bit_length() - 1) - 149
    e = min(max(14 - E, -126), 126)
    return from_bits((127 + e) << 23), from_bits((127 - e) << 23)


def scale_of(dy):
    """scale_rule of a tensor (a NaN anywhere counts as non-finite: the kernel's integer maximum sees it)"""
    if not bool(torch.isfinite(dy).all()):
        return 1.0, 1.0
    return scale_rule(float(dy.abs().max()))


def hl_split(x, saturate=True):
    """hi = fp16(x), lo = fp16(x - hi) of fp32 x; saturate: values beyond the fp16 range are clamped to +-65504 first (hl_split of
    csrc/common.h); without it an overflowing hi is inf and its remainder NaN (the plain split the issue's table was made with)"""
    x = x.float()
    if saturate:
        x = x.clamp(-65504.0, 65504.0)
    h = x.half()
    return h, (x - h.float()).half()


def to_hl8(x, s=1.0):
    """(rows, N) fp32 -> (rows, 2N) fp16: per group of 8 columns the 8 hi then the 8 lo of fp32(x * s) (hipie_to_hl8)"""
    rows, N = x.shape
    h, l = hl_split(x.float() * torch.tensor(s, dtype=torch.float32))
    return torch.stack((h.reshape(rows, N // 8, 8), l.reshape(rows, N // 8, 8)), 2).reshape(rows, 2 * N)


def to_hl8_t(x, s=1.0, pad_to=32):
    """(rows, N) fp32 -> (N, 2 rows_p) fp16 HL8 of (s x)^T, the pad columns zero (hipie_to_hl8_t)"""
    rows, N = x.shape
    rows_p = -(-rows // pad_to) * pad_to
    xt = torch.zeros(N, rows_p, dtype=torch.float32)
    xt[:, :rows] = (x.float() * torch.tensor(s, dtype=torch.float32)).t()
    return to_hl8(xt)


def column_sum_bound(dy):
    """|db - float64 column sum| <= this, per column: db adds 32 rows in order, then 4 such runs, then the tiles in order -- at most
    31 + 3 + (tiles - 1) fp32 additions on the path of any term, each within 2^-24 of the running sum, which never exceeds sum_m |dy|"""
    depth = 31 + 3 + (-(-dy.shape[0] // TILE_ROWS) - 1)
    return depth * 2.0 ** -24 * dy.double().abs().sum(0) * 1.0001


def split_product(a, b, saturate=True):
    """a (M, K) . b (N, K)^T as the split GEMM forms it -- lo.hi + hi.lo + hi.hi of the fp16 pairs -- with exact accumulation (float64)"""
    ah, al = (t.double() for t in hl_split(a, saturate))
    bh, bl = (t.double() for t in hl_split(b, saturate))
    return al @ bh.t() + ah @ bl.t() + ah @ bh.t()


def linear_problem(M, N, K, g, seed=0):
    """x ~ N(0, 1), W ~ N(0, 1) K^-1/2, dy = g N(0, 1), all fp32"""
    gen = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(M, K, generator=gen)
    w = torch.randn(N, K, generator=gen) * K ** -0.5
    dy = torch.randn(M, N, generator=gen) * g
    return x, w, dy


def emulated_errors(g, scaled, M=300, N=96, K=160):
    """(dx error, dW error), max|err| / max|ref| against float64, of the emulated backward of one linear: raw (today's split of dy, plain
    rounding) or with dy scaled by scale_rule and the products multiplied back"""
    x, w, dy = linear_problem(M, N, K, g)
    ref_dx, ref_dw = dy.double() @ w.double(), dy.double().t() @ x.double()
    s, inv = scale_of(dy) if scaled else (1.0, 1.0)
    dys = dy * torch.tensor(s, dtype=torch.float32)
    dx = split_product(dys, w.t().contiguous(), saturate=scaled) * inv
    dw = split_product(dys.t().contiguous(), x.t().contiguous(), saturate=scaled) * inv
    err = lambda got, ref: float((got - ref).abs().max() / ref.abs().max())
    return err(dx, ref_dx), err(dw, ref_dw)


# the issue's table: g -> (dx raw, dW raw, dx scaled, dW scaled); nan = not a number
TABLE = {1.0: (2.3e-7, 7.6e-8, 2.3e-7, 7.4e-8), 2.0 ** -12: (6.9e-5, 6.6e-5, 2.3e-7, 7.4e-8), 2.0 ** -20: (1.6e-2, 1.7e-2, 2.3e-7, 7.4e-8),
         2.0 ** -30: (1.0, 1.0, 2.3e-7, 7.4e-8), 2.0 ** 15: (float("nan"), float("nan"), 2.3e-7, 7.4e-8)}
