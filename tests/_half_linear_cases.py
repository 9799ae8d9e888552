"""Host restatement (torch, float64 / fp16) of what csrc/half_pack.hip and the half-precision training linears compute, shared by
tests/test_half_linears_cpu.py and tests/test_gpu_half_linears.py: the fp16 conversion with saturation, both operand layouts with the zero
pad columns, the exact product of the rounded operands, and an emulation of one linear's backward.  The scale rule, the data and the bound of
the column sums are those of tests/_grad_scale_cases.py (the pack kernel sums in hipie_grad_pack's order)."""
import torch

from _grad_scale_cases import BOUND, GAINS, INVARIANCE_EXPONENTS, column_sum_bound, linear_problem, scale_of  # noqa: F401  (shared with the tests)

# (M, N, K) of y = x (M, K) . W (N, K)^T: one chunk, sixteen chunks and two chunks of the weight gradient's contraction (64-row groups)
SHAPES = ((300, 128, 192), (1024, 64, 64), (333, 320, 256))
CHUNKS = (1, 16, 2)
PACK_SHAPES = ((40, 32), (300, 96), (257, 320), (1024, 64))
ROUNDED_BOUND = BOUND             # against half_product of the rounded operands: only fp32 accumulation separates the two
UNROUNDED_BOUND = 1e-3            # against float64 of the unrounded operands: the bound of the plain-fp16 case of tests/test_gpu_gemm.py

# rel_err of net.vit_backbone / net.encoder_layer under net.half_policy(HipBackend) against the same functions on the library's fp32
# linears (tests/test_gpu_half_linears.py, the module-level tests).  The bound cannot be derived: the WORST value over every output and
# every parameter gradient measured on the MI355X (docs/measurements.md, "Half-precision training linears"); the tests assert 2 x these.
# Measured: vit_backbone 1.175e-01 (d pos_embed; the three outputs 3.4e-4 / 2.8e-4 / 2.8e-4), encoder_layer 1.398e-01 (d linear1.weight;
# the output 2.1e-4).  Both worst values are set by single elements behind a kink, not by the rounding of the products: a 2^-11 change of
# u flips relu'(u) for the few elements of the FFN's hidden layer that sit at zero (a half MLP node with ReLU alone shows 5e-2 to 1e-1
# on dx / dW1 against 5e-4 with GELU), and the max pool behind res5 routes a cotangent to another element of a near-tie.
MODULE_WORST = {"vit_backbone": 1.175e-01, "encoder_layer": 1.398e-01}


def half(x, s=1.0):
    """fp16(s x): round to nearest even, values beyond +-65504 saturate (hp_half of csrc/half_pack.hip)"""
    return (x.float() * torch.tensor(s, dtype=torch.float32)).clamp(-65504.0, 65504.0).half()


def half_rows(x, s=1.0):
    """(rows, N) -> (rows, N) fp16 of s x: out_rows of hipie_half_pack"""
    return half(x, s)


def half_t(x, s=1.0, pad_to=64):
    """(rows, N) -> (N, rows_p) fp16 of (s x)^T, the pad columns zero: out_t of hipie_half_pack"""
    rows, N = x.shape
    rows_p = -(-rows // pad_to) * pad_to
    out = torch.zeros(N, rows_p, dtype=torch.float16)
    out[:, :rows] = half(x, s).t()
    return out


def half_product(a, b):
    """a (M, K) . b (N, K)^T of the fp16-ROUNDED operands, exact: float64 holds every fp16 x fp16 product (22 bits) and their sums over
    these K"""
    return half(a).double() @ half(b).double().t()


def chunks(M, N, K):
    """functions._weight_grad_chunks(M, N, K, 64), restated"""
    Mp = -(-M // 64) * 64
    tiles = -(-N // 256) * -(-K // 256)
    nk = 1
    while nk < 16 and tiles * nk < 256 and (Mp // 64) % (2 * nk) == 0:
        nk *= 2
    return nk


def emulated_errors(M, N, K, g, scaled):
    """(y error, dx error, dW error), max|err| / max|ref| against float64 of the UNROUNDED operands, of one half-precision linear with exact
    accumulation: dy enters as fp16(s dy) with s from the scale rule (scaled) or as fp16(dy) (not scaled)"""
    x, w, dy = linear_problem(M, N, K, g)
    ref = (x.double() @ w.double().t(), dy.double() @ w.double(), dy.double().t() @ x.double())
    s, inv = scale_of(dy) if scaled else (1.0, 1.0)
    dys = dy * torch.tensor(s, dtype=torch.float32)
    got = (half_product(x, w), half_product(dys, w.t()) * inv, half_product(dys.t(), x.t()) * inv)
    return tuple(float((a - r).abs().max() / r.abs().max()) for a, r in zip(got, ref))
