"""Exact host emulation of the `fp8x` policy's arithmetic (hipie_gemm_f8x / hipie_to_f8x, include/hipie_mi355.h).

q8 of a 32-element k block (the block aligned to four HL8 groups): amax = max |v| over the block's fp16 values; e = the largest integer with
amax * 2^e <= 448 (amax = 0: e = 0), clamped to [-127, 127]; code = RNE float8_e4m3fn(v * 2^e); E8M0 scale byte = 127 - e, so the value
the matrix pipe sees is code * 2^(byte - 127).  v * 2^e is exact in fp32 for fp16 v and never exceeds 448, so torch's fp32 -> e4m3fn cast
(round to nearest even) is the device conversion.

The product the kernel forms (fp32 accumulation; here in fp64):
    acc = W_hi . X_hi  +  q8(W_lo) . q8(X_hi)  +  q8(W_hi) . q8(X_lo)
with (hi, lo) the HL8 split of each operand.  CPU and GPU tests use this module; the study behind the policy is tools/fp8_cross_terms.py.
"""
import torch

BLOCK = 32
E4M3_MAX = 448.0


def _hl8_parts(x_hl8):
    """(..., 2K) fp16 HL8 -> (hi, lo) as (..., K) fp16"""
    K2 = x_hl8.shape[-1]
    g = x_hl8.reshape(*x_hl8.shape[:-1], K2 // 16, 2, 8)
    return g[..., 0, :].reshape(*x_hl8.shape[:-1], K2 // 2), g[..., 1, :].reshape(*x_hl8.shape[:-1], K2 // 2)


def block_exponent(amax):
    """e of the q8 rule for a tensor of block maxima (float): the largest integer with amax * 2^e <= 448, 0 for amax = 0, clamped to +-127"""
    m, x = torch.frexp(amax.double())                          # amax = m * 2^x, m in [0.5, 1)
    e = torch.where(m <= 0.875, 9 - x, 8 - x)
    return torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-127, 127).to(torch.int32)


def quantise(v16):
    """(..., K) fp16 -> (codes (..., K) uint8 e4m3fn bits, scale bytes (..., K/32) uint8)"""
    K = v16.shape[-1]
    assert K % BLOCK == 0 and v16.dtype == torch.float16
    vb = v16.float().reshape(*v16.shape[:-1], K // BLOCK, BLOCK)
    e = block_exponent(vb.abs().amax(-1))
    q = (vb * torch.exp2(e.float()).unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).reshape(v16.shape), (127 - e).to(torch.uint8)


def dequantise(codes, scale):
    """(codes (..., K) uint8, scale bytes (..., K/32)) -> (..., K) float64 values"""
    K = codes.shape[-1]
    v = codes.view(torch.float8_e4m3fn).double().reshape(*codes.shape[:-1], K // BLOCK, BLOCK)
    return (v * torch.exp2(scale.double() - 127).unsqueeze(-1)).reshape(codes.shape)


def to_f8x(x_hl8):
    """host twin of hipie_to_f8x: HL8 rows (rows, 2K) -> (out (rows, 2K) uint8: per block [q8(hi) 32 | q8(lo) 32], scale (rows, K/32, 2) [hi, lo])"""
    hi, lo = _hl8_parts(x_hl8)
    qh, sh = quantise(hi)
    ql, sl = quantise(lo)
    R, K = hi.shape
    out = torch.stack([qh.reshape(R, K // BLOCK, BLOCK), ql.reshape(R, K // BLOCK, BLOCK)], dim=2).reshape(R, 2 * K)
    return out.contiguous(), torch.stack([sh, sl], dim=-1).contiguous()


# the e4m3 half of a weight slice in the lane order of hipie_gemm_f8x (include/hipie_mi355.h): (part, 8-group) per 8 bytes, part 0 = q8(hi),
# 1 = q8(lo) -- lane half h reads [q8(lo) g h, g h+2 | q8(hi) g h, g h+2]
E4M3_ORDER = ((1, 0), (1, 2), (0, 0), (0, 2), (1, 1), (1, 3), (0, 1), (0, 3))


def pack_from_hl8(w_hl8, q=None, sc=None):
    """the f8x weight format from an HL8 weight (N, 2K) and its to_f8x result (computed here when not given): (W (N, 4K) uint8: per
    32-element block hi fp16 [64 B] | e4m3 [64 B] in E4M3_ORDER,  scales (N, K/32, 2) uint8 [lo, hi])"""
    if q is None:
        q, sc = to_f8x(w_hl8)
    N, K2 = w_hl8.shape
    K = K2 // 2
    nb = K // BLOCK
    hi, _ = _hl8_parts(w_hl8)
    hib = hi.contiguous().view(torch.uint8).reshape(N, nb, 2 * BLOCK)
    qb = q.reshape(N, nb, 2, 4, 8)
    w = torch.cat([hib] + [qb[:, :, p, g] for p, g in E4M3_ORDER], dim=-1).reshape(N, 4 * K).contiguous()
    return w, sc[..., [1, 0]].contiguous()


def hl8_split(w):
    """fp32 (N, K) -> HL8 (N, 2K) fp16 (ops.hl8_pack without the device: hi = fp16(w), lo = fp16(w - hi), saturated at fp16's range)"""
    from . import ops
    return ops.hl8_pack(w)


def pack_weight(w):
    """fp32 weight (N, K) -> the f8x weight format (W (N, 4K) uint8, scales (N, K/32, 2) uint8), on the host"""
    return pack_from_hl8(hl8_split(w.float().cpu()))


def unpack_weight(w8, wsc):
    """f8x weight (N, 4K) uint8 + scales -> (W_hi fp64, q8(W_lo) fp64, q8(W_hi) fp64), each (N, K)"""
    N, K4 = w8.shape
    K = K4 // 4
    nb = K // BLOCK
    b = w8.reshape(N, nb, 4 * BLOCK)
    hi = b[:, :, :2 * BLOCK].contiguous().view(torch.float16).reshape(N, K).double()
    e8 = b[:, :, 2 * BLOCK:].reshape(N, nb, 8, 8)
    parts = torch.empty(N, nb, 2, 4, 8, dtype=torch.uint8, device=w8.device)
    for i, (p, g) in enumerate(E4M3_ORDER):
        parts[:, :, p, g] = e8[:, :, i]
    lo8 = dequantise(parts[:, :, 1].reshape(N, K), wsc[..., 0])
    hi8 = dequantise(parts[:, :, 0].reshape(N, K), wsc[..., 1])
    return hi, lo8, hi8


def emulate_acc(x_hl8, w8, wsc):
    """the accumulator of hipie_gemm_f8x in fp64, on the operands' device: X (M, 2K) HL8 against the f8x weight -> (M, N) float64"""
    xh, xl = _hl8_parts(x_hl8)
    qh, sh = quantise(xh)
    ql, sl = quantise(xl)
    wh, wl8, wh8 = unpack_weight(w8, wsc)
    return xh.double() @ wh.t() + dequantise(qh, sh) @ wl8.t() + dequantise(ql, sl) @ wh8.t()
