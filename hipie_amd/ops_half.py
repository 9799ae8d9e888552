"""The op layer of the HALF-precision training linears (csrc/half_pack.hip, hipie_gemm_batched_f16; the opt-in policy
training/net.half_policy): one fp16 MFMA product per GEMM, fp32 master weights, fp32 accumulation and output.  The arithmetic contract is
stated in DESIGN.md section 9 and in the header.  The wrappers call the library through ops._call and check their operands with the
vocabulary of ops.py (ops._on_device / ops._layout); there is no host path."""
import torch

from . import ops
from .derived import derived
from .ops import _layout, _on_device, _ptr, _timed, _workspace


@_timed("half_pack")
def half_pack(x, scale=None, want_rows=True, want_t=True, want_bias=False, rows_p=None):
    """hipie_half_pack: ONE pass over x (rows, N), fp32 or fp16 device rows (N % 8 == 0; any row stride in 16-byte pieces), with the device
    block `scale` = {s, 1 / s} of ops.grad_scale (None: s = 1) ->
    (fp16 rows of s x, (rows, N) | None,  fp16 rows of (s x)^T, (N, rows_p) with zero pad columns | None,
     the column sums of the UNSCALED x, (N,) fp32, summed in a fixed order | None).  Round to nearest even, saturated at +-65504.
    rows_p (default: rows rounded up to 64) a multiple of 64.  Everything is refused before a launch."""
    who = "half_pack"
    _on_device(who, "x scale", x, scale)
    _layout(who, "x", x, (torch.float32, torch.float16), ndim=2, density=ops._ROWS, row_mult=4 if x.dtype is torch.float32 else 8, align16=True)
    _layout(who, "scale", scale, torch.float32, shape=(2,))
    rows, N = x.shape
    if rows == 0 or N == 0 or N % 8:
        raise RuntimeError("%s: x must be a non-empty (rows, N) tensor with N a multiple of 8, got %s" % (who, tuple(x.shape)))
    ldx = x.stride(0) if rows > 1 else N
    if ldx < N:
        raise RuntimeError("%s: x rows overlap, got strides %s" % (who, tuple(x.stride())))
    rows_p = -(-rows // 64) * 64 if rows_p is None else int(rows_p)
    if rows_p < rows or rows_p % 64:
        raise RuntimeError("%s: rows_p=%d must be a multiple of 64 and at least rows=%d" % (who, rows_p, rows))
    out_r = torch.empty(rows, N, dtype=torch.float16, device=x.device) if want_rows else None
    out_t = torch.empty(N, rows_p, dtype=torch.float16, device=x.device) if want_t else None
    db = ws = None
    if want_bias:
        db = torch.empty(N, dtype=torch.float32, device=x.device)
        ws = _workspace(None, ops._size("hipie_half_pack_ws_bytes", rows_p, N), x.device, who)
    ops._call("hipie_half_pack", x.data_ptr(), ldx, ops._DT[x.dtype], _ptr(scale), _ptr(out_r), N, _ptr(out_t), rows_p, _ptr(db), _ptr(ws), rows, N, rows_p)
    return out_r, out_t, db


@_timed("act_half")
def act_half(u, act):
    """hipie_act_half: fp16(act(u)) in one pass, u (..., N) dense fp32 device rows, N % 8 == 0, act = ops.ACT_GELU | ops.ACT_RELU -> fp16 of
    u's shape: the bits of ops.act_forward(u, act).half() without the fp32 activation in memory"""
    _on_device("act_half", "u", u)
    _layout("act_half", "u", u, torch.float32, align16=True)
    if act not in (ops.ACT_GELU, ops.ACT_RELU) or u.dim() < 1 or u.shape[-1] % 8:
        raise RuntimeError("act_half: act must be ACT_GELU or ACT_RELU and the last dimension a multiple of 8, got act=%s, u %s" % (act, tuple(u.shape)))
    a = torch.empty(u.shape, dtype=torch.float16, device=u.device)
    N = u.shape[-1]
    ops._call("hipie_act_half", u.data_ptr(), a.data_ptr(), u.numel() // N if N else 0, N, int(act))
    return a


@_timed("gemm_split_k_half")
def gemm_split_k_half(a16, w16, nk, alpha_dev=None, want_parts=False):
    """alpha_dev * a16 . w16^T for plain fp16 operands a16 (M, K), w16 (N, K) with the contraction cut into nk chunks (K / nk a multiple of
    64): one problem per chunk in ONE hipie_gemm_batched_f16 launch, the partial products added in chunk order and multiplied by the device
    scalar (None: 1) by hipie_splitk_finish -> (M, N) fp32.  One chunk: the product itself (ops.gemm_scaled), no partial products.
    want_parts: the (nk, M, N) partial products instead (each has the bits of ops.gemm(..., split=False) on its slices)."""
    who = "gemm_split_k_half"
    _on_device(who, "a16 w16 alpha_dev", a16, w16, alpha_dev)
    ops._one_f32(who, alpha_dev)
    _layout(who, "a16", a16, torch.float16, ndim=2, align16=True)
    _layout(who, "w16", w16, torch.float16, ndim=2, align16=True)
    M, K = a16.shape
    N = w16.shape[0]
    if w16.shape[1] != K or nk < 1 or nk > 64 or K % (64 * nk) or N % 8 or (M * N) % 4:
        raise RuntimeError("%s: fp16 operands (M, K) / (N, K), K a multiple of 64 * nk, nk <= 64, N a multiple of 8, got %s / %s, nk=%d"
                           % (who, tuple(a16.shape), tuple(w16.shape), nk))
    if nk == 1 and not want_parts:
        return ops.gemm_scaled(a16, w16, alpha_dev, split=False, out_fmt=ops.F32, tag="train_dw")
    Kc = K // nk
    part = torch.empty(nk, M, N, dtype=torch.float32, device=a16.device)
    ops._call("hipie_gemm_batched_f16", a16.data_ptr(), K, 0, Kc, w16.data_ptr(), K, 0, Kc, part.data_ptr(), N, 0, M * N, 1, nk, M, N, Kc, 1.0, None)
    if want_parts:
        return part
    out = torch.empty(M, N, dtype=torch.float32, device=a16.device)
    ops._call("hipie_splitk_finish", part.data_ptr(), nk, out.numel(), _ptr(alpha_dev), out.data_ptr())
    return out


def half_weight(owner, key, params, weight_fn):
    """fp16 copy of a weight: weight_fn() (N, K) -> (N, K) fp16, round to nearest even, saturated at +-65504 (the contract's W16; with
    weight_fn = lambda: w.t() the copy of W^T the input gradient reads).  Cached on ``owner`` under ``key`` and rebuilt when ``params``
    change (derived), exactly as ops.split_weight caches the HL8 copies."""
    def build():
        return weight_fn().detach().float().clamp(-65504.0, 65504.0).half().contiguous()
    return derived(owner, ("f16", key), params, build)
