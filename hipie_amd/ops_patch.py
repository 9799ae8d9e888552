"""The op layer of the training projections (csrc/patch_pack.hip; the opt-in group "projections" of training/net.py): the map-to-rows pack
that turns a convolution whose kernel equals its stride, or a transposed one, into linears over patch rows.  The contract is stated in the
header.  The wrappers call the library through ops._call / ops._size and check their operands with the vocabulary of ops.py
(ops._on_device / ops._layout); there is no host path."""
import torch

from . import ops
from .ops import _layout, _on_device, _ptr, _timed, _workspace


def _map_strides(x):
    """the element strides of a (B, C, H, W) map as the pack takes them: the stride of a dimension of size 1 is never used to step, so it
    is set to what a dense map of that layout would have (torch leaves it arbitrary)"""
    B, C, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if W == 1:
        sw = 1 if sc != 1 or C == 1 else C
    if H == 1:
        sh = W * sw
    if C == 1:
        sc = 1 if sw != 1 else H * sh
    if B == 1:
        sb = max(C * sc, H * sh)
    return sb, sc, sh, sw


@_timed("patch_pack")
def patch_pack(x, k, scale=None, want_f32=False, want_rows=True, want_t=True, want_sum=False, rows_p=None):
    """hipie_patch_pack: ONE pass over the fp32 device map x (B, C, H, W) -- NCHW-dense or channels-last, read in place through its strides
    -- with the patch size k (H % k == 0, W % k == 0) and the device block `scale` = {s, 1 / s} of ops.grad_scale (None: s = 1).  Patch row
    m = (b H/k + h) W/k + w, column n = c k^2 + i k + j: M = B (H/k) (W/k) rows of N = C k^2 columns (N % 8 == 0) ->
    (the fp32 rows (M, N) | None,  the HL8 rows of s x, (M, 2 N) fp16 | None,  the HL8 rows of (s x)^T, (N, 2 rows_p) fp16 with zero pad
     columns | None,  the per-channel sums of the UNSCALED x, (C,) fp32, summed in a fixed order | None).
    rows_p (default: M rounded up to 32) a multiple of 32.  Everything is refused before a launch."""
    who = "patch_pack"
    _on_device(who, "x scale", x, scale)
    _layout(who, "x", x, torch.float32, ndim=4, density=ops._ANY)
    _layout(who, "scale", scale, torch.float32, shape=(2,))
    k = int(k)
    B, C, H, W = x.shape
    if min(B, C, H, W) < 1 or k < 1 or H % k or W % k or (C * k * k) % 8:
        raise RuntimeError("%s: x must be a non-empty (B, C, H, W) map with k=%d dividing H and W and C k^2 a multiple of 8, got %s" % (who, k, tuple(x.shape)))
    sb, sc, sh, sw = _map_strides(x)
    if (sw != 1 and sc != 1) or min(sc, sh, sw) < 1 or sb < 0:
        raise RuntimeError("%s: x: the unit stride must be that of W (NCHW) or of C (channels-last), got strides %s" % (who, tuple(x.stride())))
    M, N = B * (H // k) * (W // k), C * k * k
    rows_p = -(-M // 32) * 32 if rows_p is None else int(rows_p)
    if rows_p < M or rows_p % 32:
        raise RuntimeError("%s: rows_p=%d must be a multiple of 32 and at least M=%d" % (who, rows_p, M))
    out_f = torch.empty(M, N, dtype=torch.float32, device=x.device) if want_f32 else None
    out_r = torch.empty(M, 2 * N, dtype=torch.float16, device=x.device) if want_rows else None
    out_t = torch.empty(N, 2 * rows_p, dtype=torch.float16, device=x.device) if want_t else None
    dsum = ws = None
    if want_sum:
        dsum = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _workspace(None, ops._size("hipie_patch_pack_ws_bytes", rows_p, N), x.device, who)
    ops._call("hipie_patch_pack", x.data_ptr(), B, C, H, W, sb, sc, sh, sw, k, _ptr(scale), _ptr(out_f), N, _ptr(out_r), 2 * N, _ptr(out_t),
              2 * rows_p, rows_p, _ptr(dsum), _ptr(ws), 0 if ws is None else ws.numel())
    return out_f, out_r, out_t, dsum


def patch_rows_view(x, k=1):
    """the (M, C) pixel rows of a k == 1 map (B, C, H, W) as a VIEW when the map is channels-last dense -- stride(1) == 1, one pixel stride
    >= C that is a multiple of 4 through all of (b, h, w), a 16-byte aligned base -- else None.  hipie_gemm, hipie_grad_scale and
    hipie_grad_pack take a row stride, so such an operand costs no launch of its own."""
    if k != 1 or x.dim() != 4 or x.dtype is not torch.float32 or x.numel() == 0:
        return None
    B, C, H, W = x.shape
    sb, sc, sh, sw = _map_strides(x)
    if sc != 1 or sw < C or sw % 4 or sh != W * sw or (B > 1 and sb != H * sh) or x.data_ptr() % 16:
        return None
    return x.as_strided((B * H * W, C), (sw, 1))
