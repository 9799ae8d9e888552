"""Operator layer: torch.Tensor in, torch.Tensor out, raw device pointers + current HIP stream across the C ABI.

Mirrors the reference's operator boundary: ``ms_deform_attn_forward`` has the signature and error
behaviour of the pybind module ``MultiScaleDeformableAttention`` (contiguity / device checks raise RuntimeError, CPU
tensors raise "Not implemented on the CPU", ops/src/ms_deform_attn.h:28-39).  All functions are inference-only.
"""
import ctypes

import torch

from . import _lib
from .derived import derived

# the HIPIE_* codes and flags of include/hipie_mi355.h, read from it (K_HL8_HI: hipie_flash_attn's keys are the hi halves of an HL8 buffer)
F32, F16, BF16, F64, HL8, OUT_F32, K_HL8_HI, ATTN_FAST = (
    _lib.CONSTANTS["HIPIE_" + n] for n in ("F32", "F16", "BF16", "F64", "HL8", "OUT_F32", "K_HL8_HI", "ATTN_FAST"))
_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}


class _Profile(object):
    """Optional live timing of the hand-written kernels with HIP events recorded on the launch stream (torch's current
    stream, the one every entry point is launched on).  Used by bench.py for the `roofline` object."""

    def __init__(self):
        self.tags, self.events = set(), {}
        self.shapes = False            # tools/stage_times.py: tag the generic GEMM launches by (M, N, K, formats)

    def enable(self, *tags):
        self.tags, self.events = set(tags), {}

    def disable(self):
        self.tags = set()

    def begin(self, tag):
        if tag not in self.tags and "all" not in self.tags:
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.events.setdefault(tag, []).append((a, b))
        return b

    def mean_ms(self, tag):
        ev = self.events.get(tag, [])
        if not ev:
            return None, 0
        torch.cuda.synchronize()
        ts = [a.elapsed_time(b) for a, b in ev]
        return sum(ts) / len(ts), len(ts)

    def summary(self):
        return {t: self.mean_ms(t) + (sum(a.elapsed_time(b) for a, b in self.events[t]),) for t in self.events}


PROFILE = _Profile()


import os as _os
import sys as _sys

_DEBUG_SYNC = _os.environ.get("HIPIE_DEBUG_SYNC") == "1"      # debugging aid: synchronise + log around every custom op


def _timed(tag):
    def deco(fn):
        def wrapper(*a, **k):
            if _DEBUG_SYNC:
                torch.cuda.synchronize()
                print("[hipie] > %s %s" % (fn.__name__, [tuple(t.shape) for t in a if torch.is_tensor(t)]), file=_sys.stderr, flush=True)
                out = fn(*a, **k)
                torch.cuda.synchronize()
                print("[hipie] < %s" % fn.__name__, file=_sys.stderr, flush=True)
                return out
            end = PROFILE.begin(tag(*a, **k) if callable(tag) else tag) if PROFILE.tags else None
            out = fn(*a, **k)
            if end is not None:
                end.record()
            return out
        wrapper.__doc__ = fn.__doc__
        wrapper.__name__ = fn.__name__
        wrapper.__wrapped__ = fn
        return wrapper
    return deco


def _stream():
    return torch.cuda.current_stream().cuda_stream


_BOUND = {}          # entry point -> its ctypes function, bound on the first call (the training forward makes thousands of calls per step)


def _call(name, *args):
    """the one checked call into the library: entry point `name` on the current stream (every entry point that returns a status takes the
    stream last); a non-zero status raises with the library's message and the symbol that was called"""
    fn = _BOUND.get(name)
    if fn is None:
        fn = _BOUND[name] = getattr(_lib.load(), name)
    rc = fn(*args, _stream())
    if rc:
        _lib.check(rc, name)


def _size(name, *args):
    """a size query of the library (*_ws_bytes, *_workspace, hipie_optim_chunk): it returns the number, takes no stream and has no status"""
    return int(getattr(_lib.load(), name)(*args))


def _code(dtype):
    """C-ABI element code of an output type: a torch dtype, or the string "hl8" (split fp16, HIPIE_HL8)."""
    return HL8 if dtype == "hl8" else _DT[dtype]


def _alloc(shape, dtype, device):
    """output buffer of logical ``shape`` in ``dtype``; "hl8": fp16 with the last dimension doubled."""
    if dtype == "hl8":
        return torch.empty(*shape[:-1], 2 * shape[-1], dtype=torch.float16, device=device)
    return torch.empty(shape, dtype=dtype, device=device)


# ---- the operand checks of every op below.  Each helper does one thing; only _dense_f32 may copy.  The rule: every tensor whose address
# goes to _call is refused by _on_device while it is a host tensor, before _call and before a _size query that depends on it.
def _on_device(op, names, *tensors):
    """refuses host tensors: `names` = the operands' names in one string, `tensors` in that order (None: an operand that is left out)"""
    for t in tensors:
        if t is not None and not t.is_cuda:
            i = [x is t for x in tensors].index(True)
            raise RuntimeError("Not implemented on the CPU (%s: %s must be a CUDA/HIP tensor)" % (op, names.split()[i]))


_DENSE, _ROWS, _ANY = 0, 1, 2          # _layout's density: contiguous | last dimension contiguous (rows may be strided) | no requirement


def _layout(op, name, t, dtype=None, shape=None, ndim=None, density=_DENSE, row_mult=1, align16=False):
    """refuses t unless it has that dtype (or one of a tuple), that shape / rank, that density (with _ROWS: a row stride that is a multiple
    of row_mult) and, with align16, a 16-byte aligned address.  Nothing is copied, the device is not looked at; returns t (None, an
    optional operand left out, passes)"""
    if t is None:
        return None
    if dtype is not None and t.dtype is not dtype and (type(dtype) is not tuple or t.dtype not in dtype):
        raise RuntimeError("%s: %s must be %s, got %s" % (op, name, " / ".join(map(str, dtype)) if type(dtype) is tuple else dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError("%s: %s must have %d dimensions, got %s" % (op, name, ndim, tuple(t.shape)))
    if shape is not None and t.shape != shape:          # torch.Size is a tuple: it compares with the tuple the caller wrote
        raise RuntimeError("%s: %s must be %s, got %s" % (op, name, tuple(shape), tuple(t.shape)))
    if density == _DENSE:
        if not t.is_contiguous():
            raise RuntimeError("%s: %s tensor has to be contiguous" % (op, name))
    elif density == _ROWS:
        if t.stride(-1) != 1:
            raise RuntimeError("%s: %s: the last dimension has to be dense (contiguous rows), got strides %s" % (op, name, tuple(t.stride())))
        if row_mult > 1 and t.shape[-2] > 1 and t.stride(-2) % row_mult:
            raise RuntimeError("%s: %s: the row stride must be a multiple of %d, got strides %s" % (op, name, row_mult, tuple(t.stride())))
    if align16 and t.data_ptr() % 16:
        raise RuntimeError("%s: %s must be 16-byte aligned" % (op, name))
    return t


def _dense_f32(op, name, t, align16=False):
    """t as a dense fp32 device tensor, with align16 on a 16-byte boundary: a strided view, or one at an odd storage offset, is copied"""
    if not t.is_cuda or t.dtype is not torch.float32:          # the refusals are the vocabulary's; the usual call pays for neither
        _on_device(op, name, t)
        _layout(op, name, t, torch.float32, density=_ANY)
    t = t.contiguous()
    return t.clone() if align16 and t.data_ptr() % 16 else t


def _ptr(t):
    """the address of an optional operand, or NULL"""
    return t.data_ptr() if t is not None else None


def _workspace(ws, need, device, what):
    """the caller's byte workspace when it is given (checked), else one that lives for the call"""
    if ws is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise RuntimeError("%s: workspace of %d contiguous uint8 elements needed, got %s %s" % (what, need, ws.dtype, tuple(ws.shape)))
    return ws


def _f16_planes(shape, device):
    """the (hi, lo) fp16 planes of a split operand, uninitialised (the sizes go to torch.empty one by one: a tuple is parsed twice as slowly)"""
    return torch.empty(*shape, dtype=torch.float16, device=device), torch.empty(*shape, dtype=torch.float16, device=device)


def _check_im2col_step(B, im2col_step):
    """the reference op processes the batch in chunks of min(B, im2col_step) images and asserts that the chunk divides the batch
    (ms_deform_attn_cuda.cu:50-52, :112-114); this kernel has no chunking (one launch over B), but a call the reference would refuse
    is refused here too, with its message."""
    step = min(int(B), int(im2col_step))
    if step <= 0 or B % step != 0:
        raise RuntimeError("batch(%d) must divide im2col_step(%d)" % (B, step))


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step=64):
    """MSDA.ms_deform_attn_forward (ops/src/vision.cpp:13-16): value (B,S,M,D), shapes (L,2) i64, level_start (L,) i64,
    sampling_loc (B,Lq,M,L,P,2), attn_weight (B,Lq,M,L,P) -> (B,Lq,M*D).  value may be f32/f16/bf16 with f32 loc/attn, or all f64."""
    B, S, M, D = value.shape
    _check_im2col_step(B, im2col_step)
    _, Lq, _, L, P, _ = sampling_loc.shape
    f64 = value.dtype == torch.float64              # the reference op's double instantiation (ops/test.py checks it)
    if value.dtype not in _DT and not f64:
        raise RuntimeError("ms_deform_attn_forward: unsupported dtype %s" % value.dtype)
    aux = torch.float64 if f64 else torch.float32
    who = "ms_deform_attn_forward"
    _on_device(who, "value spatial_shapes level_start_index sampling_loc attn_weight", value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    out = torch.empty(B, Lq, M * D, dtype=value.dtype, device=value.device)
    _call("hipie_msda_forward", _layout(who, "value", value).data_ptr(), _layout(who, "spatial_shapes", spatial_shapes, torch.int64).data_ptr(),
          _layout(who, "level_start_index", level_start_index, torch.int64).data_ptr(), _layout(who, "sampling_loc", sampling_loc, aux).data_ptr(),
          _layout(who, "attn_weight", attn_weight, aux).data_ptr(), out.data_ptr(), B, S, M, D, L, Lq, P, F64 if f64 else _DT[value.dtype])
    return out


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step=64):
    """MSDA.ms_deform_attn_backward (ops/src/vision.cpp:13-16; ms_deform_attn_cuda.cu:83-153): the gradients of the op above with
    respect to value, sampling_loc and attn_weight, all f32 or all f64 -> (grad_value, grad_sampling_loc, grad_attn_weight).
    Runs hipie_msda_backward_ws: the gather form for fp32 and D = 32, the atomic kernel of hipie_msda_backward otherwise."""
    B, S, M, D = value.shape
    _check_im2col_step(B, im2col_step)
    _, Lq, _, L, P, _ = sampling_loc.shape
    dt = value.dtype
    if dt not in (torch.float32, torch.float64):
        raise RuntimeError("ms_deform_attn_backward: float32 / float64 only (got %s)" % dt)
    who = "ms_deform_attn_backward"
    _on_device(who, "value spatial_shapes level_start_index sampling_loc attn_weight grad_output", value, spatial_shapes, level_start_index, sampling_loc,
               attn_weight, grad_output)
    gv = torch.empty_like(value, memory_format=torch.contiguous_format)
    gl = torch.empty(sampling_loc.shape, dtype=dt, device=value.device)
    ga = torch.empty(attn_weight.shape, dtype=dt, device=value.device)
    need = _size("hipie_msda_backward_workspace", B, S, M, L, Lq, P) if dt == torch.float32 and D == 32 and B * Lq > 0 else 0
    ws = _workspace(None, max(need, 16), value.device, who)      # the gather form's bins and corner records (fp32, D = 32)
    _call("hipie_msda_backward_ws", _layout(who, "value", value, dt).data_ptr(), _layout(who, "spatial_shapes", spatial_shapes, torch.int64).data_ptr(),
          _layout(who, "level_start_index", level_start_index, torch.int64).data_ptr(), _layout(who, "sampling_loc", sampling_loc, dt).data_ptr(),
          _layout(who, "attn_weight", attn_weight, dt).data_ptr(), _layout(who, "grad_output", grad_output.contiguous(), dt).data_ptr(),
          gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), B, S, M, D, L, Lq, P, F64 if dt == torch.float64 else F32, ws.data_ptr(), need)
    return gv, gl, ga


@_timed("msda")
def msda_fused(value, spatial_shapes, level_start_index, ref, offsets, logits):
    """value (B,S,M,D); ref (B,Lq,L,2|4) f32; offsets (B,Lq,M,L,P,2); logits (B,Lq,M,L*P) (f32/f16/bf16, same dtype; they
    may be column slices of ONE projection output: only the last dim block must be contiguous) -> (B,Lq,M*D)."""
    B, S, M, D = value.shape
    vrow = M * D
    if not value.is_contiguous():             # a column block of a wider (B, S, n * M * D) projection output: sampled in place
        vrow = value.stride(1)
        if value.stride(3) != 1 or value.stride(2) != D or value.stride(0) != S * vrow or vrow % 8 or vrow < M * D:
            raise RuntimeError("msda_fused: value must be dense or a column block of a dense (B, S, k*M*D) tensor")
    _, Lq, _, L, P, _ = offsets.shape
    if offsets.dtype != logits.dtype or offsets.dtype not in _DT:
        raise RuntimeError("msda_fused: offsets/logits must share a dtype in f32/f16/bf16")
    if B == 0 or Lq == 0:
        return torch.empty(B, Lq, M * D, dtype=value.dtype, device=value.device)
    off_stride, lg_stride = offsets.stride(1), logits.stride(1)
    if offsets.stride(0) != Lq * off_stride or logits.stride(0) != Lq * lg_stride or \
            offsets[0, 0].stride() != (L * P * 2, P * 2, 2, 1) or logits[0, 0].stride() != (L * P, 1):
        raise RuntimeError("msda_fused: offsets/logits rows must be dense (M,L,P,2)/(M,L*P) blocks")
    who = "msda_fused"
    _on_device(who, "offsets logits value spatial_shapes level_start_index ref", offsets, logits, value, spatial_shapes, level_start_index, ref)
    out = torch.empty(B, Lq, M * D, dtype=value.dtype, device=value.device)
    if value.dtype not in _DT:
        raise RuntimeError("msda_fused: bad value dtype")
    _layout(who, "spatial_shapes", spatial_shapes, torch.int64)
    _layout(who, "level_start_index", level_start_index, torch.int64)
    _layout(who, "ref", ref, torch.float32)
    # dense values go in with row stride 0 (= M * D inside the library): the % 8 requirement applies to strided column blocks only
    _call("hipie_msda_fused_forward_strided", value.data_ptr(), 0 if value.is_contiguous() else vrow,
          spatial_shapes.data_ptr(), level_start_index.data_ptr(), ref.data_ptr(), offsets.data_ptr(), logits.data_ptr(), out.data_ptr(),
          B, S, M, D, L, Lq, P, ref.shape[-1], _DT[value.dtype], _DT[offsets.dtype], off_stride, lg_stride)
    return out


def _raw_rows(t, name, B, Lq, inner):
    """row stride of offsets / logits or of their gradients: dense (M,L,P,2) / (M,L*P) blocks at a common distance, fp32"""
    _layout("msda_raw_backward", name, t, torch.float32, density=_ANY)
    if tuple(t.shape[:2]) != (B, Lq) or tuple(t[0, 0].stride()) != inner or t.stride(0) != Lq * t.stride(1):
        raise RuntimeError("msda_raw_backward: %s rows must be dense blocks of one (B, Lq, k) tensor" % name)
    return t.stride(1)


@_timed("msda_bwd")
def msda_raw_backward(value, spatial_shapes, level_start_index, ref, offsets, logits, grad_output, want_grad_ref=True,
                      grad_offsets=None, grad_logits=None):
    """backward of msda_fused for fp32 and D = 32 (hipie_msda_raw_backward): value (B,S,M,D) dense; ref (B,Lq,L,2|4); offsets (B,Lq,M,L,P,2)
    and logits (B,Lq,M,L*P), which may be column blocks of one projection output; grad_output (B,Lq,M*D) ->
    (grad_value, grad_offsets, grad_logits, grad_ref | None).  grad_offsets / grad_logits may be given: column blocks of one (B, Lq, k)
    buffer, written in place.  The workspace (bins, corner records, per-head partials of grad_ref) lives for this call."""
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = offsets.shape
    dev = value.device
    gv = torch.empty(B, S, M, D, dtype=torch.float32, device=dev)
    if grad_offsets is None:
        grad_offsets = torch.empty(B, Lq, M, L, P, 2, dtype=torch.float32, device=dev)
    if grad_logits is None:
        grad_logits = torch.empty(B, Lq, M, L * P, dtype=torch.float32, device=dev)
    gref = torch.empty(B, Lq, L, ref.shape[-1], dtype=torch.float32, device=dev) if want_grad_ref else None
    if B == 0:
        return gv, grad_offsets, grad_logits, gref
    if Lq == 0:
        return gv.zero_(), grad_offsets, grad_logits, gref
    who = "msda_raw_backward"
    _on_device(who, "offsets logits grad_offsets grad_logits value spatial_shapes level_start_index ref grad_output",
               offsets, logits, grad_offsets, grad_logits, value, spatial_shapes, level_start_index, ref, grad_output)
    off_in, lg_in = (L * P * 2, P * 2, 2, 1), (L * P, 1)
    strides = (_raw_rows(offsets, "offsets", B, Lq, off_in), _raw_rows(logits, "logits", B, Lq, lg_in),
               _raw_rows(grad_offsets, "grad_offsets", B, Lq, off_in), _raw_rows(grad_logits, "grad_logits", B, Lq, lg_in))
    rd = int(ref.shape[-1])
    need = _size("hipie_msda_raw_backward_ws_bytes", B, S, M, L, Lq, P, rd, int(bool(want_grad_ref)))
    ws = _workspace(None, max(need, 16), dev, who)
    go = grad_output.contiguous()
    _call("hipie_msda_raw_backward", _layout(who, "value", value, torch.float32).data_ptr(),
          _layout(who, "spatial_shapes", spatial_shapes, torch.int64).data_ptr(), _layout(who, "level_start_index", level_start_index, torch.int64).data_ptr(),
          _layout(who, "ref", ref, torch.float32).data_ptr(), offsets.data_ptr(), logits.data_ptr(),
          _layout(who, "grad_output", go, torch.float32).data_ptr(), gv.data_ptr(), grad_offsets.data_ptr(), grad_logits.data_ptr(),
          _ptr(gref), B, S, M, D, L, Lq, P, rd, *strides, ws.data_ptr(), need)
    return gv, grad_offsets, grad_logits, gref


@_timed("flash_attn")
def flash_attn(q, k, v, scale, bias_h=None, bias_w=None, key_mask=None, clamp=0.0, out_f32=False, k_hl8=False):
    """q (B,Nq,H,hd), k,v (B,Nk,H,hd) 16-bit (may be strided views with hd contiguous) -> (B,Nq,H*hd) in the operand dtype, or
    fp32 with out_f32.  bias_h (B*H,kh,Nq) / bias_w (B*H,Nq,kw) f32 decomposed rel-pos bias; key_mask (B,Nk) uint8/bool.
    A query with no attended key (a batch item whose key_mask is all zero) gives zeros.
    k_hl8: k is a contiguous (B, Nk, 2*H*hd) fp16 HL8 buffer whose hi halves are the keys (read in place, HIPIE_K_HL8_HI)."""
    B, Nq, H, hd = q.shape
    Nk = k.shape[1]
    if k_hl8:
        if k.dtype != torch.float16 or q.dtype != torch.float16 or not k.is_contiguous() or tuple(k.shape) != (B, Nk, 2 * H * hd):
            raise RuntimeError("flash_attn: k_hl8 expects a contiguous (B, Nk, 2*H*hd) fp16 HL8 buffer and fp16 q / v")
        ks = (Nk * 2 * H * hd, 2 * H * hd, 2 * hd)
    _on_device("flash_attn", "q k v bias_h bias_w key_mask", q, k, v, bias_h, bias_w if bias_h is not None else None, key_mask)
    for t, n in ((q, "q"), (v, "v")) + (() if k_hl8 else ((k, "k"),)):
        if t.dtype != q.dtype:
            raise RuntimeError("flash_attn: %s must have q's dtype %s, got %s" % (n, q.dtype, t.dtype))
        _layout("flash_attn", n, t, (torch.float16, torch.bfloat16), density=_ROWS)
    out = torch.empty(B, Nq, H * hd, dtype=torch.float32 if out_f32 else q.dtype, device=q.device)
    kh = kw = 0
    if bias_h is not None:
        kh, kw = bias_h.shape[-2], bias_w.shape[-1]
        _layout("flash_attn", "bias_h", bias_h, torch.float32)
        _layout("flash_attn", "bias_w", bias_w, torch.float32)
    if key_mask is not None:
        key_mask = key_mask.to(torch.uint8).contiguous()
    _call("hipie_flash_attn", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, Nq, Nk, hd,
          q.stride(0), q.stride(1), q.stride(2), *(ks if k_hl8 else (k.stride(0), k.stride(1), k.stride(2))),
          v.stride(0), v.stride(1), v.stride(2), Nq * H * hd, H * hd, hd, _ptr(bias_h), _ptr(bias_w) if bias_h is not None else None, kh, kw,
          _ptr(key_mask), float(scale), float(clamp),
          _DT[q.dtype] | (OUT_F32 if out_f32 else 0) | (K_HL8_HI if k_hl8 else 0))
    return out


@_timed("bi_i2t_split")
def bi_i2t_split(q_hl8, k, vl, text_mask, heads, clamp=50000.0, n_keys=None):
    """image -> text direction of the vision-language fusion at fp32-class accuracy (fuse_helper.py:77-121):
        out_v[b, i, h] = softmax_j( clamp(q[b,i,h] . k[b,j,h]) over the text tokens kept by text_mask ) . vl[b, j, h]
    q_hl8 (B, Nv, 2*E) HL8 (E = heads * hd; the scaled v_proj output straight from the GEMM epilogue), k, vl (B, L, E) fp32,
    text_mask (B, L) -> (B, Nv, E) fp32.  Texts of up to 256 tokens: TWO launches -- the batched logits GEMM with the masked row softmax in
    its epilogue (P as HL8; S never exists) and P_h.V_h as the second batched GEMM; longer texts: S = Q_h.K_h^T, hipie_softmax_hl8, P_h.V_h; the text-side operands (L x E) are padded to a
    multiple of 32 tokens and split on the way.  n_keys (host int, optional): every attended token sits in the first n_keys columns --
    the masked keys behind them have probability exactly 0 (-9e15 before the softmax) and are left out, so a PAD_MAX prompt (4096
    columns, 194 of them attended) costs what its real tokens cost and nothing of size Nv x L is allocated."""
    B, Nv, E2 = q_hl8.shape
    E = E2 // 2
    hd = E // heads
    if n_keys is not None and 0 < n_keys < k.shape[1]:
        k, vl, text_mask = k[:, :n_keys], vl[:, :n_keys], text_mask[:, :n_keys]
    L = k.shape[1]
    Lp = (L + 31) // 32 * 32
    if q_hl8.dtype != torch.float16 or not q_hl8.is_contiguous() or k.dtype != torch.float32 or vl.dtype != torch.float32 or hd % 32:
        raise RuntimeError("bi_i2t_split: q HL8 (fp16) contiguous, k / vl fp32, head_dim a multiple of 32")
    _on_device("bi_i2t_split", "q_hl8 k vl text_mask", q_hl8, k, vl, text_mask)
    dev = q_hl8.device
    kp = torch.zeros(B, Lp, E, dtype=torch.float32, device=dev)
    kp[:, :L] = k
    k_hl8 = to_hl8(kp)                                                        # (B, Lp, 2E): head h = columns [2 hd h, 2 hd (h + 1))
    vt = torch.zeros(B, heads, hd, Lp, dtype=torch.float32, device=dev)
    vt[..., :L] = vl.reshape(B, L, heads, hd).permute(0, 2, 3, 1)
    vt_hl8 = to_hl8(vt)                                                       # (B, heads, hd, 2 Lp): V_h^T, K = tokens
    P = torch.empty(B, heads, Nv, 2 * Lp, dtype=torch.float16, device=dev)
    mk = text_mask.to(torch.uint8).contiguous()
    if Lp <= 256:
        # a text of up to 256 tokens is ONE column tile: the masked softmax runs in the logits GEMM's epilogue, S never exists
        _call("hipie_gemm_batched_softmax", q_hl8.data_ptr(), 2 * E, Nv * 2 * E, 2 * hd, k_hl8.data_ptr(), 2 * E, Lp * 2 * E, 2 * hd,
              P.data_ptr(), 2 * Lp, heads * Nv * 2 * Lp, Nv * 2 * Lp, B, heads, Nv, Lp, hd, mk.data_ptr(), L, float(clamp), 1.0)
    else:
        S = torch.empty(B, heads, Nv, Lp, dtype=torch.float32, device=dev)
        _call("hipie_gemm_batched", q_hl8.data_ptr(), 2 * E, Nv * 2 * E, 2 * hd, k_hl8.data_ptr(), 2 * E, Lp * 2 * E, 2 * hd,
              S.data_ptr(), Lp, heads * Nv * Lp, Nv * Lp, B, heads, Nv, Lp, hd, F32, 1.0)
        _call("hipie_softmax_hl8", S.data_ptr(), Lp, P.data_ptr(), 2 * Lp, B * heads * Nv, L, Lp, mk.data_ptr(), heads * Nv, float(clamp))
    out = torch.empty(B, Nv, E, dtype=torch.float32, device=dev)
    _call("hipie_gemm_batched", P.data_ptr(), 2 * Lp, heads * Nv * 2 * Lp, Nv * 2 * Lp, vt_hl8.data_ptr(), 2 * Lp, heads * hd * 2 * Lp, hd * 2 * Lp,
          out.data_ptr(), E, Nv * E, hd, B, heads, Nv, hd, Lp, F32, 1.0)
    return out


def bi_i2t_folded_ok(v, L_text, n_keys=None):
    """the folded vision-language attention applies: at most 256 attended text columns (one column tile of the softmax epilogue), a visual
    width the split GEMM takes (and the fp16 attention kernel as a head dim: 256), inference"""
    L = L_text if not n_keys else min(int(n_keys), L_text)
    return v.is_cuda and v.dtype == torch.float32 and v.shape[-1] == 256 and 0 < L <= 256 and not torch.is_grad_enabled()


@_timed("bi_i2t_folded")
def bi_i2t_folded(v_hl8, M, cb, vl, text_mask, heads, wo, bo, resid=None, clamp=50000.0):
    """image -> text direction of the vision-language fusion (fuse_helper.py:62-139) at fp32-class accuracy WITHOUT the two visual-side
    projections of width E = heads * hd:
        logits[b,h][i,j] = (wq_h x_i + bq_h) . k[b,j,h] = x_i . M[b,h,j] + cb[b,h,j]       M = k_h wq_h (L x C), cb = k_h . bq_h
        out[b,i]         = wo concat_h(P_h[i] vl_h) + bo (+ resid) = sum_h P_h[i] . U[b,h] + bo      U = vl_h wo_h^T (L x C_out)
    v_hl8 (B, Nv, 2C) HL8 of the (layer-normed) visual stream x; M (B, H, L, C), cb (B, H, L) fp32 (the caller's small text-side products,
    already cut to the attended columns); vl (B, L, E) fp32 text values; wo (C_out, E), bo (C_out) the output projection; resid (B, Nv, C_out)
    fp32 or None -> (B, Nv, C_out) fp32.  TWO launches over the visual tokens (hipie_gemm_batched_softmax_bias: P as HL8, the logits never
    exist; hipie_gemm_batched_resid: K = heads * Lp).  L <= 256.  The reassociation moves the rounding of the logits at the 1e-7 level."""
    B, Nv, C2 = v_hl8.shape
    C = C2 // 2
    L = M.shape[2]
    E = vl.shape[-1]
    hd = E // heads
    Lp = (L + 31) // 32 * 32
    Co = wo.shape[0]
    if v_hl8.dtype != torch.float16 or not v_hl8.is_contiguous() or M.dtype != torch.float32 or vl.dtype != torch.float32 or Lp > 256 or Co % 8 \
            or tuple(M.shape) != (B, heads, L, C) or tuple(cb.shape) != (B, heads, L) or vl.shape[1] != L:
        raise RuntimeError("bi_i2t_folded: x HL8 (fp16) contiguous, M (B, H, L, C) / cb (B, H, L) / vl (B, L, E) fp32, at most 256 text columns")
    _on_device("bi_i2t_folded", "v_hl8 M cb vl text_mask wo bo resid", v_hl8, M, cb, vl, text_mask, wo, bo, resid)
    dev = v_hl8.device
    Mp = torch.zeros(B, heads, Lp, C, dtype=torch.float32, device=dev)
    Mp[:, :, :L] = M
    cbp = torch.zeros(B, heads, Lp, dtype=torch.float32, device=dev)
    cbp[:, :, :L] = cb
    m_hl8 = to_hl8(Mp)                                                                 # (B, H, Lp, 2C)
    U = torch.zeros(B, Co, heads, Lp, dtype=torch.float32, device=dev)
    U[..., :L] = torch.einsum("nhd,blhd->bnhl", wo.float().view(Co, heads, hd), vl.reshape(B, L, heads, hd))
    u_hl8 = to_hl8(U.view(B, Co, heads * Lp))                                          # (B, C_out, 2 H Lp): K = (head, text token)
    P = torch.empty(B, Nv, heads * 2 * Lp, dtype=torch.float16, device=dev)
    mk = text_mask.to(torch.uint8).contiguous()
    _call("hipie_gemm_batched_softmax_bias", v_hl8.data_ptr(), 2 * C, Nv * 2 * C, 0, m_hl8.data_ptr(), 2 * C, heads * Lp * 2 * C, Lp * 2 * C,
          P.data_ptr(), heads * 2 * Lp, Nv * heads * 2 * Lp, 2 * Lp, B, heads, Nv, Lp, C, mk.data_ptr(), L, cbp.data_ptr(), float(clamp), 1.0)
    out = torch.empty(B, Nv, Co, dtype=torch.float32, device=dev)
    r = None if resid is None else _layout("bi_i2t_folded", "resid", resid.reshape(B, Nv, Co), torch.float32)
    bo32 = None if bo is None else bo.float().contiguous()
    KK = heads * Lp
    _call("hipie_gemm_batched_resid", P.data_ptr(), 2 * KK, Nv * 2 * KK, 0, u_hl8.data_ptr(), 2 * KK, Co * 2 * KK, 0, _ptr(bo32), _ptr(r),
          Co, Nv * Co, 0, out.data_ptr(), Co, Nv * Co, 0, B, 1, Nv, Co, KK, 1.0)
    return out


def _small_attn_args(who, q, k, v, mask, rows=False):
    """(B, Nq, H, hd, Nk) of the small fp32 attentions: q (B, Nq, H, hd), k and v (B, Nk, H, hd) fp32 device views with hd contiguous and
    heads hd apart; mask (B, Nk), with rows (B, Nq, Nk), of any type that converts to uint8.  The kernels index k, v and the mask by q's
    B, H, hd and k's Nk, so operands that disagree about them are refused here"""
    _on_device(who, "q k v mask", q, k, v, mask)
    B, Nq, H, hd = _layout(who, "q", q, ndim=4, density=_ANY).shape
    Nk = _layout(who, "k", k, ndim=4, density=_ANY).shape[1]
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _layout(who, n, t, torch.float32, (B, Nq if t is q else Nk, H, hd), density=_ROWS)
        if H > 1 and t.stride(2) != hd:
            raise RuntimeError("%s: %s must be fp32 (B, N, H, hd) with hd contiguous and heads hd apart" % (who, n))
    _layout(who, "query_mask" if rows else "key_mask", mask, shape=(B, Nq, Nk) if rows else (B, Nk), density=_ANY)
    return B, Nq, H, hd, Nk


def _small_attn(fn_name, q, k, v, scale, key_mask):
    B, Nq, H, hd, Nk = _small_attn_args(fn_name, q, k, v, key_mask)
    out = torch.empty(B, Nq, H * hd, dtype=torch.float32, device=q.device)
    if key_mask is not None:
        key_mask = key_mask.to(torch.uint8).contiguous()
    _call(fn_name, q.data_ptr(), k.data_ptr(), v.data_ptr(), _ptr(key_mask), out.data_ptr(), B, H, Nq, Nk, hd, q.stride(0), q.stride(1),
          k.stride(0), k.stride(1), v.stride(0), v.stride(1), float(scale))
    return out


@_timed("attn_f32")
def attn_f32(q, k, v, scale, key_mask=None):
    """hipie_attn_f32: exact fp32 softmax attention.  q (B,Nq,H,hd), k, v (B,Nk,H,hd) fp32 views with hd contiguous and heads hd apart
    (column blocks of one projection output are fine); hd 32 | 64; key_mask (B,Nk) bool / uint8, non-zero = attend -> (B, Nq, H*hd) fp32.
    A batch item with no attended key gives zeros."""
    return _small_attn("hipie_attn_f32", q, k, v, scale, key_mask)


@_timed("attn_rows")
def attn_f32_rows(q, k, v, scale, query_mask, split=False):
    """hipie_attn_f32_rows (exact fp32 FMA) / hipie_attn_split_rows (split=True: matrix pipe, fp32-class under the conditions of attn_split):
    attention with a mask per query row -- query_mask (B, Nq, Nk) bool / uint8, non-zero = may attend; a row that may attend no key gives
    zeros (masked_fill(-inf).softmax gives NaN there)"""
    B, Nq, H, hd, Nk = _small_attn_args("attn_f32_rows", q, k, v, query_mask, rows=True)
    qm = query_mask.to(torch.uint8).contiguous()
    out = torch.empty(B, Nq, H * hd, dtype=torch.float32, device=q.device)
    _call("hipie_attn_split_rows" if split else "hipie_attn_f32_rows", q.data_ptr(), k.data_ptr(), v.data_ptr(), qm.data_ptr(), out.data_ptr(),
          B, H, Nq, Nk, hd, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), float(scale))
    return out


@_timed("attn_split")
def attn_split(q, k, v, scale, key_mask=None):
    """hipie_attn_split: the same attention on the matrix pipe at fp32-class accuracy (operands split into fp16 pairs in the kernel, three
    products per logit, probabilities as an fp16 pair): what the split policy runs for BERT and the decoders' query self-attention.
    fp32-class = attn_f32's bound, 1e-5 of the largest |output| of a (batch, head, 32-query block), under two conditions of the format
    (csrc/attn_split.hip, tests/test_gpu_small_attn.py): |v| of a few 1e-3 or more (v ~ N(0, 1) x 2^-8 is the last scale that holds; the
    lo halves of V are fp16 and go subnormal below it), and no row whose mass sits on one key of small V over a long tail of 2^-12 .. 2^-24
    (the lo half of P has a floor of 2^-25 of the row's largest probability: the error there was measured at 5e-7 of the largest attended |v|,
    8e-5 of the small output).  attn_f32 has neither limit."""
    return _small_attn("hipie_attn_split", q, k, v, scale, key_mask)


def attn_f32_ok(hd):
    return hd in (32, 64)


def _query_attn_args(who, qk, v, blocked, heads, out=None, d_out=None, lse=None):
    """(B, N, mask pointer) of the training query self-attention: qk (B, N, 2 heads 32), v (B, N, heads 32) fp32 device rows (column blocks of
    wider buffers are fine; the backward's out and d_out too), blocked None | (N, N) bool / uint8 dense; host tensors (lse's too) and other
    layouts / types are refused"""
    _on_device(who, "qk v blocked out d_out lse", qk, v, blocked, out, d_out, lse)
    B, N = qk.shape[0], qk.shape[1]
    C = heads * 32
    _layout(who, "qk", qk, torch.float32, (B, N, 2 * C), None, _ROWS)
    _layout(who, "v", v, torch.float32, (B, N, C), None, _ROWS)
    _layout(who, "out", out, torch.float32, (B, N, C), None, _ROWS)
    _layout(who, "d_out", d_out, torch.float32, (B, N, C), None, _ROWS)
    _layout(who, "blocked", blocked, (torch.bool, torch.uint8), (N, N))
    return B, N, _ptr(blocked)


@_timed("query_attn_train")
def query_attn_train_forward(qk, v, blocked, heads, scale):
    """hipie_attn_f32_train_forward: the decoders' query self-attention in exact fp32 for the training step.  qk (B, N, 2 heads 32) rows of the
    q | k in-projection, v (B, N, heads 32) rows, blocked None | (N, N) bool (True = may NOT attend, torch's attn_mask; its own storage is
    passed) -> (out (B, N, heads 32), lse (B, heads, N) in log2 units: what query_attn_train_backward takes)."""
    B, N, mp = _query_attn_args("query_attn_train_forward", qk, v, blocked, heads)
    out = torch.empty(B, N, heads * 32, dtype=torch.float32, device=qk.device)
    lse = torch.empty(B, heads, N, dtype=torch.float32, device=qk.device)
    _call("hipie_attn_f32_train_forward", qk.data_ptr(), v.data_ptr(), mp, out.data_ptr(), lse.data_ptr(), B, int(heads), N, 32,
          qk.stride(0), qk.stride(1), v.stride(0), v.stride(1), 0, float(scale))
    return out, lse


@_timed("query_attn_bwd")
def query_attn_train_backward(qk, v, blocked, out, lse, d_out, heads, scale, want_qk=True, want_v=True):
    """backward of query_attn_train_forward (hipie_attn_f32_train_backward): out, lse = the forward's, d_out (B, N, heads 32) rows ->
    (d_qk (B, N, 2 heads 32) | None, d_v (B, N, heads 32) | None); the probabilities are recomputed from lse, the sums run in a fixed
    order (bit-reproducible).  Without want_qk the dQ pass and the dK half are not launched, without want_v the dV half, without both
    nothing.  Nothing is cached: the workspace lives for the call."""
    who = "query_attn_train_backward"
    B, N, mp = _query_attn_args(who, qk, v, blocked, heads, out, d_out, lse)
    _layout(who, "out", out)
    _layout(who, "lse", lse, torch.float32, (B, heads, N))
    d_qk = torch.empty(B, N, 2 * heads * 32, dtype=torch.float32, device=qk.device) if want_qk else None
    d_v = torch.empty(B, N, heads * 32, dtype=torch.float32, device=qk.device) if want_v else None
    ws_bytes = _size("hipie_attn_f32_train_backward_ws_bytes", B, int(heads), N)
    ws = _workspace(None, ws_bytes, qk.device, who)
    _call("hipie_attn_f32_train_backward", qk.data_ptr(), v.data_ptr(), mp, out.data_ptr(), lse.data_ptr(),
          d_out.data_ptr(), _ptr(d_qk), _ptr(d_v), ws.data_ptr(), ws_bytes,
          B, int(heads), N, 32, qk.stride(0), qk.stride(1), v.stride(0), v.stride(1), 0, d_out.stride(0), d_out.stride(1), float(scale))
    return d_qk, d_v


def _bi_attn_args(who, q, k, vv, vl, att, heads, vis=(), txt=()):
    """(B, Nv, L) of the training fusion attention: q, vv (B, Nv, heads 256) and k, vl (B, L, heads 256) fp32 device rows (column blocks of
    wider buffers are fine), att (B, L) dense bool / uint8; `vis` / `txt`: further (name, tensor) rows of either side.  Host tensors and
    other layouts / types are refused"""
    B, Nv, L, E = q.shape[0], q.shape[1], k.shape[1], heads * 256
    rows = [("q", q, Nv), ("vv", vv, Nv), ("k", k, L), ("vl", vl, L)] + [(n, t, Nv) for n, t in vis] + [(n, t, L) for n, t in txt]
    _on_device(who, " ".join([n for n, _, _ in rows] + ["att"]), *[t for _, t, _ in rows], att)
    for n, t, r in rows:
        _layout(who, n, t, torch.float32, (B, r, E), None, _ROWS)
    _layout(who, "att", att, (torch.bool, torch.uint8), (B, L))
    return B, Nv, L


@_timed("bi_attn_train")
def bi_attn_train_forward(q, k, vv, vl, att, heads, dropout=0.0, seed=0):
    """hipie_bi_attn_train_forward: the core of the vision-language fusion attention in exact fp32 for the training step, both directions.
    q (UNSCALED v_proj rows), vv (B, Nv, heads 256), k, vl (B, L, heads 256), att (B, L) bool (True = attended), dropout in [0, 1) with the
    64-bit `seed` of the library's stateless keep function -> (out_v (B, Nv, E), out_l (B, L, E), lse_v (B, heads, Nv), lse_l (B, heads, L)
    in log2 units, stat_v (B, heads, Nv, 2), stat_l (B, heads, L, 2): what bi_attn_train_backward takes).  The workspace lives for the call."""
    B, Nv, L = _bi_attn_args("bi_attn_train_forward", q, k, vv, vl, att, heads)
    dev, E = q.device, heads * 256
    out_v = torch.empty(B, Nv, E, dtype=torch.float32, device=dev)
    out_l = torch.empty(B, L, E, dtype=torch.float32, device=dev)
    lse_v = torch.empty(B, heads, Nv, dtype=torch.float32, device=dev)
    lse_l = torch.empty(B, heads, L, dtype=torch.float32, device=dev)
    stat_v = torch.empty(B, heads, Nv, 2, dtype=torch.float32, device=dev)
    stat_l = torch.empty(B, heads, L, 2, dtype=torch.float32, device=dev)
    ws_bytes = _size("hipie_bi_attn_train_forward_ws_bytes", B, int(heads), Nv, L)
    ws = _workspace(None, ws_bytes, dev, "bi_attn_train_forward")
    _call("hipie_bi_attn_train_forward", q.data_ptr(), k.data_ptr(), vv.data_ptr(), vl.data_ptr(), att.data_ptr(), out_v.data_ptr(),
          out_l.data_ptr(), lse_v.data_ptr(), lse_l.data_ptr(), stat_v.data_ptr(), stat_l.data_ptr(), ws.data_ptr(), ws_bytes, B, int(heads), Nv, L,
          256, q.stride(0), q.stride(1), k.stride(0), k.stride(1), vv.stride(0), vv.stride(1), vl.stride(0), vl.stride(1), float(dropout), int(seed))
    return out_v, out_l, lse_v, lse_l, stat_v, stat_l


@_timed("bi_attn_bwd")
def bi_attn_train_backward(q, k, vv, vl, att, out_v, out_l, stat_v, stat_l, d_out_v, d_out_l, heads, dropout=0.0, seed=0, want=(True, True, True, True)):
    """backward of bi_attn_train_forward (hipie_bi_attn_train_backward): out_*, stat_* = the forward's, d_out_v (B, Nv, E) and d_out_l (B, L, E)
    rows, the forward's dropout and seed -> (d_q, d_k, d_vv, d_vl), None where `want` (in that order) is False: the work that serves only
    that gradient is not launched, and nothing at all without any.  Fixed order of every sum (bit-reproducible)."""
    B, Nv, L = _bi_attn_args("bi_attn_train_backward", q, k, vv, vl, att, heads, (("out_v", out_v), ("d_out_v", d_out_v)), (("out_l", out_l), ("d_out_l", d_out_l)))
    who = "bi_attn_train_backward"
    _on_device(who, "stat_v stat_l", stat_v, stat_l)
    _layout(who, "out_v", out_v)
    _layout(who, "out_l", out_l)
    _layout(who, "stat_v", stat_v, torch.float32, (B, heads, Nv, 2))
    _layout(who, "stat_l", stat_l, torch.float32, (B, heads, L, 2))
    dev, E = q.device, heads * 256
    grads = [torch.empty(B, n, E, dtype=torch.float32, device=dev) if w else None for w, n in zip(want, (Nv, L, Nv, L))]
    ws_bytes = _size("hipie_bi_attn_train_backward_ws_bytes", B, int(heads), Nv, L)
    ws = _workspace(None, ws_bytes, dev, who)
    _call("hipie_bi_attn_train_backward", q.data_ptr(), k.data_ptr(), vv.data_ptr(), vl.data_ptr(), att.data_ptr(), out_v.data_ptr(),
          out_l.data_ptr(), stat_v.data_ptr(), stat_l.data_ptr(), d_out_v.data_ptr(),
          d_out_l.data_ptr(), *[_ptr(g) for g in grads], ws.data_ptr(), ws_bytes, B, int(heads), Nv, L, 256,
          q.stride(0), q.stride(1), k.stride(0), k.stride(1), vv.stride(0), vv.stride(1), vl.stride(0), vl.stride(1),
          d_out_v.stride(0), d_out_v.stride(1), d_out_l.stride(0), d_out_l.stride(1), float(dropout), int(seed))
    return tuple(grads)


def _vit_operands(who, qkv, a, b, dtype, heads, parts=3, tables=("tab_h", "tab_w")):
    """(B, N, head dim) of the ViT attention family: qkv (B, N, parts * heads * hd) of any dtype and the two tables `a`, `b` (named by
    `tables`) of `dtype`, dense device tensors"""
    _on_device(who, "qkv %s %s" % tables, qkv, a, b)
    _layout(who, "qkv", qkv)
    _layout(who, tables[0], a, dtype)
    _layout(who, tables[1], b, dtype)
    B, N, C = qkv.shape
    return B, N, C // (parts * heads)


@_timed(lambda qkv, rel_h, rel_w, grid_hw, heads, scale: "vit_attn_global" if grid_hw[0] * grid_hw[1] > 256 else "vit_attn_window")
def vit_attn(qkv, rel_h, rel_w, grid_hw, heads, scale):
    """qkv (B, gh*gw, 3*heads*hd) 16-bit packed as (3, heads, hd); rel_h (B*heads, gh, N) f32 (key-row major),
    rel_w (B*heads, N, gw) f32 -> (B, N, heads*hd)."""
    gh, gw = grid_hw
    B, N, hd = _vit_operands("vit_attn", qkv, rel_h, rel_w, torch.float32, heads, 3, ("rel_h", "rel_w"))
    out = torch.empty(B, N, heads * hd, dtype=qkv.dtype, device=qkv.device)
    _call("hipie_vit_attn", qkv.data_ptr(), rel_h.data_ptr(), rel_w.data_ptr(), out.data_ptr(), B, gh, gw, heads, hd, float(scale), _DT[qkv.dtype])
    return out


def vit_attn_fused_ok(grid_hw, hd):
    """the geometry hipie_vit_attn_fused covers: a 64-wide token grid (1024-pixel images), <= 64 rows, head_dim 64 / 80."""
    return grid_hw[1] == 64 and 1 <= grid_hw[0] <= 64 and hd in (64, 80)


@_timed("vit_attn_global")
def vit_attn_fused(qkv, tab_h, tab_w, grid_hw, heads, scale):
    """global ViT attention with the decomposed rel-pos bias computed in the kernel prologue from the tables:
    qkv (B, gh*gw, 3*heads*hd) 16-bit, tab_h (2*gh-1, hd), tab_w (2*gw-1, hd) same dtype -> (B, N, heads*hd)."""
    gh, gw = grid_hw
    B, N, hd = _vit_operands("vit_attn_fused", qkv, tab_h, tab_w, qkv.dtype, heads)
    out = torch.empty(B, N, heads * hd, dtype=qkv.dtype, device=qkv.device)
    _call("hipie_vit_attn_fused", qkv.data_ptr(), tab_h.data_ptr(), tab_w.data_ptr(), out.data_ptr(), B, gh, gw, heads, hd, float(scale), _DT[qkv.dtype])
    return out


LOG2E = 1.4426950408889634


def vit_attn_rel_ok(grid_hw, hd):
    """the geometry hipie_vit_attn_rel covers: head_dim 64 / 80, token grids up to 96 wide (84 rows when wider than 64)."""
    gh, gw = grid_hw
    return hd in (64, 80) and 1 <= gw <= 96 and 1 <= gh <= (160 if gw <= 64 else 84)


@_timed(lambda qkv, tab_h, tab_w, grid_hw, heads, fast=False: "vit_attn_global" if grid_hw[0] * grid_hw[1] > 256 else "vit_attn_window")
def vit_attn_rel(qkv, tab_h, tab_w, grid_hw, heads, fast=False):
    """ViT attention (global or windowed) with the decomposed rel-pos bias computed in the kernel.  Operand contract of
    hipie_vit_attn_rel: qkv (B, gh*gw, 3*heads*hd) 16-bit whose q rows are PRE-SCALED by scale*log2(e); tab_h (2*gh-1, hd),
    tab_w (2*gw-1, hd) = the (re-interpolated) rel-pos tables DIVIDED by scale, same dtype -> (B, N, heads*hd)."""
    gh, gw = grid_hw
    B, N, hd = _vit_operands("vit_attn_rel", qkv, tab_h, tab_w, qkv.dtype, heads)
    out = torch.empty(B, N, heads * hd, dtype=qkv.dtype, device=qkv.device)
    _call("hipie_vit_attn_rel", qkv.data_ptr(), tab_h.data_ptr(), tab_w.data_ptr(), out.data_ptr(), B, gh, gw, heads, hd, _DT[qkv.dtype], ATTN_FAST if fast else 0)
    return out


class _Workspace(object):
    """scratch memory of a kernel family, one buffer per (device, stream): concurrent streams never share a buffer.  A buffer that turns
    out too small is replaced by one of at least twice the size and the old one is KEPT ALIVE (a captured hipGraph may still hold its
    address; geometric growth bounds what is retained by the final size).  Single assumption left: launches on one stream are ordered."""

    def __init__(self):
        self.bufs, self.retired = {}, []

    def get(self, nbytes, device):
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        b = self.bufs.get(key)
        if b is None or b.numel() < nbytes:
            if b is not None:
                self.retired.append(b)
            b = self.bufs[key] = torch.empty(max(int(nbytes), 2 * (b.numel() if b is not None else 0)), dtype=torch.uint8, device=device)
        return b


_XA_WS = _Workspace()


@_timed("bi_xattn")
def bi_xattn(q, k, vv, vl, text_mask, clamp=50000.0, out_f32=False):
    """q, vv (B,Nv,H,hd); k, vl (B,L,H,hd) 16-bit contiguous; text_mask (B,L) -> out_v (B,Nv,H*hd), out_l (B,L,H*hd) (operand dtype,
    or fp32 with out_f32: the generic flash kernel then runs both directions).  A query with no attended key gives zeros: the out_v
    rows of a batch item whose text_mask is all zero are zero at every L (whichever kernel the length selects); out_l has no mask."""
    B, Nv, H, hd = q.shape
    L = k.shape[1]
    _on_device("bi_xattn", "q k vv vl text_mask", q, k, vv, vl, text_mask)
    for n, t in (("q", q), ("k", k), ("vv", vv), ("vl", vl)):
        _layout("bi_xattn", n, t)
    text_mask = text_mask.to(torch.uint8).contiguous()
    odt = torch.float32 if out_f32 else q.dtype
    out_v = torch.empty(B, Nv, H * hd, dtype=odt, device=q.device)
    out_l = torch.empty(B, L, H * hd, dtype=odt, device=q.device)
    need = 0 if out_f32 else _size("hipie_bi_xattn_workspace", B, H, Nv, L, hd)          # split partials of the text -> image direction (0: none)
    ws = _XA_WS.get(need, q.device) if need > 0 else None
    _call("hipie_bi_xattn_ws", q.data_ptr(), k.data_ptr(), vv.data_ptr(), vl.data_ptr(), text_mask.data_ptr(),
          out_v.data_ptr(), out_l.data_ptr(), _ptr(ws), need, B, H, Nv, L, hd,
          float(clamp), _DT[q.dtype] | (OUT_F32 if out_f32 else 0))
    return out_v, out_l


_ME_WS = _Workspace()


@_timed("mask_einsum")
def mask_einsum(mask_embed, mask_features, precision=1, out_dtype=torch.float32, row_bias=None, workspace=True):
    """einsum("bqc,bchw->bqhw"): mask_embed (B,Q,C) f32, mask_features (B,C,H,W) f32 -> (B,Q,H,W) out_dtype.
    precision 0 = exact fp32 MFMA, 1 = bf16x3 split (default; ~2^-16), 2 = plain bf16.  Precisions 1 | 2 run hipie_mask_einsum_ws (the
    embedding split once into a cached scratch buffer and staged by LDS-DMA) and take row_bias (B,Q) f32, added to every pixel of
    its query row; workspace=False: the workspace-free entry point hipie_mask_einsum (every workgroup splits the embedding)."""
    B, Q, C = mask_embed.shape
    _, _, Hh, Ww = mask_features.shape
    _on_device("mask_einsum", "mask_embed mask_features row_bias", mask_embed, mask_features, row_bias)
    out = torch.empty(B, Q, Hh, Ww, dtype=out_dtype, device=mask_embed.device)
    e = _layout("mask_einsum", "mask_embed", mask_embed, torch.float32).data_ptr()
    f = _layout("mask_einsum", "mask_features", mask_features, torch.float32).data_ptr()
    if int(precision) == 0 or not workspace:
        if row_bias is not None:
            raise RuntimeError("mask_einsum: row_bias needs precision 1 | 2 and the workspace form")
        _call("hipie_mask_einsum", e, f, out.data_ptr(), B, Q, C, Hh * Ww, int(precision), _DT[out_dtype])
    else:
        rbt = None
        if row_bias is not None:
            rbt = row_bias.float().contiguous()
            if tuple(rbt.shape) != (B, Q):
                raise ValueError("mask_einsum: row_bias must be (B, Q) = (%d, %d), got %s" % (B, Q, tuple(rbt.shape)))
        need = _size("hipie_mask_einsum_workspace", B, Q, C)
        ws = _ME_WS.get(need, mask_embed.device)
        _call("hipie_mask_einsum_ws", e, f, _ptr(rbt), out.data_ptr(), ws.data_ptr(), need, B, Q, C, Hh * Ww, int(precision), _DT[out_dtype])
    return out


def _pad_last(x, n):
    if x.shape[-1] == n:
        return x.contiguous()
    out = torch.zeros(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    out[..., :x.shape[-1]] = x
    return out


@_timed("mask_einsum_bwd")
def mask_einsum_backward(mask_embed, mask_features, grad_out):
    """gradients of einsum("bqc,bchw->bqhw") (row f-4): mask_embed (B,Q,C), mask_features (B,C,H,W), grad_out (B,Q,H,W) fp32 ->
    (grad_embed (B,Q,C), grad_features (B,C,H,W)) fp32, both at fp32-class accuracy on hipie_gemm_batched (split operands):
      grad_embed[b]    = G[b] (Q x HW) . F[b]^T (HW x C)   -- K = HW split into up to 32 chunks (one problem each: Q x C is 2-5 tiles
                         per image, far fewer than the CUs), the partial products summed afterwards;
      grad_features[b] = E[b]^T (C x Q) . G[b] (Q x HW)    -- as A . W^T with A = E^T and W = G^T (both K = Q contiguous, Q padded to 32).
    The row-bias gradient of the forward's `row_bias` is grad_out.sum((2, 3)) (the caller's)."""
    B, Q, C = mask_embed.shape
    _, _, Hh, Ww = mask_features.shape
    HW = Hh * Ww
    if tuple(grad_out.shape) != (B, Q, Hh, Ww) or tuple(mask_features.shape[:2]) != (B, C):
        raise RuntimeError("mask_einsum_backward: mask_embed (B,Q,C), mask_features (B,C,H,W), grad_out (B,Q,H,W) device tensors")
    if C % 8:
        raise RuntimeError("mask_einsum_backward: C must be a multiple of 8")
    _on_device("mask_einsum_backward", "mask_embed mask_features grad_out", mask_embed, mask_features, grad_out)
    dev = grad_out.device
    G = grad_out.float().reshape(B, Q, HW)
    F_ = mask_features.float().reshape(B, C, HW)
    # ---- grad_embed: K = HW in nk chunks ----
    HWp = (HW + 31) // 32 * 32
    nk = max(n for n in range(1, 33) if (HWp // 32) % n == 0)
    Kc = HWp // nk
    gh, fh = to_hl8(_pad_last(G, HWp)), to_hl8(_pad_last(F_, HWp))              # (B, Q | C, 2 HWp)
    part = torch.empty(B, nk, Q, C, dtype=torch.float32, device=dev)
    _call("hipie_gemm_batched", gh.data_ptr(), 2 * HWp, Q * 2 * HWp, 2 * Kc, fh.data_ptr(), 2 * HWp, C * 2 * HWp, 2 * Kc,
          part.data_ptr(), C, nk * Q * C, Q * C, B, nk, Q, C, Kc, F32, 1.0)
    grad_e = part.sum(1) if nk > 1 else part[:, 0]
    # ---- grad_features: K = Q ----
    Qp = (Q + 31) // 32 * 32
    N8 = (HW + 7) // 8 * 8
    eT = to_hl8(_pad_last(mask_embed.float().transpose(1, 2), Qp))              # (B, C, 2 Qp)
    gT = torch.zeros(B, N8, Qp, dtype=torch.float32, device=dev) if (N8 != HW or Qp != Q) else torch.empty(B, N8, Qp, dtype=torch.float32, device=dev)
    gT[:, :HW, :Q] = G.transpose(1, 2)
    gTh = to_hl8(gT)                                                             # (B, N8, 2 Qp)
    gf = torch.empty(B, C, N8, dtype=torch.float32, device=dev)
    _call("hipie_gemm_batched", eT.data_ptr(), 2 * Qp, C * 2 * Qp, 0, gTh.data_ptr(), 2 * Qp, N8 * 2 * Qp, 0, gf.data_ptr(), N8, C * N8, 0,
          B, 1, C, N8, Qp, F32, 1.0)
    if N8 != HW:
        gf = gf[..., :HW].contiguous()
    return grad_e, gf.view(B, C, Hh, Ww)


@_timed("mask_einsum")
def mask_einsum16(mask_embed, mask_features, split=True, out_dtype=None, row_bias=None):
    """einsum("bqc,bchw->bqhw") on 16-bit features: mask_embed (B,Q,C) f32 (split here into 16-bit hi + lo parts: two MFMAs per
    product; split=False: hi only), mask_features (B,C,H,W) f16 | bf16 contiguous -> (B,Q,H,W) out_dtype (default: the feature
    dtype); row_bias (B,Q) is added to every pixel of its query row.  Q <= 320."""
    B, Q, C = mask_embed.shape
    _, _, Hh, Ww = mask_features.shape
    dt = mask_features.dtype
    out_dtype = out_dtype or dt
    _on_device("mask_einsum16", "mask_embed mask_features row_bias", mask_embed, mask_features, row_bias)
    _layout("mask_einsum16", "mask_features", mask_features)
    hi = mask_embed.to(dt).contiguous()
    lo = (mask_embed.float() - hi.float()).to(dt).contiguous() if split else None
    out = torch.empty(B, Q, Hh, Ww, dtype=out_dtype, device=mask_embed.device)
    rb = None if row_bias is None else row_bias.float().contiguous()
    _call("hipie_mask_einsum16", hi.data_ptr(), _ptr(lo), mask_features.data_ptr(), _ptr(rb), out.data_ptr(), B, Q, C, Hh * Ww, _DT[dt], _DT[out_dtype])
    return out


def _dynamic_mask_operands(who, mask_feats, ref_points, params, grad_out):
    _on_device(who, "mask_feats ref_points params grad_out", mask_feats, ref_points, params, grad_out)
    for n, t in (("mask_feats", mask_feats), ("ref_points", ref_points), ("params", params)) + ((("grad_out", grad_out),) if grad_out is not None else ()):
        _layout(who, n, t, torch.float32)


@_timed("dynamic_mask")
def dynamic_mask(mask_feats, ref_points, params, num_queries, stride=8, up=2, out_dtype=torch.float32, mlp_dtype=None):
    """mask_feats (B,8,H,W) f32; ref_points (B*Q,2) f32 pixels; params (B*Q,169) f32 -> (B*Q, up*H, up*W).
    mlp_dtype fp16 / bf16: the three layers on the matrix pipe with operands of that type (hipie_dynamic_mask16; up = 2,
    W % 4 == 0, stride % 4 == 0); "split": the same kernel on fp16 PAIRS (weights and activations hi + lo, three products each: fp32-class,
    the split policy); None / fp32: the fp32 VALU kernel."""
    B, C, H, W = mask_feats.shape
    if C != 8 or params.shape[-1] != 169:
        raise RuntimeError("dynamic_mask: expects 8 feature channels and 169 parameters per instance")
    n = B * num_queries
    _dynamic_mask_operands("dynamic_mask", mask_feats, ref_points, params, None)
    out = torch.empty(n, up * H, up * W, dtype=out_dtype, device=mask_feats.device)
    split = mlp_dtype == "split" and out_dtype in (torch.float32, torch.float16)
    if (split or mlp_dtype in (torch.float16, torch.bfloat16)) and up == 2 and W % 4 == 0 and stride % 4 == 0 and stride * max(H, W) <= 8192:
        _call("hipie_dynamic_mask16", mask_feats.data_ptr(), ref_points.data_ptr(), params.data_ptr(), out.data_ptr(), B, num_queries, H, W,
              int(stride), HL8 if split else _DT[mlp_dtype], _DT[out_dtype])
        return out
    _call("hipie_dynamic_mask", mask_feats.data_ptr(), ref_points.data_ptr(), params.data_ptr(), out.data_ptr(), B, num_queries, H, W,
          int(stride), int(up), _DT[out_dtype])
    return out


@_timed("dynamic_mask_bwd")
def dynamic_mask_backward(mask_feats, ref_points, params, grad_out, num_queries, stride=8, up=2):
    """gradients of dynamic_mask (row f-4; hipie_dynamic_mask_backward): mask_feats (B,8,H,W), ref_points (B*Q,2), params (B*Q,169),
    grad_out (B*Q, up*H, up*W) fp32 -> (grad_feats (B,8,H,W), grad_refs (B*Q,2), grad_params (B*Q,169)) fp32."""
    B, C, H, W = mask_feats.shape
    n = B * num_queries
    if C != 8 or params.shape[-1] != 169 or params.numel() != n * 169 or ref_points.numel() != n * 2:
        raise RuntimeError("dynamic_mask_backward: expects 8 feature channels, (B*Q, 169) parameters and (B*Q, 2) reference points")
    if tuple(grad_out.shape[-2:]) != (up * H, up * W) or grad_out.numel() != n * up * up * H * W:
        raise RuntimeError("dynamic_mask_backward: grad_out must be (B*Q, up*H, up*W), got %s" % (tuple(grad_out.shape),))
    _dynamic_mask_operands("dynamic_mask_backward", mask_feats, ref_points, params, grad_out)
    dev = mask_feats.device
    gf = torch.empty(B, 8, H, W, dtype=torch.float32, device=dev)
    gr = torch.empty(n, 2, dtype=torch.float32, device=dev)
    gp = torch.empty(n, 169, dtype=torch.float32, device=dev)
    _call("hipie_dynamic_mask_backward", mask_feats.data_ptr(), ref_points.data_ptr(), params.data_ptr(), grad_out.data_ptr(),
          gf.data_ptr(), gr.data_ptr(), gp.data_ptr(), B, num_queries, H, W, int(stride), int(up))
    return gf, gr, gp


@_timed("vit_relpos")
def vit_relpos(qkv, tab_h, tab_w, grid_hw, heads):
    """qkv (B, N, 3*heads*hd) 16-bit; tab_h (2gh-1, hd), tab_w (2gw-1, hd) same dtype -> rel_h (B*heads, gh, N), rel_w
    (B*heads, N, gw) f32, the bias tables of hipie_vit_attn."""
    gh, gw = grid_hw
    B, N, hd = _vit_operands("vit_relpos", qkv, tab_h, tab_w, qkv.dtype, heads)
    rel_h = torch.empty(B * heads, gh, N, dtype=torch.float32, device=qkv.device)
    rel_w = torch.empty(B * heads, N, gw, dtype=torch.float32, device=qkv.device)
    _call("hipie_vit_relpos", qkv.data_ptr(), tab_h.data_ptr(), tab_w.data_ptr(), rel_h.data_ptr(), rel_w.data_ptr(), B, gh, gw, heads, hd, _DT[qkv.dtype])
    return rel_h, rel_w


@_timed("add_layernorm")
def add_layernorm(x, delta, weight, bias, eps, norm_dtype, want_res=True, delta_row=None, out_src=None):
    """s = x + delta (delta may be None); returns (s in x.dtype or None, LayerNorm(s) in norm_dtype).  x (..., C).
    Row maps (int32, optional): ``out_src`` (out_rows,) = x row feeding each output row (-1: zeros) -- the normalised output
    then has out_rows rows; ``delta_row`` (rows of x,) = row of ``delta`` that belongs to x row r."""
    C = x.shape[-1]
    rows = x.numel() // C
    who = "add_layernorm"
    _on_device(who, "x delta weight bias delta_row out_src", x, delta, weight, bias, delta_row, out_src)
    res = torch.empty_like(x) if (want_res and delta is not None) else None
    if out_src is None:
        out = _alloc(tuple(x.shape), norm_dtype, x.device)
        out_rows = rows
    else:
        out_rows = int(out_src.shape[0])
        out = _alloc((out_rows, C), norm_dtype, x.device)
    args = (_layout(who, "x", x).data_ptr(), None if delta is None else _layout(who, "delta", delta).data_ptr(),
            _layout(who, "weight", weight, torch.float32).data_ptr(), _layout(who, "bias", bias, torch.float32).data_ptr(),
            _ptr(res), out.data_ptr(), out_rows, C, float(eps),
            _DT[x.dtype], _DT[x.dtype if delta is None else delta.dtype], _code(norm_dtype))
    if delta_row is None and out_src is None:
        _call("hipie_add_layernorm", *args)
    else:
        _call("hipie_add_layernorm_rows", *args, None if delta_row is None else _layout(who, "delta_row", delta_row, torch.int32).data_ptr(),
              None if out_src is None else _layout(who, "out_src", out_src, torch.int32).data_ptr())
    return (x if delta is None else res), out


@_timed("layernorm_bwd")
def layernorm_backward(s, gy, weight, eps, gres=None, want_param_grads=True):
    """backward of add_layernorm for the training step (hipie_layernorm_backward, fp32): s (..., C) = the tensor that was normalised,
    gy = gradient of the LayerNorm output, gres = gradient arriving at s from the residual stream (or None) ->
    (dx = LayerNorm input gradient + gres, dgamma, dbeta); the parameter sums are skipped (None, None) without want_param_grads.
    mean / rstd are recomputed from s; dgamma / dbeta are summed in a fixed order (bit-reproducible)."""
    who = "layernorm_backward"
    _on_device(who, "s gy weight gres", s, gy, weight, gres)
    C = s.shape[-1]
    rows = s.numel() // C if C else 0
    if gy.shape != s.shape or (gres is not None and gres.shape != s.shape) or weight.numel() != C:
        raise RuntimeError("layernorm_backward: gy / gres must have the shape of s %s and weight its last dimension" % (tuple(s.shape),))
    s, gy, weight = _dense_f32(who, "s", s, True), _dense_f32(who, "gy", gy, True), _dense_f32(who, "weight", weight, True)
    gres = None if gres is None else _dense_f32(who, "gres", gres, True)
    dx = torch.empty_like(s)
    dgamma = dbeta = ws = None
    ws_bytes = 0
    if want_param_grads:
        dgamma, dbeta = torch.empty_like(weight), torch.empty_like(weight)
        ws_bytes = _size("hipie_layernorm_backward_ws_bytes", rows, C)
        ws = _workspace(None, ws_bytes, s.device, who)
    _call("hipie_layernorm_backward", s.data_ptr(), gy.data_ptr(), _ptr(gres), weight.data_ptr(), dx.data_ptr(), _ptr(dgamma), _ptr(dbeta),
          _ptr(ws), ws_bytes, rows, C, float(eps))
    return dx, dgamma, dbeta


def _act_rows16(who, name, t):
    """(t as dense fp32 rows on a 16-byte boundary -- copied when it is not --, rows, N)"""
    t = _dense_f32(who, name, t, True)
    N = t.shape[-1] if t.dim() else 1
    return t, (t.numel() // N if N else 0), N


@_timed("act_fwd")
def act_forward(u, act):
    """a = act(u) on hipie_act_forward (fp32, last dimension % 4 == 0); act = ACT_GELU (the exact-erf formula of the GEMM epilogue, bit
    for bit) | ACT_RELU.  The forward half of the training step's MLP node (functions.MlpFunction)."""
    u, rows, N = _act_rows16("act_forward", "u", u)
    a = torch.empty_like(u)
    _call("hipie_act_forward", u.data_ptr(), a.data_ptr(), rows, N, int(act))
    return a


@_timed("act_bwd")
def act_backward(u, g, act, want_a=False, want_bias_grad=False, out=None):
    """backward of a = act(u) (hipie_act_backward, fp32, one pass over u and g): g = d loss / d a ->
    (du = g * act'(u),  a = act(u) recomputed with the bits of act_forward | None,  dbias = du summed over the rows, (N,) | None).
    out: the buffer du is written into -- it may be g itself (in place); it is used when it is dense, 16-byte aligned fp32 of u's shape.
    dbias is summed in a fixed order (bit-reproducible).  Nothing is cached: the workspace lives for the call."""
    u, rows, N = _act_rows16("act_backward", "u", u)
    if g.shape != u.shape:
        raise RuntimeError("act_backward: g %s must have the shape of u %s" % (tuple(g.shape), tuple(u.shape)))
    g_in = g
    g, _, _ = _act_rows16("act_backward", "g", g)
    _on_device("act_backward", "out", out)
    if out is not None and out is g_in:
        out = g                                             # in place on the operand the kernel reads (the dense copy, when one was made)
    usable = (out is not None and out.dtype == torch.float32 and out.shape == u.shape and out.is_contiguous() and out.data_ptr() % 16 == 0
              and out.data_ptr() != u.data_ptr())
    du = out if usable else torch.empty_like(u)
    a = torch.empty_like(u) if want_a else None
    dbias = ws = None
    if want_bias_grad:
        dbias = torch.empty(N, dtype=torch.float32, device=u.device)
        ws = _workspace(None, _size("hipie_act_backward_ws_bytes", rows, N), u.device, "act_backward")
    _call("hipie_act_backward", u.data_ptr(), g.data_ptr(), du.data_ptr(), _ptr(a), _ptr(dbias), _ptr(ws), rows, N, int(act))
    return du, a, dbias


def _point_loss_operands(who, src, tgt, tgt_index, pts):
    """the operands both point-loss passes share, the fp32 ones as dense copies where they are not dense"""
    src, tgt, pts = _dense_f32(who, "src", src), _dense_f32(who, "tgt", tgt), _dense_f32(who, "pts", pts)
    _on_device(who, "tgt_index", tgt_index)
    _layout(who, "tgt_index", tgt_index, torch.int64, density=_ANY)
    if src.dim() != 3 or tgt.dim() != 3 or pts.dim() != 3 or pts.shape[0] != src.shape[0] or pts.shape[2] != 2 or tgt_index.shape != src.shape[:1]:
        raise RuntimeError("point_mask_loss: src (N,H,W), tgt (T,Ht,Wt), tgt_index (N,), pts (N,P,2); got %s %s %s %s"
                           % (tuple(src.shape), tuple(tgt.shape), tuple(tgt_index.shape), tuple(pts.shape)))
    return src, tgt, tgt_index.contiguous(), pts


@_timed("point_loss_fwd")
def point_mask_loss_forward(src, tgt, tgt_index, pts, mode, alpha=-1.0):
    """the point-sampled mask losses of one criterion call (hipie_point_mask_loss_forward, fp32): src (N,H,W) logits, tgt (T,Ht,Wt) ALL
    target masks, tgt_index (N,) int64 rows of tgt, pts (N,P,2) (x, y) in [0,1]^2; mode 0 = sigmoid CE, 1 = focal (gamma 2, alpha) ->
    (lmask (N,), ldice (N,), sums (N,3) for point_mask_loss_backward).  Bit-reproducible; the workspace lives for the call."""
    src, tgt, tgt_index, pts = _point_loss_operands("point_mask_loss_forward", src, tgt, tgt_index, pts)
    N, P = src.shape[0], pts.shape[1]
    lmask, ldice, sums = src.new_empty(N), src.new_empty(N), src.new_empty(N, 3)
    ws_bytes = _size("hipie_point_mask_loss_ws_bytes", N, P)
    ws = _workspace(None, ws_bytes, src.device, "point_mask_loss_forward")
    _call("hipie_point_mask_loss_forward", src.data_ptr(), tgt.data_ptr(), tgt_index.data_ptr(), pts.data_ptr(), lmask.data_ptr(), ldice.data_ptr(),
          sums.data_ptr(), ws.data_ptr(), ws_bytes, N, src.shape[1], src.shape[2], tgt.shape[0], tgt.shape[1], tgt.shape[2], P, int(mode),
          float(alpha), 2.0)
    return lmask, ldice, sums


@_timed("point_loss_bwd")
def point_mask_loss_backward(src, tgt, tgt_index, pts, sums, g_mask, g_dice, mode, alpha=-1.0):
    """d_src (N,H,W) of point_mask_loss_forward for the gradients g_mask (N,), g_dice (N,) of its two outputs
    (hipie_point_mask_loss_backward): the samples are recomputed, the corners accumulated with fp32 atomics (not bit-reproducible)."""
    who = "point_mask_loss_backward"
    src, tgt, tgt_index, pts = _point_loss_operands(who, src, tgt, tgt_index, pts)
    sums, g_mask, g_dice = _dense_f32(who, "sums", sums), _dense_f32(who, "g_mask", g_mask), _dense_f32(who, "g_dice", g_dice)
    N = src.shape[0]
    if sums.shape != (N, 3) or g_mask.shape != (N,) or g_dice.shape != (N,):
        raise RuntimeError("point_mask_loss_backward: sums (N,3), g_mask (N,), g_dice (N,) for N=%d" % N)
    d_src = torch.empty_like(src)
    _call("hipie_point_mask_loss_backward", src.data_ptr(), tgt.data_ptr(), tgt_index.data_ptr(), pts.data_ptr(), sums.data_ptr(),
          g_mask.data_ptr(), g_dice.data_ptr(), d_src.data_ptr(), N, src.shape[1], src.shape[2],
          tgt.shape[0], tgt.shape[1], tgt.shape[2], pts.shape[1], int(mode), float(alpha), 2.0)
    return d_src


def _token_focal_operands(who, logits, onehot, keep):
    """logits and onehot as dense fp32 copies where they are not dense, keep as one byte per token"""
    logits, onehot = _dense_f32(who, "logits", logits), _dense_f32(who, "onehot", onehot)
    if logits.dim() != 3 or onehot.shape != logits.shape:
        raise RuntimeError("token_focal: logits and onehot (B,Q,T); got %s %s" % (tuple(logits.shape), tuple(onehot.shape)))
    if keep is not None:
        _on_device(who, "keep", keep)
        if keep.shape != (logits.shape[0], logits.shape[2]):
            raise RuntimeError("token_focal: keep %s must be (B,T) of logits %s" % (tuple(keep.shape), tuple(logits.shape)))
        keep = (keep if keep.dtype in (torch.uint8, torch.bool) else keep > 0).contiguous()           # one byte per token either way
    return logits, onehot, keep


@_timed("token_focal_fwd")
def token_focal_forward(logits, onehot, keep=None, alpha=0.25):
    """sum over (b, q, t) with keep[b, t] != 0 of the binary focal loss (gamma 2) of logits (B,Q,T) against onehot (B,Q,T)
    (hipie_token_focal_forward, fp32) -> 0-d tensor.  keep (B,T) or None.  Bit-reproducible, no host wait."""
    logits, onehot, keep = _token_focal_operands("token_focal_forward", logits, onehot, keep)
    B, Q, T = logits.shape
    out = logits.new_zeros(())
    ws_bytes = _size("hipie_token_focal_ws_bytes", logits.numel())
    ws = _workspace(None, ws_bytes, logits.device, "token_focal_forward")
    _call("hipie_token_focal_forward", logits.data_ptr(), onehot.data_ptr(), _ptr(keep), out.data_ptr(),
          ws.data_ptr(), ws_bytes, B, Q, T, float(alpha), 2.0)
    return out


@_timed("token_focal_bwd")
def token_focal_backward(logits, onehot, keep, g, alpha=0.25):
    """dlogits (B,Q,T) = g * d focal / d logits at kept tokens, exactly 0 at dropped ones (hipie_token_focal_backward); g: 0-d DEVICE
    tensor, the gradient of token_focal_forward's output."""
    logits, onehot, keep = _token_focal_operands("token_focal_backward", logits, onehot, keep)
    g = _dense_f32("token_focal_backward", "g", g)
    if g.numel() != 1:
        raise RuntimeError("token_focal_backward: g must hold one value, got %s" % (tuple(g.shape),))
    B, Q, T = logits.shape
    dlogits = torch.empty_like(logits)
    _call("hipie_token_focal_backward", logits.data_ptr(), onehot.data_ptr(), _ptr(keep), g.data_ptr(),
          dlogits.data_ptr(), B, Q, T, float(alpha), 2.0)
    return dlogits


def uncertain_points_ws_bytes(N, C):
    return _size("hipie_uncertain_points_ws_bytes", int(N), int(C))


@_timed("uncertain_points")
def uncertain_points(src, cand, rest, k, num_points=None, ws=None):
    """the importance point selection of one criterion call (hipie_uncertain_points, fp32, no gradient): src (N,H,W) logits, cand (N,C,2)
    the over-sampled candidates, rest (N,P-k,2) the fresh points (None: P = k) -> pts (N,P,2): pts[:, :k] = the k candidates whose sampled
    |logit| is smallest, in ascending candidate index (ties at the threshold by index), pts[:, k:] = rest.  Bit-reproducible.
    num_points: the P the caller expects; a rest that does not hold P - k points is refused.
    ws: uint8 tensor of at least uncertain_points_ws_bytes(N, C) elements, or None: allocated for the call.
    Nothing is copied: a strided or non-fp32 operand is refused; the layout is checked before the device."""
    who = "uncertain_points"
    _layout(who, "src", src, torch.float32, ndim=3)
    _layout(who, "cand", cand, torch.float32, ndim=3)
    N, C, k = src.shape[0], cand.shape[1], int(k)
    if cand.shape[0] != N or cand.shape[2] != 2:
        raise RuntimeError("uncertain_points: cand must be (N=%d, C, 2), got %s" % (N, tuple(cand.shape)))
    if not 0 <= k <= C:
        raise RuntimeError("uncertain_points: k=%d must be in [0, C=%d]" % (k, C))
    n_rest = 0
    if rest is not None:
        _layout(who, "rest", rest, torch.float32, ndim=3)
        if rest.shape[0] != N or rest.shape[2] != 2:
            raise RuntimeError("uncertain_points: rest must be (N=%d, P - k, 2), got %s" % (N, tuple(rest.shape)))
        n_rest = rest.shape[1]
    P = k + n_rest
    if num_points is not None and P != int(num_points):
        raise RuntimeError("uncertain_points: rest must hold P - k = %d points, got %d" % (int(num_points) - k, n_rest))
    _on_device(who, "src cand rest ws", src, cand, rest, ws)
    ws = _workspace(ws, _size("hipie_uncertain_points_ws_bytes", N, C), src.device, who)
    pts = src.new_empty(N, P, 2)
    _call("hipie_uncertain_points", src.data_ptr(), cand.data_ptr(), rest.data_ptr() if n_rest else None, pts.data_ptr(), ws.data_ptr(), ws.numel(),
          N, src.shape[1], src.shape[2], C, P, k)
    return pts


def mask_match_cost_ws_bytes(Q, T, P):
    return _size("hipie_mask_match_cost_ws_bytes", int(Q), int(T), int(P))


@_timed("mask_match_cost")
def mask_match_cost(pred, tgt, coords, ws=None, ce_out=None, dice_out=None):
    """the point-sampled mask costs of one matcher call (hipie_mask_match_cost, fp32, no gradient): pred (Q,H,W) logits, tgt (T,Ht,Wt) in
    [0,1] at its own resolution, coords (P,2) shared by all masks -> (ce (Q,T), dice (Q,T)) of matcher.mask_costs.  Bit-reproducible.
    ws: uint8 tensor of at least mask_match_cost_ws_bytes(Q, T, P) elements on a 16-byte boundary, or None: allocated for the call.
    ce_out, dice_out: both None (the two results are allocated) or both contiguous fp32 (Q, T) tensors the results are written to and that
    are returned -- views into a caller's buffer, e.g. an image's block of the packed costs of hungarian_cost.
    Nothing is copied: a strided or non-fp32 operand is refused; the layout is checked before the device."""
    who = "mask_match_cost"
    _layout(who, "pred", pred, torch.float32, ndim=3)
    _layout(who, "tgt", tgt, torch.float32, ndim=3)
    _layout(who, "coords", coords, torch.float32, ndim=2)
    Q, T, P = pred.shape[0], tgt.shape[0], coords.shape[0]
    if coords.shape[1] != 2 or (P == 0 and Q * T > 0):
        raise RuntimeError("mask_match_cost: coords must be (P > 0, 2), got %s" % (tuple(coords.shape),))
    if (ce_out is None) != (dice_out is None):
        raise RuntimeError("mask_match_cost: ce_out and dice_out come together")
    if ce_out is not None:
        _layout(who, "ce_out", ce_out, torch.float32, (Q, T))
        _layout(who, "dice_out", dice_out, torch.float32, (Q, T))
    _on_device(who, "pred tgt coords ws ce_out dice_out", pred, tgt, coords, ws, ce_out, dice_out)
    ws = _workspace(ws, _size("hipie_mask_match_cost_ws_bytes", Q, T, P), pred.device, who)
    ce, dice = (pred.new_empty(Q, T), pred.new_empty(Q, T)) if ce_out is None else (ce_out, dice_out)
    _call("hipie_mask_match_cost", pred.data_ptr(), tgt.data_ptr(), coords.data_ptr(), ce.data_ptr(), dice.data_ptr(), ws.data_ptr(), ws.numel(),
          Q, pred.shape[1], pred.shape[2], T, tgt.shape[1], tgt.shape[2], P)
    return ce, dice


OTA_MAX_Q, OTA_MAX_T, OTA_MAX_L = 4096, 256, 1024          # the limits of csrc/ota_match.hip (the match bitmap lives in LDS)


def ota_match_ws_bytes(B, Q, Tmax):
    return _size("hipie_ota_match_ws_bytes", int(B), int(Q), int(Tmax))


def _ota_results(who, res, B, device):
    """the (3, B) int32 block n_pairs | status | repair rounds of one matching call: the host reads it with one copy"""
    if res is None:
        return torch.zeros(3, B, dtype=torch.int32, device=device)
    return _layout(who, "res", res, torch.int32, (3, B))


@_timed("ota_cost")
def ota_cost(logits, boxes, tgt_boxes, pos_map, n_tgt, center_radius=2.5, stride=32, ws=None, res=None):
    """the SimOTA cost of a batch of images (hipie_ota_cost, fp32, no gradient): logits (B,Q,L) raw, boxes (B,Q,4) and tgt_boxes (B,Tmax,4)
    cxcywh, pos_map (B,Tmax,L) uint8, n_tgt (B,) int32 -> (cost, iou, res): cost and iou (B,Tmax,Q), TARGET-major views of `ws`, as
    matcher.ota_cost gives them transposed (+inf / 0 behind n_tgt[b]); res (3,B) int32 whose row 1 holds the status words (bit 0: a box with
    x1 < x0 or y1 < y0, bit 1: a target without a positive token).  Bit-reproducible.
    ws: uint8 tensor of at least ota_match_ws_bytes(B, Q, Tmax) elements, or None: allocated (it backs the two results).
    Nothing is copied: a strided operand or one of another dtype is refused; the layout is checked before the device."""
    who = "ota_cost"
    _layout(who, "logits", logits, torch.float32, ndim=3)
    _layout(who, "tgt_boxes", tgt_boxes, torch.float32, ndim=3)
    B, Q, L = logits.shape
    Tmax = tgt_boxes.shape[1]
    _layout(who, "boxes", boxes, torch.float32, (B, Q, 4))
    _layout(who, "tgt_boxes", tgt_boxes, None, (B, Tmax, 4))
    _layout(who, "pos_map", pos_map, torch.uint8, (B, Tmax, L))
    _layout(who, "n_tgt", n_tgt, torch.int32, (B,))
    res = _ota_results(who, res, B, logits.device)
    _on_device(who, "logits boxes tgt_boxes pos_map n_tgt ws res", logits, boxes, tgt_boxes, pos_map, n_tgt, ws, res)
    ws = _workspace(ws, _size("hipie_ota_match_ws_bytes", B, Q, Tmax), logits.device, who)
    n = B * Tmax * Q * 4
    cost, iou = ws[:n].view(torch.float32).view(B, Tmax, Q), ws[n:2 * n].view(torch.float32).view(B, Tmax, Q)
    _call("hipie_ota_cost", logits.data_ptr(), boxes.data_ptr(), tgt_boxes.data_ptr(), pos_map.data_ptr(), n_tgt.data_ptr(), cost.data_ptr(),
          iou.data_ptr(), res[1].data_ptr(), B, Q, Tmax, L, float(center_radius), float(stride))
    return cost, iou, res


@_timed("ota_assign")
def ota_assign(cost, iou, n_tgt, res=None):
    """SimOTA's dynamic-k assignment (hipie_ota_assign, matcher.dynamic_k_assign with every tie at the lowest index) on the two (B,Tmax,Q)
    buffers of ota_cost; `cost` is modified in place as the reference modifies it, up to its last +inf step -> (pair_q (B,Q), pair_t (B,Q),
    best (B,Tmax), res): int32; image b's matched queries in ascending order are pair_q[b, :n] with the target of each in pair_t[b, :n],
    n = res[0, b]; best[b, t] the matched query of target t with the smallest cost; res (3,B): n_pairs | status (bit 2: the repair loop was
    stopped after Q rounds) | repair rounds.  One workgroup per image, bit-reproducible."""
    who = "ota_assign"
    _layout(who, "cost", cost, torch.float32, ndim=3)
    B, Tmax, Q = cost.shape
    _layout(who, "iou", iou, torch.float32, (B, Tmax, Q))
    _layout(who, "n_tgt", n_tgt, torch.int32, (B,))
    res = _ota_results(who, res, B, cost.device)
    _on_device(who, "cost iou n_tgt res", cost, iou, n_tgt, res)
    pairs = torch.empty(2, B, Q, dtype=torch.int32, device=cost.device)
    best = torch.empty(B, Tmax, dtype=torch.int32, device=cost.device)
    _call("hipie_ota_assign", cost.data_ptr(), iou.data_ptr(), n_tgt.data_ptr(), pairs[0].data_ptr(), pairs[1].data_ptr(), best.data_ptr(),
          res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), B, Q, Tmax)
    return pairs[0], pairs[1], best, res


HUNGARIAN_MAX_Q, HUNGARIAN_MAX_T, HUNGARIAN_MAX_L = 4096, 256, 1024          # the limits of csrc/hungarian_cost.hip (those of the SimOTA kernels)
HUNGARIAN_STATUS = ((1, "a box with x1 < x0 or y1 < y0 (or a NaN)"), (8, "a label outside [0, L)"), (16, "the target offsets do not fit the packed output"))


def hungarian_cost_ws_bytes(B, Q):
    return _size("hipie_hungarian_cost_ws_bytes", int(B), int(Q))


def _image_stride(t, name, row):
    """the image stride of a fp32 (B, Q, row) tensor whose images are dense (a slice of the query dimension of a dense tensor is); nothing is
    copied, and the device is the caller's to check, after the layout"""
    _layout("hungarian_cost", name, t, torch.float32, density=_ANY)
    if t.dim() != 3 or t.shape[2] != row:
        raise RuntimeError("%s must be (B, Q, %d), got %s" % (name, row, tuple(t.shape)))
    B, Q = t.shape[:2]
    if Q * row and (t.stride(2) != 1 or t.stride(1) != row or (B > 1 and t.stride(0) < Q * row)):
        raise RuntimeError("%s tensor has to be dense within an image (strides %s)" % (name, tuple(t.stride())))
    return t.stride(0) if B > 1 else Q * row


@_timed("hungarian_cost")
def hungarian_cost(logits, boxes, tgt_boxes, n_tgt, t_off, sum_t, weights, pos_map=None, labels=None, is_thing=None, ce=None, dice=None, with_boxes=True,
                   stuff_takes_mean=True, out=None, ws=None):
    """the cost matrices of a Hungarian matcher call for a batch of images (hipie_hungarian_cost, fp32, no gradient): logits (B,Q,L) raw, boxes
    (B,Q,4) cxcywh (None with with_boxes=False; both may be slices of the query dimension of a dense tensor), tgt_boxes (B,Tmax,4), n_tgt and
    t_off (B,) int32 (t_off: the exclusive prefix sum), sum_t: the host's total of n_tgt; weights: the five (cls, l1, giou, mask, dice);
    exactly one of pos_map (B,Tmax,L) uint8 and labels (B,Tmax) int32; is_thing (B,Tmax) uint8 (needed with the stuff mean and the box costs);
    ce, dice: None or the point-sampled mask costs, fp32 (Q * sum_t,), packed like the result
    -> out, fp32 (Q * sum_t + B,): image b's costs are out[Q * t_off[b] : Q * (t_off[b] + n_tgt[b])].view(Q, n_tgt[b]) (QUERY-major, no
    padding), and out[Q * sum_t:].view(torch.int32) holds the B status words (HUNGARIAN_STATUS) -- one copy carries both to the host.
    out: such a tensor, or None: allocated.  ws: uint8 tensor of at least hungarian_cost_ws_bytes(B, Q) elements, or None: allocated when the
    stuff mean needs it.  One launch, two with the stuff mean; bit-reproducible.
    Nothing is copied: an operand of another dtype or layout, or a shape outside Q <= 4096, Tmax <= 256, 1 <= L <= 1024, B <= 65535, is
    refused; the layout is checked before the device."""
    ls = _image_stride(logits, "logits", logits.shape[2] if logits.dim() == 3 else 0)
    B, Q, L = logits.shape
    who = "hungarian_cost"
    _layout(who, "tgt_boxes", tgt_boxes, torch.float32, ndim=3)
    Tmax, sum_t = tgt_boxes.shape[1], int(sum_t)
    _layout(who, "tgt_boxes", tgt_boxes, None, (B, Tmax, 4))
    bs = 0
    if with_boxes:
        if boxes is None:
            raise RuntimeError("hungarian_cost: boxes are needed with the box costs")
        bs = _image_stride(boxes, "boxes", 4)
        _layout(who, "boxes", boxes, None, (B, Q, 4), density=_ANY)
    _layout(who, "n_tgt", n_tgt, torch.int32, (B,))
    _layout(who, "t_off", t_off, torch.int32, (B,))
    if (pos_map is None) == (labels is None):
        raise RuntimeError("hungarian_cost: exactly one of pos_map and labels")
    if pos_map is not None:
        _layout(who, "pos_map", pos_map, torch.uint8, (B, Tmax, L))
    else:
        _layout(who, "labels", labels, torch.int32, (B, Tmax))
    mean = bool(with_boxes and stuff_takes_mean)
    if mean:
        if is_thing is None:
            raise RuntimeError("hungarian_cost: is_thing is needed with the stuff mean")
        _layout(who, "is_thing", is_thing, torch.uint8, (B, Tmax))
    if (ce is None) != (dice is None):
        raise RuntimeError("hungarian_cost: ce and dice come together")
    if not 0 <= sum_t <= B * Tmax:
        raise RuntimeError("hungarian_cost: sum_t=%d outside [0, B x Tmax = %d]" % (sum_t, B * Tmax))
    if ce is not None:
        _layout(who, "ce", ce, torch.float32, (Q * sum_t,))
        _layout(who, "dice", dice, torch.float32, (Q * sum_t,))
    if Q > HUNGARIAN_MAX_Q or Tmax > HUNGARIAN_MAX_T or L > HUNGARIAN_MAX_L or (L < 1 and B * Q * Tmax > 0) or B > 65535:
        raise RuntimeError("hungarian_cost: B=%d, Q=%d, Tmax=%d, L=%d outside B <= 65535, Q <= %d, Tmax <= %d, 1 <= L <= %d"
                           % (B, Q, Tmax, L, HUNGARIAN_MAX_Q, HUNGARIAN_MAX_T, HUNGARIAN_MAX_L))
    _layout(who, "out", out, torch.float32, (Q * sum_t + B,))
    _on_device(who, "logits boxes tgt_boxes n_tgt t_off pos_map labels is_thing ce dice out ws", logits, boxes if with_boxes else None, tgt_boxes,
               n_tgt, t_off, pos_map, labels, is_thing if mean else None, ce, dice, out, ws)
    if out is None:
        out = torch.empty(Q * sum_t + B, dtype=torch.float32, device=logits.device)
    n = Q * sum_t
    status = out[n:].view(torch.int32)
    if B * Q * Tmax == 0:                                    # no launch: nothing to check either
        status.zero_()
        return out
    if mean:
        ws = _workspace(ws, _size("hipie_hungarian_cost_ws_bytes", B, Q), logits.device, who)
    w = [float(x) for x in weights]
    if len(w) != 5:
        raise RuntimeError("hungarian_cost: five weights (cls, l1, giou, mask, dice), got %d" % len(w))
    _call("hipie_hungarian_cost", logits.data_ptr(), ls, _ptr(boxes) if with_boxes else None, bs, tgt_boxes.data_ptr(), n_tgt.data_ptr(), t_off.data_ptr(),
          _ptr(pos_map), _ptr(labels), _ptr(is_thing) if mean else None, _ptr(ce), _ptr(dice), out.data_ptr() if n else None,
          status.data_ptr(), ws.data_ptr() if mean else None, ws.numel() if mean else 0, B, Q, Tmax, L, sum_t, *w,
          1 if with_boxes else 0, 1 if stuff_takes_mean else 0)
    return out


# the status words of hungarian_assign: the cost kernel's bits carried over, and the solver's own (the first two are scipy's messages)
HUNGARIAN_STATUS = HUNGARIAN_STATUS + ((32, "matrix contains invalid numeric entries"), (64, "cost matrix is infeasible"),
                                       (128, "the search of a row did not end within min(Q, T) columns"))


def hungarian_assign_ws_bytes(Q, sum_t):
    return _size("hipie_hungarian_assign_ws_bytes", int(Q), int(sum_t))


@_timed("hungarian_assign")
def hungarian_assign(costs, n_tgt, t_off, sum_t, Q, Tmax, ws=None):
    """the one-to-one assignment of every image of a batch on the device (hipie_hungarian_assign: scipy.optimize.linear_sum_assignment's
    pairs, tie for tie): costs fp32 (Q * sum_t + B,), what hungarian_cost returns -- image b's (Q, n_tgt[b]) block query-major at element
    Q * t_off[b], the B status words of the cost kernel behind the blocks; n_tgt, t_off (B,) int32; sum_t, Q, Tmax: host integers
    -> (pair_q, pair_t, status): pair_q, pair_t (B, K) int64 with K = min(Q, Tmax), image b's pairs in its first min(Q, n_tgt[b]) entries in
    ascending query order and 0 behind them; status (B,) int32 (HUNGARIAN_STATUS): the cost kernel's bits carried over, 32: a NaN or -inf in the
    block, 64: infeasible, 128: the iteration cap.  An image with a non-zero status has all-zero pairs.  Nothing is read by the host.
    ws: uint8 tensor of at least hungarian_assign_ws_bytes(Q, sum_t) elements, or None: allocated.  One launch, a workgroup per image.
    Nothing is copied: an operand of another dtype or layout, or a shape outside Q <= 4096, Tmax <= 256, B <= 65535, is refused; the layout
    is checked before the device."""
    if n_tgt.dim() != 1:
        raise RuntimeError("n_tgt must be (B,), got %s" % (tuple(n_tgt.shape),))
    B, Q, Tmax, sum_t = int(n_tgt.shape[0]), int(Q), int(Tmax), int(sum_t)
    who = "hungarian_assign"
    _layout(who, "n_tgt", n_tgt, torch.int32, (B,))
    _layout(who, "t_off", t_off, torch.int32, (B,))
    if Q < 0 or Tmax < 0 or not 0 <= sum_t <= B * Tmax:
        raise RuntimeError("hungarian_assign: Q=%d, Tmax=%d, sum_t=%d outside Q >= 0, Tmax >= 0, 0 <= sum_t <= B x Tmax = %d" % (Q, Tmax, sum_t, B * Tmax))
    _layout(who, "costs", costs, torch.float32, (Q * sum_t + B,))
    if Q > HUNGARIAN_MAX_Q or Tmax > HUNGARIAN_MAX_T or B > 65535:
        raise RuntimeError("hungarian_assign: B=%d, Q=%d, Tmax=%d outside B <= 65535, Q <= %d, Tmax <= %d" % (B, Q, Tmax, HUNGARIAN_MAX_Q, HUNGARIAN_MAX_T))
    _on_device(who, "costs n_tgt t_off ws", costs, n_tgt, t_off, ws)
    K, n = min(Q, Tmax), Q * sum_t
    pairs = torch.empty(2, B, K, dtype=torch.int64, device=costs.device)
    status = torch.empty(B, dtype=torch.int32, device=costs.device)
    if B * Q * Tmax == 0:                                    # no launch: nothing to solve (K == 0 or B == 0: the pairs are empty)
        status.copy_(costs[n:].view(torch.int32))
        return pairs[0], pairs[1], status
    ws = _workspace(ws, _size("hipie_hungarian_assign_ws_bytes", Q, sum_t), costs.device, who)
    _call("hipie_hungarian_assign", costs.data_ptr() if n else None, costs[n:].data_ptr(), n_tgt.data_ptr(), t_off.data_ptr(), pairs[0].data_ptr(),
          pairs[1].data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), B, Q, Tmax, sum_t)
    return pairs[0], pairs[1], status


PAIR_MAX_B, PAIR_MAX_K = 64, 65536            # the limits of csrc/pair_loss.hip (the pair lists live in the kernel arguments)
PAIR_STATUS = ((1, "boxes with x1 < x0 or y1 < y0 (or a NaN)"), (2, "a query or target index out of range"))


def pair_box_loss_ws_bytes(K):
    return _size("hipie_pair_box_loss_ws_bytes", int(K))


def _pair_lists(who, pairs, with_t=True):
    """the matched pairs of a batch -- per image (query idx, target idx), int64 contiguous DEVICE tensors -- as the HOST arrays of the C entries:
    (addresses of the query lists, of the target lists | None, lengths, K).  Nothing is copied; the layout is checked before the device."""
    B = len(pairs)
    qs, ts, ns = (ctypes.c_void_p * B)(), (ctypes.c_void_p * B)(), (ctypes.c_int64 * B)()
    for b, (q, t) in enumerate(pairs):
        for name, x in (("query", q), ("target", t)):
            if x.dtype != torch.int64 or x.dim() != 1 or not x.is_contiguous():
                raise RuntimeError("%s: the %s indices of image %d must be a contiguous 1-d torch.int64 tensor, got %s %s"
                                   % (who, name, b, x.dtype, tuple(x.shape)))
        if q.shape != t.shape:
            raise RuntimeError("%s: image %d has %d query and %d target indices" % (who, b, q.numel(), t.numel()))
        _on_device(who, "pair_q pair_t", q, t)
        ns[b] = q.numel()
        if q.numel():
            qs[b], ts[b] = q.data_ptr(), t.data_ptr()
    return qs, (ts if with_t else None), ns, sum(ns)


@_timed("pair_box_loss_fwd")
def pair_box_loss_forward(boxes, iou, pairs, tgt_boxes, is_thing, count, mode):
    """the box losses of the matched pairs of one criterion call (hipie_pair_box_loss_forward): boxes (B,Q,4) fp32 cxcywh -- any image and row
    stride, e.g. a slice of the query axis --, iou None or the (B,Q) box-IoU logits (strided too), pairs: per image (query idx, target idx) int64
    on the device, tgt_boxes (B,Tmax,4) fp32 and is_thing (B,Tmax) uint8 or None (functions.pack_match_targets), count: the normaliser;
    mode 0 = DetCriterion.loss_boxes, 1 = MaskCriterion.loss_boxes -> (out (8,) fp32: loss_bbox, loss_giou, loss_boxiou and the factors of the
    backward; pair_grad (K,9); status (1,) int32, PAIR_STATUS).  Two launches, no host wait, bit-reproducible.  Without pairs nothing is
    launched and out is all zero.  Nothing is copied: another dtype or layout, B > 64 or more than 65536 pairs is refused."""
    B, Q = boxes.shape[0], boxes.shape[1] if boxes.dim() == 3 else -1
    who = "pair_box_loss_forward"
    _layout(who, "boxes", boxes, torch.float32, (B, Q, 4), density=_ROWS)
    _layout(who, "iou", iou, torch.float32, (B, Q), density=_ANY)
    Tmax = tgt_boxes.shape[1] if tgt_boxes.dim() == 3 else -1
    _layout(who, "tgt_boxes", tgt_boxes, torch.float32, (B, Tmax, 4))
    _layout(who, "is_thing", is_thing, torch.uint8, (B, Tmax))
    if len(pairs) != B or B > PAIR_MAX_B:
        raise RuntimeError("pair_box_loss: %d pair lists for B=%d images (at most %d)" % (len(pairs), B, PAIR_MAX_B))
    qs, ts, ns, K = _pair_lists("pair_box_loss", pairs)
    if K > PAIR_MAX_K:
        raise RuntimeError("pair_box_loss: K=%d pairs, at most %d" % (K, PAIR_MAX_K))
    _on_device(who, "boxes iou tgt_boxes is_thing", boxes, iou, tgt_boxes, is_thing)
    out = boxes.new_zeros(8)
    pair_grad = boxes.new_empty(K, 9)
    status = torch.zeros(1, dtype=torch.int32, device=boxes.device)
    ws_bytes = _size("hipie_pair_box_loss_ws_bytes", K)
    ws = _workspace(None, ws_bytes, boxes.device, who)
    _call("hipie_pair_box_loss_forward", boxes.data_ptr(), boxes.stride(0), boxes.stride(1), _ptr(iou),
          0 if iou is None else iou.stride(0), 0 if iou is None else iou.stride(1), qs, ts, ns, tgt_boxes.data_ptr(),
          _ptr(is_thing), out.data_ptr(), pair_grad.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, B, Q,
          Tmax, int(mode), float(count))
    return out, pair_grad, status


@_timed("pair_box_loss_bwd")
def pair_box_loss_backward(pairs, out, pair_grad, g_bbox, g_giou, g_boxiou, B, Q, with_iou):
    """(d_boxes (B,Q,4), d_iou (B,Q) | None) of pair_box_loss_forward for the gradients of its three scalars, DEVICE tensors of one fp32 element
    each (hipie_pair_box_loss_backward): both results are zero-filled and every pair adds its stored gradient with an fp32 atomic -- duplicates
    of an (image, query) sum; one target per (image, query): bit-reproducible.  No host wait."""
    qs, _, ns, K = _pair_lists("pair_box_loss_backward", pairs, with_t=False)
    who = "pair_box_loss_backward"
    _layout(who, "out", out, torch.float32, (8,))
    _layout(who, "pair_grad", pair_grad, torch.float32, (K, 9))
    g_boxiou = g_boxiou if with_iou else None
    for g in (g_bbox, g_giou, g_boxiou):
        if g is not None and (g.dtype != torch.float32 or g.numel() != 1):
            raise RuntimeError("pair_box_loss_backward: an upstream gradient must hold one torch.float32 value, got %s %s" % (g.dtype, tuple(g.shape)))
    _on_device(who, "out pair_grad g_bbox g_giou g_boxiou", out, pair_grad, g_bbox, g_giou, g_boxiou)
    d_boxes = out.new_empty(B, Q, 4)
    d_iou = out.new_empty(B, Q) if with_iou else None
    _call("hipie_pair_box_loss_backward", qs, ns, out.data_ptr(), pair_grad.data_ptr(), g_bbox.data_ptr(), g_giou.data_ptr(),
          _ptr(g_boxiou), d_boxes.data_ptr(), _ptr(d_iou), B, Q)
    return d_boxes, d_iou


@_timed("positive_onehot")
def positive_onehot(pairs, pos_map, Q):
    """criterion._positive_onehot on hipie_positive_onehot: pairs as in pair_box_loss_forward, pos_map (B,Tmax,L) uint8 -> onehot (B,Q,L) fp32,
    zero but onehot[b, q_i] = (pos_map[b, t_i] != 0).  A fill and one launch, no host wait."""
    if pos_map.dim() != 3:
        raise RuntimeError("positive_onehot: pos_map must be (B, Tmax, L), got %s" % (tuple(pos_map.shape),))
    B, Tmax, L = pos_map.shape
    _layout("positive_onehot", "pos_map", pos_map, torch.uint8, (B, Tmax, L))
    if len(pairs) != B or B > PAIR_MAX_B:
        raise RuntimeError("positive_onehot: %d pair lists for B=%d images (at most %d)" % (len(pairs), B, PAIR_MAX_B))
    qs, ts, ns, K = _pair_lists("positive_onehot", pairs)
    if K > PAIR_MAX_K:
        raise RuntimeError("positive_onehot: K=%d pairs, at most %d" % (K, PAIR_MAX_K))
    _on_device("positive_onehot", "pos_map", pos_map)
    onehot = torch.empty(B, int(Q), L, dtype=torch.float32, device=pos_map.device)
    _call("hipie_positive_onehot", qs, ts, ns, pos_map.data_ptr(), onehot.data_ptr(), B, int(Q), Tmax, L)
    return onehot


OPTIM_MAX_GROUPS = 8
OPTIM_SEGMENT_WORDS = 6          # int64 words of a segment record: p, g, m, v, numel, group


def optim_chunk():
    """elements per chunk-map entry of the optimizer kernels (hipie_optim_chunk)"""
    return _size("hipie_optim_chunk")


def optim_norm_ws_bytes(n_chunks):
    return _size("hipie_optim_norm_ws_bytes", int(n_chunks))


def _optim_tables(who, table, cmap):
    """the segment table (n_seg, 6) int64 and the chunk map (n_chunks, 2) int64 of the optimizer kernels: layout, then device"""
    for t, name, words in ((table, "table", OPTIM_SEGMENT_WORDS), (cmap, "cmap", 2)):
        if t.dim() != 2:
            raise RuntimeError("%s must be (n, %d), got %s" % (name, words, tuple(t.shape)))
        _layout(who, name, t, torch.int64, (int(t.shape[0]), words))
    _on_device(who, "table cmap", table, cmap)
    if cmap.device != table.device:
        raise RuntimeError("%s: table and cmap on different devices" % who)
    return int(table.shape[0]), int(cmap.shape[0])


@_timed("optim_grad_norm")
def optim_grad_norm(table, cmap, grad_scale=1.0, ws=None):
    """the 2-norm of grad_scale x (every gradient of the segment table) as a 0-dim fp32 device tensor (hipie_optim_grad_norm: float64 sums in a
    fixed order, bit-reproducible, nothing read by the host).  table (n_seg, 6) int64: the records { p, g, m, v addresses, numel, group } (g == 0: no
    gradient); cmap (n_chunks, 2) int64: (segment, element offset) per optim_chunk() elements.  The ADDRESSES in the table are the caller's
    promise: the tensors behind them stay alive until this returns (the launches are then ordered on the stream).  ws: uint8 tensor of at least
    optim_norm_ws_bytes(n_chunks) elements, or None: allocated.  Two launches."""
    n_seg, n_chunks = _optim_tables("optim_grad_norm", table, cmap)
    out = torch.empty((), dtype=torch.float32, device=table.device)
    if n_seg == 0 or n_chunks == 0:
        return out.zero_()
    _on_device("optim_grad_norm", "ws", ws)
    ws = _workspace(ws, _size("hipie_optim_norm_ws_bytes", n_chunks), table.device, "optim_grad_norm")
    _call("hipie_optim_grad_norm", table.data_ptr(), n_seg, cmap.data_ptr(), n_chunks, ws.data_ptr(), ws.numel(), float(grad_scale), out.data_ptr())
    return out


@_timed("optim_adamw_step")
def optim_adamw_step(table, cmap, steps, bc, group_lr, group_wd, betas, eps, norm=None, max_norm=0.0, grad_scale=1.0, write_grads=False):
    """one AdamW step of every tensor of the segment table that has a gradient, in place (hipie_optim_adamw_step; table, cmap as for
    optim_grad_norm): steps (n_seg,) int32 the per-parameter step counts and bc (n_seg, 2) fp32 their bias corrections, both on the device and
    advanced by the call; group_lr, group_wd: host sequences of at most 8 floats, indexed by a record's group; betas (b1, b2), eps: host floats.
    norm: the 0-dim device tensor of optim_grad_norm -- the gradients enter as g x grad_scale x min(max_norm / (norm + 1e-6), 1) -- or None: no
    clipping.  write_grads: the clipped gradients are also written back.  Nothing is read by the host.  Two launches."""
    n_seg, n_chunks = _optim_tables("optim_adamw_step", table, cmap)
    _layout("optim_adamw_step", "steps", steps, torch.int32, (n_seg,))
    _layout("optim_adamw_step", "bc", bc, torch.float32, (n_seg, 2))
    _layout("optim_adamw_step", "norm", norm, torch.float32, ())
    _on_device("optim_adamw_step", "steps bc norm", steps, bc, norm)
    n_groups = len(group_lr)
    if len(group_wd) != n_groups or not 1 <= n_groups <= OPTIM_MAX_GROUPS:
        raise RuntimeError("optim_adamw_step: %d learning rates, %d weight decays: one each for 1 to %d groups" % (n_groups, len(group_wd), OPTIM_MAX_GROUPS))
    arr = ctypes.c_double * n_groups
    lr, wd = arr(*[float(x) for x in group_lr]), arr(*[float(x) for x in group_wd])
    _call("hipie_optim_adamw_step", table.data_ptr(), n_seg, cmap.data_ptr(), n_chunks, steps.data_ptr(), bc.data_ptr(), lr, wd, n_groups,
          float(betas[0]), float(betas[1]), float(eps), _ptr(norm),
          float(max_norm), float(grad_scale), int(bool(write_grads)))


@_timed("add_layernorm")
def add_layernorm_sum(x, delta, weight, bias, eps, addend):
    """n = LayerNorm(x + delta) and n + addend, both in x's dtype, one launch (the encoder's post-norm + next `src + pos`)."""
    C = x.shape[-1]
    rows = x.numel() // C
    if addend.dtype != x.dtype or addend.shape != x.shape:
        raise RuntimeError("add_layernorm_sum: addend must match x")
    who = "add_layernorm_sum"
    _on_device(who, "x delta weight bias addend", x, delta, weight, bias, addend)
    out, s = torch.empty_like(x), torch.empty_like(x)
    _call("hipie_add_layernorm_sum", _layout(who, "x", x).data_ptr(), _layout(who, "delta", delta).data_ptr(),
          _layout(who, "weight", weight, torch.float32).data_ptr(), _layout(who, "bias", bias, torch.float32).data_ptr(), None, out.data_ptr(),
          _layout(who, "addend", addend).data_ptr(), s.data_ptr(),
          rows, C, float(eps), _DT[x.dtype], _DT[delta.dtype], _DT[x.dtype])
    return out, s


@_timed("add_layernorm")
def add_layernorm_dec(x, delta, weight, bias, eps, aux_dtype, want16=False, addend=None):
    """n = LayerNorm(x + delta) for the fp32 query stream of the decoders: returns (n f32, n in aux_dtype or None,
    (n + addend) in aux_dtype or None) from one launch.  x (..., C) f32; delta any of f32/f16/bf16; addend aux_dtype."""
    C = x.shape[-1]
    rows = x.numel() // C
    who = "add_layernorm_dec"
    _on_device(who, "x delta weight bias addend", x, delta, weight, bias, addend)
    out = torch.empty_like(x)
    n16 = _alloc(tuple(x.shape), aux_dtype, x.device) if want16 else None
    s16 = _alloc(tuple(x.shape), aux_dtype, x.device) if addend is not None else None
    if addend is not None and ((addend.dtype != aux_dtype or addend.shape != x.shape) if aux_dtype != "hl8" else
                               (addend.dtype != torch.float16 or addend.numel() != 2 * x.numel())):
        raise RuntimeError("add_layernorm_dec: addend must match x's shape in aux_dtype")
    _layout(who, "addend", addend)
    _call("hipie_add_layernorm_dec", _layout(who, "x", x, torch.float32).data_ptr(), _layout(who, "delta", delta).data_ptr(),
          _layout(who, "weight", weight, torch.float32).data_ptr(), _layout(who, "bias", bias, torch.float32).data_ptr(), out.data_ptr(), _ptr(n16),
          _ptr(addend), _ptr(s16),
          rows, C, float(eps), _DT[delta.dtype], _code(aux_dtype))
    return out, n16, s16


_GN_WS = {}


def group_norm_ok(x, groups):
    if not x.is_cuda or x.dim() != 4 or x.dtype not in _DT or x.shape[1] != groups * 8 or groups > 64 or 256 % groups:
        return False
    return x.is_contiguous(memory_format=torch.channels_last) or (x.is_contiguous() and (x.shape[2] * x.shape[3]) % 8 == 0)


@_timed("group_norm")
def group_norm(x, groups, weight, bias, eps, relu=False, prebias=None, out_dtype=None, out_nchw=False):
    """GroupNorm(groups, C = 8 * groups)(x + prebias[c]) (+ ReLU) on a (B,C,H,W) tensor in the memory format it arrives in
    (channels-last stays channels-last: no NHWC -> NCHW copy); fp32 statistics.  out_nchw: a channels-last input leaves as a dense
    NCHW tensor (transposed inside the kernel; H*W % 64 == 0) -- what `.contiguous()` would make of the result, without that pass."""
    B, C, H, W = x.shape
    nhwc = x.is_contiguous(memory_format=torch.channels_last) and not (x.is_contiguous() and C > 1 and H * W > 1)
    if not nhwc and not x.is_contiguous():
        raise RuntimeError("group_norm: x must be NCHW- or channels-last-contiguous")
    _on_device("group_norm", "x prebias weight bias", x, prebias, weight, bias)
    out_dtype = out_dtype or x.dtype
    if out_nchw and nhwc and (H * W) % 64 == 0:
        nhwc = 2
        out = torch.empty(B, C, H, W, dtype=out_dtype, device=x.device)
    else:
        out = torch.empty_like(x, dtype=out_dtype)            # preserves the memory format
    key = (str(x.device), B * groups, torch.cuda.current_stream(x.device).cuda_stream)      # per stream: the two branches of the head overlap
    ws = _GN_WS.get(key)
    if ws is None:
        ws = _GN_WS[key] = torch.empty(2 * B * groups * 512, dtype=torch.float32, device=x.device)
    _call("hipie_group_norm", x.data_ptr(), None if prebias is None else _layout("group_norm", "prebias", prebias, torch.float32).data_ptr(),
          _layout("group_norm", "weight", weight, torch.float32).data_ptr(), _layout("group_norm", "bias", bias, torch.float32).data_ptr(), out.data_ptr(),
          ws.data_ptr(), B, C, H * W, groups, int(nhwc), float(eps), 1 if relu else 0, _DT[x.dtype], _DT[out_dtype])
    return out


def _gn_train_args(who, x, weight, bias, dy=None, stat=None):
    """(B, C, HW) of a dense NCHW fp32 map for the training GroupNorm pair; host tensors and other layouts / types are refused"""
    _on_device(who, "x weight bias dy stat", x, weight, bias, dy, stat)
    _layout(who, "x", x, torch.float32, None, 4)
    B, C, H, W = x.shape
    if weight.numel() != C or bias.numel() != C:
        raise RuntimeError("%s: weight and bias must have x's %d channels" % (who, C))
    if weight.dtype is not torch.float32 or bias.dtype is not torch.float32 or not weight.is_contiguous() or not bias.is_contiguous():
        _layout(who, "weight", weight, torch.float32)          # raises for one of the two
        _layout(who, "bias", bias, torch.float32)
    return B, C, H * W


@_timed("group_norm_train")
def group_norm_train_forward(x, groups, weight, bias, eps, relu=False):
    """GroupNorm(groups, C = 8 * groups)(x) (+ ReLU) of a dense NCHW fp32 map for the training step (hipie_group_norm_train_forward) ->
    (y, stat): y has the bits of group_norm(x, ...) on the same arguments, stat (B, groups, 2) = the (mean, rstd) it normalised with, what
    group_norm_backward takes.  The workspace lives for the call (its size is the library's query)."""
    B, C, HW = _gn_train_args("group_norm_train_forward", x, weight, bias)
    y = torch.empty_like(x)
    stat = torch.empty(B, groups, 2, dtype=torch.float32, device=x.device)
    ws = _workspace(None, _size("hipie_group_norm_backward_ws_bytes", B, C, HW), x.device, "group_norm_train_forward")
    _call("hipie_group_norm_train_forward", x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), stat.data_ptr(), ws.data_ptr(),
          B, C, HW, int(groups), float(eps), 1 if relu else 0)
    return y, stat


@_timed("group_norm_bwd")
def group_norm_backward(x, dy, stat, groups, weight, bias, relu=False, want_dx=True, want_param_grads=True):
    """backward of group_norm_train_forward (hipie_group_norm_backward, fp32 NCHW): dy = gradient of y, stat = the forward's ->
    (dx | None, dgamma | None, dbeta | None); with relu the mask is recomputed from x and stat (the forward's y > 0 bit for bit).
    Without want_dx the second pass is not launched, without want_param_grads the parameter sums are not; the sums are added in a fixed
    order (bit-reproducible).  Nothing is cached: the workspace lives for the call."""
    who = "group_norm_backward"
    B, C, HW = _gn_train_args(who, x, weight, bias, dy, stat)
    if dy.shape != x.shape or stat.shape != (B, groups, 2) or dy.dtype is not torch.float32 or stat.dtype is not torch.float32 \
            or not dy.is_contiguous() or not stat.is_contiguous():
        _layout(who, "dy", dy, torch.float32, x.shape)          # raises for one of the two
        _layout(who, "stat", stat, torch.float32, (B, groups, 2))
    dx = torch.empty_like(x) if want_dx else None
    dgamma = dbeta = None
    if want_param_grads:
        dgamma, dbeta = (torch.empty(C, dtype=torch.float32, device=x.device) for _ in range(2))
    ws_bytes = _size("hipie_group_norm_backward_ws_bytes", B, C, HW)
    ws = _workspace(None, ws_bytes, x.device, who)
    _call("hipie_group_norm_backward", x.data_ptr(), dy.data_ptr(), stat.data_ptr(), weight.data_ptr(), bias.data_ptr(), _ptr(dx),
          _ptr(dgamma), _ptr(dbeta), ws.data_ptr(), ws_bytes,
          B, C, HW, int(groups), 1 if relu else 0)
    return dx, dgamma, dbeta


@_timed("add_cast")
def add_cast(a, b):
    """(a f32 + b 16-bit) rounded once to b's dtype; same shapes, numel % 4 == 0."""
    if a.shape != b.shape:
        raise RuntimeError("add_cast: shapes differ")
    _on_device("add_cast", "a b", a, b)
    out = torch.empty_like(b)
    _call("hipie_add_cast", _layout("add_cast", "a", a, torch.float32).data_ptr(), _layout("add_cast", "b", b).data_ptr(), out.data_ptr(), a.numel(),
          _DT[b.dtype])
    return out


@_timed("add_cast")
def add_to_hl8(a, b_hl8):
    """HL8 of (a + b): a (..., C) fp32, b_hl8 (..., 2C) fp16 HL8 of the same rows -> (..., 2C) HL8, one pass (hipie_add_cast, HL8 form)."""
    if b_hl8.dtype != torch.float16 or b_hl8.numel() != 2 * a.numel() or a.shape[-1] % 8:
        raise RuntimeError("add_to_hl8: a (.., C) fp32 and b (.., 2C) HL8 device tensors, C %% 8 == 0")
    _on_device("add_to_hl8", "a b_hl8", a, b_hl8)
    out = torch.empty_like(b_hl8)
    _call("hipie_add_cast", _layout("add_to_hl8", "a", a, torch.float32).data_ptr(), _layout("add_to_hl8", "b_hl8", b_hl8).data_ptr(), out.data_ptr(),
          a.numel(), HL8)
    return out


@_timed("batched_nms")
def batched_nms(boxes, scores, classes, iou_threshold, coordinate_trick=None):
    """boxes (B,Q,4) normalised cxcywh, scores (B,Q), classes (B,Q) int64 -> keep (B,Q) int32 (query indices in
    decreasing-score order, -1 padded), count (B) int32.  torchvision.ops.batched_nms semantics per image."""
    B, Q = scores.shape
    if coordinate_trick is None:
        coordinate_trick = Q * 4 <= 4000                  # torchvision/ops/boxes.py batched_nms switch
    _on_device("batched_nms", "boxes scores classes", boxes, scores, classes)
    order = scores.sort(dim=1, descending=True, stable=True)[1].to(torch.int32)
    keep = torch.empty(B, Q, dtype=torch.int32, device=boxes.device)
    count = torch.empty(B, dtype=torch.int32, device=boxes.device)
    _call("hipie_batched_nms", _layout("batched_nms", "boxes", boxes, torch.float32).data_ptr(),
          _layout("batched_nms", "classes", classes, torch.int64).data_ptr(), order.data_ptr(),
          keep.data_ptr(), count.data_ptr(), B, Q, float(iou_threshold), int(coordinate_trick))
    return keep, count


@_timed("mask_finalize")
def mask_finalize(masks, qidx, up, crop_hw, out_hw, threshold):
    """masks (Q,hm,wm) stride-`up` logits, qidx (n) int32 rows (or None) -> (n,out_h,out_w) uint8:
    bilinear x`up` -> sigmoid > threshold -> crop -> nearest resize to out_hw."""
    Q, hm, wm = masks.shape
    n = Q if qidx is None else int(qidx.shape[0])
    _on_device("mask_finalize", "masks qidx", masks, qidx)
    out = torch.empty(n, out_hw[0], out_hw[1], dtype=torch.uint8, device=masks.device)
    _call("hipie_mask_finalize", _layout("mask_finalize", "masks", masks).data_ptr(), _DT[masks.dtype],
          None if qidx is None else _layout("mask_finalize", "qidx", qidx, torch.int32).data_ptr(),
          n, hm, wm, int(up), int(crop_hw[0]), int(crop_hw[1]), int(out_hw[0]), int(out_hw[1]), float(threshold), out.data_ptr())
    return out


SEM_PAN_CLASSES = 160          # classes per launch of hipie_sem_pan (register budget of its accumulators); more are tiled


def sem_pan_ok(n_queries, n_classes):
    return 0 < n_classes and 0 < n_queries <= 8192


@_timed("sem_pan")
def sem_pan(masks_lo, cls_all, pscore, up, crop_hw, out_hw, precision=0):
    """fused semantic + panoptic maps of one image.  masks_lo (N,hm,wm) f32 stride-`up` logits, cls_all (N,C) f32 class
    probabilities, pscore (N) f32 (score of kept queries, <= 0 otherwise) ->
    sem (C,oh,ow) f32, pan_idx (oh,ow) int32 (-1: no kept query), pan_own (oh,ow) bool, area (N) int32.
    More than SEM_PAN_CLASSES classes (ADE-847, LVIS-1203: BASELINE configs[3]/[4]) run as class tiles of one launch each;
    the panoptic outputs do not depend on the classes and are taken from the first tile."""
    N, C = cls_all.shape
    _, hm, wm = masks_lo.shape
    dev = masks_lo.device
    _on_device("sem_pan", "masks_lo cls_all pscore", masks_lo, cls_all, pscore)
    npad = (N + 15) // 16 * 16
    ps = torch.full((npad,), -1.0, dtype=torch.float32, device=dev)
    ps[:N] = pscore
    oh, ow = int(out_hw[0]), int(out_hw[1])
    sem = torch.empty(C, oh, ow, dtype=torch.float32, device=dev)
    pan_idx = torch.empty(oh, ow, dtype=torch.int32, device=dev)
    pan_own = torch.empty(oh, ow, dtype=torch.uint8, device=dev)
    area = torch.zeros(npad, dtype=torch.int32, device=dev)
    masks_ptr = _layout("sem_pan", "masks_lo", masks_lo, torch.float32).data_ptr()
    spare = None
    for c0 in range(0, C, SEM_PAN_CLASSES):
        cn = min(SEM_PAN_CLASSES, C - c0)
        cp = 32 if cn <= 32 else 96 if cn <= 96 else 160
        cls_t = torch.zeros(cp, npad, dtype=torch.float32, device=dev)
        cls_t[:cn, :N] = cls_all[:, c0:c0 + cn].t()
        hi = cls_t.to(torch.bfloat16)
        lo = (cls_t - hi.float()).to(torch.bfloat16) if precision == 0 else None
        if c0 == 0:
            outs = (pan_idx, pan_own, area)
        else:
            if spare is None:
                spare = (torch.empty_like(pan_idx), torch.empty_like(pan_own), torch.zeros_like(area))
            outs = spare
        _call("hipie_sem_pan", masks_ptr, hi.data_ptr(), _ptr(lo),
              ps.data_ptr(), sem[c0:c0 + cn].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
              N, npad, cn, hm, wm, int(up), int(crop_hw[0]), int(crop_hw[1]), oh, ow, int(precision))
    return sem, pan_idx, pan_own.bool(), area[:N]


_DIM_T = {}


def _sine_operands(ref, num_pos_feats, temperature):
    """(ref as fp32 rows, their stride, the cached frequency table) of the two sine-embedding ops"""
    nc = ref.shape[-1]
    ref = ref.float()
    rs = nc
    if ref.dim() == 3 and ref.stride(-1) == 1 and ref.stride(0) == ref.shape[1] * ref.stride(1) and ref.stride(1) >= nc:
        rs = ref.stride(1)                    # a row-strided view such as ref_in[:, :, 0, :]: read in place
    elif not ref.is_contiguous():
        ref = ref.contiguous()
    key = (num_pos_feats, temperature, str(ref.device))
    dim_t = _DIM_T.get(key)
    if dim_t is None:
        d = torch.arange(num_pos_feats, dtype=torch.float32, device=ref.device)
        dim_t = (temperature ** (2 * torch.div(d, 2, rounding_mode="floor") / num_pos_feats)).contiguous()
        _DIM_T[key] = dim_t
    return ref, rs, dim_t


@_timed("sine_embed")
def sine_embed(ref, num_pos_feats=128, temperature=10000, out_dtype=torch.float32):
    """get_sine_pos_embed(ref, exchange_xy=True): ref (..., 2|4) f32 (last-dim stride 1) -> (..., ncoord * num_pos_feats)."""
    import math
    nc = ref.shape[-1]
    _on_device("sine_embed", "ref", ref)
    ref, rs, dim_t = _sine_operands(ref, num_pos_feats, temperature)
    n = ref.numel() // nc
    out = torch.empty(ref.shape[:-1] + (nc * num_pos_feats,), dtype=out_dtype, device=ref.device)
    _call("hipie_sine_embed", ref.data_ptr(), dim_t.data_ptr(), out.data_ptr(), n, nc, num_pos_feats, rs, 2 * math.pi, _DT[out_dtype])
    return out


def _transposed(mod_layers, dtype=None):
    """(in, out) copies of the Linear weights of a small MLP head + its biases, cached on the first layer (derived)."""
    return derived(mod_layers[0], "wt", [p for l in mod_layers for p in (l.weight, l.bias)],
                   lambda: [(l.weight.t().contiguous(), l.bias.contiguous()) for l in mod_layers])


def ref_point_mlp_ok(ref, head):
    ls = getattr(head, "layers", None)
    return (ls is not None and len(ls) == 2 and ref.is_cuda and ref.shape[-1] == 4 and tuple(ls[0].weight.shape) == (256, 512)
            and tuple(ls[1].weight.shape) == (256, 256) and ls[0].weight.dtype == ls[1].weight.dtype and ls[0].weight.dtype in _DT)


@_timed("ref_point_mlp")
def ref_point_mlp(ref, head, num_pos_feats=128, temperature=10000):
    """query_pos = head(get_sine_pos_embed(ref)) in one launch: ref (B, Q, 4) f32 (row-strided view allowed), head = the
    2-layer ref_point_head (512 -> 256 -> 256) -> (B, Q, 256) in the head's weight dtype."""
    import math
    _on_device("ref_point_mlp", "ref weight", ref, head.layers[0].weight)
    ref, rs, dim_t = _sine_operands(ref, num_pos_feats, temperature)
    (w1t, b1), (w2t, b2) = _transposed(list(head.layers))
    dt = w1t.dtype
    n = ref.numel() // 4
    out = torch.empty(ref.shape[:-1] + (256,), dtype=dt, device=ref.device)
    _call("hipie_ref_point_mlp", ref.data_ptr(), dim_t.data_ptr(), w1t.data_ptr(), b1.data_ptr(), w2t.data_ptr(), b2.data_ptr(),
          out.data_ptr(), n, rs, 2 * math.pi, _DT[dt])
    return out


def box_head_ok(x, mlp):
    ls = getattr(mlp, "layers", None)
    return (ls is not None and len(ls) == 3 and x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == 256
            and [tuple(l.weight.shape) for l in ls] == [(256, 256), (256, 256), (4, 256)]
            and all(l.weight.dtype == torch.float32 for l in ls))


@_timed("box_head")
def box_head(x, ref, mlp, eps=1e-5):
    """sigmoid(mlp(x) + inverse_sigmoid(ref)) in one launch: x (..., 256) f32, ref (..., 4) f32, mlp = MLP(256, 256, 4, 3) f32."""
    _on_device("box_head", "x ref weight", x, ref, mlp.layers[0].weight)
    x, ref = _layout("box_head", "x", x, torch.float32, density=_ANY).contiguous(), ref.float().contiguous()
    (w1t, b1), (w2t, b2), (w3t, b3) = _transposed(list(mlp.layers))
    out = torch.empty_like(ref)
    _call("hipie_box_head", x.data_ptr(), ref.data_ptr(), w1t.data_ptr(), b1.data_ptr(), w2t.data_ptr(),
          b2.data_ptr(), w3t.data_ptr(), b3.data_ptr(), out.data_ptr(), ref.numel() // 4, float(eps))
    return out


@_timed("box_refine")
def box_refine(delta, ref, eps=1e-5):
    """sigmoid(delta + inverse_sigmoid(ref)): delta (..., 4) f32|f16|bf16, ref (..., 4) f32 -> (..., 4) f32."""
    _on_device("box_refine", "delta ref", delta, ref)
    delta, ref = delta.contiguous(), ref.float().contiguous()
    out = torch.empty_like(ref)
    _call("hipie_box_refine", delta.data_ptr(), ref.data_ptr(), out.data_ptr(), ref.numel(), float(eps), _DT[delta.dtype])
    return out


def selftest(which, a, b=None):
    _on_device("selftest", "a b", a, b)
    out = torch.empty(32 * 32 if which == 0 else 256, dtype=torch.float32, device=a.device)
    _call("hipie_selftest", which, a.data_ptr(), _ptr(b), out.data_ptr())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hipie_gemm: the linears on the hand-written MFMA GEMM.  HL8 ("split fp16") tensors are plain fp16 torch tensors whose last
# dimension is 2K: K/8 groups of [8 hi | 8 lo] (include/hipie_mi355.h HIPIE_HL8).
def hl8_pack(x, scale=1.0):
    """(..., K) float tensor -> (..., 2K) fp16 in HL8 layout, written with torch ops (weights, once per checkpoint; tests)."""
    K = x.shape[-1]
    assert K % 8 == 0
    xs = (x.float() * scale).clamp(-65504.0, 65504.0)      # saturate like the kernels' hl_split (no inf hi / NaN lo)
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return torch.stack([hi.reshape(*x.shape[:-1], K // 8, 8), lo.reshape(*x.shape[:-1], K // 8, 8)], dim=-2).reshape(*x.shape[:-1], 2 * K).contiguous()


def hl8_unpack(x):
    """(..., 2K) fp16 HL8 -> (..., K) fp32 (hi + lo)."""
    K2 = x.shape[-1]
    g = x.reshape(*x.shape[:-1], K2 // 16, 2, 8).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(*x.shape[:-1], K2 // 2)


@_timed("to_hl8")
def to_hl8(x, scale=1.0):
    """(rows..., K) fp32 | fp16 device tensor (last dim contiguous, uniform row stride) -> (rows..., 2K) fp16 HL8 (hipie_to_hl8)."""
    K = x.shape[-1]
    _on_device("to_hl8", "x", x)
    x2 = x.reshape(-1, K)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    out = torch.empty(*x.shape[:-1], 2 * K, dtype=torch.float16, device=x.device)
    _call("hipie_to_hl8", x2.data_ptr(), x2.stride(0), out.data_ptr(), 2 * K, x2.shape[0], K, _DT[x.dtype], float(scale))
    return out


@_timed("to_hl8_t")
def to_hl8_t(x, pad_to=32, scale=1.0):
    """(M, C) fp32 device tensor (last dim contiguous, any row stride) -> (C, 2 Mp) fp16 HL8 of x^T, Mp = M rounded up to `pad_to`, the padding
    columns zero (hipie_to_hl8_t): a split operand whose K runs over the rows of x."""
    _layout("to_hl8_t", "x", x, torch.float32, ndim=2, density=_ANY)
    _on_device("to_hl8_t", "x", x)
    if x.stride(1) != 1:
        x = x.contiguous()
    M, C = x.shape
    Mp = -(-M // pad_to) * pad_to
    out = torch.empty(C, 2 * Mp, dtype=torch.float16, device=x.device)
    _call("hipie_to_hl8_t", x.data_ptr(), x.stride(0), out.data_ptr(), 2 * Mp, M, C, Mp, float(scale))
    return out


def f16_pair(x, cols=None, scale=None):
    """fp32 (.., C) -> the two contiguous fp16 planes (hi = fp16(s x), lo = fp16(s x - hi)) of the fused training attention's operands, the
    last dimension zero-padded to `cols` (a multiple of 8); s = `scale`, a one-element DEVICE tensor (no host wait), or 1; values beyond the
    fp16 range saturate (hl_split).  One pass on the device (hipie_to_f16_pair)."""
    C = x.shape[-1]
    Cp = C if cols is None else max(cols, C)
    if x.dtype != torch.float32 or Cp % 8:
        raise RuntimeError("f16_pair: an fp32 device tensor and a column count that is a multiple of 8 (got %s %s on %s, %d columns)"
                           % (x.dtype, tuple(x.shape), x.device, Cp))
    _on_device("f16_pair", "x scale", x, scale)
    x2 = x.reshape(-1, C)
    if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < C):
        x2 = x2.contiguous()
    hi, lo = _f16_planes(x.shape[:-1] + (Cp,), x.device)
    sc = 0 if scale is None else scale.float().reshape(1).data_ptr()
    _call("hipie_to_f16_pair", x2.data_ptr(), x2.stride(0) if x2.shape[0] > 1 else C, hi.data_ptr(), lo.data_ptr(), x2.shape[0], C, Cp, sc)
    return hi, lo


# the two instances of the fused training attention (csrc/attn_train_tile.h): (entry-point stem, operand columns, rule on N, its wording)
_ATTN_TRAIN = ("attn_train", 224, lambda N: N >= 128 and N % 128 == 0, "N % 128 == 0")
_ATTN_TRAIN_WIN = ("attn_train_win", 128, lambda N: 1 <= N <= 256, "1 <= N <= 256")


def _attn_train_operands(who, inst, names, pairs, widths):
    """the checks both directions share: every plane (`names`: the pairs', whose planes are NAME_hi / NAME_lo) a contiguous fp16 device
    tensor, lo planes shaped like their hi planes, q' / k' (BH, N, cols) with N as the instance takes it, the remaining pairs
    (BH, N, widths[i]) -> (the planes in entry order, BH, N)"""
    _, cols, n_ok, rule = inst
    planes = [t for pair in pairs for t in pair]
    plane_names = [n + half for n in names.split() for half in ("_hi", "_lo")]
    _on_device(who, " ".join(plane_names), *planes)
    for n, t in zip(plane_names, planes):
        _layout(who, n, t, torch.float16)
    qh, kh = pairs[0][0], pairs[1][0]
    if qh.dim() != 3 or qh.shape[-1] != cols or kh.shape != qh.shape or not n_ok(qh.shape[1]) or qh.shape[0] < 1 \
            or any(lo.shape != hi.shape for hi, lo in pairs) \
            or any(tuple(pair[0].shape) != (qh.shape[0], qh.shape[1], w) for pair, w in zip(pairs[2:], widths)):
        raise RuntimeError("%s: q', k' (BH, N, %d) and %s pairs with %s, got %s"
                           % (who, cols, " / ".join("(BH, N, %d)" % w for w in widths), rule, " / ".join(str(tuple(pair[0].shape)) for pair in pairs)))
    return planes, qh.shape[0], qh.shape[1]


def _attn_train_forward(inst, q_pair, k_pair, v_pair):
    who = inst[0] + "_forward"
    planes, BH, N = _attn_train_operands(who, inst, "q k v", (q_pair, k_pair, v_pair), (80,))
    out = torch.empty(BH, N, 80, dtype=torch.float32, device=planes[0].device)
    lse = torch.empty(BH, N, dtype=torch.float32, device=planes[0].device)
    _call("hipie_" + who, *[t.data_ptr() for t in planes], out.data_ptr(), lse.data_ptr(), BH, N)
    return out, lse


def _attn_train_backward(inst, q_pair, k_pair, v96_pair, do96_pair, lse, delta):
    who = inst[0] + "_backward"
    planes, BH, N = _attn_train_operands(who, inst, "q k v96 do96", (q_pair, k_pair, v96_pair, do96_pair), (96, 96))
    if tuple(lse.shape) != (BH, N) or tuple(delta.shape) != (BH, N):
        raise RuntimeError("%s: lse / delta (BH, N) on the device" % who)
    _on_device(who, "lse delta", lse, delta)
    lse, delta = lse.float().contiguous(), delta.float().contiguous()
    dq = torch.empty(BH, N, inst[1], dtype=torch.float32, device=planes[0].device)
    dk = torch.empty(BH, N, 80, dtype=torch.float32, device=planes[0].device)
    dv = torch.empty(BH, N, 80, dtype=torch.float32, device=planes[0].device)
    _call("hipie_" + who, *[t.data_ptr() for t in planes], lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), BH, N)
    return dq, dk, dv


@_timed("attn_train_fwd")
def attn_train_forward(q_pair, k_pair, v_pair):
    """hipie_attn_train_forward: q', k' (BH, N, 224) and v (BH, N, 80) as fp16 pairs (f16_pair) -> (out (BH, N, 80) f32, lse (BH, N) f32)"""
    return _attn_train_forward(_ATTN_TRAIN, q_pair, k_pair, v_pair)


@_timed("attn_train_bwd")
def attn_train_backward(q_pair, k_pair, v96_pair, do96_pair, lse, delta):
    """hipie_attn_train_backward: the forward's q', k' pairs, v and dO as (BH, N, 96) pairs (f16_pair(.., 96); dO scaled into fp16's range by the
    caller), lse, delta = rowsum(dO * out) -> (dq' (BH, N, 224), dk (BH, N, 80), dv (BH, N, 80)) fp32, in the scale of the dO given"""
    return _attn_train_backward(_ATTN_TRAIN, q_pair, k_pair, v96_pair, do96_pair, lse, delta)


@_timed("attn_train_win_fwd")
def attn_train_win_forward(q_pair, k_pair, v_pair):
    """hipie_attn_train_win_forward (the windowed blocks: one (window, head) item of N <= 256 tokens per workgroup, no row padding): q', k'
    (BH, N, 128) and v (BH, N, 80) as fp16 pairs (f16_pair) -> (out (BH, N, 80) f32, lse (BH, N) f32)"""
    return _attn_train_forward(_ATTN_TRAIN_WIN, q_pair, k_pair, v_pair)


@_timed("attn_train_win_bwd")
def attn_train_win_backward(q_pair, k_pair, v96_pair, do96_pair, lse, delta):
    """hipie_attn_train_win_backward: the forward's q', k' pairs, v and dO as (BH, N, 96) pairs (f16_pair(.., 96); dO scaled into fp16's range by
    the caller), lse, delta = rowsum(dO * out) -> (dq' (BH, N, 128), dk (BH, N, 80), dv (BH, N, 80)) fp32, in the scale of the dO given"""
    return _attn_train_backward(_ATTN_TRAIN_WIN, q_pair, k_pair, v96_pair, do96_pair, lse, delta)


# ---- the pack / unpack passes around them (csrc/attn_pack.hip): the attention of a ViT block as one node, functions.VitAttentionFunction
ATTN_PACK_HD = 80


def attn_pack_rows(N, padded):
    """rows per (image, head) item in the planes: N, or N rounded up to 128 (the padded form of functions.fused_attention)"""
    return -(-N // 128) * 128 if padded else N


@_timed("attn_pack_kv")
def attn_pack_kv(qkv, heads, H, W, cols, padded=False):
    """hipie_attn_pack_kv: qkv (B', H W, 3 heads 80) fp32 rows of the qkv linear -> (rq (B' heads, N, 80) fp32: the head-major q,
    the k' pair (B' heads, Np, cols): [k | onehot(n // W) | onehot(n % W) | 0..], the v pair (B' heads, Np, 80)); cols 224 | 128;
    padded: Np = N rounded up to 128, the padding rows zero but for k' column 80 + H + W = -30000 (else Np = N)"""
    who = "attn_pack_kv"
    _on_device(who, "qkv", qkv)
    N = H * W
    if qkv.dim() != 3 or qkv.shape[1] != N or qkv.shape[2] != 3 * heads * ATTN_PACK_HD:
        raise RuntimeError("%s: qkv (B', %d, %d), got %s" % (who, N, 3 * heads * ATTN_PACK_HD, tuple(qkv.shape)))
    B = qkv.shape[0]
    _layout(who, "qkv", qkv, torch.float32)
    Np, dev = attn_pack_rows(N, padded), qkv.device
    rq = torch.empty(B * heads, N, ATTN_PACK_HD, dtype=torch.float32, device=dev)
    k, v = _f16_planes((B * heads, Np, cols), dev), _f16_planes((B * heads, Np, ATTN_PACK_HD), dev)
    _call("hipie_attn_pack_kv", qkv.data_ptr(), rq.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), B, heads,
          H, W, Np, cols)
    return rq, k, v


def _attn_pack_strides(who, name, t, shape):
    """element strides of a (BH, H, W, K) view, or of a (BH, N, K) one whose rows n = h W + w have one stride"""
    if t.dim() == 3 and tuple(t.shape) == (shape[0], shape[1] * shape[2], shape[3]):
        return (t.stride(0), t.stride(1) * shape[2], t.stride(1), t.stride(2))
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s: %s must be %s or (BH, N, K), got %s" % (who, name, tuple(shape), tuple(t.shape)))
    return tuple(t.stride())


@_timed("attn_pack_q")
def attn_pack_q(rq, rel_h, rel_w, heads, H, W, cols, padded=False):
    """hipie_attn_pack_q: rq (BH, H W, 80) of attn_pack_kv, rel_h (BH, H, W, H) and rel_w (BH, H, W, W) fp32 -- ANY strided views (also
    (BH, N, K)): the element strides go to the kernel, nothing is copied -> the q' pair (BH, Np, cols): [rq * 80^-0.5 | rel_h | rel_w | 0..],
    in the padded form column 80 + H + W = 1 on the real rows and the padding rows zero"""
    who = "attn_pack_q"
    _on_device(who, "rq rel_h rel_w", rq, rel_h, rel_w)
    N = H * W
    BH = rq.shape[0]
    _layout(who, "rq", rq, torch.float32, (BH, N, ATTN_PACK_HD))
    if rel_h.dtype is not torch.float32 or rel_w.dtype is not torch.float32:          # any strides: only the dtype is refused
        _layout(who, "rel_h", rel_h, torch.float32, None, None, _ANY)
        _layout(who, "rel_w", rel_w, torch.float32, None, None, _ANY)
    if BH % heads:
        raise RuntimeError("%s: %d items are no multiple of %d heads" % (who, BH, heads))
    sh, sw = _attn_pack_strides(who, "rel_h", rel_h, (BH, H, W, H)), _attn_pack_strides(who, "rel_w", rel_w, (BH, H, W, W))
    Np = attn_pack_rows(N, padded)
    q = _f16_planes((BH, Np, cols), rq.device)
    _call("hipie_attn_pack_q", rq.data_ptr(), rel_h.data_ptr(), *sh, rel_w.data_ptr(), *sw, q[0].data_ptr(), q[1].data_ptr(), BH // heads, heads,
          H, W, Np, cols, ATTN_PACK_HD ** -0.5)
    return q


@_timed("attn_grad_amax")
def attn_grad_amax(go):
    """hipie_attn_grad_amax: max |go| of a dense fp32 device tensor (a multiple of 4 elements) as a one-element device tensor -- the bits of
    go.abs().amax(), no host wait"""
    _on_device("attn_grad_amax", "go", go)
    _layout("attn_grad_amax", "go", go, torch.float32)
    amax = torch.empty(1, dtype=torch.float32, device=go.device)
    _call("hipie_attn_grad_amax", go.data_ptr(), go.numel(), amax.data_ptr())
    return amax


@_timed("attn_pack_grad")
def attn_pack_grad(go, out, v_pair, scale, heads, H, W):
    """hipie_attn_pack_grad: go (B', H W, heads 80) fp32 token-major, out (BH, Np, 80) fp32 and the 80-wide v pair (BH, Np, 80) of the forward,
    scale a one-element device tensor -> (the dO pair (BH, Np, 96) of scale * go, the v pair (BH, Np, 96), delta (BH, Np) fp32 =
    scale * sum_c go * out); rows >= N zero"""
    who = "attn_pack_grad"
    _on_device(who, "go out scale v_hi v_lo", go, out, scale, v_pair[0], v_pair[1])
    N = H * W
    if go.dim() != 3 or go.shape[1] != N or go.shape[2] != heads * ATTN_PACK_HD:
        raise RuntimeError("%s: go (B', %d, %d), got %s" % (who, N, heads * ATTN_PACK_HD, tuple(go.shape)))
    B = go.shape[0]
    BH, Np = B * heads, out.shape[1] if out.dim() == 3 else -1
    _layout(who, "go", go, torch.float32)
    _layout(who, "out", out, torch.float32, (BH, Np, ATTN_PACK_HD))
    _layout(who, "v_hi", v_pair[0], torch.float16, (BH, Np, ATTN_PACK_HD))
    _layout(who, "v_lo", v_pair[1], torch.float16, (BH, Np, ATTN_PACK_HD))
    _layout(who, "scale", scale, torch.float32, density=_ANY)
    if scale.numel() != 1:
        raise RuntimeError("%s: scale must have one element" % who)
    dev = go.device
    do, v96 = _f16_planes((BH, Np, 96), dev), _f16_planes((BH, Np, 96), dev)
    delta = torch.empty(BH, Np, dtype=torch.float32, device=dev)
    _call("hipie_attn_pack_grad", go.data_ptr(), out.data_ptr(), v_pair[0].data_ptr(), v_pair[1].data_ptr(), scale.data_ptr(), do[0].data_ptr(), do[1].data_ptr(),
          v96[0].data_ptr(), v96[1].data_ptr(), delta.data_ptr(), B, heads, H, W, Np)
    return do, v96, delta


@_timed("attn_unpack_grad")
def attn_unpack_grad(dq, dk, dv, dq_h, dq_w, inv, heads, H, W):
    """hipie_attn_unpack_grad: dq' (BH, Np, cols), dk, dv (BH, Np, 80) fp32 of the backward op; dq_h, dq_w (dq_w may be None): the rel-pos
    terms of dq as (BH, H, W, 80) fp32 views with ANY strides that are multiples of 4 in front of the 80 contiguous columns; inv a one-element
    device tensor -> dqkv (B', H W, 3 heads 80) fp32: q = (dq'[..., :80] * 80^-0.5 + dq_h + dq_w) * inv, k = dk * inv, v = dv * inv"""
    who = "attn_unpack_grad"
    _on_device(who, "dq dk dv dq_h dq_w inv", dq, dk, dv, dq_h, dq_w, inv)
    N = H * W
    if dq.dim() != 3 or dq.shape[0] % heads:
        raise RuntimeError("%s: dq' (BH, Np, cols), got %s" % (who, tuple(dq.shape)))
    BH, Np, cols = dq.shape
    _layout(who, "dq", dq, torch.float32)
    _layout(who, "dk", dk, torch.float32, (BH, Np, ATTN_PACK_HD))
    _layout(who, "dv", dv, torch.float32, (BH, Np, ATTN_PACK_HD))
    strides = []
    for name, t in (("dq_h", dq_h), ("dq_w", dq_w)):
        if t is None:
            strides.append((0, 0, 0))
            continue
        _layout(who, name, t, torch.float32, (BH, H, W, ATTN_PACK_HD), density=_ROWS)
        strides.append(tuple(t.stride()[:3]))
    _layout(who, "inv", inv, torch.float32, density=_ANY)
    if inv.numel() != 1:
        raise RuntimeError("%s: inv must have one element" % who)
    dqkv = torch.empty(BH // heads, N, 3 * heads * ATTN_PACK_HD, dtype=torch.float32, device=dq.device)
    _call("hipie_attn_unpack_grad", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dq_h.data_ptr(), *strides[0], _ptr(dq_w), *strides[1],
          inv.data_ptr(), dqkv.data_ptr(), BH // heads, heads, H, W, Np, cols, ATTN_PACK_HD ** -0.5)
    return dqkv


@_timed("fill_rows")
def fill_rows(dst, rows, src_row):
    """dst[rows[i]] = src_row for every i (hipie_fill_rows): dst (R, W) contiguous device tensor, rows int32 (n,), src_row (W,) of dst's
    dtype; row bytes a multiple of 16.  In place; returns dst."""
    if dst.dim() != 2 or src_row.dtype != dst.dtype or src_row.numel() != dst.shape[1]:
        raise RuntimeError("fill_rows: dst (R, W) on the device, src_row (W,) of the same dtype")
    _on_device("fill_rows", "dst rows src_row", dst, rows, src_row)
    _layout("fill_rows", "dst", dst)
    _layout("fill_rows", "rows", rows, torch.int32)
    _layout("fill_rows", "src_row", src_row)
    _call("hipie_fill_rows", dst.data_ptr(), dst.stride(0) * dst.element_size(), rows.data_ptr(), rows.numel(), src_row.data_ptr(),
          dst.shape[1] * dst.element_size())
    return dst


ACT_NONE, ACT_GELU, ACT_RELU, ACT_QGELU = 0, 1, 2, 3


def _gemm_tag(a, w, *args, **kw):
    tag = kw.get("tag", "gemm")
    if PROFILE.shapes and tag == "gemm":
        split = kw.get("split")
        K = w.shape[1] // 2 if split else w.shape[1]
        tag = "gemm M%d N%d K%d %s->%s%s" % (a.numel() // a.shape[-1], w.shape[0], K, "f32" if a.dtype == torch.float32 else ("hl8" if split else "f16"),
                                          {F32: "f32", F16: "f16", HL8: "hl8"}.get(kw.get("out_fmt", F32), "?"), " +res" if kw.get("resid") is not None else "")
    return tag


_NO_ALPHA_DEV = object()          # gemm's alpha_dev left out: hipie_gemm.  Given (a device tensor, or None for NULL): hipie_gemm_scaled


@_timed(_gemm_tag)
def gemm(a, w, bias=None, resid=None, out_fmt=F32, act=ACT_NONE, alpha=1.0, oscale=1.0, split=None, out=None, tag="gemm", out_row=None,
         out_rows=None, a_row=None, alpha_dev=_NO_ALPHA_DEV):
    """out = ((act(alpha * a . w^T + bias)) + resid) * oscale on hipie_gemm.
    a (..., K) fp16 and w (N, K) fp16 (one product), or both HL8: a (..., 2K), w (N, 2K) fp16 (three products, fp32-class);
    `split` tells which (default: inferred -- pass it when K is ambiguous).  With split=True a may also be PLAIN fp32 (..., K) rows
    (16-byte aligned): the kernel splits them after the LDS read -- no hipie_to_hl8 launch.  a may be a row-strided 2-d view.  bias (N) f32,
    resid (..., N) f32.  out_fmt F32 | F16 | HL8 -> (..., N) f32 / f16 or (..., 2N) fp16 HL8."""
    a_f32 = a.dtype == torch.float32 and bool(split)
    _on_device("gemm", "a w bias resid out out_row a_row alpha_dev", a, w, bias, resid, out, out_row, a_row, None if alpha_dev is _NO_ALPHA_DEV else alpha_dev)
    if (a.dtype != torch.float16 and not a_f32) or w.dtype != torch.float16:
        raise RuntimeError("gemm: operands must be fp16 (plain or HL8) device tensors (a may be fp32 against HL8 weights)")
    if split is None:
        raise RuntimeError("gemm: say split=True (HL8 operands) or split=False (plain fp16)")
    N = w.shape[0]
    Kw = w.shape[1] // 2 if split else w.shape[1]
    lead = a.shape[:-1]
    a2 = a if a.dim() == 2 else a.reshape(-1, a.shape[-1])
    if a2.stride(-1) != 1 or a2.shape[-1] != (Kw if a_f32 else w.shape[1]):
        raise RuntimeError("gemm: a rows must be contiguous and as long as w rows (%s vs %s)" % (tuple(a.shape), tuple(w.shape)))
    if a_f32 and (a2.stride(0) % 4 or a2.data_ptr() % 16):
        raise RuntimeError("gemm: fp32 a rows must be 16-byte aligned")
    M = a2.shape[0]
    if a_row is not None:            # gather: product row m reads operand row a_row[m] (hipie_gemm_gather); M = the map's length
        if a_row.dtype != torch.int32 or not a_row.is_contiguous() or not split:
            raise RuntimeError("gemm: a_row must be a contiguous int32 vector (split operands only)")
        M = a_row.numel()
        lead = (M,)
        if out is not None and out_row is None and out.numel() // out.shape[-1] < M:
            raise RuntimeError("gemm: `out` has fewer rows (%d) than the row map (%d)" % (out.numel() // out.shape[-1], M))
        if resid is not None and resid.numel() // N < M:
            raise RuntimeError("gemm: `resid` has fewer rows (%d) than the row map (%d)" % (resid.numel() // N, M))
    if out_row is not None:
        if out is None:
            lead = (int(out_rows),)
        if out_row.dtype != torch.int32 or out_row.numel() != M or not out_row.is_contiguous():
            raise RuntimeError("gemm: out_row must be a contiguous int32 vector with one entry per row of a")
    if out is None:
        if out_fmt == F32:
            out = torch.empty(*lead, N, dtype=torch.float32, device=a.device)
        elif out_fmt == F16:
            out = torch.empty(*lead, N, dtype=torch.float16, device=a.device)
        else:
            out = torch.empty(*lead, 2 * N, dtype=torch.float16, device=a.device)
    o2 = out if out.dim() == 2 else out.reshape(-1, out.shape[-1])
    r2 = _layout("gemm", "resid", None if resid is None else resid.reshape(-1, N), torch.float32, None, None, _ROWS)
    _layout("gemm", "bias", bias, torch.float32)
    _layout("gemm", "w", w)
    # one list for the three entries: the gather form adds the row map before w and has its own operand code (args[13]); scaled: alpha_dev
    args = [a2.data_ptr(), a2.stride(0), w.data_ptr(), w.shape[1], _ptr(bias), _ptr(r2), 0 if r2 is None else r2.stride(0), o2.data_ptr(),
            o2.stride(0), _ptr(out_row), M, N, Kw, F32 if a_f32 else (HL8 if split else F16), int(out_fmt), int(act), float(alpha), float(oscale)]
    if a_row is not None:
        _call("hipie_gemm_gather", *args[:2], a2.shape[0], a_row.data_ptr(), *args[2:13], F32 if a_f32 else HL8, *args[14:])
    elif alpha_dev is not _NO_ALPHA_DEV:
        _call("hipie_gemm_scaled", *args, _ptr(alpha_dev))
    else:
        _call("hipie_gemm", *args)
    return out


def _one_f32(who, alpha_dev):
    """the device scalar of the scaled products: one fp32 element (a view into a scale block of grad_scale), or None"""
    if alpha_dev is not None and (alpha_dev.dtype != torch.float32 or alpha_dev.numel() != 1):
        raise RuntimeError("%s: alpha_dev must be one torch.float32 element, got %s %s" % (who, alpha_dev.dtype, tuple(alpha_dev.shape)))


def gemm_scaled(a, w, alpha_dev, **kw):
    """gemm (hipie_gemm_scaled) whose alpha is multiplied by the DEVICE scalar alpha_dev (one fp32 element, e.g. grad_scale(dy)[1:]) in the
    kernel that writes the product: no host wait, no extra pass.  alpha_dev None: the NULL pointer, i.e. gemm's dispatch and bits.  The
    a_row (gather) form has no scaled entry."""
    _on_device("gemm_scaled", "a alpha_dev", a, alpha_dev)
    if kw.get("a_row") is not None:
        raise RuntimeError("gemm_scaled: the gather form (a_row) has no scaled entry")
    _one_f32("gemm_scaled", alpha_dev)
    return gemm(a, w, alpha_dev=alpha_dev, **kw)


@_timed(lambda qkv, tab_h, tab_w, grid_hw, heads: "vit_attn_global" if grid_hw[0] * grid_hw[1] > 256 else "vit_attn_window")
def vit_attn_split(qkv, tab_h, tab_w, grid_hw, heads):
    """hipie_vit_attn_split: qkv (B, gh*gw, 2 * 3*heads*hd) fp16 HL8 rows (q pre-scaled by scale*log2 e), tab_h (2*gh-1, 2*hd),
    tab_w (2*gw-1, 2*hd) HL8 (tables / scale) -> (B, N, 2 * heads*hd) HL8."""
    gh, gw = grid_hw
    if qkv.dtype != torch.float16:
        raise RuntimeError("vit_attn_split: HL8 (fp16) operands expected")
    B, N, hd = _vit_operands("vit_attn_split", qkv, tab_h, tab_w, torch.float16, heads, 6)
    out = torch.empty(B, N, 2 * heads * hd, dtype=torch.float16, device=qkv.device)
    _call("hipie_vit_attn_split", qkv.data_ptr(), tab_h.data_ptr(), tab_w.data_ptr(), out.data_ptr(), B, gh, gw, heads, hd)
    return out


def _split_k_parts(who, a_hl8, w_hl8, nk):
    """the front both split-k products share: what hipie_gemm_batched needs of the operands, then its ONE launch over the nk chunks of
    the contraction -> the partial products (nk, M, N) fp32"""
    _on_device(who, "a_hl8 w_hl8", a_hl8, w_hl8)
    _layout(who, "a_hl8", a_hl8, torch.float16, ndim=2, align16=True)
    _layout(who, "w_hl8", w_hl8, torch.float16, ndim=2, align16=True)
    M, K2 = a_hl8.shape
    N = w_hl8.shape[0]
    K = K2 // 2
    if w_hl8.shape[1] != K2 or nk < 1 or nk > 64 or K % (32 * nk):
        raise RuntimeError("%s: HL8 operands (M, 2K) / (N, 2K), K a multiple of 32 * nk, nk <= 64" % who)
    if N % 8:
        raise RuntimeError("%s: N must be a multiple of 8" % who)
    Kc = K // nk
    part = torch.empty(nk, M, N, dtype=torch.float32, device=a_hl8.device)
    _call("hipie_gemm_batched", a_hl8.data_ptr(), K2, 0, 2 * Kc, w_hl8.data_ptr(), K2, 0, 2 * Kc, part.data_ptr(), N, 0, M * N, 1, nk, M, N, Kc,
          F32, 1.0)
    return part


@_timed("gemm_split_k")
def gemm_split_k(a_hl8, w_hl8, nk):
    """a . w^T for HL8 operands a (M, 2K), w (N, 2K) with the contraction cut into nk chunks (K / nk a multiple of 32): one problem per
    chunk in ONE hipie_gemm_batched launch, partial products summed -> (M, N) fp32.  For products whose M x N is a few tiles and whose K is
    long (the weight gradients of the training step)."""
    return _split_k_parts("gemm_split_k", a_hl8, w_hl8, nk).sum(0)


@_timed("gemm_split_k")
def gemm_split_k_scaled(a_hl8, w_hl8, nk, alpha_dev):
    """gemm_split_k whose partial products are added in chunk order and multiplied by the device scalar alpha_dev (None: 1) in ONE pass
    (hipie_splitk_finish) instead of part.sum(0): the weight gradient of the scaled-gradient nodes.  M * N a multiple of 4."""
    who = "gemm_split_k_scaled"
    _on_device(who, "alpha_dev", alpha_dev)          # a_hl8 and w_hl8: _split_k_parts
    _one_f32(who, alpha_dev)
    part = _split_k_parts(who, a_hl8, w_hl8, nk)
    out = torch.empty(part.shape[1], part.shape[2], dtype=torch.float32, device=a_hl8.device)
    _call("hipie_splitk_finish", part.data_ptr(), part.shape[0], out.numel(), _ptr(alpha_dev), out.data_ptr())
    return out


def _grad_rows(who, dy):
    """the row stride of dy as the kernels of csrc/grad_pack.hip take it: 2-D fp32 on the device, contiguous rows that do not overlap, row
    stride a multiple of 4, 16-byte aligned"""
    _on_device(who, "dy", dy)
    if dy.dim() != 2 or dy.shape[0] == 0 or dy.shape[1] == 0:
        raise RuntimeError("%s: dy must be a non-empty 2-D tensor, got %s" % (who, tuple(dy.shape)))
    rows, n = dy.shape
    ld = dy.stride(0) if rows > 1 else n
    if dy.dtype is not torch.float32 or dy.stride(1) != 1 or (rows > 1 and (ld % 4 or ld < n)) or dy.data_ptr() % 16:
        _layout(who, "dy", dy, torch.float32, None, None, _ROWS, 4, True)          # the vocabulary's message; what it lets pass overlaps
        raise RuntimeError("%s: dy rows overlap, got strides %s" % (who, tuple(dy.stride())))
    return ld


@_timed("grad_scale")
def grad_scale(dy):
    """hipie_grad_scale: dy (rows, N) fp32 device rows (N % 4 == 0; any row stride that is a multiple of 4) -> the device block {s, 1 / s},
    a (2,) fp32 tensor: s = 2^e with max|dy| * 2^e in [2^14, 2^15), {1, 1} for an all-zero or non-finite dy.  No host wait."""
    ldx = _grad_rows("grad_scale", dy)
    if dy.shape[1] % 4:
        raise RuntimeError("grad_scale: N=%d must be a multiple of 4" % dy.shape[1])
    block = torch.empty(2, dtype=torch.float32, device=dy.device)
    _call("hipie_grad_scale", dy.data_ptr(), ldx, dy.shape[0], dy.shape[1], block.data_ptr())
    return block


@_timed("grad_pack")
def grad_pack(dy, scale, want_rows=True, want_t=True, want_bias=False, rows_p=None):
    """hipie_grad_pack: ONE pass over dy (rows, N) fp32 with the device block `scale` = {s, 1 / s} of grad_scale ->
    (the HL8 rows of s dy, (rows, 2N) fp16 | None,  the HL8 rows of (s dy)^T, (N, 2 rows_p) fp16 with zero pad columns | None,
     db = dy.sum(0) of the UNSCALED values, (N,) fp32, summed in a fixed order | None).  N % 8 == 0; rows_p (default: rows rounded up to 32)
    a multiple of 32.  Everything is refused before a launch."""
    ldx = _grad_rows("grad_pack", dy)
    _on_device("grad_pack", "scale", scale)
    if scale.dtype != torch.float32 or scale.numel() != 2 or not scale.is_contiguous():
        raise RuntimeError("grad_pack: scale must be the contiguous {s, 1 / s} block of grad_scale (2 x torch.float32)")
    rows, N = dy.shape
    if N % 8:
        raise RuntimeError("grad_pack: N=%d must be a multiple of 8" % N)
    rows_p = -(-rows // 32) * 32 if rows_p is None else int(rows_p)
    if rows_p < rows or rows_p % 32:
        raise RuntimeError("grad_pack: rows_p=%d must be a multiple of 32 and at least rows=%d (rows_p %% 32)" % (rows_p, rows))
    out_r = torch.empty(rows, 2 * N, dtype=torch.float16, device=dy.device) if want_rows else None
    out_t = torch.empty(N, 2 * rows_p, dtype=torch.float16, device=dy.device) if want_t else None
    db = ws = None
    if want_bias:
        db = torch.empty(N, dtype=torch.float32, device=dy.device)
        ws = _workspace(None, _size("hipie_grad_pack_ws_bytes", rows_p, N), dy.device, "grad_pack")
    _call("hipie_grad_pack", dy.data_ptr(), ldx, scale.data_ptr(), _ptr(out_r), 2 * N, _ptr(out_t), 2 * rows_p, _ptr(db), _ptr(ws), rows, N, rows_p)
    return out_r, out_t, db


@_timed("gemm_batched")
def matmul_nt_batched(a, w, alpha=1.0):
    """out[b] = alpha * a[b] . w[b]^T at fp32-class accuracy on hipie_gemm_batched: a (B, M, K), w (B, N, K) fp32 device tensors,
    K % 32 == 0 -> (B, M, N) fp32.  The operands are split to HL8 on the way in; N is padded to a multiple of 8 with zero rows.  For the
    per-image products of the heads (class logits = queries . token embeddings^T, VL_Align: deformable_detr.py:55-73)."""
    B, M, K = a.shape
    N = w.shape[1]
    if w.shape[0] != B or w.shape[2] != K or K % 32:
        raise RuntimeError("matmul_nt_batched: a (B, M, K), w (B, N, K) device tensors with K %% 32 == 0, got %s / %s" % (tuple(a.shape), tuple(w.shape)))
    _on_device("matmul_nt_batched", "a w", a, w)
    Np = (N + 7) // 8 * 8
    if Np != N:
        wp = torch.zeros(B, Np, K, dtype=torch.float32, device=w.device)
        wp[:, :N] = w
        w = wp
    ah, wh = to_hl8(a.float().contiguous()), to_hl8(w.float().contiguous())
    out = torch.empty(B, M, Np, dtype=torch.float32, device=a.device)
    _call("hipie_gemm_batched", ah.data_ptr(), 2 * K, M * 2 * K, 0, wh.data_ptr(), 2 * K, Np * 2 * K, 0, out.data_ptr(), Np, M * Np, 0,
          B, 1, M, Np, K, F32, float(alpha))
    return out if Np == N else out[..., :N]


def vit_attn_split_ok(grid_hw, hd):
    """geometry hipie_vit_attn_split covers: head_dim 64 / 80, 14-wide windows, token grids up to 96 wide (64 x 64 at 1024^2, 84 x 84 at
    1344^2) and -- walked column by column -- grids wider than 96 whose height is <= 96 (64 x 128: a 1024 x 2048 image, the eval yamls'
    MAX_SIZE_TEST).  Only grids wider than 96 in BOTH directions (beyond 1536 x 1536 pixels) are not covered."""
    gh, gw = grid_hw

    def rows_ok(kh, kw):           # LDS: the per-key-row bias table of the <= 64-wide instances holds kh rows
        return (kw <= 32 and kh <= 160) or (kw <= 64 and kh <= 132) or (64 < kw <= 96 and kh <= 160)
    return hd in (64, 80) and ((gw == 14 and gh <= 96) or rows_ok(gh, gw) or (gw > 96 and gh <= 96 and rows_ok(gw, gh)))


# ---- split ("fp32-class") linears: cached HL8 copies of (derived) weights + the GEMM call ----------------------------------
def _padded_f32(weight_fn, bias_fn):
    """(weight (Np, K), bias (Np,) | None, N) in fp32 from weight_fn / bias_fn, N padded to a multiple of 8 with zero rows"""
    w = weight_fn().detach().float()
    b = None if bias_fn is None else bias_fn()
    b = None if b is None else b.detach().float()
    N = w.shape[0]
    Np = (N + 7) // 8 * 8
    if Np != N:
        w = torch.nn.functional.pad(w, (0, 0, 0, Np - N))
        b = None if b is None else torch.nn.functional.pad(b, (0, Np - N))
    return w, None if b is None else b.contiguous(), N


def split_weight(owner, key, params, weight_fn, bias_fn=None):
    """HL8 copy of a weight (N, K) -> ((Np, 2K) fp16, bias (Np,) f32 | None, N), N padded to a multiple of 8 with zero rows.
    Cached on ``owner`` under ``key`` and rebuilt when ``params`` change (derived): load_state_dict / .to() / in-place updates
    invalidate it.  weight_fn / bias_fn build the (possibly folded / concatenated) fp32 tensors."""
    def build():
        w, b, N = _padded_f32(weight_fn, bias_fn)
        return hl8_pack(w), b, N
    return derived(owner, ("hl8", key), params, build)


def conv3x3_split_ok(x, conv):
    """3 x 3, stride 1, padding 1, dense: the shapes hipie_conv3x3_split runs well (full 256-column tiles)"""
    return (x.is_cuda and x.dim() == 4 and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.padding_mode == "zeros" and conv.groups == 1 and conv.weight.dtype == torch.float32 and conv.in_channels % 32 == 0 and conv.out_channels % 256 == 0
            and x.shape[0] * (x.shape[2] + 2) * (x.shape[3] + 2) >= 16384)


_CONV_STAGE = {}
_RETIRED = []           # evicted cache entries stay alive: a captured hipGraph may still hold their addresses (as _Workspace.retired does)


@_timed("conv3x3_split")
def conv3x3_split(x, conv, act=ACT_NONE):
    """conv(x) for a 3 x 3 / stride 1 / padding 1 nn.Conv2d at the split policy's accuracy (hipie_conv3x3_split: implicit GEMM, K = 9 C).
    x (B, C, H, W) in any memory format -> (B, N, H, W) fp32 in channels-last memory.  The input is copied once onto a zero-padded pixel grid
    (with guard rows), the kernel computes on that grid and the interior is cropped."""
    B, C, H, W = x.shape
    _on_device("conv3x3_split", "x weight bias", x, conv.weight, conv.bias)
    N = conv.out_channels
    Hp, Wp = H + 2, W + 2
    guard = Wp + 1
    rows = B * Hp * Wp
    # the zero-padded staging grid is cached per (geometry, device, stream): its border and guard rows stay zero, only the interior is
    # re-written per call (one full-map zero-fill pass less per convolution)
    skey = (B, C, H, W, str(x.device), torch.cuda.current_stream(x.device).cuda_stream)
    buf = _CONV_STAGE.get(skey)
    if buf is None:
        if len(_CONV_STAGE) >= 8:
            _RETIRED.append(_CONV_STAGE.pop(next(iter(_CONV_STAGE))))
        buf = _CONV_STAGE[skey] = torch.zeros(rows + 2 * guard, C, dtype=torch.float32, device=x.device)
    buf[guard:guard + rows].view(B, Hp, Wp, C)[:, 1:-1, 1:-1].copy_(x.permute(0, 2, 3, 1))
    w, b, _ = split_weight(conv, "w3x3", [conv.weight] + ([conv.bias] if conv.bias is not None else []),
                           lambda: conv.weight.permute(0, 2, 3, 1).reshape(N, 9 * C), (lambda: conv.bias) if conv.bias is not None else None)
    out = torch.empty(rows, N, dtype=torch.float32, device=x.device)
    xin = buf[guard:]
    _call("hipie_conv3x3_split", xin.data_ptr(), C, w.data_ptr(), _ptr(b), out.data_ptr(), N, rows, Wp, C, N,
          F32, F32, int(act))
    return out.view(B, Hp, Wp, N)[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)


# ---- the training step's 3 x 3 convolution node on the same padded grid (training/functions.Conv3x3Function) ----------------------------
CONV_WGRAD_CHUNK = 2048         # grid rows per partial of hipie_conv3x3_wgrad (csrc/conv_wgrad.hip WG_CHUNK)


def conv3x3_stage(x):
    """x (B, C, H, W) fp32 in any memory format -> its zero-padded pixel grid in a buffer of ITS OWN, (rows + 2 guard, C) fp32: rows =
    B (H + 2) (W + 2) pixel rows with a zero border, guard = W + 3 zero rows on both ends.  Not the inference cache _CONV_STAGE (eight slots
    per stream, evicted): a training node's grid must outlive other convolutions of the step, so it is allocated per call and freed with
    its last reference."""
    B, C, H, W = x.shape
    Hp, Wp = H + 2, W + 2
    guard, rows = Wp + 1, B * Hp * Wp
    buf = torch.zeros(rows + 2 * guard, C, dtype=torch.float32, device=x.device)
    buf[guard:guard + rows].view(B, Hp, Wp, C)[:, 1:-1, 1:-1].copy_(x.permute(0, 2, 3, 1))
    return buf


def conv3x3_crop(grid_rows, B, H, W):
    """(B (H + 2) (W + 2), N) rows on the padded grid -> the (B, N, H, W) interior, a VIEW (channels-last strides inside the grid)"""
    return grid_rows.view(B, H + 2, W + 2, grid_rows.shape[1])[:, 1:-1, 1:-1].permute(0, 3, 1, 2)


@_timed("conv3x3_train")
def conv3x3_grid(buf, w_hl8, bias, B, H, W, relu=False):
    """hipie_conv3x3_split on a grid of conv3x3_stage, F32 rows in and F32 out: buf (rows + 2 guard, C), w_hl8 (N, 2 * 9 C) HL8 with
    k = (3 ky + kx) C + c, bias (N) fp32 or None -> (rows, N) fp32 on the SAME grid; its border rows are meaningless."""
    Wp = W + 2
    guard, rows = Wp + 1, B * (H + 2) * Wp
    C, N = buf.shape[1], w_hl8.shape[0]
    if buf.shape[0] != rows + 2 * guard or w_hl8.shape[1] != 18 * C or w_hl8.dtype != torch.float16 or buf.dtype != torch.float32:
        raise RuntimeError("conv3x3_grid: a staged grid %s against an HL8 weight %s" % (tuple(buf.shape), tuple(w_hl8.shape)))
    _on_device("conv3x3_grid", "buf w_hl8 bias", buf, w_hl8, bias)
    _layout("conv3x3_grid", "buf", buf)
    _layout("conv3x3_grid", "w_hl8", w_hl8)
    _layout("conv3x3_grid", "bias", bias, torch.float32)
    out = torch.empty(rows, N, dtype=torch.float32, device=buf.device)
    _call("hipie_conv3x3_split", buf.data_ptr() + 4 * guard * C, C, w_hl8.data_ptr(), _ptr(bias), out.data_ptr(), N, rows, Wp, C, N, F32, F32, ACT_RELU if relu else ACT_NONE)
    return out


@_timed("conv3x3_wgrad")
def conv3x3_wgrad(xbuf, dybuf, y_rows, B, H, W, want_bias=True):
    """weight and bias gradient of the 3 x 3 convolution on the padded grid (hipie_conv3x3_wgrad): xbuf (rows + 2 guard, C) and dybuf
    (rows + 2 guard, N) grids of conv3x3_stage (dybuf's border zero), y_rows (rows, N) the forward's output on the grid or None (with it
    the gradient is masked by y > 0 as it is read) -> (dw (N, 9, C) with tap = 3 ky + kx, db (N) | None).  The partial sums of the row
    chunks are added in chunk order: bit-reproducible.  The workspace lives for the call."""
    Wp = W + 2
    guard, rows = Wp + 1, B * (H + 2) * Wp
    C, N = xbuf.shape[1], dybuf.shape[1]
    if xbuf.shape[0] != rows + 2 * guard or dybuf.shape[0] != rows + 2 * guard or (y_rows is not None and tuple(y_rows.shape) != (rows, N)):
        raise RuntimeError("conv3x3_wgrad: grids %s / %s for %d rows" % (tuple(xbuf.shape), tuple(dybuf.shape), rows))
    who = "conv3x3_wgrad"
    _on_device(who, "xbuf dybuf y_rows", xbuf, dybuf, y_rows)
    _layout(who, "xbuf", xbuf, torch.float32)
    _layout(who, "dybuf", dybuf, torch.float32)
    _layout(who, "y_rows", y_rows, torch.float32)
    dw = torch.empty(N, 9, C, dtype=torch.float32, device=xbuf.device)
    db = torch.empty(N, dtype=torch.float32, device=xbuf.device) if want_bias else None
    ws_bytes = -(-rows // CONV_WGRAD_CHUNK) * (9 * C * N + N) * 4
    ws = _workspace(None, ws_bytes, xbuf.device, who)
    _call("hipie_conv3x3_wgrad", xbuf.data_ptr() + 4 * guard * C, C, dybuf.data_ptr() + 4 * guard * N, N, _ptr(y_rows), rows, Wp, C, N,
          dw.data_ptr(), _ptr(db), ws.data_ptr(), ws_bytes)
    return dw, db


_FFN_PERM = {}


def ffn_fused_ok(x_hl8, lin1, lin2):
    """the shape hipie_ffn_fused is built for: 256 -> 2048 -> 256 on at least a few thousand tokens (the two deformable encoders)"""
    return (x_hl8.is_cuda and lin1.weight.shape == (2048, 256) and lin2.weight.shape == (256, 2048) and lin1.bias is not None
            and lin2.bias is not None and lin1.weight.dtype == torch.float32 and x_hl8.numel() // 512 >= 4096)


@_timed("ffn_fused")
def ffn_fused(x_hl8, lin1, lin2):
    """linear2(relu(linear1(x))) in ONE launch at the split policy's accuracy (hipie_ffn_fused): x (..., 2*256) HL8 -> (..., 256) fp32.
    The hidden activations stay in registers; W2's columns are permuted once per parameter version into the order the MFMA C layout
    hands them over (rows 0-3, 8-11, 4-7, 12-15 of every 16)."""
    _on_device("ffn_fused", "x_hl8 weight1 weight2", x_hl8, lin1.weight, lin2.weight)
    w1, b1, _ = split_weight(lin1, "w", [lin1.weight, lin1.bias], lambda: lin1.weight, lambda: lin1.bias)
    F_ = lin2.weight.shape[1]
    perm = _FFN_PERM.get(F_)
    if perm is None:
        base = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])
        perm = _FFN_PERM[F_] = (torch.arange(0, F_, 16)[:, None] + base[None, :]).reshape(-1)
    w2, b2, _ = split_weight(lin2, "w_ffn_perm", [lin2.weight, lin2.bias], lambda: lin2.weight[:, perm.to(lin2.weight.device)], lambda: lin2.bias)
    lead = x_hl8.shape[:-1]
    x2 = x_hl8.reshape(-1, x_hl8.shape[-1])
    if x2.dtype != torch.float16 or x2.stride(-1) != 1 or x2.shape[-1] != 512:
        raise RuntimeError("ffn_fused: x must be HL8 rows of 2 * 256 fp16 values")
    M = x2.shape[0]
    out = torch.empty(M, 256, dtype=torch.float32, device=x2.device)
    _call("hipie_ffn_fused", x2.data_ptr(), x2.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(), 256,
          M, 256, F_)
    return out.view(*lead, 256)


def split_ok(K):
    return K % 32 == 0


def split_linear(x, owner, key, weight, bias=None, act=ACT_NONE, out_fmt=F32, resid=None, x_hl8=False, weight_fn=None, bias_fn=None,
                 tag="gemm", params=None, out=None, out_row=None, a_row=None):
    """F.linear(x, weight, bias) at fp32-class accuracy on hipie_gemm's split operands.  x fp32 / fp16 (converted with hipie_to_hl8)
    or already HL8 (x_hl8).  weight_fn / bias_fn: derived weights (folded constants, concatenations) built once per parameter version."""
    if params is None:
        params = [weight] + ([bias] if bias is not None else [])
    w, b, N = split_weight(owner, key, params, weight_fn or (lambda: weight), bias_fn or ((lambda: bias) if bias is not None else None))
    if x_hl8:
        a = x
    elif x.dtype == torch.float32 and x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and (x.dim() < 2 or x.stride(-2) % 4 == 0):
        a = x if x.dim() <= 2 or x.is_contiguous() else x.contiguous()      # fp32 rows: split inside the GEMM
    else:
        a = to_hl8(x if x.dtype in (torch.float32, torch.float16) else x.float())
    if out is not None or out_row is not None or a_row is not None:
        if N != w.shape[0]:
            raise RuntimeError("split_linear: in-place / row-mapped outputs need N % 8 == 0")
        return gemm(a, w, b, resid, out_fmt=out_fmt, act=act, split=True, tag=tag, out=out, out_row=out_row, a_row=a_row)
    out = gemm(a, w, b, resid, out_fmt=out_fmt, act=act, split=True, tag=tag)
    if N != w.shape[0]:
        out = out[..., :(2 * N if out_fmt == HL8 else N)].contiguous()
    return out



# ---------------------------------------------------------------------------------------------------------------------
# hipie_gemm_f8x: the split product with its two cross terms on block-scaled e4m3 (the opt-in `fp8x` policy; hipie_amd/fp8x.py is the exact
# host emulation).  Weights in the f8x format: (N, 4K) uint8 rows of 128-byte k slices [hi fp16 | q8(lo) | q8(hi)] + (N, K/32, 2) E8M0 scales.
@_timed("to_f8x")
def to_f8x(x_hl8):
    """HL8 rows (rows, 2K) fp16 on the device -> (q (rows, 2K) uint8: per 32-element block [q8(hi) | q8(lo)] e4m3, scale (rows, K/32, 2) uint8
    E8M0 [hi, lo]) with the quantiser hipie_gemm_f8x applies to its activations (hipie_to_f8x)."""
    if x_hl8.dtype != torch.float16 or x_hl8.shape[-1] % 64:
        raise RuntimeError("to_f8x: HL8 rows (fp16, 2K columns with K a multiple of 32) on the device")
    _on_device("to_f8x", "x_hl8", x_hl8)
    x2 = x_hl8.reshape(-1, x_hl8.shape[-1])
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    R, K = x2.shape[0], x2.shape[1] // 2
    q = torch.empty(R, 2 * K, dtype=torch.uint8, device=x_hl8.device)
    sc = torch.empty(R, K // 32, 2, dtype=torch.uint8, device=x_hl8.device)
    _call("hipie_to_f8x", x2.data_ptr(), x2.stride(0), q.data_ptr(), 2 * K, sc.data_ptr(), R, K)
    return q, sc


def f8x_weight(owner, key, params, weight_fn, bias_fn=None):
    """the f8x copy of a weight (N, K) -> ((Np, 4K) uint8, scales (Np, K/32, 2) uint8, bias (Np,) f32 | None, N): the HL8 split of split_weight,
    quantised on the device by hipie_to_f8x and laid out as hipie_gemm_f8x reads it.  Cached on ``owner`` under ``key`` exactly as split_weight."""
    def build():
        from . import fp8x
        w, b, N = _padded_f32(weight_fn, bias_fn)
        w_hl8 = hl8_pack(w)
        q, sc = to_f8x(w_hl8) if w_hl8.is_cuda else (None, None)
        w8, wsc = fp8x.pack_from_hl8(w_hl8, q, sc)
        return w8, wsc, b, N
    return derived(owner, ("f8x", key), params, build)


@_timed("gemm_f8x")
def gemm_f8x(a, w8, wsc, bias=None, resid=None, out_fmt=F32, act=ACT_NONE, alpha=1.0, oscale=1.0, out=None, out_row=None, out_rows=None):
    """ops.gemm's split form with the cross terms on block-scaled e4m3 (hipie_gemm_f8x): a (..., 2K) HL8 rows against the f8x weight
    (w8 (N, 4K) uint8, wsc (N, K/32, 2) uint8, from f8x_weight or fp8x.pack_weight); epilogue, output formats and row maps as ops.gemm."""
    if a.dtype != torch.float16 or w8.dtype != torch.uint8 or wsc.dtype != torch.uint8:
        raise RuntimeError("gemm_f8x: a HL8 (fp16) rows, w8 / wsc uint8, on the device")
    _on_device("gemm_f8x", "a w8 wsc bias resid out out_row", a, w8, wsc, bias, resid, out, out_row)
    N, K = w8.shape[0], w8.shape[1] // 4
    a2 = a if a.dim() == 2 else a.reshape(-1, a.shape[-1])
    if a2.stride(-1) != 1 or a2.shape[-1] != 2 * K or not w8.is_contiguous() or tuple(wsc.shape) != (N, K // 32, 2) or not wsc.is_contiguous():
        raise RuntimeError("gemm_f8x: a rows %s against an f8x weight %s / scales %s" % (tuple(a.shape), tuple(w8.shape), tuple(wsc.shape)))
    M = a2.shape[0]
    lead = a.shape[:-1]
    if out_row is not None:
        if out is None:
            lead = (int(out_rows),)
        if out_row.dtype != torch.int32 or out_row.numel() != M or not out_row.is_contiguous():
            raise RuntimeError("gemm_f8x: out_row must be a contiguous int32 vector with one entry per row of a")
    if out is None:
        dt, width = {F32: (torch.float32, N), F16: (torch.float16, N), HL8: (torch.float16, 2 * N)}[out_fmt]
        out = torch.empty(*lead, width, dtype=dt, device=a.device)
    o2 = out.reshape(-1, out.shape[-1])
    r2 = None if resid is None else _layout("gemm_f8x", "resid", resid.reshape(-1, N), torch.float32, density=_ROWS)
    _layout("gemm_f8x", "bias", bias, torch.float32)
    _call("hipie_gemm_f8x", a2.data_ptr(), a2.stride(0), w8.data_ptr(), 2 * K, wsc.data_ptr(), _ptr(bias),
          _ptr(r2), 0 if r2 is None else r2.stride(0), o2.data_ptr(), o2.stride(0), _ptr(out_row), M, N, K, HL8, int(out_fmt), int(act), float(alpha), float(oscale))
    return out


def f8x_linear(x_hl8, owner, key, weight, bias=None, act=ACT_NONE, out_fmt=F32, resid=None, out=None):
    """split_linear (HL8 input) on hipie_gemm_f8x: the weight's f8x copy is cached on ``owner`` under ``key``"""
    params = [weight] + ([bias] if bias is not None else [])
    w8, wsc, b, N = f8x_weight(owner, key, params, lambda: weight, (lambda: bias) if bias is not None else None)
    if N != w8.shape[0]:
        raise RuntimeError("f8x_linear: N %% 8 == 0 expected (got %d)" % N)
    return gemm_f8x(x_hl8, w8, wsc, b, resid, out_fmt=out_fmt, act=act, out=out)

def split_linear_ln_ok(x, weight, norm_weight):
    """the fused projection + residual LayerNorm (hipie_gemm_ln) applies: 256 output features = one column tile, split-able K."""
    return (x.is_cuda and weight.dtype == torch.float32 and weight.shape[0] == 256 and norm_weight.numel() == 256 and weight.shape[1] % 32 == 0
            and not torch.is_grad_enabled())


@_timed("gemm_ln")
def split_linear_ln(x, owner, key, weight, bias, resid, norm_weight, norm_bias, eps, x_hl8=False, want_hl8=True):
    """LayerNorm(resid + F.linear(x, weight, bias)) over 256 features as ONE launch (hipie_gemm_ln): returns (n fp32, n as HL8 or None).
    x (..., K) fp32 rows or HL8 (x_hl8); resid (..., 256) fp32; the HL8 copy of `weight` is cached on `owner` under `key` (split_weight)."""
    who = "split_linear_ln"
    _on_device(who, "x weight bias resid norm_weight norm_bias", x, weight, bias, resid, norm_weight, norm_bias)
    w, b, N = split_weight(owner, key, [weight] + ([bias] if bias is not None else []), lambda: weight, (lambda: bias) if bias is not None else None)
    if N != 256 or w.shape[0] != 256:
        raise RuntimeError("split_linear_ln: 256 output features expected")
    K = w.shape[1] // 2
    a_f32 = not x_hl8
    if a_f32 and (x.dtype != torch.float32 or x.stride(-1) != 1):
        raise RuntimeError("split_linear_ln: x must be fp32 rows or HL8")
    a2 = x.reshape(-1, x.shape[-1])
    if a2.shape[-1] != (K if a_f32 else 2 * K) or (a_f32 and (a2.stride(0) % 4 or a2.data_ptr() % 16)):
        raise RuntimeError("split_linear_ln: operand rows %s against weight %s" % (tuple(x.shape), tuple(weight.shape)))
    r2 = resid.reshape(-1, 256)
    M = a2.shape[0]
    _layout(who, "resid", r2, torch.float32, (M, 256), density=_ROWS)
    _layout(who, "norm_weight", norm_weight, torch.float32)
    _layout(who, "norm_bias", norm_bias, torch.float32)
    _layout(who, "w", w)          # the cached HL8 copy of weight (on weight's device)
    out = torch.empty(*resid.shape[:-1], 256, dtype=torch.float32, device=x.device)
    o16 = torch.empty(*resid.shape[:-1], 512, dtype=torch.float16, device=x.device) if want_hl8 else None
    _call("hipie_gemm_ln", a2.data_ptr(), a2.stride(0), w.data_ptr(), w.shape[1], _ptr(b), r2.data_ptr(), r2.stride(0),
          norm_weight.data_ptr(), norm_bias.data_ptr(), float(eps), out.data_ptr(), 256, _ptr(o16), 512, M, K, F32 if a_f32 else HL8, 1.0)
    return out, o16


_SHUFFLE_MAPS = {}


def _shuffle_maps(B, H, W, device):
    """row maps of ConvTranspose2d(k = 2, s = 2) as four linears: input pixel (b, h, w), tap (i, j) -> row of the (B, 2H, 2W, C) output."""
    key = (B, H, W, str(device))
    m = _SHUFFLE_MAPS.get(key)
    if m is None:
        b = torch.arange(B, device=device).view(B, 1, 1)
        h = torch.arange(H, device=device).view(1, H, 1)
        w = torch.arange(W, device=device).view(1, 1, W)
        m = [((b * 2 * H + 2 * h + i) * 2 * W + 2 * w + j).reshape(-1).to(torch.int32).contiguous() for i in range(2) for j in range(2)]
        if len(_SHUFFLE_MAPS) > 16:
            _RETIRED.extend(_SHUFFLE_MAPS.values())
            _SHUFFLE_MAPS.clear()
        _SHUFFLE_MAPS[key] = m
    return m


def convt2x2_split(rows, owner, key, weight, bias, B, H, W):
    """ConvTranspose2d(kernel 2, stride 2) of a channels-last map at fp32-class accuracy: rows (B*H*W, C_in) fp32 pixel rows, weight
    (C_in, C_out, 2, 2), bias (C_out) or None -> (B, 2H, 2W, C_out) fp32 channels-last.  One split linear per tap whose output rows go
    straight to their place in the up-sampled map (hipie_gemm's row map): the pixel shuffle costs no pass of its own."""
    Cin, Cout = weight.shape[0], weight.shape[1]
    if rows.dim() != 2 or rows.shape[0] != B * H * W or rows.shape[1] != Cin or Cout % 8:
        raise RuntimeError("convt2x2_split: rows (B*H*W, C_in), weight (C_in, C_out, 2, 2) with C_out %% 8 == 0, got %s / %s" % (tuple(rows.shape), tuple(weight.shape)))
    out = torch.empty(B, 2 * H, 2 * W, Cout, dtype=torch.float32, device=rows.device)
    o2 = out.view(-1, Cout)
    maps = _shuffle_maps(B, H, W, rows.device)
    a = rows if rows.dtype == torch.float32 and rows.is_contiguous() else rows.float().contiguous()
    for t in range(4):
        i, j = divmod(t, 2)
        split_linear(a, owner, "%s_tap%d" % (key, t), weight, bias, weight_fn=lambda i=i, j=j: weight[:, :, i, j].t().contiguous(),
                     out=o2, out_row=maps[t], tag="gemm_convt")
    return out


@_timed("topk")
def topk(x, k, want_values=False):
    """row-wise top-k of a (rows, n) fp32 device tensor (row stride may exceed n), k <= 1024 -> indices (rows, k) int64 in descending value
    order (ties: ascending index) [, values].  hipie_topk: one launch, hipGraph-replay safe (torch.topk on this stack is neither)."""
    _layout("topk", "x", x, torch.float32, ndim=2, density=_ROWS)
    _on_device("topk", "x", x)
    rows, n = x.shape
    idx = torch.empty(rows, k, dtype=torch.int64, device=x.device)
    val = torch.empty(rows, k, dtype=torch.float32, device=x.device) if want_values else None
    _call("hipie_topk", x.data_ptr(), x.stride(0), rows, n, int(k), idx.data_ptr(), _ptr(val))
    return (idx, val) if want_values else idx


def topk_ok(x, k):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and 0 < k <= min(1024, x.shape[1])
