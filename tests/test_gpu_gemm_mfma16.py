"""GPU: the 16x16x32-MFMA instance of the wide split GEMM (gemm_kernel<320, true, 0 | 2, 16>, csrc/gemm_tile.h) against the float64 product
of the same operands -- the helper, the metric and the bounds of test_gpu_gemm.py: 3e-6 for fp32 and HL8 outputs, 6e-4 for fp16 outputs, and
the HL8 plane condition |lo| <= |hi| 2^-11 + 2^-24.

The instance is reached where hipie_gemm does not take the 64 x 128 tile kernel: ceil(M / 256) * (N / 320) >= 96 tiles, or any size through
the gather entry point.  HIPIE_GEMM_MFMA=16 (set for every test of this file) selects it in a study build of the library
(make EXTRA=-DHIPIE_STUDY_KNOBS); the shipped build reads no environment and runs these shapes on whichever instance hipie_gemm ships for them.
"""
import functools

import pytest
import torch

from test_gpu_gemm import _ref
from util import rel_err

torch.set_grad_enabled(False)
gpu = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _mfma16(monkeypatch):
    monkeypatch.setenv("HIPIE_GEMM_MFMA", "16")


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, scale_a=2.0, scale_w=None):
    """fp32 operands, their HL8 forms and a bias: made once per shape, never written to"""
    from hipie_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 7 * K)
    a = torch.randn(M, K, device="cuda", generator=g) * scale_a
    w = torch.randn(N, K, device="cuda", generator=g) * (K ** -0.5 if scale_w is None else scale_w)
    bias = torch.randn(N, device="cuda", generator=g)
    return a, w, bias, ops.hl8_pack(a), ops.hl8_pack(w)


def _planes_ok(out, M, N):
    pl = out.reshape(M, N // 8, 2, 8).float()
    hi, lo = pl[:, :, 0, :], pl[:, :, 1, :]
    return bool((lo.abs() <= hi.abs() * 2.0 ** -11 + 2.0 ** -24).all())


SHAPES = [  # M, N, K
    (5889, 1280, 32),         # a: one k stage; a last row tile of one row; 24 x 4 = 96 tiles
    (5889, 1280, 96),         # b: three stages, both LDS buffers are reused
    (2048, 3840, 64),         # c: 8 x 12 tiles, the group_m = 8 tile order
    (2305, 3840, 64),         # d: 10 row panels, a short last group
    (6144, 1280, 1280),       # e: ViT-H proj depth
]


@gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mfma16_fp32_class(M, N, K):
    from hipie_amd import ops
    a, w, bias, A, W = _operands(M, N, K)
    ref = _ref(a, w, bias, None, 0, 1.0, 1.0)
    out = ops.gemm(A, W, bias, split=True)
    err = rel_err(out, ref)
    out_h = ops.gemm(A, W, bias, split=True, out_fmt=ops.HL8)
    err_h = rel_err(ops.hl8_unpack(out_h), ref)
    print("mfma16 M=%d N=%d K=%d err f32 %.2e hl8 %.2e" % (M, N, K, err, err_h))
    assert err < 3e-6 and err_h < 3e-6
    assert _planes_ok(out_h, M, N)


@gpu
@pytest.mark.parametrize("M,N,K", [(257, 320, 64), (300, 1280, 256)])
@pytest.mark.parametrize("drop", [False, True])
def test_mfma16_gather_entry(M, N, K, drop):
    """f: a tiny problem on the big kernel through hipie_gemm_gather, a row map with repeats; with an out_row map that drops rows (-1) the
    rows that no product row names keep their bytes"""
    from hipie_amd import ops
    R = M // 2 + 3                                      # operand rows: every one is read about twice
    a, w, bias, A, W = _operands(R, N, K)
    g = torch.Generator(device="cuda").manual_seed(M + N)
    a_row = torch.randint(0, R, (M,), device="cuda", generator=g, dtype=torch.int32)
    full = _ref(a[a_row.long()], w, bias, None, 0, 1.0, 1.0)
    for fmt in (ops.F32, ops.HL8):
        if not drop:
            out = ops.gemm(A, W, bias, split=True, a_row=a_row, out_fmt=fmt)
            got = out if fmt == ops.F32 else ops.hl8_unpack(out)
            assert got.shape == (M, N)
            err = rel_err(got, full)
        else:
            rows_out = M + 5
            perm = torch.randperm(rows_out, device="cuda", generator=g)[:M].to(torch.int32)
            dropped = torch.rand(M, device="cuda", generator=g) < 0.25
            out_row = torch.where(dropped, torch.full_like(perm, -1), perm).contiguous()
            width = N if fmt == ops.F32 else 2 * N
            out = torch.full((rows_out, width), 7.0, device="cuda", dtype=torch.float32 if fmt == ops.F32 else torch.float16)
            ops.gemm(A, W, bias, split=True, a_row=a_row, out_row=out_row, out=out, out_fmt=fmt)
            keep = ~dropped
            got = out if fmt == ops.F32 else ops.hl8_unpack(out)
            err = rel_err(got[out_row[keep].long()], full[keep])
            untouched = torch.ones(rows_out, dtype=torch.bool, device="cuda")
            untouched[out_row[keep].long()] = False
            assert bool((out[untouched] == 7.0).all())
        print("mfma16 gather M=%d N=%d K=%d drop=%s fmt=%d err %.2e" % (M, N, K, drop, fmt, err))
        assert err < 3e-6


@gpu
@pytest.mark.parametrize("out_fmt", ["f32", "f16", "hl8"])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("with_res", [False, True])
def test_mfma16_epilogues(out_fmt, act, with_res):
    """g: alpha = 0.5, oscale = 4 for the 16-bit outputs; with a residual and an fp32 output the residual IS the output tensor"""
    from hipie_amd import ops
    M, N, K = 5889, 1280, 64
    a, w, bias, A, W = _operands(M, N, K)
    g = torch.Generator(device="cuda").manual_seed(17 + act)
    resid = torch.randn(M, N, device="cuda", generator=g) if with_res else None
    alpha, osc = 0.5, (4.0 if out_fmt != "f32" else 1.0)
    fmt = {"f32": ops.F32, "f16": ops.F16, "hl8": ops.HL8}[out_fmt]
    ref = _ref(a, w, bias, resid, act, alpha, osc)
    if with_res and out_fmt == "f32":
        out = resid.clone()
        ops.gemm(A, W, bias, out, out_fmt=fmt, act=act, alpha=alpha, oscale=osc, split=True, out=out)
    else:
        out = ops.gemm(A, W, bias, resid, out_fmt=fmt, act=act, alpha=alpha, oscale=osc, split=True)
    if out_fmt == "hl8":
        assert out.shape == (M, 2 * N) and out.dtype == torch.float16
        got, tol = ops.hl8_unpack(out), 3e-6
        assert _planes_ok(out, M, N)
    elif out_fmt == "f16":
        got, tol = out.float(), 6e-4               # one fp16 rounding of the result
    else:
        got, tol = out, 3e-6
    err = rel_err(got, ref)
    print("mfma16 epilogue out=%s act=%d res=%s err %.2e" % (out_fmt, act, with_res, err))
    assert err < tol


@gpu
def test_mfma16_fp32_rows_equal_the_converted_form_bit_for_bit():
    """h: fp32 A rows (VAR 2) give the bits of the same call on hl8_pack(a) -- a strided view, values beyond the fp16 range (saturated) and an
    fp16-subnormal remainder included"""
    from hipie_amd import ops
    M, N, K = 5889, 1280, 256
    g = torch.Generator(device="cuda").manual_seed(M + 2 * N + K)
    wide = torch.randn(M, K + 64, device="cuda", generator=g) * 2.0
    a = wide[:, 32:32 + K]                                   # row stride K + 64, 128-byte offset
    a[0, :4] = torch.tensor([7e4, -1e5, 1e-3, 65504.0], device="cuda")
    w = ops.hl8_pack(torch.randn(N, K, device="cuda", generator=g) * (K ** -0.5))
    bias = torch.randn(N, device="cuda", generator=g)
    want = ops.gemm(ops.hl8_pack(a), w, bias, split=True, act=ops.ACT_RELU)
    got = ops.gemm(a, w, bias, split=True, act=ops.ACT_RELU)
    assert torch.equal(got, want)
    want_h = ops.gemm(ops.hl8_pack(a), w, bias, split=True, out_fmt=ops.HL8)
    got_h = ops.gemm(a, w, bias, split=True, out_fmt=ops.HL8)
    assert torch.equal(got_h, want_h)


@gpu
def test_mfma16_small_magnitudes():
    """i: operands whose lo halves are fp16 subnormals (|x| ~ 1e-2): the bound of test_gemm_split_small_magnitudes"""
    from hipie_amd import ops
    M, N, K = 5889, 1280, 256
    a, w, _, A, W = _operands(M, N, K, 1e-2, 1e-2)
    out = ops.gemm(A, W, None, split=True)
    err = rel_err(out, _ref(a, w, None, None, 0, 1.0, 1.0))
    print("mfma16, subnormal lo parts: err %.2e" % err)
    assert err < 2e-5


@gpu
def test_mfma16_same_bits_from_call_to_call():
    """j: case b twice with other work in between"""
    from hipie_amd import ops
    M, N, K = 5889, 1280, 96
    a, w, bias, A, W = _operands(M, N, K)
    first = ops.gemm(A, W, bias, split=True, out_fmt=ops.HL8)
    a2, w2, bias2, A2, W2 = _operands(2048, 3840, 64)
    ops.gemm(A2, W2, bias2, split=True)
    torch.randn(1 << 20, device="cuda").sum()
    again = ops.gemm(A, W, bias, split=True, out_fmt=ops.HL8)
    assert torch.equal(first, again)
