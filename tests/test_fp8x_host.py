"""CPU: the `fp8x` policy's host side -- the f8x weight format, the q8 rule on edge blocks, the emulated product's accuracy, the two C entry
points (exported, arguments validated on the host) and the register budget of the new kernel (no scratch)."""
import ctypes
import os
import re
import shutil

import pytest
import torch

from hipie_amd import _lib, fp8x, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _q8_reference(v16):
    """the q8 rule written out per block in Python floats: (codes as floats, e) -- independent of fp8x's vectorised form"""
    vals = [float(t) for t in v16.float()]
    amax = max(abs(t) for t in vals)
    e = 0
    if amax > 0:
        e = 0
        while amax * 2.0 ** e > 448.0:
            e -= 1
        while amax * 2.0 ** (e + 1) <= 448.0:
            e += 1
    e = max(-127, min(127, e))
    codes = torch.tensor([t * 2.0 ** e for t in vals], dtype=torch.float32).to(torch.float8_e4m3fn).float()
    return codes, e


def test_weight_format_byte_layout_and_scales():
    torch.manual_seed(1)
    N, K = 24, 96
    w = torch.randn(N, K) * 0.05
    w[3, 40:50] = 0.0
    w8, wsc = fp8x.pack_weight(w)
    assert w8.dtype == torch.uint8 and tuple(w8.shape) == (N, 4 * K) and tuple(wsc.shape) == (N, K // 32, 2)
    hl8 = ops.hl8_pack(w)
    hi = hl8.reshape(N, K // 8, 2, 8)[:, :, 0].reshape(N, K)
    lo = hl8.reshape(N, K // 8, 2, 8)[:, :, 1].reshape(N, K)
    for n in range(N):
        for b in range(K // 32):
            blk = w8[n, 128 * b:128 * (b + 1)]
            assert torch.equal(blk[:64].view(torch.float16), hi[n, 32 * b:32 * (b + 1)])          # hi fp16 [64 B]
            e8 = blk[64:].view(torch.float8_e4m3fn).float().reshape(8, 8)                          # e4m3 [64 B], 8 bytes per (part, group)
            for part, src in ((0, lo), (1, hi)):                                                   # scales [lo, hi]
                codes, e = _q8_reference(src[n, 32 * b:32 * (b + 1)])
                assert int(wsc[n, b, part]) == 127 - e
                # lane half h reads [q8(lo) of groups h, h + 2 | q8(hi) of groups h, h + 2] (bytes 0-15 / 16-31 = the MFMA's two k blocks)
                for h in (0, 1):
                    for i, g in enumerate((h, h + 2)):
                        assert torch.equal(e8[4 * h + 2 * part + i], codes[8 * g:8 * g + 8])


def _block(vals):
    v = torch.tensor(vals, dtype=torch.float16)
    return v.reshape(1, 32)


@pytest.mark.parametrize("name", ["zero", "fp16_max", "subnormal", "outlier", "at_448", "just_over_448"])
def test_q8_edge_blocks(name):
    v = {"zero": _block([0.0] * 32),
         "fp16_max": _block([65504.0] + [-65504.0] + [1.0] * 30),
         "subnormal": _block([2.0 ** -24 * (i % 7) * (-1) ** i for i in range(32)]),          # the lo part of small activations
         "outlier": _block([1000.0] + [1e-3 * (i + 1) for i in range(31)]),
         "at_448": _block([448.0] + [0.5] * 31),
         "just_over_448": _block([480.0] + [0.5] * 31)}[name]
    codes, scale = fp8x.quantise(v)
    ref_codes, e = _q8_reference(v[0])
    assert int(scale[0, 0]) == 127 - e
    assert torch.equal(codes.view(torch.float8_e4m3fn).float()[0], ref_codes)
    amax = float(v.float().abs().max())
    if amax > 0:
        assert amax * 2.0 ** e <= 448.0 < amax * 2.0 ** (e + 1)
    deq = fp8x.dequantise(codes, scale)[0]
    # e4m3: 3 mantissa bits -> half an ulp of 2^-4 relative in the normal range, absolute 2^-10 * 2^-e in the subnormal one
    bound = torch.maximum(v[0].double().abs() * 2.0 ** -4, torch.full((32,), 2.0 ** (-10 - e), dtype=torch.float64))
    assert bool(((deq - v[0].double()).abs() <= bound).all()), name
    if name == "zero":
        assert int(scale[0, 0]) == 127 and int(codes.abs().sum()) == 0
    if name == "fp16_max":
        assert e == -8
    if name == "subnormal":
        assert e == 32 - 2                                   # amax = 6 * 2^-24
    if name == "at_448":
        assert e == 0 and float(deq[0]) == 448.0


@pytest.mark.parametrize("K,N", [(5120, 1280), (1280, 3840), (1280, 1280), (1280, 5120)])      # ViT-H fc2, qkv, proj, fc1
def test_emulated_product_accuracy_at_vit_h_shapes(K, N):
    """the study's 1.1e-5 (tools/fp8_cross_terms.py) from the exact emulation: between the three-product form (~6e-7) and one product (~3e-4)"""
    torch.manual_seed(K + N)
    M = 128
    A = torch.randn(M, K) * 1.5
    W = torch.randn(N, K) * K ** -0.5
    x = ops.hl8_pack(A)
    w8, wsc = fp8x.pack_weight(W)
    acc = fp8x.emulate_acc(x, w8, wsc)
    ref = ops.hl8_unpack(x).double() @ W.double().t()
    err = float((acc - ref).abs().max() / ref.abs().max())
    print("K=%d N=%d: emulated fp8x product %.2e from fp64" % (K, N, err))
    assert 3e-6 <= err <= 3e-5, err


def test_f8x_entry_points_exported_and_validated_on_the_host():
    lib = _lib.load()
    assert hasattr(lib, "hipie_gemm_f8x") and hasattr(lib, "hipie_to_f8x")
    assert lib.hipie_version() == 13
    p = ctypes.c_void_p(256)
    args = dict(A=p, lda=2 * 640, W=p, ldw=2 * 640, sc=p, bias=None, resid=None, ldr=0, out=p, ldo=160, out_row=None, M=300, N=160, K=640,
                in_fmt=ops.HL8, out_fmt=ops.F32, act=0, alpha=1.0, oscale=1.0, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hipie_gemm_f8x(*a.values())
    assert call(sc=None) == -22 and b"null" in lib.hipie_last_error()
    assert call(A=None) == -22 and b"null" in lib.hipie_last_error()
    assert call(K=650, lda=1300, ldw=1300) == -22 and b"K=650" in lib.hipie_last_error()
    assert call(N=164, ldo=164) == -22 and b"N=164" in lib.hipie_last_error()
    assert call(W=ctypes.c_void_p(264)) == -22 and b"aligned" in lib.hipie_last_error()
    assert call(in_fmt=1) == -22 and b"HL8" in lib.hipie_last_error()
    assert call(lda=640) == -22 and b"strides" in lib.hipie_last_error()
    assert lib.hipie_to_f8x(p, 64, p, 64, p, 4, 40, None) == -22 and b"K=40" in lib.hipie_last_error()
    assert lib.hipie_to_f8x(p, 64, p, 64, None, 4, 32, None) == -22 and b"null" in lib.hipie_last_error()


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_f8x_kernels_use_no_scratch():
    """gemm_f8x_kernel keeps X's q8 operands, the e4m3 W fragment and 128 accumulators in the 256 registers of a wave at two waves per SIMD:
    a spill would put scratch traffic into the k loop.  Read from the code object of a --save-temps compile with the Makefile's flags."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hazard_lint as lint
    text = lint.compile_to_asm(os.path.join(ROOT, "hipie_amd", "csrc", "gemm_f8x.hip"), [])
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    f8x = [(name, body) for name, body in kernels if "f8x" in name]
    assert len(f8x) == 2, [k for k, _ in kernels]                # gemm_f8x_kernel<256> and to_f8x_kernel
    for name, body in f8x:
        size = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        assert size == 0, (name, size)
        assert "v_mfma_scale_f32_32x32x64_f8f6f4" in text
