"""CPU: the C-ABI library builds, loads, and exports every symbol include/hipie_mi355.h declares (no compute calls)."""
import ctypes
import os
import re

from hipie_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "hipie_mi355.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(hipie_[a-z_0-9]+)\s*\(", txt)))


def test_header_and_binding_agree():
    """the binding is parsed from the header; declared_symbols() is an independent regex: a prototype the parser skipped shows here"""
    assert len(_lib.SIGNATURES) == len(declared_symbols()) == len(_lib.RESTYPES)
    assert declared_symbols() == sorted(_lib.SIGNATURES) == sorted(_lib.RESTYPES)


def test_library_loads_and_exports_all():
    lib = _lib.load()
    for name in declared_symbols():
        assert hasattr(lib, name), name
    assert lib.hipie_version() == 13
    assert lib.hipie_last_error() == b""


def test_parsed_signatures_match_hand_written_ones():
    p, i, l, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    pins = {
        # a, lda, w, ldw, bias, resid, ldr, out, ldo, out_row, M, N, K, in_fmt, out_fmt, act, alpha, oscale, stream
        "hipie_gemm": [p, l, p, l, p, p, l, p, l, p, i, i, i, i, i, i, f, f, p],
        # q, k, v, out, B, H, Nq, Nk, head_dim, 12 strides, bias_h, bias_w, kh, kw, key_mask, scale, clamp, dtype, stream
        "hipie_flash_attn": [p, p, p, p, i, i, i, i, i, l, l, l, l, l, l, l, l, l, l, l, l, p, p, i, i, p, f, f, i, p],
        # logits, stride, boxes, stride, tgt_boxes, n_tgt, t_off, pos_map, labels, is_thing, ce, dice, C, status, ws, ws_bytes, B, Q, Tmax, L, sum_t,
        # five weights, with_boxes, stuff_takes_mean, stream
        "hipie_hungarian_cost": [p, l, p, l, p, p, p, p, p, p, p, p, p, p, p, l, l, i, i, i, l, f, f, f, f, f, i, i, p],
        # table, n_seg, cmap, n_chunks, steps, bc, lr, wd, n_groups, beta1, beta2, eps, norm, max_norm, grad_scale, write_grads, stream
        "hipie_optim_adamw_step": [p, l, p, l, p, p, p, p, i, d, d, d, p, d, f, i, p],
    }
    for name, argtypes in pins.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert _lib.RESTYPES[name] is i, name


def test_return_types():
    for name, restype in _lib.RESTYPES.items():
        if name.endswith(("_ws_bytes", "_workspace")) or name == "hipie_hungarian_cost_bytes":
            assert restype is ctypes.c_int64, name
        elif name == "hipie_last_error":
            assert restype is ctypes.c_char_p
        else:
            assert restype is ctypes.c_int, name
    lib = _lib.load()
    for name, restype in _lib.RESTYPES.items():
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == _lib.SIGNATURES[name], name


def test_status_entry_points_take_the_stream_last():
    """the convention ops._call rests on: it appends the stream to the arguments of whatever it calls"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipie_mi355.h")).read(), flags=re.S)
    with_stream = 0
    for name, argtypes in _lib.SIGNATURES.items():
        if _lib.RESTYPES[name] is ctypes.c_int and argtypes:
            assert re.search(r"\b%s\s*\([^)]*,\s*void\s*\*\s*stream\s*\)\s*;" % name, txt), name
            with_stream += 1
    assert with_stream >= 75


def test_parser_refuses_what_it_does_not_know():
    import pytest
    ok = "int hipie_x(const float* a, int64_t n, void* stream);"
    assert _lib.parse_header(ok)[:2] == ({"hipie_x": [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]}, {"hipie_x": ctypes.c_int})
    for bad in ("int hipie_x(size_t n, void* stream);",             # parameter type
                "size_t hipie_x(int n, void* stream);",              # return type
                "int hipie_x(unsigned n, void* stream);",            # no parameter name / unknown type
                "typedef int hipie_t;",                              # not a prototype
                ok + ok):                                            # declared twice
        with pytest.raises(_lib.HipieLibraryError, match="hipie_"):
            _lib.parse_header(bad)


def test_constants_come_from_the_header():
    from hipie_amd import ops
    assert _lib.parse_header("#define HIPIE_A 7\n#define HIPIE_B 0x1F /* c */\n#define HIPIE_C (-3)\n#define HIPIE_GUARD_H\n")[2] == {
        "HIPIE_A": 7, "HIPIE_B": 31, "HIPIE_C": -3}
    C = _lib.CONSTANTS
    assert (C["HIPIE_F32"], C["HIPIE_F16"], C["HIPIE_BF16"], C["HIPIE_F64"], C["HIPIE_HL8"]) == (0, 1, 2, 3, 4)
    assert (C["HIPIE_OUT_F32"], C["HIPIE_K_HL8_HI"], C["HIPIE_ATTN_FAST"], C["HIPIE_EINVAL"], C["HIPIE_ELAUNCH"]) == (0x100, 0x200, 1, -22, -5)
    assert (ops.F32, ops.F16, ops.BF16, ops.F64, ops.HL8) == (0, 1, 2, 3, 4)
    assert (ops.OUT_F32, ops.K_HL8_HI, ops.ATTN_FAST) == (0x100, 0x200, 1)
    import torch
    assert ops._DT == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert _lib.load().hipie_version() == C["HIPIE_ABI_VERSION"]


def test_stale_library_is_refused(monkeypatch):
    import pytest
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.CONSTANTS, "HIPIE_ABI_VERSION", _lib.CONSTANTS["HIPIE_ABI_VERSION"] + 1)
    with pytest.raises(_lib.HipieLibraryError, match="stale build"):
        _lib.load()


def test_checked_call_without_gpu(monkeypatch):
    """ops._call appends the stream and raises with the symbol it called; the no-launch path of an entry point returns"""
    import pytest
    from hipie_amd import ops
    monkeypatch.setattr(ops, "_stream", lambda: None)
    with pytest.raises(RuntimeError, match="hipie_mask_einsum") as e:
        ops._call("hipie_mask_einsum", None, None, None, 1, 300, 256, 4096, 0, 0)
    assert "null" in str(e.value)
    assert ops._call("hipie_batched_nms", None, None, None, None, None, 0, 0, 0.7, 1) is None
    assert ops._size("hipie_mask_einsum_workspace", 1, 300, 256) > 0


def test_ops_calls_the_library_in_one_place():
    src = open(os.path.join(ROOT, "hipie_amd", "ops.py")).read()
    assert src.count("_lib.check(") == 1 and src.count("_stream())") == 1 and src.count("_lib.load()") == 2      # _call, and _size beside it


def test_argument_validation_without_gpu():
    """bad arguments are rejected on the host before any launch: callable without a device."""
    lib = _lib.load()
    rc = lib.hipie_mask_einsum(None, None, None, 1, 300, 256, 4096, 0, 0, None)
    assert rc == -22 and b"null" in lib.hipie_last_error()
    rc = lib.hipie_dynamic_mask(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16),
                                1, 1, 8, 8, 8, 3, 0, None)
    assert rc == -22 and b"up=3" in lib.hipie_last_error()


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from hipie_amd import ops
    v = torch.zeros(1, 4, 2, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.ms_deform_attn_forward(v, torch.tensor([[2, 2]]), torch.tensor([0]), torch.zeros(1, 1, 2, 1, 1, 2), torch.zeros(1, 1, 2, 1, 1))


def test_new_entry_points_validate_on_the_host():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    assert lib.hipie_batched_nms(p, p, p, p, p, 1, 2000, 0.7, 1, None) == -22 and b"Q=2000" in lib.hipie_last_error()
    assert lib.hipie_sem_pan(p, p, p, p, p, p, p, p, 10, 16, 200, 8, 8, 4, 32, 32, 32, 32, 0, None) == -22
    assert b"C=200" in lib.hipie_last_error()
    assert lib.hipie_sem_pan(p, p, p, p, p, p, p, p, 10, 10, 5, 8, 8, 4, 32, 32, 32, 32, 0, None) == -22      # Npad % 16
    assert lib.hipie_vit_attn_fused(p, p, p, p, 1, 14, 14, 1, 80, 0.1, 2, None) == -22 and b"64-wide" in lib.hipie_last_error()
    assert lib.hipie_vit_attn_rel(p, p, p, p, 1, 14, 200, 1, 80, 2, 0, None) == -22 and b"wider than 96" in lib.hipie_last_error()
    assert lib.hipie_vit_attn_rel(p, p, p, p, 1, 14, 14, 1, 48, 2, 0, None) == -22 and b"head_dim" in lib.hipie_last_error()
    assert lib.hipie_mask_finalize(p, 0, None, 1, 8, 8, 4, 40, 32, 32, 32, 0.5, p, None) == -22              # crop outside the mask
    assert lib.hipie_add_layernorm_rows(p, None, p, p, None, p, 4, 6, 1e-6, 0, 0, 0, None, None, None) == -22  # C % 4
    # HIPIE_K_HL8_HI (keys = hi halves of an HL8 buffer, which are fp16) with bf16 operands would read garbage keys: refused
    st = [64 * 128, 128, 64] * 4
    assert lib.hipie_flash_attn(p, p, p, p, 1, 2, 64, 64, 64, *st, None, None, 0, 0, None, 1.0, 0.0, 2 | 0x200, None) == -22
    assert b"HL8_HI" in lib.hipie_last_error()
    # hipie_gemm_ln: residual required, K % 32, split operands only, fp32 output rows of at least 256
    assert lib.hipie_gemm_ln(p, 256, p, 512, p, None, 256, p, p, 1e-5, p, 256, p, 512, 10, 256, 0, 1.0, None) == -22 and b"null" in lib.hipie_last_error()
    assert lib.hipie_gemm_ln(p, 256, p, 512, p, p, 256, p, p, 1e-5, p, 256, p, 512, 10, 250, 0, 1.0, None) == -22 and b"K=250" in lib.hipie_last_error()
    assert lib.hipie_gemm_ln(p, 256, p, 512, p, p, 256, p, p, 1e-5, p, 256, p, 512, 10, 256, 1, 1.0, None) == -22 and b"format" in lib.hipie_last_error()
    assert lib.hipie_gemm_ln(p, 256, p, 512, p, p, 256, p, p, 1e-5, p, 200, p, 512, 10, 256, 0, 1.0, None) == -22 and b"stride" in lib.hipie_last_error()
    # empty work is a no-op even with null data pointers
    assert lib.hipie_batched_nms(None, None, None, None, None, 0, 0, 0.7, 1, None) == 0
    assert lib.hipie_mask_finalize(None, 0, None, 0, 8, 8, 4, 32, 32, 32, 32, 0.5, None, None) == 0


def test_msda_forward_refusals_without_a_launch():
    """hipie_msda_fused_forward / _strided refuse on the host: an image whose value block does not fit the 32-bit sample offsets, a value
    row stride that is not a multiple of 8 or below M*D, a reference-point width other than 2 or 4."""
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    M, D, L, P = 8, 32, 1, 1
    shape = (M, D, L, 1, P)                                   # M, D, L, Lq, P
    tail = (0, 0, M * L * P * 2, M * L * P, None)             # value dtype, aux dtype, offset / logit row strides, stream
    fused = lambda S, ref_dim: lib.hipie_msda_fused_forward(p, p, p, p, p, p, p, 1, S, *shape, ref_dim, *tail)
    strided = lambda row, S=64: lib.hipie_msda_fused_forward_strided(p, row, p, p, p, p, p, p, 1, S, *shape, 2, *tail)
    # S * row >= 2^31: exactly at the limit is refused, one pixel below passes the check and trips the next one we provoke (ref_dim 3)
    assert fused(2 ** 31 // (M * D), 2) == -22 and b"32-bit sample offsets" in lib.hipie_last_error()
    assert fused(2 ** 31 // (M * D) - 1, 3) == -22 and b"ref_dim must be 2 or 4 (got 3)" in lib.hipie_last_error()
    assert strided(3 * M * D, 2 ** 31 // (3 * M * D) + 1) == -22 and b"32-bit sample offsets" in lib.hipie_last_error()
    assert lib.hipie_msda_forward(p, p, p, p, p, p, 1, 2 ** 31 // (M * D), M, D, L, 1, P, 0, None) == -22
    assert b"32-bit sample offsets" in lib.hipie_last_error()
    # value row stride
    for row in (M * D + 4, M * D - 8, 8):
        assert strided(row) == -22 and b"value row stride %d" % row in lib.hipie_last_error(), row
    # ref_dim
    for ref_dim in (3, 0, 1, 5):
        assert fused(64, ref_dim) == -22 and b"ref_dim must be 2 or 4 (got %d)" % ref_dim in lib.hipie_last_error()
    # a refused strided call leaves no row stride behind for the next dense call: this one passes every MSDA check up to L*P
    assert strided(M * D + 4) == -22
    assert lib.hipie_msda_fused_forward(p, p, p, p, p, p, p, 1, 64, M, D, 3, 1, 11, 2, 0, 0, M * 66, M * 33, None) == -22
    assert b"L*P=33 > 32" in lib.hipie_last_error()
