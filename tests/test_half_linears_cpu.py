"""CPU: the half-precision training linears (csrc/half_pack.hip, hipie_gemm_batched_f16, hipie_amd/ops_half.py, functions.HalfLinearFunction /
HalfMlpFunction, net.half_policy) -- the host restatement and the emulated backward table of the issue, the wrappers' refusals, the backend
classes, the eligibility rule, the header entries and the C ABI's own checks (nothing is launched here)."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch

import _half_linear_cases as H
from hipie_amd import _lib, ops, ops_half
from hipie_amd.training import functions, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hipie_half_pack_ws_bytes", "hipie_half_pack", "hipie_act_half", "hipie_gemm_batched_f16")


# ------------------------------------------------------------------------------------------------ the host restatement
def test_conversion_saturates_and_rounds_to_nearest_even():
    x = torch.tensor([1e6, -1e6, 65504.0, 65520.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 0.0])
    assert H.half(x).tolist() == [65504.0, -65504.0, 65504.0, 65504.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 0.0]       # ties to even; below half a subnormal: 0
    assert H.half(torch.tensor([3.0]), 2.0 ** 15).tolist() == [65504.0] and H.half(torch.tensor([2.0 ** -20]), 2.0 ** 20).tolist() == [1.0]


def test_both_layouts_and_the_pad_columns():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 32, generator=g) * 3e-7
    s, inv = H.scale_of(x)
    rows, t = H.half_rows(x, s), H.half_t(x, s)
    assert rows.shape == (40, 32) and t.shape == (32, 64) and rows.dtype == t.dtype == torch.float16
    assert torch.equal(t[:, :40], rows.t()) and not bool(t[:, 40:].any())
    assert float((rows.float() * inv - x).abs().max()) <= 2.0 ** -11 * float(x.abs().max())            # scaled: every entry a normal fp16 number
    assert float((H.half_rows(x).float() - x).abs().max()) > 1e-2 * float(x.abs().max())              # unscaled: subnormal fp16
    assert H.half_t(torch.zeros(128, 8)).shape == (8, 128) and H.half_t(torch.zeros(129, 8)).shape == (8, 192)
    a, b = torch.randn(7, 64, generator=g), torch.randn(5, 64, generator=g)
    assert torch.equal(H.half_product(a, b), a.half().double() @ b.half().double().t())


def test_chunk_rule_with_64_row_groups():
    for shape, nk in zip(H.SHAPES, H.CHUNKS):
        assert H.chunks(*shape) == functions._weight_grad_chunks(*shape, 64) == nk, shape
    for M, N, K in ((8192, 1280, 1280), (8192, 5120, 1280), (43520, 2048, 256), (256, 128, 128)):
        nk = functions._weight_grad_chunks(M, N, K, 64)
        assert nk == H.chunks(M, N, K) and (-(-M // 64) * 64) % (64 * nk) == 0
    # the split nodes' rule is the default and unchanged
    for M, N, K, nk in ((300, 96, 160, 2), (1024, 64, 64, 16), (333, 320, 256, 1), (8192, 1280, 1280, 16), (8192, 5120, 1280, 4)):
        assert functions._weight_grad_chunks(M, N, K) == nk


@pytest.mark.parametrize("M,N,K", H.SHAPES)
def test_emulated_backward_table(M, N, K):
    """the issue's table, both halves: with the scale y, dx and dW are between 2.6e-4 and 3.7e-4 at EVERY gain; without it dx / dW are 1.6e-2
    to 2.3e-2 at 2^-20, 1.0 at 2^-30 and 0.12 to 0.25 at 2^15 (y does not depend on the gain)"""
    for g in H.GAINS:
        scaled, raw = H.emulated_errors(M, N, K, g, True), H.emulated_errors(M, N, K, g, False)
        print("HLC emulated (%d,%d,%d) g=%.1e: scaled y %.2e dx %.2e dW %.2e | unscaled dx %.2e dW %.2e" % (M, N, K, g, *scaled, *raw[1:]))
        assert all(2.55e-4 <= e <= 3.75e-4 for e in scaled), (g, scaled)
        assert all(e < H.UNROUNDED_BOUND / 2.6 for e in scaled)                                      # the 2.7 x room of the node tests' second bound
        if g == 2.0 ** -20:
            assert all(1.55e-2 <= e <= 2.35e-2 for e in raw[1:]), raw
        elif g == 2.0 ** -30:
            assert raw[1:] == (1.0, 1.0)
        elif g == 2.0 ** 15:
            assert all(0.115 <= e <= 0.255 for e in raw[1:]), raw


# ------------------------------------------------------------------------------------------------ the wrappers
def _host_calls():
    x32, x16, blk, u = torch.zeros(64, 64), torch.zeros(64, 64, dtype=torch.float16), torch.ones(2), torch.zeros(64, 64)
    return {"half_pack": lambda: ops_half.half_pack(x32, blk), "half_pack fp16": lambda: ops_half.half_pack(x16),
            "act_half": lambda: ops_half.act_half(u, ops.ACT_GELU), "gemm_split_k_half": lambda: ops_half.gemm_split_k_half(x16, x16, 1),
            "gemm_split_k_half parts": lambda: ops_half.gemm_split_k_half(x16, x16, 1, None, True)}


def test_wrappers_refuse_cpu_tensors(monkeypatch):
    """each wrapper called with host tensors raises the ONE refusal wording (ops._on_device) before ops._call"""
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("a refused call reached the library: %s" % (a[:1],)))
    monkeypatch.setattr(ops, "_size", lambda *a: pytest.fail("a refused call reached a size query: %s" % (a[:1],)))
    for name, f in _host_calls().items():
        with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \(%s: \w+ must be a CUDA/HIP tensor\)" % name.split()[0]):
            f()
    src = open(ops_half.__file__).read()
    assert "Not implemented" not in src and "def _" not in src                                       # no wording and no checker of its own
    assert src.count("ops._call(") == 4 and "_lib" not in src


def test_wrappers_refuse_before_a_launch(monkeypatch):
    """dtype, density, alignment, N % 8, rows_p % 64, the scale block, the chunking: refused by the wrapper itself"""
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("a refused call reached the library: %s" % (a[:1],)))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    blk = torch.ones(2)
    base = torch.zeros(64 * 48 + 8)
    x = base[:64 * 32].view(64, 32)
    h = torch.zeros(64, 128, dtype=torch.float16)
    cases = ((lambda: ops_half.half_pack(x.double()), "torch.float32 / torch.float16"), (lambda: ops_half.half_pack(x.t()), "contiguous rows"),
             (lambda: ops_half.half_pack(base[:64 * 34].view(64, 34)[:, :32]), "multiple of 4"),
             (lambda: ops_half.half_pack(torch.zeros(64, 36, dtype=torch.float16)[:, :32]), "multiple of 8"),
             (lambda: ops_half.half_pack(base[1:64 * 32 + 1].view(64, 32)), "16-byte aligned"),
             (lambda: ops_half.half_pack(base[:64 * 36].view(64, 36)), "N a multiple of 8"), (lambda: ops_half.half_pack(base[:32]), "2 dimensions"),
             (lambda: ops_half.half_pack(x, rows_p=96), "multiple of 64"), (lambda: ops_half.half_pack(x, rows_p=0), "multiple of 64"),
             (lambda: ops_half.half_pack(x, torch.ones(3)), r"scale must be \(2,\)"), (lambda: ops_half.half_pack(x, blk.double()), "scale must be torch.float32"),
             (lambda: ops_half.act_half(x.half(), ops.ACT_GELU), "torch.float32"), (lambda: ops_half.act_half(x, 3), "ACT_GELU or ACT_RELU"),
             (lambda: ops_half.act_half(base[:64 * 36].view(64, 36), ops.ACT_RELU), "multiple of 8"), (lambda: ops_half.act_half(x.t(), ops.ACT_RELU), "contiguous"),
             (lambda: ops_half.gemm_split_k_half(h, h, 4), r"64 \* nk"), (lambda: ops_half.gemm_split_k_half(h, h.float(), 1), "torch.float16"),
             (lambda: ops_half.gemm_split_k_half(h, h, 2, blk), "one torch.float32 element"),
             (lambda: ops_half.gemm_split_k_half(h, torch.zeros(12, 128, dtype=torch.float16), 2), "N a multiple of 8"))
    for f, word in cases:
        with pytest.raises(RuntimeError, match=word):
            f()


def test_half_weight_is_cached_through_derived():
    w = torch.nn.Parameter(torch.tensor([[1.0 + 2.0 ** -11, 1e6], [-1e6, 3.0]]))
    a = ops_half.half_weight(w, "w", [w], lambda: w)
    assert a.dtype == torch.float16 and a.tolist() == [[1.0, 65504.0], [-65504.0, 3.0]] and not a.requires_grad
    assert ops_half.half_weight(w, "w", [w], lambda: pytest.fail("rebuilt")) is a
    t = ops_half.half_weight(w, "w.T", [w], lambda: w.t())
    assert t.is_contiguous() and torch.equal(t, a.t())
    hl, _, _ = ops.split_weight(w, "w", [w], lambda: torch.zeros(8, 8))                               # the HL8 copy under the same key: another entry
    assert hl.shape == (8, 16) and ops_half.half_weight(w, "w", [w], lambda: pytest.fail("rebuilt")) is a
    with torch.no_grad():
        w.mul_(2.0)                                                                                  # an in-place update invalidates it
    assert ops_half.half_weight(w, "w", [w], lambda: w).tolist() == [[2.0, 65504.0], [-65504.0, 6.0]]


# ------------------------------------------------------------------------------------------------ the backend classes
def test_policy_composes_and_leaves_the_tables_alone():
    known = {**net.GROUPS, **net.EXTRA_GROUPS, **net.LATER_GROUPS}
    assert net.HipBackendHalfLinears not in known.values() and not any(issubclass(c, net.HipBackendHalfLinears) for c in known.values())
    assert "half_linears" not in known and not any("half" in n for n in known)
    own = {"linear_half", "mlp_half"}
    assert own == {k for k, v in vars(net.HipBackendHalfLinears).items() if isinstance(v, staticmethod)}
    before = {n: net.backend(n) for n in known}
    every = net.backend(*known)
    plain = net.half_policy(net.HipBackend)
    assert issubclass(plain, net.HipBackendHalfLinears) and plain.__mro__[1] is net.HipBackendHalfLinears and plain.linear is net.HipBackend.linear
    assert net.half_policy(net.HipBackend) is plain and net.half_policy(plain) is plain                # built once per class
    for name, cls in known.items():
        assert not own & set(vars(cls)), name                                                        # no op a table class defines
        be = net.half_policy(net.backend(name))
        assert issubclass(be, cls) and issubclass(be, net.HipBackendHalfLinears) and be is net.half_policy(cls)
        assert be.linear_half is net.HipBackendHalfLinears.linear_half and not hasattr(cls, "linear_half")
    allh = net.half_policy(every)
    assert issubclass(allh, every) and allh.__bases__ == (net.HipBackendHalfLinears, every)
    # net.backend and its tables are what they were
    assert {n: net.backend(n) for n in known} == before and net.backend(*known) is every and net.backend() is net.HipBackend
    assert not any(issubclass(c, net.HipBackendHalfLinears) for c in net._COMPOSED.values())
    with pytest.raises(ValueError, match="unknown backend group"):
        net.backend("half_linears")


def test_blin_and_bmlp_ask_the_half_ops_first():
    calls = []
    sd = {"a.weight": torch.zeros(4, 4), "a.bias": None, "b.weight": torch.zeros(4, 4)}
    x = torch.zeros(2, 4)

    def spy(name):
        return staticmethod(lambda *a: calls.append(name) or x)
    ops_ = {n: spy(n) for n in ("linear", "linear_scaled", "mlp_scaled", "linear_half", "mlp_half")}
    half = type("Half", (net.HipBackendHalfLinears,), {k: ops_[k] for k in ("linear", "linear_half", "mlp_half")})
    half_mlp = type("HalfMlp", (half, net.HipBackendMlp), {"mlp": spy("mlp")})
    everything = type("Everything", (half_mlp, net.HipBackendScaledGrads), {k: ops_[k] for k in ("linear_scaled", "mlp_scaled")})
    for be, want_lin, want_mlp in ((half, ["linear_half"], ["linear_half", "linear_half"]), (half_mlp, ["linear_half"], ["mlp_half"]),
                                   (everything, ["linear_half"], ["mlp_half"])):
        del calls[:]
        net._blin(x, sd, "a.", be)
        assert calls == want_lin, be
        del calls[:]
        net._bmlp(x, sd, "a.", "b.", "relu", be)
        assert calls == want_mlp, be


# ------------------------------------------------------------------------------------------------ eligibility
def test_half_linear_ok_declines_what_the_kernels_do_not_take():
    def t(shape, dtype=torch.float32, cuda=True):
        return types.SimpleNamespace(shape=shape, dtype=dtype, is_cuda=cuda)
    assert functions.half_linear_ok(t((256, 128)), t((192, 128)), 256) is True
    assert not functions.half_linear_ok(t((256, 96)), t((128, 96)), 256)                              # K = 96
    assert not functions.half_linear_ok(t((256, 128)), t((96, 128)), 256)                             # N = 96: the contraction of dx
    assert not functions.half_linear_ok(t((255, 128)), t((128, 128)), 255)                            # 255 rows
    assert not functions.half_linear_ok(t((256, 128), torch.float16), t((128, 128)), 256)
    assert not functions.half_linear_ok(t((256, 128)), t((128, 128), torch.bfloat16), 256)
    assert not functions.half_linear_ok(t((256, 128), cuda=False), t((128, 128)), 256)
    # what is declined runs the split node, whose own fall-through on the host is the library
    x, w = torch.randn(8, 32), torch.randn(32, 32)
    assert torch.equal(functions.half_linear(x, w, None, w, "w"), torch.nn.functional.linear(x, w))
    want = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, w)), w)
    assert torch.equal(functions.half_mlp(x, w, None, w, None, ops.ACT_RELU), want)
    assert not functions.HALF_NODE_CALLS


# ------------------------------------------------------------------------------------------------ header, Makefile, tools, C ABI
def test_header_entries_exist_and_cite_what_they_replace():
    text = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    c_p, c_i, c_l, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.SIGNATURES["hipie_half_pack_ws_bytes"] == [c_l, c_i] and _lib.RESTYPES["hipie_half_pack_ws_bytes"] is c_l
    assert _lib.SIGNATURES["hipie_half_pack"] == [c_p, c_l, c_i, c_p, c_p, c_l, c_p, c_l, c_p, c_p, c_l, c_i, c_l, c_p]
    assert _lib.SIGNATURES["hipie_act_half"] == [c_p, c_p, c_l, c_i, c_i, c_p]
    assert _lib.SIGNATURES["hipie_gemm_batched_f16"] == [c_p, c_l, c_l, c_l, c_p, c_l, c_l, c_l, c_p, c_l, c_l, c_l, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p]
    for n in ENTRIES:
        assert hasattr(lib, n), n
    for first in ("hipie_half_pack_ws_bytes", "hipie_gemm_batched_f16"):                               # the first prototype behind each comment block
        comment = re.findall(r"/\*(.*?)\*/\s*int(?:64_t)? %s\(" % first, text, flags=re.S)
        assert len(comment) == 1
        last = comment[0].rsplit("/*", 1)[-1]
        assert "Replaces:" in last, first
        cited = last[last.rindex("Replaces:"):]                                                      # the block ENDS with a citation
        assert "vit.py:" in cited and "*/" not in cited, first
    block = text[text.index("csrc/half_pack.hip"):text.index("int64_t hipie_half_pack_ws_bytes")]
    assert block.count("Replaces:") == 2 and "hipie_act_half:" in block and "65504" in block and "bit for bit" in block
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(ROOT, "hipie_amd", "csrc", "Makefile")).read(), flags=re.M).group(1).split()
    assert "half_pack.hip" in srcs                                                                   # so the ISA lint of tests/test_isa_hazards.py walks it
    assert "DESIGN.md section 9" in open(os.path.join(ROOT, "hipie_amd", "csrc", "half_pack.hip")).read()
    assert "Half-precision training linears" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_bench_flag():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_train_step as b
    assert b.HALF_FLAG == "--half-linears" and b.HALF_FLAG not in {**b.FLAGS, **b.EXTRA_FLAGS, **b.LATER_FLAGS}
    assert b.backend_names(["2", "--fused-mlp", "4"]) == (["mlp"], ["2", "4"])


def test_entry_points_refuse_on_the_host():
    """the C ABI's own checks: nothing is launched (no device here), the status is HIPIE_EINVAL and the message names the problem"""
    lib = _lib.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    def refused(rc, word):
        assert rc == -22 and word in lib.hipie_last_error(), (rc, lib.hipie_last_error())
    pack = lambda x=p, ldx=32, fmt=0, sc=p, a=p, lda=32, t=p, ldt=64, db=p, ws=p, rows=64, N=32, rows_p=64: lib.hipie_half_pack(
        x, ldx, fmt, sc, a, lda, t, ldt, db, ws, rows, N, rows_p, None)
    refused(pack(x=None), b"null")
    refused(pack(fmt=4), b"format 4")
    refused(pack(N=36, ldx=36, lda=40), b"N=36")
    refused(pack(rows_p=96), b"rows_p=96")
    refused(pack(rows_p=32, rows=32), b"rows_p=32")                                                    # a multiple of 32 is not enough
    refused(pack(rows=65), b"rows_p=64")
    refused(pack(ldx=28), b"row stride 28")
    refused(pack(ldx=34), b"row stride 34")
    refused(pack(fmt=1, ldx=36), b"row stride 36")                                                     # fp16 rows: 16-byte pieces are 8 elements
    refused(pack(lda=24), b"stride 24")
    refused(pack(ldt=60), b"stride 60")
    refused(pack(ws=None), b"come together")
    refused(pack(db=None), b"come together")
    for kw in ({"x": odd}, {"a": odd}, {"t": odd}):
        refused(pack(**kw), b"aligned")
    assert pack(a=None, t=None, db=None, ws=None) == 0 and pack(a=None, t=None, db=None, ws=None, sc=None) == 0      # all outputs NULL: nothing is launched
    assert lib.hipie_half_pack_ws_bytes(64, 32) == 128 and lib.hipie_half_pack_ws_bytes(1024, 64) == 8 * 64 * 4
    assert lib.hipie_half_pack_ws_bytes(192, 8) == 2 * 8 * 4 and lib.hipie_half_pack_ws_bytes(0, 8) == 0
    refused(lib.hipie_act_half(p, p, 64, 36, 1, None), b"N=36")
    refused(lib.hipie_act_half(p, p, 64, 32, 3, None), b"act=3")
    refused(lib.hipie_act_half(None, p, 64, 32, 1, None), b"null")
    refused(lib.hipie_act_half(p, odd, 64, 32, 2, None), b"aligned")
    assert lib.hipie_act_half(None, None, 0, 32, 1, None) == 0
    gemm = lambda A=p, lda=128, ai=64, oi=256 * 64, nk=2, N=64, K=64, ad=None: lib.hipie_gemm_batched_f16(
        A, lda, 0, ai, p, 128, 0, 64, p, N, 0, oi, 1, nk, 256, N, K, 1.0, ad, None)
    refused(gemm(K=96), b"K=96")
    refused(gemm(K=32), b"K=32")                                                                       # the split entries' k tile is not enough
    refused(gemm(N=60), b"N=60")
    refused(gemm(A=None), b"null")
    refused(gemm(A=odd), b"aligned")
    refused(gemm(lda=60), b"strides")
    refused(gemm(ai=60), b"batch offsets")
    refused(gemm(nk=0), b"problems")
    refused(gemm(ad=ctypes.c_void_p(4098)), b"alpha_dev")
