"""CPU: the scaled gradient operands of the training linears (csrc/grad_pack.hip, the opt-in group "scaled_grads") without a GPU -- the
host restatement of the scale rule and of both HL8 layouts (tests/_grad_scale_cases.py), the loss the raw split suffers and the scale
removes (the issue's table), the group's place among the composed backends, the bench flag, and the wrappers' refusals."""
import itertools
import math
import os
import sys

import pytest
import torch

import _grad_scale_cases as C
from hipie_amd import _lib, ops
from hipie_amd.training import functions, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulation_reproduces_the_table():
    """the three-product split with exact accumulation on M, N, K = 300, 96, 160: the raw split of dy loses the gradient as g falls (and
    gives NaN above the fp16 range), the scaled one does not depend on g at all.  The issue does not name its generator, so its two-digit
    figures are met to the spread a maximum over 3e4 entries has between seeds: a factor of 1.5."""
    scaled = {g: C.emulated_errors(g, True) for g in C.GAINS}
    for g in C.GAINS:
        raw = C.emulated_errors(g, False)
        want = C.TABLE[g]
        for got, ref in zip(raw + scaled[g], want):
            if math.isnan(ref):
                assert math.isnan(got), (g, raw)
            elif ref == 1.0:
                assert got == 1.0, (g, raw)                  # every product is zero
            else:
                assert ref / 1.5 < got < ref * 1.5, (g, raw, scaled[g], want)
        assert max(scaled[g]) < C.BOUND
    assert len(set(scaled.values())) == 1                     # scaling by exact powers of two: the SAME error at every g
    assert C.emulated_errors(2.0 ** -20, False)[0] > 1e3 * C.BOUND


def test_scale_rule_edges():
    one = (1.0, 1.0)
    below_2_15 = C.from_bits(C.bits(2.0 ** 15) - 1)
    assert C.scale_rule(0.0) == one and C.scale_rule(-0.0) == one
    assert C.scale_rule(2.0 ** 14) == one                                         # already in [2^14, 2^15)
    assert C.scale_rule(below_2_15) == one
    assert C.scale_rule(2.0 ** 15) == (0.5, 2.0)
    assert C.scale_rule(C.from_bits(C.bits(2.0 ** 14) - 1)) == (2.0, 0.5)
    assert C.scale_rule(float("inf")) == one and C.scale_rule(float("-inf")) == one and C.scale_rule(float("nan")) == one
    # fp32 subnormals: e would be 14 + 149 = 163 for the smallest one; clamped to 126 so that 1 / s = 2^-126 is still normal
    for sub in (C.from_bits(1), C.from_bits(0x7FFFFF), 2.0 ** -130):
        assert C.scale_rule(sub) == (2.0 ** 126, 2.0 ** -126), sub
    assert C.scale_rule(2.0 ** -126) == (2.0 ** 126, 2.0 ** -126)                 # e = 140 -> 126
    assert C.scale_rule(2.0 ** -112) == (2.0 ** 126, 2.0 ** -126)                 # e = 126 exactly: the clamp's edge
    assert C.scale_rule(C.from_bits(0x7F7FFFFF)) == (2.0 ** -113, 2.0 ** 113)      # the largest finite fp32
    g = torch.Generator().manual_seed(5)
    for amax in (torch.randn(200, generator=g) * torch.exp2(torch.randint(-100, 100, (200,), generator=g).float())).abs().tolist():
        s, inv = C.scale_rule(amax)
        assert 2.0 ** 14 <= amax * s < 2.0 ** 15 and s * inv == 1.0 and math.frexp(s)[0] == 0.5, amax
    assert C.scale_of(torch.tensor([1.0, float("nan"), 3.0])) == one and C.scale_of(torch.tensor([-40000.0, 3.0])) == (0.5, 2.0)


def test_hl8_layouts():
    """both layouts against ops.hl8_unpack (the project's own reader of HL8 rows) and against each other"""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(40, 32, generator=g) * 3e-7
    s, inv = C.scale_of(x)
    rows = C.to_hl8(x, s)
    assert rows.shape == (40, 64) and rows.dtype == torch.float16
    back = ops.hl8_unpack(rows) * inv
    assert float((back - x).abs().max()) <= 2.0 ** -21 * float(x.abs().max())             # hi + lo == s x to 2^-22 of the largest entry
    raw = ops.hl8_unpack(C.to_hl8(x))
    assert float((raw - x).abs().max()) > 1e-3 * float(x.abs().max())                      # the unscaled split: subnormal hi, no lo
    t = C.to_hl8_t(x, s)
    assert t.shape == (32, 2 * 64)
    assert torch.equal(ops.hl8_unpack(t)[:, :40], ops.hl8_unpack(rows).t()) and not bool(t[:, 2 * 40:].any())      # 40 = 5 groups: pad groups zero
    h, l = C.hl_split(torch.tensor([1e6, -1e6]))
    assert h.tolist() == [65504.0, -65504.0] and l.tolist() == [0.0, 0.0]                 # saturation, as csrc/common.h


def test_group_composes_with_every_other_group():
    assert net.LATER_GROUPS["scaled_grads"] is net.HipBackendScaledGrads
    be = net.backend("scaled_grads")
    assert be is net.HipBackendScaledGrads and issubclass(be, net.HipBackend)
    assert be.linear is net.HipBackend.linear                                              # the existing op is not redefined
    known = {**net.GROUPS, **net.EXTRA_GROUPS, **net.LATER_GROUPS}
    own = {"linear_scaled", "mlp_scaled", "mask_einsum_scaled"}
    assert own == {k for k, v in vars(be).items() if isinstance(v, staticmethod)}
    for name, cls in known.items():
        if name != "scaled_grads":
            assert not own & set(vars(cls)), name                                          # no op defined by two groups
            both = net.backend(name, "scaled_grads")
            assert issubclass(both, cls) and issubclass(both, be) and both.linear_scaled is be.linear_scaled
    every = net.backend(*known)
    bases = [b.__name__ for b in every.__bases__]
    assert bases[-2:] == ["HipBackendQueryAttention", "HipBackendFusionAttention"]
    assert bases.index("HipBackendScaledGrads") < bases.index("HipBackendQueryAttention")
    for a, b in itertools.combinations(("scaled_grads", "query_attention", "fusion_attention", "mlp"), 2):
        names = [c.__name__ for c in net.backend(a, b).__bases__]
        if "HipBackendScaledGrads" in names:
            assert all(names.index("HipBackendScaledGrads") < names.index(n) for n in names if n.endswith(("QueryAttention", "FusionAttention")))


def test_blin_and_bmlp_ask_the_scaled_ops_first(monkeypatch):
    calls = []
    sd = {"a.weight": torch.zeros(4, 4), "a.bias": None, "b.weight": torch.zeros(4, 4)}
    x = torch.zeros(2, 4)

    def spy(name):
        return staticmethod(lambda *a: calls.append(name) or x)
    plain = type("Plain", (net.HipBackend,), {"linear": spy("linear")})
    scaled = type("Scaled", (net.HipBackendScaledGrads,), {"linear": spy("linear"), "linear_scaled": spy("linear_scaled"), "mlp_scaled": spy("mlp_scaled")})
    both = type("Both", (scaled, net.HipBackendMlp), {"mlp": spy("mlp")})
    mlp = type("Mlp", (net.HipBackendMlp,), {"mlp": spy("mlp"), "linear": spy("linear")})
    for be, want_lin, want_mlp in ((plain, ["linear"], ["linear", "linear"]), (scaled, ["linear_scaled"], ["linear_scaled", "linear_scaled"]),
                                   (both, ["linear_scaled"], ["mlp_scaled"]), (mlp, ["linear"], ["mlp"])):
        del calls[:]
        net._blin(x, sd, "a.", be)
        assert calls == want_lin, be
        del calls[:]
        net._bmlp(x, sd, "a.", "b.", "relu", be)
        assert calls == want_mlp, be


def test_existing_nodes_are_untouched():
    assert issubclass(functions.ScaledSplitLinearFunction, functions.SplitLinearFunction)
    assert issubclass(functions.ScaledMlpFunction, functions.MlpFunction)
    assert functions.ScaledSplitLinearFunction.forward is functions.SplitLinearFunction.forward
    assert functions.ScaledSplitLinearFunction.backward is not functions.SplitLinearFunction.backward
    assert functions.ScaledMlpFunction.forward is functions.MlpFunction.forward
    for M, N, K, nk in ((300, 96, 160, 2), (1024, 64, 64, 16), (333, 320, 256, 1), (8192, 1280, 1280, 16), (8192, 5120, 1280, 4)):
        assert functions._weight_grad_chunks(M, N, K) == nk
    # shapes outside the limits fall back the way split_linear / split_mlp do
    x, w = torch.randn(8, 32), torch.randn(32, 32)
    assert torch.equal(functions.split_linear_scaled(x, w, None, w, "w"), torch.nn.functional.linear(x, w))
    want = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, w)), w)
    assert torch.equal(functions.split_mlp_scaled(x, w, None, w, None, ops.ACT_RELU), want)


def test_bench_flag():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_train_step import LATER_FLAGS, backend_names
    assert LATER_FLAGS["--scaled-grads"] == "scaled_grads"
    assert backend_names(["2", "--scaled-grads", "4", "--fused-mlp"]) == (["scaled_grads", "mlp"], ["2", "4"])


def test_wrappers_refuse_cpu_tensors():
    dy, blk = torch.zeros(64, 32), torch.ones(2)
    hl = torch.zeros(64, 64, dtype=torch.float16)
    for f in (lambda: ops.grad_scale(dy), lambda: ops.grad_pack(dy, blk), lambda: ops.gemm_scaled(hl, hl, None, split=True),
              lambda: ops.gemm_split_k_scaled(hl, hl, 1, None)):
        with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \("):
            f()


def test_entry_points_refuse_on_the_host():
    """the C ABI's own checks: nothing is launched (no device here), the status is HIPIE_EINVAL and the message names the problem"""
    lib = _lib.load()
    import ctypes
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    def refused(rc, word):
        assert rc == -22 and word in lib.hipie_last_error(), (rc, lib.hipie_last_error())
    refused(lib.hipie_grad_scale(None, 32, 64, 32, p, None), b"null")
    refused(lib.hipie_grad_scale(p, 32, 64, 30, p, None), b"N=30")
    refused(lib.hipie_grad_scale(p, 30, 64, 28, p, None), b"ldx=30")
    refused(lib.hipie_grad_scale(odd, 32, 64, 32, p, None), b"aligned")
    refused(lib.hipie_grad_scale(p, 32, 64, 32, odd, None), b"aligned")
    pack = lambda dy=p, ldx=32, sc=p, a=p, lda=64, t=p, ldt=128, db=p, ws=p, rows=64, N=32, rows_p=64: lib.hipie_grad_pack(
        dy, ldx, sc, a, lda, t, ldt, db, ws, rows, N, rows_p, None)
    refused(pack(dy=None), b"null")
    refused(pack(sc=None), b"null")
    refused(pack(N=36, ldx=36, lda=72), b"N=36")
    refused(pack(rows_p=72), b"rows_p=72")
    refused(pack(rows=65), b"rows_p=64")
    refused(pack(ldx=28), b"row stride 28")
    refused(pack(ldx=34), b"row stride 34")
    refused(pack(lda=56), b"stride 56")
    refused(pack(ldt=120), b"stride 120")
    refused(pack(ws=None), b"come together")
    refused(pack(db=None), b"come together")
    refused(pack(dy=odd), b"aligned")
    refused(pack(a=odd), b"aligned")
    refused(pack(t=odd), b"aligned")
    assert lib.hipie_grad_pack_ws_bytes(64, 32) == 128 and lib.hipie_grad_pack_ws_bytes(1024, 64) == 8 * 64 * 4
    assert lib.hipie_grad_pack_ws_bytes(129, 8) == 2 * 8 * 4 and lib.hipie_grad_pack_ws_bytes(0, 8) == 0
    refused(lib.hipie_splitk_finish(None, 2, 64, None, p, None), b"null")
    refused(lib.hipie_splitk_finish(p, 0, 64, None, p, None), b"nk=0")
    refused(lib.hipie_splitk_finish(p, 2, 66, None, p, None), b"n=66")
    refused(lib.hipie_splitk_finish(p, 2, 64, None, odd, None), b"aligned")
    # the new GEMM entry refuses what hipie_gemm refuses, with its messages, before its own pointer is looked at
    gemm = lambda N=64, K=64, ad=None: lib.hipie_gemm_scaled(p, 128, p, 128, None, None, 0, p, 64, None, 256, N, K, 4, 0, 0, 1.0, 1.0, ad, None)
    refused(gemm(N=60), b"N=60")
    refused(gemm(K=48), b"K=48")
    refused(gemm(ad=ctypes.c_void_p(4098)), b"alpha_dev")


def test_wrappers_refuse_before_a_launch(monkeypatch):
    """dtype, contiguity, alignment, N % 8 and rows_p % 32: refused by the wrapper itself -- the library is never reached"""
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("a refused call reached the library: %s" % (a[:1],)))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    blk = torch.ones(2)
    base = torch.zeros(64 * 48 + 8)
    dy = base[:64 * 32].view(64, 32)
    cases = ((lambda: ops.grad_scale(dy.double()), "torch.float32"), (lambda: ops.grad_pack(dy.half(), blk), "torch.float32"),
             (lambda: ops.grad_scale(dy.t()), "contiguous"), (lambda: ops.grad_pack(base[:64 * 34].view(64, 34)[:, :32], blk), "multiple of 4"),
             (lambda: ops.grad_scale(base[1:64 * 32 + 1].view(64, 32)), "16-byte aligned"),
             (lambda: ops.grad_pack(base[:64 * 36].view(64, 36), blk), "multiple of 8"), (lambda: ops.grad_scale(base[:64 * 6].view(64, 6)), "multiple of 4"),
             (lambda: ops.grad_pack(dy, blk, rows_p=72), "rows_p % 32"), (lambda: ops.grad_pack(dy, blk, rows_p=32), "rows_p % 32"),
             (lambda: ops.grad_pack(dy, torch.ones(3)), "block of grad_scale"), (lambda: ops.grad_pack(dy, blk.double()), "block of grad_scale"),
             (lambda: ops.grad_scale(base[:32]), "2-D"),
             (lambda: ops.gemm_split_k_scaled(dy.half(), dy.half(), 1, torch.ones(2)), "one torch.float32 element"),
             (lambda: ops.gemm_split_k_scaled(dy.half(), dy.half(), 3, None), "32 \\* nk"),
             (lambda: ops.gemm_scaled(dy.half(), dy.half(), blk, split=True), "one torch.float32 element"),
             (lambda: ops.gemm_scaled(dy.half(), dy.half(), None, split=True, a_row=torch.zeros(4, dtype=torch.int32)), "gather"))
    for f, word in cases:
        with pytest.raises(RuntimeError, match=word):
            f()
