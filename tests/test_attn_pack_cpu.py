"""CPU: the pack / unpack entries around the fused training attention (csrc/attn_pack.hip) up to where a device is needed -- their ABI
surface and host-side refusals, the CPU refusal of the ops, what functions.vit_attention_packed declines, and the training net's wiring: a
backend with ``packed_attention`` replaces everything between the two linears of net.vit_attention by one call; with a plain-torch stand-in
that repeats the same operations the outputs and every gradient of vit_backbone are EQUAL to the default graph's."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from hipie_amd import _lib
from _attn_pack_cases import ALL, composition, inputs
from _layernorm_cases import loss_grads as _grads, vit_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hipie_attn_pack_kv": 13, "hipie_attn_pack_q": 21, "hipie_attn_grad_amax": 4, "hipie_attn_pack_grad": 16, "hipie_attn_unpack_grad": 21}


def test_abi_surface():
    head = open(os.path.join(ROOT, "include", "hipie_mi355.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    declared = set(re.findall(r"\b(hipie_[a-z_0-9]+)\s*\(", plain))
    lib = _lib.load()
    for n, nargs in NAMES.items():
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
        assert len(_lib.SIGNATURES[n]) == nargs, n
        proto = re.search(r"\b%s\s*\(([^;]*)\);" % n, plain).group(1)
        assert len(proto.split(",")) == nargs, n                       # the binding has the header's argument count
        assert getattr(lib, n).restype is ctypes.c_int
    assert lib.hipie_version() == 13
    # the citation of the replaced reference code
    doc = head[:head.index("int hipie_attn_pack_kv(")].rsplit("/*", 1)[1]
    assert "backbone/vit.py:67-83" in doc and "backbone/utils.py:96-125" in doc
    csrc = os.path.join(ROOT, "hipie_amd", "csrc")
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "attn_pack.hip" in srcs
    # the planes come from the one shared split (common.h), the reductions from wave.h
    text = open(os.path.join(csrc, "attn_pack.hip")).read()
    assert "hl_split(" in text and "wave_max(" in text and '#include "wave.h"' in text


P = [ctypes.c_void_p(4096 * k) for k in range(1, 14)]


def _calls(lib):
    """every entry with good arguments for a 8 x 16 grid (B' = 2, heads = 3), overridable by name"""
    def pack_kv(qkv=P[0], rq=P[1], k_hi=P[2], k_lo=P[3], v_hi=P[4], v_lo=P[5], B=2, heads=3, H=8, W=16, Np=128, cols=224):
        return lib.hipie_attn_pack_kv(qkv, rq, k_hi, k_lo, v_hi, v_lo, B, heads, H, W, Np, cols, None)

    def pack_q(rq=P[0], rel_h=P[1], rel_w=P[2], q_hi=P[3], q_lo=P[4], B=2, heads=3, H=8, W=16, Np=128, cols=224, hs=(1024, 128, 8, 1), ws=(2048, 256, 16, 1)):
        return lib.hipie_attn_pack_q(rq, rel_h, *hs, rel_w, *ws, q_hi, q_lo, B, heads, H, W, Np, cols, 80 ** -0.5, None)

    def pack_grad(go=P[0], out=P[1], v_hi=P[2], v_lo=P[3], scale=P[4], do_hi=P[5], do_lo=P[6], v96_hi=P[7], v96_lo=P[8], delta=P[9], B=2, heads=3, H=8,
                  W=16, Np=128):
        return lib.hipie_attn_pack_grad(go, out, v_hi, v_lo, scale, do_hi, do_lo, v96_hi, v96_lo, delta, B, heads, H, W, Np, None)

    def unpack_grad(dq=P[0], dk=P[1], dv=P[2], dq_h=P[3], dq_w=P[4], inv=P[5], dqkv=P[6], B=2, heads=3, H=8, W=16, Np=128, cols=224, hs=(10240, 1280, 80),
                    ws=(10240, 1280, 80)):
        return lib.hipie_attn_unpack_grad(dq, dk, dv, dq_h, *hs, dq_w, *ws, inv, dqkv, B, heads, H, W, Np, cols, 80 ** -0.5, None)
    return pack_kv, pack_q, pack_grad, unpack_grad


def test_host_refusals_without_a_launch():
    lib = _lib.load()
    pack_kv, pack_q, pack_grad, unpack_grad = _calls(lib)

    def refused(fn, word, **kw):
        assert fn(**kw) == -22, (fn.__name__, kw)
        msg = lib.hipie_last_error()
        assert b"attn_" + fn.__name__.encode() in msg and word in msg, (fn.__name__, kw, msg)
    pointers = {pack_kv: ("qkv", "rq", "k_hi", "k_lo", "v_hi", "v_lo"), pack_q: ("rq", "rel_h", "rel_w", "q_hi", "q_lo"),
                pack_grad: ("go", "out", "v_hi", "v_lo", "scale", "do_hi", "do_lo", "v96_hi", "v96_lo", "delta"),
                unpack_grad: ("dq", "dk", "dv", "dq_h", "inv", "dqkv")}
    planes = {pack_kv: ("qkv", "rq", "k_hi", "k_lo", "v_hi", "v_lo"), pack_q: ("rq", "q_hi", "q_lo"),
              pack_grad: ("go", "out", "v_hi", "v_lo", "do_hi", "do_lo", "v96_hi", "v96_lo"), unpack_grad: ("dq", "dk", "dv", "dq_h", "dq_w", "dqkv")}
    for fn in (pack_kv, pack_q, pack_grad, unpack_grad):
        for name in pointers[fn]:
            refused(fn, b"null", **{name: None})
        for name in planes[fn]:
            refused(fn, b"aligned", **{name: ctypes.c_void_p(4096 + 8)})
        for name in ("B", "heads", "H", "W"):
            for bad in (0, -3):
                refused(fn, b"%s=%d" % (name.encode(), bad), **{name: bad})
        # Np is N = 128 here; N = 120 takes 120 or 128
        for Np in (0, -128, 127, 136, 256):
            refused(fn, b"Np=%d" % Np, Np=Np)
        refused(fn, b"Np=121", H=8, W=15, Np=121)
        if fn is not pack_grad:
            for cols in (0, 96, 120, 160, 256, -224):
                refused(fn, b"cols=%d" % cols, cols=cols)
            refused(fn, b"> cols=128", cols=128, H=8, W=48, Np=384)             # 80 + 56 = 136 columns
            refused(fn, b"> cols=224", H=72, W=80, Np=5760)                     # 80 + 152 = 232 (N = 5760 is a multiple of 128)
            refused(fn, b"+1", H=70, W=74, Np=5248)                             # padded: 80 + 144 + 1 = 225; unpadded it would fit
            refused(fn, b"+1", cols=128, H=24, W=24, Np=640)                    # 80 + 48 + 1 = 129
    refused(pack_q, b"stride", hs=(1024, -128, 8, 1))
    refused(unpack_grad, b"stride", hs=(10240, 1282, 80))
    refused(unpack_grad, b"stride", ws=(-10240, 1280, 80))
    # the maximum
    amax = lambda go=P[0], n=4096, out=P[1]: lib.hipie_attn_grad_amax(go, n, out, None)
    for kw, word in (({"go": None}, b"null"), ({"out": None}, b"null"), ({"n": 0}, b"n=0"), ({"n": -4}, b"n=-4"), ({"n": 4098}, b"n=4098"),
                     ({"go": ctypes.c_void_p(4100)}, b"aligned"), ({"out": ctypes.c_void_p(4098)}, b"aligned")):
        assert amax(**kw) == -22 and b"attn_grad_amax" in lib.hipie_last_error() and word in lib.hipie_last_error(), kw


def test_ops_refuse_cpu_tensors():
    from hipie_amd import ops
    qkv, tab_h, tab_w = inputs(1, 1, 8, 16)
    half = lambda *s: torch.zeros(*s, dtype=torch.float16)
    calls = [lambda: ops.attn_pack_kv(qkv, 1, 8, 16, 224),
             lambda: ops.attn_pack_q(torch.zeros(1, 128, 80), torch.zeros(1, 128, 8), torch.zeros(1, 128, 16), 1, 8, 16, 224),
             lambda: ops.attn_grad_amax(torch.zeros(1, 128, 80)),
             lambda: ops.attn_pack_grad(torch.zeros(1, 128, 80), torch.zeros(1, 128, 80), (half(1, 128, 80), half(1, 128, 80)), torch.ones(1), 1, 8, 16),
             lambda: ops.attn_unpack_grad(torch.zeros(1, 128, 224), torch.zeros(1, 128, 80), torch.zeros(1, 128, 80), torch.zeros(1, 8, 16, 80),
                                          torch.zeros(1, 8, 16, 80), torch.ones(1), 1, 8, 16)]
    for call in calls:
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            call()


def test_instances_and_what_is_declined():
    from hipie_amd.training import functions
    inst = functions.packed_attention_instance
    for (B, heads, H, W), windows in ALL:
        want = (128, False) if windows else (224, H * W % 128 != 0)
        assert inst(H, W, windows) == want, (H, W, windows)
    assert inst(64, 64) == (224, False) and inst(64, 64, True) == (224, False) and inst(14, 14, True) == (128, False)
    assert inst(50, 76) == (224, True)                              # 3800 tokens -> 3840
    assert inst(8, 16, True) == (224, False)                        # a 128-token window goes where fused_attention sends it today
    declined = [(14, 14, False),                                    # the windows without the flag: N < 1024 and no multiple of 128
                (30, 30, False), (31, 33, True),                    # 900 / 1023 tokens: too short to pad, too long for a window
                (72, 80, False),                                    # 80 + 152 > 224 although N % 128 == 0
                (70, 74, False),                                    # padded: 80 + 144 + 1 = 225
                (1, 1, True),                                       # a one-token item is WindowAttentionFunction's closed form
                (16, 17, True), (2, 47, True)]                      # 272 tokens; 80 + 49 > 128
    for H, W, windows in declined:
        assert inst(H, W, windows) is None, (H, W, windows)
    assert inst(70, 73, False) == (224, True) and inst(1, 2, True) == (128, False) and inst(16, 16, True) == (224, False)
    assert list(inspect.signature(functions.vit_attention_packed).parameters) == ["qkv", "Rh", "Rw", "heads", "H", "W", "windows"]
    assert inspect.signature(functions.vit_attention_packed).parameters["windows"].default is False
    assert issubclass(functions.VitAttentionFunction, torch.autograd.Function)
    # host tensors are not covered: None, nothing is refused
    from hipie_amd.training import net
    qkv, tab_h, tab_w = inputs(1, 1, 8, 16)
    Rh, Rw = net.get_rel_pos(8, 8, tab_h), net.get_rel_pos(16, 16, tab_w)
    assert functions.vit_attention_packed(qkv, Rh, Rw, 1, 8, 16) is None
    assert functions.vit_attention_packed(qkv.double(), Rh.double(), Rw.double(), 1, 8, 16, windows=True) is None


def test_backends_are_opt_in():
    from hipie_amd.training import net
    from hipie_amd.training.step import TrainStep
    A, Wn = net.HipBackendPackedAttention, net.HipBackendPackedWindows
    assert issubclass(A, net.HipBackend) and issubclass(Wn, A) and issubclass(Wn, net.HipBackendWindows)
    assert Wn.window_attention is net.HipBackendWindows.window_attention and Wn.fused_attention is net.HipBackend.fused_attention
    for cls in (net.HipBackend, net.HipBackendNorms, net.HipBackendMlp, net.HipBackendWindows, net.HipBackendAll, net.HipBackendAssign):
        assert not hasattr(cls, "packed_attention"), cls
    assert not hasattr(A, "window_attention")
    assert inspect.signature(TrainStep.__init__).parameters["backend"].default is None        # None -> HipBackend (step.py)
    qkv, tab_h, tab_w = inputs(1, 1, 8, 16)
    Rh, Rw = net.get_rel_pos(8, 8, tab_h), net.get_rel_pos(16, 16, tab_w)
    assert A.packed_attention(qkv, Rh, Rw, 1, 8, 16) is None and Wn.packed_attention(qkv, Rh, Rw, 1, 8, 16) is None     # host tensors


# --------------------------------------------------------------------------------------------- wiring equivalence
class _TorchPacked:
    """stand-in backend: packed_attention in plain torch -- the operations of net.vit_attention from (qkv, Rh, Rw)"""
    calls = []

    @classmethod
    def packed_attention(cls, qkv, Rh, Rw, heads, H, W):
        cls.calls.append((tuple(qkv.shape), tuple(Rh.shape), tuple(Rw.shape), heads, H, W))
        return composition(qkv, Rh, Rw, heads, H, W)


class _Declines:
    calls = []

    @classmethod
    def packed_attention(cls, qkv, Rh, Rw, heads, H, W):
        cls.calls.append((H, W))
        return None


class _NoMethod:
    pass


def _backbone(be, dtype):
    from hipie_amd.training import net
    x, sd, cfg = vit_case(dtype)
    names = sorted(sd)
    leaves = [x] + [sd[n] for n in names]
    out = net.vit_backbone(x, sd, "", cfg, be)
    outs = [out[k] for k in sorted(out)]
    return ["res3", "res4", "res5", "d input"] + ["d " + n for n in names], [o.detach() for o in outs] + list(_grads(outs, leaves))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_vit_backbone_wiring_is_the_same_graph(dtype):
    """depth 3: blocks 0 and 2 global (a 5 x 6 grid), block 1 windowed (8 windows of 4 x 4 per batch of 2 images).  The stand-in repeats the
    default graph's operations, so everything is EQUAL -- rel_pos_h / rel_pos_w and the qkv weights included."""
    names, ref = _backbone(None, dtype)
    _TorchPacked.calls = []
    _, got = _backbone(_TorchPacked, dtype)
    assert _TorchPacked.calls == [((2, 30, 48), (5, 5, 8), (6, 6, 8), 2, 5, 6), ((8, 16, 48), (4, 4, 8), (4, 4, 8), 2, 4, 4), ((2, 30, 48), (5, 5, 8), (6, 6, 8), 2, 5, 6)]
    assert any("rel_pos_h" in n for n in names) and any("qkv.weight" in n for n in names)
    for n, a, b in zip(names, ref, got):
        assert a is not None and b is not None and torch.equal(a, b), n


def test_fp32_wiring_within_the_float64_error_of_the_default_graph():
    """the bound the issue gives for a stand-in that does NOT repeat the operations, applied to the one that does: 4 x the fp32-vs-float64
    error of the default graph on this case (figures printed)"""
    names, ref64 = _backbone(None, torch.float64)
    _, ref32 = _backbone(None, torch.float32)
    _, got = _backbone(_TorchPacked, torch.float32)
    for n, r, l, g in zip(names, ref64, ref32, got):
        e_old = float((l.double() - r).abs().max() / r.abs().max())
        e = float((g.double() - r).abs().max() / r.abs().max())
        print("ATTNPACK wiring %-34s err %.3e  e_old %.3e" % (n, e, e_old))
        assert e <= max(1e-6, 4 * e_old), n


def test_a_backend_without_the_method_or_one_that_declines_leaves_the_graph():
    names, ref = _backbone(None, torch.float32)
    _Declines.calls = []
    for be in (_NoMethod, _Declines):
        _, got = _backbone(be, torch.float32)
        for n, a, b in zip(names, ref, got):
            assert torch.equal(a, b), (be.__name__, n)
    assert _Declines.calls == [(5, 6), (4, 4), (5, 6)]
