"""CPU: the fused windowed training attention (hipie_attn_train_win_forward / _backward, csrc/attn_train_win.hip) up to where a device is
needed -- the ABI surface and the host-side refusals (no launch, so callable without a GPU), the CPU refusal of the ops, the opt-in backends
and the dispatch of net.vit_attention: a backend's window_attention is asked once per block, after fused_attention, and a None answer leaves
the materialised formulation's graph untouched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from hipie_amd import _lib
from _layernorm_cases import loss_grads, vit_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipie_attn_train_win_forward", "hipie_attn_train_win_backward")


def test_abi_surface():
    head = open(os.path.join(ROOT, "include", "hipie_mi355.h")).read()
    declared = set(re.findall(r"\b(hipie_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", head, flags=re.S)))
    lib = _lib.load()
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES[NAMES[0]]) == 11 and len(_lib.SIGNATURES[NAMES[1]]) == 16
    doc = head[:head.index("int hipie_attn_train_win_forward(")].rsplit("/*", 1)[1]
    assert "hipie/backbone/vit.py:69-80" in doc and "utils.py:96-125" in doc
    csrc = os.path.join(ROOT, "hipie_amd", "csrc")
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "attn_train_win.hip" in srcs and "attn_train.hip" in srcs
    # the existing instance keeps its shape
    old = open(os.path.join(csrc, "attn_train.hip")).read()
    assert "constexpr int AT_DQ = 224;" in old and "#define AT_WAVES 8" in old and "#define AT_TR 32" in old


def test_host_refusals_without_a_launch():
    lib = _lib.load()
    ptr = [ctypes.c_void_p(4096 * (k + 1)) for k in range(13)]

    def fwd(BH=2, N=196, null=None):
        a = list(ptr[:8])
        if null is not None:
            a[null] = None
        return lib.hipie_attn_train_win_forward(*a, BH, N, None)

    def bwd(BH=2, N=196, null=None):
        a = list(ptr)
        if null is not None:
            a[null] = None
        return lib.hipie_attn_train_win_backward(*a, BH, N, None)
    for fn, name, n_ptr in ((fwd, b"attn_train_win_forward", 8), (bwd, b"attn_train_win_backward", 13)):
        for kw in (dict(N=0), dict(N=257), dict(N=-5), dict(BH=0), dict(BH=-1), dict(N=4096)):
            assert fn(**kw) == -22, (name, kw)
            msg = lib.hipie_last_error()
            assert name in msg and b"N=%d" % kw.get("N", 196) in msg and b"BH=%d" % kw.get("BH", 2) in msg, msg
        for i in range(n_ptr):
            assert fn(null=i) == -22, (name, i)
            assert name in lib.hipie_last_error() and b"null" in lib.hipie_last_error()


def test_ops_refuse_host_tensors():
    from hipie_amd import ops
    BH, N = 2, 196
    q = (torch.zeros(BH, N, 128, dtype=torch.float16),) * 2
    v80, v96 = (torch.zeros(BH, N, 80, dtype=torch.float16),) * 2, (torch.zeros(BH, N, 96, dtype=torch.float16),) * 2
    with pytest.raises(RuntimeError):
        ops.attn_train_win_forward(q, q, v80)
    with pytest.raises(RuntimeError):
        ops.attn_train_win_backward(q, q, v96, v96, torch.zeros(BH, N), torch.zeros(BH, N))


def test_backends_are_opt_in():
    from hipie_amd.training import functions, net
    from hipie_amd.training.step import TrainStep
    assert issubclass(net.HipBackendWindows, net.HipBackend)
    for be in (net.HipBackend, net.HipBackendNorms, net.HipBackendMlp, net.HipBackendNormsMlp):
        assert not hasattr(be, "window_attention"), be
    for parent in (net.HipBackendNorms, net.HipBackendMlp, net.HipBackendWindows):
        assert issubclass(net.HipBackendAll, parent)
    assert net.HipBackendAll.add_layer_norm is net.HipBackendNorms.add_layer_norm and net.HipBackendAll.mlp is net.HipBackendMlp.mlp
    assert net.HipBackendAll.window_attention is net.HipBackendWindows.window_attention
    assert net.HipBackendAll.fused_attention is net.HipBackend.fused_attention
    assert inspect.signature(TrainStep.__init__).parameters["backend"].default is None        # None -> HipBackend (step.py)
    assert issubclass(functions.WindowAttentionFunction, torch.autograd.Function)
    assert list(inspect.signature(functions.window_attention).parameters) == ["qa", "ka", "v"]
    assert list(inspect.signature(functions.window_attention_ok).parameters) == ["qa", "ka", "v"]


def test_window_attention_declines_without_raising():
    from hipie_amd.training import functions, net
    z = torch.zeros
    for qa, ka, v in ((z(2, 196, 44), z(2, 196, 44), z(2, 196, 16)),             # head width 16
                      (z(2, 196, 129), z(2, 196, 129), z(2, 196, 80)),           # 129 operand columns
                      (z(2, 257, 108), z(2, 257, 108), z(2, 257, 80)),           # N = 257
                      (z(2, 196, 108), z(2, 196, 108), z(2, 196, 80))):          # a covered shape, but on the host
        assert not functions.window_attention_ok(qa, ka, v)
        assert functions.window_attention(qa, ka, v) is None and net.HipBackendWindows.window_attention(qa, ka, v) is None


def _stub(with_fused):
    calls = []

    class Stub:
        @staticmethod
        def window_attention(qa, ka, v):
            calls.append(("window", tuple(qa.shape), tuple(ka.shape), tuple(v.shape)))
            return None
    if with_fused:
        Stub.fused_attention = staticmethod(lambda qa, ka, v: calls.append(("fused", tuple(qa.shape), tuple(ka.shape), tuple(v.shape))))
    return Stub, calls


@pytest.mark.parametrize("with_fused", [False, True])
def test_dispatch_asks_once_per_block_and_none_changes_nothing(with_fused):
    """vit_case: blocks 0 and 2 global (5 x 6 tokens), block 1 windowed (4 x 4); 2 images x 2 heads, head width 8"""
    from hipie_amd.training import net
    x, sd, cfg = vit_case(torch.float64)
    names = sorted(sd)
    leaves = [x] + [sd[n] for n in names]
    ref = net.vit_backbone(x, sd, "", cfg, None)
    be, calls = _stub(with_fused)
    got = net.vit_backbone(x, sd, "", cfg, be)
    glob, win = ((4, 30, 8 + 5 + 6),) * 2 + ((4, 30, 8),), ((16, 16, 8 + 4 + 4),) * 2 + ((16, 16, 8),)
    per_block = [glob, win, glob]
    want = [(kind,) + shapes for shapes in per_block for kind in (("fused", "window") if with_fused else ("window",))]
    assert calls == want
    for k in ("res3", "res4", "res5"):
        assert torch.equal(got[k], ref[k]), k
    gr, gg = loss_grads([ref[k] for k in sorted(ref)], leaves), loss_grads([got[k] for k in sorted(got)], leaves)
    for n, a, b in zip(["input"] + names, gr, gg):
        assert a is not None and b is not None and torch.equal(a, b), n
