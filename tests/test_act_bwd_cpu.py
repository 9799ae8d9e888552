"""CPU: the activation operators of the training step's MLP node (hipie_act_forward / hipie_act_backward) up to where a device is
needed -- their ABI surface and host-side refusals, the workspace query, the CPU refusal of the ops, and the training net's wiring: a
backend with ``mlp`` replaces linear -> activation -> linear of vit_backbone / encoder_layer by one call without changing one operation, so
with a plain-torch stand-in the outputs and every gradient are EQUAL to the three-node graph's."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

from hipie_amd import _lib
from _layernorm_cases import encoder_case, loss_grads as _grads, vit_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipie_act_forward", "hipie_act_backward", "hipie_act_backward_ws_bytes")


def test_abi_surface():
    head = open(os.path.join(ROOT, "include", "hipie_mi355.h")).read()
    declared = set(re.findall(r"\b(hipie_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", head, flags=re.S)))
    lib = _lib.load()
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.hipie_version() == 13
    assert len(_lib.SIGNATURES["hipie_act_forward"]) == 6 and len(_lib.SIGNATURES["hipie_act_backward"]) == 10
    assert lib.hipie_act_backward_ws_bytes.restype is ctypes.c_int64
    # the citation of the replaced reference code
    doc = head[:head.index("int hipie_act_forward(")].rsplit("/*", 1)[1]
    assert "Mlp" in doc and "backbone/vit.py:193-197" in doc and "deformable_transformer_dino.py:384-394" in doc
    # the library is built from the new source, and the GELU is one shared definition
    csrc = os.path.join(ROOT, "hipie_amd", "csrc")
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "act_bwd.hip" in srcs
    defs = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and re.search(r"float\s+gm_gelu\s*\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["gelu.h"], defs


def test_host_refusals_without_a_launch():
    lib = _lib.load()
    p, q, r, s, t = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4, 5))

    def bwd(u=p, g=q, du=r, a=s, dbias=t, ws=p, rows=8, N=256, act=1):
        return lib.hipie_act_backward(u, g, du, a, dbias, ws, rows, N, act, None)

    def fwd(u=p, a=s, rows=8, N=256, act=1):
        return lib.hipie_act_forward(u, a, rows, N, act, None)

    def refused(fn, word, **kw):
        assert fn(**kw) == -22, kw
        msg = lib.hipie_last_error()
        assert (b"act_backward" if fn is bwd else b"act_forward") in msg and word in msg, (kw, msg)
    for name in ("u", "g", "du"):
        refused(bwd, b"null", **{name: None})
    for name in ("u", "a"):
        refused(fwd, b"null", **{name: None})
    for N in (6, 250, 1026, -4):
        refused(bwd, b"N=%d" % N, N=N)
        refused(fwd, b"N=%d" % N, N=N)
    for act in (0, 3, -1, 7):
        refused(bwd, b"act=%d" % act, act=act)
        refused(fwd, b"act=%d" % act, act=act)
    refused(bwd, b"workspace", ws=None)
    refused(bwd, b"workspace", ws=None, a=None)
    refused(bwd, b"alias", du=p)                        # du == u
    refused(bwd, b"alias", a=q)                         # a == g
    refused(bwd, b"alias", a=p)                         # a == u
    refused(bwd, b"alias", a=r)                         # a == du
    refused(fwd, b"alias", a=p)
    refused(bwd, b"aligned", u=ctypes.c_void_p(260))
    refused(fwd, b"aligned", a=ctypes.c_void_p(1028))
    # empty work is a no-op even with null data pointers
    assert lib.hipie_act_backward(None, None, None, None, None, None, 0, 256, 1, None) == 0
    assert lib.hipie_act_backward(None, None, None, None, None, None, 8, 0, 2, None) == 0
    assert lib.hipie_act_forward(None, None, 0, 256, 2, None) == 0
    assert lib.hipie_act_forward(None, None, 8, 0, 1, None) == 0
    # ... but not with a bad shape or activation code
    assert lib.hipie_act_backward(None, None, None, None, None, None, 0, 6, 1, None) == -22
    assert lib.hipie_act_forward(None, None, 0, 256, 5, None) == -22


def test_workspace_query():
    lib = _lib.load()
    ws = lib.hipie_act_backward_ws_bytes
    assert isinstance(ws(5, 256), int)
    for rows in (1, 2, 4, 5, 64, 257, 4096, 4097, 8192, 43520, 10 ** 6, 10 ** 9, 2 ** 40):
        for N in (4, 256, 1024, 1028, 1280, 5120):
            b = ws(rows, N)
            assert b > 0 and b == ws(rows, N)
            assert b >= ws(max(rows - 1, 1), N)                  # monotone in rows
            assert b % (N * 4) == 0                              # whole partial rows of N floats
    assert ws(0, 256) > 0 and ws(8, 0) > 0
    # the fixed grid: the number of partial rows saturates, and where it does depends on (rows, N) alone -- on N through the number of
    # column tiles, so that the product stays a few workgroups per compute unit
    for N in (4, 256, 1024, 1028, 5120, 1 << 20):
        sat = ws(2 ** 40, N) // (N * 4)
        assert sat == ws(10 ** 9, N) // (N * 4) and 1 <= sat <= 65536, (N, sat)
    assert ws(2 ** 40, 4) // 16 == ws(2 ** 40, 1024) // 4096 >= ws(2 ** 40, 1028) // (1028 * 4) >= ws(2 ** 40, 5120) // (5120 * 4) >= 64
    # below saturation: one partial row per row chunk
    assert ws(1, 1280) == 1280 * 4 and ws(64, 1280) > ws(1, 1280)


def test_ops_refuse_cpu_tensors():
    from hipie_amd import ops
    u, g = torch.zeros(3, 8), torch.zeros(3, 8)
    for act in (ops.ACT_GELU, ops.ACT_RELU):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            ops.act_forward(u, act)
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            ops.act_backward(u, g, act)
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            ops.act_backward(u, g, act, want_a=True, want_bias_grad=True, out=g)
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            ops.act_backward(u=u, g=g, act=act, want_a=False, want_bias_grad=True, out=None)


def test_hip_backend_mlp_is_opt_in():
    from hipie_amd.training import functions, net
    from hipie_amd.training.step import TrainStep
    assert issubclass(net.HipBackendMlp, net.HipBackend) and not hasattr(net.HipBackend, "mlp") and not hasattr(net.HipBackendNorms, "mlp")
    assert issubclass(net.HipBackendNormsMlp, net.HipBackendNorms) and issubclass(net.HipBackendNormsMlp, net.HipBackendMlp)
    assert net.HipBackendNormsMlp.mlp is net.HipBackendMlp.mlp and net.HipBackendNormsMlp.add_layer_norm is net.HipBackendNorms.add_layer_norm
    assert inspect.signature(TrainStep.__init__).parameters["backend"].default is None        # None -> HipBackend (step.py)
    assert list(inspect.signature(functions.split_mlp).parameters) == ["x", "w1", "b1", "w2", "b2", "act"]
    assert issubclass(functions.MlpFunction, torch.autograd.Function)
    # host tensors are no shape the split GEMM takes: the three-node composition runs (here: on the library), nothing is refused
    g = torch.Generator().manual_seed(3)
    x, w1, b1, w2, b2 = (torch.randn(*s, generator=g) for s in ((5, 8), (12, 8), (12,), (8, 12), (8,)))
    sd = {"a.weight": w1, "a.bias": b1, "b.weight": w2, "b.bias": b2}
    assert torch.equal(net.HipBackendMlp.mlp(x, sd, "a.", "b.", "gelu"), F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2))
    assert torch.equal(net.HipBackendMlp.mlp(x, sd, "a.", "b.", "relu"), F.linear(F.relu(F.linear(x, w1, b1)), w2, b2))


# --------------------------------------------------------------------------------------------- wiring equivalence
class _TorchMlp:
    """stand-in backend: mlp in plain torch -- the same operations as the three-node graph"""
    calls = []

    @classmethod
    def mlp(cls, x, sd, p_fc1, p_fc2, act):
        cls.calls.append((p_fc1, p_fc2, act))
        f = {"gelu": F.gelu, "relu": F.relu}[act]
        return F.linear(f(F.linear(x, sd[p_fc1 + "weight"], sd.get(p_fc1 + "bias"))), sd[p_fc2 + "weight"], sd.get(p_fc2 + "bias"))


class _TorchNorms:
    @staticmethod
    def add_layer_norm(x, delta, w, b, eps):
        s = x if delta is None else x + delta
        return s, F.layer_norm(s, s.shape[-1:], w, b, eps)


class _TorchNormsMlp(_TorchNorms, _TorchMlp):
    pass


@pytest.mark.parametrize("norms", [False, True])
def test_vit_backbone_wiring_is_the_same_graph(norms):
    """depth 2: block 0 global, block 1 windowed"""
    from hipie_amd.training import net
    x, sd, cfg = vit_case(torch.float64)
    cfg = dict(cfg, vit_depth=2)
    names = sorted(n for n in sd if not n.startswith("blocks.2."))
    leaves = [x] + [sd[n] for n in names]
    ref = net.vit_backbone(x, sd, "", cfg, _TorchNorms if norms else None)
    _TorchMlp.calls = []
    got = net.vit_backbone(x, sd, "", cfg, _TorchNormsMlp if norms else _TorchMlp)
    assert _TorchMlp.calls == [("blocks.%d.mlp.fc1." % i, "blocks.%d.mlp.fc2." % i, "gelu") for i in range(2)]
    for k in ("res3", "res4", "res5"):
        assert torch.equal(got[k], ref[k]), k
    gr, gg = _grads([ref[k] for k in sorted(ref)], leaves), _grads([got[k] for k in sorted(got)], leaves)
    for n, a, b in zip(["input"] + names, gr, gg):
        assert a is not None and b is not None and torch.equal(a, b), n


class _OracleMsda:
    @staticmethod
    def msda(value, shapes, loc, aw):
        from oracle import ops as oo
        return oo.ms_deform_attn_core(value, shapes, loc, aw)


class _OracleMsdaMlp(_OracleMsda, _TorchMlp):
    pass


class _OracleMsdaNorms(_OracleMsda, _TorchNorms):
    pass


class _OracleMsdaNormsMlp(_OracleMsda, _TorchNorms, _TorchMlp):
    pass


@pytest.mark.parametrize("norms", [False, True])
def test_encoder_layer_wiring_is_the_same_graph(norms):
    from hipie_amd.training import net
    src, pos, refs, shapes, pad, sd = encoder_case(torch.float64, 16)
    names = sorted(sd)
    leaves = [src, pos] + [sd[n] for n in names]
    ref = net.encoder_layer(src, pos, refs, shapes, pad, sd, "", _OracleMsdaNorms if norms else _OracleMsda)
    _TorchMlp.calls = []
    got = net.encoder_layer(src, pos, refs, shapes, pad, sd, "", _OracleMsdaNormsMlp if norms else _OracleMsdaMlp)
    assert _TorchMlp.calls == [("linear1.", "linear2.", "relu")]
    assert torch.equal(got, ref)
    for n, a, b in zip(["src", "pos"] + names, _grads([ref], leaves), _grads([got], leaves)):
        assert a is not None and b is not None and torch.equal(a, b), n
