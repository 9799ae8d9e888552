"""CPU: the LayerNorm backward operator (hipie_layernorm_backward) up to where a device is needed -- its ABI surface and host-side
refusals, the CPU refusal of the op, and the training net's wiring: a backend with ``add_layer_norm`` regroups the residual adds and
the LayerNorms of vit_backbone / encoder_layer without changing one operation, so with a plain-torch stand-in the outputs and every
gradient are EQUAL to the un-grouped graph's."""
import ctypes
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
NAMES = ("hipie_layernorm_backward", "hipie_layernorm_backward_ws_bytes")


def test_abi_surface():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipie_mi355.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hipie_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.hipie_version() == 13
    # the citation of the replaced reference code
    head = open(os.path.join(ROOT, "include", "hipie_mi355.h")).read()
    doc = head[:head.index("int hipie_layernorm_backward(")].rsplit("/*", 1)[1]
    assert "torch.nn.LayerNorm" in doc and "backbone/vit.py" in doc and "deformable_transformer_dino.py:384-394" in doc


def test_host_refusals_without_a_launch():
    lib = _lib.load()
    p, q, r = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(1024)
    big = 1 << 40

    def call(s=p, gy=q, gres=None, gamma=p, dx=r, dgamma=p, dbeta=p, ws=p, ws_bytes=big, rows=8, C=256):
        return lib.hipie_layernorm_backward(s, gy, gres, gamma, dx, dgamma, dbeta, ws, ws_bytes, rows, C, 1e-5, None)

    def refused(word, **kw):
        assert call(**kw) == -22, kw
        msg = lib.hipie_last_error()
        assert b"layernorm_backward" in msg and word in msg, (kw, msg)
    for name in ("s", "gy", "gamma", "dx"):
        refused(b"null", **{name: None})
    refused(b"go together", dgamma=None)
    refused(b"go together", dbeta=None)
    for C in (6, 250, 2052, 4096, 0, -4):
        refused(b"C=%d" % C, C=C)
    need = lib.hipie_layernorm_backward_ws_bytes(8, 256)
    refused(b"workspace", ws_bytes=need - 1)
    refused(b"workspace", ws_bytes=0)
    refused(b"workspace", ws=None)
    refused(b"alias", dx=p)                     # dx == s
    refused(b"alias", dx=q)                     # dx == gy
    refused(b"alias", dx=q, dgamma=None, dbeta=None, ws=None, ws_bytes=0)
    # empty work is a no-op even with null data pointers
    assert lib.hipie_layernorm_backward(None, None, None, None, None, None, None, None, 0, 0, 256, 1e-5, None) == 0


def test_workspace_query():
    lib = _lib.load()
    ws = lib.hipie_layernorm_backward_ws_bytes
    assert isinstance(ws(5, 256), int)
    for rows in (1, 2, 4, 5, 64, 257, 4096, 4097, 43520, 10 ** 6, 10 ** 9, 2 ** 40):
        for C in (4, 256, 1280, 2048):
            b = ws(rows, C)
            assert b > 0 and b == ws(rows, C)
            assert b >= ws(max(rows - 1, 1), C)                  # monotone in rows
            assert b % (2 * C * 4) == 0                          # whole partial rows of 2 C floats
    assert ws(8192, 1280) >= ws(8191, 1280) >= ws(1, 1280) > 0
    # the fixed grid: the number of partial rows saturates, and where it does depends on rows alone
    sat = ws(2 ** 40, 256) // (2 * 256 * 4)
    assert sat == ws(2 ** 40, 2048) // (2 * 2048 * 4) == ws(10 ** 9, 4) // (2 * 4 * 4) and 64 <= sat <= 65536


def test_op_refuses_cpu_tensors():
    from hipie_amd import ops
    s, gy, w = torch.zeros(3, 8), torch.zeros(3, 8), torch.ones(8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.layernorm_backward(s, gy, w, 1e-5)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.layernorm_backward(s, gy, w, 1e-5, gres=torch.zeros(3, 8), want_param_grads=False)


def test_hip_backend_norms_is_opt_in():
    from hipie_amd.training import net
    from hipie_amd.training.step import TrainStep
    import inspect
    assert issubclass(net.HipBackendNorms, net.HipBackend) and not hasattr(net.HipBackend, "add_layer_norm")
    assert callable(net.HipBackendNorms.add_layer_norm)
    assert inspect.signature(TrainStep.__init__).parameters["backend"].default is None       # None -> HipBackend (step.py)
    from hipie_amd.training import functions
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):                     # no host path behind the backend either
        net.HipBackendNorms.add_layer_norm(torch.zeros(2, 8), torch.zeros(2, 8), torch.ones(8), torch.zeros(8), 1e-5)
    assert functions.add_layer_norm is not None


# --------------------------------------------------------------------------------------------- wiring equivalence
class _TorchNorms:
    """stand-in backend: add_layer_norm in plain torch -- the same operations as the un-grouped graph, only regrouped"""
    calls = []

    @classmethod
    def add_layer_norm(cls, x, delta, w, b, eps):
        cls.calls.append((delta is None, eps))
        s = x if delta is None else x + delta
        return s, F.layer_norm(s, s.shape[-1:], w, b, eps)


def test_vit_backbone_wiring_is_the_same_graph():
    from hipie_amd.training import net
    x, sd, cfg = vit_case(torch.float64)
    names = sorted(sd)
    leaves = [x] + [sd[n] for n in names]
    ref = net.vit_backbone(x, sd, "", cfg, None)
    _TorchNorms.calls = []
    got = net.vit_backbone(x, sd, "", cfg, _TorchNorms)
    # 2 norms per block, all through the backend: the first takes no delta, every other one carries the residual add in front of it
    assert _TorchNorms.calls == [(True, 1e-6)] + [(False, 1e-6)] * (2 * cfg["vit_depth"] - 1)
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


class _OracleMsdaNorms(_OracleMsda, _TorchNorms):
    pass


def test_encoder_layer_wiring_is_the_same_graph():
    from hipie_amd.training import net
    src, pos, refs, shapes, pad, sd = encoder_case(torch.float64, 16)
    names = sorted(sd)
    leaves = [src, pos] + [sd[n] for n in names]
    ref = net.encoder_layer(src, pos, refs, shapes, pad, sd, "", _OracleMsda)
    _TorchNorms.calls = []
    got = net.encoder_layer(src, pos, refs, shapes, pad, sd, "", _OracleMsdaNorms)
    assert _TorchNorms.calls == [(False, 1e-5), (False, 1e-5)]
    assert torch.equal(got, ref)
    for n, a, b in zip(["src", "pos"] + names, _grads([ref], leaves), _grads([got], leaves)):
        assert a is not None and b is not None and torch.equal(a, b), n
