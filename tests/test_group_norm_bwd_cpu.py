"""CPU: the training GroupNorm (+ ReLU) node below the kernels -- the three entry points of the C ABI and their host refusals (nothing
reaches a launch: the pointers are fake), the float64 statement of the backward (tests/_group_norm_cases.py) against torch.autograd, the
wiring of the 4 + 7 conv + GN blocks of the training net through a backend's `group_norm`, and the composer's second table."""
import ctypes
import os
import re
import sys

import pytest
import torch

from hipie_amd import _lib
from hipie_amd.training import net

from _group_norm_cases import EPS, TorchGroupNorms, backward64, pre_activation64, separated_case, torch_graph, wiring_case

NAMES = ("hipie_group_norm_train_forward", "hipie_group_norm_backward", "hipie_group_norm_backward_ws_bytes")
P = [ctypes.c_void_p(4096 * (k + 1)) for k in range(9)]


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


# ------------------------------------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    c_p, c_i, c_l, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.CONSTANTS["HIPIE_ABI_VERSION"] == 13 and lib.hipie_version() == 13
    assert _lib.SIGNATURES[NAMES[0]] == [c_p] * 6 + [c_i] * 4 + [c_f, c_i, c_p] and _lib.RESTYPES[NAMES[0]] is c_i
    assert _lib.SIGNATURES[NAMES[1]] == [c_p] * 9 + [c_l] + [c_i] * 5 + [c_p] and _lib.RESTYPES[NAMES[1]] is c_i
    assert _lib.SIGNATURES[NAMES[2]] == [c_i] * 3 and _lib.RESTYPES[NAMES[2]] is c_l
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n]


def test_prototypes_cite_the_reference_code_they_replace():
    text = open(_lib.HEADER_PATH).read()
    for n in NAMES[:2]:
        comment = re.findall(r"/\*(.*?)\*/\s*int %s\(" % n, text, flags=re.S)
        assert len(comment) == 1
        last = comment[0].rsplit("/*", 1)[-1]
        assert "Replaces:" in last and "deformable_detr.py:139-160" in last and "maskdino_encoder.py:262-300" in last, n


# ------------------------------------------------------------------------------------------------ host refusals
def _fwd(x=P[0], gamma=P[1], beta=P[2], y=P[3], stat=P[4], ws=P[5], B=2, C=256, HW=64, groups=32, relu=0):
    return [x, gamma, beta, y, stat, ws, B, C, HW, groups, EPS, relu, None]


def _bwd(x=P[0], dy=P[1], stat=P[2], gamma=P[3], beta=P[4], dx=P[5], dgamma=P[6], dbeta=P[7], ws=P[8], ws_bytes=1 << 40, B=2, C=256, HW=64,
         groups=32, relu=1):
    return [x, dy, stat, gamma, beta, dx, dgamma, dbeta, ws, ws_bytes, B, C, HW, groups, relu, None]


def _refused(name, args, message):
    lib = _lib.load()
    assert len(args) == len(_lib.SIGNATURES[name])
    assert getattr(lib, name)(*args) == -22, (name, args)
    assert lib.hipie_last_error() == message, lib.hipie_last_error()


def _accepted(name, args):
    assert getattr(_lib.load(), name)(*args) == 0, (name, _lib.load().hipie_last_error())


GROUPS_MSG = b"%s: %d channels in %d groups unsupported (8 channels per group, 256 %% groups == 0)"
SHAPES = (dict(B=-1), dict(C=0, groups=0), dict(C=-8, groups=-1), dict(HW=0), dict(HW=-64))
BAD_GROUPS = ((256, 0), (256, -32), (256, 16), (260, 32), (1024, 128), (24, 3), (96, 12))
CASES = [("hipie_group_norm_train_forward", _fwd, b"group_norm_train", ("x", "gamma", "beta", "y", "stat", "ws")),
         ("hipie_group_norm_backward", _bwd, b"group_norm_backward", ("x", "dy", "stat", "gamma", "beta", "ws"))]


@pytest.mark.parametrize("entry,make,who,pointers", CASES, ids=["forward", "backward"])
def test_refusals_by_message(entry, make, who, pointers):
    for n in pointers:
        _refused(entry, make(**{n: None}), who + b": null pointer")
    for kw in SHAPES:
        _refused(entry, make(**kw), who + b": bad shape")
    for C, g in BAD_GROUPS:
        _refused(entry, make(C=C, groups=g), GROUPS_MSG % (who, C, g))
    for HW in (1, 63, 68):
        _refused(entry, make(HW=HW), who + b": NCHW needs H*W %% 8 == 0 (got %d)" % HW)
    # the order of the checks: pointers, shape, groups, H*W
    _refused(entry, make(x=None, B=-1), who + b": null pointer")
    _refused(entry, make(B=-1, groups=3), who + b": bad shape")
    _refused(entry, make(groups=3, HW=63), GROUPS_MSG % (who, 256, 3))


def test_backward_pairs_its_parameter_gradients_and_sizes_its_workspace():
    pair = b"group_norm_backward: dgamma and dbeta go together (both or neither)"
    _refused("hipie_group_norm_backward", _bwd(dgamma=None), pair)
    _refused("hipie_group_norm_backward", _bwd(dbeta=None, ws_bytes=0), pair)
    _refused("hipie_group_norm_backward", _bwd(HW=63, dbeta=None), b"group_norm_backward: NCHW needs H*W % 8 == 0 (got 63)")
    need = _lib.load().hipie_group_norm_backward_ws_bytes(2, 256, 64)
    assert need == 2 * 1 * 2 * 256 * 4
    for kw in (dict(), dict(dx=None), dict(dgamma=None, dbeta=None), dict(dx=None, dgamma=None, dbeta=None)):
        _refused("hipie_group_norm_backward", _bwd(ws_bytes=need - 1, **kw), b"group_norm_backward: workspace of %d bytes, need %d" % (need - 1, need))


def test_empty_calls_return_before_a_launch():
    _accepted("hipie_group_norm_train_forward", _fwd(B=0))
    _accepted("hipie_group_norm_backward", _bwd(B=0))
    _accepted("hipie_group_norm_backward", _bwd(B=0, dx=None, dgamma=None, dbeta=None, ws_bytes=16))
    _refused("hipie_group_norm_train_forward", _fwd(B=0, HW=63), b"group_norm_train: NCHW needs H*W % 8 == 0 (got 63)")
    # nothing wanted: nothing is launched (the pointers are fake: a launch would fault or fail)
    need = _lib.load().hipie_group_norm_backward_ws_bytes(2, 256, 64)
    _accepted("hipie_group_norm_backward", _bwd(dx=None, dgamma=None, dbeta=None, ws_bytes=need))


def test_workspace_query_counts_the_chunks_of_a_row():
    """B x chunks x 2 C floats; a row of H*W values is one chunk below 16384 values, then H*W / 8192 of them, at most 64"""
    ws = _lib.load().hipie_group_norm_backward_ws_bytes
    assert ws(0, 256, 64) == 16 and ws(2, 0, 64) == 16 and ws(2, 256, 0) == 16 and ws(-1, 256, 64) == 16
    for B, C in ((1, 8), (2, 256), (3, 512)):
        chunks = [ws(B, C, HW) // (B * 2 * C * 4) for HW in (8, 8192, 16376, 16384, 24584, 65536, 8192 * 64, 8192 * 200)]
        assert chunks == [1, 1, 1, 2, 3, 8, 64, 64] and ws(B, C, 24584) % (B * 2 * C * 4) == 0


def test_ops_refuse_host_tensors():
    from hipie_amd import ops
    x, dy, gamma, beta = separated_case(1, 1, 16)
    stat = torch.zeros(1, 1, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.group_norm_train_forward(x, 1, gamma, beta, EPS)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.group_norm_backward(x, dy, stat, 1, gamma, beta, relu=True)
    from hipie_amd.training import functions
    assert functions.group_norm(x, 1, gamma, beta, EPS, True) is None          # a host tensor is outside the kernels' limits: the torch form runs


# ------------------------------------------------------------------------------------------------ the float64 statement of the backward
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("B,groups,HW", [(1, 1, 8), (2, 1, 16), (3, 2, 16), (2, 32, 8)])
def test_backward64_is_torch_autograd(B, groups, HW, relu):
    x, dy, gamma, beta = separated_case(B, groups, HW)
    pre = pre_activation64(x, gamma, beta, groups)[0]
    assert float(pre.abs().min()) >= 1e-3                                      # no pre-activation near the ReLU's kink
    y, dx, dg, db = torch_graph(x, dy, gamma, beta, groups, EPS, relu, torch.float64)
    got = backward64(x, dy, gamma, beta, groups, EPS, (pre > 0) if relu else None)
    assert torch.equal(y > 0, pre > 0) or not relu
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, (dx, dg, db)):
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= 1e-12, (name, err)


# ------------------------------------------------------------------------------------------------ wiring
def _run_net(be, monkeypatch):
    feats, pad, sd, cfg = wiring_case()
    monkeypatch.setattr(net, "vit_backbone", lambda x, sd_, p, cfg_, be_=None: feats)
    _, srcs, masks, poses = net.backbone_and_projections(torch.zeros(2, 3, 64, 64), pad, sd, cfg, be)
    mf, outs = net.maskdino_pixel_decoder(feats, sd, "detr.mask_dino.pixel_decoder.", cfg, be)
    outputs = list(srcs) + [mf] + list(outs)
    g = torch.Generator().manual_seed(9)
    loss = sum((o * torch.randn(o.shape, generator=g)).sum() for o in outputs)
    leaves = [feats[n] for n in sorted(feats)] + [sd[n] for n in sorted(sd)]
    return outputs, torch.autograd.grad(loss, leaves, allow_unused=True)


def test_the_eleven_sites_ask_the_backend(monkeypatch):
    want_out, want_grad = _run_net(None, monkeypatch)
    be = TorchGroupNorms()
    got_out, got_grad = _run_net(be, monkeypatch)
    assert len(be.calls) == 4 + 7 and [c[3] for c in be.calls].count(True) == 2
    assert [c[3] for c in be.calls[-2:]] == [True, True] and all(c[1] == 32 and c[2] == 1e-5 for c in be.calls)
    assert be.calls[-1][0] == (2, 32, 16, 16)                                   # mask_features: the transposed convolution's 2 x map
    assert len(got_out) == len(want_out) and all(torch.equal(a, b) for a, b in zip(got_out, want_out))
    assert sum(g is None for g in want_grad) == 1 and len(want_grad) == 48        # every leaf but level_embed (no encoder layer reads the positions)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got_grad, want_grad))


def test_a_backend_that_declines_falls_back(monkeypatch):
    class Declines(TorchGroupNorms):
        def group_norm(self, *a):
            self.calls.append(a[-1])
            return None
    want_out, _ = _run_net(None, monkeypatch)
    be = Declines()
    got_out, _ = _run_net(be, monkeypatch)
    assert len(be.calls) == 11 and all(torch.equal(a, b) for a, b in zip(got_out, want_out))


# ------------------------------------------------------------------------------------------------ composer
def _public(cls):
    return {n for n in dir(cls) if not n.startswith("_")}


def test_composer_takes_the_extra_group_last():
    assert list(net.EXTRA_GROUPS) == ["group_norms"] and net.EXTRA_GROUPS["group_norms"] is net.HipBackendGroupNorms
    assert "group_norms" not in net.GROUPS and issubclass(net.HipBackendGroupNorms, net.HipBackend)
    assert net.backend("group_norms") is net.HipBackendGroupNorms and net.backend("group_norms", "group_norms") is net.HipBackendGroupNorms
    assert _public(net.HipBackendGroupNorms) - _public(net.HipBackend) == {"group_norm"}
    every = net.backend(*net.GROUPS)
    assert every.__bases__ == (net.HipBackendNorms, net.HipBackendMlp, net.HipBackendPackedWindows, net.HipBackendDeformable, net.HipBackendPairLosses)
    both = net.backend(*net.GROUPS, "group_norms")
    assert both.__bases__ == every.__bases__ + (net.HipBackendGroupNorms,) and net.backend("group_norms", *net.GROUPS) is both
    assert _public(both) == _public(every) | {"group_norm"} and both.group_norm is net.HipBackendGroupNorms.group_norm
    assert net.backend(*net.GROUPS) is every                                     # composing with the extra group left the plain one alone
    assert net.backend("norms", "group_norms").__bases__ == (net.HipBackendNorms, net.HipBackendGroupNorms)
    with pytest.raises(ValueError, match="'fused'.*known: norms, mlp, windows, .*pair_losses, group_norms"):
        net.backend("group_norms", "fused")


def test_bench_train_step_consumes_the_new_flag():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from bench_train_step import EXTRA_FLAGS, FLAGS, backend_names
    assert EXTRA_FLAGS == {"--fused-group-norms": "group_norms"} and "--fused-group-norms" not in FLAGS
    assert list(FLAGS.values()) == list(net.GROUPS) and list(EXTRA_FLAGS.values()) == list(net.EXTRA_GROUPS)
    names, rest = backend_names(["2", "--fused-group-norms", "4"])
    assert names == ["group_norms"] and rest == ["2", "4"]
    names, rest = backend_names(["2", "--hand-norms", "--fused-group-norms", "--fused-mlp", "4"])
    assert names == ["norms", "group_norms", "mlp"] and rest == ["2", "4"]
    assert net.backend(*names).__bases__ == (net.HipBackendNorms, net.HipBackendMlp, net.HipBackendGroupNorms)
