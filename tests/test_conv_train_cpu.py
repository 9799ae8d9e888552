"""CPU: the training 3 x 3 convolution (+ ReLU) node below the kernels -- the float64 statement of its backward on the padded grid
(tests/_conv_train_cases.py) against torch.autograd, the composer's table, the limits the node declines, the wiring of the convolution
sites of the training net through a backend's `conv3x3`, and the host refusals of hipie_conv3x3_wgrad (nothing reaches a launch: the
pointers are fake)."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from hipie_amd import _lib
from hipie_amd.training import functions, net

from _conv_train_cases import CHUNK, IDS, SHAPES, backward64, inputs, pre_activation64, separated_case, torch_graph

ENTRY = "hipie_conv3x3_wgrad"
P = [ctypes.c_void_p(4096 * (k + 1)) for k in range(6)]


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


def _err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ the formulation
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward64_is_autograd_of_conv2d_in_double(shape):
    """the padded-grid algebra -- flipped / swapped weight for dx, tap-shifted row contraction for dW, row sum for db, zero border -- equals
    torch.autograd.grad of F.conv2d (+ F.relu) in double to 1e-12, and so does its forward"""
    x, dy, w, b = inputs(*shape)
    pre = pre_activation64(x, w, b)
    for relu in (False, True):
        y, dx, dw, db = torch_graph(x, dy, w, b, relu, torch.float64)
        assert _err(pre.relu() if relu else pre, y) < 1e-12
        got = backward64(x, dy, w, (pre > 0) if relu else None)
        for name, g, r in zip(("dx", "dW", "db"), got, (dx, dw, db)):
            assert g.shape == r.shape and _err(g, r) < 1e-12, (name, relu, _err(g, r))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_separated_case_exists(shape):
    x, dy, w, b = separated_case(*shape)
    pre = pre_activation64(x, w, b)
    assert float(pre.abs().min()) >= 1e-3 and 0 < int((pre > 0).sum()) < pre.numel()
    assert all(t.dtype == torch.float32 for t in (x, dy, w, b))


def test_the_last_shape_is_ragged_over_more_than_two_chunks():
    B, _, _, H, W = SHAPES[-1]
    rows = B * (H + 2) * (W + 2)
    assert rows > 2 * CHUNK and rows % CHUNK and rows % 64
    from hipie_amd import ops
    assert ops.CONV_WGRAD_CHUNK == CHUNK


# ------------------------------------------------------------------------------------------------ the composer
def test_convs_joins_the_later_groups_and_composes():
    """fails on a tree without the group with net.backend's ValueError"""
    be = net.backend("convs")
    assert be is net.HipBackendConvs and callable(be.conv3x3) and issubclass(be, net.HipBackend)
    later = list(net.LATER_GROUPS)
    assert "convs" in later and later.index("convs") > later.index("fusion_attention")
    assert net.backend() is net.HipBackend and not hasattr(net.HipBackend, "conv3x3")
    others = ["norms", "mlp", "packed_windows", "deformable", "pair_losses", "group_norms", "query_attention", "fusion_attention"]
    every = net.backend("convs", *others)
    assert every is net.backend(*others, "convs") is net.backend(*reversed(others + ["convs"]))
    assert every.conv3x3 is net.HipBackendConvs.conv3x3 and every.__mro__[-2] is net.HipBackend
    known = {**net.GROUPS, **net.EXTRA_GROUPS, **net.LATER_GROUPS}
    for n in known:
        if n == "convs":
            continue
        for pair in itertools.permutations(("convs", n)):
            c = net.backend(*pair)
            assert issubclass(c, net.HipBackendConvs) and issubclass(c, known[n]) and c.conv3x3 is net.HipBackendConvs.conv3x3
    with pytest.raises(ValueError):
        net.backend("conv")


# ------------------------------------------------------------------------------------------------ the limits
def test_node_declines_what_the_kernels_do_not_take():
    x = torch.randn(2, 64, 6, 6)
    w, b = torch.randn(32, 64, 3, 3), torch.randn(32)
    ok = functions.conv3x3_train_ok
    assert not ok(x, w, b, stride=2) and not ok(x, w, b, stride=(2, 2))
    assert not ok(x, torch.randn(32, 64, 1, 1), b, padding=0) and not ok(x, torch.randn(32, 64, 1, 1), b)
    assert not ok(x, torch.randn(32, 32, 3, 3), b, groups=2)
    assert not ok(x, torch.randn(8, 64, 3, 3), torch.randn(8))
    assert not ok(x.half(), w.half(), b.half()) and not ok(x, w.half(), b) and not ok(x, w, b.half())
    assert not ok(x, w, b, padding=0) and not ok(x, w, b, dilation=2) and not ok(torch.randn(2, 48, 6, 6), torch.randn(32, 48, 3, 3), b)
    assert not ok(x, w, b)                                              # host tensors: the node is for the device
    assert functions.conv3x3_train(x, w, b, True) is None and functions.conv3x3_train(x, w, b, False, stride=2) is None


# ------------------------------------------------------------------------------------------------ the wiring
class _TorchConvs:
    """a plain-torch stand-in for net.HipBackendConvs that records its calls and declines Cout % 32 != 0"""

    def __init__(self):
        self.calls = []

    def conv3x3(self, x, weight, bias, relu):
        self.calls.append((tuple(weight.shape), bias is not None, relu))
        if weight.shape[0] % 32:
            return None
        y = F.conv2d(x, weight, bias, padding=1)
        return F.relu(y) if relu else y


def test_the_3x3_sites_ask_the_backend_and_keep_their_values():
    g = torch.Generator().manual_seed(2)
    p = "detr.mask_head."
    sd = {}
    for name, (n, c) in dict(lay3=(32, 32), lay4=(32, 32), jia_dcn=(32, 32), lay1=(64, 32), lay2=(8, 64)).items():
        sd[p + name + ".weight"] = torch.randn(n, c, 3, 3, generator=g) * 0.1
        sd[p + name + ".bias"] = torch.randn(n, generator=g) * 0.1
    feats = [torch.randn(2, 32, s, s, generator=g) for s in (8, 4, 2)]
    be = _TorchConvs()
    got = net.mask_head_small_conv(feats, sd, p, be)
    assert torch.equal(got, net.mask_head_small_conv(feats, sd, p)) and got.shape == (2, 8, 8, 8) and bool((got >= 0).all())
    assert be.calls == [((32, 32, 3, 3), True, True)] * 3 + [((64, 32, 3, 3), True, True), ((8, 64, 3, 3), True, True)]
    # conv(): only 3 x 3 / stride 1 / padding 1 sites reach the op; the declined site runs F.conv2d + F.relu
    be = _TorchConvs()
    x = feats[0]
    sd["s.weight"], sd["s.bias"] = torch.randn(32, 32, 3, 3, generator=g), None
    assert torch.equal(net.conv(x, sd, "s.", stride=2, padding=1, be=be), F.conv2d(x, sd["s.weight"], None, stride=2, padding=1)) and not be.calls
    assert torch.equal(net.conv(x, sd, "s.", padding=1, be=be), F.conv2d(x, sd["s.weight"], None, padding=1))
    assert be.calls == [((32, 32, 3, 3), False, False)]


# ------------------------------------------------------------------------------------------------ host refusals of the entry
def _args(x=P[0], ldx=64, dy=P[1], ldg=32, y=P[2], rows=100, Wp=10, C=64, N=32, dw=P[3], db=P[4], ws=P[5], ws_bytes=1 << 40):
    return [x, ldx, dy, ldg, y, rows, Wp, C, N, dw, db, ws, ws_bytes, None]


def _refused(args, message):
    lib = _lib.load()
    assert len(args) == len(_lib.SIGNATURES[ENTRY])
    assert getattr(lib, ENTRY)(*args) == -22, args
    assert lib.hipie_last_error() == message, lib.hipie_last_error()


def test_entry_is_declared_and_refuses_on_the_host():
    c_p, c_i, c_l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib.SIGNATURES[ENTRY] == [c_p, c_l, c_p, c_l, c_p, c_l, c_i, c_i, c_i, c_p, c_p, c_p, c_l, c_p] and _lib.RESTYPES[ENTRY] is c_i
    for n in ("x", "dy", "dw", "ws"):
        _refused(_args(**{n: None}), b"conv3x3_wgrad: null pointer")
    for kw in (dict(C=48), dict(C=0), dict(N=8), dict(N=40), dict(rows=0), dict(rows=1 << 31), dict(Wp=2)):
        a = _args(**kw)
        _refused(a, b"conv3x3_wgrad: rows=%d Wp=%d C=%d N=%d (C %% 32, N %% 32)" % (a[5], a[6], a[7], a[8]))
    for kw in (dict(ldx=32), dict(ldx=66), dict(ldg=16), dict(ldg=34)):
        a = _args(**kw)
        _refused(a, b"conv3x3_wgrad: row strides %d / %d (>= C / N, multiples of 4)" % (a[1], a[3]))
    for n in ("x", "dy", "y", "dw", "db", "ws"):
        _refused(_args(**{n: ctypes.c_void_p(4096 + 4)}), b"conv3x3_wgrad: pointers must be 16-byte aligned")
    need = 1 * (9 * 64 * 32 + 32) * 4
    _refused(_args(ws_bytes=need - 1), b"conv3x3_wgrad: workspace of %d bytes, need %d" % (need - 1, need))
    _refused(_args(ws_bytes=3 * need - 1, rows=2 * CHUNK + 1, db=None), b"conv3x3_wgrad: workspace of %d bytes, need %d" % (3 * need - 1, 3 * need))
