"""CPU: the training projection node (functions.PatchConvFunction) without a device -- the float64 algebra of tests/_patch_conv_cases.py
against torch's float64 autograd (pins the column order and the 2-D weight views), the host refusals of ops_patch, patch_rows_view's
layouts, the composer, the limits patch_conv_train_ok names, and the wiring of the sites in training/net.py."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from _patch_conv_cases import IDS, SHAPES, algebra64, frozen_input, gather, inputs, scatter, torch_graph
from hipie_amd import ops, ops_patch
from hipie_amd.training import functions, net


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


def _err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_float64_algebra_is_torchs_float64_autograd(shape):
    """float64 against float64: 1e-13 is ~500 roundings of 2^-53 for contractions of at most 2304 terms"""
    x, dy, w, b = inputs(shape)
    got, want = algebra64(shape, x, dy, w, b), torch_graph(shape, x, dy, w, b, torch.float64)
    for name, g, t in zip(("y", "dx", "dW", "db"), got, want):
        assert g.shape == t.shape and g.dtype == torch.float64, name
        assert _err(g, t) <= 1e-13, (name, _err(g, t))


def test_gather_and_scatter_are_inverse_and_ordered():
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).view(2, 3, 4, 6)
    r = gather(x, 2)
    assert r.shape == (2 * 2 * 3, 3 * 4) and torch.equal(scatter(r, 2, 3, 4, 6, 2), x)
    # row (b=1, h=1, w=2), column c=2, i=1, j=0
    assert r[(1 * 2 + 1) * 3 + 2, 2 * 4 + 1 * 2 + 0] == x[1, 2, 2 * 1 + 1, 2 * 2 + 0]
    assert [frozen_input(s) for s in SHAPES] == [False] * 6 + [True]


# ------------------------------------------------------------------------------------------------ the op layer on the host
@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda name, *a: pytest.fail("%s reached the library" % name))
    monkeypatch.setattr(ops, "_size", lambda name, *a: pytest.fail("%s reached the library" % name))


def test_host_tensors_are_refused_with_the_one_wording(no_library):
    x = torch.randn(1, 32, 4, 4)
    with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \(patch_pack: x must be a CUDA/HIP tensor\)"):
        ops_patch.patch_pack(x, 1)
    with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \(patch_pack: x must be a CUDA/HIP tensor\)"):
        ops_patch.patch_pack(x, 2, want_f32=True, want_rows=False, want_t=False, want_sum=True)
    import inspect
    wrappers = [n for n, f in vars(ops_patch).items()
                if inspect.isfunction(f) and not n.startswith("_") and "_call(" in inspect.getsource(inspect.unwrap(f))]
    assert wrappers == ["patch_pack"]                        # every wrapper that reaches the library; patch_rows_view only makes a view
    assert "Not implemented on the CPU" not in inspect.getsource(ops_patch)          # the wording stays the one of ops.py


def test_patch_rows_view_returns_a_view_or_none():
    view = ops_patch.patch_rows_view
    cl = torch.randn(2, 3, 5, 32).permute(0, 3, 1, 2)                       # channels-last dense
    r = view(cl)
    assert r is not None and r.shape == (30, 32) and r.stride() == (32, 1) and r.data_ptr() == cl.data_ptr()
    assert torch.equal(r, gather(cl, 1))
    wide = torch.randn(2, 3, 5, 48)[..., :32].permute(0, 3, 1, 2)           # pixel stride 48 >= C, a multiple of 4
    r = view(wide)
    assert r is not None and r.stride() == (48, 1) and torch.equal(r, gather(wide, 1))
    one = torch.randn(1, 32, 1, 1)                                          # one pixel: NCHW and channels-last at once
    assert view(one) is not None and view(one).shape == (1, 32)
    assert view(torch.randn(2, 32, 3, 5)) is None                           # NCHW
    assert view(cl, 2) is None and view(cl.double()) is None
    assert view(torch.randn(2, 3, 5, 34)[..., :32].permute(0, 3, 1, 2)) is None                 # pixel stride 34: not a multiple of 4
    assert view(torch.randn(2, 3, 5, 36)[..., 1:33].permute(0, 3, 1, 2)) is None                # base off 16 bytes
    assert view(torch.randn(2, 3, 6, 32)[:, :, :5].permute(0, 3, 1, 2)) is None                 # the row stride is not W pixel strides
    assert view(torch.randn(3, 3, 5, 32)[::2].permute(0, 3, 1, 2)) is None                      # the image stride is not H row strides


# ------------------------------------------------------------------------------------------------ the composer
def test_projections_joins_the_later_groups_and_composes():
    """fails on a tree without the group with net.backend's ValueError"""
    be = net.backend("projections")
    assert be is net.HipBackendProjections and issubclass(be, net.HipBackend)
    assert callable(be.conv_patch) and callable(be.convt2x2)
    later = list(net.LATER_GROUPS)
    assert "projections" in later and later.index("projections") > later.index("scaled_grads")
    assert not hasattr(net.HipBackend, "conv_patch") and not hasattr(net.HipBackend, "convt2x2")
    known = {**net.GROUPS, **net.EXTRA_GROUPS, **net.LATER_GROUPS}
    every = net.backend(*known)
    bases = every.__bases__
    assert bases[-2:] == (net.HipBackendQueryAttention, net.HipBackendFusionAttention) and net.HipBackendProjections in bases[:-2]
    assert every.conv_patch is net.HipBackendProjections.conv_patch and every.convt2x2 is net.HipBackendProjections.convt2x2
    for n, cls in known.items():
        if n == "projections":
            continue
        assert "conv_patch" not in vars(cls) and "convt2x2" not in vars(cls) and not hasattr(cls, "conv_patch"), n
        for pair in itertools.permutations(("projections", n)):
            c = net.backend(*pair)
            assert issubclass(c, net.HipBackendProjections) and issubclass(c, cls) and c.conv_patch is net.HipBackendProjections.conv_patch
    half = net.half_policy(be)
    assert half.conv_patch is be.conv_patch and "split" in be.__doc__.lower() and "half_policy" in be.__doc__


def test_the_bench_flag_names_the_group():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from bench_train_step import LATER_FLAGS, backend_names
    assert LATER_FLAGS["--fused-projections"] == "projections"
    assert backend_names(["2", "--fused-projections", "--fused-convs"]) == (["projections", "convs"], ["2"])


# ------------------------------------------------------------------------------------------------ the limits
class _Dev:
    """a host tensor that answers is_cuda: the predicate's other limits can be walked without a device"""

    def __init__(self, t):
        self.t = t

    def __getattr__(self, n):
        return True if n == "is_cuda" else getattr(self.t, n)


def test_predicate_declines_each_limit():
    ok = functions.patch_conv_train_ok
    d = _Dev
    x, w, b = torch.randn(2, 64, 4, 6), torch.randn(32, 64, 1, 1), torch.randn(32)
    assert ok(d(x), d(w), d(b)) and ok(d(x), d(w), None) and ok(d(x), d(torch.randn(32, 64, 2, 2)), d(b), stride=2)
    assert not ok(x, w, b) and not ok(d(x), w, d(b)) and not ok(d(x), d(w), b)                     # host tensors
    assert not ok(d(x.half()), d(w.half()), d(b.half())) and not ok(d(x), d(w.half()), d(b)) and not ok(d(x), d(w), d(b.half()))
    assert not ok(d(x), d(torch.randn(32, 64, 3, 3)), d(b)) and not ok(d(x), d(torch.randn(32, 64, 3, 3)), d(b), padding=1)        # 3 x 3
    assert not ok(d(x), d(w), d(b), stride=2) and not ok(d(x), d(torch.randn(32, 64, 2, 2)), d(b)) and not ok(d(x), d(w), d(b), stride=(1, 2))
    assert not ok(d(x), d(w), d(b), padding=1) and not ok(d(x), d(w), d(b), dilation=2)
    assert not ok(d(x), d(torch.randn(32, 32, 1, 1)), d(b), groups=2)
    assert not ok(d(torch.randn(2, 80, 4, 6)), d(torch.randn(32, 80, 1, 1)), d(b))                  # Cin k^2 % 32
    assert not ok(d(x), d(torch.randn(40, 64, 1, 1)), d(torch.randn(40)))                           # Cout % 32
    assert not ok(d(torch.randn(2, 64, 5, 6)), d(torch.randn(32, 64, 2, 2)), d(b), stride=2)        # k does not divide H
    assert not ok(d(x), d(torch.randn(32, 64, 1, 2)), d(b))                                         # not square
    # the transposed form: kernel 2, stride 2, Cin % 32, Cout % 8, no output padding
    wt, bt = torch.randn(64, 8, 2, 2), torch.randn(8)
    assert ok(d(x), d(wt), d(bt), stride=2, transposed=True) and ok(d(torch.randn(2, 64, 3, 5)), d(wt), d(bt), stride=2, transposed=True)      # any grid
    assert not ok(d(x), d(wt), d(bt), stride=2, output_padding=1, transposed=True) and not ok(d(x), d(wt), d(bt), stride=1, transposed=True)
    assert not ok(d(x), d(torch.randn(64, 12, 2, 2)), d(torch.randn(12)), stride=2, transposed=True)
    assert not ok(d(torch.randn(2, 80, 4, 6)), d(torch.randn(80, 8, 2, 2)), d(bt), stride=2, transposed=True)
    assert not ok(d(x), d(torch.randn(64, 8, 4, 4)), d(bt), stride=4, transposed=True) and not ok(x, wt, bt, stride=2, transposed=True)
    assert functions.patch_conv_train(x, w, b) is None and functions.patch_convt_train(x, wt, bt) is None


# ------------------------------------------------------------------------------------------------ the wiring
class _TorchProjections:
    """a plain-torch stand-in for net.HipBackendProjections that records its calls and declines Cin % 32 != 0"""

    def __init__(self):
        self.calls = []

    def conv_patch(self, x, weight, bias, stride):
        self.calls.append(("conv", tuple(weight.shape), bias is not None, stride))
        return None if weight.shape[1] * weight.shape[2] ** 2 % 32 else F.conv2d(x, weight, bias, stride=stride)

    def convt2x2(self, x, weight, bias):
        self.calls.append(("convt", tuple(weight.shape), bias is not None, 2))
        return None if weight.shape[0] % 32 else F.conv_transpose2d(x, weight, bias, stride=2)


def test_the_helpers_ask_the_backend_first_and_fall_back():
    g = torch.Generator().manual_seed(4)
    be = _TorchProjections()
    x = torch.randn(2, 32, 4, 6, generator=g)
    sd = {"a.weight": torch.randn(64, 32, 1, 1, generator=g), "a.bias": torch.randn(64, generator=g),
          "s.weight": torch.randn(64, 32, 3, 3, generator=g), "s.bias": torch.randn(64, generator=g)}
    want = F.conv2d(x, sd["a.weight"], sd["a.bias"])
    assert torch.equal(net.conv(x, sd, "a.", be=be), want) and torch.equal(net.conv(x, sd, "a."), want)
    assert torch.equal(net.conv(x, sd, "a.", be=be, relu=True), F.relu(want))
    assert len(be.calls) == 2 and be.calls[0] == ("conv", (64, 32, 1, 1), True, 1)
    net.conv(x, sd, "s.", stride=2, padding=1, be=be)                    # the stride-2 3 x 3 site is not asked
    net.conv(x, sd, "s.", padding=1, be=be)
    assert len(be.calls) == 2
    w80 = torch.randn(64, 80, 1, 1, generator=g)
    x80 = torch.randn(2, 80, 4, 6, generator=g)
    assert torch.equal(net.conv_patch(x80, w80, None, 1, be), F.conv2d(x80, w80)) and be.calls[-1] == ("conv", (64, 80, 1, 1), False, 1)
    wt, bt = torch.randn(32, 8, 2, 2, generator=g), torch.randn(8, generator=g)
    want = F.conv_transpose2d(x, wt, bt, stride=2)
    assert torch.equal(net.convt2x2(x, wt, bt, be), want) and torch.equal(net.convt2x2(x, wt, bt), want)
    w80t = torch.randn(80, 8, 2, 2, generator=g)
    assert torch.equal(net.convt2x2(x80, w80t, bt, be), F.conv_transpose2d(x80, w80t, bt, stride=2))          # declined: the library call runs
    assert [c[0] for c in be.calls[-2:]] == ["convt", "convt"]


def test_every_projection_site_of_net_goes_through_the_helpers():
    """no F.conv2d / F.conv_transpose2d call is left outside conv, conv_patch and convt2x2 -- but the patch embedding's, which the group
    does not route (HipBackendProjections says why)"""
    import inspect
    import re
    src = inspect.getsource(net)
    for fn in (net.conv, net.conv_patch, net.convt2x2):
        src = src.replace(inspect.getsource(fn), "")
    left = re.findall(r"^.*(?:F\.conv2d\(|F\.conv_transpose2d\().*$", src, flags=re.M)
    assert len(left) == 1 and "patch_embed.proj.weight" in left[0], left
