"""CPU: the host side of the loss kernels (csrc/point_loss.hip) -- the refusals of the four entry points through the C ABI (no launch), the
ops refusing host tensors, and the `ops` plumbing of DetCriterion / MaskCriterion: with a float64 torch object plugged in, the criteria must
give the loss dictionary and the input gradients of ops=None (the un-gathered targets + flat index against the gather), and ops=None must
be the criterion constructed without the argument, bit for bit."""
import ctypes

import pytest
import torch

from _loss_cases import TorchLossOps
from hipie_amd import _lib
from hipie_amd.training.criterion import DetCriterion, MaskCriterion


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


P_ = ctypes.c_void_p(256)


def _fwd(lib, src=P_, tgt=P_, idx=P_, pts=P_, lmask=P_, ldice=P_, sums=P_, ws=P_, ws_bytes=1 << 20, N=2, H=8, W=8, T=3, Ht=8, Wt=8, P=5, mode=0,
         alpha=0.25, gamma=2.0):
    return lib.hipie_point_mask_loss_forward(src, tgt, idx, pts, lmask, ldice, sums, ws, ws_bytes, N, H, W, T, Ht, Wt, P, mode, alpha, gamma, None)


def _bwd(lib, src=P_, tgt=P_, idx=P_, pts=P_, sums=P_, gm=P_, gd=P_, d_src=ctypes.c_void_p(512), N=2, H=8, W=8, T=3, Ht=8, Wt=8, P=5, mode=0,
         alpha=0.25, gamma=2.0):
    return lib.hipie_point_mask_loss_backward(src, tgt, idx, pts, sums, gm, gd, d_src, N, H, W, T, Ht, Wt, P, mode, alpha, gamma, None)


def _tf_fwd(lib, logits=P_, onehot=P_, keep=P_, out=P_, ws=P_, ws_bytes=1 << 20, B=2, Q=3, T=5, alpha=0.25, gamma=2.0):
    return lib.hipie_token_focal_forward(logits, onehot, keep, out, ws, ws_bytes, B, Q, T, alpha, gamma, None)


def _tf_bwd(lib, logits=P_, onehot=P_, keep=P_, g=P_, dlogits=P_, B=2, Q=3, T=5, alpha=0.25, gamma=2.0):
    return lib.hipie_token_focal_backward(logits, onehot, keep, g, dlogits, B, Q, T, alpha, gamma, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_point_mask_loss_refusals_without_a_launch(call):
    """one violated condition per call; every one returns -22 with a message before anything is launched"""
    lib = _lib.load()
    for kw, msg in (({"src": None}, b"null"), ({"tgt": None}, b"null"), ({"idx": None}, b"null"), ({"pts": None}, b"null"),
                    ({"P": 0}, b"P=0"), ({"P": -3}, b"P=-3"),
                    ({"H": 1 << 16, "W": 1 << 15}, b"H*W=2147483648"), ({"Ht": 1 << 15, "Wt": 1 << 16}, b"Ht*Wt=2147483648"),
                    ({"gamma": 1.5}, b"gamma=1.5"), ({"mode": 2}, b"mode=2"), ({"mode": -1}, b"mode=-1")):
        assert call(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    out_args = ("lmask", "ldice", "sums", "ws") if call is _fwd else ("sums", "gm", "gd", "d_src")
    for name in out_args:
        assert call(lib, **{name: None}) == -22 and b"null" in lib.hipie_last_error(), name
    # one element below the limit passes the size checks (they come after mode and gamma, before the pointers) and trips the null pointer
    assert call(lib, H=(1 << 16) - 1, W=1 << 15, src=None) == -22 and b"null" in lib.hipie_last_error()
    assert call(lib, Ht=1 << 15, Wt=(1 << 16) - 1, src=None) == -22 and b"null" in lib.hipie_last_error()


def test_point_mask_loss_workspace_and_noop():
    lib = _lib.load()
    need = lib.hipie_point_mask_loss_ws_bytes(2, 5)
    assert need >= 2 * 16 and lib.hipie_point_mask_loss_ws_bytes(2, 1 << 20) > need
    assert _fwd(lib, ws_bytes=need - 1) == -22 and b"workspace" in lib.hipie_last_error()
    # N = 0: no launch, null data pointers allowed, whatever P is
    assert lib.hipie_point_mask_loss_forward(None, None, None, None, None, None, None, None, 0, 0, 8, 8, 3, 8, 8, 0, 1, 0.25, 2.0, None) == 0
    assert lib.hipie_point_mask_loss_backward(None, None, None, None, None, None, None, None, 0, 8, 8, 3, 8, 8, 0, 0, -1.0, 2.0, None) == 0
    assert lib.hipie_point_mask_loss_ws_bytes(0, 5) > 0


def test_token_focal_refusals_and_noop():
    lib = _lib.load()
    for call, outs in ((_tf_fwd, ("out", "ws")), (_tf_bwd, ("g", "dlogits"))):
        for name in ("logits", "onehot") + outs:
            assert call(lib, **{name: None}) == -22 and b"null" in lib.hipie_last_error(), name
        assert call(lib, gamma=3.0) == -22 and b"gamma=3" in lib.hipie_last_error()
    assert _tf_fwd(lib, ws_bytes=lib.hipie_token_focal_ws_bytes(30) - 1) == -22 and b"workspace" in lib.hipie_last_error()
    assert lib.hipie_token_focal_ws_bytes(1 << 40) >= lib.hipie_token_focal_ws_bytes(30) >= 4
    for B, Q, T in ((0, 3, 5), (2, 0, 5), (2, 3, 0)):       # B*Q*T = 0: no launch, null data pointers allowed
        assert lib.hipie_token_focal_forward(None, None, None, None, None, 0, B, Q, T, 0.25, 2.0, None) == 0
        assert lib.hipie_token_focal_backward(None, None, None, None, None, B, Q, T, 0.25, 2.0, None) == 0


def test_ops_refuse_host_tensors():
    from hipie_amd import ops
    src, tgt, idx, pts = torch.zeros(2, 4, 4), torch.zeros(3, 4, 4), torch.tensor([2, 0]), torch.rand(2, 5, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.point_mask_loss_forward(src, tgt, idx, pts, 0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.point_mask_loss_backward(src, tgt, idx, pts, torch.zeros(2, 3), torch.zeros(2), torch.zeros(2), 1, 0.25)
    x = torch.zeros(2, 3, 5)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.token_focal_forward(x, x, torch.ones(2, 5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.token_focal_backward(x, x, None, torch.ones(()))


def test_functions_refuse_host_tensors_and_backend_has_the_methods():
    from hipie_amd.training import net
    assert not hasattr(net.HipBackend, "point_mask_loss") and not hasattr(net.HipBackendAll, "token_focal_sum")
    x = torch.zeros(2, 3, 5, requires_grad=True)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendLosses.token_focal_sum(x, x.detach(), None, 0.25)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendLosses.point_mask_loss(torch.zeros(2, 4, 4), torch.zeros(3, 4, 4), torch.tensor([2, 0]), torch.rand(2, 5, 2), 0, -1.0)


# ------------------------------------------------------------------------------------------------ criterion plumbing
Q, L = 9, 11
INDICES = [(torch.tensor([4, 1, 7, 2]), torch.tensor([2, 0, 2, 1])), (torch.tensor([8, 3]), torch.tensor([0, 0]))]      # repeated, unordered


def _draw(dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    return lambda shape, device: torch.rand(tuple(shape), generator=g, dtype=dtype).to(device)


def _targets(dtype, sizes):
    g = torch.Generator().manual_seed(11)
    out = []
    for n, (h, w) in zip((3, 1), sizes):                    # unequal target counts, unequal mask sizes
        pm = torch.zeros(n, L, dtype=torch.bool)
        for t in range(n):
            pm[t, 1 + 2 * t:3 + 2 * t] = True
        box = torch.cat((torch.rand(n, 2, generator=g, dtype=dtype) * 0.4 + 0.3, torch.rand(n, 2, generator=g, dtype=dtype) * 0.3 + 0.1), 1)
        out.append({"labels": torch.arange(n), "boxes": box, "positive_map": pm, "is_thing": torch.tensor([True, False, True][:n]),
                    "masks": (torch.rand(n, h, w, generator=g) < 0.4).to(dtype)})
    return out


def _text_mask():
    m = torch.ones(2, L, dtype=torch.int64)
    m[0, 8:] = 0
    m[1, 5:] = 0                                            # drops tokens that image 1's queries score
    return m


def _det_case(dtype, **kw):
    g = torch.Generator().manual_seed(3)
    leaves = {"pred_logits": torch.randn(2, Q, L, generator=g, dtype=dtype), "pred_boxes": torch.rand(2, Q, 4, generator=g, dtype=dtype) * 0.5 + 0.2,
              "m0": torch.randn(1, 4, 1, 12, 20, generator=g, dtype=dtype) * 2, "m1": torch.randn(1, 2, 1, 12, 20, generator=g, dtype=dtype) * 2}
    for v in leaves.values():
        v.requires_grad_(True)
    out = {"pred_logits": leaves["pred_logits"], "pred_boxes": leaves["pred_boxes"], "pred_masks": [leaves["m0"], leaves["m1"]],
           "text_masks": _text_mask()}
    crit = DetCriterion(None, ["labelsVL", "boxes", "masks"], num_points=50, draw=_draw(dtype), ota=True, **kw)
    losses = crit(out, _targets(dtype, ((40, 56), (64, 33))), [INDICES])
    return losses, leaves


class _FixedMatcher:
    def __call__(self, logits, boxes, targets, masks=None):
        return INDICES


def _mask_case(dtype, **kw):
    g = torch.Generator().manual_seed(4)
    leaves = {"pred_logits": torch.randn(2, Q, L, generator=g, dtype=dtype), "pred_boxes": torch.rand(2, Q, 4, generator=g, dtype=dtype) * 0.5 + 0.2,
              "pred_masks": torch.randn(2, Q, 10, 14, generator=g, dtype=dtype) * 2}
    for v in leaves.values():
        v.requires_grad_(True)
    out = dict(leaves, text_masks=_text_mask())
    crit = MaskCriterion(80, _FixedMatcher(), ["labels", "masks", "boxes"], vl_loss=True, num_points=50, draw=_draw(dtype), **kw)
    losses = crit(out, _targets(dtype, ((23, 31), (40, 17))))
    return losses, leaves


def _grads(losses, leaves):
    total = sum(v * (1.0 + 0.1 * i) for i, (_, v) in enumerate(sorted(losses.items())))
    return dict(zip(leaves, torch.autograd.grad(total, list(leaves.values()), allow_unused=True)))


@pytest.mark.parametrize("case", [_det_case, _mask_case], ids=["det", "maskdino"])
def test_criterion_with_an_ops_object_matches_the_gather_formulation(case):
    calls = {"point": 0, "token": 0}

    class Spy(TorchLossOps):
        @staticmethod
        def point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha):
            calls["point"] += 1
            assert tgt_maps.shape[0] == 2 * 3 and tgt_index.tolist() == [2, 0, 2, 1, 3, 3]        # ALL padded targets + the flat index
            assert (mode, alpha) == ((1, 0.25) if case is _det_case else (0, -1.0))
            return TorchLossOps.point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha)

        @staticmethod
        def token_focal_sum(logits, onehot, text_mask, alpha):
            calls["token"] += 1
            assert text_mask is not None and logits.shape == (2, Q, L)
            return TorchLossOps.token_focal_sum(logits, onehot, text_mask, alpha)

    want, want_leaves = case(torch.float64)
    got, got_leaves = case(torch.float64, ops=Spy)
    assert calls == {"point": 1, "token": 1}
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = float(got[k].detach()), float(want[k].detach())
        assert abs(g - w) <= 1e-12 * max(1.0, abs(w)), (k, g, w)
    assert min(float(want[k].detach()) for k in ("loss_mask", "loss_dice", "loss_ce")) > 0
    gw, gg = _grads(want, want_leaves), _grads(got, got_leaves)
    for k in gw:
        assert gw[k] is not None and float(gw[k].abs().max()) > 0, k
        assert float((gg[k] - gw[k]).abs().max()) <= 1e-12 * max(1.0, float(gw[k].abs().max())), k


@pytest.mark.parametrize("case", [_det_case, _mask_case], ids=["det", "maskdino"])
def test_ops_none_is_the_criterion_without_the_argument(case):
    a, a_leaves = case(torch.float32)
    b, b_leaves = case(torch.float32, ops=None)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    ga, gb = _grads(a, a_leaves), _grads(b, b_leaves)
    assert all(torch.equal(ga[k], gb[k]) for k in ga)
