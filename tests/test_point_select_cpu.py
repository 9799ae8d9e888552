"""CPU: the host side of csrc/point_select.hip -- the selection rule restated in torch against criterion.uncertain_points and against the
float64 selection on every real-valued seed of the case file (the cap check: the float32 torch path itself stays inside the band and the
0.1 % cap the GPU test asserts), the `ops` plumbing of the criteria and the matchers with a plain-torch object, and the refusals of the four
entry points and of the two bindings (no launch)."""
import ctypes

import pytest
import torch

from _point_select_cases import (SELECT_SEEDS, SELECT_SHAPES, TorchCriteriaOps, check_selection, cost_case, exact_case, sampled, select_case,
                                 select_points, select_rule, select_yardsticks)
from hipie_amd import _lib
from hipie_amd.training import criterion
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights, cost_matrix, mask_costs
from test_point_loss_cpu import _det_case, _draw, _grads, _mask_case, _targets


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


# ------------------------------------------------------------------------------------------------ the rule
def test_select_rule_ties_zero_signs_nan_and_order():
    v = torch.tensor([2.0, -1.0, 1.0, 0.0, -0.0, float("nan"), 1.0, -3.0])
    assert select_rule(v, 0).tolist() == []
    assert select_rule(v, 1).tolist() == [5]                     # a NaN counts as the largest score
    assert select_rule(v, 2).tolist() == [3, 5]                  # +0.0 in front of -0.0: they tie, the index decides
    assert select_rule(v, 3).tolist() == [3, 4, 5]
    assert select_rule(v, 4).tolist() == [1, 3, 4, 5]            # |-1| = |1|: the first of the three by index
    assert select_rule(v, 5).tolist() == [1, 2, 3, 4, 5]
    assert select_rule(v, 8).tolist() == list(range(8))


def test_exact_case_is_exact_and_full_of_ties():
    src, cand, rest, k, values = exact_case(3, 8, 16, 1200, 300, 100)
    assert torch.equal(sampled(src, cand, torch.float32), values) and torch.equal(sampled(src, cand, torch.float64), values.double())
    assert bool((src[0] == 0).all()) and bool(torch.signbit(src[0]).any()) and values.unique().numel() <= 7
    a = values[1].abs()
    tau = a.sort().values[k - 1]
    assert int((a == tau).sum()) > 1 and int((a < tau).sum()) < k < int((a <= tau).sum())      # the threshold value is tied: the index decides


@pytest.mark.parametrize("seed", SELECT_SEEDS)
@pytest.mark.parametrize("shape", SELECT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_rule_is_uncertain_points_and_float32_stays_inside_the_cap(shape, seed):
    src, cand, rest, k = case = select_case(*shape, seed)
    P = shape[3]
    draws = iter([cand] if rest is None else [cand, rest])
    got = criterion.uncertain_points(src[:, None], P, 3.0, 0.75, lambda s, device: next(draws))
    assert got.shape == (shape[0], P, 2) and next(draws, None) is None
    v32 = sampled(src, cand, torch.float32)
    want = select_points(v32, cand, rest, k)
    # the same set: torch.topk sorts by score and leaves ties open, so the two are compared by the sorted |sample| of what they chose
    assert torch.equal(sampled(src, got[:, :k], torch.float32).abs().sort(1).values, sampled(src, want[:, :k], torch.float32).abs().sort(1).values)
    assert torch.equal(got[:, k:], want[:, k:])
    # the cap check: the float32 selection against the float64 one, with the band and the cap of the GPU test
    v64, e_lib = select_yardsticks(*shape, seed)
    check_selection("torch float32 %s seed %d" % (shape, seed), want, case, v64, e_lib)


# ------------------------------------------------------------------------------------------------ the plumbing
@pytest.mark.parametrize("case", [_det_case, _mask_case], ids=["det", "maskdino"])
def test_criterion_selects_its_points_through_the_ops_object(case):
    calls = []

    class Spy(TorchCriteriaOps):
        @staticmethod
        def uncertain_points(src, cand, rest, k, num_points=None):
            calls.append((tuple(src.shape), tuple(cand.shape), tuple(rest.shape), k, num_points))
            return TorchCriteriaOps.uncertain_points(src, cand, rest, k, num_points)

    want, want_leaves = case(torch.float64)
    got, got_leaves = case(torch.float64, ops=Spy)
    assert len(calls) == 1 and calls[0][0][0] == 6 and calls[0][1] == (6, 150, 2) and calls[0][2] == (6, 13, 2) and calls[0][3:] == (37, 50)
    assert sorted(got) == sorted(want)
    for k in want:                                               # the same points in another order: the sums differ by rounding alone
        g, w = float(got[k].detach()), float(want[k].detach())
        assert abs(g - w) <= 1e-12 * max(1.0, abs(w)), (k, g, w)
    gw, gg = _grads(want, want_leaves), _grads(got, got_leaves)
    for k in gw:
        assert float((gg[k] - gw[k]).abs().max()) <= 1e-12 * max(1.0, float(gw[k].abs().max())), k


def _match_case(dtype, ops):
    g = torch.Generator().manual_seed(21)
    Q, L = 9, 11
    logits, boxes = torch.randn(2, Q, L, generator=g, dtype=dtype), torch.rand(2, Q, 4, generator=g, dtype=dtype) * 0.5 + 0.2
    masks = torch.randn(2, Q, 10, 14, generator=g, dtype=dtype) * 2
    draws = []

    def draw(shape, device, _d=_draw(dtype)):
        draws.append(tuple(shape))
        return _d(shape, device)
    kw = {} if ops is None else {"ops": ops}
    m = HungarianMatcher(MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0), num_points=50, draw=draw, class_mode="map", **kw)
    return m(logits, boxes, _targets(dtype, ((23, 31), (40, 17))), masks=masks), draws


def test_matcher_with_an_ops_object_assigns_as_without():
    calls = []

    class Spy(TorchCriteriaOps):
        @staticmethod
        def mask_match_costs(pred, tgt, coords):
            calls.append((tuple(pred.shape), tuple(tgt.shape), tuple(coords.shape)))
            return TorchCriteriaOps.mask_match_costs(pred, tgt, coords)

    want, want_draws = _match_case(torch.float32, None)
    got, got_draws = _match_case(torch.float32, Spy)
    assert calls == [((9, 10, 14), (3, 23, 31), (50, 2)), ((9, 10, 14), (1, 40, 17), (50, 2))]
    assert got_draws == want_draws == [(1, 50, 2)] * 2
    for (gi, gj), (wi, wj) in zip(got, want):
        assert torch.equal(gi, wi) and torch.equal(gj, wj)
    # cost_matrix: ops=None is the call without the argument, and the object's costs are the ones that are weighted in
    pred, tgt, coords = cost_case(5, 3, 5, 7, 40, True)
    t = {"labels": torch.arange(3), "boxes": torch.rand(3, 4) * 0.3 + 0.2, "is_thing": torch.tensor([True, False, True]), "masks": tgt}
    lg, bx, w = torch.randn(5, 4), torch.rand(5, 4) * 0.3 + 0.2, MatchWeights(1.0, 1.0, 1.0, 3.0, 7.0)
    base = cost_matrix(lg, bx, t, w, pred, coords, class_mode="ids")
    assert torch.equal(base, cost_matrix(lg, bx, t, w, pred, coords, class_mode="ids", ops=None))

    class Fixed:
        @staticmethod
        def mask_match_costs(pred, tgt, coords):
            return torch.full((5, 3), 1.0), torch.full((5, 3), 2.0)
    ce, dice = mask_costs(pred, tgt, coords)
    moved = cost_matrix(lg, bx, t, w, pred, coords, class_mode="ids", ops=Fixed)
    assert torch.allclose(moved - base, 3.0 * (1.0 - ce) + 7.0 * (2.0 - dice), atol=1e-5)


def test_backends_and_loss_plan_carry_the_new_methods():
    from hipie_amd.training import net
    from hipie_amd.training.weights import maskdino_loss_plan
    assert issubclass(net.HipBackendCriteria, net.HipBackendLosses)
    for be in (net.HipBackend, net.HipBackendLosses, net.HipBackendAll):
        assert not hasattr(be, "uncertain_points") and not hasattr(be, "mask_match_costs")
    plan = lambda **kw: maskdino_loss_plan(4.0, 5.0, 5.0, 5.0, 2.0, True, "seg", True, 3, True, 4.0, 5.0, 5.0, 5.0, 2.0, 50, True, **kw)[2]      # noqa: E731
    assert plan().ops is None and plan(ops=net.HipBackendCriteria).ops is net.HipBackendCriteria
    assert HungarianMatcher().ops is None
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendCriteria.uncertain_points(torch.zeros(2, 4, 4), torch.rand(2, 12, 2), torch.rand(2, 1, 2), 3)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):           # any floating dtype is cast, as the torch path takes it
        net.HipBackendCriteria.uncertain_points(torch.zeros(2, 4, 4).double(), torch.rand(2, 12, 2).double(), torch.rand(2, 1, 2).double(), 3, 4)
    with pytest.raises(RuntimeError, match="rest must hold P - k = 1 points, got 2"):           # the P the criterion hands over is checked
        net.HipBackendCriteria.uncertain_points(torch.zeros(2, 4, 4), torch.rand(2, 12, 2), torch.rand(2, 2, 2), 3, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendCriteria.mask_match_costs(torch.zeros(5, 4, 4), torch.zeros(3, 8, 8), torch.rand(7, 2))


# ------------------------------------------------------------------------------------------------ refusals, no launch
P_ = ctypes.c_void_p(256)


def _select(lib, src=P_, cand=P_, rest=P_, pts=P_, ws=P_, ws_bytes=1 << 20, N=2, H=8, W=8, C=12, P=4, k=3):
    return lib.hipie_uncertain_points(src, cand, rest, pts, ws, ws_bytes, N, H, W, C, P, k, None)


def _cost(lib, pred=P_, tgt=P_, coords=P_, ce=P_, dice=P_, ws=P_, ws_bytes=1 << 30, Q=5, H=8, W=8, T=3, Ht=16, Wt=16, P=7):
    return lib.hipie_mask_match_cost(pred, tgt, coords, ce, dice, ws, ws_bytes, Q, H, W, T, Ht, Wt, P, None)


def test_uncertain_points_refusals_without_a_launch():
    lib = _lib.load()
    for kw, msg in (({"k": 13}, b"k=13"), ({"k": -1}, b"k=-1"), ({"k": 5, "P": 4}, b"exceeds P=4"), ({"N": -1}, b"negative"),
                    ({"H": 1 << 16, "W": 1 << 15}, b"H*W=2147483648"), ({"H": 0}, b"H*W=0"), ({"C": 1 << 30, "k": 3}, b"below 2^30"),
                    ({"src": None}, b"null"), ({"cand": None}, b"null"), ({"rest": None}, b"null"), ({"pts": None}, b"null"), ({"ws": None}, b"null")):
        assert _select(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    # one element below the limit passes the size check and trips the null pointer
    assert _select(lib, H=(1 << 16) - 1, W=1 << 15, src=None) == -22 and b"null" in lib.hipie_last_error()
    need = lib.hipie_uncertain_points_ws_bytes(2, 12)
    assert need == 2 * 12 * 4 and lib.hipie_uncertain_points_ws_bytes(200, 37632) == 200 * 37632 * 4 and lib.hipie_uncertain_points_ws_bytes(0, 12) > 0
    assert _select(lib, ws_bytes=need - 1) == -22 and b"workspace" in lib.hipie_last_error()
    # N = 0 or P = 0: no launch, null data pointers allowed
    assert lib.hipie_uncertain_points(None, None, None, None, None, 0, 0, 8, 8, 12, 4, 3, None) == 0
    assert lib.hipie_uncertain_points(None, None, None, None, None, 0, 2, 8, 8, 12, 0, 0, None) == 0


def test_mask_match_cost_refusals_without_a_launch():
    lib = _lib.load()
    for kw, msg in (({"P": 0}, b"P=0"), ({"P": -2}, b"P=-2"), ({"Q": -1}, b"negative"), ({"H": 1 << 16, "W": 1 << 15}, b"H*W=2147483648"),
                    ({"Ht": 1 << 15, "Wt": 1 << 16}, b"Ht*Wt=2147483648"), ({"Wt": 0}, b"Ht*Wt=0"), ({"ws": ctypes.c_void_p(260)}, b"aligned"),
                    ({"pred": None}, b"null"), ({"tgt": None}, b"null"), ({"coords": None}, b"null"), ({"ce": None}, b"null"), ({"dice": None}, b"null"),
                    ({"ws": None}, b"null")):
        assert _cost(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    assert _cost(lib, H=(1 << 16) - 1, W=1 << 15, pred=None) == -22 and b"null" in lib.hipie_last_error()
    need = lib.hipie_mask_match_cost_ws_bytes(5, 3, 7)
    assert need >= 3 * 7 * 4 and lib.hipie_mask_match_cost_ws_bytes(900, 100, 12544) > lib.hipie_mask_match_cost_ws_bytes(300, 8, 12544) > need
    assert lib.hipie_mask_match_cost_ws_bytes(900, 100, 12544) < 16 << 20          # the targets once, not the Q x P samples (45 MB)
    assert _cost(lib, ws_bytes=need - 1) == -22 and b"workspace" in lib.hipie_last_error()
    # Q = 0 or T = 0: the empty result, no launch, null data pointers allowed
    for Q, T in ((0, 3), (5, 0), (0, 0)):
        assert lib.hipie_mask_match_cost(None, None, None, None, None, None, 0, Q, 8, 8, T, 16, 16, 7, None) == 0
    assert lib.hipie_mask_match_cost_ws_bytes(0, 3, 7) > 0


def test_bindings_refuse_before_the_device_is_asked():
    from hipie_amd import ops
    src, cand, rest = torch.zeros(2, 4, 4), torch.rand(2, 12, 2), torch.rand(2, 1, 2)
    for args, msg in (((src.double(), cand, rest, 3), "src must be torch.float32"), ((src, cand.half(), rest, 3), "cand must be torch.float32"),
                      ((src[0], cand, rest, 3), "src must have 3 dimensions"), ((src, cand[0], rest, 3), "cand must have 3 dimensions"),
                      ((src, cand, rest[0], 3), "rest must have 3 dimensions"), ((src.transpose(1, 2), cand, rest, 3), "src tensor has to be contiguous"),
                      ((torch.zeros(2, 4, 8)[:, :, ::2], cand, rest, 3), "src tensor has to be contiguous"),
                      ((src, cand, rest, 13), r"k=13 must be in \[0, C=12\]"), ((src, cand, rest, -1), "k=-1"),
                      ((src, cand[:1], rest, 3), r"cand must be \(N=2"), ((src, cand, torch.rand(3, 1, 2), 3), r"rest must be \(N=2")):
        with pytest.raises(RuntimeError, match=msg):
            ops.uncertain_points(*args)
    with pytest.raises(RuntimeError, match="rest must hold P - k = 1 points, got 2"):
        ops.uncertain_points(src, cand, torch.rand(2, 2, 2), 3, num_points=4)
    with pytest.raises(RuntimeError, match="rest must hold P - k = 1 points, got 0"):
        ops.uncertain_points(src, cand, None, 3, num_points=4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.uncertain_points(src, cand, rest, 3, num_points=4)
    pred, tgt, coords = torch.zeros(5, 4, 4), torch.zeros(3, 8, 8), torch.rand(7, 2)
    for args, msg in (((pred.double(), tgt, coords), "pred must be torch.float32"), ((pred, tgt.bool(), coords), "tgt must be torch.float32"),
                      ((pred[0], tgt, coords), "pred must have 3 dimensions"), ((pred, tgt, coords[None]), "coords must have 2 dimensions"),
                      ((pred, tgt.transpose(1, 2), coords), "tgt tensor has to be contiguous"), ((pred, tgt, torch.rand(7, 3)), r"coords must be \(P > 0, 2\)"),
                      ((pred, tgt, torch.rand(0, 2)), r"coords must be \(P > 0, 2\)")):
        with pytest.raises(RuntimeError, match=msg):
            ops.mask_match_cost(*args)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.mask_match_cost(pred, tgt, coords)
