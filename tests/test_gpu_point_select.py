"""GPU: hipie_uncertain_points and hipie_mask_match_cost (csrc/point_select.hip) through the ops, and the opt-in HipBackendCriteria wiring of
the criteria and the matchers.

Selection, exact: integer maps with candidates at pixel centres -- pts must equal the restated rule bit for bit (the tie rule, the zero
signs, NaN, the ascending order, rest).  Selection, real-valued and the costs: tests/_point_select_cases.py -- the float64 formulas on the
CPU as the reference, the float32 ones as e_lib; every case prints its figures (lines starting with SELECT / COST) before it asserts."""
import os
import sys

import pytest
import torch

from _point_select_cases import (SELECT_SEEDS, SELECT_SHAPES, assignment_total, bound_of, check_costs, check_selection, cost_case, cost_yardsticks, err,
                                 exact_case, mask_costs_in, sampled, second_best_gap, select_case, select_points, select_yardsticks)
from test_point_loss_cpu import INDICES, _targets


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _select(src, cand, rest, k):
    from hipie_amd import ops
    pts = ops.uncertain_points(src.to(DEV), cand.to(DEV), None if rest is None else rest.to(DEV), k)
    assert pts.dtype == torch.float32 and pts.is_contiguous()
    return pts


# ------------------------------------------------------------------------------------------------ selection, exact
# (N, H, W, C, k, rest): one pixel; C = 1200 (no multiple of 256 or 1024) with a tied threshold; the production C and k (37 key chunks, 3
# index segments per wave); k = 0; no rest; k = C
EXACT = [(1, 1, 1, 12, 3, 1), (3, 8, 16, 1200, 300, 100), (2, 64, 64, 37632, 9408, 3136), (2, 8, 16, 1200, 0, 400), (2, 8, 16, 1200, 300, 0),
         (2, 8, 16, 1200, 1200, 0), (2, 8, 16, 1200, 1200, 7), (2, 2, 2, 64, 63, 1), (1, 8, 16, 1025, 1024, 1)]


@pytest.mark.parametrize("geom", EXACT, ids=lambda g: "x".join(map(str, g)))
def test_selection_is_the_rule_bit_for_bit(geom):
    src, cand, rest, k, values = exact_case(*geom)
    want = select_points(values, cand, rest, k)
    got = _select(src, cand, rest, k)
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    torch.randn(1 << 20, device=DEV).sum()                     # other work in between
    assert torch.equal(_bits(_select(src, cand, rest, k)), _bits(got))            # two calls give identical bits


def test_selection_takes_nan_first_and_both_zeros_as_one_value():
    src = torch.tensor([[[float("nan"), -0.0, 0.0, 1.0], [2.0, -1.0, float("nan"), 3.0]]])          # (1, 2, 4)
    xi = torch.tensor([3, 0, 1, 2, 1, 2, 0, 3, 2])
    yi = torch.tensor([0, 1, 0, 0, 1, 1, 0, 1, 0])
    cand = torch.stack(((xi.float() + 0.5) / 4, (yi.float() + 0.5) / 2), -1)[None]
    values = src[0, yi, xi][None]                             # 1, 2, -0, 0, -1, nan, nan, 3, 0
    for k, chosen in ((1, [5]), (2, [5, 6]), (3, [2, 5, 6]), (4, [2, 3, 5, 6]), (5, [2, 3, 5, 6, 8]), (6, [0, 2, 3, 5, 6, 8]), (7, [0, 2, 3, 4, 5, 6, 8])):
        want = select_points(values, cand, None, k)
        assert torch.equal(want[0], cand[0, chosen])
        assert torch.equal(_bits(_select(src, cand, None, k)), _bits(want)), k


# ------------------------------------------------------------------------------------------------ selection, real-valued
@pytest.mark.parametrize("seed", SELECT_SEEDS)
@pytest.mark.parametrize("shape", SELECT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_against_float64(shape, seed):
    case = select_case(*shape, seed)
    v64, e_lib = select_yardsticks(*shape, seed)
    got = _select(*case)
    check_selection("hip %s seed %d" % (shape, seed), got.cpu(), case, v64, e_lib)
    assert torch.equal(_bits(_select(*case)), _bits(got))


@pytest.mark.parametrize("oversample,importance", [(3.0, 0.0), (3.0, 1.0), (1.0, 1.0)], ids=["k=0", "no-rest", "k=C"])
def test_selection_edges(oversample, importance):
    N, H, W, P = 3, 5, 7, 400
    src, cand, rest, k = case = select_case(N, H, W, P, 0, oversample, importance)
    assert (k, rest is None, cand.shape[1]) == {(3.0, 0.0): (0, False, 1200), (3.0, 1.0): (400, True, 1200), (1.0, 1.0): (400, True, 400)}[(oversample, importance)]
    v64 = sampled(src, cand, torch.float64)
    e_lib = float((sampled(src, cand, torch.float32).double() - v64).abs().max())
    got = _select(*case).cpu()
    check_selection("hip edge oversample %g importance %g" % (oversample, importance), got, case, v64, e_lib)
    if k == cand.shape[1]:
        assert torch.equal(got, cand)                         # every candidate, in its place


def test_selection_of_nothing():
    from hipie_amd import ops
    pts = ops.uncertain_points(torch.zeros(0, 8, 8, device=DEV), torch.zeros(0, 12, 2, device=DEV), torch.zeros(0, 1, 2, device=DEV), 3)
    assert pts.shape == (0, 4, 2)


# ------------------------------------------------------------------------------------------------ costs
def _costs(case):
    from hipie_amd import ops
    pred, tgt, coords = (t.to(DEV) for t in case)
    ce, dice = ops.mask_match_cost(pred, tgt, coords)
    assert ce.shape == dice.shape == (pred.shape[0], tgt.shape[0]) and ce.dtype == dice.dtype == torch.float32
    return ce, dice


@pytest.mark.parametrize("T", [1, 3, 17])
@pytest.mark.parametrize("Q", [1, 5, 300])
def test_mask_costs_against_float64(Q, T):
    for H, W in ((1, 1), (5, 7), (64, 64)):
        for P in (7, 400):
            for big in (False, True):
                key = (Q, T, H, W, P, big)
                ref, lib = cost_yardsticks(*key)
                check_costs("Q=%d T=%d %dx%d P=%d %s" % (Q, T, H, W, P, "hard 4x" if big else "soft"), _costs(cost_case(*key)), ref, lib)


def test_mask_costs_at_the_production_point_count_and_twice_the_same_bits():
    key = (5, 3, 64, 64, 12544, True)                          # 7 chunks of 2048 points, the last one partly filled
    ref, lib = cost_yardsticks(*key)
    first = _costs(cost_case(*key))
    check_costs("Q=5 T=3 64x64 P=12544 hard 4x", first, ref, lib)
    _costs(cost_case(5, 3, 5, 7, 400, False))                  # other work in between
    torch.randn(1 << 20, device=DEV).sum()
    second = _costs(cost_case(*key))
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    for other in ((300, 17, 64, 64, 400, True), (5, 3, 5, 7, 7, False)):
        a, b = _costs(cost_case(*other)), _costs(cost_case(*other))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("Q,T", [(300, 17), (5, 3), (17, 17)])
def test_assignment_from_the_kernel_costs_is_the_float64_optimum(Q, T):
    """robust to ties: the assignment computed from the kernel's costs, priced with the float64 costs, against the float64 optimum"""
    case = cost_case(Q, T, 64, 64, 400, True)
    ce64, dice64 = mask_costs_in(*(t.double() for t in case))
    C64 = 5.0 * ce64 + 5.0 * dice64
    ce, dice = _costs(case)
    got, best = assignment_total((5.0 * ce + 5.0 * dice).cpu(), C64), assignment_total(C64, C64)
    print("COST assignment Q=%d T=%d: priced %.9f, optimum %.9f" % (Q, T, got, best))
    assert abs(got - best) <= 1e-5 * abs(best)


def test_mask_costs_of_nothing():
    from hipie_amd import ops
    for Q, T in ((0, 3), (5, 0)):
        ce, dice = ops.mask_match_cost(torch.zeros(Q, 8, 8, device=DEV), torch.zeros(T, 16, 16, device=DEV), torch.rand(7, 2, device=DEV))
        assert ce.shape == dice.shape == (Q, T)


# ------------------------------------------------------------------------------------------------ wiring
def _hash_draw(dtype=torch.float32):
    sys.path.insert(0, GOLD)
    import _synth
    d = _synth.HashDraws()
    return d, lambda shape, device: d.rand(tuple(shape), device).to(dtype)


def _loss_masks(kind, ops, dev, dtype=torch.float32):
    """loss_masks of one criterion on the fixture of test_point_loss_cpu (6 matched instances, unequal target sizes) -> (losses, draws)"""
    from hipie_amd.training.criterion import DetCriterion, MaskCriterion
    g = torch.Generator().manual_seed(3 if kind == "det" else 4)
    d, draw = _hash_draw(dtype)
    if kind == "det":
        out = {"pred_masks": [(torch.randn(1, n, 1, 12, 20, generator=g) * 2).to(dev, dtype) for n in (4, 2)]}
        crit = DetCriterion(None, ["masks"], num_points=400, draw=draw, ota=True, ops=ops)
        sizes = ((40, 56), (64, 33))
    else:
        out = {"pred_masks": (torch.randn(2, 9, 10, 14, generator=g) * 2).to(dev, dtype)}
        crit = MaskCriterion(80, None, ["masks"], num_points=400, draw=draw, ops=ops)
        sizes = ((23, 31), (40, 17))
    targets = [{k: (v.to(dev, dtype) if v.is_floating_point() else v.to(dev)) for k, v in t.items()} for t in _targets(torch.float32, sizes)]
    with torch.no_grad():
        losses = crit.loss_masks(out, targets, INDICES, 6.0)
    return {k: v.detach().cpu() for k, v in losses.items()}, d.calls


@pytest.mark.parametrize("kind", ["det", "maskdino"])
def test_criterion_with_the_selection_kernel_matches_the_loss_backend(kind):
    from hipie_amd.training import net
    want, want_draws = _loss_masks(kind, net.HipBackendLosses, DEV)
    got, got_draws = _loss_masks(kind, net.HipBackendCriteria, DEV)
    ref64, _ = _loss_masks(kind, None, "cpu", torch.float64)
    lib32, _ = _loss_masks(kind, None, "cpu", torch.float32)
    assert got_draws == want_draws == 2                       # the candidates, then the rest
    assert sorted(got) == sorted(want) == ["loss_dice", "loss_mask"]
    for k in want:
        bound = bound_of(lib32[k], ref64[k])
        print("SELECT wiring %-8s %-9s against HipBackendLosses %.3e  against float64 %.3e (HipBackendLosses %.3e)  e_lib %.3e  bound %.3e"
              % (kind, k, err(got[k], want[k]), err(got[k], ref64[k]), err(want[k], ref64[k]), err(lib32[k], ref64[k]), bound))
        assert err(got[k], want[k]) <= bound and err(got[k], ref64[k]) <= bound


def _matcher_case(dtype, dev, ops, seed):
    from hipie_amd.training.matcher import HungarianMatcher, MatchWeights
    g = torch.Generator().manual_seed(seed)
    Q, L = 9, 11
    logits, boxes = torch.randn(2, Q, L, generator=g), torch.rand(2, Q, 4, generator=g) * 0.5 + 0.2
    masks = torch.randn(2, Q, 10, 14, generator=g) * 2
    targets = _targets(torch.float32, ((23, 31), (40, 17)))
    d, draw = _hash_draw()
    w = MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0)
    kw = {} if ops is None else {"ops": ops}
    m = HungarianMatcher(w, num_points=400, draw=draw, class_mode="map", **kw)
    pairs = m(logits.to(dev, dtype), boxes.to(dev, dtype), [{k: (v.to(dev, dtype) if v.is_floating_point() else v.to(dev)) for k, v in t.items()} for t in targets],
              masks=masks.to(dev, dtype))
    return pairs, d.calls, (logits, boxes, masks, targets, w)


def _float64_gap(logits, boxes, masks, targets, w):
    """the smallest relative distance between the best and the second-best assignment of the float64 cost matrices, over the images"""
    from hipie_amd.training.matcher import cost_matrix
    d, draw = _hash_draw(torch.float64)
    gaps = []
    for b, t in enumerate(targets):
        coords = draw((1, 400, 2), "cpu")[0]
        t64 = {k: (v.double() if v.is_floating_point() else v) for k, v in t.items()}
        C = cost_matrix(logits[b].double(), boxes[b].double(), t64, w, class_mode="map")
        ce, dice = mask_costs_in(masks[b].double(), t64["masks"], coords)
        gaps.append(second_best_gap(C + w.mask * ce + w.dice * dice)[1])
    return min(gaps)


@pytest.mark.parametrize("seed", [22, 23])
def test_matcher_with_the_cost_kernel_assigns_as_without(seed):
    from hipie_amd.training import net
    want, want_draws, tensors = _matcher_case(torch.float32, DEV, None, seed)
    gap = _float64_gap(*tensors)
    print("COST matcher seed %d: second-best assignment %.3e away" % (seed, gap))
    assert gap >= 1e-3                                        # the float64 optimum is unique: the pairs can be compared
    got, got_draws, _ = _matcher_case(torch.float32, DEV, net.HipBackendCriteria, seed)
    assert got_draws == want_draws == 2
    for (gi, gj), (wi, wj) in zip(got, want):
        assert torch.equal(gi, wi) and torch.equal(gj, wj)
