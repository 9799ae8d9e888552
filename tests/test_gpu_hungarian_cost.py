"""GPU: hipie_hungarian_cost (csrc/hungarian_cost.hip) through ops.hungarian_cost, functions.hungarian_costs and the opt-in
net.HipBackendHungarian wiring of HungarianMatcher.forward / forward_boxes_only and TrainStep.

Costs: tests/_hungarian_cases.py -- matcher.cost_matrix in float64 on the CPU as the reference, in float32 as e_lib, NaN positions first and
exactly; every case prints its figures (lines starting with HUNG) before it asserts.  Assignment: scipy on a copy of the kernel's own block
(exact), the float64 total of the returned pairs against the float64 optimum (optimality), and equality with the torch path's pairs where the
float64 optimum is separated from the second-best assignment."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from _hungarian_cases import (IDS, SEEDS, SHAPES, SMALL, W_BOX, Golden, assignment_gap, bound_of, case_coords, err, golden_cases, hungarian_case, optimum,
                              reference_cost, same_pairs, slack, total_cost)
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights
from test_training import Replay


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W_ALL = MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0)
# map / ids x boxes on / off x stuff mean on / off x masks off / on
MATRIX = [(mode, boxes, stuff, masks) for mode in ("map", "ids") for boxes in (True, False) for stuff in (True, False) for masks in (False, True)]
CASES = [pytest.param(s + (seed, "mixed"), id="%s-%d" % (IDS(s), seed)) for s in SHAPES for seed in SEEDS] + [
    pytest.param(SHAPES[3] + (0, "none"), id="no-thing"), pytest.param(SHAPES[3] + (0, "all"), id="only-things")]


def _on(dev, targets):
    return [{k: v.to(dev) for k, v in t.items()} for t in targets]


@functools.lru_cache(maxsize=None)
def _device_case(key):
    logits, boxes, targets, pred = hungarian_case(*key)
    return logits.to(DEV), boxes.to(DEV), _on(DEV, targets), pred.to(DEV)


def _kernel_costs(key, combo, P=300, targets=None):
    """functions.hungarian_costs on one case and one row of the matrix -> per image the (Q, T_i) host array"""
    from hipie_amd.training import functions
    mode, with_boxes, stuff, with_masks = combo
    logits, boxes, dev_targets, pred = _device_case(key)
    packed = functions.pack_match_targets(dev_targets if targets is None else _on(DEV, targets), DEV)
    coords = case_coords(logits.shape[0], P, key[5]).to(DEV)
    Cs = functions.hungarian_costs(logits, boxes, packed, W_ALL, masks=list(pred) if with_masks else None, coords=list(coords) if with_masks else None,
                                   stuff_takes_mean=stuff, with_boxes=with_boxes, class_mode=mode)
    assert Cs is not None and [C.shape for C in Cs] == [(logits.shape[1], n) for n in packed.counts] and all(C.dtype == np.float32 for C in Cs)
    return Cs


def _references(key, combo, P=300, targets=None):
    mode, with_boxes, stuff, with_masks = combo
    logits, boxes, case_targets, pred = hungarian_case(*key)
    coords = case_coords(logits.shape[0], P, key[5])
    out = []
    for b, t in enumerate(case_targets if targets is None else targets):
        if len(t["boxes"]) == 0:                              # nothing to compare but the shape
            out.append((torch.zeros(logits.shape[1], 0, dtype=torch.float64), torch.zeros(logits.shape[1], 0)))
            continue
        kw = dict(masks=pred[b] if with_masks else None, coords=coords[b] if with_masks else None, stuff_takes_mean=stuff, with_boxes=with_boxes, class_mode=mode)
        out.append((reference_cost(logits[b], boxes[b], t, W_ALL, torch.float64, **kw), reference_cost(logits[b], boxes[b], t, W_ALL, torch.float32, **kw)))
    return out


def _compare(tag, Cs, refs):
    worst = 0.0
    for b, (C, (c64, c32)) in enumerate(zip(Cs, refs)):
        got = torch.from_numpy(np.array(C))
        assert got.shape == c64.shape, (tag, b)
        nan = torch.isnan(c64)
        assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(c32), nan), (tag, b, "NaN positions")
        if got.numel() == 0:
            continue
        g, r, l = got[~nan], c64[~nan], c32[~nan]
        e, e_lib, bound = err(g, r), err(l, r), bound_of(l, r)
        print("HUNG %-44s image %d err %.3e  e_lib %.3e  bound %.3e" % (tag, b, e, e_lib, bound))
        assert e <= bound, (tag, b, e, e_lib, bound)
        worst = max(worst, e / bound)
    return worst


# ------------------------------------------------------------------------------------------------ 1. costs
@pytest.mark.parametrize("key", CASES)
def test_costs_against_float64(key):
    for combo in MATRIX:
        tag = "%s-%d-%s %s boxes=%d stuff=%d masks=%d" % ((IDS(key), key[5], key[6]) + tuple(combo[:1]) + tuple(int(x) for x in combo[1:]))
        _compare(tag, _kernel_costs(key, combo), _references(key, combo))


def test_costs_with_the_production_point_count():
    key = SHAPES[3] + (0, "mixed")
    for combo in (("map", True, True, True), ("ids", False, False, True)):
        _compare("70x9 P=12544 %s" % (combo,), _kernel_costs(key, combo, P=12544), _references(key, combo, P=12544))


def test_a_target_without_positive_tokens_stays_nan():
    key = SHAPES[3] + (1, "mixed")
    targets = [dict(t) for t in hungarian_case(*key)[2]]
    targets[1]["positive_map"] = targets[1]["positive_map"].clone()
    targets[1]["positive_map"][4] = False
    for combo in (("map", True, False, False), ("map", True, False, True), ("map", False, False, False)):
        Cs = _kernel_costs(key, combo, targets=targets)
        assert bool(np.isnan(Cs[1][:, 4]).all()) and int(np.isnan(Cs[1]).sum()) == Cs[1].shape[0] and not np.isnan(Cs[0]).any()
        _compare("70x9 no positive token %s" % (combo,), Cs, _references(key, combo, targets=targets))


# ------------------------------------------------------------------------------------------------ 2. reproducibility
def test_two_calls_give_identical_bytes():
    for key, combo in ((SHAPES[5] + (0, "mixed"), ("map", True, True, False)), (SHAPES[3] + (1, "mixed"), ("ids", True, True, True)),
                       (SHAPES[4] + (0, "mixed"), ("map", True, False, False))):
        first = _kernel_costs(key, combo)
        torch.randn(1 << 20, device=DEV).sum()                    # other work in between
        second = _kernel_costs(key, combo)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes(), (key, combo)


# ------------------------------------------------------------------------------------------------ 3. assignment
def _spy(monkeypatch):
    from hipie_amd.training import functions
    answers = []

    def spied(*a, _f=functions.hungarian_costs, **k):
        answers.append(_f(*a, **k))
        return answers[-1]
    monkeypatch.setattr(functions, "hungarian_costs", spied)
    return answers


def _check_assignment(tag, pairs, blocks, refs, torch_pairs=None, must_be_separated=False):
    """(a) exact on the kernel's own block, (b) optimality in float64, (c) equality with the torch path under its precondition"""
    for b, ((q, t), C, (c64, c32)) in enumerate(zip(pairs, blocks, refs)):
        assert q.dtype == t.dtype == torch.int64
        if C.shape[1] == 0:
            assert q.numel() == 0 and t.numel() == 0
            continue
        i, j = linear_sum_assignment(np.array(C))
        assert np.array_equal(q.numpy(), i) and np.array_equal(t.numpy(), j), (tag, b, "the pairs are not scipy's on the kernel's block")
        bound = bound_of(c32, c64)
        room, over = slack(c64, bound), total_cost(c64, (q.numpy(), t.numpy())) - optimum(c64)[0]
        gap = assignment_gap(c64)
        print("HUNG %-44s image %d over the optimum %.3e  room %.3e  gap %.3e" % (tag, b, over, room, gap))
        assert over <= room, (tag, b, over, room)
        if must_be_separated:
            assert gap > room, (tag, b, gap, room)
        if torch_pairs is not None and gap > room:
            assert same_pairs([(q, t)], [torch_pairs[b]]), (tag, b)


@pytest.mark.parametrize("stuff", [True, False], ids=["stuff-mean", "own-boxes"])
@pytest.mark.parametrize("key", [pytest.param(s + (seed, "mixed"), id="%s-%d" % (IDS(s), seed)) for s in SHAPES for seed in SEEDS])
def test_assignment_on_the_kernel_costs(monkeypatch, key, stuff):
    """class + box costs with the weights (2, 5, 2)"""
    from hipie_amd.training import net
    answers = _spy(monkeypatch)
    logits, boxes, targets, _ = _device_case(key)
    cpu = hungarian_case(*key)
    pairs = HungarianMatcher(W_BOX, stuff_takes_mean=stuff, class_mode="map", ops=net.HipBackendHungarian)(logits, boxes, targets)
    assert len(answers) == 1 and answers[0] is not None
    torch_pairs = HungarianMatcher(W_BOX, stuff_takes_mean=stuff, class_mode="map")(cpu[0], cpu[1], cpu[2])
    refs = [(reference_cost(cpu[0][b], cpu[1][b], t, W_BOX, torch.float64, stuff_takes_mean=stuff),
             reference_cost(cpu[0][b], cpu[1][b], t, W_BOX, torch.float32, stuff_takes_mean=stuff)) for b, t in enumerate(cpu[2])]
    _check_assignment("%s-%d stuff=%d" % (IDS(key), key[5], stuff), pairs, answers[0], refs, torch_pairs, must_be_separated=key[:5] in SMALL)


# ------------------------------------------------------------------------------------------------ 4. the reference's own instances
def test_the_backend_gives_the_reference_fixtures(monkeypatch):
    from hipie_amd.training import net
    answers = _spy(monkeypatch)
    for name, (got, want) in Golden(DEV).run(net.HipBackendHungarian, Replay).items():
        assert same_pairs(got, want), (name, got, want)
    assert len(answers) == 5 and all(a is not None for a in answers)


def test_the_tie_instance_is_scipys_and_optimal(monkeypatch):
    from hipie_amd.training import net
    answers = _spy(monkeypatch)
    logits, boxes, targets, _, _ = golden_cases()["tie"]
    targets = [dict(targets[0], is_thing=torch.ones(3, dtype=torch.bool))]
    for stuff in (True, False):
        pairs = HungarianMatcher(W_BOX, stuff_takes_mean=stuff, class_mode="map", ops=net.HipBackendHungarian)(logits.to(DEV), boxes.to(DEV), _on(DEV, targets))
        refs = [(reference_cost(logits[0], boxes[0], targets[0], W_BOX, torch.float64, stuff_takes_mean=stuff),
                 reference_cost(logits[0], boxes[0], targets[0], W_BOX, torch.float32, stuff_takes_mean=stuff))]
        _check_assignment("tie stuff=%d" % stuff, pairs, answers[-1], refs)
    assert len(answers) == 2


# ------------------------------------------------------------------------------------------------ 5. status
def test_status_words_raise_and_name_the_image():
    from hipie_amd.training import functions
    key = SHAPES[3] + (0, "mixed")
    logits, boxes, targets, _ = _device_case(key)
    cpu_targets = hungarian_case(*key)[2]
    bad_t = [dict(t) for t in cpu_targets]
    bad_t[1]["boxes"] = cpu_targets[1]["boxes"].clone()
    bad_t[1]["boxes"][3, 2] = -0.1                                # a target box with negative width
    packed = functions.pack_match_targets(_on(DEV, bad_t), DEV)
    with pytest.raises(ValueError, match="image 1: a box with x1 < x0"):
        functions.hungarian_costs(logits, boxes, packed, W_BOX)
    assert functions.hungarian_costs(logits, boxes, packed, W_BOX, with_boxes=False) is not None          # checked with the box costs only
    bad_q = boxes.clone()
    bad_q[2, 69, 3] = float("nan")                                # a query box of the image WITHOUT targets: the torch path raises there too
    with pytest.raises(ValueError, match="image 2: a box with x1 < x0"):
        functions.hungarian_costs(logits, bad_q, functions.pack_match_targets(targets, DEV), W_BOX)
    bad_l = [dict(t) for t in cpu_targets]
    bad_l[0]["labels"] = cpu_targets[0]["labels"].clone()
    bad_l[0]["labels"][8] = 33                                    # L = 33
    packed = functions.pack_match_targets(_on(DEV, bad_l), DEV)
    with pytest.raises(ValueError, match=r"image 0: a label outside \[0, L\)"):
        functions.hungarian_costs(logits, boxes, packed, W_BOX, class_mode="ids")
    assert functions.hungarian_costs(logits, boxes, packed, W_BOX, class_mode="map") is not None


def test_a_shape_outside_the_limits_runs_the_torch_path(monkeypatch):
    from hipie_amd.training import net
    lg, bx, tg, _ = hungarian_case(1, 300, 257, 16, False, 0)
    answers = _spy(monkeypatch)
    with_ops = HungarianMatcher(W_BOX, class_mode="map", ops=net.HipBackendHungarian)(lg.to(DEV), bx.to(DEV), _on(DEV, tg))
    assert answers == [None]
    assert same_pairs(with_ops, HungarianMatcher(W_BOX, class_mode="map")(lg.to(DEV), bx.to(DEV), _on(DEV, tg)))


def test_query_slices_are_read_in_place():
    """the step hands the matcher slices of the query dimension: no copy, the same bytes as the dense operand"""
    from hipie_amd.training import functions
    key = SHAPES[3] + (0, "mixed")
    logits, boxes, targets, _ = _device_case(key)
    packed = functions.pack_match_targets(targets, DEV)
    wide_l, wide_b = torch.randn(3, 100, 33, device=DEV), torch.rand(3, 100, 4, device=DEV)
    wide_l[:, 20:90], wide_b[:, 20:90] = logits, boxes
    dense = functions.hungarian_costs(logits, boxes, packed, W_BOX)
    sliced = functions.hungarian_costs(wide_l[:, 20:90], wide_b[:, 20:90], packed, W_BOX)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dense, sliced))


# ------------------------------------------------------------------------------------------------ 6. the step
def test_train_step_with_the_hungarian_kernel_matches_the_matching_backend(monkeypatch):
    """one TrainStep forward on the small fixture model with net.HipBackendHungarian against net.HipBackendMatching: every loss entry within the
    2e-3 of the step comparisons of the opt-in loss backends (test_gpu_point_loss / test_gpu_ota_match: |a - b| / max(1, |b|)), against the
    recorded reference too, and the same matched pairs in every Hungarian matcher call (every level of the background queries, the encoder
    proposals, every MaskDINO output)."""
    from hipie_amd.training import net
    from _train_step_cases import train_step_case as _train_step_case
    seen = []
    for name in ("forward", "forward_boxes_only"):
        def recorded(self, *a, _f=getattr(HungarianMatcher, name), **k):
            out = _f(self, *a, **k)
            seen.append(out)
            return out
        monkeypatch.setattr(HungarianMatcher, name, recorded)
    answers = _spy(monkeypatch)
    runs = {}
    for be in (net.HipBackendHungarian, net.HipBackendMatching):
        del seen[:]
        z, meta, model, step, batch, targets = _train_step_case("cuda", be)
        assert step.matcher_bg.ops is be and step.md_criterion.matcher.ops is be
        with torch.enable_grad():
            losses = step.loss_dict(batch, targets)
        assert step.draws.calls == int(z["n_rand"])                               # the same random draws, in the same order
        runs[be] = ({k: float(v.detach()) for k, v in losses.items()}, list(seen))
        if be is net.HipBackendHungarian:
            n_calls = len(answers)
            assert n_calls == len(seen) and all(a is not None for a in answers)
    assert len(answers) == n_calls                                               # the other backend never asks
    (got, got_pairs), (want, want_pairs) = runs[net.HipBackendHungarian], runs[net.HipBackendMatching]
    assert len(got_pairs) == len(want_pairs) >= step.cfg["dec_layers"] + 2
    for i, (g, w) in enumerate(zip(got_pairs, want_pairs)):
        assert same_pairs(g, w), ("matcher call", i, g, w)
    recorded_ref = {k[5:]: float(z[k]) * float(z["weight/" + k[5:]]) for k in z.files if k.startswith("loss/")}
    assert sorted(got) == sorted(want) == sorted(recorded_ref)
    tol = 2e-3
    worst = max((abs(got[k] - want[k]) / max(1.0, abs(want[k])), k) for k in want)
    worst_ref = max((abs(got[k] - recorded_ref[k]) / max(1.0, abs(recorded_ref[k])), k) for k in want)
    print("HUNG step: %d Hungarian matcher calls; worst loss entry against the matching backend %.1e (%s), against the reference %.1e (%s)"
          % (n_calls, worst[0], worst[1], worst_ref[0], worst_ref[1]))
    assert worst[0] < tol and worst_ref[0] < tol, (worst, worst_ref)
