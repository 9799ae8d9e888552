"""GPU: hipie_ota_cost and hipie_ota_assign (csrc/ota_match.hip) through the ops, functions.ota_match and the opt-in net.HipBackendMatching
wiring of HungarianMatcher.forward_ota and TrainStep.

Costs: tests/_ota_cases.py -- matcher.ota_cost in float64 on the CPU as the reference, in float32 as e_lib, the two penalty terms compared as
masks first; every case prints its figures (lines starting with OTA) before it asserts.  Assignment: matcher.dynamic_k_assign on the CPU on
a copy of the kernel's own cost and iou, no tolerance -- pairs, best, repair rounds and the final cost bit for bit.  Each case runs the two
kernels once (`_run`) and the tests share what they returned."""
import functools

import pytest
import torch

from _ota_cases import (IDS, SEEDS, SHAPES, assign_rule, bound_of, centre_masks, err, golden_cases, masks_of_cost, ota_case, preconditions, repair_case,
                        same_best, same_pairs)
from hipie_amd.training import matcher
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [pytest.param(("case",) + s + (seed,), id="%s-%d" % (IDS(s), seed)) for s in SHAPES for seed in SEEDS] + [pytest.param(("repair",), id="repair")]


def _case(key):
    return repair_case() if key[0] == "repair" else ota_case(*key[1:])


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _kernels(case):
    """the two kernels on one case -> everything they wrote, on the CPU; cost0 / iou0: the copy taken between the two launches"""
    from hipie_amd import ops
    from hipie_amd.training.functions import pack_ota_targets
    logits, boxes, targets = case
    p = pack_ota_targets(targets, DEV)
    cost, iou, res = ops.ota_cost(logits.to(DEV), boxes.to(DEV), p.tgt_boxes, p.pos_map, p.n_tgt)
    assert cost.shape == iou.shape == (logits.shape[0], p.tgt_boxes.shape[1], logits.shape[1]) and cost.dtype == iou.dtype == torch.float32
    cost0, iou0, status0 = cost.cpu().clone(), iou.cpu().clone(), res[1].cpu().clone()
    pair_q, pair_t, best, res2 = ops.ota_assign(cost, iou, p.n_tgt, res)
    assert res2 is res and pair_q.dtype == pair_t.dtype == best.dtype == torch.int32 and torch.equal(iou.cpu(), iou0)
    return dict(counts=p.counts, cost0=cost0, iou0=iou0, status0=status0, cost=cost.cpu(), pair_q=pair_q.cpu(), pair_t=pair_t.cpu(), best=best.cpu(),
                res=res.cpu())


@functools.lru_cache(maxsize=None)
def _run(key):
    return _kernels(_case(key))


# ------------------------------------------------------------------------------------------------ costs
@pytest.mark.parametrize("key", CASES)
def test_costs_against_float64(key):
    case = _case(key)
    refs = preconditions(case, ties_allowed=key[0] == "repair")
    out = _run(key)
    assert out["status0"].tolist() == [0] * len(refs)
    for b, ref in enumerate(refs):
        n = out["counts"][b]
        assert bool((out["cost0"][b, n:] == float("inf")).all()) and bool((out["iou0"][b, n:] == 0).all())          # behind n_tgt: defined
        if ref is None:
            continue
        c64, i64, c32, i32 = ref
        cost, iou = out["cost0"][b, :n].t(), out["iou0"][b, :n].t()
        # the +100 / +10000 terms, as masks, entry for entry
        far, none = centre_masks(case[1][b], case[2][b])
        got_far, got_none = masks_of_cost(cost)
        assert torch.equal(masks_of_cost(c64)[0], far) and torch.equal(masks_of_cost(c64)[1], none)          # the masks read off a cost are its masks
        assert torch.equal(got_far, far) and torch.equal(got_none, none), (b, int((got_far != far).sum()), int((got_none != none).sum()))
        # the magnitudes, per tensor
        for name, g, r, l in (("cost", cost, c64, c32), ("iou", iou, i64, i32)):
            print("OTA %-22s image %d %-5s err %.3e  e_lib %.3e  bound %.3e" % ("-".join(map(str, key[1:])) or "repair", b, name, err(g, r), err(l, r), bound_of(l, r)))
            assert err(g, r) <= bound_of(l, r), (name, b)
        # the entries without a penalty are not hidden behind the 10000s: the same yardstick on them alone
        plain = ~far & ~none[:, None]
        if bool(plain.any()):
            g, r, l = cost[plain], c64[plain], c32[plain]
            print("OTA %-22s image %d plain err %.3e  e_lib %.3e  bound %.3e  (%d entries)" % ("-".join(map(str, key[1:])) or "repair", b, err(g, r), err(l, r),
                                                                                            bound_of(l, r), int(plain.sum())))
            assert err(g, r) <= bound_of(l, r), ("plain", b)


# ------------------------------------------------------------------------------------------------ assignment
@pytest.mark.parametrize("key", CASES)
def test_assignment_is_dynamic_k_assign_on_the_kernel_costs(key):
    case = _case(key)
    preconditions(case, ties_allowed=key[0] == "repair")
    out = _run(key)
    n_pairs, status, rounds = out["res"].tolist()
    assert status == [0] * len(out["counts"])
    ran = 0
    for b, n in enumerate(out["counts"]):
        got = (out["pair_q"][b, :n_pairs[b]].long(), out["pair_t"][b, :n_pairs[b]].long())
        assert bool((out["cost"][b, n:] == float("inf")).all())
        if n == 0:
            assert n_pairs[b] == 0 and rounds[b] == 0
            continue
        cost0, iou0 = out["cost0"][b, :n].t().contiguous(), out["iou0"][b, :n].t().contiguous()
        want_cost = cost0.clone()
        want, want_best = matcher.dynamic_k_assign(want_cost, iou0.clone())
        rule, rule_best, rule_cost, rule_rounds = assign_rule(cost0, iou0)
        assert same_pairs([rule], [want]) and torch.equal(rule_best, want_best)                      # the rule the kernel is written to, on these very inputs
        assert same_pairs([got], [want]), (b, got, want)
        assert torch.equal(out["best"][b, :n].long(), want_best), (b, out["best"][b, :n], want_best)
        assert rounds[b] == rule_rounds
        final = out["cost"][b, :n].t().contiguous()
        kept = torch.isfinite(want_cost)                          # the reference's last step: +inf on everything unmatched
        assert torch.equal(_bits(final)[kept], _bits(want_cost)[kept]) and int(kept.sum()) >= n
        assert torch.equal(_bits(final), _bits(rule_cost))        # and elsewhere what the reference held before that step
        ran += rounds[b]
    print("OTA %-22s pairs %s  repair rounds %s" % ("-".join(map(str, key[1:])) or "repair", n_pairs, rounds))
    if key[0] == "repair":
        assert ran >= 1


def test_the_cases_run_the_repair_loop_and_wide_rows():
    """what the cases are there for: some of the seeded cases enter the repair loop, and the 37- and 100-target ones use several bitmap words"""
    assert sum(sum(_run(k.values[0])["res"][2].tolist()) for k in CASES) >= 3
    for shape, words in ((SHAPES[3], 2), (SHAPES[4], 4)):
        out = _run(("case",) + shape + (0,))
        assert int(out["pair_t"][0, :int(out["res"][0, 0])].max()) >= 32 * (words - 1)


def test_two_calls_give_identical_bits():
    for key in (("case",) + SHAPES[4] + (0,), ("case",) + SHAPES[2] + (1,), ("repair",)):
        first = _run(key)
        torch.randn(1 << 20, device=DEV).sum()                    # other work in between
        second = _kernels(_case(key))
        for k in ("cost0", "iou0", "cost", "best", "res"):
            assert torch.equal(_bits(first[k]), _bits(second[k])), (key, k)
        for b, n in enumerate(first["res"][0].tolist()):          # the compacted lists are written up to n_pairs
            assert torch.equal(first["pair_q"][b, :n], second["pair_q"][b, :n]) and torch.equal(first["pair_t"][b, :n], second["pair_t"][b, :n])


# ------------------------------------------------------------------------------------------------ the wiring
def _on(dev, targets):
    return [{k: v.to(dev) for k, v in t.items()} for t in targets]


def _spy(monkeypatch):
    from hipie_amd.training import functions
    answers = []

    def spied(*a, _f=functions.ota_match, **k):
        answers.append(_f(*a, **k))
        return answers[-1]
    monkeypatch.setattr(functions, "ota_match", spied)
    return answers


def test_forward_ota_with_the_backend_gives_the_reference_fixtures(monkeypatch):
    from hipie_amd.training import net
    answers = _spy(monkeypatch)
    for name, (logits, boxes, targets, pairs, best) in golden_cases().items():
        m = HungarianMatcher(MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0), class_mode="map", ops=net.HipBackendMatching)
        got, gbest = m.forward_ota(logits.to(DEV), boxes.to(DEV), _on(DEV, targets))
        assert len(answers) > 0 and answers[-1] is not None
        assert same_pairs(got, pairs) and same_best(gbest, best), (name, got, pairs, gbest, best)
        for (q, t), bq in zip(got, gbest):
            assert q.dtype == t.dtype == torch.int64 and q.is_cuda and t.is_cuda
            assert bq == [] or (bq.dtype == torch.int64 and bq.is_cuda)
    assert len(answers) == 2
    assert answers[0][1][2] == [] and answers[0][0][2][0].numel() == 0          # the image without targets: the empty pair and []


def test_refusals(monkeypatch):
    from hipie_amd.training import functions, net
    logits, boxes, targets = ota_case(2, 70, 9, 33, True, 0)
    packed = functions.pack_ota_targets(targets, DEV)
    assert functions.ota_match(logits.to(DEV), boxes.to(DEV), packed) is not None
    bad = boxes.clone()
    bad[1, 40, 2] = -0.1                                          # x1 < x0
    with pytest.raises(ValueError, match="image 1: a box with x1 < x0"):
        functions.ota_match(logits.to(DEV), bad.to(DEV), packed)
    bad_t = [dict(t) for t in targets]
    bad_t[0]["boxes"] = targets[0]["boxes"].clone()
    bad_t[0]["boxes"][8, 3] = -0.2                                # a target box with y1 < y0
    with pytest.raises(ValueError, match="image 0: a box with x1 < x0 or y1 < y0"):
        functions.ota_match(logits.to(DEV), boxes.to(DEV), functions.pack_ota_targets(bad_t, DEV))
    no_tok = [dict(t) for t in targets]
    no_tok[1]["positive_map"] = targets[1]["positive_map"].clone()
    no_tok[1]["positive_map"][5] = False
    with pytest.raises(ValueError, match="image 1: a target without a positive token"):
        functions.ota_match(logits.to(DEV), boxes.to(DEV), functions.pack_ota_targets(no_tok, DEV))
    # more targets than the bitmap holds: the op declines and forward_ota answers through its torch path
    lg, bx, tg = ota_case(1, 300, 257, 16, False, 0)
    answers = _spy(monkeypatch)
    with_ops = HungarianMatcher(class_mode="map", ops=net.HipBackendMatching).forward_ota(lg.to(DEV), bx.to(DEV), _on(DEV, tg))
    assert answers == [None]
    without = HungarianMatcher(class_mode="map").forward_ota(lg.to(DEV), bx.to(DEV), _on(DEV, tg))
    assert same_pairs(with_ops[0], without[0]) and same_best(with_ops[1], without[1]) and len(with_ops[0][0][0]) >= 257


# ------------------------------------------------------------------------------------------------ the step
def test_train_step_with_the_matching_kernels_matches_the_reference(monkeypatch):
    """test_gpu_point_loss.test_train_step_with_the_loss_kernels_matches_the_reference with backend=net.HipBackendMatching: the same fixture, the
    same assertions and bounds (loss entries 2e-3, the three gradient classes 5e-3 / 5e-3 / 8e-2, the same random draws); the SimOTA matching
    of every decoder level goes through the kernels."""
    from hipie_amd.training import net
    from _train_step_cases import check_step_against_golden, train_step_case
    z, meta, model, step, batch, targets = train_step_case("cuda", net.HipBackendMatching)
    assert step.matcher.ops is net.HipBackendMatching and step.criterion.ops is net.HipBackendMatching
    answers = _spy(monkeypatch)
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    assert len(answers) == step.cfg["dec_layers"] and all(a is not None for a in answers)
    print("OTA step: %d matching calls, pairs per call %s" % (len(answers), [sum(len(p[0]) for p in a[0]) for a in answers]))
    check_step_against_golden(z, model, step, losses, total, "cuda", "OTA step")
