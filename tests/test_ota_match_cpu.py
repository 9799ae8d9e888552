"""CPU: the host side of csrc/ota_match.hip -- the ABI surface and the refusals of the three entry points and of the bindings (no launch),
the assignment rule restated with loops and lowest-index ties against matcher.dynamic_k_assign on every case of tests/_ota_cases.py and on
the reference's own fixtures, the `ops` plumbing of HungarianMatcher.forward_ota with a plain-torch object, the packing of ragged targets
and the place of net.HipBackendMatching among the backends."""
import ctypes

import pytest
import torch

from _ota_cases import (IDS, SEEDS, SHAPES, TorchMatchingOps, assign_rule, golden_cases, ota_case, preconditions, reference_costs, repair_case,
                        same_best, same_pairs)
from hipie_amd import _lib
from hipie_amd.training import matcher
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights

P_ = ctypes.c_void_p(256)


# ------------------------------------------------------------------------------------------------ the ABI, refusals without a launch
def _cost(lib, ptrs=None, B=2, Q=70, Tmax=9, L=33, radius=2.5, stride=32.0):
    return lib.hipie_ota_cost(*(ptrs or [P_] * 8), B, Q, Tmax, L, radius, stride, None)


def _assign(lib, ptrs=None, B=2, Q=70, Tmax=9):
    return lib.hipie_ota_assign(*(ptrs or [P_] * 9), B, Q, Tmax, None)


def test_abi_surface():
    c_p, c_i, c_l, c_f = _lib.c_p, _lib.c_i, _lib.c_l, _lib.c_f
    assert _lib.SIGNATURES["hipie_ota_cost"] == [c_p] * 8 + [c_l, c_i, c_i, c_i, c_f, c_f, c_p]
    assert _lib.SIGNATURES["hipie_ota_assign"] == [c_p] * 9 + [c_l, c_i, c_i, c_p]
    assert _lib.SIGNATURES["hipie_ota_match_ws_bytes"] == [c_l, c_l, c_l]
    lib = _lib.load()
    for name in ("hipie_ota_cost", "hipie_ota_assign", "hipie_ota_match_ws_bytes"):
        assert hasattr(lib, name)
    assert lib.hipie_ota_match_ws_bytes.restype is ctypes.c_int64
    for B, Q, T in ((1, 4, 3), (2, 900, 100), (3, 4096, 256), (70000, 4096, 256)):
        assert lib.hipie_ota_match_ws_bytes(B, Q, T) >= 2 * B * T * Q * 4
    assert lib.hipie_ota_match_ws_bytes(0, 4, 3) > 0


def test_limits_and_null_pointers_are_refused_without_a_launch():
    lib = _lib.load()
    for kw, msg in (({"Q": 4097}, b"Q=4097"), ({"Tmax": 257}, b"Tmax=257"), ({"L": 1025}, b"L=1025"), ({"L": 0}, b"L=0"), ({"B": -1}, b"negative"),
                    ({"B": 65536}, b"exceed the grid"), ({"stride": 0.0}, b"stride")):
        assert _cost(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    for kw, msg in (({"Q": 4097}, b"Q=4097"), ({"Tmax": 257}, b"Tmax=257"), ({"Q": -1}, b"negative")):
        assert _assign(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    for i in range(8):
        assert _cost(lib, [None if j == i else P_ for j in range(8)]) == -22 and b"null" in lib.hipie_last_error(), i
    for i in range(9):
        assert _assign(lib, [None if j == i else P_ for j in range(9)]) == -22 and b"null" in lib.hipie_last_error(), i
    # at the limits the size check passes and the null pointer trips
    assert _cost(lib, [None] * 8, Q=4096, Tmax=256, L=1024) == -22 and b"null" in lib.hipie_last_error()
    assert _assign(lib, [None] * 9, Q=4096, Tmax=256) == -22 and b"null" in lib.hipie_last_error()


def test_empty_problems_return_without_a_launch():
    lib = _lib.load()
    for B, Q, T in ((0, 70, 9), (2, 0, 9), (2, 70, 0), (0, 0, 0)):
        assert _cost(lib, [None] * 8, B=B, Q=Q, Tmax=T) == 0
        assert _assign(lib, [None] * 9, B=B, Q=Q, Tmax=T) == 0


def test_bindings_refuse_before_the_device_is_asked():
    from hipie_amd import ops
    lg, bx, tb = torch.zeros(2, 7, 5), torch.zeros(2, 7, 4), torch.zeros(2, 3, 4)
    pm, n = torch.zeros(2, 3, 5, dtype=torch.uint8), torch.tensor([3, 1], dtype=torch.int32)
    for args, msg in (((lg.double(), bx, tb, pm, n), "logits must be torch.float32"), ((lg[0], bx, tb, pm, n), "logits must have 3 dimensions"),
                      ((lg, torch.zeros(2, 7, 3), tb, pm, n), r"boxes must be \(2, 7, 4\)"), ((lg, bx, tb.transpose(0, 1), pm, n), "tgt_boxes tensor has to be contiguous"),
                      ((lg, bx, tb, pm.bool(), n), "pos_map must be torch.uint8"), ((lg, bx, tb, pm[:, :, :4], n), r"pos_map must be \(2, 3, 5\)"),
                      ((lg, bx, tb, pm, n.long()), "n_tgt must be torch.int32"), ((lg, bx, tb, pm, n[:1]), r"n_tgt must be \(2,\)")):
        with pytest.raises(RuntimeError, match=msg):
            ops.ota_cost(*args)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.ota_cost(lg, bx, tb, pm, n)
    cost = torch.zeros(2, 3, 7)
    for args, msg in (((cost.double(), cost, n), "cost must be torch.float32"), ((cost, cost[:, :2], n), r"iou must be \(2, 3, 7\)"),
                      ((cost, cost, n.long()), "n_tgt must be torch.int32"), ((cost, cost, n, torch.zeros(2, 2, dtype=torch.int32)), r"res must be \(3, 2\)")):
        with pytest.raises(RuntimeError, match=msg):
            ops.ota_assign(*args)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.ota_assign(cost, cost.clone(), n)
    assert ops.ota_match_ws_bytes(2, 7, 3) >= 2 * 2 * 3 * 7 * 4
    assert (ops.OTA_MAX_Q, ops.OTA_MAX_T, ops.OTA_MAX_L) == (4096, 256, 1024)


# ------------------------------------------------------------------------------------------------ the rule
def _rule_is_the_reference(cost, iou):
    want_cost = cost.clone()
    (wq, wt), wbest = matcher.dynamic_k_assign(want_cost, iou.clone())
    (gq, gt), gbest, got_cost, rounds = assign_rule(cost, iou)
    assert torch.equal(gq, wq) and torch.equal(gt, wt) and torch.equal(gbest, wbest)
    kept = torch.isfinite(want_cost)                           # the reference's last step puts +inf on everything unmatched
    assert torch.equal(got_cost[kept], want_cost[kept]) and int(kept.sum()) >= cost.shape[1]
    return rounds


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_restated_rule_is_dynamic_k_assign(shape, seed):
    case = ota_case(*shape, seed)
    for ref in preconditions(case):
        if ref is not None:
            _rule_is_the_reference(ref[2], ref[3])


def test_the_repair_case_runs_the_repair_loop():
    case = repair_case()
    (c64, i64, c32, i32), = preconditions(case, ties_allowed=True)
    assert torch.equal(c32[:, 0], c32[:, 1]) and torch.equal(c32[:, 0], c32[:, 2])          # three identical columns
    assert _rule_is_the_reference(c32, i32) >= 1


def test_the_restated_rule_on_the_reference_fixtures():
    for name, (logits, boxes, targets, pairs, best) in golden_cases().items():
        for b, t in enumerate(targets):
            if len(t["boxes"]) == 0:
                continue
            cost, iou = reference_costs(logits[b], boxes[b], t, torch.float32)
            _rule_is_the_reference(cost, iou)
            got, gbest, _, _ = assign_rule(cost, iou)
            assert same_pairs([got], [pairs[b]]) and torch.equal(gbest, best[b]), (name, b)


def test_rule_ties_go_to_the_lowest_index():
    cost = torch.tensor([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]])          # every entry ties
    iou = torch.full((3, 2), 0.1)
    (q, t), best, final, rounds = assign_rule(cost, iou)
    # both targets take query 0; it keeps target 0; the repair round moves it back and target 1 takes query 1
    assert q.tolist() == [0, 1] and t.tolist() == [0, 1] and best.tolist() == [0, 1] and rounds == 1
    assert final.tolist() == [[100001.0, 100001.0], [1.0, 1.0], [1.0, 1.0]]


# ------------------------------------------------------------------------------------------------ the plumbing
def test_forward_ota_asks_the_ops_object_first():
    TorchMatchingOps.calls = 0
    for name, (logits, boxes, targets, pairs, best) in golden_cases().items():
        before = TorchMatchingOps.calls
        m = HungarianMatcher(MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0), class_mode="map", ops=TorchMatchingOps)
        got, gbest = m.forward_ota(logits, boxes, targets)
        assert TorchMatchingOps.calls == before + 1
        assert same_pairs(got, pairs) and same_best(gbest, best), name
        packed = m.pack_ota(targets, "cpu")                      # packed once by the caller: the same answer
        again, abest = m.forward_ota(logits, boxes, targets, packed=packed)
        assert same_pairs(again, pairs) and same_best(abest, best) and TorchMatchingOps.calls == before + 2
        plain = HungarianMatcher(MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0), class_mode="map")
        assert plain.pack_ota(targets, "cpu") is None
        want, wbest = plain.forward_ota(logits, boxes, targets)
        assert same_pairs(want, pairs) and same_best(wbest, best)


def test_forward_ota_falls_through_when_the_op_declines():
    class Declines(TorchMatchingOps):
        asked = 0

        @classmethod
        def ota_match(cls, logits, boxes, packed, center_radius=2.5, stride=32):
            cls.asked += 1
            return None
    logits, boxes, targets, pairs, best = golden_cases()["ota"]
    got, gbest = HungarianMatcher(class_mode="map", ops=Declines).forward_ota(logits, boxes, targets)
    assert Declines.asked == 1 and same_pairs(got, pairs) and same_best(gbest, best)


def test_pack_ota_targets_round_trips_ragged_targets():
    from hipie_amd.training.functions import pack_ota_targets
    logits, boxes, targets = ota_case(2, 70, 9, 33, True, 0)
    p = pack_ota_targets(targets, "cpu")
    assert p.counts == [9, 6, 0] and p.n_tgt.dtype == torch.int32 and p.n_tgt.tolist() == p.counts
    assert p.tgt_boxes.shape == (3, 9, 4) and p.tgt_boxes.dtype == torch.float32 and p.pos_map.shape == (3, 9, 33) and p.pos_map.dtype == torch.uint8
    for b, t in enumerate(targets):
        n = p.counts[b]
        assert torch.equal(p.tgt_boxes[b, :n], t["boxes"]) and torch.equal(p.pos_map[b, :n].bool(), t["positive_map"])
        assert not p.tgt_boxes[b, n:].any() and not p.pos_map[b, n:].any()
    none = pack_ota_targets([targets[2]], "cpu")
    assert none.counts == [0] and none.tgt_boxes.shape == (1, 0, 4)
    with pytest.raises(ValueError, match="positive_map of image 1"):
        pack_ota_targets([targets[0], dict(targets[1], positive_map=targets[1]["positive_map"][:, :5])], "cpu")


def test_ota_match_declines_and_short_cuts_on_the_host():
    from hipie_amd.training import functions
    logits, boxes, targets = ota_case(2, 70, 9, 33, True, 0)
    packed = functions.pack_ota_targets(targets, "cpu")
    assert functions.ota_match(torch.zeros(3, 4097, 33), torch.zeros(3, 4097, 4), packed) is None          # outside the limits: no launch
    with pytest.raises(ValueError, match="packed for 3 images"):
        functions.ota_match(logits[:2], boxes[:2], packed)
    none = functions.pack_ota_targets([targets[2]] * 2, "cpu")
    pairs, best = functions.ota_match(logits[:2], boxes[:2], none)                                       # no target anywhere: no launch
    assert best == [[], []] and all(p[0].numel() == 0 and p[0].dtype == torch.int64 and p[1].numel() == 0 for p in pairs)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        functions.ota_match(logits, boxes, packed)


def test_backend_matching_is_opt_in():
    from hipie_amd.training import net
    from hipie_amd.training.step import TrainStep      # noqa: F401
    assert issubclass(net.HipBackendMatching, net.HipBackendCriteria)
    for be in (net.HipBackend, net.HipBackendLosses, net.HipBackendCriteria, net.HipBackendAll):
        assert not hasattr(be, "ota_match") and not hasattr(be, "pack_ota_targets") and not issubclass(net.HipBackendAll, net.HipBackendMatching)
    assert HungarianMatcher().ops is None and HungarianMatcher().pack_ota([], "cpu") is None
    logits, boxes, targets = ota_case(1, 4, 3, 8, False, 0)
    packed = net.HipBackendMatching.pack_ota_targets(targets, "cpu")
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendMatching.ota_match(logits, boxes, packed)
