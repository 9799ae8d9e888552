"""CPU: the host side of csrc/hungarian_cost.hip -- the ABI surface and the refusals of the entry point and of the bindings (no launch), the
packing of ragged targets, the `ops` plumbing of HungarianMatcher.forward / forward_boxes_only with a plain-torch object that restates the
packed layout (same draws in the same order, fall-back when the op declines), every recorded Hungarian pair set of the reference through
that plumbing, the yardsticks of the GPU tests on the seeded cases, and the place of net.HipBackendHungarian among the backends."""
import ctypes

import numpy as np
import pytest
import torch

from _hungarian_cases import (IDS, SEEDS, SHAPES, SMALL, W_BOX, Golden, TorchHungarianOps, assignment_gap, bound_of, hungarian_case, optimum,
                              reference_cost, same_pairs, slack, total_cost)
from hipie_amd import _lib
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights, assign, assign_host
from test_training import Replay

P_ = ctypes.c_void_p(256)
NAMES = ("logits", "boxes", "tgt_boxes", "n_tgt", "t_off", "pos_map", "labels", "is_thing", "ce", "dice", "C", "status", "ws")


def _cost(lib, B=2, Q=70, Tmax=9, L=33, sum_t=15, with_boxes=1, stuff=1, ls=None, bs=None, ws_bytes=1 << 20, **ptrs):
    """the entry with made-up pointers (map mode, no mask costs unless `ptrs` says otherwise): only calls that are refused or return early"""
    v = dict({k: P_ for k in NAMES}, labels=None, ce=None, dice=None)
    v.update(ptrs)
    return lib.hipie_hungarian_cost(v["logits"], Q * L if ls is None else ls, v["boxes"], Q * 4 if bs is None else bs, v["tgt_boxes"], v["n_tgt"], v["t_off"],
                                    v["pos_map"], v["labels"], v["is_thing"], v["ce"], v["dice"], v["C"], v["status"], v["ws"], ws_bytes, B, Q, Tmax, L, sum_t,
                                    2.0, 5.0, 2.0, 5.0, 5.0, with_boxes, stuff, None)


# ------------------------------------------------------------------------------------------------ the ABI, refusals without a launch
def test_abi_surface():
    c_p, c_i, c_l, c_f = _lib.c_p, _lib.c_i, _lib.c_l, _lib.c_f
    assert _lib.SIGNATURES["hipie_hungarian_cost"] == [c_p, c_l, c_p, c_l] + [c_p] * 11 + [c_l, c_l, c_i, c_i, c_i, c_l] + [c_f] * 5 + [c_i, c_i, c_p]
    lib = _lib.load()
    for name in ("hipie_hungarian_cost", "hipie_hungarian_cost_bytes", "hipie_hungarian_cost_ws_bytes"):
        assert hasattr(lib, name)
    assert lib.hipie_hungarian_cost_bytes.restype is ctypes.c_int64 and lib.hipie_hungarian_cost_ws_bytes.restype is ctypes.c_int64
    assert lib.hipie_hungarian_cost_bytes(70, 15) == 70 * 15 * 4 and lib.hipie_hungarian_cost_bytes(70, 0) == 0
    for B, Q in ((1, 4), (2, 900), (3, 4096), (65535, 4096)):
        assert lib.hipie_hungarian_cost_ws_bytes(B, Q) >= B * -(-Q // 64) * 16
    assert lib.hipie_hungarian_cost_ws_bytes(0, 4) > 0


def test_limits_and_null_pointers_are_refused_without_a_launch():
    lib = _lib.load()
    for kw, msg in (({"Q": 4097}, b"Q=4097"), ({"Tmax": 257}, b"Tmax=257"), ({"L": 1025}, b"L=1025"), ({"L": 0}, b"L=0"), ({"B": -1}, b"negative"),
                    ({"B": 65536}, b"exceed the grid"), ({"sum_t": 19}, b"sum_t=19"), ({"sum_t": -1}, b"negative"),
                    ({"labels": P_}, b"exactly one of pos_map and labels"), ({"pos_map": None}, b"exactly one of pos_map and labels"),
                    ({"ce": P_}, b"ce and dice come together"), ({"dice": P_}, b"ce and dice come together"), ({"ls": 70 * 33 - 1}, b"image strides"),
                    ({"bs": 70 * 4 - 1}, b"image strides"), ({"ws_bytes": 2 * 2 * 16 - 1}, b"workspace"), ({"ws": ctypes.c_void_p(260)}, b"workspace")):
        assert _cost(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    for name in ("logits", "n_tgt", "t_off", "C", "status", "boxes", "tgt_boxes", "is_thing", "ws"):
        assert _cost(lib, **{name: None}) == -22 and b"null" in lib.hipie_last_error(), name
    # at the limits the size check passes and the null pointer trips
    assert _cost(lib, Q=4096, Tmax=256, L=1024, ls=4096 * 1024, bs=4096 * 4, logits=None) == -22 and b"null" in lib.hipie_last_error()


def test_empty_problems_return_without_a_launch():
    lib = _lib.load()
    none = {k: None for k in NAMES}
    for B, Q, T in ((0, 70, 9), (2, 0, 9), (2, 70, 0), (0, 0, 0)):
        assert _cost(lib, B=B, Q=Q, Tmax=T, sum_t=0, **none) == 0


def test_bindings_refuse_before_the_device_is_asked():
    from hipie_amd import ops
    lg, bx, tb = torch.zeros(2, 7, 5), torch.zeros(2, 7, 4), torch.zeros(2, 3, 4)
    pm, lab, th = torch.zeros(2, 3, 5, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.int32), torch.ones(2, 3, dtype=torch.uint8)
    n, off, w = torch.tensor([3, 1], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32), (2.0, 5.0, 2.0, 5.0, 5.0)
    ok = dict(pos_map=pm, is_thing=th)
    for args, kw, msg in (((lg.double(), bx, tb, n, off, 4, w), ok, "logits must be torch.float32"), ((lg[0], bx, tb, n, off, 4, w), ok, r"logits must be \(B, Q"),
                          ((lg.transpose(1, 2), bx, tb, n, off, 4, w), ok, "logits tensor has to be dense within an image"),
                          ((lg, torch.zeros(2, 6, 4), tb, n, off, 4, w), ok, r"boxes must be \(2, 7, 4\)"), ((lg, None, tb, n, off, 4, w), ok, "boxes are needed"),
                          ((lg, bx, tb.transpose(0, 1), n, off, 4, w), ok, "tgt_boxes"), ((lg, bx, tb, n.long(), off, 4, w), ok, "n_tgt must be torch.int32"),
                          ((lg, bx, tb, n, off[:1], 4, w), ok, r"t_off must be \(2,\)"), ((lg, bx, tb, n, off, 4, w), dict(is_thing=th), "exactly one of pos_map and labels"),
                          ((lg, bx, tb, n, off, 4, w), dict(ok, labels=lab), "exactly one of pos_map and labels"),
                          ((lg, bx, tb, n, off, 4, w), dict(ok, pos_map=pm.bool()), "pos_map must be torch.uint8"),
                          ((lg, bx, tb, n, off, 4, w), dict(labels=lab.long(), is_thing=th), "labels must be torch.int32"),
                          ((lg, bx, tb, n, off, 4, w), dict(pos_map=pm), "is_thing is needed"), ((lg, bx, tb, n, off, 4, w), dict(ok, ce=torch.zeros(28)), "ce and dice come together"),
                          ((lg, bx, tb, n, off, 4, w), dict(ok, ce=torch.zeros(28), dice=torch.zeros(27)), r"dice must be \(28,\)"),
                          ((lg, bx, tb, n, off, 7, w), ok, "sum_t=7"), ((lg, bx, tb, n, off, 4, w), dict(ok, out=torch.zeros(28)), r"out must be \(30,\)")):
        with pytest.raises(RuntimeError, match=msg):
            ops.hungarian_cost(*args, **kw)
    # the shapes outside the kernel's limits, on host tensors: refused before the device is asked
    for B, Q, T, L, msg in ((1, 4097, 3, 5, "Q=4097"), (1, 7, 257, 5, "Tmax=257"), (1, 7, 3, 1025, "L=1025")):
        with pytest.raises(RuntimeError, match=msg + ".*outside"):
            ops.hungarian_cost(torch.zeros(B, Q, L), torch.zeros(B, Q, 4), torch.zeros(B, T, 4), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32), 0, w,
                               pos_map=torch.zeros(B, T, L, dtype=torch.uint8), is_thing=torch.zeros(B, T, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.hungarian_cost(lg, bx, tb, n, off, 4, w, **ok)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.hungarian_cost(lg[:, 1:6], None, tb, n, off, 4, w, labels=lab, with_boxes=False)          # a slice of the query dimension is taken as it is
    assert (ops.HUNGARIAN_MAX_Q, ops.HUNGARIAN_MAX_T, ops.HUNGARIAN_MAX_L) == (4096, 256, 1024)
    # the output views of the mask costs
    pred, tgt, pts = torch.zeros(7, 4, 4), torch.zeros(3, 8, 8), torch.zeros(5, 2)
    for kw, msg in ((dict(ce_out=torch.zeros(7, 3)), "ce_out and dice_out come together"), (dict(ce_out=torch.zeros(7, 3), dice_out=torch.zeros(3, 7)), r"dice_out must be \(7, 3\)"),
                    (dict(ce_out=torch.zeros(3, 7).t(), dice_out=torch.zeros(7, 3)), "ce_out tensor has to be contiguous"),
                    (dict(ce_out=torch.zeros(7, 3), dice_out=torch.zeros(7, 3)), "Not implemented on the CPU")):
        with pytest.raises(RuntimeError, match=msg):
            ops.mask_match_cost(pred, tgt, pts, **kw)


# ------------------------------------------------------------------------------------------------ the packing
def test_pack_match_targets_pads_and_offsets_ragged_targets():
    from hipie_amd.training.functions import pack_match_targets
    logits, boxes, targets, pred = hungarian_case(2, 70, 9, 33, True, 0)
    p = pack_match_targets(targets, "cpu")
    assert p.counts == [9, 6, 0] and p.n_tgt.dtype == p.t_off.dtype == torch.int32 and p.n_tgt.tolist() == [9, 6, 0] and p.t_off.tolist() == [0, 9, 15]
    assert p.tgt_boxes.shape == (3, 9, 4) and p.tgt_boxes.dtype == torch.float32 and p.pos_map.shape == (3, 9, 33) and p.pos_map.dtype == torch.uint8
    assert p.labels.shape == (3, 9) and p.labels.dtype == torch.int32 and p.is_thing.shape == (3, 9) and p.is_thing.dtype == torch.uint8
    for b, t in enumerate(targets):
        n = p.counts[b]
        assert torch.equal(p.tgt_boxes[b, :n], t["boxes"]) and torch.equal(p.pos_map[b, :n].bool(), t["positive_map"])
        assert torch.equal(p.labels[b, :n].long(), t["labels"]) and torch.equal(p.is_thing[b, :n].bool(), t["is_thing"])
        assert not p.tgt_boxes[b, n:].any() and not p.pos_map[b, n:].any() and not p.labels[b, n:].any() and not p.is_thing[b, n:].any()
        assert p.tgt_masks[b] is None if n == 0 else (p.tgt_masks[b].dtype == torch.float32 and torch.equal(p.tgt_masks[b], t["masks"]))
    assert pack_match_targets(targets, "cpu", with_masks=False).tgt_masks is None
    none = pack_match_targets([targets[2]], "cpu")
    assert none.counts == [0] and none.tgt_boxes.shape == (1, 0, 4) and none.t_off.tolist() == [0]
    ids_only = pack_match_targets([{k: v for k, v in t.items() if k not in ("positive_map", "is_thing")} for t in targets], "cpu")
    assert ids_only.pos_map is None and ids_only.labels is not None and bool(ids_only.is_thing[0, :9].all())          # no is_thing: every target a thing
    with pytest.raises(ValueError, match="positive_map of image 1"):
        pack_match_targets([targets[0], dict(targets[1], positive_map=targets[1]["positive_map"][:, :5])], "cpu")


def test_hungarian_costs_declines_and_short_cuts_on_the_host():
    from hipie_amd.training import functions
    logits, boxes, targets, pred = hungarian_case(2, 70, 9, 33, True, 0)
    packed = functions.pack_match_targets(targets, "cpu")
    assert functions.hungarian_costs(torch.zeros(3, 4097, 33), torch.zeros(3, 4097, 4), packed, W_BOX) is None          # outside the limits: no launch
    with pytest.raises(ValueError, match="packed for 3 images"):
        functions.hungarian_costs(logits[:2], boxes[:2], packed, W_BOX)
    with pytest.raises(ValueError, match="packed for 33 tokens"):
        functions.hungarian_costs(logits[..., :8], boxes, packed, W_BOX)
    with pytest.raises(KeyError, match="without masks"):
        functions.hungarian_costs(logits, boxes, functions.pack_match_targets(targets, "cpu", False), W_BOX, masks=pred, coords=[None] * 3)
    none = functions.pack_match_targets([targets[2]] * 2, "cpu")
    Cs = functions.hungarian_costs(logits[:2], boxes[:2], none, W_BOX)                                   # no target anywhere: no launch
    assert [C.shape for C in Cs] == [(70, 0), (70, 0)]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        functions.hungarian_costs(logits, boxes, packed, W_BOX)


# ------------------------------------------------------------------------------------------------ the plumbing
class Recording:
    """a `draw` that records what it was asked for and answers from a seeded generator"""

    def __init__(self):
        self.asked, self.g = [], torch.Generator().manual_seed(11)

    def __call__(self, shape, device):
        self.asked.append(tuple(shape))
        return torch.rand(shape, generator=self.g).to(device)


def test_the_matcher_asks_the_ops_object_first_and_draws_as_the_torch_path():
    logits, boxes, targets, pred = hungarian_case(2, 70, 9, 33, True, 0)
    w = MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0)
    plain_draw, ops_draw, declined_draw = Recording(), Recording(), Recording()
    plain = HungarianMatcher(w, num_points=50, draw=plain_draw, class_mode="map")
    with_ops = HungarianMatcher(w, num_points=50, draw=ops_draw, class_mode="map", ops=TorchHungarianOps)
    assert plain.pack(targets, "cpu") is None and with_ops.pack(targets, "cpu").counts == [9, 6, 0]
    TorchHungarianOps.calls, TorchHungarianOps.decline = [], False
    want = [plain(logits, boxes, targets), plain(logits, boxes, targets, masks=pred), plain(logits, boxes, targets, masks=pred, costs=("cls", "mask")),
            plain.forward_boxes_only(logits, boxes, targets)]
    packed = with_ops.pack(targets, "cpu")
    got = [with_ops(logits, boxes, targets), with_ops(logits, boxes, targets, masks=pred, packed=packed),
           with_ops(logits, boxes, targets, masks=pred, costs=("cls", "mask"), packed=packed), with_ops.forward_boxes_only(logits, boxes, targets, packed=packed)]
    assert TorchHungarianOps.calls == [(True, True, "map", False), (True, True, "map", True), (True, False, "map", True), (False, True, "map", False)]
    assert all(same_pairs(g, w_) for g, w_ in zip(got, want))
    assert plain_draw.asked == ops_draw.asked == [(1, 50, 2)] * 6                          # one draw per image, the image without targets included
    assert all(len(g[2][0]) == 0 and g[2][0].dtype == torch.int64 for g in got)              # the empty index pair
    # the op declines: the same draws, then the loop
    TorchHungarianOps.calls, TorchHungarianOps.decline = [], True
    try:
        declined = HungarianMatcher(w, num_points=50, draw=declined_draw, class_mode="map", ops=TorchHungarianOps)
        again = [declined(logits, boxes, targets), declined(logits, boxes, targets, masks=pred, packed=packed),
                 declined(logits, boxes, targets, masks=pred, costs=("cls", "mask")), declined.forward_boxes_only(logits, boxes, targets)]
    finally:
        TorchHungarianOps.decline = False
    assert len(TorchHungarianOps.calls) == 4 and declined_draw.asked == plain_draw.asked
    assert all(same_pairs(g, w_) for g, w_ in zip(again, want))

    class NoMaskCosts:                                     # mask costs need a mask_match_costs op beside hungarian_costs: the loop runs
        pack_match_targets = TorchHungarianOps.pack_match_targets
        asked = 0

        @classmethod
        def hungarian_costs(cls, *a, **k):
            cls.asked += 1
            return TorchHungarianOps.hungarian_costs(*a, **k)
    m = HungarianMatcher(w, num_points=50, draw=Recording(), class_mode="map", ops=NoMaskCosts)
    assert same_pairs(m(logits, boxes, targets, masks=pred), want[1]) and NoMaskCosts.asked == 0
    assert same_pairs(m(logits, boxes, targets), want[0]) and NoMaskCosts.asked == 1


def test_assign_host_is_assign():
    C = torch.randn(7, 4, generator=torch.Generator().manual_seed(3))
    a, b = assign(C), assign_host(C.numpy())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[0].dtype == b[1].dtype == torch.int64
    e = assign_host(np.zeros((7, 0), dtype=np.float32))
    assert e[0].numel() == 0 and e[1].numel() == 0 and e[0].dtype == torch.int64


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "packs-itself"])
def test_the_reference_fixtures_through_the_ops_plumbing(packed):
    TorchHungarianOps.calls, TorchHungarianOps.decline = [], False
    for name, (got, want) in Golden().run(TorchHungarianOps, Replay, packed).items():
        assert same_pairs(got, want), name
    assert len(TorchHungarianOps.calls) == 5


def test_nan_costs_reach_scipy_as_today():
    logits, boxes, targets, pred = hungarian_case(1, 4, 3, 8, False, 0)
    bad = [dict(targets[0], positive_map=targets[0]["positive_map"].clone())]
    bad[0]["positive_map"][1] = False
    for ops in (None, TorchHungarianOps):
        with pytest.raises(ValueError, match="invalid numeric"):
            HungarianMatcher(W_BOX, stuff_takes_mean=False, class_mode="map", ops=ops)(logits, boxes, bad)


# ------------------------------------------------------------------------------------------------ the yardsticks of the GPU tests
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", SMALL, ids=IDS)
@pytest.mark.parametrize("stuff", [True, False], ids=["stuff-mean", "own-boxes"])
def test_the_small_cases_have_a_separated_optimum(shape, seed, stuff):
    """the CPU precondition of the GPU test's equality with the torch path: class + box costs with the weights (2, 5, 2)"""
    logits, boxes, targets, _ = hungarian_case(*shape, seed)
    for b, t in enumerate(targets):
        if len(t["boxes"]) == 0:
            continue
        c64 = reference_cost(logits[b], boxes[b], t, W_BOX, torch.float64, stuff_takes_mean=stuff)
        c32 = reference_cost(logits[b], boxes[b], t, W_BOX, torch.float32, stuff_takes_mean=stuff)
        gap, room = assignment_gap(c64), slack(c64, bound_of(c32, c64))
        assert gap > room, (b, gap, room)
        # and the torch path itself sits inside the optimality band
        assert total_cost(c64, assign(c32)) - optimum(c64)[0] <= room


# ------------------------------------------------------------------------------------------------ the backends
def test_backend_hungarian_is_opt_in():
    from hipie_amd.training import net
    from hipie_amd.training.step import TrainStep      # noqa: F401
    assert issubclass(net.HipBackendHungarian, net.HipBackendMatching)
    for be in (net.HipBackend, net.HipBackendLosses, net.HipBackendCriteria, net.HipBackendMatching, net.HipBackendAll):
        assert not hasattr(be, "hungarian_costs") and not hasattr(be, "pack_match_targets")
    assert not issubclass(net.HipBackendAll, net.HipBackendHungarian)
    assert HungarianMatcher().ops is None and HungarianMatcher().pack([], "cpu") is None
    logits, boxes, targets, _ = hungarian_case(1, 4, 3, 8, False, 0)
    packed = net.HipBackendHungarian.pack_match_targets(targets, "cpu")
    assert packed.t_off.tolist() == [0]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendHungarian.hungarian_costs(logits, boxes, packed, W_BOX)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        HungarianMatcher(W_BOX, class_mode="map", ops=net.HipBackendHungarian)(logits, boxes, targets)
