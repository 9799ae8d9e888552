"""CPU: the C entries of csrc/pair_loss.hip refuse on the host without a launch, the criteria's plumbing of the `pair_box_loss` /
`positive_onehot` ops (checked with the float64 plain-torch stand-in of _pair_loss_cases.py against ops=None), the place of
net.HipBackendPairLosses among the backends and the limits outside which the wrappers answer None."""
import ctypes

import pytest
import torch

from _pair_loss_cases import PAD, TorchPairLossOps, both_criteria, criterion_of, explicit_case, pair_case, to_dtype
from hipie_amd import _lib
from hipie_amd.training.criterion import DetCriterion, _positive_onehot


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


P_ = ctypes.c_void_p(256)


def _lists(ns, ptr=256):
    B = len(ns)
    q, t, n = (ctypes.c_void_p * B)(), (ctypes.c_void_p * B)(), (ctypes.c_int64 * B)(*ns)
    for b, k in enumerate(ns):
        if k and ptr:
            q[b] = t[b] = ptr
    return q, t, n


def _forward(lib, ns=(3, 0, 2), Q=10, Tmax=4, mode=0, count=2.0, ws_bytes=1 << 12, lists=None, B=None, strides=(0, 0), **ptrs):
    """hipie_pair_box_loss_forward with made-up pointers: only calls that are refused or return early"""
    v = {k: P_ for k in ("boxes", "tgt_boxes", "is_thing", "out", "pair_grad", "status", "ws")}
    v["iou"] = None
    v.update(ptrs)
    q, t, n = lists or _lists(ns)
    B = len(ns) if B is None else B
    return lib.hipie_pair_box_loss_forward(v["boxes"], strides[0] or Q * 4, strides[1] or 4, v["iou"], Q, 1, q, t, n, v["tgt_boxes"], v["is_thing"], v["out"],
                                           v["pair_grad"], v["status"], v["ws"], ws_bytes, B, Q, Tmax, mode, count, None)


# ------------------------------------------------------------------------------------------------ the ABI, refusals without a launch
def test_abi_surface():
    p, i, l, d = _lib.c_p, _lib.c_i, _lib.c_l, _lib.c_d
    assert _lib.SIGNATURES["hipie_pair_box_loss_forward"] == [p, l, l, p, l, l] + [p] * 9 + [l, i, i, i, i, d, p]
    assert _lib.SIGNATURES["hipie_pair_box_loss_backward"] == [p] * 9 + [i, i, p]
    assert _lib.SIGNATURES["hipie_positive_onehot"] == [p] * 5 + [i, i, i, i, p]
    assert _lib.SIGNATURES["hipie_pair_box_loss_ws_bytes"] == [l] and _lib.RESTYPES["hipie_pair_box_loss_ws_bytes"] is l
    assert _lib.load().hipie_version() == 13                                                # new entries, the ABI number stays


def test_the_workspace_query_is_monotone_and_never_zero():
    ws = _lib.load().hipie_pair_box_loss_ws_bytes
    sizes = [ws(k) for k in range(-1, 2000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    chunk = next(k for k in range(1, 1 << 14) if ws(k + 1) > ws(k))
    assert chunk == 256 and ws(65536) >= 256 * 36


def test_forward_refusals():
    lib = _lib.load()
    for kw, msg in (({"mode": 2}, b"mode=2"), ({"mode": -1}, b"mode=-1"), ({"count": 0.0}, b"count"), ({"count": float("nan")}, b"count"),
                    ({"count": float("inf")}, b"count"), ({"mode": 1, "iou": P_}, b"mode 1 has no box-IoU"), ({"Q": -1}, b"negative"),
                    ({"Tmax": -1}, b"negative"), ({"B": -1}, b"negative"), ({"ns": (1,) * 65}, b"B=65"), ({"ns": (3, -2, 2)}, b"image 1 has -2 pairs"),
                    ({"ns": (65536, 1)}, b"more than 65536 pairs"), ({"Q": 0}, b"Q=0"), ({"Tmax": 0}, b"Tmax=0"),
                    ({"lists": (None,) + _lists((3, 0, 2))[1:]}, b"null pair list"), ({"lists": _lists((3, 0, 2), ptr=0)}, b"image 0: null pair list"),
                    ({"strides": (40, 3)}, b"box strides"), ({"strides": (39, 4)}, b"box strides"),
                    ({"ws_bytes": 47}, b"workspace of 47 bytes"), ({"ws": ctypes.c_void_p(260)}, b"8-byte aligned"),
                    ({"out": ctypes.c_void_p(260)}, b"8-byte aligned")):
        assert _forward(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    for name in ("boxes", "tgt_boxes", "out", "pair_grad", "status", "ws"):
        assert _forward(lib, **{name: None}) == -22 and b"null pointer" in lib.hipie_last_error(), name
    q, t, n = _lists((3, 0, 2))
    assert lib.hipie_pair_box_loss_forward(P_, 40, 4, P_, 10, 0, q, t, n, P_, P_, P_, P_, P_, P_, 1 << 12, 3, 10, 4, 0, 2.0, None) == -22
    assert b"iou strides" in lib.hipie_last_error()


def test_backward_and_onehot_refusals():
    lib = _lib.load()
    q, t, n = _lists((3, 0, 2))
    bwd = lambda B=3, Q=10, q=q, n=n, out=P_, pg=P_, g=P_, gi=P_, d=P_, di=P_: lib.hipie_pair_box_loss_backward(q, n, out, pg, g, g, gi, d, di, B, Q, None)  # noqa: E731
    for kw, msg in (({"B": 65, "n": _lists((1,) * 65)[2], "q": _lists((1,) * 65)[0]}, b"B=65"), ({"Q": -1}, b"negative"), ({"q": None}, b"null pair list"),
                    ({"n": None}, b"null pair list"), ({"Q": 0}, b"Q=0"), ({"d": None}, b"null pointer"), ({"out": None}, b"null pointer"),
                    ({"pg": None}, b"null pointer"), ({"g": None}, b"null pointer"), ({"gi": None}, b"null pointer"),
                    ({"out": ctypes.c_void_p(260)}, b"8-byte aligned"), ({"n": _lists((3, -1, 2))[2]}, b"image 1 has -1 pairs")):
        assert bwd(**kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    hot = lambda B=3, Q=10, T=4, L=5, q=q, t=t, n=n, pm=P_, oh=P_: lib.hipie_positive_onehot(q, t, n, pm, oh, B, Q, T, L, None)  # noqa: E731
    for kw, msg in (({"L": -1}, b"negative"), ({"T": -1}, b"negative"), ({"T": 0}, b"Tmax=0"), ({"Q": 0}, b"Q=0"), ({"t": None}, b"null pair list"),
                    ({"pm": None}, b"null pointer"), ({"oh": None}, b"null pointer"), ({"n": _lists((65536, 0, 1))[2]}, b"more than 65536 pairs")):
        assert hot(**kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())


def test_empty_calls_return_without_a_launch():
    lib = _lib.load()
    none = {k: None for k in ("boxes", "tgt_boxes", "is_thing", "out", "pair_grad", "status", "ws")}
    for ns in ((), (0,), (0, 0, 0)):
        lists = _lists(ns)
        assert _forward(lib, ns=ns, ws_bytes=0, **none) == 0
        assert _forward(lib, ns=ns, ws_bytes=0, lists=(None, None, lists[2]) if not ns else lists, Q=0, Tmax=0, **none) == 0
    assert lib.hipie_pair_box_loss_backward(None, None, None, None, None, None, None, None, None, 0, 10, None) == 0
    assert lib.hipie_pair_box_loss_backward(*_lists((0, 0))[::2], None, None, None, None, None, None, None, 2, 0, None) == 0
    assert lib.hipie_positive_onehot(None, None, None, None, None, 0, 10, 4, 5, None) == 0
    assert lib.hipie_positive_onehot(*_lists((0, 0)), None, None, 2, 10, 4, 0, None) == 0


def test_the_binding_refuses_before_the_device_is_asked():
    from hipie_amd import ops
    case = pair_case((3, 0, 2))
    from hipie_amd.training import functions
    packed = functions.pack_match_targets(case.targets, "cpu", False)
    boxes, iou = case.big[:, PAD:], case.iou_big[:, PAD:, 0]
    ok = (boxes, iou, case.pairs, packed.tgt_boxes, packed.is_thing, 2.0, 0)
    swap = lambda i, x: ok[:i] + (x,) + ok[i + 1:]          # noqa: E731
    for args, msg in ((swap(0, boxes.double()), "boxes must be torch.float32"), (swap(0, boxes[..., :3]), r"boxes must be \(3, 5, 4\)"),
                      (swap(0, boxes.transpose(1, 2).contiguous().transpose(1, 2)), "last dimension has to be dense"),
                      (swap(1, iou.double()), "iou must be torch.float32"), (swap(1, iou[:, :4]), r"iou must be \(3, 5\)"),
                      (swap(3, packed.tgt_boxes.double()), "tgt_boxes must be torch.float32"), (swap(4, packed.is_thing.bool()), "is_thing must be torch.uint8"),
                      (swap(2, case.pairs[:2]), "2 pair lists for B=3"), (swap(2, [(q.int(), t) for q, t in case.pairs]), "contiguous 1-d torch.int64"),
                      (swap(2, [(q, t[:1]) for q, t in case.pairs]), "query and 1 target indices")):
        with pytest.raises(RuntimeError, match=msg):
            ops.pair_box_loss_forward(*args)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.pair_box_loss_forward(*ok)
    with pytest.raises(RuntimeError, match="pos_map must be torch.uint8"):
        ops.positive_onehot(case.pairs, packed.pos_map.bool(), 5)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.positive_onehot(case.pairs, packed.pos_map, 5)
    assert [bit for bit, _ in ops.PAIR_STATUS] == [1, 2] and (ops.PAIR_MAX_B, ops.PAIR_MAX_K) == (64, 65536)


# ------------------------------------------------------------------------------------------------ the limits: None, the torch path runs
def test_outside_the_limits_the_wrappers_answer_none():
    from hipie_amd.training import functions
    case = pair_case((3, 0, 2))
    packed = functions.pack_match_targets(case.targets, "cpu", False)
    boxes, iou = case.big[:, PAD:], case.iou_big[:, PAD:]
    f = functions.pair_box_loss
    assert f(boxes.double(), None, case.pairs, packed, 2.0, 0) is None                                   # dtype
    assert f(boxes.half(), None, case.pairs, packed, 2.0, 0) is None
    assert f(boxes, iou.double(), case.pairs, packed, 2.0, 0) is None
    assert f(boxes, iou, case.pairs, packed, 2.0, 1) is None                                             # no box-IoU loss in mode 1
    assert f(boxes, None, [(q[:0], t[:0]) for q, t in case.pairs], packed, 2.0, 0) is None              # K = 0: the criterion's own expression
    assert f(boxes[:2], None, case.pairs[:2], packed, 2.0, 0) is None                                    # packed for another B
    many = [(torch.zeros(1, dtype=torch.long),) * 2] * 65
    assert f(torch.zeros(65, 4, 4), None, many, functions.pack_match_targets(case.targets[:1] * 65, "cpu", False), 2.0, 0) is None          # B
    big = [(torch.zeros(65537, dtype=torch.long),) * 2]
    assert f(boxes[:1], None, big, functions.pack_match_targets(case.targets[:1], "cpu", False), 2.0, 0) is None                            # K
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        f(boxes, iou, case.pairs, packed, 2.0, 0)
    h = functions.positive_onehot
    logits = torch.zeros(3, 5, 5)
    assert h(logits.double(), case.pairs, packed) is None
    assert h(torch.zeros(3, 5, 6), case.pairs, packed) is None                                           # another L
    assert h(logits, case.pairs, functions.pack_match_targets([{k: v for k, v in t.items() if k != "positive_map"} for t in case.targets], "cpu", False)) is None
    assert h(torch.zeros(65, 9, 5), many, functions.pack_match_targets(case.targets[:1] * 65, "cpu", False)) is None
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        h(logits, case.pairs, packed)


def test_the_dtype_rule_of_the_onehot_path():
    """bool and uint8 maps go through the op; any other dtype (a map that may hold values other than 0 / 1) runs today's loop"""
    case = pair_case((3, 0, 2))
    asked = []

    class Ops(TorchPairLossOps):
        @classmethod
        def positive_onehot(cls, logits, pairs, packed):
            asked.append(1)
            return super().positive_onehot(logits, pairs, packed)
    logits = torch.randn(3, 5, 5)
    for dtype, through in ((torch.bool, True), (torch.uint8, True), (torch.float32, False), (torch.int64, False)):
        targets = [dict(t, positive_map=t["positive_map"].to(dtype) if through else t["positive_map"].to(dtype) * 3) for t in case.targets]
        crit = DetCriterion(None, ["labelsVL"], ops=Ops)
        del asked[:]
        got = crit._onehot(logits, targets, case.pairs)
        assert bool(asked) is through, dtype
        assert torch.equal(got, _positive_onehot(logits, targets, case.pairs)), dtype
    assert torch.equal(DetCriterion(None, ["labelsVL"])._onehot(logits, case.targets, case.pairs), _positive_onehot(logits, case.targets, case.pairs))


# ------------------------------------------------------------------------------------------------ the stand-in through both criteria
def _same(a, b, tag):
    assert sorted(a) == sorted(b), tag
    for k in a:
        assert torch.allclose(a[k], b[k], rtol=1e-11, atol=1e-13), (tag, k, float(a[k].detach()), float(b[k].detach()))


@pytest.mark.parametrize("mode,ota", [(0, False), (0, True), (1, False)], ids=["det", "det-ota", "maskdino"])
@pytest.mark.parametrize("panoptic", [False, True])
def test_loss_boxes_through_the_stand_in_is_todays(mode, ota, panoptic):
    """the strided-slice input, pred_boxious, an image with no pair (MaskCriterion has no ota switch)"""
    for counts, things in (((5, 0, 9), "mixed"), ((4,), "all"), ((6, 2), "none")):
        case = pair_case(counts, 1, things)
        runs = []
        for ops in (None, TorchPairLossOps):
            big, iou_big = case.big.double().requires_grad_(), case.iou_big.double().requires_grad_()
            out = {"pred_boxes": big[:, PAD:], "pred_boxious": iou_big[:, PAD:]}
            crit = criterion_of(mode, ops, ota, panoptic)
            res = crit.loss_boxes(out, to_dtype(case.targets, torch.float64), case.pairs, case.count)
            sum(g * v for g, v in zip(case.g.double(), res.values())).backward()
            assert len(crit.pending) == (ops is not None) and (ops is None or crit.pending[0][0].tolist() == [0])
            runs.append((res, {"d_boxes": big.grad, "d_iou": torch.zeros(()) if iou_big.grad is None else iou_big.grad}))
            crit.check()
            assert crit.pending == []
        if things == "none" and panoptic and mode == 0:
            # today's "no thing among the pairs" branch leaves the key out; the op has no such branch (it would be a host wait) and
            # answers the exact zero the entry is worth
            assert "loss_boxiou" not in runs[0][0] and float(runs[1][0]["loss_boxiou"].detach()) == 0.0
            assert all(float(v.detach()) == 0.0 for v in runs[1][0].values()) and all(not bool(g.any()) for g in runs[1][1].values())
            runs[0][0]["loss_boxiou"] = runs[1][0]["loss_boxiou"]
            runs[0][1]["d_iou"] = torch.zeros_like(runs[1][1]["d_iou"])                 # today's branch does not touch the IoU logits
        _same(runs[0][0], runs[1][0], (counts, things))
        _same(runs[0][1], runs[1][1], (counts, things))
        assert ("loss_boxiou" in runs[1][0]) is (mode == 0)


def test_the_blockwise_reference_is_the_criterions():
    """the reference of the GPU test at 16 385 pairs takes the GIoU diagonal block by block; here against the criterion's own (K, K) form"""
    from _pair_loss_cases import mask_loss_boxes_blockwise
    case = pair_case((700, 0, 900))
    for panoptic in (False, True):
        boxes = case.big[:, PAD:].double()
        want = criterion_of(1, None, panoptic=panoptic).loss_boxes({"pred_boxes": boxes}, to_dtype(case.targets, torch.float64), case.pairs, 3.0)
        got = mask_loss_boxes_blockwise({"pred_boxes": boxes}, to_dtype(case.targets, torch.float64), case.pairs, 3.0, panoptic)
        assert sorted(got) == sorted(want) and all(torch.allclose(got[k], want[k], rtol=1e-13, atol=0) for k in want)


def test_no_pair_makes_no_call_of_the_op():
    case = pair_case((0, 0))

    class Ops(TorchPairLossOps):
        @classmethod
        def pair_box_loss(cls, *a, **k):
            raise AssertionError("asked without a pair")
    big = case.big.clone().requires_grad_()
    res = criterion_of(0, Ops).loss_boxes({"pred_boxes": big[:, PAD:]}, case.targets, case.pairs, 3.0)
    assert float(res["loss_bbox"]) == 0.0 and float(res["loss_giou"]) == 0.0 and res["loss_bbox"].requires_grad


def test_a_degenerate_box_is_deferred_to_check():
    case = explicit_case([[0.5, 0.5, -0.2, 0.2], [0.3, 0.3, 0.2, 0.2]], [[0.5, 0.5, 0.3, 0.3], [0.3, 0.3, 0.1, 0.1]])
    crit = criterion_of(1, TorchPairLossOps, panoptic=False)
    res = crit.loss_boxes({"pred_boxes": case.big[:, PAD:]}, case.targets, case.pairs, 2.0)
    assert all(bool(torch.isfinite(v)) for v in res.values()) and crit.pending[0][0].tolist() == [1]
    with pytest.raises(ValueError, match=r"MaskCriterion\.loss_boxes call 1.*boxes with x1 < x0 or y1 < y0"):
        crit.check()
    assert crit.pending == []
    with pytest.raises(ValueError, match="boxes with x1 < x0 or y1 < y0"):                              # today's path raises at once
        criterion_of(1, None, panoptic=False).loss_boxes({"pred_boxes": case.big[:, PAD:]}, case.targets, case.pairs, 2.0)


def _both_criteria(ops, given=None):
    losses, grads, criteria, _ = both_criteria(ops, omit_ops=given == "omitted")
    for c in criteria:
        c.check()
        assert c._packs == [] and c.pending == []
    return losses, grads


def test_both_criteria_through_the_stand_in_are_todays():
    want, want_g = _both_criteria(None)
    got, got_g = _both_criteria(TorchPairLossOps)
    boxes = [k for k in want if "bbox" in k or "giou" in k or "boxiou" in k]
    assert len(boxes) >= 2 * (3 + 3 + 1) + 2 and any("boxiou" in k for k in boxes) and any(k.endswith("_enc") for k in boxes)
    _same(want, got, "losses")
    _same(want_g, got_g, "gradients")
    assert all(torch.equal(want[k], got[k]) for k in want if "loss_ce" in k)                            # exact 0 / 1 entries: not a bit moves


def test_ops_none_is_the_criterion_built_without_the_argument():
    a, ag = _both_criteria(None)
    b, bg = _both_criteria(None, given="omitted")
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(ag[k], bg[k]) for k in ag)


# ------------------------------------------------------------------------------------------------ the backend
def test_backend_pair_losses_is_opt_in():
    from hipie_amd.training import net
    from hipie_amd.training.step import TrainStep          # noqa: F401
    assert issubclass(net.HipBackendPairLosses, net.HipBackendAssign)
    assert set(vars(net.HipBackendPairLosses)) - {"__doc__", "__module__"} == {"pair_box_loss", "positive_onehot", "pack_pair_targets"}          # nothing else
    packed = net.HipBackendPairLosses.pack_pair_targets(pair_case((3, 0, 2)).targets, "cpu")
    assert packed.n_tgt is None and packed.t_off is None and packed.tgt_masks is None and packed.counts == [7, 7, 7]          # nothing copied from the host
    for be in (net.HipBackend, net.HipBackendLosses, net.HipBackendCriteria, net.HipBackendMatching, net.HipBackendHungarian, net.HipBackendAssign,
               net.HipBackendAll, net.HipBackendNorms, net.HipBackendMlp, net.HipBackendWindows, net.HipBackendDeformable, net.HipBackendPackedWindows):
        assert not any(hasattr(be, n) for n in ("pair_box_loss", "positive_onehot", "pack_pair_targets")), be
    assert not issubclass(net.HipBackendAll, net.HipBackendPairLosses)
    case = pair_case((3, 0, 2))
    packed = net.HipBackendPairLosses.pack_match_targets(case.targets, "cpu", False)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendPairLosses.pair_box_loss(case.big[:, PAD:], None, case.pairs, packed, 2.0, 0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendPairLosses.positive_onehot(torch.zeros(3, 5, 5), case.pairs, packed)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        criterion_of(0, net.HipBackendPairLosses).loss_boxes({"pred_boxes": case.big[:, PAD:]}, case.targets, case.pairs, 2.0)
