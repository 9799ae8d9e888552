"""GPU: hipie_pair_box_loss_forward / _backward and hipie_positive_onehot (csrc/pair_loss.hip) through functions.pair_box_loss /
positive_onehot, both criteria with ops=net.HipBackendPairLosses, and the opt-in wiring of the training step.

Reference, metric and bound: tests/_pair_loss_cases.py -- `loss_boxes` of the criteria with ops=None on the CPU in float64 (reference) and
float32 (e_lib); max|got - ref64| / max|ref64| per output tensor against max(1e-6, 4 x e_lib).  Every case prints its figures (lines starting
with LOSS) before it asserts."""
import pytest
import torch

from _hungarian_cases import W_BOX, hungarian_case
from _ota_cases import same_pairs
from _pair_loss_cases import (FINISHER_ROWS, NAMES, PAD, ReplayMatcher, TorchPairLossOps, both_criteria, check, criterion_of, err, explicit_case, host_waits,
                              pair_case, reference, yardsticks)
from hipie_amd.training.criterion import DetCriterion, MaskCriterion, _positive_onehot
from hipie_amd.training.dn import dn_match_indices
from hipie_amd.training.matcher import HungarianMatcher


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [pytest.param(0, True, id="det-iou"), pytest.param(0, False, id="det"), pytest.param(1, False, id="maskdino")]


def _chunk():
    """pairs per workgroup, read off the workspace query: it holds one partial row per chunk of pairs"""
    from hipie_amd import _lib
    ws = _lib.load().hipie_pair_box_loss_ws_bytes
    return next(k for k in range(1, 1 << 14) if ws(k + 1) > ws(k))


def _on(dev, targets):
    return [{k: v.to(dev) for k, v in t.items()} for t in targets]


def _run(case, mode, with_iou, use_thing=True, ota=False):
    """functions.pair_box_loss on the slices [:, PAD:] and the backward of sum_i g[i] loss_i -> ((the five tensors of NAMES), status)"""
    from hipie_amd.training import functions
    big, iou_big = case.big.to(DEV).requires_grad_(), case.iou_big.to(DEV).requires_grad_()
    packed = functions.pack_match_targets(_on(DEV, case.targets), DEV, False)
    pairs = [(q.to(DEV), t.to(DEV)) for q, t in case.pairs]
    iou = iou_big[:, PAD:] if with_iou and mode == 0 else None
    lb, lg, li, status = functions.pair_box_loss(big[:, PAD:], iou, pairs, packed, case.K if ota else case.count, mode, use_thing)
    assert (li is not None) is (iou is not None) and status.shape == (1,) and status.dtype == torch.int32
    assert all(t.dtype == torch.float32 and t.dim() == 0 for t in (lb, lg))
    g = case.g.to(DEV)
    (g[0] * lb + g[1] * lg + (g[2] * li if li is not None else 0.0)).backward()
    assert not bool(big.grad[:, :PAD].any())                                           # outside the slice nothing arrives
    d_iou = torch.zeros_like(iou_big) if iou_big.grad is None else iou_big.grad
    assert not bool(d_iou[:, :PAD].any())
    return (lb.detach(), lg.detach(), torch.zeros((), device=DEV) if li is None else li.detach(), big.grad[:, PAD:], d_iou[:, PAD:]), status


# ------------------------------------------------------------------------------------------------ 1. conformance
@pytest.mark.parametrize("mode,with_iou", MODES)
def test_pair_box_loss_against_float64(mode, with_iou):
    chunk = _chunk()
    assert 64 <= chunk <= 1 << 12
    sizes = [(1,), (63,), (64,), (65,), (chunk + 1,), (chunk + 2,), (FINISHER_ROWS * chunk + 1,), (FINISHER_ROWS * chunk + 2,), (5, 0, 9), (chunk, 0, chunk + 3)]
    for counts in sizes:
        ref, lib = yardsticks(counts, mode, with_iou)
        got, status = _run(pair_case(counts), mode, with_iou)
        check("pairs=%s mode=%d iou=%d" % (counts, mode, with_iou), NAMES, got, ref, lib)
        assert status.tolist() == [0], counts


@pytest.mark.parametrize("mode", [0, 1])
def test_ota_count_and_unweighted_pairs(mode):
    """count = K (the `ota` normaliser of DetCriterion) and panoptic_box_loss / panoptic_on off"""
    for ota, panoptic in ((True, True), (False, False), (True, False)):
        if mode == 1 and ota:
            continue                                                                   # MaskCriterion has no ota switch
        counts = (70, 3)
        ref, lib = yardsticks(counts, mode, mode == 0, ota=ota, panoptic=panoptic)
        got, _ = _run(pair_case(counts), mode, mode == 0, use_thing=panoptic, ota=ota)
        check("pairs=%s mode=%d ota=%d panoptic=%d" % (counts, mode, ota, panoptic), NAMES, got, ref, lib)


# ------------------------------------------------------------------------------------------------ 2. named cases
E = 2.0 ** -13                                  # about 1.2e-4: exactly representable, as are 0.25, 0.5, 0.75
NAMED = {
    "disjoint": ([[0.2, 0.2, 0.1, 0.1], [0.8, 0.2, 0.1, 0.3]], [[0.7, 0.7, 0.2, 0.2], [0.2, 0.8, 0.3, 0.1]]),
    "nested": ([[0.5, 0.5, 0.2, 0.2], [0.5, 0.5, 0.6, 0.6]], [[0.5, 0.5, 0.6, 0.6], [0.5, 0.5, 0.2, 0.2]]),
    "src == tgt": ([[0.5, 0.5, 0.25, 0.25], [0.3, 0.7, 0.1, 0.2]], [[0.5, 0.5, 0.25, 0.25], [0.3, 0.7, 0.1, 0.2]]),
    "shared edges": ([[0.25, 0.5, 0.5, 0.5], [0.5, 0.25, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5]], [[0.75, 0.5, 0.5, 0.5], [0.5, 0.75, 0.5, 0.5], [0.5, 0.5, 0.5, 0.25]]),
    "sizes 1e-4 and 0.999": ([[0.5, 0.5, 1e-4, 1e-4], [0.5, 0.5, 0.999, 0.999], [0.25, 0.25, E, E], [0.5, 0.5, 0.999, 1e-4]],
                             [[0.5, 0.5, 0.999, 0.999], [0.5, 0.5, 1e-4, 1e-4], [0.25 + E / 2, 0.25, E, E], [0.5, 0.5, 1e-4, 0.999]]),
}


@pytest.mark.parametrize("name", sorted(NAMED))
@pytest.mark.parametrize("mode", [0, 1])
def test_named_boxes(name, mode):
    case = explicit_case(*NAMED[name])
    ref, lib = reference(case, mode, True, torch.float64), reference(case, mode, True, torch.float32)
    got, status = _run(case, mode, True)
    check("%s mode=%d" % (name, mode), NAMES, got, ref, lib)
    assert status.tolist() == [0]
    if name == "src == tgt":                                                           # the tie convention: half the gradient to each side
        assert float(got[0]) == 0.0 and bool(torch.isfinite(got[3]).all()) and abs(float(got[1]) - float(ref[1])) <= 1e-7
        assert float((got[3].double().cpu() - ref[3]).abs().max()) <= 1e-7                 # in absolute terms: in mode 1 the reference is 0


def test_a_duplicated_query_receives_the_sum():
    case = explicit_case([[0.4, 0.4, 0.3, 0.2], [0.6, 0.5, 0.2, 0.4]], [[0.45, 0.4, 0.25, 0.3], [0.5, 0.55, 0.3, 0.3]], duplicate=True)
    single = explicit_case([[0.4, 0.4, 0.3, 0.2], [0.6, 0.5, 0.2, 0.4]], [[0.45, 0.4, 0.25, 0.3], [0.5, 0.55, 0.3, 0.3]])
    for mode in (0, 1):
        ref, lib = reference(case, mode, True, torch.float64), reference(case, mode, True, torch.float32)
        got, _ = _run(case, mode, True)
        check("duplicated (image, query) mode=%d" % mode, NAMES, got, ref, lib)
        assert err(got[3], reference(single, mode, True, torch.float64)[3]) > 0.1       # it is not the gradient of one of the two


@pytest.mark.parametrize("mode", [0, 1])
def test_no_thing_among_the_pairs_is_exactly_zero(mode):
    """what DetCriterion's `thing.sum() == 0` branch returns, without the branch; MaskCriterion's filter leaves nothing"""
    got, status = _run(pair_case((70, 0, 300), 0, "none"), mode, True)
    for name, t in zip(NAMES, got):
        assert not bool(t.any()) and bool(torch.isfinite(t).all()), name
    assert status.tolist() == [0]


@pytest.mark.parametrize("mode,with_iou", MODES)
def test_all_things(mode, with_iou):
    counts = (70, 0, 300)
    got, _ = _run(pair_case(counts, 0, "all"), mode, with_iou)
    check("all things mode=%d" % mode, NAMES, got, *yardsticks(counts, mode, with_iou, 0, "all"))


def test_a_degenerate_box_sets_the_status_bit_and_the_deferred_check_raises():
    from hipie_amd.training import net
    src, tgt = [[0.5, 0.5, -0.2, 0.2], [0.3, 0.3, 0.2, 0.2]], [[0.5, 0.5, 0.3, 0.3], [0.3, 0.3, 0.1, 0.1]]
    case = explicit_case(src, tgt)
    got, status = _run(case, 1, False)
    assert status.tolist() == [1] and all(bool(torch.isfinite(t).all()) for t in got)
    big = case.big.double().requires_grad_()
    lb, lg, _, st = TorchPairLossOps.pair_box_loss(big[:, PAD:], None, case.pairs, TorchPairLossOps.pack_match_targets(case.targets, "cpu", False), case.count, 1)
    (case.g[0].double() * lb + case.g[1].double() * lg).backward()
    assert st.tolist() == [1]
    for name, g, r in zip(("loss_bbox", "loss_giou", "d_boxes"), (got[0], got[1], got[3]), (lb, lg, big.grad[:, PAD:])):
        print("LOSS degenerate box %-10s err %.3e" % (name, err(g, r)))
        assert err(g, r) <= 1e-6, name
    assert _run(explicit_case(src, tgt, thing=[False, True]), 1, False)[1].tolist() == [0]          # the filter leaves the degenerate pair out
    assert _run(case, 0, True)[1].tolist() == [0]                                                    # mode 0 has no such check (nor has the torch path)
    crit = criterion_of(1, net.HipBackendPairLosses, panoptic=False)
    res = crit.loss_boxes({"pred_boxes": case.big[:, PAD:].to(DEV)}, _on(DEV, case.targets), [(q.to(DEV), t.to(DEV)) for q, t in case.pairs], 2.0)
    assert all(bool(torch.isfinite(v)) for v in res.values()) and len(crit.pending) == 1
    with pytest.raises(ValueError, match="boxes with x1 < x0 or y1 < y0"):
        crit.check()
    assert crit.pending == []


def test_an_index_out_of_range_is_left_out_and_flagged():
    from hipie_amd.training import functions
    case = pair_case((5, 0, 9))
    packed = functions.pack_match_targets(_on(DEV, case.targets), DEV, False)
    big = case.big.to(DEV).requires_grad_()
    good = [(q.to(DEV), t.to(DEV)) for q, t in case.pairs]
    Q, T = big.shape[1] - PAD, packed.tgt_boxes.shape[1]
    bad = [(torch.cat((good[0][0], torch.tensor([Q, -1, 0], device=DEV))), torch.cat((good[0][1], torch.tensor([0, 0, T], device=DEV))))] + good[1:]
    want = functions.pair_box_loss(big[:, PAD:], None, good, packed, 4.0, 1)
    got = functions.pair_box_loss(big[:, PAD:], None, bad, packed, 4.0, 1)
    assert got[3].tolist() == [2] and want[3].tolist() == [0]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    (got[0] + got[1]).backward()
    d_bad, big.grad = big.grad.clone(), None
    (want[0] + want[1]).backward()
    assert torch.equal(d_bad, big.grad)


# ------------------------------------------------------------------------------------------------ 3. the positive one-hot
@pytest.mark.parametrize("L", [1, 30, 257])
def test_positive_onehot_is_the_loop(L):
    from hipie_amd.training import functions, net
    logits, boxes, targets, _ = hungarian_case(2, 40, 5, L, True, 0)
    logits, boxes, targets = logits.to(DEV), boxes.to(DEV), _on(DEV, targets)
    packed = functions.pack_match_targets(targets, DEV, False)
    matcher = HungarianMatcher(W_BOX, class_mode="map", ops=net.HipBackendPairLosses, defer_status=True)
    kinds = {"hungarian": matcher(logits, boxes, targets), "ota": matcher.forward_ota(logits, boxes, targets)[0],
             "de-noising": dn_match_indices(targets, {"dn_num": 3, "single_padding": 10}, DEV)}
    matcher.check()
    for kind, pairs in kinds.items():
        assert all(q.is_cuda and q.dtype == torch.int64 for q, _ in pairs) and sum(len(q) for q, _ in pairs) >= 5, kind
        got = functions.positive_onehot(logits, pairs, packed)
        want = _positive_onehot(logits, targets, pairs)
        assert got.dtype == torch.float32 and torch.equal(got, want) and bool(want.any()), (kind, L)
        crit = DetCriterion(None, ["labelsVL"], ops=net.HipBackendPairLosses)
        assert torch.equal(crit._onehot(logits, targets, pairs), want), (kind, L)
    none = [(q[:0], t[:0]) for q, t in kinds["ota"]]
    assert not bool(functions.positive_onehot(logits, none, packed).any())


# ------------------------------------------------------------------------------------------------ 4. determinism, no host wait
@pytest.mark.parametrize("mode,with_iou", MODES)
def test_two_runs_give_identical_bytes(mode, with_iou):
    for counts in ((300, 0, 500), (FINISHER_ROWS * _chunk() + 1,)):
        first, _ = _run(pair_case(counts), mode, with_iou)
        torch.randn(1 << 20, device=DEV).sum()                    # other work in between
        second, _ = _run(pair_case(counts), mode, with_iou)
        assert all(torch.equal(a, b) for a, b in zip(first, second)), counts


@pytest.mark.parametrize("mode", [0, 1])
def test_loss_boxes_and_the_onehot_make_no_host_wait(mode):
    """a loss_boxes call (forward and backward) and a one-hot through the new backend; the same calls through net.HipBackendAssign wait"""
    from hipie_amd.training import net
    case = pair_case((200, 0, 300))
    targets = _on(DEV, case.targets)
    pairs = [(q.to(DEV), t.to(DEV)) for q, t in case.pairs]
    logits = torch.randn(3, case.big.shape[1] - PAD, 5, device=DEV)
    waits = {}
    for be in (net.HipBackendPairLosses, net.HipBackendAssign):
        crit = criterion_of(mode, be)
        big, iou_big = case.big.to(DEV).requires_grad_(), case.iou_big.to(DEV).requires_grad_()
        out = {"pred_boxes": big[:, PAD:], "pred_boxious": iou_big[:, PAD:]}
        up = torch.ones((), device=DEV)

        def call():
            res = crit.loss_boxes(out, targets, pairs, 7.0)          # noqa: B023
            sum(res.values()).backward(up)          # noqa: B023
            return res
        call()                                                                         # loads the kernels, packs the targets of this list
        crit._onehot(logits, targets, pairs)
        waits[be] = (host_waits(call)[0], host_waits(lambda: crit._onehot(logits, targets, pairs))[0])          # noqa: B023
        crit.check()
    print("LOSS host waits of a loss_boxes call / a one-hot (mode %d): %s with the pair kernels, %s without" % (mode, waits[net.HipBackendPairLosses],
                                                                                                              waits[net.HipBackendAssign]))
    assert waits[net.HipBackendPairLosses] == (0, 0)
    assert waits[net.HipBackendAssign][0] >= 1


# ------------------------------------------------------------------------------------------------ 5. both criteria end to end
def _is_box(key):
    return any(s in key for s in ("loss_bbox", "loss_giou", "loss_boxiou"))


def test_both_criteria_end_to_end():
    """B = 2, Q = 30, two auxiliary layers, encoder outputs, de-noising parts.  The box entries and the gradients of every box / box-IoU input
    against ops=None in float64 on the CPU, scoring the pairs the GPU run's matchers chose; the other entries equal to the HipBackendAssign run"""
    from hipie_amd.training import net
    got, got_g, criteria, matcher = both_criteria(net.HipBackendPairLosses, torch.float32, DEV, matcher_ops=net.HipBackendPairLosses)
    recorded = list(matcher.recorded)
    matcher.matcher.check()
    for c in criteria:
        assert len(c.pending) >= 5
        c.check()
    parent, _, _, parent_matcher = both_criteria(net.HipBackendAssign, torch.float32, DEV, matcher_ops=net.HipBackendAssign)
    assert len(recorded) == len(parent_matcher.recorded) >= 5 and all(same_pairs(a, b) for a, b in zip(recorded, parent_matcher.recorded))
    ref, ref_g, _, _ = both_criteria(None, torch.float64, "cpu", matcher=ReplayMatcher(recorded))
    lib, lib_g, _, _ = both_criteria(None, torch.float32, "cpu", matcher=ReplayMatcher(recorded))
    assert sorted(got) == sorted(ref) == sorted(parent)
    boxes = [k for k in sorted(ref) if _is_box(k)]
    assert len(boxes) >= 30 and any("boxiou" in k for k in boxes) and any(k.endswith("_enc") for k in boxes) and any("_dn" in k for k in boxes)
    check("criteria", boxes, [got[k] for k in boxes], [ref[k] for k in boxes], [lib[k] for k in boxes])
    inputs = [p for p in sorted(ref_g) if p.endswith("pred_boxes") or p.endswith("pred_boxious")]
    assert len(inputs) >= 16
    check("criteria", ["d" + p for p in inputs], [got_g[p] for p in inputs], [ref_g[p] for p in inputs], [lib_g[p] for p in inputs])
    differ = {k: (float(got[k]), float(parent[k])) for k in got if not _is_box(k) and not torch.equal(got[k], parent[k])}
    assert not differ, differ
    assert sum(1 for k in got if "loss_ce" in k) >= 10 and sum(1 for k in got if "loss_mask" in k or "loss_dice" in k) >= 8


# ------------------------------------------------------------------------------------------------ 6. the step
def test_train_step_with_the_pair_kernels_matches_the_assign_backend(monkeypatch):
    """one TrainStep forward on the small fixture model with net.HipBackendPairLosses against net.HipBackendAssign (deterministic convolutions, as
    test_gpu_hungarian_assign sets them): identical matcher pairs, the same number of draws, every entry that is not a box entry EQUAL; the box
    entries against today's formula evaluated in float64 on the CPU on the arguments of every loss_boxes call of the parent run -- the new
    entry's error within max(1e-6, 4 x the parent entry's error); and the host waits of loss_dict."""
    from hipie_amd.training import net
    from _train_step_cases import train_step_case as _train_step_case
    seen = []
    for name in ("forward", "forward_boxes_only", "forward_ota"):
        def recorded(self, *a, _f=getattr(HungarianMatcher, name), _n=name, **k):
            out = _f(self, *a, **k)
            seen.append(out[0] if _n == "forward_ota" else out)
            return out
        monkeypatch.setattr(HungarianMatcher, name, recorded)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    today = {DetCriterion: DetCriterion.loss_boxes, MaskCriterion: MaskCriterion.loss_boxes}
    calls = []                                               # the arguments of every loss_boxes call of the run in flight (references: no copy, no wait)
    replay = []                                              # float64 results handed out instead, call by call

    def patched(cls):
        def loss_boxes(self, out, targets, indices, count, _f=cls.loss_boxes):
            if replay:
                return {k: v.to(out["pred_boxes"].device) for k, v in replay.pop(0).items()}
            calls.append((self, {k: out[k].detach() for k in ("pred_boxes", "pred_boxious") if k in out}, targets, indices, count))
            return _f(self, out, targets, indices, count)
        monkeypatch.setattr(cls, "loss_boxes", loss_boxes)
    patched(DetCriterion)
    patched(MaskCriterion)

    def run(step, batch, targets):
        step.draws.calls = 0
        del seen[:], calls[:]
        with torch.enable_grad():
            waits, losses = host_waits(lambda: step.loss_dict(batch, targets))
        assert all(m.pending == [] for m in step.matchers) and step.criterion.pending == [] and step.md_criterion.pending == []
        return {k: v.detach().double().cpu() for k, v in losses.items()}, [[(q.cpu(), t.cpu()) for q, t in out] for out in seen], waits, step.draws.calls

    z, meta, model, step, batch, targets = _train_step_case("cuda", net.HipBackendAssign)
    want, want_pairs, want_waits, want_draws = run(step, batch, targets)
    n_calls = len(calls)
    n_with_pairs = sum(1 for c in calls if sum(len(p[0]) for p in c[3]) > 0)
    assert want_draws == int(z["n_rand"])
    for crit, out, tg, idx, count in calls:                  # today's formula in float64 on the CPU on the recorded arguments
        twin = (DetCriterion(None, ["boxes"], panoptic_box_loss=crit.panoptic_box_loss, ota=crit.ota) if isinstance(crit, DetCriterion)
                else MaskCriterion(1, None, ["boxes"], panoptic_on=crit.panoptic_on))
        tg64 = [{k: (v.double().cpu() if v.is_floating_point() else v.cpu()) for k, v in t.items() if torch.is_tensor(v)} for t in tg]
        replay.append(today[type(twin)](twin, {k: v.double().cpu() for k, v in out.items()}, tg64, [(q.cpu(), t.cpu()) for q, t in idx], count))
    assert len(replay) == n_calls
    ref, _, _, _ = run(step, batch, targets)                 # the same step again, its loss_boxes answering with the float64 values
    assert replay == []
    z, meta, model, step, batch, targets = _train_step_case("cuda", net.HipBackendPairLosses)
    assert step.criterion.ops is net.HipBackendPairLosses and step.md_criterion.ops is net.HipBackendPairLosses
    got, got_pairs, got_waits, got_draws = run(step, batch, targets)
    assert got_draws == want_draws and len(calls) == n_calls >= 10
    assert len(got_pairs) == len(want_pairs) and all(same_pairs(g, w) for g, w in zip(got_pairs, want_pairs))
    assert sorted(got) == sorted(want) == sorted(ref)
    differ = {k: (float(got[k]), float(want[k])) for k in want if not _is_box(k) and not torch.equal(got[k], want[k])}
    assert not differ, differ
    fails = []
    for k in sorted(k for k in want if _is_box(k)):
        scale = max(abs(float(ref[k])), 1e-300)
        e, e_parent = abs(float(got[k]) - float(ref[k])) / scale, abs(float(want[k]) - float(ref[k])) / scale
        print("LOSS step %-32s err %.3e  parent %.3e  bound %.3e" % (k, e, e_parent, max(1e-6, 4 * e_parent)))
        if not e <= max(1e-6, 4 * e_parent):
            fails.append((k, e, e_parent))
    assert not fails, fails
    print("LOSS step: %d loss_boxes calls (%d with pairs); host waits of loss_dict %d with the pair kernels, %d without"
          % (n_calls, n_with_pairs, got_waits, want_waits))
    assert got_waits <= want_waits - n_calls + 1, (got_waits, want_waits, n_calls)
