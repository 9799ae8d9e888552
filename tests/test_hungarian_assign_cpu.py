"""CPU: the assignment kernel's algorithm restated (tests/_assign_cases.py) against the installed scipy on matrices with real ties; the ABI
surface and the refusals of hipie_hungarian_assign; the binding; the plumbing of HungarianMatcher with a plain-torch stand-in for
net.HipBackendAssign (device pairs, defer_status / check); the backend being opt-in."""
import ctypes

import numpy as np
import pytest
import torch

from _assign_cases import (FILLS, RAW_SHAPES, ST_INFEASIBLE, ST_INVALID, TorchAssignOps, adversarial, duplicated, filled, lsa_restated, lsa_sequential,
                           scipy_pairs, tie_matrices)
from _hungarian_cases import W_BOX, Golden, TorchHungarianOps, hungarian_case, same_pairs
from hipie_amd import _lib
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights
from test_training import Replay

P_ = ctypes.c_void_p(256)
NAMES = ("C", "cost_status", "n_tgt", "t_off", "pair_q", "pair_t", "status", "ws")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype == np.int64


# ------------------------------------------------------------------------------------------------ the restatement is scipy's solver
def test_the_restatement_is_scipy_on_tie_heavy_integer_matrices():
    """1000 seeded matrices of shapes 1..13 x 1..13 with 0/1 and 0..2 costs: the data-parallel selection AND the sequential scan"""
    for k, C in enumerate(tie_matrices(0)):
        want = scipy_pairs(C)
        assert _same(lsa_restated(C), want), (k, C)
        assert _same(lsa_sequential(C), want), (k, C)


@pytest.mark.parametrize("shape", [(20, 37), (300, 37), (900, 100)], ids=lambda s: "%dx%d" % s)
def test_the_restatement_is_scipy_with_duplicated_rows_and_columns(shape):
    for seed in (0, 1):
        C = duplicated(*shape, seed)
        assert _same(lsa_restated(C), scipy_pairs(C)), seed
    assert _same(lsa_restated(C.T.copy()), scipy_pairs(C.T.copy()))


def test_the_restatement_is_scipy_on_the_fills_of_the_gpu_test():
    for Q, T in RAW_SHAPES[:-1]:
        for fill in FILLS:
            C = filled(Q, T, fill)
            assert _same(lsa_restated(C), scipy_pairs(C)), (Q, T, fill)
    for fill in ("zeros", "dup"):
        C = filled(*RAW_SHAPES[-1], fill)
        assert _same(lsa_restated(C), scipy_pairs(C)), fill


def test_the_adversarial_matrix_takes_the_longest_path():
    for (Q, T), inner in (((900, 100), 4951), ((100, 100), 5050)):
        C, count = adversarial(Q, T), []
        assert float(np.abs(C).max()) < 2 ** 24
        assert _same(lsa_restated(C, count), scipy_pairs(C)) and count == [inner]
    big = adversarial(4096, 256).astype(np.float64)
    assert float(np.abs(big).max()) < 2 ** 24 and np.array_equal(big, np.rint(big))          # exact in fp32 at the limit shape


def test_the_restatement_raises_where_scipy_raises():
    C = np.arange(12, dtype=np.float32).reshape(4, 3)
    for bad, msg in ((np.nan, "invalid numeric"), (-np.inf, "invalid numeric")):
        D = C.copy()
        D[2, 1] = bad
        for f in (scipy_pairs, lsa_restated):
            with pytest.raises(ValueError, match=msg):
                f(D)
    col = C.copy()
    col[:, 1] = np.inf                                                   # 4 x 3 is solved transposed: the solver's row 1 is all +inf
    row = C.T.copy()
    row[1, :] = np.inf                                                   # 3 x 4: row 1 is all +inf
    for D in (col, row, np.full((2, 2), np.inf, dtype=np.float32)):
        for f in (scipy_pairs, lsa_restated):
            with pytest.raises(ValueError, match="infeasible"):
                f(D)
    E = C.copy()
    E[0, 0] = E[3, 2] = np.inf                                           # +inf entries are legal
    assert _same(lsa_restated(E), scipy_pairs(E))


# ------------------------------------------------------------------------------------------------ the ABI, refusals without a launch
def _assign(lib, B=2, Q=70, Tmax=9, sum_t=15, ws_bytes=1 << 20, **ptrs):
    """the entry with made-up pointers: only calls that are refused or return early"""
    v = {k: P_ for k in NAMES}
    v.update(ptrs)
    return lib.hipie_hungarian_assign(v["C"], v["cost_status"], v["n_tgt"], v["t_off"], v["pair_q"], v["pair_t"], v["status"], v["ws"], ws_bytes, B, Q, Tmax,
                                      sum_t, None)


def test_abi_surface():
    c_p, c_i, c_l = _lib.c_p, _lib.c_i, _lib.c_l
    assert _lib.SIGNATURES["hipie_hungarian_assign"] == [c_p] * 8 + [c_l, c_l, c_i, c_i, c_l, c_p]
    lib = _lib.load()
    assert hasattr(lib, "hipie_hungarian_assign") and hasattr(lib, "hipie_hungarian_assign_ws_bytes")
    assert lib.hipie_hungarian_assign_ws_bytes.restype is ctypes.c_int64
    assert lib.hipie_hungarian_assign_ws_bytes(70, 15) == 70 * 15 * 4 and lib.hipie_hungarian_assign_ws_bytes(70, 0) > 0
    assert lib.hipie_version() == 13                                                       # a new entry, the ABI number stays


def test_limits_and_null_pointers_are_refused_without_a_launch():
    lib = _lib.load()
    for kw, msg in (({"Q": 4097}, b"Q=4097"), ({"Tmax": 257}, b"Tmax=257"), ({"B": -1}, b"negative"), ({"B": 65536}, b"exceed the grid"),
                    ({"sum_t": 19}, b"sum_t=19"), ({"sum_t": -1}, b"negative"), ({"ws_bytes": 70 * 15 * 4 - 1}, b"workspace"),
                    ({"ws": ctypes.c_void_p(258)}, b"workspace")):
        assert _assign(lib, **kw) == -22 and msg in lib.hipie_last_error(), (kw, lib.hipie_last_error())
    for name in NAMES:
        assert _assign(lib, **{name: None}) == -22 and b"null" in lib.hipie_last_error(), name
    assert _assign(lib, Q=4096, Tmax=256, sum_t=512, ws_bytes=1 << 30, status=None) == -22 and b"null" in lib.hipie_last_error()


def test_empty_problems_return_without_a_launch():
    lib = _lib.load()
    none = {k: None for k in NAMES}
    for B, Q, T in ((0, 70, 9), (2, 0, 9), (2, 70, 0), (0, 0, 0)):
        assert _assign(lib, B=B, Q=Q, Tmax=T, sum_t=0, ws_bytes=0, **none) == 0


def test_the_binding_refuses_before_the_device_is_asked():
    from hipie_amd import ops
    costs = torch.zeros(7 * 4 + 2)
    n, off = torch.tensor([3, 1], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    for args, kw, msg in (((costs.double(), n, off, 4, 7, 3), {}, "costs must be torch.float32"), ((costs[:-1], n, off, 4, 7, 3), {}, r"costs must be \(30,\)"),
                          ((costs, n.long(), off, 4, 7, 3), {}, "n_tgt must be torch.int32"), ((costs, n[None], off, 4, 7, 3), {}, r"n_tgt must be \(B,\)"),
                          ((costs, n, off[:1], 4, 7, 3), {}, r"t_off must be \(2,\)"), ((costs, n, off, 7, 7, 3), {}, "sum_t=7"),
                          ((torch.zeros(64)[::2][:30], n, off, 4, 7, 3), {}, "costs tensor has to be contiguous")):
        with pytest.raises(RuntimeError, match=msg):
            ops.hungarian_assign(*args, **kw)
    for Q, T, msg in ((4097, 3, "Q=4097"), (7, 257, "Tmax=257")):
        with pytest.raises(RuntimeError, match=msg + ".*outside"):
            ops.hungarian_assign(torch.zeros(1), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0, Q, T)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.hungarian_assign(costs, n, off, 4, 7, 3)
    assert [bit for bit, _ in ops.HUNGARIAN_STATUS] == [1, 8, 16, 32, 64, 128]
    msgs = dict(ops.HUNGARIAN_STATUS)
    assert "invalid numeric" in msgs[32] and "infeasible" in msgs[64]


def test_hungarian_match_declines_and_short_cuts_on_the_host():
    from hipie_amd.training import functions
    logits, boxes, targets, pred = hungarian_case(2, 70, 9, 33, True, 0)
    packed = functions.pack_match_targets(targets, "cpu")
    assert functions.hungarian_match(torch.zeros(3, 4097, 33), torch.zeros(3, 4097, 4), packed, W_BOX) is None          # outside the limits: no launch
    with pytest.raises(ValueError, match="hungarian_match: targets packed for 3 images"):
        functions.hungarian_match(logits[:2], boxes[:2], packed, W_BOX)
    with pytest.raises(KeyError, match="without masks"):
        functions.hungarian_match(logits, boxes, functions.pack_match_targets(targets, "cpu", False), W_BOX, masks=pred, coords=[None] * 3)
    none = functions.pack_match_targets([targets[2]] * 2, "cpu")
    pairs, status = functions.hungarian_match(logits[:2], boxes[:2], none, W_BOX)                        # no target anywhere: no launch
    assert [(len(q), len(t), q.dtype) for q, t in pairs] == [(0, 0, torch.int64)] * 2 and status.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        functions.hungarian_match(logits, boxes, packed, W_BOX)


# ------------------------------------------------------------------------------------------------ the plumbing
class Recording:
    """a `draw` that records what it was asked for and answers from a seeded generator"""

    def __init__(self):
        self.asked, self.g = [], torch.Generator().manual_seed(11)

    def __call__(self, shape, device):
        self.asked.append(tuple(shape))
        return torch.rand(shape, generator=self.g).to(device)


def _reset():
    TorchHungarianOps.calls, TorchHungarianOps.decline, TorchAssignOps.match_calls = [], False, []


def test_the_matcher_asks_hungarian_match_and_draws_as_the_torch_path():
    logits, boxes, targets, pred = hungarian_case(2, 70, 9, 33, True, 0)
    w = MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0)
    plain_draw, ops_draw, declined_draw = Recording(), Recording(), Recording()
    plain = HungarianMatcher(w, num_points=50, draw=plain_draw, class_mode="map")
    with_ops = HungarianMatcher(w, num_points=50, draw=ops_draw, class_mode="map", ops=TorchAssignOps)
    _reset()
    want = [plain(logits, boxes, targets), plain(logits, boxes, targets, masks=pred), plain(logits, boxes, targets, masks=pred, costs=("cls", "mask")),
            plain.forward_boxes_only(logits, boxes, targets)]
    packed = with_ops.pack(targets, "cpu")
    assert packed.counts == [9, 6, 0]
    got = [with_ops(logits, boxes, targets), with_ops(logits, boxes, targets, masks=pred, packed=packed),
           with_ops(logits, boxes, targets, masks=pred, costs=("cls", "mask"), packed=packed), with_ops.forward_boxes_only(logits, boxes, targets, packed=packed)]
    assert TorchAssignOps.match_calls == [(True, True, "map", False), (True, True, "map", True), (True, False, "map", True), (False, True, "map", False)]
    assert all(same_pairs(g, w_) for g, w_ in zip(got, want))
    assert plain_draw.asked == ops_draw.asked == [(1, 50, 2)] * 6
    assert all(len(g[2][0]) == 0 and g[2][0].dtype == torch.int64 for g in got)
    assert with_ops.pending == [] and with_ops.calls == 4                                  # defer_status=False: checked inside the call
    # the op declines: the same draws, then the loop
    _reset()
    TorchHungarianOps.decline = True
    try:
        declined = HungarianMatcher(w, num_points=50, draw=declined_draw, class_mode="map", ops=TorchAssignOps, defer_status=True)
        again = [declined(logits, boxes, targets), declined(logits, boxes, targets, masks=pred, packed=packed),
                 declined(logits, boxes, targets, masks=pred, costs=("cls", "mask")), declined.forward_boxes_only(logits, boxes, targets)]
    finally:
        TorchHungarianOps.decline = False
    assert len(TorchAssignOps.match_calls) == 4 and declined_draw.asked == plain_draw.asked and declined.pending == []
    assert all(same_pairs(g, w_) for g, w_ in zip(again, want))

    class MatchOnly:                                       # an ops object with hungarian_match alone is asked, and packs
        pack_match_targets = TorchAssignOps.pack_match_targets
        hungarian_match = TorchAssignOps.hungarian_match
    m = HungarianMatcher(w, num_points=50, draw=Recording(), class_mode="map", ops=MatchOnly)
    assert m.pack(targets, "cpu") is not None and same_pairs(m(logits, boxes, targets), want[0])
    assert same_pairs(m(logits, boxes, targets, masks=pred), want[1])                      # no mask_match_costs op beside it: the loop


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "packs-itself"])
def test_the_reference_fixtures_through_the_assign_plumbing(packed):
    _reset()
    for name, (got, want) in Golden().run(TorchAssignOps, Replay, packed).items():
        assert same_pairs(got, want), name
    assert len(TorchAssignOps.match_calls) == 5


def _bad_targets():
    logits, boxes, targets, pred = hungarian_case(2, 70, 9, 33, True, 0)
    bad = [dict(t) for t in targets]
    bad[1]["positive_map"] = targets[1]["positive_map"].clone()
    bad[1]["positive_map"][4] = False                                                      # no positive token: a NaN column in image 1
    return logits, boxes, targets, bad


def test_status_words_raise_at_once_or_at_check():
    logits, boxes, targets, bad = _bad_targets()
    _reset()
    now = HungarianMatcher(W_BOX, stuff_takes_mean=False, class_mode="map", ops=TorchAssignOps)
    with pytest.raises(ValueError, match="image 1: matrix contains invalid numeric entries"):
        now(logits, boxes, bad)
    assert now.pending == []
    later = HungarianMatcher(W_BOX, stuff_takes_mean=False, class_mode="map", ops=TorchAssignOps, defer_status=True)
    good = later(logits, boxes, targets)
    pairs = later.forward_boxes_only(logits, boxes, bad)                                   # returns: nothing was read
    assert len(later.pending) == 2 and all(s.dtype == torch.int32 and s.shape == (3,) for s, _ in later.pending)
    assert not pairs[1][0].any() and not pairs[1][1].any() and len(pairs[1][0]) == 6       # the refused image: all-zero pairs, valid indices
    assert same_pairs([pairs[0]], [good[0]])                                               # the other images are solved
    with pytest.raises(ValueError, match=r"call 2 \(Q=70, class \+ box\): image 1: matrix contains invalid numeric entries"):
        later.check()
    assert later.pending == []                                                             # cleared by the raise too
    later.check()                                                                          # nothing pending: nothing read
    later(logits, boxes, targets)
    later.check()
    assert later.pending == []
    # check_all: several matchers, one list
    a = HungarianMatcher(W_BOX, class_mode="map", ops=TorchAssignOps, defer_status=True)
    b = HungarianMatcher(W_BOX, stuff_takes_mean=False, class_mode="map", ops=TorchAssignOps, defer_status=True)
    a(logits, boxes, targets)
    b(logits, boxes, bad)
    with pytest.raises(ValueError, match="image 1"):
        HungarianMatcher.check_all((a, b))
    assert a.pending == [] and b.pending == []


def test_an_infeasible_image_is_named():
    C = np.zeros((4, 3), dtype=np.float32)
    C[:, 1] = np.inf

    class Fixed(TorchAssignOps):
        @classmethod
        def hungarian_costs(cls, logits, *a, **k):
            return [C]
    logits, boxes, targets, _ = hungarian_case(1, 4, 3, 8, False, 0)
    with pytest.raises(ValueError, match="image 0: cost matrix is infeasible"):
        HungarianMatcher(W_BOX, class_mode="map", ops=Fixed)(logits, boxes, targets)
    assert (ST_INVALID, ST_INFEASIBLE) == (32, 64)


# ------------------------------------------------------------------------------------------------ the backends
def test_backend_assign_is_opt_in():
    from hipie_amd.training import net
    from hipie_amd.training.step import TrainStep      # noqa: F401
    assert issubclass(net.HipBackendAssign, net.HipBackendHungarian)
    for be in (net.HipBackend, net.HipBackendLosses, net.HipBackendCriteria, net.HipBackendMatching, net.HipBackendHungarian, net.HipBackendAll,
               net.HipBackendNorms, net.HipBackendMlp, net.HipBackendWindows):
        assert not hasattr(be, "hungarian_match"), be
    assert not issubclass(net.HipBackendAll, net.HipBackendAssign)
    assert set(vars(net.HipBackendAssign)) - {"__doc__", "__module__"} == {"hungarian_match"}          # it holds nothing else new
    m = HungarianMatcher()
    assert m.defer_status is False and m.pending == []
    logits, boxes, targets, _ = hungarian_case(1, 4, 3, 8, False, 0)
    packed = net.HipBackendAssign.pack_match_targets(targets, "cpu")
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        net.HipBackendAssign.hungarian_match(logits, boxes, packed, W_BOX)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        HungarianMatcher(W_BOX, class_mode="map", ops=net.HipBackendAssign)(logits, boxes, targets)
