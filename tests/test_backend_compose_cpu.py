"""CPU: net.backend(*names) -- the composer of the opt-in kernel groups of the training step -- over EVERY subset of net.GROUPS, what
TrainStep derives from a composed class, and the flags of tools/bench_train_step.py.  No kernel runs: classes are built and looked at."""
import os
import sys

import pytest

from hipie_amd.training import net

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from bench_train_step import FLAGS, backend_names  # noqa: E402

NAMES = list(net.GROUPS)
VIT = ("norms", "mlp", "packed_windows", "deformable")


def _public(cls):
    return {n for n in dir(cls) if not n.startswith("_")}


def _own(cls):
    return {n for n in vars(cls) if not n.startswith("_")}


def _definers(cls):
    """op -> the class of cls's MRO whose own function cls resolves it to"""
    return {op: next(c for c in cls.__mro__ if op in vars(c)) for op in _public(cls)}


def test_every_subset_composes_to_the_union_of_its_groups():
    base = _definers(net.HipBackend)
    per_group = {n: _definers(c) for n, c in net.GROUPS.items()}
    for bits in range(1 << len(NAMES)):
        subset = [n for i, n in enumerate(NAMES) if bits >> i & 1]
        be = net.backend(*subset)
        candidates = {}
        for d in [base] + [per_group[n] for n in subset]:
            for op, c in d.items():
                candidates.setdefault(op, set()).add(c)
        assert _public(be) == set(candidates), subset
        for op, cs in candidates.items():
            top = [c for c in cs if all(issubclass(c, o) for o in cs)]          # the definer every other definer is a base of
            assert len(top) == 1 and getattr(be, op) is vars(top[0])[op].__func__, (subset, op)


def test_no_op_is_defined_by_two_unrelated_groups():
    groups = list(net.GROUPS.values())
    shared = [(a, b, _own(a) & _own(b)) for i, a in enumerate(groups) for b in groups[i + 1:] if _own(a) & _own(b)]
    assert shared == [(net.HipBackendPackedAttention, net.HipBackendPackedWindows, {"packed_attention"})] and issubclass(shared[0][1], shared[0][0])


def test_backend_returns_existing_classes_and_one_object_per_set():
    assert NAMES == ["norms", "mlp", "windows", "packed_attention", "packed_windows", "deformable",
                     "losses", "criteria", "matching", "hungarian", "assign", "pair_losses"]
    assert net.backend() is net.HipBackend
    for n, c in net.GROUPS.items():
        assert net.backend(n) is c and net.backend(n, n) is c
    assert net.backend("losses", "matching") is net.HipBackendMatching and net.backend("pair_losses", "criteria", "losses", "assign") is net.HipBackendPairLosses
    assert net.backend("windows", "packed_attention", "packed_windows") is net.HipBackendPackedWindows
    assert net.backend("norms", "mlp") is net.HipBackendNormsMlp and net.backend("windows", "mlp", "norms") is net.HipBackendAll
    be = net.backend(*VIT, "pair_losses")
    assert be.__bases__ == (net.HipBackendNorms, net.HipBackendMlp, net.HipBackendPackedWindows, net.HipBackendDeformable, net.HipBackendPairLosses)
    assert net.backend("pair_losses", "deformable", "packed_windows", "mlp", "norms") is be
    assert net.backend(*NAMES) is be and _public(be) == set().union(*map(_public, net.GROUPS.values()))
    with pytest.raises(ValueError, match="'fused'.*known: norms, mlp, windows, .*pair_losses"):
        net.backend("norms", "fused")


@pytest.mark.parametrize("extra", [(), ("losses",), ("matching",), ("pair_losses",)], ids=lambda e: e[0] if e else "none")
def test_train_step_derives_the_ops_of_the_criteria_and_matchers_from_a_composed_backend(extra):
    from _train_step_cases import train_step_case
    be = net.backend(*VIT, *extra)
    step = train_step_case("cpu", be)[3]
    loss_ops = be if hasattr(be, "point_mask_loss") else None
    match_ops = be if any(hasattr(be, op) for op in ("mask_match_costs", "ota_match", "hungarian_costs")) else None
    assert (loss_ops is None) == (extra == ()) and (match_ops is None) == (extra in ((), ("losses",)))              # the four cases differ
    assert step.be is be and step.criterion.ops is loss_ops and step.md_criterion.ops is loss_ops
    assert step.matchers == (step.matcher, step.matcher_bg, step.md_criterion.matcher) and all(m.ops is match_ops for m in step.matchers)
    assert all(m.defer_status is hasattr(be, "hungarian_match") for m in step.matchers) and hasattr(be, "hungarian_match") == (extra == ("pair_losses",))


# the flags as tools/bench_train_step.py read them before net.backend(): the classes its `if` chain mixed for each command line
FLAG_SETS = [
    ("", [net.HipBackend]),
    ("--hand-norms --fused-mlp", [net.HipBackendNormsMlp]),
    ("--fused-losses --fused-criteria", [net.HipBackendCriteria]),
    ("--fused-criteria --fused-hungarian", [net.HipBackendHungarian]),
    ("--fused-losses --fused-assign --hand-norms", [net.HipBackendNorms, net.HipBackendAssign]),
    ("--packed-attention --packed-windows --fused-windows", [net.HipBackendWindows, net.HipBackendPackedWindows]),
    ("--hand-norms --fused-mlp --packed-windows --fused-msda --fused-pair-losses",
     [net.HipBackendNormsMlp, net.HipBackendPackedWindows, net.HipBackendDeformable, net.HipBackendPairLosses]),
    (" ".join(FLAGS), [net.HipBackendAll, net.HipBackendPackedWindows, net.HipBackendDeformable, net.HipBackendPairLosses]),
]


@pytest.mark.parametrize("line,classes", FLAG_SETS, ids=["none"] + [f for f, _ in FLAG_SETS[1:-1]] + ["all"])
def test_bench_train_step_flags_select_the_ops_they_did(line, classes):
    names, rest = backend_names(["4"] + line.split() + ["7"])
    assert rest == ["4", "7"] and list(FLAGS.values()) == NAMES                  # batch and steps survive; one flag per group
    be = net.backend(*names)
    want = {}
    for c in classes:                                                            # a later class of a list overrides, as the tool's mix-ins did
        want.update({op: getattr(c, op) for op in _public(c)})
    assert _public(be) == set(want) and all(getattr(be, op) is f for op, f in want.items())
    assert len(classes) > 1 or be is classes[0]
