"""hipie_amd/derived.py: the one cache for values derived from parameters -- when it hits, when it misses, what it keeps alive --
and the call sites whose hand-written keys had holes (biases left out of the key)."""
import gc
import weakref

import torch
import torch.nn as nn

from hipie_amd import derived as D
from hipie_amd.derived import derived


class _Owner:
    pass


def _counted(value_of):
    calls = []

    def build():
        calls.append(1)
        return value_of()
    return build, calls


def test_hit_returns_the_same_object_and_builds_once():
    lin, own = nn.Linear(8, 4), _Owner()
    build, calls = _counted(lambda: lin.weight.detach() * 2)
    a = derived(own, "w2", [lin.weight, lin.bias], build)
    b = derived(own, "w2", [lin.weight, lin.bias], build)
    assert a is b and len(calls) == 1
    assert not a.requires_grad                                           # build() runs under no_grad
    grad_seen = []
    derived(own, "g", [lin.weight], lambda: grad_seen.append(torch.is_grad_enabled()))
    assert grad_seen == [False]
    D.clear(lin)                                                         # clear() walks modules: `own` is not one, its entries stay
    assert derived(own, "w2", [lin.weight, lin.bias], build) is a and len(calls) == 1


def test_every_way_of_changing_a_parameter_misses_exactly_once():
    lin, own = nn.Linear(8, 4), _Owner()
    build, calls = _counted(lambda: lin.weight.detach().float().clone())

    def get(extra=()):
        return derived(own, "w", [lin.weight, lin.bias], build, extra=extra)
    seen = [get()]

    def rebuilt_once(extra=()):
        n = len(calls)
        v = get(extra)
        assert len(calls) == n + 1 and all(v is not s for s in seen)
        assert get(extra) is v and len(calls) == n + 1
        seen.append(v)
        return v
    with torch.no_grad():
        lin.weight.mul_(2)                                               # in place: _version
    assert torch.equal(rebuilt_once(), lin.weight.detach())
    lin.weight.data = lin.weight.data.clone()                            # data_ptr
    rebuilt_once()
    lin.weight.data = lin.weight.data.half()                             # dtype (what cast_head / cast_weights / set_compute_dtype do)
    rebuilt_once()
    lin.weight.data = lin.weight.data.float()
    rebuilt_once()
    lin.load_state_dict({"weight": torch.ones(4, 8), "bias": torch.zeros(4)})
    assert torch.equal(rebuilt_once(), torch.ones(4, 8))
    rebuilt_once(extra=(7, 7))                                           # what is not a tensor: the token grid, a dtype, a format tag
    rebuilt_once(extra=())                                               # keep=1: ONE entry per name, the other grid replaced it
    assert len(own.__dict__["_derived"]["w"]) == 1


def test_keep_holds_several_extras_side_by_side():
    p, own = nn.Parameter(torch.zeros(3)), _Owner()
    build, calls = _counted(lambda: torch.zeros(1))
    for i in range(5):
        derived(own, "g", [p], build, extra=i, keep=3)
    assert len(calls) == 5 and list(own.__dict__["_derived"]["g"]) == [2, 3, 4]
    derived(own, "g", [p], build, extra=3, keep=3)
    assert len(calls) == 5
    derived(own, "g", [p], build, extra=0, keep=3)                       # evicted: rebuilt
    assert len(calls) == 6


def test_none_is_a_parameter_too():
    w, b, own = nn.Parameter(torch.zeros(4, 8)), nn.Parameter(torch.zeros(4)), _Owner()
    build, calls = _counted(lambda: torch.zeros(1))
    a = derived(own, "x", [w, None], build)
    assert derived(own, "x", [w, None], build) is a and len(calls) == 1
    c = derived(own, "x", [w, b], build)                                 # a bias appears
    assert c is not a and len(calls) == 2
    assert derived(own, "x", [w, None], build) is not c and len(calls) == 3       # ... and disappears
    assert D.stamp([w, None])[1] is None


def test_entry_keeps_no_parameter_alive_and_a_forged_stamp_misses(monkeypatch):
    lin, own = nn.Linear(8, 4), _Owner()
    build, calls = _counted(lambda: torch.zeros(1))
    derived(own, "w", [lin.weight, lin.bias], build)
    refs, st, _ = own.__dict__["_derived"]["w"][()]
    assert all(r() is not None for r in refs)
    del lin
    gc.collect()
    assert all(r() is None for r in refs)                                # the entry held the parameters weakly
    fresh = nn.Linear(8, 4)
    monkeypatch.setattr(D, "stamp", lambda params: st)                   # as if the allocator had handed out the same addresses again
    assert D.stamp([fresh.weight, fresh.bias]) == st
    derived(own, "w", [fresh.weight, fresh.bias], build)
    assert len(calls) == 2                                               # equal stamp, other tensors: a miss
    derived(own, "w", [fresh.weight, fresh.bias], build)
    assert len(calls) == 2


def test_clear_drops_every_entry_of_a_module_tree():
    net = nn.Sequential(nn.Linear(4, 4), nn.Sequential(nn.Linear(4, 4)))
    for m in net.modules():
        if isinstance(m, nn.Linear):
            derived(m, "w", [m.weight], lambda: torch.zeros(1))
    assert sum("_derived" in m.__dict__ for m in net.modules()) == 2
    D.clear(net)
    assert sum("_derived" in m.__dict__ for m in net.modules()) == 0
    assert "_derived" not in net.state_dict() and not any("_derived" in k for k in net.state_dict())


def test_batched_decoder_values_follow_a_bias_changed_alone():
    """the concatenated value projections of the decoder layers: the biases were not in the hand-written key, so a bias changed alone
    kept the old concatenation (this test fails on the commit before the helper)"""
    from hipie_amd.modeling import transformer as T
    torch.manual_seed(0)
    layers = nn.ModuleList(T.DeformableTransformerDecoderLayer(32, 64, 2, 4, 2, torch.float32) for _ in range(2))
    owner, src = nn.Module(), torch.randn(1, 5, 32)
    with torch.no_grad():
        first = [v.clone() for v in T.batched_decoder_values(owner, layers, src)]
        vp = layers[1].cross_attn.value_proj
        vp.bias.add_(1.0)
        got = T.batched_decoder_values(owner, layers, src)
        want = [nn.functional.linear(src, l.cross_attn.value_proj.weight, l.cross_attn.value_proj.bias) for l in layers]
    for g, w, f in zip(got, want, first):
        assert torch.allclose(g.flatten(2), w, atol=1e-6)
    assert torch.equal(got[0], first[0]) and not torch.allclose(got[1], first[1])


def test_transposed_mlp_head_follows_a_replaced_bias():
    """ops._transposed (box head, reference-point MLP): the hand-written key carried only the bias's version counter, which a bias
    replaced through ``.data =`` does not move.  The biases here are strided views, so that what is cached is a real copy and not the
    parameter object itself (this test fails on the commit before the helper)"""
    from hipie_amd import ops
    from hipie_amd.modeling import transformer as T
    mlp = T.MLP(8, 8, 4, 3)
    mlp.layers[1].bias.data = torch.zeros(16)[::2]
    before = ops._transposed(list(mlp.layers))
    assert ops._transposed(list(mlp.layers)) is before and torch.equal(before[1][1], torch.zeros(8))
    mlp.layers[1].bias.data = torch.full((16,), 3.0)[::2]
    after = ops._transposed(list(mlp.layers))
    assert torch.equal(after[1][1], torch.full((8,), 3.0))
    for (wt, b), l in zip(after, mlp.layers):
        assert torch.equal(wt, l.weight.detach().t()) and torch.equal(b, l.bias.detach())


def test_training_weight_copies_die_with_the_weight():
    """training/net.py HipBackend.linear: the HL8 copies of W and W^T live on the weight tensor (they used to live in a class-global
    dict keyed by parameter NAME, which a second model in the process could hit and which outlived every model)"""
    from hipie_amd import ops
    from hipie_amd.training.net import HipBackend
    assert not hasattr(HipBackend, "_owners")
    w = nn.Parameter(torch.randn(16, 32))
    # what functions.SplitLinearFunction does with the (owner, key) = (weight, "w") that HipBackend.linear hands it
    w_hl8 = ops.split_weight(w, "w", [w], lambda: w)[0]
    wt_hl8 = ops.split_weight(w, "w.T", [w], lambda: w.t().contiguous())[0]
    assert ops.split_weight(w, "w", [w], lambda: w)[0] is w_hl8 and tuple(wt_hl8.shape) == (32, 32)
    assert torch.allclose(ops.hl8_unpack(w_hl8), w.detach(), atol=1e-6)
    alive = [weakref.ref(w_hl8), weakref.ref(wt_hl8), weakref.ref(w)]
    del w, w_hl8, wt_hl8
    gc.collect()
    assert all(r() is None for r in alive)
