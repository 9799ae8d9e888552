"""GPU: hipie_msda_raw_backward (csrc/msda_bwd.hip: the gather form with the location and the softmax recomputed from ref / offsets /
logits), the autograd node over it (functions.DeformSampleFunction) and the opt-in HipBackendDeformable wiring of the training step.

Yardstick: torch.autograd.grad in float64 through the plain composition over oracle.ops.ms_deform_attn_core (tests/_msda_raw_cases.py),
gradients with respect to value, offsets, logits and ref, measured with util.rel_err.  Bound: 2e-5 for each -- the project's bound for
grad_sampling_loc / grad_attn_weight; grad_value gets it too (not the 3e-6 of the loc-fed kernel) because the location is now computed in
fp32 from ref and offsets.  The same composition in fp32 on the CPU stays below 1e-5 on these inputs (test_msda_raw_cpu.py)."""

import pytest
import torch

import _msda_raw_cases as cases
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-5
WIDE = 384                                           # columns of the buffer the "strided" case cuts its blocks from; logits start at 256


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


_CACHE = {}


def _case(name):
    """(inputs, float64 gradients, fp32 device tensors) of a case, computed once and shared"""
    if name not in _CACHE:
        c = cases.build(name)
        d = {k: c[k].float().to(DEV) for k in ("value", "ref", "offsets", "logits", "gout")}
        d["sh"], d["ls"] = c["sh"].to(DEV), c["ls"].to(DEV)
        _CACHE[name] = (c, cases.gradients(c), d)
    return _CACHE[name]


def _raw(c, d, want_ref=True, strided=False):
    """one call of the entry itself with every output NaN-filled before it -> (grad_value, grad_offsets, grad_logits, grad_ref | None,
    workspace bytes, the output buffer of the strided form | None)"""
    from hipie_amd import _lib
    lib = _lib.load()
    B, S, M, L, Lq, P, rd = c["B"], c["S"], c["M"], c["L"], c["Lq"], c["P"], c["ref_dim"]
    offw, logw = M * L * P * 2, M * L * P
    nan = float("nan")
    gv = torch.full((B, S, M, cases.D), nan, device=DEV)
    gref = torch.full((B, Lq, L, rd), nan, device=DEV) if want_ref else None
    off, lg, buf = d["offsets"], d["logits"], None
    if strided:
        assert offw <= 256 and 256 + logw <= WIDE
        src = torch.full((B, Lq, WIDE), nan, device=DEV)
        src[..., :offw] = off.reshape(B, Lq, offw)
        src[..., 256:256 + logw] = lg.reshape(B, Lq, logw)
        off, lg = src[..., :offw], src[..., 256:256 + logw]
        buf = torch.full((B, Lq, WIDE), nan, device=DEV)
        goff, glog = buf[..., :offw], buf[..., 256:256 + logw]
        strides = (WIDE, WIDE, WIDE, WIDE)
    else:
        goff, glog = torch.full((B, Lq, offw), nan, device=DEV), torch.full((B, Lq, logw), nan, device=DEV)
        strides = (offw, logw, offw, logw)
    need = int(lib.hipie_msda_raw_backward_ws_bytes(B, S, M, L, Lq, P, rd, int(want_ref)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.hipie_msda_raw_backward(d["value"].data_ptr(), d["sh"].data_ptr(), d["ls"].data_ptr(), d["ref"].data_ptr(), off.data_ptr(), lg.data_ptr(),
                                     d["gout"].data_ptr(), gv.data_ptr(), goff.data_ptr(), glog.data_ptr(), gref.data_ptr() if want_ref else None,
                                     B, S, M, cases.D, L, Lq, P, rd, *strides, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.hipie_last_error()
    torch.cuda.synchronize()
    return gv, goff.reshape(B, Lq, M, L, P, 2), glog.reshape(B, Lq, M, L * P), gref, need, buf


def _check(name, got, want):
    """all four gradients finite everywhere and within BOUND of float64; figures printed before the assertion"""
    errs = []
    for g, w in zip(got[:4], want):
        assert bool(torch.isfinite(g).all())
        errs.append(rel_err(g.cpu(), w))
    print("MSDA_RAW %s: value %.1e offsets %.1e logits %.1e ref %.1e (bound %.0e)" % (name, *errs, BOUND))
    assert max(errs) < BOUND, errs


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_msda_raw_backward_against_float64_autograd(name):
    c, want, d = _case(name)
    got = _raw(c, d)
    _check(name, got, want)
    if name == "all_outside":                        # all four exactly zero, grad_value fully written
        assert all(float(g.abs().max()) == 0.0 for g in got[:4])
    if name == "flat":                               # equal logits: the softmax backward sums to zero over an item
        assert float(got[2].sum(-1).abs().max()) <= 1e-6 * float(want[2].abs().max())
    if name == "gapped":                             # rows no level covers
        gap = torch.ones(c["S"], dtype=torch.bool)
        gap[c["rows"]] = False
        assert int(gap.sum()) == cases.GAP * c["L"] and float(got[0][:, gap.to(DEV)].abs().max()) == 0.0


def test_msda_raw_backward_strided_blocks_equal_the_dense_call_bit_for_bit():
    c, want, d = _case("enc3")
    dense, wide = _raw(c, d), _raw(c, d, strided=True)
    _check("strided", wide, want)
    assert torch.equal(wide[1], dense[1]) and torch.equal(wide[2], dense[2]) and torch.equal(wide[3], dense[3])
    assert float((wide[0] - dense[0]).abs().max()) <= BOUND * float(want[0].abs().max())      # grad_value sums in arrival order
    # nothing outside the two column blocks of the output buffer was written
    offw, logw = c["M"] * c["L"] * c["P"] * 2, c["M"] * c["L"] * c["P"]
    untouched = torch.ones(WIDE, dtype=torch.bool)
    untouched[:offw] = False
    untouched[256:256 + logw] = False
    assert bool(torch.isnan(wide[5][..., untouched.to(DEV)]).all())


def test_msda_raw_backward_without_grad_ref():
    c, want, d = _case("enc3")
    full, bare = _raw(c, d), _raw(c, d, want_ref=False)
    assert bare[3] is None and bare[4] < full[4]                                              # the workspace query is smaller
    assert torch.equal(bare[1], full[1]) and torch.equal(bare[2], full[2])
    assert bool(torch.isfinite(bare[0]).all()) and float((bare[0] - full[0]).abs().max()) <= BOUND * float(want[0].abs().max())
    assert rel_err(bare[0].cpu(), want[0]) < BOUND


@pytest.mark.parametrize("name", ["enc3", "dec4"])
def test_msda_raw_backward_is_bit_reproducible(name):
    c, _, d = _case(name)
    a, b = _raw(c, d), _raw(c, d)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


@pytest.mark.parametrize("name", ["enc3", "dec4"])
def test_msda_raw_backward_against_the_existing_pair(name):
    """loc / aw built with fp32 torch, ops.ms_deform_attn_backward, autograd's chain back to the projections: all four gradients within
    2e-5 of each one's scale of the node's; the op layer's call equals the direct one"""
    from hipie_amd import ops
    c, want, d = _case(name)
    got = _raw(c, d)
    ref, off, lg = (d[k].clone().requires_grad_(True) for k in ("ref", "offsets", "logits"))
    wh = torch.tensor([[w, h] for h, w in c["shapes"]], dtype=torch.float32, device=DEV)[None, None, None, :, None, :]
    if c["ref_dim"] == 2:
        loc = ref[:, :, None, :, None, :] + off / wh
    else:
        loc = ref[:, :, None, :, None, :2] + off / c["P"] * ref[:, :, None, :, None, 2:] * 0.5
    aw = torch.softmax(lg, -1).view(c["B"], c["Lq"], c["M"], c["L"], c["P"])
    gv, gloc, gaw = ops.ms_deform_attn_backward(d["value"], d["sh"], d["ls"], loc.detach().contiguous(), aw.detach().contiguous(), d["gout"], 64)
    goff, glg, gref = torch.autograd.grad((loc, aw), (off, lg, ref), (gloc, gaw))
    diffs = []
    for mine, theirs, w in zip(got[:4], (gv, goff, glg, gref), want):
        diffs.append(float((mine - theirs).abs().max()) / float(w.abs().max()))
    print("MSDA_RAW %s vs the existing pair: value %.1e offsets %.1e logits %.1e ref %.1e" % (name, *diffs))
    assert max(diffs) <= BOUND, diffs
    via_ops = ops.msda_raw_backward(d["value"], d["sh"], d["ls"], d["ref"], d["offsets"], d["logits"], d["gout"])
    assert torch.equal(via_ops[1], got[1]) and torch.equal(via_ops[2].reshape(got[2].shape), got[2]) and torch.equal(via_ops[3], got[3])
    assert rel_err(via_ops[0].cpu(), want[0]) < BOUND


@pytest.mark.parametrize("name", ["enc3", "dec4"])
def test_deform_sample_function(name, monkeypatch):
    """the node: forward = ops.msda_fused, backward fills .grad of value / offsets / logits and of ref only when it requires grad"""
    from hipie_amd import ops
    from hipie_amd.training import functions
    c, want, d = _case(name)
    asked = []
    real = ops.msda_raw_backward

    def spy(*a, **k):
        asked.append(bool(k["want_grad_ref"]))
        out = real(*a, **k)
        assert (out[3] is not None) == asked[-1]
        return out
    monkeypatch.setattr(ops, "msda_raw_backward", spy)
    for ref_grad in (True, False):
        value, off, lg = (d[k].clone().requires_grad_(True) for k in ("value", "offsets", "logits"))
        ref = d["ref"].clone().requires_grad_(ref_grad)
        out = functions.deform_sample(value, c["shapes"], ref, off, lg)
        assert out is not None and torch.equal(out, ops.msda_fused(d["value"], d["sh"], d["ls"], d["ref"], d["offsets"], d["logits"]))
        out.backward(d["gout"])
        grads = (value.grad, off.grad, lg.grad) + ((ref.grad,) if ref_grad else ())
        assert (ref.grad is not None) == ref_grad and asked[-1] == ref_grad
        for g, w in zip(grads, want):
            assert g is not None and rel_err(g.cpu(), w) < BOUND
    assert asked == [True, False]


def test_deform_sample_declines_without_a_launch(monkeypatch):
    from hipie_amd import ops
    from hipie_amd.training import functions

    def no_call(*a, **k):
        raise AssertionError("a library call")
    for name in ("_call", "_size", "msda_fused", "msda_raw_backward"):
        monkeypatch.setattr(ops, name, no_call)
    shapes = [(4, 4), (2, 2)]

    def args(D=32, S=20, dtype=torch.float32):
        return (torch.empty(1, S, 8, D, dtype=dtype, device=DEV), shapes, torch.empty(1, 5, 2, 2, dtype=dtype, device=DEV),
                torch.empty(1, 5, 8, 2, 4, 2, dtype=dtype, device=DEV), torch.empty(1, 5, 8, 8, dtype=dtype, device=DEV))
    assert functions.deform_sample_ok(*[a for a in args() if torch.is_tensor(a)])
    for kw in (dict(D=64), dict(dtype=torch.float64), dict(S=functions.MSDA_RAW_MAX_ROWS + 1)):
        assert functions.deform_sample(*args(**kw)) is None, kw


def test_train_step_with_the_deformable_node_matches_the_reference(monkeypatch):
    """test_training.test_train_step_losses_and_gradients_match_the_reference with backend=net.HipBackendDeformable: the same fixture, the same
    assertions and bounds for cuda (loss entries 2e-3, the three gradient classes 5e-3 / 5e-3 / 8e-2, the same random draws), and every
    msda_module call of the step answered by the node, at both reference-point widths"""
    from _train_step_cases import check_step_against_golden, train_step_case
    from hipie_amd.training import functions, net
    z, meta, model, step, batch, targets = train_step_case("cuda", net.HipBackendDeformable)
    modules, answered = [], []

    def counted_module(*a, _f=net.msda_module, **k):
        modules.append(1)
        return _f(*a, **k)

    def counted_node(value, shapes, ref, offsets, logits, _f=functions.deform_sample):
        out = _f(value, shapes, ref, offsets, logits)
        answered.append((int(ref.shape[-1]), out is not None))
        return out
    monkeypatch.setattr(net, "msda_module", counted_module)
    monkeypatch.setattr(functions, "deform_sample", counted_node)
    losses = step.loss_dict(batch, targets)
    total = sum(losses.values())
    total.backward()
    widths = sorted(set(w for w, _ in answered))
    print("MSDA_RAW step: %d msda_module calls, %d answered by the node, reference-point widths %s" % (len(modules), sum(ok for _, ok in answered), widths))
    assert len(modules) > 0 and len(answered) == len(modules) and all(ok for _, ok in answered) and widths == [2, 4]
    check_step_against_golden(z, model, step, losses, total, "cuda", "MSDA_RAW step")
