"""GPU: hipie_point_mask_loss_forward / _backward and hipie_token_focal_forward / _backward (csrc/point_loss.hip) through the ops, the two
autograd Functions over them (functions.PointMaskLossFunction / TokenFocalFunction) and the opt-in HipBackendLosses wiring of the training
step.

Reference, metric and bound: tests/_loss_cases.py -- today's criterion.py / matcher.point_sample formulas on the CPU in float64 (reference)
and float32 (e_lib); max|got - ref64| / max|ref64| per output tensor against max(1e-6, 4 x e_lib).  Every case prints its figures (lines
starting with LOSS) before it asserts."""
import pytest
import torch

from _loss_cases import (POINT_NAMES, _special_points, bound_of, check, point_case, point_reference, point_yardsticks, token_case, token_reference)
from _train_step_cases import check_step_against_golden, train_step_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [pytest.param(0, -1.0, id="bce"), pytest.param(1, 0.25, id="focal"), pytest.param(1, -1.0, id="focal-no-alpha")]


def _point_chunk():
    """points per workgroup, read off the workspace query: it holds one partial per (instance, chunk of P)"""
    from hipie_amd import _lib
    ws = _lib.load().hipie_point_mask_loss_ws_bytes
    return next(p for p in range(1, 1 << 16) if ws(1, p + 1) > ws(1, p))


def _run_point(case, mode, alpha):
    from hipie_amd import ops
    src, tgt, idx, pts, gm, gd = (t.to(DEV) for t in case)
    lmask, ldice, sums = ops.point_mask_loss_forward(src, tgt, idx, pts, mode, alpha)
    d_src = ops.point_mask_loss_backward(src, tgt, idx, pts, sums, gm, gd, mode, alpha)
    assert lmask.shape == gm.shape and ldice.shape == gm.shape and sums.shape == (len(gm), 3) and d_src.shape == src.shape
    assert all(t.dtype == torch.float32 for t in (lmask, ldice, sums, d_src))
    assert torch.equal(gm, case[4].to(DEV)) and torch.equal(gd, case[5].to(DEV))          # the upstream gradients are left alone
    return lmask, ldice, sums, d_src


GEOMETRIES = [(1, 1, 1, 1, 1), (3, 5, 7, 20, 28), (2, 16, 16, 16, 16)]


@pytest.mark.parametrize("mode,alpha", MODES)
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_point_mask_loss_against_float64(geom, mode, alpha):
    chunk = _point_chunk()
    assert 64 <= chunk <= 1 << 14
    for P in (1, 63, 64, 65, 257, 400, chunk + 1, 2 * chunk + 3):
        key = geom + (P,)
        ref, lib = point_yardsticks(*key, mode, alpha)
        check("%s P=%d mode=%d alpha=%g" % (geom, P, mode, alpha), POINT_NAMES, _run_point(point_case(*key), mode, alpha), ref, lib)


def test_point_case_holds_the_special_points_and_index():
    src, tgt, idx, pts, _, _ = point_case(3, 5, 7, 20, 28, 65)
    p = pts[0]
    assert torch.equal(p[:11], torch.tensor(_special_points(5, 7)))               # pixel centres and boundaries among them
    assert (p == 0).all(1).any() and (p == 1).all(1).any() and (p < 0).any() and (p > 1).any()
    assert idx.tolist() == [3, 2, 3] and bool((tgt == 0).any()) and bool((tgt == 1).any()) and bool(((tgt > 0) & (tgt < 1)).any())


@pytest.mark.parametrize("mode,alpha", MODES)
def test_point_mask_loss_special_values(mode, alpha):
    """logits +-40 and +-100 against targets 0, 1 and 0.5 (every pairing): finite losses and gradients, within the bound of the case"""
    logit, label = [40.0, -40.0, 100.0, -100.0], [0.0, 1.0, 0.5]
    N, P = 12, 65
    src = torch.stack([torch.full((4, 4), logit[n % 4]) for n in range(N)])
    tgt = torch.stack([torch.full((6, 6), v) for v in label])
    idx = torch.tensor([n // 4 for n in range(N)])
    g = torch.Generator().manual_seed(5)
    pts = torch.rand(N, P, 2, generator=g)                       # near the border the zero padding blends the logits down: mid-range values too
    case = (src, tgt, idx, pts, torch.randn(N, generator=g), torch.randn(N, generator=g))
    got = _run_point(case, mode, alpha)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    check("special values mode=%d alpha=%g" % (mode, alpha), POINT_NAMES, got, point_reference(*case, mode, alpha, torch.float64),
          point_reference(*case, mode, alpha, torch.float32))


@pytest.mark.parametrize("mode,alpha", MODES[:2])
def test_point_mask_loss_exact_zeros(mode, alpha):
    from hipie_amd import ops
    src, tgt, idx, _, gm, gd = (t.to(DEV) for t in point_case(2, 16, 16, 16, 16, 400))
    # pixel coordinates in [1.1, 5.9]: the corners are rows and columns 1..6, nothing reads row / column 0 or those from 7 on
    pts = (torch.rand(2, 400, 2, generator=torch.Generator().manual_seed(9)) * 0.3 + 0.1).to(DEV)
    _, _, sums = ops.point_mask_loss_forward(src, tgt, idx, pts, mode, alpha)
    d = ops.point_mask_loss_backward(src, tgt, idx, pts, sums, gm, gd, mode, alpha)
    assert float(d[:, 1:7, 1:7].abs().min()) > 0
    assert max(float(t.abs().max()) for t in (d[:, 7:], d[:, :, 7:], d[:, 0], d[:, :, 0])) == 0
    zero = ops.point_mask_loss_backward(src, tgt, idx, pts, sums, torch.zeros_like(gm), torch.zeros_like(gd), mode, alpha)
    assert float(zero.abs().max()) == 0


@pytest.mark.parametrize("mode,alpha", MODES[:2])
def test_point_mask_loss_determinism(mode, alpha):
    from hipie_amd import ops
    key = (3, 5, 7, 20, 28, 2 * _point_chunk() + 3)
    case = point_case(*key)
    ref, lib = point_yardsticks(*key, mode, alpha)
    first = _run_point(case, mode, alpha)
    ops.point_mask_loss_forward(*(t.to(DEV) for t in point_case(2, 16, 16, 16, 16, 400)[:4]), 1 - mode, 0.5)     # other work in between
    torch.randn(1 << 20, device=DEV).sum()
    second = _run_point(case, mode, alpha)
    for a, b in zip(first[:3], second[:3]):
        assert torch.equal(a, b)                                 # the forward is bit-reproducible
    diff = float((first[3].double() - second[3].double()).abs().max() / ref[3].abs().max())
    print("LOSS determinism mode=%d: backward run-to-run %.3e, bound %.3e" % (mode, diff, bound_of(lib[3], ref[3])))
    assert diff <= bound_of(lib[3], ref[3])                      # atomics: the order of the additions is free


def test_point_mask_loss_out_of_range_index_reads_a_zero_target():
    from hipie_amd import ops
    src, tgt, idx, pts, _, _ = (t.to(DEV) for t in point_case(2, 16, 16, 16, 16, 65))
    got = ops.point_mask_loss_forward(src, tgt, torch.tensor([-1, 99], device=DEV), pts, 0)
    want = ops.point_mask_loss_forward(src, torch.zeros_like(tgt), idx, pts, 0)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------ token focal loss
TOKEN_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 40, 19), (3, 7, 257), (2, 900, 256)]


@pytest.mark.parametrize("keep", ["null", "all", "some", "image", "none"])
@pytest.mark.parametrize("B,Q,T", TOKEN_SHAPES)
def test_token_focal_against_float64(B, Q, T, keep):
    from hipie_amd import ops
    logits, onehot, mask = token_case(B, Q, T, keep)
    if keep == "image" and B == 1:
        keep = "none"                                            # one image with every token dropped IS everything dropped
    for alpha in (0.25, -1.0):
        ref, lib = token_reference(logits, onehot, mask, alpha, torch.float64), token_reference(logits, onehot, mask, alpha, torch.float32)
        ld, od = logits.to(DEV), onehot.to(DEV)
        kd = None if mask is None else (mask > 0).to(DEV)
        loss = ops.token_focal_forward(ld, od, kd, alpha)
        g = torch.tensor(1.7, device=DEV)
        d = ops.token_focal_backward(ld, od, kd, g, alpha)
        assert loss.shape == () and d.shape == logits.shape and float(g) == float(torch.tensor(1.7))
        check("token (%d,%d,%d) keep=%s alpha=%g" % (B, Q, T, keep, alpha), ("loss", "dlogits"), (loss, d / 1.7), ref, lib)
        assert torch.equal(loss, ops.token_focal_forward(ld, od, None if kd is None else kd.to(torch.uint8), alpha))      # bit-reproducible
        if mask is not None:
            dropped = (mask == 0)[:, None, :].expand_as(logits)
            assert float(d.cpu()[dropped].abs().max() if dropped.any() else 0.0) == 0
        if keep == "none":
            assert float(loss) == 0 and float(d.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ the Functions
@pytest.mark.parametrize("strided", [False, True], ids=["dense-targets", "strided-targets"])
def test_point_mask_loss_function_gradient_and_saved_storage(strided):
    """strided: the targets arrive as DetCriterion hands them over at mask stride 4 -- a view t[..., 2::4, 2::4] of full-resolution masks.
    What the node keeps is counted as the STORAGE behind every saved tensor (each storage once), so a saved view counts as what it pins."""
    from hipie_amd.training import functions
    key = (3, 5, 7, 20, 28, 257)
    src, tgt, idx, pts, gm, gd = (t.to(DEV) for t in point_case(*key))
    ref, lib = point_yardsticks(*key, 1, 0.25)
    if strided:
        full = torch.zeros(tgt.shape[0], 4 * tgt.shape[1], 4 * tgt.shape[2], device=DEV)
        full[:, 2::4, 2::4] = tgt
        tgt = full[:, 2::4, 2::4]
        assert not tgt.is_contiguous() and tgt.untyped_storage().nbytes() == 16 * tgt.numel() * 4
    src.requires_grad_(True)
    saved = {}
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.update({t.untyped_storage().data_ptr(): t.untyped_storage().nbytes()}) or t,
                                                  lambda t: t):
        lmask, ldice = functions.point_mask_loss(src, tgt, idx, pts, 1, 0.25)
    allowed = sum(t.numel() * t.element_size() for t in (src, pts, tgt, idx)) + len(gm) * 3 * 4
    print("LOSS Function (%s): saved storages %d bytes, allowed %d" % ("strided" if strided else "dense", sum(saved.values()), allowed))
    assert sum(saved.values()) <= allowed                        # nothing of N x P or N x Ht x Wt elements, no full-resolution storage pinned
    ((lmask * gm).sum() + (ldice * gd).sum()).backward()
    check("PointMaskLossFunction", ("lmask", "ldice", "d_src"), (lmask, ldice, src.grad), ref[:2] + ref[3:], lib[:2] + lib[3:])


def test_frozen_inputs_launch_no_backward(monkeypatch):
    from hipie_amd import ops
    from hipie_amd.training import functions
    calls = []
    for name in ("point_mask_loss_backward", "token_focal_backward"):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: calls.append(n) or f(*a, **k))(getattr(ops, name), name))
    src, tgt, idx, pts, gm, gd = (t.to(DEV) for t in point_case(2, 16, 16, 16, 16, 65))
    pts.requires_grad_(True)                                     # the node exists, src is frozen
    lmask, ldice = functions.point_mask_loss(src, tgt, idx, pts, 0, -1.0)
    (lmask.sum() + ldice.sum()).backward()
    assert calls == [] and src.grad is None and pts.grad is None
    logits, onehot, mask = (t.to(DEV) for t in token_case(2, 3, 5, "some"))
    onehot.requires_grad_(True)
    functions.token_focal_sum(logits, onehot, mask, 0.25).backward()
    assert calls == [] and logits.grad is None and onehot.grad is None
    src.requires_grad_(True)
    logits.requires_grad_(True)
    lmask, ldice = functions.point_mask_loss(src, tgt, idx, pts, 0, -1.0)
    (lmask.sum() + ldice.sum() + functions.token_focal_sum(logits, onehot, mask, 0.25)).backward()
    assert sorted(calls) == ["point_mask_loss_backward", "token_focal_backward"] and src.grad is not None and logits.grad is not None


def test_token_focal_function_matches_the_criterion_formula():
    from hipie_amd.training import functions
    logits, onehot, mask = token_case(2, 40, 19, "some")
    ref, lib = token_reference(logits, onehot, mask, 0.25, torch.float64), token_reference(logits, onehot, mask, 0.25, torch.float32)
    x = logits.to(DEV).requires_grad_(True)
    loss = functions.token_focal_sum(x, onehot.to(DEV), mask.to(DEV), 0.25)
    (loss * 3.0).backward()
    check("TokenFocalFunction", ("loss", "dlogits"), (loss, x.grad / 3.0), ref, lib)


# ------------------------------------------------------------------------------------------------ the step
def _spy_on_the_criteria(monkeypatch, step):
    """counts, per loss_masks / loss_labels call of the two criteria that has matched instances, how often the Function under it was applied"""
    from hipie_amd.training import functions
    applied = {"point": 0, "token": 0}
    seen = {"point": [], "token": []}
    for kind, name in (("point", "point_mask_loss"), ("token", "token_focal_sum")):
        def counted(*a, _f=getattr(functions, name), _k=kind, **k):
            applied[_k] += 1
            return _f(*a, **k)
        monkeypatch.setattr(functions, name, counted)
    for crit in (step.criterion, step.md_criterion):
        for kind, name in (("point", "loss_masks"), ("token", "loss_labels")):
            def wrapped(out, targets, indices, count, _f=getattr(crit, name), _k=kind):
                before = applied[_k]
                res = _f(out, targets, indices, count)
                if sum(len(p[0]) for p in indices) > 0:
                    seen[_k].append(applied[_k] - before)
                return res
            monkeypatch.setattr(crit, name, wrapped)
    return seen


def test_train_step_with_the_loss_kernels_matches_the_reference(monkeypatch):
    """test_training.test_train_step_losses_and_gradients_match_the_reference with backend=net.HipBackendLosses: the same fixture, the same
    assertions and bounds (loss entries 2e-3, the three gradient classes 5e-3 / 5e-3 / 8e-2, the same random draws)."""
    from hipie_amd.training import net
    z, meta, model, step, batch, targets = train_step_case("cuda", net.HipBackendLosses)
    assert step.criterion.ops is net.HipBackendLosses and step.md_criterion.ops is net.HipBackendLosses
    seen = _spy_on_the_criteria(monkeypatch, step)
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    print("LOSS step: %d mask-loss calls and %d label-loss calls with matched instances" % (len(seen["point"]), len(seen["token"])))
    assert len(seen["point"]) >= 4 and len(seen["token"]) >= 4 and set(seen["point"]) == {1} and set(seen["token"]) == {1}
    check_step_against_golden(z, model, step, losses, total, "cuda", "LOSS step")
