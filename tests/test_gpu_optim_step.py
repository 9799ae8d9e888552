"""GPU: the optimizer-step kernels (csrc/optim_step.hip) through ops and training/optim.py's HipAdamW.

Accuracy is measured against a float64 restatement of the kernel's contract on the SAME fp32 inputs (tests/_optim_cases.py run_f64).  The
yardstick is torch's own fp32 path -- clip_grad_norm_(foreach=False) + torch.optim.AdamW(foreach=False) on the CPU, from the same inputs -- and
ITS distance to that truth, per quantity and as the worst over the three steps and all tensors: the norm as a relative error, p, exp_avg and
exp_avg_sq as max |error| / max |value| per tensor.  The kernels may be at most 4 x as far: they perform torch's operations in torch's order, but
take the bias corrections from float64 through one more fp32 rounding (lr / bc1 is a float division where torch divides doubles), multiply by the
clip coefficient and the gradient scale separately, and divide and take roots with the device's own sequences -- a few ulp over about six
operations.  The yardsticks are the constants below (they do not depend on the kernels' output).

Sizes (tests/_optim_cases.py SHAPES, C = the chunk of 16384 elements): 1, 3, 255, 256, 257, C - 1, C, C + 1, 2 C + 5, a (33, 129) matrix, and a
parameter that never has a gradient; two groups with lr 1e-2 and 1e-3, weight decay 0.1, so that a wrong update is far above the rounding of p;
gradient norms of about 290, 0.29 and 88 against max_norm = 1: both sides of the clamp; three steps, for the exponents of the bias corrections."""
import pytest
import torch

import _optim_cases as oc

pytestmark = pytest.mark.gpu

# python tests/_optim_cases.py   (torch 2.10, CPU):
# YARDSTICK = {'norm': 2.572096874608537e-07, 'p': 1.7232218750211855e-07, 'exp_avg': 2.0056357236097196e-07, 'exp_avg_sq': 3.714520017845798e-07}
YARDSTICK = {"norm": 2.572096874608537e-07, "p": 1.7232218750211855e-07, "exp_avg": 2.0056357236097196e-07, "exp_avg_sq": 3.714520017845798e-07}
FACTOR = 4.0
DEV = "cuda:0"
_SHARED = {}


def shared():
    """the inputs and the two references, computed once and never written"""
    if not _SHARED:
        params, grads = oc.make_case()
        _SHARED.update(params=params, grads=grads, truth=oc.run_f64(params, grads), torch=oc.run_torch(params, grads))
    return _SHARED


def hip_optimizer(params):
    from hipie_amd.training import HipAdamW
    ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
    return ps, HipAdamW(oc.groups_of(ps), betas=oc.BETAS, eps=oc.EPS)


def snapshot(ps, opt, norm):
    # a never-stepped parameter reads None, as in run_torch / run_f64
    st = [opt.state[p] for p in ps]
    has = [i != oc.NO_GRAD for i in range(len(ps))]
    return (None if norm is None else norm.cpu().clone(), [p.detach().cpu().clone() for p in ps],
            [s["exp_avg"].cpu().clone() if h else None for s, h in zip(st, has)], [s["exp_avg_sq"].cpu().clone() if h else None for s, h in zip(st, has)])


def run_hip(params, grads, max_norm=oc.MAX_NORM, as_views=False, lr_at=None, write_grads=False, keep=None):
    """HipAdamW over the case on the device -> per step (norm, [p], [exp_avg], [exp_avg_sq]) on the CPU, as oc.run_torch"""
    ps, opt = hip_optimizer(params)
    out = []
    for k, gs in enumerate(grads):
        for gi, lr in enumerate((lr_at or {}).get(k, ())):
            opt.param_groups[gi]["lr"] = lr
        gd = oc.views_at(gs, device=DEV) if as_views else [g.clone().to(DEV) for g in gs]
        for i, (p, g) in enumerate(zip(ps, gd)):
            p.grad = None if i == oc.NO_GRAD else g
        norm = opt.clip_and_step(max_norm, write_grads=write_grads)
        out.append(snapshot(ps, opt, norm))
    if keep is not None:
        keep.update(ps=ps, opt=opt)
    return out


def check(errs, what):
    print("%s: " % what + "  ".join("%s %.3e (yardstick %.3e)" % (k, errs[k], YARDSTICK[k]) for k in sorted(errs)))
    for k, e in errs.items():
        assert e <= FACTOR * YARDSTICK[k], (what, k, e, YARDSTICK[k])


def test_both_sides_of_the_clamp():
    s = shared()
    norms = [float(n) for n, _, _, _ in s["truth"]]
    assert norms[0] > oc.MAX_NORM and norms[1] < oc.MAX_NORM and norms[2] > oc.MAX_NORM
    print("torch's fp32 path against float64 here: %r" % (oc.errors(s["torch"], s["truth"]),))


def test_accuracy_against_float64():
    from hipie_amd import ops
    assert ops.optim_chunk() == oc.CHUNK
    s = shared()
    check(oc.errors(run_hip(s["params"], s["grads"]), s["truth"]), "separate gradients")


def test_misaligned_bucket_views():
    """every gradient a view into one flat buffer at element offsets 1, 2, 3 modulo 4: the same bound, and the same BITS as with aligned gradients
    (which element a thread owns does not depend on the address)"""
    s = shared()
    views = run_hip(s["params"], s["grads"], as_views=True)
    check(oc.errors(views, s["truth"]), "bucket views")
    plain = run_hip(s["params"], s["grads"])
    for (n0, p0, m0, v0), (n1, p1, m1, v1) in zip(plain, views):
        assert torch.equal(n0, n1)
        for a, b in zip(p0 + m0 + v0, p1 + m1 + v1):
            assert (a is None and b is None) or torch.equal(a, b)


def test_misaligned_parameters_and_moments():
    """the entries themselves take p, m and v at any 4-byte aligned address too: one step over hand-built tables, all four tensors of every
    segment at odd offsets, gives the bits of the aligned run"""
    from hipie_amd import ops
    s = shared()
    params, grads = s["params"][:-1], s["grads"][0][:-1]
    res = []
    for odd in (False, True):
        place = (lambda ts, r: oc.views_at(ts, r, device=DEV)) if odd else (lambda ts, r: [t.clone().to(DEV) for t in ts])
        ps, gs = place(params, (1, 2, 3)), place(grads, (3, 1, 2))
        ms, vs = place([torch.zeros_like(p) for p in params], (2, 3, 1)), place([torch.zeros_like(p) for p in params], (1, 3, 2))
        if odd:
            assert all(t.data_ptr() % 16 for t in ps + gs + ms + vs)
        table, cmap = oc.tables(ps, gs, ms, vs, oc.GROUP_OF[:-1])
        steps, bc = torch.zeros(len(ps), dtype=torch.int32, device=DEV), torch.ones(len(ps), 2, device=DEV)
        norm = ops.optim_grad_norm(table, cmap)
        ops.optim_adamw_step(table, cmap, steps, bc, oc.LRS, (oc.WD, oc.WD), oc.BETAS, oc.EPS, norm=norm, max_norm=oc.MAX_NORM)
        assert steps.tolist() == [1] * len(ps)
        res.append([norm.cpu()] + [t.cpu().clone() for t in ps + ms + vs])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    want = s["truth"][0]
    n = len(params)
    check({"norm": abs(float(res[1][0]) - float(want[0])) / float(want[0]),
           "p": max(oc.tensor_err(a, b) for a, b in zip(res[1][1:1 + n], want[1])),
           "exp_avg": max(oc.tensor_err(a, b) for a, b in zip(res[1][1 + n:1 + 2 * n], want[2])),
           "exp_avg_sq": max(oc.tensor_err(a, b) for a, b in zip(res[1][1 + 2 * n:], want[3]))}, "odd addresses")


def test_grid_stride():
    """one tensor with one chunk more than the grid cap of 2048 workgroups (and a ragged tail): one clipped step against float64 on the device"""
    from hipie_amd.training import HipAdamW
    n = 2048 * oc.CHUNK + 5
    gen = torch.Generator(device=DEV).manual_seed(7)
    p0 = torch.randn(n, device=DEV, generator=gen)
    g0 = torch.randn(n, device=DEV, generator=gen) * 1e-3
    p = torch.nn.Parameter(p0.clone())
    opt = HipAdamW([p], lr=1e-2, betas=oc.BETAS, eps=oc.EPS, weight_decay=oc.WD)
    p.grad = g0.clone()
    norm = opt.clip_and_step(oc.MAX_NORM)
    g = g0.double()
    tn = g.square().sum().sqrt()
    g = g * torch.clamp(oc.MAX_NORM / (tn + 1e-6), max=1.0)
    assert float(tn) > oc.MAX_NORM
    b1, b2 = oc.BETAS
    m, v = (1 - b1) * g, (1 - b2) * g * g
    tp = p0.double() * (1 - 1e-2 * oc.WD) - (1e-2 / (1 - b1)) * m / (v.sqrt() / (1 - b2) ** 0.5 + oc.EPS)
    st = opt.state[p]
    check({"norm": abs(float(norm) - float(tn)) / float(tn), "p": oc.tensor_err(p.detach(), tp), "exp_avg": oc.tensor_err(st["exp_avg"], m),
           "exp_avg_sq": oc.tensor_err(st["exp_avg_sq"], v)}, "2049 chunks")
    # the last chunk is the ragged one: its five elements moved
    assert not torch.equal(p.detach()[-5:], p0[-5:]) and not torch.equal(p.detach()[:4], p0[:4])


def test_determinism():
    s = shared()
    a, b = run_hip(s["params"], s["grads"]), run_hip(s["params"], s["grads"])
    for (n0, p0, m0, v0), (n1, p1, m1, v1) in zip(a, b):
        assert torch.equal(n0, n1)
        for x, y in zip(p0 + m0 + v0, p1 + m1 + v1):
            assert (x is None and y is None) or torch.equal(x, y)


def test_skipped_parameter():
    s = shared()
    keep = {}
    run_hip(s["params"], s["grads"], keep=keep)
    ps, opt = keep["ps"], keep["opt"]
    i = oc.NO_GRAD
    assert torch.equal(ps[i].detach().cpu(), s["params"][i])                              # not even the weight decay
    assert not opt.state[ps[i]]["exp_avg"].any() and not opt.state[ps[i]]["exp_avg_sq"].any()
    by_id = dict(zip([id(p) for g in opt.param_groups for p in g["params"]], opt.steps()))
    assert [by_id[id(p)] for p in ps] == [0 if j == i else oc.STEPS for j in range(len(ps))]
    sd = opt.state_dict()["state"]                                # ids count group by group: group 0 holds parameters 0, 2, .., 10
    assert len(sd) == len(ps) - 1 and i // 2 not in sd


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient(bad):
    """inf: the norm is inf and the coefficient 0, so that element becomes NaN and the rest take a zero gradient; NaN: the coefficient is NaN
    and stays one through the clamp (fminf would return 1 and un-clip), everything becomes NaN.  The pattern equals torch's in both cases."""
    s = shared()
    grads = [[g.clone() for g in s["grads"][0]]]
    grads[0][5][17] = bad
    want = oc.run_torch(s["params"], grads)[0]
    got = run_hip(s["params"], grads)[0]
    assert torch.equal(got[0].isnan(), want[0].isnan()) and torch.equal(got[0].isinf(), want[0].isinf())
    for key in (1, 2, 3):
        for a, b in zip(got[key], want[key]):
            if b is not None:
                assert torch.equal(a.isfinite(), b.isfinite()) and torch.equal(a.isnan(), b.isnan())
    if bad == bad:
        assert got[0].isinf() and got[1][5][17].isnan() and got[1][5][16].isfinite() and got[1][0].isfinite().all()
    else:
        assert got[0].isnan() and all(p.isnan().all() for i, p in enumerate(got[1]) if i != oc.NO_GRAD) and got[1][oc.NO_GRAD].isfinite().all()


def test_write_grads():
    s = shared()
    keep = {}
    run_hip(s["params"], s["grads"][:1], write_grads=True, keep=keep)
    tn = s["truth"][0][0]
    c = torch.clamp(oc.MAX_NORM / (tn + 1e-6), max=1.0)
    worst = 0.0
    for i, (p, g) in enumerate(zip(keep["ps"], s["grads"][0])):
        if i != oc.NO_GRAD:
            worst = max(worst, oc.tensor_err(p.grad.cpu(), g.double() * c))
    print("clipped gradients written back: %.3e (yardstick %.3e)" % (worst, YARDSTICK["exp_avg"]))
    assert worst <= FACTOR * YARDSTICK["exp_avg"]                 # exp_avg after one step is 0.1 x the clipped gradient: the same roundings
    keep2 = {}
    run_hip(s["params"], s["grads"][:1], keep=keep2)
    for i, (p, g) in enumerate(zip(keep2["ps"], s["grads"][0])):
        if i != oc.NO_GRAD:
            assert torch.equal(p.grad.cpu(), g)                  # the default leaves them alone


def test_learning_rate_change_needs_no_upload():
    s = shared()
    lr_at = {1: (5e-3, 2e-3), 2: (1e-4, 3e-2)}
    params, grads = s["params"], s["grads"]
    ps, opt = hip_optimizer(params)
    gd = oc.views_at(grads[0], device=DEV)                       # stable addresses, as with GradientBuckets
    out = []
    for k in range(oc.STEPS):
        for gi, lr in enumerate(lr_at.get(k, ())):
            opt.param_groups[gi]["lr"] = lr
        for i, (p, g, src) in enumerate(zip(ps, gd, grads[k])):
            g.copy_(src)
            p.grad = None if i == oc.NO_GRAD else g
        out.append(snapshot(ps, opt, opt.clip_and_step(oc.MAX_NORM)))
    assert opt.table_uploads == 1
    check(oc.errors(out, oc.run_f64(params, grads, lr_at=lr_at)), "lr changed between steps")
    unchanged = oc.errors(out, s["truth"])
    assert unchanged["p"] > 100 * YARDSTICK["p"]                  # and the change is far above the bound: it did take effect


def test_against_torch_fused():
    """HipAdamW and torch.optim.AdamW(fused=True) + clip_grad_norm_, both on the device: each within its bound of the truth (ours: 4 x the
    yardstick), hence within the sum of the two of each other"""
    s = shared()
    ours = run_hip(s["params"], s["grads"])
    fused = oc.run_torch(s["params"], s["grads"], device=DEV, fused=True)
    e_ours, e_fused = oc.errors(ours, s["truth"]), oc.errors(fused, s["truth"])
    check(e_ours, "ours")
    print("torch fused: " + "  ".join("%s %.3e" % kv for kv in sorted(e_fused.items())))
    both = oc.errors(ours, [(n, p, m, v) for n, p, m, v in fused])
    for k in both:
        assert both[k] <= FACTOR * YARDSTICK[k] + 1.01 * e_fused[k], (k, both[k], e_fused[k])
