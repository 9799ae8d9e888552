"""GPU: hipie_group_norm_train_forward / hipie_group_norm_backward (csrc/groupnorm.hip, groupnorm_bwd.hip) through ops.group_norm_train_forward
/ ops.group_norm_backward, the autograd Function over them and the opt-in HipBackendGroupNorms wiring of the training step.

Reference: the float64 formulas of tests/_group_norm_cases.py (checked against torch.autograd in test_group_norm_bwd_cpu.py); with ReLU its
mask is the kernel forward's own y > 0.  Metric: max|got - ref64| / max|ref64| per output tensor.  Bound per case: max(1e-6, 4 x e_lib),
e_lib = the same metric for PyTorch's own fp32 op on the CPU -- torch.native_group_norm for the statistics, autograd through F.group_norm
(+ F.relu) for the gradients.  Every case prints its figures (lines starting with GNB) before it asserts."""
import pytest
import torch
import torch.nn.functional as F

from _group_norm_cases import EPS, backward64, inputs, pre_activation64, torch_graph
from _train_step_cases import check_step_against_golden, train_step_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _err(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _check(tag, names, got, ref64, lib32):
    fails = []
    for n, g, r, l in zip(names, got, ref64, lib32):
        if g is None:
            continue
        e, e_lib = _err(g, r), _err(l, r)
        bound = max(1e-6, 4 * e_lib)
        print("GNB %-40s %-7s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


def _chunks(B, C, HW):
    from hipie_amd import _lib
    return _lib.load().hipie_group_norm_backward_ws_bytes(B, C, HW) // (B * 2 * C * 4)


def _stat_refs(x, gamma, beta, groups):
    """(mean, rstd) stacked as the kernel's (B, groups, 2): float64, and torch.native_group_norm in fp32 on the CPU"""
    B, C = x.shape[:2]
    _, _, mean, rstd = pre_activation64(x, gamma, beta, groups)
    _, m32, r32 = torch.native_group_norm(x, gamma, beta, B, C, x[0, 0].numel(), groups, EPS)
    return (mean, rstd), (m32, r32)


def _operator_case(tag, B, groups, HW, offset=0.0, seed=0):
    from hipie_amd import ops
    x, dy, gamma, beta = inputs(B, groups, HW, seed, offset)
    xd, dyd, gd, bd = (t.to(DEV) for t in (x, dy, gamma, beta))
    ref_stat, lib_stat = _stat_refs(x, gamma, beta, groups)
    for relu in (False, True):
        y, stat = ops.group_norm_train_forward(xd, groups, gd, bd, EPS, relu)
        assert torch.equal(y, ops.group_norm(xd, groups, gd, bd, EPS, relu=relu))             # the inference entry's bits
        assert stat.shape == (B, groups, 2) and stat.dtype == torch.float32
        _check("%s relu=%d" % (tag, relu), ("mean", "rstd"), (stat[..., 0], stat[..., 1]), ref_stat, lib_stat)
        mask = (y > 0).cpu() if relu else None
        ref = backward64(x, dy, gamma, beta, groups, EPS, mask)
        lib = torch_graph(x, dy, gamma, beta, groups, EPS, relu, torch.float32)[1:]
        for want_dx, want_p in ((True, True), (True, False), (False, True)):
            got = ops.group_norm_backward(xd, dyd, stat, groups, gd, bd, relu, want_dx=want_dx, want_param_grads=want_p)
            assert (got[0] is None) == (not want_dx) and (got[1] is None) == (got[2] is None) == (not want_p)
            _check("%s relu=%d dx=%d par=%d" % (tag, relu, want_dx, want_p), ("dx", "dgamma", "dbeta"), got, ref, lib)


# HW: 8 one vector per channel; 16 the real 4 x 4 level; 264 a channel shorter than one workgroup sweep (2048 values); 8 * 257 a second sweep
# with idle tail threads
@pytest.mark.parametrize("HW", [8, 16, 264, 8 * 257])
@pytest.mark.parametrize("B,groups", [(1, 1), (2, 32), (3, 64), (3, 1), (1, 64)])
def test_operator_against_float64(B, groups, HW):
    assert _chunks(B, 8 * groups, HW) == 1
    _operator_case("(%d,%d,%d)" % (B, 8 * groups, HW), B, groups, HW)


def test_operator_with_a_ragged_last_chunk():
    """24584 values per channel: 3 chunks of 8200, 8200 and 8184"""
    assert _chunks(1, 8, 24584) == 3 and _chunks(1, 8, 16376) == 1 and _chunks(1, 8, 16384) == 2
    _operator_case("(1,8,24584)", 1, 1, 24584)
    _operator_case("(2,16,16384)", 2, 2, 16384, seed=1)


@pytest.mark.parametrize("B,groups,HW", [(2, 32, 16), (3, 1, 8 * 257), (1, 1, 24584)])
def test_operator_with_a_large_mean(B, groups, HW):
    _operator_case("mean 40 (%d,%d,%d)" % (B, 8 * groups, HW), B, groups, HW, offset=40.0, seed=2)


# --------------------------------------------------------------------------------------------- the recomputed mask
@pytest.mark.parametrize("B,groups,HW", [(3, 32, 264), (2, 1, 24584), (2, 64, 8)])
def test_recomputed_mask_is_the_forwards(B, groups, HW):
    """dy = 1 and x on a grid of 1/4, every channel mirrored about 1/2 so that each group's mean IS 1/2 and one value in 13 sits on it; every
    second beta is 0, a few gammas too.  There the pre-activation is 0 in exact arithmetic and the forward's fmaf(x, sc, sh) is the rounding
    residue of mean * sc: either sign.  dbeta[c] must be the NUMBER of positive outputs of channel c -- an integer below 2^24, exact in any
    order of the additions -- whatever the forward rounded to"""
    from hipie_amd import ops
    C = 8 * groups
    g = torch.Generator().manual_seed(5 + HW)
    half = torch.randint(-6, 7, (B, C, HW // 8, 4), generator=g).float() / 4
    x = torch.cat((half, 1.0 - half.flip(2)), 2).to(DEV)
    gamma = torch.randint(-4, 5, (C,), generator=g).float() / 2 + 0.125 * torch.randint(0, 2, (C,), generator=g).float()
    beta = torch.randint(-4, 5, (C,), generator=g).float() / 4
    beta[::2] = 0
    gamma, beta = gamma.to(DEV), beta.to(DEV)
    y, stat = ops.group_norm_train_forward(x, groups, gamma, beta, EPS, True)
    assert torch.equal(y, ops.group_norm(x, groups, gamma, beta, EPS, relu=True))
    count = (y > 0).sum((0, 2, 3))
    near = int((pre_activation64(x.cpu(), gamma.cpu(), beta.cpu(), groups)[0].abs() < 1e-6).sum())
    dx, dg, db = ops.group_norm_backward(x, torch.ones_like(x), stat, groups, gamma, beta, True)
    print("GNB mask identity (%d,%d,%d): %d positive outputs, %d pre-activations within 1e-6 of zero, dbeta - count: max %g"
          % (B, C, HW, int(count.sum()), near, float((db - count.float()).abs().max())))
    assert int(count.max()) < 2 ** 24 and 0 < int(count.sum()) < x.numel() and near > 0
    assert torch.equal(db, count.float())


# --------------------------------------------------------------------------------------------- the autograd Function
def _function_run(x, dy, gamma, beta, groups, relu, grad_x=True, grad_p=True):
    from hipie_amd.training import functions
    xd = x.to(DEV).requires_grad_(grad_x)
    gd, bd = gamma.to(DEV).requires_grad_(grad_p), beta.to(DEV).requires_grad_(grad_p)
    y = functions.group_norm(xd, groups, gd, bd, EPS, relu)
    assert y is not None and y.requires_grad == (grad_x or grad_p)
    return xd, gd, bd, y


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_function_forward_backward_and_frozen_inputs(relu, monkeypatch):
    from hipie_amd import ops
    from hipie_amd.training import functions
    B, groups, HW = 2, 32, 264
    x, dy, gamma, beta = inputs(B, groups, HW, seed=3)
    seen = []
    real = ops.group_norm_backward

    def spy(*a, **k):
        seen.append((k["want_dx"], k["want_param_grads"]))
        return real(*a, **k)
    monkeypatch.setattr(functions.ops, "group_norm_backward", spy)
    xd, gd, bd, y = _function_run(x, dy, gamma, beta, groups, relu)
    assert torch.equal(y, ops.group_norm(xd.detach(), groups, gd.detach(), bd.detach(), EPS, relu=relu))
    saved = y.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [tuple(x.shape), (B, groups, 2), (8 * groups,), (8 * groups,)]     # x is the only map kept
    mask = (y > 0).cpu() if relu else None
    ref = backward64(x, dy, gamma, beta, groups, EPS, mask)
    lib = torch_graph(x, dy, gamma, beta, groups, EPS, relu, torch.float32)[1:]
    y.backward(dy.to(DEV))
    _check("Function relu=%d" % relu, ("dx", "dgamma", "dbeta"), (xd.grad, gd.grad, bd.grad), ref, lib)
    full = (xd.grad, gd.grad, bd.grad)
    # frozen input, frozen parameters: the same bits from fewer launches; both frozen: no node at all
    xd, gd, bd, y = _function_run(x, dy, gamma, beta, groups, relu, grad_x=False)
    y.backward(dy.to(DEV))
    assert xd.grad is None and torch.equal(gd.grad, full[1]) and torch.equal(bd.grad, full[2])
    xd, gd, bd, y = _function_run(x, dy, gamma, beta, groups, relu, grad_p=False)
    y.backward(dy.to(DEV))
    assert gd.grad is None and bd.grad is None and torch.equal(xd.grad, full[0])
    assert seen == [(True, True), (False, True), (True, False)]
    xd, gd, bd, y = _function_run(x, dy, gamma, beta, groups, relu, grad_x=False, grad_p=False)
    assert y.grad_fn is None
    # a frozen weight beside a trainable bias still needs the sums
    xd = x.to(DEV).requires_grad_(True)
    bt = beta.to(DEV).requires_grad_(True)
    functions.group_norm(xd, groups, gamma.to(DEV), bt, EPS, relu).backward(dy.to(DEV))
    assert seen[-1] == (True, True) and torch.equal(bt.grad, full[2]) and torch.equal(xd.grad, full[0])


def test_function_takes_a_strided_output_gradient_and_repeats_its_bits():
    B, groups, HW = 3, 1, 8 * 257
    x, dy, gamma, beta = inputs(B, groups, HW, seed=4)
    wide = torch.randn(B, 8, HW // 4, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    view = wide[..., ::2]
    assert not view.is_contiguous() and view.shape == x.shape
    runs = []
    for g in (view, view.contiguous(), view):
        xd, gd, bd, y = _function_run(x, dy, gamma, beta, groups, True)
        torch.randn(1 << 18, device=DEV).sum()                  # other work in between
        y.backward(g)
        runs.append((y.detach(), xd.grad, gd.grad, bd.grad))
    assert all(torch.equal(a, b) for r in runs[1:] for a, b in zip(runs[0], r))
    mask = (runs[0][0] > 0).cpu()
    _check("strided dy", ("dx", "dgamma", "dbeta"), runs[0][1:], backward64(x, view.cpu(), gamma, beta, groups, EPS, mask),
           torch_graph(x, view.cpu(), gamma, beta, groups, EPS, True, torch.float32)[1:])


def test_function_declines_what_the_kernels_do_not_take():
    from hipie_amd.training import functions
    w, b = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    x = torch.randn(2, 256, 4, 17, device=DEV)                                                  # H*W = 68
    assert functions.group_norm(x, 32, w, b, EPS, False) is None
    x = torch.randn(2, 256, 8, 8, device=DEV)
    assert functions.group_norm(x.half(), 32, w, b, EPS, False) is None
    assert functions.group_norm(x.to(memory_format=torch.channels_last), 32, w, b, EPS, True) is None
    assert functions.group_norm(x, 16, w, b, EPS, True) is None and functions.group_norm(x.cpu(), 32, w.cpu(), b.cpu(), EPS, True) is None
    assert functions.group_norm(x, 32, w, b, EPS, True) is not None


# --------------------------------------------------------------------------------------------- what the entry points write
def test_outputs_stay_inside_their_buffers():
    """guard bands around y, stat, dx, dgamma, dbeta and behind the workspace's ws_bytes keep their fill"""
    from hipie_amd import _lib
    lib = _lib.load()
    GUARD, FILL = 64, 12345.0
    for B, groups, HW in ((3, 1, 264), (1, 1, 24584), (2, 64, 8)):
        C = 8 * groups
        x, dy, gamma, beta = (t.to(DEV) for t in inputs(B, groups, HW, seed=6))
        nbytes = lib.hipie_group_norm_backward_ws_bytes(B, C, HW)
        sizes = dict(y=x.numel(), stat=B * groups * 2, dx=x.numel(), dgamma=C, dbeta=C, ws=nbytes // 4)
        bufs = {n: torch.full((k + 2 * GUARD,), FILL, device=DEV) for n, k in sizes.items()}
        ptr = {n: t[GUARD:].data_ptr() for n, t in bufs.items()}
        st = torch.cuda.current_stream().cuda_stream
        rc = lib.hipie_group_norm_train_forward(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ptr["y"], ptr["stat"], ptr["ws"], B, C, HW, groups, EPS, 1, st)
        assert rc == 0, lib.hipie_last_error()
        rc = lib.hipie_group_norm_backward(x.data_ptr(), dy.data_ptr(), ptr["stat"], gamma.data_ptr(), beta.data_ptr(), ptr["dx"], ptr["dgamma"],
                                           ptr["dbeta"], ptr["ws"], nbytes, B, C, HW, groups, 1, st)
        assert rc == 0, lib.hipie_last_error()
        torch.cuda.synchronize()
        for n, t in bufs.items():
            inner = t[GUARD:GUARD + sizes[n]]
            assert bool((t[:GUARD] == FILL).all()) and bool((t[GUARD + sizes[n]:] == FILL).all()), n
            assert n == "ws" or not bool((inner == FILL).any()), n
        from hipie_amd import ops
        y, stat = ops.group_norm_train_forward(x, groups, gamma, beta, EPS, True)
        got = ops.group_norm_backward(x, dy, stat, groups, gamma, beta, True)
        mine = [bufs[n][GUARD:GUARD + sizes[n]] for n in ("y", "stat", "dx", "dgamma", "dbeta")]
        assert all(torch.equal(a.reshape(-1), b) for a, b in zip((y, stat) + tuple(got), mine))


# --------------------------------------------------------------------------------------------- one training step
STEP_GROUPS = [("group_norms",), ("norms", "mlp", "packed_windows", "deformable", "pair_losses", "group_norms")]


@pytest.mark.parametrize("names", STEP_GROUPS, ids=["alone", "every-group"])
def test_train_step_with_group_norm_nodes_matches_the_reference(names, monkeypatch):
    from hipie_amd.training import functions, net
    be = net.backend(*names)
    assert be.__mro__[0] is be and net.HipBackendGroupNorms in be.__mro__
    ran, declined, copied = [], [], []
    real, real_op = functions.group_norm, net.HipBackendGroupNorms.group_norm

    def spy(x, *a):
        y = real(x, *a)
        (declined if y is None else ran).append(tuple(x.shape))
        return y

    def spy_op(x, *a):                                                           # the backend's op: which maps it has to copy to NCHW
        if not x.is_contiguous():
            copied.append((tuple(x.shape), tuple(x.stride())))
        return real_op(x, *a)
    monkeypatch.setattr(functions, "group_norm", spy)
    monkeypatch.setattr(net.HipBackendGroupNorms, "group_norm", staticmethod(spy_op))
    z, meta, model, step, batch, targets = train_step_case("cuda", be)
    assert step.be is be
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    print("GNB step %s: node ran on %s, declined %s, copied to NCHW first %s" % ("+".join(names), ran, declined, copied))
    assert not declined and len(ran) == 11                                     # levels 32^2 ... 4^2 twice, 32^2, 32^2, 64^2: none falls back
    check_step_against_golden(z, model, step, losses, total, "cuda", "GROUP NORMS step (%s)" % "+".join(names))
