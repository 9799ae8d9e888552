"""GPU: the training 3 x 3 convolution (+ ReLU) node -- hipie_conv3x3_split forward and input gradient, hipie_conv3x3_wgrad
(csrc/conv_wgrad.hip) for the weight and bias gradient -- through the ops wrappers, functions.Conv3x3Function and the opt-in HipBackendConvs
wiring of the training step.

Reference: the float64 padded-grid algebra of tests/_conv_train_cases.py (checked against torch.autograd in test_conv_train_cpu.py); with
ReLU its mask is the kernel forward's own y > 0.  Metric: max|got - ref64| / max|ref64| per tensor.  Bound per case: max(3e-6, 4 x e_lib);
3e-6 is what test_conv3x3_split_matches_fp64 (tests/test_gpu_gemm.py) gives the forward kernel, e_lib the same metric for the library's
fp32 F.conv2d (+ F.relu) autograd on the device on the same inputs in the same run, 4 the margin of the GroupNorm tests.  Every case prints
its figures (lines starting with CVT) before it asserts.  The shapes and what each reaches: _conv_train_cases.SHAPES; the last one,
(1, 32, 32, 64, 64), has 4356 grid rows = chunks of 2048, 2048 and 260 rows of the weight-gradient kernel."""
import pytest
import torch

from _conv_train_cases import CHUNK, IDS, SHAPES, backward64, inputs, pre_activation64, separated_case, torch_graph
from _train_step_cases import check_step_against_golden, train_step_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 3e-6


def _err(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _check(tag, names, got, ref64, lib32):
    fails = []
    for n, g, r, l in zip(names, got, ref64, lib32):
        if g is None:
            continue
        e, e_lib = _err(g, r), _err(l, r)
        bound = max(FLOOR, 4 * e_lib)
        print("CVT %-34s %-3s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


def _operator(x, dy, w, b, relu):
    """the three passes through the ops wrappers, as Conv3x3Function composes them with a trainable input -> (y, dx, dW, db); and the
    weight pass again with the mask applied inside the kernel (the frozen-input form): the same bits"""
    from hipie_amd import ops
    B, C, H, W = x.shape
    N = w.shape[0]
    xd, dyd, wd, bd = (t.to(DEV) for t in (x, dy, w, b))
    xg = ops.conv3x3_stage(xd)
    yg = ops.conv3x3_grid(xg, ops.hl8_pack(wd.permute(0, 2, 3, 1).reshape(N, 9 * C)), bd, B, H, W, relu)
    g = ops.conv3x3_stage(dyd)
    in_kernel = ops.conv3x3_wgrad(xg, g, yg if relu else None, B, H, W)
    if relu:
        g[W + 3:W + 3 + yg.shape[0]].masked_fill_(~(yg > 0), 0.0)
    dx = ops.conv3x3_crop(ops.conv3x3_grid(g, ops.hl8_pack(wd.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9 * N)), None, B, H, W), B, H, W)
    dw, db = ops.conv3x3_wgrad(xg, g, None, B, H, W)
    assert torch.equal(dw, in_kernel[0]) and torch.equal(db, in_kernel[1])
    dw_only, none = ops.conv3x3_wgrad(xg, g, None, B, H, W, want_bias=False)
    assert none is None and torch.equal(dw_only, dw)
    return ops.conv3x3_crop(yg, B, H, W), dx, dw.view(N, 3, 3, C).permute(0, 3, 1, 2), db


# --------------------------------------------------------------------------------------------- the operators
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_operator_against_float64(shape, relu):
    x, dy, w, b = inputs(*shape)
    y, dx, dw, db = _operator(x, dy, w, b, relu)
    pre = pre_activation64(x, w, b)
    lib = torch_graph(x, dy, w, b, relu, torch.float32, DEV)
    mask = (y > 0).cpu() if relu else None
    ref = (pre.relu() if relu else pre,) + backward64(x, dy, w, mask)
    _check("%s relu=%d" % ("x".join(map(str, shape)), relu), ("y", "dx", "dW", "db"), (y, dx, dw, db), ref, lib)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mask_is_the_float64_sign_on_a_separated_input(shape):
    """pre-activations that all stay 1e-3 away from zero: the node's y > 0 is the float64 sign at EVERY element, and db of dy = 1 counts them"""
    from hipie_amd import ops
    x, dy, w, b = separated_case(*shape)
    pre = pre_activation64(x, w, b)
    assert float(pre.abs().min()) >= 1e-3
    y, dx, dw, db = _operator(x, torch.ones_like(dy), w, b, True)
    mask = (y > 0).cpu()
    print("CVT mask identity %s: %d of %d outputs positive, %d differ from the float64 sign" %
          ("x".join(map(str, shape)), int(mask.sum()), mask.numel(), int((mask != (pre > 0)).sum())))
    assert mask.shape == pre.shape and torch.equal(mask, pre > 0)
    assert torch.equal(db.cpu(), mask.sum((0, 2, 3)).float())                      # integers below 2^24: exact in any order


# --------------------------------------------------------------------------------------------- the autograd Function
def _function_run(x, w, b, relu, grad_x=True, grad_w=True, grad_b=True):
    from hipie_amd.training import functions
    xd = x.to(DEV).requires_grad_(grad_x)
    wd, bd = w.to(DEV).requires_grad_(grad_w), b.to(DEV).requires_grad_(grad_b)
    y = functions.conv3x3_train(xd, wd, bd, relu)
    assert y is not None and y.shape == (x.shape[0], w.shape[0]) + tuple(x.shape[2:]) and y.requires_grad == (grad_x or grad_w or grad_b)
    return xd, wd, bd, y


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_function_forward_backward_and_frozen_inputs(relu, monkeypatch):
    from hipie_amd import ops
    from hipie_amd.training import functions
    shape = SHAPES[2]
    x, dy, w, b = inputs(*shape, seed=3)
    calls = []
    real_grid, real_wgrad = ops.conv3x3_grid, ops.conv3x3_wgrad

    def spy_grid(*a, **k):
        calls.append("conv")
        return real_grid(*a, **k)

    def spy_wgrad(xg, g, yg, *a, **k):
        calls.append(("wgrad", yg is not None, k["want_bias"]))
        return real_wgrad(xg, g, yg, *a, **k)
    monkeypatch.setattr(functions.ops, "conv3x3_grid", spy_grid)
    monkeypatch.setattr(functions.ops, "conv3x3_wgrad", spy_wgrad)
    xd, wd, bd, y = _function_run(x, w, b, relu)
    saved = y.grad_fn.saved_tensors
    rows = shape[0] * (shape[3] + 2) * (shape[4] + 2)
    assert [tuple(t.shape) for t in saved] == [tuple(x.shape), tuple(w.shape)] + ([(rows, shape[2])] if relu else [])
    assert not relu or saved[2].data_ptr() <= y.data_ptr() < saved[2].data_ptr() + 4 * saved[2].numel()     # the output's own storage
    lib = torch_graph(x, dy, w, b, relu, torch.float32, DEV)
    pre = pre_activation64(x, w, b)
    mask = (y > 0).cpu() if relu else None
    ref = (pre.relu() if relu else pre,) + backward64(x, dy, w, mask)
    y.backward(dy.to(DEV))
    assert calls == ["conv", "conv", ("wgrad", False, True)]
    _check("Function relu=%d" % relu, ("y", "dx", "dW", "db"), (y, xd.grad, wd.grad, bd.grad), ref, lib)
    assert wd.grad.shape == w.shape and wd.grad.is_contiguous()
    full = (y.detach().clone(), xd.grad, wd.grad, bd.grad)
    # frozen input: no dx pass, the mask is applied inside the weight kernel; frozen weight and bias: no weight pass; the same bits
    del calls[:]
    xd, wd, bd, y = _function_run(x, w, b, relu, grad_x=False)
    y.backward(dy.to(DEV))
    assert calls == ["conv", ("wgrad", relu, True)]
    assert xd.grad is None and torch.equal(wd.grad, full[2]) and torch.equal(bd.grad, full[3])
    del calls[:]
    xd, wd, bd, y = _function_run(x, w, b, relu, grad_w=False, grad_b=False)
    y.backward(dy.to(DEV))
    assert calls == ["conv", "conv"]
    assert wd.grad is None and bd.grad is None and torch.equal(xd.grad, full[1]) and torch.equal(y, full[0])
    # a frozen weight beside a trainable bias still runs the weight pass, and returns no weight gradient
    del calls[:]
    xd, wd, bd, y = _function_run(x, w, b, relu, grad_w=False)
    y.backward(dy.to(DEV))
    assert calls == ["conv", "conv", ("wgrad", False, True)] and wd.grad is None and torch.equal(bd.grad, full[3])
    xd, wd, bd, y = _function_run(x, w, b, relu, grad_x=False, grad_w=False, grad_b=False)
    assert y.grad_fn is None
    # no bias
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    del calls[:]
    y = functions.conv3x3_train(xd, wd, None, relu)
    y.backward(dy.to(DEV))
    assert calls[-1] == ("wgrad", False, False)
    nb = torch_graph(x, dy, w, torch.zeros_like(b), relu, torch.float32, DEV)
    pre0 = pre_activation64(x, w, None)
    ref0 = (pre0.relu() if relu else pre0,) + backward64(x, dy, w, (y > 0).cpu() if relu else None)
    _check("Function no bias relu=%d" % relu, ("y", "dx", "dW"), (y, xd.grad, wd.grad), ref0, nb)


def test_function_takes_a_strided_output_gradient_and_repeats_its_bits():
    shape = SHAPES[3]
    B, Cin, Cout, H, W = shape
    x, dy, w, b = inputs(*shape, seed=4)
    wide = torch.randn(B, Cout, H, 2 * W, generator=torch.Generator().manual_seed(1)).to(DEV)
    view = wide[..., ::2]
    assert not view.is_contiguous() and view.shape == dy.shape
    runs = []
    for g in (view, view.contiguous(), view):
        xd, wd, bd, y = _function_run(x.contiguous(memory_format=torch.channels_last) if g is view else x, w, b, True)
        torch.randn(1 << 18, device=DEV).sum()                  # other work in between
        y.backward(g)
        runs.append((y.detach(), xd.grad, wd.grad, bd.grad))
    assert all(torch.equal(a, b_) for r in runs[1:] for a, b_ in zip(runs[0], r))
    mask = (runs[0][0] > 0).cpu()
    _check("strided dy", ("dx", "dW", "db"), runs[0][1:], backward64(x, view.cpu(), w, mask), torch_graph(x, view.cpu(), w, b, True, torch.float32, DEV)[1:])


def test_function_declines_what_the_kernels_do_not_take():
    from hipie_amd.training import functions
    x = torch.randn(2, 64, 6, 6, device=DEV)
    w, b = torch.randn(32, 64, 3, 3, device=DEV), torch.randn(32, device=DEV)
    assert functions.conv3x3_train(x, w, b, True) is not None
    assert functions.conv3x3_train(x, w, b, True, stride=2) is None and functions.conv3x3_train(x, w, b, True, padding=0) is None
    assert functions.conv3x3_train(x, torch.randn(32, 64, 1, 1, device=DEV), b, False) is None
    assert functions.conv3x3_train(x, torch.randn(32, 32, 3, 3, device=DEV), b, False, groups=2) is None
    assert functions.conv3x3_train(x, torch.randn(8, 64, 3, 3, device=DEV), torch.randn(8, device=DEV), True) is None        # lay2's shape
    assert functions.conv3x3_train(x.half(), w.half(), b.half(), True) is None
    assert functions.conv3x3_train(x.cpu(), w.cpu(), b.cpu(), True) is None


# --------------------------------------------------------------------------------------------- what the entry points write
def _raw_case(shape, seed=6):
    """device inputs on their grids and the raw-call geometry of a shape"""
    from hipie_amd import ops
    B, C, N, H, W = shape
    x, dy, w, b = (t.to(DEV) for t in inputs(*shape, seed=seed))
    xg, g = ops.conv3x3_stage(x), ops.conv3x3_stage(dy)
    Wp = W + 2
    rows, guard = B * (H + 2) * Wp, Wp + 1
    yg = ops.conv3x3_grid(xg, ops.hl8_pack(w.permute(0, 2, 3, 1).reshape(N, 9 * C)), b, B, H, W, True)
    wt = ops.hl8_pack(w.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9 * N))
    return xg, g, yg, wt, rows, guard, Wp


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_outputs_stay_inside_their_buffers(shape):
    """guard bands around dw, db, dx and behind the workspace's stated size keep their fill"""
    from hipie_amd import _lib, ops
    lib = _lib.load()
    B, C, N, H, W = shape
    GUARD, FILL = 64, 12345.0
    xg, g, yg, wt, rows, guard, Wp = _raw_case(shape)
    nbytes = -(-rows // CHUNK) * (9 * C * N + N) * 4
    sizes = dict(dw=9 * C * N, db=N, ws=nbytes // 4, dx=rows * C)
    bufs = {n: torch.full((k + 2 * GUARD,), FILL, device=DEV) for n, k in sizes.items()}
    ptr = {n: t[GUARD:].data_ptr() for n, t in bufs.items()}
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.hipie_conv3x3_wgrad(xg[guard:].data_ptr(), C, g[guard:].data_ptr(), N, yg.data_ptr(), rows, Wp, C, N, ptr["dw"], ptr["db"], ptr["ws"],
                                 nbytes, st)
    assert rc == 0, lib.hipie_last_error()
    rc = lib.hipie_conv3x3_split(g[guard:].data_ptr(), N, wt.data_ptr(), None, ptr["dx"], C, rows, Wp, N, C, ops.F32, ops.F32, 0, st)
    assert rc == 0, lib.hipie_last_error()
    torch.cuda.synchronize()
    for n, t in bufs.items():
        assert bool((t[:GUARD] == FILL).all()) and bool((t[GUARD + sizes[n]:] == FILL).all()), n
        assert not bool((t[GUARD:GUARD + sizes[n]] == FILL).any()), n            # and every element inside was written
    dw, db = ops.conv3x3_wgrad(xg, g, yg, B, H, W)
    assert torch.equal(dw.reshape(-1), bufs["dw"][GUARD:GUARD + sizes["dw"]]) and torch.equal(db, bufs["db"][GUARD:GUARD + N])
    assert torch.equal(ops.conv3x3_grid(g, wt, None, B, H, W).reshape(-1), bufs["dx"][GUARD:GUARD + sizes["dx"]])


def test_refusals_through_the_c_abi_launch_nothing():
    from hipie_amd import _lib
    lib = _lib.load()
    shape = SHAPES[1]
    B, C, N, H, W = shape
    xg, g, yg, wt, rows, guard, Wp = _raw_case(shape)
    FILL = 777.0
    nbytes = (9 * C * N + N) * 4
    dw, db, ws = (torch.full((k,), FILL, device=DEV) for k in (9 * C * N, N, nbytes // 4))
    st = torch.cuda.current_stream().cuda_stream

    def call(x=xg[guard:].data_ptr(), dy=g[guard:].data_ptr(), y=yg.data_ptr(), C_=C, dw_=dw.data_ptr(), ws_bytes=nbytes):
        return lib.hipie_conv3x3_wgrad(x, C, dy, N, y, rows, Wp, C_, N, dw_, db.data_ptr(), ws.data_ptr(), ws_bytes, st)
    for kw, msg in ((dict(x=None), b"conv3x3_wgrad: null pointer"), (dict(dw_=None), b"conv3x3_wgrad: null pointer"),
                    (dict(C_=C - 8), b"conv3x3_wgrad: rows=%d Wp=%d C=%d N=%d (C %% 32, N %% 32)" % (rows, Wp, C - 8, N)),
                    (dict(ws_bytes=nbytes - 4), b"conv3x3_wgrad: workspace of %d bytes, need %d" % (nbytes - 4, nbytes)),
                    (dict(dy=g[guard:].data_ptr() + 4), b"conv3x3_wgrad: pointers must be 16-byte aligned"),
                    (dict(y=yg.data_ptr() + 8), b"conv3x3_wgrad: pointers must be 16-byte aligned")):
        assert call(**kw) == -22 and lib.hipie_last_error() == msg, (kw, lib.hipie_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (dw, db, ws))                    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((dw == FILL).any()) and not bool((db == FILL).any())


# --------------------------------------------------------------------------------------------- one training step
STEP_GROUPS = [("convs",), ("norms", "mlp", "packed_windows", "deformable", "pair_losses", "group_norms", "query_attention", "fusion_attention", "convs")]


@pytest.mark.parametrize("names", STEP_GROUPS, ids=["alone", "every-group"])
def test_train_step_with_convolution_nodes_matches_the_reference(names, monkeypatch):
    from hipie_amd.training import functions, net
    be = net.backend(*names)
    assert be.__mro__[0] is be and net.HipBackendConvs in be.__mro__
    ran, declined = [], []
    real = functions.conv3x3_train

    def spy(x, weight, bias=None, relu=False, **k):
        y = real(x, weight, bias, relu, **k)
        (declined if y is None else ran).append((tuple(weight.shape[:2]), bool(relu)))
        return y
    monkeypatch.setattr(functions, "conv3x3_train", spy)
    z, meta, model, step, batch, targets = train_step_case("cuda", be)
    assert step.be is be
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    print("CVT step %s: node ran on %s, declined %s" % ("+".join(names), ran, declined))
    # lay3, lay4, jia_dcn, lay1 of the mask head with their ReLU and layer_1 of the pixel decoder without; lay2 (64 -> 8) falls back
    assert sorted(ran) == sorted([((256, 256), True)] * 3 + [((64, 256), True), ((256, 256), False)]) and declined == [((8, 64), True)]
    check_step_against_golden(z, model, step, losses, total, "cuda", "CONVS step (%s)" % "+".join(names))
