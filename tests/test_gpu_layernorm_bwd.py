"""GPU: hipie_layernorm_backward (csrc/layernorm_bwd.hip) through ops.layernorm_backward, the autograd Function over it and the opt-in
HipBackendNorms wiring of the training net.

Reference: F.layer_norm under autograd in float64 on the same fp32-representable inputs.  Metric: max|got - ref64| / max|ref64| per output
tensor.  Bound per case: max(1e-6, 4 x e_lib), e_lib = the same metric for PyTorch's own fp32 F.layer_norm backward (+ the accumulation
of the residual gradient) on the same inputs -- on the CPU for the operator cases, on the device for the end-to-end case.  The factor 4
covers the different summation order and the recomputed statistics (the convention of the MSDA tests).  Every case prints its figures
(lines starting with LNB) before it asserts."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _layernorm_cases import encoder_case, loss_grads, vit_case

@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _grid_workgroups():
    """the fixed grid of the row kernel, read off the workspace query: it holds one partial row of 2 C floats per workgroup"""
    from hipie_amd import _lib
    return _lib.load().hipie_layernorm_backward_ws_bytes(2 ** 40, 256) // (2 * 256 * 4)


def _torch_backward(s, gy, w, eps, gres, dtype):
    """(dx, dgamma, dbeta) of F.layer_norm under autograd on the CPU in `dtype`, the residual gradient accumulated by autograd"""
    s_ = s.detach().cpu().to(dtype).requires_grad_(True)
    w_ = w.detach().cpu().to(dtype).requires_grad_(True)
    b_ = torch.zeros_like(w_).requires_grad_(True)
    y = F.layer_norm(s_, s_.shape[-1:], w_, b_, eps)
    outs, grads = [y], [gy.detach().cpu().to(dtype)]
    if gres is not None:
        outs.append(s_ * 1.0)
        grads.append(gres.detach().cpu().to(dtype))
    torch.autograd.backward(outs, grads)
    return s_.grad, w_.grad, b_.grad


def _err(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _check(tag, got, ref64, lib32, names=("dx", "dgamma", "dbeta")):
    fails = []
    for n, g, r, l in zip(names, got, ref64, lib32):
        if g is None:
            continue
        e, e_lib = _err(g, r), _err(l, r)
        bound = max(1e-6, 4 * e_lib)
        print("LNB %-34s %-7s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


def _inputs(rows, C, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + rows * 31 + C)
    s = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    gy = torch.randn(rows, C, generator=g)
    gres = torch.randn(rows, C, generator=g)
    w = torch.randn(C, generator=g) * 0.5 + 1.0
    return s, gy, gres, w


def _run_all_modes(tag, s, gy, gres, w, eps):
    from hipie_amd import ops
    refs = {True: _torch_backward(s, gy, w, eps, gres, torch.float64), False: _torch_backward(s, gy, w, eps, None, torch.float64)}
    libs = {True: _torch_backward(s, gy, w, eps, gres, torch.float32), False: _torch_backward(s, gy, w, eps, None, torch.float32)}
    sd, gyd, grd, wd = s.to(DEV), gy.to(DEV), gres.to(DEV), w.to(DEV)
    for with_res in (True, False):
        for params in (True, False):
            got = ops.layernorm_backward(sd, gyd, wd, eps, gres=grd if with_res else None, want_param_grads=params)
            assert got[0].shape == s.shape and got[0].dtype == torch.float32
            assert (got[1] is None and got[2] is None) if not params else (got[1].shape == w.shape and got[2].shape == w.shape)
            _check("%s eps=%g res=%d par=%d" % (tag, eps, with_res, params), got, refs[with_res], libs[with_res])


SHAPES = [(1, 4), (3, 8), (5, 252), (4, 256), (7, 260), (257, 1280), (6, 2048), (64, 1028)]


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_operator_against_float64(rows, C, eps):
    _run_all_modes("(%d,%d)" % (rows, C), *_inputs(rows, C), eps)


def test_operator_resizer_eps():
    _run_all_modes("(4,256)", *_inputs(4, 256, seed=1), 1e-12)


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_more_rows_than_one_grid_stride(eps):
    wg = _grid_workgroups()
    assert 64 <= wg <= 65536
    rows = 4 * wg + 3                                   # four waves per workgroup, one row per wave and stride: 3 rows into the second stride
    _run_all_modes("(%d,256)" % rows, *_inputs(rows, 256), eps)


# --------------------------------------------------------------------------------------------- adversarial rows
@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_constant_rows_are_exact(eps):
    """xhat = 0 and rstd = eps^-1/2: dx = rstd (g - mean g), dgamma = 0, dbeta = sum gy; absolute 1e-6 x max|gy gamma| x rstd"""
    from hipie_amd import ops
    rows, C = 6, 256
    _, gy, _, w = _inputs(rows, C, seed=2)
    s = torch.tensor([0.7, -1.3, 2.9, 1000.25, 0.0, -3e-3])[:, None].expand(rows, C).contiguous()
    rstd = eps ** -0.5
    g = gy.double() * w.double()
    want_dx = rstd * (g - g.mean(-1, keepdim=True))
    tol = 1e-6 * float(g.abs().max()) * rstd
    dx, dg, db = ops.layernorm_backward(s.to(DEV), gy.to(DEV), w.to(DEV), eps)
    e_dx, e_dg = float((dx.double().cpu() - want_dx).abs().max()), float(dg.double().cpu().abs().max())
    e_db = _err(db, gy.double().sum(0))
    print("LNB constant rows eps=%g  |dx - want| %.3e  |dgamma| %.3e  tol %.3e  dbeta err %.3e" % (eps, e_dx, e_dg, tol, e_db))
    assert e_dx <= tol and e_dg <= tol and e_db <= 1e-6


def test_zero_output_gradient_is_exact():
    from hipie_amd import ops
    s, gy, gres, w = _inputs(9, 260, seed=3)
    sd, z, wd, grd = s.to(DEV), torch.zeros(9, 260, device=DEV), w.to(DEV), gres.to(DEV)
    dx, dg, db = ops.layernorm_backward(sd, z, wd, 1e-5, gres=grd)
    assert torch.equal(dx, grd) and not dg.any() and not db.any()
    dx, dg, db = ops.layernorm_backward(sd, z, wd, 1e-5)
    assert not dx.any() and not dg.any() and not db.any()


def test_common_offset_rows():
    """mean 1000, unit noise: a one-pass variance (E x^2 - mean^2) loses every digit here"""
    s, gy, gres, w = _inputs(33, 256, seed=4)
    _run_all_modes("offset 1000 (33,256)", s / 1.5 + 1000.0, gy, gres, w, 1e-5)


def test_one_dominant_element():
    s, gy, gres, w = _inputs(12, 1280, seed=5)
    s[:, 7] *= 1e4
    s[3, 1279] = 4e4
    _run_all_modes("outlier 1e4 (12,1280)", s, gy, gres, w, 1e-6)


def test_non_contiguous_output_gradient():
    from hipie_amd import ops
    s, gy, gres, w = _inputs(10, 260, seed=6)
    wide = torch.randn(10, 520, generator=torch.Generator().manual_seed(1)).to(DEV)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    got = ops.layernorm_backward(s.to(DEV), view, w.to(DEV), 1e-5, gres=gres.to(DEV))
    same = ops.layernorm_backward(s.to(DEV), view.contiguous(), w.to(DEV), 1e-5, gres=gres.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(got, same))
    gyc = view.contiguous().cpu()
    _check("strided gy (10,260)", got, _torch_backward(s, gyc, w, 1e-5, gres, torch.float64), _torch_backward(s, gyc, w, 1e-5, gres, torch.float32))


def test_empty_input():
    from hipie_amd import ops
    dx, dg, db = ops.layernorm_backward(torch.zeros(0, 8, device=DEV), torch.zeros(0, 8, device=DEV), torch.ones(8, device=DEV), 1e-5)
    assert dx.shape == (0, 8) and not dg.any() and not db.any() and dg.shape == (8,)


# --------------------------------------------------------------------------------------------- aliasing, determinism
def test_dx_may_alias_gres():
    from hipie_amd import _lib, ops
    lib = _lib.load()
    for rows, C in ((7, 260), (4099, 256)):
        s, gy, gres, w = (t.to(DEV) for t in _inputs(rows, C, seed=7))
        want = ops.layernorm_backward(s, gy, w, 1e-5, gres=gres)
        buf = gres.clone()
        dg, db = torch.empty_like(w), torch.empty_like(w)
        nbytes = lib.hipie_layernorm_backward_ws_bytes(rows, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        rc = lib.hipie_layernorm_backward(s.data_ptr(), gy.data_ptr(), buf.data_ptr(), w.data_ptr(), buf.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                          ws.data_ptr(), nbytes, rows, C, 1e-5, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.hipie_last_error()
        torch.cuda.synchronize()
        assert torch.equal(buf, want[0]) and torch.equal(dg, want[1]) and torch.equal(db, want[2])


def test_bit_reproducible():
    from hipie_amd import ops
    s, gy, gres, w = (t.to(DEV) for t in _inputs(5000, 256, seed=8))
    a = ops.layernorm_backward(s, gy, w, 1e-5, gres=gres)
    torch.randn(1 << 20, device=DEV).sum()                  # other work in between
    b = ops.layernorm_backward(s, gy, w, 1e-5, gres=gres)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# --------------------------------------------------------------------------------------------- the autograd Function
def _function_case(with_delta, seed):
    g = torch.Generator().manual_seed(seed)
    rows, C = 37, 260
    x, delta = torch.randn(3, rows, C, generator=g), torch.randn(3, rows, C, generator=g) * 0.5
    w, b = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g)
    ca, cb = torch.randn(3, rows, C, generator=g), torch.randn(3, rows, C, generator=g)
    return x, (delta if with_delta else None), w, b, ca, cb


def _torch_graph(x, delta, w, b, ca, cb, eps, dtype, dev):
    leaves = [t.detach().to(dev, dtype).requires_grad_(True) for t in (x, delta, w, b) if t is not None]
    x_, d_, w_, b_ = leaves if delta is not None else (leaves[0], None, leaves[1], leaves[2])
    s = x_ if d_ is None else x_ + d_
    y = F.layer_norm(s, s.shape[-1:], w_, b_, eps)
    loss = (y * ca.to(dev, dtype)).sum() + (s * cb.to(dev, dtype)).sum()
    return torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize("with_delta", [True, False])
def test_function_forward_and_backward(with_delta):
    from hipie_amd import ops
    from hipie_amd.training.functions import add_layer_norm
    eps = 1e-6
    x, delta, w, b, ca, cb = _function_case(with_delta, 21)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, delta, w, b) if t is not None]
    x_, d_, w_, b_ = leaves if with_delta else (leaves[0], None, leaves[1], leaves[2])
    s, y = add_layer_norm(x_, d_, w_, b_, eps)
    s0, y0 = ops.add_layernorm(x_.detach(), None if d_ is None else d_.detach(), w_.detach(), b_.detach(), eps, torch.float32)
    assert torch.equal(s, s0) and torch.equal(y, y0) and s.requires_grad and y.requires_grad
    loss = (y * ca.to(DEV)).sum() + (s * cb.to(DEV)).sum()             # both incoming gradients live
    got = torch.autograd.grad(loss, leaves)
    names = ("x", "delta", "weight", "bias") if with_delta else ("x", "weight", "bias")
    if with_delta:
        assert torch.equal(got[0], got[1])
    _check("Function delta=%d" % with_delta, got, _torch_graph(x, delta, w, b, ca, cb, eps, torch.float64, "cpu"),
           _torch_graph(x, delta, w, b, ca, cb, eps, torch.float32, "cpu"), names)


def test_function_single_live_gradient():
    """only y consumed (the encoder's post-norms), only s consumed: either incoming gradient may be absent"""
    from hipie_amd.training.functions import add_layer_norm
    x, delta, w, b, ca, cb = _function_case(True, 22)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, delta, w, b)]
    s, y = add_layer_norm(*leaves, 1e-5)
    got = torch.autograd.grad((y * ca.to(DEV)).sum(), leaves)
    zero = torch.zeros_like(cb)
    _check("Function y only", got, _torch_graph(x, delta, w, b, ca, zero, 1e-5, torch.float64, "cpu"),
           _torch_graph(x, delta, w, b, ca, zero, 1e-5, torch.float32, "cpu"), ("x", "delta", "weight", "bias"))
    s, y = add_layer_norm(*leaves, 1e-5)
    gx, gd, gw, gb = torch.autograd.grad((s * cb.to(DEV)).sum(), leaves, allow_unused=True)
    assert torch.equal(gx, cb.to(DEV)) and torch.equal(gd, gx) and (gw is None or not gw.any()) and (gb is None or not gb.any())


def test_function_frozen_parameters(monkeypatch):
    from hipie_amd import ops
    from hipie_amd.training import functions
    x, delta, w, b, ca, cb = _function_case(True, 23)
    xd, dd = x.to(DEV).requires_grad_(True), delta.to(DEV).requires_grad_(True)
    wd, bd = w.to(DEV), b.to(DEV)                                     # frozen
    seen = []
    real = ops.layernorm_backward

    def spy(*a, **k):
        seen.append(k.get("want_param_grads"))
        return real(*a, **k)
    monkeypatch.setattr(functions.ops, "layernorm_backward", spy)
    s, y = functions.add_layer_norm(xd, dd, wd, bd, 1e-6)
    ((y * ca.to(DEV)).sum() + (s * cb.to(DEV)).sum()).backward()
    assert seen == [False] and wd.grad is None and bd.grad is None
    ref = _torch_graph(x, delta, w, b, ca, cb, 1e-6, torch.float64, "cpu")
    lib = _torch_graph(x, delta, w, b, ca, cb, 1e-6, torch.float32, "cpu")
    _check("Function frozen", (xd.grad, dd.grad), ref[:2], lib[:2], ("x", "delta"))
    # a frozen weight with a trainable bias still needs the sums
    seen.clear()
    bt = b.to(DEV).requires_grad_(True)
    s, y = functions.add_layer_norm(xd, dd, wd, bt, 1e-6)
    (y * ca.to(DEV)).sum().backward()
    assert seen == [True] and wd.grad is None
    _check("Function frozen weight", (bt.grad,), (ref[3] * 0 + ca.double().sum((0, 1)),), (lib[3] * 0 + ca.sum((0, 1)),), ("bias",))


# --------------------------------------------------------------------------------------------- end to end: HipBackendNorms against HipBackend
def _to_dev(leaves):
    return [t.detach().to(DEV).requires_grad_(True) for t in leaves]


def test_vit_backbone_with_hand_norms():
    from hipie_amd.training import net
    x, sd, cfg = vit_case(torch.float32)
    names = sorted(sd)

    def run(dev, dtype, be):
        leaves = [t.detach().to(dev, dtype).requires_grad_(True) for t in [x] + [sd[n] for n in names]]
        out = net.vit_backbone(leaves[0], dict(zip(names, leaves[1:])), "", cfg, be)
        outs = [out[k] for k in sorted(out)]
        return outs + list(loss_grads(outs, leaves))
    ref = run("cpu", torch.float64, None)
    lib = run(DEV, torch.float32, net.HipBackend)
    got = run(DEV, torch.float32, net.HipBackendNorms)
    _check("vit_backbone", got, ref, lib, ["res3", "res4", "res5", "d input"] + ["d " + n for n in names])


def test_encoder_layer_with_hand_norms():
    from hipie_amd.training import net
    src, pos, refs, shapes, pad, sd = encoder_case(torch.float32, 256)
    names = sorted(sd)

    class OracleMsda:
        @staticmethod
        def msda(value, shapes, loc, aw):
            from oracle import ops as oo
            return oo.ms_deform_attn_core(value, shapes, loc, aw)

    def run(dev, dtype, be):
        leaves = [t.detach().to(dev, dtype).requires_grad_(True) for t in [src, pos] + [sd[n] for n in names]]
        out = net.encoder_layer(leaves[0], leaves[1], refs.to(dev, dtype), shapes, pad.to(dev), dict(zip(names, leaves[2:])), "", be)
        return [out] + list(loss_grads([out], leaves))
    ref = run("cpu", torch.float64, OracleMsda)
    lib = run(DEV, torch.float32, net.HipBackend)
    got = run(DEV, torch.float32, net.HipBackendNorms)
    _check("encoder_layer", got, ref, lib, ["out", "d src", "d pos"] + ["d " + n for n in names])
