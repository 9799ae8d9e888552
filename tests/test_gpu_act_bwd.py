"""GPU: hipie_act_forward / hipie_act_backward (csrc/act_bwd.hip) through ops.act_forward / ops.act_backward, the one-node MLP over them
(functions.MlpFunction / split_mlp) and the opt-in HipBackendMlp / HipBackendNormsMlp wiring of the training net.

Reference: float64 on the CPU on the same fp32-representable inputs -- a64 = act(u64) (torch.erf for the GELU), du64 through torch.autograd,
dbias64 = du64.sum(0).  Metric: max|got - ref64| / max|ref64| per output tensor.  Bound per case: max(1e-6, 4 x e_lib), e_lib = the same
metric for PyTorch's own fp32 F.gelu / F.relu forward and backward and .sum(0) on the CPU with the same inputs (the convention and the floor
of test_gpu_layernorm_bwd.py); for the Function and the end-to-end cases the yardstick is the error of the existing three-node HipBackend
formulation on the same device and inputs.  Every case prints its figures (lines starting with ACT) before it asserts."""
import pytest
import torch
import torch.nn.functional as F

from _act_cases import encoder_case_wide, vit_case_wide
from _layernorm_cases import encoder_case, loss_grads, vit_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GELU, RELU = 1, 2
NAME = {GELU: "gelu", RELU: "relu"}


def _kernel_geometry(N=256):
    """(row chunk, fixed number of workgroups along the rows for width N), read off the workspace query: it holds one partial row of N
    floats per workgroup, and one more workgroup per row chunk until the grid is full"""
    from hipie_amd import _lib
    ws = _lib.load().hipie_act_backward_ws_bytes
    chunk = next(r for r in range(1, 65) if ws(r + 1, N) > ws(1, N))
    return chunk, ws(2 ** 40, N) // (N * 4)


def _torch_act(u, g, act, dtype):
    """(du, a, dbias) of F.gelu / F.relu under autograd on the CPU in `dtype`"""
    u_ = u.detach().cpu().to(dtype).requires_grad_(True)
    a = (F.gelu if act == GELU else F.relu)(u_)
    du, = torch.autograd.grad(a, u_, g.detach().cpu().to(dtype))
    return du, a.detach(), du.sum(0)


def _err(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _check(tag, got, ref64, lib32, names=("du", "a", "dbias")):
    fails = []
    for n, g, r, l in zip(names, got, ref64, lib32):
        if g is None:
            continue
        e, e_lib = _err(g, r), _err(l, r)
        bound = max(1e-6, 4 * e_lib)
        print("ACT %-36s %-12s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


def _inputs(rows, N, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + rows * 31 + N)
    return torch.randn(rows, N, generator=g) * 1.5 + 0.1, torch.randn(rows, N, generator=g)


def _run_all_modes(rows, N, act):
    from hipie_amd import ops
    u, g = _inputs(rows, N)
    ref, lib = _torch_act(u, g, act, torch.float64), _torch_act(u, g, act, torch.float32)
    ud, gd = u.to(DEV), g.to(DEV)
    fwd = ops.act_forward(ud, act)
    assert fwd.shape == u.shape and fwd.dtype == torch.float32
    _check("(%d,%d) %s forward" % (rows, N, NAME[act]), (None, fwd, None), ref, lib)
    first = None
    for want_a in (True, False):
        for want_b in (True, False):
            got = ops.act_backward(ud, gd, act, want_a=want_a, want_bias_grad=want_b)
            assert got[0].shape == u.shape and got[0].dtype == torch.float32 and got[0].data_ptr() != gd.data_ptr()
            assert (got[1] is not None) == want_a and (got[2] is not None) == want_b
            assert got[2] is None or got[2].shape == (N,)
            _check("(%d,%d) %s a=%d b=%d" % (rows, N, NAME[act], want_a, want_b), got, ref, lib)
            if want_a:
                assert torch.equal(got[1], fwd)                     # the recomputation has the forward's bits
            if first is None:
                first = got
            assert torch.equal(got[0], first[0])                    # the optional outputs do not change du
    assert torch.equal(gd, g.to(DEV))                               # without out=, g is left alone


SHAPES = [(1, 4), (3, 8), (5, 252), (7, 260), (257, 1280), (64, 5120), (33, 2052)]       # 2052: two column tiles + 4 columns of a third


@pytest.mark.parametrize("act", [GELU, RELU])
@pytest.mark.parametrize("rows,N", SHAPES)
def test_operator_against_float64(rows, N, act):
    _run_all_modes(rows, N, act)


@pytest.mark.parametrize("act", [GELU, RELU])
def test_more_rows_than_one_grid_stride(act):
    chunk, wg = _kernel_geometry(256)
    assert 1 <= chunk <= 64 and 64 <= wg <= 65536
    _run_all_modes(wg * chunk + 3, 256, act)                        # 3 rows into the second grid stride: a partial row chunk


def test_column_tile_is_not_a_divisor():
    """the widths of SHAPES against the column tile, read off the workspace query: the row grid shrinks when a second tile is needed"""
    _, wg1 = _kernel_geometry(4)
    tile = next(n for n in range(4, 1 << 16, 4) if _kernel_geometry(n + 4)[1] < wg1)
    assert any(N % tile and N > tile for _, N in SHAPES) and any(N < tile for _, N in SHAPES) and any(N % tile == 0 for _, N in SHAPES), tile


# --------------------------------------------------------------------------------------------- special values
def test_gelu_special_values():
    from hipie_amd import ops
    vals = [0.0, -0.0, 1e-8, -1e-8, 0.75, -0.75, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0]
    u = torch.tensor([vals, vals[::-1]], dtype=torch.float32)
    g = torch.tensor([[1.5] * 12, [-3.0] * 12], dtype=torch.float32)
    du, a, db = ops.act_backward(u.to(DEV), g.to(DEV), GELU, want_a=True, want_bias_grad=True)
    assert bool(torch.isfinite(du).all()) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(db).all())
    d = (du.cpu() / g)
    print("ACT gelu special values: act'(u) =", ["%g: %.9g" % (x, y) for x, y in zip(vals, d[0].tolist())])
    assert d[0, 10] == 1.0 and d[0, 11] == 0.0 and d[1, 1] == 1.0 and d[1, 0] == 0.0          # +-40: exactly 1 / 0, no 0 x inf
    assert a[0, 10] == 40.0 and a[0, 11] == 0.0
    assert a[0, 0] == 0.0 and a[0, 1] == 0.0 and abs(float(d[0, 0]) - 0.5) <= 1e-6 and d[0, 0] == d[0, 1]
    _check("gelu special values", (du, a, db), _torch_act(u, g, GELU, torch.float64), _torch_act(u, g, GELU, torch.float32))


def test_gelu_derivative_on_a_grid():
    """absolute error of act'(u) (g = 1) against float64 on 4096 points of a uniform grid over [-8, 8]"""
    from hipie_amd import ops
    u = torch.linspace(-8.0, 8.0, 4096, dtype=torch.float64).float().view(4, 1024)
    g = torch.ones_like(u)
    ref, lib = _torch_act(u, g, GELU, torch.float64)[0], _torch_act(u, g, GELU, torch.float32)[0]
    du = ops.act_backward(u.to(DEV), g.to(DEV), GELU)[0].double().cpu()
    e, e_lib = float((du - ref).abs().max()), float((lib.double() - ref).abs().max())
    bound = max(1e-6, 4 * e_lib)
    print("ACT gelu derivative on [-8, 8]: max abs err %.3e  e_lib %.3e  bound %.3e" % (e, e_lib, bound))
    assert e <= bound


def test_relu_zero_and_negative_zero():
    from hipie_amd import ops
    u = torch.tensor([[0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 1e-30, -1e-30]], dtype=torch.float32)
    g = torch.tensor([[2.0, 3.0, 4.0, 5.0, -2.0, -3.0, 6.0, 7.0]], dtype=torch.float32)
    du, a, db = ops.act_backward(u.to(DEV), g.to(DEV), RELU, want_a=True, want_bias_grad=True)
    assert torch.equal(du.cpu(), torch.tensor([[0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 6.0, 0.0]]))                  # 0 exactly at u = 0 and u = -0.0
    assert torch.equal(a.cpu(), torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1e-30, 0.0]])) and torch.equal(a, ops.act_forward(u.to(DEV), RELU))
    assert torch.equal(db, du[0])


@pytest.mark.parametrize("act", [GELU, RELU])
def test_zero_gradient_is_exact(act):
    from hipie_amd import ops
    u, _ = _inputs(9, 260, seed=3)
    du, a, db = ops.act_backward(u.to(DEV), torch.zeros(9, 260, device=DEV), act, want_a=True, want_bias_grad=True)
    assert not du.any() and not db.any() and torch.equal(a, ops.act_forward(u.to(DEV), act))


def test_empty_input():
    from hipie_amd import ops
    for act in (GELU, RELU):
        du, a, db = ops.act_backward(torch.zeros(0, 8, device=DEV), torch.zeros(0, 8, device=DEV), act, want_a=True, want_bias_grad=True)
        assert du.shape == (0, 8) and a.shape == (0, 8) and db.shape == (8,) and not db.any()
        assert ops.act_forward(torch.zeros(0, 8, device=DEV), act).shape == (0, 8)


# --------------------------------------------------------------------------------------------- aliasing, determinism, views
@pytest.mark.parametrize("act", [GELU, RELU])
def test_du_may_alias_g(act):
    from hipie_amd import ops
    chunk, wg = _kernel_geometry(260)
    for rows, N in ((7, 260), (wg * chunk + 3, 260)):
        u, g = (t.to(DEV) for t in _inputs(rows, N, seed=7))
        want = ops.act_backward(u, g, act, want_a=True, want_bias_grad=True)
        buf = g.clone()
        got = ops.act_backward(u, buf, act, want_a=True, want_bias_grad=True, out=buf)
        assert got[0].data_ptr() == buf.data_ptr()
        assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_bit_reproducible():
    from hipie_amd import ops
    u, g = (t.to(DEV) for t in _inputs(5000, 1024, seed=8))
    for act in (GELU, RELU):
        a = ops.act_backward(u, g, act, want_a=True, want_bias_grad=True)
        torch.randn(1 << 20, device=DEV).sum()                  # other work in between
        b = ops.act_backward(u, g, act, want_a=True, want_bias_grad=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("act", [GELU, RELU])
def test_strided_and_offset_views(act):
    from hipie_amd import ops
    rows, N = 10, 260
    gen = torch.Generator().manual_seed(1)
    wide = torch.randn(rows, 2 * N, generator=gen).to(DEV)
    u = (torch.randn(rows, N, generator=gen) * 1.5).to(DEV)
    view = wide[:, ::2]                                              # column-sliced gradient
    assert not view.is_contiguous()
    got = ops.act_backward(u, view, act, want_a=True, want_bias_grad=True)
    same = ops.act_backward(u, view.contiguous(), act, want_a=True, want_bias_grad=True)
    assert all(torch.equal(x, y) for x, y in zip(got, same))
    flat_u, flat_g = torch.zeros(rows * N + 1, device=DEV), torch.zeros(rows * N + 1, device=DEV)
    flat_u[1:], flat_g[1:] = u.reshape(-1), view.reshape(-1)
    ou, og = flat_u[1:].view(rows, N), flat_g[1:].view(rows, N)      # 4 bytes past a 16-byte boundary
    assert ou.data_ptr() % 16 == 4 and og.data_ptr() % 16 == 4
    off = ops.act_backward(ou, og, act, want_a=True, want_bias_grad=True, out=og)
    assert all(torch.equal(x, y) for x, y in zip(off, same))
    assert torch.equal(ops.act_forward(ou, act), same[1])
    gc = view.contiguous().cpu()
    _check("strided g (10,260) %s" % NAME[act], got, _torch_act(u, gc, act, torch.float64), _torch_act(u, gc, act, torch.float32))


# --------------------------------------------------------------------------------------------- the autograd Function
def _mlp_case(M, C, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, M // 2, C, generator=g)
    w1, b1 = torch.randn(hidden, C, generator=g) * C ** -0.5, torch.randn(hidden, generator=g) * 0.3
    w2, b2 = torch.randn(C, hidden, generator=g) * hidden ** -0.5, torch.randn(C, generator=g) * 0.3
    return [x, w1, b1, w2, b2], torch.randn(2, M // 2, C, generator=g)


def _three_nodes(x, w1, b1, w2, b2, act):
    """the expression of net.vit_backbone / net.encoder_layer under HipBackend (on the device), or plain torch (on the host)"""
    f = F.gelu if act == GELU else F.relu
    if x.is_cuda:
        from hipie_amd.training.functions import split_linear
        return split_linear(f(split_linear(x, w1, b1, w1, "w")), w2, b2, w2, "w")
    return F.linear(f(F.linear(x, w1, b1)), w2, b2)


def _mlp_run(fn, tensors, cot, act, dev, dtype, frozen=()):
    leaves = [t.detach().to(dev, dtype).requires_grad_(i not in frozen) for i, t in enumerate(tensors)]
    y = fn(*leaves, act)
    grads = torch.autograd.grad((y * cot.to(dev, dtype)).sum(), [l for l in leaves if l.requires_grad])
    it = iter(grads)
    return [y.detach()] + [next(it) if l.requires_grad else None for l in leaves]


MLP_NAMES = ("y", "d x", "d w1", "d b1", "d w2", "d b2")
MLP_CASES = [(300, 64, 128, GELU), (512, 256, 1024, RELU)]


@pytest.mark.parametrize("M,C,hidden,act", MLP_CASES)
def test_mlp_function_against_float64(M, C, hidden, act, monkeypatch):
    from hipie_amd.training import functions
    tensors, cot = _mlp_case(M, C, hidden, 40 + act)
    ref = _mlp_run(_three_nodes, tensors, cot, act, "cpu", torch.float64)
    parent = _mlp_run(_three_nodes, tensors, cot, act, DEV, torch.float32)
    applied = []
    real = functions.MlpFunction.apply
    monkeypatch.setattr(functions.MlpFunction, "apply", lambda *a: applied.append(1) or real(*a))
    got = _mlp_run(functions.split_mlp, tensors, cot, act, DEV, torch.float32)
    assert applied == [1]                                       # the one-node path, not the fall-through
    _check("MlpFunction (%d,%d,%d) %s" % (M, C, hidden, NAME[act]), got, ref, parent, MLP_NAMES)
    # frozen inputs: their gradients are not computed, the others keep their bits
    no_x = _mlp_run(functions.split_mlp, tensors, cot, act, DEV, torch.float32, frozen=(0,))
    no_b = _mlp_run(functions.split_mlp, tensors, cot, act, DEV, torch.float32, frozen=(2, 4))
    assert no_x[1] is None and no_b[3] is None and no_b[5] is None
    for i, n in enumerate(MLP_NAMES):
        assert i == 1 or torch.equal(no_x[i], got[i]), n
        assert i in (3, 5) or torch.equal(no_b[i], got[i]), n


def test_mlp_function_returns_none_for_frozen_inputs(monkeypatch):
    """what backward() itself returns (autograd.grad above would hide a gradient that was computed and dropped)"""
    from hipie_amd import ops
    from hipie_amd.training import functions
    tensors, cot = _mlp_case(300, 64, 128, 50)
    seen = []
    real = ops.act_backward

    def spy(*a, **k):
        seen.append((k.get("want_a"), k.get("want_bias_grad")))
        return real(*a, **k)
    monkeypatch.setattr(functions.ops, "act_backward", spy)
    for frozen, want in (((), (True, True)), ((2, 4), (True, False)), ((3,), (False, True)), ((0,), (True, True))):
        seen.clear()
        leaves = [t.to(DEV).requires_grad_(i not in frozen) for i, t in enumerate(tensors)]
        y = functions.split_mlp(*leaves, GELU)
        out = y.grad_fn.apply(cot.to(DEV))                          # the node's own backward
        assert seen == [want], (frozen, seen)
        assert len(out) == 6 and out[5] is None
        for i in range(5):
            assert (out[i] is None) == (i in frozen), (frozen, i)


def _saved_bytes(fn):
    seen = {}

    def pack(t):
        if t.is_cuda:
            st = t.untyped_storage()
            seen[st.data_ptr()] = st.nbytes()
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = fn()
    assert y.requires_grad
    return sum(seen.values())


def test_saved_bytes():
    """bytes of the distinct storages one forward saves for the backward.  GELU: the three nodes keep u (F.gelu's input) AND a (the second
    linear's input); the one node keeps u alone -- exactly M x hidden x 4 bytes less.  ReLU: the library's relu saves its RESULT, which is
    the storage the second linear saves as well, so the three nodes keep a alone and there is nothing to gain: the one node (u instead of
    a) must not save more."""
    from hipie_amd.training import functions
    M, C, hidden = 512, 256, 1024
    for act in (GELU, RELU):
        tensors, _ = _mlp_case(M, C, hidden, 60)
        leaves = [t.to(DEV).requires_grad_(True) for t in tensors]
        one = _saved_bytes(lambda: functions.split_mlp(*leaves, act))
        three = _saved_bytes(lambda: _three_nodes(*leaves, act))
        most = 4 * (M * C + M * hidden + 2 * C * hidden)             # x + u + W1 + W2
        print("ACT saved bytes %s: one node %d, three nodes %d, x + u + W1 + W2 = %d, M x hidden x 4 = %d" % (NAME[act], one, three, most, M * hidden * 4))
        assert one <= most and one <= three
        if act == GELU:
            assert three - one == M * hidden * 4


def test_split_mlp_falls_through_below_the_split_gemm_shapes():
    """fewer than 256 rows, or a width that is no multiple of 32: the three-node composition, bit for bit"""
    from hipie_amd.training import functions
    for M, C, hidden in ((60, 64, 128), (300, 48, 128), (300, 64, 80)):
        tensors, cot = _mlp_case(M, C, hidden, 70)
        for act in (GELU, RELU):
            a = _mlp_run(functions.split_mlp, tensors, cot, act, DEV, torch.float32)
            b = _mlp_run(_three_nodes, tensors, cot, act, DEV, torch.float32)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (M, C, hidden, act)


# --------------------------------------------------------------------------------------------- end to end against HipBackend
def _mlp_calls(monkeypatch):
    from hipie_amd.training import functions
    applied = []
    real = functions.MlpFunction.apply
    monkeypatch.setattr(functions.MlpFunction, "apply", lambda *a: applied.append(1) or real(*a))
    return applied


@pytest.mark.parametrize("case,nodes", [(vit_case, 0), (vit_case_wide, 3)])
def test_vit_backbone_with_one_node_mlp(case, nodes, monkeypatch):
    """vit_case: 60 token rows, width 16 -- split_mlp falls through; vit_case_wide: 264 rows, width 32 -- one MlpFunction per block"""
    from hipie_amd.training import net
    x, sd, cfg = case(torch.float32)
    names = sorted(sd)

    def run(dev, dtype, be):
        leaves = [t.detach().to(dev, dtype).requires_grad_(True) for t in [x] + [sd[n] for n in names]]
        out = net.vit_backbone(leaves[0], dict(zip(names, leaves[1:])), "", cfg, be)
        outs = [out[k] for k in sorted(out)]
        return outs + list(loss_grads(outs, leaves))
    ref = run("cpu", torch.float64, None)
    lib = run(DEV, torch.float32, net.HipBackend)
    applied = _mlp_calls(monkeypatch)
    for be in (net.HipBackendMlp, net.HipBackendNormsMlp):
        applied.clear()
        got = run(DEV, torch.float32, be)
        assert len(applied) == nodes
        _check("%s %s" % (case.__name__, be.__name__), got, ref, lib, ["res3", "res4", "res5", "d input"] + ["d " + n for n in names])


@pytest.mark.parametrize("case,nodes", [(lambda dt: encoder_case(dt, 256), 0), (encoder_case_wide, 1)])
def test_encoder_layer_with_one_node_mlp(case, nodes, monkeypatch):
    """encoder_case: 38 rows, a 24-wide FFN -- the fall-through; encoder_case_wide: 322 rows, width 256, a 64-wide FFN -- one MlpFunction"""
    from hipie_amd.training import net
    src, pos, refs, shapes, pad, sd = case(torch.float32)
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
    applied = _mlp_calls(monkeypatch)
    for be in (net.HipBackendMlp, net.HipBackendNormsMlp):
        applied.clear()
        got = run(DEV, torch.float32, be)
        assert len(applied) == nodes
        _check("encoder_layer rows=%d %s" % (src.shape[0] * src.shape[1], be.__name__), got, ref, lib, ["out", "d src", "d pos"] + ["d " + n for n in names])
