"""GPU: the training projections -- hipie_patch_pack (csrc/patch_pack.hip) through ops_patch, functions.PatchConvFunction for the
convolutions whose kernel equals their stride and the transposed 2 x 2 ones, and the opt-in HipBackendProjections wiring of the step.

Reference: the float64 algebra of tests/_patch_conv_cases.py (checked against torch.autograd in test_patch_conv_cpu.py).  Metric:
max|got - ref64| / max|ref64| per tensor.  Bound per case: max(3e-6, 4 x e_lib), the convolution node's (tests/test_gpu_conv_train.py):
e_lib is the same metric for the library's fp32 F.conv2d / F.conv_transpose2d autograd on the device on the same inputs in the same run.
Every case prints its figures (lines starting with PCV) before it asserts.  The shapes and what each reaches: _patch_conv_cases.SHAPES."""
import ctypes
import itertools

import pytest
import torch

from _patch_conv_cases import IDS, SHAPES, algebra64, frozen_input, gather, inputs, out_shape, torch_graph
from _train_step_cases import check_step_against_golden, train_step_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 3e-6
NAMES = ("y", "dx", "dW", "db")


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
        print("PCV %-40s %-4s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


def _tag(shape):
    return "x".join(map(str, shape))


def _layout(t, layout):
    """the map on the device, NCHW dense or channels-last"""
    t = t.to(DEV)
    return t.contiguous() if layout == "nchw" else t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _packed_map(shape):
    """the map of a shape that is packed with the shape's own k: the input of a convolution, the output gradient of a transposed one"""
    x, dy, w, b = inputs(shape)
    return dy if shape[6] == "transposed" else x


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))


# --------------------------------------------------------------------------------------------- the pack
@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pack_has_the_bits_of_the_row_entries(shape, layout):
    from hipie_amd import ops, ops_patch
    k = shape[5]
    host = _packed_map(shape)
    for scaled in (False, True):
        src = host * 2.0 ** -20 if scaled else host
        m = _layout(src, layout)
        blk = ops.grad_scale(m.contiguous().view(-1, 4)) if scaled else None
        s = float(blk[0]) if scaled else 1.0
        if scaled:                                    # amax 2^-20 * ~4 lands in [2^14, 2^15): the scale is far from 1
            assert s >= 2.0 ** 30 and float(blk[0] * blk[1]) == 1.0
        rows = gather(m, k).contiguous()
        f32, hl, hlt, dsum = ops_patch.patch_pack(m, k, blk, want_f32=True, want_rows=True, want_t=True, want_sum=True)
        M, N = rows.shape
        Mp = -(-M // 32) * 32
        assert f32.shape == (M, N) and hl.shape == (M, 2 * N) and hlt.shape == (N, 2 * Mp) and dsum.shape == (m.shape[1],)
        assert _same_bits(f32, rows)
        assert torch.equal(hl, ops.to_hl8(rows, scale=s))
        assert torch.equal(hlt, ops.to_hl8_t(rows, 32, scale=s))                  # pad columns included
        if Mp > M:
            assert not bool(hlt.view(N, Mp // 8, 16)[:, -(-M // 8):].any())         # whole groups of 8 beyond M are zero
        ref = src.double().sum((0, 2, 3))
        lib = m.sum((0, 2, 3))
        _check("pack %s %s scaled=%d" % (_tag(shape), layout, scaled), ("dsum",), (dsum,), (ref,), (lib,))
        other = torch.randn(257, 33, device=DEV) @ torch.randn(33, 65, device=DEV)         # other work in between
        again = ops_patch.patch_pack(m, k, blk, want_f32=False, want_rows=False, want_t=False, want_sum=True)
        assert again[:3] == (None, None, None) and _same_bits(again[3], dsum) and other.shape == (257, 65)
        # each output alone has the bits of all four together
        for i, kw in enumerate(({"want_f32": True}, {"want_rows": True}, {"want_t": True})):
            want = dict(want_f32=False, want_rows=False, want_t=False)
            want.update(kw)
            alone = ops_patch.patch_pack(m, k, blk, **want)
            assert torch.equal(alone[i], (f32, hl, hlt)[i]) and [o is None for o in alone] == [j != i for j in range(4)]


def test_pack_reads_strided_and_unaligned_maps_in_place():
    """a channel slice of an NCHW map, a W slice (rows off 16 bytes), a channels-last map with a wider pixel stride, a larger rows_p"""
    from hipie_amd import ops, ops_patch
    g = torch.Generator().manual_seed(5)
    big = torch.randn(2, 48, 6, 9, generator=g).to(DEV)
    wide = torch.randn(2, 4, 8, 40, generator=g).to(DEV)
    cases = [(big[:, 8:40], 1), (big[:, :32, :, 1:9], 1), (big[:, :32, :, 1:9], 2), (wide[..., 4:36].permute(0, 3, 1, 2), 1),
             (wide[..., 4:36].permute(0, 3, 1, 2), 2), (wide[..., 1:33].permute(0, 3, 1, 2), 1), (wide.permute(0, 3, 1, 2)[:, :, :, ::2], 2)]
    for m, k in cases:
        rows = gather(m, k).contiguous()
        f32, hl, hlt, dsum = ops_patch.patch_pack(m, k, None, want_f32=True, want_sum=True, rows_p=128)
        assert _same_bits(f32, rows) and torch.equal(hl, ops.to_hl8(rows)) and hlt.shape == (rows.shape[1], 256)
        assert torch.equal(hlt[:, :2 * (-(-rows.shape[0] // 32) * 32)], ops.to_hl8_t(rows, 32)) and not bool(hlt[:, 2 * (-(-rows.shape[0] // 32) * 32):].any())
        assert _err(dsum, m.double().sum((0, 2, 3))) <= FLOOR


# --------------------------------------------------------------------------------------------- the operator passes
def _run(shape, x, dy, w, b, grad_x=None, grad_w=True, grad_b=True, dy_dev=None):
    """the node's forward and backward on NCHW device inputs -> (y, dx, dW, db, the leaves)"""
    from hipie_amd.training import functions
    grad_x = (not frozen_input(shape)) if grad_x is None else grad_x
    xd = x.to(DEV).requires_grad_(grad_x)
    wd, bd = w.to(DEV).requires_grad_(grad_w), b.to(DEV).requires_grad_(grad_b)
    y = functions.patch_convt_train(xd, wd, bd) if shape[6] == "transposed" else functions.patch_conv_train(xd, wd, bd, stride=shape[5])
    assert y is not None and y.shape == out_shape(shape) and y.requires_grad == (grad_x or grad_w or grad_b)
    assert y.permute(0, 2, 3, 1).is_contiguous()                                 # a channels-last view of the rows
    if y.requires_grad:
        y.backward(dy.to(DEV) if dy_dev is None else dy_dev)
    return y.detach(), xd.grad, wd.grad, bd.grad, (xd, wd, bd)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_operator_against_float64(shape):
    x, dy, w, b = inputs(shape)
    y, dx, dw, db, _ = _run(shape, x, dy, w, b)
    assert (dx is None) == frozen_input(shape) and dw.shape == w.shape and dw.is_contiguous() and db.shape == b.shape
    assert dx is None or dx.shape == x.shape
    _check(_tag(shape), NAMES, (y, dx, dw, db), algebra64(shape, x, dy, w, b), torch_graph(shape, x, dy, w, b, torch.float32, DEV))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gradients_scale_exactly_with_dy(shape):
    x, dy, w, b = inputs(shape, seed=1)
    base = _run(shape, x, dy, w, b)
    small = _run(shape, x, dy * 2.0 ** -20, w, b)
    for n, g0, g1 in zip(NAMES[1:], base[1:4], small[1:4]):
        if g0 is not None:
            assert _same_bits(g0 * 2.0 ** -20, g1), n
    for e in (-30, 15):
        f = 2.0 ** e
        got = _run(shape, x, dy * f, w, b)
        _check("%s dy*2^%d" % (_tag(shape), e), NAMES, got[:4], algebra64(shape, x, dy * f, w, b), torch_graph(shape, x, dy * f, w, b, torch.float32, DEV))


# --------------------------------------------------------------------------------------------- the autograd Function
def _spies(monkeypatch):
    from hipie_amd import ops, ops_patch
    calls = []

    def spy(mod, name, describe):
        real = getattr(mod, name)

        def wrapped(*a, **k):
            calls.append(describe(*a, **k))
            return real(*a, **k)
        monkeypatch.setattr(mod, name, wrapped)
    spy(ops_patch, "patch_pack", lambda x, k, scale=None, want_f32=False, want_rows=True, want_t=True, want_sum=False, rows_p=None:
        ("pack", "grad" if scale is not None else "act", bool(want_f32), bool(want_rows), bool(want_t), bool(want_sum)))
    spy(ops, "grad_pack", lambda dy, scale, want_rows=True, want_t=True, want_bias=False, rows_p=None:
        ("pack", "grad", False, bool(want_rows), bool(want_t), bool(want_bias)))
    spy(ops, "to_hl8_t", lambda x, pad_to=32, scale=1.0: ("pack", "act", False, False, True, False))
    spy(ops, "gemm_scaled", lambda a, w, alpha_dev, **kw: ("gemm", kw.get("tag")))
    spy(ops, "gemm_split_k_scaled", lambda a, w, nk, alpha_dev: ("gemm", "train_dw"))
    spy(ops, "grad_scale", lambda dy: ("scale",))
    return calls


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[4], SHAPES[6]], ids=[IDS[1], IDS[3], IDS[4], IDS[6]])
@pytest.mark.parametrize("dy_layout", ["nchw", "cl"])
def test_function_honours_every_requires_grad_combination(shape, dy_layout, monkeypatch):
    x, dy, w, b = inputs(shape, seed=2)
    dyd = _layout(dy, dy_layout)
    full = _run(shape, x, dy, w, b)
    calls = _spies(monkeypatch)
    for grad_x, grad_w, grad_b in itertools.product((False, True), repeat=3):
        if grad_x and frozen_input(shape):
            continue
        del calls[:]
        y, dx, dw, db, (xd, wd, bd) = _run(shape, x, dy, w, b, grad_x, grad_w, grad_b, dy_dev=dyd)
        combo = "x=%d w=%d b=%d" % (grad_x, grad_w, grad_b)
        assert _same_bits(y, full[0]), combo                                      # no forward differs between the combinations
        back = [c for c in calls if not (c[0] == "pack" and c[1] == "act" and c[2])]          # without the forward's fp32 rows of x
        print("PCV function %s dy=%s %s: %s" % (_tag(shape), dy_layout, combo, back))
        if not (grad_x or grad_w or grad_b):
            assert back == [] and dx is None and dw is None and db is None
            continue
        # ONE pass over dy with exactly the wanted forms; the transposed x only for dW; one GEMM per wanted product
        assert [c for c in back if c[0] == "scale"] == [("scale",)]
        assert [c for c in back if c[:2] == ("pack", "grad")] == [("pack", "grad", False, grad_x, grad_w, grad_b)], combo
        assert [c for c in back if c[:2] == ("pack", "act")] == ([("pack", "act", False, False, True, False)] if grad_w else []), combo
        assert sorted(c[1] for c in back if c[0] == "gemm") == sorted(["train_dx"] * grad_x + ["train_dw"] * grad_w), combo
        for n, g, want, on in zip(NAMES[1:], (dx, dw, db), full[1:4], (grad_x, grad_w, grad_b)):
            assert (g is not None) == on, (combo, n)
            if on:
                assert _same_bits(g, want), (combo, n)                             # a frozen operand changes no other gradient; dy's layout neither
        if grad_w:
            assert wd.grad.shape == w.shape and wd.grad.is_contiguous()


def test_function_saves_x_and_weight_only_and_reads_strided_dy():
    from hipie_amd.training import functions
    for shape in (SHAPES[2], SHAPES[5]):
        x, dy, w, b = inputs(shape, seed=3)
        full = _run(shape, x, dy, w, b)
        xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
        y = functions.patch_convt_train(xd, wd, bd) if shape[6] == "transposed" else functions.patch_conv_train(xd, wd, bd, stride=shape[5])
        saved = y.grad_fn.saved_tensors
        assert len(saved) == 2 and saved[0].data_ptr() == xd.data_ptr() and saved[1].data_ptr() == wd.data_ptr()
        # a channel slice of a larger NCHW map, a W-strided map (copied once), an expanded one-value gradient
        B, C, H, W = dy.shape
        big = torch.zeros(B, C + 8, H, W, device=DEV)
        big[:, 4:C + 4] = dy.to(DEV)
        wide = torch.zeros(B, C, H, 2 * W, device=DEV)
        wide[..., ::2] = dy.to(DEV)
        for name, g in (("channel slice", big[:, 4:C + 4]), ("w stride 2", wide[..., ::2])):
            for t in (xd, wd, bd):
                t.grad = None
            y.backward(g, retain_graph=True)
            for n, got, want in zip(NAMES[1:], (xd.grad, wd.grad, bd.grad), full[1:4]):
                assert _same_bits(got, want), (shape, name, n)
        for t in (xd, wd, bd):
            t.grad = None
        y.sum().backward()                                                          # dy = ones, every stride 0
        ones = _run(shape, x, torch.ones_like(dy), w, b)
        assert all(_same_bits(g, o) for g, o in zip((xd.grad, wd.grad, bd.grad), ones[1:4]))


def test_node_declines_what_it_does_not_take():
    from hipie_amd.training import functions
    conv, convt = functions.patch_conv_train, functions.patch_convt_train
    x = torch.randn(2, 64, 4, 6, device=DEV)
    w, b = torch.randn(32, 64, 1, 1, device=DEV), torch.randn(32, device=DEV)
    w2 = torch.randn(32, 64, 2, 2, device=DEV)
    assert conv(x, w, b) is not None and conv(x, w2, b, stride=2) is not None
    assert conv(x, torch.randn(32, 64, 3, 3, device=DEV), b, padding=1) is None and conv(x, torch.randn(32, 64, 3, 3, device=DEV), b) is None     # 3 x 3
    assert conv(x, w, b, stride=2) is None and conv(x, w2, b) is None                                   # stride != kernel
    assert conv(x, w, b, padding=1) is None and conv(x, torch.randn(32, 32, 1, 1, device=DEV), b, groups=2) is None
    assert conv(x.half(), w.half(), b.half()) is None and conv(x, w.half(), b) is None                  # fp16
    assert conv(x.cpu(), w.cpu(), b.cpu()) is None and conv(x, w.cpu(), b) is None                      # host tensors
    assert conv(torch.randn(2, 80, 4, 6, device=DEV), torch.randn(32, 80, 1, 1, device=DEV), b) is None       # C_in = 80
    img = torch.randn(1, 3, 32, 32, device=DEV)
    w16 = torch.randn(32, 3, 16, 16, device=DEV)
    assert conv(img, w16, b, stride=16) is not None and conv(img.clone().requires_grad_(True), w16, b, stride=16) is None    # trainable input, k = 16
    assert conv(x.clone().requires_grad_(True), w2, b, stride=2) is None
    wt, bt = torch.randn(64, 8, 2, 2, device=DEV), torch.randn(8, device=DEV)
    assert convt(x, wt, bt) is not None and convt(x, wt, bt, stride=1) is None and convt(x, wt, bt, output_padding=1) is None
    assert convt(torch.randn(2, 80, 4, 6, device=DEV), torch.randn(80, 8, 2, 2, device=DEV), bt) is None
    assert convt(x, torch.randn(64, 12, 2, 2, device=DEV), torch.randn(12, device=DEV)) is None and convt(x.cpu(), wt.cpu(), bt.cpu()) is None


# --------------------------------------------------------------------------------------------- the C ABI
def _guarded(n, dtype, fill, guard=64):
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    return buf, buf[guard:guard + n]


def _guards_intact(buf, n, fill, guard=64):
    return bool((buf[:guard] == fill).all()) and bool((buf[guard + n:] == fill).all())


@pytest.mark.parametrize("shape,layout", [(SHAPES[2], "nchw"), (SHAPES[2], "cl"), (SHAPES[4], "nchw"), (SHAPES[5], "cl"), (SHAPES[6], "nchw")],
                         ids=["ragged-nchw", "ragged-cl", "transposed-nchw", "transposed-cl", "patch16-nchw"])
def test_pack_writes_every_element_and_nothing_else(shape, layout):
    from hipie_amd import _lib, ops
    lib = _lib.load()
    k = shape[5]
    m = _layout(_packed_map(shape), layout)
    B, C, H, W = m.shape
    M, N = B * (H // k) * (W // k), C * k * k
    Mp = -(-M // 32) * 32
    need = ops._size("hipie_patch_pack_ws_bytes", Mp, N)
    assert need == -(-Mp // 128) * N * 4
    fbuf, f = _guarded(M * N, torch.float32, 12345.0)
    rbuf, r = _guarded(M * 2 * N, torch.float16, -7.0)
    tbuf, t = _guarded(N * 2 * Mp, torch.float16, -7.0)
    dbuf, d = _guarded(C, torch.float32, 12345.0)
    wbuf, ws = _guarded(need // 4, torch.float32, 12345.0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.hipie_patch_pack(m.data_ptr(), B, C, H, W, *m.stride(), k, None, f.data_ptr(), N, r.data_ptr(), 2 * N, t.data_ptr(), 2 * Mp, Mp,
                              d.data_ptr(), ws.data_ptr(), need, st)
    assert rc == 0, lib.hipie_last_error()
    torch.cuda.synchronize()
    for buf, view, fill in ((fbuf, f, 12345.0), (rbuf, r, -7.0), (tbuf, t, -7.0), (dbuf, d, 12345.0), (wbuf, ws, 12345.0)):
        assert _guards_intact(buf, view.numel(), fill) and not bool((view == fill).any())
    rows = gather(m, k).contiguous()
    assert torch.equal(f.view(M, N), rows) and torch.equal(r.view(M, 2 * N), ops.to_hl8(rows)) and torch.equal(t.view(N, 2 * Mp), ops.to_hl8_t(rows, 32))


def test_refusals_through_the_c_abi_launch_nothing():
    from hipie_amd import _lib
    lib = _lib.load()
    m = torch.randn(1, 32, 4, 8, device=DEV)
    B, C, H, W = m.shape
    M, N, Mp = 32, 32, 32
    fbuf, f = _guarded(M * N, torch.float32, 12345.0)
    rbuf, r = _guarded(M * 2 * N, torch.float16, -7.0)
    tbuf, t = _guarded(N * 2 * Mp, torch.float16, -7.0)
    dbuf, d = _guarded(C, torch.float32, 12345.0)
    wbuf, ws = _guarded(N, torch.float32, 12345.0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(x=m.data_ptr(), C_=C, H_=H, strides=tuple(m.stride()), k=1, f_=f.data_ptr(), ldf=N, r_=r.data_ptr(), ldo=2 * N, t_=t.data_ptr(), ldt=2 * Mp,
             rows_p=Mp, d_=d.data_ptr(), ws_=ws.data_ptr(), ws_bytes=4 * N):
        return lib.hipie_patch_pack(x, B, C_, H_, W, *strides, k, None, f_, ldf, r_, ldo, t_, ldt, rows_p, d_, ws_, ws_bytes, st)
    for kw, msg in ((dict(x=None), b"patch_pack: null pointer"),
                    (dict(C_=31), b"patch_pack: N=31 (C k^2 must be a multiple of 8, below 2^22), M=32 (below 2^31)"),
                    (dict(k=3), b"patch_pack: k=3 must divide H=4 and W=8"),
                    (dict(H_=6, k=4), b"patch_pack: k=4 must divide H=6 and W=8"),
                    (dict(rows_p=48), b"patch_pack: rows_p=48 (>= M=32, a multiple of 32)"),
                    (dict(H_=8, rows_p=32), b"patch_pack: rows_p=32 (>= M=64, a multiple of 32)"),
                    (dict(strides=(1024, 32, 8, 2)), b"patch_pack: strides (1024, 32, 8, 2): the unit stride must be that of W or of C"),
                    (dict(f_=f.data_ptr() + 4), b"patch_pack: the outputs must be 16-byte aligned"),
                    (dict(r_=r.data_ptr() + 2), b"patch_pack: the outputs must be 16-byte aligned"),
                    (dict(t_=t.data_ptr() + 8), b"patch_pack: the outputs must be 16-byte aligned"),
                    (dict(ldf=34), b"patch_pack: fp32 row stride 34 (>= N=32, a multiple of 4)"),
                    (dict(ldo=60), b"patch_pack: row operand stride 60 (>= 2 N, a multiple of 8)"),
                    (dict(ldt=68), b"patch_pack: transposed operand stride 68 (>= 2 rows_p, a multiple of 8)"),
                    (dict(ws_=None), b"patch_pack: dsum and its workspace come together"),
                    (dict(d_=None), b"patch_pack: dsum and its workspace come together"),
                    (dict(ws_bytes=4 * N - 4), b"patch_pack: workspace of 124 bytes, need 128")):
        assert call(**kw) == -22 and lib.hipie_last_error() == msg, (kw, lib.hipie_last_error())
    assert call(f_=None, r_=None, t_=None, d_=None, ws_=None) == 0                 # all outputs NULL: a no-op
    torch.cuda.synchronize()
    for buf, fill in ((fbuf, 12345.0), (rbuf, -7.0), (tbuf, -7.0), (dbuf, 12345.0), (wbuf, 12345.0)):
        assert bool((buf == fill).all())                                           # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((f == 12345.0).any()) and not bool((d == 12345.0).any())


# --------------------------------------------------------------------------------------------- one training step
STEP_GROUPS = [("projections",), None]


@pytest.mark.parametrize("names", STEP_GROUPS, ids=["alone", "every-group"])
def test_train_step_with_projection_nodes_matches_the_reference(names, monkeypatch):
    """The issue behind this group also lists the patch embedding among the sites that run in the step.  Measured on the MI355X with it
    routed (sampling-offsets figure of check_step_against_golden, bound 5e-3; cudnn.deterministic off / on): the group alone 5.46e-3 /
    1.48e-3, every group 3.85e-4 / 5.50e-3, the patch embedding as the only site 5.45e-3 / 5.43e-3 alone and 5.51e-3 / 5.47e-3 composed;
    every site BUT the patch embedding 1.24e-4 / 1.09e-3 alone and 3.85e-4 / 3.84e-4 composed.  The group therefore leaves the patch
    embedding on the library; this test asserts the sites the group does route."""
    from hipie_amd.training import functions, net
    if names is None:
        names = tuple({**net.GROUPS, **net.EXTRA_GROUPS, **net.LATER_GROUPS})
    be = net.backend(*names)
    assert be.__mro__[0] is be and net.HipBackendProjections in be.__mro__
    ran, declined = [], []

    def spy(name, form):
        real = getattr(functions, name)

        def wrapped(x, weight, *a, **k):
            y = real(x, weight, *a, **k)
            (declined if y is None else ran).append((form, tuple(weight.shape)))
            return y
        monkeypatch.setattr(functions, name, wrapped)
    spy("patch_conv_train", "conv")
    spy("patch_convt_train", "convt")
    z, meta, model, step, batch, targets = train_step_case("cuda", be)
    assert step.be is be
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    print("PCV step %s: node ran on %s, declined %s" % ("+".join(names), ran, declined))
    # fpn1.0, input_proj.1 / .2 of both heads, mask_features.0 and mask_features.3 run, in this order; the C_in = 80 sites -- input_proj.0
    # of both heads and adapter_1 -- decline (80 % 32 != 0) and run the library convolution.  The patch embedding (160, 3, 16, 16) is NOT
    # routed through the group (net.HipBackendProjections): the k = 16 form runs in the operator tests above, not in the step.
    assert ran == [("convt", (160, 80, 2, 2)), ("conv", (256, 160, 1, 1)), ("conv", (256, 160, 1, 1)), ("conv", (256, 160, 1, 1)),
                   ("conv", (256, 160, 1, 1)), ("convt", (256, 256, 2, 2)), ("conv", (256, 256, 1, 1))]
    assert declined == [("conv", (256, 80, 1, 1))] * 3
    check_step_against_golden(z, model, step, losses, total, "cuda", "PROJECTIONS step (%s)" % "+".join(names))
