"""GPU: the half-precision training linears -- hipie_half_pack / hipie_act_half (csrc/half_pack.hip), hipie_gemm_batched_f16, the wrappers of
hipie_amd/ops_half.py, the nodes over them (functions.HalfLinearFunction / HalfMlpFunction) and the precision policy net.half_policy.

References: the host restatement of tests/_half_linear_cases.py for the kernels (bit for bit); for the nodes float64 on the CPU, twice:
the exact product of the fp16-ROUNDED operands (bound 5e-6, _grad_scale_cases.BOUND: only fp32 accumulation separates the two) and the
product of the unrounded operands (bound 1e-3, the plain-fp16 case of tests/test_gpu_gemm.py; the emulation of test_half_linears_cpu.py
leaves 2.7 x room).  Metric: util.rel_err = max|got - ref| / max|ref| per tensor.  The gradients are linear in dy and every gain is a power
of two, so the float64 references of a shape are computed once at g = 1 and multiplied by g; the MLP's rounded reference is formed per run
from the operands the node rounded (_mlp_rounded).  Every case prints its figures (lines starting with HLC) before it asserts.

Module level: the bound is 2 x the worst value measured on the MI355X (_half_linear_cases.MODULE_WORST: 1.175e-01 for net.vit_backbone,
1.398e-01 for net.encoder_layer, while the outputs agree to 3.4e-4).  Those worst values are single gradient elements behind a kink --
relu'(u) of a hidden element at zero, the argmax of the max pool behind res5 -- that a 2^-11 change of the forward flips; they are not the
rounding error of a product (that is what the node tests bound).  The 2-norm of the same differences is printed next to them."""
import ctypes
import functools

import pytest
import torch

import _half_linear_cases as H
from _train_step_cases import train_step_case
from hipie_amd import _lib, ops, ops_half
from hipie_amd.training import functions, net
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
F = torch.nn.functional


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


def _same_bits(a, b):
    view = lambda t: t.cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(view(a), view(b))


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


# ------------------------------------------------------------------------------------------------ the pack kernel
@pytest.mark.parametrize("scaled", (False, True), ids=("s=1", "grad_scale"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("from_f32", "from_f16"))
@pytest.mark.parametrize("rows,N,strided", [(r, n, False) for r, n in H.PACK_SHAPES] + [(300, 96, True)])
def test_pack_matches_the_host_restatement_bit_for_bit(rows, N, strided, dtype, scaled):
    g = torch.Generator().manual_seed(rows + N)
    host = torch.randn(rows, N, generator=g) * (3e-6 if scaled else 3.0)      # 3e-6: unscaled fp16 of this is subnormal, the scale matters
    saturating = not scaled and dtype is torch.float32
    if saturating:
        host[3, 5], host[rows - 1, N - 1] = 7e4, -7e4                          # beyond fp16: both saturate
    host = host.to(dtype)
    if strided:
        base = torch.full((rows, N + 8), 7e3, dtype=dtype, device=DEV)       # the columns beside the view would move the scale and the sums
        base[:, :N] = host.to(DEV)
        x = base[:, :N]
    else:
        x = host.to(DEV)
    rows_p = -(-rows // 64) * 64
    s = 1.0
    block = None
    if scaled:
        s, inv = H.scale_of(host.float())
        block = ops.grad_scale(x.float())
        assert _same_bits(block, torch.tensor((s, inv), dtype=torch.float32))
    want_r, want_t = H.half_rows(host.float(), s), H.half_t(host.float(), s)
    ws_bytes = ops._size("hipie_half_pack_ws_bytes", rows_p, N)
    assert ws_bytes == -(-rows_p // 128) * N * 4
    rbuf, r = _guarded(rows * N, torch.float16, -7.0)
    tbuf, t = _guarded(N * rows_p, torch.float16, -7.0)
    dbuf, db = _guarded(N, torch.float32, 12345.0)
    wbuf, ws = _guarded(ws_bytes // 4, torch.float32, 12345.0)

    def pack(pr, pt, pdb):
        ops._call("hipie_half_pack", x.data_ptr(), x.stride(0), ops._DT[dtype], None if block is None else block.data_ptr(), pr, N, pt, rows_p, pdb,
                  ws.data_ptr() if pdb else None, rows, N, rows_p)
    pack(r.data_ptr(), t.data_ptr(), db.data_ptr())
    r2, t2 = r.view(rows, N), t.view(N, rows_p)
    assert _same_bits(r2, want_r)                                               # (a) the rows
    assert _same_bits(t2, want_t) and not bool(t2[:, rows:].any())              # (b) the transpose with its zero pad columns
    if saturating:
        assert float(r2[3, 5]) == 65504.0 and float(t2[N - 1, rows - 1]) == -65504.0
    want = host.double().sum(0)                                                 # (c) the column sums, from the UNSCALED values
    err = (db.cpu().double() - want).abs()
    bound = H.column_sum_bound(host.float())
    print("HLC pack (%d, %d)%s %s s=2^%d: db max err %.2e (bound %.2e at that column), max|db| %.2e" % (
        rows, N, " strided" if strided else "", str(dtype)[6:], round(torch.log2(torch.tensor(s)).item()), float(err.max()), float(bound[err.argmax()]),
        float(want.abs().max())))
    assert bool((err <= bound).all())
    for buf, n, fill in ((rbuf, r.numel(), -7.0), (tbuf, t.numel(), -7.0), (dbuf, N, 12345.0), (wbuf, ws.numel(), 12345.0)):
        assert _guards_intact(buf, n, fill)
    # the same bits on a second call; each output ALONE (the other pointers NULL) has the same bits and leaves the other buffers untouched
    keep = (r.clone(), t.clone(), db.clone())
    pack(r.data_ptr(), t.data_ptr(), db.data_ptr())
    assert _same_bits(r, keep[0]) and _same_bits(t, keep[1]) and _same_bits(db, keep[2])
    for on in range(3):
        r.fill_(-7.0), t.fill_(-7.0), db.fill_(12345.0)
        pack(r.data_ptr() if on == 0 else None, t.data_ptr() if on == 1 else None, db.data_ptr() if on == 2 else None)
        for i, (got, kept, fill) in enumerate(((r, keep[0], -7.0), (t, keep[1], -7.0), (db, keep[2], 12345.0))):
            assert _same_bits(got, kept) if i == on else bool((got == fill).all()), (on, i)
        for buf, n, fill in ((rbuf, r.numel(), -7.0), (tbuf, t.numel(), -7.0), (dbuf, N, 12345.0)):
            assert _guards_intact(buf, n, fill)
    # all pointers NULL launches nothing (the workspace would be written by a launch that took db's branch; nothing else can show)
    r.fill_(-7.0), t.fill_(-7.0), db.fill_(12345.0), ws.fill_(12345.0)
    ops._call("hipie_half_pack", x.data_ptr(), x.stride(0), ops._DT[dtype], None, None, N, None, rows_p, None, None, rows, N, rows_p)
    assert all(bool((b == f).all()) for b, f in ((rbuf, -7.0), (tbuf, -7.0), (dbuf, 12345.0), (wbuf, 12345.0)))
    # the wrapper
    wr, wt, wdb = ops_half.half_pack(x, block, want_bias=True)
    assert _same_bits(wr, keep[0].view(rows, N)) and _same_bits(wt, keep[1].view(N, rows_p)) and _same_bits(wdb, keep[2])
    assert ops_half.half_pack(x, block, want_rows=False, want_t=False) == (None, None, None)
    only_t = ops_half.half_pack(x, block, want_rows=False)
    assert only_t[0] is None and only_t[2] is None and _same_bits(only_t[1], wt)


@pytest.mark.parametrize("act", (ops.ACT_GELU, ops.ACT_RELU), ids=("gelu", "relu"))
@pytest.mark.parametrize("rows,N", ((300, 96), (257, 320)))
def test_act_half_is_the_rounded_forward_activation(rows, N, act):
    u = (torch.randn(rows, N, generator=torch.Generator().manual_seed(rows + act)) * 3.0).to(DEV)
    u[0, :4] = torch.tensor([0.0, -0.0, 1e5, -1e5], device=DEV)                   # GELU(1e5) = 1e5: beyond fp16, inf like the library's cast
    abuf, a = _guarded(rows * N, torch.float16, -7.0)
    ops._call("hipie_act_half", u.data_ptr(), a.data_ptr(), rows, N, int(act))
    want = ops.act_forward(u, act).half()
    assert _same_bits(a.view(rows, N), want) and _guards_intact(abuf, a.numel(), -7.0)
    assert _same_bits(ops_half.act_half(u, act), want) and _same_bits(ops_half.act_half(u.view(rows, 2, N // 2), act), want.view(rows, 2, N // 2))


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
def test_refusals_through_the_c_abi_launch_nothing():
    lib = _lib.load()
    x = torch.randn(64, 32, device=DEV)
    rbuf, r = _guarded(64 * 32, torch.float16, -7.0)
    tbuf, t = _guarded(32 * 64, torch.float16, -7.0)
    dbuf, db = _guarded(32, torch.float32, 12345.0)
    wbuf, ws = _guarded(32, torch.float32, 12345.0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def pack(ldx=32, ldo=32, ldt=64, rows=64, N=32, rows_p=64, x_ptr=x.data_ptr(), r_ptr=r.data_ptr()):
        return lib.hipie_half_pack(x_ptr, ldx, 0, None, r_ptr, ldo, t.data_ptr(), ldt, db.data_ptr(), ws.data_ptr(), rows, N, rows_p, st)
    for kw in ({"rows_p": 96}, {"rows_p": 32, "rows": 32}, {"N": 36, "ldx": 36, "ldo": 40}, {"x_ptr": x.data_ptr() + 4}, {"r_ptr": r.data_ptr() + 2},
               {"ldx": 30}, {"ldt": 60}):
        assert pack(**kw) == -22 and b"half_pack" in lib.hipie_last_error(), kw
    a16 = torch.randn(256, 128, device=DEV).half()
    out = torch.full((2, 256, 256), 12345.0, device=DEV)

    def gemm(K=64, A=a16.data_ptr()):
        return lib.hipie_gemm_batched_f16(A, 128, 0, K, a16.data_ptr(), 128, 0, K, out.data_ptr(), 256, 0, 256 * 256, 1, 2, 256, 256, K, 1.0, None, st)
    assert gemm(K=96) == -22 and b"K=96" in lib.hipie_last_error()               # K % 64
    assert gemm(K=32) == -22 and gemm(A=a16.data_ptr() + 2) == -22
    abuf, a = _guarded(64 * 32, torch.float16, -7.0)
    assert lib.hipie_act_half(x.data_ptr(), a.data_ptr(), 64, 36, 1, st) == -22 and lib.hipie_act_half(x.data_ptr(), a.data_ptr() + 2, 64, 32, 1, st) == -22
    torch.cuda.synchronize()
    for buf, fill in ((rbuf, -7.0), (tbuf, -7.0), (dbuf, 12345.0), (wbuf, 12345.0), (abuf, -7.0), (out, 12345.0)):
        assert bool((buf == fill).all())


# ------------------------------------------------------------------------------------------------ the batched F16 GEMM
@pytest.mark.parametrize("M,N,K,nk", ((64, 192, 1024, 16), (320, 256, 384, 2)))
def test_batched_f16_gemm_has_the_bits_of_hipie_gemm_on_the_chunks(M, N, K, nk):
    g = torch.Generator().manual_seed(M + nk)
    a, w = torch.randn(M, K, generator=g).half().to(DEV), (torch.randn(N, K, generator=g) * K ** -0.5).half().to(DEV)
    Kc = K // nk
    part = ops_half.gemm_split_k_half(a, w, nk, None, want_parts=True)
    assert part.shape == (nk, M, N)
    for k in range(nk):
        want = ops.gemm(a[:, k * Kc:(k + 1) * Kc], w[:, k * Kc:(k + 1) * Kc].contiguous(), split=False)
        assert torch.equal(part[k], want), k
    # a NULL alpha_dev is a block holding 1.0; a power of two scales exactly; the sum is in chunk order
    blk = torch.tensor([4.0, 1.0, 0.25], device=DEV)
    pbuf, p1 = _guarded(nk * M * N, torch.float32, 12345.0)
    ops._call("hipie_gemm_batched_f16", a.data_ptr(), K, 0, Kc, w.data_ptr(), K, 0, Kc, p1.data_ptr(), N, 0, M * N, 1, nk, M, N, Kc, 1.0, blk[1:2].data_ptr())
    assert torch.equal(p1.view(nk, M, N), part) and _guards_intact(pbuf, p1.numel(), 12345.0)
    ops._call("hipie_gemm_batched_f16", a.data_ptr(), K, 0, Kc, w.data_ptr(), K, 0, Kc, p1.data_ptr(), N, 0, M * N, 1, nk, M, N, Kc, 2.0, blk[2:].data_ptr())
    assert torch.equal(p1.view(nk, M, N), part * 0.5)
    want = part[0]
    for k in range(1, nk):
        want = want + part[k]
    assert torch.equal(ops_half.gemm_split_k_half(a, w, nk), want) and torch.equal(ops_half.gemm_split_k_half(a, w, nk, blk[2:]), want * 0.25)
    ref = a.double().cpu() @ w.double().cpu().t()
    e = rel_err(want.cpu(), ref)
    print("HLC batched f16 (%d, %d, %d) nk=%d against float64 of the same fp16 operands: %.2e" % (M, N, K, nk, e))
    assert e < H.ROUNDED_BOUND
    assert torch.equal(ops_half.gemm_split_k_half(a, w, 1, blk[2:]), ops.gemm(a, w, split=False) * 0.25)          # one chunk: the product itself


# ------------------------------------------------------------------------------------------------ the nodes against float64
LIN_NAMES = ("y", "dx", "dW", "db")
MLP_NAMES = ("y", "dx", "dW1", "db1", "dW2", "db2")


@functools.lru_cache(maxsize=None)
def _linear_case(M, N, K):
    """x, W, b, dy at g = 1 and, at g = 1, (y, dx, dW, db) in float64 of the UNROUNDED operands and of the ROUNDED ones (dy rounded after
    its scale: every g is a power of two, so fp16(s dy) / s at g = 1 is what every gain sees), computed once per shape"""
    x, w, dy = H.linear_problem(M, N, K, 1.0, seed=M + N + K)
    b = torch.randn(N, generator=torch.Generator().manual_seed(N))
    xd, wd, dyd = x.double(), w.double(), dy.double()
    exact = (xd @ wd.t() + b.double(), dyd @ wd, dyd.t() @ xd, dyd.sum(0))
    s, inv = H.scale_of(dy)
    rounded = (H.half_product(x, w) + b.double(), H.half_product(dy * s, w.t()) * inv, H.half_product((dy * s).t(), x.t()) * inv, dyd.sum(0))
    return x, w, b, dy, exact, rounded


@functools.lru_cache(maxsize=None)
def _mlp_case(M, N, K, bias=True):
    """x (M, K), W1 (N, K), b1, W2 (K, N), b2, the cotangent at g = 1 and float64 autograd of linear -> GELU -> linear on the unrounded
    operands: (y, dx, dW1, db1, dW2, db2), computed once per shape"""
    g = torch.Generator().manual_seed(7 * M + N + K)
    x = torch.randn(M, K, generator=g)
    w1, b1 = torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g) * 0.5
    w2, b2 = torch.randn(K, N, generator=g) * N ** -0.5, torch.randn(K, generator=g) * 0.5
    dy = torch.randn(M, K, generator=g)
    if not bias:
        b1 = b2 = None
    leaves = [None if t is None else t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = F.linear(F.gelu(F.linear(leaves[0], leaves[1], leaves[2])), leaves[3], leaves[4])
    grads = iter(torch.autograd.grad(y, [t for t in leaves if t is not None], dy.double()))
    return (x, w1, b1, w2, b2), dy, (y.detach(),) + tuple(None if t is None else next(grads) for t in leaves)


class _Recorder:
    """what the MLP node feeds its GEMMs: the inputs (and scale blocks) of every ops_half.half_pack call and the (u, a16) of act_half, in call
    order.  The fp16 operands of the node's products are a pure function of these (the pack test holds the kernel to the host restatement)."""

    def __init__(self, monkeypatch):
        self.packs, self.acts = [], []
        real_pack, real_act = ops_half.half_pack, ops_half.act_half

        def pack(x, scale=None, **kw):
            self.packs.append((x.detach().float().cpu(), None if scale is None else float(scale[0])))
            return real_pack(x, scale, **kw)

        def act(u, a):
            out = real_act(u, a)
            self.acts.append((u.detach().cpu(), out.cpu()))
            return out
        monkeypatch.setattr(ops_half, "half_pack", pack)
        monkeypatch.setattr(ops_half, "act_half", act)


def _mlp_rounded(rec, tensors, dy):
    """the node's arithmetic in float64 on the operands it rounded: every product is the exact product of its fp16 operands.  The
    intermediate results that are rounded again (u -> a16, du -> fp16(su du)) are the device's own: a host value 1e-7 away rounds to the
    neighbouring fp16 number in one element of a few thousand, which is 2^-11 of that element, not an accumulation error."""
    x, w1, b1, w2, b2 = tensors
    (xr, _), (dyr, sy), (ar, _), (dur, su), (x16r, _) = rec.packs
    (u, a16), = rec.acts
    half = lambda t, s=1.0: H.half(t, s).double() / s
    assert torch.equal(xr, x) and torch.equal(x16r, H.half(x).float()) and torch.equal(H.half(ar), a16)       # the recomputed a rounds to the forward's a16
    w1h, w2h, x16, g16, u16 = half(w1), half(w2), half(x), half(dyr, sy), half(dur, su)
    u_ref = x16 @ w1h.t() + (0 if b1 is None else b1.double())
    ud = u.double().requires_grad_(True)
    du_ref = torch.autograd.grad(F.gelu(ud), ud, g16 @ w2h)[0]
    e_u, e_du = rel_err(u, u_ref), rel_err(dur, du_ref)
    print("HLC   mlp intermediates vs rounded: u %.2e du %.2e" % (e_u, e_du))
    assert e_u < H.ROUNDED_BOUND and e_du < H.ROUNDED_BOUND
    return (a16.double() @ w2h.t() + (0 if b2 is None else b2.double()), u16 @ w1h, u16.t() @ x16, None if b1 is None else dur.double().sum(0),
            g16.t() @ a16.double(), None if b2 is None else dy.double().sum(0))


def _run_linear(fn, x, w, b, dy, frozen=()):
    leaves = [None if t is None else t.to(DEV).requires_grad_(i not in frozen) for i, t in enumerate((x, w, b))]
    owner = type("_W", (), {})()
    y = fn(leaves[0], leaves[1], leaves[2], owner, "w")
    wanted = [t for t in leaves if t is not None and t.requires_grad]
    got = iter(torch.autograd.grad(y, wanted, dy.to(DEV)))
    return [y.detach()] + [None if t is None or not t.requires_grad else next(got) for t in leaves]


def _run_mlp(fn, tensors, dy, frozen=()):
    leaves = [None if t is None else t.to(DEV).requires_grad_(i not in frozen) for i, t in enumerate(tensors)]
    y = fn(*leaves, ops.ACT_GELU)
    wanted = [t for t in leaves if t is not None and t.requires_grad]
    got = iter(torch.autograd.grad(y, wanted, dy.to(DEV)))
    return [y.detach()] + [None if t is None or not t.requires_grad else next(got) for t in leaves]


def _check_against(label, kind, got, ref, g, names, bound):
    """g = None: ref is at the gain of got; else ref is at g = 1 and the forward (index 0) does not scale"""
    errs = {n: rel_err(a.cpu(), r if g is None or i == 0 else r * g) for i, (n, a, r) in enumerate(zip(names, got, ref)) if a is not None}
    print("HLC %s vs %s: %s" % (label, kind, " ".join("%s %.2e" % kv for kv in errs.items())))
    for n, e in errs.items():
        assert e < bound, (label, kind, n, e)


GAIN_IDS = ["g=2^%d" % round(torch.log2(torch.tensor(g)).item()) for g in H.GAINS]


@pytest.mark.parametrize("g", H.GAINS, ids=GAIN_IDS)
@pytest.mark.parametrize("M,N,K", H.SHAPES)
def test_half_linear_against_float64_at_every_magnitude(M, N, K, g):
    """with bias, without, with frozen x and with frozen W; the node, not the fall-through, ran (the counter its forward keeps)"""
    x, w, b, dy, exact, rounded = _linear_case(M, N, K)
    before = functions.HALF_NODE_CALLS["linear"]
    dyg = dy * g
    full = _run_linear(functions.half_linear, x, w, b, dyg)
    label = "linear (%d,%d,%d) g=%.1e" % (M, N, K, g)
    _check_against(label, "rounded", full, rounded, g, LIN_NAMES, H.ROUNDED_BOUND)
    _check_against(label, "unrounded", full, exact, g, LIN_NAMES, H.UNROUNDED_BOUND)
    nob = _run_linear(functions.half_linear, x, w, None, dyg)
    assert nob[3] is None and torch.equal(nob[1], full[1]) and torch.equal(nob[2], full[2])
    _check_against(label + " no bias", "rounded", nob[:1], (rounded[0] - b.double(),), g, LIN_NAMES, H.ROUNDED_BOUND)
    for frozen in ((0,), (1,)):
        part = _run_linear(functions.half_linear, x, w, b, dyg, frozen)
        assert part[1 + frozen[0]] is None and all(p is None or torch.equal(p, f) for p, f in zip(part, full)), frozen
    assert functions.HALF_NODE_CALLS["linear"] - before == 4


@pytest.mark.parametrize("g", H.GAINS, ids=GAIN_IDS)
@pytest.mark.parametrize("M,N,K", H.SHAPES)
def test_half_mlp_against_float64_at_every_magnitude(M, N, K, g, monkeypatch):
    before = functions.HALF_NODE_CALLS["mlp"]
    for bias in (True, False):
        tensors, dy, exact = _mlp_case(M, N, K, bias)
        dyg = dy * g
        label = "mlp (%d,%d,%d) g=%.1e%s" % (M, N, K, g, "" if bias else " no bias")
        with monkeypatch.context() as mp:
            rec = _Recorder(mp)
            got = _run_mlp(functions.half_mlp, tensors, dyg)
        _check_against(label, "rounded", got, _mlp_rounded(rec, tensors, dyg), None, MLP_NAMES, H.ROUNDED_BOUND)
        _check_against(label, "unrounded", got, exact, g, MLP_NAMES, H.UNROUNDED_BOUND)
        if bias:
            full = got
    tensors, dy, _ = _mlp_case(M, N, K)
    dyg = dy * g
    for frozen in ((0,), (1, 3), (2, 4)):
        part = _run_mlp(functions.half_mlp, tensors, dyg, frozen)
        assert all(part[1 + i] is None for i in frozen) and all(p is None or torch.equal(p, f) for p, f in zip(part, full)), frozen
    assert functions.HALF_NODE_CALLS["mlp"] - before == 5


@pytest.mark.parametrize("M,N,K", H.SHAPES)
def test_scale_invariance_bit_for_bit(M, N, K):
    """every scaling is by an exact power of two and no sum's order depends on the values: the results for 2^e dy are 2^e times the results
    for dy, with no tolerance, for every gradient of both nodes; and two calls on the same input give the same bits"""
    x, w, b, dy = _linear_case(M, N, K)[:4]
    tensors, dym = _mlp_case(M, N, K)[:2]
    lin = _run_linear(functions.half_linear, x, w, b, dy)
    mlp = _run_mlp(functions.half_mlp, tensors, dym)
    assert all(torch.equal(a, c) for a, c in zip(lin, _run_linear(functions.half_linear, x, w, b, dy)))
    assert all(torch.equal(a, c) for a, c in zip(mlp, _run_mlp(functions.half_mlp, tensors, dym)))
    for e in H.INVARIANCE_EXPONENTS:
        f = 2.0 ** e
        for name, a, c in list(zip(LIN_NAMES, _run_linear(functions.half_linear, x, w, b, dy * f), lin))[1:]:
            assert torch.equal(a, c * f), ("linear", e, name)
        for name, a, c in list(zip(MLP_NAMES, _run_mlp(functions.half_mlp, tensors, dym * f), mlp))[1:]:
            assert torch.equal(a, c * f), ("mlp", e, name)


def test_a_linear_outside_the_conditions_has_the_bits_of_the_split_node():
    """K = 96 under the policy: HipBackend.linear's bits, forward and backward, and no half node"""
    g = torch.Generator().manual_seed(4)
    x, w, b, dy = torch.randn(300, 96, generator=g), torch.randn(128, 96, generator=g) * 0.1, torch.randn(128, generator=g), torch.randn(300, 128, generator=g)
    before = dict(functions.HALF_NODE_CALLS)
    be = net.half_policy(net.HipBackend)
    out = []
    for f in (be.linear_half, net.HipBackend.linear):
        sd = {"l.weight": w.to(DEV).requires_grad_(True), "l.bias": b.to(DEV).requires_grad_(True)}
        xd = x.to(DEV).requires_grad_(True)
        y = f(xd, sd, "l.")
        out.append((y.detach(),) + torch.autograd.grad(y, (xd, sd["l.weight"], sd["l.bias"]), dy.to(DEV)))
    assert all(torch.equal(a, c) for a, c in zip(*out)) and dict(functions.HALF_NODE_CALLS) == before
    sd = {"l.weight": w.to(DEV), "l.bias": b.to(DEV)}
    assert torch.equal(net._blin(x.to(DEV), sd, "l.", be), out[1][0])


# ------------------------------------------------------------------------------------------------ module level, no discrete decisions
def _leaf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV).requires_grad_(True)


def _module_errors(label, run, sd, inputs):
    """rel_err per output and per parameter gradient of run(be) under the policy against run(reference backend); gradients finite, and
    non-zero where the reference's are"""
    results = []
    for be in ("ref", "half"):
        outs = run(be)
        cots = [torch.randn(o.shape, generator=torch.Generator().manual_seed(11 + i)).to(DEV) for i, o in enumerate(outs)]
        leaves = list(sd.values()) + inputs
        grads = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), leaves, allow_unused=True)
        results.append(([o.detach().cpu() for o in outs], [None if g is None else g.cpu() for g in grads]))
    (ro, rg), (ho, hg) = results
    errs = {"out%d" % i: rel_err(h, r) for i, (h, r) in enumerate(zip(ho, ro))}
    l2 = {}
    for name, h, r in zip(list(sd) + ["input%d" % i for i in range(len(inputs))], hg, rg):
        assert (h is None) == (r is None), name
        if r is not None:
            assert bool(torch.isfinite(h).all()), name
            assert bool((h != 0).any()) or not bool((r != 0).any()), name
            if bool((r != 0).any()):
                errs["d " + name] = rel_err(h, r)
                l2["d " + name] = float((h.double() - r.double()).norm() / r.double().norm())
    worst = max(errs.items(), key=lambda kv: kv[1])
    worst2 = max(l2.items(), key=lambda kv: kv[1])
    # the figure next to the asserted one (printed only): the same difference in the 2-norm, which a handful of elements does not set
    print("HLC module %s: worst %.3e (%s) of %d tensors; outputs %s; gradients in the 2-norm: worst %.3e (%s)" % (
        label, worst[1], worst[0], len(errs), " ".join("%.2e" % errs[k] for k in errs if k.startswith("out")), worst2[1], worst2[0]))
    return worst[1]


def _assert_module_bound(name, worst):
    recorded = H.MODULE_WORST[name]
    assert recorded is not None, "%s: measured %.3e, no value recorded in _half_linear_cases.MODULE_WORST" % (name, worst)
    assert worst < 2.0 * recorded, (name, worst, recorded)


def test_vit_backbone_under_the_policy():
    """width 128, MLP 512, 2 heads, depth 2 (block 0 in 8 x 8 windows, block 1 global), a 16 x 16 token grid, one image = 256 rows: every ViT
    linear takes a half node.  Reference: the same function with be=None (library fp32 under autograd)."""
    g = torch.Generator().manual_seed(31)
    C, Hd, heads, p = 128, 512, 2, "v."
    sd = {p + "patch_embed.proj.weight": _leaf(g, C, 3, 4, 4, scale=0.2), p + "patch_embed.proj.bias": _leaf(g, C, scale=0.1),
          p + "pos_embed": _leaf(g, 1, 257, C, scale=0.2), p + "fpn1.0.weight": _leaf(g, C, 32, 2, 2, scale=0.1), p + "fpn1.0.bias": _leaf(g, 32, scale=0.1)}
    for i, size in enumerate((8, 16)):
        bp = "%sblocks.%d." % (p, i)
        for n in ("norm1.", "norm2."):
            sd[bp + n + "weight"], sd[bp + n + "bias"] = (1.0 + _leaf(g, C, scale=0.1)).detach().requires_grad_(True), _leaf(g, C, scale=0.1)
        sd[bp + "attn.qkv.weight"], sd[bp + "attn.qkv.bias"] = _leaf(g, 3 * C, C, scale=C ** -0.5), _leaf(g, 3 * C, scale=0.1)
        sd[bp + "attn.proj.weight"], sd[bp + "attn.proj.bias"] = _leaf(g, C, C, scale=C ** -0.5), _leaf(g, C, scale=0.1)
        sd[bp + "attn.rel_pos_h"], sd[bp + "attn.rel_pos_w"] = _leaf(g, 2 * size - 1, C // heads, scale=0.1), _leaf(g, 2 * size - 1, C // heads, scale=0.1)
        sd[bp + "mlp.fc1.weight"], sd[bp + "mlp.fc1.bias"] = _leaf(g, Hd, C, scale=C ** -0.5), _leaf(g, Hd, scale=0.1)
        sd[bp + "mlp.fc2.weight"], sd[bp + "mlp.fc2.bias"] = _leaf(g, C, Hd, scale=Hd ** -0.5), _leaf(g, C, scale=0.1)
    cfg = {"vit_patch": 4, "vit_depth": 2, "vit_window": 8, "vit_window_blocks": [0], "vit_heads": heads}
    img = _leaf(g, 1, 3, 64, 64)
    half = net.half_policy(net.backend("mlp"))
    before = dict(functions.HALF_NODE_CALLS)

    def run(be):
        out = net.vit_backbone(img, sd, p, cfg, None if be == "ref" else half)
        return [out["res3"], out["res4"], out["res5"]]
    worst = _module_errors("vit_backbone", run, sd, [img])
    assert functions.HALF_NODE_CALLS["linear"] - before.get("linear", 0) == 4 and functions.HALF_NODE_CALLS["mlp"] - before.get("mlp", 0) == 2
    _assert_module_bound("vit_backbone", worst)


def test_encoder_layer_under_the_policy():
    """one deformable encoder layer at 340 tokens (4 levels from 16 x 16 down), width 256, FFN 512: the FFN takes the half MLP node.
    Reference: the same function on a backend that has HipBackend's msda and no linear op, so every linear is the library's fp32."""
    g = torch.Generator().manual_seed(37)
    C, Hd, p = 256, 512, "e."
    shapes = [(16, 16), (8, 8), (4, 4), (2, 2)]
    S = sum(h * w for h, w in shapes)
    sd = {}
    for n, (o, i), sc in (("self_attn.value_proj.", (C, C), C ** -0.5), ("self_attn.sampling_offsets.", (256, C), 0.02), ("self_attn.attention_weights.", (128, C), 0.05),
                          ("self_attn.output_proj.", (C, C), C ** -0.5), ("linear1.", (Hd, C), C ** -0.5), ("linear2.", (C, Hd), Hd ** -0.5)):
        sd[p + n + "weight"], sd[p + n + "bias"] = _leaf(g, o, i, scale=sc), _leaf(g, o, scale=0.1)
    for n in ("norm1.", "norm2."):
        sd[p + n + "weight"], sd[p + n + "bias"] = (1.0 + _leaf(g, C, scale=0.1)).detach().requires_grad_(True), _leaf(g, C, scale=0.1)
    src, pos = _leaf(g, 1, S, C), _leaf(g, 1, S, C, scale=0.5)
    refs = net.encoder_ref_points(shapes, torch.ones(1, 4, 2, device=DEV))
    reference = type("MsdaOnly", (), {"msda": net.HipBackend.msda})
    half = net.half_policy(net.backend("mlp"))
    before = functions.HALF_NODE_CALLS["mlp"]

    def run(be):
        return [net.encoder_layer(src, pos, refs, shapes, None, sd, p, reference if be == "ref" else half)]
    worst = _module_errors("encoder_layer", run, sd, [src, pos])
    assert functions.HALF_NODE_CALLS["mlp"] - before == 1
    _assert_module_bound("encoder_layer", worst)


# ------------------------------------------------------------------------------------------------ the whole step
def test_step_under_the_policy_runs_and_every_gradient_is_finite():
    """the train_step_tiny fixture under net.half_policy(net.backend("mlp")).  NO accuracy bound against the golden here: the step contains
    top-k selections and three matchers, and a 2^-11 change of the features can flip a discrete choice and move the losses by a finite
    amount -- a bound would test the fixture's luck.  The differences are printed; measured on the MI355X (docs/measurements.md): total
    466.633 against the golden's 467.362, worst loss entry 1.0e-2 (loss_mask), parameter gradients worst 2.5e-1 (a sampling_offsets
    weight), median 1.9e-2."""
    be = net.half_policy(net.backend("mlp"))
    before = dict(functions.HALF_NODE_CALLS)
    z, meta, model, step, batch, targets = train_step_case(DEV, be)
    assert step.be is be
    losses = step.loss_dict(batch, targets)
    total = sum(losses.values())
    total.backward()
    assert step.draws.calls == int(z["n_rand"])
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()) and bool(torch.isfinite(total))
    ran = {k: functions.HALF_NODE_CALLS[k] - before.get(k, 0) for k in ("linear", "mlp")}
    # the fixture's ViT is 160 wide (K % 64 != 0): its linears and MLPs fall through to the split nodes; the FFNs of its four encoder layers
    # (256 <-> 256) take the half MLP node
    assert ran["linear"] + ran["mlp"] > 0 and ran["mlp"] > 0, ran
    with_grad = 0
    for name, prm in model.named_parameters():
        if prm.requires_grad and prm.grad is not None:
            assert bool(torch.isfinite(prm.grad).all()), name
            with_grad += 1
    assert with_grad > 400
    want = {k[5:]: float(z[k]) * float(z["weight/" + k[5:]]) for k in z.files if k.startswith("loss/")}
    worst_l = max((abs(float(losses[k]) - want[k]) / max(1.0, abs(want[k])), k) for k in want)
    import json
    steps = json.loads(bytes(z["grad_steps"]).decode())
    params = dict(model.named_parameters(remove_duplicate=False))
    errs = []
    for k in z.files:
        if k.startswith("grad/"):
            prm = params[k[5:]]
            gr = (torch.zeros_like(prm) if prm.grad is None else prm.grad).reshape(-1).cpu()
            gr = gr[::steps[k[5:]]] if k[5:] in steps else gr
            wv = torch.from_numpy(z[k])
            errs.append((float((gr - wv).abs().max() / (wv.abs().max() + 1e-12)), k[5:]))
    errs.sort(reverse=True)
    print("HLC step under the policy: half linear nodes %d, half MLP nodes %d; total %.5f (golden %.5f), worst loss entry %.2e (%s); parameter "
          "gradients against the golden: worst %.2e (%s), median %.2e" % (ran["linear"], ran["mlp"], float(total), float(z["total"]), worst_l[0], worst_l[1],
                                                                         errs[0][0], errs[0][1], errs[len(errs) // 2][0]))
