"""GPU: hipie_bi_attn_train_forward / hipie_bi_attn_train_backward (csrc/bi_attn_train.hip) through ops.bi_attn_train_forward /
ops.bi_attn_train_backward, the autograd Function over them and the opt-in HipBackendFusionAttention wiring of the training step.

Reference: the float64 statements of tests/_fusion_attention_cases.py (checked against torch.autograd in test_fusion_attention_cpu.py).
Metric: max|got - ref64| / max|ref64| per tensor (a tensor that is exactly zero in the reference has to be exactly zero).  Bound per case and
tensor: max(1e-5, 4 x e_lib), e_lib = the same metric for torch's fp32 materialised formulation and its autograd on the same device (the
log-sum-exps, which that formulation does not produce: 1e-5).  Every case prints its figures (lines starting with FAT) before it asserts.

Worst figures measured on one MI355X: see docs/measurements.md (training fusion attention)."""
import pytest
import torch

from _fusion_attention_cases import HD, backward64, block_case, clamp_case, forward64, masks_for, operands, torch_graph
from _train_step_cases import check_step_against_golden, train_step_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H = 2, 2
E = H * HD
NAMES = ("out_v", "out_l", "d_q", "d_k", "d_vv", "d_vl")


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float((got - ref).abs().max() / top)


def _check(tag, got, ref64, lib32, names=NAMES):
    fails = []
    for n, g, r, l in zip(names, got, ref64, lib32):
        e, e_lib = _err(g, r), (0.0 if l is None else _err(l, r))
        bound = max(1e-5, 4 * e_lib)
        print("FAT %-30s %-5s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


def _lse_err(got, ref):
    """the metric over the finite entries; -inf has to sit where the reference has it"""
    inf = ref == float("-inf")
    assert torch.equal(got.cpu() == float("-inf"), inf)
    return _err(got.cpu().masked_fill(inf, 0.0), ref.masked_fill(inf, 0.0))


def _run(ops, t, att, r=0.0, seed=0, want=(True, True, True, True)):
    q, k, vv, vl, gv, gl = t
    out_v, out_l, lse_v, lse_l, st_v, st_l = ops.bi_attn_train_forward(q, k, vv, vl, att, H, r, seed)
    grads = ops.bi_attn_train_backward(q, k, vv, vl, att, out_v, out_l, st_v, st_l, gv, gl, H, r, seed, want)
    return (out_v, out_l) + grads, (lse_v, lse_l)


def _case(tag, t, att, r=0.0, seed=0):
    from hipie_amd import ops
    host = [x.cpu() for x in t]
    got, lse = _run(ops, t, att.to(DEV), r, seed)
    Nv, L = t[0].shape[1], t[1].shape[1]
    assert got[0].shape == (B, Nv, E) and got[1].shape == (B, L, E) and lse[0].shape == (B, H, Nv) and lse[1].shape == (B, H, L)
    assert all(g.is_contiguous() and bool(torch.isfinite(g).all()) for g in got)
    f64 = forward64(*host[:4], att, H, r, seed)
    ref = f64[:2] + backward64(*host[:4], att, H, host[4], host[5], r, seed)
    lib = torch_graph(*t[:4], att, H, t[4], t[5], torch.float32, DEV, r, seed)
    e_v, e_l = _lse_err(lse[0], f64[2]), _lse_err(lse[1], f64[3])
    print("FAT %-30s lse_v err %.3e  lse_l err %.3e  bound 1.000e-05" % (tag, e_v, e_l))
    assert e_v <= 1e-5 and e_l <= 1e-5
    _check(tag, got, ref, lib)
    return got, ref


# --------------------------------------------------------------------------------------------- the operator against float64
@pytest.mark.parametrize("mask", ["all", "prefix", "scattered"])
@pytest.mark.parametrize("Nv,L", [(1, 1), (33, 7), (130, 77), (300, 256)])
def test_operator_against_float64(Nv, L, mask):
    """a V workgroup is 32 visual rows x the whole text, a T workgroup 32 text rows x a segment of 128-row sweep steps.  (1, 1) a single row
    and column; (33, 7) a second visual block of one row, one partial text tile; (130, 77) two segments, the second of two rows, three text
    tiles (13 rows in the last); (300, 256) three segments, ten visual blocks, the full key tile (both tiles of every wave)"""
    got, _ = _case("Nv=%d L=%d %s" % (Nv, L, mask), operands(B, Nv, L, H, seed=1, dev=DEV), masks_for(B, L)[mask])
    # one row and one column: both probabilities are 1, d_q = d_k = 0 in exact arithmetic -- and exactly here (float64 leaves 1e-17 of its
    # two summation orders, so the relative metric says nothing at this shape)
    assert (Nv, L) != (1, 1) or (not bool(got[2].any()) and not bool(got[3].any()))


@pytest.mark.parametrize("Nv,L", [(33, 7), (130, 77)])
def test_operator_with_dropout(Nv, L):
    from hipie_amd import ops
    t, att, seed = operands(B, Nv, L, H, seed=2, dev=DEV), masks_for(B, L)["prefix"], 0x0123456789ABCDEF
    got, _ = _case("Nv=%d L=%d prefix r=0.1" % (Nv, L), t, att, 0.1, seed)
    plain, _ = _run(ops, t, att.to(DEV))
    assert not torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1])              # the masks entered


def test_clamped_rows():
    Nv, L = 33, 7
    t = clamp_case(B, Nv, L, H, seed=3, dev=DEV)
    att = masks_for(B, L)["all"]
    raw = HD ** -0.5 * torch.einsum("bihd,bjhd->bhij", t[0].double().cpu().view(B, Nv, H, HD), t[1].double().cpu().view(B, L, H, HD))
    assert bool((raw[:, :, 0] > 50000).all()) and bool((raw[:, :, 1] < -50000).all())
    got, ref = _case("clamp Nv=33 L=7", t, att)
    mean = t[3].double().cpu().view(B, L, H, HD).mean(1).reshape(B, E)
    for row in (0, 1):
        assert float((got[0][:, row].double().cpu() - mean).abs().max()) <= 1e-5 * float(mean.abs().max())
        assert not bool(got[2][:, row].any())                                                   # d_q exactly 0
    assert float((got[1].cpu() - t[2][:, :1].cpu()).abs().max()) <= 1e-5 * float(t[2][:, 0].abs().max())      # out_l = vv row 0


def test_an_image_without_attended_tokens():
    from hipie_amd import ops
    Nv, L = 33, 7
    t = operands(B, Nv, L, H, seed=4, dev=DEV)
    att = masks_for(B, L)["scattered"].clone()
    att[1] = False
    got, lse = _run(ops, t, att.to(DEV))
    assert not bool(got[0][1].any()) and bool((lse[0][1] == float("-inf")).all())
    assert all(bool(torch.isfinite(g).all()) for g in got) and bool(torch.isfinite(lse[1]).all()) and bool(torch.isfinite(lse[0][0]).all())
    host = [x.cpu() for x in t]
    ref = forward64(*host[:4], att, H)[:2] + backward64(*host[:4], att, H, host[4], host[5])
    only_l = backward64(*host[:4], att, H, host[4], host[5], directions=(False, True))
    assert torch.equal(ref[2][1], only_l[0][1]) and torch.equal(ref[3][1], only_l[1][1])       # the statement: image 1 has the one direction
    att0 = att.clone()
    att0[1] = True
    lib0 = torch_graph(*t[:4], att0, H, t[4], t[5], torch.float32, DEV)
    _check("masked image: image 0", [g[:1] for g in got], [r[:1] for r in ref], [x[:1] for x in lib0])
    # image 1: d_q and d_k are the text -> image direction's alone; the library has no such formulation: the floor of 1e-5 is the bound
    _check("masked image: image 1", [got[2][1], got[3][1], got[1][1], got[4][1]], [only_l[0][1], only_l[1][1], ref[1][1], ref[4][1]], [None] * 4,
           names=("d_q", "d_k", "out_l", "d_vv"))
    assert not bool(got[5][1].any())                                                            # no image -> text probability: d_vl = 0


# --------------------------------------------------------------------------------------------- the autograd Function
def _function_run(t, att, grad=(True, True, True, True), r=0.0, seed=None):
    from hipie_amd.training import functions
    leaves = [x.detach().requires_grad_(g) for x, g in zip(t[:4], grad)]
    y = functions.fusion_attention(*leaves, att, H, r, seed)
    assert y is not None and all(o.requires_grad == any(grad) for o in y)
    return leaves, y


def _backward(y, gv, gl):
    torch.autograd.backward(y, (gv, gl))


def test_function_forward_backward_and_frozen_inputs(monkeypatch):
    from hipie_amd import ops
    from hipie_amd.training import functions
    Nv, L = 130, 77
    t = operands(B, Nv, L, H, seed=5, dev=DEV)
    att = masks_for(B, L)["prefix"]
    ad = att.to(DEV)
    seen = []
    real = ops.bi_attn_train_backward

    def spy(*a):
        seen.append(tuple(a[-1]))
        return real(*a)
    monkeypatch.setattr(functions.ops, "bi_attn_train_backward", spy)
    leaves, y = _function_run(t, ad)
    saved = sorted(tuple(s.shape) for s in y[0].grad_fn.saved_tensors)
    assert saved == sorted([(B, Nv, E)] * 3 + [(B, L, E)] * 3 + [(B, H, Nv, 2), (B, H, L, 2), (B, L)])      # nothing of Nv x L elements
    _backward(y, t[4], t[5])
    host = [x.cpu() for x in t]
    _check("Function Nv=130 L=77 prefix", [x.grad for x in leaves], backward64(*host[:4], att, H, host[4], host[5]),
           torch_graph(*t[:4], att, H, t[4], t[5], torch.float32, DEV)[2:], names=NAMES[2:])
    full = [x.grad for x in leaves]
    for frozen in range(4):
        grad = tuple(x != frozen for x in range(4))
        leaves, y = _function_run(t, ad, grad)
        _backward(y, t[4], t[5])
        assert leaves[frozen].grad is None and all(torch.equal(x.grad, f) for n, (x, f) in enumerate(zip(leaves, full)) if n != frozen)
        assert seen[-1] == grad
    assert len(seen) == 5
    leaves, y = _function_run(t, ad, (False,) * 4)
    assert y[0].grad_fn is None and y[1].grad_fn is None and len(seen) == 5


def test_function_output_gradients_seeds_and_repeats():
    Nv, L = 130, 77
    t = operands(B, Nv, L, H, seed=6, dev=DEV)
    ad = masks_for(B, L)["scattered"].to(DEV)
    wide = torch.randn(B, Nv, E, 2, generator=torch.Generator().manual_seed(1)).to(DEV)
    view = wide[..., 0]                                                       # column stride 2: copied by the node
    rows = torch.randn(B, Nv, E + 4, generator=torch.Generator().manual_seed(2)).to(DEV)[..., :E]      # row stride > width: read in place
    assert view.stride(2) == 2 and rows.stride(1) == E + 4 and not rows.is_contiguous()

    def run(gv, r=0.0, seed=None):
        leaves, y = _function_run(t, ad, r=r, seed=seed)
        torch.randn(1 << 18, device=DEV).sum()                                # other work in between
        _backward(y, gv, t[5])
        return [o.detach() for o in y] + [x.grad for x in leaves]

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))
    for g in (view, rows):
        first = run(g)
        assert same(first, run(g.contiguous())) and same(first, run(g))
    a = run(t[4], 0.1, 11)
    assert same(a, run(t[4], 0.1, 11)) and not same(a[:2], run(t[4], 0.1, 12)[:2])
    assert same(run(t[4], 0.0, 11), run(t[4], 0.0, 12))
    # no seed given: drawn from torch's default CPU generator, so the call repeats under torch.manual_seed
    torch.manual_seed(5)
    b = run(t[4], 0.1)
    torch.manual_seed(5)
    assert same(b, run(t[4], 0.1)) and not same(b[:2], run(t[4], 0.1)[:2])


# --------------------------------------------------------------------------------------------- what the entry points write
@pytest.mark.parametrize("Nv,L", [(33, 7), (130, 77)])
def test_outputs_stay_inside_their_buffers(Nv, L):
    """guard bands around the outputs, the log-sum-exps, the statistics, the four gradients and the two workspaces keep their fill, and every
    element between them is written"""
    from hipie_amd import _lib, ops
    lib = _lib.load()
    GUARD, FILL = 64, 12345.0
    t = operands(B, Nv, L, H, seed=7, dev=DEV)
    q, k, vv, vl, gv, gl = t
    ad = masks_for(B, L)["prefix"].to(DEV)
    nf, nb = lib.hipie_bi_attn_train_forward_ws_bytes(B, H, Nv, L), lib.hipie_bi_attn_train_backward_ws_bytes(B, H, Nv, L)
    sizes = dict(out_v=B * Nv * E, out_l=B * L * E, lse_v=B * H * Nv, lse_l=B * H * L, st_v=2 * B * H * Nv, st_l=2 * B * H * L, d_q=B * Nv * E,
                 d_k=B * L * E, d_vv=B * Nv * E, d_vl=B * L * E, wf=nf // 4, wb=nb // 4)
    bufs = {n: torch.full((s + 2 * GUARD,), FILL, device=DEV) for n, s in sizes.items()}
    ptr = {n: b[GUARD:].data_ptr() for n, b in bufs.items()}
    st = torch.cuda.current_stream().cuda_stream
    strides = [x for s in (q, k, vv, vl) for x in (s.stride(0), s.stride(1))]
    ins = [x.data_ptr() for x in (q, k, vv, vl, ad)]
    rc = lib.hipie_bi_attn_train_forward(*ins, *[ptr[n] for n in ("out_v", "out_l", "lse_v", "lse_l", "st_v", "st_l", "wf")], nf, B, H, Nv, L, HD, *strides, 0.1, 5, st)
    assert rc == 0, lib.hipie_last_error()
    rc = lib.hipie_bi_attn_train_backward(*ins, *[ptr[n] for n in ("out_v", "out_l", "st_v", "st_l")], gv.data_ptr(), gl.data_ptr(),
                                          *[ptr[n] for n in ("d_q", "d_k", "d_vv", "d_vl", "wb")], nb, B, H, Nv, L, HD, *strides,
                                          gv.stride(0), gv.stride(1), gl.stride(0), gl.stride(1), 0.1, 5, st)
    assert rc == 0, lib.hipie_last_error()
    torch.cuda.synchronize()
    pad = {"wb": ((B * H * Nv + 3) // 4 * 4 - B * H * Nv, (B * H * L + 3) // 4 * 4 - B * H * L)}      # alignment gaps behind the two deltas
    for n, b in bufs.items():
        assert bool((b[:GUARD] == FILL).all()) and bool((b[GUARD + sizes[n]:] == FILL).all()), n
        unwritten = int((b[GUARD:GUARD + sizes[n]] == FILL).sum())
        assert unwritten == sum(pad.get(n, ())), (n, unwritten)
    got, lse = _run(ops, t, ad, 0.1, 5)
    mine = [bufs[n][GUARD:GUARD + sizes[n]] for n in ("out_v", "out_l", "d_q", "d_k", "d_vv", "d_vl", "lse_v", "lse_l")]
    assert all(torch.equal(a.reshape(-1), b) for a, b in zip(got + lse, mine))


# --------------------------------------------------------------------------------------------- declines
def test_declines_and_the_block_falls_back(monkeypatch):
    from hipie_amd.training import functions, net
    q, k, vv, vl, _, _ = operands(B, 20, 257, H, seed=8, dev=DEV)
    att = torch.ones(B, 257, dtype=torch.bool, device=DEV)
    assert functions.fusion_attention(q, k[:, :256], vv, vl[:, :256], att[:, :256], H, 0.0) is not None
    assert functions.fusion_attention(q, k, vv, vl, att, H, 0.0) is None                        # L = 257
    assert functions.fusion_attention(*[x[:, :9].half() for x in (q, k, vv, vl)], att[:, :9], H, 0.0) is None      # fp16 operands
    answers = []
    real = functions.fusion_attention

    def spy(*a):
        answers.append(real(*a))
        return answers[-1]
    monkeypatch.setattr(functions, "fusion_attention", spy)
    be = net.backend("fusion_attention")
    v, l, mask, sd = block_case()
    v, l, mask = v.to(DEV), l.to(DEV), mask.to(DEV)
    sd = {n: x.to(DEV) for n, x in sd.items()}
    want = net.bi_attention_block(v, l, mask, sd, "b.", heads=2)
    got = net.bi_attention_block(v, l, mask, sd, "b.", heads=2, be=be)
    assert len(answers) == 1 and answers[0] is not None
    assert all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(got, want))
    long_l = torch.randn(B, 257, l.shape[2], generator=torch.Generator().manual_seed(3)).to(DEV)
    long_m = torch.ones(B, 257, dtype=torch.int64, device=DEV)
    got = net.bi_attention_block(v, long_l, long_m, sd, "b.", heads=2, be=be)
    assert len(answers) == 2 and answers[1] is None
    assert all(torch.equal(a, b) for a, b in zip(got, net.bi_attention_block(v, long_l, long_m, sd, "b.", heads=2)))
    half = {n: x.half() for n, x in sd.items()}
    got = net.bi_attention_block(v.half(), l.half(), mask, half, "b.", heads=2, be=be)
    assert len(answers) == 3 and answers[2] is None
    assert all(torch.equal(a, b) for a, b in zip(got, net.bi_attention_block(v.half(), l.half(), mask, half, "b.", heads=2)))


# --------------------------------------------------------------------------------------------- one training step
def _every_group():
    from hipie_amd.training import net
    return tuple(net.GROUPS) + tuple(net.EXTRA_GROUPS) + tuple(net.LATER_GROUPS)


@pytest.mark.parametrize("names", [lambda: ("fusion_attention",), _every_group], ids=["alone", "every-group"])
def test_train_step_with_fusion_attention_nodes_matches_the_reference(names, monkeypatch):
    from hipie_amd.training import functions, net
    names = names()
    be = net.backend(*names)
    assert net.HipBackendFusionAttention in be.__mro__ and all(c in be.__mro__ for c in list(net.GROUPS.values()) * (len(names) > 1))
    ran, declined = [], []
    real = functions.fusion_attention

    def spy(q, k, vv, vl, text_mask, heads, dropout):
        y = real(q, k, vv, vl, text_mask, heads, dropout)
        (declined if y is None else ran).append((tuple(q.shape), tuple(k.shape), dropout))
        return y
    monkeypatch.setattr(functions, "fusion_attention", spy)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    z, meta, model, step, batch, targets = train_step_case("cuda", be)
    assert step.be is be
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    print("FAT step %s: node ran on %s, declined %s" % ("+".join(names), ran, declined))
    assert not declined and len(ran) == meta["cfg"]["num_vl_layers"] > 0 and all(r[0][2] == 2048 and r[2] == 0.0 for r in ran)
    check_step_against_golden(z, model, step, losses, total, "cuda", "FUSION ATTENTION step (%s)" % "+".join(names))
