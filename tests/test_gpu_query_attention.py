"""GPU: hipie_attn_f32_train_forward / hipie_attn_f32_train_backward (csrc/attn_f32_train.hip) through ops.query_attn_train_forward /
ops.query_attn_train_backward, the autograd Function over them and the opt-in HipBackendQueryAttention wiring of the training step.

Reference: the float64 statements of tests/_query_attention_cases.py (checked against torch.autograd in test_query_attention_cpu.py).
Metric: max|got - ref64| / max|ref64| per tensor (a tensor that is exactly zero in the reference has to be exactly zero).  Forward bound:
1e-5, what test_attn_f32_exact holds this arithmetic to at this operand scale.  Gradient bound per case: max(1e-5, 4 x e_lib), e_lib = the
same metric for torch's fp32 materialised formulation and its autograd on the same device.  Every case prints its figures (lines starting
with QAT) before it asserts."""
import pytest
import torch

from _query_attention_cases import HD, SCALE, backward64, forward64, masks_for, operands, torch_graph
from _train_step_cases import check_step_against_golden, train_step_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H = 2, 3


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float((got - ref).abs().max() / top)


def _check_grads(tag, got, ref64, lib32):
    fails = []
    for n, g, r, l in zip(("d_qk", "d_v"), got, ref64, lib32):
        e, e_lib = _err(g, r), _err(l, r)
        bound = max(1e-5, 4 * e_lib)
        print("QAT %-28s %-5s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


# --------------------------------------------------------------------------------------------- the operator against float64
@pytest.mark.parametrize("mask", ["none", "dn", "random"])
@pytest.mark.parametrize("N", [1, 33, 129, 200])
def test_operator_against_float64(N, mask):
    """a workgroup is 64 rows x 4 waves, wave s taking keys 32 s .. 32 s + 31 of every chunk of 128.  N: 1 a single row, three waves without
    a key; 33 the second wave has one key; 129 a third workgroup of one row and a second chunk of one key; 200 the de-noising geometry
    (pad 72, 4 groups)"""
    from hipie_amd import ops
    qk, v, d_out = operands(B, N, H, seed=1, dev=DEV)
    assert qk.stride(1) > qk.shape[2] and v.stride(1) > v.shape[2] and d_out.stride(1) > d_out.shape[2]
    blocked = masks_for(N)[mask]
    bd = None if blocked is None else blocked.to(DEV)
    tag = "N=%d %s" % (N, mask)
    out, lse = ops.query_attn_train_forward(qk, v, bd, H, SCALE)
    ref_out, ref_lse = forward64(qk.cpu(), v.cpu(), blocked, H)
    assert out.shape == (B, N, H * HD) and lse.shape == (B, H, N) and out.is_contiguous()
    e_out, e_lse = _err(out, ref_out), _err(lse, ref_lse)
    print("QAT %-28s out   err %.3e  lse err %.3e  bound 1.000e-05" % (tag, e_out, e_lse))
    assert e_out <= 1e-5 and e_lse <= 1e-5
    ref = backward64(qk.cpu(), v.cpu(), blocked, H, d_out.cpu())
    lib = torch_graph(qk, v, bd, H, d_out, torch.float32, DEV)[1:]
    got = ops.query_attn_train_backward(qk, v, bd, out, lse, d_out, H, SCALE)
    assert got[0].shape == (B, N, 2 * H * HD) and got[1].shape == (B, N, H * HD)
    _check_grads(tag, got, ref, lib)
    assert N > 1 or (not bool(ref[0].any()) and not bool(got[0].any()))          # one key: p = 1, d_q = d_k = 0 exactly
    # one side wanted: the same bits from fewer launches
    only_qk = ops.query_attn_train_backward(qk, v, bd, out, lse, d_out, H, SCALE, want_v=False)
    only_v = ops.query_attn_train_backward(qk, v, bd, out, lse, d_out, H, SCALE, want_qk=False)
    assert only_qk[1] is None and only_v[0] is None and torch.equal(only_qk[0], got[0]) and torch.equal(only_v[1], got[1])


def test_a_fully_blocked_row():
    """N = 33 with row 5 blocked everywhere: zeros out, lse = -inf, d_q exactly 0, and d_k / d_v those of the attention without that query"""
    from hipie_amd import ops
    N = 33
    qk, v, d_out = operands(B, N, H, seed=2, dev=DEV)
    blocked = masks_for(N)["random"].clone()
    blocked[5] = True
    bd = blocked.to(DEV)
    out, lse = ops.query_attn_train_forward(qk, v, bd, H, SCALE)
    assert bool((out[:, 5] == 0).all()) and bool((lse[:, :, 5] == float("-inf")).all()) and bool(torch.isfinite(out).all())
    rows = torch.tensor([i for i in range(N) if i != 5])
    assert bool(torch.isfinite(lse[:, :, rows.to(DEV)]).all())
    d_qk, d_v = ops.query_attn_train_backward(qk, v, bd, out, lse, d_out, H, SCALE)
    assert bool(torch.isfinite(d_qk).all()) and bool(torch.isfinite(d_v).all())
    assert bool((d_qk[:, 5, :H * HD] == 0).all())
    ref = backward64(qk.cpu(), v.cpu(), blocked, H, d_out.cpu(), query_rows=rows)
    lib = torch_graph(qk, v, bd, H, d_out, torch.float32, DEV, query_rows=rows)[1:]      # the library without that query (its softmax of the row is NaN)
    _check_grads("N=33 row 5 blocked", (d_qk, d_v), ref, lib)
    # exactly zero: the same call with row 5's output gradient replaced gives the same d_k / d_v bits
    other = d_out.clone()
    other[:, 5] = 1e3
    again = ops.query_attn_train_backward(qk, v, bd, out, lse, other, H, SCALE)
    assert torch.equal(again[0], d_qk) and torch.equal(again[1], d_v)


# --------------------------------------------------------------------------------------------- the autograd Function
def _function_run(qk, v, bd, grad_qk=True, grad_v=True):
    from hipie_amd.training import functions
    qk_, v_ = qk.detach().requires_grad_(grad_qk), v.detach().requires_grad_(grad_v)
    y = functions.query_attention(qk_, v_, bd, H)
    assert y is not None and y.requires_grad == (grad_qk or grad_v)
    return qk_, v_, y


def test_function_forward_backward_and_frozen_inputs(monkeypatch):
    from hipie_amd import ops
    from hipie_amd.training import functions
    N = 129
    qk, v, d_out = operands(B, N, H, seed=3, dev=DEV)
    blocked = masks_for(N)["dn"]
    bd = blocked.to(DEV)
    seen = []
    real = ops.query_attn_train_backward

    def spy(*a, **k):
        seen.append((k["want_qk"], k["want_v"]))
        return real(*a, **k)
    monkeypatch.setattr(functions.ops, "query_attn_train_backward", spy)
    qk_, v_, y = _function_run(qk, v, bd)
    assert torch.equal(y, ops.query_attn_train_forward(qk, v, bd, H, SCALE)[0])
    saved = [tuple(t.shape) for t in y.grad_fn.saved_tensors]
    assert saved == [(B, N, 2 * H * HD), (B, N, H * HD), (B, N, H * HD), (B, H, N), (N, N)]           # the caller's mask is the only N x N
    y.backward(d_out)
    _check_grads("Function N=129 dn", (qk_.grad, v_.grad), backward64(qk.cpu(), v.cpu(), blocked, H, d_out.cpu()),
                 torch_graph(qk, v, bd, H, d_out, torch.float32, DEV)[1:])
    full = (qk_.grad, v_.grad)
    # a frozen v, a frozen qk: the same bits from fewer launches; both frozen: no node at all
    qk_, v_, y = _function_run(qk, v, bd, grad_v=False)
    y.backward(d_out)
    assert v_.grad is None and torch.equal(qk_.grad, full[0])
    qk_, v_, y = _function_run(qk, v, bd, grad_qk=False)
    y.backward(d_out)
    assert qk_.grad is None and torch.equal(v_.grad, full[1])
    assert seen == [(True, True), (True, False), (False, True)]
    qk_, v_, y = _function_run(qk, v, bd, grad_qk=False, grad_v=False)
    assert y.grad_fn is None and len(seen) == 3


def test_function_takes_a_strided_output_gradient_and_repeats_its_bits():
    N = 129
    qk, v, _ = operands(B, N, H, seed=4, dev=DEV)
    bd = masks_for(N)["random"].to(DEV)
    wide = torch.randn(B, N, H * HD, 2, generator=torch.Generator().manual_seed(1)).to(DEV)
    view = wide[..., 0]                                                       # column stride 2: copied by the node
    rows = torch.randn(B, N, H * HD + 4, generator=torch.Generator().manual_seed(2)).to(DEV)[..., :H * HD]      # row stride > width: read in place
    assert view.stride(2) == 2 and rows.stride(1) == H * HD + 4 and not rows.is_contiguous()
    for g in (view, rows):
        runs = []
        for d in (g, g.contiguous(), g):
            qk_, v_, y = _function_run(qk, v, bd)
            torch.randn(1 << 18, device=DEV).sum()                              # other work in between
            y.backward(d)
            runs.append((y.detach(), qk_.grad, v_.grad))
        assert all(torch.equal(a, b) for r in runs[1:] for a, b in zip(runs[0], r))


def test_declines_and_mha_falls_back(monkeypatch):
    from hipie_amd.training import functions, net
    from _query_attention_cases import wiring_case
    N = 20
    qk, v, _ = operands(B, N, 2, seed=5, dev=DEV)
    ok_mask = masks_for(N)["dn"].to(DEV)
    assert functions.query_attention(qk, v, ok_mask, 2) is not None
    assert functions.query_attention(qk, v, ok_mask, 1) is None                             # one head of 64
    assert functions.query_attention(qk.half(), v.half(), ok_mask, 2) is None              # fp16 operands
    assert functions.query_attention(qk, v, ok_mask[None].expand(B, N, N), 2) is None       # a (B, N, N) mask
    assert functions.query_attention(qk.cpu(), v.cpu(), ok_mask.cpu(), 2) is None           # host tensors
    assert functions.query_attention(qk, v, ok_mask.cpu(), 2) is None and functions.query_attention(qk, v, ok_mask.float(), 2) is None
    # net.mha with the group: the node where it is covered, today's formulation bit for bit where the op declines
    tgt, qpos, _, _, _, _, sd, attn_mask = wiring_case()
    tgt, qpos, attn_mask = tgt.detach().to(DEV), qpos.detach().to(DEV), attn_mask.to(DEV)
    sd = {k: t.detach().to(DEV) for k, t in sd.items()}
    host = {k: t.cpu() for k, t in sd.items()}
    be = net.backend("query_attention")
    answers = []
    real = functions.query_attention

    def spy(*a):
        answers.append(real(*a))
        return answers[-1]
    monkeypatch.setattr(functions, "query_attention", spy)
    want = net.mha(tgt + qpos, tgt, sd, "l.self_attn.", attn_mask)
    got = net.mha(tgt + qpos, tgt, sd, "l.self_attn.", attn_mask, be=be)
    assert len(answers) == 1 and answers[0] is not None and float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert torch.equal(net.mha(tgt + qpos, tgt, sd, "l.self_attn.", attn_mask, heads=4, be=be), net.mha(tgt + qpos, tgt, sd, "l.self_attn.", attn_mask, heads=4))
    assert len(answers) == 2 and answers[1] is None                                          # 4 heads of 64
    x, t = (tgt + qpos).cpu(), tgt.cpu()
    assert torch.equal(net.mha(x, t, host, "l.self_attn.", attn_mask.cpu(), be=be), net.mha(x, t, host, "l.self_attn.", attn_mask.cpu()))
    assert len(answers) == 3 and answers[2] is None                                          # host tensors


# --------------------------------------------------------------------------------------------- what the entry points write
@pytest.mark.parametrize("N", [33, 129])
def test_outputs_stay_inside_their_buffers(N):
    """guard bands around out, lse, d_qk, d_v and the workspace keep their fill, and every element between them is written"""
    from hipie_amd import _lib, ops
    lib = _lib.load()
    GUARD, FILL = 64, 12345.0
    qk, v, d_out = operands(B, N, H, seed=6, dev=DEV)
    bd = masks_for(N)["random"].to(DEV)
    C = H * HD
    nbytes = lib.hipie_attn_f32_train_backward_ws_bytes(B, H, N)
    assert nbytes == B * H * N * 4
    sizes = dict(out=B * N * C, lse=B * H * N, d_qk=B * N * 2 * C, d_v=B * N * C, ws=nbytes // 4)
    bufs = {n: torch.full((k + 2 * GUARD,), FILL, device=DEV) for n, k in sizes.items()}
    ptr = {n: t[GUARD:].data_ptr() for n, t in bufs.items()}
    st = torch.cuda.current_stream().cuda_stream
    strides = (qk.stride(0), qk.stride(1), v.stride(0), v.stride(1), 0)
    rc = lib.hipie_attn_f32_train_forward(qk.data_ptr(), v.data_ptr(), bd.data_ptr(), ptr["out"], ptr["lse"], B, H, N, HD, *strides, SCALE, st)
    assert rc == 0, lib.hipie_last_error()
    rc = lib.hipie_attn_f32_train_backward(qk.data_ptr(), v.data_ptr(), bd.data_ptr(), ptr["out"], ptr["lse"], d_out.data_ptr(), ptr["d_qk"], ptr["d_v"],
                                           ptr["ws"], nbytes, B, H, N, HD, *strides, d_out.stride(0), d_out.stride(1), SCALE, st)
    assert rc == 0, lib.hipie_last_error()
    torch.cuda.synchronize()
    for n, t in bufs.items():
        assert bool((t[:GUARD] == FILL).all()) and bool((t[GUARD + sizes[n]:] == FILL).all()), n
        assert not bool((t[GUARD:GUARD + sizes[n]] == FILL).any()), n
    out, lse = ops.query_attn_train_forward(qk, v, bd, H, SCALE)
    got = ops.query_attn_train_backward(qk, v, bd, out, lse, d_out, H, SCALE)
    mine = [bufs[n][GUARD:GUARD + sizes[n]] for n in ("out", "lse", "d_qk", "d_v")]
    assert all(torch.equal(a.reshape(-1), b) for a, b in zip((out, lse) + tuple(got), mine))


# --------------------------------------------------------------------------------------------- one training step
def _every_group():
    from hipie_amd.training import net
    return tuple(net.GROUPS) + tuple(net.EXTRA_GROUPS) + tuple(net.LATER_GROUPS)


@pytest.mark.parametrize("names", [lambda: ("query_attention",), _every_group], ids=["alone", "every-group"])
def test_train_step_with_query_attention_nodes_matches_the_reference(names, monkeypatch):
    from hipie_amd.training import functions, net
    names = names()
    be = net.backend(*names)
    assert net.HipBackendQueryAttention in be.__mro__ and all(c in be.__mro__ for c in list(net.GROUPS.values()) * (len(names) > 1))
    ran, declined = [], []
    real = functions.query_attention

    def spy(qk, v, attn_mask, heads):
        y = real(qk, v, attn_mask, heads)
        (declined if y is None else ran).append((tuple(qk.shape), attn_mask is not None))
        return y
    monkeypatch.setattr(functions, "query_attention", spy)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    z, meta, model, step, batch, targets = train_step_case("cuda", be)
    assert step.be is be
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    print("QAT step %s: node ran on %s, declined %s" % ("+".join(names), ran, declined))
    layers = meta["cfg"]["dec_layers"] + meta["cfg"]["md_dec_layers"]
    assert not declined and len(ran) == layers and any(m for _, m in ran)      # one node per decoder layer, the de-noising mask among them
    check_step_against_golden(z, model, step, losses, total, "cuda", "QUERY ATTENTION step (%s)" % "+".join(names))
