"""GPU: the pack / unpack kernels of csrc/attn_pack.hip through their ops, the one-node ViT attention over them
(functions.VitAttentionFunction / vit_attention_packed) and the opt-in HipBackendPackedAttention / HipBackendPackedWindows wiring.

Bit equality (conditions): the planes against ops.f16_pair of the operands net.vit_attention builds in torch (for the padded form: of the
operands functions.fused_attention pads), rq against the permute copy of q, the maximum against go.abs().amax(), the k / v slots of d(qkv)
against dk * inv / dv * inv, the node's output against today's HipBackend / HipBackendWindows composition, and two runs against each other.
Tolerances: max|got - ref64| / max|ref64| per tensor against the float64 formulation on the host on the same fp32-representable inputs,
bound max(1e-6, 4 x e_old), e_old = the same metric for today's torch formulation on the same device and inputs.  Every case prints its
figures (lines starting with ATTNPACK) before it asserts."""
import functools

import pytest
import torch

from _attn_pack_cases import ALL, composition, inputs, operands, vit_case_packed
from _layernorm_cases import loss_grads, vit_case


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["%dx%dx%dx%d%s" % (s + ("w" if w else "",)) for s, w in ALL]


def _err(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _check(tag, names, got, ref64, old):
    fails = []
    for n, g, r, o in zip(names, got, ref64, old):
        e, e_old = _err(g, r), _err(o, r)
        bound = max(1e-6, 4 * e_old)
        print("ATTNPACK %-40s %-12s err %.3e  e_old %.3e  bound %.3e" % (tag, n, e, e_old, bound))
        if not e <= bound:
            fails.append((n, e, e_old, bound))
    assert not fails, (tag, fails)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _case(shape, windows, seed=0, extremes=False, dev=DEV, dtype=torch.float32):
    from hipie_amd.training import functions, net
    B, heads, H, W = shape
    qkv, tab_h, tab_w = inputs(B, heads, H, W, seed, extremes)
    Rh, Rw = net.get_rel_pos(H, H, tab_h), net.get_rel_pos(W, W, tab_w)
    return [t.to(dev, dtype) for t in (qkv, Rh, Rw)], functions.packed_attention_instance(H, W, windows)


def _padded_operands(qa, ka, v, Np):
    """the operands functions.fused_attention hands to the kernels for a token count that is no multiple of 128"""
    BH, N, C = qa.shape
    pad = torch.nn.functional.pad
    bias = ka.new_zeros(BH, Np, 1)
    bias[:, N:] = -30000.0
    return (pad(torch.cat((qa, qa.new_ones(BH, N, 1)), -1), (0, 0, 0, Np - N)), torch.cat((pad(ka, (0, 0, 0, Np - N)), bias), -1),
            pad(v, (0, 0, 0, Np - N)))


# --------------------------------------------------------------------------------------------- forward packs
@pytest.mark.parametrize("shape,windows", ALL, ids=IDS)
def test_planes_are_f16_pair_of_the_torch_operands(shape, windows):
    from hipie_amd import ops
    B, heads, H, W = shape
    N, BH = H * W, B * heads
    (qkv, Rh, Rw), (cols, padded) = _case(shape, windows, extremes=True)
    q, k, v, _, rel_h, rel_w, qa, ka = operands(qkv, Rh, Rw, heads, H, W)
    Np = ops.attn_pack_rows(N, padded)
    assert (Np != N) == padded
    if padded:
        qa, ka, v = _padded_operands(qa, ka, v, Np)
    rq, kp, vp = ops.attn_pack_kv(qkv, heads, H, W, cols, padded)
    assert rq.shape == (BH, N, 80) and torch.equal(rq, q.contiguous())
    for name, got, ref in (("k'", kp, ops.f16_pair(ka, cols)), ("v", vp, ops.f16_pair(v))):
        assert got[0].shape == (BH, Np, cols if name == "k'" else 80)
        assert _same_bits(got[0], ref[0]) and _same_bits(got[1], ref[1]), name
    assert float(kp[0].float().abs().max()) == 65504.0                           # the +-1e6 entries saturate
    want = ops.f16_pair(qa, cols)
    assert float(want[0].float().abs().max()) == 65504.0
    layouts = {"dense (BH, N, K)": (rel_h, rel_w),
               "rel_w with the K stride outermost": (rel_h, rel_w.permute(2, 0, 1).contiguous().permute(1, 2, 0)),
               "the layouts of the node's products": (rel_h.view(BH, H, W, H).permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3),
                                                      rel_w.view(BH, H, W, W).permute(2, 0, 1, 3).contiguous().permute(1, 2, 0, 3))}
    assert not layouts["rel_w with the K stride outermost"][1].is_contiguous()
    for name, (rh, rw) in layouts.items():
        got = ops.attn_pack_q(rq, rh, rw, heads, H, W, cols, padded)
        assert got[0].shape == (BH, Np, cols) and _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), name


# --------------------------------------------------------------------------------------------- the range of dO
def test_amax_is_abs_amax():
    from hipie_amd import ops
    g = torch.Generator().manual_seed(4)
    for shape in ((1, 128, 80), (3, 196, 160), (1, 1155, 160), (2, 2048, 640)):         # the last: more float4 than one grid stride
        go = torch.randn(*shape, generator=g).to(DEV)
        for mag in (1e-4, 1.0, 30.0):
            x = go * mag
            got = ops.attn_grad_amax(x)
            assert got.shape == (1,) and _same_bits(got, x.abs().amax().reshape(1)), (shape, mag)
        x = torch.zeros_like(go)
        assert _same_bits(ops.attn_grad_amax(x), torch.zeros(1, device=DEV))            # an all-zero dO
        for at in (0, -1, go.numel() // 2 + 1):
            x.view(-1)[at] = -7.5                                                       # one entry, negative, first / last / in the middle
            assert float(ops.attn_grad_amax(x)) == 7.5
            x.view(-1)[at] = 0.0


def _scale_of(go):
    return torch.exp2(torch.floor(torch.log2(16.0 / go.abs().amax().clamp_min(1e-30)))).reshape(1)


@pytest.mark.parametrize("shape,windows", ALL, ids=IDS)
def test_pack_grad(shape, windows):
    from hipie_amd import ops
    B, heads, H, W = shape
    N, BH = H * W, B * heads
    (qkv, Rh, Rw), (cols, padded) = _case(shape, windows)
    Np = ops.attn_pack_rows(N, padded)
    _, _, vp = ops.attn_pack_kv(qkv, heads, H, W, cols, padded)
    v = operands(qkv, Rh, Rw, heads, H, W)[2]
    g = torch.Generator().manual_seed(9)
    out = torch.randn(BH, Np, 80, generator=g).to(DEV)                                  # rows >= N hold anything: they must not be read into delta
    for mag in (1e-4, 1.0, 30.0):
        go = (torch.randn(B, N, heads * 80, generator=g) * mag).to(DEV)
        scale = _scale_of(go)
        go_hm = go.view(B, N, heads, 80).permute(0, 2, 1, 3).reshape(BH, N, 80)
        dop, v96, delta = ops.attn_pack_grad(go, out, vp, scale, heads, H, W)
        assert _same_bits(scale, torch.exp2(torch.floor(torch.log2(16.0 / ops.attn_grad_amax(go).clamp_min(1e-30)))))
        for name, got, ref in (("dO", dop, ops.f16_pair(go_hm, 96, scale)), ("v96", v96, ops.f16_pair(v, 96))):
            for a, b in zip(got, ref):
                assert a.shape == (BH, Np, 96) and _same_bits(a[:, :N], b), (name, mag)
                assert not a[:, N:].any() and not a[..., 80:].any(), (name, mag)
        assert delta.shape == (BH, Np) and not delta[:, N:].any()
        ref64 = (go_hm.double() * out[:, :N].double()).sum(-1) * scale.double()
        old = (go_hm * out[:, :N]).sum(-1) * scale
        _check("pack_grad %s |dO|~%g" % (shape, mag), ["delta"], [delta[:, :N]], [ref64], [old])


# --------------------------------------------------------------------------------------------- d(qkv)
@pytest.mark.parametrize("shape,windows", ALL, ids=IDS)
def test_unpack_grad(shape, windows):
    from hipie_amd import ops
    B, heads, H, W = shape
    N, BH = H * W, B * heads
    _, (cols, padded) = _case(shape, windows)
    Np = ops.attn_pack_rows(N, padded)
    g = torch.Generator().manual_seed(13)
    dq, dk, dv = (torch.randn(BH, Np, c, generator=g).to(DEV) for c in (cols, 80, 80))
    # the rel-pos terms in the layouts of their batched products: (H, BH W, 80) and (W, BH H, 80)
    dq_h = torch.randn(H, BH, W, 80, generator=g).to(DEV).permute(1, 0, 2, 3)
    dq_w = torch.randn(W, BH, H, 80, generator=g).to(DEV).permute(1, 2, 0, 3)
    inv = torch.full((1,), 2.0 ** -7, device=DEV)
    s = 80 ** -0.5

    def slots(t):                                                   # (BH, N, 80) head-major -> its place in (B', N, heads, 80)
        return t.reshape(B, heads, N, 80).permute(0, 2, 1, 3)
    got = ops.attn_unpack_grad(dq, dk, dv, dq_h, dq_w, inv, heads, H, W)
    assert got.shape == (B, N, 3 * heads * 80) and got.is_contiguous()
    got = got.view(B, N, 3, heads, 80)
    assert torch.equal(got[:, :, 1], slots((dk * inv)[:, :N])) and torch.equal(got[:, :, 2], slots((dv * inv)[:, :N]))
    rel = dq_h.reshape(BH, N, 80), dq_w.reshape(BH, N, 80)
    ref64 = (dq[:, :N, :80].double() * s + rel[0].double() + rel[1].double()) * inv.double()
    old = dq[:, :N, :80] * inv * s + rel[0] * inv + rel[1] * inv                     # today: dq' * inv, then autograd's scale and sums
    _check("unpack_grad %s" % (shape,), ["q slot"], [got[:, :, 0]], [slots(ref64)], [slots(old)])
    # one term alone
    one = ops.attn_unpack_grad(dq, dk, dv, dq_h, None, inv, heads, H, W).view(B, N, 3, heads, 80)
    zero = ops.attn_unpack_grad(dq, dk, dv, dq_h, torch.zeros_like(dq_w), inv, heads, H, W).view(B, N, 3, heads, 80)
    assert torch.equal(one, zero)


# --------------------------------------------------------------------------------------------- the node
NODE_NAMES = ("y", "d qkv [q]", "d qkv [k]", "d qkv [v]", "d Rh", "d Rw")


def _cot(shape, mag):
    B, heads, H, W = shape
    return torch.randn(B, H * W, heads * 80, generator=torch.Generator().manual_seed(17)) * mag


def _run(fn, shape, windows, mag, dev, dtype):
    """[y, dqkv q / k / v slots, dRh, dRw] of fn(qkv, Rh, Rw) with the cotangent _cot(shape, mag)"""
    B, heads, H, W = shape
    leaves = [t.requires_grad_(True) for t in _case(shape, windows, seed=1, dev=dev, dtype=dtype)[0]]
    y = fn(*leaves)
    dqkv, dRh, dRw = torch.autograd.grad((y * _cot(shape, mag).to(dev, dtype)).sum(), leaves)
    d = dqkv.view(B, H * W, 3, heads, 80)
    return [y.detach(), d[:, :, 0], d[:, :, 1], d[:, :, 2], dRh, dRw]


@functools.lru_cache(maxsize=None)
def _reference(shape, windows, mag):
    B, heads, H, W = shape
    return tuple(_run(lambda qkv, Rh, Rw: composition(qkv, Rh, Rw, heads, H, W), shape, windows, mag, "cpu", torch.float64))


def _today(shape, windows):
    from hipie_amd.training import net
    B, heads, H, W = shape
    be = net.HipBackendWindows if windows else net.HipBackend
    return lambda qkv, Rh, Rw: composition(qkv, Rh, Rw, heads, H, W, be)


def _node(shape, windows, applied=None):
    from hipie_amd.training import functions
    B, heads, H, W = shape

    def fn(qkv, Rh, Rw):
        y = functions.vit_attention_packed(qkv, Rh, Rw, heads, H, W, windows=windows)
        assert y is not None and type(y.grad_fn).__name__ == "VitAttentionFunctionBackward"
        return y
    return fn


@pytest.mark.parametrize("mag", [1e-4, 1.0, 30.0])
@pytest.mark.parametrize("shape,windows", ALL, ids=IDS)
def test_node_against_float64_and_todays_graph(shape, windows, mag, monkeypatch):
    from hipie_amd.training import functions
    fused = []
    for cls in (functions.FusedAttentionFunction, functions.WindowAttentionFunction):
        real = cls.apply
        monkeypatch.setattr(cls, "apply", lambda *a, real=real, name=cls.__name__: fused.append(name) or real(*a))
    old = _run(_today(shape, windows), shape, windows, mag, DEV, torch.float32)
    assert fused == ["WindowAttentionFunction" if windows else "FusedAttentionFunction"]      # the yardstick ran the fused kernels
    got = _run(_node(shape, windows), shape, windows, mag, DEV, torch.float32)
    assert len(fused) == 1
    assert _same_bits(got[0], old[0])                               # the same planes into the same kernel
    _check("node %s%s |dO|~%g" % (shape, " windows" if windows else "", mag), NODE_NAMES, got, _reference(shape, windows, mag), old)


@pytest.mark.parametrize("shape,windows", ALL, ids=IDS)
def test_node_is_deterministic_and_honours_frozen_tables(shape, windows):
    from hipie_amd.training import functions
    B, heads, H, W = shape
    a = _run(_node(shape, windows), shape, windows, 1.0, DEV, torch.float32)
    torch.randn(1 << 20, device=DEV).sum()                          # other work in between
    b = _run(_node(shape, windows), shape, windows, 1.0, DEV, torch.float32)
    for n, x, y in zip(NODE_NAMES, a, b):
        assert _same_bits(x, y), n
    # tables that need no gradient: none is computed, rq is not saved, d(qkv) keeps its bits
    qkv, Rh, Rw = _case(shape, windows, seed=1)[0]
    qkv.requires_grad_(True)
    y = functions.vit_attention_packed(qkv, Rh, Rw, heads, H, W, windows=windows)
    out = y.grad_fn.apply(_cot(shape, 1.0).to(DEV))
    assert len(out) == 8 and all(o is None for o in out[1:])
    assert _same_bits(out[0].view(B, H * W, 3, heads, 80)[:, :, 0], a[1])


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
    return seen


@pytest.mark.parametrize("shape,windows", [ALL[2], ALL[3], ALL[4]], ids=[IDS[2], IDS[3], IDS[4]])
def test_saved_tensors(shape, windows):
    """bytes of the distinct device storages one forward keeps for the backward: the node keeps the planes the composition keeps, the 80-wide
    v pair instead of the fp32 v (a view of the reshape copy of ALL of qkv), rq instead of the tensors autograd keeps for the scale, the
    einsums and the cats -- never more than the composition, and nothing of the size of qkv"""
    leaves = [t.requires_grad_(True) for t in _case(shape, windows, seed=1)[0]]
    node, today = _saved_bytes(lambda: _node(shape, windows)(*leaves)), _saved_bytes(lambda: _today(shape, windows)(*leaves))
    qkv_bytes = leaves[0].numel() * 4
    print("ATTNPACK saved bytes %s: node %d in %d storages (largest %d), composition %d in %d storages (largest %d), qkv %d"
          % (shape, sum(node.values()), len(node), max(node.values()), sum(today.values()), len(today), max(today.values()), qkv_bytes))
    assert sum(node.values()) <= sum(today.values())
    assert leaves[0].untyped_storage().data_ptr() not in node and max(node.values()) < qkv_bytes


# --------------------------------------------------------------------------------------------- end to end against HipBackend
@pytest.mark.parametrize("case,nodes", [(vit_case, (0, 0)), (vit_case_packed, (1, 2))], ids=["vit_case", "vit_case_packed"])
def test_vit_backbone_under_the_new_backends(case, nodes, monkeypatch):
    """vit_case: head width 8 -- the node declines, today's code runs; vit_case_packed: head width 80, a 128-token grid and 16-token windows --
    one node per global block, and one per windowed block under HipBackendPackedWindows"""
    from hipie_amd.training import functions, net
    x, sd, cfg = case(torch.float32)
    names = sorted(sd)

    def run(dev, dtype, be):
        leaves = [t.detach().to(dev, dtype).requires_grad_(True) for t in [x] + [sd[n] for n in names]]
        out = net.vit_backbone(leaves[0], dict(zip(names, leaves[1:])), "", cfg, be)
        outs = [out[k] for k in sorted(out)]
        loss = sum(o.double().square().mean() for o in outs)
        return [loss.detach()] + [o.detach() for o in outs] + list(loss_grads(outs, leaves))
    ref = run("cpu", torch.float64, None)
    old = run(DEV, torch.float32, net.HipBackend)
    applied = []
    real = functions.VitAttentionFunction.apply
    monkeypatch.setattr(functions.VitAttentionFunction, "apply", lambda *a: applied.append(a[4:6]) or real(*a))
    composed = net.backend("norms", "mlp", "packed_windows")      # the node beside two unrelated opt-in groups: the same rule, HipBackendPackedWindows' count
    for be, n in zip((net.HipBackendPackedAttention, net.HipBackendPackedWindows, composed), nodes + nodes[1:]):
        applied.clear()
        got = run(DEV, torch.float32, be)
        assert len(applied) == n, applied
        _check("%s %s" % (case.__name__, be.__name__), ["loss", "res3", "res4", "res5", "d input"] + ["d " + n for n in names], got, ref, old)
