"""CPU: the statements, wiring and refusals around the training fusion attention (csrc/bi_attn_train.hip, functions.FusionAttentionFunction,
net.HipBackendFusionAttention).  The kernels themselves run in test_gpu_fusion_attention.py."""
import ctypes
import math
import os
import sys

import pytest
import torch

from hipie_amd import _lib
from hipie_amd.training import functions, net

from _fusion_attention_cases import (HD, backward64, block_case, clamp_case, forward64, keep, keep_threshold, masks_for, operands, standin_backend,
                                     torch_graph)

NAMES = ("hipie_bi_attn_train_forward", "hipie_bi_attn_train_backward", "hipie_bi_attn_train_backward_ws_bytes", "hipie_bi_attn_train_forward_ws_bytes")


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


def _rel(got, ref):
    top = float(ref.abs().max())
    return float((got.double() - ref).abs().max()) / top if top > 0 else float(got.abs().max())


# ------------------------------------------------------------------------------------------------ the float64 statement
@pytest.mark.parametrize("r", [0.0, 0.1])
def test_statement_is_torch_autograd_over_the_materialised_formulation(r):
    """(Nv, L) = (37, 9), a prefix mask, visual rows 0 and 1 clamped on both sides, float64: outputs and all four gradients to 1e-12"""
    B, Nv, L, heads, seed = 2, 37, 9, 2, 1234567890123
    q, k, vv, vl, gv, gl = clamp_case(B, Nv, L, heads, seed=1)
    att = masks_for(B, L)["prefix"]
    raw = HD ** -0.5 * torch.einsum("bihd,bjhd->bhij", q.double().view(B, Nv, heads, HD), k.double().view(B, L, heads, HD))
    assert bool((raw[:, :, 0] > 50000).all()) and bool((raw[:, :, 1] < -50000).all()) and bool((raw[:, :, 2:].abs() < 50000).all())
    ref = torch_graph(q, k, vv, vl, att, heads, gv, gl, torch.float64, r=r, seed=seed)
    got = forward64(q, k, vv, vl, att, heads, r, seed)[:2] + backward64(q, k, vv, vl, att, heads, gv, gl, r, seed)
    for n, a, b in zip(("out_v", "out_l", "d_q", "d_k", "d_vv", "d_vl"), got, ref):
        assert _rel(a, b) <= 1e-12, (n, _rel(a, b))
    assert not bool(got[2][:, :2].any())                                      # clamped rows: d_q exactly 0
    if r > 0:                                                                 # the masks entered: the result differs from r = 0
        assert _rel(got[0], forward64(q, k, vv, vl, att, heads)[0]) > 1e-3


def test_statement_of_an_image_without_attended_tokens():
    B, Nv, L, heads = 2, 11, 5, 1
    q, k, vv, vl, gv, gl = operands(B, Nv, L, heads, seed=2)
    att = masks_for(B, L)["all"].clone()
    att[1] = False
    out_v, out_l, lse_v, lse_l = forward64(q, k, vv, vl, att, heads)
    assert not bool(out_v[1].any()) and bool((lse_v[1] == float("-inf")).all()) and bool(torch.isfinite(out_l).all()) and bool(torch.isfinite(lse_l).all())
    both, only_l = backward64(q, k, vv, vl, att, heads, gv, gl), backward64(q, k, vv, vl, att, heads, gv, gl, directions=(False, True))
    assert all(bool(torch.isfinite(t).all()) for t in both)
    assert torch.equal(both[0][1], only_l[0][1]) and torch.equal(both[1][1], only_l[1][1]) and not bool(both[3][1].any())


# ------------------------------------------------------------------------------------------------ the keep function
def test_keep_function():
    B, heads, Nv, L, r, seed = 2, 2, 300, 77, 0.1, 0x1234567890ABCDEF
    n = B * heads * Nv * L
    assert n == 92400
    a, b = keep(seed, 0, B, heads, Nv, L, r), keep(seed, 1, B, heads, Nv, L, r)
    assert torch.equal(a, keep(seed, 0, B, heads, Nv, L, r)) and not torch.equal(a, b) and not torch.equal(a, keep(seed + 1, 0, B, heads, Nv, L, r))
    tol = 5 * math.sqrt(r * (1 - r) / n)
    assert abs(float(a.double().mean()) - (1 - r)) <= tol and abs(float(b.double().mean()) - (1 - r)) <= tol
    agree = r * r + (1 - r) * (1 - r)
    assert abs(float((a == b).double().mean()) - agree) <= 5 * math.sqrt(agree * (1 - agree) / n)
    assert bool(keep(seed, 0, B, heads, 9, 7, 0.0).all()) and keep_threshold(0.0) == 0 and keep_threshold(0.1) == 429496730
    # a sub-block of a larger problem has the larger problem's mask: the function sees indices, not shapes
    assert torch.equal(keep(seed, 1, B, heads, 40, 9, r), b[:, :, :40, :9])


# ------------------------------------------------------------------------------------------------ composer
def _public(cls):
    return {n for n in dir(cls) if not n.startswith("_")}


def test_backend_group_and_composition():
    assert net.backend("fusion_attention") is net.HipBackendFusionAttention and issubclass(net.HipBackendFusionAttention, net.HipBackend)
    assert _public(net.HipBackendFusionAttention) - _public(net.HipBackend) == {"fusion_attention"}
    later = list(net.LATER_GROUPS)
    assert later.index("fusion_attention") > later.index("query_attention")
    assert net.backend("query_attention", "fusion_attention").__bases__ == (net.HipBackendQueryAttention, net.HipBackendFusionAttention)
    assert net.backend("fusion_attention", "query_attention") is net.backend("query_attention", "fusion_attention")
    # no op is defined by two groups
    groups = {**net.GROUPS, **net.EXTRA_GROUPS, **net.LATER_GROUPS}
    own = {n: {m for m in vars(c) if not m.startswith("_")} for n, c in groups.items()}
    names = list(own)
    unrelated = [(a, b) for x, a in enumerate(names) for b in names[x + 1:] if not issubclass(groups[a], groups[b]) and not issubclass(groups[b], groups[a])]
    assert all(not (own[a] & own[b]) for a, b in unrelated) and sum("fusion_attention" in pair for pair in unrelated) == len(names) - 1
    assert [n for n in names if "fusion_attention" in own[n]] == ["fusion_attention"]
    # every earlier key is still there, in its place
    assert list(net.GROUPS) == ["norms", "mlp", "windows", "packed_attention", "packed_windows", "deformable", "losses", "criteria", "matching",
                                "hungarian", "assign", "pair_losses"]
    assert list(net.EXTRA_GROUPS) == ["group_norms"] and later[0] == "query_attention"
    every = net.backend(*groups)
    assert every.__bases__[-1] is net.HipBackendFusionAttention and every.fusion_attention is net.HipBackendFusionAttention.fusion_attention


# ------------------------------------------------------------------------------------------------ wiring
def _run_block(be, dropout=0.0):
    v, l, mask, sd = block_case()
    return net.bi_attention_block(v, l, mask, sd, "b.", heads=2, dropout=dropout, be=be)


def test_bi_attention_block_asks_the_backend():
    want = _run_block(None)
    be, rec = standin_backend()
    got = _run_block(be, dropout=0.0)
    assert len(rec.calls) == 1 and rec.calls[0][1:] == (2, 0.0)
    v, l, mask, sd = block_case()
    rows = torch.nn.functional.linear(torch.nn.functional.layer_norm(v, v.shape[-1:], sd["b.layer_norm_v.weight"], sd["b.layer_norm_v.bias"], 1e-5),
                                      sd["b.attn.v_proj.weight"], sd["b.attn.v_proj.bias"])
    assert torch.equal(rec.calls[0][0], rows)                                 # the UNSCALED v_proj rows
    assert all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(got, want))
    # the dropout rate reaches the op
    be, rec = standin_backend()
    _run_block(be, dropout=0.25)
    assert rec.calls[0][2] == 0.25
    # an op that declines: today's result bit for bit
    be, rec = standin_backend(declines=True)
    got = _run_block(be)
    assert len(rec.calls) == 1 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(_run_block(object), want))  # a backend without the op


def test_hipie_transformer_hands_the_backend_through():
    from _train_step_cases import OracleBackend, train_step_case
    be, rec = standin_backend(base=OracleBackend)
    z, meta, model, step, batch, targets = train_step_case("cpu", be)
    with torch.no_grad():
        step.loss_dict(batch, targets)
    assert len(rec.calls) == meta["cfg"]["num_vl_layers"] > 0 and all(c[1] == 8 and c[0].shape[2] == 2048 and c[2] == 0.0 for c in rec.calls)


# ------------------------------------------------------------------------------------------------ limits
class _Dev:
    """a tensor that says it lives on the device: fusion_attention_ok reads attributes only"""

    def __init__(self, t):
        self._t = t
    is_cuda = True

    def __getattr__(self, n):
        return getattr(self._t, n)


def test_fusion_attention_ok_names_each_limit(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _Dev)))
    B, Nv, L, heads = 2, 5, 7, 2

    def case(L=L, Nv=Nv):
        q, k, vv, vl, _, _ = operands(B, max(Nv, 1), max(L, 1), heads)
        return [q[:, :Nv], k[:, :L], vv[:, :Nv], vl[:, :L], torch.ones(B, L, dtype=torch.bool)]

    def ok(ts, heads=heads, r=0.0, dev=True):
        return functions.fusion_attention_ok(*[(_Dev(t) if dev else t) for t in ts], heads, r)
    assert ok(case())
    assert not ok(case(), dev=False)                                          # host tensors
    assert functions.fusion_attention(*case(), heads, 0.0) is None            # and the op declines them
    assert not ok([t.half() if t.dtype == torch.float32 else t for t in case()])
    assert not ok(case(), heads=1) and not ok(case(), heads=4)                # E != heads * 256
    assert not ok(case(L=0)) and not ok(case(Nv=0)) and ok(case(L=256)) and not ok(case(L=257))
    assert not ok(case(), r=-0.1) and not ok(case(), r=1.0) and ok(case(), r=0.999)
    ts = case()
    assert not ok(ts[:4] + [torch.ones(B, L + 1, dtype=torch.bool)]) and not ok(ts[:4] + [torch.ones(L, dtype=torch.bool)])
    wide = torch.randn(B, Nv, heads * HD + 2)                                 # row stride 514: not a multiple of 4
    assert not ok([wide[..., :heads * HD]] + ts[1:])
    off = torch.randn(B, Nv, heads * HD + 4)[..., 1:heads * HD + 1]           # off a 16-byte boundary
    assert not ok([off] + ts[1:])


def test_bench_train_step_consumes_the_new_flag():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from bench_train_step import LATER_FLAGS, backend_names
    assert LATER_FLAGS["--fused-fusion-attention"] == "fusion_attention"
    names, rest = backend_names(["2", "--fused-fusion-attention", "4"])
    assert names == ["fusion_attention"] and rest == ["2", "4"]
    names, rest = backend_names(["--fused-query-attention", "--fused-fusion-attention"])
    assert net.backend(*names).__bases__ == (net.HipBackendQueryAttention, net.HipBackendFusionAttention)


# ------------------------------------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    sigs, res = _lib.SIGNATURES, _lib.RESTYPES
    c_p, c_i, c_l, c_d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    parsed = _lib.parse_header(open(_lib.HEADER_PATH).read())[0]
    assert all(n in parsed and parsed[n] == sigs[n] for n in NAMES)
    assert sigs[NAMES[0]] == [c_p] * 12 + [c_l] + [c_i] * 5 + [c_l] * 8 + [c_d, c_l, c_p] and res[NAMES[0]] is c_i
    assert sigs[NAMES[1]] == [c_p] * 16 + [c_l] + [c_i] * 5 + [c_l] * 12 + [c_d, c_l, c_p] and res[NAMES[1]] is c_i
    assert sigs[NAMES[2]] == [c_i] * 4 and sigs[NAMES[3]] == [c_i] * 4 and res[NAMES[2]] is c_l and res[NAMES[3]] is c_l
    assert _lib.CONSTANTS["HIPIE_ABI_VERSION"] == 13


def test_refusals_by_message():
    lib = _lib.load()
    P = [4096 * (x + 1) for x in range(16)]
    B, H, Nv, L, E = 2, 2, 40, 9, 512
    need_f, need_b = lib.hipie_bi_attn_train_forward_ws_bytes(B, H, Nv, L), lib.hipie_bi_attn_train_backward_ws_bytes(B, H, Nv, L)
    assert need_f == (1 * B * H * L * (2 + 256)) * 4 and need_b == (B * H * Nv + B * H * L + 2 * B * H * L * 256) * 4
    assert lib.hipie_bi_attn_train_forward_ws_bytes(B, H, 128 * 9, L) == 5 * B * H * L * (2 + 256) * 4          # 9 sweep steps: 5 segments of 2

    def fwd(ptrs=None, ws=need_f, H=H, L=L, hd=256, strides=None, r=0.0):
        ptrs = list(P[:12]) if ptrs is None else ptrs
        return lib.hipie_bi_attn_train_forward(*ptrs, ws, B, H, Nv, L, hd, *(strides or [Nv * E, E, L * E, E] * 2), r, 7, None)

    def bwd(ptrs=None, ws=need_b, dstr=None):
        ptrs = list(P[:16]) if ptrs is None else ptrs
        return lib.hipie_bi_attn_train_backward(*ptrs, ws, B, H, Nv, L, 256, *([Nv * E, E, L * E, E] * 2), *(dstr or [Nv * E, E, L * E, E]), 0.0, 7, None)

    def refused(rc, text):
        assert rc != 0 and text in lib.hipie_last_error(), (rc, lib.hipie_last_error())
    for x in range(12):
        refused(fwd([None if y == x else p for y, p in enumerate(P[:12])]), b"bi_attn_train_forward: null pointer")
    for x in list(range(11)) + [15]:
        refused(bwd([None if y == x else p for y, p in enumerate(P[:16])]), b"bi_attn_train_backward: null pointer")
    refused(fwd(hd=128), b"head_dim 256 only (got 128)")
    refused(fwd(L=0), b"text rows only (got 0)")
    refused(fwd(L=257), b"text rows only (got 257)")
    refused(fwd(ws=need_f - 1), b"workspace of %d bytes, need %d" % (need_f - 1, need_f))
    refused(bwd(ws=need_b - 4), b"workspace of %d bytes, need %d" % (need_b - 4, need_b))
    refused(fwd(strides=[Nv * E, E + 2, L * E, E, Nv * E, E, L * E, E]), b"16-byte aligned and strides multiples of 4")
    refused(fwd(strides=[Nv * E, E - 4, L * E, E, Nv * E, E, L * E, E]), b"a row stride below the row's width")
    refused(fwd([P[0] + 4] + P[1:12]), b"16-byte aligned")
    refused(bwd(dstr=[Nv * E, E + 1, L * E, E]), b"16-byte aligned and strides multiples of 4")
    refused(bwd(P[:11] + [P[11] + 8] + P[12:16]), b"16-byte aligned")
    refused(fwd(r=1.0), b"dropout rate 1 outside [0, 1)")
    refused(fwd(r=-0.5), b"outside [0, 1)")
    # no gradient wanted: returns before a launch (the pointers are fake: a launch would fail)
    assert bwd(P[:11] + [None] * 4 + [P[15]]) == 0
