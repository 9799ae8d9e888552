"""CPU: the training query self-attention node below the kernels -- the three entry points of the C ABI and their host refusals (nothing
reaches a launch: the pointers are fake, and every call here is either refused or asks for no gradient), the float64 statement of the
backward (tests/_query_attention_cases.py) against torch.autograd, the wiring of net.mha / net.decoder_layer and of a whole training step
through a backend's `query_attention`, and the composer's third table."""
import ctypes
import os
import re
import sys

import pytest
import torch

from hipie_amd import _lib
from hipie_amd.training import net

from _query_attention_cases import (backward64, forward64, masks_for, operands, standin_backend, torch_graph, wiring_case)
from _train_step_cases import check_step_against_golden, train_step_case

NAMES = ("hipie_attn_f32_train_forward", "hipie_attn_f32_train_backward", "hipie_attn_f32_train_backward_ws_bytes")
P = [ctypes.c_void_p(4096 * (k + 1)) for k in range(9)]


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


# ------------------------------------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    c_p, c_i, c_l, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.CONSTANTS["HIPIE_ABI_VERSION"] == 13 and lib.hipie_version() == 13
    assert _lib.SIGNATURES[NAMES[0]] == [c_p] * 5 + [c_i] * 4 + [c_l] * 5 + [c_f, c_p] and _lib.RESTYPES[NAMES[0]] is c_i
    assert _lib.SIGNATURES[NAMES[1]] == [c_p] * 9 + [c_l] + [c_i] * 4 + [c_l] * 7 + [c_f, c_p] and _lib.RESTYPES[NAMES[1]] is c_i
    assert _lib.SIGNATURES[NAMES[2]] == [c_i] * 3 and _lib.RESTYPES[NAMES[2]] is c_l
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n]


def test_prototypes_cite_the_reference_code_they_replace():
    text = open(_lib.HEADER_PATH).read()
    for n in NAMES[:2]:
        comment = re.findall(r"/\*(.*?)\*/\s*int %s\(" % n, text, flags=re.S)
        assert len(comment) == 1
        last = comment[0].rsplit("/*", 1)[-1]
        assert "Replaces:" in last, n
        cited = last[last.index("Replaces:"):]                                # the block ENDS with the citation
        assert "deformable_transformer_dino.py:418-436" in cited and "dino_decoder.py:222-248" in cited, n


def test_the_kernel_file_is_built_and_attn_f32_is_left_alone():
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH))
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "attn_f32_train.hip" in srcs and "attn_f32.hip" in srcs
    includes = re.findall(r'#include\s+"([^"]+)"', open(os.path.join(csrc, "attn_f32.hip")).read())
    assert includes == ["common.h"]                                            # the inference kernel shares no header with the training file


# ------------------------------------------------------------------------------------------------ host refusals
def _fwd(qk=P[0], v=P[1], blocked=P[2], out=P[3], lse=P[4], B=2, H=8, N=100, hd=32, qk_sb=100 * 512, qk_st=512, v_sb=100 * 256, v_st=256, m_sb=0):
    return [qk, v, blocked, out, lse, B, H, N, hd, qk_sb, qk_st, v_sb, v_st, m_sb, 32 ** -0.5, None]


def _bwd(qk=P[0], v=P[1], blocked=P[2], out=P[3], lse=P[4], d_out=P[5], d_qk=P[6], d_v=P[7], ws=P[8], ws_bytes=1 << 40, B=2, H=8, N=100, hd=32,
         qk_sb=100 * 512, qk_st=512, v_sb=100 * 256, v_st=256, m_sb=0, do_sb=100 * 256, do_st=256):
    return [qk, v, blocked, out, lse, d_out, d_qk, d_v, ws, ws_bytes, B, H, N, hd, qk_sb, qk_st, v_sb, v_st, m_sb, do_sb, do_st, 32 ** -0.5, None]


def _refused(name, args, message):
    lib = _lib.load()
    assert len(args) == len(_lib.SIGNATURES[name])
    assert getattr(lib, name)(*args) == -22, (name, args)
    assert lib.hipie_last_error() == message, lib.hipie_last_error()


ALIGN = b": pointers must be 16-byte aligned and strides multiples of 4 elements"
STRIDE = b": a row stride below the row's width, or a negative mask stride"
ODD = ctypes.c_void_p(4096 + 4)
CASES = [("hipie_attn_f32_train_forward", _fwd, b"attn_f32_train_forward", ("qk", "v", "out", "lse"), ("qk", "v", "out")),
         ("hipie_attn_f32_train_backward", _bwd, b"attn_f32_train_backward", ("qk", "v", "out", "lse", "d_out", "ws"),
          ("qk", "v", "out", "d_out", "d_qk", "d_v"))]


@pytest.mark.parametrize("entry,make,who,pointers,aligned", CASES, ids=["forward", "backward"])
def test_refusals_by_message(entry, make, who, pointers, aligned):
    for n in pointers:
        _refused(entry, make(**{n: None}), who + b": null pointer")
    for hd in (64, 16, 0, 33):
        _refused(entry, make(hd=hd), who + b": head_dim 32 only (got %d)" % hd)
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(N=0), dict(N=-5)):
        a = dict(B=2, H=8, N=100)
        a.update(kw)
        _refused(entry, make(**kw), who + b": bad shape B=%d H=%d N=%d" % (a["B"], a["H"], a["N"]))
    for n in aligned:
        _refused(entry, make(**{n: ODD}), who + ALIGN)
    for n in ("qk_sb", "qk_st", "v_sb", "v_st"):
        _refused(entry, make(**{n: 514}), who + ALIGN)
    _refused(entry, make(qk_st=508), who + STRIDE)                              # q | k rows of 512 columns
    _refused(entry, make(v_st=252), who + STRIDE)
    _refused(entry, make(m_sb=-4), who + STRIDE)
    # the order of the checks: pointers, head width, shape, alignment, strides
    _refused(entry, make(qk=None, hd=64), who + b": null pointer")
    _refused(entry, make(hd=64, N=0), who + b": head_dim 32 only (got 64)")
    _refused(entry, make(N=0, v=ODD), who + b": bad shape B=2 H=8 N=0")
    _refused(entry, make(v=ODD, qk_st=508), who + ALIGN)
    # a NULL mask is no refusal reason: the call gets as far as the next check
    _refused(entry, make(blocked=None, v_st=252), who + STRIDE)


def test_backward_checks_its_own_strides_and_sizes_its_workspace():
    who = b"attn_f32_train_backward"
    for n in ("do_sb", "do_st"):
        _refused(NAMES[1], _bwd(**{n: 258}), who + ALIGN)
    _refused(NAMES[1], _bwd(do_st=252), who + STRIDE)
    ws = _lib.load().hipie_attn_f32_train_backward_ws_bytes
    assert ws(2, 8, 100) == 2 * 8 * 100 * 4 and ws(2, 8, 1110) == 2 * 8 * 1110 * 4 and ws(1, 1, 1) == 4
    assert ws(0, 8, 100) == 16 and ws(2, 0, 100) == 16 and ws(2, 8, 0) == 16 and ws(-1, 8, 100) == 16
    need = ws(2, 8, 100)
    for kw in (dict(), dict(d_qk=None), dict(d_v=None), dict(d_qk=None, d_v=None)):
        _refused(NAMES[1], _bwd(ws_bytes=need - 1, **kw), who + b": workspace of %d bytes, need %d" % (need - 1, need))
    _refused(NAMES[1], _bwd(ws_bytes=0, do_st=252), who + STRIDE)              # the workspace is the last check


def test_no_gradient_wanted_returns_before_a_launch():
    """the pointers are fake: a launch would fault or fail"""
    lib = _lib.load()
    need = lib.hipie_attn_f32_train_backward_ws_bytes(2, 8, 100)
    assert lib.hipie_attn_f32_train_backward(*_bwd(d_qk=None, d_v=None, ws_bytes=need)) == 0, lib.hipie_last_error()


def test_ops_refuse_host_tensors():
    from hipie_amd import ops
    from hipie_amd.training import functions
    qk, v, d_out = operands(1, 5, 2)
    mask = masks_for(5)["random"]
    out, lse = torch.zeros(1, 5, 64), torch.zeros(1, 2, 5)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.query_attn_train_forward(qk, v, mask, 2, 32 ** -0.5)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.query_attn_train_backward(qk, v, None, out, lse, d_out, 2, 32 ** -0.5)
    assert not functions.query_attention_ok(qk, v, mask, 2)
    assert functions.query_attention(qk, v, mask, 2) is None                    # a host tensor is outside the kernels' limits: the torch form runs
    assert net.HipBackendQueryAttention.query_attention(qk, v, None, 2) is None


# ------------------------------------------------------------------------------------------------ the float64 statement
@pytest.mark.parametrize("mask", ["none", "dn", "random"])
@pytest.mark.parametrize("B,N,heads", [(1, 2, 1), (2, 7, 3), (2, 33, 2)])
def test_backward64_is_torch_autograd(B, N, heads, mask):
    qk, v, d_out = operands(B, N, heads, seed=2)
    blocked = masks_for(N)[mask]
    out, d_qk, d_v = torch_graph(qk, v, blocked, heads, d_out, torch.float64)
    got_out, lse = forward64(qk, v, blocked, heads)
    got = backward64(qk, v, blocked, heads, d_out)
    assert lse.shape == (B, heads, N) and bool(torch.isfinite(lse).all())
    for name, a, b in zip(("out", "d_qk", "d_v"), (got_out,) + got, (out, d_qk, d_v)):
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= 1e-12, (name, err)


def test_statement_of_a_fully_blocked_row():
    """a row with every key blocked: zeros, lse = -inf, and the gradients of the attention with that QUERY removed (it stays a key)"""
    B, N, heads = 2, 9, 2
    qk, v, d_out = operands(B, N, heads, seed=3)
    blocked = masks_for(N)["random"].clone()
    blocked[5] = True
    out, lse = forward64(qk, v, blocked, heads)
    assert bool((out[:, 5] == 0).all()) and bool((lse[:, :, 5] == float("-inf")).all()) and bool(torch.isfinite(out).all())
    rows = torch.tensor([i for i in range(N) if i != 5])
    full, removed = backward64(qk, v, blocked, heads, d_out), backward64(qk, v, blocked, heads, d_out, query_rows=rows)
    assert all(torch.equal(a, b) for a, b in zip(full, removed)) and bool((full[0][:, 5, :heads * 32] == 0).all())
    auto = torch_graph(qk, v, blocked, heads, d_out, torch.float64, query_rows=rows)[1:]
    assert all(float((a - b).abs().max() / b.abs().max()) <= 1e-12 for a, b in zip(removed, auto))


# ------------------------------------------------------------------------------------------------ wiring
def _leaves(sd, *more):
    return list(more) + [sd[n] for n in sorted(sd)]


def _run_layer(be):
    tgt, qpos, refs_in, src, shapes, pad_mask, sd, attn_mask = wiring_case()
    out = net.decoder_layer(tgt, qpos, refs_in, src, shapes, pad_mask, sd, "l.", be, attn_mask)
    g = torch.Generator().manual_seed(11)
    return out, torch.autograd.grad((out * torch.randn(out.shape, generator=g)).sum(), _leaves(sd, tgt, qpos, src))


def _run_mha(be, with_mask):
    tgt, qpos, _, _, _, _, sd, attn_mask = wiring_case()
    out = net.mha(tgt + qpos, tgt, sd, "l.self_attn.", attn_mask if with_mask else None, be=be)
    names = [n for n in sorted(sd) if n.startswith("l.self_attn.")]
    g = torch.Generator().manual_seed(12)
    return out, torch.autograd.grad((out * torch.randn(out.shape, generator=g)).sum(), [tgt, qpos] + [sd[n] for n in names])


def _close(got, want, tol=1e-6):
    return all(float((a - b).detach().abs().max()) <= tol * float(b.detach().abs().max()) for a, b in zip(got, want))


def test_decoder_layer_and_mha_ask_the_backend():
    from _train_step_cases import OracleBackend
    want_out, want_grad = _run_layer(OracleBackend)
    be, rec = standin_backend()
    got_out, got_grad = _run_layer(be)
    assert rec.calls == [((2, 13, 512), (2, 13, 256), True, 8)]                  # q | k from ONE linear, the layer's mask, 8 heads
    assert _close([got_out], [want_out]) and len(got_grad) == len(want_grad) == 3 + 22 and _close(got_grad, want_grad)
    for with_mask in (True, False):
        want = _run_mha(None, with_mask)
        be, rec = standin_backend()
        got = _run_mha(be, with_mask)
        assert rec.calls == [((2, 13, 512), (2, 13, 256), with_mask, 8)]
        assert _close([got[0]], [want[0]]) and _close(got[1], want[1])


def test_a_backend_that_declines_falls_back_bit_for_bit():
    from _train_step_cases import OracleBackend
    want_out, want_grad = _run_layer(OracleBackend)
    be, rec = standin_backend(declines=True)
    got_out, got_grad = _run_layer(be)
    assert len(rec.calls) == 1 and torch.equal(got_out, want_out) and all(torch.equal(a, b) for a, b in zip(got_grad, want_grad))
    want = _run_mha(None, True)
    be, rec = standin_backend(declines=True)
    got = _run_mha(be, True)
    assert len(rec.calls) == 1 and torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))


def test_cpu_train_step_through_the_stand_in_op():
    be, rec = standin_backend()
    z, meta, model, step, batch, targets = train_step_case("cpu", be)
    assert step.be is be
    losses = step.loss_dict(batch, targets)
    total = sum(losses.values())
    total.backward()
    layers = meta["cfg"]["dec_layers"] + meta["cfg"]["md_dec_layers"]
    assert len(rec.calls) == layers and any(c[2] for c in rec.calls)             # one call per decoder layer; the de-noising mask arrives
    assert all(c[3] == 8 and c[0][2] == 512 and c[1][2] == 256 for c in rec.calls)
    check_step_against_golden(z, model, step, losses, total, "cpu", "QUERY ATTENTION stand-in step (cpu)")


# ------------------------------------------------------------------------------------------------ composer
def _public(cls):
    return {n for n in dir(cls) if not n.startswith("_")}


def test_composer_takes_the_later_group_last():
    """membership and relative order in LATER_GROUPS only: the table grows"""
    assert net.LATER_GROUPS["query_attention"] is net.HipBackendQueryAttention and issubclass(net.HipBackendQueryAttention, net.HipBackend)
    assert "query_attention" not in net.GROUPS and "query_attention" not in net.EXTRA_GROUPS
    assert net.backend("query_attention") is net.HipBackendQueryAttention
    assert net.backend("query_attention", "query_attention") is net.HipBackendQueryAttention
    assert _public(net.HipBackendQueryAttention) - _public(net.HipBackend) == {"query_attention"}
    before = net.backend(*net.GROUPS, "group_norms")
    every = net.backend(*net.GROUPS, "group_norms", "query_attention")
    assert every.__bases__ == before.__bases__ + (net.HipBackendQueryAttention,)
    assert before.__bases__[-1] is net.HipBackendGroupNorms and net.backend("query_attention", "group_norms", *net.GROUPS) is every
    assert _public(every) == _public(before) | {"query_attention"} and every.query_attention is net.HipBackendQueryAttention.query_attention
    # composing with it left the classes without it alone
    assert net.backend(*net.GROUPS, "group_norms") is before and "query_attention" not in _public(before)
    assert net.backend(*net.GROUPS).__bases__ == before.__bases__[:-1]
    assert net.backend("norms", "query_attention").__bases__ == (net.HipBackendNorms, net.HipBackendQueryAttention)
    assert net.backend("query_attention", "group_norms").__bases__ == (net.HipBackendGroupNorms, net.HipBackendQueryAttention)
    with pytest.raises(ValueError, match="'fused'.*known: norms, mlp, windows, .*pair_losses, group_norms.*query_attention"):
        net.backend("query_attention", "fused")


def test_bench_train_step_consumes_the_new_flag():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from bench_train_step import EXTRA_FLAGS, FLAGS, LATER_FLAGS, backend_names
    assert LATER_FLAGS["--fused-query-attention"] == "query_attention"
    assert "--fused-query-attention" not in FLAGS and "--fused-query-attention" not in EXTRA_FLAGS
    assert all(net.LATER_GROUPS[g] is not None for g in LATER_FLAGS.values())    # every later flag names a later group
    names, rest = backend_names(["2", "--fused-query-attention", "4"])
    assert names == ["query_attention"] and rest == ["2", "4"]
    names, rest = backend_names(["2", "--fused-query-attention", "--hand-norms", "--fused-group-norms", "--fused-mlp", "4"])
    assert names == ["query_attention", "norms", "group_norms", "mlp"] and rest == ["2", "4"]
    assert net.backend(*names).__bases__ == (net.HipBackendNorms, net.HipBackendMlp, net.HipBackendGroupNorms, net.HipBackendQueryAttention)
