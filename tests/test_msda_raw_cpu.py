"""CPU: the host side of the deformable-attention node from the raw projections -- the refusals of hipie_msda_raw_backward (no launch), its
workspace query, the host-checked declines of functions.deform_sample, the conditioning of the inputs the GPU file uses, and msda_module's
unchanged graph for a backend without msda_raw."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _msda_raw_cases as cases
from hipie_amd import _lib
from util import rel_err


def test_msda_raw_backward_refusals_without_a_launch():
    """every host refusal of hipie_msda_raw_backward: -22 and its message, nothing launched (the pointers are not memory)"""
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    M, D, L, P, Lq, S = 8, 32, 4, 4, 3, 64
    offw, logw = M * L * P * 2, M * L * P

    def call(S=S, M=M, D=D, L=L, P=P, ref_dim=2, strides=None, ptrs=None, ws=p, ws_bytes=0, gref=p):
        strides = strides or (M * L * P * 2, M * L * P, M * L * P * 2, M * L * P)
        ptrs = ptrs or [p] * 10                          # value, shapes, level_start, ref, offsets, logits, gout, gvalue, goff, glogit
        return lib.hipie_msda_raw_backward(*ptrs, gref, 1, S, M, D, L, Lq, P, ref_dim, *strides, ws, ws_bytes, None)

    for d in (64, 16, 31):
        assert call(D=d) == -22 and b"D=%d" % d in lib.hipie_last_error()
    assert call(S=40961) == -22 and b"S=40961 pixel rows" in lib.hipie_last_error()
    assert call(L=3, P=11) == -22 and b"L*P=33 > 32" in lib.hipie_last_error()
    for ref_dim in (3, 0, 1, 5):
        assert call(ref_dim=ref_dim) == -22 and b"ref_dim must be 2 or 4 (got %d)" % ref_dim in lib.hipie_last_error()
    for k in range(4):
        strides = [offw, logw, offw, logw]
        strides[k] -= 1
        assert call(strides=tuple(strides)) == -22 and b"row stride" in lib.hipie_last_error(), k
        assert (b"offsets" if k % 2 == 0 else b"logits") in lib.hipie_last_error()
    for k in range(10):
        ptrs = [p] * 10
        ptrs[k] = None
        assert call(ptrs=ptrs) == -22 and b"null pointer" in lib.hipie_last_error(), k
    # the workspace: absent, too small (with and without grad_ref the size that is needed differs, and the message names it)
    for gref in (p, None):
        need = lib.hipie_msda_raw_backward_ws_bytes(1, S, M, L, Lq, P, 2, int(gref is not None))
        assert call(ws=None, ws_bytes=need, gref=gref) == -22 and b"%d needed" % need in lib.hipie_last_error()
        assert call(ws_bytes=need - 1, gref=gref) == -22 and b"workspace of %d bytes, %d needed" % (need - 1, need) in lib.hipie_last_error()
    assert call(ws=ctypes.c_void_p(264), ws_bytes=1 << 40) == -22 and b"16-byte aligned" in lib.hipie_last_error()
    # an empty batch is a no-op even with null data pointers
    assert lib.hipie_msda_raw_backward(*[None] * 11, 0, S, M, D, L, Lq, P, 2, offw, logw, offw, logw, None, 0, None) == 0


def test_msda_raw_backward_ws_bytes():
    lib = _lib.load()
    q = lib.hipie_msda_raw_backward_ws_bytes
    for bad in ((0, 64, 8, 4, 3, 4, 2, 1), (1, 0, 8, 4, 3, 4, 2, 1), (1, 64, 0, 4, 3, 4, 2, 1), (1, 64, 8, 0, 3, 4, 2, 1), (1, 64, 8, 4, -1, 4, 2, 1),
                (1, 64, 8, 4, 3, 0, 2, 1), (1, 64, 8, 4, 3, 4, 3, 1), (1, 64, 8, 3, 3, 11, 2, 1), (1, 40961, 8, 4, 3, 4, 2, 1)):
        assert q(*bad) == 0, bad
    for B, S, M, L, Lq, P in ((2, 1008, 8, 3, 1203, 4), (2, 21760, 8, 4, 21760, 4), (3, 1008, 16, 3, 517, 2), (2, 2125, 8, 4, 7, 4)):
        for ref_dim in (2, 4):
            without, with_ref = q(B, S, M, L, Lq, P, ref_dim, 0), q(B, S, M, L, Lq, P, ref_dim, 1)
            assert lib.hipie_msda_backward_workspace(B, S, M, L, Lq, P) <= without < with_ref
            assert with_ref - without >= B * Lq * M * L * ref_dim * 4                  # the per-head partials of grad_ref


def test_deform_sample_declines_on_the_host_without_a_library_call(monkeypatch):
    """what the entry would refuse is answered None before anything is called (the tensors are host tensors: also declined)"""
    from hipie_amd import ops
    from hipie_amd.training import functions

    def no_call(*a, **k):
        raise AssertionError("a library call")
    monkeypatch.setattr(ops, "_call", no_call)
    monkeypatch.setattr(ops, "_size", no_call)
    monkeypatch.setattr(ops, "msda_fused", no_call)
    shapes = [(4, 4), (2, 2)]

    def args(D=32, S=20, L=2, P=4, ref_dim=2, dtype=torch.float32, device="cpu"):
        return (torch.zeros(1, S, 8, D, dtype=dtype, device=device), shapes, torch.zeros(1, 5, L, ref_dim, dtype=dtype, device=device),
                torch.zeros(1, 5, 8, L, P, 2, dtype=dtype, device=device), torch.zeros(1, 5, 8, L * P, dtype=dtype, device=device))
    for kw in (dict(), dict(D=64), dict(dtype=torch.float64), dict(S=functions.MSDA_RAW_MAX_ROWS + 1), dict(L=3, P=11), dict(ref_dim=3),
               dict(device="meta"), dict(device="meta", D=64), dict(device="meta", dtype=torch.float64), dict(device="meta", dtype=torch.float16)):
        assert functions.deform_sample(*args(**kw)) is None, kw
    # shape-only checks, seen through tensors that claim to be fp32 device tensors
    class Claims(torch.Tensor):
        is_cuda = True
    v, _, r, o, lg = args()
    as_dev = lambda t: t.as_subclass(Claims)
    assert functions.deform_sample_ok(as_dev(v), as_dev(r), as_dev(o), as_dev(lg))
    for kw in (dict(D=64), dict(S=functions.MSDA_RAW_MAX_ROWS + 1), dict(L=3, P=11), dict(ref_dim=3), dict(dtype=torch.float64)):
        v, _, r, o, lg = args(**kw)
        assert not functions.deform_sample_ok(as_dev(v), as_dev(r), as_dev(o), as_dev(lg)), kw
    v, _, r, o, lg = args()
    wide = torch.zeros(1, 5, 8 * 2 * 4 * 2 + 8 * 2 * 4)            # both projections as column blocks of one buffer: taken
    assert functions.deform_sample_ok(as_dev(v), as_dev(r), as_dev(wide[..., :128].view(1, 5, 8, 2, 4, 2)), as_dev(wide[..., 128:].view(1, 5, 8, 8)))
    assert not functions.deform_sample_ok(as_dev(v), as_dev(r), as_dev(o.transpose(3, 4).contiguous().transpose(3, 4)), as_dev(lg))
    assert not functions.deform_sample_ok(as_dev(v.transpose(1, 2).contiguous().transpose(1, 2)), as_dev(r), as_dev(o), as_dev(lg))


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_inputs_are_well_conditioned(case):
    """the composition in fp32 torch stays within 1e-5 of float64 on all four gradients -- half the GPU file's bound, so its inputs, not the
    kernel, are shown to be well conditioned -- and the fp32 locations stay >= 0.04 px from a pixel boundary"""
    c = cases.build(case)
    want, got = cases.gradients(c, torch.float64), cases.gradients(c, torch.float32)
    errs = [rel_err(g, w) for g, w in zip(got, want)]
    dist = cases.boundary_distance(c)
    print("%s: fp32 composition vs float64: value %.1e offsets %.1e logits %.1e ref %.1e; %.3f px from a boundary" % (case, *errs, dist))
    assert max(errs) < 1e-5, errs
    assert dist >= 0.04
    if case == "all_outside":
        assert all(float(w.abs().max()) == 0.0 for w in want)
    else:
        assert all(float(w.abs().max()) > 0.0 for w in want)


class _OracleBackend:
    """the operator as the oracle's CPU restatement (test_training._OracleBackend's msda): a backend WITHOUT msda_raw"""

    @staticmethod
    def msda(value, shapes, loc, aw):
        from oracle import ops as oo
        return oo.ms_deform_attn_core(value, shapes, loc, aw)


def _parent_msda_module(query, ref_points, src, shapes, pad_mask, sd, p, be, heads=8, levels=4, points=4):
    """msda_module as it stood before the node existed, line for line"""
    from hipie_amd.training.net import level_tensors, lin
    N, Lq, C = query.shape
    S = src.shape[1]
    value = lin(src, sd, p + "value_proj.")
    if pad_mask is not None:
        value = value.masked_fill(pad_mask[..., None], 0.0)
    value = value.view(N, S, heads, C // heads)
    off = lin(query, sd, p + "sampling_offsets.").view(N, Lq, heads, levels, points, 2)
    aw = F.softmax(lin(query, sd, p + "attention_weights.").view(N, Lq, heads, levels * points), -1).view(N, Lq, heads, levels, points)
    if ref_points.shape[-1] == 2:
        loc = ref_points[:, :, None, :, None, :] + off / level_tensors(shapes, query.device, "wh")[None, None, None, :, None, :]
    else:
        loc = ref_points[:, :, None, :, None, :2] + off / points * ref_points[:, :, None, :, None, 2:] * 0.5
    return lin(be.msda(value, shapes, loc, aw), sd, p + "output_proj.")


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_msda_module_without_msda_raw_is_the_parent_graph(ref_dim):
    """a backend that lacks msda_raw, and one whose msda_raw declines, give the parent's output and gradients bit for bit; the declining
    backend was handed the two raw projections as views"""
    from hipie_amd.training import net
    shapes = [(6, 8), (3, 4)]
    N, Lq, C, heads, L, P = 2, 11, 64, 8, 2, 4
    S = sum(h * w for h, w in shapes)
    g = torch.Generator().manual_seed(5)
    sd = {}
    for name, n_out in (("value_proj.", C), ("sampling_offsets.", heads * L * P * 2), ("attention_weights.", heads * L * P), ("output_proj.", C)):
        sd["a." + name + "weight"] = (torch.randn(n_out, C, generator=g) * 0.2).requires_grad_(True)
        sd["a." + name + "bias"] = (torch.randn(n_out, generator=g) * 0.2).requires_grad_(True)
    query, src = torch.randn(N, Lq, C, generator=g).requires_grad_(True), torch.randn(N, S, C, generator=g).requires_grad_(True)
    ref = torch.rand(N, Lq, L, ref_dim, generator=g).requires_grad_(True)
    pad = torch.zeros(N, S, dtype=torch.bool)
    pad[1, -5:] = True
    gout = torch.randn(N, Lq, C, generator=g)
    leaves = [query, src, ref] + list(sd.values())
    seen = []

    class Declines(_OracleBackend):
        @staticmethod
        def msda_raw(value, shapes_, ref_, offsets, logits):
            seen.append((tuple(value.shape), tuple(offsets.shape), tuple(logits.shape), offsets._base is not None, logits._base is not None))
            return None

    with torch.enable_grad():
        want = _parent_msda_module(query, ref, src, shapes, pad, sd, "a.", _OracleBackend, heads, L, P)
        gwant = torch.autograd.grad(want, leaves, gout)
        for be in (_OracleBackend, Declines):
            got = net.msda_module(query, ref, src, shapes, pad, sd, "a.", be, heads, L, P)
            ggot = torch.autograd.grad(got, leaves, gout)
            assert torch.equal(got, want) and all(torch.equal(a, b) for a, b in zip(ggot, gwant)), be
    assert seen == [((N, S, heads, C // heads), (N, Lq, heads, L, P, 2), (N, Lq, heads, L * P), True, True)]
    assert not hasattr(net.HipBackend, "msda_raw") and hasattr(net.HipBackendDeformable, "msda_raw")
