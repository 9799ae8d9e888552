"""GPU: the fused windowed training attention (hipie_attn_train_win_forward / _backward, csrc/attn_train_win.hip) against the materialised
formulation in double.  The operands are what hipie_amd/training/net.vit_attention builds for a window (test_gpu_attn_train.py::_operands):
q' = [scale q, rel_h, rel_w], k' = [k, one-hot key row, one-hot key column], head width 80.  Tolerances: the project's own for the same
arithmetic at longer rows (test_gpu_attn_train.py) -- output rel_err < 3e-6, lse < 2e-5 absolute, dq' / dk / dv rel_err < 1e-5, the gradient of
the indicator columns of k' exactly 0.  Every case prints its figures (lines starting with WIN) before it asserts."""
import pytest
import torch

from _layernorm_cases import loss_grads
from _window_cases import vit_case_windows
from test_gpu_act_bwd import _check, _err
from test_gpu_attn_train import _operands
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


# (BH, H, W, upstream gradient scale): 196 = the workload's item (28 masked keys in the last 32-key tile, a partial last query tile); 16 = a
# single key tile, half of it masked; 63 = one short of a tile boundary; 256 = the largest item, no masking, odd BH, 112 columns; 192 = a
# non-square grid, BH no multiple of 8, 112 columns.  BH >= 2: a store past an item's last row lands in the next item.  128 | 129 and
# 224 | 225: the last full item and the first item on each side of the 4 -> 7 and 7 -> 8 wave selection.
SHAPES = [(3, 14, 14, 1.0), (2, 4, 4, 1e-4), (2, 7, 9, 30.0), (5, 16, 16, 1e-4), (9, 8, 24, 30.0),
          (2, 8, 16, 1.0), (2, 3, 43, 30.0), (2, 14, 16, 1e-4), (2, 15, 15, 1.0)]
_REF = {}


def _reference(BH, H, W, gscale):
    """operands, upstream gradient and the double results, computed once per shape and left unchanged"""
    key = (BH, H, W, gscale)
    if key not in _REF:
        qa, ka, v = _operands(BH, H, W, BH * 100 + H)
        g = torch.Generator().manual_seed(5)
        go = torch.randn(v.shape, generator=g, dtype=torch.float64) * gscale
        with torch.enable_grad():
            ql, kl, vl = (t.clone().requires_grad_(True) for t in (qa, ka, v))
            s = ql @ kl.transpose(1, 2)
            out = torch.softmax(s, -1) @ vl
            grads = torch.autograd.grad(out, (ql, kl, vl), go)
        _REF[key] = (qa, ka, v, go, out.detach(), torch.logsumexp(s.detach(), -1), grads)
    return _REF[key]


@pytest.mark.parametrize("BH,H,W,gscale", SHAPES)
def test_forward_vs_materialised(BH, H, W, gscale):
    from hipie_amd import ops
    qa, ka, v, _, want, want_lse, _ = _reference(BH, H, W, gscale)
    f = lambda t: t.float().to(DEV)
    out, lse = ops.attn_train_win_forward(ops.f16_pair(f(qa), 128), ops.f16_pair(f(ka), 128), ops.f16_pair(f(v)))
    assert out.shape == (BH, H * W, 80) and lse.shape == (BH, H * W)
    e, el = rel_err(out.cpu(), want), float((lse.cpu().double() - want_lse).abs().max())
    print("WIN forward (%d,%d,%d): out rel_err %.3e  lse abs %.3e" % (BH, H, W, e, el))
    assert e < 3e-6 and el < 2e-5


@pytest.mark.parametrize("BH,H,W,gscale", SHAPES)
def test_function_gradients_vs_autograd_in_double(BH, H, W, gscale):
    from hipie_amd.training.functions import WindowAttentionFunction, window_attention_ok
    qa, ka, v, go, want_o, _, want = _reference(BH, H, W, gscale)
    dq, dk, dv = (t.float().to(DEV).requires_grad_(True) for t in (qa, ka, v))
    assert window_attention_ok(dq, dk, dv)
    out = WindowAttentionFunction.apply(dq, dk, dv)
    got = torch.autograd.grad(out, (dq, dk, dv), go.float().to(DEV))
    assert got[0].shape == qa.shape and got[1].shape == ka.shape and got[2].shape == v.shape       # dq' with the caller's column count
    errs = (rel_err(out.detach().cpu(), want_o), rel_err(got[0].cpu(), want[0]), rel_err(got[1][..., :80].cpu(), want[1][..., :80]),
            rel_err(got[2].cpu(), want[2]))
    print("WIN function (%d,%d,%d) g %g: out %.3e  dq' %.3e  dk %.3e  dv %.3e" % ((BH, H, W, gscale) + errs))
    assert errs[0] < 3e-6 and errs[1] < 1e-5 and errs[2] < 1e-5 and errs[3] < 1e-5
    assert float(got[1][..., 80:].abs().max()) == 0.0


def _single_token():
    from hipie_amd.training.functions import WindowAttentionFunction
    qa, ka, v = _operands(1, 1, 1, 101)
    g = torch.Generator().manual_seed(5)
    go = torch.randn(v.shape, generator=g, dtype=torch.float64).float()
    dq, dk, dv = (t.float().to(DEV).requires_grad_(True) for t in (qa, ka, v))
    out = WindowAttentionFunction.apply(dq, dk, dv)
    got = torch.autograd.grad(out, (dq, dk, dv), go.to(DEV))
    return qa.float(), ka.float(), v.float(), go, out.detach().cpu(), [t.cpu() for t in got]


def test_single_token_item_is_exact():
    """(BH, H, W) = (1, 1, 1) through WindowAttentionFunction: a softmax over one key -- the output equals v, dq' = 0, dk = 0 and dv = dO, all
    exact (upstream scale 1.0).  The Function takes the closed form for a one-token item; the kernels' own results at N = 1 are bounded in
    test_single_token_kernels_within_tolerance (they carry v and dO as fp16 pairs and cannot be exact)."""
    qa, ka, v, go, out, got = _single_token()
    print("WIN single token: max|out - v| %.3e  max|dq'| %.3e  max|dk| %.3e  max|dv - dO| %.3e" % (
        float((out - v).abs().max()), float(got[0].abs().max()), float(got[1].abs().max()), float((got[2] - go).abs().max())))
    assert out.shape == v.shape and got[0].shape == qa.shape and got[1].shape == ka.shape and got[2].shape == go.shape
    assert torch.equal(out, v)
    assert float(got[0].abs().max()) == 0.0 and float(got[1].abs().max()) == 0.0
    assert torch.equal(got[2], go)


def test_single_token_kernels_within_tolerance():
    """the KERNELS at N = 1 (through the ops, as WindowAttentionFunction drives them for longer items), under the tolerances of the other
    shapes: out against v, lse against the one logit and dv against dO; dq' and dk, whose reference is 0, absolutely: dS = dP - delta is the
    difference of two evaluations of sum_d dO_d v_d, each within the gradient tolerance 1e-5 of sum_d |dO_d v_d|, and dq' = dS k',
    dk = dS q'[:80].  BH = 3: a store past the one row of an item lands in the next item."""
    from hipie_amd import ops
    qa, ka, v = (t.float() for t in _operands(3, 1, 1, 101))
    g = torch.Generator().manual_seed(5)
    go = torch.randn(v.shape, generator=g)
    f = lambda t: t.to(DEV)
    qp, kp = ops.f16_pair(f(qa), 128), ops.f16_pair(f(ka), 128)
    out, lse = ops.attn_train_win_forward(qp, kp, ops.f16_pair(f(v)))
    scale = torch.tensor([4.0], device=DEV)
    delta = (f(go) * out).sum(-1) * scale
    dq, dk, dv = (t.cpu() / 4.0 for t in ops.attn_train_win_backward(qp, kp, ops.f16_pair(f(v), 96), ops.f16_pair(f(go), 96, scale), lse, delta))
    want_lse = (qa.double() * ka.double()).sum(-1)
    ds = 2e-5 * float((go * v).abs().sum(-1).max())
    print("WIN single token kernels: out %.3e  lse %.3e  dv %.3e  max|dq'| %.3e  max|dk| %.3e  (dS bound %.3e)" % (
        rel_err(out.cpu(), v), float((lse.cpu().double() - want_lse).abs().max()), rel_err(dv, go), float(dq.abs().max()), float(dk.abs().max()), ds))
    assert rel_err(out.cpu(), v) < 3e-6 and float((lse.cpu().double() - want_lse).abs().max()) < 2e-5 and rel_err(dv, go) < 1e-5
    assert float(dq.abs().max()) <= ds * float(ka.abs().max()) and float(dk.abs().max()) <= ds * float(qa.abs().max())


def test_masking_does_not_depend_on_what_lies_beyond_the_item():
    """(2, 14, 14): the operands are the first 196 rows of buffers with 224 rows per item, handed over as their own contiguous (BH, 196, .)
    planes (columns 108.. zero, as f16_pair fills them).  Replacing the q' / k' pairs of item 1 by 1e4 must leave item 0's outputs and gradients
    bit-identical: the kernels never read another item's rows as data."""
    from hipie_amd import ops
    BH, N = 2, 196
    g = torch.Generator().manual_seed(77)
    big = [torch.randn(BH, 224, C, generator=g) * s for C, s in ((108, 0.5), (108, 1.0), (80, 1.0), (80, 1.0))]
    qa, ka, v, go = (t[:, :N].contiguous().to(DEV) for t in big)
    scale = torch.tensor([4.0], device=DEV)

    def run(poison):
        qp, kp = [list(ops.f16_pair(t, 128)) for t in (qa, ka)]
        for pl in qp + kp:
            assert pl.shape == (BH, N, 128) and pl.is_contiguous() and float(pl[..., 108:].abs().max()) == 0.0
            if poison:
                pl[1] = 1e4
        out, lse = ops.attn_train_win_forward(qp, kp, ops.f16_pair(v))
        delta = (go * out).sum(-1) * scale
        dq, dk, dv = ops.attn_train_win_backward(qp, kp, ops.f16_pair(v, 96), ops.f16_pair(go, 96, scale), lse, delta)
        return out, lse, dq, dk, dv
    a, b = run(False), run(True)
    for name, x, y in zip(("out", "lse", "dq'", "dk", "dv"), a, b):
        assert bool(torch.isfinite(x[0]).all()), name
        assert torch.equal(x[0], y[0]), name
    assert not torch.equal(a[0][1], b[0][1])                        # the replacement did change item 1


def test_wrapper_coverage():
    from hipie_amd.training.functions import fused_attention, window_attention
    w = [t.float().to(DEV) for t in _operands(4, 14, 14, 1)]
    out = window_attention(*w)
    assert out is not None and out.shape == (4, 196, 80)
    assert fused_attention(*w) is None


def test_vit_backbone_with_fused_windows(monkeypatch):
    """_window_cases.vit_case_windows under HipBackend, HipBackendWindows and HipBackendAll against be=None on the CPU in double: the three
    feature maps, the input gradient and every parameter gradient.  The rule is test_gpu_act_bwd.py::_check (yardstick: the HipBackend error
    on the same device and inputs); on top of it, the error is at most the larger of twice the HipBackend error and 3e-6 (outputs) / 1e-5
    (gradients)."""
    from hipie_amd.training import functions, net
    x, sd, cfg = vit_case_windows(torch.float32)
    names = sorted(sd)

    def run(dev, dtype, be):
        leaves = [t.detach().to(dev, dtype).requires_grad_(True) for t in [x] + [sd[n] for n in names]]
        out = net.vit_backbone(leaves[0], dict(zip(names, leaves[1:])), "", cfg, be)
        outs = [out[k] for k in sorted(out)]
        return outs + list(loss_grads(outs, leaves))
    applied = []
    real = functions.WindowAttentionFunction.apply
    monkeypatch.setattr(functions.WindowAttentionFunction, "apply", lambda *a: applied.append(tuple(a[0].shape)) or real(*a))
    ref = run("cpu", torch.float64, None)
    lib = run(DEV, torch.float32, net.HipBackend)
    assert applied == []
    labels = ["res3", "res4", "res5", "d input"] + ["d " + n for n in names]
    for be in (net.HipBackendWindows, net.HipBackendAll):
        applied.clear()
        got = run(DEV, torch.float32, be)
        assert applied == [(16, 196, 108)]                      # block 1 alone: 2 images x 4 windows x 2 heads
        _check("vit_case_windows %s" % be.__name__, got, ref, lib, labels)
        fails = []
        for i, (n, g_, r, l) in enumerate(zip(labels, got, ref, lib)):
            e, bound = _err(g_, r), max(2 * _err(l, r), 3e-6 if i < 3 else 1e-5)
            if not e <= bound:
                fails.append((n, e, bound))
        assert not fails, (be.__name__, fails)
