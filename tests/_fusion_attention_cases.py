"""shared by test_fusion_attention_cpu.py and test_gpu_fusion_attention.py: the core of the vision-language fusion attention for the training
step (csrc/bi_attn_train.hip) stated in float64 -- forward and backward by the kernel file's own formulas, not by autograd --, the
materialised formulation (net.bi_attention_block's op chain) under autograd with the restated keep factors in F.dropout's place, the
dropout keep function in integer torch ops, the operand and mask builders and a plain-torch stand-in for net.HipBackendFusionAttention.
Everything is drawn in fp32, so a float64 copy holds fp32-representable values."""
import math

import torch

HD = 256
SCALE = HD ** -0.5
LOG2E = 1.4426950408889634
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ operands and masks
def operands(B, Nv, L, heads, seed=0, dev="cpu"):
    """(q, k, vv, vl, d_out_v, d_out_l) fp32 on `dev`: the operands randn * 1.5, the output gradients randn, drawn on the host and cut as
    column blocks of wider buffers, so the row strides exceed the row lengths (multiples of 4 elements, blocks on 16-byte boundaries)"""
    E = heads * HD
    g = torch.Generator().manual_seed(seed * 7919 + B * 131 + Nv * 17 + L * 5 + heads)
    vis = (torch.randn(B, Nv, 2 * E + 8, generator=g) * 1.5).to(dev)
    txt = (torch.randn(B, L, 2 * E + 8, generator=g) * 1.5).to(dev)
    dv = torch.randn(B, Nv, E + 12, generator=g).to(dev)
    dl = torch.randn(B, L, E + 12, generator=g).to(dev)
    return vis[..., :E], txt[..., :E], vis[..., E + 4:2 * E + 4], txt[..., E + 4:2 * E + 4], dv[..., 8:E + 8], dl[..., 4:E + 4]


def masks_for(B, L):
    """{name: (B, L) bool, True = attended}: all attended; a prefix per image (L for image 0, max(1, L // 3) for the others); scattered:
    a random half with token 0 forced attended"""
    prefix = torch.zeros(B, L, dtype=torch.bool)
    prefix[0] = True
    prefix[1:, :max(1, L // 3)] = True
    scattered = torch.rand(B, L, generator=torch.Generator().manual_seed(900 + L)) < 0.5
    scattered[:, 0] = True
    return {"all": torch.ones(B, L, dtype=torch.bool), "prefix": prefix, "scattered": scattered}


# ------------------------------------------------------------------------------------------------ the dropout keep function
def _mix(x):
    """the 32-bit finaliser of csrc/bi_attn_train.hip on int64 tensors holding 32-bit words (int64 products wrap; the low 32 bits are right)"""
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def keep_threshold(r):
    """round(r 2^32) as the kernel forms it; 0 = keep everything"""
    return 0 if r == 0 else int(min(4294967295.0, max(1.0, math.floor(r * 4294967296.0 + 0.5))))


def keep(seed, direction, B, heads, Nv, L, r):
    """(B, heads, Nv, L) bool: keep(seed, direction, b, h, i, j) of the kernels; direction 0 = image -> text, 1 = text -> image"""
    if r == 0:
        return torch.ones(B, heads, Nv, L, dtype=torch.bool)
    lo, hi = seed & M32, (seed >> 32) & M32
    i = torch.arange(Nv, dtype=torch.int64).view(1, 1, Nv, 1)
    j = torch.arange(L, dtype=torch.int64).view(1, 1, 1, L)
    h = torch.arange(heads, dtype=torch.int64).view(1, heads, 1, 1)
    b = torch.arange(B, dtype=torch.int64).view(B, 1, 1, 1)
    x = _mix(i ^ lo)
    x = _mix(x ^ hi ^ (j | (direction << 8) | (h << 9) | (b << 19)))
    return x >= keep_threshold(r)


def keep_factors(seed, B, heads, Nv, L, r, dtype=torch.float64):
    """(kv, kl) (B, heads, Nv, L): 0 or 1 / (1 - r)"""
    return tuple(keep(seed, d, B, heads, Nv, L, r).to(dtype) / (1.0 - r) for d in (0, 1))


# ------------------------------------------------------------------------------------------------ the float64 statements
def _heads(t, heads):
    B, N, _ = t.shape
    return t.double().reshape(B, N, heads, HD).transpose(1, 2)              # (B, H, N, 256)


def _rows(t):
    B, H, N, _ = t.shape
    return t.transpose(1, 2).reshape(B, N, H * HD)


def _probabilities(q, k, att, heads):
    """raw, pv, pl, lse_v, lse_l (log2 units) in float64; an image without attended token: pv = 0, lse_v = -inf"""
    raw = SCALE * (_heads(q, heads) @ _heads(k, heads).transpose(-1, -2))   # (B, H, Nv, L)
    s = raw.clamp(-50000.0, 50000.0)
    a = att.to(s.device).bool()[:, None, None, :]
    sm = s.masked_fill(~a, float("-inf"))
    mx = sm.max(-1, keepdim=True)[0]
    dead = mx == float("-inf")
    e = torch.where(dead | ~a, torch.zeros_like(s), torch.exp(sm - mx.masked_fill(dead, 0.0)))
    sv = e.sum(-1, keepdim=True)
    pv = torch.where(dead, torch.zeros_like(s), e / sv.masked_fill(dead, 1.0))
    lse_v = torch.where(dead, mx, (mx.masked_fill(dead, 0.0) + torch.log(sv.masked_fill(dead, 1.0)))).squeeze(-1) * LOG2E
    lse_v = lse_v.masked_fill(dead.squeeze(-1), float("-inf"))
    ml = s.max(-2, keepdim=True)[0]
    el = torch.exp(s - ml)
    sl = el.sum(-2, keepdim=True)
    return raw, pv, el / sl, lse_v, ((ml + torch.log(sl)) * LOG2E).squeeze(-2)


def forward64(q, k, vv, vl, att, heads, r=0.0, seed=0):
    """(out_v (B, Nv, E), out_l (B, L, E), lse_v (B, H, Nv), lse_l (B, H, L)) in float64 from the formulas; q UNSCALED"""
    B, Nv, L = q.shape[0], q.shape[1], k.shape[1]
    _, pv, pl, lse_v, lse_l = _probabilities(q, k, att, heads)
    kv, kl = keep_factors(seed, B, heads, Nv, L, r)
    return _rows((pv * kv) @ _heads(vl, heads)), _rows((pl * kl).transpose(-1, -2) @ _heads(vv, heads)), lse_v, lse_l


def backward64(q, k, vv, vl, att, heads, d_out_v, d_out_l, r=0.0, seed=0, directions=(True, True)):
    """(d_q, d_k, d_vv, d_vl) in float64 by the kernel file's formulas; directions: (image -> text, text -> image) terms included"""
    B, Nv, L = q.shape[0], q.shape[1], k.shape[1]
    raw, pv, pl, _, _ = _probabilities(q, k, att, heads)
    kv, kl = keep_factors(seed, B, heads, Nv, L, r)
    qh, kh, vvh, vlh, gv, gl = (_heads(t, heads) for t in (q, k, vv, vl, d_out_v, d_out_l))
    if not directions[0]:
        pv = torch.zeros_like(pv)
    if not directions[1]:
        pl = torch.zeros_like(pl)
    out_v, out_l = (pv * kv) @ vlh, (pl * kl).transpose(-1, -2) @ vvh
    dv = (gv * out_v).sum(-1, keepdim=True)                                   # (B, H, Nv, 1)
    dl = (gl * out_l).sum(-1)[:, :, None, :]                                  # (B, H, 1, L)
    ds = pv * (kv * (gv @ vlh.transpose(-1, -2)) - dv) + pl * (kl * (vvh @ gl.transpose(-1, -2)) - dl)
    ds = ds * ((raw >= -50000.0) & (raw <= 50000.0)).double()
    return (_rows(SCALE * (ds @ kh)), _rows(SCALE * (ds.transpose(-1, -2) @ qh)), _rows((pl * kl) @ gl), _rows((pv * kv).transpose(-1, -2) @ gv))


# ------------------------------------------------------------------------------------------------ the materialised formulation
def materialised(q, k, vv, vl, att, heads, r=0.0, seed=0):
    """net.bi_attention_block's op chain between the projections, in the operands' dtype: q UNSCALED (the chain scales it), the restated
    keep factors in F.dropout's place -> (out_v, out_l)"""
    B, Nv, E = q.shape
    L = k.shape[1]
    hd = E // heads

    def split(t, n):
        return t.reshape(B, n, heads, hd).transpose(1, 2).reshape(B * heads, n, hd)
    qs, ks, vvs, vls = split(q * hd ** -0.5, Nv), split(k, L), split(vv, Nv), split(vl, L)
    w = torch.bmm(qs, ks.transpose(1, 2)).clamp(min=-50000).clamp(max=50000)
    wT = w.transpose(1, 2)
    wl = (wT - torch.max(wT, dim=-1, keepdim=True)[0]).clamp(min=-50000).clamp(max=50000).softmax(dim=-1)
    am = att.to(torch.int64)[:, None, None, :].expand(B, 1, Nv, L)
    am = am.masked_fill(am == 0, int(-9e15))
    wv = torch.softmax((w.view(B, heads, Nv, L) + am).view(B * heads, Nv, L), dim=-1)
    if r > 0:
        kv, kl = keep_factors(seed, B, heads, Nv, L, r, q.dtype)
        wv = wv * kv.to(q.device).reshape(B * heads, Nv, L)
        wl = wl * kl.to(q.device).reshape(B * heads, Nv, L).transpose(1, 2)
    ov = torch.bmm(wv, vls).view(B, heads, Nv, hd).transpose(1, 2).reshape(B, Nv, E)
    ol = torch.bmm(wl, vvs).view(B, heads, L, hd).transpose(1, 2).reshape(B, L, E)
    return ov, ol


def torch_graph(q, k, vv, vl, att, heads, d_out_v, d_out_l, dtype, dev="cpu", r=0.0, seed=0):
    """(out_v, out_l, d_q, d_k, d_vv, d_vl) of the materialised formulation under torch.autograd in `dtype` on `dev`"""
    leaves = [t.detach().to(dev, dtype).requires_grad_(True) for t in (q, k, vv, vl)]
    with torch.enable_grad():
        ov, ol = materialised(*leaves, att.to(dev), heads, r, seed)
        grads = torch.autograd.grad((ov, ol), leaves, (d_out_v.detach().to(dev, dtype), d_out_l.detach().to(dev, dtype)))
    return (ov.detach(), ol.detach()) + tuple(grads)


def clamp_case(B, Nv, L, heads, seed=0, dev="cpu"):
    """the operands with k := sgn |k| for a fixed +-1 pattern over the 256 columns, visual row 0 = 1e4 sgn and row 1 = -1e4 sgn: every
    logit of row 0 is above 50000 and every logit of row 1 below -50000"""
    q, k, vv, vl, gv, gl = operands(B, Nv, L, heads, seed, dev)
    sgn = (1.0 - 2.0 * ((torch.arange(heads * HD) * 7 // 3) % 2)).to(dev)
    q, k = q.clone(), k.abs() * sgn
    q[:, 0] = 1e4 * sgn
    q[:, 1] = -1e4 * sgn
    return q, k, vv, vl, gv, gl


# ------------------------------------------------------------------------------------------------ a stand-in backend
class TorchFusionAttention:
    """a plain-torch stand-in for net.HipBackendFusionAttention's op that records its calls: (q, heads, dropout)"""

    def __init__(self):
        self.calls = []

    def fusion_attention(self, q, k, vv, vl, text_mask, heads, dropout):
        self.calls.append((q.detach().clone(), heads, dropout))
        return materialised(q, k, vv, vl, text_mask, heads)


def standin_backend(declines=False, base=object):
    """(a class with the stand-in `fusion_attention` on top of `base`, its recorder); declines: the op records and returns None"""
    rec = TorchFusionAttention()

    def op(q, k, vv, vl, text_mask, heads, dropout):
        y = rec.fusion_attention(q, k, vv, vl, text_mask, heads, dropout)
        return None if declines else y
    return type("StandIn", (base,), {"fusion_attention": staticmethod(op)}), rec


def block_case(seed=3, B=2, Nv=21, L=6, C=256, Cl=768, heads=2):
    """(v, l, text_mask, sd) for net.bi_attention_block with prefix "b.": embed width heads * 256"""
    g = torch.Generator().manual_seed(seed)
    E = heads * HD

    def rnd(*shape, scale=0.05):
        return torch.randn(*shape, generator=g) * scale
    sd = {"b.gamma_v": rnd(C, scale=1.0), "b.gamma_l": rnd(Cl, scale=1.0)}
    for n, width in (("layer_norm_v", C), ("layer_norm_l", Cl)):
        sd.update({"b.%s.weight" % n: 1.0 + rnd(width), "b.%s.bias" % n: rnd(width)})
    for n, (o, i) in (("v_proj", (E, C)), ("l_proj", (E, Cl)), ("values_v_proj", (E, C)), ("values_l_proj", (E, Cl)), ("out_v_proj", (C, E)), ("out_l_proj", (Cl, E))):
        sd.update({"b.attn.%s.weight" % n: rnd(o, i), "b.attn.%s.bias" % n: rnd(o)})
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, L // 2:] = 0
    return torch.randn(B, Nv, C, generator=g), torch.randn(B, L, Cl, generator=g), mask, sd
