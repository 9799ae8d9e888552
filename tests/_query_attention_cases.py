"""shared by test_query_attention_cpu.py and test_gpu_query_attention.py: the decoders' query self-attention for the training step
(csrc/attn_f32_train.hip) stated in float64 -- the forward with its log-sum-exp in log2 units and the backward by the kernel file's own
formulas, not by autograd --, torch's materialised formulation under autograd (what net.mha runs today), the operand and mask builders, a
plain-torch stand-in for net.HipBackendQueryAttention and the smallest parameter set that runs net.mha / net.decoder_layer.
Everything is drawn in fp32, so a float64 copy holds fp32-representable values."""
import math

import torch

HD = 32
SCALE = HD ** -0.5


# ------------------------------------------------------------------------------------------------ operands and masks
def operands(B, N, heads, seed=0, dev="cpu"):
    """(qk (B, N, 2 C), v (B, N, C), d_out (B, N, C)) fp32 on `dev`, randn * 1.5 (d_out: randn), drawn on the host: column blocks of wider
    buffers, so the row strides exceed the row lengths (and stay multiples of 4 elements, the blocks on 16-byte boundaries)"""
    C = heads * HD
    g = torch.Generator().manual_seed(seed * 7919 + B * 131 + N * 17 + heads)
    wide = (torch.randn(B, N, 3 * C + 8, generator=g) * 1.5).to(dev)
    dwide = torch.randn(B, N, C + 12, generator=g).to(dev)
    return wide[..., :2 * C], wide[..., 2 * C + 4:3 * C + 4], dwide[..., 8:C + 8]


def dn_mask(N, pad, groups):
    """the de-noising self-attention mask of dn.cdn_queries / dn.maskdino_dn_queries: the first `pad` queries are `groups` de-noising groups
    that see only themselves (and the matching queries), the matching queries behind them see no de-noising query.  True = blocked"""
    group = torch.arange(pad) // max(pad // groups, 1)
    mask = torch.zeros(N, N, dtype=torch.bool)
    mask[:pad, :pad] = group[:, None] != group[None, :]
    mask[pad:, :pad] = True
    return mask


def random_mask(N, blocked=0.7, seed=0):
    """a random mask with `blocked` of the pairs blocked and the diagonal forced open: no row is fully blocked"""
    g = torch.Generator().manual_seed(1000 + seed * 31 + N)
    mask = torch.rand(N, N, generator=g) < blocked
    mask[torch.arange(N), torch.arange(N)] = False
    return mask


def masks_for(N):
    """{name: mask} of the operator cases at N tokens; the de-noising pattern: at N = 200 pad = 72 in 4 groups, below that about a third
    of the tokens in as many groups as fit (N = 1: the one matching query)"""
    pad, groups = (72, 4) if N == 200 else (N // 3, max(1, min(3, N // 3)))
    return {"none": None, "dn": dn_mask(N, pad, groups), "random": random_mask(N)}


# ------------------------------------------------------------------------------------------------ the float64 statements
def _heads(t, heads):
    B, N, _ = t.shape
    return t.double().reshape(B, N, heads, HD).transpose(1, 2)              # (B, H, N, 32)


def _rows(t):
    B, H, N, _ = t.shape
    return t.transpose(1, 2).reshape(B, N, H * HD)


def _probabilities64(q, k, blocked):
    """(p (B, H, Nq, Nk), lse (B, H, Nq) in log2 units) of s = SCALE log2(e) q . k: a row with every key blocked has p = 0, lse = -inf"""
    s = (q @ k.transpose(-1, -2)) * (SCALE * math.log2(math.e))
    if blocked is not None:
        s = s.masked_fill(blocked[None, None], float("-inf"))
    m = s.max(-1, keepdim=True)[0]
    e = torch.exp2(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = e.sum(-1, keepdim=True)
    dead = l == 0
    p = torch.where(dead, torch.zeros_like(e), e / torch.where(dead, torch.ones_like(l), l))
    lse = torch.where(dead, torch.full_like(l, float("-inf")), m + torch.log2(torch.where(dead, torch.ones_like(l), l)))
    return p, lse[..., 0]


def forward64(qk, v, blocked, heads):
    """(out (B, N, C), lse (B, H, N)) in float64"""
    C = heads * HD
    p, lse = _probabilities64(_heads(qk[..., :C], heads), _heads(qk[..., C:], heads), blocked)
    return _rows(p @ _heads(v, heads)), lse


def backward64(qk, v, blocked, heads, d_out, query_rows=None):
    """(d_qk (B, N, 2 C), d_v (B, N, C)) in float64 by the kernel file's formulas: p = 2^(s - lse), delta = dO . O, dp = dO v^T,
    ds = p (dp - delta), dq = SCALE ds k, dk = SCALE ds^T q, dv = p^T dO.  query_rows (an index tensor): only these rows act as QUERIES
    (every row stays a key) -- the statement `with the other query rows removed`; their d_q is returned as zeros"""
    C = heads * HD
    q, k, vv, g = _heads(qk[..., :C], heads), _heads(qk[..., C:], heads), _heads(v, heads), _heads(d_out, heads)
    if query_rows is not None:
        q_all, q, g = q, q[:, :, query_rows], g[:, :, query_rows]
        blocked = None if blocked is None else blocked[query_rows]
    p, _ = _probabilities64(q, k, blocked)
    o = p @ vv
    delta = (g * o).sum(-1, keepdim=True)
    # dp by the same elementwise sum as delta, not a matrix product: at N = 1 (p = 1, o = v) the two are then the same float64 operations and
    # ds is EXACTLY zero, as it is in exact arithmetic -- a product's other summation order would leave a 1e-17 residue as the "reference"
    dp = (g[:, :, :, None, :] * vv[:, :, None, :, :]).sum(-1)
    ds = p * (dp - delta)
    dq, dk, dv = SCALE * (ds @ k), SCALE * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ g
    if query_rows is not None:
        full = torch.zeros_like(q_all)
        full[:, :, query_rows] = dq
        dq = full
    return torch.cat((_rows(dq), _rows(dk)), -1), _rows(dv)


def materialised(qk, v, blocked, heads, query_rows=None):
    """net.mha's formulation between its in-projection and out_proj, in the operands' dtype on their device.  query_rows (an index tensor):
    only these rows act as queries (every row stays a key); the result has their rows"""
    B, N, C = v.shape
    sp = lambda t: t.reshape(B, t.shape[1], heads, HD).transpose(1, 2)       # noqa: E731
    q = qk[..., :C]
    if query_rows is not None:
        q, blocked = q[:, query_rows], None if blocked is None else blocked[query_rows]
    a = (sp(q) * SCALE) @ sp(qk[..., C:]).transpose(-1, -2)
    if blocked is not None:
        a = a.masked_fill(blocked[None, None], float("-inf"))
    return (a.softmax(-1) @ sp(v)).transpose(1, 2).reshape(B, q.shape[1], C)


def torch_graph(qk, v, blocked, heads, d_out, dtype, dev="cpu", query_rows=None):
    """(out, d_qk, d_v) of the materialised formulation under torch.autograd in `dtype` on `dev`; query_rows: as in materialised (d_out's
    rows are cut likewise)"""
    qk_, v_ = (t.detach().to(dev, dtype).requires_grad_(True) for t in (qk, v))
    g = d_out.detach().to(dev, dtype)
    if query_rows is not None:
        query_rows = query_rows.to(dev)
        g = g[:, query_rows]
    with torch.enable_grad():
        out = materialised(qk_, v_, None if blocked is None else blocked.to(dev), heads, query_rows)
        grads = torch.autograd.grad(out, (qk_, v_), g)
    return (out.detach(),) + tuple(grads)


# ------------------------------------------------------------------------------------------------ stand-in backends and the wiring case
def _oracle_backend():
    from _train_step_cases import OracleBackend
    return OracleBackend


class TorchQueryAttention:
    """a plain-torch stand-in for net.HipBackendQueryAttention's op that records its calls: (shape of qk, shape of v, mask given, heads)"""

    def __init__(self):
        self.calls = []

    def query_attention(self, qk, v, attn_mask, heads):
        self.calls.append((tuple(qk.shape), tuple(v.shape), attn_mask is not None, heads))
        return materialised(qk, v, attn_mask, heads)


def standin_backend(declines=False):
    """(an OracleBackend subclass with the stand-in `query_attention`, its recorder); declines: the op records and returns None"""
    rec = TorchQueryAttention()

    def op(qk, v, attn_mask, heads):
        y = rec.query_attention(qk, v, attn_mask, heads)
        return None if declines else y
    return type("StandIn", (_oracle_backend(),), {"query_attention": staticmethod(op)}), rec


def wiring_case(seed=5, B=2, N=13, C=256):
    """(tgt, qpos, refs_in, src, shapes, pad_mask, sd, attn_mask) for net.decoder_layer with prefix "l." (net.mha: "l.self_attn."):
    8 heads of 32, four small levels, a de-noising mask over the first 6 queries"""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=0.1):
        return (torch.randn(*shape, generator=g) * scale).requires_grad_(True)
    shapes = [(4, 4), (2, 2), (2, 2), (1, 1)]
    S = sum(h * w for h, w in shapes)
    sd = {"l.self_attn.in_proj_weight": rnd(3 * C, C), "l.self_attn.in_proj_bias": rnd(3 * C), "l.self_attn.out_proj.weight": rnd(C, C),
          "l.self_attn.out_proj.bias": rnd(C), "l.linear1.weight": rnd(64, C), "l.linear1.bias": rnd(64), "l.linear2.weight": rnd(C, 64),
          "l.linear2.bias": rnd(C)}
    for n in ("norm1", "norm2", "norm3"):
        sd.update({"l.%s.weight" % n: rnd(C, scale=1.0), "l.%s.bias" % n: rnd(C)})
    for n, width in (("value_proj", C), ("sampling_offsets", 8 * 4 * 4 * 2), ("attention_weights", 8 * 4 * 4), ("output_proj", C)):
        sd.update({"l.cross_attn.%s.weight" % n: rnd(width, C), "l.cross_attn.%s.bias" % n: rnd(width)})
    tgt, qpos, src = rnd(B, N, C, scale=1.0), rnd(B, N, C, scale=1.0), rnd(B, S, C, scale=1.0)
    refs_in = torch.rand(B, N, 4, 4, generator=g) * 0.5 + 0.25
    pad_mask = torch.zeros(B, S, dtype=torch.bool)
    pad_mask[1, -3:] = True
    return tgt, qpos, refs_in, src, shapes, pad_mask, sd, dn_mask(N, 6, 2)
