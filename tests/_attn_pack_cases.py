"""shared by test_attn_pack_cpu.py and test_gpu_attn_pack.py: the shapes of the packed ViT attention (functions.VitAttentionFunction,
csrc/attn_pack.hip), their inputs, and `composition`: net.vit_attention between its two linears, restated from (qkv, Rh, Rw) operation for
operation -- the float64 reference on the host, the graph of today's backends on the device, and the stand-in backend of the wiring test
(which also checks that the restatement IS net.vit_attention's graph: equal outputs and gradients).  Everything is drawn in fp32, so an fp64
copy holds fp32-representable values."""
import torch

# (B', heads, H, W); heads = 3: not a power of two.  33 x 35: N = 1155 -> 1280 rows, cq + 1 = 149 puts the tail inside an 8-column vector
GLOBAL = [(1, 1, 8, 16), (2, 3, 16, 16), (1, 2, 32, 32)]
PADDED = [(1, 2, 33, 35)]
WINDOW = [(3, 2, 14, 14), (2, 1, 5, 7)]
ALL = [(s, False) for s in GLOBAL + PADDED] + [(s, True) for s in WINDOW]          # (shape, windows)
HD = 80


def inputs(B, heads, H, W, seed=0, extremes=False):
    """qkv (B', H W, 3 heads 80) and the rel-pos tables (2 H - 1, 80), (2 W - 1, 80); extremes: entries of +-1e6 in q and k (beyond fp16)"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 31 * heads + 7 * H + W)
    qkv = torch.randn(B, H * W, 3 * heads * HD, generator=g) * 0.5
    tab_h, tab_w = torch.randn(2 * H - 1, HD, generator=g) * 0.2, torch.randn(2 * W - 1, HD, generator=g) * 0.2
    if extremes:
        flat = qkv.view(B, H * W, 3, heads * HD)
        flat[0, 0, 0, 0], flat[0, 1, 0, 5], flat[-1, -1, 0, -1] = 1e6, -1e6, 1e6
        flat[0, 0, 1, 3], flat[0, 2, 1, 9], flat[-1, -1, 1, -2] = -1e6, 1e6, -1e6
    return qkv, tab_h, tab_w


def operands(qkv, Rh, Rw, heads, H, W):
    """(q, k, v, rq, rel_h, rel_w, qa, ka) as net.vit_attention builds them"""
    from hipie_amd.training import net
    B = qkv.shape[0]
    hd = qkv.shape[-1] // (3 * heads)
    t = qkv.reshape(B, H * W, 3, heads, -1).permute(2, 0, 3, 1, 4)
    q, k, v = t.reshape(3, B * heads, H * W, -1).unbind(0)
    rq = q.reshape(B * heads, H, W, hd)
    rel_h = torch.einsum("bhwc,hkc->bhwk", rq, Rh).reshape(B * heads, H * W, H)
    rel_w = torch.einsum("bhwc,wkc->bhwk", rq, Rw).reshape(B * heads, H * W, W)
    qa = torch.cat((q * hd ** -0.5, rel_h, rel_w), -1)
    ka = torch.cat((k, net._key_axis_indicators(H, W, k.device, k.dtype).expand(B * heads, -1, -1)), -1)
    return q, k, v, rq, rel_h, rel_w, qa, ka


def composition(qkv, Rh, Rw, heads, H, W, be=None):
    """net.vit_attention from behind the qkv linear to in front of the proj linear (FOLD_REL_POS on) -> (B', H W, heads hd)"""
    B = qkv.shape[0]
    q, k, v, rq, rel_h, rel_w, qa, ka = operands(qkv, Rh, Rw, heads, H, W)
    fused, windows = getattr(be, "fused_attention", None), getattr(be, "window_attention", None)
    o = None
    if fused is not None:
        o = fused(qa, ka, v)
    if o is None and windows is not None:
        o = windows(qa, ka, v)
    if o is None:
        o = (qa @ ka.transpose(-2, -1)).softmax(dim=-1) @ v
    return o.view(B, heads, H, W, -1).permute(0, 2, 3, 1, 4).reshape(B, H * W, -1)


def vit_case_packed(dtype):
    """a ViT whose blocks the packed node covers: depth 2 (block 0 global, block 1 windowed), width 160 = 2 heads of 80, an 8 x 16 token grid
    (N = 128) cut into 4 x 4 windows without padding, 2 images (256 token rows: the split GEMM's linears) -> (image, sd, cfg)"""
    from _layernorm_cases import _leaf_maker
    rnd = _leaf_maker(21, dtype)
    C, heads, depth, patch, win = 160, 2, 2, 2, 4
    gh, gw = 8, 16
    cfg = dict(vit_patch=patch, vit_depth=depth, vit_window=win, vit_window_blocks=[1], vit_heads=heads)
    s = C ** -0.5
    sd = {"patch_embed.proj.weight": rnd(C, 3, patch, patch), "patch_embed.proj.bias": rnd(C), "pos_embed": rnd(1, 1 + 4 * 4, C),
          "fpn1.0.weight": rnd(C, C, 2, 2, scale=s), "fpn1.0.bias": rnd(C)}
    for i in range(depth):
        bp = "blocks.%d." % i
        rh, rw = (win, win) if i in cfg["vit_window_blocks"] else (gh, gw)
        sd.update({bp + "norm1.weight": rnd(C, scale=1.0), bp + "norm1.bias": rnd(C), bp + "norm2.weight": rnd(C, scale=1.0), bp + "norm2.bias": rnd(C),
                   bp + "attn.qkv.weight": rnd(3 * C, C, scale=s), bp + "attn.qkv.bias": rnd(3 * C), bp + "attn.proj.weight": rnd(C, C, scale=s),
                   bp + "attn.proj.bias": rnd(C), bp + "attn.rel_pos_h": rnd(2 * rh - 1, C // heads), bp + "attn.rel_pos_w": rnd(2 * rw - 1, C // heads),
                   bp + "mlp.fc1.weight": rnd(4 * C, C, scale=s), bp + "mlp.fc1.bias": rnd(4 * C), bp + "mlp.fc2.weight": rnd(C, 4 * C, scale=s / 2),
                   bp + "mlp.fc2.bias": rnd(C)})
    x = rnd(2, 3, gh * patch, gw * patch, scale=1.0)
    return x, sd, cfg
