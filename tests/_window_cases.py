"""shared by the tests of the fused windowed training attention (test_gpu_attn_train_win.py): a ViT parameter set like
_act_cases.vit_case_wide, but with the head width (80) and the window (14 x 14 = 196 tokens) of the product's ViT-H, so that the windowed
block runs functions.WindowAttentionFunction.  Everything is drawn in fp32 and returned as leaves of ``dtype``."""
from _layernorm_cases import _leaf_maker


def vit_case_windows(dtype):
    """depth 3 (block 1 windowed), width 160, 2 heads (head width 80), hidden 640, a 20 x 17 token grid with window 14 (padded to 28 x 28: 4
    windows per image), patch 2, 2 images: 680 token rows in the global blocks (340-token items: neither fused path takes them), 16 items of
    196 tokens and 108 operand columns in the windowed one -> (image, sd, cfg)"""
    rnd = _leaf_maker(41, dtype)
    C, heads, depth, patch, win = 160, 2, 3, 2, 14
    gh, gw = 20, 17
    hd = C // heads
    cfg = dict(vit_patch=patch, vit_depth=depth, vit_window=win, vit_window_blocks=[1], vit_heads=heads)
    sd = {"patch_embed.proj.weight": rnd(C, 3, patch, patch), "patch_embed.proj.bias": rnd(C), "pos_embed": rnd(1, 1 + 4 * 4, C),
          "fpn1.0.weight": rnd(C, C, 2, 2, scale=0.2), "fpn1.0.bias": rnd(C)}
    for i in range(depth):
        bp = "blocks.%d." % i
        rh, rw = (win, win) if i in cfg["vit_window_blocks"] else (gh, gw)
        sd.update({bp + "norm1.weight": rnd(C, scale=1.0), bp + "norm1.bias": rnd(C), bp + "norm2.weight": rnd(C, scale=1.0), bp + "norm2.bias": rnd(C),
                   bp + "attn.qkv.weight": rnd(3 * C, C, scale=0.2), bp + "attn.qkv.bias": rnd(3 * C), bp + "attn.proj.weight": rnd(C, C, scale=0.2),
                   bp + "attn.proj.bias": rnd(C), bp + "attn.rel_pos_h": rnd(2 * rh - 1, hd), bp + "attn.rel_pos_w": rnd(2 * rw - 1, hd),
                   bp + "mlp.fc1.weight": rnd(4 * C, C, scale=0.2), bp + "mlp.fc1.bias": rnd(4 * C), bp + "mlp.fc2.weight": rnd(C, 4 * C, scale=0.1),
                   bp + "mlp.fc2.bias": rnd(C)})
    x = rnd(2, 3, gh * patch, gw * patch, scale=1.0)
    return x, sd, cfg
