"""shared by the tests of the one-node MLP (test_gpu_act_bwd.py): a ViT and a deformable-encoder-layer parameter set like the ones of
_layernorm_cases.py, but WIDE enough for functions.split_mlp to take its fused path -- widths that are multiples of 32 and at least 256
token rows (the cases of _layernorm_cases.py have 60 and 38 rows: there the backend's mlp falls through to the three nodes).  Everything
is drawn in fp32 and returned as leaves of ``dtype``."""
import torch

from _layernorm_cases import _leaf_maker


def vit_case_wide(dtype):
    """depth 3 (block 1 windowed), width 32, 2 heads, hidden 128, a 12 x 11 token grid with window 4 (padded to 12 x 12), 2 images: 264 token
    rows in the global blocks, 288 in the windowed one -> (image, sd, cfg)"""
    rnd = _leaf_maker(31, dtype)
    C, heads, depth, patch, win = 32, 2, 3, 2, 4
    gh, gw = 12, 11
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


def encoder_case_wide(dtype):
    """one DeformableTransformerEncoderLayer of width 256 with a 64-wide FFN (8 heads, 4 levels, 4 points), 2 images of 161 pyramid tokens
    (322 rows), two padded tokens -> (src, pos, reference points, shapes, pad_mask, sd)"""
    from hipie_amd.training import net
    rnd = _leaf_maker(32, dtype)
    C, ffn, B = 256, 64, 2
    shapes = [(12, 10), (6, 5), (3, 3), (2, 1)]
    S = sum(h * w for h, w in shapes)
    sd = {"self_attn.value_proj.weight": rnd(C, C, scale=0.06), "self_attn.value_proj.bias": rnd(C),
          "self_attn.sampling_offsets.weight": rnd(8 * 4 * 4 * 2, C, scale=0.02), "self_attn.sampling_offsets.bias": rnd(8 * 4 * 4 * 2, scale=1.0),
          "self_attn.attention_weights.weight": rnd(8 * 4 * 4, C, scale=0.06), "self_attn.attention_weights.bias": rnd(8 * 4 * 4),
          "self_attn.output_proj.weight": rnd(C, C, scale=0.06), "self_attn.output_proj.bias": rnd(C),
          "norm1.weight": rnd(C, scale=1.0), "norm1.bias": rnd(C), "norm2.weight": rnd(C, scale=1.0), "norm2.bias": rnd(C),
          "linear1.weight": rnd(ffn, C, scale=0.06), "linear1.bias": rnd(ffn), "linear2.weight": rnd(C, ffn, scale=0.1), "linear2.bias": rnd(C)}
    src, pos = rnd(B, S, C, scale=1.0), rnd(B, S, C)
    pad = torch.zeros(B, S, dtype=torch.bool)
    pad[1, -2:] = True
    refs = net.encoder_ref_points(shapes, torch.ones(B, 4, 2, dtype=dtype))
    return src, pos, refs, shapes, pad, sd
