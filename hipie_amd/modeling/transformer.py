"""Language-fused Deformable-DETR/DINO "thing" branch.

Mirrors, with the reference's parameter names:
  hipie/models/deformable_detr/deformable_transformer_dino.py  (DeformableTransformerVLDINO, encoder/decoder layers, MLP,
                                                               FeatureResizer, get_sine_pos_embed)
  hipie/models/deformable_detr/ops/modules/ms_deform_attn.py   (MSDeformAttn -> hipie_msda_fused_forward)
  hipie/models/deformable_detr/fuse_helper.py, vlfusion.py     (BiMultiHeadAttention -> hipie_bi_xattn)
  hipie/models/deformable_detr/deformable_detr.py              (VL_Align, Still_Classifier, DeformableDETRDINO)
  hipie/models/deformable_detr/position_encoding.py, backbone.py, hipie/backbone/masked_backbone.py
Inference only.  Residual streams, LayerNorm/GroupNorm, softmax and all geometry stay fp32; linears/convs run in the
policy's ``head`` dtype (fp32 by default, like the reference's custom_fwd(cast_inputs=float32)).
"""
import collections
import copy
import os
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..derived import derived


# --------------------------------------------------------------------------- policy-aware primitives
def _lin(owner, key, x, w, b, act=ops.ACT_NONE, out_fmt=ops.F32, x_hl8=False, rows=None):
    """F.linear(x, w, b) in the weight's dtype -- or, when ``owner.split`` is set (Precision.split3: set_split below), the same product
    at fp32-class accuracy on hipie_gemm's split-fp16 operands (the HL8 copy of ``w`` is cached on ``owner`` under ``key``).
    ``rows``: the slice of output features to compute; ``w`` / ``b`` stay the whole parameters, which is what the cache watches."""
    if getattr(owner, "split", False) and x.is_cuda and w.dtype == torch.float32 and ops.split_ok(w.shape[1] if not x_hl8 else w.shape[1]):
        fns = {} if rows is None else dict(weight_fn=lambda: w[rows], bias_fn=lambda: b[rows])
        return ops.split_linear(x, owner, key, w, b, act=act, out_fmt=out_fmt, x_hl8=x_hl8, **fns)
    if rows is not None:
        w, b = w[rows], b[rows]
    y = F.linear(x.to(w.dtype), w, b)
    return F.relu(y) if act == ops.ACT_RELU else y


def set_split(module, on=True):
    """Precision.split3: every linear of ``module`` runs as the split-fp16 GEMM (weights stay fp32 parameters)."""
    for m in module.modules():
        m.split = bool(on)
    return module


class PLinear(nn.Linear):
    """nn.Linear whose GEMM runs in the weight's dtype; input is cast in, output returned in ``out_dtype`` (fp32 unless
    the policy stores activations in 16 bit).  With ``split`` set: hipie_gemm on split-fp16 operands (fp32-class, fp32 out)."""
    out_dtype = torch.float32
    split = False

    def forward(self, x, x_hl8=False, out_fmt=ops.F32):
        if self.split and x.is_cuda and self.weight.dtype == torch.float32 and ops.split_ok(self.in_features):
            return ops.split_linear(x, self, "w", self.weight, self.bias, out_fmt=out_fmt, x_hl8=x_hl8)
        return F.linear(x.to(self.weight.dtype), self.weight, self.bias).to(self.out_dtype)

    def forward_relu(self, x, out_fmt=ops.F32, x_hl8=False):
        """relu(linear(x)) with the ReLU in the GEMM's epilogue (exact: ReLU commutes with the output rounding);
        removes one read+write of the (tokens, d_ffn) hidden tensor per FFN."""
        if self.split and x.is_cuda and self.weight.dtype == torch.float32 and ops.split_ok(self.in_features):
            return ops.split_linear(x, self, "w", self.weight, self.bias, act=ops.ACT_RELU, out_fmt=out_fmt, x_hl8=x_hl8)
        x = x.to(self.weight.dtype)
        if x.is_cuda and self.bias is not None:
            y = torch._addmm_activation(self.bias, x.reshape(-1, x.shape[-1]), self.weight.t(), use_gelu=False)
            return y.view(*x.shape[:-1], -1).to(self.out_dtype)
        return F.relu(F.linear(x, self.weight, self.bias)).to(self.out_dtype)


class PConv2d(nn.Conv2d):
    out_dtype = torch.float32
    nhwc = False          # 16-bit k>1 convs run channels-last (MIOpen's NHWC implicit-GEMM kernels)
    split = False         # Precision.split3 (set_split): 1x1 convolutions of channels-last maps run as the split-fp16 GEMM

    def forward(self, x):
        if (self.split and x.is_cuda and x.dim() == 4 and self.kernel_size == (1, 1) and self.stride == (1, 1) and self.padding == (0, 0)
                and self.groups == 1 and self.weight.dtype == torch.float32 and ops.split_ok(self.in_channels)):
            xb = x.permute(0, 2, 3, 1)
            if xb.is_contiguous():          # a 1x1 convolution of an NHWC map IS a linear over its pixel rows (fp32 MIOpen: ~35 TFLOP/s here)
                B, H, W, C = xb.shape
                w = self.weight
                y = ops.split_linear(xb.float().reshape(B * H * W, C), self, "w1x1", w, self.bias, weight_fn=lambda: w.reshape(w.shape[0], C))
                return y.view(B, H, W, -1).permute(0, 3, 1, 2).to(self.out_dtype)
        if self.split and ops.conv3x3_split_ok(x, self):
            # split policy: 3 x 3 convolutions with full 256-column tiles as an implicit GEMM of the split kernel (K = 9 C_in), instead of
            # the library's fp32 implicit GEMM (1.3 ms -> ~0.5 ms for 256 -> 256 at 128 x 128, bs 8)
            return ops.conv3x3_split(x, self).to(self.out_dtype)
        x = x.to(self.weight.dtype)
        if self.nhwc:
            x = x.contiguous(memory_format=torch.channels_last)
        return self._conv_forward(x, self.weight, self.bias).to(self.out_dtype)


class PLayerNorm(nn.LayerNorm):
    """LayerNorm on whatever activation dtype arrives (fp32 parameters, fp32 statistics inside the kernel)."""

    def forward(self, x):
        C = x.shape[-1]
        if x.is_cuda and C % 4 == 0 and C <= 2048 and self.weight.dtype == torch.float32 and x.dtype in ops._DT:
            return ops.add_layernorm(x.contiguous(), None, self.weight, self.bias, self.eps, x.dtype)[1]   # fp32 statistics
        return F.layer_norm(x, self.normalized_shape, self.weight.to(x.dtype), self.bias.to(x.dtype), self.eps)


class PGroupNorm(nn.GroupNorm):
    """GroupNorm on whatever activation dtype / memory format arrives (fp32 parameters and statistics): hipie_group_norm for
    GroupNorm(32, 256) on the GPU, optionally with the ReLU that follows and a per-channel bias that precedes it."""

    def forward(self, x, relu=False, prebias=None, out_nchw=False):
        """out_nchw: the caller wants a dense NCHW result whatever layout x has (a hint: other paths return x's layout)."""
        if self.weight.dtype == torch.float32 and ops.group_norm_ok(x, self.num_groups):
            return ops.group_norm(x, self.num_groups, self.weight, self.bias, self.eps, relu=relu, prebias=prebias, out_nchw=out_nchw)
        if prebias is not None:
            x = x + prebias.view(1, -1, 1, 1).to(x.dtype)
        y = F.group_norm(x, self.num_groups, self.weight.to(x.dtype), self.bias.to(x.dtype), self.eps)
        return F.relu(y) if relu else y


def cast_head(module, dtype, act=torch.float32):
    """put the GEMM/conv weights (only) of the policy-aware layers in ``dtype`` and make them emit ``act``;
    norm parameters and embeddings stay fp32."""
    for m in module.modules():
        if isinstance(m, (PLinear, PConv2d, nn.ConvTranspose2d)):
            m.weight.data = m.weight.data.to(dtype)
            if m.bias is not None:
                m.bias.data = m.bias.data.to(dtype)
            if isinstance(m, (PLinear, PConv2d)):
                m.out_dtype = act
            if isinstance(m, PConv2d) and dtype != torch.float32:
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
                m.nhwc = True
        elif isinstance(m, MultiheadAttention):           # packed q/k/v projection (a bare Parameter, not a PLinear)
            m.in_proj_weight.data = m.in_proj_weight.data.to(dtype)
            m.in_proj_bias.data = m.in_proj_bias.data.to(dtype)
    return module


_CONST_CACHE = {}


def level_tensors(shapes_list, device):
    """(L,2) int64 spatial shapes + (L,) level start offsets on the device, cached per geometry: building them is a
    host->device copy, which would otherwise happen in every MSDeformAttn call site and forbids hipGraph capture."""
    key = (tuple(shapes_list), str(device))
    v = _CONST_CACHE.get(key)
    if v is None:
        ss = torch.as_tensor(shapes_list, dtype=torch.long, device=device)
        v = (ss, torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1])))
        _CONST_CACHE[key] = v
    return v


def _add_norm(x, delta, norm):
    """LayerNorm(x + delta) in x's dtype through the fused kernel (post-norm residual of the encoder layers)."""
    x = x.contiguous()
    return ops.add_layernorm(x, delta.to(x.dtype).contiguous(), norm.weight, norm.bias, norm.eps, x.dtype, want_res=False)[1]


def _get_clones(module, n):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(n)])


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(PLinear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = layer.forward_relu(x) if i < self.num_layers - 1 else layer(x)      # ReLU in the GEMM epilogue
        return x


class FeatureResizer(nn.Module):
    def __init__(self, input_feat_size, output_feat_size):
        super().__init__()
        self.fc = PLinear(input_feat_size, output_feat_size)
        self.layer_norm = PLayerNorm(output_feat_size, eps=1e-12)

    def forward(self, x):
        return self.layer_norm(self.fc(x))


# --------------------------------------------------------------------------- backbone wrappers + sine position
_GEO_CACHE = collections.OrderedDict()


def geo_cached(geo_key, what, build):
    """Everything that depends only on the padding masks -- level masks, sine position embeddings, valid ratios, encoder
    reference points, two-stage proposals -- is a function of the batch geometry (image sizes + padded canvas).  An
    evaluation run repeats a handful of geometries, so these are computed once per geometry and reused (read-only)
    instead of re-issuing a few hundred tiny cumsum / sin / cos / sum / cat kernels per forward.  geo_key None: no caching.
    Values that also depend on parameters go through ``derived`` (level_pos_flat)."""
    if geo_key is None:
        return build()
    cache = _GEO_CACHE
    key = (geo_key, what)
    v = cache.get(key)
    if v is None:
        v = build()
        cache[key] = v
        if len(cache) > 512:
            cache.popitem(last=False)
    else:
        cache.move_to_end(key)
    return v


def level_pos_flat(enc, pos_embeds, dtype, geo_key):
    """position + level embedding of all pyramid levels, flattened to (B, tokens, C) in ``dtype``: a function of the geometry AND of
    enc.level_embed, so it is cached on ``enc`` per level_embed stamp with up to 32 geometries alive.  geo_key None: no caching."""
    def build():
        return torch.cat([p.flatten(2).transpose(1, 2) + enc.level_embed[i].view(1, 1, -1) for i, p in enumerate(pos_embeds)], 1).to(dtype)
    return build() if geo_key is None else derived(enc, "pos_flat", [enc.level_embed], build, extra=geo_key, keep=32)


class NestedTensor(object):
    def __init__(self, tensors, mask, geo_key=None):
        self.tensors, self.mask, self.geo_key = tensors, mask, geo_key

    def decompose(self):
        return self.tensors, self.mask


def nested_tensor_from_images(images, size_divisibility=32, stacked=None):
    """hipie/util/misc.py:288-316: zero-pad to the batch max rounded up to size_divisibility; mask True on padding.
    ``stacked``: the same images as one (B,3,H,W) tensor, used as is when no image needs padding."""
    H = max(int(im.shape[1]) for im in images)
    W = max(int(im.shape[2]) for im in images)
    H = (H + size_divisibility - 1) // size_divisibility * size_divisibility
    W = (W + size_divisibility - 1) // size_divisibility * size_divisibility
    dev = images[0].device
    if stacked is not None and tuple(stacked.shape[-2:]) == (H, W) and all(tuple(im.shape[1:]) == (H, W) for im in images):
        geo_key = (tuple((H, W) for _ in images), (H, W), str(dev))
        return NestedTensor(stacked, geo_cached(geo_key, "pixel_mask", lambda: torch.zeros(
            len(images), H, W, dtype=torch.bool, device=dev)), geo_key)
    t = torch.zeros(len(images), 3, H, W, dtype=images[0].dtype, device=dev)
    geo_key = (tuple((int(im.shape[1]), int(im.shape[2])) for im in images), (H, W), str(dev))

    def build_mask():
        m = torch.ones(len(images), H, W, dtype=torch.bool, device=dev)
        for i, im in enumerate(images):
            m[i, :im.shape[1], :im.shape[2]] = False
        return m
    for i, im in enumerate(images):
        t[i, :, :im.shape[1], :im.shape[2]].copy_(im)
    return NestedTensor(t, geo_cached(geo_key, "pixel_mask", build_mask), geo_key)


class PositionEmbeddingSine(nn.Module):
    """normalize=True, T=10000, scale=2pi.  offset -0.5: deformable_detr/position_encoding.py:36-56;
    offset 0: maskdino/pixel_decoder/position_encoding.py:31-52."""

    def __init__(self, num_pos_feats=128, offset=-0.5):
        super().__init__()
        self.num_pos_feats, self.offset = num_pos_feats, offset

    def forward(self, mask):
        not_mask = ~mask
        y = not_mask.cumsum(1, dtype=torch.float32)
        x = not_mask.cumsum(2, dtype=torch.float32)
        y = (y + self.offset) / (y[:, -1:, :] + 1e-6) * (2 * math.pi)
        x = (x + self.offset) / (x[:, :, -1:] + 1e-6) * (2 * math.pi)
        dim_t = torch.arange(self.num_pos_feats, dtype=torch.float32, device=mask.device)
        dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / self.num_pos_feats)
        px, py = x[:, :, :, None] / dim_t, y[:, :, :, None] / dim_t
        px = torch.stack((px[:, :, :, 0::2].sin(), px[:, :, :, 1::2].cos()), dim=4).flatten(3)
        py = torch.stack((py[:, :, :, 0::2].sin(), py[:, :, :, 1::2].cos()), dim=4).flatten(3)
        return torch.cat((py, px), dim=3).permute(0, 3, 1, 2)


class MaskedBackbone(nn.Module):
    """hipie/backbone/masked_backbone.py: backbone + per-level nearest-resized padding mask."""

    def __init__(self, backbone, strides, channels):
        super().__init__()
        self.backbone = backbone
        self.feature_strides, self.num_channels = strides, channels

    def forward(self, tensor_list):
        xs = self.backbone(tensor_list.tensors)
        out = {}
        gk = tensor_list.geo_key
        for name, x in xs.items():
            hw = tuple(x.shape[-2:])
            mask = geo_cached(gk, ("level_mask", hw),
                              lambda: F.interpolate(tensor_list.mask[None].float(), size=hw).to(torch.bool)[0])
            out[name] = NestedTensor(x, mask, gk)
        return out


class Joiner(nn.Sequential):
    """hipie/models/deformable_detr/backbone.py:114-129 (levels sorted by name: res3, res4, res5)."""

    def __init__(self, backbone, position_embedding):
        super().__init__(backbone, position_embedding)

    def forward(self, tensor_list):
        xs = self[0](tensor_list)
        out = [x for _, x in sorted(xs.items())]
        pos = [geo_cached(x.geo_key, ("pos", tuple(x.mask.shape), x.tensors.dtype, self[1].offset),
                          lambda x=x: self[1](x.mask).to(x.tensors.dtype)) for x in out]
        return out, pos


# --------------------------------------------------------------------------- MSDeformAttn
class MSDeformAttn(nn.Module):
    """ops/modules/ms_deform_attn.py:30-116 on hipie_msda_fused_forward (sampling locations + softmax in-kernel)."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4, value_dtype=torch.float32):
        super().__init__()
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = PLinear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = PLinear(d_model, n_heads * n_levels * n_points)
        self.value_proj = PLinear(d_model, d_model)
        self.output_proj = PLinear(d_model, d_model)
        self.value_dtype = value_dtype

    def project_value(self, input_flatten, input_padding_mask=None, x_hl8=False):
        N, S, _ = input_flatten.shape
        vp = self.value_proj                       # GEMM output stays in the weight dtype: no fp32 round trip, mask in place
        value = _lin(vp, "w", input_flatten, vp.weight, vp.bias, x_hl8=x_hl8)
        if input_padding_mask is not None:
            value.masked_fill_(input_padding_mask[..., None], 0.0)
        return value.to(self.value_dtype).view(N, S, self.n_heads, self.d_model // self.n_heads)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None):
        N, Lq, _ = query.shape
        value = self.project_value(input_flatten, input_padding_mask)
        if reference_points.shape[-1] not in (2, 4):
            raise ValueError("Last dim of reference_points must be 2 or 4, but get {} instead.".format(reference_points.shape[-1]))
        # sampling_offsets and attention_weights share their input: one GEMM on the concatenated weights, and the kernel
        # reads both column blocks of that single output in place (row strides), in whatever dtype the GEMM produced
        w, b = self._fused_proj()
        no = self.n_heads * self.n_levels * self.n_points * 2
        proj = _lin(self, "offlog", query, w, b)
        off = proj[..., :no].unflatten(-1, (self.n_heads, self.n_levels, self.n_points, 2))
        logits = proj[..., no:].unflatten(-1, (self.n_heads, self.n_levels * self.n_points))
        out = ops.msda_fused(value.contiguous(), input_spatial_shapes, input_level_start_index,
                             reference_points.float().contiguous(), off, logits)
        return self.output_proj(out)

    def forward_projected(self, query, reference_points, value, input_spatial_shapes, input_level_start_index, x_hl8=False, project=True):
        """forward with the value projection done by the caller (one GEMM for all decoder layers): `value` (N, S, heads, hd),
        dense or a column block of the batched projection (sampled in place through its row stride).  project=False: the sampled
        values before output_proj (the caller fuses the projection with what follows it)."""
        w, b = self._fused_proj()
        no = self.n_heads * self.n_levels * self.n_points * 2
        proj = _lin(self, "offlog", query, w, b, x_hl8=x_hl8)
        off = proj[..., :no].unflatten(-1, (self.n_heads, self.n_levels, self.n_points, 2))
        logits = proj[..., no:].unflatten(-1, (self.n_heads, self.n_levels * self.n_points))
        out = ops.msda_fused(value, input_spatial_shapes, input_level_start_index, reference_points.float().contiguous(), off, logits)
        return self.output_proj(out) if project else out

    def _fused_proj(self):
        so, aw = self.sampling_offsets, self.attention_weights
        return derived(self, "fused_proj", (so.weight, aw.weight, so.bias, aw.bias), lambda: (
            torch.cat([so.weight, aw.weight], 0).contiguous(), torch.cat([so.bias, aw.bias], 0).contiguous()))


# --------------------------------------------------------------------------- VL fusion
class BiMultiHeadAttention(nn.Module):
    """fuse_helper.py:8-139; the two softmax(QK^T)V products run on hipie_bi_xattn."""

    def __init__(self, v_dim, l_dim, embed_dim, num_heads, attn_dtype):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.scale = self.head_dim ** (-0.5)
        self.v_proj, self.l_proj = PLinear(v_dim, embed_dim), PLinear(l_dim, embed_dim)
        self.values_v_proj, self.values_l_proj = PLinear(v_dim, embed_dim), PLinear(l_dim, embed_dim)
        self.out_v_proj, self.out_l_proj = PLinear(embed_dim, v_dim), PLinear(embed_dim, l_dim)
        self.attn_dtype = attn_dtype

    def forward(self, v, l, attention_mask_l=None, gamma_v=None, n_keys=None, resid_v=None):
        """resid_v: the block's residual for the visual stream; the split path adds it in the epilogue of the output projection
        (`self.resid_fused` tells the caller) instead of leaving a (B, Nv, 256) add pass behind.  n_keys: host-known number of leading text columns that hold every attended token (BertEncoder.forward): the image -> text
        direction of the split policy runs over those keys only -- masked keys have probability exactly 0 (fuse_helper.py:96-109)."""
        B, Nv, _ = v.shape
        L = l.shape[1]
        H, hd, dt = self.num_heads, self.head_dim, self.attn_dtype
        wq, bq = self._scaled_q()                              # v_proj with the 1/sqrt(head_dim) folded in: no (B, Nv, 2048) multiply pass
        if getattr(self, "split", False) and v.is_cuda and self.v_proj.weight.dtype == torch.float32 and hd % 32 == 0 and ops.split_ok(v.shape[-1]):
            return self._forward_split(v, l, attention_mask_l, gamma_v, wq, bq, n_keys, resid_v)
        self.resid_fused = False
        # the GEMM epilogue rounds to the attention operand dtype itself (bit-identical to fp32 out + .to(fp16), minus
        # a 178M-element cast pass per visual projection)
        of = ops.F16 if (getattr(self, "split", False) and dt == torch.float16) else ops.F32
        q = _lin(self, "q_scaled", v, wq, bq, out_fmt=of).to(dt).view(B, Nv, H, hd)
        k = self.l_proj(l, out_fmt=of).to(dt).view(B, L, H, hd)
        vv = self.values_v_proj(v, out_fmt=of).to(dt).view(B, Nv, H, hd)
        vl = self.values_l_proj(l, out_fmt=of).to(dt).view(B, L, H, hd)
        if attention_mask_l is None:
            attention_mask_l = torch.ones(B, L, dtype=torch.uint8, device=v.device)
        ov, ol = ops.bi_xattn(q, k, vv, vl, attention_mask_l != 0, clamp=50000.0, out_f32=getattr(self, "split", False))
        if gamma_v is None:
            return self.out_v_proj(ov), self.out_l_proj(ol)
        wo, bo = self._scaled_out(gamma_v)
        return _lin(self, "out_scaled", ov, wo, bo).to(self.out_v_proj.out_dtype), self.out_l_proj(ol)

    def _forward_split(self, v, l, attention_mask_l, gamma_v, wq, bq, n_keys=None, resid_v=None):
        """Precision.split3.  image -> text (the update of the 21760-token visual stream, whose error the decoder amplifies): fp32-class
        -- S = Q.K^T per (image, head) as one batched split GEMM from the HL8 projection, masked softmax -> HL8, P.V_text as the second
        batched GEMM (ops.bi_i2t_split).  text -> image (the language stream; its softmax averages over all visual tokens): the fp16
        MFMA flash kernel with fp32 output.  tools/dec_err_full.py: with single-fp16 q / k in BOTH directions pred_masks is 1.5e-3 off at
        the headline configuration, with this formulation and the P pair of the ViT attention 1-3e-4."""
        B, Nv, _ = v.shape
        L = l.shape[1]
        H, hd = self.num_heads, self.head_dim
        if attention_mask_l is None:
            attention_mask_l = torch.ones(B, L, dtype=torch.uint8, device=v.device)
        keep = attention_mask_l != 0
        if ops.bi_i2t_folded_ok(v, L, n_keys):
            return self._forward_folded(v, l, keep, gamma_v, wq, bq, n_keys, resid_v)
        vh = ops.to_hl8(v.float().contiguous())                                 # the visual stream once, for its three projections
        q_hl8 = _lin(self, "q_scaled", vh, wq, bq, out_fmt=ops.HL8, x_hl8=True)
        # the text -> image direction reads the same scaled projection as single fp16: that is the `hi` half of every HL8 group (hi = fp16(x)
        # by construction of hl_split), read in place by the attention kernel (HIPIE_K_HL8_HI) -- no second 174080 x 2048 x 256 GEMM, no copy
        vv16 = self.values_v_proj(vh, x_hl8=True, out_fmt=ops.F16).view(B, Nv, H, hd)
        k32 = self.l_proj(l)
        vl32 = self.values_l_proj(l)
        ov = ops.bi_i2t_split(q_hl8.view(B, Nv, -1), k32.view(B, L, -1), vl32.view(B, L, -1), keep, H, clamp=50000.0, n_keys=n_keys)
        # text -> image: queries = text tokens, keys / values = visual tokens, no mask on that side (fuse_helper.py:85-95)
        ol = ops.flash_attn(k32.half().view(B, L, H, hd), q_hl8.view(B, Nv, 2 * H * hd), vv16, 1.0, clamp=50000.0, out_f32=True, k_hl8=True)
        self.resid_fused = False
        if gamma_v is None:
            return self.out_v_proj(ov), self.out_l_proj(ol)
        wo, bo = self._scaled_out(gamma_v)
        if resid_v is not None and resid_v.dtype == torch.float32 and resid_v.is_contiguous() and self.out_v_proj.out_dtype == torch.float32:
            self.resid_fused = True
            return ops.split_linear(ov, self, "out_scaled", wo, bo, resid=resid_v), self.out_l_proj(ol)
        return _lin(self, "out_scaled", ov, wo, bo).to(self.out_v_proj.out_dtype), self.out_l_proj(ol)

    def _forward_folded(self, v, l, keep, gamma_v, wq, bq, n_keys, resid_v):
        """Precision.split3, texts with at most 256 attended tokens (every shipped prompt but the open-vocabulary captions of configs[3] / [4]):
        both directions WITHOUT the two visual-side projections of width embed_dim (174080 x 2048 x 256 each at the headline size).  With
        M[b,h,j] = k_{b,j,h} W_q,h (a 256-vector per text token and head) the logits are x_i . M[b,h,j] + b_q,h . k_{b,j,h} -- the visual
        stream itself is the operand:
          image -> text  ops.bi_i2t_folded: softmax_j in the epilogue of ONE batched split GEMM over x (P as HL8), then out = P . (V_text W_o^T)
                         with bias, gamma and the block's residual in the epilogue of the second (fuse_helper.py:77-121, 131-137);
          text -> image  queries M (fp16), keys AND values the fp16 visual stream shared by all heads (hipie_flash_attn, head stride 0);
                         the value projection moves behind the attention, onto the L text rows: sum_i P'[j,i] (W_v x_i + b_v) =
                         W_v (sum_i P'[j,i] x_i) + b_v (fuse_helper.py:85-95, 122-130).  The per-text-token logit bias is constant along the
                         visual tokens and drops out of that softmax."""
        B, Nv, C = v.shape
        L = l.shape[1]
        H, hd = self.num_heads, self.head_dim
        v = v.contiguous()
        vh = ops.to_hl8(v)
        k32 = self.l_proj(l)                                                    # (B, L, E)
        vl32 = self.values_l_proj(l)
        kh = k32.view(B, L, H, hd).permute(0, 2, 1, 3)                          # (B, H, L, hd)
        M = torch.matmul(kh, wq.float().view(1, H, hd, C))                      # (B, H, L, C): k_h W_q,h, fp32
        cb = (kh * bq.float().view(1, H, 1, hd)).sum(-1)                        # (B, H, L)
        Lk = L if not n_keys or n_keys >= L else int(n_keys)
        if gamma_v is None:
            wo, bo = self.out_v_proj.weight, self.out_v_proj.bias
        else:
            wo, bo = self._scaled_out(gamma_v)
        fuse_resid = resid_v is not None and resid_v.dtype == torch.float32 and resid_v.is_contiguous() and gamma_v is not None
        ov = ops.bi_i2t_folded(vh, M[:, :, :Lk].contiguous(), cb[:, :, :Lk].contiguous(), vl32[:, :Lk].contiguous(), keep[:, :Lk], H, wo, bo,
                               resid=resid_v if fuse_resid else None, clamp=50000.0)
        self.resid_fused = fuse_resid
        x16 = v.half()
        kx = x16.view(B, Nv, 1, C).expand(B, Nv, H, C)                          # every head reads the same keys / values
        q16 = M.half().permute(0, 2, 1, 3)                                      # (B, L, H, C) view
        olx = ops.flash_attn(q16, kx, kx, 1.0, clamp=50000.0, out_f32=True)     # (B, L, H * C): sum_i P'[j,i] x_i per head
        wv = self.values_v_proj
        ol = torch.einsum("blhc,hec->blhe", olx.view(B, L, H, C), wv.weight.float().view(H, hd, C)).reshape(B, L, H * hd) + wv.bias.float()
        return ov.to(self.out_v_proj.out_dtype), self.out_l_proj(ol)

    def _scaled_out(self, gamma):
        p = self.out_v_proj
        return derived(self, "scaled_out", (p.weight, p.bias, gamma), lambda: (
            (p.weight.float() * gamma.float()[:, None]).to(p.weight.dtype), (p.bias.float() * gamma.float()).to(p.bias.dtype)))

    def _scaled_q(self):
        p = self.v_proj
        return derived(self, "scaled_q", (p.weight, p.bias), lambda: (
            (p.weight.float() * self.scale).to(p.weight.dtype), (p.bias.float() * self.scale).to(p.bias.dtype)))


class BiAttentionBlockForCheckpoint(nn.Module):
    """fuse_helper.py:142-179."""

    def __init__(self, v_dim, l_dim, embed_dim, num_heads, init_values, attn_dtype):
        super().__init__()
        self.layer_norm_v, self.layer_norm_l = PLayerNorm(v_dim), PLayerNorm(l_dim)
        self.attn = BiMultiHeadAttention(v_dim, l_dim, embed_dim, num_heads, attn_dtype)
        self.gamma_v = nn.Parameter(init_values * torch.ones(v_dim))
        self.gamma_l = nn.Parameter(init_values * torch.ones(l_dim))

    def forward(self, v, l, attention_mask_l=None, task=None, n_keys=None):
        v, l = self.layer_norm_v(v), self.layer_norm_l(l)
        dv, dl = self.attn(v, l, attention_mask_l=attention_mask_l, gamma_v=self.gamma_v, n_keys=n_keys, resid_v=v)
        if self.attn.resid_fused:
            return dv, l + self.gamma_l * dl
        # gamma_v is folded into the visual output projection (weights only), so the 21760-token stream stays in its own
        # dtype: `v + gamma_v * dv` would promote it to fp32 and every later encoder GEMM would cast it back
        return v + dv.to(v.dtype), l + self.gamma_l * dl


class VLFuse(nn.Module):
    """vlfusion.py:74-120."""

    def __init__(self, cfg, precision):
        super().__init__()
        self.b_attn = BiAttentionBlockForCheckpoint(cfg.hidden_dim, cfg.lang_dim, cfg.vl_hidden_dim, 8,
                                                    1.0 / cfg.enc_layers, precision.attn)

    def forward(self, x, task=None):
        lang = x["lang"]
        fv, fl = self.b_attn(x["visual"], lang["hidden"], lang["masks"], task, n_keys=lang.get("n_keys"))
        lang["hidden"] = fl
        return {"visual": fv, "lang": lang}


# --------------------------------------------------------------------------- encoder / decoder
class DeformableTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, n_levels, n_heads, n_points, value_dtype):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points, value_dtype)
        self.norm1 = PLayerNorm(d_model)
        self.linear1, self.linear2 = PLinear(d_model, d_ffn), PLinear(d_ffn, d_model)
        self.norm2 = PLayerNorm(d_model)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None, query=None, want_query=False):
        """query: `src + pos` when the previous layer already produced it; want_query: also return the NEXT layer's `src + pos`,
        emitted by the last LayerNorm pass (hipie_add_layernorm_sum) instead of a separate add over the 21760-token stream."""
        if getattr(self, "split", False) and src.is_cuda and src.dtype == torch.float32 and self.linear1.weight.dtype == torch.float32:
            return self._forward_split(src, pos, reference_points, spatial_shapes, level_start_index, padding_mask, query, want_query)
        q = src + pos if query is None else query
        src2 = self.self_attn(q, reference_points, src, spatial_shapes, level_start_index, padding_mask)
        src = _add_norm(src, src2, self.norm1)
        src2 = self.linear2(self.linear1.forward_relu(src))
        if want_query and src.is_cuda and src.dtype == pos.dtype and src.dtype in ops._DT:
            n = self.norm2
            return ops.add_layernorm_sum(src.contiguous(), src2.to(src.dtype).contiguous(), n.weight, n.bias, n.eps, pos.contiguous())
        out = _add_norm(src, src2, self.norm2)
        return (out, None) if want_query else out


def _enc_layer_forward_split(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask, carry, want_query):
    """the encoder layer of the split policy (Precision.split3): every linear is the three-product GEMM and takes its operand as
    HL8 straight from the pass that produced it -- the post-norm LayerNorm passes emit the fp32 stream, its HL8 copy and (for the
    next layer's query) `src + pos` as HL8 in ONE launch (hipie_add_layernorm_dec), linear1 writes relu(.) as HL8 for linear2; only
    the deformable-attention output is converted by hipie_to_hl8.  ``carry``: {"src_h", "q_h"} from the previous layer, or None."""
    attn = self.self_attn
    src = src.contiguous()
    if isinstance(carry, dict):
        src_h, q_h = carry["src_h"], carry["q_h"]
    elif carry is None:                     # first layer: the query src + pos as ONE pass over the cached HL8 position embedding
        src_h, q_h = ops.to_hl8(src), ops.add_to_hl8(src, _pos_hl8(self, pos))
    else:
        src_h, q_h = ops.to_hl8(src), ops.to_hl8(carry)
    value = attn.project_value(src_h, padding_mask, x_hl8=True)
    n, op = self.norm1, attn.output_proj
    if ops.split_linear_ln_ok(src, op.weight, n.weight):
        # output_proj + residual + norm1 as ONE launch (hipie_gemm_ln: 256 features = one column tile, the rows are whole in the epilogue)
        sampled = attn.forward_projected(q_h, reference_points, value.contiguous(), spatial_shapes, level_start_index, x_hl8=True, project=False)
        src, s_h = ops.split_linear_ln(sampled, op, "w", op.weight, op.bias, src, n.weight, n.bias, n.eps)
    else:
        src2 = attn.forward_projected(q_h, reference_points, value.contiguous(), spatial_shapes, level_start_index, x_hl8=True)
        src, s_h, _ = ops.add_layernorm_dec(src, src2.contiguous(), n.weight, n.bias, n.eps, "hl8", want16=True)
    if ops.ffn_fused_ok(s_h, self.linear1, self.linear2):
        src2 = ops.ffn_fused(s_h, self.linear1, self.linear2)          # one launch, the (tokens x 2048) hidden tensor never exists
    else:
        src2 = self.linear2(self.linear1.forward_relu(s_h, out_fmt=ops.HL8, x_hl8=True), x_hl8=True)
    n = self.norm2
    if not want_query:
        return ops.add_layernorm_dec(src, src2, n.weight, n.bias, n.eps, "hl8")[0]
    out, o_h, q_h = ops.add_layernorm_dec(src, src2, n.weight, n.bias, n.eps, "hl8", want16=True, addend=_pos_hl8(self, pos))
    return out, {"src_h": o_h, "q_h": q_h}


def _pos_hl8(layer, pos):
    """HL8 copy of the position embedding, cached on the layer: a per-geometry constant"""
    return derived(layer, "pos_hl8", [pos], lambda: ops.to_hl8(pos.contiguous()))


DeformableTransformerEncoderLayer._forward_split = _enc_layer_forward_split


def encoder_reference_points(spatial_shapes, valid_ratios, device):
    """deformable_transformer_dino.py:313-325."""
    refs = []
    for lvl, (H_, W_) in enumerate(spatial_shapes):
        ref_y, ref_x = torch.meshgrid(torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32, device=device),
                                      torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32, device=device), indexing="ij")
        ref_y = ref_y.reshape(-1)[None] / (valid_ratios[:, None, lvl, 1] * H_)
        ref_x = ref_x.reshape(-1)[None] / (valid_ratios[:, None, lvl, 0] * W_)
        refs.append(torch.stack((ref_x, ref_y), -1))
    r = torch.cat(refs, 1)
    return r[:, :, None] * valid_ratios[:, None]


class DeformableTransformerEncoderVL(nn.Module):
    """deformable_transformer_dino.py:302-351: VLFuse only on the first num_vl_layers layers."""

    def __init__(self, vl_fusion_layer, encoder_layer, num_layers, num_vl_layers):
        super().__init__()
        self.vl_layers = nn.ModuleList([copy.deepcopy(vl_fusion_layer) if i < num_vl_layers else nn.Identity()
                                        for i in range(num_layers)])
        self.layers = _get_clones(encoder_layer, num_layers)
        self.lang_layers = nn.ModuleList([nn.Identity() for _ in range(num_layers)])

    def forward(self, src, shapes_list, spatial_shapes, level_start_index, valid_ratios, pos, padding_mask, lang, task=None,
                geo_key=None):
        output = {"visual": src, "lang": lang}
        refs = geo_cached(geo_key, "enc_refs", lambda: encoder_reference_points(shapes_list, valid_ratios, src.device))
        q, n = None, len(self.layers)
        for i, (vl_layer, layer) in enumerate(zip(self.vl_layers, self.layers)):
            if not isinstance(vl_layer, nn.Identity):
                output = vl_layer(output, task=task)
                q = None                                  # the fusion changed the stream: its `src + pos` is recomputed
            nxt_plain = i + 1 < n and isinstance(self.vl_layers[i + 1], nn.Identity)
            res = layer(output["visual"], pos, refs, spatial_shapes, level_start_index, padding_mask, query=q, want_query=nxt_plain)
            output["visual"], q = res if nxt_plain else (res, None)
        return output


class MultiheadAttention(nn.Module):
    """nn.MultiheadAttention parameters (in_proj_weight/in_proj_bias/out_proj), q = k = x_qk, v = x_v, batch-first
    (deformable_transformer_dino.py:435-436, dino_decoder.py:246-248).  The softmax(QK^T)V core runs on hipie_flash_attn
    (head dim 32, 16-bit operands, fp32 softmax / accumulation) -- no library / Triton attention on the path."""

    def __init__(self, d_model, n_heads, attn_dtype=torch.float16):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = PLinear(d_model, d_model)
        self.n_heads = n_heads
        self.attn_dtype = attn_dtype
        nn.init.xavier_uniform_(self.in_proj_weight)

    def forward(self, x_qk, x_v):
        B, N, C = x_qk.shape
        w, b = self.in_proj_weight, self.in_proj_bias
        hd = C // self.n_heads
        split = getattr(self, "split", False)
        if split and x_qk.is_cuda and w.dtype == torch.float32 and ops.attn_f32_ok(hd):
            # split policy: fp32 projections (split GEMM) and the fp32-CLASS attention core (hipie_attn_split) -- the query self-attention is 0.1 % of the
            # step's flops, and fp16 q / k / v here cost 5e-4 .. 1e-3 on the decoder states at the headline configuration
            qk = _lin(self, "in_qk", x_qk, w, b, rows=slice(0, 2 * C)).view(B, N, 2, self.n_heads, hd)
            v = _lin(self, "in_v", x_v, w, b, rows=slice(2 * C, None)).view(B, N, self.n_heads, hd)
            return self.out_proj(ops.attn_split(qk[:, :, 0], qk[:, :, 1], v, hd ** -0.5))
        of = ops.F16 if (split and self.attn_dtype == torch.float16) else ops.F32
        qk = _lin(self, "in_qk", x_qk, w, b, out_fmt=of, rows=slice(0, 2 * C)).to(self.attn_dtype).view(B, N, 2, self.n_heads, hd)
        v = _lin(self, "in_v", x_v, w, b, out_fmt=of, rows=slice(2 * C, None)).to(self.attn_dtype).view(B, N, self.n_heads, hd)
        o = ops.flash_attn(qk[:, :, 0], qk[:, :, 1], v, hd ** -0.5, out_f32=split)   # strided q / k views of one GEMM output
        return self.out_proj(o)


class DeformableTransformerDecoderLayer(nn.Module):
    """deformable_transformer_dino.py:397-450 == maskdino/transformer_decoder/dino_decoder.py:171-270 (batch-first here)."""

    def __init__(self, d_model, d_ffn, n_levels, n_heads, n_points, value_dtype, attn_dtype=torch.float16):
        super().__init__()
        self.cross_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points, value_dtype)
        self.norm1 = PLayerNorm(d_model)
        self.self_attn = MultiheadAttention(d_model, n_heads, attn_dtype)
        self.norm2 = PLayerNorm(d_model)
        self.linear1, self.linear2 = PLinear(d_model, d_ffn), PLinear(d_ffn, d_model)
        self.norm3 = PLayerNorm(d_model)

    def forward(self, tgt, query_pos, reference_points, src, spatial_shapes, level_start_index, src_padding_mask=None, value=None):
        """every residual add + LayerNorm is one hipie_add_layernorm launch; the stream keeps the dtype it arrives in.
        value: this layer's pre-projected (N, S, heads, hd) block of batched_decoder_values (src is then not read)."""
        qk = tgt + query_pos
        tgt = _add_norm(tgt, self.self_attn(qk, tgt), self.norm2)
        if value is not None:
            tgt2 = self.cross_attn.forward_projected(tgt + query_pos, reference_points, value, spatial_shapes, level_start_index)
        else:
            tgt2 = self.cross_attn(tgt + query_pos, reference_points, src, spatial_shapes, level_start_index, src_padding_mask)
        tgt = _add_norm(tgt, tgt2, self.norm1)
        tgt2 = self.linear2(self.linear1.forward_relu(tgt))
        return _add_norm(tgt, tgt2, self.norm3)


    def forward16(self, t32, t16, qp16, reference_points, value, spatial_shapes, level_start_index):
        """the same layer for an fp32 query stream with 16-bit GEMMs, 15 launches: t32 the stream, t16 its copy in the GEMM
        dtype, qp16 the positional query in the GEMM dtype, value this layer's (pre-projected) block.  Every LayerNorm launch
        also emits the 16-bit operands of the GEMMs that follow it (hipie_add_layernorm_dec); returns (t32, t16)."""
        wd = t16.dtype
        sa = self.self_attn(ops.add_cast(t32, qp16), t16)
        n = self.norm2
        t32, _, q16 = ops.add_layernorm_dec(t32, sa, n.weight, n.bias, n.eps, wd, addend=qp16)
        ca = self.cross_attn.forward_projected(q16, reference_points, value, spatial_shapes, level_start_index)
        n = self.norm1
        t32, t16, _ = ops.add_layernorm_dec(t32, ca, n.weight, n.bias, n.eps, wd, want16=True)
        ff = self.linear2(self.linear1.forward_relu(t16))
        n = self.norm3
        t32, t16, _ = ops.add_layernorm_dec(t32, ff, n.weight, n.bias, n.eps, wd, want16=True)
        return t32, t16


def decoder_fast_path(layers, stream_dtype):
    """fp32 query stream + 16-bit layer weights + value tensor in the weight dtype: the launch-lean formulation applies."""
    l0 = layers[0]
    wd = l0.linear1.weight.dtype
    return (stream_dtype == torch.float32 and wd in (torch.float16, torch.bfloat16) and l0.cross_attn.value_dtype == wd
            and l0.linear1.out_dtype == wd and l0.linear1.weight.is_cuda)


def decoder_split_values(decoder, src):
    """split policy, inference: the value projections of all decoder layers read the same fp32 memory -> one batched GEMM."""
    l0 = decoder.layers[0].cross_attn
    return (bool(getattr(decoder, "split", False)) and src.is_cuda and src.dtype == torch.float32 and not torch.is_grad_enabled()
            and l0.value_proj.weight.dtype == torch.float32 and l0.value_dtype == torch.float32)


def batched_decoder_values(owner, layers, src, padding_mask=None):
    """value projections of ALL decoder layers as one GEMM on the concatenated weights (they read the same memory); returns
    the per-layer (N, S, heads, hd) column blocks (views: hipie_msda samples them in place)."""
    ps = [l.cross_attn.value_proj for l in layers]
    w, b = derived(owner, "bv", [t for p in ps for t in (p.weight, p.bias)], lambda: (
        torch.cat([p.weight for p in ps], 0).contiguous(), torch.cat([p.bias for p in ps], 0).contiguous()))
    v = _lin(owner, "bv", src, w, b)           # split policy: ONE thin-K split GEMM (N = layers x 256) instead of one 256-column GEMM per layer
    if padding_mask is not None:
        v.masked_fill_(padding_mask[..., None], 0.0)
    N, S, _ = v.shape
    d, H = ps[0].weight.shape[0], layers[0].cross_attn.n_heads
    return [v[:, :, i * d:(i + 1) * d].unflatten(-1, (H, d // H)) for i in range(len(ps))]


def ref_point_query(ref_point_head, sine):
    """the 2-layer ref_point_head on a 16-bit sine embedding, output left in the GEMM dtype (no cast to the stream dtype)."""
    l0, l1 = ref_point_head.layers
    h = torch._addmm_activation(l0.bias, sine.reshape(-1, sine.shape[-1]), l0.weight.t(), use_gelu=False)   # ReLU epilogue
    return F.linear(h, l1.weight, l1.bias).view(*sine.shape[:-1], -1)


# The two small per-layer heads as ONE launch each (hipie_ref_point_mlp, hipie_box_head; exact fp32 FMAs): 75 launches fewer per step.
# fast policy: slower than the fp16 library GEMMs it replaces (A/B on one box: 100.0 vs 99.2 ms per step) -> not used there.
# split policy: the same speed as the 5 small split GEMMs + 2 glue launches per layer (224.5 vs 224.9 ms, same box, same 4.2e-4 parity
# error) -> used there.
def _fused_heads(module):
    return bool(getattr(module, "split", False))


def decoder_query_pos(ref_point_head, ref, wdt):
    """query_pos of a decoder layer in the GEMM dtype: one launch (sine features + both layers) for the standard 512-256-256 head."""
    if _fused_heads(ref_point_head) and ops.ref_point_mlp_ok(ref, ref_point_head) and ref_point_head.layers[0].weight.dtype == wdt:
        return ops.ref_point_mlp(ref, ref_point_head)
    return ref_point_query(ref_point_head, ops.sine_embed(ref, out_dtype=wdt))


def decoder_box_refine(bbox_embed, t32, ref):
    """sigmoid(bbox_embed(t) + inverse_sigmoid(ref)): one launch for the standard fp32 MLP(256, 256, 4, 3)."""
    if _fused_heads(bbox_embed) and ops.box_head_ok(t32, bbox_embed):
        return ops.box_head(t32, ref, bbox_embed)
    return ops.box_refine(bbox_embed(t32), ref)


def get_sine_pos_embed(pos_tensor, num_pos_feats=128, temperature=10000, exchange_xy=True):
    """deformable_transformer_dino.py:636-670 (== gen_sineembed_for_position, maskdino/utils/utils.py:74-100)."""
    scale = 2 * math.pi
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=pos_tensor.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)

    def sine_func(x):
        s = x * scale / dim_t
        return torch.stack((s[..., 0::2].sin(), s[..., 1::2].cos()), dim=-1).flatten(-2)
    res = [sine_func(x) for x in pos_tensor.split([1] * pos_tensor.shape[-1], dim=-1)]
    if exchange_xy:
        res[0], res[1] = res[1], res[0]
    return torch.cat(res, dim=-1)


class DeformableTransformerDecoder(nn.Module):
    """deformable_transformer_dino.py:453-525 (return_intermediate, look_forward_twice, iterative box refinement)."""

    def __init__(self, embed_dim, decoder_layer, num_layers):
        super().__init__()
        self.layers = _get_clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.ref_point_head = MLP(2 * embed_dim, embed_dim, embed_dim, 2)
        self.bbox_embed = None
        self.class_embed = None

    def forward(self, tgt, reference_points, src, spatial_shapes, level_start_index, valid_ratios, src_padding_mask=None):
        sdt = torch.float32                                  # query stream dtype: fp32 in every policy (910 queries: the traffic is negligible)
        output, inter, inter_refs = tgt.to(sdt), [], []
        vr2 = torch.cat([valid_ratios, valid_ratios], -1)[:, None]
        wdt = self.ref_point_head.layers[0].weight.dtype
        if decoder_fast_path(self.layers, sdt) and wdt == self.layers[0].linear1.weight.dtype:
            values = batched_decoder_values(self, self.layers, src, src_padding_mask)
            t32 = output.contiguous()
            t16 = t32.to(wdt)
            for lid, layer in enumerate(self.layers):
                ref_in = reference_points[:, :, None] * vr2
                qp16 = decoder_query_pos(self.ref_point_head, ref_in[:, :, 0, :], wdt)
                t32, t16 = layer.forward16(t32, t16, qp16, ref_in, values[lid], spatial_shapes, level_start_index)
                reference_points = decoder_box_refine(self.bbox_embed[lid], t32, reference_points)
                inter.append(t32)
                inter_refs.append(reference_points)
            return torch.stack(inter), torch.stack(inter_refs)
        values = batched_decoder_values(self, self.layers, src, src_padding_mask) if decoder_split_values(self, src) else None
        for lid, layer in enumerate(self.layers):
            ref_in = reference_points[:, :, None] * vr2
            query_pos = self.ref_point_head(ops.sine_embed(ref_in[:, :, 0, :], out_dtype=wdt))      # one launch (was ~21)
            output = layer(output, query_pos, ref_in, src, spatial_shapes, level_start_index, src_padding_mask,
                           value=None if values is None else values[lid])
            new_ref = ops.box_refine(self.bbox_embed[lid](output), reference_points)               # one launch (was ~8)
            reference_points = new_ref
            inter.append(output)
            inter_refs.append(new_ref)
        return torch.stack(inter).float(), torch.stack(inter_refs)


def gen_encoder_output_proposals(memory, memory_padding_mask, shapes_list, geo_key=None):
    """deformable_transformer_dino.py:138-166 / maskdino/utils/utils.py:33-71 (without the enc_output projection).
    The proposals and the keep mask depend only on the geometry (cached); the memory masking is one masked_fill."""
    keep, prop = geo_cached(geo_key, ("proposals", tuple(shapes_list)),
                            lambda: _proposal_geometry(memory_padding_mask, shapes_list, memory.shape[0], memory.device))
    return torch.where(keep, memory, memory.new_zeros(())), prop          # one pass (masked_fill on a copy was two)


def _proposal_geometry(memory_padding_mask, shapes_list, N_, device):
    memory = None
    proposals, _cur = [], 0
    for lvl, (H_, W_) in enumerate(shapes_list):
        m = memory_padding_mask[:, _cur:_cur + H_ * W_].view(N_, H_, W_, 1)
        valid_H = torch.sum(~m[:, :, 0, 0], 1)
        valid_W = torch.sum(~m[:, 0, :, 0], 1)
        gy, gx = torch.meshgrid(torch.linspace(0, H_ - 1, H_, dtype=torch.float32, device=device),
                                torch.linspace(0, W_ - 1, W_, dtype=torch.float32, device=device), indexing="ij")
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.cat([valid_W.unsqueeze(-1), valid_H.unsqueeze(-1)], 1).view(N_, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(N_, -1, -1, -1) + 0.5) / scale
        wh = torch.ones_like(grid) * 0.05 * (2.0 ** lvl)
        proposals.append(torch.cat((grid, wh), -1).view(N_, -1, 4))
        _cur += H_ * W_
    prop = torch.cat(proposals, 1)
    valid = ((prop > 0.01) & (prop < 0.99)).all(-1, keepdim=True)
    prop = torch.log(prop / (1 - prop))
    prop = prop.masked_fill(memory_padding_mask.unsqueeze(-1), float("inf")).masked_fill(~valid, float("inf"))
    keep = (~memory_padding_mask.unsqueeze(-1)) & valid
    return keep, prop


def get_valid_ratio(mask):
    _, H, W = mask.shape
    vh = torch.sum(~mask[:, :, 0], 1).float() / H
    vw = torch.sum(~mask[:, 0, :], 1).float() / W
    return torch.stack([vw, vh], -1)


def expand_tokens(logits, full_len):
    """(..., live) per-token logits -> (..., full_len): BertEncoder(compact=True) dropped the padding rows behind `live` because they
    are all the same row (zero hidden state, zero mask: bert_model.py:118-127); their class logits are the last computed column."""
    n = logits.shape[-1]
    if full_len is None or n >= full_len:
        return logits
    out = logits.new_empty(*logits.shape[:-1], full_len)
    out[..., :n] = logits
    out[..., n:] = logits[..., -1:]
    return out


def agg_lang_feat(features, mask):
    return (features * mask.unsqueeze(-1).float()).sum(1) / mask.sum(-1).unsqueeze(-1).float()


class DeformableTransformerVLDINO(nn.Module):
    """deformable_transformer_dino.py:49-299, eval path (two-stage, mixed selection, bg queries, DECOUPLE_TGT &
    STILL_TGT_FOR_BOTH)."""

    def __init__(self, cfg, precision):
        super().__init__()
        d = cfg.hidden_dim
        self.d_model, self.nhead = d, cfg.nheads
        self.two_stage_num_proposals = cfg.num_queries
        enc_layer = DeformableTransformerEncoderLayer(d, cfg.dim_feedforward, cfg.num_feature_levels, cfg.nheads,
                                                      cfg.enc_n_points, precision.value)
        self.encoder = DeformableTransformerEncoderVL(VLFuse(cfg, precision), enc_layer, cfg.enc_layers, cfg.num_vl_layers)
        dec_layer = DeformableTransformerDecoderLayer(d, cfg.dim_feedforward, cfg.num_feature_levels, cfg.nheads,
                                                      cfg.dec_n_points, precision.value, precision.attn)
        self.decoder = DeformableTransformerDecoder(d, dec_layer, cfg.dec_layers)
        self.level_embed = nn.Parameter(torch.randn(cfg.num_feature_levels, d))
        self.tgt_embed = nn.Embedding(cfg.num_queries, d)
        self.background_proposals = cfg.num_bg_queries
        if cfg.num_bg_queries > 0:
            self.tgt_embed_bg = nn.Embedding(cfg.num_bg_queries, d)
            self.bg_query_refs = nn.Embedding(cfg.num_bg_queries, 4)
        self.enc_output = PLinear(d, d)
        self.enc_output_norm = PLayerNorm(d)
        self.resizer = FeatureResizer(cfg.lang_dim, d)
        self.pinned_topk = None          # test hook: indices for the discontinuous top-k (SURVEY 7 hard part (c))
        self.last_topk = None

    def forward(self, srcs, masks, pos_embeds, language_dict_features, task=None, geo_key=None):
        shapes_list = [tuple(int(v) for v in s.shape[-2:]) for s in srcs]
        src = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)
        gk = None if geo_key is None else (geo_key, tuple(shapes_list), src.dtype)
        mask = geo_cached(gk, "mask_flat", lambda: torch.cat([m.flatten(1) for m in masks], 1))
        # position + level embedding, one cast (src + pos would promote per layer); constant per geometry at inference
        pos = level_pos_flat(self, pos_embeds, src.dtype, gk)
        spatial_shapes, level_start_index = level_tensors(shapes_list, src.device)
        valid_ratios = geo_cached(gk, "valid_ratios", lambda: torch.stack([get_valid_ratio(m) for m in masks], 1))

        # a batch whose images all fill the canvas has an all-False padding mask: known on the host from the geometry, so the
        # 12 value projections skip their masked_fill pass (the masked formulation is what runs for ragged batches)
        no_pad = geo_key is not None and all(tuple(sz) == tuple(geo_key[1]) for sz in geo_key[0])
        layer_mask = None if no_pad else mask
        enc = self.encoder(src, shapes_list, spatial_shapes, level_start_index, valid_ratios, pos, layer_mask,
                           language_dict_features, task=task, geo_key=gk)
        memory, language_dict_features = enc["visual"], enc["lang"]
        bs = memory.shape[0]
        om, prop = gen_encoder_output_proposals(memory, mask, shapes_list, gk)
        om = self.enc_output_norm(self.enc_output(om))
        nd = self.decoder.num_layers
        enc_cls = self.decoder.class_embed[nd](om, None)
        # inference: the box head runs on the SELECTED proposals only (row-wise the same arithmetic as heading every token and gathering
        # afterwards -- deformable_transformer_dino.py:216-231 -- minus a 3-layer MLP over all 21760 tokens per image); the per-token
        # boxes are an output of the training step alone (encoder loss), which keeps the full form
        lazy_boxes = not torch.is_grad_enabled()
        enc_coord = None if lazy_boxes else self.decoder.bbox_embed[nd](om) + prop
        if self.pinned_topk is not None:
            topk = self.pinned_topk.to(src.device)
        else:
            topk = _select_topk(enc_cls[..., 0], self.two_stage_num_proposals)
        self.last_topk = topk
        if lazy_boxes:
            ref = selected_proposal_boxes(self.decoder.bbox_embed[nd], om, prop, topk).sigmoid()
        else:
            ref = torch.gather(enc_coord, 1, topk.unsqueeze(-1).repeat(1, 1, 4)).sigmoid()
        tgt = self.tgt_embed.weight[None].repeat(bs, 1, 1)
        if self.background_proposals > 0:
            tgt = torch.cat([self.tgt_embed_bg.weight[None].repeat(bs, 1, 1), tgt], dim=1)
            ref = torch.cat([self.bg_query_refs.weight[None].repeat(bs, 1, 1), ref], dim=1)
        init_ref = ref
        hs, inter_refs = self.decoder(tgt.float(), ref.float(), memory, spatial_shapes, level_start_index, valid_ratios, layer_mask)
        return hs, memory, init_ref, inter_refs, enc_cls, enc_coord, language_dict_features, shapes_list


def selected_proposal_boxes(bbox_embed, om, prop, topk):
    """bbox_embed(om)[topk] + prop[topk] computed on the gathered rows: (B, k, 4) un-activated boxes of the selected proposals."""
    om_k = torch.gather(om, 1, topk.unsqueeze(-1).expand(-1, -1, om.shape[-1]))
    prop_k = torch.gather(prop.expand(om.shape[0], -1, -1), 1, topk.unsqueeze(-1).expand(-1, -1, prop.shape[-1]))
    return bbox_embed(om_k) + prop_k


def _select_topk(scores, k):
    """indices of the k largest scores per row, descending (deformable_transformer_dino.py:222-230).  On the device this is hipie_topk: one
    launch and hipGraph-replay safe -- torch.topk is 12 launches here and faults under graph replay."""
    scores = scores.float().contiguous()
    if not ops.topk_ok(scores, k):
        # outside the kernel's range (k > 1024: e.g. TWO_STAGE_NUM_PROPOSALS 2000): the library selection on the device -- except inside a
        # hipGraph capture, where torch.topk is known to fault on replay, and never on the host
        if scores.is_cuda and not torch.cuda.is_current_stream_capturing():
            return torch.topk(scores, k, dim=1)[1]
        raise RuntimeError("two-stage selection: k=%d of %s scores on %s is outside hipie_topk's range (device tensor, k <= 1024) and "
                           "torch.topk is not usable here (host tensor or hipGraph capture)" % (k, tuple(scores.shape), scores.device))
    return ops.topk(scores, k)


# --------------------------------------------------------------------------- heads
class VL_Align(nn.Module):
    """deformable_detr.py:40-73 (LOG_SCALE 0.0, PRIOR_PROB 0.01, CLAMP_DOT_PRODUCT True)."""

    def __init__(self, cfg):
        super().__init__()
        bias_value = -math.log((1 - cfg.prior_prob) / cfg.prior_prob)
        self.dot_product_projection_text = PLinear(cfg.lang_dim, cfg.hidden_dim)
        self.log_scale = nn.Parameter(torch.Tensor([cfg.log_scale]))
        self.bias_lang = nn.Parameter(torch.zeros(cfg.lang_dim))
        self.bias0 = nn.Parameter(torch.Tensor([bias_value]))

    def forward(self, x, embedding):
        embedding = F.normalize(embedding, p=2, dim=-1)
        p = self.dot_product_projection_text
        if (getattr(p, "split", False) and x.is_cuda and x.dim() == 3 and embedding.dim() == 3 and p.weight.dtype == torch.float32
                and ops.split_ok(embedding.shape[-1]) and ops.split_ok(p.weight.shape[0])):
            # split policy: no library GEMM here either.  The token projection and the language bias `embedding . bias_lang` are ONE
            # hipie_gemm (the bias vector is an extra output row of the projection: the operand is embedding / 2, so the row is 2 bias_lang),
            # the per-image logits `x . tok^T` one hipie_gemm_batched launch
            d = p.weight.shape[0]
            ta = ops.split_linear((embedding * 0.5).contiguous(), self, "tok_aug", p.weight, p.bias,
                                  weight_fn=lambda: torch.cat([p.weight.float(), 2.0 * self.bias_lang.float()[None]], 0),
                                  bias_fn=lambda: torch.cat([p.bias.float(), torch.zeros(1, device=p.bias.device)], 0),
                                  params=[p.weight, p.bias, self.bias_lang])
            tok, bias = ta[..., :d], ta[..., d] + self.bias0
            logit = ops.matmul_nt_batched(x.float(), tok.contiguous()) / self.log_scale.exp() + bias.unsqueeze(1)
            return logit.clamp(max=50000).clamp(min=-50000)
        tok = p(embedding / 2.0)
        bias = torch.matmul(embedding, self.bias_lang) + self.bias0
        logit = torch.matmul(x, tok.transpose(-1, -2)) / self.log_scale.exp() + bias.unsqueeze(1)
        return logit.clamp(max=50000).clamp(min=-50000)


class Still_Classifier(nn.Module):
    def __init__(self, hidden_dim):
        super().__init__()
        self.body = PLinear(hidden_dim, 1)

    def forward(self, x, lang_feat=None):
        return self.body(x)


def input_proj_list(channels, hidden_dim, num_levels):
    lst = [nn.Sequential(PConv2d(c, hidden_dim, kernel_size=1), PGroupNorm(32, hidden_dim)) for c in channels]
    c = channels[-1]
    for _ in range(num_levels - len(channels)):
        lst.append(nn.Sequential(PConv2d(c, hidden_dim, kernel_size=3, stride=2, padding=1), PGroupNorm(32, hidden_dim)))
        c = hidden_dim
    return nn.ModuleList(lst)


class DeformableDETRDINO(nn.Module):
    """deformable_detr.py:181-291 (with_box_refine, two_stage, USE_IOU_BRANCH, STILL_CLS_FOR_ENCODER)."""

    def __init__(self, backbone, transformer, cfg):
        super().__init__()
        self.transformer = transformer
        d = cfg.hidden_dim
        num_pred = cfg.dec_layers + 1
        self.class_embed = _get_clones(VL_Align(cfg), num_pred)
        self.bbox_embed = _get_clones(MLP(d, d, 4, 3), num_pred)
        self.iou_head = _get_clones(PLinear(d, 1), num_pred - 1)
        self.num_feature_levels = cfg.num_feature_levels
        self.input_proj = input_proj_list(backbone.num_channels, d, cfg.num_feature_levels)
        self.backbone = backbone
        self.transformer.decoder.bbox_embed = self.bbox_embed
        self.transformer.decoder.class_embed = self.class_embed
        self.transformer.decoder.class_embed[-1] = Still_Classifier(d)
