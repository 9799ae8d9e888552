"""The network of the TRAINING step: a differentiable forward over the parameters of the product model (the same
state_dict layout as the reference, hipie_amd/hipie_img.py), written for autograd instead of for speed -- the inference path's fused
kernels have no backward.  What is hand-written HIP here is what has a backward kernel: multi-scale deformable attention
(hipie_msda_forward / hipie_msda_backward), the mask contraction and the CondInst dynamic mask head (training/functions.py); the dense
linears, LayerNorm / GroupNorm, the softmax attentions and the convolutions run on the library kernels PyTorch-ROCm dispatches to, with
torch.autograd providing their backward (the dense 3 x 3 convolutions have a node of their own in the opt-in group "convs", the 1 x 1 and transposed ones in "projections").  More of the step runs on hand-written kernels opt-in, one HipBackend* class per kernel group:
GROUPS, EXTRA_GROUPS and LATER_GROUPS below name them, backend(*names) composes any of them into the class TrainStep takes.

Functional style over a dict ``sd`` of LIVE parameters (model.named_parameters() + buffers, reference key names), so gradients land in the
model's own parameters.  Every function cites the reference code it follows.  Training-mode differences from the inference path:
de-noising queries and their attention masks in both decoders, per-layer outputs, reference points detached between decoder layers
(deformable_transformer_dino.py:505, dino_decoder.py:160), the encoder's proposal logits / boxes for the encoder loss.

The three operator kernels come from a ``Backend``; the default is the HIP library and refuses host tensors.  tests/ plug the oracle's
restatements in to check the host logic without a GPU."""
import math

import torch
import torch.nn.functional as F


_LEVELS = {}


def level_tensors(shapes, device, which="int"):
    """the pyramid's [(H, W)] as device tensors, built once per geometry: (spatial_shapes int64, level_start_index) or, which="wh", the
    (L, 2) float (W, H) normaliser.  A host list -> device tensor is a pageable copy, i.e. a host wait for everything queued on the stream:
    two of them per MSDeformAttn call kept the host from ever running ahead of the GPU (127 ms per forward of it sitting there, sampled)."""
    key = (tuple((int(h), int(w)) for h, w in (shapes.tolist() if torch.is_tensor(shapes) else shapes)), str(device))
    if key not in _LEVELS:
        ss = torch.as_tensor(key[0], dtype=torch.int64, device=device)
        ls = torch.cat((ss.new_zeros(1), ss.prod(1).cumsum(0)[:-1]))
        _LEVELS[key] = (ss, ls, torch.stack((ss[:, 1], ss[:, 0]), -1).float())
    ss, ls, wh = _LEVELS[key]
    return wh if which == "wh" else (ss, ls)


class HipBackend:
    """the operator kernels with a hand-written backward (libhipie_mi355.so); no host path"""

    @staticmethod
    def linear(x, sd, p):
        """the big linears (ViT qkv / proj / mlp, encoder FFN) on the split-fp16 GEMM, forward and backward (functions.SplitLinearFunction);
        the HL8 copies of W and W^T are cached on the weight tensor itself, so they die with it"""
        from .functions import split_linear
        w = sd[p + "weight"]
        return split_linear(x, w, sd.get(p + "bias"), w, "w")

    @staticmethod
    def msda(value, shapes, loc, aw):
        """value (B,S,M,D), shapes [(H,W)], loc (B,Lq,M,L,P,2), aw (B,Lq,M,L,P) -> (B,Lq,M*D)"""
        from ..msda_shim import MSDeformAttnFunction
        ss, ls = level_tensors(shapes, value.device)
        return MSDeformAttnFunction.apply(value.contiguous(), ss, ls, loc.contiguous(), aw.contiguous(), 64)

    @staticmethod
    def fused_attention(qa, ka, v):
        """softmax(q' k'^T) v of a ViT block on the fused split-fp16 kernels when the shape is covered (head width 80, <= 224 operand columns;
        large token counts that are not a multiple of 128 are padded with masked keys), else None: the caller's materialised formulation
        runs (the 196-token windows, where it is the faster one)"""
        from .functions import fused_attention
        return fused_attention(qa, ka, v)

    @staticmethod
    def mask_einsum(mask_embed, mask_features):
        from .functions import mask_einsum
        return mask_einsum(mask_embed, mask_features)

    @staticmethod
    def dynamic_mask(mask_feats, ref_points, params, num_insts, stride, up):
        """mask_feats (B,8,H,W); ref_points (sum n_i, 2) pixels; params (sum n_i, 169); num_insts per image -> (sum n_i, up*H, up*W)"""
        from .functions import dynamic_mask
        outs, st = [], 0
        for b, n in enumerate(num_insts):
            if n:
                outs.append(dynamic_mask(mask_feats[b:b + 1], ref_points[st:st + n], params[st:st + n], n, stride, up).reshape(n, up * mask_feats.shape[2], -1))
            st += n
        if not outs:
            return mask_feats.new_zeros(0, up * mask_feats.shape[2], up * mask_feats.shape[3])
        return torch.cat(outs, 0)


class HipBackendNorms(HipBackend):
    """HipBackend + the LayerNorms of the ViT blocks and of the deformable encoder layers on the hand-written pair hipie_add_layernorm /
    hipie_layernorm_backward (opt-in: TrainStep's default stays HipBackend).  The decoder layers, the fusion block, BERT and the head
    norms keep F.layer_norm: a few hundred rows each, launch-bound."""

    @staticmethod
    def add_layer_norm(x, delta, weight, bias, eps):
        """(s, y) = (x + delta, LayerNorm(s) * weight + bias); delta None: s = x (functions.AddLayerNormFunction)"""
        from .functions import add_layer_norm
        return add_layer_norm(x, delta, weight, bias, eps)


class HipBackendMlp(HipBackend):
    """HipBackend + the MLP of every ViT block and the FFN of every deformable encoder layer as ONE autograd node (functions.MlpFunction:
    hipie_act_forward / hipie_act_backward between the split GEMMs; the activation is recomputed in the backward instead of saved).
    Opt-in: TrainStep's default stays HipBackend."""

    @staticmethod
    def mlp(x, sd, p_fc1, p_fc2, act):
        """linear(act(linear(x, p_fc1)), p_fc2); act = "gelu" | "relu" (functions.split_mlp: shapes the split GEMM does not take run the
        three-node composition)"""
        from .. import ops
        from .functions import split_mlp
        return split_mlp(x, sd[p_fc1 + "weight"], sd.get(p_fc1 + "bias"), sd[p_fc2 + "weight"], sd.get(p_fc2 + "bias"),
                         {"gelu": ops.ACT_GELU, "relu": ops.ACT_RELU}[act])


class HipBackendNormsMlp(HipBackendNorms, HipBackendMlp):
    """both opt-in groups: the hand-written LayerNorm pair and the one-node MLP"""


class HipBackendWindows(HipBackend):
    """HipBackend + the attention of the WINDOWED ViT blocks (196-token windows) on the short-sequence instance of the fused split-fp16
    kernels (functions.WindowAttentionFunction, csrc/attn_train_win.hip): no (windows x heads, 196, 196) tensor in HBM, forward or backward.
    Opt-in: TrainStep's default stays HipBackend."""

    @staticmethod
    def window_attention(qa, ka, v):
        """softmax(q' k'^T) v for items of at most 256 tokens (head width 80, <= 128 operand columns), else None: the materialised
        formulation runs.  Asked only where fused_attention declined."""
        from .functions import window_attention
        return window_attention(qa, ka, v)


class HipBackendPackedAttention(HipBackend):
    """HipBackend + the attention of the GLOBAL ViT blocks as ONE autograd node from the rows of the qkv linear to the rows of the proj linear
    (functions.VitAttentionFunction): the operands of the fused kernels are packed from / unpacked into the token-major rows by
    hipie_attn_pack_* (csrc/attn_pack.hip) instead of a chain of torch passes, the attention kernels and their operand bits being the same.
    The windowed blocks keep the materialised formulation.  Opt-in: TrainStep's default stays HipBackend."""

    @staticmethod
    def packed_attention(qkv, Rh, Rw, heads, H, W):
        """qkv (B', H W, 3 heads hd), Rh (H, H, hd), Rw (W, W, hd) of get_rel_pos -> (B', H W, heads hd), or None: vit_attention's own
        composition runs (functions.vit_attention_packed names what is covered)"""
        from .functions import vit_attention_packed
        return vit_attention_packed(qkv, Rh, Rw, heads, H, W, windows=False)


class HipBackendPackedWindows(HipBackendPackedAttention, HipBackendWindows):
    """HipBackendPackedAttention + the same node over the short-sequence kernels of HipBackendWindows for the WINDOWED blocks (a block the
    node does not cover falls to HipBackendWindows' composition)"""

    @staticmethod
    def packed_attention(qkv, Rh, Rw, heads, H, W):
        from .functions import vit_attention_packed
        return vit_attention_packed(qkv, Rh, Rw, heads, H, W, windows=True)


class HipBackendAll(HipBackendNorms, HipBackendMlp, HipBackendWindows):
    """the three opt-in groups: the hand-written LayerNorm pair, the one-node MLP and the fused windowed attention"""


class HipBackendDeformable(HipBackend):
    """HipBackend + every MSDeformAttn module's sampling as ONE autograd node from the raw sampling_offsets / attention_weights projections
    (functions.DeformSampleFunction: hipie_msda_fused_forward / hipie_msda_raw_backward): no location tensor, no softmax output and none of
    the torch passes between the projections and the operator, forward or backward.  The value mask fill and the three linears stay torch
    nodes.  Opt-in: TrainStep's default stays HipBackend."""

    @staticmethod
    def msda_raw(value, shapes, ref, offsets, logits):
        """value (B,S,M,D), shapes [(H,W)], ref (B,Lq,L,2|4), offsets (B,Lq,M,L,P,2), logits (B,Lq,M,L*P) -> (B,Lq,M*D), or None: msda_module's
        own composition runs (functions.deform_sample names what is covered)"""
        from .functions import deform_sample
        return deform_sample(value, shapes, ref, offsets, logits)


class HipBackendLosses(HipBackend):
    """HipBackend + the element-wise losses of both criteria on csrc/point_loss.hip: the point-sampled mask losses of a criterion call as one
    node that indexes the un-gathered targets (functions.PointMaskLossFunction) and the token focal loss with the pad tokens dropped inside
    the kernel (functions.TokenFocalFunction).  TrainStep hands the backend to DetCriterion / MaskCriterion as their `ops`.
    Opt-in: TrainStep's default stays HipBackend; HipBackendAll does not include it."""

    @staticmethod
    def point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha):
        """src (N,H,W), tgt_maps (T,Ht,Wt), tgt_index (N,), pts (N,P,2); mode 0 = sigmoid CE, 1 = focal -> (lmask (N,), ldice (N,))"""
        from .functions import point_mask_loss
        return point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha)

    @staticmethod
    def token_focal_sum(logits, onehot, text_mask, alpha):
        """logits, onehot (B,Q,T), text_mask (B,T) or None -> the scalar criterion.token_focal_loss returns"""
        from .functions import token_focal_sum
        return token_focal_sum(logits, onehot, text_mask, alpha)


class HipBackendCriteria(HipBackendLosses):
    """HipBackendLosses + the two no_grad places that sample a mask at points, on csrc/point_select.hip: the importance point selection of both
    criteria (functions.uncertain_points: the candidates' samples, the selection and the gather as two launches) and the mask costs of the
    matchers (functions.mask_match_costs: the targets sampled once, the (Q, P) samples never written).  TrainStep hands the backend to the
    criteria AND the matchers as their `ops`; with it nothing in them that samples a mask at points goes through grid_sample.
    Opt-in: TrainStep's default stays HipBackend; HipBackendLosses and HipBackendAll do not include it."""

    @staticmethod
    def uncertain_points(src, cand, rest, k, num_points=None):
        """src (N,H,W), cand (N,C,2), rest (N,P-k,2) or None -> pts (N,P,2): the k candidates with the smallest |sampled logit| in ascending
        candidate index, then rest.  num_points: the caller's P (a rest of another length than P - k is refused)"""
        from .functions import uncertain_points
        return uncertain_points(src, cand, rest, k, num_points)

    @staticmethod
    def mask_match_costs(pred, tgt, coords):
        """pred (Q,H,W), tgt (T,Ht,Wt), coords (P,2) -> (ce (Q,T), dice (Q,T)) of matcher.mask_costs"""
        from .functions import mask_match_costs
        return mask_match_costs(pred, tgt, coords)


class HipBackendMatching(HipBackendCriteria):
    """HipBackendCriteria + the one-to-many SimOTA matching of the foreground queries on csrc/ota_match.hip (functions.ota_match: the cost of
    the whole batch from the raw logits and the dynamic-k assignment with its repair loop as two launches and one host read per decoder
    level, instead of a Python loop over the images and the targets with a host wait each).  TrainStep packs the targets once per step
    (functions.pack_ota_targets) and hands the backend to the matchers as their `ops`; HungarianMatcher.forward_ota asks it first and keeps
    its torch path for shapes outside the kernels' limits.
    Opt-in: TrainStep's default stays HipBackend; HipBackendCriteria and HipBackendAll do not include it."""

    @staticmethod
    def pack_ota_targets(targets, device):
        """per-image target dicts -> functions.OtaTargets (padded boxes and positive maps, the counts on the device and on the host)"""
        from .functions import pack_ota_targets
        return pack_ota_targets(targets, device)

    @staticmethod
    def ota_match(logits, boxes, packed, center_radius=2.5, stride=32):
        """logits (B,Q,L), boxes (B,Q,4), packed -> (pairs, best) of HungarianMatcher.forward_ota, or None outside the kernels' limits"""
        from .functions import ota_match
        return ota_match(logits, boxes, packed, center_radius, stride)


class HipBackendHungarian(HipBackendMatching):
    """HipBackendMatching + the cost matrices of the one-to-one Hungarian matchers on csrc/hungarian_cost.hip (functions.hungarian_costs: the
    class, box and stuff-mean costs of the whole batch as one or two launches on top of the three mask-cost launches per image, ONE device ->
    host copy per matcher call, scipy on host slices of it -- instead of about forty launches and two host waits per image).  TrainStep packs
    the background targets once per step and the criteria pack theirs once per call (functions.pack_match_targets); HungarianMatcher.forward /
    forward_boxes_only ask the backend first and keep their torch loop for shapes outside the kernel's limits.
    Opt-in: TrainStep's default stays HipBackend; HipBackendMatching and HipBackendAll do not include it."""

    @staticmethod
    def pack_match_targets(targets, device, with_masks=True):
        """per-image target dicts -> functions.MatchTargets (padded boxes, positive maps / labels, is_thing, counts and offsets, fp32 masks)"""
        from .functions import pack_match_targets
        return pack_match_targets(targets, device, with_masks)

    @staticmethod
    def hungarian_costs(logits, boxes, packed, w, masks=None, coords=None, stuff_takes_mean=True, with_boxes=True, class_mode="auto"):
        """logits (B,Q,L), boxes (B,Q,4), packed -> per image the (Q, T_i) cost matrix on the host, or None outside the kernel's limits"""
        from .functions import hungarian_costs
        return hungarian_costs(logits, boxes, packed, w, masks, coords, stuff_takes_mean, with_boxes, class_mode)


class HipBackendAssign(HipBackendHungarian):
    """HipBackendHungarian + the one-to-one assignment itself on csrc/hungarian_assign.hip (functions.hungarian_match: the packed costs stay
    on the device and one more launch solves every image's assignment there, with scipy's pairs tie for tie -- no device -> host copy of the
    costs, no scipy, no host -> device copy of the pairs).  A matcher call is two or three kinds of launches and no host wait; the pairs are
    device int64 tensors whose lengths the host knows from the packed counts.  TrainStep builds its matchers with defer_status=True and reads
    the status words of all their calls once, at the end of loss_dict (HungarianMatcher.check).
    Opt-in: TrainStep's default stays HipBackend; HipBackendHungarian and HipBackendAll do not include it."""

    @staticmethod
    def hungarian_match(logits, boxes, packed, w, masks=None, coords=None, stuff_takes_mean=True, with_boxes=True, class_mode="auto"):
        """logits (B,Q,L), boxes (B,Q,4), packed -> (per image (query idx, target idx) int64 on the device, status (B,) int32 on the device),
        or None outside the kernels' limits"""
        from .functions import hungarian_match
        return hungarian_match(logits, boxes, packed, w, masks, coords, stuff_takes_mean, with_boxes, class_mode)


class HipBackendPairLosses(HipBackendAssign):
    """HipBackendAssign + what the criteria do with the matched pairs, on csrc/pair_loss.hip: loss_boxes of both criteria as one node that
    reads the pairs where the matchers left them (functions.PairBoxLossFunction: two launches forward, one backward, the final scalars; no
    gather, no `thing.sum() == 0` / degenerate-box read on the host) and the positive one-hot in front of every token focal loss as a fill and
    one scatter (functions.positive_onehot).  The criteria keep the status words of their loss_boxes calls pending; TrainStep reads them with
    the matchers' in the one copy at the end of loss_dict.
    Opt-in: TrainStep's default stays HipBackend; HipBackendAssign and HipBackendAll do not include it."""

    @staticmethod
    def pack_pair_targets(targets, device):
        """per-image target dicts -> functions.MatchTargets without masks and count vectors: no host -> device copy (the matcher's own
        packing serves the two ops as well)"""
        from .functions import pack_pair_targets
        return pack_pair_targets(targets, device)

    @staticmethod
    def pair_box_loss(pred_boxes, pred_iou, pairs, packed, count, mode, use_thing=True):
        """pred_boxes (B,Q,4), pred_iou None | (B,Q[,1]), pairs, packed targets -> (loss_bbox, loss_giou, loss_boxiou | None, status), or None
        outside the kernels' limits"""
        from .functions import pair_box_loss
        return pair_box_loss(pred_boxes, pred_iou, pairs, packed, count, mode, use_thing)

    @staticmethod
    def positive_onehot(logits, pairs, packed):
        """logits (B,Q,L), pairs, packed targets -> onehot (B,Q,L), or None outside the kernel's limits"""
        from .functions import positive_onehot
        return positive_onehot(logits, pairs, packed)


class HipBackendGroupNorms(HipBackend):
    """HipBackend + the GroupNorm (+ ReLU) of the 11 conv + GN blocks of a step -- input_proj.0-3 of the detection head and of the MaskDINO
    pixel decoder, its adapter_1, layer_1 and mask_features, the last two with their ReLU -- as ONE autograd node each on
    hipie_group_norm_train_forward / hipie_group_norm_backward (functions.GroupNormFunction; opt-in: TrainStep's default stays HipBackend).
    NCHW fp32 as the convolutions hand it over.  Not here: channels-last maps, 16-bit operands, the transposed convolution's bias as a
    pre-bias (it keeps its bias), writing the normalised levels straight into the token stream."""

    @staticmethod
    def group_norm(x, groups, weight, bias, eps, relu):
        """GroupNorm(groups)(x) * weight + bias (+ ReLU), or None outside the kernels' limits (gn then runs F.group_norm).  A map the
        convolution left in another layout (the library picks channels-last outputs for the 1 x 1 / strided projections when the other ViT
        groups are composed in) is copied to NCHW first, the kernels' training layout; no copy where the map is NCHW already"""
        from .functions import group_norm
        return group_norm(x.contiguous(), groups, weight, bias, eps, relu)


class HipBackendQueryAttention(HipBackend):
    """HipBackend + the query self-attention of every decoder layer -- 6 in the thing branch, 9 in MaskDINO: nn.MultiheadAttention with
    q = k = tgt + query_pos, v = tgt, 8 heads of 32 and the de-noising attn_mask -- as ONE autograd node between the in-projection and
    out_proj on hipie_attn_f32_train_forward / hipie_attn_f32_train_backward (functions.QueryAttentionFunction, csrc/attn_f32_train.hip):
    exact fp32 as the inference path's attn_f32, no (B, 8, N, N) tensor in HBM forward or backward, q | k from one linear.
    Opt-in: TrainStep's default stays HipBackend.  Not here: the layers' LayerNorms and FFN, the vision-language fusion attention, head
    widths other than 32, dropout."""

    @staticmethod
    def query_attention(qk, v, attn_mask, heads):
        """qk (B, N, 2 C) rows of the q | k in-projection, v (B, N, C) rows, attn_mask None | (N, N) bool (True = blocked) -> (B, N, C), or
        None outside the kernels' limits (mha then runs its materialised formulation; functions.query_attention_ok names the limits)"""
        from .functions import query_attention
        return query_attention(qk, v, attn_mask, heads)


class HipBackendFusionAttention(HipBackend):
    """HipBackend + the vision-language fusion attention of every vl layer -- BiMultiHeadAttention.forward (fuse_helper.py:54-139), 8 heads of
    256, both directions, with the block's attention dropout -- as ONE autograd node between the four input projections and the two output
    projections on hipie_bi_attn_train_forward / hipie_bi_attn_train_backward (functions.FusionAttentionFunction, csrc/bi_attn_train.hip):
    exact fp32, no (B 8, Nv, L) tensor in HBM forward or backward, the 256^-0.5 scale folded into the kernels.  The dropout masks are a
    stateless function of a per-call 64-bit seed (torch's default CPU generator) and the element's indices, not F.dropout's random stream.
    An image with NO attended text token is outside the contract: its out_v rows are 0 and that direction gives no gradient, where the
    reference gives a uniform row.
    Opt-in: TrainStep's default stays HipBackend.  Not here: the folded form of the inference path (no (B, Nv, 2048) projection at all),
    16-bit operands, L > 256 (declined), a pad mask on the visual side (the reference has none), the block's LayerNorms and projections,
    making the group the default."""

    @staticmethod
    def fusion_attention(q, k, vv, vl, text_mask, heads, dropout):
        """q (B, Nv, E) UNSCALED v_proj rows, k (B, L, E) l_proj rows, vv / vl the value projections, text_mask (B, L) (non-zero = attended),
        the dropout rate -> (out_v (B, Nv, E), out_l (B, L, E)), or None outside the kernels' limits (bi_attention_block then runs its
        materialised formulation; functions.fusion_attention_ok names the limits)"""
        from .functions import fusion_attention
        return fusion_attention(q, k, vv, vl, text_mask, heads, dropout)


class HipBackendConvs(HipBackend):
    """HipBackend + the dense 3 x 3 / stride 1 / padding 1 convolutions that carry the conv flops of a step -- lay3, lay4, jia_dcn and lay1 of
    the CondInst mask head with their ReLU, layer_1 of the MaskDINO pixel decoder without one (its ReLU stays with the GroupNorm behind it)
    -- as ONE autograd node each (functions.Conv3x3Function): forward and input gradient on hipie_conv3x3_split, the inference path's
    implicit GEMM on a zero-padded pixel grid, weight and bias gradient on hipie_conv3x3_wgrad (csrc/conv_wgrad.hip); three-product split
    fp16 with fp32 accumulation in all three passes.  With ReLU the backward's mask is the node's own y > 0: no pre-ReLU map is kept.
    Opt-in: TrainStep's default stays HipBackend.  Not here: the stride-2 and 1 x 1 projections, the transposed convolutions, 16-bit
    operands, lay2 (64 -> 8 channels: declined, F.conv2d runs), making the group the default."""

    @staticmethod
    def conv3x3(x, weight, bias, relu):
        """conv2d(x, weight, bias, padding=1) (+ ReLU) -> (B, N, H, W), a channels-last view of the node's output grid, or None outside the
        kernels' limits (conv then runs F.conv2d; functions.conv3x3_train_ok names the limits)"""
        from .functions import conv3x3_train
        return conv3x3_train(x, weight, bias, relu)


class HipBackendProjections(HipBackend):
    """HipBackend + the convolutions whose kernel equals their stride, and the two transposed ones, as ONE autograd node each
    (functions.PatchConvFunction): the simple feature pyramid's fpn1.0 and the pixel decoder's mask_features.0 (ConvTranspose2d 2 x 2 /
    stride 2), the 1 x 1 input_proj.0-2 of both heads, adapter_1 and mask_features.3.  Each is a linear over patch rows on the split GEMM
    -- forward, device-scaled input gradient and split-K weight gradient are the entries the linears use -- plus a layout change done once
    by the operand producer hipie_patch_pack (csrc/patch_pack.hip); a channels-last map is its own rows.  Outputs and input gradients
    are channels-last views.  NEW ops, so no op is defined by two groups.  The group runs on SPLIT operands under half_policy too: the
    policy composes the half-precision linears in front of a backend and does not touch these ops.
    Opt-in: TrainStep's default stays HipBackend.  NOT routed: the 16 x 16 patch embedding.  The node takes it (k = 16, input frozen;
    tests/test_gpu_patch_conv.py, tools/bench_patch_conv.py), but with it in the group the golden step's sampling-offsets gradients are
    5.5e-3 of their largest entry off the fixture, in every composition measured, where the step checker allows 5e-3: a 1e-7 change at
    the root of the ViT moves a sampling point of the pixel decoder's first encoder layer across a pixel boundary, where that gradient is
    discontinuous (docs/measurements.md).  vit_backbone keeps F.conv2d for it.  Not here either: the stride-2 3 x 3 input_proj.3 (two
    sites of 512 rows x K = 11520), dy scaling of the 3 x 3 node, a scatter for a trainable input with k > 1 (declined), 16-bit
    operands, making the group the default."""

    @staticmethod
    def conv_patch(x, weight, bias, stride):
        """conv2d(x, weight, bias, stride=stride) for a k x k kernel with stride k and no padding -> (B, Cout, H/k, W/k), a channels-last
        view, or None outside the limits (the caller's F.conv2d then runs; functions.patch_conv_train_ok names the limits)"""
        from .functions import patch_conv_train
        return patch_conv_train(x, weight, bias, stride)

    @staticmethod
    def convt2x2(x, weight, bias):
        """conv_transpose2d(x, weight, bias, stride=2) for a 2 x 2 kernel -> (B, Cout, 2 H, 2 W), a channels-last view, or None outside the
        limits (the caller's F.conv_transpose2d then runs)"""
        from .functions import patch_convt_train
        return patch_convt_train(x, weight, bias)


class HipBackendScaledGrads(HipBackend):
    """HipBackend + SCALED gradient operands in the backward of the split linears -- the ViT qkv / proj / fc1 / fc2 and the encoder FFNs: every
    output gradient that enters a split GEMM is first multiplied by a power of two chosen on the device from its largest magnitude, in the
    one pass that writes both of its operand forms and the bias gradient (csrc/grad_pack.hip), and the product is multiplied back where it is
    stored (functions.ScaledSplitLinearFunction / ScaledMlpFunction).  The raw split of HipBackend.linear is 2^-22 accurate only while dy
    is a normal fp16 number (6.1e-5 .. 65504 per element); with the scale the accuracy does not depend on the magnitude of dy.  The
    forward is HipBackend.linear's, bit for bit.  NEW ops, so no op is defined by two groups: _blin asks linear_scaled first, _bmlp
    asks mlp_scaled first when the backend also has `mlp` (without it: the three nodes over _blin), and the mask logits ask
    mask_einsum_scaled first -- the mask contraction's backward splits its output gradient too, and with a small loss it is the first to
    lose it (tests/test_gpu_grad_scale.py, the step with the loss multiplied by 2^-20).
    Opt-in: TrainStep's default stays HipBackend.  Not here: dy of the convolution node (functions.Conv3x3Function), the decoder / head
    F.linear calls, loss scaling of the whole step, making the group the default."""

    @staticmethod
    def linear_scaled(x, sd, p):
        """HipBackend.linear with the scaled-gradient backward (functions.split_linear_scaled)"""
        from .functions import split_linear_scaled
        w = sd[p + "weight"]
        return split_linear_scaled(x, w, sd.get(p + "bias"), w, "w")

    @staticmethod
    def mask_einsum_scaled(mask_embed, mask_features):
        """HipBackend.mask_einsum whose backward scales the output gradient in front of its two split products (functions.ScaledMaskEinsumFunction):
        the per-pixel gradient of the mask losses is the smallest of the step"""
        from .functions import mask_einsum_scaled
        return mask_einsum_scaled(mask_embed, mask_features)

    @staticmethod
    def mlp_scaled(x, sd, p_fc1, p_fc2, act):
        """HipBackendMlp.mlp with the scaled-gradient backward (functions.split_mlp_scaled)"""
        from .. import ops
        from .functions import split_mlp_scaled
        return split_mlp_scaled(x, sd[p_fc1 + "weight"], sd.get(p_fc1 + "bias"), sd[p_fc2 + "weight"], sd.get(p_fc2 + "bias"),
                                {"gelu": ops.ACT_GELU, "relu": ops.ACT_RELU}[act])


class HipBackendHalfLinears(HipBackend):
    """HipBackend + the linears that carry the step's flops -- the ViT qkv / proj / fc1 / fc2 and the encoder FFNs -- in HALF precision: ONE
    fp16 MFMA product per GEMM instead of the three of the split GEMM, fp32 master weights, fp32 accumulation and output, the output
    gradient scaled by a power of two chosen on the device (functions.HalfLinearFunction / HalfMlpFunction, csrc/half_pack.hip).
    A PRECISION POLICY, not a bit-compatible group: results differ from HipBackend's at the 2^-11 level of an fp16 operand, so it is NOT a
    member of GROUPS / EXTRA_GROUPS / LATER_GROUPS (whose every name is held to the fp32-class bounds of the golden step) and net.backend
    never returns it; half_policy(backend_class) composes it in front of a backend class.  NEW ops, so no op is defined twice: _blin asks
    linear_half first, _bmlp asks mlp_half first when the backend also has `mlp` (without it: the three nodes over _blin).  Linears outside
    functions.half_linear_ok run the split node."""

    @staticmethod
    def linear_half(x, sd, p):
        """HipBackend.linear on single fp16 operands (functions.half_linear)"""
        from .functions import half_linear
        w = sd[p + "weight"]
        return half_linear(x, w, sd.get(p + "bias"), w, "w")

    @staticmethod
    def mlp_half(x, sd, p_fc1, p_fc2, act):
        """HipBackendMlp.mlp on single fp16 operands (functions.half_mlp)"""
        from .. import ops
        from .functions import half_mlp
        return half_mlp(x, sd[p_fc1 + "weight"], sd.get(p_fc1 + "bias"), sd[p_fc2 + "weight"], sd.get(p_fc2 + "bias"),
                        {"gelu": ops.ACT_GELU, "relu": ops.ACT_RELU}[act])


_HALF_POLICY = {}


def half_policy(backend_class):
    """backend_class (HipBackend, or any class net.backend returns) with the half-precision linears composed in front of it: one class per
    backend class, built once.  Opt-in; TrainStep's default stays HipBackend."""
    if issubclass(backend_class, HipBackendHalfLinears):
        return backend_class
    if backend_class not in _HALF_POLICY:
        _HALF_POLICY[backend_class] = type("Half" + backend_class.__name__, (HipBackendHalfLinears, backend_class),
                                           {"__doc__": "the half-precision linears in front of " + backend_class.__name__})
    return _HALF_POLICY[backend_class]


# the opt-in kernel groups by name; a composed class lists its bases in this order
GROUPS = {"norms": HipBackendNorms, "mlp": HipBackendMlp, "windows": HipBackendWindows, "packed_attention": HipBackendPackedAttention,
          "packed_windows": HipBackendPackedWindows, "deformable": HipBackendDeformable, "losses": HipBackendLosses, "criteria": HipBackendCriteria,
          "matching": HipBackendMatching, "hungarian": HipBackendHungarian, "assign": HipBackendAssign, "pair_losses": HipBackendPairLosses}
# the groups that joined after GROUPS' keys and order were pinned (tests/test_backend_compose_cpu.py): a composed class lists them last
EXTRA_GROUPS = {"group_norms": HipBackendGroupNorms}
# the table every later group joins, at its end: a composed class lists these after the GROUPS and EXTRA_GROUPS classes.
# It GROWS: a test may assert that a name is in it and where it stands relative to another name, never the table's full contents.
LATER_GROUPS = {"query_attention": HipBackendQueryAttention, "fusion_attention": HipBackendFusionAttention, "convs": HipBackendConvs,
                "scaled_grads": HipBackendScaledGrads, "projections": HipBackendProjections}
# Among the bases of a composed class the two attention groups keep the END, in this order (tests/test_fusion_attention_cpu.py pins
# HipBackendFusionAttention as the last base of the every-group class); a group that joins LATER_GROUPS behind them is listed in front of
# them.  The groups are unrelated by inheritance and share no op, so the order of the bases changes nothing a step computes.
_LAST_BASES = ("query_attention", "fusion_attention")
_COMPOSED = {("norms", "mlp"): HipBackendNormsMlp, ("norms", "mlp", "windows"): HipBackendAll}


def backend(*names):
    """the backend class with the named opt-in groups (keys of GROUPS, EXTRA_GROUPS and LATER_GROUPS); none: HipBackend.  A group another named group inherits from is
    implied by it and dropped ("losses" beside "matching", "windows" and "packed_attention" beside "packed_windows"): what is left is
    unrelated by inheritance, so its classes compose as bases in any order, and no op is defined by two of them (tests/
    test_backend_compose_cpu.py, every subset).  One group left: its own class; several: one class per set of groups, built once."""
    known = {**GROUPS, **EXTRA_GROUPS, **LATER_GROUPS}
    unknown = sorted(set(names) - set(known))
    if unknown:
        raise ValueError("unknown backend group(s) %s; known: %s" % (", ".join(map(repr, unknown)), ", ".join(known)))
    named = [known[n] for n in names]
    order = [n for n in known if n not in _LAST_BASES] + list(_LAST_BASES)
    left = tuple(n for n in order if known[n] in named and not any(o is not known[n] and issubclass(o, known[n]) for o in named))
    if len(left) < 2:
        return known[left[0]] if left else HipBackend
    if left not in _COMPOSED:
        bases = tuple(known[n] for n in left)
        _COMPOSED[left] = type("HipBackend" + "".join(c.__name__[len("HipBackend"):] for c in bases), bases, {"__doc__": "the opt-in groups " + ", ".join(left)})
    return _COMPOSED[left]


# ------------------------------------------------------------------------------------------------ small helpers
def lin(x, sd, p):
    return F.linear(x, sd[p + "weight"], sd.get(p + "bias"))


def ln(x, sd, p, eps=1e-5):
    return F.layer_norm(x, x.shape[-1:], sd[p + "weight"], sd[p + "bias"], eps)


def mlp(x, sd, p, n):
    """MLP (deformable_transformer_dino.py:599-633): Linear -> ReLU -> ... -> Linear"""
    for i in range(n):
        x = lin(x, sd, "%slayers.%d." % (p, i))
        if i < n - 1:
            x = F.relu(x)
    return x


def conv(x, sd, p, stride=1, padding=0, be=None, relu=False):
    """conv2d (+ ReLU); a backend with a `conv3x3` op is asked first for the 3 x 3 / stride 1 / padding 1 sites, one with a `conv_patch` op
    for the sites without padding whose kernel equals the stride (None: outside its limits)"""
    w, b = sd[p + "weight"], sd.get(p + "bias")
    op = getattr(be, "conv3x3", None) if (stride, padding) == (1, 1) else None
    y = op(x, w, b, relu) if op is not None else None
    if y is None and padding == 0 and tuple(w.shape[2:]) == (stride, stride):
        y = conv_patch(x, w, b, stride, be)
        if relu:
            y = F.relu(y)
        return y
    if y is None:
        y = F.conv2d(x, w, b, stride=stride, padding=padding)
        if relu:
            y = F.relu(y)
    return y


def conv_patch(x, weight, bias, stride, be=None):
    """conv2d whose kernel equals its stride, no padding; a backend with a `conv_patch` op is asked first (None: outside its limits)"""
    op = getattr(be, "conv_patch", None)
    y = op(x, weight, bias, stride) if op is not None else None
    return F.conv2d(x, weight, bias, stride=stride) if y is None else y


def convt2x2(x, weight, bias, be=None):
    """conv_transpose2d 2 x 2 / stride 2; a backend with a `convt2x2` op is asked first (None: outside its limits)"""
    op = getattr(be, "convt2x2", None)
    y = op(x, weight, bias) if op is not None else None
    return F.conv_transpose2d(x, weight, bias, stride=2) if y is None else y


def gn(x, sd, p, groups=32, be=None, relu=False):
    """GroupNorm (+ ReLU) of a conv + GN block; a backend with a `group_norm` op is asked first (None: outside its kernels' limits)"""
    op = getattr(be, "group_norm", None)
    y = op(x, groups, sd[p + "weight"], sd[p + "bias"], 1e-5, relu) if op is not None else None
    if y is None:
        y = F.group_norm(x, groups, sd[p + "weight"], sd[p + "bias"], 1e-5)
        if relu:
            y = F.relu(y)
    return y


def inverse_sigmoid(x, eps=1e-5):
    """util/misc.py:493-497"""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


# ------------------------------------------------------------------------------------------------ ViT backbone (backbone/vit.py, utils.py)
_RESIZE_OPS = {}


def _bicubic_operator(src, dst, device, dtype=torch.float32):
    """(dst, src) matrix of F.interpolate(mode="bicubic", align_corners=False) along one axis, read off the library itself (the identity
    pushed through it), so the border clamping and the A = -0.75 kernel are the library's own"""
    key = (src, dst, str(device), dtype)
    if key not in _RESIZE_OPS:
        eye = torch.eye(src, device=device, dtype=dtype).view(1, src, src, 1)
        _RESIZE_OPS[key] = F.interpolate(eye, size=(dst, 1), mode="bicubic", align_corners=False)[0, :, :, 0].t().contiguous()
    return _RESIZE_OPS[key]


def get_abs_pos(abs_pos, hw):
    """utils.py:128-157 (has_cls_token).  The bicubic resize is linear and separable: it is applied as two small matrix products
    (rows, then columns) with the library's own weights -- the same map as F.interpolate, whose BACKWARD kernel
    (upsample_bicubic2d_backward_out_frame) takes 92 ms per step for this one (1, 1280, 64, 64) tensor on gfx950; as products it is 0.1 ms."""
    h, w = hw
    abs_pos = abs_pos[:, 1:]
    size = int(math.sqrt(abs_pos.shape[1]))
    if size != h or size != w:
        grid = abs_pos.reshape(size, size, -1)
        ah, aw = _bicubic_operator(size, h, abs_pos.device, abs_pos.dtype), _bicubic_operator(size, w, abs_pos.device, abs_pos.dtype)
        rows = torch.matmul(ah, grid.reshape(size, -1)).reshape(h, size, -1)                  # (h, size, C)
        return torch.matmul(aw, rows.permute(1, 0, 2).reshape(size, -1)).reshape(w, h, -1).permute(1, 0, 2)[None]
    return abs_pos.reshape(1, h, w, -1)


def window_partition(x, ws):
    """utils.py:16-38"""
    B, H, W, C = x.shape
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    if ph or pw:
        x = F.pad(x, (0, 0, 0, pw, 0, ph))
    Hp, Wp = H + ph, W + pw
    x = x.view(B, Hp // ws, ws, Wp // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C), (Hp, Wp)


def window_unpartition(win, ws, pad_hw, hw):
    """utils.py:41-60"""
    Hp, Wp = pad_hw
    H, W = hw
    B = win.shape[0] // (Hp * Wp // ws // ws)
    x = win.view(B, Hp // ws, Wp // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, -1)
    return x[:, :H, :W, :].contiguous()


def get_rel_pos(q_size, k_size, rel_pos):
    """utils.py:63-93"""
    n = int(2 * max(q_size, k_size) - 1)
    if rel_pos.shape[0] != n:
        r = F.interpolate(rel_pos.reshape(1, rel_pos.shape[0], -1).permute(0, 2, 1), size=n, mode="linear")
        r = r.reshape(-1, n).permute(1, 0)
    else:
        r = rel_pos
    dev = rel_pos.device
    qc = torch.arange(q_size, device=dev)[:, None] * max(k_size / q_size, 1.0)
    kc = torch.arange(k_size, device=dev)[None, :] * max(q_size / k_size, 1.0)
    rel = (qc - kc) + (k_size - 1) * max(q_size / k_size, 1.0)
    return r[rel.long()]


def _blin(x, sd, p, be):
    """a linear that carries flops: the backend's split-GEMM form when it has one (HipBackend.linear; HipBackendScaledGrads.linear_scaled
    in front of it, HipBackendHalfLinears.linear_half in front of both), else F.linear"""
    f = getattr(be, "linear_half", None) or getattr(be, "linear_scaled", None) or getattr(be, "linear", None)
    return f(x, sd, p) if f is not None else lin(x, sd, p)


def _bmlp(x, sd, p_fc1, p_fc2, act, be):
    """linear -> activation -> linear: the backend's one-node form when it has one (HipBackendMlp.mlp; with it, HipBackendScaledGrads.mlp_scaled
    in front of it, HipBackendHalfLinears.mlp_half in front of both), else the three nodes"""
    f = getattr(be, "mlp", None)
    if f is not None:
        f = getattr(be, "mlp_half", None) or getattr(be, "mlp_scaled", None) or f
        return f(x, sd, p_fc1, p_fc2, act)
    return _blin((F.gelu if act == "gelu" else F.relu)(_blin(x, sd, p_fc1, be)), sd, p_fc2, be)


_KEY_AXES = {}
FOLD_REL_POS = True


def _key_axis_indicators(H, W, device, dtype):
    """(H*W, H + W) constant: row n = key (n // W, n % W) has a one in column n // W and a one in column H + n % W"""
    key = (H, W, str(device), dtype)
    if key not in _KEY_AXES:
        n = torch.arange(H * W, device=device)
        ind = torch.zeros(H * W, H + W, device=device, dtype=dtype)
        ind[n, torch.div(n, W, rounding_mode="floor")] = 1
        ind[n, H + n % W] = 1
        _KEY_AXES[key] = ind
    return _KEY_AXES[key]


def vit_attention(x, sd, p, heads, be=None):
    """Attention.forward (vit.py:67-83) + add_decomposed_rel_pos (utils.py:96-125): the bias is computed from the UNSCALED q.
    The decomposed bias rel_h[q, kh] + rel_w[q, kw] is a product as well -- [rel_h(q, :), rel_w(q, :)] . [onehot(kh), onehot(kw)] -- so it
    rides in the logits' GEMM as H + W extra columns of the operands (q' = [scale q, rel_h, rel_w], k' = [k, indicators]) instead of two
    broadcast additions over the (heads, HW, HW) logits forward and two reductions over their gradient backward (at 64 x 64 tokens: four
    passes over 2 GB per block)."""
    B, H, W, C = x.shape
    hd = C // heads
    qkv = _blin(x, sd, p + "qkv.", be)
    Rh, Rw = get_rel_pos(H, H, sd[p + "rel_pos_h"]), get_rel_pos(W, W, sd[p + "rel_pos_w"])
    packed = getattr(be, "packed_attention", None)
    if packed is not None:
        # HipBackendPackedAttention: everything between the two linears as one node (functions.VitAttentionFunction, csrc/attn_pack.hip)
        o = packed(qkv.reshape(B, H * W, -1), Rh, Rw, heads, H, W)
        if o is not None:
            return _blin(o.view(B, H, W, -1), sd, p + "proj.", be)
    qkv = qkv.reshape(B, H * W, 3, heads, -1).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.reshape(3, B * heads, H * W, -1).unbind(0)
    rq = q.reshape(B * heads, H, W, hd)
    rel_h = torch.einsum("bhwc,hkc->bhwk", rq, Rh).reshape(B * heads, H * W, H)
    rel_w = torch.einsum("bhwc,wkc->bhwk", rq, Rw).reshape(B * heads, H * W, W)
    if FOLD_REL_POS:
        qa = torch.cat((q * hd ** -0.5, rel_h, rel_w), -1)
        ka = torch.cat((k, _key_axis_indicators(H, W, k.device, k.dtype).expand(B * heads, -1, -1)), -1)
        fused, windows = getattr(be, "fused_attention", None), getattr(be, "window_attention", None)
        o = None
        if fused is not None:
            o = fused(qa, ka, v)                      # HipBackend: forward + backward without the (heads, HW, HW) tensors (csrc/attn_train.hip)
        if o is None and windows is not None:
            o = windows(qa, ka, v)                    # HipBackendWindows: the short items fused_attention leaves out (csrc/attn_train_win.hip)
        if o is not None:
            o = o.view(B, heads, H, W, -1).permute(0, 2, 3, 1, 4).reshape(B, H, W, -1)
            return _blin(o, sd, p + "proj.", be)
        attn = qa @ ka.transpose(-2, -1)
    else:
        attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
        attn = (attn.view(B * heads, H, W, H, W) + rel_h.view(B * heads, H, W, H)[:, :, :, :, None]
                + rel_w.view(B * heads, H, W, W)[:, :, :, None, :]).view(B * heads, H * W, H * W)
    o = attn.softmax(dim=-1) @ v
    o = o.view(B, heads, H, W, -1).permute(0, 2, 3, 1, 4).reshape(B, H, W, -1)
    return _blin(o, sd, p + "proj.", be)


def vit_backbone(x, sd, p, cfg, be=None):
    """ViT.forward (vit.py:357-374) + the simple feature pyramid of D2ViT (fpn1 = ConvTranspose, identity, max pool)"""
    # the patch embedding stays on the library: functions.PatchConvFunction takes it (k = 16, frozen input), but its fp32-class difference at
    # the root of the ViT moves the sampling-offsets gradients of the golden step past the checker's bound (HipBackendProjections)
    x = F.conv2d(x, sd[p + "patch_embed.proj.weight"], sd[p + "patch_embed.proj.bias"], stride=cfg["vit_patch"]).permute(0, 2, 3, 1)
    x = x + get_abs_pos(sd[p + "pos_embed"], (x.shape[1], x.shape[2]))
    aln = getattr(be, "add_layer_norm", None)       # HipBackendNorms: every residual add is paired with the LayerNorm that follows it
    pending = None                                  # the mlp branch of the previous block, not yet added to x
    for i in range(cfg["vit_depth"]):
        bp = "%sblocks.%d." % (p, i)
        win = cfg["vit_window"] if i in cfg["vit_window_blocks"] else 0
        if aln is None:
            h = ln(x, sd, bp + "norm1.", 1e-6)
        else:                                     # x + (the previous block's mlp branch) and this norm1 as one node
            x, h = aln(x, pending, sd[bp + "norm1.weight"], sd[bp + "norm1.bias"], 1e-6)
        if win > 0:
            H, W = h.shape[1], h.shape[2]
            h, pad_hw = window_partition(h, win)
        h = vit_attention(h, sd, bp + "attn.", cfg["vit_heads"], be)
        if win > 0:
            h = window_unpartition(h, win, pad_hw, (H, W))
        if aln is None:
            x = x + h
            h = ln(x, sd, bp + "norm2.", 1e-6)
            x = x + _bmlp(h, sd, bp + "mlp.fc1.", bp + "mlp.fc2.", "gelu", be)
        else:
            x, h = aln(x, h, sd[bp + "norm2.weight"], sd[bp + "norm2.bias"], 1e-6)
            pending = _bmlp(h, sd, bp + "mlp.fc1.", bp + "mlp.fc2.", "gelu", be)
            if i == cfg["vit_depth"] - 1:         # no norm follows the last block: a plain add
                x = x + pending
    xp = x.permute(0, 3, 1, 2)
    return {"res3": convt2x2(xp, sd[p + "fpn1.0.weight"], sd[p + "fpn1.0.bias"], be), "res4": xp, "res5": F.max_pool2d(xp, 2, 2)}


# ------------------------------------------------------------------------------------------------ masks, positions
def pos_sine(mask, num_pos_feats=128, offset=-0.5):
    """PositionEmbeddingSine (normalize, T 1e4, scale 2 pi): deformable_detr/position_encoding.py:36-56 (offset -0.5) and
    maskdino/pixel_decoder/position_encoding.py:31-52 (offset 0)"""
    not_mask = ~mask
    y = not_mask.cumsum(1, dtype=torch.float32)
    x = not_mask.cumsum(2, dtype=torch.float32)
    y = (y + offset) / (y[:, -1:, :] + 1e-6) * (2 * math.pi)
    x = (x + offset) / (x[:, :, -1:] + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=mask.device)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    px, py = x[:, :, :, None] / dim_t, y[:, :, :, None] / dim_t
    px = torch.stack((px[:, :, :, 0::2].sin(), px[:, :, :, 1::2].cos()), dim=4).flatten(3)
    py = torch.stack((py[:, :, :, 0::2].sin(), py[:, :, :, 1::2].cos()), dim=4).flatten(3)
    return torch.cat((py, px), dim=3).permute(0, 3, 1, 2)


def down_mask(m, size):
    """MaskedBackbone.forward: nearest resize of the padding mask (masked_backbone.py:21-29)"""
    return F.interpolate(m[None].float(), size=size).to(torch.bool)[0]


def valid_ratio(mask):
    """deformable_transformer_dino.py:170-177"""
    _, H, W = mask.shape
    return torch.stack([torch.sum(~mask[:, 0, :], 1).float() / W, torch.sum(~mask[:, :, 0], 1).float() / H], -1)


def encoder_ref_points(shapes, vr):
    """deformable_transformer_dino.py:313-325"""
    refs = []
    for lvl, (H, W) in enumerate(shapes):
        ry, rx = torch.meshgrid(torch.linspace(0.5, H - 0.5, H, device=vr.device), torch.linspace(0.5, W - 0.5, W, device=vr.device), indexing="ij")
        ry = ry.reshape(-1)[None] / (vr[:, None, lvl, 1] * H)
        rx = rx.reshape(-1)[None] / (vr[:, None, lvl, 0] * W)
        refs.append(torch.stack((rx, ry), -1))
    return torch.cat(refs, 1)[:, :, None] * vr[:, None]


def sine_embed_4(pos):
    """get_sine_pos_embed (deformable_transformer_dino.py:636-670) == gen_sineembed_for_position (maskdino/utils/utils.py:74-100)"""
    dim_t = torch.arange(128, dtype=torch.float32, device=pos.device)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / 128)

    def f(x):
        s = x * (2 * math.pi) / dim_t
        return torch.stack((s[..., 0::2].sin(), s[..., 1::2].cos()), dim=-1).flatten(-2)
    res = [f(pos[..., i:i + 1]) for i in range(pos.shape[-1])]
    res[0], res[1] = res[1], res[0]
    return torch.cat(res, dim=-1)


def agg_lang_feat(hidden, mask):
    """deformable_transformer_dino.py:27-43 (average)"""
    return (hidden * mask.unsqueeze(-1).float()).sum(1) / mask.sum(-1).unsqueeze(-1).float()


def vl_align(x, emb, sd, p):
    """VL_Align.forward (deformable_detr.py:55-73)"""
    emb = F.normalize(emb, p=2, dim=-1)
    tok = lin(emb / 2.0, sd, p + "dot_product_projection_text.")
    bias = torch.matmul(emb, sd[p + "bias_lang"]) + sd[p + "bias0"]
    logit = torch.matmul(x, tok.transpose(-1, -2)) / sd[p + "log_scale"].exp() + bias.unsqueeze(1)
    return logit.clamp(max=50000).clamp(min=-50000)


# ------------------------------------------------------------------------------------------------ deformable attention, encoder / decoder layers
def msda_module(query, ref_points, src, shapes, pad_mask, sd, p, be, heads=8, levels=4, points=4):
    """MSDeformAttn.forward (ops/modules/ms_deform_attn.py:79-116)"""
    N, Lq, C = query.shape
    S = src.shape[1]
    value = lin(src, sd, p + "value_proj.")
    if pad_mask is not None:
        value = value.masked_fill(pad_mask[..., None], 0.0)
    value = value.view(N, S, heads, C // heads)
    off = lin(query, sd, p + "sampling_offsets.").view(N, Lq, heads, levels, points, 2)
    raw = getattr(be, "msda_raw", None)             # HipBackendDeformable: locations, softmax and sampling as one node from the raw projections
    if raw is not None:
        logits = lin(query, sd, p + "attention_weights.").view(N, Lq, heads, levels * points)
        out = raw(value, shapes, ref_points, off, logits)
        if out is not None:
            return lin(out, sd, p + "output_proj.")
        aw = F.softmax(logits, -1).view(N, Lq, heads, levels, points)
    else:
        aw = F.softmax(lin(query, sd, p + "attention_weights.").view(N, Lq, heads, levels * points), -1).view(N, Lq, heads, levels, points)
    if ref_points.shape[-1] == 2:
        loc = ref_points[:, :, None, :, None, :] + off / level_tensors(shapes, query.device, "wh")[None, None, None, :, None, :]
    else:
        loc = ref_points[:, :, None, :, None, :2] + off / points * ref_points[:, :, None, :, None, 2:] * 0.5
    return lin(be.msda(value, shapes, loc, aw), sd, p + "output_proj.")


def encoder_layer(src, pos, refs, shapes, pad_mask, sd, p, be):
    """DeformableTransformerEncoderLayer.forward (deformable_transformer_dino.py:384-394), dropout 0"""
    aln = getattr(be, "add_layer_norm", None)
    if aln is not None:                             # HipBackendNorms: both post-norms with their residual adds, one node each
        _, src = aln(src, msda_module(src + pos, refs, src, shapes, pad_mask, sd, p + "self_attn.", be), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5)
        return aln(src, _bmlp(src, sd, p + "linear1.", p + "linear2.", "relu", be), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5)[1]
    src = ln(src + msda_module(src + pos, refs, src, shapes, pad_mask, sd, p + "self_attn.", be), sd, p + "norm1.")
    return ln(src + _bmlp(src, sd, p + "linear1.", p + "linear2.", "relu", be), sd, p + "norm2.")


def mha(x_qk, x_v, sd, p, attn_mask=None, heads=8, be=None):
    """nn.MultiheadAttention (q = k = tgt + pos, v = tgt), batch first; attn_mask (Nq, Nq) bool, True = blocked.  A backend with a
    `query_attention` op (HipBackendQueryAttention) is asked first, with q | k from ONE linear over in_proj_weight[:2 C] as the inference
    module computes them (None: outside its kernels' limits, the materialised formulation below runs)"""
    B, N, C = x_qk.shape
    w, b = sd[p + "in_proj_weight"], sd[p + "in_proj_bias"]
    hd = C // heads
    op = getattr(be, "query_attention", None)
    if op is not None:
        o = op(F.linear(x_qk, w[:2 * C], b[:2 * C]), F.linear(x_v, w[2 * C:], b[2 * C:]), attn_mask, heads)
        if o is not None:
            return lin(o, sd, p + "out_proj.")

    def sp(t):
        return t.view(B, N, heads, hd).transpose(1, 2)
    q, k, v = sp(F.linear(x_qk, w[:C], b[:C])), sp(F.linear(x_qk, w[C:2 * C], b[C:2 * C])), sp(F.linear(x_v, w[2 * C:], b[2 * C:]))
    a = (q * hd ** -0.5) @ k.transpose(-1, -2)
    if attn_mask is not None:
        a = a.masked_fill(attn_mask[None, None], float("-inf"))
    return lin((a.softmax(-1) @ v).transpose(1, 2).reshape(B, N, C), sd, p + "out_proj.")


def decoder_layer(tgt, qpos, refs_in, src, shapes, pad_mask, sd, p, be, attn_mask=None):
    """DeformableTransformerDecoderLayer.forward (deformable_transformer_dino.py:432-450; maskdino dino_decoder.py:221-270)"""
    tgt = ln(tgt + mha(tgt + qpos, tgt, sd, p + "self_attn.", attn_mask, be=be), sd, p + "norm2.")
    tgt = ln(tgt + msda_module(tgt + qpos, refs_in, src, shapes, pad_mask, sd, p + "cross_attn.", be), sd, p + "norm1.")
    return ln(tgt + lin(F.relu(lin(tgt, sd, p + "linear1.")), sd, p + "linear2."), sd, p + "norm3.")


def gen_proposals(memory, pad_mask, shapes):
    """gen_encoder_output_proposals before enc_output (deformable_transformer_dino.py:138-166; maskdino/utils/utils.py:33-71)"""
    N, dev = memory.shape[0], memory.device
    props, cur = [], 0
    for lvl, (H, W) in enumerate(shapes):
        m = pad_mask[:, cur:cur + H * W].view(N, H, W, 1)
        vH, vW = torch.sum(~m[:, :, 0, 0], 1), torch.sum(~m[:, 0, :, 0], 1)
        gy, gx = torch.meshgrid(torch.linspace(0, H - 1, H, device=dev), torch.linspace(0, W - 1, W, device=dev), indexing="ij")
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.cat([vW.unsqueeze(-1), vH.unsqueeze(-1)], 1).view(N, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(N, -1, -1, -1) + 0.5) / scale
        props.append(torch.cat((grid, torch.ones_like(grid) * 0.05 * (2.0 ** lvl)), -1).view(N, -1, 4))
        cur += H * W
    prop = torch.cat(props, 1)
    valid = ((prop > 0.01) & (prop < 0.99)).all(-1, keepdim=True)
    prop = torch.log(prop / (1 - prop)).masked_fill(pad_mask.unsqueeze(-1), float("inf")).masked_fill(~valid, float("inf"))
    return memory.masked_fill(pad_mask.unsqueeze(-1), 0.0).masked_fill(~valid, 0.0), prop


# ------------------------------------------------------------------------------------------------ vision-language fusion (fuse_helper.py)
def bi_attention_block(v, l, text_mask, sd, p, heads=8, dropout=0.0, be=None):
    """BiAttentionBlockForCheckpoint.forward (fuse_helper.py:170-179) + BiMultiHeadAttention.forward (:54-139).  dropout: the functional
    attention dropout of :111-112 (0.1 in vlfusion.py:81; 0 reproduces the deterministic fixture).  A backend with a `fusion_attention` op
    (HipBackendFusionAttention) is asked first, with the UNSCALED v_proj rows (None: outside its kernels' limits, the materialised
    formulation below runs)"""
    v, l = ln(v, sd, p + "layer_norm_v."), ln(l, sd, p + "layer_norm_l.")
    a = p + "attn."
    B, Nv, _ = v.shape
    L = l.shape[1]
    E = sd[a + "v_proj.weight"].shape[0]
    hd = E // heads
    op = getattr(be, "fusion_attention", None)
    if op is not None:
        o = op(lin(v, sd, a + "v_proj."), lin(l, sd, a + "l_proj."), lin(v, sd, a + "values_v_proj."), lin(l, sd, a + "values_l_proj."), text_mask, heads, dropout)
        if o is not None:
            return v + sd[p + "gamma_v"] * lin(o[0], sd, a + "out_v_proj."), l + sd[p + "gamma_l"] * lin(o[1], sd, a + "out_l_proj.")

    def split(t, n):
        return t.view(B, n, heads, hd).transpose(1, 2).reshape(B * heads, n, hd)
    q = split(lin(v, sd, a + "v_proj.") * hd ** -0.5, Nv)
    k = split(lin(l, sd, a + "l_proj."), L)
    vv, vl = split(lin(v, sd, a + "values_v_proj."), Nv), split(lin(l, sd, a + "values_l_proj."), L)
    w = torch.bmm(q, k.transpose(1, 2)).clamp(min=-50000).clamp(max=50000)
    wT = w.transpose(1, 2)
    wl = (wT - torch.max(wT, dim=-1, keepdim=True)[0]).clamp(min=-50000).clamp(max=50000).softmax(dim=-1)
    am = text_mask.to(torch.int64)[:, None, None, :].expand(B, 1, Nv, L)
    am = am.masked_fill(am == 0, int(-9e15))                  # int64 mask: 0 -> -9e15, 1 stays +1 (fuse_helper.py:97-108)
    wv = F.softmax((w.view(B, heads, Nv, L) + am).view(B * heads, Nv, L), dim=-1)
    if dropout > 0:
        wv, wl = F.dropout(wv, dropout, True), F.dropout(wl, dropout, True)
    ov = torch.bmm(wv, vl).view(B, heads, Nv, hd).transpose(1, 2).reshape(B, Nv, E)
    ol = torch.bmm(wl, vv).view(B, heads, L, hd).transpose(1, 2).reshape(B, L, E)
    return v + sd[p + "gamma_v"] * lin(ov, sd, a + "out_v_proj."), l + sd[p + "gamma_l"] * lin(ol, sd, a + "out_l_proj.")


# ------------------------------------------------------------------------------------------------ the thing branch's transformer
def hipie_transformer(srcs, masks, poses, lang, sd, p, cfg, be, query_label=None, query_bbox=None, attn_mask=None, fusion_dropout=0.0, topk_override=None):
    """DeformableTransformerVLDINO.forward (deformable_transformer_dino.py:180-299): two-stage, mixed selection, DECOUPLE_TGT +
    STILL_TGT_FOR_BOTH, look-forward-twice.  query_label (B, P, 256) / query_bbox (B, P, 4, un-sigmoided) = the de-noising part in front of
    the queries, attn_mask (Nq, Nq) its self-attention mask.  Returns hs (layers, B, Nq, 256), memory, init_ref, inter_refs, the
    proposals' class logits and un-activated boxes (for the encoder loss), the fused language features."""
    shapes = [tuple(s.shape[-2:]) for s in srcs]
    src = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)
    mask = torch.cat([m.flatten(1) for m in masks], 1)
    pos = torch.cat([pe.flatten(2).transpose(1, 2) + sd[p + "level_embed"][i].view(1, 1, -1) for i, pe in enumerate(poses)], 1)
    vr = torch.stack([valid_ratio(m) for m in masks], 1)
    refs = encoder_ref_points(shapes, vr)
    hidden, lmask = lang["hidden"], lang["masks"]
    for i in range(cfg["enc_layers"]):
        if i < cfg["num_vl_layers"]:
            src, hidden = bi_attention_block(src, hidden, lmask, sd, "%sencoder.vl_layers.%d.b_attn." % (p, i), dropout=fusion_dropout, be=be)
        src = encoder_layer(src, pos, refs, shapes, mask, sd, "%sencoder.layers.%d." % (p, i), be)
    memory = src
    lang_pool = agg_lang_feat(hidden, lmask)
    ref_feat = ln(lin(lang_pool, sd, p + "resizer.fc."), sd, p + "resizer.layer_norm.", 1e-12).unsqueeze(1)       # FeatureResizer, dropout 0
    om, prop = gen_proposals(memory, mask, shapes)
    om = ln(lin(om, sd, p + "enc_output."), sd, p + "enc_output_norm.")
    nd = cfg["dec_layers"]
    enc_cls = lin(om, sd, "%sdecoder.class_embed.%d.body." % (p, nd))          # Still_Classifier (STILL_CLS_FOR_ENCODER)
    enc_coord = mlp(om, sd, "%sdecoder.bbox_embed.%d." % (p, nd), 3) + prop
    topk = torch.topk(enc_cls[..., 0], cfg["num_queries"], dim=1)[1] if topk_override is None else topk_override
    ref = torch.gather(enc_coord, 1, topk.unsqueeze(-1).repeat(1, 1, 4)).sigmoid()
    bs = memory.shape[0]
    tgt = sd[p + "tgt_embed.weight"][None].repeat(bs, 1, 1)
    if cfg["num_bg_queries"] > 0:
        tgt = torch.cat([sd[p + "tgt_embed_bg.weight"][None].repeat(bs, 1, 1), tgt], 1)
        ref = torch.cat([sd[p + "bg_query_refs.weight"][None].repeat(bs, 1, 1), ref], 1)
    if query_bbox is not None:
        ref = torch.cat([query_bbox.sigmoid(), ref], 1)
    init_ref = ref
    if query_label is not None:
        tgt = torch.cat([query_label, tgt], 1)
    out = tgt + 0.0 * ref_feat                                                  # decouple_tgt & still_tgt_for_both (:262-266)
    hs, inter = [], []
    for l in range(nd):
        ref_in = ref[:, :, None] * torch.cat([vr, vr], -1)[:, None]
        qpos = mlp(sine_embed_4(ref_in[:, :, 0, :]), sd, p + "decoder.ref_point_head.", 2)
        out = decoder_layer(out, qpos, ref_in, memory, shapes, mask, sd, "%sdecoder.layers.%d." % (p, l), be, attn_mask)
        new_ref = (mlp(out, sd, "%sdecoder.bbox_embed.%d." % (p, l), 3) + inverse_sigmoid(ref)).sigmoid()
        ref = new_ref.detach()                                                  # :505
        hs.append(out)
        inter.append(new_ref)                                                   # look_forward_twice
    return dict(hs=torch.stack(hs), memory=memory, init_ref=init_ref, inter_refs=torch.stack(inter), lang_hidden=hidden, topk=topk, shapes=shapes,
                enc_cls=enc_cls, enc_coord=enc_coord, valid_ratios=vr)


# ------------------------------------------------------------------------------------------------ MaskDINO branch
def maskdino_pixel_decoder(feats, sd, p, cfg, be):
    """MaskDINOEncoder.forward_features (maskdino/pixel_decoder/maskdino_encoder.py:368-434), low2high, masks None"""
    f3, f4, f5 = feats["res3"], feats["res4"], feats["res5"]
    extra = gn(conv(f5, sd, p + "input_proj.3.0.", stride=2, padding=1), sd, p + "input_proj.3.1.", be=be)
    srcs = [gn(conv(f, sd, "%sinput_proj.%d.0." % (p, i), be=be), sd, "%sinput_proj.%d.1." % (p, i), be=be) for i, f in enumerate((f3, f4, f5))] + [extra]
    B, dev = f3.shape[0], f3.device
    zero = [torch.zeros(B, s.shape[2], s.shape[3], dtype=torch.bool, device=dev) for s in srcs]
    poses = [pos_sine(z, 128, offset=0.0) for z in zero]
    shapes = [tuple(s.shape[-2:]) for s in srcs]
    t = p + "transformer."
    src = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)
    pos = torch.cat([pe.flatten(2).transpose(1, 2) + sd[t + "level_embed"][i].view(1, 1, -1) for i, pe in enumerate(poses)], 1)
    mask = torch.cat([z.flatten(1) for z in zero], 1)
    refs = encoder_ref_points(shapes, torch.ones(B, 4, 2, device=dev))
    for i in range(cfg["md_enc_layers"]):
        src = encoder_layer(src, pos, refs, shapes, mask, sd, "%sencoder.layers.%d." % (t, i), be)
    outs, st = [], 0
    for (H, W) in shapes:
        outs.append(src[:, st:st + H * W].transpose(1, 2).reshape(B, -1, H, W))
        st += H * W
    cur = gn(conv_patch(f3, sd[p + "adapter_1.weight"], None, 1, be), sd, p + "adapter_1.norm.", be=be)
    y = cur + F.interpolate(outs[0], size=cur.shape[-2:], mode="bilinear", align_corners=False)
    y = gn(conv(y, sd, p + "layer_1.", padding=1, be=be), sd, p + "layer_1.norm.", be=be, relu=True)       # the ReLU stays with GroupNorm
    mf = gn(convt2x2(y, sd[p + "mask_features.0.weight"], sd[p + "mask_features.0.bias"], be), sd, p + "mask_features.1.", be=be, relu=True)
    return conv(mf, sd, p + "mask_features.3.", be=be), outs


def maskdino_decoder(ms_feats, mask_features, sd, p, cfg, be, dn=None, topk_override=None):
    """MaskDINODecoder.forward in TRAINING mode (maskdino_decoder.py:377-518) + TransformerDecoder.forward (dino_decoder.py:94-168):
    two-stage initialisation from the flattened memory (reversed level order), the proposals' own predictions (interm_outputs), the
    de-noising queries in front (dn = (label queries (B,P,256), boxes (B,P,4) un-sigmoided, self-attention mask) or None), a class / mask /
    box prediction from the initial queries and after every layer.  Returns per-prediction lists (initial + layers) over ALL queries and the
    interm outputs; the caller splits off the de-noising part."""
    nl = len(ms_feats)
    xs = [ms_feats[nl - 1 - i] for i in range(nl)]
    shapes = [tuple(x.shape[-2:]) for x in xs]
    src = torch.cat([x.flatten(2).transpose(1, 2) for x in xs], 1)
    B, dev = src.shape[0], src.device
    mask = torch.zeros(B, src.shape[1], dtype=torch.bool, device=dev)
    vr = torch.ones(B, nl, 2, device=dev)
    om, prop = gen_proposals(src, mask, shapes)
    om = ln(lin(om, sd, p + "enc_output."), sd, p + "enc_output_norm.")
    cls_un = lin(om, sd, p + "class_embed.")
    coord_un = mlp(om, sd, p + "_bbox_embed.", 3) + prop
    nq = cfg["md_num_queries"]
    topk = torch.topk(cls_un.max(-1)[0], nq, dim=1)[1] if topk_override is None else topk_override
    ref_undetach = torch.gather(coord_un, 1, topk.unsqueeze(-1).repeat(1, 1, 4))
    tgt_undetach = torch.gather(om, 1, topk.unsqueeze(-1).repeat(1, 1, om.shape[-1]))

    def heads(x):
        d = ln(x, sd, p + "decoder_norm.")
        einsum = getattr(be, "mask_einsum_scaled", None) or be.mask_einsum       # HipBackendScaledGrads: the same forward, a scaled backward
        return lin(d, sd, p + "class_embed."), einsum(mlp(d, sd, p + "mask_embed.", 3), mask_features)
    ic, im = heads(tgt_undetach)
    interm = {"pred_logits": ic, "pred_boxes": ref_undetach.sigmoid(), "pred_masks": im}
    tgt, ref_un, tgt_mask = tgt_undetach.detach(), ref_undetach.detach(), None
    if dn is not None:
        tgt, ref_un, tgt_mask = torch.cat([dn[0], tgt], 1), torch.cat([dn[1], ref_un], 1), dn[2]
    cls0, m0 = heads(tgt)
    classes, masks_ = [cls0], [m0]
    ref = ref_un.sigmoid()
    refs, out, hs = [ref], tgt, []
    for l in range(cfg["md_dec_layers"]):
        ref_in = ref[:, :, None] * torch.cat([vr, vr], -1)[:, None]
        qpos = mlp(sine_embed_4(ref_in[:, :, 0, :]), sd, p + "decoder.ref_point_head.", 2)
        out = decoder_layer(out, qpos, ref_in, src, shapes, mask, sd, "%sdecoder.layers.%d." % (p, l), be, tgt_mask)
        new_ref = (mlp(out, sd, p + "_bbox_embed.", 3) + inverse_sigmoid(ref)).sigmoid()
        ref = new_ref.detach()
        refs.append(new_ref)
        hs.append(ln(out, sd, p + "decoder.norm."))
    for h in hs:
        c, m = heads(h)
        classes.append(c)
        masks_.append(m)
    boxes = [ref_un.sigmoid()] + [(mlp(h, sd, p + "_bbox_embed.", 3) + inverse_sigmoid(r)).sigmoid() for r, h in zip(refs[:-1], hs)]   # pred_box (:357-375)
    return dict(classes=classes, masks=masks_, boxes=boxes, interm=interm, topk=topk)


# ------------------------------------------------------------------------------------------------ CondInst mask branch
def mask_head_small_conv(feats, sd, p, be=None):
    """MaskHeadSmallConv.forward, fpns None (ddetrs_dn.py:1633-1689); feats = [s8, s16, s32] NCHW"""
    x = conv(feats[-1], sd, p + "lay3.", padding=1, be=be, relu=True)
    x = feats[-2] + F.interpolate(x, size=feats[-2].shape[-2:], mode="nearest")
    x = conv(x, sd, p + "lay4.", padding=1, be=be, relu=True)
    x = feats[-3] + F.interpolate(x, size=feats[-3].shape[-2:], mode="nearest")
    x = conv(x, sd, p + "jia_dcn.", padding=1, be=be, relu=True)
    return conv(conv(x, sd, p + "lay1.", padding=1, be=be, relu=True), sd, p + "lay2.", padding=1, be=be, relu=True)


def backbone_and_projections(x, pad, sd, cfg, be=None):
    """HIPIE_IMG.detr.detr.backbone (MaskedBackbone + Joiner) and input_proj of coco_forward (ddetrs_dn.py:271-320): the three backbone
    levels + the stride-2 extra level whose mask is a resize of the LEVEL-0 mask"""
    p = "detr.detr."
    if cfg.get("backbone", "vit") != "vit":
        raise NotImplementedError("training step: ViT backbones only")
    feats = vit_backbone(x, sd, p + "backbone.0.backbone.", cfg, be)
    names = ["res3", "res4", "res5"]
    fmasks = [down_mask(pad, feats[n].shape[-2:]) for n in names]
    poses = [pos_sine(m, cfg["hidden_dim"] // 2) for m in fmasks]
    srcs = [gn(conv(feats[n], sd, "%sinput_proj.%d.0." % (p, i), be=be), sd, "%sinput_proj.%d.1." % (p, i), be=be) for i, n in enumerate(names)]
    s4 = gn(conv(feats["res5"], sd, p + "input_proj.3.0.", stride=2, padding=1), sd, p + "input_proj.3.1.", be=be)
    m4 = down_mask(fmasks[0], s4.shape[-2:])
    return feats, srcs + [s4], fmasks + [m4], poses + [pos_sine(m4, cfg["hidden_dim"] // 2)]
