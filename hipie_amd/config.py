"""Hyper-parameters of the hot path (the yacs keys the reference reads, flattened) and the precision policy.

``add_hipie_config`` / ``HipieConfig.from_yacs`` map the reference's CfgNode (projects/HIPIE/hipie/config.py:5-284 and
configs/mask_dino/*.yaml) onto this dataclass when detectron2/yacs are installed; without them the presets below are
used (the GPU box has neither).
"""
from dataclasses import asdict, dataclass, field
from typing import List

import torch


@dataclass
class Precision:
    """Arithmetic types of the path.  fp32 accumulate / softmax / LayerNorm everywhere.

    gemm      dtype of the ViT linears (qkv, proj, mlp) -- library GEMMs (hipBLASLt through torch)
    attn      16-bit operand type of the hand-written attention kernels (fp16 or bf16)
    head      dtype of the linears/convs after the backbone (the reference runs them in fp32)
    value     dtype of the MSDeformAttn value tensor (fp32 as the reference, or 16-bit to halve the gather traffic)
    einsum    mask contraction: fp32 features with 0 exact fp32 MFMA, 1 bf16x3, 2 bf16 (hipie_mask_einsum); features in the 16-bit
              activation dtype with 3 one product, 4 query embedding split hi + lo (hipie_mask_einsum16; needs act 16 bit)
    act       storage dtype of the activations between kernels: backbone features, the encoder streams, mask logits (fp32, or
              16 bit to halve the elementwise traffic and drop the cast kernels; statistics of LayerNorm / softmax stay fp32)
    resid     dtype of the ViT residual stream (64 additions deep: fp32 keeps the 16-bit policies inside the tolerance at
              +1.5 % of the step; bf16 only in the bf16 policy)
    attn_fast attention kernels: deferred running max + row sums from the matrix pipe (HIPIE_ATTN_FAST); False = classic
              running max and fp32 sums of the unrounded probabilities
    """
    gemm: torch.dtype = torch.bfloat16
    attn: torch.dtype = torch.bfloat16
    head: torch.dtype = torch.float32
    value: torch.dtype = torch.float32
    einsum: int = 1
    act: torch.dtype = torch.float32
    resid: torch.dtype = torch.float32
    attn_fast: bool = True
    name: str = "default"
    text: torch.dtype = torch.float32      # BERT GEMM / stream dtype (16 bit: fused QKV + hipie_flash_attn + hipie_add_layernorm)
    split: bool = False                    # every linear as hipie_gemm on SPLIT fp16 operands (hi + lo, three MFMA products, fp32
                                           # accumulation = fp32-class results), ViT attention logits likewise (hipie_vit_attn_split)
    vit_attn16: bool = False               # with split: the ViT attention core on single fp16 operands (hipie_vit_attn_rel) -- `mixed`
    fp8x_linears: tuple = ()               # with split: the ViT linear families ("qkv", "proj", "fc1", "fc2") whose product runs with its two
                                           # cross terms on block-scaled e4m3 (hipie_gemm_f8x) -- `fp8x`; wired for "fc2" (Mlp.forward_split)

    @staticmethod
    def parity():
        """closest to the reference's fp32 eval arithmetic: only the attention operands are 16 bit (fp16)."""
        return Precision(torch.float32, torch.float16, torch.float32, torch.float32, 0, torch.float32, torch.float32, False, "parity")

    @staticmethod
    def split3():
        """the TIMED policy: the reference's fp32 arithmetic reproduced on the 16-bit matrix pipe.  Every linear runs as the split-fp16
        GEMM (hipie_gemm, HIPIE_HL8 operands: x.w = x_lo.w_hi + x_hi.w_lo + x_hi.w_hi with fp32 accumulation, ~2^-22 operand error);
        the ViT attention forms its logits AND its P.V product the same way (hipie_vit_attn_split: q, k, P, V are fp16 pairs); BERT and
        the decoders' query self-attention run at fp32-class accuracy on fp16 pairs split in the kernel (hipie_attn_split; round 3: exact fp32 FMA chains, hipie_attn_f32); the image -> text direction of the vision-language fusion
        as batched split GEMMs around a masked softmax (ops.bi_i2t_split), the text -> image direction on fp16 operands with fp32 output;
        streams / norms / softmax / deformable sampling / convolutions fp32 as in the parity policy, the mask contraction as three bf16
        products of split operands.  Measured against the reference's own coco_inference: 1.6e-4 at the headline configuration
        (tests/golden/e2e_full.npz: full ViT-H, 1024 x 1024), 4e-5 on the full-depth narrow fixture.  tests/study/prec_sim.py and
        tools/dec_err_full.py hold the attribution that led here."""
        p = Precision.parity()
        p.split, p.name = True, "split"
        p.einsum = 1          # mask contraction: bf16 x 3 split products (2^-16 relative, hipie_mask_einsum precision 1) instead of the fp32 MFMA
        return p

    @staticmethod
    def mixed():
        """split3 with the ViT attention core on SINGLE fp16 operands (2 MFMA products per tile instead of 6: the global attention is
        a fifth of the split step).  Where it stands (round 4 study): with weights drawn from the reference's OWN
        initialisation (tests/golden/refinit_stats.json, fixture e2e_full_refinit) the a22 outputs stay within 1e-3 at the headline
        configuration; with the harder default synthetic distribution (e2e_full), whose decoder amplifies rounding ~60x more, they do not
        (P as one fp16 alone costs 1e-3 there).  Reported by bench.py beside the headline as `mixed_policy`; NOT the timed policy."""
        p = Precision.split3()
        p.vit_attn16, p.name, p.attn_fast = True, "mixed", True
        return p

    @staticmethod
    def fp8x():
        """split3 with the ViT MLP output (fc2) on hipie_gemm_f8x: W_hi.X_hi on fp16 plus the two cross terms W_lo.X_hi and W_hi.X_lo on e4m3
        operands with a power-of-two scale per 32 k-elements (v_mfma_scale_f32_32x32x64_f8f6f4, twice the fp16 rate): 2 + 2 fp16-equivalent
        MFMA passes per 32 k instead of 6.  Where it stands: the product is 1.1e-5 from fp64 (three fp16 products: 6e-7; tools/fp8_cross_terms.py);
        measured a22 errors (tools/bench_fp8x.py, profiles/fp8x_bench.json): e2e_tiny 5.1e-5, e2e_deep 1.6e-4, e2e_full 6.6e-4, e2e_full_refinit
        2.5e-5, e2e_full_c80 6.5e-4 -- inside the 1e-3 tolerance.  The f8x kernel is not faster than the split one yet (docs/measurements.md).
        Other families may be listed in `fp8x_linears` by a user, but the study (tools/fp8_e2e_study.py, profiles/r06_fp8_cross_terms_study.txt)
        puts them at or over the gate (qkv alone 8.7e-4; proj and fc1 over it; every ViT linear 2.4e-3), and only fc2 is wired to the kernel.
        NOT the timed policy."""
        p = Precision.split3()
        p.fp8x_linears, p.name = ("fc2",), "fp8x"
        return p

    @staticmethod
    def fast():
        """fp16 operands everywhere (same MFMA rate as bf16, 3 more mantissa bits), fp32 accumulation, fp32 ViT residual stream.
        OUTSIDE the north star's 1e-3 tolerance (measured 1e-3 .. 6e-3 on the 3-block fixture, 1.2e-2 at the shipped depths):
        an opt-in throughput mode, not the default and not the headline."""
        return Precision(torch.float16, torch.float16, torch.float16, torch.float16, 4, torch.float16, torch.float32, True, "fast",
                         torch.float16)

    @staticmethod
    def bf16():
        """bf16 operands and streams everywhere (round 1's timed policy): widest range, 8 mantissa bits."""
        return Precision(torch.bfloat16, torch.bfloat16, torch.bfloat16, torch.bfloat16, 3, torch.bfloat16, torch.bfloat16, True, "bf16",
                         torch.bfloat16)


@dataclass
class HipieConfig:
    backbone: str = "vit"                       # "vit" | "r50"
    vit_embed_dim: int = 1280
    vit_depth: int = 32
    vit_heads: int = 16
    vit_window: int = 14
    vit_window_blocks: List[int] = field(default_factory=lambda: [0, 1, 3, 4, 6, 7, 9, 10])   # vit.py:412-421
    vit_img_size: int = 1024
    vit_patch: int = 16
    vit_pretrain_img_size: int = 224
    vit_mlp_ratio: float = 4.0
    hidden_dim: int = 256
    nheads: int = 8
    dim_feedforward: int = 2048
    enc_layers: int = 6
    dec_layers: int = 6
    num_feature_levels: int = 4
    enc_n_points: int = 4
    dec_n_points: int = 4
    num_queries: int = 900
    num_bg_queries: int = 10
    num_vl_layers: int = 1
    vl_hidden_dim: int = 2048
    lang_dim: int = 768
    mask_stride: int = 4
    ctrl_layers: int = 3
    md_num_queries: int = 300
    md_dec_layers: int = 9
    md_enc_layers: int = 6
    md_dim_feedforward: int = 2048
    md_enc_dim_feedforward: int = 2048
    md_mask_dim: int = 256
    md_conv_dim: int = 256
    bert_layers: int = 12
    bert_hidden: int = 768
    bert_heads: int = 12
    bert_intermediate: int = 3072
    bert_vocab: int = 30522
    bert_max_pos: int = 512
    pixel_mean: List[float] = field(default_factory=lambda: [123.675, 116.280, 103.530])
    pixel_std: List[float] = field(default_factory=lambda: [58.395, 57.120, 57.375])
    log_scale: float = 0.0
    prior_prob: float = 0.01
    max_query_len: int = 256                    # MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN (hipie/config.py:84; 4096 / 8192 in the eval yamls)
    pad_max: bool = True                        # MODEL.LANGUAGE_BACKBONE.PAD_MAX (hipie/config.py:88): padding="max_length" else "longest"
    clip_enabled: bool = False                  # MODEL.CLIP.ENABLED: MaskCLIP score fusion (hipie_amd/open_vocab.py; on in 10 / 11 eval yamls)
    clip_name: str = "ViT-L-14-336"             # MODEL.CLIP.NAME (hipie/config.py:153-161)
    clip_alpha: float = 0.35                    # weight of the CLIP probability for classes that overlap the training vocabulary
    clip_beta: float = 0.7                      # ... for novel classes
    clip_fg_a: float = 0.3                      # instance score = sqrt(prob^a * sigmoid(iou)^b)
    clip_fg_b: float = 1.7
    clip_agg_mode: str = "MUL"                  # "MUL": geometric fusion, "ADD": arithmetic
    pano_temp_fg: float = 0.06                  # MODEL.PANO_TEMPERATURE_CLIP_FG (hipie/config.py:222)
    # post-processing (hipie_img.py:60-135: values of hipie/config.py:190-257; the eval yamls override the last three)
    ota: bool = True
    mask_thres: float = 0.5
    transform_eval: bool = True
    pano_temp: float = 0.06
    overlap_threshold: float = 0.8
    object_mask_threshold: float = 0.25
    mode_free: bool = False
    nms_thresh: float = 0.7                     # hipie_img.py:629 (literal)
    use_bg_for_pano: bool = True
    bg_cls_agnostic: bool = False
    max_pool: bool = False

    # ---- presets -------------------------------------------------------------------------------------------
    @staticmethod
    def vit_huge():
        """configs/eval/image_joint_vit_huge_32g_pan_maskdino_ade_test.yaml (ViT-huge: vit.py:392-396)."""
        return HipieConfig()

    @staticmethod
    def vit_base():
        return HipieConfig(vit_embed_dim=768, vit_depth=12, vit_heads=12)

    @staticmethod
    def vit_large():
        return HipieConfig(vit_embed_dim=1024, vit_depth=24, vit_heads=16)

    @staticmethod
    def r50():
        """configs/eval/image_joint_r50_pan_maskdino_ade_test.yaml."""
        return HipieConfig(backbone="r50")

    @staticmethod
    def from_dict(d):
        names = set(HipieConfig.__dataclass_fields__)
        return HipieConfig(**{k: v for k, v in d.items() if k in names})

    def to_dict(self):
        return asdict(self)

    @property
    def backbone_channels(self):
        if self.backbone == "r50":
            return [512, 1024, 2048]
        e = self.vit_embed_dim
        return [e // 2, e, e]

    @staticmethod
    def from_yacs(cfg, md_cfg=None):
        """reference CfgNode (after add_hipie_config + yaml merge) -> HipieConfig."""
        m = cfg.MODEL
        c = HipieConfig()
        # the eval path built here is the one every shipped eval yaml selects; any other switch position would silently
        # compute something else, so it is refused (hipie/config.py:12-217 for the keys)
        required = [("MODEL.PARALLEL_DET", m.PARALLEL_DET, False), ("MODEL.DECOUPLE_TGT", m.DECOUPLE_TGT, True),
                    ("MODEL.STILL_TGT_FOR_BOTH", m.STILL_TGT_FOR_BOTH, True), ("MODEL.USE_IOU_BRANCH", m.USE_IOU_BRANCH, True),
                    ("MODEL.STILL_CLS_FOR_ENCODER", m.STILL_CLS_FOR_ENCODER, True), ("MODEL.LANG_GUIDE_DET", m.LANG_GUIDE_DET, True),
                    ("MODEL.DDETRS.USE_DINO", m.DDETRS.USE_DINO, True), ("MODEL.DDETRS.TWO_STAGE", m.DDETRS.TWO_STAGE, True),
                    ("MODEL.DDETRS.MIXED_SELECTION", m.DDETRS.MIXED_SELECTION, True),
                    ("MODEL.DDETRS.LOOK_FORWARD_TWICE", m.DDETRS.LOOK_FORWARD_TWICE, True),
                    ("MODEL.DDETRS.BG_QUERY_FROM_LANG", m.DDETRS.BG_QUERY_FROM_LANG, False),
                    ("MODEL.DDETRS.NEW_MASK_HEAD", m.DDETRS.NEW_MASK_HEAD, False), ("MODEL.DDETRS.USE_RAFT", m.DDETRS.USE_RAFT, False),
                    ("MODEL.DDETRS.USE_REL_COORD", m.DDETRS.USE_REL_COORD, True), ("MODEL.CLIP.ENABLED_TRAIN", m.CLIP.ENABLED_TRAIN, False),
                    # the decoupled MaskDINO branch with its own class heads (ddetrs_dn.py:172-215) and the mask outputs (hipie_img.py:59)
                    ("MODEL.MASK_ON", m.MASK_ON, True), ("MODEL.MASKDINO.ENABLED", m.MASKDINO.ENABLED, True),
                    ("MODEL.MASKDINO.SHARE_CLS_HEAD", m.MASKDINO.SHARE_CLS_HEAD, False),
                    ("MODEL.MASKDINO.FIXED_LINEAR_HEAD", m.MASKDINO.FIXED_LINEAR_HEAD, False)]
        if m.BACKBONE.NAME != "D2ViT":           # the R50 of the shipped yamls: depth 50, stride in the 3x3 (resnet.py of this package)
            required += [("MODEL.RESNETS.STRIDE_IN_1X1", m.RESNETS.STRIDE_IN_1X1, False), ("MODEL.RESNETS.DEPTH == 50", m.RESNETS.DEPTH == 50, True)]
        bad = ["%s=%r (supported: %r)" % (k, v, want) for k, v, want in required if bool(v) != want]
        if bad:
            raise NotImplementedError("hipie_amd builds the shipped eval configuration only; unsupported: " + "; ".join(bad))
        c.max_query_len, c.pad_max = int(m.LANGUAGE_BACKBONE.MAX_QUERY_LEN), bool(m.LANGUAGE_BACKBONE.PAD_MAX)
        c.clip_enabled, c.clip_name = bool(m.CLIP.ENABLED), str(m.CLIP.NAME)
        c.clip_alpha, c.clip_beta, c.clip_agg_mode = float(m.CLIP.ALPHA), float(m.CLIP.BETA), str(m.CLIP.AGG_MODE)
        c.clip_fg_a, c.clip_fg_b = float(m.CLIP.FG_IOU_A), float(m.CLIP.FG_IOU_B)
        c.pano_temp_fg = float(m.PANO_TEMPERATURE_CLIP_FG)
        if m.BACKBONE.NAME == "D2ViT":
            geo = {"ViT-Base": (768, 12, 12), "ViT-Large": (1024, 24, 16), "ViT-huge": (1280, 32, 16)}[m.VIT.NAME]
            c.backbone, (c.vit_embed_dim, c.vit_depth, c.vit_heads) = "vit", geo
        else:
            c.backbone = "r50"
        d = m.DDETRS
        c.hidden_dim, c.nheads, c.dim_feedforward = d.HIDDEN_DIM, d.NHEADS, d.DIM_FEEDFORWARD
        c.enc_layers, c.dec_layers, c.num_feature_levels = d.ENC_LAYERS, d.DEC_LAYERS, d.NUM_FEATURE_LEVELS
        c.enc_n_points, c.dec_n_points = d.ENC_N_POINTS, d.DEC_N_POINTS
        c.num_queries, c.num_bg_queries = d.TWO_STAGE_NUM_PROPOSALS, d.TWO_STAGE_NUM_BG_PROPOSALS
        c.num_vl_layers, c.vl_hidden_dim = d.NUM_VL_LAYERS, d.VL_HIDDEN_DIM
        c.mask_stride, c.ctrl_layers = d.MASK_STRIDE, d.CTRL_LAYERS
        c.lang_dim = m.LANGUAGE_BACKBONE.LANG_DIM
        c.pixel_mean, c.pixel_std = list(m.PIXEL_MEAN), list(m.PIXEL_STD)
        c.log_scale, c.prior_prob = m.DYHEAD.LOG_SCALE, m.DYHEAD.PRIOR_PROB
        c.ota, c.mask_thres, c.mode_free = m.OTA, d.MASK_THRES, m.MODE_FREE_MATCHING_INFERENCE
        c.transform_eval, c.pano_temp = m.PANO_TRANSFORM_EVAL, m.PANO_TEMPERATURE
        c.overlap_threshold, c.object_mask_threshold = m.OVERLAP_THRESHOLD, m.OBJECT_MASK_THRESHOLD
        c.use_bg_for_pano, c.bg_cls_agnostic, c.max_pool = cfg.TEST.USE_BG_FOR_PANO_ON, cfg.TEST.BG_CLS_AGNOSTIC, cfg.TEST.MAX_POOL
        if md_cfg is not None:
            md, sh = md_cfg.MODEL.MaskDINO, md_cfg.MODEL.SEM_SEG_HEAD
            c.md_num_queries, c.md_dec_layers, c.md_dim_feedforward = md.NUM_OBJECT_QUERIES, md.DEC_LAYERS, md.DIM_FEEDFORWARD
            c.md_enc_layers, c.md_enc_dim_feedforward = sh.TRANSFORMER_ENC_LAYERS, sh.DIM_FEEDFORWARD
            c.md_mask_dim, c.md_conv_dim = sh.MASK_DIM, sh.CONVS_DIM
        return c
