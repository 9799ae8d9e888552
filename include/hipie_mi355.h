/*
 * hipie_mi355.h -- C ABI of libhipie_mi355.so: the hand-written HIP (gfx950 / CDNA4) kernels of HIPIE's
 * single-image inference hot path.
 *
 * Conventions:
 *   - plain C, no exceptions, no torch types; every pointer is a DEVICE pointer unless it says "host";
 *   - the caller owns all buffers (inputs are borrowed, outputs are pre-allocated), nothing is allocated here;
 *   - every entry point takes the hipStream_t to launch on (as void*) and returns 0 on success or a negative
 *     HIPIE_E* code; hipie_last_error() gives the text for the calling thread;
 *   - stateless and thread-safe; launches are asynchronous (no sync inside), so they can be captured in hipGraphs;
 *   - tensors are dense row-major with the last index fastest unless explicit strides are given.
 *
 * Each function names the reference interface it replaces (paths relative to projects/HIPIE/hipie/).
 */
#ifndef HIPIE_MI355_H
#define HIPIE_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPIE_ABI_VERSION 13

/* element types of activations */
#define HIPIE_F32 0
#define HIPIE_F16 1
#define HIPIE_BF16 2
#define HIPIE_F64 3          /* hipie_msda_forward only (the reference op dispatches float | double) */
#define HIPIE_HL8 4          /* SPLIT fp16 ("hi + lo in groups of 8"): a logical row of K values is stored as K/8 groups of 32 bytes,
                                8 fp16 hi[0..7] then 8 fp16 lo[0..7], with hi = fp16(x), lo = fp16(x - hi): hi + lo == x to 2^-22.
                                Same bytes as fp32; the operand format of the fp32-class products on the 16-bit matrix pipe
                                (hipie_gemm, hipie_vit_attn_rel with HIPIE_ATTN_SPLIT).  Row strides are given in fp16 elements (>= 2K). */

#define HIPIE_OUT_F32 0x100   /* or-ed into the `dtype` of hipie_flash_attn / hipie_bi_xattn(_ws): q, k, v stay 16 bit, the OUTPUT(S) are written as
                                fp32 (output strides in fp32 elements): the attention result enters the next linear unrounded */
#define HIPIE_K_HL8_HI 0x200  /* or-ed into the `dtype` of hipie_flash_attn: `k` points at an HIPIE_HL8 buffer and the keys are its `hi` halves (hi = fp16(x)
                                by construction): the 8-element chunks of a head row are 16 elements apart; k_sb / k_st / k_sh are strides of
                                the HL8 buffer in fp16 elements (k_sh = 2 * head_dim).  Saves the strided copy that extracts them. */

/* flags of the attention entry points that take a `flags` argument */
#define HIPIE_ATTN_FAST 1    /* deferred running max (rescale only when a row maximum grows by > 2^8) and, where the head dim
                                leaves a padded MFMA row, softmax denominators from a ones column of V (same 16-bit-rounded
                                probabilities as the numerator).  Without it: classic running max, fp32 sums of the
                                unrounded probabilities (the parity policy). */

/* error codes */
#define HIPIE_OK 0
#define HIPIE_EINVAL (-22)   /* bad shape / dtype / null pointer / unsupported geometry */
#define HIPIE_ELAUNCH (-5)   /* hipLaunchKernel failed (hipie_last_error() has hipGetErrorString) */

int hipie_version(void);
/* text of the last error raised on the calling thread ("" when none). */
const char* hipie_last_error(void);

/*
 * Multi-scale deformable attention sampling, forward.
 * Replaces: MultiScaleDeformableAttention.ms_deform_attn_forward (pybind, models/deformable_detr/ops/src/vision.cpp:13-16)
 *           = ms_deform_attn_cuda_forward (ops/src/cuda/ms_deform_attn_cuda.cu:20-80)
 *           -> ms_deformable_im2col_gpu_kernel (ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299),
 *           and the identical copy under models/maskdino/pixel_decoder/ops/.
 *   value          (B, S, M, D)        dtype `value_dtype` (f32 as the reference; f16/bf16 halve the gather traffic; f64: the
 *                                      reference's double instantiation -- then sampling_loc, attn_weight and out are f64 too)
 *   spatial_shapes (L, 2) int64 (H, W) device
 *   level_start    (L,)   int64        device
 *   sampling_loc   (B, Lq, M, L, P, 2) f32 (f64 with an f64 value), (x, y) normalised to [0,1] (values outside sample zero padding)
 *   attn_weight    (B, Lq, M, L, P)    f32 (f64 with an f64 value)
 *   out            (B, Lq, M*D)        dtype `value_dtype`; fully overwritten (the reference at::zeros + writes all)
 * im2col_step of the reference is a batching detail of its host loop and has no equivalent here.
 */
int hipie_msda_forward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start,
                       const void* sampling_loc, const void* attn_weight, void* out,
                       int B, int S, int M, int D, int L, int Lq, int P, int value_dtype, void* stream);

/*
 * Backward of the operator above -- the plugin's second entry point.
 * Replaces: ms_deform_attn_backward of the `MultiScaleDeformableAttention` extension (ops/src/vision.cpp:13-16; called by
 *           MSDeformAttnFunction.backward, ops/functions/ms_deform_attn_func.py:32-41)
 *           = ms_deform_attn_cuda_backward (ops/src/cuda/ms_deform_attn_cuda.cu:83-153)
 *           -> ms_deformable_col2im_gpu_kernel_* (ops/src/cuda/ms_deform_im2col_cuda.cuh:301-1320).  Training only.
 *   value, spatial_shapes, level_start, sampling_loc, attn_weight: as hipie_msda_forward;  dtype HIPIE_F32 | HIPIE_F64 for all
 *   grad_output       (B, Lq, M*D)
 *   grad_value        (B, S, M, D)         zeroed here, then accumulated with hardware atomics (arrival order, as the reference)
 *   grad_sampling_loc (B, Lq, M, L, P, 2)  fully written, deterministic
 *   grad_attn_weight  (B, Lq, M, L, P)     fully written, deterministic
 */
int hipie_msda_backward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const void* sampling_loc,
                        const void* attn_weight, const void* grad_output, void* grad_value, void* grad_sampling_loc,
                        void* grad_attn_weight, int B, int S, int M, int D, int L, int Lq, int P, int dtype, void* stream);

/*
 * The same operator with a caller-provided workspace: for fp32 and D = 32 (every MSDA of the model) grad_value is computed from the
 * destination side -- sampling corners are binned by (pixel, head) with integer atomics, then every destination sums its own list in
 * registers and is written once -- instead of B*Lq*M*L*P*4*D floating-point atomics (which bound the form above: ~460 G adds/s).
 * Other dtypes / widths run the kernel above (the workspace is ignored).  Same arguments and results; grad_value needs no zeroing and
 * is summed in slot (arrival) order.  workspace: at least hipie_msda_backward_workspace(...) bytes, 16-byte aligned, contents
 * irrelevant before and after.  Replaces the same reference entry as hipie_msda_backward (ms_deform_attn_cuda.cu:83-153).
 */
int64_t hipie_msda_backward_workspace(int B, int S, int M, int L, int Lq, int P);
int hipie_msda_backward_ws(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const void* sampling_loc,
                           const void* attn_weight, const void* grad_output, void* grad_value, void* grad_sampling_loc,
                           void* grad_attn_weight, int B, int S, int M, int D, int L, int Lq, int P, int dtype, void* workspace,
                           int64_t workspace_bytes, void* stream);

/*
 * Fused form used by the product path: sampling locations and the 16-way softmax are computed in the kernel from
 * the raw projections, so neither (B,Lq,M,L,P,2) locations nor normalised weights ever reach HBM.
 * Replaces: MSDeformAttn.forward lines 99-114 (ops/modules/ms_deform_attn.py) + the op above.
 *   offsets: row (b,q) at offsets + (b*Lq+q)*off_row_stride holds (M, L, P, 2) = sampling_offsets(query)
 *   logits:  row (b,q) at logits  + (b*Lq+q)*logit_row_stride holds (M, L*P) = attention_weights(query)
 *            (both `aux_dtype` f32|f16|bf16; the strides let one concatenated projection GEMM feed both)
 *   ref     (B, Lq, L, ref_dim) f32, ref_dim 2: loc = ref + off/(W_l,H_l); ref_dim 4: loc = ref_xy + off/P*ref_wh*0.5
 */
int hipie_msda_fused_forward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start,
                             const float* ref, const void* offsets, const void* logits, void* out,
                             int B, int S, int M, int D, int L, int Lq, int P, int ref_dim, int value_dtype,
                             int aux_dtype, int64_t off_row_stride, int64_t logit_row_stride, void* stream);

/*
 * hipie_msda_fused_forward on a value tensor whose pixel rows are `value_row_stride` elements apart (>= M*D, a multiple of 8):
 * the value projections of all decoder layers read the same memory, so they run as ONE GEMM on the concatenated weights
 * (deformable_transformer_dino.py:418-450, one value_proj per layer) and every layer samples its own column block in place.
 */
int hipie_msda_fused_forward_strided(const void* value, int64_t value_row_stride, const int64_t* spatial_shapes,
                                     const int64_t* level_start, const float* ref, const void* offsets, const void* logits,
                                     void* out, int B, int S, int M, int D, int L, int Lq, int P, int ref_dim, int value_dtype,
                                     int aux_dtype, int64_t off_row_stride, int64_t logit_row_stride, void* stream);

/*
 * Backward of hipie_msda_fused_forward for fp32 and D = 32 (training only): the gather form of hipie_msda_backward_ws with the location and the
 * softmax recomputed in its count, fill and coefficient kernels from (ref, offsets, logits), and the chain rule through both applied in
 * the coefficient kernel -- no (B,Lq,M,L,P,.) tensor other than the two gradient outputs and the corner records reaches HBM.
 * Replaces: the autograd chain of MSDeformAttn.forward lines 99-114 (ops/modules/ms_deform_attn.py) + MSDeformAttnFunction.backward.
 *   value, spatial_shapes, level_start, ref, offsets, logits, the two input row strides: as hipie_msda_fused_forward, all fp32, value dense
 *   grad_output  (B, Lq, M*D)
 *   grad_value   (B, S, M, D)   every row written (no zeroing needed; rows no level covers are zero), summed in slot (arrival) order
 *   grad_offsets row (b,q) at grad_offsets + (b*Lq+q)*goff_row_stride holds (M, L, P, 2):  ref_dim 2: gloc / (W_l, H_l);
 *                ref_dim 4: gloc * ref_wh * 0.5 / P          (gloc, gA, A: grad_sampling_loc, grad_attn_weight, softmax(logits))
 *   grad_logits  row (b,q) at grad_logits + (b*Lq+q)*glogit_row_stride holds (M, L*P):  A_i (gA_i - sum_j A_j gA_j)
 *                (the two output strides let both be column blocks of one (B, Lq, k) buffer)
 *   grad_ref     (B, Lq, L, ref_dim) or NULL:  xy: sum_{m,p} gloc;  wh (ref_dim 4): sum_{m,p} gloc * off * 0.5 / P -- per-head partials in
 *                the workspace, added in head order
 * grad_offsets, grad_logits and grad_ref are bit-reproducible (no floating-point atomics anywhere).  workspace: at least
 * hipie_msda_raw_backward_ws_bytes(..., grad_ref != NULL) bytes, 16-byte aligned: the gather form's bins and corner records, the softmax's
 * (max, 1 / sum) per (b, q, head) -- computed once, by the count pass -- and, with grad_ref, its per-head partials.  Refused (HIPIE_EINVAL, nothing launched): D != 32, S above
 * the 40960 pixel rows whose counters fit the LDS, L*P > 32, ref_dim not 2 | 4, a row stride below the row's width, null pointers, a
 * workspace that is too small (the message names the size needed).  The size query answers 0 for shapes the entry refuses.
 */
int64_t hipie_msda_raw_backward_ws_bytes(int B, int S, int M, int L, int Lq, int P, int ref_dim, int want_grad_ref);
int hipie_msda_raw_backward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const float* ref,
                            const void* offsets, const void* logits, const void* grad_output, void* grad_value, void* grad_offsets,
                            void* grad_logits, void* grad_ref, int B, int S, int M, int D, int L, int Lq, int P, int ref_dim,
                            int64_t off_row_stride, int64_t logit_row_stride, int64_t goff_row_stride, int64_t glogit_row_stride,
                            void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Fused (flash-style) attention core shared by the ViT blocks and the VL fusion:
 *     out[b,i,h,:] = softmax_j( clamp(scale * q[b,i,h,:].k[b,j,h,:], +-clamp) + bias_h[bh,j / kw,i] + bias_w[bh,i,j % kw]
 *                               + (key_mask[b,j] ? 0 : -inf) ) . v[b,j,h,:]
 * with fp32 scores / softmax / accumulation, 16-bit MFMA operands, nothing of size Nq x Nk in HBM.
 * A query with no attended key (key_mask all zero for its batch item) gives zeros, as in hipie_attn_f32 / hipie_attn_split.
 * q,k,v,out are addressed with explicit element strides (batch, token, head); head_dim contiguous.
 *   dtype      HIPIE_F16 or HIPIE_BF16 (q, k, v, out)
 *   head_dim   80 (ViT-H), 64 (ViT-B/L), 256 (VL fusion), 32
 *   bias_h     (B*H, kh, Nq) f32 (key-row major: one coalesced line per key row) or NULL;  bias_w (B*H, Nq, kw) f32 or
 *              NULL  (both or none; needs Nk == kh*kw)
 *   key_mask   (B, Nk) uint8 (1 = keep) or NULL
 *   clamp      <= 0 disables the clamp
 * Replaces: Attention.forward's (q*scale)@k^T -> add_decomposed_rel_pos -> softmax -> @v (backbone/vit.py:72-80,
 *           backbone/utils.py:96-125) and the two softmax(QK^T)V products of BiMultiHeadAttention.forward
 *           (models/deformable_detr/fuse_helper.py:69-121).
 */
int hipie_flash_attn(const void* q, const void* k, const void* v, void* out,
                     int B, int H, int Nq, int Nk, int head_dim,
                     int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                     int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                     const float* bias_h, const float* bias_w, int kh, int kw,
                     const uint8_t* key_mask, float scale, float clamp, int dtype, void* stream);

/*
 * ViT attention with decomposed relative position bias on a packed qkv tensor.
 * Replaces: Attention.forward between the qkv and proj Linears (backbone/vit.py:69-80) for both the 14x14 windowed
 * blocks (x already window-partitioned, B = batch*windows, gh=gw=14) and the global blocks (gh x gw token grid).
 *   qkv    (B, gh*gw, 3, heads, hd) 16-bit;  rel_h (B*heads, gh, gh*gw) f32 = q.Rh[hq,hk] (key row major);
 *          rel_w (B*heads, gh*gw, gw) f32 = q.Rw[wq,wk]
 *   out    (B, gh*gw, heads*hd) 16-bit
 */
int hipie_vit_attn(const void* qkv, const float* rel_h, const float* rel_w, void* out,
                   int B, int gh, int gw, int heads, int hd, float scale, int dtype, void* stream);

/*
 * Bi-directional text<->vision cross attention core of the VL early-fusion block.
 * Replaces: BiMultiHeadAttention.forward lines 69-121 (models/deformable_detr/fuse_helper.py), i.e. everything between
 * the four input projections and the two output projections; clamp +-50000, text key mask, no mask on the image side.
 *   q (B,Nv,H,hd) = v_proj(v)*scale, k (B,L,H,hd) = l_proj(l), vv (B,Nv,H,hd), vl (B,L,H,hd): 16-bit
 *   text_mask (B,L) uint8;  out_v (B,Nv,H*hd), out_l (B,L,H*hd) 16-bit
 */
int hipie_bi_xattn(const void* q, const void* k, const void* vv, const void* vl, const uint8_t* text_mask,
                   void* out_v, void* out_l, int B, int H, int Nv, int L, int hd, float clamp, int dtype, void* stream);

/*
 * hipie_bi_xattn with a caller-provided workspace (the library never allocates).  For one short text per image
 * (64 < L <= 224, head dim 256: the class captions of the detection task) both directions run specialised kernels: image -> text
 * as one softmax window over the resident text, text -> image with the text block in registers and the image range split over
 * workgroups, whose partial (max, sum, accumulator) triples live in `workspace` until a combine kernel reduces them.
 * hipie_bi_xattn_workspace returns the bytes needed (0: the shape takes the generic kernel and needs none); a null / short
 * workspace is not an error -- the text -> image direction then runs the generic kernel.
 */
int64_t hipie_bi_xattn_workspace(int B, int H, int Nv, int L, int head_dim);
int hipie_bi_xattn_ws(const void* q, const void* k, const void* vv, const void* vl, const uint8_t* text_mask,
                      void* out_v, void* out_l, void* workspace, int64_t workspace_bytes, int B, int H, int Nv, int L,
                      int head_dim, float clamp, int dtype, void* stream);

/*
 * Mask-logit contraction  out[b,q,p] = sum_c embed[b,q,c] * feats[b,c,p].
 * Replaces: torch.einsum("bqc,bchw->bqhw") in MaskDINODecoder.forward_prediction_heads
 *           (models/maskdino/transformer_decoder/maskdino_decoder.py:520-529).
 *   embed (B,Q,C) f32, feats (B,C,HW) f32, out (B,Q,HW) `out_dtype` (f32 | f16 | bf16).
 *   precision 0: exact fp32 (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain); 1: bf16x3 split (3 bf16 MFMAs per
 *   product, ~2^-16 relative); 2: single bf16 MFMA.   C % 16 == 0.
 */
int hipie_mask_einsum(const float* embed, const float* feats, void* out, int B, int Q, int C, int HW,
                      int precision, int out_dtype, void* stream);

/*
 * The same contraction with a caller-provided workspace, plus a per-row constant:
 *   out[b,q,p] = row_bias[b,q] + sum_c embed[b,q,c] * feats[b,c,p],   row_bias (B,Q) f32 or NULL, precision 1 or 2.
 * The embedding is split ONCE per call into the workspace (bf16 hi + lo parts in the layout of the kernel's LDS tile) and staged
 * by LDS-DMA, instead of being split by every workgroup (hipie_mask_einsum): the faster form.  hipie_mask_einsum_workspace
 * returns the bytes needed; the workspace is scratch (nothing is kept between calls), 16-byte aligned.
 * With embed' = embed . W and row_bias = embed . b the last 1x1 convolution of the pixel decoder's mask_features head
 * (Conv2d(256,256,1), maskdino_encoder.py:283-300) folds into the contraction of maskdino_decoder.py:527: the (B,256,H/4,W/4)
 * map is neither convolved nor written a second time.
 */
int64_t hipie_mask_einsum_workspace(int B, int Q, int C);
int hipie_mask_einsum_ws(const float* embed, const float* feats, const float* row_bias, void* out, void* workspace,
                         int64_t workspace_bytes, int B, int Q, int C, int HW, int precision, int out_dtype, void* stream);

/*
 * The same contraction on 16-bit features (the activation dtype of the 16-bit policies): out[b,q,p] = sum_c embed[b,q,c] *
 * feats[b,c,p] with feats (B,C,HW) `dtype` (f16 | bf16), the query embedding pre-split by the caller into embed_hi + embed_lo
 * (both (B,Q,C) `dtype`; embed_lo NULL: single product), out (B,Q,HW) `out_dtype` (= dtype, or f32).  fp32 accumulation.
 * row_bias (B,Q) f32 or NULL is added to every pixel of a query row: with embed' = embed . W and row_bias = embed . b the last
 * 1x1 convolution of the pixel decoder's mask_features head (maskdino_encoder.py:283-300) folds into this contraction.
 * Replaces the same torch.einsum (maskdino_decoder.py:527).  Q <= 320, C % 16 == 0, HW % 8 == 0 (HW even for f32 output).
 */
int hipie_mask_einsum16(const void* embed_hi, const void* embed_lo, const void* feats, const float* row_bias, void* out, int B,
                        int Q, int C, int HW, int dtype, int out_dtype, void* stream);

/*
 * Fused CondInst dynamic mask head: relative-coordinate generation + per-instance 10->8->8->1 MLP (ReLU, ReLU, none)
 * + aligned_bilinear x`up`, without materialising the (1, N*10, H, W) input or running a grouped conv.
 * Replaces: DDETRSegmUniDN.dynamic_mask_with_coords (models/ddetrs_dn.py:1411-1502) incl. compute_locations (:1857),
 *           parse_dynamic_params (:1806), mask_heads_forward (:1390) and aligned_bilinear (:1832).
 *   feats (B,8,H,W) f32;  refs (B*Q,2) f32 pixels (x,y);  params (B*Q,169) f32 = [w0 8x10 | w1 8x8 | w2 1x8 | b0 8 | b1 8 | b2 1]
 *   out (B*Q, up*H, up*W) `out_dtype`;  instance n uses feats[n / Q];  up in {1,2};  stride = mask feature stride (8)
 */
int hipie_dynamic_mask(const float* feats, const float* refs, const float* params, void* out,
                       int B, int Q, int H, int W, int stride, int up, int out_dtype, void* stream);

/*
 * Backward of hipie_dynamic_mask (fp32, up in {1,2}): gradients of a scalar loss with respect to the mask features, the reference
 * points and the 169 controller parameters per instance, given grad_out (B*Q, up*H, up*W) f32 = d loss / d out.
 * Replaces: torch.autograd through DDETRSegmUniDN.dynamic_mask_with_coords / mask_heads_forward / aligned_bilinear
 *           (models/ddetrs_dn.py:1411-1502, 1390-1408, 1832-1854) in the training forward (coco_forward, :264-750).
 *   grad_feats (B,8,H,W), grad_refs (B*Q,2), grad_params (B*Q,169) f32, overwritten (zeroed here, then accumulated: fp32 atomics, so the
 *   sums over pixels / instances run in arrival order like the reference's cuDNN / atomics-based conv backward).
 *   Ragged instance counts per image (the matched instances of training): one call per image with B = 1.
 */
int hipie_dynamic_mask_backward(const float* feats, const float* refs, const float* params, const float* grad_out, float* grad_feats,
                                float* grad_refs, float* grad_params, int B, int Q, int H, int W, int stride, int up, void* stream);

/*
 * hipie_dynamic_mask (up = 2) with the three layers on the matrix pipe: 16-bit operands (`dtype` f16 / bf16: the features,
 * the layer weights and the hidden activations are rounded to it; the coordinate weights are split hi + lo), fp32 accumulate,
 * fp32 biases and reference-point terms.  Same replaced reference code and argument meaning as hipie_dynamic_mask.
 * W % 4 == 0, stride % 4 == 0, stride * max(H, W) <= 8192 (pixel coordinates exact in 16 bit); else HIPIE_EINVAL.
 */
int hipie_dynamic_mask16(const float* feats, const float* refs, const float* params, void* out,
                         int B, int Q, int H, int W, int stride, int dtype, int out_dtype, void* stream);

/*
 * Decomposed relative-position bias tables of one ViT block, straight from the packed 16-bit qkv tensor.
 * Replaces: add_decomposed_rel_pos's two einsums + get_rel_pos gathers (backbone/utils.py:63-125) feeding hipie_vit_attn.
 *   qkv (B, gh*gw, 3, heads, hd) 16-bit;  tab_h (2*gh-1, hd), tab_w (2*gw-1, hd) 16-bit = rel_pos_h / rel_pos_w after the
 *   reference's linear re-interpolation to length 2*size-1;  rel_h (B*heads, gh, gh*gw) f32,  rel_w (B*heads, gh*gw, gw) f32.
 *   hd in {64, 80}; gh, gw <= 96.
 */
int hipie_vit_relpos(const void* qkv, const void* tab_h, const void* tab_w, float* rel_h, float* rel_w,
                     int B, int gh, int gw, int heads, int hd, int dtype, void* stream);

/*
 * Fused residual add + LayerNorm + cast:  s = x + delta;  res_out = s (optional);  norm_out = LN(s) * gamma + beta.
 * Replaces the add -> nn.LayerNorm -> cast chains of Block.forward (backbone/vit.py:212-230, eps 1e-6) and of the post-norm
 * residuals in DeformableTransformerEncoderLayer.forward (models/deformable_detr/deformable_transformer_dino.py:384-394).
 *   x (rows, C) x_dtype; delta (rows, C) delta_dtype or NULL; gamma, beta (C) f32; res_out (rows, C) x_dtype or NULL;
 *   norm_out (rows, C) norm_dtype.  C % 4 == 0, C <= 2048.  fp32 statistics (two-pass mean / centred variance).
 */
int hipie_add_layernorm(const void* x, const void* delta, const float* gamma, const float* beta, void* res_out,
                        void* norm_out, int64_t rows, int C, float eps, int x_dtype, int delta_dtype, int norm_dtype,
                        void* stream);

/*
 * Backward of hipie_add_layernorm for the training step (fp32): the input gradient with the residual stream's gradient added, and the
 * parameter gradients, in one pass over the rows.
 * Replaces: torch.autograd through torch.nn.LayerNorm as used by Block.forward (backbone/vit.py:212-230) and by the post-norm residuals
 *           of DeformableTransformerEncoderLayer.forward (models/deformable_detr/deformable_transformer_dino.py:384-394), plus the
 *           accumulation of the residual branch's gradient that autograd runs as a pass of its own.
 *   s (rows, C): the tensor that was normalised (x + delta, the forward's res_out);  gy (rows, C): gradient of the LayerNorm output;
 *   gres (rows, C) or NULL: gradient arriving at s from the residual stream;  gamma (C).
 *   mean / rstd are recomputed from s with the forward's arithmetic;  xhat = (s - mean) * rstd,  g = gy * gamma:
 *   dx (rows, C) = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) + gres;  dx may alias gres (not s, not gy).
 *   dgamma (C) = sum_rows gy * xhat,  dbeta (C) = sum_rows gy: overwritten; both NULL = input gradient only.  Summed without atomics in a
 *   fixed order (one partial row per workgroup in `ws`, then a second kernel): bit-reproducible from call to call.
 *   ws: at least hipie_layernorm_backward_ws_bytes(rows, C) bytes when dgamma is wanted = min(ceil(rows / 4), 1024) workgroups x 2 C floats.
 *   C % 4 == 0, C <= 2048, 16-byte aligned buffers.  rows == 0: returns 0, zero-fills dgamma / dbeta when given.
 */
int hipie_layernorm_backward(const float* s, const float* gy, const float* gres, const float* gamma, float* dx, float* dgamma,
                             float* dbeta, void* ws, int64_t ws_bytes, int64_t rows, int C, float eps, void* stream);
int64_t hipie_layernorm_backward_ws_bytes(int64_t rows, int C);

/*
 * The pointwise activation between the two linears of an MLP, for the training step (fp32): forward, and a backward that produces the
 * input gradient, the RECOMPUTED activation and the bias gradient of the first linear in one pass over u and g.
 * Replaces: in the backward of timm's Mlp (fc1 -> nn.GELU() -> fc2, backbone/vit.py:193-197) and of the FFN of
 *           DeformableTransformerEncoderLayer.forward (linear1 -> ReLU -> linear2, models/deformable_detr/deformable_transformer_dino.py:384-394):
 *           the library's gelu_backward / threshold_backward, the separate row sum of the first linear's bias gradient, and the saved copy of
 *           a = act(u) -- the graph keeps u alone.
 *   act: 1 = exact-erf GELU (the branch-free formula of hipie_gemm's epilogue, bit for bit), 2 = ReLU -- hipie_gemm's numbering.
 *   u, g, du, a: (rows, N) fp32, dense rows;  N % 4 == 0;  16-byte aligned buffers.
 * hipie_act_forward:   a = act(u).
 * hipie_act_backward:  du = g * act'(u);  du may alias g (not u).  GELU: act'(u) = Phi(u) + u phi(u), Phi and phi from the forward's own
 *                      h(|u|) and exp2;  ReLU: act'(u) = (u > 0).
 *                      a (or NULL) = act(u), the bits hipie_act_forward writes for the same u;  a aliases nothing.
 *                      dbias (N) (or NULL) = sum_rows du: overwritten.  Summed without atomics in a fixed order (register partials per
 *                      thread, one partial row per workgroup in `ws`, then a second kernel): bit-reproducible from call to call.
 *                      ws: at least hipie_act_backward_ws_bytes(rows, N) bytes when dbias is given
 *                          = min(ceil(rows / 4), max(1, 2048 / ceil(N / 1024))) partial rows x N floats.
 * rows == 0 or N == 0: returns 0 without a launch; rows == 0 zero-fills dbias when given.
 */
int hipie_act_forward(const float* u, float* a, int64_t rows, int N, int act, void* stream);
int hipie_act_backward(const float* u, const float* g, float* du, float* a, float* dbias, void* ws, int64_t rows, int N, int act,
                       void* stream);
int64_t hipie_act_backward_ws_bytes(int64_t rows, int N);

/*
 * The point-sampled mask losses of the training criteria (fp32), forward and backward.
 * Replaces: DetCriterion.loss_masks (SetCriterion.loss_masks, models/deformable_detr/deformable_detr.py:452-524: point_sample of the
 *           predictions and of the gathered targets, sigmoid_focal_loss + dice_loss, models/deformable_detr/segmentation.py:92-117,
 *           jit_loss.py:28-48) and MaskCriterion.loss_masks (models/maskdino/criterion.py:286-336: sigmoid_ce_loss_jit + dice_loss_jit,
 *           jit_loss.py:4-48), with point_sample = detectron2 point_rend/point_features.py:19-42 -- the gather of the matched target
 *           masks, two grid_sample launches, the element-wise passes and their autograd mirrors (the grid-sampler backward among them).
 *   src (N, H, W): matched mask logits, dense.   tgt (T, Ht, Wt): ALL target masks, not gathered; Ht, Wt independent of H, W.
 *   tgt_index (N) int64: row of tgt per instance, in any order, repeats allowed; a value outside [0, T) reads as an all-zero target.
 *   pts (N, P, 2): (x, y) in [0, 1]^2.  Sampling: bilinear, align_corners = false, pixel centres at (i + 0.5) / size, zero outside.
 *   mode: 0 = sigmoid cross entropy, 1 = focal with exponent gamma = 2 (any other gamma is refused) and alpha (alpha < 0: no alpha term).
 *   With lg, lab the two samples of a point and s = sigmoid(lg) -- lab is a bilinear sample, anything in [0, 1]:
 *     lmask[n] = mean_p term(lg, lab)           CE in the softplus form max(lg, 0) - lg lab + log1p(exp(-|lg|)): finite for any logit
 *     ldice[n] = 1 - (2 sum s lab + 1) / (sum s + sum lab + 1)
 *     sums (N, 3) = (sum s lab, sum s, sum lab): what the backward needs of the forward.
 * hipie_point_mask_loss_forward:  a workgroup per 1024 points of an instance, partial sums in `ws` (hipie_point_mask_loss_ws_bytes(N, P) =
 *     N x ceil(P / 1024) x 16 bytes), added by a second kernel in a fixed order.  No atomics: bit-reproducible from call to call.
 * hipie_point_mask_loss_backward: d_src (N, H, W) = d (sum_n g_mask[n] lmask[n] + g_dice[n] ldice[n]) / d src.  The samples are recomputed
 *     (nothing of size N x P is kept); every point adds to the corners it read with fp32 hardware atomics into d_src, which is zeroed
 *     here.  NOT bit-reproducible.  No gradient for tgt or pts.  d_src must not alias src; g_mask, g_dice are read only.
 * Refused (-22): mode outside {0, 1}, gamma != 2, P <= 0 with N > 0, H*W or Ht*Wt >= 2^31 (offsets inside a map are 32-bit, the base of
 *     an instance 64-bit), null pointers, a workspace that is too small.  N == 0: returns 0 without a launch, null pointers allowed.
 */
int hipie_point_mask_loss_forward(const float* src, const float* tgt, const int64_t* tgt_index, const float* pts, float* lmask, float* ldice,
                                  float* sums, void* ws, int64_t ws_bytes, int64_t N, int H, int W, int64_t T, int Ht, int Wt, int P, int mode,
                                  float alpha, float gamma, void* stream);
int64_t hipie_point_mask_loss_ws_bytes(int64_t N, int P);
int hipie_point_mask_loss_backward(const float* src, const float* tgt, const int64_t* tgt_index, const float* pts, const float* sums,
                                   const float* g_mask, const float* g_dice, float* d_src, int64_t N, int H, int W, int64_t T, int Ht, int Wt,
                                   int P, int mode, float alpha, float gamma, void* stream);

/*
 * The token-level focal loss of the vision-language class heads (fp32), forward and backward.
 * Replaces: token_sigmoid_binary_focal_loss (models/deformable_detr/segmentation.py:120-166) as called by SetCriterion.loss_labelsVL
 *           (deformable_detr.py:353-381) and MaskDINO's loss_labels_vl (maskdino/criterion.py:209-238): the boolean indexing with the
 *           text mask (a nonzero, i.e. a host wait for everything queued), the element-wise passes and their autograd mirrors.
 *   logits, onehot (B, Q, T);  keep (B, T) bytes or NULL: token t of image b counts when keep[b, t] != 0;  gamma must be 2.
 * hipie_token_focal_forward:  out[0] = sum over kept (b, q, t) of alpha_t ce (1 - p_t)^2 (alpha < 0: no alpha_t).  A fixed grid of
 *     min(ceil(n / 1024), 1024) workgroups, one partial each in `ws` (hipie_token_focal_ws_bytes(n = B Q T)), added by one workgroup in
 *     a fixed order.  No atomics: bit-reproducible.
 * hipie_token_focal_backward: dlogits = g[0] * d focal / d logits at kept tokens, exactly 0 at dropped ones; g is a DEVICE scalar.
 * Neither waits on the host.  B*Q*T == 0: returns 0 without a launch and writes nothing, null pointers allowed.
 */
int hipie_token_focal_forward(const float* logits, const float* onehot, const uint8_t* keep, float* out, void* ws, int64_t ws_bytes, int B, int Q,
                              int T, float alpha, float gamma, void* stream);
int64_t hipie_token_focal_ws_bytes(int64_t n);
int hipie_token_focal_backward(const float* logits, const float* onehot, const uint8_t* keep, const float* g, float* dlogits, int B, int Q, int T,
                               float alpha, float gamma, void* stream);

/*
 * The importance point selection of the training criteria (fp32, forward only).
 * Replaces: get_uncertain_point_coords_with_randomness (detectron2 point_rend/point_features.py:63-116) as called by SetCriterion.loss_masks
 *           (models/deformable_detr/deformable_detr.py:452-524) and models/maskdino/criterion.py:286-336 with the uncertainty -|logit|: the
 *           (N, C) grid_sample of the candidates, abs / neg, torch.topk (12 launches), the gather of the chosen candidates and the cat.
 *   src (N, H, W): mask logits, dense.   cand (N, C, 2): the over-sampled uniform candidates, (x, y) in [0, 1]^2.
 *   rest (N, P - k, 2): the fresh uniform points.   pts (N, P, 2): the output.   Sampling as in hipie_point_mask_loss_forward.
 *   Score of candidate c = -|sample(src[n], cand[n, c])|.  The k candidates with the LARGEST score (the smallest |logit|) are chosen; ties at
 *   the threshold are taken in ascending candidate index, -0.0 ties with +0.0, a NaN sample counts as the largest score (torch.topk,
 *   hipie_topk).  pts[n, 0:k] = the chosen candidates in ASCENDING CANDIDATE INDEX (torch.topk returns them sorted by score: the losses are
 *   sums over the points, only their summation order differs);  pts[n, k:P] = rest[n].
 *   Two launches: the keys of the candidates into `ws` (hipie_uncertain_points_ws_bytes(N, C) = N x C x 4 bytes), then a 4-pass radix
 *   select and a ballot-ranked compaction per instance; no limit on k.  No floating-point atomics, grids that are functions of (N, C):
 *   bit-reproducible from call to call.
 * Refused (-22): k outside [0, min(C, P)], P or C >= 2^30, H*W outside [1, 2^31) with k > 0, null pointers (src, cand, ws may be null when
 *     k == 0, rest when k == P), a workspace that is too small.  N == 0 or P == 0: returns 0 without a launch, null pointers allowed.
 */
int hipie_uncertain_points(const float* src, const float* cand, const float* rest, float* pts, void* ws, int64_t ws_bytes, int64_t N, int H,
                           int W, int C, int P, int k, void* stream);
int64_t hipie_uncertain_points_ws_bytes(int64_t N, int C);

/*
 * The point-sampled mask costs of the matchers (fp32, forward only).
 * Replaces: batch_sigmoid_ce_loss + batch_dice_loss over point_sample (models/deformable_detr/matcher.py:22-69, 567-597;
 *           models/maskdino/matcher.py:21-68): two grid_sample launches, the (Q, P) tensors softplus(-x), softplus(x) and sigmoid(x), the
 *           (T, P) tensor 1 - t, three GEMMs and the broadcast arithmetic of the dice quotient.
 *   pred (Q, H, W): mask logits.   tgt (T, Ht, Wt): target masks in [0, 1] at their own resolution.   coords (P, 2): (x, y) in [0, 1]^2,
 *   the SAME points for every mask.   Sampling as in hipie_point_mask_loss_forward.   ce, dice (Q, T): the outputs.
 *   With x = sample(pred[q]), t = sample(tgt[j]), s = sigmoid(x):
 *     ce[q, j]   = (sum_p softplus(-x) t + softplus(x) (1 - t)) / P, computed as (sum_p softplus(x) - sum_p x t) / P
 *     dice[q, j] = 1 - (2 sum_p s t + 1) / (sum_p s + sum_p t + 1)
 *   Three launches: the targets are sampled once into `ws`; a workgroup per (4 queries, 2048 points) samples its queries into registers
 *   (the Q x P samples are never written) and leaves its partial dot products in `ws`; a last kernel adds them in a fixed order.
 *   ws: 16-byte aligned, at least hipie_mask_match_cost_ws_bytes(Q, T, P) bytes.  No atomics: bit-reproducible from call to call.
 * Refused (-22): P outside [1, 2^30), H*W or Ht*Wt outside [1, 2^31), null pointers, a workspace that is too small or misaligned.
 *     Q == 0 or T == 0: returns 0 without a launch, null pointers allowed.
 */
int hipie_mask_match_cost(const float* pred, const float* tgt, const float* coords, float* ce, float* dice, void* ws, int64_t ws_bytes, int64_t Q,
                          int H, int W, int64_t T, int Ht, int Wt, int P, void* stream);
int64_t hipie_mask_match_cost_ws_bytes(int64_t Q, int64_t T, int P);

/*
 * The SimOTA cost of a batch of images (fp32, forward only).
 * Replaces: the cost side of HungarianMatcherVL.forward_ota (hipie/models/deformable_detr/matcher.py:347-509: the sigmoid, the token
 *           focal class cost against the positive map, generalized_box_iou with its host-side assert, the in-box / in-centre masks and the
 *           two penalties), about forty launches and one host wait per image.
 *   logits (B, Q, L): raw logits (the sigmoid is taken inside).   boxes (B, Q, 4), tgt_boxes (B, Tmax, 4): cxcywh.
 *   pos_map (B, Tmax, L): uint8, non-zero = a positive token of the target.   n_tgt (B,): the targets of every image, the rest is padding.
 *   cost, iou (B, Tmax, Q): the outputs, TARGET-major.  For t < n_tgt[b]:
 *     cost = mean over the target's positive tokens (ascending) of the focal token cost - 3 x GIoU (the 1e-7 of box_ops.generalized_box_iou)
 *            + 100 where the query centre is not both strictly inside the target box and within center_radius / stride of its centre
 *            + 10000 on queries that are inside or near no target of their image;     iou = inter / union.
 *     A target without a positive token gives NaN (the reference's mean over nothing).  For t >= n_tgt[b]: cost = +inf, iou = 0.
 *   status (B,): written, not accumulated.  Bit 0: a query box or a target box of the image has x1 < x0 or y1 < y0 (the reference's assert);
 *     bit 1: a target in front of n_tgt[b] has no positive token.
 *   One launch; the token costs of a query row are computed once (LDS).  No atomics on memory: bit-reproducible from call to call.
 * Refused (-22): Q > 4096, Tmax > 256, L outside [1, 1024], B > 65535, stride <= 0, null pointers.
 *     B == 0, Q == 0 or Tmax == 0: returns 0 without a launch, null pointers allowed.
 */
int hipie_ota_cost(const float* logits, const float* boxes, const float* tgt_boxes, const unsigned char* pos_map, const int* n_tgt, float* cost,
                   float* iou, int* status, int64_t B, int Q, int Tmax, int L, float center_radius, float stride, void* stream);

/*
 * SimOTA's dynamic-k assignment on the two buffers of hipie_ota_cost, one workgroup per image.
 * Replaces: dynamic_k_matching (hipie/models/deformable_detr/matcher.py:347-509): per target a topk, an index-put and a host wait, the
 *           host-side `while` of the repair loop and two nonzero.
 *   cost (B, Tmax, Q): MODIFIED IN PLACE as the reference modifies it (+100000 on the rows that hold a match, once per repair round; the
 *   reference's last step, +inf on everything unmatched, is not applied).   iou (B, Tmax, Q).   n_tgt (B,).
 *   Target t takes its k_t cheapest queries, k_t = max(1, (int)(the sum of its min(Q, 10) largest IoUs, added in descending order)); a
 *   query claimed by several targets keeps the cheapest; while a target is empty, every matched row gets +100000, every empty target takes
 *   the arg-min of its column, and if a row then has several matches the rows that were contested BEFORE the loop (the reference re-uses
 *   that mask) are reset to their current cheapest target.  Every tie goes to the lowest index.
 *   pair_q, pair_t (B, Q): the matched queries of image b in ascending order and the first target of each, n_pairs[b] of them.
 *   best (B, Tmax): per target the matched query of the smallest cost (0 behind n_tgt[b]).   rounds (B,): the repair rounds that ran.
 *   status (B,): bit 2 is ORed in when the repair loop was stopped after Q rounds (the reference would not return).
 *   n_tgt[b] == 0: n_pairs[b] = 0.  The only atomics are integer LDS atomics: bit-reproducible from call to call.
 * Refused (-22): Q > 4096, Tmax > 256 (the match bitmap, Q x ceil(Tmax / 32) words, lives in LDS), null pointers.
 *     B == 0, Q == 0 or Tmax == 0: returns 0 without a launch, null pointers allowed.
 */
int hipie_ota_assign(float* cost, const float* iou, const int* n_tgt, int* pair_q, int* pair_t, int* best, int* n_pairs, int* status, int* rounds,
                     int64_t B, int Q, int Tmax, void* stream);
/* bytes of the two (B, Tmax, Q) fp32 buffers, cost first (hipie/models/deformable_detr/matcher.py:347-509) */
int64_t hipie_ota_match_ws_bytes(int64_t B, int64_t Q, int64_t Tmax);

/*
 * The cost matrices of the one-to-one Hungarian matchers for a whole batch (fp32, forward only).
 * Replaces: the cost side of HungarianMatcherVL.forward / forward with force_box_loss (models/deformable_detr/matcher.py:511-729) and of
 *           MaskDINO's HungarianMatcher (models/maskdino/matcher.py:76-259), per image: the sigmoid, the element-wise passes of the focal
 *           token cost, the matmul with the positive map (or the column gather by class id), cdist, generalized_box_iou with its host-side
 *           assert, the index puts of the stuff mean, two nan_to_num and the weighted sums -- about forty launches and a host wait.
 *   logits (B, Q, L): raw logits (the sigmoid is taken inside); image b starts at element b * logits_stride, its (Q, L) rows are dense.
 *   boxes (B, Q, 4): cxcywh, image stride boxes_stride; tgt_boxes (B, Tmax, 4).  Both may be null when with_boxes == 0.
 *   n_tgt (B,): the targets of every image, the rest is padding.   t_off (B,): the exclusive prefix sum of n_tgt.   sum_t: their total.
 *   The class side is exactly one of   pos_map (B, Tmax, L): uint8, non-zero = a positive token of the target (map mode), and
 *                                      labels (B, Tmax): int32, the class cost is the token cost of column labels[t] (ids mode).
 *   is_thing (B, Tmax): uint8, read only with with_boxes && stuff_takes_mean.
 *   ce, dice: both null, or both packed exactly like C and holding the point-sampled mask costs (hipie_mask_match_cost writes them there).
 *   C: the output, PACKED and QUERY-major: image b is a dense row-major (Q, n_tgt[b]) block starting at element Q * t_off[b]; Q * sum_t
 *   elements in all, no padding columns, an image without targets takes none.  In the order of matcher.cost_matrix:
 *     cls = the sum over the target's positive tokens (ascending) of the focal token cost / their count (none: NaN, the reference's mean
 *           over nothing; scipy refuses the matrix as it does today)            l1 = the sum of the four |differences|         gi = -GIoU
 *     with stuff_takes_mean: every non-thing column of l1 takes the mean of l1 over all Q x thing entries of its image, the same for gi;
 *           then every NaN of l1 and gi becomes 0 and infinities stay (an image without things gets 0).  Without it nothing is zeroed.
 *     C = (((w_cls cls + w_l1 l1) + w_giou gi) + w_mask ce) + w_dice dice, the box terms and the mask terms left out when absent.
 *   status (B,): written, not accumulated.  Bit 0: with_boxes and a query or target box of the image has a corner pair out of order or a
 *     NaN (the ValueError of boxes.generalized_box_iou); bit 3: ids mode and a label outside [0, L) (its column is NaN); bit 4: t_off[b] +
 *     n_tgt[b] does not fit sum_t (nothing of the image is written).
 *   One launch; with the stuff mean a pre-pass leaves float64 partial sums per 64 queries in `ws` (8-byte aligned, at least
 *   hipie_hungarian_cost_ws_bytes(B, Q) bytes; may be null otherwise) and every workgroup adds them in the same order.  No floating-point
 *   atomics, grids are functions of (B, Q): bit-reproducible from call to call.
 * Refused (-22): Q > 4096, Tmax > 256, L outside [1, 1024], B > 65535, sum_t > B x Tmax, both or neither of pos_map / labels, one of ce /
 *     dice alone, an image stride below a dense image, null pointers, a workspace that is too small or misaligned.
 *     B == 0, Q == 0 or Tmax == 0: returns 0 without a launch, null pointers allowed.
 */
int hipie_hungarian_cost(const float* logits, int64_t logits_stride, const float* boxes, int64_t boxes_stride, const float* tgt_boxes,
                         const int* n_tgt, const int* t_off, const unsigned char* pos_map, const int* labels, const unsigned char* is_thing,
                         const float* ce, const float* dice, float* C, int* status, void* ws, int64_t ws_bytes, int64_t B, int Q, int Tmax,
                         int L, int64_t sum_t, float w_cls, float w_l1, float w_giou, float w_mask, float w_dice, int with_boxes,
                         int stuff_takes_mean, void* stream);
/* bytes of the packed output, Q * sum_t fp32 elements */
int64_t hipie_hungarian_cost_bytes(int64_t Q, int64_t sum_t);
/* bytes of the stuff mean's partial sums */
int64_t hipie_hungarian_cost_ws_bytes(int64_t B, int64_t Q);

/*
 * The one-to-one assignment of the Hungarian matchers for a batch of images, on the packed costs of hipie_hungarian_cost: per image the pairs
 * of scipy.optimize.linear_sum_assignment on its (Q, n_tgt[b]) block, tie for tie, as int64 on the device.  One launch, one workgroup of 256
 * threads per image; nothing is read by the host.
 * Replaces: `C.cpu()` and linear_sum_assignment per image (models/deformable_detr/matcher.py:599-606, models/maskdino/matcher.py:171-178) and
 *           the host -> device copies of the index tensors wherever the criteria index with them.
 *   C: hipie_hungarian_cost's output, unchanged: image b is a dense row-major (Q, n_tgt[b]) block at element Q * t_off[b], Q * sum_t elements.
 *   cost_status (B,): the status words the cost kernel wrote (they sit behind the blocks of its output).
 *   n_tgt, t_off (B,), sum_t: as for hipie_hungarian_cost.
 *   pair_q, pair_t (B, K) int64, K = min(Q, Tmax): image b's min(Q, n_tgt[b]) pairs (query, target) in ascending query order, 0 behind them.
 *   status (B,): written, not accumulated.  cost_status[b], bit 4 when t_off[b] + n_tgt[b] does not fit sum_t, and the solver's own bits:
 *     bit 5 (32): the block holds a NaN or -inf ("matrix contains invalid numeric entries"; +inf entries are legal), bit 6 (64): "cost matrix is
 *     infeasible", bit 7 (128): the search of a row did not end within min(Q, n) columns (valid input cannot get there; the bound of the loop).
 *     An image with a non-zero status is not solved and all its pairs are 0: valid indices, whatever is indexed with them before the status is read.
 *   The solver is scipy's (Crouse 2016, shortest augmenting paths) operation for operation: float64 adds, subtracts and compares on the widened
 *     costs, reduced cost ((minVal + C[i][j]) - u[i]) - v[j], the unscanned columns listed in reverse with a removed entry replaced by the last,
 *     the lowest candidate chosen as the sequential scan chooses it (an unassigned column at the largest list position, else the smallest position).
 *     With Q > n_tgt[b] the rows are the targets (scipy's transposition); the block is first written target-major into `ws`.
 *   ws: 4-byte aligned, at least hipie_hungarian_assign_ws_bytes(Q, sum_t) bytes.  Bit-reproducible; every loop is bounded by min(Q, Tmax) <= 256.
 * Refused (-22): Q > 4096, Tmax > 256, B > 65535, sum_t > B x Tmax, null pointers, a workspace that is too small or misaligned.
 *     B == 0, Q == 0 or Tmax == 0: returns 0 without a launch, null pointers allowed.
 */
int hipie_hungarian_assign(const float* C, const int* cost_status, const int* n_tgt, const int* t_off, int64_t* pair_q, int64_t* pair_t, int* status,
                           void* ws, int64_t ws_bytes, int64_t B, int Q, int Tmax, int64_t sum_t, void* stream);
/* bytes of the target-major copy of the costs, Q * sum_t fp32 elements (never 0) */
int64_t hipie_hungarian_assign_ws_bytes(int64_t Q, int64_t sum_t);

/*
 * What the training criteria do with the matched (query, target) pairs of one call (csrc/pair_loss.hip; fp32 operands, a pair is evaluated
 * in float64 and rounded once), forward and backward.
 * Replaces: SetCriterion.loss_boxes (models/deformable_detr/deformable_detr.py:397-450, mode 0) and models/maskdino/criterion.py:240-284
 *           (mode 1): the gathers of the matched boxes, box_cxcywh_to_xyxy, l1_loss, giou_loss / generalized_box_iou, the box-IoU BCE, the
 *           thing mask and its re-weighting with their autograd mirrors, and the host wait of `thing.sum() == 0` / the degenerate-box assert;
 *           the loop over the images in front of every loss_labelsVL that writes the matched rows of the positive maps into the one-hot.
 *   The pairs: pair_q, pair_t are HOST arrays of B device addresses -- per image the int64 query and target indices of its pairs, as the
 *     matchers return them --, pair_n the HOST array of their lengths.  They are placed in the kernel arguments: B <= 64, at most 65536 pairs;
 *     nothing is copied to the device and nothing waits.  A pair with an index outside [0, Q) x [0, Tmax) is left out and sets status bit 2.
 *   boxes (B, Q, 4) cxcywh by element strides (box_stride_b, box_stride_q; the 4 coordinates dense): a slice of the query axis needs no copy.
 *   iou: NULL or the (B, Q) box-IoU logits by element strides.   tgt_boxes (B, Tmax, 4), is_thing (B, Tmax) bytes or NULL (every pair counts).
 *   mode 0: w = is_thing != 0 (or 1), reweight = K / (sum w + 1e-6);  loss_bbox = reweight sum w |src - tgt|_1 / count;  loss_giou = reweight
 *     sum w (1 - GIoU) / count with the intersection counted only where the boxes overlap and 1e-7 in both quotients (fvcore giou_loss);
 *     loss_boxiou = reweight mean w BCE_with_logits(iou logit, IoU), the IoU target without gradient.  With no thing among the pairs the three
 *     losses and every gradient are exactly 0.
 *   mode 1: the pairs with is_thing == 0 are left out;  loss_bbox = sum |src - tgt|_1 / count;  loss_giou = sum (1 - GIoU) / count with every
 *     extent clamped at 0 and 1e-7 in the hull quotient only (util/box_ops.py generalized_box_iou).  A box with x1 < x0 or y1 < y0 (or a NaN)
 *     among the evaluated pairs sets status bit 1 -- the reference's assert; the outputs are still those of the formula.
 *   Ties of max / min give half the gradient to each side, |x| has gradient 0 at 0, a clamp passes the gradient at exactly 0 (torch).
 * hipie_pair_box_loss_forward:  out (8 floats, 8-byte aligned) = loss_bbox, loss_giou, loss_boxiou, 0 and two float64 factors for the
 *     backward;  pair_grad (K, 9) the weighted per-pair gradients;  status (1) int32.  A workgroup per 256 pairs, float64 partial sums in `ws`
 *     (hipie_pair_box_loss_ws_bytes(K), 8-byte aligned), added by one workgroup in a fixed order.  No atomics: bit-reproducible.  Two launches.
 * hipie_pair_box_loss_backward: d_boxes (B, Q, 4) and d_iou (B, Q; NULL without iou), dense, are zero-filled here and every pair adds
 *     g x factor x its stored gradient with a global fp32 atomic: duplicates of an (image, query) sum; with one target per (image, query)
 *     every element receives one addition and the result is bit-reproducible.  g_bbox, g_giou, g_boxiou: DEVICE scalars.  One launch.
 * hipie_positive_onehot: onehot (B, Q, L) fp32 is zero-filled, then onehot[b, q_i] = (pos_map[b, t_i] != 0) for every pair; pos_map
 *     (B, Tmax, L) bytes.  One launch.
 * Refused (-22): mode outside {0, 1}, iou with mode 1, count <= 0 or not finite, B > 64, more than 65536 pairs, a negative size or length,
 *     pairs with Q == 0 or Tmax == 0, strides that do not describe the rows, null pointers, a workspace that is too small or misaligned.
 *     No pairs: the forward returns 0 without a launch and writes nothing, the backward and the one-hot only zero-fill; null pointers allowed.
 */
int hipie_pair_box_loss_forward(const float* boxes, int64_t box_stride_b, int64_t box_stride_q, const float* iou, int64_t iou_stride_b,
                                int64_t iou_stride_q, const int64_t* const* pair_q, const int64_t* const* pair_t, const int64_t* pair_n,
                                const float* tgt_boxes, const uint8_t* is_thing, float* out, float* pair_grad, int* status, void* ws,
                                int64_t ws_bytes, int B, int Q, int Tmax, int mode, double count, void* stream);
int64_t hipie_pair_box_loss_ws_bytes(int64_t K);
int hipie_pair_box_loss_backward(const int64_t* const* pair_q, const int64_t* pair_n, const float* out, const float* pair_grad,
                                 const float* g_bbox, const float* g_giou, const float* g_boxiou, float* d_boxes, float* d_iou, int B, int Q,
                                 void* stream);
int hipie_positive_onehot(const int64_t* const* pair_q, const int64_t* const* pair_t, const int64_t* pair_n, const uint8_t* pos_map,
                          float* onehot, int B, int Q, int Tmax, int L, void* stream);

/*
 * The tail of a training iteration behind backward() as two passes over memory (csrc/optim_step.hip): the total gradient norm, and the clip
 * and the AdamW update of EVERY parameter tensor in one launch; fp32, nothing is read by the host, bit-reproducible from call to call.
 * Replaces: torch.nn.utils.clip_grad_norm_ inside FullModelGradientClippingOptimizer.step (projects/HIPIE/train_net.py:199-228, with
 *           scale_norm's multiply of every gradient by 1 / ACC_ITER in front of it): the per-tensor norms, their stack and norm, the
 *           coefficient and the multiply that reads and writes every gradient -- here the coefficient is a scalar of the update;
 *           torch.optim.AdamW as used by projects/HIPIE/train_net.py:189-239: the multi-tensor step over 1241 tensors, with the
 *           per-parameter learning-rate groups of :167-187 as a group index per tensor.
 *   table: n_seg records of 48 bytes on the device, one per parameter tensor: { float* p, g, m, v; int64 numel; int32 group; int32 0 }.
 *     g == NULL: the tensor has no gradient this step -- it adds nothing to the norm and the update skips it whole (no weight decay, m, v
 *     and its step count untouched, as torch does).  Any 4-byte aligned addresses: a tensor whose address is 16-byte aligned is accessed
 *     16 bytes at a time, another one 4 bytes at a time (gradients that are views into a flat bucket), per tensor.
 *   map: n_chunks pairs { int64 segment; int64 offset } on the device: the elements [offset, min(offset + hipie_optim_chunk(), numel)) of the
 *     segment, every element of every segment exactly once, offsets multiples of hipie_optim_chunk().  A function of the sizes alone.  An
 *     entry outside its segment or the table is skipped.
 *   hipie_optim_grad_norm: *norm = (float)(sqrt(sum of g^2) x |grad_scale|): squares and sums in float64, one partial sum per chunk in its
 *     own slot of `ws` (8-byte aligned, hipie_optim_norm_ws_bytes(n_chunks) bytes), every sum in a fixed order that depends on neither the
 *     grid nor the alignment of a gradient; no atomics.  Two launches.
 *   hipie_optim_adamw_step: steps (n_seg) int32, the per-parameter step counts, and bc (n_seg, 2) f32 live on the device: every segment with
 *     a gradient gets t = ++steps[s] and bc[s] = (1 - beta1^t, sqrt(1 - beta2^t)), computed in float64.  Then per element, in fp32 without
 *     contraction and in the order of torch's single-tensor AdamW:
 *       c = norm ? min(max_norm / (*norm + 1e-6), 1) : 1 (a NaN stays a NaN, as torch.clamp keeps it);  g' = (g x grad_scale) x c;
 *       p = p x (1 - lr wd);  m = lerp(m, g', 1 - beta1);  v = v x beta2 + ((1 - beta2) g') g';  p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 *     group_lr, group_wd: n_groups <= 8 doubles each on the HOST, read during the call and passed to the kernel by value (a scheduler that
 *     changes lr every iteration uploads nothing).  norm: the device float of hipie_optim_grad_norm, or NULL for no clipping (max_norm is
 *     then ignored).  write_grads != 0: g' is also written back into g.  Two launches.
 * Refused (-22): a negative count, more than 8 groups, a beta outside [0, 1), eps <= 0, max_norm < 0 with a norm, a null table, map,
 *     workspace, norm output, steps, bc or group array, a misaligned table, map or workspace, a workspace that is too small.
 *     n_seg == 0 or n_chunks == 0: returns 0 without a launch, null pointers allowed.
 */
#define HIPIE_OPTIM_CHUNK 16384
int hipie_optim_chunk(void);
/* bytes of the float64 partial sums, one per chunk (never 0) */
int64_t hipie_optim_norm_ws_bytes(int64_t n_chunks);
int hipie_optim_grad_norm(const void* table, int64_t n_seg, const void* map, int64_t n_chunks, void* ws, int64_t ws_bytes, float grad_scale,
                          float* norm, void* stream);
int hipie_optim_adamw_step(const void* table, int64_t n_seg, const void* map, int64_t n_chunks, int32_t* steps, float* bc,
                           const double* group_lr, const double* group_wd, int n_groups, double beta1, double beta2, double eps,
                           const float* norm, double max_norm, float grad_scale, int write_grads, void* stream);

/*
 * hipie_vit_attn with the decomposed relative-position bias computed INSIDE the kernel from the (re-interpolated) tables
 * (get_rel_pos + add_decomposed_rel_pos, hipie/backbone/utils.py:63-125): bias_w[q, kx] = q . Rw[qx - kx + gw - 1] and
 * bias_h[q, ky] = q . Rh[qy - ky + gh - 1] are two MFMA products per wave in the prologue, so neither hipie_vit_relpos nor
 * its (B*heads, N, gh + gw) fp32 outputs are needed.  tab_h (2*gh-1, hd), tab_w (2*gw-1, hd) in `dtype`, entry
 * [q - k + size - 1].  Geometry: gw == 64, gh <= 64, hd in {64, 80} (the 1024-pixel global blocks); else HIPIE_EINVAL and the
 * caller uses hipie_vit_relpos + hipie_vit_attn.
 */
int hipie_vit_attn_fused(const void* qkv, const void* tab_h, const void* tab_w, void* out, int B, int gh, int gw, int heads,
                         int hd, float scale, int dtype, void* stream);

/*
 * ViT attention of one block with the decomposed relative-position bias computed inside the kernel -- global blocks (one
 * key tile = one key row of the gh x gw token grid) and the 14 x 14 windowed blocks (B = batch * windows; two key rows per
 * tile) alike.  Replaces: Attention.forward between the qkv and proj Linears (backbone/vit.py:69-80) including
 * get_rel_pos + add_decomposed_rel_pos (backbone/utils.py:63-125).
 * Operand contract (the two constants are folded into the weights once by the host, hipie_amd/modeling/vit.py):
 *   qkv   (B, gh*gw, 3, heads, hd) 16-bit with the q rows PRE-SCALED:  q' = scale * log2(e) * q
 *   tab_h (2*gh-1, hd), tab_w (2*gw-1, hd) 16-bit = rel_pos_h / rel_pos_w after the reference's linear re-interpolation to
 *         2*size-1 rows, DIVIDED by scale (entry [q - k + size - 1])
 *   so that q'.k + q'.tab_h' + q'.tab_w' is the attention logit in the exp2 domain.
 *   out   (B, gh*gw, heads*hd) 16-bit.   hd in {64, 80};  gw <= 96;  gh <= 84 when gw > 64 (LDS);  flags: HIPIE_ATTN_FAST.
 */
int hipie_vit_attn_rel(const void* qkv, const void* tab_h, const void* tab_w, void* out, int B, int gh, int gw, int heads,
                       int hd, int dtype, int flags, void* stream);

/*
 * hipie_add_layernorm with row maps, so that window_partition / window_unpartition (hipie/backbone/utils.py:16-60) around
 * the windowed ViT blocks (backbone/vit.py:214-225) cost no pass of their own:
 *   for every OUTPUT row j < out_rows:  r = out_src ? out_src[j] : j;   r < 0: norm_out[j] = 0 (a pad token);  otherwise
 *   s = x[r] + delta[delta_row ? delta_row[r] : r];  res_out[r] = s (optional);  norm_out[j] = LN(s) * gamma + beta.
 *   out_src (out_rows) int32: token row feeding each row of the (padded, window-ordered) output, or NULL;
 *   delta_row (rows of x) int32: where the residual branch of token r lives (the window-ordered attention output), or NULL.
 */
int hipie_add_layernorm_rows(const void* x, const void* delta, const float* gamma, const float* beta, void* res_out,
                             void* norm_out, int64_t out_rows, int C, float eps, int x_dtype, int delta_dtype,
                             int norm_dtype, const int32_t* delta_row, const int32_t* out_src, void* stream);

/*
 * hipie_add_layernorm with a second output  sum_out = norm_out + addend  (both `norm_dtype`, (rows, C)): the post-norm residual of
 * a deformable ENCODER layer that also prepares the next layer's query `src + pos`
 * (deformable_transformer_dino.py:384-394, with_pos_embed :380) in the same pass.
 */
int hipie_add_layernorm_sum(const void* x, const void* delta, const float* gamma, const float* beta, void* res_out,
                            void* norm_out, const void* addend, void* sum_out, int64_t rows, int C, float eps,
                            int x_dtype, int delta_dtype, int norm_dtype, void* stream);

/*
 * The post-norm residual of a DINO decoder layer (deformable_transformer_dino.py:418-450 == dino_decoder.py:222-268) when the
 * query stream is fp32 and the GEMMs take 16-bit operands:  n = LayerNorm(x + delta) is written once in fp32 (norm_out, the next
 * residual) and, optionally and in the same pass, as norm16_out = (aux)n and sum16_out = (aux)(n + addend)  (addend = the
 * positional query, `aux_dtype`): the inputs of the next value / FFN / box GEMMs and of the next attention's query GEMM.
 *   x (rows, C) f32; delta (rows, C) `delta_dtype`; aux_dtype f16 | bf16; C % 4 == 0, C <= 2048; fp32 two-pass statistics.
 */
int hipie_add_layernorm_dec(const float* x, const void* delta, const float* gamma, const float* beta, float* norm_out,
                            void* norm16_out, const void* addend, void* sum16_out, int64_t rows, int C, float eps,
                            int delta_dtype, int aux_dtype, void* stream);

/*
 * The two small MLP heads of a decoder layer, one launch each (they were a sine kernel + 2 GEMMs, and 3 GEMMs + the refinement):
 *   hipie_ref_point_mlp: query_pos = ref_point_head(get_sine_pos_embed(ref)) -- deformable_transformer_dino.py:484-490 / dino_decoder.py
 *     :126-131; ref (n, ref_stride >= 4) f32 boxes (x, y, w, h); dim_t (128) as in hipie_sine_embed; w1t (512, 256), w2t (256, 256) =
 *     the layers' weights TRANSPOSED to (in, out), biases, output (n, 256) all in `dtype`; sine features and the hidden activations are
 *     rounded to `dtype` where the GEMM path rounded them, fp32 accumulation.
 *   hipie_box_head: new_ref = sigmoid(bbox_embed(x) + inverse_sigmoid(ref)) -- :502-520 with MLP(256, 256, 4, 3); everything f32;
 *     w1t, w2t (256, 256), w3t (256, 4) transposed weights; x (n, 256), ref, out (n, 4).
 */
int hipie_ref_point_mlp(const float* ref, const float* dim_t, const void* w1t, const void* b1, const void* w2t, const void* b2,
                        void* out, int64_t n, int ref_stride, float scale, int dtype, void* stream);
int hipie_box_head(const float* x, const float* ref, const float* w1t, const float* b1, const float* w2t, const float* b2,
                   const float* w3t, const float* b3, float* out, int64_t n, float eps, void* stream);

/*
 * GroupNorm with 8 channels per group (GroupNorm(32, 256) of every conv + GN block after the backbone: input_proj of both heads,
 * deformable_detr.py:139-160; the pixel decoder's lateral / output convs and mask_features head, maskdino_encoder.py:262-300),
 * on the layout the tensor arrives in, with an optional per-channel pre-bias (y = GN(x + prebias[c])) and an optional ReLU.
 *   x, out (B, C, H*W) when channels_last == 0, (B, H*W, C) when 1;  channels_last == 2: x (B, H*W, C), out (B, C, H*W) -- the map
 *   leaves pixel-fastest (the mask_features operand of hipie_mask_einsum) through an LDS tile, no transposing copy; H*W % 64 == 0;
 *   workspace: 2 * B * groups * 512 floats (partial sums);
 *   gamma, beta (C) f32;  statistics fp32 (sum / sum of squares per group, biased variance, eps inside the sqrt).
 *   C == 8 * groups, 256 % groups == 0;  NCHW: H*W % 8 == 0.  Two launches, no atomics (deterministic).
 */
int hipie_group_norm(const void* x, const float* prebias, const float* gamma, const float* beta, void* out, float* workspace,
                     int B, int C, int HW, int groups, int channels_last, float eps, int relu, int x_dtype, int out_dtype,
                     void* stream);

/*
 * hipie_group_norm for the training step: NCHW, fp32, no pre-bias, with the statistics the apply pass used as a second output.
 * Replaces: the forward of torch.nn.GroupNorm(32, 256) (+ F.relu) as the conv + GN blocks use it in training (deformable_detr.py:139-160,
 *           maskdino_encoder.py:262-300), and the mean / rstd tensors torch.native_group_norm saves for its backward.
 *   x, y (B, C, H*W) f32;  y: the bits hipie_group_norm(channels_last 0, f32 -> f32, prebias NULL) writes for the same arguments;
 *   stat (B, groups, 2) f32 = (mean, rstd) per (image, group), written by a third small launch from the same partial sums;
 *   workspace: hipie_group_norm_backward_ws_bytes(B, C, HW) bytes (2 floats per image, channel and chunk of a row).
 *   C == 8 * groups, 256 % groups == 0, H*W % 8 == 0.  B == 0: returns 0.
 */
int hipie_group_norm_train_forward(const float* x, const float* gamma, const float* beta, float* y, float* stat, float* workspace,
                                   int B, int C, int HW, int groups, float eps, int relu, void* stream);

/*
 * Backward of hipie_group_norm_train_forward: the input gradient and the parameter gradients of GroupNorm (+ ReLU) in two passes over
 * x and dy and a partial-row sum.
 * Replaces: torch.autograd through torch.nn.GroupNorm(32, 256) and the F.relu behind it in the conv + GN blocks (input_proj of both heads,
 *           deformable_detr.py:139-160; adapter_1 / layer_1 / mask_features of the pixel decoder, maskdino_encoder.py:262-300): the
 *           library's group-norm backward, the ReLU backward in front of it and the pre-ReLU map autograd keeps for the two.
 *   x, dy (B, C, H*W) f32;  stat (B, groups, 2): the forward's (mean, rstd);  gamma, beta (C).
 *   xhat = (x - mean) * rstd;  g = dy, with relu g = dy * [fmaf(x, sc, sh) > 0] from the forward's own scale / shift -- the forward's y > 0
 *   bit for bit, no mask is saved;  n = 8 H*W;  s1 = sum_group gamma_c g,  s2 = sum_group gamma_c g xhat:
 *   dx (B, C, H*W) = rstd * (gamma_c g - (s1 + xhat s2) / n), or NULL (frozen input: the second pass is not launched);
 *   dgamma (C) = sum g xhat,  dbeta (C) = sum g over images and pixels: overwritten; both NULL = input gradient only; all three NULL:
 *   nothing is launched.  No atomics, fixed order of the additions: bit-reproducible from call to call.
 *   ws: at least hipie_group_norm_backward_ws_bytes(B, C, HW) bytes = B x chunks x 2 C floats, chunks = the runs a row of H*W values is
 *   cut into (one below 16384 values, at most 64).  C == 8 * groups, 256 % groups == 0, H*W % 8 == 0.  B == 0: returns 0.
 */
int hipie_group_norm_backward(const float* x, const float* dy, const float* stat, const float* gamma, const float* beta, float* dx,
                              float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, int B, int C, int HW, int groups, int relu,
                              void* stream);
int64_t hipie_group_norm_backward_ws_bytes(int B, int C, int HW);

/* out = (dtype)(a + b): a (n) f32, b (n) `dtype` f16 | bf16 -- `tgt + query_pos` rounded once to the GEMM operand type. */
int hipie_add_cast(const float* a, const void* b, void* out, int64_t n, int dtype, void* stream);

/*
 * Batched (class-aware) NMS for one batch of images, the device form of the per-image
 *   keep_indices = torchvision.ops.batched_nms(box_cxcywh_to_xyxy(box_pred), nms_scores, idxs, 0.7)
 * in HIPIE_IMG.inference (projects/HIPIE/hipie/hipie_img.py:626-629).
 *   boxes (B, Q, 4) f32 normalised cxcywh; classes (B, Q) int64; order (B, Q) int32 = stable descending argsort of the
 *   NMS scores (positions into Q); keep (B, Q) int32 out: surviving query indices in decreasing-score order, -1 padded;
 *   count (B) int32 out.  coordinate_trick 1: torchvision's <=4000-coordinate path (every box offset by
 *   class * (max_coordinate + 1), all pairs compared); 0: only same-class pairs on the raw boxes (its >4000 path).
 *   IoU = inter / (area_i + area_j - inter) > iou_threshold suppresses, evaluated with single IEEE roundings (no FMA),
 *   so keep/count are bit-exact against the CPU algorithm.  Q <= 1024 (the Q x Q bit matrix lives in LDS).
 */
int hipie_batched_nms(const float* boxes, const int64_t* classes, const int32_t* order, int32_t* keep, int32_t* count,
                      int B, int Q, float iou_threshold, int coordinate_trick, void* stream);

/*
 * Instance-mask finalisation for one image:  F.interpolate(x`up`, bilinear, align_corners=False) -> sigmoid -> "> threshold"
 * -> crop to (crop_h, crop_w)  (hipie_img.py:693-699)  -> F.interpolate(size=(out_h, out_w), mode="nearest") -> byte
 * (segmentation_postprocess, hipie/models/ddetrs.py:1065-1070), in one pass over the stride-`up` logits.
 *   masks (*, hm, wm) `dtype`; qidx (n) int32 rows of `masks` to process (NULL: rows 0..n-1); out (n, out_h, out_w) uint8.
 */
int hipie_mask_finalize(const void* masks, int dtype, const int32_t* qidx, int n, int hm, int wm, int up, int crop_h,
                        int crop_w, int out_h, int out_w, float threshold, uint8_t* out, void* stream);

/*
 * Fused semantic + panoptic maps of one image -- the tensor part of the detection tail of HIPIE_IMG.inference
 * (hipie_img.py:716-748), semantic_inference (:870-878) and panoptic_inference (:473-505):
 *   sig[q] = sigmoid(resize(masks[q]))  with resize = bilinear x`up` -> crop (crop_h, crop_w) -> bilinear to (out_h, out_w);
 *   sem[c] = sum_q cls[q, c] * sig[q];   pan_idx = argmax_q pscore[q] * sig[q] over pscore > 0 (first index on ties, -1 if
 *   none);  pan_own = sig[pan_idx] >= 0.5;   area[q] += #pixels with sig[q] >= 0.5.
 * The N x out_h x out_w sigmoid tensor never exists: each value is produced in registers as an MFMA B-operand element.
 *   masks (N, hm, wm) f32; cls_hi / cls_lo (ceil32(C) rounded to 32/96/160, Npad) bf16: class probabilities TRANSPOSED,
 *   zero padded, split as value = hi + lo (cls_lo unused and may be NULL for precision 1); pscore (Npad) f32 (<= 0: query
 *   not kept; padding -1); sem (C, out_h, out_w) f32; pan_idx (out_h, out_w) int32; pan_own (out_h, out_w) uint8;
 *   area (Npad) int32, zero-initialised by the caller.  Npad % 16 == 0, C <= 160.
 *   precision 0: bf16 hi+lo operands, 3 MFMAs per product (~2^-16);  1: plain bf16.
 */
int hipie_sem_pan(const float* masks, const void* cls_hi, const void* cls_lo, const float* pscore, float* sem,
                  int32_t* pan_idx, uint8_t* pan_own, int32_t* area, int N, int Npad, int C, int hm, int wm, int up,
                  int crop_h, int crop_w, int out_h, int out_w, int precision, void* stream);

/*
 * Sine embedding of reference points / boxes: the query_pos input of both DINO decoders.
 * Replaces: get_sine_pos_embed (models/deformable_detr/deformable_transformer_dino.py:636-670) == gen_sineembed_for_position
 *           (models/maskdino/utils/utils.py:74-100), ~21 eager launches per decoder layer.
 *   ref (n, ref_stride >= n_coord) f32, n_coord 2 | 4 coordinates (x, y[, w, h]);  dim_t (num_pos_feats) f32 = T^(2*floor(i/2)/F)
 *   (computed by the caller with the reference's formula);  out (n, n_coord * num_pos_feats) `out_dtype`, coordinate blocks in
 *   the reference's order (y, x, w, h);  value = sin | cos (even | odd feature) of ref * scale / dim_t, fp32.
 */
int hipie_sine_embed(const float* ref, const float* dim_t, void* out, int64_t n, int n_coord, int num_pos_feats, int ref_stride,
                     float scale, int out_dtype, void* stream);

/*
 * Iterative box refinement: out = sigmoid(delta + inverse_sigmoid(ref)), inverse_sigmoid with the reference's clamps (eps 1e-5).
 * Replaces: deformable_transformer_dino.py:502-520 / dino_decoder.py:150-160 + util/misc.py:493-497 (8 eager launches per layer).
 *   delta (n) `delta_dtype`, ref (n) f32, out (n) f32 (n = boxes * 4).
 */
int hipie_box_refine(const void* delta, const float* ref, float* out, int64_t n, float eps, int delta_dtype, void* stream);

/*
 * The linears of the path as one hand-written MFMA GEMM:   out = epilogue( alpha * A (M x K) . W^T + bias ),  W (N x K) as
 * torch.nn.Linear stores it.  Replaces: nn.Linear / F.linear of Attention.qkv / proj and Mlp.fc1 / fc2 (hipie/backbone/vit.py:
 * 67-83, 193-197, 212-230), BertLayer's dense layers (transformers BertModel via models/deformable_detr/bert_model.py:54-58), the
 * FFNs and projections of the deformable encoder / decoder layers (models/deformable_detr/deformable_transformer_dino.py:378-394,
 * 418-450; ops/modules/ms_deform_attn.py:95-99) -- which the reference runs in fp32.
 *   in_fmt   HIPIE_F16: A (M, K) and W (N, K) fp16, one MFMA per product;
 *            HIPIE_HL8: both operands split fp16 (rows of 2K fp16); the product is W_lo.A_hi + W_hi.A_lo + W_hi.A_hi with fp32
 *            accumulation = fp32-class results (every fp16 x fp16 product is exact in fp32; the dropped lo x lo term is 2^-22).
 *            HIPIE_F32: A (M, K) plain fp32 rows (lda in fp32 elements, a multiple of 4) against an HL8 W: the kernel splits the A
 *            fragments into hi / lo after the LDS read (an fp32 group of 8 takes the 32 bytes of an HL8 group) -- the same results
 *            as hipie_to_hl8 followed by the HL8 form, bit for bit, without the conversion launch.
 *   lda, ldw row strides in fp16 elements (multiples of 8);  K a multiple of 64 (F16) / 32 (HL8);  N a multiple of 8
 *   bias     (N) f32 or NULL;   resid (M, N) f32 with row stride ldr, or NULL
 *   epilogue y = alpha * acc + bias;  act 1: exact-erf GELU(y), 2: ReLU(y), 3: QuickGELU y * sigmoid(1.702 y) (the OpenAI CLIP towers of
 *            MaskCLIP, hipie/open_vocab/clip.py via open_clip);  y = (y + resid) * oscale
 *   out      (M, N) in out_fmt HIPIE_F32 | HIPIE_F16 | HIPIE_HL8 (row stride ldo in elements of that format; HL8: fp16 elements >= 2N):
 *            the HL8 form is directly the A operand of a following hipie_gemm.  out may alias resid (in-place residual update).
 *   out_row  (M) int32 or NULL: product row m is written to output row out_row[m] and takes its residual from resid row out_row[m];
 *            negative entries are dropped -- window_unpartition (hipie/backbone/utils.py:40-60) as the store index of the projection.
 * All pointers 16-byte aligned.  Deterministic (fixed accumulation order).
 */
int hipie_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
               void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt, int out_fmt, int act, float alpha,
               float oscale, void* stream);

/*
 * hipie_gemm with a DEVICE factor of alpha: y = (alpha * alpha_dev[0]) * acc + bias, everything else as hipie_gemm.  alpha_dev is read once
 * per workgroup; it is the 1 / s of hipie_grad_scale when A holds a gradient that was scaled by s (hipie_grad_pack), so the product leaves
 * un-scaled without a pass of its own.  alpha_dev NULL: hipie_gemm, the same dispatch and the same bits.  With the pointer the call never
 * goes to the thin-K kernel (which has no alpha); every tile kernel honours it.
 * Replaces: a separate `dx * inv` pass over the input gradient of torch.nn.functional.linear's backward.
 */
int hipie_gemm_scaled(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                      void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt, int out_fmt, int act, float alpha,
                      float oscale, const float* alpha_dev, void* stream);

/*
 * hipie_gemm (HIPIE_HL8 activations) with the two CROSS terms on block-scaled FP8 -- the opt-in `fp8x` precision policy:
 *     acc = W_hi . A_hi  +  q8(W_lo) . q8(A_hi)  +  q8(W_hi) . q8(A_lo)          fp32 accumulation
 * q8 = OCP e4m3 with one power-of-two (E8M0) scale per 32 k-elements: e = the largest integer with amax * 2^e <= 448 over the block (amax = 0:
 * e = 0, clamped to [-127, 127]), code = RNE e4m3fn(v * 2^e), scale byte = 127 - e (hipie_amd/fp8x.py is the exact host emulation).  The
 * cross terms run on v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 at twice the fp16 rate): 2 + 2 fp16-equivalent MFMA passes per 32 k instead of 6
 * (the 256 x 256 tile of hipie_gemm's kernel: the 320-column one does not fit the register file with the e4m3 operands beside it).
 * ~1e-5 relative against the exact product (three-product form: ~6e-7).  Replaces, under that policy, Mlp.fc2 of the ViT blocks
 * (hipie/backbone/vit.py:193-197), which the reference runs in fp32.
 *   A        HL8 rows as hipie_gemm's (in_fmt must be HIPIE_HL8); A's q8 is formed in the kernel, in registers
 *   W        the f8x weight format, (N, 2K) in fp16 units: each 32-element k slice of a row is 128 bytes, hi fp16 [64 B] then the e4m3
 *            codes [64 B] in the scaled MFMA's lane order, 8 bytes per (part, 8-group g):  lo g0, lo g2, hi g0, hi g2, lo g1, lo g3, hi g1, hi g3
 *            (hi, lo = the HL8 split of the fp32 weight; lo / hi here = q8(W_lo) / q8(W_hi); hipie_amd/fp8x.py pack_from_hl8)
 *   w_scale  (N, K/32, 2) uint8 E8M0 scales of the [lo, hi] e4m3 parts (contiguous)
 *   the rest as hipie_gemm: ldw >= 2K fp16 elements, K a multiple of 32, N of 8; bias, resid, epilogue, out_fmt, out_row (resid may alias out).
 * All pointers but w_scale 16-byte aligned.  Deterministic (fixed accumulation order).
 */
int hipie_gemm_f8x(const void* A, int64_t lda, const void* W, int64_t ldw, const void* w_scale, const float* bias, const float* resid,
                   int64_t ldr, void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt, int out_fmt, int act,
                   float alpha, float oscale, void* stream);

/*
 * HL8 rows -> q8 of their hi and lo parts with the device function hipie_gemm_f8x quantises its activations with (bit for bit the same codes):
 * x (rows, 2K) fp16 HL8, row stride ldx fp16 elements;  out (rows, 2K) bytes, row stride ldo BYTES (multiple of 16): per 32-element k block
 * [q8(hi) e4m3 32 B | q8(lo) e4m3 32 B];  scale (rows, K/32, 2) uint8 E8M0 [hi, lo], contiguous.  K a multiple of 32.  The weight packing of the
 * `fp8x` policy runs on it (hipie_amd/ops.py f8x_weight).
 */
int hipie_to_f8x(const void* x, int64_t ldx, void* out, int64_t ldo, void* scale, int64_t rows, int K, void* stream);

/*
 * hipie_gemm (split operands, N = 256) with the post-norm residual LayerNorm of the deformable encoder layer in its epilogue:
 *     y = LayerNorm_256( resid + alpha * A . W^T + bias ) * gamma + beta;   out = y as fp32 rows;  out_hl8 (or NULL) = y as HIPIE_HL8 rows
 * Replaces `src = norm1(src + dropout1(output_proj(msda)))` (models/deformable_detr/deformable_transformer_dino.py:387-389 with
 * ops/modules/ms_deform_attn.py:114) as ONE launch: N = 256 is one column tile, so the workgroup that owns 256 rows holds them whole and the
 * row statistics (two passes, fp32, as hipie_add_layernorm_dec) are two LDS exchanges away; the projection never exists in memory.
 * A in_fmt HIPIE_HL8 | HIPIE_F32 (lda as in hipie_gemm); W (256, 2K) HL8; bias (256) or NULL; resid (M, 256) fp32, required, may alias out
 * (every residual value of a row is read before any value of that row is stored); gamma, beta (256); ldo >= 256 (fp32 elements),
 * ldo_hl8 >= 512 (fp16 elements).  K a multiple of 32.  All pointers 16-byte aligned.
 */
int hipie_gemm_ln(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                  const float* gamma, const float* beta, float eps, float* out, int64_t ldo, void* out_hl8, int64_t ldo_hl8, int M, int K,
                  int in_fmt, float alpha, void* stream);

/*
 * hipie_gemm whose product row m READS operand row a_row[m] (0 <= a_row[m] < a_rows; A is a_rows x K; split formats only; the whole operand
 * below 4 GiB): the linears of the windowed ViT blocks run over the REAL tokens only and pick them out of / scatter them into (out_row) the
 * zero-padded window layout (window_partition pads 64 x 64 tokens to 70 x 70: 19.6 % more rows, whose qkv is the bias and whose projection
 * is discarded -- hipie/backbone/utils.py:16-60, hipie/backbone/vit.py:212-230).
 */
int hipie_gemm_gather(const void* A, int64_t lda, int64_t a_rows, const int32_t* a_row, const void* W, int64_t ldw, const float* bias,
                      const float* resid, int64_t ldr, void* out, int64_t ldo, const int32_t* out_row, int M, int N, int K, int in_fmt,
                      int out_fmt, int act, float alpha, float oscale, void* stream);

/*
 * hipie_vit_attn_rel on SPLIT operands (fp32-class logits): qkv (B, gh*gw, 3, heads, hd) as HIPIE_HL8 rows (2 * 3 * heads * hd fp16
 * per token) with the q rows pre-scaled by scale * log2(e); tab_h (2*gh-1, hd), tab_w (2*gw-1, hd) = the rel-pos tables / scale, HL8.
 * Scores and both bias terms are three-product sums (q_lo.k_hi + q_hi.k_lo + q_hi.k_hi), the probabilities one fp16, V both halves;
 * classic running maximum, fp32 row sums.  out (B, gh*gw, heads*hd) as HIPIE_HL8: the A operand of the projection hipie_gemm.
 * Replaces: Attention.forward between the qkv and proj Linears (hipie/backbone/vit.py:69-80) + add_decomposed_rel_pos / get_rel_pos
 * (hipie/backbone/utils.py:63-125) at the reference's fp32 accuracy.  Geometry: head_dim 64 | 80; 14-wide windows, grids up to 64 wide.
 */
int hipie_vit_attn_split(const void* qkv, const void* tab_h, const void* tab_w, void* out, int B, int gh, int gw, int heads,
                         int hd, void* stream);

/*
 * Fused attention for the TRAINING step's global ViT blocks: O = softmax(q' k'^T) v and its gradients, no (heads, N, N) tensor
 * in HBM.  Replaces Attention.forward between the qkv and proj Linears (hipie/backbone/vit.py:69-80) and its autograd, with
 * add_decomposed_rel_pos (hipie/backbone/utils.py:96-125) folded into the operands by the caller:
 *   q' = [scale q, rel_h(q, :), rel_w(q, :), 0..], k' = [k, onehot(key row), onehot(key column), 0..]   -- 224 columns; v, O: 80 columns
 * Every operand is an fp16 pair given as two planes (hi = fp16(x), lo = fp16(x - hi), row-major, contiguous); products are three fp16 MFMAs
 * accumulated in fp32 (the library's split form).  N a multiple of 128; BH = batch x heads <= 65535.
 *   forward:   q', k' (BH, N, 224) pairs, v (BH, N, 80) pair -> out (BH, N, 80) f32, lse (BH, N) f32 (log of the softmax denominator + row max)
 *   backward:  the same operands, v and dO (scaled by the caller into fp16's range) as (BH, N, 96) pairs (columns 80.. zero), lse, delta (BH, N)
 *              f32 = rowsum(dO * out) -> dq' (BH, N, 224) f32 (columns 80.. are d rel_h | d rel_w), dk (BH, N, 80) f32, dv (BH, N, 80) f32
 */
int hipie_attn_train_forward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                             void* out, void* lse, int BH, int N, void* stream);
/* fp32 rows (row stride ldx elements) -> the two fp16 planes (rows x Cp, contiguous) of an operand of the two entries below: hi = fp16(s x),
 * lo = fp16(s x - hi), columns C.. zero; s = *scale (a DEVICE float, e.g. the power of two that lifts dO into fp16's range) or 1 when NULL. */
int hipie_to_f16_pair(const void* x, int64_t ldx, void* hi, void* lo, int64_t rows, int C, int Cp, const void* scale, void* stream);
int hipie_attn_train_backward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                              const void* do_hi, const void* do_lo, const void* lse, const void* delta, void* dq, void* dk, void* dv,
                              int BH, int N, void* stream);

/* The short-sequence instance of the two entries above (csrc/attn_train_win.hip; the same kernels, csrc/attn_train_tile.h, built for 128
 * operand columns, two tiles per wave and ragged items): the attention of the WINDOWED ViT blocks of the training
 * step -- Attention.forward, hipie/backbone/vit.py:69-80, with add_decomposed_rel_pos (hipie/backbone/utils.py:96-125) folded into the operands
 * -- over items of N tokens, 1 <= N <= 256, one (window, head) each, dense in memory (no row padding), one workgroup per item.
 *   q', k' (BH, N, 128) pairs (a 14 x 14 window has 80 + 14 + 14 live columns, the rest zero); v (BH, N, 80) pair; same arithmetic as above.
 *   forward:   -> out (BH, N, 80) f32, lse (BH, N) f32
 *   backward:  v and dO (scaled by the caller into fp16's range) as (BH, N, 96) pairs, lse, delta (BH, N) f32 = rowsum(dO * out)
 *              -> dq' (BH, N, 128) f32, dk (BH, N, 80) f32, dv (BH, N, 80) f32
 * Rows beyond N exist only inside the kernels: keys >= N get probability exactly 0 (masked by index), rows >= N are neither read as data nor
 * written.  HIPIE_EINVAL without a launch for N < 1, N > 256, BH < 1 or a null pointer. */
int hipie_attn_train_win_forward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                                 void* out, void* lse, int BH, int N, void* stream);
int hipie_attn_train_win_backward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                                  const void* do_hi, const void* do_lo, const void* lse, const void* delta, void* dq, void* dk, void* dv,
                                  int BH, int N, void* stream);

/*
 * The operand pack / unpack passes around the four entries above (csrc/attn_pack.hip), which make the attention of a ViT block of the training
 * step ONE node from the qkv rows to the token-major output: what Attention.forward (hipie/backbone/vit.py:67-83) and add_decomposed_rel_pos
 * (hipie/backbone/utils.py:96-125) do between the qkv Linear and the attention product -- the reshape / permute / unbind of qkv, the scale,
 * the two concatenations -- and what autograd does to undo them.  Shared geometry: B images or windows, heads, an H x W grid, N = H W rows per
 * (image, head) item, head width 80; the planes hold Np rows per item: Np = N, or N rounded up to 128 (the padded form: padding keys are
 * masked through operand column cq = 80 + H + W, which is 1 in q' on real rows and -30000 in k' on padding rows; padding rows are zero
 * otherwise); cols = 224 (csrc/attn_train.hip) | 128 (csrc/attn_train_win.hip) operand columns.  Planes are the fp16 pairs of hipie_to_f16_pair,
 * bit for bit.  Every pointer 16-byte aligned.  HIPIE_EINVAL without a launch for a null pointer, a non-positive size, another cols, an Np that
 * is neither of the two, 80 + H + W (+ 1 when padded) > cols, or a misaligned operand.
 *   pack_kv:     qkv (B, N, 3, heads, 80) f32 -> rq (B heads, N, 80) f32, the head-major q; the k' pair (B heads, Np, cols): [k | onehot(n / W) |
 *                onehot(n % W) | 0..]; the v pair (B heads, Np, 80)
 *   pack_q:      rq, rel_h (B heads, H, W, H) and rel_w (B heads, H, W, W) f32 given with their four ELEMENT strides (whatever layout the
 *                library product left) -> the q' pair (B heads, Np, cols): [rq * qscale | rel_h | rel_w | 0..]
 *   grad_amax:   max |go| over n f32 values (n a multiple of 4) -> one device float; the bits of a max reduction in any order
 *   pack_grad:   go (B, N, heads, 80) f32 token-major, out (B heads, Np, 80) f32, the 80-wide v pair, scale (device float) -> the dO pair
 *                (B heads, Np, 96) of scale * go, the v pair (B heads, Np, 96), columns 80.. zero; delta (B heads, Np) f32 = scale * sum_c go * out
 *                in a fixed order; padding rows zero
 *   unpack_grad: dq' (B heads, Np, cols), dk, dv (B heads, Np, 80) f32; dq_h and dq_w (dq_w may be NULL), the rel-pos terms of dq as
 *                (B heads, H, W, 80) f32 with three element strides each (multiples of 4; the 80 columns contiguous); inv (device float)
 *                -> dqkv (B, N, 3, heads, 80) f32: q = (dq'[:80] * qscale + dq_h + dq_w) * inv, k = dk * inv, v = dv * inv; rows >= N are dropped
 */
int hipie_attn_pack_kv(const void* qkv, void* rq, void* k_hi, void* k_lo, void* v_hi, void* v_lo, int B, int heads, int H, int W, int Np, int cols,
                       void* stream);
int hipie_attn_pack_q(const void* rq, const void* rel_h, int64_t hs_b, int64_t hs_h, int64_t hs_w, int64_t hs_k, const void* rel_w, int64_t ws_b,
                      int64_t ws_h, int64_t ws_w, int64_t ws_k, void* q_hi, void* q_lo, int B, int heads, int H, int W, int Np, int cols, float qscale,
                      void* stream);
int hipie_attn_grad_amax(const void* go, int64_t n, void* amax, void* stream);
int hipie_attn_pack_grad(const void* go, const void* out, const void* v_hi, const void* v_lo, const void* scale, void* do_hi, void* do_lo,
                         void* v96_hi, void* v96_lo, void* delta, int B, int heads, int H, int W, int Np, void* stream);
int hipie_attn_unpack_grad(const void* dq, const void* dk, const void* dv, const void* dq_h, int64_t hs_b, int64_t hs_h, int64_t hs_w,
                           const void* dq_w, int64_t ws_b, int64_t ws_h, int64_t ws_w, const void* inv, void* dqkv, int B, int heads, int H, int W,
                           int Np, int cols, float qscale, void* stream);

/* dst + rows[i] * ld_bytes <- the row_bytes bytes at src_row, for i < n_rows (negative entries are skipped): one constant row into a
 * listed set of rows.  Used to write the HL8 qkv BIAS row into the padding rows of a window-layout qkv buffer -- the qkv of a padding token
 * of window_partition is the bias, its LayerNorm output being zero (hipie/backbone/utils.py:29-37, vit.py:67-71).  16-byte units. */
int hipie_fill_rows(void* dst, int64_t ld_bytes, const int32_t* rows, int64_t n_rows, const void* src_row, int64_t row_bytes, void* stream);

/* rows of `x_dtype` (HIPIE_F32 | HIPIE_F16) values -> HIPIE_HL8 rows of scale * x (K a multiple of 8; ldx in elements of x, ldo in
 * fp16 elements >= 2K): the generic producer of split operands (the LayerNorm / GEMM epilogues emit HL8 directly). */
int hipie_to_hl8(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t rows, int K, int x_dtype, float scale, void* stream);

/* x (rows x C fp32 values, row stride ldx elements) -> out (C x 2 rows_p) HIPIE_HL8 rows of scale * x^T: the transpose as a split operand in ONE
 * pass (a strided transpose copy + hipie_to_hl8 otherwise), columns rows <= m < rows_p zero (rows_p a multiple of 8; 32 for a GEMM operand).
 * The producer of both operands of the weight gradient dW = dy^T . x of a Linear (torch.nn.functional.linear's backward in the reference's
 * training step, hipie/backbone/vit.py:67-83 and every other Linear): the contraction runs over the token rows. */
int hipie_to_hl8_t(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t rows, int C, int64_t rows_p, float scale, void* stream);

/*
 * Scaled gradient operands of the training linears (csrc/grad_pack.hip; the opt-in backend group "scaled_grads"): the output gradient dy of
 * a Linear is multiplied by a power of two s chosen ON THE DEVICE before it is split into fp16 pairs, and the products are multiplied by 1 / s
 * where they are written.  The raw split is 2^-22 accurate only while dy is a normal fp16 number (6.1e-5 .. 65504); with s the accuracy
 * does not depend on the magnitude of dy.  No host wait, no floating-point atomic, the same bits on every call.
 *
 * hipie_grad_scale:  x (rows, N) f32, row stride ldx (N and ldx multiples of 4, 16-byte aligned) -> scale = {s, 1 / s} (two device floats,
 *   8-byte aligned): s = 2^e with max|x| * 2^e in [2^14, 2^15), e taken from the exponent bits of the maximum (an integer maximum of the bit
 *   patterns) and clamped to +-126 so that both floats are normal; max|x| == 0, inf or NaN: {1, 1}.
 *   Replaces: the torch.exp2(torch.floor(torch.log2(...))) chain the attention nodes form their scale with (training/functions.py).
 * hipie_grad_pack:  ONE pass over dy (rows, N) f32 (row stride ldx; N a multiple of 8) that reads scale[0] = s and writes, each unless NULL,
 *   out_rows (rows, 2 N) HL8 of s dy, row stride ldo: the A operand of dx = dy . W, the bits of hipie_to_hl8(dy, scale = s);
 *   out_t    (N, 2 rows_p) HL8 of (s dy)^T, row stride ldt, columns rows <= m < rows_p zero (rows_p a multiple of 32): the operand of
 *            dW = dy^T . x, the bits of hipie_to_hl8_t(dy, scale = s);
 *   dbias    (N) f32 = sum over the rows of the UNSCALED dy: per-tile column sums in ws (hipie_grad_pack_ws_bytes(rows_p, N) bytes), added in
 *            tile order.  dbias and ws come together.
 *   Replaces: the three readers of dy in torch.nn.functional.linear's backward on the split GEMM -- the in-kernel split of hipie_gemm's
 *   HIPIE_F32 rows, hipie_to_hl8_t and dy.sum(0) (hipie/backbone/vit.py:67-83, 193-197 and every other big Linear of the step).
 * hipie_splitk_finish:  out (n) f32 = (part[0] + part[1] + .. + part[nk - 1]) * alpha_dev[0], part (nk, n) f32 the partial products of one
 *   hipie_gemm_batched launch over chunks of the contraction, added in chunk order; alpha_dev NULL: 1.  n a multiple of 4, nk <= 64.
 *   Replaces: part.sum(0) behind the split-K weight gradient, and the multiplication by 1 / s.
 */
int hipie_grad_scale(const void* x, int64_t ldx, int64_t rows, int N, void* scale, void* stream);
int64_t hipie_grad_pack_ws_bytes(int64_t rows_p, int N);
int hipie_grad_pack(const void* dy, int64_t ldx, const void* scale, void* out_rows, int64_t ldo, void* out_t, int64_t ldt, void* dbias, void* ws,
                    int64_t rows, int N, int64_t rows_p, void* stream);
int hipie_splitk_finish(const void* part, int nk, int64_t n, const float* alpha_dev, void* out, void* stream);

/*
 * Half-precision operands of the training linears (csrc/half_pack.hip; the opt-in precision policy net.half_policy): ONE fp16 MFMA product
 * per GEMM instead of the three of the split GEMM, fp32 master weights, fp32 accumulation and output.  Arithmetic contract of a linear
 * y = x . W^T + b:  x16 = fp16(x), W16 = fp16(W), round to nearest even, values beyond +-65504 saturate (as the split's hi does), no scale on
 * activations or weights;  y = x16 . W16^T + b (hipie_gemm, HIPIE_F16);  {s, 1 / s} = hipie_grad_scale(dy), g16 = fp16(s dy);
 * dx = (1 / s) g16 . W16 (hipie_gemm_scaled, HIPIE_F16);  dW = (1 / s) g16^T . x16^T over the token rows padded to 64, in chunks
 * (hipie_gemm_batched_f16) added in chunk order (hipie_splitk_finish);  db = column sums of the unscaled dy.  All scale factors are exact
 * powers of two and every sum has a fixed order: the results for 2^e dy are 2^e times the results for dy, bit for bit.  Relative accuracy
 * 2^-11 per operand, NOT the fp32 class of the split GEMM.
 *
 * hipie_half_pack:  ONE pass over x (rows, N), x_fmt HIPIE_F32 | HIPIE_F16 rows with row stride ldx (elements; 16-byte pieces), N a multiple
 *   of 8.  scale: the device block of hipie_grad_scale (s = scale[0]) or NULL: s = 1.  Writes, each unless NULL,
 *   out_rows (rows, N) fp16 of s x, row stride ldo;
 *   out_t    (N, rows_p) fp16 of (s x)^T, row stride ldt, columns rows <= m < rows_p zero, rows_p a multiple of 64 (the F16 k tile);
 *   dbias    (N) f32 = sum over the rows of the UNSCALED x: per-tile column sums in ws (hipie_half_pack_ws_bytes(rows_p, N) bytes), added in
 *            tile order, the order of hipie_grad_pack.  dbias and ws come together.
 *   All three NULL: nothing is launched.  Refused (HIPIE_EINVAL, nothing launched): N % 8, rows_p % 64 or < rows, strides below the row
 *   length or off 16-byte pieces, x / out_rows / out_t off a 16-byte boundary.
 *   Replaces: the readers of dy in torch.nn.functional.linear's backward under autocast -- the fp16 cast of dy, its transposed copy and
 *   dy.sum(0) -- and the casts of x and of the recomputed activation (hipie/backbone/vit.py:67-83, 193-197;
 *   models/deformable_detr/deformable_transformer_dino.py:384-394).
 * hipie_act_half:  a16 (rows, N) fp16 = fp16(act(u)), u (rows, N) f32 dense rows, N a multiple of 8, act 1 = GELU | 2 = ReLU: the value
 *   hipie_act_forward writes, rounded once -- the fp16 operand of the second linear without an fp32 activation in HBM.
 *   Replaces: nn.GELU() / ReLU followed by the autocast cast in front of fc2 / linear2 (hipie/backbone/vit.py:193-197,
 *   models/deformable_detr/deformable_transformer_dino.py:384-394).
 */
int64_t hipie_half_pack_ws_bytes(int64_t rows_p, int N);
int hipie_half_pack(const void* x, int64_t ldx, int x_fmt, const void* scale, void* out_rows, int64_t ldo, void* out_t, int64_t ldt, void* dbias,
                    void* ws, int64_t rows, int N, int64_t rows_p, void* stream);
int hipie_act_half(const void* u, void* a16, int64_t rows, int N, int act, void* stream);

/*
 * The map-to-rows pack of the training projections (csrc/patch_pack.hip; the opt-in backend group "projections"): a convolution whose
 * kernel equals its stride, and a transposed one, are linears over patch rows plus a layout change; this entry does the layout change
 * once, as the producer of the split GEMM's operands.
 *
 * hipie_patch_pack:  ONE pass over the fp32 map x of logical shape (B, C, H, W) with the element strides (sb, sc, sh, sw) -- NCHW-dense and
 *   channels-last maps are read in place -- and the patch size k (any k <= 64 that divides H and W).  Patch row m = (b H/k + h) W/k + w,
 *   column n = c k^2 + i k + j holds x[b, c, h k + i, w k + j]: M = B (H/k) (W/k) rows of N = C k^2 columns, the column order of
 *   weight.reshape(Cout, Cin k k) of a convolution and of weight.view(Cin, Cout k k) of a transposed one.  scale: the device block of
 *   hipie_grad_scale (s = scale[0]) or NULL: s = 1.  Writes, each unless NULL,
 *   out_f32  (M, N) f32 rows, row stride ldf: the A operand of the forward GEMM of a map that is not channels-last;
 *   out_rows (M, 2 N) HL8 of s x, row stride ldo: the bits of hipie_to_hl8 of the gathered rows with scale = s;
 *   out_t    (N, 2 rows_p) HL8 of (s x)^T, row stride ldt, columns M <= m < rows_p zero (rows_p a multiple of 32): the bits of hipie_to_hl8_t;
 *   dsum     (C) f32 = per-CHANNEL sums of the UNSCALED values over all pixels: per-tile column sums in ws
 *            (hipie_patch_pack_ws_bytes(rows_p, N) bytes; ws_bytes = what the caller has), added in tile order and, per channel, in column
 *            order: no floating-point atomic, the same bits on every call.  dsum and ws come together.
 *   All outputs NULL: nothing is launched (HIPIE_OK).  Refused (HIPIE_EINVAL with a hipie_last_error() text, nothing launched): a NULL x,
 *   N % 8, k not dividing H or W, rows_p % 32 or rows_p < M, a map whose unit stride is neither that of W nor that of C, output pointers or
 *   strides off 16 bytes (or below the row length), dsum without ws or ws without dsum, a workspace that is too small.
 *   Replaces: the .permute / .contiguous copies around F.conv2d / F.conv_transpose2d whose kernel equals its stride, the transposed copies
 *   and the channel sums of the backward of torch's conv2d and conv_transpose2d at those sites -- PatchEmbed.proj and the simple feature
 *   pyramid's ConvTranspose2d (backbone/vit.py:357-374), the 1 x 1 input_proj of both heads (models/ddetrs_dn.py:271-320,
 *   maskdino/pixel_decoder/maskdino_encoder.py:368-434), adapter_1 and mask_features of the pixel decoder (ibid.).
 */
int64_t hipie_patch_pack_ws_bytes(int64_t rows_p, int N);
int hipie_patch_pack(const void* x, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int k, const void* scale,
                     void* out_f32, int64_t ldf, void* out_rows, int64_t ldo, void* out_t, int64_t ldt, int64_t rows_p, void* dsum, void* ws,
                     int64_t ws_bytes, void* stream);

/*
 * hipie_gemm_batched for PLAIN fp16 operands (HIPIE_F16 rows of K elements, K a multiple of 64: one product per k tile), fp32 output, with
 * the device factor of hipie_gemm_scaled (alpha_dev, NULL: 1): the batched launch of the tile instances hipie_gemm runs for HIPIE_F16, so a
 * problem of the batch has the bits of the hipie_gemm call on its operands.  Offsets in elements as hipie_gemm_batched (A / W: fp16, out: fp32).
 * Replaces: the per-chunk launches and the `* inv` pass of the split-K weight gradient dW = dy^T . x of torch.nn.functional.linear's
 * backward in half precision (hipie/backbone/vit.py:67-83 and every other big Linear of the step).
 */
int hipie_gemm_batched_f16(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                           int64_t w_inner, void* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner, int M, int N,
                           int K, float alpha, const float* alpha_dev, void* stream);

/*
 * hipie_gemm on n_outer x n_inner independent problems in ONE launch (split-fp16 HL8 operands only, no bias / residual / activation):
 * problem (o, i) reads A + o * a_outer + i * a_inner (fp16 elements), W + o * w_outer + i * w_inner, writes out + o * o_outer +
 * i * o_inner (elements of out_fmt: fp32, or fp16 units for HL8).  Used for the image -> text direction of the vision-language fusion
 * in the split policy: per (image, head)  S = Q_h . K_h^T  and  out_h = P_h . V_h  (models/deformable_detr/fuse_helper.py:77-121).
 * n_outer * n_inner <= 65535; offsets keep 16-byte alignment.
 */
int hipie_gemm_batched(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                       int64_t w_inner, void* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner, int M, int N,
                       int K, int out_fmt, float alpha, void* stream);

/*
 * hipie_gemm_batched whose epilogue is the masked row softmax (N <= 256: the whole row is one column tile) -- the logits of the image -> text
 * fusion attention never reach HBM:  P[b][h] = softmax_j( clamp(alpha * A . W^T, +-clamp) over the columns j < L with mask[b][j] ) written as
 * HIPIE_HL8 (the A operand of the P . V product that follows); masked and padding columns (L <= j < N) are 0, a row without a valid column is 0.
 * mask (n_outer, L) uint8 or NULL.  Replaces hipie_gemm_batched(F32 out) + hipie_softmax_hl8 for texts of up to 256 tokens
 * (attn_weights_v of BiMultiHeadAttention.forward, models/deformable_detr/fuse_helper.py:77-111).
 */
int hipie_gemm_batched_softmax(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                               int64_t w_inner, void* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner, int M,
                               int N, int K, const unsigned char* mask, int L, float clamp, float alpha, void* stream);

/*
 * The image -> text direction of BiMultiHeadAttention (models/deformable_detr/fuse_helper.py:62-139) with the two visual-side projections
 * FOLDED into the text side, so that nothing of width embed_dim (2048) is ever computed per visual token:
 *     logits[b,h][i,j] = (W_q,h x_i + b_q,h) . k_{b,j,h} = x_i . M_{b,h,j} + c_{b,h,j},      M = k_h W_q,h  (L x 256),  c = k_h . b_q,h
 *     out_v[b][i]      = W_o concat_h( P_h[i,:] V_h ) + b_o = sum_h P_h[i,:] . U_{b,h} + b_o,   U = V_h W_o,h^T  (L x 256)
 * hipie_gemm_batched_softmax_bias: hipie_gemm_batched_softmax with col_bias (n_outer * n_inner, N) fp32 added to the scaled accumulator BEFORE
 * the clamp (the reference clamps q . k including the bias); A may be shared by the inner index (a_inner = 0: every head reads x).
 * hipie_gemm_batched_resid: hipie_gemm_batched (fp32 out) with hipie_gemm's bias (shared) and residual epilogue; resid moves with the
 * problem index like out (r_outer / r_inner in fp32 elements).  One launch each per fusion layer.
 */
int hipie_gemm_batched_softmax_bias(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                                    int64_t w_inner, void* out, int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner,
                                    int M, int N, int K, const unsigned char* mask, int L, const float* col_bias, float clamp, float alpha,
                                    void* stream);
int hipie_gemm_batched_resid(const void* A, int64_t lda, int64_t a_outer, int64_t a_inner, const void* W, int64_t ldw, int64_t w_outer,
                             int64_t w_inner, const float* bias, const float* resid, int64_t ldr, int64_t r_outer, int64_t r_inner, float* out,
                             int64_t ldo, int64_t o_outer, int64_t o_inner, int n_outer, int n_inner, int M, int N, int K, float alpha,
                             void* stream);

/*
 * Row softmax of fp32 logits written as an HL8 operand:  P[r, :Lp] = softmax over the L valid columns of clamp(S[r, :L], +-clamp) with
 * columns masked by mask[r / rows_per_batch, :] (uint8, 1 = keep; NULL = all) or beyond L set to 0.  S rows lds floats apart, P rows
 * ldp fp16 elements apart (>= 2 * Lp);  Lp a multiple of 8, <= 4096.  A row with no valid column gives zeros (DEVIATION, never reached
 * on the path: the reference's additive -9e15 mask makes such a row a UNIFORM average over all L columns; a caption always keeps [CLS]
 * and [SEP], so every text has valid tokens -- same convention in hipie_attn_f32 / hipie_attn_split / hipie_flash_attn).
 * Replaces: attn_weights_v = softmax(clamp(attn_weights) + attention_mask) of BiMultiHeadAttention.forward (fuse_helper.py:97-111).
 */
int hipie_softmax_hl8(const float* S, int64_t lds, void* P, int64_t ldp, int64_t rows, int L, int Lp, const unsigned char* mask,
                      int64_t rows_per_batch, float clamp, void* stream);

/*
 * EXACT fp32 softmax attention for the small attentions of the path (fp32 operands, fp32 FMA products, fp32 softmax):
 *     out[b,i,h,:] = softmax_j( scale * q[b,i,h,:].k[b,j,h,:] + (key_mask[b,j] ? 0 : -inf) ) . v[b,j,h,:]
 * q, k, v fp32 with element strides (batch, token); head h is the head_dim contiguous elements at h * head_dim (so the three may be
 * column blocks of ONE projection output); out (B, Nq, H * head_dim) fp32 contiguous; head_dim 32 | 64; key_mask (B, Nk) uint8 or NULL
 * (a row whose keys are all masked gives zeros).  Deterministic.
 * Replaces: BertSelfAttention's matmul -> softmax -> matmul (transformers, behind models/deformable_detr/bert_model.py:54-58) and
 *           nn.MultiheadAttention's core in the decoder layers (models/deformable_detr/deformable_transformer_dino.py:418-432,
 *           models/maskdino/transformer_decoder/dino_decoder.py:222-240), which the reference computes in fp32.
 */
int hipie_attn_f32(const float* q, const float* k, const float* v, const unsigned char* key_mask, float* out, int B, int H, int Nq, int Nk,
                   int head_dim, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, float scale,
                   void* stream);

/*
 * hipie_attn_f32 with a mask per QUERY row: query_mask (B, Nq, Nk) uint8, 1 = row i may attend to key j (NULL = all).  The mask tokens of
 * MaskCLIP: every mask token sees only the image patches its mask covers, plus the class token.
 * Replaces: the attn_mask path of open_clip's ResidualAttentionBlock as the reference's MaskCLIP drives it (hipie/clip.py:158-215, :249-262) --
 * logits, masked_fill(-inf), softmax, P . V of the mask tokens' rows (hipie_amd/open_vocab.py: ResidualAttentionBlock.forward_mask_rows).
 */
int hipie_attn_f32_rows(const float* q, const float* k, const float* v, const unsigned char* query_mask, float* out, int B, int H, int Nq,
                        int Nk, int head_dim, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, float scale,
                        void* stream);
/* the same on the matrix pipe at fp32-class accuracy (the arithmetic of hipie_attn_split; what the product runs: one thread per query row of the
 * exact kernel is 0.83 ms per layer at 150 mask tokens per image, this one 0.05 ms) */
int hipie_attn_split_rows(const float* q, const float* k, const float* v, const unsigned char* query_mask, float* out, int B, int H, int Nq,
                          int Nk, int head_dim, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, float scale,
                          void* stream);

/*
 * The same attention (same operands, same output, same mask semantics) on the matrix pipe at fp32-CLASS accuracy: q (pre-multiplied by
 * scale * log2 e), k, v are split in the kernel into fp16 pairs (22 mantissa bits), logits = three-product sums with fp32 accumulation, the
 * probabilities an fp16 pair, O += V_hi.(P_hi + P_lo) + V_lo.P_hi -- the arithmetic of hipie_vit_attn_split.  Within 2e-6 of
 * hipie_attn_f32; what the split policy runs (27 launches per step: 4.4 -> ~1 ms).  Replaces: the same reference code as hipie_attn_f32.
 */
int hipie_attn_split(const float* q, const float* k, const float* v, const unsigned char* key_mask, float* out, int B, int H, int Nq, int Nk,
                   int head_dim, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, float scale,
                   void* stream);

/*
 * hipie_attn_f32 for the TRAINING step: the decoders' query self-attention (q = k rows, Nq = Nk = N, head_dim 32) with the log-sum-exp of
 * every row as a second output and a mask per (query, key) pair.  Exact fp32 FMA chains in a fixed order, no atomics: deterministic.
 *   qk (B, N, 2 H 32) f32 rows of the q | k in-projection: q of head h at column h * 32, k at H * 32 + h * 32; batch / row strides
 *   qk_sb / qk_st in elements;  v (B, N, H 32) f32 rows, strides v_sb / v_st (both may be column blocks of wider buffers);
 *   blocked (N, N) uint8, 1 = query i may NOT see key j (torch's attn_mask convention: a bool tensor's own storage), image b's mask at
 *   blocked + b * mask_sb (0: one mask for every image and head); NULL = no mask;
 *   out (B, N, H 32) f32 contiguous = softmax_j(scale q_i . k_j) v_j;  lse (B, H, N) f32 = max_j s_ij + log2 sum_j 2^(s_ij - max) with
 *   s = scale * log2(e) * q . k, i.e. in log2 units.  A row with every key blocked gives zeros and lse = -inf.
 * Refused (HIPIE_EINVAL, nothing launched): null pointers, head_dim != 32, B, H or N < 1, qk / v / out off a 16-byte boundary, strides
 * that are no multiple of 4, a row stride below the row's width.
 * Replaces: the forward of nn.MultiheadAttention's core under torch.autograd in the decoder layers -- scale, masked_fill(attn_mask, -inf),
 *           softmax, two batched products and the (B, 8, N, N) logits and probabilities they keep
 *           (models/deformable_detr/deformable_transformer_dino.py:418-436, models/maskdino/transformer_decoder/dino_decoder.py:222-248).
 */
int hipie_attn_f32_train_forward(const float* qk, const float* v, const unsigned char* blocked, float* out, float* lse, int B, int H, int N,
                                 int head_dim, int64_t qk_sb, int64_t qk_st, int64_t v_sb, int64_t v_st, int64_t mask_sb, float scale,
                                 void* stream);

/*
 * Backward of hipie_attn_f32_train_forward in two passes that recompute the probabilities from lse: nothing of N x N elements is read or
 * written.  p_ij = 2^(s_ij - lse_i) with s from the forward's own chains, delta_i = d_out_i . out_i, dp_ij = d_out_i . v_j,
 * ds_ij = p_ij (dp_ij - delta_i):
 *   pass 1, one thread per query row:  d_qk[b, i, h * 32 ..]         = scale sum_j ds_ij k_j, and delta into the workspace;
 *   pass 2, one thread per key row:    d_qk[b, j, H * 32 + h * 32 ..] = scale sum_i ds_ij q_i,  d_v[b, j, h * 32 ..] = sum_i p_ij d_out_i,
 *   summed in query order.  d_qk (B, N, 2 H 32) and d_v (B, N, H 32) f32 contiguous, every element overwritten.
 *   qk, v, blocked, out, lse, the strides and scale: the forward's;  d_out (B, N, H 32) f32 with strides do_sb / do_st.
 *   d_qk NULL (frozen q | k rows): pass 1 and the dK half of pass 2 are skipped;  d_v NULL: the dV half;  both NULL: nothing is launched.
 *   ws: at least hipie_attn_f32_train_backward_ws_bytes(B, H, N) bytes = (B, H, N) floats.
 * A row with lse = -inf contributes exactly zero to every gradient.  Fixed order of the additions, no atomics: bit-reproducible.
 * Refused (HIPIE_EINVAL, nothing launched): what the forward refuses, d_out / d_qk / d_v off a 16-byte boundary, do_sb / do_st no
 * multiple of 4, a workspace that is too small (the message names the size needed).
 * Replaces: torch.autograd through the same code -- the softmax backward over the saved (B, 8, N, N) probabilities, four batched products,
 *           the transposing copies and the zero-filled slice gradients of the three in-projection slices
 *           (models/deformable_detr/deformable_transformer_dino.py:418-436, models/maskdino/transformer_decoder/dino_decoder.py:222-248).
 */
int hipie_attn_f32_train_backward(const float* qk, const float* v, const unsigned char* blocked, const float* out, const float* lse,
                                  const float* d_out, float* d_qk, float* d_v, void* ws, int64_t ws_bytes, int B, int H, int N, int head_dim,
                                  int64_t qk_sb, int64_t qk_st, int64_t v_sb, int64_t v_st, int64_t mask_sb, int64_t do_sb, int64_t do_st,
                                  float scale, void* stream);
int64_t hipie_attn_f32_train_backward_ws_bytes(int B, int H, int N);

/*
 * The core of the vision-language fusion attention for the TRAINING step, both directions in one call, exact fp32 on the f32-input MFMA
 * (bitwise fmaf chains in a fixed order, no atomics: deterministic), with the block's attention dropout.  Head width 256, L <= 256.
 *   q, vv (B, Nv, H 256) f32 rows of v_proj (UNSCALED: scale = 256^-0.5 is applied here) and values_v_proj; k, vl (B, L, H 256) f32 rows
 *   of l_proj and values_l_proj; head h at column h * 256; batch / row strides *_sb / *_st in elements (column blocks of wider buffers
 *   are read in place);  att (B, L) uint8, 1 = attended text token.
 *   raw_ij = scale q_i . k_j, s_ij = clamp(raw_ij, -50000, 50000);  pv = softmax of s over the ATTENDED j (0 elsewhere);  pl = softmax of s
 *   over ALL i per column j (no mask);  out_v (B, Nv, H 256) = sum_j pv_ij kv_ij vl_j;  out_l (B, L, H 256) = sum_i pl_ij kl_ij vv_i.
 *   kv, kl: dropout keep factors, 0 or 1 / (1 - dropout), from a stateless hash of (seed, direction, b, h, i, j) -- the same function in
 *   the forward and the backward, independent of the launch geometry; not torch's random stream.  dropout = 0 keeps everything.
 *   lse_v (B, H, Nv) and lse_l (B, H, L): log-sum-exp of the rows / columns in LOG2 units (s * log2 e);  stat_v (B, H, Nv, 2) and
 *   stat_l (B, H, L, 2): the same as a pair (maximum, log2 of the sum of 2^(s - maximum)) -- what the backward reads: a clamped row's
 *   logits are 72135 in log2 units, where a single float's ulp of 0.008 would cost 0.5 % in every probability.
 *   An image with NO attended token is outside the contract: out_v = 0, lse_v = -inf, and its image -> text direction gives zero gradient.
 *   ws: at least hipie_bi_attn_train_forward_ws_bytes(B, H, Nv, L) bytes: the partial column statistics and out_l rows of at most 8
 *   segments of the visual rows, folded in segment order.  Nothing of Nv x L elements is written.
 * Refused (HIPIE_EINVAL, nothing launched): null pointers, head_dim != 256, L outside 1 .. 256, B, H or Nv < 1, pointers off a 16-byte
 * boundary, strides that are no multiple of 4, a row stride below the row's width, dropout outside [0, 1), a workspace that is too small.
 * Replaces: the forward of BiMultiHeadAttention.forward between the four input and two output projections under torch.autograd -- two
 *           batched products, four clamps, a max, two softmaxes, the int64 mask, two dropouts and the dozen (B 8, Nv, L) tensors they
 *           keep (models/fuse_helper.py:54-139).
 */
int hipie_bi_attn_train_forward(const float* q, const float* k, const float* vv, const float* vl, const unsigned char* att, float* out_v,
                                float* out_l, float* lse_v, float* lse_l, float* stat_v, float* stat_l, void* ws, int64_t ws_bytes, int B,
                                int H, int Nv, int L, int head_dim, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t vv_sb,
                                int64_t vv_st, int64_t vl_sb, int64_t vl_st, double dropout, int64_t seed, void* stream);
int64_t hipie_bi_attn_train_forward_ws_bytes(int B, int H, int Nv, int L);

/*
 * Backward of hipie_bi_attn_train_forward; the probabilities of both directions are recomputed from stat_v / stat_l with the forward's
 * own logit chains and keep function.  With dv_i = d_out_v_i . out_v_i and dl_j = d_out_l_j . out_l_j:
 *   ds_ij = (pv_ij (kv_ij d_out_v_i . vl_j - dv_i) + pl_ij (kl_ij vv_i . d_out_l_j - dl_j)) [|raw_ij| <= 50000]
 *   d_q_i = scale sum_j ds_ij k_j,  d_k_j = scale sum_i ds_ij q_i,  d_vl_j = sum_i pv_ij kv_ij d_out_v_i,  d_vv_i = sum_j pl_ij kl_ij d_out_l_j
 *   d_q, d_vv (B, Nv, H 256) and d_k, d_vl (B, L, H 256) f32 contiguous, every element overwritten;  d_out_v (B, Nv, H 256) and
 *   d_out_l (B, L, H 256) f32 with strides dov_* / dol_*.  A NULL gradient pointer skips the work that serves only it; all four NULL:
 *   nothing is launched.  The sums over the visual rows run per segment in row order, the segments are folded in order: bit-reproducible.
 *   ws: at least hipie_bi_attn_train_backward_ws_bytes(B, H, Nv, L) bytes.
 * Refused (HIPIE_EINVAL, nothing launched): what the forward refuses, gradients off a 16-byte boundary, dov_* / dol_* no multiple of 4,
 * a workspace that is too small (the message names the size needed).
 * Replaces: torch.autograd through the same code (models/fuse_helper.py:54-139).
 */
int hipie_bi_attn_train_backward(const float* q, const float* k, const float* vv, const float* vl, const unsigned char* att,
                                 const float* out_v, const float* out_l, const float* stat_v, const float* stat_l, const float* d_out_v,
                                 const float* d_out_l, float* d_q, float* d_k, float* d_vv, float* d_vl, void* ws, int64_t ws_bytes, int B,
                                 int H, int Nv, int L, int head_dim, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t vv_sb,
                                 int64_t vv_st, int64_t vl_sb, int64_t vl_st, int64_t dov_sb, int64_t dov_st, int64_t dol_sb,
                                 int64_t dol_st, double dropout, int64_t seed, void* stream);
int64_t hipie_bi_attn_train_backward_ws_bytes(int B, int H, int Nv, int L);

/*
 * The FFN of a deformable encoder layer in ONE launch at the split policy's accuracy:  out = W2 . relu(W1 . x + b1) + b2.
 *   x    (M, 2 D) HIPIE_HL8 rows (row stride ldx in fp16 elements);  w1 (F, 2 D) HL8;  b1 (F) fp32;
 *   w2p  (D, 2 F) HL8 of W2 with its COLUMNS permuted inside every block of 16 into the order 0-3, 8-11, 4-7, 12-15 (the order in which
 *        the MFMA C layout of the hidden tile hands its rows to the next product);  b2 (D) fp32;  out (M, D) fp32, row stride ldo.
 *   D = 256, F = 2048 (the shipped sizes of both deformable encoders).
 * Each product is the three-term split sum with fp32 accumulation; the hidden activations (ReLU, then split into an fp16 pair exactly as
 * hipie_gemm's HL8 epilogue does) never leave the registers -- no (M, F) tensor exists.
 * Replaces: linear2(dropout(relu(linear1(src)))) of DeformableTransformerEncoderLayer.forward_ffn
 *           (models/deformable_detr/deformable_transformer_dino.py:378-394) and MSDeformAttnTransformerEncoderLayer.forward_ffn
 *           (models/maskdino/pixel_decoder/maskdino_encoder.py:142-157), fp32 nn.Linear in the reference.
 */
int hipie_ffn_fused(const void* x, int64_t ldx, const void* w1, const float* b1, const void* w2p, const float* b2, float* out, int64_t ldo,
                    int M, int D, int F, void* stream);

/*
 * 3 x 3 convolution (stride 1, padding 1, no groups) at the split policy's accuracy as an IMPLICIT GEMM of hipie_gemm's kernel: K = 9 taps x C.
 * The caller provides the input on a zero-PADDED pixel grid: x = row 0 of a (B, H + 2, W + 2, C) channels-last tensor (rows = pixels, fp32 or
 * HIPIE_HL8, row stride ldx elements) with at least Wp + 1 readable rows before and after it (Wp = W + 2); tap (dy, dx) of output row r reads
 * input row r + (dy - 1) * Wp + (dx - 1).  w (N, 9 * C) as HIPIE_HL8 with k = (3 * dy + dx) * C + c, bias (N) fp32 or NULL; out = `rows`
 * rows on the SAME padded grid (the border rows are meaningless and cropped by the caller), fp32 or HL8, row stride ldo; act 0 | 1 GELU | 2 ReLU.
 * C a multiple of 32.  Three products per tap and channel with fp32 accumulation, like every split linear.
 * Replaces: the fp32 nn.Conv2d 3 x 3 of the MaskDINO pixel decoder's FPN output (detectron2 Conv2d + GN, maskdino_encoder.py:294-310) and of
 * MaskHeadSmallConv (ddetrs_dn.py:1633-1689), MIOpen implicit-GEMM fp32 kernels before (1.3 ms per 256 -> 256 map at 128 x 128, bs 8).
 */
int hipie_conv3x3_split(const void* x, int64_t ldx, const void* w, const float* bias, void* out, int64_t ldo, int64_t rows, int Wp, int C,
                        int N, int in_fmt, int out_fmt, int act, void* stream);

/*
 * Weight and bias gradient of hipie_conv3x3_split's convolution for the TRAINING step, on the same zero-padded pixel grid:
 *   dw[n, tap, c] = sum_rows g[row, n] * x[row + (ty - 1) * Wp + (tx - 1), c],  tap = 3 ty + tx;   db[n] = sum_rows g[row, n]
 *   g = dy, or with y given (the ReLU fused into the node) dy * [y > 0].
 *   x: row 0 of the input grid, `rows` rows of C f32 values, row stride ldx elements, at least Wp + 1 readable rows before and after it;
 *   dy: row 0 of the output-gradient grid, `rows` rows of N f32 values, row stride ldg -- its BORDER rows must be zero (the forward computes
 *   border rows too; their gradient is not part of the problem); no guard rows are read;  y: the forward's output on that grid with dy's
 *   row stride, or NULL;  dw (N, 9, C) and db (N) f32 contiguous, every element overwritten; db NULL: not computed.
 *   ws: at least ceil(rows / 2048) * (9 C N + N) * 4 bytes: one partial [dw | db] per chunk of 2048 rows, added in chunk order by a second
 *   launch.  Three-product split fp16 with fp32 accumulation; db from the fp32 values.  No atomics: two calls give the same bits.
 *   Every read stays inside rows -(Wp + 1) .. rows + Wp of x and rows 0 .. rows - 1 of dy / y.
 * Refused (HIPIE_EINVAL, nothing launched): null x / dy / dw / ws, rows outside 1 .. 2^31 - 1, Wp < 3, C or N no positive multiple of 32,
 * row strides below the row's width or no multiple of 4, a pointer off a 16-byte boundary, a workspace that is too small (the message
 * names the size needed).
 * Replaces: the weight / bias gradient kernels the library runs under torch.autograd for the 3 x 3 convolutions of MaskHeadSmallConv
 *           (ddetrs_dn.py:1633-1689) and of the pixel decoder's layer_1 (maskdino_encoder.py:294-310), and the ReLU backward in front of them.
 */
int hipie_conv3x3_wgrad(const float* x, int64_t ldx, const float* dy, int64_t ldg, const float* y, int64_t rows, int Wp, int C, int N,
                        float* dw, float* db, void* ws, int64_t ws_bytes, void* stream);

/*
 * Row-wise top-k of fp32 scores, k <= 1024: idx_out (rows, k) int64 in descending value order (ascending index among equal values;
 * NaN sorts as the largest value), val_out (rows, k) f32 or NULL.  One launch, hipGraph-replay safe.
 * Replaces: torch.topk in the two-stage query selections (models/deformable_detr/deformable_transformer_dino.py:222-230, 900 of Nv;
 * models/maskdino/transformer_decoder/maskdino_decoder.py:413-426, 300 of Nv) and in HIPIE_IMG.inference (hipie_img.py:640-648).
 */
int hipie_topk(const float* x, int64_t row_stride, int rows, int n, int k, int64_t* idx_out, float* val_out, void* stream);

/* device-side self-test helpers used by tests/ to pin the MFMA / LDS-transpose lane layouts this library assumes.
 *   which 0: D = A(32x16) . B(16x32) with v_mfma_f32_32x32x16_bf16, operands loaded with the layouts documented in
 *            csrc/mfma.h; out (32,32) f32.   which 1: ds_read_b64_tr_b16 of a (64,16) bf16 tile; out (64,4) f32 per lane.
 *   a, b: bf16 (as uint16) inputs. */
int hipie_selftest(int which, const uint16_t* a, const uint16_t* b, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPIE_MI355_H */
