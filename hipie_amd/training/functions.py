"""autograd Functions over the hand-written kernels that have a backward.  Forward and backward both run on
libhipie_mi355.so; there is no CPU implementation (the ops raise on host tensors)."""
import collections

import numpy as np
import torch

from .. import ops, ops_half


class MaskEinsumFunction(torch.autograd.Function):
    """einsum("bqc,bchw->bqhw") [+ row_bias[b, q]]: MaskDINO's mask logits (maskdino_decoder.py forward_prediction_heads) and the
    FoldedMaskFeatures form of the inference path.  forward = hipie_mask_einsum (three-product split), backward = two
    hipie_gemm_batched products (ops.mask_einsum_backward) + a row sum for the bias."""

    @staticmethod
    def forward(ctx, mask_embed, mask_features, row_bias=None):
        ctx.save_for_backward(mask_embed, mask_features)
        ctx.has_bias = row_bias is not None
        return ops.mask_einsum(mask_embed.float().contiguous(), mask_features.float().contiguous(), precision=1, row_bias=row_bias)

    @staticmethod
    def backward(ctx, grad_out):
        e, f = ctx.saved_tensors
        ge, gf = ops.mask_einsum_backward(e, f, grad_out.contiguous())
        gb = grad_out.sum((2, 3)) if ctx.has_bias else None
        return ge.to(e.dtype), gf.to(f.dtype), gb


def mask_einsum(mask_embed, mask_features, row_bias=None):
    return MaskEinsumFunction.apply(mask_embed, mask_features, row_bias)


class DynamicMaskFunction(torch.autograd.Function):
    """the CondInst dynamic mask head (DDETRSegmUniDN.dynamic_mask_with_coords, models/ddetrs_dn.py:1411-1502) with gradients for the
    mask features, the reference points and the controller parameters: forward = hipie_dynamic_mask (fp32 kernel), backward =
    hipie_dynamic_mask_backward.  mask_feats (B,8,H,W), ref_points (B*Q,2) pixels, params (B*Q,169) -> (B*Q, up*H, up*W)."""

    @staticmethod
    def forward(ctx, mask_feats, ref_points, params, num_queries, stride=8, up=2):
        mask_feats, ref_points, params = mask_feats.float().contiguous(), ref_points.float().contiguous(), params.float().contiguous()
        ctx.save_for_backward(mask_feats, ref_points, params)
        ctx.geom = (int(num_queries), int(stride), int(up))
        return ops.dynamic_mask(mask_feats, ref_points, params, num_queries, stride=stride, up=up)

    @staticmethod
    def backward(ctx, grad_out):
        feats, refs, params = ctx.saved_tensors
        q, stride, up = ctx.geom
        gf, gr, gp = ops.dynamic_mask_backward(feats, refs, params, grad_out.float().contiguous(), q, stride=stride, up=up)
        return gf, gr, gp, None, None, None


def dynamic_mask(mask_feats, ref_points, params, num_queries, stride=8, up=2):
    return DynamicMaskFunction.apply(mask_feats, ref_points, params, num_queries, stride, up)


class DeformSampleFunction(torch.autograd.Function):
    """MSDeformAttn's sampling from the RAW projections as one node (ops/modules/ms_deform_attn.py:99-114 + the operator): forward =
    hipie_msda_fused_forward (locations and the softmax in the kernel), backward = hipie_msda_raw_backward (the gather form; the chain rule
    through the location and the softmax in its coefficient kernel).  value (B,S,M,32) dense; ss / ls: the level tensors; ref (B,Lq,L,2|4);
    offsets (B,Lq,M,L,P,2) and logits (B,Lq,M,L*P), views of the projections' outputs -> (B,Lq,M*32).  Saved: value, ref, offsets, logits --
    no location, no softmax output.  grad_ref is computed only when ref needs it."""

    @staticmethod
    def forward(ctx, value, ss, ls, ref, offsets, logits):
        ref = ref.contiguous()
        ctx.save_for_backward(value, ref, offsets, logits)
        ctx.levels = (ss, ls)                        # the pyramid's cached constants (net.level_tensors)
        return ops.msda_fused(value, ss, ls, ref, offsets, logits)

    @staticmethod
    def backward(ctx, grad_out):
        value, ref, offsets, logits = ctx.saved_tensors
        ss, ls = ctx.levels
        gv, goff, glog, gref = ops.msda_raw_backward(value, ss, ls, ref, offsets, logits, grad_out, want_grad_ref=ctx.needs_input_grad[3])
        return gv, None, None, gref, goff, glog


MSDA_RAW_MAX_ROWS = 160 * 1024 // 4           # kBwdMaxRows of csrc/msda_bwd.hip: pixel rows whose counters fit the LDS of a CU
MSDA_RAW_MAX_POINTS = 32                      # kMaxLP: L * P of the in-kernel softmax


def deform_sample_ok(value, ref, offsets, logits):
    """what hipie_msda_raw_backward takes, checked on the host before anything is launched"""
    if value.dim() != 4 or offsets.dim() != 6 or logits.dim() != 4 or ref.dim() != 4:
        return False
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = offsets.shape
    if D != 32 or S > MSDA_RAW_MAX_ROWS or L * P > MSDA_RAW_MAX_POINTS or ref.shape[-1] not in (2, 4) or B == 0 or Lq == 0:
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 for t in (value, ref, offsets, logits)) or not value.is_contiguous():
        return False
    return (tuple(offsets[0, 0].stride()) == (L * P * 2, P * 2, 2, 1) and offsets.stride(0) == Lq * offsets.stride(1)
            and tuple(logits[0, 0].stride()) == (L * P, 1) and logits.stride(0) == Lq * logits.stride(1))


def deform_sample(value, shapes, ref, offsets, logits):
    """DeformSampleFunction on value (B,S,M,D), shapes [(H,W)], ref (B,Lq,L,2|4), offsets (B,Lq,M,L,P,2), logits (B,Lq,M,L*P) -> (B,Lq,M*D),
    or None -- before any launch -- for what the backward entry would refuse (D != 32, more pixel rows than the LDS counters hold, L*P > 32,
    anything but fp32 device tensors): the caller's composition then runs"""
    if not deform_sample_ok(value, ref, offsets, logits):
        return None
    from .net import level_tensors
    ss, ls = level_tensors(shapes, value.device)
    return DeformSampleFunction.apply(value, ss, ls, ref, offsets, logits)


# ---- the training linears: TWO graphs, y = x . W^T + b and linear -> act -> linear, each written once (_linear_forward / _linear_backward,
# _mlp_forward / _mlp_backward) over THREE operand policies, SPLIT, SCALED and HALF.  A policy answers only what differs between the formats:
# which shapes it takes, how an operand is made (of x, of a weight, of the activation, of an output gradient) and which GEMM entry
# consumes it.  The graph -- which gradient is needed when, what is recomputed, what is freed where -- is not the policy's business, and
# the bodies do not ask which policy they run.  The six node classes below hand a policy to a body; they are the public names.
def _weight_grad_chunks(M, N, K, group=32):
    """the chunks a weight gradient cuts the M rows into: doubled while the N x K tiles leave CUs idle and the 32-row groups divide evenly
    (group: the rows of one k tile -- 32 for the split operands, 64 for plain fp16)"""
    Mp = -(-M // group) * group
    tiles = -(-N // 256) * -(-K // 256)
    nk = 1
    while nk < 16 and tiles * nk < 256 and (Mp // group) % (2 * nk) == 0:
        nk *= 2
    return nk


def _grad_rows(gy, N):
    """the output gradient as the (M, N) fp32 rows ops.grad_scale / ops.grad_pack take: a view where the strides and the alignment allow"""
    g2 = gy.reshape(-1, N).float()
    if g2.stride(-1) != 1 or (g2.shape[0] > 1 and (g2.stride(0) < N or g2.stride(0) % 4)):
        g2 = g2.contiguous()
    return g2.clone() if g2.data_ptr() % 16 else g2


def _scaled_operands(pack, gy, N, need_rows, need_t, need_b):
    """an output gradient for the policies that scale it: {s, 1/s} = grad_scale(dy), then ONE pass of `pack` (ops.grad_pack |
    ops_half.half_pack) over dy -> ((s dy) rows, (s dy)^T, the column sums of the unscaled dy, the device scalar 1/s); a form that is not
    needed is not written"""
    g2 = _grad_rows(gy, N)
    scale = ops.grad_scale(g2)
    ga, gt, gb = pack(g2, scale, want_rows=need_rows, want_t=need_t, want_bias=need_b)
    return ga, gt, gb, scale[1:]


def _product_t(at, bt, rows, inv):
    """inv * at . bt^T for two TRANSPOSED HL8 operands (Na, 2 Mp), (Nb, 2 Mp) whose contraction runs over `rows` rows: cut into the chunks of
    _weight_grad_chunks, one problem each in ONE hipie_gemm_batched launch, the partial products added in chunk order and multiplied by the
    device scalar inv in one pass (or, one chunk, in the GEMM's store).  The weight gradient of every scaled split node."""
    nk = _weight_grad_chunks(rows, at.shape[0], bt.shape[0])
    if nk == 1:
        return ops.gemm_scaled(at, bt, inv, split=True, out_fmt=ops.F32, tag="train_dw")
    return ops.gemm_split_k_scaled(at, bt, nk, inv)


def _split_linear_ok(x, weight, rows):
    """the linears the split nodes take"""
    K, N = weight.shape[1], weight.shape[0]
    return x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and K % 32 == 0 and N % 32 == 0 and rows >= 256


def half_linear_ok(x, weight, rows):
    """the linears the half nodes take: fp32 device tensors, at least 256 rows, K % 64 == 0 (the contraction of y and the output rows of
    dW) and N % 64 == 0 (the contraction of dx): the F16 k tile is 64 elements"""
    K, N = weight.shape[1], weight.shape[0]
    return bool(x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and K % 64 == 0 and N % 64 == 0 and rows >= 256)


class _SplitOperands:
    """SPLIT: split-fp16 (HL8) weights against fp32 rows, three MFMA products per GEMM; the output gradient enters as it arrives.
    dW = dy^T . x (N x K, the contraction over the M token rows): N x K is 25-100 tiles of 256 x 256 for the ViT-H linears -- a fraction of
    the 256 CUs -- so the M rows (padded to 32) are cut into chunks, one problem each in ONE hipie_gemm_batched launch, and the partial
    products are summed (the 64 x 128-tile kernel the single problem fell to ran at 160 TFLOP/s: 0.51 ms per linear)."""
    split = True                                  # the operand code of the forward products
    ok = staticmethod(_split_linear_ok)

    def rows(self, x, keep):
        """(the forward operand of x, what is saved of it): the fp32 rows, always saved"""
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        return x2, x2

    def weight(self, owner, key, w, transposed=False):
        """the HL8 copy of W, or of W^T under key + ".T", cached on `owner` (ops.split_weight; the training net passes the weight tensor
        itself, so the copies die with it)"""
        if transposed:
            return ops.split_weight(owner, key + ".T", [w], lambda: w.t().contiguous())[0]
        return ops.split_weight(owner, key, [w], lambda: w)[0]

    def act(self, u, act):
        return ops.act_forward(u, act)

    def grads(self, gy, N, need_rows, need_t, need_b):
        """(dy fp32 rows, the same rows for dw, db = sum_m dy, no scale).  dy^T is NOT made here: dw transposes the rows itself, next to
        the product that reads them, as the node always did (made here, its 126 MB at qkv would wait through the dx product)"""
        g2 = gy.reshape(-1, N).float()
        if g2.stride(-1) != 1:
            g2 = g2.contiguous()
        return g2, g2, g2.sum(0) if need_b else None, None

    def dx(self, ga, wt, inv):
        return ops.gemm(ga, wt, None, split=True, out_fmt=ops.F32, tag="train_dx")

    def transposed(self, x):
        """the operand dw takes of the rows (M, K) a weight gradient contracts with: x^T as HL8 (K, 2 Mp), one pass"""
        return ops.to_hl8_t(x, 32)

    def dw(self, g2, xt, rows, inv):
        gt = ops.to_hl8_t(g2, 32)                                                             # (N, 2 Mp) fp16 pairs, one pass
        nk = _weight_grad_chunks(rows, gt.shape[0], xt.shape[0])
        if nk == 1:
            return ops.gemm(gt, xt, None, split=True, out_fmt=ops.F32, tag="train_dw")
        return ops.gemm_split_k(gt, xt, nk)


# SCALED gradient operands (csrc/grad_pack.hip; the opt-in group "scaled_grads" of training/net.py).  The split hi = fp16(dy),
# lo = fp16(dy - hi) is 2^-22 accurate only while dy is a normal fp16 number: a gradient of 1e-6 per element reaches the products above with
# ~1.6 % error, one of 1e-9 as zero, one above 65504 saturated.  Here every output gradient that enters a split GEMM is first multiplied by
# a power of two chosen on the device from its largest magnitude (ops.grad_scale: amax lands in [2^14, 2^15)), in the ONE pass that also
# writes both of its operand forms and the bias gradient (ops.grad_pack: three readers of dy become one), and the products are multiplied
# back by the kernel that writes them (ops.gemm_scaled, ops.gemm_split_k_scaled).  All factors are exact powers of two and every sum has a
# fixed order: the results for 2^e dy are 2^e times the results for dy, bit for bit.
class _ScaledOperands(_SplitOperands):
    """SCALED: SPLIT's forward; the output gradient arrives PACKED -- (s dy) rows and (s dy)^T as HL8, 1/s applied where a product is stored"""

    def grads(self, gy, N, need_rows, need_t, need_b):
        return _scaled_operands(ops.grad_pack, gy, N, need_rows, need_t, need_b)

    def dx(self, ga, wt, inv):
        return ops.gemm_scaled(ga, wt, inv, split=True, out_fmt=ops.F32, tag="train_dx")

    dw = staticmethod(_product_t)


# HALF precision (csrc/half_pack.hip, ops_half.py; the opt-in policy net.half_policy): ONE fp16 MFMA product per GEMM instead of three, fp32
# master weights, fp32 accumulation and output.  A precision policy, not a bit-compatible group: 2^-11 per operand.  Contract (DESIGN.md
# section 9): x16 = fp16(x), W16 = fp16(W), round to nearest even, saturated at +-65504, no scale;  y = x16 . W16^T + b;
# {s, 1/s} = grad_scale(dy), g16 = fp16(s dy);  dx = (1/s) g16 . W16;  dW = (1/s) g16^T . x16^T over the token rows padded to 64, in the
# chunks of _weight_grad_chunks(group=64), added in chunk order;  db = the column sums of the unscaled dy.  All scale factors are powers of
# two, every sum has a fixed order: the results for 2^e dy are 2^e times the results for dy, bit for bit.
class _HalfOperands:
    """HALF: single fp16 operands everywhere, the output gradient scaled as SCALED's is"""
    split = False
    ok = staticmethod(half_linear_ok)

    def rows(self, x, keep):
        """x16 = half_pack(x): fp16 rows, half the bytes of x; saved only when the weight needs a gradient (nothing else reads them)"""
        x16 = ops_half.half_pack(_grad_rows(x, x.shape[-1]), None, want_rows=True, want_t=False)[0]
        return x16, x16 if keep else None

    def weight(self, owner, key, w, transposed=False):
        """W16, or W16^T under key + ".T", cached on `owner` (ops_half.half_weight)"""
        if transposed:
            return ops_half.half_weight(owner, key + ".T", [w], lambda: w.t())
        return ops_half.half_weight(owner, key, [w], lambda: w)

    def act(self, u, act):
        return ops_half.act_half(u, act)

    def grads(self, gy, N, need_rows, need_t, need_b):
        return _scaled_operands(ops_half.half_pack, gy, N, need_rows, need_t, need_b)

    def dx(self, ga, wt, inv):
        return ops.gemm_scaled(ga, wt, inv, split=False, out_fmt=ops.F32, tag="train_dx")

    def transposed(self, x):
        """x16^T (K, Mp) of the rows (M, K), fp16 (the saved x16) or fp32 (the recomputed activation), in one pass"""
        return ops_half.half_pack(x, None, want_rows=False, want_t=True)[1]

    def dw(self, gt, xt, rows, inv):
        """dW = (1/s) g16^T . x16^T: gt = (s dy)^T as fp16 (N, Mp), inv the device scalar 1 / s; one chunk is the product itself"""
        return ops_half.gemm_split_k_half(gt, xt, _weight_grad_chunks(rows, gt.shape[0], xt.shape[0], 64), inv)


SPLIT, SCALED, HALF = _SplitOperands(), _ScaledOperands(), _HalfOperands()


def _forward_product(policy, a, w, bias):
    return ops.gemm(a, w, None if bias is None else bias.detach().float().contiguous(), split=policy.split, out_fmt=ops.F32, tag="train_fwd")


def _linear_forward(policy, ctx, x, weight, bias, owner, key):
    """y = x . W^T + b"""
    w_op = policy.weight(owner, key, weight)
    x_op, x_saved = policy.rows(x, ctx.needs_input_grad[1])
    ctx.save_for_backward(x_saved, weight)
    ctx.owner, ctx.key, ctx.lead, ctx.has_bias = owner, key, x.shape[:-1], bias is not None
    return _forward_product(policy, x_op, w_op, bias).view(*x.shape[:-1], weight.shape[0])


def _linear_backward(policy, ctx, gy):
    """dx = dy . W      dW = dy^T . x      db = sum_m dy;  a frozen input skips its operand form and its product"""
    x_saved, weight = ctx.saved_tensors
    N, K = weight.shape
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    need_b = ctx.has_bias and ctx.needs_input_grad[2]
    gx = gw = None
    if not (need_x or need_w or need_b):
        return None, None, None, None, None
    ga, gt, gb, inv = policy.grads(gy, N, need_x, need_w, need_b)
    if need_x:
        gx = policy.dx(ga, policy.weight(ctx.owner, ctx.key, weight, transposed=True), inv).view(*ctx.lead, K)
    if need_w:
        gw = policy.dw(gt, policy.transposed(x_saved), x_saved.shape[0], inv)
    return gx, gw, gb, None, None


def _mlp_forward(policy, ctx, x, w1, b1, w2, b2, act):
    """u = x . W1^T + b1     a = act(u)     y = a . W2^T + b2.  Saved: x's operand, u (fp32) and the two weights.  a is NOT saved -- it is a
    pointwise function of u, and the backward's one pass over u and da writes it again, with the forward's bits."""
    w1_op, w2_op = policy.weight(w1, "w", w1), policy.weight(w2, "w", w2)
    x_op, x_saved = policy.rows(x, ctx.needs_input_grad[1])
    u = _forward_product(policy, x_op, w1_op, b1)
    y = _forward_product(policy, policy.act(u, act), w2_op, b2)
    ctx.save_for_backward(x_saved, u, w1, w2)
    ctx.act, ctx.lead, ctx.has_b1, ctx.has_b2 = int(act), x.shape[:-1], b1 is not None, b2 is not None
    return y.view(*x.shape[:-1], w2.shape[0])


def _mlp_backward(policy, ctx, gy):
    """da = dy . W2                    dW2 = dy^T . a      db2 = sum_m dy      (a dies here)
    du, a, db1 = act_backward       dW1 = du^T . x      dx  = du . W1
    ops.act_backward writes du = da * act'(u) in place in da, a with the forward's bits only when W2 needs it, and db1 = sum_m du.  dy and
    du each get operands (and, where the policy scales, a scale) of their own; du is unscaled -- it is a product, so a power of two in da
    passes through it exactly.  With x, W1 and b1 frozen there is no da: a is recomputed alone."""
    x_saved, u, w1, w2 = ctx.saved_tensors
    need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:5]
    need_b1, need_b2 = need_b1 and ctx.has_b1, need_b2 and ctx.has_b2
    gx = gw1 = gb1 = gw2 = du = a = at = None
    if not (need_x or need_w1 or need_b1 or need_w2 or need_b2):
        return None, None, None, None, None, None
    need_da = need_x or need_w1 or need_b1
    ga, gt, gb2, inv = policy.grads(gy, w2.shape[0], need_da, need_w2, need_b2)
    if need_da:
        da = policy.dx(ga, policy.weight(w2, "w", w2, transposed=True), inv)
        ga = None
        du, a, gb1 = ops.act_backward(u, da, ctx.act, want_a=need_w2, want_bias_grad=need_b1, out=da)
        del da
    elif need_w2:
        a = policy.act(u, ctx.act)
    if need_w2:
        at = policy.transposed(a)
        a = None                                  # the product below runs without the fp32 activation in memory
        gw2 = policy.dw(gt, at, u.shape[0], inv)
    a = at = gt = None
    if need_x or need_w1:
        ua, ut, _, inv = policy.grads(du, w1.shape[0], need_x, need_w1, False)
        del du
        if need_w1:
            gw1 = policy.dw(ut, policy.transposed(x_saved), u.shape[0], inv)
        if need_x:
            gx = policy.dx(ua, policy.weight(w1, "w", w1, transposed=True), inv).view(*ctx.lead, w1.shape[1])
    return gx, gw1, gb1, gw2, gb2, None


class SplitLinearFunction(torch.autograd.Function):
    """F.linear(x, weight, bias) with forward AND backward on hipie_gemm's split-fp16 operands (three MFMA products, fp32 accumulation:
    fp32-class results at ~2.7x the rate of the fp32 matrix pipe): the linears of the training step that carry its flops (ViT qkv / proj /
    fc1 / fc2, the encoder FFNs).
        y  = x . W^T + b            hipie_gemm(A = x fp32 rows, W as HL8)
        dx = dy . W                 hipie_gemm(A = dy fp32 rows, W^T as HL8)
        dW = dy^T . x               split operands dy^T and x^T, the contraction over the M rows (padded to 32) cut into chunks that run as
                                    one hipie_gemm_batched launch (SPLIT.dw)
        db = sum_m dy
    The two transposed operands cost one pass each; the HL8 copies of W and W^T are cached on `owner`."""

    @staticmethod
    def forward(ctx, x, weight, bias, owner, key):
        return _linear_forward(SPLIT, ctx, x, weight, bias, owner, key)

    @staticmethod
    def backward(ctx, gy):
        return _linear_backward(SPLIT, ctx, gy)


class ScaledSplitLinearFunction(SplitLinearFunction):
    """SplitLinearFunction (its forward, unchanged) with a backward on scaled operands:
        {s, 1/s} = grad_scale(dy)       (s dy) rows, (s dy)^T, db = grad_pack(dy)        one pass over dy; a frozen input skips its form
        dx = (1/s) (s dy) . W           dW = (1/s) (s dy)^T . x                          the factor is applied where the product is stored"""

    @staticmethod
    def backward(ctx, gy):
        return _linear_backward(SCALED, ctx, gy)


HALF_NODE_CALLS = collections.Counter()          # forward calls of the two half nodes by name (tests: the node ran, not the fall-through)


class HalfLinearFunction(torch.autograd.Function):
    """F.linear(x, weight, bias) with forward AND backward on single fp16 operands (hipie_gemm with HIPIE_F16):
        x16 = half_pack(x)              y  = x16 . W16^T + b                               W16 / W16^T cached on `owner` (ops_half.half_weight)
        {s, 1/s} = grad_scale(dy)       (s dy) rows, (s dy)^T, db = half_pack(dy)          one pass over dy; a frozen input skips its form
        dx = (1/s) (s dy) . W16         dW = (1/s) (s dy)^T . x16^T                        the factor is applied where the product is stored
    Saved: x16 (fp16 rows, half the bytes of x) and the weight."""

    @staticmethod
    def forward(ctx, x, weight, bias, owner, key):
        HALF_NODE_CALLS["linear"] += 1
        return _linear_forward(HALF, ctx, x, weight, bias, owner, key)

    @staticmethod
    def backward(ctx, gy):
        return _linear_backward(HALF, ctx, gy)


class MlpFunction(torch.autograd.Function):
    """linear -> activation -> linear as ONE node of the graph: timm's Mlp of a ViT block (fc1 -> GELU -> fc2, backbone/vit.py:193-197) and the
    FFN of an encoder layer (linear1 -> ReLU -> linear2, deformable_transformer_dino.py:384-394): _mlp_forward / _mlp_backward on the split
    GEMM of SplitLinearFunction, ops.act_forward between.  act = ops.ACT_GELU | ops.ACT_RELU.  The HL8 copies of the weights are the ones
    SplitLinearFunction caches (on the weight, key "w")."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act):
        return _mlp_forward(SPLIT, ctx, x, w1, b1, w2, b2, act)

    @staticmethod
    def backward(ctx, gy):
        return _mlp_backward(SPLIT, ctx, gy)


class ScaledMlpFunction(MlpFunction):
    """MlpFunction (its forward, unchanged) with a backward on scaled operands; dy and du each get a scale of their own:
        {sy, 1/sy} = grad_scale(dy)     (sy dy) rows, (sy dy)^T, db2 = grad_pack(dy)
        da = (1/sy) (sy dy) . W2        dW2 = (1/sy) (sy dy)^T . a
        du, a, db1 = act_backward       (unscaled)
        {su, 1/su} = grad_scale(du)     (su du) rows, (su du)^T = grad_pack(du)
        dW1 = (1/su) (su du)^T . x      dx = (1/su) (su du) . W1"""

    @staticmethod
    def backward(ctx, gy):
        return _mlp_backward(SCALED, ctx, gy)


class HalfMlpFunction(torch.autograd.Function):
    """linear -> activation -> linear as ONE node in half precision (MlpFunction's graph):
        x16 = half_pack(x)      u = x16 . W1_16^T + b1 (fp32)      a16 = act_half(u)      y = a16 . W2_16^T + b2
    Saved: x16, u (fp32: act_backward needs it) and the two weights.  dy and du each get a scale of their own:
        {sy, 1/sy} = grad_scale(dy)     (sy dy) rows, (sy dy)^T, db2 = half_pack(dy)
        da = (1/sy) (sy dy) . W2_16     du, a, db1 = act_backward(u, da)     dW2 = (1/sy) (sy dy)^T . fp16(a)^T   (a: recomputed, fp32, dies here)
        {su, 1/su} = grad_scale(du)     (su du) rows, (su du)^T = half_pack(du)
        dW1 = (1/su) (su du)^T . x16^T  dx = (1/su) (su du) . W1_16"""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act):
        HALF_NODE_CALLS["mlp"] += 1
        return _mlp_forward(HALF, ctx, x, w1, b1, w2, b2, act)

    @staticmethod
    def backward(ctx, gy):
        return _mlp_backward(HALF, ctx, gy)


def _library_linear(x, weight, bias, owner, key):
    return torch.nn.functional.linear(x, weight, bias)


def _linear_or(policy, node, otherwise, x, weight, bias, owner, key):
    """the front door of a linear node: the node where the policy takes the shape, `otherwise` where it does not"""
    if policy.ok(x, weight, x.numel() // weight.shape[1] if weight.shape[1] else 0):
        return node.apply(x, weight, bias, owner, key)
    return otherwise(x, weight, bias, owner, key)


def _mlp_or(policy, node, otherwise, x, w1, b1, w2, b2, act):
    """the front door of an MLP node: the node when the policy takes BOTH linears, `otherwise` for any other shape, so nothing is refused"""
    rows = x.numel() // w1.shape[1] if w1.shape[1] else 0
    if policy.ok(x, w1, rows) and policy.ok(x, w2, rows) and act in (ops.ACT_GELU, ops.ACT_RELU):
        return node.apply(x, w1, b1, w2, b2, act)
    return otherwise(x, w1, b1, w2, b2, act)


def _three_nodes(linear, x, w1, b1, w2, b2, act):
    """the composition an MLP node replaces: linear -> library activation -> linear"""
    f = {ops.ACT_GELU: torch.nn.functional.gelu, ops.ACT_RELU: torch.nn.functional.relu}[act]
    return linear(f(linear(x, w1, b1, w1, "w")), w2, b2, w2, "w")


def split_linear(x, weight, bias, owner, key):
    """F.linear on the split GEMM with a backward (SplitLinearFunction); shapes it does not cover fall through to the library"""
    return _linear_or(SPLIT, SplitLinearFunction, _library_linear, x, weight, bias, owner, key)


def split_linear_scaled(x, weight, bias, owner, key):
    """split_linear with the scaled-gradient backward (ScaledSplitLinearFunction); the same shapes, the same fall-through to the library"""
    return _linear_or(SCALED, ScaledSplitLinearFunction, _library_linear, x, weight, bias, owner, key)


def half_linear(x, weight, bias, owner, key):
    """F.linear in half precision with a backward (HalfLinearFunction); a shape outside half_linear_ok runs the split node (split_linear)"""
    return _linear_or(HALF, HalfLinearFunction, split_linear, x, weight, bias, owner, key)


def split_mlp(x, w1, b1, w2, b2, act):
    """linear(act(linear(x, w1, b1)), w2, b2) as one node (MlpFunction) when BOTH linears are ones split_linear takes; any other shape runs
    the three-node composition (split_linear -> library activation -> split_linear)"""
    return _mlp_or(SPLIT, MlpFunction, lambda *a: _three_nodes(split_linear, *a), x, w1, b1, w2, b2, act)


def split_mlp_scaled(x, w1, b1, w2, b2, act):
    """split_mlp with the scaled-gradient backward (ScaledMlpFunction) under the same conditions; any other shape runs the three-node
    composition over split_linear_scaled"""
    return _mlp_or(SCALED, ScaledMlpFunction, lambda *a: _three_nodes(split_linear_scaled, *a), x, w1, b1, w2, b2, act)


def half_mlp(x, w1, b1, w2, b2, act):
    """linear(act(linear(x, w1, b1)), w2, b2) as one node in half precision (HalfMlpFunction) when BOTH linears are ones half_linear takes;
    any other shape runs the split node (split_mlp)"""
    return _mlp_or(HALF, HalfMlpFunction, split_mlp, x, w1, b1, w2, b2, act)


class ScaledMaskEinsumFunction(MaskEinsumFunction):
    """MaskEinsumFunction (its forward, unchanged) whose backward scales the output gradient the same way: its two hipie_gemm_batched products
    split grad_out into fp16 pairs too, and the per-pixel gradient of a mask loss is the smallest of the step (with the loss multiplied by
    2^-20 every gradient behind the mask logits of the tiny fixture came out as zero).  The scale is the device block of ops.grad_scale; the
    two multiplications are library passes over grad_out and the results (the products have no device-side alpha), not part of the linears'
    pack.  A grad_out whose size is not a multiple of 4 runs the unscaled backward."""

    @staticmethod
    def backward(ctx, grad_out):
        go = grad_out.float().contiguous()
        if go.numel() % 4 or go.data_ptr() % 16 or go.numel() == 0:
            return MaskEinsumFunction.backward(ctx, grad_out)
        e, f = ctx.saved_tensors
        hw = go.shape[2] * go.shape[3]
        scale = ops.grad_scale(go.view(-1, hw) if hw % 4 == 0 else go.view(1, -1))
        ge, gf = ops.mask_einsum_backward(e, f, go * scale[0])
        gb = grad_out.sum((2, 3)) if ctx.has_bias else None
        return (ge * scale[1]).to(e.dtype), (gf * scale[1]).to(f.dtype), gb


def mask_einsum_scaled(mask_embed, mask_features, row_bias=None):
    return ScaledMaskEinsumFunction.apply(mask_embed, mask_features, row_bias)


def _attention_forward(ctx, qa, ka, v, cols, forward_op):
    """the forward of FusedAttentionFunction / WindowAttentionFunction: q', k' padded to `cols` operand columns"""
    qp, kp = ops.f16_pair(qa, cols), ops.f16_pair(ka, cols)
    out, lse = forward_op(qp, kp, ops.f16_pair(v))
    ctx.save_for_backward(qp[0], qp[1], kp[0], kp[1], v, out, lse)
    ctx.cols = (qa.shape[-1], ka.shape[-1])
    return out


def _attention_backward(ctx, go, backward_op):
    """their backward"""
    qh, ql, kh, kl, v, out, lse = ctx.saved_tensors
    go = go.float().contiguous()
    # dO enters the kernels as fp16 pairs: scaled by a power of two so that its largest entry sits in [8, 16) (a device scalar: no host
    # wait) -- high enough for the pairs of dO and dS = P (dP - delta) to be normal fp16 numbers, low enough for |dP| <= 16 * 80 * max|v|
    scale = torch.exp2(torch.floor(torch.log2(16.0 / go.abs().amax().clamp_min(1e-30))))
    delta = (go * out).sum(-1) * scale
    dq, dk, dv = backward_op((qh, ql), (kh, kl), ops.f16_pair(v, 96), ops.f16_pair(go, 96, scale), lse, delta)
    inv = 1.0 / scale
    cq, ck = ctx.cols
    return dq[..., :cq] * inv, torch.nn.functional.pad(dk * inv, (0, ck - 80)), dv * inv


class FusedAttentionFunction(torch.autograd.Function):
    """softmax(q' k'^T) v with the decomposed rel-pos bias folded into q' / k' (net.vit_attention), forward and backward on
    hipie_attn_train_forward / _backward (csrc/attn_train.hip): no (heads, N, N) tensor in HBM.  q' (BH, N, <= 224), k' (BH, N, <= 224) whose
    columns from 80 on are CONSTANT (the key-axis indicators: they get a zero gradient), v (BH, N, 80), N a multiple of 128.
    Saved for the backward: the fp16 pairs of q' and k' (the bytes of the fp32 operands), v, the output and the log-sum-exp row."""

    @staticmethod
    def forward(ctx, qa, ka, v):
        return _attention_forward(ctx, qa, ka, v, 224, ops.attn_train_forward)

    @staticmethod
    def backward(ctx, go):
        return _attention_backward(ctx, go, ops.attn_train_backward)


def fused_attention_ok(qa, ka, v):
    """operands FusedAttentionFunction takes as they are (the global blocks of the ViT at grids whose token count is a multiple of 128)"""
    return (qa.is_cuda and qa.dtype == torch.float32 and v.shape[-1] == 80 and qa.shape[-1] <= 224 and ka.shape[-1] == qa.shape[-1]
            and qa.shape[1] % 128 == 0)


def fused_attention(qa, ka, v):
    """softmax(q' k'^T) v on the fused kernels, or None when the operands are not covered.  Token counts that are not a multiple of 128 (a
    50 x 76 grid: 3800) are padded: the padding KEYS get a bias of -30000 through one more operand column (q' column 1, k' column -30000
    on the padding rows) so they receive probability 0; the padding QUERY rows are zeros and their outputs are dropped (no gradient
    reaches them)."""
    BH, N, C = qa.shape
    if N % 128 == 0:
        return FusedAttentionFunction.apply(qa, ka, v) if fused_attention_ok(qa, ka, v) else None
    if N < 1024:
        # the 196-token windows: correct on this path (tests) but SLOWER than the materialised formulation -- the kernels always run 224
        # operand columns (a window has 108) and 256 rows: 752 against 720 ms per training step
        return None
    Np = -(-N // 128) * 128
    pad = torch.nn.functional.pad
    if not fused_attention_ok(pad(qa[:, :0], (0, 1, 0, Np)), pad(ka[:, :0], (0, 1, 0, Np)), pad(v[:, :0], (0, 0, 0, Np))):
        return None
    bias = ka.new_zeros(BH, Np, 1)
    bias[:, N:] = -30000.0
    qa_p = pad(torch.cat((qa, qa.new_ones(BH, N, 1)), -1), (0, 0, 0, Np - N))
    ka_p = torch.cat((pad(ka, (0, 0, 0, Np - N)), bias), -1)
    return FusedAttentionFunction.apply(qa_p, ka_p, pad(v, (0, 0, 0, Np - N)))[:, :N]


class WindowAttentionFunction(torch.autograd.Function):
    """FusedAttentionFunction for the WINDOWED blocks: softmax(q' k'^T) v over items of N <= 256 tokens (one (window, head) each, no row
    padding) on hipie_attn_train_win_forward / _backward (csrc/attn_train_win.hip).  q', k' (BH, N, <= 128) whose columns from 80 on are
    CONSTANT in k' (the key-axis indicators: they get a zero gradient), v (BH, N, 80).  Saved for the backward: the fp16 pairs of q' and k',
    v, the output and the log-sum-exp row.
    A ONE-token item is the closed form, not a launch: a softmax over one key is the identity, so out = v, dq' = 0, dk' = 0 and dv = dO hold
    exactly, whereas the kernels (which take v and dO as fp16 pairs: 22 of fp32's 24 significant bits) reach them to ~2e-7 only.  The
    kernels themselves take N = 1 (tests/test_gpu_attn_train_win.py runs them there through the ops)."""

    @staticmethod
    def forward(ctx, qa, ka, v):
        ctx.single = qa.shape[1] == 1
        if ctx.single:
            ctx.shapes = (qa.shape, ka.shape)
            return v.clone()
        return _attention_forward(ctx, qa, ka, v, 128, ops.attn_train_win_forward)

    @staticmethod
    def backward(ctx, go):
        if ctx.single:
            return go.new_zeros(ctx.shapes[0]), go.new_zeros(ctx.shapes[1]), go
        return _attention_backward(ctx, go, ops.attn_train_win_backward)


def window_attention_ok(qa, ka, v):
    """operands WindowAttentionFunction takes: device fp32, head width 80, at most 128 operand columns, items of at most 256 tokens"""
    return (qa.dim() == 3 and qa.is_cuda and qa.dtype == torch.float32 and v.shape[-1] == 80 and 80 <= qa.shape[-1] <= 128
            and ka.shape[-1] == qa.shape[-1] and 1 <= qa.shape[1] <= 256 and qa.shape[0] >= 1)


def window_attention(qa, ka, v):
    """softmax(q' k'^T) v of the windowed ViT blocks on the short-sequence fused kernels, or None when the operands are not covered"""
    return WindowAttentionFunction.apply(qa, ka, v) if window_attention_ok(qa, ka, v) else None


def _rows_of_grid_row(t):
    """(BH, H, W, C) -> (H, BH W, C), the operand of a rel-pos product batched over the grid rows h.  The rows (item, w) of one grid row do
    not merge into one stride: a copy"""
    BH, H, W, C = t.shape
    return t.permute(1, 0, 2, 3).reshape(H, BH * W, C)


def _rows_of_grid_column(t):
    """(BH, H, W, C) -> (W, BH H, C), the operand of a rel-pos product batched over the grid columns w.  The rows (item, h) of one grid column
    merge into ONE stride whenever an item's rows are dense (stride(0) == H * stride(1)): a view, which the library product takes as it is"""
    BH, H, W, C = t.shape
    return t.permute(2, 0, 1, 3).reshape(W, BH * H, C)


class VitAttentionFunction(torch.autograd.Function):
    """The attention of a ViT block between its two linears as ONE node: qkv (B', N, 3 heads 80), the rows of the qkv linear, and the
    gathered rel-pos tables Rh (H, H, 80), Rw (W, W, 80) of net.get_rel_pos -> (B', N, heads 80), the rows of the proj linear.  What
    net.vit_attention composes from reshape / permute / unbind, the scale, two einsums, two cats and FusedAttentionFunction /
    WindowAttentionFunction (three f16_pair passes forward; amax, delta, two f16_pair passes, three rescales and a pad backward, and
    autograd's undoing of the views at full qkv size) is here
        forward   ops.attn_pack_kv -> two library batched products on rq -> ops.attn_pack_q -> the forward op -> one copy to token-major
        backward  ops.attn_grad_amax -> ops.attn_pack_grad -> the backward op -> four (six with table gradients) batched products on strided
                  views of dq' -> ops.attn_unpack_grad, which writes d(qkv) once
    with the operand planes, the bits and the attention kernels of the composition.  fp32 q' / k' are never built.  Saved: the q' / k' pairs,
    the 80-wide v pair, out, lse, Rh, Rw, and rq only when a table needs its gradient -- nothing is a view of qkv.
    cols 224: hipie_attn_train_* (N a multiple of 128, or `padded` to one as functions.fused_attention pads); cols 128: hipie_attn_train_win_*."""

    @staticmethod
    def forward(ctx, qkv, Rh, Rw, heads, H, W, cols, padded):
        B, N, BH = qkv.shape[0], H * W, qkv.shape[0] * heads
        rq, kp, vp = ops.attn_pack_kv(qkv.contiguous(), heads, H, W, cols, padded)
        a_h, a_w = _rows_of_grid_row(rq.view(BH, H, W, 80)), _rows_of_grid_column(rq.view(BH, H, W, 80))
        # rel_h[b, h, w, k] = rq[b, h, w, :] . Rh[h, k, :] and rel_w[b, h, w, k] = rq[b, h, w, :] . Rw[w, k, :], left in the layouts of the
        # products: pack_q reads them through their strides
        rel_h = torch.bmm(a_h, Rh.transpose(1, 2)).view(H, BH, W, H).permute(1, 0, 2, 3)
        rel_w = torch.bmm(a_w, Rw.transpose(1, 2)).view(W, BH, H, W).permute(1, 2, 0, 3)
        qp = ops.attn_pack_q(rq, rel_h, rel_w, heads, H, W, cols, padded)
        out, lse = (ops.attn_train_forward if cols == 224 else ops.attn_train_win_forward)(qp, kp, vp)
        tables = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ctx.save_for_backward(qp[0], qp[1], kp[0], kp[1], vp[0], vp[1], out, lse, Rh, Rw, rq if tables else None)
        ctx.geom = (heads, H, W, cols)
        return out.view(B, heads, -1, 80)[:, :, :N].permute(0, 2, 1, 3).reshape(B, N, heads * 80)

    @staticmethod
    def backward(ctx, go):
        qh, ql, kh, kl, vh, vl, out, lse, Rh, Rw, rq = ctx.saved_tensors
        heads, H, W, cols = ctx.geom
        BH, Np = out.shape[:2]
        N = H * W
        go = go.reshape(BH // heads, N, heads * 80).float().contiguous()
        # dO enters the kernels as fp16 pairs scaled by a power of two (_attention_backward); the maximum comes from one kernel, the scalar
        # expression stays on its one element: no host wait
        scale = torch.exp2(torch.floor(torch.log2(16.0 / ops.attn_grad_amax(go).clamp_min(1e-30))))
        inv = 1.0 / scale
        dop, v96, delta = ops.attn_pack_grad(go, out, (vh, vl), scale, heads, H, W)
        dq, dk, dv = (ops.attn_train_backward if cols == 224 else ops.attn_train_win_backward)((qh, ql), (kh, kl), v96, dop, lse, delta)
        d4 = dq[:, :N].view(BH, H, W, cols)
        g_h, g_w = _rows_of_grid_row(d4[..., 80:80 + H]), _rows_of_grid_column(d4[..., 80 + H:80 + H + W])
        # the rel-pos terms of dq, each in the layout of its product; unpack_grad adds them through their strides
        dq_h = torch.bmm(g_h, Rh).view(H, BH, W, 80).permute(1, 0, 2, 3)
        dq_w = torch.bmm(g_w, Rw).view(W, BH, H, 80).permute(1, 2, 0, 3)
        dqkv = ops.attn_unpack_grad(dq, dk, dv, dq_h, dq_w, inv, heads, H, W)
        dRh = dRw = None
        if rq is not None:
            if ctx.needs_input_grad[1]:
                dRh = torch.bmm(g_h.transpose(1, 2), _rows_of_grid_row(rq.view(BH, H, W, 80))) * inv
            if ctx.needs_input_grad[2]:
                dRw = torch.bmm(g_w.transpose(1, 2), _rows_of_grid_column(rq.view(BH, H, W, 80))) * inv
        return dqkv, dRh, dRw, None, None, None, None, None


def packed_attention_instance(H, W, windows=False):
    """(operand columns, padded) of the kernel instance VitAttentionFunction runs an H x W grid on, or None when none covers it"""
    N = H * W
    if N >= 128 and N % 128 == 0 and 80 + H + W <= 224:
        return 224, False
    if N % 128 and N >= 1024 and 80 + H + W + 1 <= 224:
        return 224, True
    if windows and 2 <= N <= 256 and 80 + H + W <= 128:
        return 128, False
    return None


def vit_attention_packed(qkv, Rh, Rw, heads, H, W, windows=False):
    """the attention of a ViT block from the rows of its qkv linear, qkv (B', H W, 3 heads 80), and the gathered rel-pos tables Rh (H, H, 80),
    Rw (W, W, 80) as one node (VitAttentionFunction) -> (B', H W, heads 80), or None when not covered (the caller's composition runs).
    Covered: device fp32, head width 80, net.FOLD_REL_POS on, and
        the global instance      H W a multiple of 128 and 80 + H + W <= 224
        its padded form          H W >= 1024 and 80 + H + W + 1 <= 224 (the padding of functions.fused_attention)
        the window instance      only with `windows`: 2 <= H W <= 256 and 80 + H + W <= 128"""
    from . import net
    N = H * W
    tensors = (qkv, Rh, Rw)
    if not (net.FOLD_REL_POS and all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and qkv.dim() == 3 and heads >= 1
            and tuple(qkv.shape[1:]) == (N, 3 * heads * 80) and qkv.shape[0] >= 1 and tuple(Rh.shape) == (H, H, 80) and tuple(Rw.shape) == (W, W, 80)):
        return None
    inst = packed_attention_instance(H, W, windows)
    if inst is None:
        return None
    cols, padded = inst
    return VitAttentionFunction.apply(qkv, Rh, Rw, heads, H, W, cols, padded)


class AddLayerNormFunction(torch.autograd.Function):
    """s = x + delta;  y = LayerNorm(s) * weight + bias  -> (s, y): a residual add and the LayerNorm that follows it (Block.forward,
    backbone/vit.py:212-230; the post-norms of DeformableTransformerEncoderLayer.forward, deformable_transformer_dino.py:384-394) as one
    node of the graph.  forward = hipie_add_layernorm (the inference path's kernel, fp32 in and out), backward = ONE
    hipie_layernorm_backward launch (+ its partial-row sum) that takes the gradient of y AND the gradient arriving at s from the residual
    stream: d loss / d s, which is the gradient of x and of delta alike.  Saved: s and weight (the statistics are recomputed)."""

    @staticmethod
    def forward(ctx, x, delta, weight, bias, eps):
        x = x.contiguous()
        s, y = ops.add_layernorm(x, None if delta is None else delta.contiguous(), weight.detach(), bias.detach(), eps, torch.float32)
        ctx.save_for_backward(s, weight)
        ctx.eps, ctx.has_delta = float(eps), delta is not None
        ctx.set_materialize_grads(False)          # an output nothing consumed arrives as None, not as a tensor of zeros to stream through
        return s, y

    @staticmethod
    def backward(ctx, g_s, g_y):
        s, weight = ctx.saved_tensors
        want = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        if g_s is None and g_y is None:
            return None, None, None, None, None
        if g_y is None:                       # the normalised output went nowhere: s is a plain sum
            dx, dg, db = g_s, (torch.zeros_like(weight) if want else None), (torch.zeros_like(weight) if want else None)
        else:
            dx, dg, db = ops.layernorm_backward(s, g_y, weight, ctx.eps, gres=g_s, want_param_grads=want)
        return (dx if ctx.needs_input_grad[0] else None, dx if ctx.has_delta and ctx.needs_input_grad[1] else None,
                dg if ctx.needs_input_grad[2] else None, db if ctx.needs_input_grad[3] else None, None)


def add_layer_norm(x, delta, weight, bias, eps):
    """(s, y) = (x + delta, LayerNorm(x + delta)) with a hand-written backward (AddLayerNormFunction); delta=None: s is x"""
    return AddLayerNormFunction.apply(x, delta, weight, bias, eps)


class GroupNormFunction(torch.autograd.Function):
    """y = GroupNorm(groups, C = 8 * groups)(x) [then ReLU] of a dense NCHW fp32 map: the conv + GN blocks after the backbone (input_proj of
    both heads, deformable_detr.py:139-160; adapter_1 / layer_1 / mask_features of the pixel decoder, maskdino_encoder.py:262-300) as ONE node
    of the graph.  forward = hipie_group_norm_train_forward (the inference path's two NCHW launches + the statistics), backward =
    hipie_group_norm_backward.  Saved: x, stat (B, groups, 2), weight, bias -- nothing else of x's size: with ReLU the mask is recomputed."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, relu):
        y, stat = ops.group_norm_train_forward(x, groups, weight.detach(), bias.detach(), eps, relu)
        ctx.save_for_backward(x, stat, weight, bias)
        ctx.groups, ctx.relu = int(groups), bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stat, weight, bias = ctx.saved_tensors
        want_x, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (want_x or want_p):
            return None, None, None, None, None, None
        dx, dg, db = ops.group_norm_backward(x, dy.contiguous(), stat, ctx.groups, weight, bias, ctx.relu, want_dx=want_x, want_param_grads=want_p)
        return dx, dg if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None, None, None


def group_norm_ok(x, groups):
    """the limits of the training GroupNorm kernels: a dense NCHW fp32 device map, C = 8 * groups, groups a power of two <= 64, H*W % 8 == 0"""
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous() and 0 < groups <= 64 and 256 % groups == 0
            and x.shape[1] == 8 * groups and x.shape[0] > 0 and x.shape[2] * x.shape[3] > 0 and (x.shape[2] * x.shape[3]) % 8 == 0)


def group_norm(x, groups, weight, bias, eps, relu=False):
    """GroupNorm (+ ReLU) with a hand-written backward (GroupNormFunction), or None outside the kernels' limits: the caller's torch form runs"""
    if not group_norm_ok(x, groups) or weight.dtype != torch.float32 or bias.dtype != torch.float32:
        return None
    return GroupNormFunction.apply(x, weight, bias, groups, eps, relu)


class Conv3x3Function(torch.autograd.Function):
    """y = conv2d(x, weight, bias, stride 1, padding 1) [then ReLU] for a dense 3 x 3 fp32 convolution as ONE node of the graph: the
    MaskHeadSmallConv convolutions (ddetrs_dn.py:1633-1689) and the pixel decoder's layer_1 (maskdino_encoder.py:294-310).  All three passes
    work on the zero-padded pixel grid of ops.conv3x3_stage (B (H+2) (W+2) rows of channels, zero border, W + 3 guard rows on both ends):
        y  = hipie_conv3x3_split(x grid, W as HL8 (N, 9 C))                  F32 rows in and out, bias / ReLU in the epilogue
        dx = hipie_conv3x3_split(g grid, Wt as HL8 (C, 9 N))                 Wt[c, (2 - ky, 2 - kx), n] = W[n, c, ky, kx]
        dW, db = hipie_conv3x3_wgrad(x grid, g grid)                         the row contraction per tap, csrc/conv_wgrad.hip
    with g = dy, or dy * [y > 0] under ReLU.  Saved: x as it came in, and with ReLU the output grid -- the storage the returned y is a view
    of, so the mask costs no memory of its own; no pre-ReLU map, no mask tensor.  x is RE-STAGED in the backward rather than keeping its
    grid: the step's convolution inputs are kept by their producers anyway, a saved grid would be a second copy of each until its backward
    (about 35 MB per 128 x 128 site at 2 images), and the re-staging is one copy pass.  Only the saved-x form was built and measured.
    The HL8 copies of W and Wt are cached on the weight tensor (ops.split_weight) and rebuilt when it changes.
    needs_input_grad is honoured: a frozen input skips the dx pass, a frozen weight and bias skip hipie_conv3x3_wgrad."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        B, C, H, W = x.shape
        N = weight.shape[0]
        w_hl8, _, _ = ops.split_weight(weight, "w3x3", [weight], lambda: weight.permute(0, 2, 3, 1).reshape(N, 9 * C))
        yg = ops.conv3x3_grid(ops.conv3x3_stage(x), w_hl8, None if bias is None else bias.detach().contiguous(), B, H, W, relu)
        ctx.save_for_backward(x, weight, *((yg,) if relu else ()))
        ctx.owner, ctx.relu, ctx.has_bias = weight, bool(relu), bias is not None
        return ops.conv3x3_crop(yg, B, H, W)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors[:2]
        yg = ctx.saved_tensors[2] if ctx.relu else None
        B, C, H, W = x.shape
        N = weight.shape[0]
        want_x, want_w, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (want_x or want_w or want_b):
            return None, None, None, None
        g = ops.conv3x3_stage(dy)                              # border and guard rows zero; a strided dy is read in place by the copy
        guard = W + 3
        if yg is not None and want_x:                          # the dx convolution needs the masked map itself; the weight pass then reads it
            g[guard:guard + yg.shape[0]].masked_fill_(~(yg > 0), 0.0)
            yg = None
        dx = dw = db = None
        if want_x:
            wt_hl8, _, _ = ops.split_weight(ctx.owner, "w3x3.T", [weight], lambda: weight.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9 * N))
            dx = ops.conv3x3_crop(ops.conv3x3_grid(g, wt_hl8, None, B, H, W), B, H, W)
        if want_w or want_b:
            dw, db = ops.conv3x3_wgrad(ops.conv3x3_stage(x), g, yg, B, H, W, want_bias=want_b)
            dw = dw.view(N, 3, 3, C).permute(0, 3, 1, 2).contiguous() if want_w else None
        return dx, dw, db, None


def conv3x3_train_ok(x, weight, bias=None, stride=1, padding=1, dilation=1, groups=1):
    """the limits of the training convolution node: fp32 device tensors, kernel 3 x 3, stride 1, padding 1 (zeros), dilation 1, groups 1,
    Cin % 32 == 0 and Cout % 32 == 0 (the input-gradient pass swaps the channel roles, and hipie_conv3x3_split needs C % 32), and the
    byte-offset limit hipie_conv3x3_split checks on a row stride, for both channel counts"""
    def one(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        return False
    if one(stride) != (1, 1) or one(padding) != (1, 1) or one(dilation) != (1, 1) or groups != 1:
        return False
    N, C = weight.shape[0], weight.shape[1]
    if C != x.shape[1] or C % 32 or N % 32 or min(x.shape) < 1:
        return False
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        return False
    if (256 + x.shape[3] + 4) * 4 * max(C, N) >= 1 << 31 or x.shape[0] * (x.shape[2] + 2) * (x.shape[3] + 2) >= 1 << 31:
        return False
    return x.is_cuda and weight.is_cuda and (bias is None or bias.is_cuda)


def conv3x3_train(x, weight, bias=None, relu=False, stride=1, padding=1, dilation=1, groups=1):
    """conv2d (+ ReLU) with a hand-written backward (Conv3x3Function), or None outside conv3x3_train_ok's limits: the caller's F.conv2d runs"""
    if not conv3x3_train_ok(x, weight, bias, stride, padding, dilation, groups):
        return None
    return Conv3x3Function.apply(x, weight, bias, relu)


def _patch_source(t):
    """a map the pack reads in place: fp32, the unit stride that of W or of C, no dimension expanded (a broadcast gradient has stride 0), on
    a 16-byte boundary (ops.grad_scale reads it too); anything else is copied to NCHW once"""
    from ..ops_patch import _map_strides
    t = t.float()
    sb, sc, sh, sw = _map_strides(t)
    if (sw != 1 and sc != 1) or min(sc, sh, sw) < 1 or sb < max(t.shape[1] * sc if sw == 1 else 0, t.shape[2] * sh) or t.data_ptr() % 16:
        t = t.contiguous()
        t = t.clone() if t.data_ptr() % 16 else t
    return t


def _patch_operands(t, k, scale=None, want_f32=False, want_rows=False, want_t=False, want_sum=False):
    """(fp32 rows, HL8 rows, HL8 transpose, channel sums) of the map t in ONE pass: a channels-last k == 1 map IS its rows (a view), and the
    existing row entries take it -- ops.grad_pack for a gradient, ops.to_hl8_t for an activation; every other map goes through
    ops_patch.patch_pack"""
    from .. import ops_patch
    rows = ops_patch.patch_rows_view(t, k)
    if rows is None:
        return ops_patch.patch_pack(t, k, scale, want_f32=want_f32, want_rows=want_rows, want_t=want_t, want_sum=want_sum)
    if scale is not None:
        return (rows if want_f32 else None,) + tuple(ops.grad_pack(rows, scale, want_rows=want_rows, want_t=want_t, want_bias=want_sum))
    if want_rows or want_sum:          # no caller: an unscaled map is an activation, wanted as fp32 rows or as the transposed operand
        raise RuntimeError("_patch_operands: an unscaled rows view gives fp32 rows and the transposed operand only")
    return rows if want_f32 else None, None, ops.to_hl8_t(rows, 32) if want_t else None, None


def _amax_rows(t):
    """a 2-D view of the map _patch_source returned for ops.grad_scale: the maximum does not depend on the layout"""
    from .. import ops_patch
    if t.is_contiguous():
        return t.view(-1, t.shape[1] if t.shape[1] % 4 == 0 else 4)
    rows = ops_patch.patch_rows_view(t, 1)
    return rows if rows is not None else _amax_rows(t.contiguous())


class PatchConvFunction(torch.autograd.Function):
    """A convolution whose kernel equals its stride (k x k / stride k / padding 0: the 1 x 1 projections, the 16 x 16 patch embedding), or a
    transposed 2 x 2 / stride 2 one, as ONE node of the graph: a linear over patch rows plus a layout change that is done once, by the
    producer of the GEMM operands (ops_patch.patch_pack, csrc/patch_pack.hip; a channels-last k == 1 map is its own rows and costs no pass).
    Patch row m = (b, h, w), column n = c k^2 + i k + j, W2 the 2-D view of the weight in that column order:
      convolution   W2 = weight.reshape(Cout, Cin k k)      y rows = X . W2^T + b                  ops.gemm on split operands
      transposed    W2 = weight.view(Cin, 4 Cout)           the k = 2 patch rows of y = X . W2 + b   the four row-mapped tap linears of
                                                            ops.convt2x2_split: no shuffle pass
    Both return a channels-last VIEW of the rows they wrote ((B, Cout, H/k, W/k) / (B, Cout, 2 H, 2 W)), as Conv3x3Function does.
    Backward, always device-scaled ({s, 1/s} = ops.grad_scale(dy); G = the patch rows of s dy, k = 1 / k = 2 for the transposed form):
      ONE pass over dy: G as HL8 rows if dx is needed, G^T if dW is needed, db = the channel sums of the unscaled dy if db is needed
      convolution   dx rows = (1/s) G . W2          dW2 = (1/s) G^T . X         (Cout, Cin k k)
      transposed    dx rows = (1/s) G . W2^T        dW2 = (1/s) X^T . G         (Cin, 4 Cout): one GEMM each, not four
    dx is returned as a channels-last view; dW in the weight's own shape, contiguous.  Saved: x and weight only -- X^T is produced in the
    backward by a pass over the saved x, no gathered copy is kept.  The weight products are cut into chunks over the rows and added in
    chunk order (_product_t, the scaled linears' own).  needs_input_grad is honoured: a frozen input, weight or bias skips its operand form and its
    GEMM.  A trainable input with k > 1 has no scatter kernel: patch_conv_train declines it (the patch embedding's input is the image)."""

    @staticmethod
    def forward(ctx, x, weight, bias, k, transposed):
        B, C, H, W = x.shape
        xs = _patch_source(x)
        rows = _patch_operands(xs, k, want_f32=True)[0]
        if transposed:
            Cout = weight.shape[1]
            y = ops.convt2x2_split(rows, weight, "patch_t", weight, None if bias is None else bias.detach(), B, H, W)
        else:
            Cout = weight.shape[0]
            w_hl8, _, _ = ops.split_weight(weight, "patch", [weight], lambda: weight.reshape(Cout, C * k * k))
            y = ops.gemm(rows, w_hl8, None if bias is None else bias.detach().contiguous(), split=True, out_fmt=ops.F32, tag="train_fwd")
            y = y.view(B, H // k, W // k, Cout)
        ctx.save_for_backward(x, weight)
        ctx.k, ctx.transposed, ctx.has_bias = int(k), bool(transposed), bias is not None
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None
        B, C, H, W = x.shape
        k, tr = ctx.k, ctx.transposed
        M = B * (H // k) * (W // k)
        g = _patch_source(dy)
        scale = ops.grad_scale(_amax_rows(g))
        inv = scale[1:]
        _, ga, gt, gb = _patch_operands(g, 2 if tr else 1, scale, want_rows=need_x, want_t=need_w, want_sum=need_b)
        dx = dw = None
        if need_x:
            if tr:                 # (N = Cin, K = 4 Cout): the weight's own view
                w2, _, _ = ops.split_weight(weight, "patch_t.dx", [weight], lambda: weight.reshape(C, -1))
            else:                  # k == 1: (N = Cin, K = Cout)
                w2, _, _ = ops.split_weight(weight, "patch.T", [weight], lambda: weight.reshape(weight.shape[0], C).t().contiguous())
            dx = ops.gemm_scaled(ga, w2, inv, split=True, out_fmt=ops.F32, tag="train_dx").view(B, H, W, C).permute(0, 3, 1, 2)
        if need_w:
            xt = _patch_operands(_patch_source(x), k, want_t=True)[2]
            dw = (_product_t(xt, gt, M, inv) if tr else _product_t(gt, xt, M, inv)).view(weight.shape)
        return dx, dw, gb, None, None


def patch_conv_train_ok(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, output_padding=0, transposed=False):
    """the limits of the training projection node: fp32 device tensors; groups 1, dilation 1, padding 0, no output padding, a square kernel
    equal to the stride (k = 2 for the transposed form) that divides H and W; both the contraction width and the output width of every
    GEMM the node launches multiples of 32 -- Cin k^2 % 32 == 0 and Cout % 32 == 0 for a convolution, Cin % 32 == 0 and Cout % 8 == 0 (the
    input gradient contracts over 4 Cout) for the transposed form -- which also makes every operand row a whole number of 16-byte pieces;
    fewer than 2^31 patch rows.  No lower limit on the row count: the GEMM entries take one row."""
    def one(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if x.dim() != 4 or weight.dim() != 4 or min(x.shape) < 1:
        return False
    k = weight.shape[2]
    if weight.shape[3] != k or one(stride) != (k, k) or one(padding) != (0, 0) or one(dilation) != (1, 1) or groups != 1:
        return False
    if one(output_padding) != (0, 0) or (not transposed and (x.shape[2] % k or x.shape[3] % k)):
        return False
    if transposed:
        Cin, Cout = weight.shape[0], weight.shape[1]
        if k != 2 or Cin % 32 or Cout % 8:
            return False
    else:
        Cout, Cin = weight.shape[0], weight.shape[1]
        if (Cin * k * k) % 32 or Cout % 32:
            return False
    if Cin != x.shape[1] or x.shape[0] * x.shape[2] * x.shape[3] >= 1 << 31 or (bias is not None and tuple(bias.shape) != (Cout,)):
        return False
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        return False
    return x.is_cuda and weight.is_cuda and (bias is None or bias.is_cuda)


def patch_conv_train(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    """conv2d with kernel == stride as one node (PatchConvFunction), or None outside patch_conv_train_ok's limits and for a TRAINABLE input
    with k > 1 (no scatter kernel): the caller's F.conv2d runs"""
    if not patch_conv_train_ok(x, weight, bias, stride, padding, dilation, groups):
        return None
    if weight.shape[2] > 1 and x.requires_grad and torch.is_grad_enabled():
        return None
    return PatchConvFunction.apply(x, weight, bias, weight.shape[2], False)


def patch_convt_train(x, weight, bias=None, stride=2, padding=0, output_padding=0, groups=1, dilation=1):
    """conv_transpose2d 2 x 2 / stride 2 as one node (PatchConvFunction), or None outside patch_conv_train_ok's limits: the caller's
    F.conv_transpose2d runs"""
    if not patch_conv_train_ok(x, weight, bias, stride, padding, dilation, groups, output_padding, transposed=True):
        return None
    return PatchConvFunction.apply(x, weight, bias, 1, True)


def _rows_ok(t):
    """rows the query-attention kernels read in place: contiguous columns, strides multiples of 4 elements, a 16-byte boundary"""
    return t.stride(2) == 1 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0


class QueryAttentionFunction(torch.autograd.Function):
    """the core of the decoder layers' query self-attention (nn.MultiheadAttention with q = k = tgt + query_pos, v = tgt, heads of 32 and the
    de-noising attn_mask: deformable_transformer_dino.py:418-436, dino_decoder.py:222-248) as ONE node between the in-projection and
    out_proj: qk (B, N, 2 C) rows of the q | k linear, v (B, N, C) rows, mask None | (N, N) bool (True = blocked) -> (B, N, C).
    forward = hipie_attn_f32_train_forward, backward = hipie_attn_f32_train_backward, exact fp32 (csrc/attn_f32_train.hip).
    Saved: qk, v, out, lse (B, heads, N) and the mask -- nothing of N x N elements besides the mask the caller owns.  The backward writes
    ONE d_qk buffer for both column blocks; a frozen input skips its launches."""

    @staticmethod
    def forward(ctx, qk, v, mask, heads):
        scale = 32 ** -0.5
        out, lse = ops.query_attn_train_forward(qk, v, mask, heads, scale)
        ctx.save_for_backward(qk, v, out, lse, mask)
        ctx.heads, ctx.scale = int(heads), scale
        return out

    @staticmethod
    def backward(ctx, d_out):
        want_qk, want_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_qk or want_v):
            return None, None, None, None
        qk, v, out, lse, mask = ctx.saved_tensors
        if d_out.dtype != torch.float32 or not _rows_ok(d_out):
            d_out = d_out.float().contiguous()
        d_qk, d_v = ops.query_attn_train_backward(qk, v, mask, out, lse, d_out, ctx.heads, ctx.scale, want_qk=want_qk, want_v=want_v)
        return d_qk, d_v, None, None


def query_attention_ok(qk, v, attn_mask, heads):
    """the limits of the training query-attention kernels: fp32 device rows qk (B, N, 2 C) and v (B, N, C) with C = heads * 32, read in
    place (contiguous columns, strides multiples of 4 elements, 16-byte boundaries); attn_mask None or an (N, N) bool on the same device"""
    if not (torch.is_tensor(qk) and torch.is_tensor(v) and qk.is_cuda and v.is_cuda and qk.dtype == torch.float32 and v.dtype == torch.float32):
        return False
    if qk.dim() != 3 or v.dim() != 3 or heads <= 0 or qk.shape[0] == 0 or qk.shape[1] == 0:
        return False
    B, N, C = v.shape
    if C != heads * 32 or tuple(qk.shape) != (B, N, 2 * C) or not _rows_ok(qk) or not _rows_ok(v):
        return False
    return attn_mask is None or (attn_mask.is_cuda and attn_mask.dtype == torch.bool and tuple(attn_mask.shape) == (N, N))


def query_attention(qk, v, attn_mask, heads):
    """softmax(q k^T / sqrt(32) with attn_mask) v of the decoders' query self-attention with a hand-written backward
    (QueryAttentionFunction) -> (B, N, C), or None outside the kernels' limits: the caller's materialised formulation runs"""
    if not query_attention_ok(qk, v, attn_mask, heads):
        return None
    return QueryAttentionFunction.apply(qk, v, None if attn_mask is None else attn_mask.contiguous(), heads)


class FusionAttentionFunction(torch.autograd.Function):
    """the core of the vision-language fusion attention (BiMultiHeadAttention.forward, fuse_helper.py:54-139) as ONE node between the four
    input projections and the two output projections, both directions: q (UNSCALED v_proj rows), vv (B, Nv, E), k, vl (B, L, E), att (B, L)
    bool (True = attended), heads of 256, the attention dropout rate and its 64-bit seed -> (out_v (B, Nv, E), out_l (B, L, E)).
    forward = hipie_bi_attn_train_forward, backward = hipie_bi_attn_train_backward, exact fp32 (csrc/bi_attn_train.hip).
    Saved: the four operands, out_v, out_l, the two (maximum, log2 sum) statistics (B, heads, Nv | L, 2), att; the seed and the rate in ctx --
    nothing of Nv x L elements.  The dropout masks are a stateless function of (seed, direction, b, h, i, j), recomputed in the backward;
    they are NOT F.dropout's random stream.  A frozen input skips the launches that serve only it.
    An image with no attended token is outside the contract: its out_v rows are 0 and that direction gives it no gradient (the reference
    gives a uniform row).  Not here: the folded form of the inference path, 16-bit operands, L > 256, a pad mask on the visual side
    (the reference has none), the block's LayerNorms and projections."""

    @staticmethod
    def forward(ctx, q, k, vv, vl, att, heads, dropout, seed):
        out_v, out_l, _, _, stat_v, stat_l = ops.bi_attn_train_forward(q, k, vv, vl, att, heads, dropout, seed)
        ctx.save_for_backward(q, k, vv, vl, att, out_v, out_l, stat_v, stat_l)
        ctx.heads, ctx.dropout, ctx.seed = int(heads), float(dropout), int(seed)
        return out_v, out_l

    @staticmethod
    def backward(ctx, d_out_v, d_out_l):
        want = tuple(ctx.needs_input_grad[:4])
        if not any(want):
            return (None,) * 8
        q, k, vv, vl, att, out_v, out_l, stat_v, stat_l = ctx.saved_tensors
        if d_out_v.dtype != torch.float32 or not _rows_ok(d_out_v):
            d_out_v = d_out_v.float().contiguous()
        if d_out_l.dtype != torch.float32 or not _rows_ok(d_out_l):
            d_out_l = d_out_l.float().contiguous()
        grads = ops.bi_attn_train_backward(q, k, vv, vl, att, out_v, out_l, stat_v, stat_l, d_out_v, d_out_l, ctx.heads, ctx.dropout, ctx.seed, want)
        return grads + (None, None, None, None)


def fusion_attention_ok(q, k, vv, vl, text_mask, heads, dropout):
    """the limits of the training fusion-attention kernels: fp32 device rows q, vv (B, Nv, E) and k, vl (B, L, E) with E = heads * 256, read in
    place (contiguous columns, strides multiples of 4 elements, 16-byte boundaries), 1 <= L <= 256, Nv >= 1, text_mask (B, L) on the same
    device, 0 <= dropout < 1"""
    ts = (q, k, vv, vl)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in ts):
        return False
    if not (torch.is_tensor(text_mask) and text_mask.is_cuda) or not 0.0 <= float(dropout) < 1.0 or heads <= 0:
        return False
    B, Nv, E = q.shape
    L = k.shape[1]
    if E != heads * 256 or B == 0 or Nv == 0 or not 1 <= L <= 256:
        return False
    if tuple(vv.shape) != (B, Nv, E) or tuple(k.shape) != (B, L, E) or tuple(vl.shape) != (B, L, E) or tuple(text_mask.shape) != (B, L):
        return False
    return all(_rows_ok(t) for t in ts)


def fusion_attention(q, k, vv, vl, text_mask, heads, dropout=0.0, seed=None):
    """both directions of the fusion attention from the UNSCALED v_proj rows q, the l_proj rows k and the two value projections, with a
    hand-written backward (FusionAttentionFunction) -> (out_v, out_l), or None outside the kernels' limits: the caller's materialised
    formulation runs.  seed None: with dropout > 0 one 64-bit seed per call from torch's default CPU generator (no device work; reproduces
    under torch.manual_seed), none drawn at dropout 0"""
    if not fusion_attention_ok(q, k, vv, vl, text_mask, heads, dropout):
        return None
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) if dropout > 0 else 0
    att = (text_mask != 0).contiguous()
    return FusionAttentionFunction.apply(q, k, vv, vl, att, heads, float(dropout), seed)


class PointMaskLossFunction(torch.autograd.Function):
    """the point-sampled mask losses of ONE criterion call as one node (criterion.loss_masks: point_sample of the predictions and of the
    targets, focal / sigmoid-CE + dice): src (N,H,W) logits, tgt_maps (T,Ht,Wt) ALL padded targets -- indexed by tgt_index (N,) inside the
    kernel, never gathered --, pts (N,P,2) -> (lmask (N,), ldice (N,)), the caller forms sum / count.  forward = ops.point_mask_loss_forward,
    backward = ops.point_mask_loss_backward.  Saved: the four inputs (dense: a strided view is copied once, before it is saved) and the
    (N,3) sums; the samples are recomputed -- nothing of N x P or N x Ht x Wt elements is kept.  Gradient for src only."""

    @staticmethod
    def forward(ctx, src, tgt_maps, tgt_index, pts, mode, alpha):
        # dense copies are made HERE, once: a strided view (the targets sub-sampled at the mask stride) would otherwise be copied by the
        # forward and again by the backward, and saving it would pin the storage it is a view of
        src, tgt_maps, tgt_index, pts = src.contiguous(), tgt_maps.contiguous(), tgt_index.contiguous(), pts.contiguous()
        lmask, ldice, sums = ops.point_mask_loss_forward(src, tgt_maps, tgt_index, pts, mode, alpha)
        ctx.save_for_backward(src, tgt_maps, tgt_index, pts, sums)
        ctx.mode, ctx.alpha = int(mode), float(alpha)
        return lmask, ldice

    @staticmethod
    def backward(ctx, g_mask, g_dice):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        src, tgt_maps, tgt_index, pts, sums = ctx.saved_tensors
        d_src = ops.point_mask_loss_backward(src, tgt_maps, tgt_index, pts, sums, g_mask.float().contiguous(), g_dice.float().contiguous(), ctx.mode,
                                             ctx.alpha)
        return (d_src,) + (None,) * 5


def point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha=-1.0):
    """(lmask (N,), ldice (N,)) on hipie_point_mask_loss_forward / _backward; mode 0 = sigmoid CE, 1 = focal (gamma 2, alpha; alpha < 0: none)"""
    return PointMaskLossFunction.apply(src, tgt_maps, tgt_index, pts, mode, alpha)


class TokenFocalFunction(torch.autograd.Function):
    """criterion.token_focal_loss as one node: the sum over (image, query, token) of the binary focal loss (gamma 2) of logits (B,Q,T)
    against onehot, pad tokens (text_mask (B,T) == 0) left out INSIDE the kernel -- no boolean indexing, so no host wait.
    forward = ops.token_focal_forward, backward = ops.token_focal_backward.  Gradient for logits only."""

    @staticmethod
    def forward(ctx, logits, onehot, text_mask, alpha):
        keep = None if text_mask is None else text_mask > 0
        ctx.save_for_backward(logits, onehot, keep)
        ctx.alpha = float(alpha)
        return ops.token_focal_forward(logits, onehot, keep, alpha)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 4
        logits, onehot, keep = ctx.saved_tensors
        return (ops.token_focal_backward(logits, onehot, keep, g.float(), ctx.alpha),) + (None,) * 3


def token_focal_sum(logits, onehot, text_mask=None, alpha=0.25):
    """scalar: token_focal_loss(logits, onehot, text_mask, alpha) on hipie_token_focal_forward / _backward"""
    return TokenFocalFunction.apply(logits, onehot, text_mask, alpha)


@torch.no_grad()
def uncertain_points(src, cand, rest, k, num_points=None):
    """criterion.uncertain_points after its two draws, on hipie_uncertain_points: src (N,H,W) logits, cand (N,C,2), rest (N,P-k,2) or None ->
    pts (N,P,2) in cand's dtype, the k candidates closest to logit 0 in ascending candidate index, then rest.  num_points: the caller's P; a
    rest that does not hold P - k points is refused.  The operands are cast to fp32 and made dense, as mask_match_costs does (the torch
    path takes any floating dtype).  No gradient; the key workspace lives for the call."""
    ws = torch.empty(ops.uncertain_points_ws_bytes(src.shape[0], cand.shape[1]), dtype=torch.uint8, device=src.device)
    pts = ops.uncertain_points(src.detach().float().contiguous(), cand.float().contiguous(), None if rest is None else rest.float().contiguous(), k,
                               num_points=num_points, ws=ws)
    return pts.to(cand.dtype)


@torch.no_grad()
def mask_match_costs(pred, tgt, coords):
    """matcher.mask_costs on hipie_mask_match_cost: pred (Q,H,W) logits, tgt (T,Ht,Wt), coords (P,2) -> (ce (Q,T), dice (Q,T)).  No gradient; the
    workspace (the sampled targets and the partial sums) lives for the call."""
    ws = torch.empty(ops.mask_match_cost_ws_bytes(pred.shape[0], tgt.shape[0], coords.shape[0]), dtype=torch.uint8, device=pred.device)
    return ops.mask_match_cost(pred.detach().float().contiguous(), tgt.float().contiguous(), coords.float().contiguous(), ws=ws)


OtaTargets = collections.namedtuple("OtaTargets", "tgt_boxes pos_map n_tgt counts")
OTA_STATUS = ((1, "a box with x1 < x0 or y1 < y0"), (2, "a target without a positive token"), (4, "the repair loop did not end within Q rounds"))


@torch.no_grad()
def pack_ota_targets(targets, device):
    """the targets of one step as hipie_ota_cost reads them, packed ONCE for all decoder levels: per-image dicts with "boxes" (T_i, 4) cxcywh
    and "positive_map" (T_i, L) -> OtaTargets(tgt_boxes (B,Tmax,4) fp32 and pos_map (B,Tmax,L) uint8, zero behind T_i; n_tgt (B,) int32 on
    the device; counts: the T_i as a host list).  Images without targets take no row; L is that of the maps (0 when no image has a map)."""
    counts = [int(t["boxes"].shape[0]) for t in targets]
    B, Tmax = len(targets), max(counts, default=0)
    L = max((int(t["positive_map"].shape[1]) for t in targets if "positive_map" in t), default=0)
    tgt_boxes = torch.zeros(B, Tmax, 4, dtype=torch.float32, device=device)
    pos_map = torch.zeros(B, Tmax, L, dtype=torch.uint8, device=device)
    for b, (t, n) in enumerate(zip(targets, counts)):
        if n:
            if t["positive_map"].shape != (n, L):
                raise ValueError("pack_ota_targets: positive_map of image %d is %s, expected %s" % (b, tuple(t["positive_map"].shape), (n, L)))
            tgt_boxes[b, :n] = t["boxes"].to(device)
            pos_map[b, :n] = (t["positive_map"] != 0).to(device)
    return OtaTargets(tgt_boxes, pos_map, torch.tensor(counts, dtype=torch.int32).to(device), counts)


@torch.no_grad()
def ota_match(logits, boxes, packed, center_radius=2.5, stride=32):
    """HungarianMatcher.forward_ota on hipie_ota_cost + hipie_ota_assign: logits (B,Q,L), boxes (B,Q,4), packed = pack_ota_targets(...) ->
    (pairs, best) in forward_ota's format: per image (query idx, target idx of each), int64 on the device, slices of the kernel's compacted
    lists cut with the counts of ONE host copy; per image the best query of every target (images without targets: the empty pair and []).
    Two launches for the batch.  A status bit raises ValueError (a degenerate box: the reference's assert; a target without a positive token;
    a repair loop that does not end).  Shapes outside the kernels' limits (Q <= 4096, Tmax <= 256, L <= 1024): None, the torch path runs."""
    B, Q, L = logits.shape
    Tmax = packed.tgt_boxes.shape[1]
    if len(packed.counts) != B or (Tmax and packed.pos_map.shape[2] != L):
        raise ValueError("ota_match: targets packed for %d images and %d tokens, logits are %s" % (len(packed.counts), packed.pos_map.shape[2], tuple(logits.shape)))
    dev = logits.device
    if Q > ops.OTA_MAX_Q or Tmax > ops.OTA_MAX_T or L > ops.OTA_MAX_L:
        return None
    if Q == 0 or Tmax == 0:
        e = torch.zeros(0, dtype=torch.int64, device=dev)
        return [(e, e.clone()) for _ in range(B)], [[] if n == 0 else e.clone() for n in packed.counts]
    cost, iou, res = ops.ota_cost(logits.detach().float().contiguous(), boxes.detach().float().contiguous(), packed.tgt_boxes, packed.pos_map, packed.n_tgt,
                                  center_radius, stride)
    pair_q, pair_t, best, res = ops.ota_assign(cost, iou, packed.n_tgt, res)
    n_pairs, status, _ = res.cpu().tolist()                  # the one host read of the call
    for b, s in enumerate(status):
        if s:
            raise ValueError("ota_match: image %d: %s" % (b, "; ".join(msg for bit, msg in OTA_STATUS if s & bit)))
    pair_q, pair_t, best = pair_q.long(), pair_t.long(), best.long()
    pairs = [(pair_q[b, :n], pair_t[b, :n]) for b, n in enumerate(n_pairs)]
    return pairs, [best[b, :n] if n else [] for b, n in enumerate(packed.counts)]


MatchTargets = collections.namedtuple("MatchTargets", "tgt_boxes pos_map labels is_thing n_tgt t_off counts tgt_masks")


@torch.no_grad()
def pack_match_targets(targets, device, with_masks=True, with_counts=True):
    """the targets of a Hungarian matcher as hipie_hungarian_cost reads them, packed ONCE for many calls (every decoder level, every output of a
    criterion call): per-image dicts with "boxes" (T_i, 4) cxcywh, "positive_map" (T_i, L) and / or "labels" (T_i,), optionally "is_thing"
    (T_i,; absent: every target is a thing) and "masks" (T_i, H_i, W_i) -> MatchTargets(tgt_boxes (B,Tmax,4) fp32, pos_map (B,Tmax,L) uint8 or
    None when no image has a map, labels (B,Tmax) int32 or None when an image with targets has none, is_thing (B,Tmax) uint8 -- all zero behind
    T_i; n_tgt and t_off (B,) int32 on the device, t_off the exclusive prefix sum; counts: the T_i as a host list; tgt_masks: per image the
    fp32 dense masks on the device, or None (with_masks=False, or an image with targets has none)).  with_counts=False: n_tgt and t_off are
    None and NOTHING is copied from the host -- the packing of pack_pair_targets, whose readers take the counts from the pair lists."""
    counts = [int(t["boxes"].shape[0]) for t in targets]
    B, Tmax = len(targets), max(counts, default=0)
    has_map = any("positive_map" in t for t in targets)
    L = max((int(t["positive_map"].shape[1]) for t in targets if "positive_map" in t), default=0)
    tgt_boxes = torch.zeros(B, Tmax, 4, dtype=torch.float32, device=device)
    pos_map = torch.zeros(B, Tmax, L, dtype=torch.uint8, device=device) if has_map else None
    has_labels = all("labels" in t for t, n in zip(targets, counts) if n)
    labels = torch.zeros(B, Tmax, dtype=torch.int32, device=device) if has_labels else None
    is_thing = torch.zeros(B, Tmax, dtype=torch.uint8, device=device)
    for b, (t, n) in enumerate(zip(targets, counts)):
        if n:
            if has_map and (t.get("positive_map") is None or t["positive_map"].shape != (n, L)):
                raise ValueError("pack_match_targets: positive_map of image %d is %s, expected %s"
                                 % (b, None if t.get("positive_map") is None else tuple(t["positive_map"].shape), (n, L)))
            tgt_boxes[b, :n] = t["boxes"].to(device)
            if has_map:
                pos_map[b, :n] = (t["positive_map"] != 0).to(device)
            if has_labels:
                labels[b, :n] = t["labels"].to(device)
            is_thing[b, :n] = (t["is_thing"] != 0).to(device) if "is_thing" in t else 1
    offs = [0]
    for n in counts[:-1]:
        offs.append(offs[-1] + n)
    # one host -> device copy for the two count vectors
    if not with_counts:
        both = (None, None)
    else:
        both = torch.tensor([counts, offs[:B]], dtype=torch.int32).to(device) if B else torch.zeros(2, 0, dtype=torch.int32, device=device)
    tgt_masks = None
    if with_masks and all("masks" in t for t, n in zip(targets, counts) if n):
        tgt_masks = [t["masks"].to(device).float().contiguous() if n else None for t, n in zip(targets, counts)]
    return MatchTargets(tgt_boxes, pos_map, labels, is_thing, both[0], both[1], counts, tgt_masks)


def _hungarian_device_costs(what, logits, boxes, packed, w, masks, coords, stuff_takes_mean, with_boxes, class_mode):
    """everything of hungarian_costs / hungarian_match in front of the first use of the costs: the checks, the mask costs of every image and
    hipie_hungarian_cost -> None (a shape outside the kernel's limits: the torch path runs), or (out, offs): the packed device buffer of
    ops.hungarian_cost (None when there is nothing to compute: no image, no query or no target) and the host list of the images' offsets"""
    B, Q, L = logits.shape
    Tmax, sum_t = packed.tgt_boxes.shape[1], sum(packed.counts)
    if len(packed.counts) != B:
        raise ValueError("%s: targets packed for %d images, logits are %s" % (what, len(packed.counts), tuple(logits.shape)))
    use_map = packed.pos_map is not None if class_mode == "auto" else class_mode == "map"
    if use_map and packed.pos_map is None:
        raise KeyError("%s: targets have no positive_map" % what)
    if not use_map and packed.labels is None:
        raise KeyError("%s: targets have no labels" % what)
    if use_map and Tmax and packed.pos_map.shape[2] != L:
        raise ValueError("%s: targets packed for %d tokens, logits are %s" % (what, packed.pos_map.shape[2], tuple(logits.shape)))
    if masks is not None and packed.tgt_masks is None:
        raise KeyError("%s: targets were packed without masks" % what)
    if Q > ops.HUNGARIAN_MAX_Q or Tmax > ops.HUNGARIAN_MAX_T or L > ops.HUNGARIAN_MAX_L or L < 1 or B > 65535:
        return None
    offs = [0]
    for n in packed.counts[:-1]:
        offs.append(offs[-1] + n)
    if B == 0 or Q == 0 or sum_t == 0:
        return None, offs[:B]
    dev = logits.device

    def images(t, row):                       # a slice of the query dimension keeps its images dense: no copy
        t = t.detach()
        if t.dtype != torch.float32:
            t = t.float()
        return t if t.stride(2) == 1 and t.stride(1) == row and (B == 1 or t.stride(0) >= Q * row) else t.contiguous()
    ce = dice = None
    if masks is not None:
        both = torch.empty(2, Q * sum_t, dtype=torch.float32, device=dev)
        ce, dice = both[0], both[1]
        for b, n in enumerate(packed.counts):
            if n:
                pred, pts = masks[b].detach().float().contiguous(), coords[b].float().contiguous()
                ws = torch.empty(ops.mask_match_cost_ws_bytes(Q, n, pts.shape[0]), dtype=torch.uint8, device=dev)
                lo, hi = Q * offs[b], Q * (offs[b] + n)
                ops.mask_match_cost(pred, packed.tgt_masks[b], pts, ws=ws, ce_out=ce[lo:hi].view(Q, n), dice_out=dice[lo:hi].view(Q, n))
    out = ops.hungarian_cost(images(logits, L), images(boxes, 4) if with_boxes else None, packed.tgt_boxes, packed.n_tgt, packed.t_off, sum_t,
                             (w.cls, w.l1, w.giou, w.mask, w.dice), pos_map=packed.pos_map if use_map else None,
                             labels=None if use_map else packed.labels, is_thing=packed.is_thing, ce=ce, dice=dice, with_boxes=with_boxes,
                             stuff_takes_mean=stuff_takes_mean)
    return out, offs


@torch.no_grad()
def hungarian_costs(logits, boxes, packed, w, masks=None, coords=None, stuff_takes_mean=True, with_boxes=True, class_mode="auto"):
    """matcher.cost_matrix of every image of a batch on hipie_hungarian_cost (+ hipie_mask_match_cost per image with `masks`): logits (B,Q,L),
    boxes (B,Q,4), packed = pack_match_targets(...), w: matcher.MatchWeights; masks: None or per image the (Q,H,W) mask logits, coords: then per
    image the (P,2) points -> per image the (Q, T_i) cost matrix as a float32 numpy array on the HOST, views of ONE device -> host copy that
    carries the costs of all images and their status words.  The mask costs of an image land directly in its block of the packed operands.
    class_mode as matcher.class_cost: "map", "ids", or "auto" (the map when the targets have one).  A status bit raises ValueError and names the
    image (a degenerate box: the ValueError of boxes.generalized_box_iou; a label outside [0, L)).  Shapes outside the kernel's limits
    (Q <= 4096, Tmax <= 256, L <= 1024, B <= 65535): None, the torch path runs."""
    got = _hungarian_device_costs("hungarian_costs", logits, boxes, packed, w, masks, coords, stuff_takes_mean, with_boxes, class_mode)
    if got is None:
        return None
    out, offs = got
    Q, sum_t = logits.shape[1], sum(packed.counts)
    if out is None:
        return [np.zeros((Q, n), dtype=np.float32) for n in packed.counts]
    host = out.cpu().numpy()                                  # the one host read of the call: the costs and the status words
    status = host[Q * sum_t:].view(np.int32)
    for b, s in enumerate(status.tolist()):
        if s:
            raise ValueError("hungarian_costs: image %d: %s" % (b, "; ".join(msg for bit, msg in ops.HUNGARIAN_STATUS if s & bit)))
    return [host[Q * o:Q * (o + n)].reshape(Q, n) for o, n in zip(offs, packed.counts)]


@torch.no_grad()
def hungarian_match(logits, boxes, packed, w, masks=None, coords=None, stuff_takes_mean=True, with_boxes=True, class_mode="auto"):
    """HungarianMatcher.forward / forward_boxes_only without a host wait: the costs of hungarian_costs stay on the device and
    hipie_hungarian_assign solves every image's assignment there (scipy's pairs, tie for tie) -> (pairs, status): per image (query idx, target
    idx) int64 on the DEVICE, views of the kernel's (B, K) outputs whose lengths min(Q, T_i) the host knows from the packed counts; status (B,)
    int32 on the device (ops.HUNGARIAN_STATUS): the caller decides when to read it (HungarianMatcher: at once, or at check()).  An image with a non-zero
    status has all-zero pairs, which index nothing out of range.  The same arguments as hungarian_costs, and None under the same conditions."""
    got = _hungarian_device_costs("hungarian_match", logits, boxes, packed, w, masks, coords, stuff_takes_mean, with_boxes, class_mode)
    if got is None:
        return None
    out, offs = got
    B, Q = logits.shape[:2]
    dev = logits.device
    if out is None:
        e = torch.zeros(0, dtype=torch.int64, device=dev)
        return [(e, e.clone()) for _ in range(B)], torch.zeros(B, dtype=torch.int32, device=dev)
    pair_q, pair_t, status = ops.hungarian_assign(out, packed.n_tgt, packed.t_off, sum(packed.counts), Q, packed.tgt_boxes.shape[1])
    return [(pair_q[b, :min(Q, n)], pair_t[b, :min(Q, n)]) for b, n in enumerate(packed.counts)], status



class PairBoxLossFunction(torch.autograd.Function):
    """the box losses of the matched pairs of ONE criterion call as one node (criterion.DetCriterion.loss_boxes: mode 0, MaskCriterion.loss_boxes:
    mode 1): pred_boxes (B,Q,4) -- a slice of the query axis is read through its strides, never copied --, pred_iou None | (B,Q) logits, pairs:
    per image (query idx, target idx) int64 on the device, tgt_boxes / is_thing of pack_match_targets, the normaliser `count` -> (loss_bbox,
    loss_giou, loss_boxiou, status): the FINAL scalars (views of one 8-element buffer) and the (1,) int32 status word (ops.PAIR_STATUS), which
    nobody reads here.  forward = ops.pair_box_loss_forward, backward = ops.pair_box_loss_backward with the three upstream scalars taken from
    the device.  Kept for the backward: that buffer, the (K,9) per-pair gradients and the pair lists -- no operand.  Gradients for pred_boxes
    and pred_iou only."""

    @staticmethod
    def forward(ctx, pred_boxes, pred_iou, pairs, tgt_boxes, is_thing, count, mode):
        out, pair_grad, status = ops.pair_box_loss_forward(pred_boxes, pred_iou, pairs, tgt_boxes, is_thing, count, mode)
        ctx.save_for_backward(out, pair_grad)
        ctx.pairs, ctx.shape, ctx.iou_shape = pairs, pred_boxes.shape, None if pred_iou is None else pred_iou.shape
        ctx.mark_non_differentiable(status)
        return out[0], out[1], out[2], status

    @staticmethod
    def backward(ctx, g_bbox, g_giou, g_boxiou, _):
        want_iou = ctx.iou_shape is not None and ctx.needs_input_grad[1]
        if not (ctx.needs_input_grad[0] or want_iou):
            return (None,) * 7
        out, pair_grad = ctx.saved_tensors
        d_boxes, d_iou = ops.pair_box_loss_backward(ctx.pairs, out, pair_grad, g_bbox.float(), g_giou.float(), g_boxiou.float(), ctx.shape[0],
                                                    ctx.shape[1], want_iou)
        return (d_boxes if ctx.needs_input_grad[0] else None, d_iou.reshape(ctx.iou_shape) if want_iou else None) + (None,) * 5


def pack_pair_targets(targets, device):
    """the targets of a criterion call as pair_box_loss / positive_onehot read them: pack_match_targets without masks and without the count
    vectors, whose host -> device copy is a host wait (tgt_boxes, is_thing, pos_map, the counts as a host list).  A packing the matcher
    already made (pack_match_targets) serves as well."""
    return pack_match_targets(targets, device, with_masks=False, with_counts=False)


def _device_pairs(pairs, device):
    """the pairs as the kernels read them: int64, contiguous, on `device` (what the device matchers and dn_match_indices return is passed on
    as it is; host pairs -- a matcher that ran its torch path -- are copied over)"""
    def one(x):
        if x.device != device or x.dtype != torch.int64:
            x = x.to(device=device, dtype=torch.int64)
        return x.reshape(-1) if x.is_contiguous() and x.dim() == 1 else x.reshape(-1).contiguous()
    return [(one(q), one(t)) for q, t in pairs]


def _pairs_fit(pairs, B):
    return len(pairs) == B and B <= ops.PAIR_MAX_B and sum(int(q.shape[0]) for q, _ in pairs) <= ops.PAIR_MAX_K


def pair_box_loss(pred_boxes, pred_iou, pairs, packed, count, mode, use_thing=True):
    """loss_boxes of a criterion call on hipie_pair_box_loss_forward / _backward: pred_boxes (B,Q,4), pred_iou None | (B,Q) | (B,Q,1) logits (mode
    0 only), pairs: per image (query idx, target idx), packed = pack_pair_targets(targets, device) (or a pack_match_targets packing), count: the normaliser the
    criterion divides by (under `ota` the number of pairs), mode 0 = DetCriterion, 1 = MaskCriterion, use_thing: weight (mode 0) / keep (mode 1)
    the pairs by the targets' is_thing -> (loss_bbox, loss_giou, loss_boxiou | None, status (1,) int32 on the device), or None: the criterion's
    torch path runs.  The limits: fp32 operands whose last dimension is dense, B <= 64 images, 1 <= K <= 65536 pairs (K = 0 is the criterion's
    own `src.sum() * 0.0`: no launch), targets packed for the same B.  No host wait and no host -> device copy."""
    if pred_boxes.dim() != 3 or pred_boxes.shape[2] != 4 or pred_boxes.dtype != torch.float32 or pred_boxes.stride(2) != 1:
        return None
    B, Q = pred_boxes.shape[:2]
    if pred_iou is not None:
        if mode != 0 or pred_iou.dtype != torch.float32 or tuple(pred_iou.shape) not in ((B, Q), (B, Q, 1)):
            return None
        pred_iou = pred_iou.reshape(B, Q) if pred_iou.dim() == 2 else pred_iou[:, :, 0]
    if not _pairs_fit(pairs, B) or sum(int(q.shape[0]) for q, _ in pairs) == 0 or packed.tgt_boxes.shape[0] != B:
        return None
    lb, lg, li, status = PairBoxLossFunction.apply(pred_boxes, pred_iou, _device_pairs(pairs, pred_boxes.device), packed.tgt_boxes,
                                                   packed.is_thing if use_thing else None, float(count), int(mode))
    return lb, lg, (li if pred_iou is not None else None), status


@torch.no_grad()
def positive_onehot(logits, pairs, packed):
    """criterion._positive_onehot on hipie_positive_onehot: logits (B,Q,L) fp32, pairs as above, packed.pos_map (B,Tmax,L) uint8 -> onehot (B,Q,L)
    of exact 0 / 1, or None: the criterion's loop runs (logits of another dtype, targets packed without maps or for another B or L, B > 64, more
    than 65536 pairs).  The CALLER decides from the dtype of the targets' maps whether the packed map ((map != 0) as bytes) equals them."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or packed.pos_map is None:
        return None
    B, Q, L = logits.shape
    if not _pairs_fit(pairs, B) or packed.pos_map.shape[0] != B or (packed.pos_map.shape[1] and packed.pos_map.shape[2] != L):
        return None
    if packed.pos_map.shape[1] == 0:                           # no image has a target: nothing to scatter (pack_match_targets then has no L)
        return torch.zeros_like(logits)
    return ops.positive_onehot(_device_pairs(pairs, logits.device), packed.pos_map, Q)
