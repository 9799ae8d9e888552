"""Every op of hipie_amd/ops.py that hands a tensor's address to the library refuses a host tensor before the call: the table below holds one
call per public op with correctly shaped HOST tensors at the smallest legal sizes, and `_call` / `_size` are replaced by functions that fail the
test, so nothing here needs the built library or a GPU and no host pointer can reach a kernel.  The `gpu` cases put ONE operand on the host and
the rest on the device (still with `_call` replaced: nothing is launched)."""
import inspect
import re

import pytest
import torch

from hipie_amd import ops

REFUSAL = "Not implemented on the CPU"


def f32(*s):
    return torch.zeros(*s)


def f16(*s):
    return torch.zeros(*s, dtype=torch.float16)


def u8(*s):
    return torch.zeros(*s, dtype=torch.uint8)


def i32(*s):
    return torch.zeros(*s, dtype=torch.int32)


def i64(*s):
    return torch.zeros(*s, dtype=torch.int64)


def mlp(n):
    head = torch.nn.Module()
    head.layers = torch.nn.ModuleList(torch.nn.Linear(2, 2) for _ in range(n))
    return head


MSDA = (f32(1, 4, 1, 32), i64(1, 2), i64(1), f32(1, 1, 1, 1, 1, 2), f32(1, 1, 1, 1, 1))          # value, shapes, level starts, locations, weights
RAW = (MSDA[0], MSDA[1], MSDA[2], f32(1, 1, 1, 2), MSDA[3], f32(1, 1, 1, 1))                       # value, shapes, level starts, ref, offsets, logits
Q4, QH = f32(1, 1, 1, 32), f16(1, 1, 1, 32)
QKV, TAB = f16(1, 1, 192), f16(1, 64)
ROW8, W8, X4 = f32(1, 8), f32(8), f32(1, 8, 1, 1)
PAIRS = [(i64(1), i64(1))]
N1 = i32(1)
BIG, WIN = (f16(1, 128, 224),) * 2, (f16(1, 1, 128),) * 2
E256 = f32(1, 1, 256)
HL, WHL = f16(1, 64), f16(8, 64)
GRID = f32(17, 1)          # conv3x3_stage of a (1, 1, 1, 1) map: 9 grid rows and 4 guard rows on both ends

HOST = {
    "ms_deform_attn_forward": lambda: ops.ms_deform_attn_forward(*MSDA),
    "ms_deform_attn_backward": lambda: ops.ms_deform_attn_backward(*MSDA, f32(1, 1, 32)),
    "msda_fused": lambda: ops.msda_fused(*RAW),
    "msda_raw_backward": lambda: ops.msda_raw_backward(*RAW, f32(1, 1, 32)),
    "flash_attn": lambda: ops.flash_attn(QH, QH, QH, 1.0),
    "bi_i2t_split": lambda: ops.bi_i2t_split(f16(1, 1, 64), f32(1, 1, 32), f32(1, 1, 32), u8(1, 1), 1),
    "bi_i2t_folded": lambda: ops.bi_i2t_folded(f16(1, 1, 16), f32(1, 1, 1, 8), f32(1, 1, 1), f32(1, 1, 32), u8(1, 1), 1, f32(8, 32), f32(8)),
    "attn_f32": lambda: ops.attn_f32(Q4, Q4, Q4, 1.0),
    "attn_f32_rows": lambda: ops.attn_f32_rows(Q4, Q4, Q4, 1.0, u8(1, 1, 1)),
    "attn_split": lambda: ops.attn_split(Q4, Q4, Q4, 1.0),
    "query_attn_train_forward": lambda: ops.query_attn_train_forward(f32(1, 1, 64), f32(1, 1, 32), None, 1, 1.0),
    "query_attn_train_backward": lambda: ops.query_attn_train_backward(f32(1, 1, 64), f32(1, 1, 32), None, f32(1, 1, 32), f32(1, 1, 1), f32(1, 1, 32), 1, 1.0),
    "bi_attn_train_forward": lambda: ops.bi_attn_train_forward(E256, E256, E256, E256, u8(1, 1), 1),
    "bi_attn_train_backward": lambda: ops.bi_attn_train_backward(E256, E256, E256, E256, u8(1, 1), E256, E256, f32(1, 1, 1, 2), f32(1, 1, 1, 2), E256, E256, 1),
    "vit_attn": lambda: ops.vit_attn(QKV, f32(1, 1, 1), f32(1, 1, 1), (1, 1), 1, 1.0),
    "vit_attn_fused": lambda: ops.vit_attn_fused(QKV, TAB, TAB, (1, 1), 1, 1.0),
    "vit_attn_rel": lambda: ops.vit_attn_rel(QKV, TAB, TAB, (1, 1), 1),
    "vit_attn_split": lambda: ops.vit_attn_split(f16(1, 1, 384), f16(1, 128), f16(1, 128), (1, 1), 1),
    "vit_relpos": lambda: ops.vit_relpos(QKV, TAB, TAB, (1, 1), 1),
    "bi_xattn": lambda: ops.bi_xattn(QH, QH, QH, QH, u8(1, 1)),
    "mask_einsum": lambda: ops.mask_einsum(ROW8[None], X4),
    "mask_einsum_backward": lambda: ops.mask_einsum_backward(ROW8[None], X4, f32(1, 1, 1, 1)),
    "mask_einsum16": lambda: ops.mask_einsum16(ROW8[None], X4.half()),
    "dynamic_mask": lambda: ops.dynamic_mask(X4, f32(1, 2), f32(1, 169), 1),
    "dynamic_mask_backward": lambda: ops.dynamic_mask_backward(X4, f32(1, 2), f32(1, 169), f32(1, 2, 2), 1),
    "add_layernorm": lambda: ops.add_layernorm(ROW8, None, W8, W8, 1e-5, torch.float32),
    "add_layernorm_sum": lambda: ops.add_layernorm_sum(ROW8, ROW8, W8, W8, 1e-5, ROW8),
    "add_layernorm_dec": lambda: ops.add_layernorm_dec(ROW8, ROW8, W8, W8, 1e-5, torch.float16),
    "layernorm_backward": lambda: ops.layernorm_backward(ROW8, ROW8, W8, 1e-5),
    "act_forward": lambda: ops.act_forward(ROW8, ops.ACT_RELU),
    "act_backward": lambda: ops.act_backward(ROW8, ROW8, ops.ACT_RELU),
    "point_mask_loss_forward": lambda: ops.point_mask_loss_forward(f32(1, 2, 2), f32(1, 2, 2), i64(1), f32(1, 1, 2), 0),
    "point_mask_loss_backward": lambda: ops.point_mask_loss_backward(f32(1, 2, 2), f32(1, 2, 2), i64(1), f32(1, 1, 2), f32(1, 3), f32(1), f32(1), 0),
    "token_focal_forward": lambda: ops.token_focal_forward(f32(1, 1, 1), f32(1, 1, 1)),
    "token_focal_backward": lambda: ops.token_focal_backward(f32(1, 1, 1), f32(1, 1, 1), None, f32(())),
    "uncertain_points": lambda: ops.uncertain_points(f32(1, 2, 2), f32(1, 2, 2), None, 1),
    "mask_match_cost": lambda: ops.mask_match_cost(f32(1, 2, 2), f32(1, 2, 2), f32(1, 2)),
    "ota_cost": lambda: ops.ota_cost(f32(1, 1, 1), f32(1, 1, 4), f32(1, 1, 4), u8(1, 1, 1), N1),
    "ota_assign": lambda: ops.ota_assign(f32(1, 1, 1), f32(1, 1, 1), N1),
    "hungarian_cost": lambda: ops.hungarian_cost(f32(1, 1, 1), f32(1, 1, 4), f32(1, 1, 4), N1, N1, 1, (1.0,) * 5, pos_map=u8(1, 1, 1), is_thing=u8(1, 1)),
    "hungarian_assign": lambda: ops.hungarian_assign(f32(2), N1, N1, 1, 1, 1),
    "pair_box_loss_forward": lambda: ops.pair_box_loss_forward(f32(1, 1, 4), None, PAIRS, f32(1, 1, 4), None, 1.0, 0),
    "pair_box_loss_backward": lambda: ops.pair_box_loss_backward(PAIRS, f32(8), f32(1, 9), f32(1), f32(1), f32(1), 1, 1, False),
    "positive_onehot": lambda: ops.positive_onehot(PAIRS, u8(1, 1, 1), 1),
    "optim_grad_norm": lambda: ops.optim_grad_norm(i64(1, 6), i64(1, 2)),
    "optim_adamw_step": lambda: ops.optim_adamw_step(i64(1, 6), i64(1, 2), i32(1), f32(1, 2), [1e-3], [0.0], (0.9, 0.999), 1e-8),
    "group_norm": lambda: ops.group_norm(X4, 1, W8, W8, 1e-5),
    "group_norm_train_forward": lambda: ops.group_norm_train_forward(X4, 1, W8, W8, 1e-5),
    "group_norm_backward": lambda: ops.group_norm_backward(X4, X4, f32(1, 1, 2), 1, W8, W8),
    "add_cast": lambda: ops.add_cast(f32(4), f16(4)),
    "add_to_hl8": lambda: ops.add_to_hl8(ROW8, f16(1, 16)),
    "batched_nms": lambda: ops.batched_nms(f32(1, 1, 4), f32(1, 1), i64(1, 1), 0.5),
    "mask_finalize": lambda: ops.mask_finalize(f32(1, 1, 1), None, 1, (1, 1), (1, 1), 0.5),
    "sem_pan": lambda: ops.sem_pan(f32(1, 1, 1), f32(1, 1), f32(1), 1, (1, 1), (1, 1)),
    "sine_embed": lambda: ops.sine_embed(f32(1, 2)),
    "ref_point_mlp": lambda: ops.ref_point_mlp(f32(1, 1, 4), mlp(2)),
    "box_head": lambda: ops.box_head(f32(1, 256), f32(1, 4), mlp(3)),
    "box_refine": lambda: ops.box_refine(f32(1, 4), f32(1, 4)),
    "selftest": lambda: ops.selftest(0, f32(4)),
    "to_hl8": lambda: ops.to_hl8(ROW8),
    "to_hl8_t": lambda: ops.to_hl8_t(ROW8),
    "f16_pair": lambda: ops.f16_pair(ROW8),
    "attn_train_forward": lambda: ops.attn_train_forward(BIG, BIG, (f16(1, 128, 80),) * 2),
    "attn_train_backward": lambda: ops.attn_train_backward(BIG, BIG, (f16(1, 128, 96),) * 2, (f16(1, 128, 96),) * 2, f32(1, 128), f32(1, 128)),
    "attn_train_win_forward": lambda: ops.attn_train_win_forward(WIN, WIN, (f16(1, 1, 80),) * 2),
    "attn_train_win_backward": lambda: ops.attn_train_win_backward(WIN, WIN, (f16(1, 1, 96),) * 2, (f16(1, 1, 96),) * 2, f32(1, 1), f32(1, 1)),
    "attn_pack_kv": lambda: ops.attn_pack_kv(f32(1, 1, 240), 1, 1, 1, 128),
    "attn_pack_q": lambda: ops.attn_pack_q(f32(1, 1, 80), f32(1, 1, 1, 1), f32(1, 1, 1, 1), 1, 1, 1, 128),
    "attn_grad_amax": lambda: ops.attn_grad_amax(f32(4)),
    "attn_pack_grad": lambda: ops.attn_pack_grad(f32(1, 1, 80), f32(1, 1, 80), (f16(1, 1, 80),) * 2, f32(1), 1, 1, 1),
    "attn_unpack_grad": lambda: ops.attn_unpack_grad(f32(1, 1, 128), f32(1, 1, 80), f32(1, 1, 80), f32(1, 1, 1, 80), None, f32(1), 1, 1, 1),
    "fill_rows": lambda: ops.fill_rows(f32(1, 4), N1, f32(4)),
    "gemm": lambda: ops.gemm(HL, WHL, split=True),
    "gemm_scaled": lambda: ops.gemm_scaled(HL, WHL, None, split=True),
    "gemm_split_k": lambda: ops.gemm_split_k(HL, WHL, 1),
    "gemm_split_k_scaled": lambda: ops.gemm_split_k_scaled(HL, WHL, 1, None),
    "grad_scale": lambda: ops.grad_scale(f32(1, 4)),
    "grad_pack": lambda: ops.grad_pack(ROW8, f32(2)),
    "matmul_nt_batched": lambda: ops.matmul_nt_batched(f32(1, 1, 32), f32(1, 8, 32)),
    "conv3x3_split": lambda: ops.conv3x3_split(f32(1, 1, 1, 1), torch.nn.Conv2d(1, 1, 3, padding=1)),
    "conv3x3_grid": lambda: ops.conv3x3_grid(GRID, f16(8, 18), None, 1, 1, 1),
    "conv3x3_wgrad": lambda: ops.conv3x3_wgrad(GRID, GRID, None, 1, 1, 1),
    "ffn_fused": lambda: ops.ffn_fused(f16(1, 512), torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)),
    "to_f8x": lambda: ops.to_f8x(HL),
    "gemm_f8x": lambda: ops.gemm_f8x(HL, u8(8, 128), u8(8, 1, 2)),
    "split_linear_ln": lambda: ops.split_linear_ln(f32(1, 32), torch.nn.Module(), "w", f32(256, 32), None, f32(1, 256), f32(256), f32(256), 1e-5),
    "topk": lambda: ops.topk(f32(1, 4), 1),
}

EXEMPT = ()          # public ops that reach _call without taking a tensor: none today (the *_ws_bytes queries and optim_chunk go through _size)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda name, *a: pytest.fail("%s reached the library" % name))
    monkeypatch.setattr(ops, "_size", lambda name, *a: pytest.fail("%s reached the library" % name))


@pytest.mark.parametrize("name", sorted(HOST))
def test_host_tensors_are_refused_before_the_library(no_library, name):
    with pytest.raises(RuntimeError, match=REFUSAL):
        HOST[name]()


def _source(fn):
    return inspect.getsource(inspect.unwrap(fn))


def _reaches_call(fn, helpers):
    src = _source(fn)
    return "_call(" in src or any(re.search(r"\b%s\(" % h, src) for h in helpers)


def test_the_table_holds_every_op_that_reaches_the_library():
    """one level of private helper is followed.  A public op that reaches the library only through another public op need not be in the
    table: the inner op refuses its host operands."""
    own = {n: f for n, f in vars(ops).items() if inspect.isfunction(f) and inspect.unwrap(f).__module__ == ops.__name__}
    helpers = {n for n, f in own.items() if n.startswith("_") and n not in ("_call", "_size", "_timed") and "_call(" in _source(f)}
    reaching = {n for n, f in own.items() if not n.startswith("_") and _reaches_call(f, helpers)}
    assert len(reaching) >= 80, sorted(reaching)
    missing = reaching - set(HOST) - set(EXEMPT)
    assert not missing, "ops that reach _call without a line in the refusal table: %s" % sorted(missing)


def test_one_wording():
    """the refusal is raised in ONE place of ops.py and names the op and the operand"""
    assert inspect.getsource(ops).count('RuntimeError("' + REFUSAL) == 1          # the module docstring quotes the reference's wording as well
    with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \(fill_rows: rows must be a CUDA/HIP tensor\)"):
        ops._on_device("fill_rows", "dst rows src_row", None, f32(1), f32(1))


# ---- one operand on the host, the rest on the device: per op one case per operand class it treats differently (rows, plane pairs, index /
# mask tensors, workspaces, optional outputs).  `d(name, tensor)` leaves the named operand on the host and moves every other one to the device
# (a module stands for its weights: ops that take one refuse its first weight).
MSDA_NAMES = ("value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight")
RAW_NAMES = ("value", "spatial_shapes", "level_start_index", "ref", "offsets", "logits")


def named(d, names, tensors):
    return [d(n, t) for n, t in zip(names, tensors)]


def pair(d, name, plane):
    return d(name + "_hi", plane), d(name + "_lo", plane.clone())


def _mixed():
    a32, bias, res = f32(32, 32), f32(64), f32(32, 64)
    rows = i32(32)
    dy = f32(32, 32)
    lg, bx, tb = f32(1, 2, 3), f32(1, 2, 4), f32(1, 2, 4)
    qk, v32 = f32(1, 2, 64), f32(1, 2, 32)
    hw = f16(64, 64)
    return {
        "gemm": (("a", "w", "bias", "resid", "out", "out_row"), lambda d: ops.gemm(
            d("a", a32), d("w", hw), d("bias", bias), d("resid", res), split=True, out=d("out", f32(32, 64)), out_row=d("out_row", rows))),
        "gemm gather": (("a_row",), lambda d: ops.gemm(d("a", a32), d("w", hw), split=True, a_row=d("a_row", rows))),
        "gemm_scaled": (("alpha_dev",), lambda d: ops.gemm_scaled(d("a", a32), d("w", hw), d("alpha_dev", f32(1)), split=True)),
        "gemm_split_k_scaled": (("w_hl8", "alpha_dev"), lambda d: ops.gemm_split_k_scaled(d("a_hl8", hw), d("w_hl8", hw), 1, d("alpha_dev", f32(1)))),
        "gemm_split_k": (("w_hl8",), lambda d: ops.gemm_split_k(d("a_hl8", hw), d("w_hl8", hw), 1)),
        "fill_rows": (("rows", "src_row"), lambda d: ops.fill_rows(d("dst", f32(4, 4)), d("rows", i32(2)), d("src_row", f32(4)))),
        "act_backward": (("g", "out"), lambda d: ops.act_backward(d("u", dy), d("g", dy.clone()), ops.ACT_RELU, out=d("out", f32(32, 32)))),
        "layernorm_backward": (("gy", "weight", "gres"), lambda d: ops.layernorm_backward(d("s", dy), d("gy", dy), d("weight", f32(32)), 1e-5, gres=d("gres", dy))),
        "grad_pack": (("scale",), lambda d: ops.grad_pack(d("dy", dy), d("scale", f32(2)))),
        "add_layernorm": (("weight", "delta", "delta_row", "out_src"), lambda d: ops.add_layernorm(
            d("x", dy), d("delta", dy), d("weight", f32(32)), d("bias", f32(32)), 1e-5, torch.float32, delta_row=d("delta_row", rows), out_src=d("out_src", rows))),
        "flash_attn": (("k", "bias_h", "key_mask"), lambda d: ops.flash_attn(
            d("q", QH), d("k", QH), d("v", QH), 1.0, d("bias_h", f32(1, 1, 1)), d("bias_w", f32(1, 1, 1)), d("key_mask", u8(1, 1)))),
        "msda_fused": (("spatial_shapes", "ref", "logits"), lambda d: ops.msda_fused(*[d(n, t) for n, t in zip(
            ("value", "spatial_shapes", "level_start_index", "ref", "offsets", "logits"), RAW)])),
        "query_attn_train_backward": (("v", "blocked", "out", "lse", "d_out"), lambda d: ops.query_attn_train_backward(
            d("qk", qk), d("v", v32), d("blocked", u8(2, 2)), d("out", v32), d("lse", f32(1, 1, 2)), d("d_out", v32), 1, 1.0)),
        "bi_attn_train_backward": (("att", "out_l", "stat_v", "d_out_v"), lambda d: ops.bi_attn_train_backward(
            d("q", E256), d("k", E256), d("vv", E256), d("vl", E256), d("att", u8(1, 1)), d("out_v", E256), d("out_l", E256),
            d("stat_v", f32(1, 1, 1, 2)), d("stat_l", f32(1, 1, 1, 2)), d("d_out_v", E256), d("d_out_l", E256), 1)),
        "group_norm_backward": (("dy", "stat", "weight"), lambda d: ops.group_norm_backward(
            d("x", X4), d("dy", X4), d("stat", f32(1, 1, 2)), 1, d("weight", W8), d("bias", W8))),
        "attn_pack_grad": (("out", "v_lo", "scale"), lambda d: ops.attn_pack_grad(
            d("go", f32(1, 1, 80)), d("out", f32(1, 1, 80)), (d("v_hi", f16(1, 1, 80)), d("v_lo", f16(1, 1, 80))), d("scale", f32(1)), 1, 1, 1)),
        "attn_unpack_grad": (("dq_h", "inv"), lambda d: ops.attn_unpack_grad(
            d("dq", f32(1, 1, 128)), d("dk", f32(1, 1, 80)), d("dv", f32(1, 1, 80)), d("dq_h", f32(1, 1, 1, 80)), None, d("inv", f32(1)), 1, 1, 1)),
        "conv3x3_grid": (("w_hl8", "bias"), lambda d: ops.conv3x3_grid(d("buf", GRID), d("w_hl8", f16(8, 18)), d("bias", W8), 1, 1, 1)),
        "conv3x3_wgrad": (("dybuf", "y_rows"), lambda d: ops.conv3x3_wgrad(d("xbuf", GRID), d("dybuf", GRID), d("y_rows", f32(9, 1)), 1, 1, 1)),
        "hungarian_cost": (("boxes", "n_tgt", "pos_map", "is_thing", "out", "ws"), lambda d: ops.hungarian_cost(
            d("logits", lg), d("boxes", bx), d("tgt_boxes", tb), d("n_tgt", N1), d("t_off", N1), 2, (1.0,) * 5, pos_map=d("pos_map", u8(1, 2, 3)),
            is_thing=d("is_thing", u8(1, 2)), out=d("out", f32(5)), ws=d("ws", u8(1 << 16)))),
        "mask_match_cost": (("coords", "ws", "dice_out"), lambda d: ops.mask_match_cost(
            d("pred", f32(1, 2, 2)), d("tgt", f32(1, 2, 2)), d("coords", f32(1, 2)), ws=d("ws", u8(1 << 16)), ce_out=d("ce_out", f32(1, 1)), dice_out=d("dice_out", f32(1, 1)))),
        "uncertain_points": (("rest", "ws"), lambda d: ops.uncertain_points(d("src", f32(1, 2, 2)), d("cand", f32(1, 2, 2)), d("rest", f32(1, 1, 2)), 1, ws=d("ws", u8(1 << 16)))),
        "ota_cost": (("pos_map", "n_tgt", "res"), lambda d: ops.ota_cost(
            d("logits", lg), d("boxes", bx), d("tgt_boxes", tb), d("pos_map", u8(1, 2, 3)), d("n_tgt", N1), res=d("res", i32(3, 1)))),
        "pair_box_loss_forward": (("iou", "pair_t", "is_thing"), lambda d: ops.pair_box_loss_forward(
            d("boxes", bx), d("iou", f32(1, 2)), [(d("pair_q", i64(1)), d("pair_t", i64(1)))], d("tgt_boxes", tb), d("is_thing", u8(1, 2)), 1.0, 0)),
        "pair_box_loss_backward": (("pair_grad", "g_giou"), lambda d: ops.pair_box_loss_backward(
            [(d("pair_q", i64(1)), d("pair_t", i64(1)))], d("out", f32(8)), d("pair_grad", f32(1, 9)), d("g_bbox", f32(1)), d("g_giou", f32(1)), None, 1, 2, False)),
        "optim_adamw_step": (("cmap", "steps", "norm"), lambda d: ops.optim_adamw_step(
            d("table", i64(1, 6)), d("cmap", i64(1, 2)), d("steps", i32(1)), d("bc", f32(1, 2)), [1e-3], [0.0], (0.9, 0.999), 1e-8, norm=d("norm", f32(())))),
        "token_focal_forward": (("onehot", "keep"), lambda d: ops.token_focal_forward(d("logits", f32(1, 1, 2)), d("onehot", f32(1, 1, 2)), d("keep", u8(1, 2)))),
        "point_mask_loss_forward": (("tgt_index", "pts"), lambda d: ops.point_mask_loss_forward(
            d("src", f32(1, 2, 2)), d("tgt", f32(1, 2, 2)), d("tgt_index", i64(1)), d("pts", f32(1, 1, 2)), 0)),
        "gemm_f8x": (("wsc", "bias", "out_row"), lambda d: ops.gemm_f8x(
            d("a", HL), d("w8", u8(8, 128)), d("wsc", u8(8, 1, 2)), d("bias", W8), out_row=d("out_row", N1), out_rows=1)),
        "gemm_f8x resid": (("resid", "out"), lambda d: ops.gemm_f8x(
            d("a", HL), d("w8", u8(8, 128)), d("wsc", u8(8, 1, 2)), resid=d("resid", f32(1, 8)), out=d("out", f32(1, 8)))),
        "ms_deform_attn_forward": (("spatial_shapes", "sampling_loc"), lambda d: ops.ms_deform_attn_forward(*named(d, MSDA_NAMES, MSDA))),
        "ms_deform_attn_backward": (("level_start_index", "grad_output"), lambda d: ops.ms_deform_attn_backward(
            *named(d, MSDA_NAMES, MSDA), d("grad_output", f32(1, 1, 32)))),
        "msda_raw_backward": (("level_start_index", "ref", "grad_output"), lambda d: ops.msda_raw_backward(
            *named(d, RAW_NAMES, RAW), d("grad_output", f32(1, 1, 32)))),
        "flash_attn k_hl8": (("k",), lambda d: ops.flash_attn(d("q", QH), d("k", f16(1, 1, 64)), d("v", QH), 1.0, k_hl8=True)),
        "bi_i2t_split": (("k", "vl", "text_mask"), lambda d: ops.bi_i2t_split(
            d("q_hl8", f16(1, 1, 64)), d("k", f32(1, 1, 32)), d("vl", f32(1, 1, 32)), d("text_mask", u8(1, 1)), 1)),
        "bi_i2t_folded": (("M", "text_mask", "wo", "bo", "resid"), lambda d: ops.bi_i2t_folded(
            d("v_hl8", f16(1, 1, 16)), d("M", f32(1, 1, 1, 8)), d("cb", f32(1, 1, 1)), d("vl", f32(1, 1, 32)), d("text_mask", u8(1, 1)), 1,
            d("wo", f32(8, 32)), d("bo", f32(8)), d("resid", f32(1, 1, 8)))),
        "attn_f32": (("k", "mask"), lambda d: ops.attn_f32(d("q", Q4), d("k", Q4), d("v", Q4), 1.0, d("mask", u8(1, 1)))),
        "attn_split": (("mask",), lambda d: ops.attn_split(d("q", Q4), d("k", Q4), d("v", Q4), 1.0, d("mask", u8(1, 1)))),
        "attn_f32_rows": (("mask",), lambda d: ops.attn_f32_rows(d("q", Q4), d("k", Q4), d("v", Q4), 1.0, d("mask", u8(1, 1, 1)))),
        "vit_attn": (("rel_w",), lambda d: ops.vit_attn(d("qkv", QKV), d("rel_h", f32(1, 1, 1)), d("rel_w", f32(1, 1, 1)), (1, 1), 1, 1.0)),
        "vit_attn_fused": (("tab_w",), lambda d: ops.vit_attn_fused(d("qkv", QKV), d("tab_h", TAB), d("tab_w", TAB), (1, 1), 1, 1.0)),
        "vit_attn_rel": (("tab_h",), lambda d: ops.vit_attn_rel(d("qkv", QKV), d("tab_h", TAB), d("tab_w", TAB), (1, 1), 1)),
        "vit_attn_split": (("tab_w",), lambda d: ops.vit_attn_split(d("qkv", f16(1, 1, 384)), d("tab_h", f16(1, 128)), d("tab_w", f16(1, 128)), (1, 1), 1)),
        "vit_relpos": (("tab_w",), lambda d: ops.vit_relpos(d("qkv", QKV), d("tab_h", TAB), d("tab_w", TAB), (1, 1), 1)),
        "bi_xattn": (("k", "text_mask"), lambda d: ops.bi_xattn(d("q", QH), d("k", QH), d("vv", QH), d("vl", QH), d("text_mask", u8(1, 1)))),
        "mask_einsum": (("mask_features", "row_bias"), lambda d: ops.mask_einsum(d("mask_embed", ROW8[None]), d("mask_features", X4), row_bias=d("row_bias", f32(1, 1)))),
        "mask_einsum_backward": (("mask_features", "grad_out"), lambda d: ops.mask_einsum_backward(
            d("mask_embed", ROW8[None]), d("mask_features", X4), d("grad_out", f32(1, 1, 1, 1)))),
        "mask_einsum16": (("mask_features", "row_bias"), lambda d: ops.mask_einsum16(
            d("mask_embed", ROW8[None]), d("mask_features", X4.half()), row_bias=d("row_bias", f32(1, 1)))),
        "dynamic_mask": (("ref_points", "params"), lambda d: ops.dynamic_mask(d("mask_feats", X4), d("ref_points", f32(1, 2)), d("params", f32(1, 169)), 1)),
        "dynamic_mask_backward": (("params", "grad_out"), lambda d: ops.dynamic_mask_backward(
            d("mask_feats", X4), d("ref_points", f32(1, 2)), d("params", f32(1, 169)), d("grad_out", f32(1, 2, 2)), 1)),
        "add_layernorm_sum": (("delta", "addend"), lambda d: ops.add_layernorm_sum(
            d("x", ROW8), d("delta", ROW8), d("weight", W8), d("bias", W8), 1e-5, d("addend", ROW8))),
        "add_layernorm_dec": (("bias", "delta"), lambda d: ops.add_layernorm_dec(d("x", ROW8), d("delta", ROW8), d("weight", W8), d("bias", W8), 1e-5, torch.float16)),
        "matmul_nt_batched": (("w",), lambda d: ops.matmul_nt_batched(d("a", f32(1, 1, 32)), d("w", f32(1, 8, 32)))),
        "group_norm": (("prebias", "weight"), lambda d: ops.group_norm(d("x", X4), 1, d("weight", W8), d("bias", W8), 1e-5, prebias=d("prebias", W8))),
        "batched_nms": (("scores", "classes"), lambda d: ops.batched_nms(d("boxes", f32(1, 1, 4)), d("scores", f32(1, 1)), d("classes", i64(1, 1)), 0.5)),
        "mask_finalize": (("qidx",), lambda d: ops.mask_finalize(d("masks", f32(1, 1, 1)), d("qidx", i32(1)), 1, (1, 1), (1, 1), 0.5)),
        "sem_pan": (("cls_all", "pscore"), lambda d: ops.sem_pan(d("masks_lo", f32(1, 1, 1)), d("cls_all", f32(1, 1)), d("pscore", f32(1)), 1, (1, 1), (1, 1))),
        "ref_point_mlp": (("weight",), lambda d: ops.ref_point_mlp(d("ref", f32(1, 1, 4)), d("weight", mlp(2)))),
        "box_head": (("ref", "weight"), lambda d: ops.box_head(d("x", f32(1, 256)), d("ref", f32(1, 4)), d("weight", mlp(3)))),
        "selftest": (("b",), lambda d: ops.selftest(0, d("a", f32(4)), d("b", f32(4)))),
        "f16_pair": (("scale",), lambda d: ops.f16_pair(d("x", ROW8), scale=d("scale", f32(1)))),
        "conv3x3_split": (("weight",), lambda d: ops.conv3x3_split(d("x", f32(1, 1, 1, 1)), d("weight", torch.nn.Conv2d(1, 1, 3, padding=1)))),
        "ffn_fused": (("weight1", "weight2"), lambda d: ops.ffn_fused(
            d("x_hl8", f16(1, 512)), d("weight1", torch.nn.Linear(2, 2)), d("weight2", torch.nn.Linear(2, 2)))),
        "split_linear_ln": (("weight", "resid", "norm_weight", "norm_bias"), lambda d: ops.split_linear_ln(
            d("x", f32(1, 32)), torch.nn.Module(), "w", d("weight", f32(256, 32)), None, d("resid", f32(1, 256)), d("norm_weight", f32(256)),
            d("norm_bias", f32(256)), 1e-5)),
        "attn_pack_q": (("rel_h", "rel_w"), lambda d: ops.attn_pack_q(d("rq", f32(1, 1, 80)), d("rel_h", f32(1, 1, 1, 1)), d("rel_w", f32(1, 1, 1, 1)), 1, 1, 1, 128)),
        "attn_train_forward": (("k_lo", "v_hi"), lambda d: ops.attn_train_forward(
            pair(d, "q", f16(1, 128, 224)), pair(d, "k", f16(1, 128, 224)), pair(d, "v", f16(1, 128, 80)))),
        "attn_train_win_backward": (("do96_hi", "delta"), lambda d: ops.attn_train_win_backward(
            pair(d, "q", f16(1, 1, 128)), pair(d, "k", f16(1, 1, 128)), pair(d, "v96", f16(1, 1, 96)), pair(d, "do96", f16(1, 1, 96)),
            d("lse", f32(1, 1)), d("delta", f32(1, 1)))),
        "ota_assign": (("iou", "n_tgt"), lambda d: ops.ota_assign(d("cost", f32(1, 1, 1)), d("iou", f32(1, 1, 1)), d("n_tgt", N1))),
        "hungarian_assign": (("n_tgt", "t_off"), lambda d: ops.hungarian_assign(d("costs", f32(2)), d("n_tgt", N1), d("t_off", N1), 1, 1, 1)),
        "positive_onehot": (("pair_t", "pos_map"), lambda d: ops.positive_onehot(
            [(d("pair_q", i64(1)), d("pair_t", i64(1)))], d("pos_map", u8(1, 1, 1)), 1)),
    }


MIXED = _mixed()


@pytest.mark.gpu
@pytest.mark.parametrize("op,operand", [(op, operand) for op in sorted(MIXED) for operand in MIXED[op][0]])
def test_one_host_operand_is_refused_before_the_library(monkeypatch, op, operand):
    monkeypatch.setattr(ops, "_call", lambda name, *a: pytest.fail("%s reached the library with %s on the host" % (name, operand)))
    with pytest.raises(RuntimeError, match=r"%s \(.*\b%s must be" % (REFUSAL, operand)):
        MIXED[op][1](lambda name, t: t if name == operand else t.cuda())
