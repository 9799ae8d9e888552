"""Inputs and the float64 yardstick shared by test_msda_raw_cpu.py and test_gpu_msda_raw.py: deformable-attention sampling from the RAW
projections (ref, offsets, logits), as hipie_msda_fused_forward / hipie_msda_raw_backward take them.

Inputs are built as test_gpu_kernels.test_msda_backward_gather_form_... builds its locations: target pixel positions 0.05 px away from
every pixel boundary, from 1.5 px outside the map on one side to 1.5 px outside on the other (grad_sampling_loc jumps at a boundary, and an
fp32 rounding of the location would pick the other side); then a reference point is drawn and the offsets are SOLVED for, in float64, and
rounded to fp32 -- the yardstick reads the rounded values, so both sides see the same inputs."""
import torch

from oracle import ops as oo

ENC3 = [(24, 32), (12, 16), (6, 8)]
FOUR = [(40, 40), (20, 20), (10, 10), (5, 5)]

#          ref_dim, levels, B, Lq, M, P
CASES = {
    "enc3": (2, ENC3, 2, 1203, 8, 4),
    "dec3_few37": (4, ENC3, 2, 37, 8, 4),
    "dec3_few7": (4, ENC3, 2, 7, 8, 4),
    "dec4": (4, FOUR, 2, 301, 8, 4),
    "sharp": (2, FOUR, 2, 801, 8, 4),
    "flat": (2, ENC3, 2, 1203, 8, 4),
    "heads5": (2, ENC3, 2, 603, 5, 4),
    "heads16_batch3": (2, ENC3, 3, 517, 16, 2),
    "all_outside": (2, ENC3, 2, 1203, 8, 4),
    "one_pixel_hot": (2, ENC3, 2, 1203, 8, 4),
    "gapped": (2, ENC3, 2, 1203, 8, 4),
}
D = 32
GAP = 5                                              # unused rows between the levels of "gapped"


def lsi(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def build(case, seed=3):
    """dict of float64 tensors holding fp32-representable values: value (B,S,M,D), ref (B,Lq,L,ref_dim), offsets (B,Lq,M,L,P,2), logits
    (B,Lq,M,L*P), gout (B,Lq,M*D); sh / ls (L,2) / (L,) int64; rows: the pixel rows of value the levels cover; pix: the target positions"""
    ref_dim, shapes, B, Lq, M, P = CASES[case]
    L = len(shapes)
    sh = torch.as_tensor(shapes, dtype=torch.long)
    ls = lsi(sh)
    S = int(sh.prod(1).sum())
    if case == "gapped":
        ls = ls + torch.arange(L) * GAP
        S += GAP * L
    rows = torch.cat([torch.arange(int(ls[l]), int(ls[l]) + shapes[l][0] * shapes[l][1]) for l in range(L)])
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    value = torch.randn(B, S, M, D, generator=g, dtype=f64)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=f64)[None, None, None, :, None, :]
    raw = torch.rand(B, Lq, M, L, P, 2, generator=g, dtype=f64) * (wh + 3) - 2.0
    if case == "all_outside":
        raw = raw + 2 * wh
    if case == "one_pixel_hot":
        raw = torch.floor(wh / 2) + torch.rand(raw.shape, generator=g, dtype=f64)
    pix = torch.floor(raw) + 0.05 + 0.9 * (raw - torch.floor(raw))
    loc = (pix + 0.5) / wh
    ref = torch.rand(B, Lq, L, ref_dim, generator=g, dtype=f64)
    if ref_dim == 4:
        ref[..., 2:] = 0.05 + 0.6 * ref[..., 2:]                                  # ref_wh in [0.05, 0.65]
    ref = ref.float().double()
    rxy = ref[:, :, None, :, None, :2]
    if ref_dim == 2:
        offsets = (loc - rxy) * wh
    else:
        offsets = (loc - rxy) * P / (ref[:, :, None, :, None, 2:] * 0.5)
    logits = torch.randn(B, Lq, M, L * P, generator=g, dtype=f64)
    if case == "sharp":
        logits = logits * 8
    if case == "flat":
        logits = torch.full_like(logits, 0.75)
    gout = torch.randn(B, Lq, M * D, generator=g, dtype=f64)
    r32 = lambda t: t.float().double()
    return dict(case=case, ref_dim=ref_dim, shapes=shapes, B=B, Lq=Lq, M=M, P=P, L=L, S=S, sh=sh, ls=ls, rows=rows, pix=pix,
                value=r32(value), ref=ref, offsets=r32(offsets), logits=r32(logits), gout=r32(gout))


def locations(c, ref, offsets):
    """the module's location arithmetic (ops/modules/ms_deform_attn.py:99-110) in the dtype of its arguments"""
    wh = torch.tensor([[w, h] for h, w in c["shapes"]], dtype=ref.dtype)[None, None, None, :, None, :]
    if c["ref_dim"] == 2:
        return ref[:, :, None, :, None, :] + offsets / wh
    return ref[:, :, None, :, None, :2] + offsets / c["P"] * ref[:, :, None, :, None, 2:] * 0.5


def composition(c, value, ref, offsets, logits):
    """softmax of the logits, the locations, oracle.ops.ms_deform_attn_core on the rows the levels cover"""
    aw = torch.softmax(logits, -1).view(c["B"], c["Lq"], c["M"], c["L"], c["P"])
    return oo.ms_deform_attn_core(value[:, c["rows"]], c["sh"], locations(c, ref, offsets), aw)


def gradients(c, dtype=torch.float64):
    """(grad_value, grad_offsets, grad_logits, grad_ref) of the composition under the cotangent gout, by torch.autograd.grad in `dtype`"""
    with torch.enable_grad():
        leaves = [c[k].to(dtype).clone().requires_grad_(True) for k in ("value", "offsets", "logits", "ref")]
        out = composition(c, leaves[0], leaves[3], leaves[1], leaves[2])
        return torch.autograd.grad(out, leaves, c["gout"].to(dtype))


def boundary_distance(c, dtype=torch.float32):
    """smallest distance, in pixels, of a location computed in `dtype` from a pixel boundary (an integer of loc * size - 0.5)"""
    loc = locations(c, c["ref"].to(dtype), c["offsets"].to(dtype)).double()
    wh = torch.tensor([[w, h] for h, w in c["shapes"]], dtype=torch.float64)[None, None, None, :, None, :]
    im = loc * wh - 0.5
    return float((im - torch.round(im)).abs().min())
