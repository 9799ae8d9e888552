"""Seeded inputs and the yardsticks of the loss-kernel tests (csrc/point_loss.hip): test_point_loss_cpu.py, test_gpu_point_loss.py.

Reference: the formulas of hipie_amd/training/criterion.py (`_focal`, binary_cross_entropy_with_logits, the dice quotient) over
matcher.point_sample, evaluated on the CPU in float64 on the same fp32-representable inputs; e_lib: the same code in float32.
Metric: max|got - ref64| / max|ref64| per output tensor.  Bound per case: max(1e-6, 4 x e_lib) (the convention and the floor of
test_gpu_act_bwd.py / test_gpu_layernorm_bwd.py).  `check` prints every figure (lines starting with LOSS) before it asserts."""
import functools

import torch
import torch.nn.functional as F

from hipie_amd.training.criterion import _focal, token_focal_loss
from hipie_amd.training.matcher import point_sample


# ------------------------------------------------------------------------------------------------ the two formulations in plain torch
def torch_point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha):
    """(lmask (N,), ldice (N,), sums (N,3)) as criterion.loss_masks computes them (gathered targets, two point_sample calls), any dtype"""
    lab = point_sample(tgt_maps[tgt_index][:, None], pts)[:, 0]
    lg = point_sample(src[:, None], pts)[:, 0]
    term = _focal(lg, lab, alpha, 2.0) if mode == 1 else F.binary_cross_entropy_with_logits(lg, lab, reduction="none")
    s = lg.sigmoid()
    a, b, c = (s * lab).sum(-1), s.sum(-1), lab.sum(-1)
    return term.mean(1), 1 - (2 * a + 1) / (b + c + 1), torch.stack((a, b, c), 1)


class TorchLossOps:
    """the `ops` object of the criteria in plain torch, in the dtype of its inputs"""

    @staticmethod
    def point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha):
        return torch_point_mask_loss(src, tgt_maps, tgt_index, pts, mode, alpha)[:2]

    @staticmethod
    def token_focal_sum(logits, onehot, text_mask, alpha):
        return token_focal_loss(logits, onehot, text_mask, alpha)


# ------------------------------------------------------------------------------------------------ metric and bound
def err(got, ref):
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "not finite"
    if ref.numel() == 0:
        return 0.0
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def bound_of(lib, ref):
    return max(1e-6, 4 * err(lib, ref))


def check(tag, names, got, ref64, lib32):
    fails = []
    for n, g, r, l in zip(names, got, ref64, lib32):
        e, e_lib = err(g, r), err(l, r)
        bound = max(1e-6, 4 * e_lib)
        print("LOSS %-44s %-8s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)


# ------------------------------------------------------------------------------------------------ point-sampled mask loss
def _special_points(H, W):
    """(x, y): exactly 0 and 1, pixel centres, pixel boundaries, and a few outside [0, 1] whose corners fall off the map"""
    cx, cy = (min(W - 1, 2) + 0.5) / W, (min(H - 1, 1) + 0.5) / H
    bx, by = min(W, 3) / W, min(H, 2) / H
    return [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (cx, cy), (bx, by), (cx, by), (-0.02, 0.5), (0.5, 1.03), (1.0 + 0.4 / W, -0.4 / H), (-3.0, 0.5), (0.5, 7.0)]


@functools.lru_cache(maxsize=None)
def point_case(N, H, W, Ht, Wt, P, seed=0):
    """fp32 CPU tensors (src, tgt, tgt_index, pts, g_mask, g_dice): T = N + 1 target maps with soft values in [0, 1], the index descending
    with a repeat (and one map unused), the special points first (at most half of P), uniform points after them"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 31 * H + 17 * W + 13 * Ht + 11 * Wt + P)
    T = N + 1
    src = torch.randn(N, H, W, generator=g) * 3.0
    tgt = (torch.rand(T, Ht, Wt, generator=g) * 1.5 - 0.25).clamp(0, 1)                  # a good share of exact 0 and 1
    idx = torch.arange(T - 1, T - 1 - N, -1)
    if N > 1:
        idx[-1] = idx[0]
    pts = torch.rand(N, P, 2, generator=g)
    sp = torch.tensor(_special_points(H, W), dtype=torch.float32)[:P // 2]
    pts[:, :len(sp)] = sp
    return src, tgt, idx, pts, torch.randn(N, generator=g), torch.randn(N, generator=g)


def point_reference(src, tgt, idx, pts, g_mask, g_dice, mode, alpha, dtype):
    """(lmask, ldice, sums, d_src) in `dtype` on the CPU"""
    s = src.detach().cpu().to(dtype).requires_grad_(True)
    lmask, ldice, sums = torch_point_mask_loss(s, tgt.cpu().to(dtype), idx.cpu(), pts.cpu().to(dtype), mode, alpha)
    d, = torch.autograd.grad((lmask * g_mask.cpu().to(dtype)).sum() + (ldice * g_dice.cpu().to(dtype)).sum(), s)
    return lmask.detach(), ldice.detach(), sums.detach(), d


@functools.lru_cache(maxsize=None)
def point_yardsticks(N, H, W, Ht, Wt, P, mode, alpha, seed=0):
    """(ref64, lib32) of point_case, computed once and shared; treat as read-only"""
    c = point_case(N, H, W, Ht, Wt, P, seed)
    return point_reference(*c, mode, alpha, torch.float64), point_reference(*c, mode, alpha, torch.float32)


POINT_NAMES = ("lmask", "ldice", "sums", "d_src")


# ------------------------------------------------------------------------------------------------ token focal loss
@functools.lru_cache(maxsize=None)
def token_case(B, Q, T, keep, seed=0):
    """fp32 CPU (logits, onehot, text_mask | None); keep: "null" | "all" | "some" (tokens dropped in every image) | "image" (image 0 loses
    every token) | "none" (everything dropped)"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 31 * Q + T)
    logits = torch.randn(B, Q, T, generator=g) * 3.0
    onehot = (torch.rand(B, Q, T, generator=g) < 0.15).float()
    if keep == "null":
        return logits, onehot, None
    mask = torch.ones(B, T, dtype=torch.int64)
    if keep == "some":
        mask[:, T // 2:] = 0
        mask[-1, 0] = 0
    elif keep == "image":
        mask[0] = 0
    elif keep == "none":
        mask[:] = 0
    return logits, onehot, mask


def token_reference(logits, onehot, mask, alpha, dtype):
    """(loss 0-d, dlogits) of criterion.token_focal_loss in `dtype` on the CPU"""
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    loss = token_focal_loss(x, onehot.cpu().to(dtype), None if mask is None else mask.cpu(), alpha)
    d, = torch.autograd.grad(loss, x)
    return loss.detach(), d
