"""Seeded inputs and the yardsticks of the point-selection and mask-cost tests (csrc/point_select.hip): test_point_select_cpu.py,
test_gpu_point_select.py.

Reference: the formulas of hipie_amd/training/criterion.py (`uncertain_points`) and matcher.py (`mask_costs`) over matcher.point_sample,
evaluated on the CPU in float64 on the same fp32 inputs; e_lib: the same code in float32.  Costs: max|got - ref64| / max|ref64| per
output tensor against max(1e-6, 4 x e_lib) (_loss_cases.err / bound_of).  Selection: the chosen SET against the float64 selection -- a
candidate may differ only when its float64 |logit| lies within max(1e-6 max|src|, 4 x e_lib) of the float64 threshold (e_lib = the largest
|float32 sample - float64 sample| of the case), and at most 0.1 % of k may differ (`check_selection`)."""
import functools

import torch
import torch.nn.functional as F

from _loss_cases import TorchLossOps, _special_points, bound_of, err          # noqa: F401  (re-exported to the two test files)
from hipie_amd.training.matcher import point_sample


# ------------------------------------------------------------------------------------------------ the selection rule, restated
def select_rule(values, k):
    """values (C,) sampled logits of one instance -> the indices of the k candidates with the smallest |value| in ascending order: ties at
    the threshold by ascending index (a STABLE sort), -0.0 ties with +0.0 (abs), a NaN counts as the largest score (it sorts in front)"""
    a = values.abs()
    a = torch.where(torch.isnan(a), torch.full_like(a, -1.0), a)
    return a.sort(stable=True).indices[:k].sort().values


def select_points(values, cand, rest, k):
    """values (N, C), cand (N, C, 2), rest (N, P - k, 2) | None -> pts (N, P, 2) by the rule of hipie_uncertain_points"""
    idx = torch.stack([select_rule(v, k) for v in values]) if len(values) else torch.zeros(0, k, dtype=torch.int64)
    pts = torch.gather(cand, 1, idx[:, :, None].expand(-1, -1, 2))
    return pts if rest is None else torch.cat((pts, rest), 1)


def sampled(src, cand, dtype):
    """(N, C) bilinear samples of src (N, H, W) at cand, computed in `dtype` on the CPU by matcher.point_sample"""
    return point_sample(src[:, None].cpu().to(dtype), cand.cpu().to(dtype))[:, 0]


def mask_costs_in(pred, tgt, coords):
    """matcher.mask_costs in the dtype of its inputs (the matcher's own casts everything to float32): (ce (Q,T), dice (Q,T))"""
    P = coords.shape[0]
    x = point_sample(pred[:, None], coords[None].expand(pred.shape[0], P, 2))[:, 0]
    t = point_sample(tgt[:, None], coords[None].expand(tgt.shape[0], P, 2))[:, 0]
    ce = (F.softplus(-x) @ t.t() + F.softplus(x) @ (1 - t).t()) / P
    s = x.sigmoid()
    return ce, 1 - (2 * (s @ t.t()) + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)


class TorchCriteriaOps(TorchLossOps):
    """the `ops` object of the criteria AND the matchers in plain torch, in the dtype of its inputs"""

    @staticmethod
    def uncertain_points(src, cand, rest, k, num_points=None):
        assert num_points is None or num_points == k + (0 if rest is None else rest.shape[1])
        return select_points(point_sample(src[:, None], cand)[:, 0], cand, rest, k)

    @staticmethod
    def mask_match_costs(pred, tgt, coords):
        return mask_costs_in(pred, tgt, coords)


# ------------------------------------------------------------------------------------------------ selection cases
def counts(P, oversample, importance):
    """(C, k) as criterion.uncertain_points derives them"""
    return int(P * oversample), int(importance * P)


# (N, H, W, P): C = 3 P, k = 0.75 P -- one point, an odd map, C = 1200 (no multiple of 256 or 1024), the production C and k (several chunks)
SELECT_SHAPES = [(1, 1, 1, 4), (3, 5, 7, 12), (2, 64, 64, 400), (1, 64, 64, 12544)]
SELECT_SEEDS = (0, 1)


@functools.lru_cache(maxsize=None)
def select_case(N, H, W, P, seed=0, oversample=3.0, importance=0.75):
    """fp32 CPU (src (N,H,W) = randn * 3, cand (N,C,2) with the special points first (at most half of C), rest (N,P-k,2) | None, k)"""
    C, k = counts(P, oversample, importance)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 31 * H + 17 * W + P)
    src = torch.randn(N, H, W, generator=g) * 3.0
    cand = torch.rand(N, C, 2, generator=g)
    sp = torch.tensor(_special_points(H, W), dtype=torch.float32)[:C // 2]
    cand[:, :len(sp)] = sp
    rest = torch.rand(N, P - k, 2, generator=g) if P - k > 0 else None
    return src, cand, rest, k


@functools.lru_cache(maxsize=None)
def select_yardsticks(N, H, W, P, seed=0):
    """(v64 (N,C) float64 samples, e_lib) of select_case, computed once and shared; treat as read-only"""
    src, cand, _, _ = select_case(N, H, W, P, seed)
    v64 = sampled(src, cand, torch.float64)
    return v64, float((sampled(src, cand, torch.float32).double() - v64).abs().max())


def chosen_indices(pts_k, cand):
    """pts_k (k, 2): rows of cand (C, 2) in ascending candidate index -> those indices (k,), by the bits of (x, y): one scan over cand, a row
    is matched with the first candidate behind the previous match (of two candidates at one place the rule takes the first)"""
    def bits(t):
        b = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return ((b[:, 0] << 32) | b[:, 1]).tolist()
    have, out, j = bits(cand), [], 0
    for want in bits(pts_k):
        while j < len(have) and have[j] != want:
            j += 1
        assert j < len(have), "a selected point is no candidate behind the one before it: not in ascending candidate index"
        out.append(j)
        j += 1
    return torch.tensor(out, dtype=torch.int64)


def check_selection(tag, pts, case, v64, e_lib):
    """pts (N, P, 2) on the CPU against the float64 selection of `case`: rest copied bit for bit, the chosen candidates distinct and in
    ascending candidate index, their set within the band and the cap of the module docstring.  Prints its figures (lines starting with
    SELECT) before it asserts; returns the number of candidates that differ."""
    src, cand, rest, k = case
    N, P = src.shape[0], k + (0 if rest is None else rest.shape[1])
    assert pts.shape == (N, P, 2) and pts.dtype == torch.float32
    if rest is not None:
        assert torch.equal(pts[:, k:], rest), tag
    band = max(1e-6 * float(src.abs().max()), 4 * e_lib)
    differ, most, worst = 0, 0, 0.0
    for n in range(N):
        got = chosen_indices(pts[n, :k], cand[n])
        assert bool((got[1:] > got[:-1]).all()), (tag, n, "not in ascending candidate index")
        want = select_rule(v64[n], k)
        a = v64[n].abs()
        tau = float(a[want].max()) if k else 0.0
        off = torch.tensor(sorted(set(got.tolist()) ^ set(want.tolist())), dtype=torch.int64)
        differ += len(off) // 2
        most = max(most, len(off) // 2)
        if len(off):
            worst = max(worst, float((a[off] - tau).abs().max()))
    print("SELECT %-40s k %5d  differ %d, at most %d per instance (cap %.2f)  farthest from the threshold %.3e  band %.3e  e_lib %.3e"
          % (tag, k, differ, most, 1e-3 * k, worst, band, e_lib))
    assert worst <= band, (tag, worst, band)
    assert most <= 1e-3 * k, (tag, most, k)
    return differ


# ------------------------------------------------------------------------------------------------ the exact selection case
@functools.lru_cache(maxsize=None)
def exact_case(N, H, W, C, k, n_rest, seed=0):
    """maps of small integers (instance 0 all zero, a -0.0 among them when there is room), candidates at pixel centres of a map whose sides
    are powers of two (the coordinate (i + 0.5) / size and the sample are exact in fp32), many duplicates: (src, cand, rest | None, k, values
    (N, C) = the map value under every candidate)"""
    assert H & (H - 1) == 0 and W & (W - 1) == 0
    g = torch.Generator().manual_seed(77 + 1000003 * seed + 31 * H + W + C)
    src = torch.randint(-3, 4, (N, H, W), generator=g).float()
    src[0] = 0.0
    if H * W > 1:
        src[:, 0, 1] = -0.0
    xi, yi = torch.randint(0, W, (N, C), generator=g), torch.randint(0, H, (N, C), generator=g)
    cand = torch.stack(((xi.float() + 0.5) / W, (yi.float() + 0.5) / H), -1)
    values = torch.stack([src[n, yi[n], xi[n]] for n in range(N)])
    rest = torch.rand(N, n_rest, 2, generator=g) if n_rest else None
    return src, cand, rest, k, values


# ------------------------------------------------------------------------------------------------ mask-cost cases
@functools.lru_cache(maxsize=None)
def cost_case(Q, T, H, W, P, big_targets, seed=0):
    """fp32 CPU (pred (Q,H,W) = randn * 3, tgt (T,Ht,Wt), coords (P,2) with the special points first (at most half of P)); big_targets: hard
    {0, 1} targets at 4x the predictions' size, else soft values in [0, 1] (a good share of exact 0 and 1) at the predictions' size"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * Q + 613 * T + 31 * H + 17 * W + P + (5 if big_targets else 0))
    pred = torch.randn(Q, H, W, generator=g) * 3.0
    if big_targets:
        tgt = (torch.rand(T, 4 * H, 4 * W, generator=g) < 0.4).float()
    else:
        tgt = (torch.rand(T, H, W, generator=g) * 1.5 - 0.25).clamp(0, 1)
    coords = torch.rand(P, 2, generator=g)
    sp = torch.tensor(_special_points(H, W), dtype=torch.float32)[:P // 2]
    coords[:len(sp)] = sp
    return pred, tgt, coords


@functools.lru_cache(maxsize=None)
def cost_yardsticks(Q, T, H, W, P, big_targets, seed=0):
    """((ce64, dice64), (ce32, dice32)) of the matcher's formulas on cost_case, computed once and shared; treat as read-only"""
    c = cost_case(Q, T, H, W, P, big_targets, seed)
    return mask_costs_in(*(t.double() for t in c)), mask_costs_in(*c)


def assignment_total(C_from, C_price):
    """the scipy assignment computed from C_from, priced with C_price (both (Q, T) on the CPU)"""
    from scipy.optimize import linear_sum_assignment
    i, j = linear_sum_assignment(C_from.double().numpy())
    return float(C_price.double().numpy()[i, j].sum())


def second_best_gap(C):
    """(best total, relative distance of the second-best assignment's total) of a (Q, T) float64 cost matrix: every pair of the optimum is
    forbidden in turn and the rest solved again; the cheapest of those is the second best"""
    from scipy.optimize import linear_sum_assignment
    C = C.double().numpy()
    i, j = linear_sum_assignment(C)
    best, second = float(C[i, j].sum()), float("inf")
    for a, b in zip(i, j):
        D = C.copy()
        D[a, b] = 1e30
        ii, jj = linear_sum_assignment(D)
        second = min(second, float(D[ii, jj].sum()))
    return best, (second - best) / max(abs(best), 1e-300)


def check_costs(tag, got, ref64, lib32):
    fails = []
    for n, g, r, l in zip(("ce", "dice"), got, ref64, lib32):
        e, e_lib, bound = err(g, r), err(l, r), bound_of(l, r)
        print("COST %-44s %-5s err %.3e  e_lib %.3e  bound %.3e" % (tag, n, e, e_lib, bound))
        if not e <= bound:
            fails.append((n, e, e_lib, bound))
    assert not fails, (tag, fails)
