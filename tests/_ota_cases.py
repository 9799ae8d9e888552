"""Seeded inputs, the restated assignment rule and the yardsticks of the SimOTA matching tests (csrc/ota_match.hip): test_ota_match_cpu.py,
test_gpu_ota_match.py.

Costs.  Reference: matcher.ota_cost evaluated on the CPU in float64 on the same fp32 inputs (the sigmoid included); e_lib: the same code in
float32.  max|got - ref64| / max|ref64| per tensor against max(1e-6, 4 x e_lib) (_loss_cases.err / bound_of); the +100 / +10000 terms are
compared as masks, entry for entry, before any magnitude.
Assignment.  No tolerance: matcher.dynamic_k_assign on the CPU in fp32 on a copy of the kernel's own cost and iou.  `assign_rule` restates
it with loops and every tie at the lowest index -- torch.argmin / min / max document that rule, torch.topk documents none, so the cases
stay away from ties there (`preconditions`): in float64 every target's top-10 IoU sum lies at least 1e-4 from an integer, and in the fp32
torch cost the k_t + 1 cheapest entries of every column are pairwise distinct.  The repair case is excepted from the second: its ties are
the point."""
import functools
import os

import numpy as np
import torch

from _loss_cases import bound_of, err          # noqa: F401  (re-exported to the two test files)
from hipie_amd.training import matcher

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (B, Q, T, L, an extra image without targets): Q < 10 (the top-min(Q, 10) path); one target; nothing a multiple of anything, the second image
# with fewer targets than Tmax and a third without any; a bitmap row wider than one word; the production width
SHAPES = [(1, 4, 3, 8, False), (1, 40, 1, 16, False), (2, 70, 9, 33, True), (1, 300, 37, 64, False), (2, 900, 100, 256, False)]
SEEDS = (0, 1)
IDS = lambda s: "x".join(map(str, s[:4]))          # noqa: E731


def _image(g, Q, T, L):
    """one image of the generator: (logits (Q, L), boxes (Q, 4), target dict)"""
    u = lambda *s: torch.rand(*s, generator=g)          # noqa: E731
    tb = torch.cat((0.2 + 0.6 * u(T, 2), 0.05 + 0.3 * u(T, 2)), 1)
    qb = torch.cat((u(Q, 2), 0.02 + 0.4 * u(Q, 2)), 1)
    n = min(3 * T, Q)
    if n:
        qb[:n] = tb[torch.arange(n) % T] + 0.02 * torch.randn(n, 4, generator=g)
    qb[:, 2:] = qb[:, 2:].clamp(min=0.02)
    logits = 2.0 * torch.randn(Q, L, generator=g)
    pm = torch.zeros(T, L, dtype=torch.bool)
    for t in range(T):
        run = int(torch.randint(1, 4, (1,), generator=g))
        run = min(run, L)
        start = int(torch.randint(0, L - run + 1, (1,), generator=g))
        pm[t, start:start + run] = True
    return logits, qb, {"boxes": tb, "positive_map": pm, "labels": torch.zeros(T, dtype=torch.long)}


@functools.lru_cache(maxsize=None)
def ota_case(B, Q, T, L, empty, seed):
    """-> (logits (B', Q, L), boxes (B', Q, 4), targets): image 0 has T targets, the later ones two thirds of them (at least one); with
    `empty` a last image without targets is appended (B' = B + 1).  Cached: shared by the tests and never written to."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Q + T)
    counts = [T] + [max(1, (2 * T) // 3)] * (B - 1) + ([0] if empty else [])
    imgs = [_image(g, Q, n, L) for n in counts]
    return torch.stack([i[0] for i in imgs]), torch.stack([i[1] for i in imgs]), [i[2] for i in imgs]


@functools.lru_cache(maxsize=None)
def repair_case():
    """Q = 8, T = 6, the targets 1 and 2 copies of target 0 with its positive map: three identical columns, every claim of theirs is contested
    and two of the three are left empty -- the repair loop has to run"""
    g = torch.Generator().manual_seed(5)
    logits, qb, t = _image(g, 8, 6, 8)
    t["boxes"][1:3] = t["boxes"][0]
    t["positive_map"][1:3] = t["positive_map"][0]
    n = 8
    qb[:n] = t["boxes"][torch.arange(n) % 6] + 0.02 * torch.randn(n, 4, generator=g)
    qb[:, 2:] = qb[:, 2:].clamp(min=0.02)
    return logits[None], qb[None], [t]


def golden_cases(dev="cpu"):
    """the reference's own instances (tests/golden/train_matcher.npz): -> {"ota": (logits, boxes, targets, pairs, best), "tie": ...}; the
    third image of "ota" has no target, "tie" has two coinciding targets"""
    z = np.load(os.path.join(GOLD, "train_matcher.npz"))
    f = lambda k: torch.from_numpy(z[k]).to(dev)          # noqa: E731
    keys = ("labels", "boxes", "positive_map", "is_thing", "masks")
    targets = [{k: f("t%d_%s" % (i, k)) for k in keys if "t%d_%s" % (i, k) in z.files} for i in range(3)]
    empty = {k: v[:0] for k, v in targets[2].items()}
    pairs = lambda p, n: [(f("%s%d_q" % (p, i)).cpu(), f("%s%d_t" % (p, i)).cpu()) for i in range(n)]          # noqa: E731
    tie_t = [{"labels": torch.zeros(3, dtype=torch.long, device=dev), "boxes": f("tie_boxes"), "positive_map": targets[0]["positive_map"][:3]}]
    return {"ota": (f("logits"), f("ota_boxes"), targets[:2] + [empty], pairs("ota", 3), [f("ota_best%d" % i).cpu() for i in range(3)]),
            "tie": (f("tie_logits"), f("tie_queries"), tie_t, pairs("tie", 1), [f("tie_best").cpu()])}


def same_pairs(got, want):
    return len(got) == len(want) and all(torch.equal(g[0].cpu(), w[0].cpu()) and torch.equal(g[1].cpu(), w[1].cpu()) for g, w in zip(got, want))


def same_best(got, want):
    return len(got) == len(want) and all(torch.equal(torch.as_tensor(g).cpu().long(), torch.as_tensor(w).cpu().long()) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ the cost, its masks, the yardsticks
def centre_masks(boxes, target, center_radius=2.5, stride=32):
    """the two penalty masks of matcher.ota_cost in the dtype of its inputs: (not (inside & near) (Q, T), not candidate (Q,))"""
    tb = target["boxes"]
    txy = matcher.box_cxcywh_to_xyxy(tb)
    cx, cy = boxes[:, 0:1], boxes[:, 1:2]
    inside = (cx > txy[None, :, 0]) & (cx < txy[None, :, 2]) & (cy > txy[None, :, 1]) & (cy < txy[None, :, 3])
    r = center_radius / stride
    near = (cx > tb[None, :, 0] - r) & (cx < tb[None, :, 0] + r) & (cy > tb[None, :, 1] - r) & (cy < tb[None, :, 1] + r)
    return ~(inside & near), ~(inside.any(1) | near.any(1))


def masks_of_cost(cost):
    """the same two masks read off a cost matrix (Q, T): the class and GIoU terms stay far below 50 in magnitude"""
    far = cost > 5000.0
    return (cost - 10000.0 * far.to(cost.dtype)) > 50.0, far.all(1)


def reference_costs(logits, boxes, target, dtype):
    """matcher.ota_cost of one image in `dtype` on the CPU -> (cost (Q, T), iou (Q, T))"""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in target.items()}
    return matcher.ota_cost(logits.to(dtype).sigmoid(), boxes.to(dtype), t)


def preconditions(case, ties_allowed=False):
    """asserted on the CPU before any comparison (see the module docstring) -> per image with targets (cost64, iou64, cost32, iou32)"""
    logits, boxes, targets = case
    out = []
    for b, t in enumerate(targets):
        if len(t["boxes"]) == 0:
            out.append(None)
            continue
        c64, i64 = reference_costs(logits[b], boxes[b], t, torch.float64)
        c32, i32 = reference_costs(logits[b], boxes[b], t, torch.float32)
        Q = logits.shape[1]
        s = i64.topk(min(Q, 10), dim=0)[0].sum(0)
        away = float((s - s.round()).abs().min())
        assert away >= 1e-4, ("a top-10 IoU sum within 1e-4 of an integer", b, away)
        m64, m32 = centre_masks(boxes[b].double(), {"boxes": t["boxes"].double()}), centre_masks(boxes[b], t)
        assert torch.equal(m64[0], m32[0]) and torch.equal(m64[1], m32[1]), ("a centre on a box edge: the fp32 and float64 masks differ", b)
        if not ties_allowed:
            k = s.int().clamp(min=1)
            for j in range(c32.shape[1]):
                head = c32[:, j].sort().values[:min(Q, int(k[j]) + 1)]
                assert head.unique().numel() == head.numel(), ("a tie among the k + 1 cheapest queries of a target", b, j)
        out.append((c64, i64, c32, i32))
    return out


# ------------------------------------------------------------------------------------------------ the assignment rule, restated
def assign_rule(cost, iou):
    """matcher.dynamic_k_assign with loops, fp32 arithmetic and EVERY tie at the lowest index.  cost, iou (Q, T) fp32 (not modified) ->
    ((query idx, target idx of each), best query of every target, the final cost BEFORE the reference's last +inf step, repair rounds)"""
    cost = cost.detach().cpu().numpy().astype(np.float32).copy()
    iou = iou.detach().cpu().numpy().astype(np.float32)
    Q, T = cost.shape

    def first_min(v, allowed=None):
        """the lowest index among the smallest allowed values"""
        idx = np.arange(len(v)) if allowed is None else np.flatnonzero(allowed)
        return int(idx[np.flatnonzero(v[idx] == v[idx].min())[0]])

    match = np.zeros((Q, T), dtype=bool)
    for t in range(T):
        free = np.ones(Q, dtype=bool)
        s = np.float32(0.0)
        for _ in range(min(Q, 10)):                       # the largest IoUs in descending order, added one by one in fp32
            i = first_min(-iou[:, t], free)
            free[i] = False
            s = np.float32(s + iou[i, t])
        k = max(1, int(s))
        free = np.ones(Q, dtype=bool)
        for _ in range(k):
            i = first_min(cost[:, t], free)
            free[i] = False
            match[i, t] = True
    contested = match.sum(1) > 1                          # evaluated once: the stale set of the repair loop

    def keep_cheapest():
        for q in np.flatnonzero(contested):
            match[q] = False
            match[q, first_min(cost[q])] = True
    if contested.any():
        keep_cheapest()
    rounds = 0
    while (match.sum(0) == 0).any():
        rounds += 1
        assert rounds <= Q, "the repair loop does not end"
        cost[match.sum(1) > 0] += np.float32(100000.0)
        for t in np.flatnonzero(match.sum(0) == 0):
            match[first_min(cost[:, t]), t] = True
        if (match.sum(1) > 1).any():
            keep_cheapest()
    chosen = np.flatnonzero(match.sum(1) > 0)
    tgt = [int(np.flatnonzero(match[q])[0]) for q in chosen]          # the first target of the row
    best = [first_min(np.where(match[:, t], cost[:, t], np.float32(np.inf))) for t in range(T)]
    as_t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int64))          # noqa: E731
    return (as_t(chosen), as_t(tgt)), as_t(best), torch.from_numpy(cost), rounds


class TorchMatchingOps:
    """a stand-in for net.HipBackendMatching in plain torch on any device: the restated rule on matcher.ota_cost"""
    calls = 0

    @staticmethod
    def pack_ota_targets(targets, device):
        from hipie_amd.training.functions import pack_ota_targets
        return pack_ota_targets(targets, device)

    @classmethod
    def ota_match(cls, logits, boxes, packed, center_radius=2.5, stride=32):
        cls.calls += 1
        pairs, best = [], []
        for b, n in enumerate(packed.counts):
            if n == 0:
                e = torch.zeros(0, dtype=torch.int64, device=logits.device)
                pairs.append((e, e.clone()))
                best.append([])
                continue
            t = {"boxes": packed.tgt_boxes[b, :n], "positive_map": packed.pos_map[b, :n].bool()}
            p, q, _, _ = assign_rule(*matcher.ota_cost(logits[b].sigmoid(), boxes[b], t, center_radius, stride))
            pairs.append((p[0].to(logits.device), p[1].to(logits.device)))
            best.append(q.to(logits.device))
        return pairs, best
