"""Seeded inputs, a plain-torch stand-in for net.HipBackendHungarian and the yardsticks of the Hungarian cost tests (csrc/hungarian_cost.hip):
test_hungarian_cost_cpu.py, test_gpu_hungarian_cost.py.

Costs.  Reference: matcher.cost_matrix evaluated on the CPU in float64 on the same fp32 inputs (the mask costs from matcher.mask_costs in
float64); e_lib: the same code in float32.  Per image block max|got - ref64| / max|ref64| against max(1e-6, 4 x e_lib) (_loss_cases.err /
bound_of).  NaN positions are compared first and exactly; the magnitudes then on everything else.
Assignment.  (a) exact: the returned pairs are scipy's on a copy of the kernel's own block.  (b) optimality: an entry-wise error of `bound` x
max|ref64| moves the total of any assignment of n = min(Q, T) pairs by at most n times that, so the float64 total of the returned pairs lies
within 2 n x bound x max|ref64| of the float64 optimum.  (c) equality with the torch path's pairs only where the float64 optimum is separated
from the second-best assignment (`assignment_gap`) by more than the quantity of (b): otherwise two assignments may legitimately swap."""
import functools
import os

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from _loss_cases import bound_of, err          # noqa: F401  (re-exported to the two test files)
from _ota_cases import GOLD, _image, golden_cases          # noqa: F401
from _point_select_cases import mask_costs_in
from hipie_amd.training import matcher
from hipie_amd.training.matcher import MatchWeights

# (B, Q, T, L, an extra image without targets): the smallest; one target; more targets than queries; nothing a multiple of anything with the
# packed offsets of three images; several bit words per target row; the production width
SHAPES = [(1, 4, 3, 8, False), (1, 40, 1, 16, False), (1, 20, 37, 16, False), (2, 70, 9, 33, True), (1, 300, 37, 64, False), (2, 900, 100, 256, False)]
SMALL = SHAPES[:4]                               # Q x T <= 740: the shapes whose optimum is asserted to be separated (see (c))
SEEDS = (0, 1)
IDS = lambda s: "x".join(map(str, s[:4]))          # noqa: E731
MASK_HW, TGT_HW = (8, 10), (32, 40)              # predicted masks (Q, 8, 10), target masks (T, 32, 40)
W_BOX = MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0)


@functools.lru_cache(maxsize=None)
def hungarian_case(B, Q, T, L, empty, seed, things="mixed"):
    """-> (logits (B', Q, L), boxes (B', Q, 4), targets, pred masks (B', Q, 8, 10)): the images of _ota_cases._image (image 0 has T targets, the
    later ones two thirds of them, with `empty` a last image without any) with labels in [0, L), is_thing = arange(T) % 3 != 1 ("none": no
    thing in image 0, "all": only things everywhere) and soft target masks.  Cached: shared by the tests and never written to."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Q + T)
    counts = [T] + [max(1, (2 * T) // 3)] * (B - 1) + ([0] if empty else [])
    imgs = [_image(g, Q, n, L) for n in counts]
    h = torch.Generator().manual_seed(77 + 1000 * seed + 7 * Q + T)
    targets = []
    for b, (_, _, t) in enumerate(imgs):
        n = len(t["boxes"])
        t = dict(t)
        t["labels"] = torch.randint(0, L, (n,), generator=h)
        t["is_thing"] = torch.arange(n) % 3 != 1
        if things == "all" or (things == "none" and b > 0):
            t["is_thing"] = torch.ones(n, dtype=torch.bool)
        elif things == "none":
            t["is_thing"] = torch.zeros(n, dtype=torch.bool)
        t["masks"] = (torch.rand(n, *TGT_HW, generator=h) * 1.5 - 0.25).clamp(0, 1)
        targets.append(t)
    pred = 3.0 * torch.randn(len(counts), Q, *MASK_HW, generator=h)
    return torch.stack([i[0] for i in imgs]), torch.stack([i[1] for i in imgs]), targets, pred


@functools.lru_cache(maxsize=None)
def case_coords(n_images, P, seed):
    """one (P, 2) point set per image, a few of them on the border and on pixel centres"""
    g = torch.Generator().manual_seed(4242 + seed + P)
    c = torch.rand(n_images, P, 2, generator=g)
    c[:, 0] = 0.0
    c[:, 1] = 1.0
    c[:, 2] = torch.tensor([2.5 / MASK_HW[1], 1.5 / MASK_HW[0]])
    return c


def to_dtype(target, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in target.items()}


class _MaskCostsIn:
    """matcher.mask_costs casts its operands to float32; _point_select_cases.mask_costs_in is the same code in the dtype of its inputs"""
    mask_match_costs = staticmethod(mask_costs_in)


def reference_cost(logits, boxes, target, w, dtype, masks=None, coords=None, stuff_takes_mean=True, with_boxes=True, class_mode="map"):
    """matcher.cost_matrix of one image in `dtype` on the CPU (its mask costs: matcher.mask_costs in that dtype) -> (Q, T)"""
    return matcher.cost_matrix(logits.to(dtype), boxes.to(dtype), to_dtype(target, dtype), w, None if masks is None else masks.to(dtype),
                               None if coords is None else coords.to(dtype), stuff_takes_mean, with_boxes, class_mode, _MaskCostsIn)


def same_pairs(got, want):
    return len(got) == len(want) and all(torch.equal(g[0].cpu(), w[0].cpu()) and torch.equal(g[1].cpu(), w[1].cpu()) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ the assignment yardsticks
def total_cost(C64, pairs):
    """the float64 total of an assignment on the float64 matrix"""
    C = np.asarray(C64, dtype=np.float64)
    return float(C[np.asarray(pairs[0]), np.asarray(pairs[1])].sum())


def optimum(C64):
    C = np.asarray(C64, dtype=np.float64)
    i, j = linear_sum_assignment(C)
    return float(C[i, j].sum()), (i, j)


def assignment_gap(C64):
    """second-best total - best total of the float64 matrix: the second-best assignment differs from the optimum in at least one pair, so it
    is the minimum over the re-solves with one optimal pair forbidden (+inf when no other complete assignment exists)"""
    C = np.asarray(C64, dtype=np.float64)
    best, (i, j) = optimum(C)
    second = np.inf
    for a, b in zip(i, j):
        D = C.copy()
        D[a, b] = np.inf
        try:
            second = min(second, optimum(D)[0])
        except ValueError:                                   # infeasible without that pair
            pass
    return second - best


def slack(C64, bound):
    """what an entry-wise error of bound x max|ref64| can move the total of an assignment by, twice (the optimum and its rival)"""
    C = np.asarray(C64, dtype=np.float64)
    return 2.0 * min(C.shape) * bound * float(np.abs(C).max())


# ------------------------------------------------------------------------------------------------ the reference's own instances
class Golden:
    """tests/golden/train_matcher.npz: the inputs, the recorded draws and every Hungarian pair set of the reference's matchers"""

    def __init__(self, dev="cpu"):
        self.z = np.load(os.path.join(GOLD, "train_matcher.npz"))
        self.dev = dev
        keys = ("labels", "boxes", "positive_map", "is_thing", "masks")
        self.targets = [{k: self["t%d_%s" % (i, k)] for k in keys if "t%d_%s" % (i, k) in self.z.files} for i in range(3)]
        self.ones = [dict(t, positive_map=torch.ones(len(t["boxes"]), 1, dtype=torch.bool, device=dev)) for t in self.targets]
        self.w = MatchWeights(*[float(x) for x in self.z["weights"]])
        self.md_w = MatchWeights(*[float(x) for x in self.z["md_weights"]])

    def __getitem__(self, k):
        return torch.from_numpy(self.z[k]).to(self.dev)

    def pairs(self, prefix):
        return [(self["%s%d_q" % (prefix, i)].cpu(), self["%s%d_t" % (prefix, i)].cpu()) for i in range(3)]

    def rands(self, prefix):
        out, i = [], 0
        while "%s%d" % (prefix, i) in self.z.files:
            out.append(self["%s%d" % (prefix, i)])
            i += 1
        return out

    def run(self, ops, draw_of, packed=True):
        """every recorded Hungarian pair set through HungarianMatcher(ops=ops) -> {set: (got, want)}; draw_of(tensors) makes the replaying
        `draw`; packed: hand the matcher targets packed once per matcher (False: it packs them itself)"""
        from hipie_amd.training.matcher import HungarianMatcher
        out = {}
        draw = draw_of(self.rands("rand"))
        m = HungarianMatcher(self.w, num_points=112 * 112, stuff_takes_mean=True, draw=draw, class_mode="map", ops=ops)
        kw = lambda t, masks=True: {"packed": m.pack(t, self.dev, masks)} if packed else {}          # noqa: E731
        p = kw(self.targets)
        out["box"] = (m(self["logits"], self["boxes"], self.targets, **p), self.pairs("box"))
        out["mask"] = (m(self["logits"], self["boxes"], self.targets, masks=self["pmasks"], **p), self.pairs("mask"))
        assert draw.done()
        out["enc"] = (m.forward_boxes_only(self["logits"][..., :1], self["boxes"], self.ones, **kw(self.ones, False)), self.pairs("enc"))
        draw = draw_of(self.rands("md_rand"))
        md = HungarianMatcher(self.md_w, num_points=300, stuff_takes_mean=True, draw=draw, class_mode="ids", ops=ops)
        out["md"] = (md(self["md_logits"], self["boxes"], self.targets, masks=self["md_masks"], **kw(self.targets)), self.pairs("md"))
        md.class_mode = "map"
        out["mdvl"] = (md(self["logits"], self["boxes"], self.targets, masks=self["md_masks"], **kw(self.targets)), self.pairs("mdvl"))
        assert draw.done()
        return out


# ------------------------------------------------------------------------------------------------ the stand-in
class TorchHungarianOps:
    """a stand-in for net.HipBackendHungarian in plain torch on any device: the packed layout of hipie_hungarian_cost restated -- image b's
    (Q, n_b) block is written query-major at element Q * t_off[b] of ONE flat buffer, which goes to the host in one piece -- with
    matcher.cost_matrix per image for the arithmetic"""
    calls = []                                   # (stuff_takes_mean, with_boxes, class_mode, masks given) of every hungarian_costs call
    decline = False

    @staticmethod
    def pack_match_targets(targets, device, with_masks=True):
        from hipie_amd.training.functions import pack_match_targets
        return pack_match_targets(targets, device, with_masks)

    @staticmethod
    def mask_match_costs(pred, tgt, coords):
        return matcher.mask_costs(pred, tgt, coords)

    @classmethod
    def hungarian_costs(cls, logits, boxes, packed, w, masks=None, coords=None, stuff_takes_mean=True, with_boxes=True, class_mode="auto"):
        cls.calls.append((stuff_takes_mean, with_boxes, class_mode, masks is not None))
        if cls.decline:
            return None
        B, Q, L = logits.shape
        n_tgt, t_off = packed.n_tgt.tolist(), packed.t_off.tolist()
        assert n_tgt == packed.counts and t_off == [sum(n_tgt[:b]) for b in range(B)]
        flat = torch.full((Q * sum(n_tgt),), float("nan"), dtype=torch.float32, device=logits.device)
        for b, n in enumerate(n_tgt):
            t = {"boxes": packed.tgt_boxes[b, :n], "is_thing": packed.is_thing[b, :n]}
            if packed.pos_map is not None:
                t["positive_map"] = packed.pos_map[b, :n].bool()
            if packed.labels is not None:
                t["labels"] = packed.labels[b, :n].long()
            if masks is not None:
                t["masks"] = packed.tgt_masks[b] if n else logits.new_zeros(0, 1, 1)
            C = matcher.cost_matrix(logits[b].float(), boxes[b].float(), t, w, None if masks is None else masks[b].float(), None if masks is None else coords[b],
                                    stuff_takes_mean, with_boxes, class_mode, cls)
            flat[Q * t_off[b]:Q * (t_off[b] + n)] = C.reshape(-1)
        host = flat.cpu().numpy()
        return [host[Q * o:Q * (o + n)].reshape(Q, n) for o, n in zip(t_off, n_tgt)]
