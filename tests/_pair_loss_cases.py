"""Seeded inputs, a plain-torch stand-in for net.HipBackendPairLosses and the yardsticks of the pair-loss tests (csrc/pair_loss.hip):
test_pair_loss_cpu.py, test_gpu_pair_loss.py.

Reference: `loss_boxes` of the two criteria with ops=None -- today's criterion.py / boxes.py formulas -- on the CPU in float64 with autograd, on
the same fp32-representable inputs; e_lib: the same code in float32.  Metric: max|got - ref64| / max|ref64| per output tensor, bound per case
max(1e-6, 4 x e_lib) (_loss_cases.check, which prints every figure on a line starting with LOSS before it asserts)."""
import functools
import warnings

import torch
import torch.nn.functional as F

from _loss_cases import TorchLossOps, check, err          # noqa: F401  (re-exported to the two test files)
from hipie_amd.training import boxes as box_ops
from hipie_amd.training import functions
from hipie_amd.training.criterion import DetCriterion, MaskCriterion

NAMES = ("loss_bbox", "loss_giou", "loss_boxiou", "d_boxes", "d_iou")
PAD = 3                                         # the predictions are the slice [:, PAD:] of a larger tensor
FINISHER_ROWS = 64                              # partial rows one pass of the finishing workgroup covers (PB_GROUPS of csrc/pair_loss.hip)


# ------------------------------------------------------------------------------------------------ the stand-in
class TorchPairLossOps(TorchLossOps):
    """the `ops` object of the criteria with the two pair ops in plain torch, in the dtype of the predictions: the formulas of the kernels --
    no gather of per-image lists, no `thing.sum() == 0` branch, the stuff pairs of mode 1 filtered by a mask -- over the packed targets"""

    pack_match_targets = staticmethod(functions.pack_match_targets)
    pack_pair_targets = staticmethod(functions.pack_pair_targets)

    @staticmethod
    def _flat(pairs, which):
        return torch.cat([torch.full_like(p[0], b) for b, p in enumerate(pairs)]), torch.cat([p[which] for p in pairs])

    @classmethod
    def pair_box_loss(cls, pred_boxes, pred_iou, pairs, packed, count, mode, use_thing=True):
        bi, qi = cls._flat(pairs, 0)
        ti = cls._flat(pairs, 1)[1]
        if len(qi) == 0:
            return None
        src, tgt = pred_boxes[bi, qi], packed.tgt_boxes[bi, ti].to(pred_boxes.dtype)
        w = packed.is_thing[bi, ti].to(src.dtype) if use_thing else torch.ones_like(src[:, 0])
        sx, tx = box_ops.box_cxcywh_to_xyxy(src), box_ops.box_cxcywh_to_xyxy(tgt)
        status = torch.zeros(1, dtype=torch.int32)
        l1 = (src - tgt).abs().sum(1)
        if mode == 0:
            reweight = len(qi) / (w.float().sum() + 1e-6)                               # the criterion's `thing` is float32 whatever the boxes are
            res = [(l1 * w).sum() * reweight / count, (box_ops.paired_giou_loss(sx, tx) * w).sum() * reweight / count, None]
            if pred_iou is not None:
                score = pred_iou.reshape(pred_iou.shape[0], -1)[bi, qi]
                res[2] = (F.binary_cross_entropy_with_logits(score, box_ops.paired_iou(sx, tx).detach(), reduction="none") * w).sum() / len(qi) * reweight
            return (*res, status)
        keep = w != 0
        sx, tx = sx[keep], tx[keep]
        if bool(((sx[:, 2:] < sx[:, :2]) | (tx[:, 2:] < tx[:, :2])).any()):
            status += 1
        lo, hi = torch.maximum(sx[:, :2], tx[:, :2]), torch.minimum(sx[:, 2:], tx[:, 2:])
        inter = (hi - lo).clamp(min=0).prod(1)
        union = box_ops._area(sx) + box_ops._area(tx) - inter
        hull = (torch.maximum(sx[:, 2:], tx[:, 2:]) - torch.minimum(sx[:, :2], tx[:, :2])).clamp(min=0).prod(1)
        giou = inter / union - (hull - union) / (hull + 1e-7)
        return l1[keep].sum() / count, (1 - giou).sum() / count, None, status

    @classmethod
    def positive_onehot(cls, logits, pairs, packed):
        if packed.pos_map is None:
            return None
        onehot = torch.zeros_like(logits)
        bi, qi = cls._flat(pairs, 0)
        onehot[bi, qi] = packed.pos_map[bi, cls._flat(pairs, 1)[1]].to(logits.dtype)
        return onehot


# ------------------------------------------------------------------------------------------------ cases
class PairCase:
    """big (B, PAD + Q, 4) fp32 cxcywh and iou_big (B, PAD + Q, 1) logits -- the predictions are their slices [:, PAD:] --, per-image target
    dicts, pairs [(query idx, target idx)] and the upstream gradients g (3,) of the three scalars"""

    def __init__(self, big, iou_big, targets, pairs, g, count):
        self.big, self.iou_big, self.targets, self.pairs, self.g, self.count = big, iou_big, targets, pairs, g, count
        self.K = sum(len(q) for q, _ in pairs)


def _targets(gen, T, L, things):
    tb = torch.cat((0.2 + 0.6 * torch.rand(T, 2, generator=gen), 0.05 + 0.3 * torch.rand(T, 2, generator=gen)), 1)
    thing = {"mixed": torch.arange(T) % 3 != 1, "all": torch.ones(T, dtype=torch.bool), "none": torch.zeros(T, dtype=torch.bool)}[things]
    return {"boxes": tb, "is_thing": thing, "labels": torch.zeros(T, dtype=torch.long), "positive_map": torch.rand(T, L, generator=gen) < 0.2}


@functools.lru_cache(maxsize=None)
def pair_case(counts, seed=0, things="mixed", T=7, L=5):
    """counts: pairs per image (0: an image without a pair, which still has targets).  Every query is matched at most once; a third of the
    predictions sit near their target, the rest anywhere.  Cached: shared by the tests and never written to."""
    gen = torch.Generator().manual_seed(31 * seed + 1009 * sum(counts) + len(counts))
    B, Q = len(counts), max(max(counts), 1) + 2
    big = torch.cat((torch.rand(B, PAD + Q, 2, generator=gen), 0.02 + 0.5 * torch.rand(B, PAD + Q, 2, generator=gen)), 2)
    targets = [_targets(gen, T, L, things) for _ in counts]
    pairs = []
    for b, k in enumerate(counts):
        q = torch.randperm(Q, generator=gen)[:k]
        t = torch.randint(0, T, (k,), generator=gen)
        near = torch.arange(k) % 3 == 0
        big[b, PAD + q[near]] = targets[b]["boxes"][t[near]] + 0.02 * torch.randn(int(near.sum()), 4, generator=gen)
        pairs.append((q, t))
    big[..., 2:] = big[..., 2:].clamp(min=0.01)
    iou_big = 2.0 * torch.randn(B, PAD + Q, 1, generator=gen)
    g = torch.tensor([1.0, 0.7, 1.3]) + 0.2 * torch.rand(3, generator=gen)
    return PairCase(big, iou_big, targets, pairs, g, float(max(sum(counts), 1)) * 0.75)


def explicit_case(src, tgt, thing=None, duplicate=False):
    """one image whose pair i is (query i, target i) with the given cxcywh rows; duplicate: every pair is listed again against target 0"""
    src, tgt = torch.tensor(src, dtype=torch.float32), torch.tensor(tgt, dtype=torch.float32)
    K = len(src)
    big = torch.cat((torch.full((1, PAD, 4), 0.3), src[None]), 1)
    gen = torch.Generator().manual_seed(K)
    targets = [{"boxes": tgt, "is_thing": torch.ones(K, dtype=torch.bool) if thing is None else torch.tensor(thing, dtype=torch.bool),
                "labels": torch.zeros(K, dtype=torch.long), "positive_map": torch.ones(K, 1, dtype=torch.bool)}]
    q = t = torch.arange(K)
    if duplicate:
        q, t = torch.cat((q, q)), torch.cat((t, torch.zeros(K, dtype=torch.long)))
    return PairCase(big, torch.randn(1, PAD + K, 1, generator=gen), targets, [(q, t)], torch.tensor([1.0, 0.7, 1.3]), 2.0)


def to_dtype(targets, dtype):
    return [{k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()} for t in targets]


def criterion_of(mode, ops=None, ota=False, panoptic=True):
    if mode == 0:
        return DetCriterion(None, ["boxes"], panoptic_box_loss=panoptic, ota=ota, ops=ops)
    return MaskCriterion(1, None, ["boxes"], panoptic_on=panoptic, ops=ops)


def mask_loss_boxes_blockwise(out, targets, indices, count, panoptic, block=512):
    """MaskCriterion.loss_boxes with the diagonal of boxes.generalized_box_iou taken block by block: the criterion forms the (K, K) matrix of
    all pairs, 2 GiB in float64 at the 16 385 pairs of the largest case.  The same boxes.py code on every pair; test_pair_loss_cpu checks that
    it is the criterion's"""
    bi = torch.cat([torch.full_like(q, b) for b, (q, _) in enumerate(indices)])
    src = out["pred_boxes"][bi, torch.cat([q for q, _ in indices])]
    tgt = torch.cat([t["boxes"][j] for t, (_, j) in zip(targets, indices)])
    if panoptic:
        thing = torch.cat([t["is_thing"][j] for t, (_, j) in zip(targets, indices)]).bool()
        src, tgt = src[thing], tgt[thing]
    sx, tx = box_ops.box_cxcywh_to_xyxy(src), box_ops.box_cxcywh_to_xyxy(tgt)
    giou = torch.cat([torch.diagonal(box_ops.generalized_box_iou(sx[i:i + block], tx[i:i + block])) for i in range(0, len(sx), block)] or [sx[:, 0]])
    return {"loss_bbox": F.l1_loss(src, tgt, reduction="none").sum() / count, "loss_giou": (1 - giou).sum() / count}


def reference(case, mode, with_iou, dtype, ota=False, panoptic=True):
    """(loss_bbox, loss_giou, loss_boxiou, d_boxes, d_iou) of today's loss_boxes (ops=None) in `dtype` on the CPU: the gradients of
    sum_i g[i] loss_i for the (B, Q, 4) / (B, Q, 1) slices"""
    boxes = case.big[:, PAD:].to(dtype).requires_grad_()
    iou = case.iou_big[:, PAD:].to(dtype).requires_grad_()
    out = {"pred_boxes": boxes}
    if with_iou and mode == 0:
        out["pred_boxious"] = iou
    if mode == 1 and case.K > 2048:
        res = mask_loss_boxes_blockwise(out, to_dtype(case.targets, dtype), case.pairs, case.count, panoptic)
    else:
        res = criterion_of(mode, None, ota, panoptic).loss_boxes(out, to_dtype(case.targets, dtype), case.pairs, case.count)
    zero = boxes.sum() * 0.0
    losses = [res["loss_bbox"], res["loss_giou"], res.get("loss_boxiou", zero)]
    total = sum(g * l for g, l in zip(case.g.to(dtype), losses)) + zero + iou.sum() * 0.0
    total.backward()
    return (*[l.detach() for l in losses], boxes.grad, iou.grad)


@functools.lru_cache(maxsize=None)
def yardsticks(counts, mode, with_iou, seed=0, things="mixed", ota=False, panoptic=True):
    case = pair_case(counts, seed, things)
    return reference(case, mode, with_iou, torch.float64, ota, panoptic), reference(case, mode, with_iou, torch.float32, ota, panoptic)


# ------------------------------------------------------------------------------------------------ both criteria end to end
def criteria_case(seed=0, B=2, Q=30, L=12, aux=2, groups=2):
    """outputs, targets and de-noising parts for DetCriterion.forward and MaskCriterion.forward: B images, Q queries, `aux` auxiliary layers,
    encoder outputs, a de-noising part of `groups` groups; fp32 leaves with requires_grad, masks of 16 x 16"""
    gen = torch.Generator().manual_seed(900 + seed)
    counts = [4, 3][:B] + [2] * (B - 2)
    P = max(counts)
    targets = []
    for n in counts:
        t = _targets(gen, n, L, "mixed")
        t["positive_map"][:, 0] = True                                               # every target has a positive token
        t["masks"] = (torch.rand(n, 16, 16, generator=gen) > 0.5).float()
        t["labels"] = torch.randint(0, L, (n,), generator=gen)
        targets.append(t)

    def layer(q, masks=True, iou=False, tokens=L):
        o = {"pred_logits": torch.randn(B, q, tokens, generator=gen).requires_grad_(),
             "pred_boxes": torch.cat((0.2 + 0.6 * torch.rand(B, q, 2, generator=gen), 0.05 + 0.3 * torch.rand(B, q, 2, generator=gen)), 2).requires_grad_(),
             "text_masks": torch.ones(B, tokens, dtype=torch.bool)}
        if masks:
            o["pred_masks"] = torch.randn(B, q, 8, 8, generator=gen).requires_grad_()
        if iou:
            o["pred_boxious"] = torch.randn(B, q, 1, generator=gen).requires_grad_()
        return o
    pad = 2 * P * groups
    det = layer(Q, masks=False)
    det["aux_outputs"] = [layer(Q, masks=False, iou=True) for _ in range(aux)]
    det["enc_outputs"] = layer(Q, masks=False, tokens=1)                               # the binary objectness of the encoder proposals
    known = layer(pad, masks=False)
    known["aux_outputs"] = [layer(pad, masks=False) for _ in range(aux)]
    dn_meta = {"dn_num": groups, "single_padding": 2 * P, "output_known_lbs_bboxes": known}
    det_idx = [[(torch.randperm(Q, generator=gen)[:n], torch.randperm(n, generator=gen)) for n in counts] for _ in range(aux + 1)]
    md = layer(Q)
    md["aux_outputs"] = [layer(Q) for _ in range(aux)]
    md["interm_outputs"] = layer(Q)
    md_known = layer(P * groups)
    md_known["aux_outputs"] = [layer(P * groups) for _ in range(aux)]
    mask_dict = {"output_known_lbs_bboxes": md_known, "scalar": groups, "pad_size": P * groups}
    return targets, det, det_idx, dn_meta, md, mask_dict


class ReplayMatcher:
    """a matcher that hands out, call by call, the pairs another run's matcher returned (moved to the host): the float64 reference of a GPU
    run then scores the same pairs whatever a near-tie in the costs would have done"""

    def __init__(self, recorded):
        self.recorded = list(recorded)

    def _next(self, *a, **k):
        return [(q.cpu(), t.cpu()) for q, t in self.recorded.pop(0)]

    __call__ = forward_boxes_only = _next


class RecordingMatcher:
    """a HungarianMatcher whose answers are kept in `recorded`"""

    def __init__(self, matcher):
        self.matcher, self.recorded = matcher, []
        if getattr(matcher, "pack", None) is not None and matcher.ops is not None:
            self.pack = matcher.pack

    def __call__(self, *a, **k):
        self.recorded.append(self.matcher(*a, **k))
        return self.recorded[-1]

    def forward_boxes_only(self, *a, **k):
        self.recorded.append(self.matcher.forward_boxes_only(*a, **k))
        return self.recorded[-1]


def _draw(dtype, device):
    gen = torch.Generator().manual_seed(5)
    return lambda shape, dev: torch.rand(tuple(shape), generator=gen, dtype=dtype).to(device)


def both_criteria(ops, dtype=torch.float64, device="cpu", matcher=None, omit_ops=False, matcher_ops=None):
    """DetCriterion.forward and MaskCriterion.forward on criteria_case in `dtype` on `device` -> (loss dict, gradient of every input by path for
    sum_k w_k loss_k with w_k = 1 + 0.01 x the rank of the key, the two criteria, the matcher).  matcher: None = a HungarianMatcher with
    `matcher_ops` whose answers are recorded, or a ReplayMatcher"""
    from hipie_amd.training.matcher import HungarianMatcher, MatchWeights
    targets, det, det_idx, dn_meta, md, mask_dict = convert(criteria_case(), dtype, device)
    kw = {} if omit_ops else {"ops": ops}
    if matcher is None:                                      # matcher.mask_costs samples in float32
        matcher = RecordingMatcher(HungarianMatcher(MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0), num_points=16, draw=_draw(torch.float32, device), class_mode="map",
                                                    ops=matcher_ops, defer_status=matcher_ops is not None))
    dc = DetCriterion(matcher, ["labelsVL", "boxes"], still_cls_for_encoder=True, ota=True, draw=_draw(dtype, device), **kw)
    mc = MaskCriterion(12, matcher, ["labels", "masks", "boxes"], vl_loss=True, num_points=16, dn="seg", dn_losses=["labels", "masks", "boxes"],
                       draw=_draw(dtype, device), **kw)
    losses = {"det/" + k: v for k, v in dc(det, targets, det_idx, dn_meta).items()}
    losses.update({"md/" + k: v for k, v in mc(md, targets, mask_dict).items()})
    sum((1.0 + 0.01 * i) * losses[k] for i, k in enumerate(sorted(losses))).backward()
    grads = {p: (torch.zeros_like(x) if x.grad is None else x.grad) for p, x in leaves([det, dn_meta, md, mask_dict])}
    return {k: v.detach() for k, v in losses.items()}, grads, (dc, mc), matcher


def leaves(tree):
    """the requires_grad tensors of a nested dict / list, in a fixed order, with their paths"""
    out = []

    def walk(x, path):
        if torch.is_tensor(x):
            if x.requires_grad:
                out.append((path, x))
        elif isinstance(x, dict):
            for k in sorted(x):
                walk(x[k], path + "/" + str(k))
        elif isinstance(x, (list, tuple)):
            for i, v in enumerate(x):
                walk(v, path + "/%d" % i)
    walk(tree, "")
    return out


def convert(tree, dtype=None, device=None):
    """a deep copy of a nested dict / list with fresh leaves: floating tensors in `dtype`, everything on `device`"""
    if torch.is_tensor(tree):
        x = tree.detach().to(device=device, dtype=dtype if tree.is_floating_point() else None).clone()
        return x.requires_grad_() if tree.requires_grad else x
    if isinstance(tree, dict):
        return {k: convert(v, dtype, device) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(convert(v, dtype, device) for v in tree)
    return tree


def host_waits(fn):
    """the synchronising calls of fn() as torch's sync debug mode reports them (one warning each) -> (count, fn's result)"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for w in seen if "synchroniz" in str(w.message).lower()), out
