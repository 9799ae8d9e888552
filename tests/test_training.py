"""Training-side host logic (matching costs + assignment, the set-prediction losses of both heads, contrastive de-noising
queries) against the reference's OWN classes, run on the CPU of the build container by tests/golden/gen_train_golden.py
(HungarianMatcherVL, MaskDINO's HungarianMatcher, SetCriterion / DINOCriterion, MaskDINO's SetCriterion, prepare_for_cdn).  The fixtures
hold the inputs, every random tensor the reference drew (replayed here in the same order) and its outputs.  Device-agnostic: the same
checks run on the GPU under -m gpu."""
import os

import numpy as np
import pytest
import torch

from hipie_amd.training import (prepare_targets, split_things_stuff, maskdino_dn_queries, maskdino_loss_plan, weighted_merge, DetCriterion, HungarianMatcher, MaskCriterion, MatchWeights, cdn_queries, dn_match_indices, dn_split_outputs,
                                generalized_box_iou, paired_giou_loss, paired_iou, box_cxcywh_to_xyxy)
from hipie_amd.training.criterion import uncertain_points
from hipie_amd.training.matcher import class_cost, mask_costs

from _train_step_cases import OracleBackend as _OracleBackend, check_step_against_golden, train_step_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="cuda", marks=pytest.mark.gpu)]


class Fixture:
    def __init__(self, name, device):
        self.z = np.load(os.path.join(GOLD, name + ".npz"))
        self.dev = device

    def __getitem__(self, k):
        return torch.from_numpy(self.z[k]).to(self.dev)

    def __contains__(self, k):
        return k in self.z.files

    def targets(self, prefix, n):
        keys = ("labels", "boxes", "positive_map", "is_thing", "masks")
        return [{k: self["%s%d_%s" % (prefix, i, k)] for k in keys if "%s%d_%s" % (prefix, i, k) in self} for i in range(n)]

    def pairs(self, prefix, n):
        return [(self["%s%d_q" % (prefix, i)].cpu(), self["%s%d_t" % (prefix, i)].cpu()) for i in range(n)]

    def rands(self, prefix="rand"):
        out, i = [], 0
        while "%s%d" % (prefix, i) in self:
            out.append(self["%s%d" % (prefix, i)])
            i += 1
        return out


class Replay:
    """a `draw` that hands out the reference's recorded random tensors in call order and insists on the shapes"""

    def __init__(self, tensors):
        self.t, self.i = list(tensors), 0

    def __call__(self, shape, device):
        r = self.t[self.i]
        self.i += 1
        assert tuple(r.shape) == tuple(shape), "draw %d: reference drew %s, the build asks for %s" % (self.i - 1, tuple(r.shape), tuple(shape))
        return r.to(device)

    def done(self):
        return self.i == len(self.t)


def same_pairs(got, want):
    return len(got) == len(want) and all(torch.equal(g[0].cpu(), w[0]) and torch.equal(g[1].cpu(), w[1]) for g, w in zip(got, want))


def close(a, b, tol=2e-5):
    a, b = a.double().cpu(), b.double().cpu()
    if a.shape != b.shape:
        return False
    if a.numel() == 0:
        return True
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("dev", DEVICES)
def test_matchers_give_the_reference_assignments(dev):
    f = Fixture("train_matcher", dev)
    targets = f.targets("t", 3)
    w = MatchWeights(*[float(x) for x in f.z["weights"]])
    draw = Replay(f.rands())
    m = HungarianMatcher(w, num_points=112 * 112, stuff_takes_mean=True, draw=draw, class_mode="map")
    assert same_pairs(m(f["logits"], f["boxes"], targets), f.pairs("box", 3))                       # box + class costs; image 2 holds stuff only
    assert same_pairs(m(f["logits"], f["boxes"], targets, masks=f["pmasks"]), f.pairs("mask", 3))    # + point-sampled mask costs
    assert draw.done()
    ones = [dict(t, positive_map=torch.ones(len(t["boxes"]), 1, dtype=torch.bool, device=dev)) for t in targets]
    assert same_pairs(m.forward_boxes_only(f["logits"][..., :1], f["boxes"], ones), f.pairs("enc", 3))
    # the cost terms themselves
    assert close(class_cost(f["logits"][0].sigmoid(), targets[0], "map"), f["cls0"], 1e-6)
    ce, dice = mask_costs(f["pmasks"][0], targets[0]["masks"], f["rand0"][0])
    assert close(ce, f["ce0"], 1e-5) and close(dice, f["dice0"], 1e-5)
    assert close(generalized_box_iou(box_cxcywh_to_xyxy(f["boxes"][0]), box_cxcywh_to_xyxy(targets[0]["boxes"])), f["giou0"], 1e-6)
    # MaskDINO's matcher: class ids, then positive maps
    draw = Replay(f.rands("md_rand"))
    wm = MatchWeights(*[float(x) for x in f.z["md_weights"]])
    md = HungarianMatcher(wm, num_points=300, stuff_takes_mean=True, draw=draw, class_mode="ids")
    assert same_pairs(md(f["md_logits"], f["boxes"], targets, masks=f["md_masks"]), f.pairs("md", 3))
    md.class_mode = "map"
    assert same_pairs(md(f["logits"], f["boxes"], targets, masks=f["md_masks"]), f.pairs("mdvl", 3))
    assert draw.done()
    # SimOTA: one-to-many pairs and the best query of every target; the third image has no target
    empty = {k: v[:0] for k, v in targets[2].items()}
    got, best = m.forward_ota(f["logits"], f["ota_boxes"], targets[:2] + [empty])
    assert same_pairs(got, f.pairs("ota", 3)) and len(got[0][0]) > len(targets[0]["boxes"])          # more queries than targets: one-to-many
    assert all(torch.equal(torch.as_tensor(best[i]).cpu().long(), f["ota_best%d" % i].cpu()) for i in range(3))
    tie_t = [{"labels": torch.zeros(3, dtype=torch.long, device=dev), "boxes": f["tie_boxes"], "positive_map": targets[0]["positive_map"][:3]}]
    got, best = m.forward_ota(f["tie_logits"], f["tie_queries"], tie_t)                  # two coinciding targets: the repair loop runs
    assert same_pairs(got, f.pairs("tie", 1)) and torch.equal(best[0].cpu(), f["tie_best"].cpu())
    with pytest.raises(ValueError):
        HungarianMatcher(MatchWeights(0, 0, 0, 0, 1))
    with pytest.raises(ValueError):
        generalized_box_iou(torch.tensor([[0.5, 0.5, 0.4, 0.6]]), torch.tensor([[0.1, 0.1, 0.2, 0.2]]))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("tag", ["dyn", "ids", "one"])
def test_cdn_queries_match_prepare_for_cdn(dev, tag):
    f = Fixture("train_dn", dev)
    n_img = {"dyn": 3, "ids": 2, "one": 1}[tag]
    targets = f.targets(tag + "_t", n_img)
    dn_number, ratio, scale, nq, ncls = [float(x) for x in f.z[tag + "_args"]]
    r = f.rands(tag + "_rand")
    emb = f[tag + "_emb"]
    if tag == "ids":                                        # class-id embeddings with label noise: p, new labels, then the box noise
        noise = {"p": r[0], "new_label": r[1], "sign": r[2] * 2 - 1, "part": r[3]}
        label_embed = lambda ids: emb[ids]                  # noqa: E731
    else:
        noise = {"sign": r[0] * 2 - 1, "part": r[1]}
        label_embed = emb
    ql, qb, mask, meta = cdn_queries(targets, int(dn_number), scale, int(nq), label_embed, noise, ratio, int(ncls))
    assert [meta["single_padding"], meta["dn_num"], meta["dp_num"]] == [int(x) for x in f.z[tag + "_meta"]]
    assert torch.equal(mask.cpu(), f[tag + "_mask"].cpu())
    assert close(ql, f[tag + "_label"], 1e-7) and close(qb, f[tag + "_box"], 1e-6)
    assert same_pairs(dn_match_indices(targets, meta), f.pairs(tag + "_idx", n_img))
    # the de-noising / matching split of the decoder outputs
    pad = meta["single_padding"] * meta["dn_num"]
    x = torch.arange(2 * n_img * (pad + int(nq)) * 3, device=dev).reshape(2, n_img, pad + int(nq), 3)
    known, match = dn_split_outputs(x, meta)
    assert known.shape[2] == pad and match.shape[2] == int(nq) and torch.equal(torch.cat((known, match), 2), x)
    assert dn_split_outputs(x, None)[0] is None


def test_cdn_queries_without_targets_or_groups():
    empty = [{"labels": torch.zeros(0, dtype=torch.long), "boxes": torch.zeros(0, 4)}]
    assert cdn_queries(empty, 10, 0.4, 5, torch.zeros(1, 4)) == (None, None, None, None)
    one = [{"labels": torch.zeros(2, dtype=torch.long), "boxes": torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.3, 0.3, 0.1, 0.1]])}]
    assert cdn_queries(one, 0, 0.4, 5, torch.zeros(1, 4))[0] is None
    ql, qb, mask, meta = cdn_queries(one, 1, 0.4, 5, torch.ones(1, 4))       # fewer requested queries than targets: still one group
    assert meta == {"single_padding": 4, "dn_num": 1, "dp_num": 0} and ql.shape == (1, 4, 4) and mask.shape == (9, 9)
    assert bool(mask[4:, :4].all()) and not bool(mask[:4, :4].any()) and not bool(mask[:, 4:].any())
    b = torch.sigmoid(qb[0])                                                  # positives stay within half a box of their target, negatives leave it
    assert float((b[:2, :2] - one[0]["boxes"][:, :2]).abs().max()) <= 0.4 * 0.1 + 1e-6


def _det_outputs(f, layers):
    outs = []
    for i in range(layers):
        outs.append({"pred_logits": f["l%d_logits" % i], "pred_boxes": f["l%d_boxes" % i], "pred_boxious": f["l%d_boxious" % i], "text_masks": f["text_masks"],
                     "pred_masks": [f["l%d_pred_masks%d" % (i, b)] for b in range(2)]})
    return outs


@pytest.mark.parametrize("dev", DEVICES)
def test_detection_criterion_matches_dino_criterion(dev):
    f = Fixture("train_criterion", dev)
    SP, G, layers = [int(x) for x in f.z["meta"]]
    targets = f.targets("t", 2)
    outs = _det_outputs(f, layers)
    indices = [f.pairs("l%d_idx" % i, 2) for i in range(layers)]
    indices = [[(a.to(dev), b.to(dev)) for a, b in layer] for layer in indices]
    outputs = dict(outs[-1])
    outputs["aux_outputs"] = outs[:-1]
    outputs["enc_outputs"] = {"pred_logits": f["enc_logits"], "pred_boxes": f["enc_boxes"], "text_masks": f["text_masks"]}
    known = {"pred_logits": f["known_logits"], "pred_boxes": f["known_boxes"], "text_masks": f["text_masks"],
             "aux_outputs": [{"pred_logits": f["known_aux%d_logits" % i], "pred_boxes": f["known_aux%d_boxes" % i], "text_masks": f["text_masks"]}
                             for i in range(layers - 1)]}
    dn_meta = {"single_padding": SP, "dn_num": G, "dp_num": 0, "output_known_lbs_bboxes": known}
    draw = Replay(f.rands())
    matcher = HungarianMatcher(MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0), class_mode="map")
    crit = DetCriterion(matcher, ["labelsVL", "boxes", "masks"], still_cls_for_encoder=True, num_points=500, draw=draw)
    got = crit(outputs, targets, indices, dn_meta)
    want = {k[5:]: float(f.z[k]) for k in f.z.files if k.startswith("loss_")}
    assert set(got) == set(want), (sorted(set(got) ^ set(want)))
    bad = {k: (float(got[k]), want[k]) for k in want if abs(float(got[k]) - want[k]) > 2e-5 * max(1.0, abs(want[k]))}
    assert not bad, bad
    assert draw.done()
    assert len(want) == 6 * layers + 3 + 3 * layers       # per layer ce / bbox / giou / boxiou / mask / dice; encoder and de-noising (no IoU head): 3 each
    # OTA: one-to-many pairs from forward_ota, every loss normalised by the number of matched pairs
    ota_out = dict(outs[-1], pred_boxes=f["ota_boxes"], pred_masks=[f["ota_masks0"], f["ota_masks1"]])
    ota_idx, _ = matcher.forward_ota(ota_out["pred_logits"], ota_out["pred_boxes"], targets)
    assert same_pairs(ota_idx, f.pairs("ota_idx", 2))
    draw = Replay(f.rands("ota_rand"))
    got = DetCriterion(matcher, ["labelsVL", "boxes", "masks"], num_points=300, draw=draw, ota=True)(ota_out, targets, [ota_idx])
    want = {k[8:]: float(f.z[k]) for k in f.z.files if k.startswith("otaloss_")}
    got = {k: v for k, v in got.items() if "_dn" not in k}               # SetCriterion.forward (no de-noising part) is what the fixture ran
    assert set(got) == set(want) and not {k: (float(got[k]), want[k]) for k in want if abs(float(got[k]) - want[k]) > 2e-5 * max(1.0, abs(want[k]))}
    assert draw.done()
    # full-resolution (not point-sampled) mask losses, the zero entries without de-noising queries, the third-party box formulas
    dense = DetCriterion(matcher, ["masks"], point_sample_masks=False).loss_masks(outs[-1], targets, indices[-1], 7.0)
    assert abs(float(dense["loss_mask"]) - float(f.z["dense_loss_mask"])) < 1e-5 and abs(float(dense["loss_dice"]) - float(f.z["dense_loss_dice"])) < 1e-5
    nodn = crit.dn_losses(None, targets, layers - 1, 7.0, dev)
    assert set(nodn) == {k[5:] for k in f.z.files if k.startswith("nodn_")} and all(float(v) == 0 for v in nodn.values())
    assert close(paired_giou_loss(f["giou_a"], f["giou_b"]), 1 - f["giou_pairwise_diag"], 1e-6)
    assert close(paired_iou(f["giou_a"], f["giou_b"]), f["iou_diag"], 1e-6)


@pytest.mark.parametrize("dev", DEVICES)
def test_maskdino_criterion_matches_the_reference(dev):
    f = Fixture("train_maskdino", dev)
    groups, single, NC = [int(x) for x in f.z["meta"]]
    targets = f.targets("t", 2)

    def out(prefix):
        return {k: f[prefix + k] for k in ("pred_logits", "pred_boxes", "pred_masks")}
    outputs = out("main_")
    outputs["aux_outputs"] = [out("aux0_"), out("aux1_")]
    outputs["interm_outputs"] = out("interm_")
    known = out("known_")
    known["aux_outputs"] = [out("known_aux0_"), out("known_aux1_")]
    mask_dict = {"output_known_lbs_bboxes": known, "scalar": groups, "pad_size": groups * single}

    def build(draw):
        matcher = HungarianMatcher(MatchWeights(4.0, 5.0, 2.0, 5.0, 5.0), num_points=200, stuff_takes_mean=True, draw=draw, class_mode="ids")
        return MaskCriterion(NC, matcher, ["labels", "masks", "boxes"], vl_loss=False, num_points=200, dn="seg", dn_losses=["labels", "masks", "boxes"],
                             panoptic_on=True, draw=draw)
    for prefix, rprefix, outs, md in (("loss_", "rand", outputs, mask_dict), ("nodn_", "nodn_rand", {k: v for k, v in outputs.items() if k != "interm_outputs"}, None)):
        draw = Replay(f.rands(rprefix))
        got = build(draw)(outs, targets, md)
        want = {k[len(prefix):]: float(f.z[k]) for k in f.z.files if k.startswith(prefix) and not k.startswith("nodn_rand")}
        assert set(got) == set(want), sorted(set(got) ^ set(want))
        bad = {k: (float(got[k]), want[k]) for k in want if abs(float(got[k]) - want[k]) > 2e-5 * max(1.0, abs(want[k]))}
        assert not bad, bad
        assert draw.done()
    with pytest.raises(ValueError):
        build(Replay(f.rands()))(outputs, targets, dict(mask_dict, pad_size=5))


def test_uncertain_points_prefer_the_decision_boundary():
    g = torch.Generator().manual_seed(0)
    logits = torch.linspace(-8, 8, 64).repeat(64, 1)[None, None]            # the boundary (logit 0) is the vertical centre line
    pts = uncertain_points(logits, 200, 3.0, 0.75, lambda shape, device: torch.rand(shape, generator=g))
    assert pts.shape == (1, 200, 2)
    assert float((pts[0, :150, 0] - 0.5).abs().mean()) < 0.1 < float((pts[0, 150:, 0] - 0.5).abs().mean())


def test_maskdino_loss_plan_and_merge():
    import json
    plans = json.load(open(os.path.join(GOLD, "train_weights.json")))
    for tag, p in plans.items():
        a = p["args"]
        w, dn_losses, matcher, losses = maskdino_loss_plan(4.0, 5.0, 5.0, 5.0, 2.0, a["TWO_STAGE"], a["DN"], a["DEEP_SUPERVISION"], 3, a["BOX_LOSS"],
                                                           4.0, 5.0, 5.0, 5.0, 2.0, 12544, True)
        assert w == p["weights"] and dn_losses == p["dn_losses"] and losses == p["losses"], tag
        mw = matcher.w
        assert [mw.cls, mw.l1, mw.giou, mw.mask, mw.dice, matcher.num_points, matcher.class_mode == "map", matcher.stuff_takes_mean] == p["matcher"]
    merged = weighted_merge([{"a": torch.tensor(1.0), "b": torch.tensor(2.0)}, {"a": torch.tensor(3.0)}], [2.0, 0.5])
    assert float(merged["a"]) == 3.5 and float(merged["b"]) == 4.0


def test_empty_targets_flow_through_matcher_and_criteria():
    """an image without annotations: empty assignment, zero box / mask losses that still depend on the predictions (a graph for autograd),
    label loss over the remaining image's queries, count clamped at 1"""
    g = torch.Generator().manual_seed(3)
    B, Q, L = 2, 6, 5
    pm = torch.zeros(2, L, dtype=torch.bool)
    pm[0, 1] = pm[1, 3] = True
    full = {"labels": torch.tensor([0, 1]), "boxes": torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.3, 0.6, 0.1, 0.3]]), "positive_map": pm,
            "is_thing": torch.tensor([True, True]), "masks": (torch.rand(2, 32, 32, generator=g) > 0.5).float()}
    none = {"labels": torch.zeros(0, dtype=torch.long), "boxes": torch.zeros(0, 4), "positive_map": torch.zeros(0, L, dtype=torch.bool),
            "is_thing": torch.zeros(0, dtype=torch.bool), "masks": torch.zeros(0, 32, 32)}
    logits = torch.randn(B, Q, L, generator=g, requires_grad=True)
    boxes = torch.rand(B, Q, 4, generator=g) * 0.4 + 0.2
    m = HungarianMatcher(MatchWeights(2, 5, 2, 5, 5), num_points=50, class_mode="map")
    idx = m(logits.detach(), boxes, [full, none])
    assert len(idx[0][0]) == 2 and len(idx[1][0]) == 0
    outputs = {"pred_logits": logits, "pred_boxes": boxes, "text_masks": torch.ones(B, L, dtype=torch.long),
               "pred_masks": [torch.randn(1, 2, 1, 8, 8, generator=g), torch.zeros(1, 0, 1, 8, 8)]}
    with torch.enable_grad():                                                  # other test modules switch autograd off process-wide
        losses = DetCriterion(m, ["labelsVL", "boxes", "masks"], num_points=40)(outputs, [full, none], [idx])
        assert all(torch.isfinite(v).all() for v in losses.values()) and float(losses["loss_ce"].detach()) > 0
        losses["loss_ce"].backward()
    assert float(logits.grad[1].abs().sum()) > 0                               # the empty image's queries are all negatives: they get gradient
    both_empty = DetCriterion(m, ["labelsVL", "boxes", "masks"], num_points=40)(
        dict(outputs, pred_masks=[torch.zeros(1, 0, 1, 8, 8)] * 2), [none, none], [m(logits.detach(), boxes, [none, none])])
    assert float(both_empty["loss_bbox"]) == 0 and float(both_empty["loss_mask"]) == 0 and torch.isfinite(both_empty["loss_ce"])


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("tag,n_img", [("md_dyn", 2), ("md_ids", 3)])
def test_maskdino_dn_queries_match_prepare_for_dn(dev, tag, n_img):
    f = Fixture("train_dn", dev)
    targets = f.targets(tag + "_t", n_img)
    dn_num, scale, nq, ncls = [float(x) for x in f.z[tag + "_args"]]
    r = f.rands(tag + "_rand")
    emb = f[tag + "_emb"]
    label_embed = emb if tag == "md_dyn" else (lambda ids: emb[ids])
    ql, qb, mask, md = maskdino_dn_queries(targets, int(dn_num), scale, int(nq), label_embed, f[tag + "_tgt"], f[tag + "_refp"],
                                           {"p": r[0], "new_label": r[1], "box": r[2]}, int(ncls))
    assert [md["pad_size"], md["scalar"]] == [int(x) for x in f.z[tag + "_meta"]]
    assert torch.equal(mask.cpu(), f[tag + "_mask"].cpu()) and close(ql, f[tag + "_label"], 1e-7) and close(qb, f[tag + "_box"], 1e-6)
    assert maskdino_dn_queries(targets, 1, scale, int(nq), label_embed)[0] is None          # fewer requested copies than targets: no group


def test_prepare_targets_and_the_thing_stuff_split():
    from hipie_amd.structures import Boxes, Instances
    z = np.load(os.path.join(GOLD, "train_targets.npz"))
    insts = []
    for i in range(3):
        inst = Instances(tuple(int(v) for v in z["in%d_hw" % i]))
        inst.gt_boxes = Boxes(torch.from_numpy(z["in%d_boxes" % i]))
        inst.gt_classes = torch.from_numpy(z["in%d_classes" % i])
        inst.positive_map = torch.from_numpy(z["in%d_pm" % i])
        inst.is_thing = torch.from_numpy(z["in%d_thing" % i])
        inst.gt_masks = torch.from_numpy(z["in%d_masks" % i])
        insts.append(inst)
    got = prepare_targets(insts)
    for i, t in enumerate(got):
        assert set(t) == {k[5:] for k in z.files if k.startswith("out%d_" % i)}
        for k, v in t.items():
            w = torch.from_numpy(z["out%d_%s" % (i, k)])
            assert v.dtype == w.dtype and (torch.equal(v, w) if v.dtype != torch.float32 else close(v, w, 1e-7)), (i, k)
    fg, bg = split_things_stuff(got)
    for t, f_, b_ in zip(got, fg, bg):
        n_thing = int(t["is_thing"].sum())
        assert len(f_["labels"]) == n_thing and len(b_["labels"]) == len(t["labels"]) - n_thing and bool(f_["is_thing"].all()) and not bool(b_["is_thing"].any())
        assert torch.equal(f_["boxes"], t["boxes"][t["is_thing"]]) and torch.equal(b_["masks"], t["masks"][~t["is_thing"]]) and f_["image_size"] is t["image_size"]
    assert prepare_targets(insts, half=True)[0]["boxes"].dtype == torch.float16


# --------------------------------------------------------------------------------------------- ONE TRAINING STEP against the reference's own
def _train_step_case(dev):
    return train_step_case(dev, _OracleBackend if dev == "cpu" else None)


@pytest.mark.parametrize("dev", DEVICES)
def test_train_step_losses_and_gradients_match_the_reference(dev):
    """ONE TRAINING STEP on the e2e_tiny configuration against the REFERENCE's own (tests/golden/train_step_tiny.npz:
    DDETRSegmUniDN.coco_forward + three DINO criterion calls + the MaskDINO criterion + backward, run on the CPU through
    tests/golden/gen_train_step_golden.py): every entry of the weighted loss dictionary, the total, and the gradient of EVERY trainable
    parameter (407 tensors, large ones on a strided subsample).  cpu: the step's host logic with the oracle's operator kernels plugged in;
    cuda (-m gpu): the product as shipped -- hipie_msda_forward / _backward, the mask contraction and the dynamic mask head on their HIP
    kernels (forward AND backward), the dense layers on the library with torch.autograd."""
    z, meta, model, step, batch, targets = _train_step_case(dev)
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    check_step_against_golden(z, model, step, losses, total, dev, "train step on %s" % dev)


@pytest.mark.gpu
def test_vit_backbone_full_token_grid_fused_attention_against_float64_attention():
    """The fused attention of the global ViT blocks (csrc/attn_train.hip) INSIDE the training step's backbone at the full 64 x 64 token grid --
    1024 x 1024 image, ViT-H width (16 heads x 80), 128 rel-pos columns, two windowed + two global blocks, weights as bench.py draws them
    (the reference-generated fixture of the whole step, train_step_tiny.npz, has 16 x 16 token grids).  Forward features and the gradient of
    every backbone parameter under a fixed cotangent, three ways: global blocks fused, materialised in fp32 (library GEMMs + softmax), and
    materialised in float64 -- the yardstick.  The fused step has to be as close to it as the fp32 one is.  (The whole step's LOSSES are not
    the right observable here: top-k point sampling and the matchers turn 1e-6 feature differences into discrete changes.)"""
    import sys
    import bench
    from hipie_amd.config import HipieConfig, Precision
    from hipie_amd.hipie_img import HIPIE_IMG
    from hipie_amd.training import net
    from hipie_amd.training.step import TrainStep
    dev = torch.device("cuda", 0)
    cfg = HipieConfig(vit_depth=4, vit_window_blocks=[0, 2])
    torch.manual_seed(0)
    model = HIPIE_IMG(cfg, Precision.parity(), device=dev)
    bench.randomize_degenerate_inits(model)
    model.finalize()
    step = TrainStep(model)
    sd, c = step.params(), step.cfg
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    results, calls = {}, []
    fused = net.HipBackend.fused_attention

    def counting(qa, ka, v):
        o = fused(qa, ka, v)
        calls.append((tuple(qa.shape), o is not None))
        return o

    def in_double(qa, ka, v):
        if qa.shape[1] != 4096:
            return None
        return (torch.softmax(qa.double() @ ka.double().transpose(-2, -1), -1) @ v.double()).float()
    cot = None
    for mode, fn in (("fused", counting), ("fp32", lambda qa, ka, v: None), ("float64", in_double)):
        net.HipBackend.fused_attention = staticmethod(fn)
        try:
            model.zero_grad(set_to_none=True)
            with torch.enable_grad():
                feats = net.vit_backbone(x, sd, "detr.detr.backbone.0.backbone.", c, step.be)
                if cot is None:
                    cot = {k: torch.randn(v.shape, generator=g).to(dev) for k, v in feats.items()}
                sum((feats[k] * cot[k]).sum() for k in feats).backward()
            results[mode] = ({k: v.detach().clone() for k, v in feats.items()},
                             {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        finally:
            net.HipBackend.fused_attention = fused
    # the two global blocks ran fused on (16 heads, 4096 tokens, 80 + 64 + 64 columns); the windowed ones (196-token windows) did not
    assert [c_ for c_ in calls if c_[1]] == [((16, 4096, 208), True)] * 2 and len(calls) == 4

    def worst(a, b):
        return max(float((a[k] - b[k]).abs().max() / (b[k].abs().max() + 1e-30)) for k in b)
    (ff, gf), (f32, g32), (fd, gd) = results["fused"], results["fp32"], results["float64"]
    assert len(gd) > 40 and gf.keys() == gd.keys()
    ef, e32, egf, eg32 = worst(ff, fd), worst(f32, fd), worst(gf, gd), worst(g32, gd)
    print("ViT at the full token grid, against float64 attention: features fused %.1e / fp32 %.1e; worst of %d parameter gradients fused %.1e / fp32 %.1e"
          % (ef, e32, len(gd), egf, eg32))
    assert ef < max(2 * e32, 3e-6) and egf < max(4 * eg32, 1e-5), (ef, e32, egf, eg32)        # measured 9.0e-7 / 1.0e-6 and 2.5e-6 / 1.0e-6


def test_train_step_has_no_host_path_by_default():
    """the default backend is the HIP library: on host tensors the step fails loudly instead of computing something else"""
    z, meta, model, step, batch, targets = _train_step_case("cpu")
    from hipie_amd.training import net
    step.be = net.HipBackend
    with pytest.raises(RuntimeError), torch.enable_grad():
        step.loss_dict(batch, targets)


def test_abs_pos_resize_as_matrix_products_is_the_library_bicubic():
    """training/net.get_abs_pos applies the bicubic resize of the position table (backbone/utils.py:128-157) as two matrix products with the
    library's own per-axis weights: same values and same gradient as F.interpolate(mode="bicubic", align_corners=False), in double"""
    import torch.nn.functional as F
    from hipie_amd.training import net
    g = torch.Generator().manual_seed(3)
    for size, (h, w) in ((14, (64, 64)), (14, (16, 24)), (32, (20, 7)), (8, (8, 8))):
        p = torch.randn(1, 1 + size * size, 24, generator=g, dtype=torch.float64, requires_grad=True)
        with torch.enable_grad():                      # other test modules switch autograd off at import
            got = net.get_abs_pos(p, (h, w))
            a = p[:, 1:].reshape(1, size, size, -1)
            ref = F.interpolate(a.permute(0, 3, 1, 2), size=(h, w), mode="bicubic", align_corners=False).permute(0, 2, 3, 1) if (size, size) != (h, w) else a
            go = torch.randn(ref.shape, generator=g, dtype=torch.float64)
            g1, = torch.autograd.grad(got, p, go, retain_graph=True)
            g2, = torch.autograd.grad(ref, p, go)
        assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-13 and float((g1 - g2).abs().max()) < 1e-12
