#!/usr/bin/env python3
"""A `loss_boxes` call (forward + backward) of the two criteria and a positive one-hot with the pair kernels (net.HipBackendPairLosses:
functions.pair_box_loss / positive_onehot on csrc/pair_loss.hip) against the same calls of the torch path (ops = net.HipBackendAssign, which has
neither op).  One process, the two sides alternated call by call on the same inputs, the targets packed outside the call; prints the median and
minimum wall time of a synchronised call, the device launches per call (kernels, copies and fills, counted by torch.profiler) and the host
waits per call (the synchronising calls torch's sync debug mode reports).  The hard condition of the new path -- no host wait -- is asserted.
    python tools/bench_pair_loss.py [reps]
B = 2 images, Q = 900 queries (the predictions a slice [:, 100:] of a (2, 1000, .) tensor), K = 14 / 200 / 2000 matched pairs over the two images,
20 targets per image (a third of them stuff), L = 256 tokens; mode 0 = DetCriterion.loss_boxes with pred_boxious (panoptic_box_loss, ota),
mode 1 = MaskCriterion.loss_boxes."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_hungarian_cost import host_waits, launches, timed  # noqa: E402
from hipie_amd.training import net  # noqa: E402
from hipie_amd.training.criterion import DetCriterion, MaskCriterion  # noqa: E402

DEV = torch.device("cuda", 0)
B, Q, PAD, T, L = 2, 900, 100, 20, 256


def case(K, seed=0):
    g = torch.Generator().manual_seed(seed + K)
    big = torch.cat((torch.rand(B, PAD + Q, 2, generator=g), 0.02 + 0.4 * torch.rand(B, PAD + Q, 2, generator=g)), 2).to(DEV).requires_grad_()
    iou = torch.randn(B, PAD + Q, 1, generator=g).to(DEV).requires_grad_()
    logits = torch.randn(B, Q, L, generator=g).to(DEV)
    targets, pairs = [], []
    for b in range(B):
        k = K // B + (b < K % B)
        pm = torch.zeros(T, L, dtype=torch.bool)
        pm[torch.arange(T), torch.randint(0, L, (T,), generator=g)] = True
        targets.append({"boxes": torch.cat((0.2 + 0.6 * torch.rand(T, 2, generator=g), 0.05 + 0.3 * torch.rand(T, 2, generator=g)), 1).to(DEV),
                        "is_thing": (torch.arange(T) % 3 != 1).to(DEV), "positive_map": pm.to(DEV), "labels": torch.zeros(T, dtype=torch.long, device=DEV)})
        # one-to-many pairs as SimOTA leaves them: every query at most once, a target many times (K = 2000 is more than the 2 x 900 queries: there
        # the queries repeat, and the backward's additions to one element with them)
        q = torch.randperm(Q, generator=g)[:k] if k <= Q else torch.randint(0, Q, (k,), generator=g)
        pairs.append((q.to(DEV), torch.randint(0, T, (k,), generator=g).to(DEV)))
    return big, iou, logits, targets, pairs


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    print("median of %d calls, the two sides alternated; B = %d, Q = %d, T = %d per image, L = %d" % (reps, B, Q, T, L))
    up = torch.ones((), device=DEV)
    for mode in (0, 1):
        for K in (14, 200, 2000):
            big, iou, logits, targets, pairs = case(K)
            out = {"pred_boxes": big[:, PAD:], "pred_boxious": iou[:, PAD:]}
            sides, hot, crits = {}, {}, []
            for name, be in (("torch", net.HipBackendAssign), ("kernels", net.HipBackendPairLosses)):
                crit = DetCriterion(None, ["boxes"], ota=True, ops=be) if mode == 0 else MaskCriterion(1, None, ["boxes"], ops=be)

                def call(crit=crit):
                    big.grad = iou.grad = None
                    res = crit.loss_boxes(out, targets, pairs, float(K))
                    sum(res.values()).backward(up)
                    return res
                crits.append(crit)
                sides[name] = call
                hot[name] = lambda crit=crit: crit._onehot(logits, targets, pairs)
            rows = []
            for what, fns in (("loss_boxes fwd+bwd", sides), ("positive one-hot", hot)):
                if what == "positive one-hot" and mode == 1:
                    continue                                 # the same call in both criteria
                res = {k: [] for k in fns}
                for it in range(reps + 3):                   # three untimed rounds: allocator pools, kernel load, the packing of the targets
                    for k, fn in fns.items():
                        t = timed(fn)
                        if it >= 3:
                            res[k].append(t)
                med = {k: statistics.median(v) for k, v in res.items()}
                lo = {k: min(v) for k, v in res.items()}
                n = {k: launches(fn) for k, fn in fns.items()}
                hw = {k: host_waits(fn) for k, fn in fns.items()}
                rows.append((what, med, lo, n, hw))
                assert hw["kernels"] == 0, ("the hard condition of the new path: no host wait", what, hw)
            a, b = sides["torch"](), sides["kernels"]()
            worst = max(abs(float(a[k].detach()) - float(b[k].detach())) / max(abs(float(a[k].detach())), 1e-30) for k in a)
            for what, med, lo, n, hw in rows:
                print("mode %d K=%-4d %-18s | torch %7.3f ms (min %7.3f) %3d launches %d host waits | kernels %7.3f ms (min %7.3f) %3d launches %d host waits | "
                      "x%.2f" % (mode, K, what, med["torch"], lo["torch"], n["torch"], hw["torch"], med["kernels"], lo["kernels"], n["kernels"], hw["kernels"],
                                 med["torch"] / med["kernels"]))
            print("mode %d K=%-4d the two sides' losses agree to %.1e (relative)" % (mode, K, worst))
            for crit in crits:                               # the status words of the calls above, one read
                crit.check()


if __name__ == "__main__":
    main()
