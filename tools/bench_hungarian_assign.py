#!/usr/bin/env python3
"""A one-to-one Hungarian matcher call with the assignment on the device (net.HipBackendAssign: functions.hungarian_match on
csrc/hungarian_cost.hip + csrc/hungarian_assign.hip, device pairs, the status words deferred) against the same call of net.HipBackendHungarian
(the costs on the kernel, ONE device -> host copy, scipy on host slices).  One process, the two sides alternated call by call on the same
inputs and the same points, the targets packed once outside the call; prints the median and minimum wall time of a synchronised call, the
device launches per call (kernels, copies and fills, counted by torch.profiler), the host waits per call (the synchronising calls torch's
sync debug mode reports) and whether the two sides return the same pairs.  The hard conditions of the new path -- no host wait and at most
3 + 3 x (images with masks) launches per call -- are asserted.

Then the assignment kernel alone, by HIP events around ops.hungarian_assign (median and minimum of `reps` launches), beside scipy's wall time
on the same blocks on the host: on the seeded costs of the cases above, and on the adversarial matrix C[q, t] = -(q + t) t at 900 x 100 and
4096 x 256, where the solver takes close to min(Q, T) (min(Q, T) + 1) / 2 inner iterations (4951 and 32641) -- the longest searches the
bounded loops see.
    python tools/bench_hungarian_assign.py [reps]
B = 2 images, L = 256 tokens, Q = 900 queries, T = 7 / 20 / 100 targets per image (boxes and logits as in tests/_ota_cases.py), class + box
costs with the stuff mean; with masks: + the mask costs at P = 12544 points, predicted masks (Q, 64, 64), 256 x 256 targets."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from _assign_cases import adversarial, pack_blocks, scipy_pairs  # noqa: E402
from _ota_cases import ota_case  # noqa: E402
from bench_hungarian_cost import host_waits, launches, same_pairs, timed  # noqa: E402
from hipie_amd import ops  # noqa: E402
from hipie_amd.training import functions, net  # noqa: E402
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights  # noqa: E402

DEV = torch.device("cuda", 0)
P = 112 * 112


def kernel_ms(args, reps):
    """HIP-event ms of ops.hungarian_assign alone: (median, min) of `reps` launches after three untimed ones"""
    ws = torch.empty(ops.hungarian_assign_ws_bytes(args[4], args[3]), dtype=torch.uint8, device=DEV)
    ts = []
    for it in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = ops.hungarian_assign(*args, ws=ws)
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), out


def scipy_ms(blocks, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for C in blocks:
            scipy_pairs(C)
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    print("median of %d calls, the two sides alternated; B = 2, Q = 900, L = 256, weights (2, 5, 2, 5, 5), stuff mean on" % reps)
    w = MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0)
    g = torch.Generator().manual_seed(5)
    points = torch.rand(2, 1, P, 2, generator=g).to(DEV)

    class Points:                                            # the same points on both sides, no launch of their own
        def __init__(self):
            self.i = 0

        def __call__(self, shape, device):
            self.i += 1
            return points[(self.i - 1) % 2]
    Q = 900
    seeded = []
    for with_masks in (False, True):
        for T in (7, 20, 100):
            logits, boxes, targets = ota_case(2, Q, T, 256, False, 0)
            logits, boxes = logits.to(DEV), boxes.to(DEV)
            targets = [dict(t, is_thing=torch.arange(len(t["boxes"])) % 3 != 1, masks=(torch.rand(len(t["boxes"]), 256, 256, generator=g) < 0.3).float())
                       for t in targets]
            targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
            pred = [3.0 * torch.randn(Q, 64, 64, generator=g).to(DEV) for _ in range(2)] if with_masks else None
            host_side = HungarianMatcher(w, num_points=P, draw=Points(), class_mode="map", ops=net.HipBackendHungarian)
            dev_side = HungarianMatcher(w, num_points=P, draw=Points(), class_mode="map", ops=net.HipBackendAssign, defer_status=True)
            packed = dev_side.pack(targets, DEV)
            sides = {"scipy": lambda: host_side(logits, boxes, targets, masks=pred, packed=packed),
                     "device": lambda: dev_side(logits, boxes, targets, masks=pred, packed=packed)}
            res = {k: [] for k in sides}
            for it in range(reps + 3):                       # three untimed rounds: allocator pools, kernel load
                for k, fn in sides.items():
                    t = timed(fn)
                    if it >= 3:
                        res[k].append(t)
            dev_side.check()
            med = {k: statistics.median(v) for k, v in res.items()}
            lo = {k: min(v) for k, v in res.items()}
            n = {k: launches(fn) for k, fn in sides.items()}
            hw = {k: host_waits(fn) for k, fn in sides.items()}
            a, b = sides["scipy"](), sides["device"]()
            same = same_pairs(a, [(q.cpu(), t.cpu()) for q, t in b])
            dev_side.check()
            print("forward masks=%d Q=%-4d T=%-3d (%d + %d targets) | scipy on the host %7.3f ms (min %7.3f) %2d launches %d host waits | on the device %7.3f ms "
                  "(min %7.3f) %2d launches %d host waits | x%.2f | the same pairs on both sides: %s"
                  % (with_masks, Q, T, packed.counts[0], packed.counts[1], med["scipy"], lo["scipy"], n["scipy"], hw["scipy"], med["device"], lo["device"],
                     n["device"], hw["device"], med["scipy"] / med["device"], same))
            budget = 3 + (3 * 2 if with_masks else 0)        # the cost kernel's two launches, the assignment, three per image with masks
            assert hw["device"] == 0 and n["device"] <= budget and same, ("the hard conditions of the device path", hw["device"], n["device"], budget, same)
            if not with_masks:
                Cs = functions.hungarian_costs(logits, boxes, packed, w)
                seeded.append(("seeded costs T=%d" % T, [np.array(C) for C in Cs]))
    print("the assignment kernel alone (HIP events around ops.hungarian_assign, %d launches) | scipy on the same blocks on the host (wall)" % reps)
    for name, blocks in seeded + [("adversarial 900 x 100", [adversarial(900, 100)]), ("adversarial 4096 x 256", [adversarial(4096, 256)])]:
        args = pack_blocks(blocks, DEV)
        args = (args[0], args[1], args[2], args[3], blocks[0].shape[0], args[4])
        med, lo, (pq, pt, st) = kernel_ms(args, reps)
        ok = st.tolist() == [0] * len(blocks) and all(
            np.array_equal(pq[b, :len(i)].cpu().numpy(), i) and np.array_equal(pt[b, :len(i)].cpu().numpy(), j) for b, (i, j) in enumerate(map(scipy_pairs, blocks)))
        print("kernel %-24s B=%d | %9.3f ms (min %9.3f) | scipy %8.3f ms | scipy's pairs: %s" % (name, len(blocks), med, lo, scipy_ms(blocks, max(3, reps // 4)), ok))


if __name__ == "__main__":
    main()
