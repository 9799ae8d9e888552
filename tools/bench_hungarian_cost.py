#!/usr/bin/env python3
"""A one-to-one Hungarian matcher call, in both formulations of the same tree: the torch loop of HungarianMatcher.forward (matcher.cost_matrix
per image, `C.cpu()` and scipy per image; with masks its mask costs on hipie_mask_match_cost, as net.HipBackendMatching runs them) and the
batched path of net.HipBackendHungarian (functions.hungarian_costs on csrc/hungarian_cost.hip: one or two launches for the batch on top of
the three mask-cost launches per image, ONE device -> host copy, scipy on host slices; the targets packed once outside the call, as
TrainStep and the criteria pack them).  One process, the two sides alternated call by call on the same inputs and the same points; prints
the median and minimum wall time of a synchronised call (the call ends on the host, in scipy), the device launches per call (kernels,
copies and fills, counted by torch.profiler), the host waits per call (the synchronising calls torch's sync debug mode reports) and whether
the two sides return the same pairs.  The hard conditions of the batched path -- at most one host wait and at most 2 + 3 x (images with
masks) launches per call -- are asserted.
    python tools/bench_hungarian_cost.py [reps]
B = 2 images, L = 256 tokens, Q = 100 / 300 / 1000 queries, T = 7 / 20 / 100 targets per image (boxes and logits as in tests/_ota_cases.py),
class + box costs with the stuff mean; with masks: + the mask costs at P = 12544 points, predicted masks (Q, 64, 64), 256 x 256 targets."""
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from _ota_cases import ota_case  # noqa: E402
from hipie_amd.training import net  # noqa: E402
from hipie_amd.training.matcher import HungarianMatcher, MatchWeights  # noqa: E402

DEV = torch.device("cuda", 0)
P = 112 * 112


def timed(fn):
    """wall ms of the synchronised call"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def launches(fn):
    """device activities (kernels, copies, fills) of one call"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def host_waits(fn):
    """synchronising calls of one call, as torch's sync debug mode reports them (one warning each)"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for w in seen if "synchroniz" in str(w.message).lower())


def same_pairs(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    print("median of %d calls, the two sides alternated; B = 2, L = 256, weights (2, 5, 2, 5, 5), stuff mean on" % reps)
    w = MatchWeights(2.0, 5.0, 2.0, 5.0, 5.0)
    g = torch.Generator().manual_seed(5)
    points = torch.rand(2, 1, P, 2, generator=g).to(DEV)

    class Points:                                            # the same points on both sides, no launch of their own
        def __init__(self):
            self.i = 0

        def __call__(self, shape, device):
            self.i += 1
            return points[(self.i - 1) % 2]
    for with_masks in (False, True):
        for Q in (100, 300, 1000):
            for T in (7, 20, 100):
                logits, boxes, targets = ota_case(2, Q, T, 256, False, 0)
                logits, boxes = logits.to(DEV), boxes.to(DEV)
                targets = [dict(t, is_thing=torch.arange(len(t["boxes"])) % 3 != 1, masks=(torch.rand(len(t["boxes"]), 256, 256, generator=g) < 0.3).float())
                           for t in targets]
                targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
                pred = [3.0 * torch.randn(Q, 64, 64, generator=g).to(DEV) for _ in range(2)] if with_masks else None
                torch_side = HungarianMatcher(w, num_points=P, draw=Points(), class_mode="map", ops=net.HipBackendMatching)
                hip_side = HungarianMatcher(w, num_points=P, draw=Points(), class_mode="map", ops=net.HipBackendHungarian)
                packed = hip_side.pack(targets, DEV)
                sides = {"torch": lambda: torch_side(logits, boxes, targets, masks=pred), "hip": lambda: hip_side(logits, boxes, targets, masks=pred, packed=packed)}
                res = {k: [] for k in sides}
                for it in range(reps + 3):                   # three untimed rounds: allocator pools, kernel load
                    for k, fn in sides.items():
                        t = timed(fn)
                        if it >= 3:
                            res[k].append(t)
                med = {k: statistics.median(v) for k, v in res.items()}
                lo = {k: min(v) for k, v in res.items()}
                n = {k: launches(fn) for k, fn in sides.items()}
                hw = {k: host_waits(fn) for k, fn in sides.items()}
                same = same_pairs(sides["torch"](), sides["hip"]())
                print("forward masks=%d Q=%-4d T=%-3d (%d + %d targets) | torch %8.3f ms (min %8.3f) %4d launches %3d host waits | hip %7.3f ms (min %7.3f) "
                      "%2d launches %d host waits | x%.1f | the same pairs on both sides: %s"
                      % (with_masks, Q, T, packed.counts[0], packed.counts[1], med["torch"], lo["torch"], n["torch"], hw["torch"], med["hip"], lo["hip"], n["hip"],
                         hw["hip"], med["torch"] / med["hip"], same))
                budget = 2 + 1 + (3 * 2 if with_masks else 0)          # the kernel's two launches, the copy to the host, three per image with masks
                assert hw["hip"] <= 1 and n["hip"] <= budget, ("the hard conditions of the batched path", hw["hip"], n["hip"], budget)


if __name__ == "__main__":
    main()
