#!/usr/bin/env python3
"""The one-to-many SimOTA matching of the foreground queries, per call, in both formulations of the same tree: the torch path of
HungarianMatcher.forward_ota (matcher.ota_cost + dynamic_k_assign, per image and target) and the kernels of csrc/ota_match.hip
(functions.ota_match, what net.HipBackendMatching calls; the targets packed once outside the call, as TrainStep packs them once per step).
One process, the two sides alternated call by call on the same inputs; prints the median and minimum time between two device events around
a call and its wall time, the device launches per call (kernels, copies and fills, counted by torch.profiler), the host waits per call
(the synchronising calls torch's sync debug mode reports) and whether the two sides return the same pairs.
    python tools/bench_ota_match.py [reps]
B = 2 images, Q = 900 queries, L = 256 tokens, T = 7 / 20 / 100 targets per image (boxes and logits as in tests/_ota_cases.py)."""
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from _ota_cases import ota_case, same_best, same_pairs  # noqa: E402
from hipie_amd.training import functions  # noqa: E402
from hipie_amd.training.matcher import HungarianMatcher  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn):
    """(ms between two events around the call, wall ms of the synchronised call)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), 1e3 * (time.perf_counter() - t0)


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


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    print("median of %d calls, the two sides alternated; B = 2, Q = 900, L = 256" % reps)
    plain = HungarianMatcher(class_mode="map")
    for T in (7, 20, 100):
        logits, boxes, targets = ota_case(2, 900, T, 256, False, 0)
        logits, boxes = logits.to(DEV), boxes.to(DEV)
        targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
        packed = functions.pack_ota_targets(targets, DEV)
        sides = {"torch": lambda: plain.forward_ota(logits, boxes, targets), "hip": lambda: functions.ota_match(logits, boxes, packed)}
        res = {k: [] for k in sides}
        for it in range(reps + 3):                           # three untimed rounds: allocator pools, kernel load
            for k, fn in sides.items():
                t = timed(fn)
                if it >= 3:
                    res[k].append(t)
        ev = {k: statistics.median(t[0] for t in v) for k, v in res.items()}
        lo = {k: min(t[0] for t in v) for k, v in res.items()}
        wall = {k: statistics.median(t[1] for t in v) for k, v in res.items()}
        n = {k: launches(fn) for k, fn in sides.items()}
        w = {k: host_waits(fn) for k, fn in sides.items()}
        a, b = sides["torch"](), sides["hip"]()
        same = same_pairs(a[0], b[0]) and same_best(a[1], b[1])
        print("forward_ota T=%-3d (%d + %d targets) | torch %8.3f ms (min %8.3f, wall %8.3f) %4d launches %3d host waits | hip %7.3f ms (min %7.3f, "
              "wall %7.3f) %2d launches %d host waits | x%.1f | %d + %d pairs, the same on both sides: %s"
              % (T, packed.counts[0], packed.counts[1], ev["torch"], lo["torch"], wall["torch"], n["torch"], w["torch"], ev["hip"], lo["hip"], wall["hip"],
                 n["hip"], w["hip"], ev["torch"] / ev["hip"], len(b[0][0][0]), len(b[0][1][0]), same))


if __name__ == "__main__":
    main()
