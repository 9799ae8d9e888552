#!/usr/bin/env python3
"""The two no_grad places of the criteria and matchers that sample a mask at points, per call, in both formulations: the torch code of
criterion.uncertain_points / matcher.mask_costs and the kernels of csrc/point_select.hip (functions.uncertain_points / mask_match_costs,
what net.HipBackendCriteria calls).  One process, the two sides alternated call by call on the same inputs; prints the median and minimum
wall time of a synchronised call, the device launches per call (kernels, copies and fills, counted by the profiler) and how far the two
results are apart.
    python tools/bench_criteria_points.py [reps]
Selection: N = 14 and 200 instances (2 images x 8 targets less two; 200 = the de-noising part), 256 x 256 logits, P = 12544 (C = 37632
candidates, k = 9408).  Costs: Q = 300 and 900 queries, T = 8 and 100 targets, 256 x 256 predictions, 1024 x 1024 hard targets, P = 12544."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hipie_amd.training import criterion, functions, matcher  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def launches(fn):
    """device activities (kernels, copies, fills) of one call"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def compare(tag, sides, reps, apart):
    res = {k: [] for k in sides}
    for it in range(reps + 3):                               # three untimed rounds: allocator pools, kernel load
        for k, fn in sides.items():
            t = timed(fn)
            if it >= 3:
                res[k].append(t)
    ms = {k: 1e3 * statistics.median(v) for k, v in res.items()}
    lo = {k: 1e3 * min(v) for k, v in res.items()}
    n = {k: launches(fn) for k, fn in sides.items()}
    print("%-40s torch %8.3f ms (min %8.3f) %3d launches | hip %8.3f ms (min %8.3f) %3d launches | x%.2f | %s"
          % (tag, ms["torch"], lo["torch"], n["torch"], ms["hip"], lo["hip"], n["hip"], ms["torch"] / ms["hip"], apart(sides["torch"](), sides["hip"]())))


def selection_case(N, size=256, P=12544, oversample=3.0, importance=0.75):
    g = torch.Generator().manual_seed(N)
    src = (torch.randn(N, 1, size, size, generator=g) * 3).to(DEV)
    draw_g = torch.Generator(device=DEV)
    draw = lambda shape, device: torch.rand(tuple(shape), device=device, generator=draw_g)          # noqa: E731

    def side(select):
        def run():
            draw_g.manual_seed(7)                            # the same candidates and rest on both sides
            with torch.no_grad():
                return criterion.uncertain_points(src, P, oversample, importance, draw, select)
        return run

    def apart(a, b):
        k = int(importance * P)
        rows = lambda t: t[:, :k].contiguous().view(torch.int64)[:, :, 0].sort(1).values          # noqa: E731  (x, y) as one 64-bit word
        same = (rows(a) == rows(b)).all(1)
        return "chosen sets equal in %d of %d instances, rest equal %s" % (int(same.sum()), N, bool(torch.equal(a[:, k:], b[:, k:])))
    return {"torch": side(None), "hip": side(functions.uncertain_points)}, apart


def cost_case(Q, T, size_p=256, size_t=1024, P=12544):
    g = torch.Generator().manual_seed(Q + T)
    pred = (torch.randn(Q, size_p, size_p, generator=g) * 3).to(DEV)
    tgt = (torch.rand(T, size_t, size_t, generator=g) < 0.3).float().to(DEV)
    coords = torch.rand(P, 2, generator=g).to(DEV)

    def apart(a, b):
        return "ce apart %.1e, dice apart %.1e (of the largest)" % tuple(float((x - y).abs().max() / x.abs().max()) for x, y in zip(a, b))
    return {"torch": lambda: matcher.mask_costs(pred, tgt, coords), "hip": lambda: functions.mask_match_costs(pred, tgt, coords)}, apart


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    print("median of %d synchronised calls, the two sides alternated" % reps)
    for N in (14, 200):
        sides, apart = selection_case(N)
        compare("uncertain_points N=%d 256^2 P=12544" % N, sides, reps, apart)
        del sides, apart
        torch.cuda.empty_cache()
    for Q in (300, 900):
        for T in (8, 100):
            sides, apart = cost_case(Q, T)
            with torch.no_grad():
                compare("mask_costs Q=%d T=%d 256^2 / 1024^2" % (Q, T), sides, reps, apart)
            del sides, apart
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
