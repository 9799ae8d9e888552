#!/usr/bin/env python3
"""time of ONE ops.act_backward call (du, a recomputed, the bias gradient) against the library chain it replaces in the
backward of an MLP -- aten.gelu_backward | threshold_backward, .sum(0) for the bias gradient, and F.gelu | F.relu for the recomputation of
a -- at the two shapes of the training step: 8192 x 5120 (ViT-H MLP, GELU) and 43520 x 1024 (encoder FFN, ReLU).
    python tools/bench_act_bwd.py [calls] [repetitions]
torch.cuda.Event around `calls` calls (default 200) after 20 warm-up calls, `repetitions` (default 5) times, the two forms alternated;
prints min / median / max in ms and the achieved bytes/s of the hand-written call (4 tensors of rows x N x 4 bytes: u, g, du, a)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hipie_amd import ops  # noqa: E402


def timed(fn, calls):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)
    for rows, N, act in ((8192, 5120, ops.ACT_GELU), (43520, 1024, ops.ACT_RELU)):
        gen = torch.Generator(device=dev).manual_seed(rows + N)
        u = torch.randn(rows, N, device=dev, generator=gen) * 1.5
        g0 = torch.randn(rows, N, device=dev, generator=gen)
        buf = torch.empty_like(g0)                  # du goes into a buffer of the caller, as in MlpFunction (there it is g itself: the same traffic)

        def hand():
            return ops.act_backward(u, g0, act, want_a=True, want_bias_grad=True, out=buf)

        def chain():
            if act == ops.ACT_GELU:
                du = torch.ops.aten.gelu_backward(g0, u)
                return du, F.gelu(u), du.sum(0)
            du = torch.ops.aten.threshold_backward(g0, u, 0.0)
            return du, F.relu(u), du.sum(0)
        got, want = hand(), chain()
        agree = ["%.2e" % float((x.double() - y.double()).abs().max() / y.double().abs().max()) for x, y in zip(got, want)]
        th, tc = [], []
        for _ in range(reps):
            th.append(timed(hand, calls))
            tc.append(timed(chain, calls))
        nbytes = 4 * rows * N * 4

        def fmt(t):
            return "%.4f / %.4f / %.4f" % (min(t), statistics.median(t), max(t))
        print("act_backward %s %d x %d: hand-written %s ms, torch chain %s ms, ratio %.2f x, achieved %.2f TB/s (%d MB per call; last-level cache 256 MB); "
              "agreement du / a / dbias %s" % ("gelu" if act == ops.ACT_GELU else "relu", rows, N, fmt(th), fmt(tc), statistics.median(tc) / statistics.median(th),
                                              nbytes / statistics.median(th) / 1e9, nbytes // 2 ** 20, " / ".join(agree)), flush=True)
        fw = [timed(lambda: ops.act_forward(u, act), calls) for _ in range(reps)]
        fl = [timed(lambda: (F.gelu if act == ops.ACT_GELU else F.relu)(u), calls) for _ in range(reps)]
        print("act_forward  %s %d x %d: hand-written %s ms, library %s ms, achieved %.2f TB/s" % (
            "gelu" if act == ops.ACT_GELU else "relu", rows, N, fmt(fw), fmt(fl), 2 * rows * N * 4 / statistics.median(fw) / 1e9), flush=True)


if __name__ == "__main__":
    main()
