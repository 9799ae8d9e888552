#!/usr/bin/env python3
"""forward + backward of the training step's big linears, the split nodes (functions.split_linear / split_mlp: three fp16 products, fp32
class) against the half-precision nodes of net.half_policy (functions.half_linear / half_mlp: ONE fp16 product, 2^-11 per operand), per
shape family: the four ViT-H linears and the MLP pair at 8192 token rows (2 images of 1024^2), the encoder FFN (256 <-> 2048, ReLU) at
43 520 tokens.  Both sides alternate in ONE process (the sampling of tools/bench_grad_scale.py: a timed sample is a block of 5 queued calls
of one side between two events).  Per family: median and minimum in microseconds per call, the split node's own run-to-run spread
(max - min of its samples over its median) from the same run, the ratio of the medians, device launches and peak memory of one call, and
the verdict of the project's keep-the-faster-form rule: the half node is kept for a family only if its median is below the split node's by
more than that spread (functions.half_linear_ok declines a family that is not).
    python tools/bench_half_linears.py [repeats] [vit_rows] [ffn_rows]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_grad_scale import LINEARS, launches, one_call, peak, timed  # noqa: E402
from hipie_amd import ops  # noqa: E402
from hipie_amd.training import functions  # noqa: E402


def compare(name, shape, split, half, leaves, dy, reps):
    for _ in range(3):
        one_call(split, leaves, dy)
        one_call(half, leaves, dy)
    ts, th = [], []
    for _ in range(reps):
        ts.append(timed(split, leaves, dy))
        th.append(timed(half, leaves, dy))
    ms, mh = statistics.median(ts), statistics.median(th)
    spread = (max(ts) - min(ts)) / ms
    print("%-18s %-14s | %9.1f %9.1f %6.1f%% | %9.1f %9.1f | %6.3f | %-6s | %4d %4d | %8.1f %8.1f" % (
        name, shape, ms, min(ts), 100 * spread, mh, min(th), mh / ms, "keep" if mh < ms * (1 - spread) else "DECLINE", launches(split, leaves, dy),
        launches(half, leaves, dy), peak(split, leaves, dy), peak(half, leaves, dy)))
    return ms, mh


def mlp_leaves(M, C, H, dev):
    x = torch.randn(M, C, device=dev).requires_grad_(True)
    w1, b1 = (torch.randn(H, C, device=dev) * C ** -0.5).requires_grad_(True), (torch.randn(H, device=dev) * 0.1).requires_grad_(True)
    w2, b2 = (torch.randn(C, H, device=dev) * H ** -0.5).requires_grad_(True), (torch.randn(C, device=dev) * 0.1).requires_grad_(True)
    return [x, w1, b1, w2, b2], torch.randn(M, C, device=dev) * 1e-3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    Mf = int(sys.argv[3]) if len(sys.argv) > 3 else 43520
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    print("linears forward + backward, split node against half node, %d alternated samples of 5 queued calls per side; us per call, MiB" % reps)
    print("%-18s %-14s | %9s %9s %7s | %9s %9s | %6s | %-6s | %4s %4s | %8s %8s" % ("node", "(N, K)", "split med", "split min", "spread", "half med", "half min",
                                                                                 "h/s", "rule", "s ln", "h ln", "s peak", "h peak"))
    tot_s = tot_h = 0.0
    for name, N, K in LINEARS:
        x = torch.randn(M, K, device=dev).requires_grad_(True)
        w = (torch.randn(N, K, device=dev) * K ** -0.5).requires_grad_(True)
        b = (torch.randn(N, device=dev) * 0.1).requires_grad_(True)
        dy = torch.randn(M, N, device=dev) * 1e-3
        ms, mh = compare("linear %s M=%d" % (name, M), "(%d, %d)" % (N, K), lambda x, w, b: functions.split_linear(x, w, b, w, "w"),
                         lambda x, w, b: functions.half_linear(x, w, b, w, "w"), [x, w, b], dy, reps)
        tot_s += ms
        tot_h += mh
        del x, w, b, dy
    print("the 4 linears of a ViT-H block, medians added: split %.0f us, half %.0f us (%.3f)" % (tot_s, tot_h, tot_h / tot_s))
    leaves, dy = mlp_leaves(M, 1280, 5120, dev)
    compare("mlp gelu M=%d" % M, "(5120, 1280)", lambda *a: functions.split_mlp(*a, ops.ACT_GELU), lambda *a: functions.half_mlp(*a, ops.ACT_GELU), leaves, dy, reps)
    del leaves, dy
    leaves, dy = mlp_leaves(Mf, 256, 2048, dev)
    compare("ffn relu M=%d" % Mf, "(2048, 256)", lambda *a: functions.split_mlp(*a, ops.ACT_RELU), lambda *a: functions.half_mlp(*a, ops.ACT_RELU), leaves, dy, reps)
    print("half node calls: %s" % dict(functions.HALF_NODE_CALLS))


if __name__ == "__main__":
    main()
