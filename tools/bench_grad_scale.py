#!/usr/bin/env python3
"""forward + backward of the training step's split linears at the ViT-H shapes (M = 8192 token rows: 2 images of 1024^2; qkv, proj, fc1,
fc2), today's nodes against the scaled-gradient nodes of the opt-in group "scaled_grads": functions.SplitLinearFunction against
ScaledSplitLinearFunction per linear, and functions.MlpFunction against ScaledMlpFunction for fc1 -> GELU -> fc2.  The scaled backward adds
a maximum pass over dy and one pack pass (two reads of dy, one extra write: the HL8 rows of s dy) and drops three readers of dy (the GEMM's
in-kernel split, hipie_to_hl8_t, dy.sum(0)).  Both sides alternate in ONE process; a timed sample is a block of 5 queued calls of one side
between two events; per shape: median and minimum of the samples in microseconds per call, the ratio of the medians, the device launches of
one call and the peak memory of a call above its inputs.
    python tools/bench_grad_scale.py [rows] [repeats]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hipie_amd import ops  # noqa: E402
from hipie_amd.training import functions  # noqa: E402

# (name, N, K) of y = x (M, K) . W (N, K)^T
LINEARS = [("qkv", 3840, 1280), ("proj", 1280, 1280), ("fc1", 5120, 1280), ("fc2", 1280, 5120)]
BLOCK = 5           # queued calls per timed sample


def one_call(fn, leaves, dy):
    for t in leaves:
        t.grad = None
    fn(*leaves).backward(dy)


def timed(fn, leaves, dy):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(BLOCK):
        one_call(fn, leaves, dy)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / BLOCK


def peak(fn, leaves, dy):
    one_call(fn, leaves, dy)
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(*leaves).backward(dy)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def launches(fn, leaves, dy):
    from torch.profiler import ProfilerActivity, profile
    one_call(fn, leaves, dy)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        one_call(fn, leaves, dy)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def compare(name, shape, raw, scaled, leaves, dy, reps):
    for _ in range(3):
        one_call(raw, leaves, dy)
        one_call(scaled, leaves, dy)
    tr, ts = [], []
    for _ in range(reps):
        tr.append(timed(raw, leaves, dy))
        ts.append(timed(scaled, leaves, dy))
    mr, ms = statistics.median(tr), statistics.median(ts)
    print("%-16s %-18s | %9.1f %9.1f | %9.1f %9.1f | %6.3f | %6d %6d | %9.1f %9.1f" % (
        name, shape, mr, min(tr), ms, min(ts), ms / mr, launches(raw, leaves, dy), launches(scaled, leaves, dy), peak(raw, leaves, dy), peak(scaled, leaves, dy)))
    return mr, ms


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    print("split linears forward + backward, M = %d rows, fp32, %d alternated samples of %d queued calls per side; us per call, MiB" % (M, reps, BLOCK))
    print("%-16s %-18s | %9s %9s | %9s %9s | %6s | %6s %6s | %9s %9s" % ("node", "(N, K)", "raw med", "raw min", "scl med", "scl min", "scl/raw", "raw ln",
                                                                   "scl ln", "raw peak", "scl peak"))
    tot_r = tot_s = 0.0
    for name, N, K in LINEARS:
        x = torch.randn(M, K, device=dev).requires_grad_(True)
        w = (torch.randn(N, K, device=dev) * K ** -0.5).requires_grad_(True)
        b = (torch.randn(N, device=dev) * 0.1).requires_grad_(True)
        dy = torch.randn(M, N, device=dev) * 1e-3
        mr, ms = compare("linear " + name, "(%d, %d)" % (N, K), lambda x, w, b: functions.split_linear(x, w, b, w, "w"),
                         lambda x, w, b: functions.split_linear_scaled(x, w, b, w, "w"), [x, w, b], dy, reps)
        tot_r += mr
        tot_s += ms
        del x, w, b, dy
    print("the 4 linears of a block, medians added: raw %.0f us, scaled %.0f us (%.3f)" % (tot_r, tot_s, tot_s / tot_r))
    C, H = 1280, 5120
    x = torch.randn(M, C, device=dev).requires_grad_(True)
    w1, b1 = (torch.randn(H, C, device=dev) * C ** -0.5).requires_grad_(True), (torch.randn(H, device=dev) * 0.1).requires_grad_(True)
    w2, b2 = (torch.randn(C, H, device=dev) * H ** -0.5).requires_grad_(True), (torch.randn(C, device=dev) * 0.1).requires_grad_(True)
    dy = torch.randn(M, C, device=dev) * 1e-3
    compare("mlp fc1-gelu-fc2", "(%d, %d)" % (H, C), lambda *a: functions.split_mlp(*a, ops.ACT_GELU), lambda *a: functions.split_mlp_scaled(*a, ops.ACT_GELU),
            [x, w1, b1, w2, b2], dy, reps)


if __name__ == "__main__":
    main()
