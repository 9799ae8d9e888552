#!/usr/bin/env python3
"""forward + backward of the GroupNorm (+ ReLU) of each of the 11 conv + GN sites of a training step at ViT-H 1024^2, 2 images per GPU
(C = 256 in 32 groups, NCHW fp32): the one-node form (functions.GroupNormFunction: hipie_group_norm_train_forward / hipie_group_norm_backward)
against F.group_norm (+ F.relu) under autograd.  Both sides alternate in ONE process; a timed sample is a block of 10 queued calls of one side
between two events (what a call adds to a busy stream: the larger of its host side and its kernels), per site: median and minimum of 20
samples in microseconds per call, the peak memory of a call above its inputs, and the bytes a call has to move (forward 2 reads + 1 write, backward 4 reads + 1
write of the map = 8 transfers) over the node's median time beside the 6.3 TB/s a copy reaches on this part (MI355X_MICROARCH.md).
    python tools/bench_group_norm_train.py [batch] [repeats]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hipie_amd.training import functions  # noqa: E402

# (site, how many of them in a step, H = W, ReLU)
SITES = [("input_proj.0 (both heads), adapter_1", 3, 128, False), ("input_proj.1 (both heads)", 2, 64, False), ("input_proj.2 (both heads)", 2, 32, False),
         ("input_proj.3 (both heads)", 2, 16, False), ("layer_1 + ReLU", 1, 128, True), ("mask_features + ReLU", 1, 256, True)]
COPY_TBS = 6.3
BLOCK = 10          # queued calls per timed sample


def node(x, w, b, relu):
    return functions.group_norm(x, 32, w, b, 1e-5, relu)


def library(x, w, b, relu):
    y = F.group_norm(x, 32, w, b, 1e-5)
    return F.relu(y) if relu else y


def one_call(fn, x, w, b, dy, relu):
    x.grad = w.grad = b.grad = None
    fn(x, w, b, relu).backward(dy)


def timed(fn, args):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(BLOCK):
        one_call(fn, *args)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / BLOCK


def peak_above_inputs(fn, args):
    one_call(fn, *args)
    args[0].grad = args[1].grad = args[2].grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    one_call(fn, *args)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    print("GroupNorm(32, 256) forward + backward, B = %d, fp32 NCHW, %d alternated samples of %d queued calls per side; us per call" % (B, reps, BLOCK))
    print("%-38s %2s %5s | %9s %9s | %9s %9s | %6s | %8s %8s | %s" % ("site", "n", "H=W", "node med", "node min", "lib med", "lib min", "lib/nd",
                                                                       "node MiB", "lib MiB", "node TB/s of %.1f" % COPY_TBS))
    step_node = step_lib = 0.0
    for name, count, hw, relu in SITES:
        x = torch.randn(B, 256, hw, hw, device=dev).requires_grad_(True)
        w = (torch.randn(256, device=dev) * 0.5 + 1).requires_grad_(True)
        b = torch.randn(256, device=dev).requires_grad_(True)
        dy = torch.randn(B, 256, hw, hw, device=dev)
        args = (x, w, b, dy, relu)
        assert node(x, w, b, relu) is not None
        for _ in range(5):
            one_call(node, *args)
            one_call(library, *args)
        tn, tl = [], []
        for _ in range(reps):
            tn.append(timed(node, args))
            tl.append(timed(library, args))
        mn, ml = statistics.median(tn), statistics.median(tl)
        moved = 8 * x.numel() * 4
        print("%-38s %2d %5d | %9.1f %9.1f | %9.1f %9.1f | %6.2f | %8.1f %8.1f | %.2f" % (
            name, count, hw, mn, min(tn), ml, min(tl), ml / mn, peak_above_inputs(node, args), peak_above_inputs(library, args), moved / (mn * 1e-6) / 1e12))
        step_node += count * mn
        step_lib += count * ml
    print("the 11 sites of a step, medians added: node %.0f us, library %.0f us" % (step_node, step_lib))


if __name__ == "__main__":
    main()
