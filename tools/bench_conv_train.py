#!/usr/bin/env python3
"""forward + backward of each dense 3 x 3 / stride 1 / padding 1 convolution site of a training step at ViT-H 1024^2, 2 images per GPU
(fp32, 256 input channels): the one-node form (functions.Conv3x3Function: hipie_conv3x3_split forward and input gradient,
hipie_conv3x3_wgrad for the weight and bias gradient) against F.conv2d (+ F.relu) under autograd.  Both sides alternate in ONE process; a
timed sample is a block of 5 queued calls of one side between two events (what a call adds to a busy stream: the larger of its host side
and its kernels), per site: median and minimum of the samples in microseconds per call, the launches of one call (torch.profiler's
device-side kernel and memcpy / memset events), the bytes autograd keeps between forward and backward above the node's inputs, the peak
memory of a call above its inputs, and the node's 6 B Hp Wp 9 Cin Cout flops (three passes of the dense product, border rows included) over
its median time.
    python tools/bench_conv_train.py [batch] [repeats]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hipie_amd.training import functions  # noqa: E402

# (site, H = W at 1024^2 inputs, Cout, ReLU inside the node)
SITES = [("mask_head.lay3 + ReLU", 32, 256, True), ("mask_head.lay4 + ReLU", 64, 256, True), ("mask_head.jia_dcn + ReLU", 128, 256, True),
         ("mask_head.lay1 + ReLU", 128, 64, True), ("pixel_decoder.layer_1", 128, 256, False)]
CIN = 256
BLOCK = 5           # queued calls per timed sample


def node(x, w, b, relu):
    return functions.conv3x3_train(x, w, b, relu)


def library(x, w, b, relu):
    y = F.conv2d(x, w, b, padding=1)
    return F.relu(y) if relu else y


def one_call(fn, x, w, b, dy, relu):
    x.grad = w.grad = None
    if b is not None:
        b.grad = None
    fn(x, w, b, relu).backward(dy)


def timed(fn, args):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(BLOCK):
        one_call(fn, *args)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / BLOCK


def memory(fn, args):
    """(MiB alive between forward and backward above the inputs, output included; peak MiB of the call above the inputs)"""
    one_call(fn, *args)
    x, w, b, dy, relu = args
    x.grad = w.grad = None
    if b is not None:
        b.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = fn(x, w, b, relu)
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - base
    y.backward(dy)
    del y
    torch.cuda.synchronize()
    return kept / 2 ** 20, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def launches(fn, args):
    from torch.profiler import ProfilerActivity, profile
    one_call(fn, *args)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        one_call(fn, *args)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    # the library side as the step runs it: HIPIE_IMG.finalize lets MIOpen benchmark its solvers once per configuration unless HIPIE_MIOPEN_FIND=0
    torch.backends.cudnn.benchmark = os.environ.get("HIPIE_MIOPEN_FIND", "1") != "0"
    print("conv 3 x 3 (%d -> Cout) forward + backward, B = %d, fp32, %d alternated samples of %d queued calls per side; us per call" % (CIN, B, reps, BLOCK))
    print("%-26s %5s %4s | %9s %9s | %9s %9s | %6s | %7s %7s | %9s %9s | %9s %9s | %s" % (
        "site", "H=W", "Cout", "node med", "node min", "lib med", "lib min", "lib/nd", "node ln", "lib ln", "node kept", "lib kept", "node peak", "lib peak",
        "node TFLOP/s"))
    step_node = step_lib = 0.0
    for name, hw, cout, relu in SITES:
        has_bias = not name.startswith("pixel_decoder")
        x = torch.randn(B, CIN, hw, hw, device=dev).requires_grad_(True)
        w = (torch.randn(cout, CIN, 3, 3, device=dev) * (9 * CIN) ** -0.5).requires_grad_(True)
        b = (torch.randn(cout, device=dev) * 0.1).requires_grad_(True) if has_bias else None
        dy = torch.randn(B, cout, hw, hw, device=dev)
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
        flops = 6.0 * B * (hw + 2) * (hw + 2) * 9 * CIN * cout
        kn, pn = memory(node, args)
        kl, pl = memory(library, args)
        print("%-26s %5d %4d | %9.1f %9.1f | %9.1f %9.1f | %6.2f | %7d %7d | %9.1f %9.1f | %9.1f %9.1f | %.1f" % (
            name, hw, cout, mn, min(tn), ml, min(tl), ml / mn, launches(node, args), launches(library, args), kn, kl, pn, pl, flops / (mn * 1e-6) / 1e12))
        step_node += mn
        step_lib += ml
    print("the 5 sites of a step, medians added: node %.0f us, library %.0f us" % (step_node, step_lib))


if __name__ == "__main__":
    main()
