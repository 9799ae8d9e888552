#!/usr/bin/env python3
"""forward + backward of each projection site of a training step at ViT-H 1024^2, 2 images per GPU (fp32) -- the convolutions whose
kernel equals their stride and the two transposed 2 x 2 ones: the one-node form (functions.PatchConvFunction: hipie_patch_pack + the split
GEMM entries) against F.conv2d / F.conv_transpose2d under autograd.  Both sides alternate in ONE process; a timed sample is a block of 5
queued calls of one side between two events.  Per site and per layout of the input and of the output gradient (NCHW dense, or
channels-last as the node's own outputs and the ViT's token rows are): median and minimum of the samples in microseconds per call, the
launches of one call (torch.profiler's device-side kernel and memcpy / memset events), the peak memory of a call above its inputs, and the
node's flops (2 M K N per product: forward, input gradient unless the input is frozen, weight gradient) over its median time.
    python tools/bench_patch_conv.py [batch] [repeats]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hipie_amd.training import functions  # noqa: E402

# (site, form, Cin, Cout, H = W of the input at 1024^2, k, bias, trainable input)
SITES = [("vit.patch_embed.proj", "conv", 3, 1280, 1024, 16, True, False),
         ("vit.fpn1.0", "convt", 1280, 640, 64, 2, True, True),
         ("input_proj.0.0 (x2)", "conv", 640, 256, 128, 1, True, True),
         ("input_proj.1.0 (x2)", "conv", 1280, 256, 64, 1, True, True),
         ("input_proj.2.0 (x2)", "conv", 1280, 256, 32, 1, True, True),
         ("pixel_decoder.adapter_1", "conv", 640, 256, 128, 1, False, True),
         ("pixel_decoder.mask_features.0", "convt", 256, 256, 128, 2, True, True),
         ("pixel_decoder.mask_features.3", "conv", 256, 256, 256, 1, True, True)]
BLOCK = 5           # queued calls per timed sample


def node(form, x, w, b, k):
    return functions.patch_convt_train(x, w, b) if form == "convt" else functions.patch_conv_train(x, w, b, stride=k)


def library(form, x, w, b, k):
    return F.conv_transpose2d(x, w, b, stride=2) if form == "convt" else F.conv2d(x, w, b, stride=k)


def one_call(fn, form, x, w, b, k, dy):
    x.grad = w.grad = None
    if b is not None:
        b.grad = None
    fn(form, x, w, b, k).backward(dy)


def timed(fn, args):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(BLOCK):
        one_call(fn, *args)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / BLOCK


def peak(fn, args):
    """peak MiB of a call above its inputs"""
    one_call(fn, *args)
    args[1].grad = args[2].grad = None
    if args[3] is not None:
        args[3].grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(*args[:5]).backward(args[5])
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def launches(fn, args):
    from torch.profiler import ProfilerActivity, profile
    one_call(fn, *args)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        one_call(fn, *args)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def as_layout(t, layout):
    return t.contiguous() if layout == "nchw" else t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    # the library side as the step runs it: HIPIE_IMG.finalize lets MIOpen benchmark its solvers once per configuration unless HIPIE_MIOPEN_FIND=0
    torch.backends.cudnn.benchmark = os.environ.get("HIPIE_MIOPEN_FIND", "1") != "0"
    print("projections forward + backward, B = %d, fp32, %d alternated samples of %d queued calls per side; us per call" % (B, reps, BLOCK))
    print("%-30s %-6s %7s | %9s %9s | %9s %9s | %6s | %7s %7s | %9s %9s | %s" % (
        "site", "layout", "M", "node med", "node min", "lib med", "lib min", "lib/nd", "node ln", "lib ln", "node peak", "lib peak", "node TFLOP/s"))
    for name, form, cin, cout, hw, k, has_bias, grad_x in SITES:
        for layout in ("nchw", "cl"):
            if layout == "cl" and not grad_x:
                continue                                   # the image is NCHW
            x = as_layout(torch.randn(B, cin, hw, hw, device=dev), layout).requires_grad_(grad_x)
            fan = cin if form == "convt" else cin * k * k
            w = (torch.randn((cin, cout, 2, 2) if form == "convt" else (cout, cin, k, k), device=dev) * fan ** -0.5).requires_grad_(True)
            b = (torch.randn(cout, device=dev) * 0.1).requires_grad_(True) if has_bias else None
            ohw = 2 * hw if form == "convt" else hw // k
            dy = as_layout(torch.randn(B, cout, ohw, ohw, device=dev), layout)
            args = (form, x, w, b, k, dy)
            assert node(form, x, w, b, k) is not None
            for _ in range(3):
                one_call(node, *args)
                one_call(library, *args)
            tn, tl = [], []
            for _ in range(reps):
                tn.append(timed(node, args))
                tl.append(timed(library, args))
            mn, ml = statistics.median(tn), statistics.median(tl)
            M = B * hw * hw if form == "convt" else B * (hw // k) ** 2
            flops = 2.0 * M * (cin * (1 if form == "convt" else k * k)) * (cout * (4 if form == "convt" else 1)) * (3 if grad_x else 2)
            print("%-30s %-6s %7d | %9.1f %9.1f | %9.1f %9.1f | %6.2f | %7d %7d | %9.1f %9.1f | %.1f" % (
                name, layout, M, mn, min(tn), ml, min(tl), ml / mn, launches(node, args), launches(library, args), peak(node, args), peak(library, args),
                flops / (mn * 1e-6) / 1e12))
            del x, w, b, dy, args
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
