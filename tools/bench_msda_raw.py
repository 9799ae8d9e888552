#!/usr/bin/env python3
"""forward + backward of ONE MSDeformAttn module call of the training step (training/net.py::msda_module, hidden 256, 8 heads, 4 levels x 4
points), the one-node form (net.HipBackendDeformable: hipie_msda_fused_forward / hipie_msda_raw_backward) against the composition of
net.HipBackend (torch ops for the locations and the softmax around hipie_msda_forward / hipie_msda_backward_ws), in one process, alternated:
    python tools/bench_msda_raw.py [reps] [encoder | decoder]
  encoder geometry: B = 2, 21760 queries over the 21760 tokens of a 1024^2 pyramid (128, 64, 32, 16), 2-wide reference points
  decoder geometry: B = 2, 1100 queries over the same tokens, 4-wide reference points (boxes)
Prints per geometry and form: ms per call (median of reps, HIP events around forward + backward), device launches of one call (torch
profiler), and the peak memory of one call above what is held before it."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hipie_amd.training import net  # noqa: E402

SHAPES = [(128, 128), (64, 64), (32, 32), (16, 16)]
C, HEADS, L, P = 256, 8, 4, 4


def module_inputs(B, Lq, ref_dim, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in SHAPES)
    sd = {}
    for name, n_out, scale in (("value_proj.", C, 0.06), ("sampling_offsets.", HEADS * L * P * 2, 0.03), ("attention_weights.", HEADS * L * P, 0.06),
                               ("output_proj.", C, 0.06)):
        sd["a." + name + "weight"] = (torch.randn(n_out, C, generator=g) * scale).to(dev).requires_grad_(True)
        sd["a." + name + "bias"] = (torch.randn(n_out, generator=g) * (2.0 if name == "sampling_offsets." else 0.1)).to(dev).requires_grad_(True)
    query = torch.randn(B, Lq, C, generator=g).to(dev).requires_grad_(True)
    src = torch.randn(B, S, C, generator=g).to(dev).requires_grad_(True)
    ref = torch.rand(B, Lq, L, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] = 0.05 + 0.3 * ref[..., 2:]
    ref = ref.to(dev).requires_grad_(True)
    pad = torch.zeros(B, S, dtype=torch.bool, device=dev)
    gout = torch.randn(B, Lq, C, generator=g).to(dev)
    return sd, query, src, ref, pad, gout


def one_call(be, sd, query, src, ref, pad, gout):
    for t in [query, src, ref] + list(sd.values()):
        t.grad = None
    with torch.enable_grad():
        out = net.msda_module(query, ref, src, SHAPES, pad, sd, "a.", be, HEADS, L, P)
    out.backward(gout)
    return out


def measure(be, args, reps):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        one_call(be, *args)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        one_call(be, *args)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    for t in [args[1], args[2], args[3]] + list(args[0].values()):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    one_call(be, *args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        one_call(be, *args)
        torch.cuda.synchronize()
    launches = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    return times, launches, peak


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    only = sys.argv[2] if len(sys.argv) > 2 else None            # one geometry: for a kernel trace of it
    dev = torch.device("cuda", 0)
    for geom, Lq, ref_dim in (("encoder", sum(h * w for h, w in SHAPES), 2), ("decoder", 1100, 4)):
        if only not in (None, geom):
            continue
        args = module_inputs(2, Lq, ref_dim, dev)
        res = {}
        for rnd in range(2):                                     # alternated: composition, node, composition, node
            for name, be in (("composition", net.HipBackend), ("node", net.HipBackendDeformable)):
                times, launches, peak = measure(be, args, reps)
                res.setdefault(name, []).append((statistics.median(times), min(times), launches, peak))
        for name, rows in res.items():
            print("msda module, %s (B=2, Lq=%d, ref_dim %d), %-11s: %s ms per forward+backward (median of %d, two rounds; min %s); %d device launches; "
                  "peak memory of one call %.1f MB" % (geom, Lq, ref_dim, name, " / ".join("%.3f" % r[0] for r in rows), reps,
                                                       " / ".join("%.3f" % r[1] for r in rows), rows[-1][2], rows[-1][3] / 2 ** 20))
        out_c, out_n = one_call(net.HipBackend, *args), one_call(net.HipBackendDeformable, *args)
        print("   outputs of the two forms differ by %.1e of the output scale" % float((out_c - out_n).detach().abs().max() / out_c.detach().abs().max()))


if __name__ == "__main__":
    main()
