#!/usr/bin/env python3
"""forward + backward of the core of the vision-language fusion attention at the training geometry (8 heads of 256, fp32, B = 2,
Nv = 128² + 64² + 32² + 16² = 21 760 visual tokens of a 1024² image): the one node over csrc/bi_attn_train.hip
(functions.FusionAttentionFunction, net.HipBackendFusionAttention) against the materialised formulation, net.bi_attention_block's op chain
between the projections under autograd (with F.dropout at r > 0; the node has its own keep function, so the two sides' masks differ).
L = 194 (the 80-class caption) and L = 40, each with r = 0 and r = 0.1.  Both sides alternate in ONE process per case; a timed sample is one
call between two events on an idle stream: median and minimum of `repeats` in microseconds, the device launches of one call (kernels,
copies, fills, from the profiler) and the peak memory of a call above its inputs.  No threshold: it reports.  Every case runs in a child
process of its own under a time limit, so a case that hangs ends alone.
    python tools/bench_fusion_attention.py [batch] [repeats]"""
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADS, E, NV = 8, 2048, 128 * 128 + 64 * 64 + 32 * 32 + 16 * 16
CASES = [(194, 0.0), (194, 0.1), (40, 0.0), (40, 0.1)]
CASE_SECONDS = 240


def materialised(q, k, vv, vl, mask, heads, dropout):
    import torch
    import torch.nn.functional as F
    B, Nv, Ee = q.shape
    L = k.shape[1]
    hd = Ee // heads

    def split(t, n):
        return t.view(B, n, heads, hd).transpose(1, 2).reshape(B * heads, n, hd)
    qs, ks, vvs, vls = split(q * hd ** -0.5, Nv), split(k, L), split(vv, Nv), split(vl, L)
    w = torch.bmm(qs, ks.transpose(1, 2)).clamp(min=-50000).clamp(max=50000)
    wT = w.transpose(1, 2)
    wl = (wT - torch.max(wT, dim=-1, keepdim=True)[0]).clamp(min=-50000).clamp(max=50000).softmax(dim=-1)
    am = mask.to(torch.int64)[:, None, None, :].expand(B, 1, Nv, L)
    am = am.masked_fill(am == 0, int(-9e15))
    wv = F.softmax((w.view(B, heads, Nv, L) + am).view(B * heads, Nv, L), dim=-1)
    if dropout > 0:
        wv, wl = F.dropout(wv, dropout, True), F.dropout(wl, dropout, True)
    return (torch.bmm(wv, vls).view(B, heads, Nv, hd).transpose(1, 2).reshape(B, Nv, Ee),
            torch.bmm(wl, vvs).view(B, heads, L, hd).transpose(1, 2).reshape(B, L, Ee))


def run_case(B, L, r, reps):
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    from hipie_amd.training import functions
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(L)
    leaves = [(torch.randn(B, n, E, generator=g) * 1.5).to(dev).requires_grad_(True) for n in (NV, L, NV, L)]
    gv, gl = torch.randn(B, NV, E, generator=g).to(dev), torch.randn(B, L, E, generator=g).to(dev)
    mask = torch.ones(B, L, dtype=torch.int64, device=dev)
    mask[1, L * 2 // 3:] = 0
    assert functions.fusion_attention(*leaves, mask, HEADS, r) is not None

    def side(fn):
        def one_call():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(fn(*leaves, mask, HEADS, r), (gv, gl))
        return one_call
    node, lib = side(functions.fusion_attention), side(materialised)

    def timed(call):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3

    def launches(call):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)

    def peak(call):
        call()
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        call()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(2):
        node()
        lib()
    tn, tl = [], []
    for _ in range(reps):
        tn.append(timed(node))
        tl.append(timed(lib))
    mn, ml = statistics.median(tn), statistics.median(tl)
    print("%5d %5d %4.1f | %10.1f %10.1f | %10.1f %10.1f | %7.2f | %9d %10d | %9.1f %9.1f" % (
        NV, L, r, mn, min(tn), ml, min(tl), ml / mn, launches(node), launches(lib), peak(node), peak(lib)), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]))
        return
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    print("fusion attention core forward + backward, B = %d, %d heads of 256, fp32; %d alternated samples per side; us per call" % (B, HEADS, reps))
    print("%5s %5s %4s | %10s %10s | %10s %10s | %7s | %9s %10s | %9s %9s" % ("Nv", "L", "r", "node med", "node min", "torch med", "torch min", "torch/nd",
                                                                             "node lnch", "torch lnch", "node MiB", "torch MiB"), flush=True)
    for L, r in CASES:
        # a fresh child per case, under its own time limit; a failed or timed-out case ends the tool: nothing more is started on the device
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(B), str(L), str(r), str(reps)], timeout=CASE_SECONDS).returncode
        if rc != 0:
            sys.exit("case L=%d r=%g ended with status %d: stopping" % (L, r, rc))
    print("kernel-only times and counters: not taken by this tool (it times whole calls)")


if __name__ == "__main__":
    main()
