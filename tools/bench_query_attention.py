#!/usr/bin/env python3
"""forward + backward of the decoders' query self-attention at the two training geometries (8 heads of 32, fp32): the one node over
csrc/attn_f32_train.hip (functions.QueryAttentionFunction, net.HipBackendQueryAttention) against net.mha's materialised formulation under
autograd.  B = 2, N = 1110 (200 de-noising + 10 background + 900 queries, the mask by dn.cdn_queries' rule) and N = 400 (100 de-noising + 300
queries, dn.maskdino_dn_queries' rule).  Two scopes per geometry: `mha` = net.mha from (tgt + pos, tgt) to out_proj's output with the
parameters trainable (what a decoder layer runs: the node side computes q | k with one linear), `core` = from the projected rows to the
attention output alone.  Both sides alternate in ONE process; a timed sample is a block of queued calls of one side between two events (what
a call adds to a busy stream: the larger of its host side and its kernels): median and minimum in microseconds per call, the device launches
of one call (kernels, copies, fills, from the profiler) and the peak memory of a call above its inputs.  No threshold: it reports.
    python tools/bench_query_attention.py [batch] [repeats]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hipie_amd.training import functions, net  # noqa: E402

HEADS, C = 8, 256
# (name, N, de-noising queries in front, queries per de-noising group)
GEOMETRIES = [("thing decoder", 1110, 200, 20), ("MaskDINO decoder", 400, 100, 10)]
BLOCK = 10          # queued calls per timed sample


def dn_mask(N, pad, per_group, dev):
    """dn.cdn_queries (groups of 2 P) / dn.maskdino_dn_queries (groups of P): a group sees itself only, the matching queries see no de-noising query"""
    group = torch.arange(pad, device=dev) // per_group
    mask = torch.zeros(N, N, dtype=torch.bool, device=dev)
    mask[:pad, :pad] = group[:, None] != group[None, :]
    mask[pad:, :pad] = True
    return mask


def materialised_core(qk, v, mask, heads):
    B, N, Cc = v.shape
    hd = Cc // heads

    def sp(t):
        return t.reshape(B, N, heads, hd).transpose(1, 2)
    a = (sp(qk[..., :Cc]) * hd ** -0.5) @ sp(qk[..., Cc:]).transpose(-1, -2)
    a = a.masked_fill(mask[None, None], float("-inf"))
    return (a.softmax(-1) @ sp(v)).transpose(1, 2).reshape(B, N, Cc)


def make_case(scope, side, B, N, mask, dev):
    """a closure running one forward + backward of (scope, side) and the tensors whose .grad it fills"""
    g = torch.Generator().manual_seed(N)
    if scope == "mha":
        sd = {"a.in_proj_weight": torch.randn(3 * C, C, generator=g) * C ** -0.5, "a.in_proj_bias": torch.randn(3 * C, generator=g) * 0.1,
              "a.out_proj.weight": torch.randn(C, C, generator=g) * C ** -0.5, "a.out_proj.bias": torch.randn(C, generator=g) * 0.1}
        sd = {k: t.to(dev).requires_grad_(True) for k, t in sd.items()}
        tgt, pos = (torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True) for _ in range(2))
        dy = torch.randn(B, N, C, generator=g).to(dev)
        be = net.HipBackendQueryAttention if side == "node" else None
        leaves = [tgt, pos] + list(sd.values())

        def call():
            net.mha(tgt + pos, tgt, sd, "a.", mask, HEADS, be=be).backward(dy)
    else:
        qk = (torch.randn(B, N, 2 * C, generator=g) * 1.5).to(dev).requires_grad_(True)
        v = (torch.randn(B, N, C, generator=g) * 1.5).to(dev).requires_grad_(True)
        dy = torch.randn(B, N, C, generator=g).to(dev)
        leaves = [qk, v]
        fn = functions.query_attention if side == "node" else materialised_core
        assert side != "node" or fn(qk, v, mask, HEADS) is not None

        def call():
            fn(qk, v, mask, HEADS).backward(dy)

    def one_call():
        for t in leaves:
            t.grad = None
        call()
    return one_call, leaves


def timed(one_call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(BLOCK):
        one_call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / BLOCK


def launches(one_call):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        one_call()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def peak_above_inputs(one_call, leaves):
    one_call()
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    one_call()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    print("query self-attention forward + backward, B = %d, %d heads of 32, fp32; %d alternated samples of %d queued calls per side; us per call" % (B, HEADS, reps, BLOCK))
    print("%-18s %5s %-5s | %9s %9s | %9s %9s | %7s | %9s %9s | %9s %9s" % ("geometry", "N", "scope", "node med", "node min", "torch med", "torch min", "torch/nd",
                                                                              "node lnch", "torch lnch", "node MiB", "torch MiB"))
    for name, N, pad, per_group in GEOMETRIES:
        mask = dn_mask(N, pad, per_group, dev)
        for scope in ("mha", "core"):
            node, node_leaves = make_case(scope, "node", B, N, mask, dev)
            lib, lib_leaves = make_case(scope, "torch", B, N, mask, dev)
            for _ in range(5):
                node()
                lib()
            tn, tl = [], []
            for _ in range(reps):
                tn.append(timed(node))
                tl.append(timed(lib))
            mn, ml = statistics.median(tn), statistics.median(tl)
            print("%-18s %5d %-5s | %9.1f %9.1f | %9.1f %9.1f | %7.2f | %9d %9d | %9.1f %9.1f" % (
                name, N, scope, mn, min(tn), ml, min(tl), ml / mn, launches(node), launches(lib), peak_above_inputs(node, node_leaves),
                peak_above_inputs(lib, lib_leaves)))
    print("kernel-only times and counters: not taken by this tool (it times calls on a busy stream)")


if __name__ == "__main__":
    main()
