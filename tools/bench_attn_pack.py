#!/usr/bin/env python3
"""The attention of ONE ViT block between its two linears, from the rows of the qkv linear to the rows of the proj linear: today's composition
(net.vit_attention under HipBackend / HipBackendWindows: reshape + permute + unbind, scale, two einsums, two cats, three f16_pair passes, the
fused kernels, and autograd's undoing of all of it; for the windowed blocks also under the default HipBackend, which materialises the logits) against the one node (functions.VitAttentionFunction over csrc/attn_pack.hip), at the
training step's ViT-H shapes: the global blocks (B = 2, 64 x 64 tokens, 16 heads) and the windowed blocks (50 windows of 14 x 14, 16 heads).
Both sides run in ONE process, alternated, `ROUNDS` times; per side: forward and forward + backward time (host clock around a device
synchronise), device launches of one forward + backward (torch profiler, a run of its own), and the peak memory above the inputs.  The two
sides' outputs and gradients are compared on the spot.
    python tools/bench_attn_pack.py            env: ROUNDS (3), ITERS (20), SMALL=1 (toy shapes: a rehearsal of the script, not a measurement)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hipie_amd.training import functions, net  # noqa: E402

DEV = "cuda"
ROUNDS, ITERS = int(os.environ.get("ROUNDS", 3)), int(os.environ.get("ITERS", 20))
SMALL = os.environ.get("SMALL") == "1"


def composition(qkv, Rh, Rw, heads, H, W, be):
    """net.vit_attention between its two linears"""
    B = qkv.shape[0]
    hd = qkv.shape[-1] // (3 * heads)
    t = qkv.reshape(B, H * W, 3, heads, -1).permute(2, 0, 3, 1, 4)
    q, k, v = t.reshape(3, B * heads, H * W, -1).unbind(0)
    rq = q.reshape(B * heads, H, W, hd)
    rel_h = torch.einsum("bhwc,hkc->bhwk", rq, Rh).reshape(B * heads, H * W, H)
    rel_w = torch.einsum("bhwc,wkc->bhwk", rq, Rw).reshape(B * heads, H * W, W)
    qa = torch.cat((q * hd ** -0.5, rel_h, rel_w), -1)
    ka = torch.cat((k, net._key_axis_indicators(H, W, k.device, k.dtype).expand(B * heads, -1, -1)), -1)
    o = be.fused_attention(qa, ka, v)
    if o is None and hasattr(be, "window_attention"):
        o = be.window_attention(qa, ka, v)
    if o is None:                                               # HipBackend on the windows: the materialised formulation
        o = (qa @ ka.transpose(-2, -1)).softmax(dim=-1) @ v
    return o.view(B, heads, H, W, -1).permute(0, 2, 3, 1, 4).reshape(B, H * W, -1)


def timed(fn, go, backward):
    for _ in range(3):
        y = fn()
        if backward:
            y.backward(go)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(ITERS):
        y = fn()
        if backward:
            y.backward(go)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / ITERS * 1e3


def launches(fn, go):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn().backward(go)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def peak(fn, go):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = fn()
    fwd = torch.cuda.max_memory_allocated() - base
    held = torch.cuda.memory_allocated() - base                 # what the graph keeps alive between the forward and the backward (+ y)
    y.backward(go)
    torch.cuda.synchronize()
    return fwd / 2 ** 20, held / 2 ** 20, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def block(name, B, heads, H, W, windows):
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = (torch.randn(B, H * W, 3 * heads * 80, device=DEV, generator=g) * 0.5).requires_grad_(True)
    tabs = [(torch.randn(2 * s - 1, 80, device=DEV, generator=g) * 0.2).requires_grad_(True) for s in (H, W)]
    go = torch.randn(B, H * W, heads * 80, device=DEV, generator=g) * 1e-3
    be = net.HipBackendWindows if windows else net.HipBackend

    def rel():
        return net.get_rel_pos(H, H, tabs[0]), net.get_rel_pos(W, W, tabs[1])
    sides = [("composition (%s)" % be.__name__, lambda: composition(qkv, *rel(), heads, H, W, be)),
             ("one node (VitAttentionFunction)", lambda: functions.vit_attention_packed(qkv, *rel(), heads, H, W, windows=windows))]
    print("== %s: B' = %d, %d x %d tokens, %d heads; qkv %.1f MB" % (name, B, H, W, heads, qkv.numel() * 4 / 2 ** 20))
    outs = []
    for _, fn in sides:
        for t in [qkv] + tabs:
            t.grad = None
        y = fn()
        y.backward(go)
        outs.append([y.detach()] + [t.grad.clone() for t in [qkv] + tabs])
    for n, a, b in zip(("y", "d qkv", "d rel_pos_h", "d rel_pos_w"), *outs):
        print("   node vs composition %-12s equal bits %-5s max|diff| / max|composition| %.2e" % (n, torch.equal(a, b), float((b - a).abs().max() / a.abs().max())))
    if windows:                                                 # what the DEFAULT backend runs on the windowed blocks: no fused kernel
        sides.insert(0, ("composition (HipBackend: materialised)", lambda: composition(qkv, *rel(), heads, H, W, net.HipBackend)))
    for rnd in range(ROUNDS):
        for side, fn in sides:
            f, fb = timed(fn, go, False), timed(fn, go, True)
            print("   round %d  %-36s forward %.3f ms, forward + backward %.3f ms" % (rnd, side, f, fb))
    for side, fn in sides:
        for t in [qkv] + tabs:
            t.grad = None
        n = launches(fn, go)
        p = peak(fn, go)
        print("   %-36s %d device launches per forward + backward; above the inputs: forward peak %.0f MB, held for the backward %.0f MB, "
              "peak %.0f MB" % (side, n, *p))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_attn_pack: needs the GPU (no host path)")
    print("bench_attn_pack: ROUNDS %d, ITERS %d%s" % (ROUNDS, ITERS, "  SMALL=1: toy shapes, NOT a measurement" if SMALL else ""))
    if SMALL:
        block("global", 1, 2, 8, 16, False)
        block("windows", 3, 2, 14, 14, True)
    else:
        block("global blocks", 2, 16, 64, 64, False)
        block("windowed blocks", 50, 16, 14, 14, True)
