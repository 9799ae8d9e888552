#!/usr/bin/env python3
"""The fused windowed training attention (csrc/attn_train_win.hip, training/functions.WindowAttentionFunction) against the materialised torch
formulation at the training step's windowed-block shape: 2 images x 25 windows x 16 heads = 800 items of 14 x 14 = 196 tokens, q' / k' of 108
columns (80 + 14 + 14), v of 80.  Forward and forward + backward, ms per ViT block, both sides in one process."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hipie_amd.training.functions import WindowAttentionFunction  # noqa: E402

BH, N, DQ, DV = int(os.environ.get("BH", 800)), 196, 108, 80
g = torch.Generator(device="cuda").manual_seed(0)
qa = (torch.randn(BH, N, DQ, device="cuda", generator=g) * 0.5).requires_grad_(True)
ka = torch.randn(BH, N, DQ, device="cuda", generator=g).requires_grad_(True)
v = torch.randn(BH, N, DV, device="cuda", generator=g).requires_grad_(True)
go = torch.randn(BH, N, DV, device="cuda", generator=g) * 1e-3


def materialised():
    return (qa @ ka.transpose(-2, -1)).softmax(dim=-1) @ v


def fused():
    return WindowAttentionFunction.apply(qa, ka, v)


def bench(fn, backward, n=20):
    for _ in range(3):
        o = fn()
        if backward:
            o.backward(go)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        o = fn()
        if backward:
            o.backward(go)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


for rnd in range(2):                                            # both sides twice, alternating: the second round is the steady one
    for name, fn in (("materialised (library fp32 GEMMs + softmax)", materialised), ("fused (hipie_attn_train_win_*)", fused)):
        f = bench(fn, False)
        fb = bench(fn, True)
        torch.cuda.reset_peak_memory_stats()
        fn().backward(go)
        torch.cuda.synchronize()
        print("round %d  %-46s forward %.3f ms, forward + backward %.3f ms per block (BH = %d, N = %d); peak memory of one block %.3f GB"
              % (rnd, name, f, fb, BH, N, torch.cuda.max_memory_allocated() / 2 ** 30))
