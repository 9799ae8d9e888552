#!/usr/bin/env python3
"""the amax the scale kernel sees at the split linears of one synthetic ViT-H training step (tools/bench_train_step.py's step, random-init
weights): every ops.grad_scale call of the LAST backward, in call order, with the scale chosen.  ops.grad_scale is wrapped to keep dy.abs().amax() and the
block on the device; they are read after the run.
    python tools/grad_scale_amax.py"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from hipie_amd import ops  # noqa: E402

seen = []
real = ops.grad_scale


def spy(dy):
    blk = real(dy)
    seen.append((tuple(dy.shape), blk, dy.abs().amax()))          # device tensors: read after the run
    return blk


ops.grad_scale = spy
import bench_train_step as bts  # noqa: E402

sys.argv = ["bench_train_step.py", "2", "1", "--scaled-grads", "--fused-mlp"]
bts.main()
torch.cuda.synchronize()
per_step = len(seen) // 3                                         # 2 untimed steps + 1
last = seen[-per_step:]
print("AMAX %d grad_scale calls per step" % per_step)
for i, (shape, blk, amax) in enumerate(last):
    if i < 14 or i >= per_step - 14 or i % 16 == 0:
        print("AMAX call %3d dy %-14s amax %.3e  s = 2^%d" % (i, shape, float(amax), round(math.log2(float(blk[0])))))
am = sorted(float(a) for _, _, a in last)
print("AMAX over the step: min %.3e median %.3e max %.3e; calls with amax < 6.1e-5 (fp16 subnormal hi): %d of %d" % (
    am[0], am[len(am) // 2], am[-1], sum(1 for a in am if a < 6.1e-5), len(am)))
