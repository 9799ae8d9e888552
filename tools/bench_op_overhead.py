#!/usr/bin/env python
"""Host cost of an op call: the Python time hipie_amd/ops.py spends per call on checks, allocations and argument lists.  `ops._call` is
replaced by a no-op, so nothing is launched; the operands are device tensors at the smallest legal shapes.

    python tools/bench_op_overhead.py [path/to/another/ops.py]

With a path that file is loaded in place of hipie_amd.ops (to compare two versions of the op layer on one machine).  Per op: 20 000 calls
after 2 000 warm-up calls, the median of five repeats, in microseconds per call; one JSON line."""
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hipie_amd  # noqa: E402

if len(sys.argv) > 1:
    spec = importlib.util.spec_from_file_location("hipie_amd.ops", sys.argv[1])
    ops = sys.modules["hipie_amd.ops"] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ops)
    hipie_amd.ops = ops
else:
    from hipie_amd import ops  # noqa: E402

CALLS, WARMUP, REPEATS = 20000, 2000, 5


def cases():
    f = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")          # noqa: E731
    a, w = f(256, 32), f(32, 64, dt=torch.float16)
    u, blk = f(256, 32), torch.ones(2, device="cuda")
    rq, rel_h, rel_w = f(1, 128, 80), f(1, 128, 8), f(1, 128, 16)
    x, stat, g = f(1, 8, 4, 4), f(1, 1, 2), f(8)
    qk, v = f(1, 4, 64), f(1, 4, 32)
    boxes, tgt, pairs = f(1, 4, 4), f(1, 3, 4), [(f(2, dt=torch.int64), f(2, dt=torch.int64))]
    msda = (f(1, 4, 1, 32), torch.tensor([[2, 2]], device="cuda"), f(1, dt=torch.int64), f(1, 1, 1, 2), f(1, 1, 1, 1, 1, 2), f(1, 1, 1, 1))
    return {"gemm": lambda: ops.gemm(a, w, split=True), "act_forward": lambda: ops.act_forward(u, ops.ACT_GELU),
            "grad_pack": lambda: ops.grad_pack(u, blk), "attn_pack_q": lambda: ops.attn_pack_q(rq, rel_h, rel_w, 1, 8, 16, 224),
            "group_norm_backward": lambda: ops.group_norm_backward(x, x, stat, 1, g, g),
            "query_attn_train_forward": lambda: ops.query_attn_train_forward(qk, v, None, 1, 32 ** -0.5),
            "pair_box_loss_forward": lambda: ops.pair_box_loss_forward(boxes, None, pairs, tgt, None, 1.0, 0),
            "msda_fused": lambda: ops.msda_fused(*msda)}


def main():
    ops._call = lambda name, *args: None
    out = {}
    for name, call in cases().items():
        for _ in range(WARMUP):
            call()
        per_call = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            per_call.append((time.perf_counter() - t0) / CALLS * 1e6)
        out[name] = round(statistics.median(per_call), 3)
    print(json.dumps({"ops_py": sys.argv[1] if len(sys.argv) > 1 else "hipie_amd/ops.py", "us_per_call": out}))


if __name__ == "__main__":
    main()
