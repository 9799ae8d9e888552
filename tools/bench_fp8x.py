#!/usr/bin/env python3
"""The `fp8x` policy's numbers (Precision.fp8x: split3 with the ViT MLP output fc2 on hipie_gemm_f8x), printed as ONE JSON line:
  (a) fc2 at the headline shape (M = 32768 tokens, K = 5120, N = 1280, residual added in place): HIP-event median of hipie_gemm (split, three
      fp16 products) and hipie_gemm_f8x (cross terms on block-scaled e4m3) in the same process, and their TFLOP/s (2 M N K per launch);
  (b) the timed step (ViT-H, 1024^2, bs 8, 80-class caption: bench.py's workload) under split3 and fp8x in one process, alternated A B A B as
      tools/ab_step.py does (one model; the policy's fc2 switch flipped between rounds);
  (c) bench.parity_error(Precision.fp8x()) on the five gate fixtures.
python tools/bench_fp8x.py [--rounds R] [--skip-step] [--skip-parity]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from hipie_amd import fp8x, ops  # noqa: E402
from hipie_amd.config import HipieConfig, Precision  # noqa: E402


def _median_ms(fn, n=50, warm=10):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def fc2_launch(dev):
    M, K, N = 32768, 5120, 1280
    g = torch.Generator().manual_seed(0)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    x = ops.to_hl8(torch.randn(M, K, device=dev))
    w_hl8 = ops.hl8_pack(W.to(dev))
    w8, wsc = fp8x.pack_from_hl8(w_hl8, *ops.to_f8x(w_hl8))
    bias = torch.randn(N, device=dev) * 0.1
    res = torch.randn(M, N, device=dev)
    t_split = _median_ms(lambda: ops.gemm(x, w_hl8, bias, res, split=True, out=res))
    t_f8x = _median_ms(lambda: ops.gemm_f8x(x, w8, wsc, bias, res, out=res))
    fl = 2.0 * M * N * K
    return {"shape": {"M": M, "K": K, "N": N, "resid_in_place": True}, "split_ms": round(t_split, 4), "f8x_ms": round(t_f8x, 4),
            "ratio": round(t_f8x / t_split, 3), "split_tflops": round(fl / t_split * 1e-9, 1), "f8x_tflops": round(fl / t_f8x * 1e-9, 1)}


def step_ab(dev, rounds):
    from hipie_amd.hipie_img import HIPIE_IMG
    from hipie_amd.postprocess import inference_compact
    torch.set_grad_enabled(False)
    cfg = HipieConfig.vit_huge()
    torch.manual_seed(0)
    model = HIPIE_IMG(cfg, Precision.split3(), device=dev)
    bench.randomize_degenerate_inits(model)
    model.finalize()
    batch = bench.synth_batch(cfg, 8, 1024, 80, 194, dev, seed=0)
    precs = {id(m.precision): m.precision for m in model.modules() if isinstance(getattr(m, "precision", None), Precision)}

    def switch(on):
        for p in precs.values():
            p.fp8x_linears = ("fc2",) if on else ()

    def timed(n=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            inference_compact(model, model.forward_raw(batch), batch, topk=100)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    for on in (False, True):
        switch(on)
        for _ in range(3):
            inference_compact(model, model.forward_raw(batch), batch, topk=100)
    res = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            switch(on)
            res[on].append(timed())
    switch(False)
    a, b = sum(res[False]) / rounds, sum(res[True]) / rounds
    return {"split3_ms": round(a, 2), "fp8x_ms": round(b, 2), "delta_ms": round(b - a, 2), "split3_rounds": [round(t, 2) for t in res[False]],
            "fp8x_rounds": [round(t, 2) for t in res[True]], "workload": "ViT-H 1024^2 bs 8, 80-class caption (L 194), eager steps"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-parity", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"policy": "fp8x", "fc2_launch": fc2_launch(dev)}
    if not args.skip_step:
        out["step"] = step_ab(dev, args.rounds)
        torch.cuda.empty_cache()
    if not args.skip_parity:
        out["parity_err"] = bench.parity_error(Precision.fp8x(), dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
