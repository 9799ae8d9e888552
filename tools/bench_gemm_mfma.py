#!/usr/bin/env python3
"""A/B of the two MFMA shapes of the wide split GEMM (gemm_kernel<320, true, VAR, 32 | 16>, csrc/gemm_tile.h) on the ViT-H linears at
32768 tokens.  Needs a study build of the library (make EXTRA=-DHIPIE_STUDY_KNOBS; select it with HIPIE_LIB_PATH): HIPIE_GEMM_MFMA is read
at every launch there, so the two instances alternate round by round inside ONE process, on RANDOM operands (zeros rank the shapes by cycles
and miss the clock the chip holds on each: MI355X_MICROARCH.md, DVFS give-back).

    bench_gemm_mfma.py [rounds [launches]]        the A/B: median and minimum over the rounds of the per-launch time of each side
    bench_gemm_mfma.py pmc <case> <16|32> [n]     n launches of one case on one instance and nothing else (counter passes)

The bar of docs/measurements.md: the 16x16x32 instance ships for a shape only if its MEDIAN is below the 32x32x16 instance's MINIMUM."""
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from hipie_amd import ops  # noqa: E402
from hipie_amd.modeling.vit import window_row_maps  # noqa: E402

M = 32768
C = 1280


def cases():
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    ws = {}

    def weight(N, K):
        if (N, K) not in ws:
            ws[(N, K)] = (ops.hl8_pack(torch.randn(N, K, device=dev, generator=g) * K ** -0.5), torch.randn(N, device=dev, generator=g))
        return ws[(N, K)]

    x1 = ops.to_hl8(torch.randn(M, C, device=dev, generator=g))
    x4 = ops.to_hl8(torch.randn(M, 4 * C, device=dev, generator=g))
    stream = torch.randn(M, C, device=dev, generator=g)
    # the gathered qkv of a windowed block: 8 images of 64 x 64 tokens in 14 x 14 windows; the operand and the output are in window layout
    # (padding rows included), the product runs over the real tokens only
    out_src, _, nwin = window_row_maps(8, 64, 64, 14, dev)
    rows = out_src.numel()
    tok2win = torch.empty(M, dtype=torch.int32, device=dev)
    valid = out_src >= 0
    tok2win[out_src[valid].long()] = torch.arange(rows, dtype=torch.int32, device=dev)[valid]
    xw = ops.to_hl8(torch.randn(rows, C, device=dev, generator=g))
    qkv_win = torch.zeros(rows, 6 * C, dtype=torch.float16, device=dev)

    def lin(x, N, K, **kw):
        w, b = weight(N, K)
        return lambda: ops.gemm(x, w, b, split=True, **kw)

    out = [
        ("qkv", 3 * C, C, lin(x1, 3 * C, C, out_fmt=ops.HL8)),
        ("fc1+gelu", 4 * C, C, lin(x1, 4 * C, C, out_fmt=ops.HL8, act=ops.ACT_GELU)),
        ("proj", C, C, lin(x1, C, C, out_fmt=ops.HL8)),
        ("fc2", C, 4 * C, lin(x4, C, 4 * C, out_fmt=ops.HL8)),
        ("proj f32+res", C, C, lin(x1, C, C, resid=stream, out=stream)),
        ("fc2 f32+res", C, 4 * C, lin(x4, C, 4 * C, resid=stream, out=stream)),
        ("qkv gathered", 3 * C, C, lin(xw, 3 * C, C, out_fmt=ops.HL8, out=qkv_win, out_row=tok2win, a_row=tok2win)),
    ]
    return out


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "pmc":
        name, ms = sys.argv[2], sys.argv[3]
        n = int(sys.argv[4]) if len(sys.argv) > 4 else 6
        os.environ["HIPIE_GEMM_MFMA"] = ms
        fn = {c[0].split()[0] + ("_f32" if "f32" in c[0] else "_win" if "gathered" in c[0] else ""): c[3] for c in cases()}[name]
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return
    rounds = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    n = max(50, int(sys.argv[2])) if len(sys.argv) > 2 else 50
    print("lib: %s   rounds %d x %d launches, random operands" % (os.environ.get("HIPIE_LIB_PATH", "(in-tree)"), rounds, n), flush=True)
    for name, N, K, fn in cases():
        t = {"32": [], "16": []}
        for ms in ("32", "16"):                       # warm-up of both instances
            os.environ["HIPIE_GEMM_MFMA"] = ms
            timed(fn, 10)
        for _ in range(rounds):
            for ms in ("32", "16"):
                os.environ["HIPIE_GEMM_MFMA"] = ms
                t[ms].append(timed(fn, n))
        med = {k: statistics.median(v) for k, v in t.items()}
        lo = {k: min(v) for k, v in t.items()}
        tf = 6.0 * M * N * K / 1e9
        print("%-13s N=%4d K=%4d  32x32x16: median %.4f min %.4f ms (%4.0f TF)   16x16x32: median %.4f min %.4f ms (%4.0f TF)   "
              "ratio of medians %.3f   16 median < 32 min: %s" % (name, N, K, med["32"], lo["32"], tf / med["32"], med["16"], lo["16"],
                                                                    tf / med["16"], med["32"] / med["16"], med["16"] < lo["32"]), flush=True)


if __name__ == "__main__":
    main()
