#!/usr/bin/env python3
"""The tail of a training iteration behind backward() -- gradient clipping + AdamW -- on the trainable parameters of ViT-H (the shapes of
HIPIE_IMG(HipieConfig.vit_huge()), text encoder frozen), random gradients, timed per call and alternated in ONE process:

    torch         clip_grad_norm_(params, 0.1) + torch.optim.AdamW(fused=True).step()      what build_optimizer(model) gives
    hand, fresh   HipAdamW.clip_and_step(0.1), the gradient tensors at other addresses every call (zero_grad(set_to_none=True): a table upload per call)
    hand, views   the same with the gradients as views into GradientBuckets' flat buffers (stable addresses: no upload after the first call)
    norm, update  the two entries on their own (hipie_optim_grad_norm, hipie_optim_adamw_step with the norm of the former)

Device time from events around the call, host time = the wall clock of the call itself (the enqueue; nothing waits), launches and host waits of
one call from the profiler and torch's sync debug mode, GB/s against the 32 bytes per parameter the two passes have to move (norm: 4, update: 28).
    python tools/bench_optim_step.py [--rounds N] [--iteration]
--iteration: also train_iteration (tools/bench_train_step.py's batch) with build_optimizer(model) and build_optimizer(model, hand=True), three
alternated passes each after two untimed ones."""
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import bench  # noqa: E402
from hipie_amd import ops  # noqa: E402
from hipie_amd.config import HipieConfig, Precision  # noqa: E402
from hipie_amd.hipie_img import HIPIE_IMG  # noqa: E402
from hipie_amd.training import GradientBuckets, HipAdamW, TrainStep, build_optimizer, train_iteration  # noqa: E402

CLIP = 0.1
PEAK_GBS = 6300.0                                # what a streaming kernel reaches on this chip


def timed(fn):
    """(device ms, host ms) of one call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), 1e3 * (t1 - t0)


def counts(fn):
    """(device launches, host waits) of one call"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen, profile(activities=[ProfilerActivity.CUDA]) as prof:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA), sum(1 for w in seen if "synchroniz" in str(w.message).lower())


def copies_of(shapes, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]


def random_grads(ps, seed):
    gen = torch.Generator(device=ps[0].device).manual_seed(seed)
    return [torch.randn(p.shape, device=p.device, generator=gen) * 1e-3 for p in ps]


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 10
    dev = torch.device("cuda", 0)
    cfg = HipieConfig.vit_huge()
    torch.manual_seed(0)
    model = HIPIE_IMG(cfg, Precision.parity(), device=dev)
    for p in model.text_encoder.parameters():
        p.requires_grad_(False)
    groups = build_optimizer(model).param_groups
    shapes = [[tuple(p.shape) for p in g["params"]] for g in groups]
    lrs = [g["lr"] for g in groups]
    n_par = sum(p.numel() for g in groups for p in g["params"])
    n_tensors = sum(len(s) for s in shapes)
    if "--iteration" not in sys.argv:
        del model, groups
        torch.cuda.empty_cache()
    print("ViT-H trainable parameters: %d tensors, %.1f M elements, groups %s; floor at %.1f TB/s: %.2f ms (32 B per parameter)"
          % (n_tensors, n_par / 1e6, [len(s) for s in shapes], PEAK_GBS / 1e3, 32 * n_par / PEAK_GBS / 1e6))

    def build(kind):
        ps = [copies_of(s, dev) for s in shapes]
        spec = [{"params": p, "lr": lr} for p, lr in zip(ps, lrs)]
        flat = [p for g in ps for p in g]
        opt = torch.optim.AdamW(spec, lr=lrs[0], weight_decay=0.01, fused=True) if kind == "torch" else HipAdamW(spec, lr=lrs[0], weight_decay=0.01)
        return flat, opt

    # torch: its gradients stay where they are (clip_grad_norm_ rewrites them in place: from the second call on their norm is the clip value)
    tp, topt = build("torch")
    for p, g in zip(tp, random_grads(tp, 1)):
        p.grad = g

    def call_torch():
        torch.nn.utils.clip_grad_norm_(tp, CLIP)
        topt.step()

    # hand, fresh: two sets of gradient tensors, alternated
    fp, fopt = build("hand")
    fsets, turn = [random_grads(fp, 2), random_grads(fp, 3)], [0]

    def call_fresh():
        for p, g in zip(fp, fsets[turn[0] & 1]):
            p.grad = g
        turn[0] += 1
        fopt.clip_and_step(CLIP)

    # hand, views: GradientBuckets owns the gradients
    vp, vopt = build("hand")
    buckets = GradientBuckets(vp)
    for flat, _, _ in buckets.buckets:
        flat.copy_(torch.randn(flat.shape, device=dev) * 1e-3)

    def call_views():
        vopt.clip_and_step(CLIP)

    call_views()                                                 # builds the table the two entries are timed on
    norm_box = [None]

    def call_norm():
        norm_box[0] = ops.optim_grad_norm(vopt._table, vopt._cmap, ws=vopt._ws)

    def call_update():
        ops.optim_adamw_step(vopt._table, vopt._cmap, vopt._steps, vopt._bc, lrs, [0.01] * len(lrs), (0.9, 0.999), 1e-8, norm=norm_box[0], max_norm=CLIP)

    calls = [("torch", call_torch, 32), ("hand, fresh", call_fresh, 32), ("hand, views", call_views, 32), ("norm", call_norm, 4), ("update", call_update, 28)]
    for _, fn, _ in calls:                                       # warm up every path
        fn()
        fn()
    torch.cuda.synchronize()
    dev_ms, host_ms = {n: [] for n, _, _ in calls}, {n: [] for n, _, _ in calls}
    for _ in range(rounds):
        for name, fn, _ in calls:
            d, h = timed(fn)
            dev_ms[name].append(d)
            host_ms[name].append(h)
    print("table uploads: fresh %d in %d calls, views %d in %d calls" % (fopt.table_uploads, turn[0], vopt.table_uploads, rounds + 3))
    for name, fn, nbytes in calls:
        launches, waits = counts(fn)
        d = statistics.median(dev_ms[name])
        print("%-12s device %7.3f ms (min %7.3f, max %7.3f over %d), host %6.2f ms, %4d launches, %d host waits, %6.0f GB/s of %d B/parameter = %4.1f %% of %.1f TB/s"
              % (name, d, min(dev_ms[name]), max(dev_ms[name]), rounds, statistics.median(host_ms[name]), launches, waits, nbytes * n_par / d / 1e6, nbytes,
                 100 * nbytes * n_par / d / 1e6 / PEAK_GBS, PEAK_GBS / 1e3))

    if "--iteration" in sys.argv:
        from bench_train_step import targets_for
        bench.randomize_degenerate_inits(model)
        model.finalize()
        size, L, B = 1024, 194, 2
        batch = bench.synth_batch(cfg, B, size, 80, L, dev)
        targets = targets_for(B, 6, 2, size, L, dev)
        step = TrainStep(model)
        opts = [("build_optimizer(model)", build_optimizer(model)), ("build_optimizer(model, hand=True)", build_optimizer(model, hand=True))]
        times = {n: [] for n, _ in opts}
        for it in range(5):
            for name, opt in opts:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, norm = train_iteration(step, opt, batch, targets, clip_norm=CLIP)
                torch.cuda.synchronize()
                if it >= 2:
                    times[name].append(1e3 * (time.perf_counter() - t0))
        for name, _ in opts:
            print("train_iteration, ViT-H 1024^2, 2 images, %-34s %s ms (median %.1f)" % (name + ":", " ".join("%.1f" % t for t in times[name]), statistics.median(times[name])))
        print("last gradient norm %.4e" % float(norm))


if __name__ == "__main__":
    main()
