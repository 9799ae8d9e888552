#!/usr/bin/env python3
"""One MaskCriterion.loss_masks call and one loss_labels call (hipie_amd/training/criterion.py), forward + backward, in both formulations:
ops=None (torch: gather of the matched targets, two grid_sample launches, element-wise passes; boolean indexing with the text mask) and
ops=net.HipBackendLosses (csrc/point_loss.hip).  One process, the two sides alternated call by call; prints the median wall time of a
synchronised forward + backward and the peak memory above the inputs.
    python tools/bench_point_loss.py [reps]
BENCH_PLAIN_ATOMICS=1 with a study build of the library (make EXTRA=-DHIPIE_STUDY_KNOBS, HIPIE_LIB_PATH): a third side, the kernels with
one atomic per lane and corner in the backward instead of add_corner's merged form.
Geometries: N = 14 and 200 matched instances (2 images x 8 targets; 200 = the de-noising part, targets repeated), 256 x 256 predictions,
256 x 256 and 1024 x 1024 targets, P = 12544 points.  loss_labels: logits (2, 900, 256), half of the tokens padding."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hipie_amd.training import net  # noqa: E402
from hipie_amd.training.criterion import MaskCriterion  # noqa: E402

DEV = torch.device("cuda", 0)
PLAIN = os.environ.get("BENCH_PLAIN_ATOMICS") == "1"          # needs a library built with EXTRA=-DHIPIE_STUDY_KNOBS (HIPIE_LIB_PATH)


def timed(fn, leaf):
    """(seconds, peak bytes above what was allocated before the call) of one synchronised forward + backward"""
    leaf.grad = None
    os.environ.pop("HIPIE_POINT_LOSS_PLAIN", None)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    loss = fn()
    loss.backward()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base


def compare(tag, make, leaf, reps):
    """make(ops) -> closure returning the scalar loss; alternates ops=None and the kernels"""
    sides = {"torch": make(None), "hip": make(net.HipBackendLosses)}
    if PLAIN:                                                # study build: the backward with one atomic per lane and corner (no add_corner)
        hip = sides["hip"]

        def plain():
            os.environ["HIPIE_POINT_LOSS_PLAIN"] = "1"
            return hip()
        sides["hip_plain"] = plain
    res = {k: [] for k in sides}
    for it in range(reps + 3):                               # three untimed rounds: allocator pools, kernel load
        for k, fn in sides.items():
            r = timed(fn, leaf)
            if it >= 3:
                res[k].append(r)
    vals = {}
    for k, fn in sides.items():
        leaf.grad = None
        v = fn()
        v.backward()
        vals[k] = (float(v.detach()), leaf.grad.clone())
    dg = float((vals["hip"][1] - vals["torch"][1]).abs().max() / vals["torch"][1].abs().max())
    ms = {k: 1e3 * statistics.median(t for t, _ in v) for k, v in res.items()}
    lo = {k: 1e3 * min(t for t, _ in v) for k, v in res.items()}
    mem = {k: max(m for _, m in v) / 2 ** 20 for k, v in res.items()}
    if PLAIN:
        print("%-34s hip with plain atomics %8.3f ms (min %8.3f)" % (tag, ms["hip_plain"], lo["hip_plain"]))
    print("%-34s torch %8.3f ms (min %8.3f) peak %8.1f MiB | hip %8.3f ms (min %8.3f) peak %8.1f MiB | x%.2f | loss %.6f / %.6f, grad diff %.1e"
          % (tag, ms["torch"], lo["torch"], mem["torch"], ms["hip"], lo["hip"], mem["hip"], ms["torch"] / ms["hip"], vals["torch"][0], vals["hip"][0], dg))


def mask_case(N, size_t, P=12544, Q=300, n_tgt=8, size_p=256):
    g = torch.Generator().manual_seed(N + size_t)
    pred = (torch.randn(2, Q, size_p, size_p, generator=g) * 3).to(DEV).requires_grad_(True)
    targets = [{"masks": (torch.rand(n_tgt, size_t, size_t, generator=g) < 0.3).float().to(DEV)} for _ in range(2)]
    per = N // 2
    indices = [(torch.randperm(Q, generator=g)[:per], torch.arange(per) % n_tgt) for _ in range(2)]
    draw_g = torch.Generator(device=DEV)

    def make(ops):
        crit = MaskCriterion(80, None, ["masks"], vl_loss=True, num_points=P, ops=ops,
                             draw=lambda shape, device: torch.rand(tuple(shape), device=device, generator=draw_g))

        def run():
            draw_g.manual_seed(7)                            # the same points on both sides
            crit._padded = None                              # ONE call: the padded targets are built inside it on both sides
            out = crit.loss_masks({"pred_masks": pred}, targets, indices, float(2 * n_tgt))
            return out["loss_mask"] + out["loss_dice"]
        return run
    return make, pred


def label_case(Q=900, L=256, n_tgt=8):
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(2, Q, L, generator=g) * 2 - 2).to(DEV).requires_grad_(True)
    text_mask = torch.ones(2, L, dtype=torch.int64)
    text_mask[:, L // 2:] = 0
    text_mask = text_mask.to(DEV)
    targets = []
    for _ in range(2):
        pm = torch.zeros(n_tgt, L, dtype=torch.bool)
        for t in range(n_tgt):
            pm[t, 1 + 3 * t:3 + 3 * t] = True
        targets.append({"positive_map": pm.to(DEV)})
    indices = [(torch.randperm(Q, generator=g)[:n_tgt], torch.arange(n_tgt)) for _ in range(2)]

    def make(ops):
        crit = MaskCriterion(80, None, ["labels"], vl_loss=True, ops=ops)
        return lambda: crit.loss_labels({"pred_logits": logits, "text_masks": text_mask}, targets, indices, float(2 * n_tgt))["loss_ce"]
    return make, logits


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    print("median of %d synchronised forward + backward calls, the two sides alternated" % reps)
    for N in (14, 200):
        for size_t in (256, 1024):
            make, leaf = mask_case(N, size_t)
            compare("loss_masks N=%d tgt %d^2 P=12544" % (N, size_t), make, leaf, reps)
            del make, leaf
            torch.cuda.empty_cache()
    make, leaf = label_case()
    compare("loss_labels (2,900,256)", make, leaf, reps)


if __name__ == "__main__":
    main()
