"""Shared by tests/test_optim_step_cpu.py and tests/test_gpu_optim_step.py: the plain-torch stand-in for HipAdamW's kernel layer, the two references
(torch's own single-tensor path and a float64 restatement of the formulas) and the error measures.

    python tests/_optim_cases.py        prints the yardsticks of tests/test_gpu_optim_step.py (torch's fp32 path against float64, on the CPU)
"""
import os
import sys

import torch

CHUNK = 16384                                    # hipie_optim_chunk(); the GPU tests assert it


class TorchKernels(object):
    """HipAdamW's two passes with torch's own single-tensor operation sequence (torch/optim/adam.py _single_tensor_adam with decoupled weight
    decay; torch/nn/utils/clip_grad.py without foreach), on whatever device the tensors are: what the result must EQUAL on the CPU."""

    def grad_norm(self, plan, grad_scale):
        grads = [g if grad_scale == 1.0 else g * grad_scale for _, g, _, _, _ in plan.segments if g is not None]
        if not grads:
            return torch.zeros((), device=plan.steps.device)
        return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in grads]), 2.0)

    def adamw_update(self, plan, norm, max_norm, grad_scale, write_grads):
        coef = None if norm is None else torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        b1, b2 = plan.betas
        for i, (p, g, m, v, gi) in enumerate(plan.segments):
            if g is None:
                continue
            lr, wd = plan.group_lr[gi], plan.group_wd[gi]
            if grad_scale != 1.0:
                g = g.mul_(grad_scale) if write_grads else g * grad_scale
            if coef is not None:
                g = g.mul_(coef) if write_grads else g * coef
            plan.steps[i] += 1
            step = int(plan.steps[i])
            if wd != 0:
                p.mul_(1 - lr * wd)
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
            denom = (v.sqrt() / (bc2 ** 0.5)).add_(plan.eps)
            p.addcdiv_(m, denom, value=-(lr / bc1))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
# the smallest sizes that reach every path of the kernels: a lone element, less than a group of four, around a pass of the workgroup (256 threads),
# around one chunk, more than two chunks with a ragged tail, a matrix; entry NO_GRAD never has a gradient
SHAPES = [(1,), (3,), (255,), (256,), (257,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), (2 * CHUNK + 5,), (33, 129), (7,)]
NO_GRAD = len(SHAPES) - 1
GROUP_OF = [i % 2 for i in range(len(SHAPES))]                       # two groups, alternating
LRS, WD, BETAS, EPS = (1e-2, 1e-3), 0.1, (0.9, 0.999), 1e-8
MAX_NORM = 1.0
GRAD_AMP = (1.0, 1e-3, 0.3)                                          # per step: the norm is far above MAX_NORM, far below it, above it
STEPS = 3


def make_case(seed=20, shapes=SHAPES, steps=STEPS, amps=GRAD_AMP):
    """fp32 CPU inputs: parameters ~ N(0, 1) and `steps` gradient sets, set s ~ amps[s] x N(0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) * amps[k] for s in shapes] for k in range(steps)]
    return params, grads


def groups_of(params, group_of=GROUP_OF, lrs=LRS, wd=WD):
    return [{"params": [p for p, g in zip(params, group_of) if g == gi], "lr": lr, "weight_decay": wd} for gi, lr in enumerate(lrs)]


def run_torch(params, grads, max_norm=MAX_NORM, no_grad=(NO_GRAD,), device="cpu", lr_at=None, **opt_kw):
    """torch's own path: clip_grad_norm_ + torch.optim.AdamW on copies of the inputs -> per step (norm, [p], [exp_avg], [exp_avg_sq]) on the CPU;
    entries without state are None.  lr_at: {step index: (lr of group 0, lr of group 1)} set before that step."""
    ps = [torch.nn.Parameter(p.clone().to(device)) for p in params]
    kw = dict(foreach=False) if not opt_kw else opt_kw
    opt = torch.optim.AdamW(groups_of(ps), betas=BETAS, eps=EPS, **kw)
    out = []
    for k, gs in enumerate(grads):
        for gi, lr in enumerate((lr_at or {}).get(k, ())):
            opt.param_groups[gi]["lr"] = lr
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if i in no_grad else g.clone().to(device)
        with_grad = [p for p in ps if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(with_grad, max_norm, foreach=kw.get("foreach")) if max_norm is not None else None
        opt.step()
        st = [opt.state.get(p, {}) for p in ps]
        out.append((None if norm is None else norm.detach().cpu().clone(), [p.detach().cpu().clone() for p in ps],
                    [s["exp_avg"].cpu().clone() if s else None for s in st], [s["exp_avg_sq"].cpu().clone() if s else None for s in st]))
    return out


def run_f64(params, grads, max_norm=MAX_NORM, no_grad=(NO_GRAD,), lr_at=None, device="cpu"):
    """the truth: the formulas of the kernel's contract in float64 on the same fp32 inputs, state carried in float64 -> as run_torch (float64)"""
    ps = [p.to(device).double() for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    t = [0] * len(ps)
    b1, b2 = BETAS
    lrs = list(LRS)
    out = []
    for k, gs in enumerate(grads):
        lrs = list((lr_at or {}).get(k, lrs))
        gs = [None if i in no_grad else g.to(device).double() for i, g in enumerate(gs)]
        norm, c = None, 1.0
        if max_norm is not None:
            norm = torch.sqrt(sum((g * g).sum() for g in gs if g is not None))
            c = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        for i, g in enumerate(gs):
            if g is None:
                continue
            lr = lrs[GROUP_OF[i]]
            t[i] += 1
            g = c * g
            ps[i] = ps[i] * (1 - lr * WD)
            ms[i] = b1 * ms[i] + (1 - b1) * g
            vs[i] = b2 * vs[i] + (1 - b2) * g * g
            bc1, bc2 = 1 - b1 ** t[i], 1 - b2 ** t[i]
            ps[i] = ps[i] - (lr / bc1) * ms[i] / (vs[i].sqrt() / bc2 ** 0.5 + EPS)
        out.append((None if norm is None else norm.cpu(), [p.cpu() for p in ps], [m.cpu() if t[i] else None for i, m in enumerate(ms)],
                    [v.cpu() if t[i] else None for i, v in enumerate(vs)]))
    return out


def tables(ps, gs, ms, vs, group_of, chunk=CHUNK):
    """the segment table and the chunk map of ops.optim_grad_norm / optim_adamw_step for lists of device tensors (gs entries may be None), built
    by hand: (table (n, 6) int64, cmap (chunks, 2) int64) on the tensors' device.  The caller keeps the tensors alive."""
    rows = [[p.data_ptr(), 0 if g is None else g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi] for p, g, m, v, gi in zip(ps, gs, ms, vs, group_of)]
    cmap = [[i, off] for i, p in enumerate(ps) for off in range(0, p.numel(), chunk)]
    dev = ps[0].device
    return torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(cmap, dtype=torch.int64).reshape(-1, 2).to(dev)


def views_at(tensors, residues=(1, 2, 3), device="cpu"):
    """copies of the tensors as views into ONE flat buffer (the layout of GradientBuckets), tensor i starting at an element offset that is
    residues[i % len] modulo 4: only 4-byte aligned"""
    starts, at = [], 0
    for i, t in enumerate(tensors):
        at += (residues[i % len(residues)] - at) % 4
        starts.append(at)
        at += t.numel()
    flat = torch.zeros(at + 4, dtype=torch.float32, device=device)
    out = []
    for s, t in zip(starts, tensors):
        v = flat[s:s + t.numel()].view(t.shape)
        v.copy_(t)
        out.append(v)
    return out


def tensor_err(got, want):
    """max |got - want| / max |want| of one tensor against the float64 truth"""
    d = (got.double() - want.double()).abs().max().item()
    return d / max(want.double().abs().max().item(), 1e-300)


def errors(result, truth):
    """the four distances of a run to the truth, each the worst over the steps (and the tensors): norm (relative), p, exp_avg, exp_avg_sq"""
    e = {"norm": 0.0, "p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    for (n, p, m, v), (tn, tp, tm, tv) in zip(result, truth):
        if tn is not None:
            e["norm"] = max(e["norm"], abs(float(n.double()) - float(tn)) / float(tn))
        for key, got, want in (("p", p, tp), ("exp_avg", m, tm), ("exp_avg_sq", v, tv)):
            for a, b in zip(got, want):
                if b is not None:
                    e[key] = max(e[key], tensor_err(a, b))
    return e


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    params, grads = make_case()
    print("YARDSTICK = %r" % errors(run_torch(params, grads), run_f64(params, grads)))
