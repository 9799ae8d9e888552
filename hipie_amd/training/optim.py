"""Gradient clipping + AdamW as two passes over memory on the device (csrc/optim_step.hip): what torch.nn.utils.clip_grad_norm_ followed by
torch.optim.AdamW.step() do at the end of train_iteration (the reference: FullModelGradientClippingOptimizer over torch.optim.AdamW,
projects/HIPIE/train_net.py:167-244), opt-in.

  HipAdamW(params or groups, lr, betas, eps, weight_decay)    up to 8 groups with their own lr / weight_decay, one (betas, eps) for all
  .clip_and_step(max_norm, grad_scale, write_grads)           -> the gradient norm before clipping (0-dim device tensor), None without clipping
  .step()                                                     == clip_and_step(None)

The clipped gradients are never written (write_grads=True writes them, for whoever logs them): the clip coefficient is a scalar of the update
pass.  A call makes no host wait.  The norm is a float64 sum in a fixed order: the same bits from call to call and from rank to rank.

State.  exp_avg and exp_avg_sq live in one flat buffer each, `state[p]` holds views of it under torch's names and shapes; the step count is PER
PARAMETER as in torch (a parameter without a gradient in some iteration lags) and lives on the device -- `state[p]["step"]` is refreshed from it
when state_dict() is called, never during a step.  state_dict() / load_state_dict() interchange with torch.optim.AdamW in both directions.

The kernels take ADDRESSES: a table with one record per parameter (p, grad, exp_avg, exp_avg_sq, numel, group) on the device.  Every call collects
the addresses of the tensors that are alive NOW (a gradient of None is a null record, a non-contiguous gradient is copied for the step), holds
those tensors until the kernels are enqueued, and uploads the table only when an address differs from the last upload -- with GradientBuckets
(gradients are views into flat buffers) never after the first step, with zero_grad(set_to_none=True) whenever the allocator hands out other
blocks.  A table that matches was built from the same addresses, and the tensors at those addresses are the ones held: no stale address is ever
launched.  The upload goes through a fresh pinned buffer per upload (torch's pinned allocator does not hand a block out again before the copy
that reads it has run) and a non-blocking copy on the launch stream.

`kernels`: the object that runs the two passes, grad_norm(plan, grad_scale) and adamw_update(plan, norm, max_norm, grad_scale, write_grads) over a
StepPlan.  The default runs the HIP entries through hipie_amd.ops; a test passes a plain-torch stand-in (tests/_optim_cases.py)."""
import numpy as np
import torch


class StepPlan(object):
    """what one clip_and_step hands to the kernel layer.  Device side: table (n_seg, 6) int64 -- the records {p, g, m, v addresses, numel,
    group} --, cmap (n_chunks, 2) int64, steps (n_seg,) int32, bc (n_seg, 2) fp32, ws (uint8).  Host side: segments [(p, grad | None, exp_avg,
    exp_avg_sq, group index)] in table order, group_lr, group_wd, betas, eps."""
    __slots__ = ("table", "cmap", "steps", "bc", "ws", "segments", "group_lr", "group_wd", "betas", "eps")


class HipKernels(object):
    """the two passes on the hand-written kernels"""

    def grad_norm(self, plan, grad_scale):
        from .. import ops
        return ops.optim_grad_norm(plan.table, plan.cmap, grad_scale, ws=plan.ws)

    def adamw_update(self, plan, norm, max_norm, grad_scale, write_grads):
        from .. import ops
        ops.optim_adamw_step(plan.table, plan.cmap, plan.steps, plan.bc, plan.group_lr, plan.group_wd, plan.betas, plan.eps, norm=norm,
                             max_norm=0.0 if norm is None else max_norm, grad_scale=grad_scale, write_grads=write_grads)


MAX_GROUPS = 8


class HipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, kernels=None):
        if not 0.0 <= lr:
            raise ValueError("HipAdamW: lr=%r is negative" % (lr,))
        self._built = False
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize))
        self._built = True
        self.kernels = HipKernels() if kernels is None else kernels
        self._check_groups()
        self._params = [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        if not self._params:
            raise ValueError("HipAdamW: no parameters")
        dev = self._params[0][0].device
        for p, _ in self._params:
            if p.dtype != torch.float32:
                raise ValueError("HipAdamW: fp32 parameters only, got %s" % p.dtype)
            if not p.is_contiguous():
                raise ValueError("HipAdamW: a parameter of shape %s is not contiguous" % (tuple(p.shape),))
            if p.device != dev:
                raise ValueError("HipAdamW: parameters on more than one device (%s, %s)" % (dev, p.device))
        self.device = dev
        # the moments: one flat buffer each, every tensor on a 16-byte boundary of it
        numels = self._numels = [p.numel() for p, _ in self._params]
        starts, at = [], 0
        for n in numels:
            starts.append(at)
            at += (n + 3) // 4 * 4
        self._exp_avg = torch.zeros(max(at, 4), dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(max(at, 4), dtype=torch.float32, device=dev)
        self._m = [self._exp_avg[s:s + n].view_as(p) for s, n, (p, _) in zip(starts, numels, self._params)]
        self._v = [self._exp_avg_sq[s:s + n].view_as(p) for s, n, (p, _) in zip(starts, numels, self._params)]
        n_seg = len(self._params)
        self._steps = torch.zeros(n_seg, dtype=torch.int32, device=dev)
        self._bc = torch.ones(n_seg, 2, dtype=torch.float32, device=dev)
        for i, (p, _) in enumerate(self._params):
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": self._m[i], "exp_avg_sq": self._v[i]}
        # the chunk map: a function of the sizes alone
        chunk = self._chunk()
        per = [(n + chunk - 1) // chunk for n in numels]
        cmap = np.empty((sum(per), 2), dtype=np.int64)
        cmap[:, 0] = np.repeat(np.arange(n_seg, dtype=np.int64), per)
        cmap[:, 1] = np.concatenate([np.arange(k, dtype=np.int64) for k in per] or [np.empty(0, np.int64)]) * chunk
        self._cmap = torch.from_numpy(cmap).to(dev)
        self._ws = torch.empty(max(8 * cmap.shape[0], 8), dtype=torch.uint8, device=dev)
        # the segment table: the host copy keeps the columns that never change, the device copy is what the kernels read
        self._host_table = np.zeros((n_seg, 6), dtype=np.int64)
        self._host_table[:, 2] = [m.data_ptr() for m in self._m]
        self._host_table[:, 3] = [v.data_ptr() for v in self._v]
        self._host_table[:, 4] = numels
        self._host_table[:, 5] = [gi for _, gi in self._params]
        self._table = torch.zeros(n_seg, 6, dtype=torch.int64, device=dev)
        self._table_key = None
        self.table_uploads = 0

    def _chunk(self):
        if self.device.type == "cuda":
            from .. import ops
            return ops.optim_chunk()
        return 16384                                             # a stand-in kernel layer on the host: the map is built all the same

    def _check_groups(self):
        gs = self.param_groups
        if len(gs) > MAX_GROUPS:
            raise ValueError("HipAdamW: %d parameter groups, at most %d" % (len(gs), MAX_GROUPS))
        for g in gs:
            if g.get("amsgrad"):
                raise ValueError("HipAdamW: amsgrad is not supported")
            if g.get("maximize"):
                raise ValueError("HipAdamW: maximize is not supported")
            if tuple(g["betas"]) != tuple(gs[0]["betas"]) or g["eps"] != gs[0]["eps"]:
                raise ValueError("HipAdamW: one (betas, eps) for all groups, got %r / %r and %r / %r" % (gs[0]["betas"], gs[0]["eps"], g["betas"], g["eps"]))
            b1, b2 = g["betas"]
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not g["eps"] > 0.0 or not g["weight_decay"] >= 0.0 or not g["lr"] >= 0.0:
                raise ValueError("HipAdamW: betas %r in [0, 1), eps %r > 0, weight_decay %r >= 0, lr %r >= 0 needed" % (g["betas"], g["eps"], g["weight_decay"], g["lr"]))

    def add_param_group(self, group):
        if self._built:
            raise ValueError("HipAdamW: the parameter groups are fixed at construction (the moment buffers and the chunk map are built from them)")
        super().add_param_group(group)

    # ---- the step ----------------------------------------------------------------------------------------------------------------------
    def _collect(self):
        """the tensors of this step and their addresses: ([(p, g | None, m, v, group)], [tensors to hold], key, [(grad, contiguous copy)])"""
        segs, key, copies = [], [], []
        for i, (p, gi) in enumerate(self._params):
            g = p.grad
            if g is not None:
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise RuntimeError("HipAdamW: the gradient of a %s parameter is %s %s on %s: dense fp32 of the parameter's shape and device needed"
                                       % (tuple(p.shape), "sparse" if g.is_sparse else g.dtype, tuple(g.shape), g.device))
                if not g.is_contiguous():
                    c = g.contiguous()
                    copies.append((g, c))
                    g = c
            if p.numel() != self._numels[i] or not p.is_contiguous():
                raise RuntimeError("HipAdamW: a parameter changed its size or layout after construction")
            segs.append((p, g, self._m[i], self._v[i], gi))
            key.append(p.data_ptr())
            key.append(0 if g is None or g.numel() == 0 else g.data_ptr())
        return segs, tuple(key), copies

    def _upload(self, key):
        t = self._host_table
        t[:, 0:2] = np.asarray(key, dtype=np.int64).reshape(-1, 2)
        host = torch.from_numpy(t)
        if self.device.type == "cuda":
            stage = torch.empty(t.shape, dtype=torch.int64, pin_memory=True)      # a fresh pinned block per upload (see the module docstring)
            stage.copy_(host)
            self._table.copy_(stage, non_blocking=True)
        else:
            self._table.copy_(host)
        self._table_key = key
        self.table_uploads += 1

    @torch.no_grad()
    def clip_and_step(self, max_norm=None, grad_scale=1.0, write_grads=False):
        """g' = grad_scale x g, clipped to a total norm of max_norm (None: not clipped); AdamW with g'.  Returns the norm of grad_scale x g before
        clipping as a 0-dim device tensor, or None without clipping.  .grad keeps the unclipped gradients unless write_grads."""
        self._check_groups()
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError("HipAdamW: max_norm=%r is negative" % (max_norm,))
        segs, key, copies = self._collect()                      # `segs` holds every tensor whose address is in the table until the return below
        if key != self._table_key:
            self._upload(key)
        plan = StepPlan()
        plan.table, plan.cmap, plan.steps, plan.bc, plan.ws, plan.segments = self._table, self._cmap, self._steps, self._bc, self._ws, segs
        plan.group_lr = [float(g["lr"]) for g in self.param_groups]
        plan.group_wd = [float(g["weight_decay"]) for g in self.param_groups]
        plan.betas, plan.eps = tuple(float(b) for b in self.param_groups[0]["betas"]), float(self.param_groups[0]["eps"])
        norm = None if max_norm is None else self.kernels.grad_norm(plan, float(grad_scale))
        self.kernels.adamw_update(plan, norm, None if max_norm is None else float(max_norm), float(grad_scale), bool(write_grads))
        if write_grads:
            for g, c in copies:
                g.copy_(c)
        self._opt_called = True                                  # what torch's LR schedulers look at to see that the optimizer stepped first
        return norm

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.clip_and_step(None)
        return loss

    # ---- state -------------------------------------------------------------------------------------------------------------------------
    def steps(self):
        """the per-parameter step counts, read from the device (a host wait): a list of ints in the order of the parameters group by group"""
        return [int(s) for s in self._steps.tolist()]

    def state_dict(self):
        """torch.optim.AdamW's state dictionary: a parameter that never took a step has no entry, as there"""
        counts = self.steps()
        for (p, _), n in zip(self._params, counts):
            self.state[p]["step"] = torch.tensor(float(n))
        sd = super().state_dict()
        sd["state"] = {k: v for k, v in sd["state"].items() if float(v["step"]) > 0}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)                      # torch's own checks of the groups; the loaded tensors are copies
        self._check_groups()
        counts = []
        for i, (p, _) in enumerate(self._params):
            st = self.state.get(p, {})
            if "exp_avg" in st:
                if "max_exp_avg_sq" in st:
                    raise ValueError("HipAdamW: the state holds amsgrad's max_exp_avg_sq")
                self._m[i].copy_(st["exp_avg"])
                self._v[i].copy_(st["exp_avg_sq"])
                counts.append(int(round(float(st["step"]))))
            else:
                self._m[i].zero_()
                self._v[i].zero_()
                counts.append(0)
            self.state[p] = {"step": torch.tensor(float(counts[-1])), "exp_avg": self._m[i], "exp_avg_sq": self._v[i]}
        self._steps.copy_(torch.tensor(counts, dtype=torch.int32))
        b1, b2 = (float(b) for b in self.param_groups[0]["betas"])
        t = torch.tensor(counts, dtype=torch.float64)
        self._bc.copy_(torch.stack([1.0 - b1 ** t, (1.0 - b2 ** t).sqrt()], 1).float())      # rewritten by the next step of each parameter anyway
