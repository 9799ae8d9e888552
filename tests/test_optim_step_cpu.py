"""CPU: the optimizer-step entries (csrc/optim_step.hip) -- their ABI surface and host refusals -- and training/optim.py's HipAdamW around a
plain-torch stand-in for the kernel layer (tests/_optim_cases.py): everything but the kernels' arithmetic, which tests/test_gpu_optim_step.py pins.
With the stand-in the results must EQUAL torch's clip_grad_norm_(foreach=False) + torch.optim.AdamW(foreach=False)."""
import ctypes
import os
import re

import pytest
import torch

import _optim_cases as oc
from hipie_amd import _lib, ops
from hipie_amd.training import GradientBuckets, HipAdamW, build_optimizer, train_iteration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["hipie_optim_chunk", "hipie_optim_norm_ws_bytes", "hipie_optim_grad_norm", "hipie_optim_adamw_step"]


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_abi_surface():
    header = open(os.path.join(ROOT, "include", "hipie_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"\b(hipie_[a-z_0-9]+)\s*\(", code)
    at = [declared.index(n) for n in ENTRIES]
    assert at == sorted(at) and at[-1] - at[0] == len(ENTRIES) - 1                    # declared, together, in this order
    bound = list(_lib.SIGNATURES)                                                    # the binding lists them in the header's order, behind the same entry
    assert bound[bound.index(ENTRIES[0]):][:len(ENTRIES)] == ENTRIES and bound[bound.index(ENTRIES[0]) - 1] == declared[at[0] - 1]
    lib = _lib.load()
    for n in ENTRIES:
        assert hasattr(lib, n), n
    assert lib.hipie_version() == 13
    assert lib.hipie_optim_norm_ws_bytes.restype is ctypes.c_int64
    makefile = open(os.path.join(ROOT, "hipie_amd", "csrc", "Makefile")).read()
    assert "optim_step.hip" in re.search(r"^SRCS\s*=\s*(.+)$", makefile, re.M).group(1).split()
    comment = header[header.index("csrc/optim_step.hip"):header.index("int hipie_optim_chunk")]
    for cite in ("torch.nn.utils.clip_grad_norm_", "torch.optim.AdamW", "projects/HIPIE/train_net.py:189-239", "FullModelGradientClippingOptimizer.step"):
        assert cite in comment, cite
    assert lib.hipie_optim_chunk() == oc.CHUNK == ops.optim_chunk()


def _step(lib, table=256, n_seg=2, cmap=512, n_chunks=3, steps=768, bc=1024, lr=(1e-3,), wd=(0.0,), n_groups=None, betas=(0.9, 0.999), eps=1e-8, norm=1280,
          max_norm=0.1):
    p = lambda a: None if a is None else ctypes.c_void_p(a)
    arr = lambda xs: None if xs is None else (ctypes.c_double * max(len(xs), 1))(*xs)
    return lib.hipie_optim_adamw_step(p(table), n_seg, p(cmap), n_chunks, p(steps), p(bc), arr(lr), arr(wd), len(lr) if n_groups is None else n_groups,
                                      betas[0], betas[1], eps, p(norm), max_norm, 1.0, 0, None)


def _norm(lib, table=256, n_seg=2, cmap=512, n_chunks=3, ws=768, ws_bytes=24, norm=1280):
    p = lambda a: None if a is None else ctypes.c_void_p(a)
    return lib.hipie_optim_grad_norm(p(table), n_seg, p(cmap), n_chunks, p(ws), ws_bytes, 1.0, p(norm), None)


def test_host_refusals():
    """every refusal is made on the host, before a launch, with fake addresses; the message names the entry and the condition"""
    lib = _lib.load()

    def refused(rc, word):
        msg = lib.hipie_last_error()
        assert rc == -22 and word in msg and (b"optim_adamw_step" in msg or b"optim_grad_norm" in msg), (rc, msg)
    refused(_norm(lib, table=None), b"null")
    refused(_norm(lib, cmap=None), b"null")
    refused(_norm(lib, ws=None), b"null")
    refused(_norm(lib, norm=None), b"null")
    refused(_norm(lib, n_seg=-1), b"negative")
    refused(_norm(lib, n_chunks=-1), b"negative")
    refused(_norm(lib, ws_bytes=23), b"workspace")
    refused(_norm(lib, ws=772), b"workspace")
    refused(_step(lib, table=None), b"null")
    refused(_step(lib, cmap=None), b"null")
    refused(_step(lib, steps=None), b"null")
    refused(_step(lib, bc=None), b"null")
    refused(_step(lib, lr=None, n_groups=1), b"null")
    refused(_step(lib, n_seg=-2), b"negative")
    refused(_step(lib, n_chunks=-2), b"negative")
    refused(_step(lib, n_groups=-1), b"negative")
    refused(_step(lib, lr=(1e-3,) * 9, wd=(0.0,) * 9), b"9 groups")
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, float("nan"))):
        refused(_step(lib, betas=betas), b"betas")
    refused(_step(lib, eps=0.0), b"eps")
    refused(_step(lib, eps=-1e-8), b"eps")
    refused(_step(lib, max_norm=-0.5), b"max_norm")
    refused(_step(lib, max_norm=float("nan")), b"max_norm")
    # nothing to do: 0 without a launch, null pointers allowed
    assert _norm(lib, table=None, cmap=None, ws=None, norm=None, n_seg=0, n_chunks=0) == 0
    assert _step(lib, table=None, cmap=None, steps=None, bc=None, n_seg=0, n_chunks=0) == 0
    assert _step(lib, n_chunks=0) == 0 and _norm(lib, n_seg=0) == 0
    # the workspace query grows with the chunks and is never 0
    sizes = [lib.hipie_optim_norm_ws_bytes(n) for n in (-1, 0, 1, 2, 3, 2048, 2049, 1 << 20)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[3] < sizes[4] < sizes[5] < sizes[6] < sizes[7] and sizes[2] >= 8


def test_ops_refuse_cpu_tensors():
    table, cmap = torch.zeros(2, 6, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.optim_grad_norm(table, cmap)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.optim_adamw_step(table, cmap, torch.zeros(2, dtype=torch.int32), torch.ones(2, 2), [1e-3], [0.0], (0.9, 0.999), 1e-8)
    with pytest.raises(RuntimeError, match="table must be"):
        ops.optim_grad_norm(torch.zeros(2, 5, dtype=torch.int64), cmap)


# ---- HipAdamW around the stand-in ---------------------------------------------------------------------------------------------------------------
SHAPES = [(5,), (4, 3), (17,), (2, 2, 2), (1,)]
GROUP_OF = [0, 1, 0, 1, 0]
LAGS = 2                                         # this parameter has no gradient in step 2


def _case(steps=3, seed=3):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=gen) for s in SHAPES]
    amps = (3.0, 1e-2, 1.0, 0.5)
    grads = [[torch.randn(s, generator=gen) * amps[k] for s in SHAPES] for k in range(steps)]
    return params, grads


def _groups(ps):
    return [{"params": [p for p, g in zip(ps, GROUP_OF) if g == 0], "lr": 1e-2, "weight_decay": 0.1},
            {"params": [p for p, g in zip(ps, GROUP_OF) if g == 1], "lr": 3e-3, "weight_decay": 0.02}]


def _set_grads(ps, gs, k, scale=1.0):
    for i, (p, g) in enumerate(zip(ps, gs)):
        p.grad = None if (i == LAGS and k == 1) else g.clone() * scale


def _both(params):
    a = [torch.nn.Parameter(p.clone()) for p in params]
    b = [torch.nn.Parameter(p.clone()) for p in params]
    return a, torch.optim.AdamW(_groups(a), foreach=False), b, HipAdamW(_groups(b), kernels=oc.TorchKernels())


def _hip_steps(opt, ps):
    """HipAdamW.steps() (group by group) in the order of the list ps"""
    by_id = dict(zip([id(p) for g in opt.param_groups for p in g["params"]], opt.steps()))
    return [by_id[id(p)] for p in ps]


def _torch_step(ps, opt, max_norm):
    with_grad = [p for p in ps if p.grad is not None]
    norm = torch.nn.utils.clip_grad_norm_(with_grad, max_norm, foreach=False) if max_norm is not None else None
    opt.step()
    return norm


def _assert_same_state(pa, oa, pb, ob):
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        sa, sb = oa.state.get(a, {}), ob.state[b]
        if sa:
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
            assert sb["exp_avg"].shape == b.shape and sb["exp_avg_sq"].shape == b.shape
        else:
            assert not sb["exp_avg"].any() and not sb["exp_avg_sq"].any()


@pytest.mark.parametrize("max_norm", [1.0, None])
def test_three_steps_equal_torch(max_norm):
    params, grads = _case()
    pa, oa, pb, ob = _both(params)
    for k in range(3):
        _set_grads(pa, grads[k], k)
        _set_grads(pb, grads[k], k)
        before = [t.clone() for t in (pb[LAGS], ob.state[pb[LAGS]]["exp_avg"], ob.state[pb[LAGS]]["exp_avg_sq"])]
        na, nb = _torch_step(pa, oa, max_norm), ob.clip_and_step(max_norm)
        if max_norm is None:
            assert nb is None
        else:
            assert nb.dim() == 0 and torch.equal(na, nb)
            assert (float(na) > max_norm) == (k != 1)            # both sides of the clamp are taken
        if k == 1:                                               # no gradient: untouched, and its count lags from here on
            after = (pb[LAGS], ob.state[pb[LAGS]]["exp_avg"], ob.state[pb[LAGS]]["exp_avg_sq"])
            assert all(torch.equal(x, y) for x, y in zip(before, after))
        _assert_same_state(pa, oa, pb, ob)
    assert _hip_steps(ob, pb) == [3, 3, 2, 3, 3] == [int(oa.state[p]["step"]) for p in pa]
    sd = ob.state_dict()
    assert [float(sd["state"][i]["step"]) for i in range(5)] == [float(oa.state_dict()["state"][i]["step"]) for i in range(5)]


def test_step_is_clip_and_step_without_clipping():
    params, grads = _case(1)
    pa, oa, pb, ob = _both(params)
    _set_grads(pa, grads[0], 0)
    _set_grads(pb, grads[0], 0)
    oa.step()
    assert ob.step() is None
    assert float(ob.step(lambda: torch.tensor(2.5))) == 2.5      # the closure's loss is handed back
    oa.step()
    _assert_same_state(pa, oa, pb, ob)


def test_grad_scale_equals_halving_the_gradients():
    params, grads = _case(2)
    pa, _, pb, ob = _both(params)
    oa = HipAdamW(_groups(pa), kernels=oc.TorchKernels())
    for k in range(2):
        _set_grads(pa, grads[k], k, scale=0.5)
        _set_grads(pb, grads[k], k)
        na, nb = oa.clip_and_step(1.0), ob.clip_and_step(1.0, grad_scale=0.5)
        assert torch.equal(na, nb)
        _assert_same_state(pa, oa, pb, ob)


def test_write_grads():
    params, grads = _case(1)
    pa, oa, pb, ob = _both(params)
    pc = [torch.nn.Parameter(p.clone()) for p in params]
    oc_ = HipAdamW(_groups(pc), kernels=oc.TorchKernels())
    for ps in (pa, pb, pc):
        _set_grads(ps, grads[0], 0)
    pc[1].grad = pc[1].grad.t().contiguous().t()                  # a non-contiguous gradient: copied for the step, written back
    assert not pc[1].grad.is_contiguous()
    _torch_step(pa, oa, 1.0)
    ob.clip_and_step(1.0)
    oc_.clip_and_step(1.0, write_grads=True)
    for a, b, c, g in zip(pa, pb, pc, grads[0]):
        assert torch.equal(b.grad, g)                            # the default leaves the gradients as they were
        assert torch.equal(c.grad, a.grad) and not torch.equal(c.grad, g)
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("direction", ["torch_to_hip", "hip_to_torch"])
def test_state_dict_interchange(direction):
    params, grads = _case(3)
    pa, oa, pb, ob = _both(params)                               # a: torch throughout;  b: two steps of one kind, then one of the other
    src, dst_ps = (torch.optim.AdamW(_groups(pb), foreach=False), pb) if direction == "torch_to_hip" else (ob, pb)
    for k in range(2):
        _set_grads(pa, grads[k], k)
        _set_grads(pb, grads[k], k)
        _torch_step(pa, oa, 1.0)
        if direction == "torch_to_hip":
            _torch_step(pb, src, 1.0)
        else:
            src.clip_and_step(1.0)
    sd = src.state_dict()
    assert sorted(sd["state"]) == sorted(oa.state_dict()["state"])
    dst = HipAdamW(_groups(pb), kernels=oc.TorchKernels()) if direction == "torch_to_hip" else torch.optim.AdamW(_groups(pb), foreach=False)
    dst.load_state_dict(sd)
    _set_grads(pa, grads[2], 2)
    _set_grads(pb, grads[2], 2)
    na = _torch_step(pa, oa, 1.0)
    nb = dst.clip_and_step(1.0) if direction == "torch_to_hip" else _torch_step(pb, dst, 1.0)
    assert torch.equal(na, nb)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert torch.equal(oa.state[a]["exp_avg"], dst.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], dst.state[b]["exp_avg_sq"])
    want = [3, 3, 2, 3, 3]
    assert (_hip_steps(dst, pb) if direction == "torch_to_hip" else [int(dst.state[b]["step"]) for b in pb]) == want


def test_a_parameter_that_never_stepped_has_no_entry():
    params, grads = _case(1)
    _, _, pb, ob = _both(params)
    _set_grads(pb, grads[0], 0)
    pb[3].grad = None
    ob.clip_and_step(1.0)
    sd = ob.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]                    # the ids count group by group: parameters 0, 2, 4, then 1, 3
    pf = [torch.nn.Parameter(p.clone()) for p in params]
    fresh = HipAdamW(_groups(pf), kernels=oc.TorchKernels())
    fresh.load_state_dict(sd)
    assert _hip_steps(fresh, pf) == [1, 1, 1, 0, 1]


def test_class_refusals():
    p = lambda *s: torch.nn.Parameter(torch.zeros(*s))
    with pytest.raises(ValueError, match="amsgrad"):
        HipAdamW([p(3)], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        HipAdamW([p(3)], maximize=True)
    with pytest.raises(ValueError, match="betas"):
        HipAdamW([{"params": [p(3)]}, {"params": [p(3)], "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="eps"):
        HipAdamW([{"params": [p(3)]}, {"params": [p(3)], "eps": 1e-6}])
    with pytest.raises(ValueError, match="9 parameter groups"):
        HipAdamW([{"params": [p(2)]} for _ in range(9)])
    HipAdamW([{"params": [p(2)]} for _ in range(8)])
    with pytest.raises(ValueError, match="fp32"):
        HipAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(ValueError, match="contiguous"):
        HipAdamW([torch.nn.Parameter(torch.zeros(3, 4).t())])
    with pytest.raises(ValueError, match="betas"):
        HipAdamW([p(3)], betas=(1.0, 0.999))
    opt = HipAdamW([p(3)])
    with pytest.raises(ValueError, match="fixed at construction"):
        opt.add_param_group({"params": [p(2)]})
    with pytest.raises(ValueError, match="max_norm"):
        opt.clip_and_step(-1.0)


# ---- train_iteration ---------------------------------------------------------------------------------------------------------------------------
class _StubStep(object):
    def __init__(self, net):
        self.net = net

    def loss_dict(self, batched_inputs, targets, task):
        y = self.net(batched_inputs)
        return {"loss_a": ((y - targets) ** 2).sum(), "loss_b": y.abs().sum() * 0.5}


def _net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 9), torch.nn.Tanh(), torch.nn.Linear(9, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))


@pytest.mark.parametrize("with_buckets", [False, True])
def test_train_iteration(with_buckets):
    gen = torch.Generator().manual_seed(5)
    xs, ts = torch.randn(2, 4, 6, generator=gen), torch.randn(2, 4, 3, generator=gen)
    na, nb = _net(), _net()
    oa = torch.optim.AdamW(na.parameters(), lr=1e-2, weight_decay=0.1, foreach=False)
    ob = HipAdamW(nb.parameters(), lr=1e-2, weight_decay=0.1, kernels=oc.TorchKernels())
    ba = GradientBuckets(na.parameters()) if with_buckets else None
    bb = GradientBuckets(nb.parameters()) if with_buckets else None
    for k in range(2):
        la, norm_a = train_iteration(_StubStep(na), oa, xs[k], ts[k], buckets=ba, clip_norm=0.1)
        lb, norm_b = train_iteration(_StubStep(nb), ob, xs[k], ts[k], buckets=bb, clip_norm=0.1)
        assert torch.equal(norm_a, norm_b) and float(norm_a) > 0.1
        assert sorted(la) == sorted(lb) and all(torch.equal(la[n], lb[n]) for n in la)
    for a, b in zip(na.parameters(), nb.parameters()):
        assert torch.equal(a, b)
    if with_buckets:
        assert ob.table_uploads == 1                             # the gradients are views into the buckets: their addresses never change
    else:
        assert ob.table_uploads >= 1
    _, none = train_iteration(_StubStep(nb), ob, xs[0], ts[0], buckets=bb, clip_norm=0)
    assert none is None and ob.steps() == [3] * 6


def test_build_optimizer_hand():
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.detr = torch.nn.ModuleDict({"backbone": torch.nn.Sequential(torch.nn.Linear(3, 4)), "head": torch.nn.Linear(4, 2)})
            self.text_encoder = torch.nn.Linear(2, 2)
            self.frozen = torch.nn.Parameter(torch.zeros(2), requires_grad=False)
    model = Model()
    a, b = build_optimizer(model), build_optimizer(model, hand=True)
    assert isinstance(a, torch.optim.AdamW) and isinstance(b, HipAdamW)
    assert len(a.param_groups) == len(b.param_groups) == 2
    for ga, gb in zip(a.param_groups, b.param_groups):
        assert [id(p) for p in ga["params"]] == [id(p) for p in gb["params"]]
        assert ga["lr"] == gb["lr"] and ga["weight_decay"] == gb["weight_decay"] and tuple(ga["betas"]) == tuple(gb["betas"]) and ga["eps"] == gb["eps"]
    assert len(b.param_groups[1]["params"]) == 2 and b.param_groups[1]["lr"] == pytest.approx(1e-5)
    assert build_optimizer(model, base_lr=2e-4, hand=True).param_groups[0]["lr"] == 2e-4
