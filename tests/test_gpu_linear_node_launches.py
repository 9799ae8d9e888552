"""GPU: the library entry points one forward + backward of each training linear node reaches (functions.SplitLinearFunction /
ScaledSplitLinearFunction / HalfLinearFunction, MlpFunction / ScaledMlpFunction / HalfMlpFunction), recorded at ops._call.  The float64
tests of these nodes hold their results; this holds that a node did not gain (or lose) a pass.  The lists are literal: they were recorded
from the six hand-written bodies before the nodes were folded over the operand policies of functions.py."""
import pytest
import torch

from hipie_amd import ops
from hipie_amd.training import functions

pytestmark = pytest.mark.gpu
DEV = "cuda"

SPLIT_SHAPE = (300, 96, 160)          # (M, N, K): two chunks in every weight gradient
HALF_SHAPE = (300, 128, 192)          # one chunk (five 64-row groups): the product itself, no partial sums

GEMM, SCALED, BATCHED, FINISH = "hipie_gemm", "hipie_gemm_scaled", "hipie_gemm_batched", "hipie_splitk_finish"
T, GSCALE, GPACK, HPACK = "hipie_to_hl8_t", "hipie_grad_scale", "hipie_grad_pack", "hipie_half_pack"
ACT, ACT_BWD, ACT_HALF = "hipie_act_forward", "hipie_act_backward", "hipie_act_half"

# front door -> (the forward, the backward with everything trainable, the backward with x frozen), in launch order
LAUNCHES = {
    "split_linear": ([GEMM], [GEMM, T, T, BATCHED], [T, T, BATCHED]),
    "split_linear_scaled": ([GEMM], [GSCALE, GPACK, SCALED, T, BATCHED, FINISH], [GSCALE, GPACK, T, BATCHED, FINISH]),
    "half_linear": ([HPACK, GEMM], [GSCALE, HPACK, SCALED, HPACK, SCALED], [GSCALE, HPACK, HPACK, SCALED]),
    "split_mlp": ([GEMM, ACT, GEMM], [GEMM, ACT_BWD, T, T, BATCHED, T, T, BATCHED, GEMM], [GEMM, ACT_BWD, T, T, BATCHED, T, T, BATCHED]),
    "split_mlp_scaled": ([GEMM, ACT, GEMM],
                         [GSCALE, GPACK, SCALED, ACT_BWD, T, BATCHED, FINISH, GSCALE, GPACK, T, BATCHED, FINISH, SCALED],
                         [GSCALE, GPACK, SCALED, ACT_BWD, T, BATCHED, FINISH, GSCALE, GPACK, T, BATCHED, FINISH]),
    "half_mlp": ([HPACK, GEMM, ACT_HALF, GEMM],
                 [GSCALE, HPACK, SCALED, ACT_BWD, HPACK, SCALED, GSCALE, HPACK, HPACK, SCALED, SCALED],
                 [GSCALE, HPACK, SCALED, ACT_BWD, HPACK, SCALED, GSCALE, HPACK, HPACK, SCALED]),
}


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules of the suite switch autograd off for the whole process"""
    with torch.enable_grad():
        yield


def _recorded(monkeypatch, run):
    names = []
    real = ops._call
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_call", lambda name, *a: names.append(name) or real(name, *a))
        run()
    return names


@pytest.mark.parametrize("door", list(LAUNCHES))
def test_gpu_linear_node_launches(door, monkeypatch):
    """The ORDER is asserted for all six nodes: the shared graph kept each node's sequence of entry points.  (Library passes are not
    entry points: the unscaled nodes' db = dy.sum(0) now runs before the dx product instead of last.)  The first, unrecorded pass builds
    the cached copies of W and W^T."""
    want_fwd, want_all, want_frozen = LAUNCHES[door]
    mlp = door.endswith(("mlp", "mlp_scaled"))
    M, N, K = HALF_SHAPE if door.startswith("half") else SPLIT_SHAPE
    g = torch.Generator().manual_seed(M + N + K)
    rand = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x, dy = rand(M, K), rand(M, K if mlp else N)
    w1, b1 = (rand(N, K) * K ** -0.5).requires_grad_(True), rand(N).requires_grad_(True)
    w2, b2 = (rand(K, N) * N ** -0.5).requires_grad_(True), rand(K).requires_grad_(True)
    fn = getattr(functions, door)
    before = dict(functions.HALF_NODE_CALLS)
    for frozen, want_bwd in ((False, None), (False, want_all), (True, want_frozen)):
        xin = x.clone().requires_grad_(not frozen)
        leaves = [t for t in (xin, w1, b1) + ((w2, b2) if mlp else ()) if t.requires_grad]
        y = []
        got_fwd = _recorded(monkeypatch, lambda: y.append(fn(xin, w1, b1, w2, b2, ops.ACT_GELU) if mlp else fn(xin, w1, b1, w1, "w")))
        got_bwd = _recorded(monkeypatch, lambda: torch.autograd.grad(y[0], leaves, dy))
        if want_bwd is None:
            continue
        print("LNL %s, x %s: forward %s backward %s" % (door, "frozen" if frozen else "trainable", got_fwd, got_bwd))
        assert got_fwd == want_fwd, (door, frozen, got_fwd)
        assert got_bwd == want_bwd, (door, frozen, got_bwd)
    if door.startswith("half"):          # the node ran, not the fall-through
        assert functions.HALF_NODE_CALLS["mlp" if mlp else "linear"] - before.get("mlp" if mlp else "linear", 0) == 3
