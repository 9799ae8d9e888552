"""The assignment kernel's yardsticks (csrc/hungarian_assign.hip): test_hungarian_assign_cpu.py, test_gpu_hungarian_assign.py.

`lsa_restated` is the algorithm of the kernel in numpy, as documentation and as a CPU yardstick: scipy's shortest-augmenting-path solver
(Crouse 2016) operation for operation -- float64 adds, subtracts and compares only, the list of unscanned columns filled in reverse with a
removed entry replaced by the last one, and the selection among equal candidates in its data-parallel form (an unassigned column at the
LARGEST list position, else the SMALLEST position).  The tests hold it, and the kernel, to the pairs of the installed
scipy.optimize.linear_sum_assignment exactly.

The case generators produce matrices with real ties; `TorchAssignOps` is a plain-torch stand-in for net.HipBackendAssign: the cost block of
_hungarian_cases.TorchHungarianOps, scipy, and the pairs moved to the tensors' device."""
import functools

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from _hungarian_cases import TorchHungarianOps

ST_INVALID, ST_INFEASIBLE, ST_CAP = 32, 64, 128
# the raw op's shapes (Q, T): the smallest; more queries than targets and the reverse; one target, one query; nothing a multiple of anything;
# the production shape; both limits at once
RAW_SHAPES = [(1, 1), (4, 3), (40, 1), (1, 40), (20, 37), (70, 9), (300, 37), (900, 100), (4096, 256)]
FILLS = ("zeros", "01", "012", "dup", "inf")


def lsa_restated(C, count=None):
    """scipy.optimize.linear_sum_assignment(C) restated -> (rows, cols) int64; raises ValueError with scipy's messages.  count: a list that
    receives the number of inner iterations (scanned columns)."""
    C = np.asarray(C)
    if C.ndim != 2:
        raise ValueError("expected a matrix")
    if np.any(np.isnan(C) | np.isneginf(C)):
        raise ValueError("matrix contains invalid numeric entries")
    transposed = C.shape[1] < C.shape[0]
    M = (C.T if transposed else C).astype(np.float64)          # the widening of fp32 costs is exact
    nr, nc = M.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    path = np.full(nc, -1)
    inner = 0
    for cur in range(nr):
        minVal, i = 0.0, cur
        remaining = np.arange(nc - 1, -1, -1)
        n_rem = nc
        shortest = np.full(nc, np.inf)
        scanned, sink = [], -1
        for _ in range(nr):                                  # the kernel's cap: a search scans at most cur + 1 columns
            inner += 1
            js = remaining[:n_rem]
            r = ((minVal + M[i, js]) - u[i]) - v[js]         # this order
            better = r < shortest[js]
            path[js[better]] = i
            shortest[js[better]] = r[better]
            s = shortest[js]
            lowest = s.min()
            if lowest == np.inf:
                raise ValueError("cost matrix is infeasible")
            ties = np.nonzero(s == lowest)[0]
            free = ties[row4col[js[ties]] == -1]
            index = int(free[-1]) if len(free) else int(ties[0])
            minVal = lowest
            j = int(js[index])
            scanned.append(j)
            n_rem -= 1
            remaining[index] = remaining[n_rem]              # swap with the last
            if row4col[j] == -1:
                sink = j
                break
            i = int(row4col[j])
        if sink < 0:
            raise ValueError("the iteration cap was hit")
        u[cur] += minVal
        for j in scanned[:-1]:                               # the rows that own the scanned columns: col4row[row4col[j]] == j
            u[row4col[j]] += minVal - shortest[j]
        for j in scanned:
            v[j] -= minVal - shortest[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if count is not None:
        count.append(inner)
    if transposed:
        order = np.argsort(col4row)
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


def lsa_sequential(C):
    """the same algorithm with scipy's SEQUENTIAL column scan (`s < lowest or (s == lowest and row4col[j] == -1)`), small matrices only: what
    the data-parallel selection rule of lsa_restated is the equivalent of"""
    C = np.asarray(C)
    transposed = C.shape[1] < C.shape[0]
    M = (C.T if transposed else C).astype(np.float64)
    nr, nc = M.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col, path = [-1] * nr, [-1] * nc, [-1] * nc
    for cur in range(nr):
        minVal, i = 0.0, cur
        remaining = [nc - 1 - it for it in range(nc)]
        n_rem = nc
        SR, SC = [False] * nr, [False] * nc
        shortest = [np.inf] * nc
        sink = -1
        while sink == -1:
            index, lowest = -1, np.inf
            SR[i] = True
            for it in range(n_rem):
                j = remaining[it]
                r = ((minVal + M[i, j]) - u[i]) - v[j]
                if r < shortest[j]:
                    path[j], shortest[j] = i, r
                if shortest[j] < lowest or (shortest[j] == lowest and row4col[j] == -1):
                    lowest, index = shortest[j], it
            minVal = lowest
            if minVal == np.inf:
                raise ValueError("cost matrix is infeasible")
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            n_rem -= 1
            remaining[index] = remaining[n_rem]
        u[cur] += minVal
        for i in range(nr):
            if SR[i] and i != cur:
                u[i] += minVal - shortest[col4row[i]]
        for j in range(nc):
            if SC[j]:
                v[j] -= minVal - shortest[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    col4row = np.asarray(col4row)
    if transposed:
        order = np.argsort(col4row)
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


# ------------------------------------------------------------------------------------------------ the cases
def adversarial(Q, T):
    """C[q, t] = -(q + t) t: integers below 2^24 at every limit shape (exact in fp32); every search scans about as many columns as rows are assigned
    already: 5050 = nr (nr + 1) / 2 inner iterations at 100 x 100, 4951 at 900 x 100, 32641 at 4096 x 256"""
    q, t = np.arange(Q, dtype=np.float64)[:, None], np.arange(T, dtype=np.float64)[None, :]
    return (-(q + t) * t).astype(np.float32)


@functools.lru_cache(maxsize=None)
def filled(Q, T, fill, seed=0):
    """a (Q, T) float32 cost matrix with ties; cached, shared by the tests and never written to"""
    g = np.random.default_rng(1000 * seed + 7 * Q + T)
    if fill == "zeros":
        C = np.zeros((Q, T), dtype=np.float32)
    elif fill == "01":
        C = g.integers(0, 2, (Q, T)).astype(np.float32)
    elif fill == "012":
        C = g.integers(0, 3, (Q, T)).astype(np.float32)
    elif fill == "dup":                                      # float32 normals with two equal columns and two equal rows
        C = g.standard_normal((Q, T)).astype(np.float32)
        if T > 1:
            C[:, T - 1] = C[:, 0]
        if Q > 1:
            C[Q - 1, :] = C[0, :]
    elif fill == "inf":                                      # +inf on a sixteenth of the entries, none on the diagonal: the problem stays feasible
        C = g.standard_normal((Q, T)).astype(np.float32)
        n = max(1, (Q * T) // 16)
        qi, ti = g.integers(0, Q, n), g.integers(0, T, n)
        keep = qi != ti
        C[qi[keep], ti[keep]] = np.inf
    else:
        raise KeyError(fill)
    C.setflags(write=False)
    return C


def tie_matrices(seed, n=1000):
    """n tie-heavy integer matrices of shapes 1..13 x 1..13: 0/1 and 0..2 costs, every fourth with a duplicated column"""
    g = np.random.default_rng(seed)
    for k in range(n):
        Q, T = int(g.integers(1, 14)), int(g.integers(1, 14))
        C = g.integers(0, 2 + k % 2, (Q, T)).astype(np.float32)
        if k % 4 == 0 and T > 1:
            C[:, -1] = C[:, 0]
        yield C


def duplicated(Q, T, seed):
    """float32 normals with duplicated rows and columns (an eighth of each)"""
    g = np.random.default_rng(seed + 31 * Q + T)
    C = g.standard_normal((Q, T)).astype(np.float32)
    for _ in range(max(1, T // 8)):
        a, b = g.integers(0, T, 2)
        C[:, a] = C[:, b]
    for _ in range(max(1, Q // 8)):
        a, b = g.integers(0, Q, 2)
        C[a, :] = C[b, :]
    return C


def pack_blocks(blocks, device, cost_status=None):
    """[(Q, n_b) float32 arrays] of one Q -> the operands of ops.hungarian_assign: (costs fp32 (Q * sum_t + B,) as hipie_hungarian_cost leaves
    them, n_tgt, t_off int32 (B,), sum_t, Tmax)"""
    Q = blocks[0].shape[0]
    counts = [int(c.shape[1]) for c in blocks]
    offs = [sum(counts[:b]) for b in range(len(blocks))]
    flat = np.concatenate([np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in blocks] + [np.zeros(0, np.float32)])
    st = np.asarray(cost_status if cost_status is not None else [0] * len(blocks), dtype=np.int32)
    out = torch.from_numpy(np.concatenate([flat, st.view(np.float32)])).to(device)
    both = torch.tensor([counts, offs], dtype=torch.int32).to(device)
    return out, both[0], both[1], sum(counts), max(counts)


def scipy_pairs(C):
    i, j = linear_sum_assignment(np.asarray(C))
    return i.astype(np.int64), j.astype(np.int64)


# ------------------------------------------------------------------------------------------------ the stand-in
class TorchAssignOps(TorchHungarianOps):
    """a stand-in for net.HipBackendAssign in plain torch on any device: TorchHungarianOps' cost blocks, scipy per image, the pairs moved to the
    tensors' device; a matrix scipy refuses sets the image's status (32: invalid numeric entries, 64: infeasible) and leaves its pairs 0"""
    match_calls = []

    @classmethod
    def hungarian_match(cls, logits, boxes, packed, w, masks=None, coords=None, stuff_takes_mean=True, with_boxes=True, class_mode="auto"):
        cls.match_calls.append((stuff_takes_mean, with_boxes, class_mode, masks is not None))
        Cs = cls.hungarian_costs(logits, boxes, packed, w, masks, coords, stuff_takes_mean, with_boxes, class_mode)
        if Cs is None:
            return None
        dev = logits.device
        pairs, status = [], []
        for C in Cs:
            try:
                i, j = scipy_pairs(C)
                status.append(0)
            except ValueError as e:
                k = min(C.shape)
                i = j = np.zeros(k, dtype=np.int64)
                status.append(ST_INVALID if "invalid numeric" in str(e) else ST_INFEASIBLE)
            pairs.append((torch.from_numpy(i).to(dev), torch.from_numpy(j).to(dev)))
        return pairs, torch.tensor(status, dtype=torch.int32).to(dev)
