"""shared by test_conv_train_cpu.py and test_gpu_conv_train.py: inputs of the training 3 x 3 convolution (+ ReLU) node, its backward in
float64 as the kernels state it -- on the zero-padded pixel grid, with the flipped / swapped weight for dx, the tap-shifted row contraction
for dW and the row sum for db; NOT a call to torch's convolution backward -- and torch's own graph.  The ReLU mask is an INPUT: the GPU
tests take it from the kernel forward's own y > 0.  Everything is drawn in fp32, so a float64 copy holds fp32-representable values."""
import torch
import torch.nn.functional as F

CHUNK = 2048        # grid rows per partial of hipie_conv3x3_wgrad (csrc/conv_wgrad.hip WG_CHUNK); a stage of the kernel is 64 rows

# (B, Cin, Cout, H, W): the smallest shapes that reach each way the kernels can go wrong
SHAPES = [
    (1, 32, 32, 1, 1),        # one pixel, all eight neighbours are border
    (2, 32, 64, 3, 3),        # the halo crosses from image 0's last padded row into image 1's first
    (3, 64, 32, 5, 7),        # odd Wp, two k tiles per tap, ragged last row chunk
    (2, 32, 288, 4, 6),       # more than one 256-column tile in the forward and in n blocks (and a ragged 64-wide n block: 288 = 4.5 x 64)
    (2, 288, 32, 6, 4),       # the same for the input-gradient pass (and a ragged c block)
    (1, 32, 32, 64, 64),      # 66 x 66 = 4356 grid rows: chunks of 2048, 2048 and 260 -- more than two, the last one ragged (4 stages + 4 rows)
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def inputs(B, Cin, Cout, H, W, seed=0):
    """x (B, Cin, H, W), dy (B, Cout, H, W), weight (Cout, Cin, 3, 3) at the variance-preserving scale, bias (Cout) in fp32"""
    g = torch.Generator().manual_seed(seed * 7919 + B * 131 + Cin * 17 + Cout * 3 + H * 1009 + W)
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g) * 0.3
    return x, dy, w, b


def grid64(t):
    """(B, C, H, W) -> (the float64 padded grid (rows + 2 guard, C): B (H+2) (W+2) pixel rows with a zero border, guard = W + 3 zero rows on
    both ends; guard; rows)"""
    B, C, H, W = t.shape
    Wp = W + 2
    guard, rows = Wp + 1, B * (H + 2) * Wp
    buf = torch.zeros(rows + 2 * guard, C, dtype=torch.float64)
    buf[guard:guard + rows].view(B, H + 2, Wp, C)[:, 1:-1, 1:-1] = t.double().permute(0, 2, 3, 1)
    return buf, guard, rows


def _crop(rows_c, B, H, W):
    return rows_c.view(B, H + 2, W + 2, -1)[:, 1:-1, 1:-1].permute(0, 3, 1, 2)


def _shift(tap, Wp):
    return (tap // 3 - 1) * Wp + (tap % 3 - 1)


def pre_activation64(x, w, b):
    """conv(x) + b in float64 as the forward kernel states it: y[row, n] = sum_tap sum_c x[row + shift(tap), c] W[n, c, tap] + b[n]"""
    B, C, H, W = x.shape
    X, guard, rows = grid64(x)
    wk = w.double().permute(2, 3, 1, 0).reshape(9, C, -1)
    y = sum(X[guard + _shift(t, W + 2):guard + _shift(t, W + 2) + rows] @ wk[t] for t in range(9))
    return _crop(y if b is None else y + b.double(), B, H, W)


def backward64(x, dy, w, mask):
    """(dx, dW, db) in float64 on the padded grid, g = dy * mask (mask None: 1) on its own zero-bordered grid:
    dx[row, c] = sum_tap sum_n g[row + shift(tap), n] Wt[c, tap, n],  Wt[c, (2 - ky, 2 - kx), n] = W[n, c, ky, kx];
    dW[n, tap, c] = sum_rows g[row, n] x[row + shift(tap), c];  db[n] = sum_rows g[row, n]"""
    B, C, H, W = x.shape
    N, Wp = w.shape[0], W + 2
    X, guard, rows = grid64(x)
    G, _, _ = grid64(dy.double() if mask is None else dy.double() * mask.to(torch.float64))
    wt = w.double().flip(2, 3).permute(2, 3, 0, 1).reshape(9, N, C)                       # [tap', n, c] = W[n, c, 2 - ky, 2 - kx]
    dxg = sum(G[guard + _shift(t, Wp):guard + _shift(t, Wp) + rows] @ wt[t] for t in range(9))
    g = G[guard:guard + rows]
    dw = torch.stack([g.t() @ X[guard + _shift(t, Wp):guard + _shift(t, Wp) + rows] for t in range(9)], 1)      # (N, 9, C)
    return _crop(dxg, B, H, W), dw.view(N, 3, 3, C).permute(0, 3, 1, 2), g.sum(0)


def torch_graph(x, dy, w, b, relu, dtype, dev="cpu"):
    """(y, dx, dW, db) of F.conv2d (+ F.relu) under autograd in `dtype`"""
    x_, w_, b_ = (t.detach().to(dev, dtype).requires_grad_(True) for t in (x, w, b))
    with torch.enable_grad():
        y = F.conv2d(x_, w_, b_, padding=1)
        if relu:
            y = F.relu(y)
        grads = torch.autograd.grad(y, (x_, w_, b_), dy.detach().to(dev, dtype))
    return (y.detach(),) + tuple(grads)


def lattice_inputs(B, Cin, Cout, H, W, seed=0):
    """inputs() on a dyadic lattice: x and weight multiples of 1/16, bias an ODD multiple of 1/512.  Every pre-activation is then a multiple
    of 1/256 plus an odd multiple of 1/512: at least 1/512 away from zero, whatever the draw.  Plain normal draws cannot give that: at the
    1e5 pre-activations of the largest shape about a hundred fall within 1e-3 of zero for every seed."""
    x, dy, w, b = inputs(B, Cin, Cout, H, W, seed)
    x = (x * 16).round() / 16
    w = (w * (9 * Cin) ** 0.5).round() / 16
    b = ((b * 256).round() * 2 + 1) / 512
    return x, dy, w, b


def separated_case(B, Cin, Cout, H, W, margin=1e-3):
    """inputs whose pre-activations all stay `margin` away from zero (the ReLU mask is then the same in every precision) and take both signs:
    the first seed that gives them"""
    for seed in range(20):
        x, dy, w, b = lattice_inputs(B, Cin, Cout, H, W, seed)
        pre = pre_activation64(x, w, b)
        if float(pre.abs().min()) >= margin and bool((pre > 0).any()) and bool((pre < 0).any()):
            return x, dy, w, b
    raise AssertionError("no separated case")
