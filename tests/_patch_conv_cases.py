"""Cases of the training projection node (functions.PatchConvFunction, csrc/patch_pack.hip), shared by the CPU and the GPU tests.

A shape is (B, C_in, C_out, H, W, k, form): x is (B, C_in, H, W); form "conv" is conv2d k x k / stride k, form "transposed" is
conv_transpose2d 2 x 2 / stride 2 (k names the kernel; its output and dy are (B, C_out, 2 H, 2 W)).  The smallest shapes that reach each way
the pack kernel (tiles of 128 patch rows x 64 columns) and the node can go wrong:
  one pixel                                                      a single row, M = 1 -> 32 pad columns
  2 x 32 -> 64 x 3 x 3                                           a row tile that spans two images; odd W: NCHW rows are unaligned
  96 -> 32 x 5 x 7                                               channels ragged against the 64-column tile, M = 35 -> rows_p = 64
  32 -> 32 x 48 x 48                                             2304 rows = 18 row tiles: the order of the dsum partials matters
  transposed 2 x 32 -> 8 x 3 x 5                                 an odd patch grid, dy is 6 x 10
  transposed 64 -> 72 x 4 x 4                                    4 x 72 = 288 columns: more than one 256-column GEMM tile, 5 column tiles
  patch 2 x 3 -> 32 x 32 x 48, k = 16                            the patch embedding: 768 columns, the input frozen
The float64 algebra below is the node's own statement -- gathered patch rows, the 2-D weight views, the three products, channel sums --
NOT a call to torch's convolution backward; test_patch_conv_cpu.py checks it against torch's float64 autograd."""
import torch
import torch.nn.functional as F

SHAPES = [(1, 32, 32, 1, 1, 1, "conv"), (2, 32, 64, 3, 3, 1, "conv"), (1, 96, 32, 5, 7, 1, "conv"), (1, 32, 32, 48, 48, 1, "conv"),
          (2, 32, 8, 3, 5, 2, "transposed"), (1, 64, 72, 4, 4, 2, "transposed"), (2, 3, 32, 32, 48, 16, "conv")]
IDS = ["one-pixel", "two-images-odd-w", "ragged-channels", "many-tiles", "transposed-odd-grid", "transposed-wide", "patch16-frozen"]


def frozen_input(shape):
    """the patch form's input is the image: it has no gradient (a trainable input with k > 1 is declined)"""
    return shape[6] == "conv" and shape[5] > 1


def out_shape(shape):
    B, Cin, Cout, H, W, k, form = shape
    return (B, Cout, 2 * H, 2 * W) if form == "transposed" else (B, Cout, H // k, W // k)


def weight_shape(shape):
    B, Cin, Cout, H, W, k, form = shape
    return (Cin, Cout, 2, 2) if form == "transposed" else (Cout, Cin, k, k)


def inputs(shape, seed=0):
    """(x, dy, weight, bias), drawn in fp32"""
    B, Cin, Cout, H, W, k, form = shape
    g = torch.Generator().manual_seed(1000 * seed + B + 3 * Cin + 5 * Cout + 7 * H + 11 * W + 13 * k)
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(out_shape(shape), generator=g)
    fan = Cin * (1 if form == "transposed" else k * k)
    w = torch.randn(weight_shape(shape), generator=g) * fan ** -0.5
    b = torch.randn(Cout, generator=g)
    return x, dy, w, b


def gather(x, k):
    """(B, C, H, W) -> the patch rows (B H/k W/k, C k k): row (b, h, w), column c k^2 + i k + j"""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // k, k, W // k, k).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // k) * (W // k), C * k * k)


def scatter(rows, B, C, H, W, k):
    """the inverse of gather"""
    return rows.reshape(B, H // k, W // k, C, k, k).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def algebra64(shape, x, dy, w, b):
    """(y, dx, dW, db) in float64 as the node states them"""
    B, Cin, Cout, H, W, k, form = shape
    x, dy, w, b = (t.double() for t in (x, dy, w, b))
    db = dy.sum((0, 2, 3))
    if form == "transposed":
        X, W2 = gather(x, 1), w.reshape(Cin, Cout * 4)
        y = scatter(X @ W2, B, Cout, 2 * H, 2 * W, 2) + b.view(1, -1, 1, 1)
        G = gather(dy, 2)
        return y, scatter(G @ W2.t(), B, Cin, H, W, 1), (X.t() @ G).reshape(w.shape), db
    X, W2 = gather(x, k), w.reshape(Cout, Cin * k * k)
    y = scatter(X @ W2.t() + b, B, Cout, H // k, W // k, 1)
    G = gather(dy, 1)
    return y, scatter(G @ W2, B, Cin, H, W, k), (G.t() @ X).reshape(w.shape), db


def torch_graph(shape, x, dy, w, b, dtype, device="cpu"):
    """(y, dx, dW, db) of torch's own conv2d / conv_transpose2d autograd in `dtype` on `device`"""
    k, form = shape[5], shape[6]
    x, w, b = (t.to(device=device, dtype=dtype).requires_grad_(True) for t in (x, w, b))
    with torch.enable_grad():
        y = F.conv_transpose2d(x, w, b, stride=2) if form == "transposed" else F.conv2d(x, w, b, stride=k)
        y.backward(dy.to(device=device, dtype=dtype))
    return y.detach(), x.grad, w.grad, b.grad
