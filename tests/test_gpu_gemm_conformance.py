"""The tile GEMM family (hipie_amd/csrc/gemm.hip, gemm_tile.h, gemm_k256.hip and the VAR 8 entry of gemm_ln.hip: ops.gemm,
ops.matmul_nt_batched, ops.gemm_split_k, ops.convt2x2_split and the raw batched / softmax / 3 x 3 convolution entries) against float64
references, over every launch line a shipped build can reach, per 32 x 32 output block.

Launch lines (`launch_line` below restates the dispatch) and a test id that reaches each:

  hipie_gemm / hipie_gemm_gather
    k256/hl8, k256/f32       gemm_k256_kernel<false | true>      test_thin_k[m8192-n384-k256-hl8-f32], test_thin_k[m8193-n416-k256-f32-f32-strided]
    small/hl8, small/f32     gemm_small_kernel<0 | 2>            test_small[m1-n8-k32-hl8-f32], test_small[m1-n8-k32-f32-f32]
    wide16/hl8, wide16/f32   gemm_kernel<320,true,0 | 2,16>      test_wide16[m257-n320-k32-hl8-f32-gid], test_wide16[m300-n640-k96-f32-f32-gperm-strided];
                                                                 the full-size shapes: tests/test_gpu_gemm_mfma16.py::test_mfma16_fp32_class,
                                                                 ::test_mfma16_gather_entry, ::test_mfma16_epilogues, ::test_mfma16_small_magnitudes
    big256/hl8, big256/f32   gemm_kernel<256,true,0 | 2>         test_big_direct[m24321-n8-k32-hl8-f32], test_big_direct[m12033-n264-k64-f32-f32],
                                                                 test_big_gather[m2305-n1288-k32-hl8-f32-gperm] (group_m = 8, a short last group)
    plain256, plain320       gemm_kernel<256 | 320,false>        test_plain[m257-n264-k64-f16-f32], test_plain[m257-n320-k64-f16-f32]
    the epilogue matrix on small/hl8, big256/hl8, big256/f32, wide16/hl8, plain256, plain320: test_epilogue[<line>-...]
    out aliases resid, out_row with dropped rows, on small/hl8 and big256/hl8: test_row_map[...]
    operands whose lo halves are fp16 subnormals, on small/hl8, big256/hl8, big256/f32, wide16/hl8, k256/hl8: test_subnormal_lo_halves[...]
  hipie_gemm_batched         batched256, batched320   gemm_kernel<256 | 320,true>, gridDim.y > 1   test_batched[m257-n264-k32-f32-sharea], [m1-n320-k96-hl8-sharew]
  hipie_gemm_batched_resid   bresid256, bresid320     the same instances, bias + residual          test_batched_resid[m257-n264-k32-res], [m257-n320-k96-res]
  hipie_gemm_batched_softmax       softmax            gemm_kernel<256,true,0>, p.softmax           test_softmax[softmax-n136-L133-m257-none-c50000]
  hipie_gemm_batched_softmax_bias  softmax_bias       gemm_kernel<256,true,8>                      test_softmax[softmax_bias-n256-L256-m257-item-c50000]
  hipie_conv3x3_split        conv256/hl8, conv256/f32   gemm_kernel<256,true,0 | 2>, conv_kpt > 0  test_conv3x3[c32-n264-3x3-hl8-f32], [c64-n264-5x7-f32-hl8-relu]
                             conv320/hl8, conv320/f32   gemm_kernel<320,true,0 | 2> on 32x32x16 MFMAs: the only shipped route to these two
                                                        instances besides the batched entries     test_conv3x3[c64-n320-3x3-hl8-hl8], [c32-n320-5x7-f32-f32-relu]
  wrappers                   ops.matmul_nt_batched, ops.gemm_split_k, ops.convt2x2_split           test_matmul_nt_batched, test_gemm_split_k, test_convt2x2_split

Not reachable from a shipped build, hence not tested here: everything behind HIPIE_STUDY_KNOBS / HIPIE_GEMM_VARIANTS -- the forced
thin-K / small-kernel switches (HIPIE_GEMM_K256, HIPIE_GEMM_SMALL, HIPIE_GEMM_SMALL_MAXTILES), gemm_kernel<320,true,0 | 2> on 32x32x16
MFMAs from hipie_gemm (HIPIE_GEMM_MFMA=32), the VAR 1 / 3 instances and launch_gemm2 / 3 / 4.  No environment variable is set here.
Out of scope (they keep their own tests): the LayerNorm epilogue of gemm_ln.hip (hipie_gemm_ln), gemm_f8x.hip and ffn_fused.hip.

References.  Float64 on the CPU of the values the kernel reads: for split operands (HL8 or fp32 rows) the ORIGINAL fp32 values, the
project's convention (tests/test_gpu_gemm.py); for plain fp16 operands the rounded ones.  The epilogue is `_ref` of test_gpu_gemm.py
(exact-erf GELU, QuickGELU y * sigmoid(1.702 y)) in float64.  `ref_softmax` is what the softmax epilogue does:
softmax(clamp(alpha * a . w^T + colbias, +-clamp) + (0 | -inf)) over the first L columns, a row with no attended column gives zeros, masked
and padded columns exactly 0.  `loops_gemm` / `loops_softmax` state the same in plain numpy loops and serve the tiny edge inputs;
test_references_agree checks the pairs to 1e-12 on the CPU.

Contract of values beyond the fp16 range (one case per epilogue line): an HL8 output saturates -- gm_split2 clamps to +-65504 before the
split, so the hi plane is +-65504 and the lo plane finite (the reference is clamped the same way); an F16 output is `.half()` of the fp32
output of the same call, bit for bit (+-inf beyond 65520).

A fully masked outer item of the softmax entries gives rows of zeros.  oracle.ops.bi_attention_core (the model's own formulation) fills
masked logits with -9e15 instead of -inf, so for a text with no attended token it gives a distribution that sums to 1 over the L columns
(uniform in fp32, where -9e15 absorbs the logits), not zeros: the same difference as the masked-row contract of the flash attention family (tests/test_gpu_flash_attn.py); no product path
sends such a mask (a prompt keeps its CLS token), and the kernel is left as it is.

Metric: `block_err` = max|got - ref| over a block / max|ref| over the same block, maximised over the 32-row x 32-column blocks of the
output (the MFMA block, the smallest unit any of these kernels owns); a block whose reference is all zero must be exactly zero.  With
out_row maps the blocks are those of the PRODUCT rows.  Column blocks are not scaled by powers of two: weights of size K^-0.5 times 1/8
have their lo halves in the fp16 subnormals, which raises the format's own error to 1e-5; the per-block normalisation does that job.

Bounds, the project's own (header of tests/test_gpu_gemm.py): 3e-6 for fp32 and HL8 outputs, 6e-4 for fp16 outputs, 2e-5 for operands
whose lo halves are fp16 subnormals (test_gemm_split_small_magnitudes), and the HL8 plane condition |lo| <= |hi| 2^-11 + 2^-24.  No bound comes from a kernel.  Attainable: `emu_gemm` emulates the format choice only (hi / lo
split of both operands, W_lo.X_hi + W_hi.X_lo + W_hi.X_hi in fp32, the epilogue in fp32, the output rounding) and
test_emulation_within_bound asserts block_err(emu) <= bound / 2 (fp32, HL8) and <= 2^-11 + 1.5e-6 (fp16: one rounding of the element plus
the fp32-class part) on every case of every matrix; EMULATION_ERR records the largest value per group (docs/measurements.md).  All
matrices use K <= 256 (K = 9 C <= 576 for the convolution): that is where the stage and slot edges are, and the emulation's own error
grows to 1.75e-6 at K = 5120.  The softmax epilogue has no project bound for P: SOFTMAX_BOUND is 4 x the worst block_err of the fp32
emulation `emu_softmax` on the matrix of this file (the margin is for v_exp_f32 and the MFMA summation order); the rows must sum to 1
within it and masked columns must be exact zeros.

Output buffers: `poisoned` frees a NaN block of the same size before each call that allocates its own output; where the test passes
`out=` the buffer is pre-filled with a sentinel, and rows / columns / batch items the call must not touch have to keep it."""
import collections
import functools
import itertools
import math
import os
import zlib

import numpy as np
import pytest
import torch

from test_gpu_gemm import _ref as ref_epilogue

torch.set_grad_enabled(False)
DEV = "cuda"
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = {"f32": 3e-6, "hl8": 3e-6, "f16": 6e-4}
EMU_BOUND = {"f32": 1.5e-6, "hl8": 1.5e-6, "f16": 2.0 ** -11 + 1.5e-6}
SENTINEL = 7.0
EXTREMES = (-100.0, -20.0, -5.0, -0.0, 5.0, 20.0, 100.0)       # bias columns 8 .. 14: every activation at its extremes, no NaN
OVER = 70000.0                                                    # bias columns 40 / 41 of the `over` cases: beyond the fp16 range
ZERO_ROWS = (0, 31, 100, 256)                                     # all-zero A rows: their pre-activation is the bias
BIND_SHARE = 0.05

# Largest block_err of the CPU emulation against the float64 reference per (group, output format), measured by
# test_emulation_within_bound, which re-measures them: each must stay at or below its entry and above half of it (the entries are the
# measured values plus 1 %).  Half of the bound is 1.5e-6 (fp32, HL8), 1e-5 (subnormal lo halves); fp16 outputs: 2^-11 + 1.5e-6 = 4.898e-4.
# ("softmax", "hl8") is the fp32 emulation of the softmax epilogue; SOFTMAX_BOUND = 4 x that entry.
EMULATION_ERR = {
    ("small", "f32"): 7.115e-07, ("big", "f32"): 6.086e-07, ("wide16", "f32"): 6.713e-07, ("plain", "f32"): 6.277e-07,
    ("epilogue", "f32"): 5.240e-07, ("epilogue", "hl8"): 5.800e-07, ("epilogue", "f16"): 4.886e-04,
    ("rowmap", "f32"): 4.088e-07, ("rowmap", "hl8"): 4.030e-07, ("k256", "f32"): 1.287e-06, ("subnormal", "f32"): 4.946e-06,
    ("batched", "f32"): 7.131e-07, ("batched", "hl8"): 5.988e-07, ("bresid", "f32"): 2.205e-07,
    ("conv", "f32"): 9.399e-07, ("conv", "hl8"): 7.849e-07, ("wrappers", "f32"): 5.886e-07,
    ("softmax", "hl8"): 3.182e-06,
}
SOFTMAX_BOUND = 4 * EMULATION_ERR["softmax", "hl8"]


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------------- mirror of the dispatch
def launch_line(entry, M=0, N=0, K=0, in_fmt="hl8", out_fmt="f32", act=0, resid=False, out_row=False, alpha=1.0, oscale=1.0, dense_w=True,
                lda_bytes=None):
    """the kernel a shipped build launches: gemm_impl (entry "gemm" | "gather") and the other entry points of gemm.hip / gemm_ln.hip"""
    wide = N % 320 == 0
    if entry in ("batched", "bresid"):
        return entry + ("320" if wide else "256")
    if entry in ("softmax", "softmax_bias"):
        return entry
    if entry == "conv":
        return "conv%s/%s" % ("320" if wide else "256", in_fmt)
    assert entry in ("gemm", "gather") and (entry == "gemm" or in_fmt != "f16")
    a_row = entry == "gather"
    split = in_fmt in ("hl8", "f32")
    lda_bytes = 4 * K if lda_bytes is None else lda_bytes
    if (N >= 384 and split and K == 256 and out_fmt == "f32" and act == 0 and not resid and not out_row and not a_row and alpha == 1.0
            and oscale == 1.0 and N % 32 == 0 and M >= 8192 and dense_w and M * lda_bytes < (1 << 32)):
        return "k256/" + in_fmt
    tiles = -(-M // 256) * -(-N // (320 if wide else 256))
    if split and tiles < 96 and not a_row:
        return "small/" + in_fmt
    if split and wide:
        return "wide16/" + in_fmt
    if split:
        return "big256/" + in_fmt
    return "plain320" if wide else "plain256"


ALL_LINES = (["%s/%s" % (k, f) for k in ("k256", "small", "wide16", "big256", "conv256", "conv320") for f in ("hl8", "f32")]
             + ["plain256", "plain320", "batched256", "batched320", "bresid256", "bresid320", "softmax", "softmax_bias"])


# --------------------------------------------------------------------------------------------------------------- the case matrices
_G = collections.namedtuple("G", "group M N K inf outf act res bias alpha osc gather out_row inplace wide_w strided over mag")


def G(group, M, N, K, inf="hl8", outf="f32", act=0, res=False, bias="rand", alpha=1.0, osc=1.0, gather=None, out_row=False, inplace=False,
      wide_w=False, strided=False, over=False, mag=1.0):
    return _G(group, M, N, K, inf, outf, act, res, bias, alpha, osc, gather, out_row, inplace, wide_w, strided, over, mag)


def gid(c):
    s = "m%d-n%d-k%d-%s-%s" % (c.M, c.N, c.K, c.inf, c.outf)
    s += "".join(t for t, on in (("-act%d" % c.act, c.act), ("-res", c.res), ("-nobias", c.bias is None), ("-ext", c.bias == "ext"),
                                 ("-a%g" % c.alpha, c.alpha != 1.0), ("-g%s" % c.gather, c.gather), ("-rowmap", c.out_row),
                                 ("-inplace", c.inplace), ("-widew", c.wide_w), ("-strided", c.strided), ("-over", c.over), ("-mag%g" % c.mag, c.mag != 1.0)) if on)
    return s


def line_of(c):
    return launch_line("gather" if c.gather else "gemm", c.M, c.N, c.K, c.inf, c.outf, c.act, c.res, c.out_row, c.alpha, c.osc, not c.wide_w,
                       lda_bytes=4 * (c.K + 64) if c.strided else None)


# small/*: 64 x 128 tiles, 3 LDS slots.  K = 32: one stage (the nkt > 1 guard); 96: all three slots; 128: the first slot reuse
SMALL_MNK = [(1, 8, 32), (63, 128, 64), (65, 136, 96), (129, 264, 128), (1, 264, 256), (63, 8, 96), (65, 128, 32), (129, 136, 64),
             (63, 264, 32), (65, 8, 128), (129, 128, 256), (1, 136, 128)]
SMALL = [G("small", M, N, K, inf) for M, N, K in SMALL_MNK for inf in ("hl8", "f32")]
# big256/* by the direct entry: exactly 96 tiles (a last row tile of one row; an N tail of 8 columns) and the neighbours with 95 / 94
BIG_DIRECT = [G("big", M, N, K, inf) for M, N, K in ((24321, 8, 32), (12033, 264, 64), (24320, 8, 32), (12032, 264, 64)) for inf in ("hl8", "f32")]
BIG_DIRECT_LINE = {24321: "big256", 12033: "big256", 24320: "small", 12032: "small"}
# big256/* by the gather entry (a row map keeps any size on the big kernel): 1 / 2 / 3 stages; 6 column tiles -> group_m = 8 with 10 row
# panels (the last group is short); a map with repeats; fp32 rows through a strided view
BIG_GATHER = ([G("big", 257, 264, K, "hl8", gather="id") for K in (32, 64, 96)]
              + [G("big", 2305, 1288, 32, "hl8", gather="perm"), G("big", 2305, 1288, 32, "f32", gather="id", strided=True),
                 G("big", 257, 264, 64, "hl8", gather="rep"), G("big", 257, 264, 96, "f32", gather="perm", strided=True),
                 G("big", 257, 264, 32, "f32", gather="rep")])
WIDE16 = [G("wide16", 257, 320, 32, "hl8", gather="id"), G("wide16", 300, 640, 96, "hl8", gather="perm"),
          G("wide16", 257, 320, 32, "f32", gather="rep"), G("wide16", 300, 640, 96, "f32", gather="perm", strided=True)]
PLAIN = [G("plain", 257, N, K, "f16") for N in (264, 320) for K in (64, 128, 192)]

# the epilogue matrix: line -> (N, operand format, gather)
EPI_LINES = {"small/hl8": (264, "hl8", None), "big256/hl8": (264, "hl8", "id"), "big256/f32": (264, "f32", "id"),
             "wide16/hl8": (320, "hl8", "id"), "plain256": (264, "f16", None), "plain320": (320, "f16", None)}


def _epilogue_cases():
    out = []
    for line, (N, inf, gather) in EPI_LINES.items():
        for outf, act, res in itertools.product(("f32", "f16", "hl8"), (0, 1, 2, 3), (False, True)):
            out.append(G("epilogue", 257, N, 64, inf, outf, act, res, "ext", 0.5, 1.0 if outf == "f32" else 4.0, gather))
        out.append(G("epilogue", 257, N, 64, inf, "f32", 1, True, None, 0.5, 1.0, gather))
        for outf in ("hl8", "f16"):
            out.append(G("epilogue", 257, N, 64, inf, outf, 0, False, "rand", 0.5, 4.0, gather, over=True))
    return out


EPILOGUE = _epilogue_cases()
# out aliases resid; out_row = a permutation into a buffer with 5 spare rows, a quarter of the entries -1; the residual comes from the OUTPUT row
ROW_MAP = [G("rowmap", 257, 264, 64, "hl8", outf, 0, True, "rand", gather=g, out_row=True, inplace=outf == "f32")
           for g in (None, "id") for outf in ("f32", "hl8")]
# thin-K: N = 416 is 13 chunks (the double buffer ends on the odd side); X as HL8 or strided fp32; with and without bias; strided output
THIN = [G("k256", 8192, 384, 256, "hl8"), G("k256", 8193, 416, 256, "f32", strided=True), G("k256", 8319, 384, 256, "f32", bias=None, strided=True),
        G("k256", 8192, 416, 256, "hl8", bias=None), G("k256", 8193, 384, 256, "hl8", strided=True), G("k256", 8319, 416, 256, "hl8")]
# neighbours that must NOT take the thin-K kernel, each inside the bound on whatever kernel it gets
THIN_NEIGHBOURS = [G("k256", 8191, 384, 256), G("k256", 8192, 352, 256), G("k256", 8192, 392, 256), G("k256", 8192, 384, 256, act=2),
                   G("k256", 8192, 384, 256, res=True), G("k256", 8192, 384, 256, alpha=0.5), G("k256", 8192, 384, 256, out_row=True),
                   G("k256", 8192, 384, 256, wide_w=True)]
# operands of size 1e-2: their lo halves are fp16 subnormals, which the matrix pipe must not flush (the error would be ~1e-4); bound 2e-5
SUBNORMAL = [G("subnormal", 257, 264, 64, "hl8", bias=None, mag=1e-2), G("subnormal", 257, 264, 64, "hl8", bias=None, gather="id", mag=1e-2),
             G("subnormal", 257, 264, 64, "f32", bias=None, gather="id", mag=1e-2), G("subnormal", 257, 320, 64, "hl8", bias=None, gather="id", mag=1e-2),
             G("subnormal", 8192, 384, 256, "hl8", bias=None, mag=1e-2)]
SUBNORMAL_BOUND = 2e-5
TILE_CASES = SMALL + BIG_DIRECT + BIG_GATHER + WIDE16 + PLAIN + EPILOGUE + ROW_MAP + THIN + THIN_NEIGHBOURS + SUBNORMAL


def bound_of(c):
    return SUBNORMAL_BOUND if c.mag != 1.0 else BOUND[c.outf]

_B = collections.namedtuple("B", "M N K outf share resid")       # the batched entries: n_outer x n_inner = 2 x 3, alpha 0.25
NO, NI = 2, 3
BATCHED = [_B(257, 264, 32, "f32", "a", None), _B(1, 320, 96, "hl8", "w", None), _B(257, 640, 96, "f32", "w", None), _B(1, 264, 96, "f32", "a", None),
           _B(257, 320, 32, "hl8", "a", None), _B(1, 640, 32, "hl8", "w", None), _B(257, 264, 96, "hl8", "w", None), _B(1, 320, 32, "f32", "a", None)]
BRESID = [_B(257, 264, 32, "f32", "a", "res"), _B(257, 320, 96, "f32", "w", "res"), _B(1, 264, 96, "f32", "w", "nores"), _B(1, 320, 32, "f32", "a", "res")]


def bid(c):
    return "m%d-n%d-k%d-%s" % (c.M, c.N, c.K, c.resid if c.resid else "%s-share%s" % (c.outf, c.share))


_V = collections.namedtuple("V", "C N hw inf outf relu")         # hipie_conv3x3_split, B = 2
CONV = [_V(32, 264, (3, 3), "hl8", "f32", False), _V(64, 264, (5, 7), "f32", "hl8", True), _V(64, 320, (3, 3), "hl8", "hl8", False),
        _V(32, 320, (5, 7), "f32", "f32", True), _V(64, 264, (5, 7), "hl8", "hl8", True), _V(32, 264, (3, 3), "f32", "f32", False),
        _V(32, 320, (5, 7), "hl8", "f32", True), _V(64, 320, (3, 3), "f32", "hl8", False)]


def vid(c):
    return "c%d-n%d-%dx%d-%s-%s%s" % (c.C, c.N, c.hw[0], c.hw[1], c.inf, c.outf, "-relu" if c.relu else "")


_S = collections.namedtuple("S", "entry N L M mask clamp")       # the softmax epilogues: batches 2 x 3, K = 32, alpha 0.5
SM_K, SM_ALPHA, CLAMP_BIND = 32, 0.5, 1.0                        # unit-scale logits: about 30 % lie outside +-1
SM_MASKS = ("none", "holes", "item")
SM_CLAMPS = (0.0, 50000.0, CLAMP_BIND)
CLAMP_NAME = {0.0: "c0", 50000.0: "c50000", CLAMP_BIND: "cbind"}


def _softmax_cases():
    out = []
    for entry in ("softmax", "softmax_bias"):
        for shift in (0, 1):
            for iN, N in enumerate((8, 136, 256)):
                for iL, L in enumerate((1, N - 3, N)):
                    out.append(_S(entry, N, L, (1, 257)[(iN + iL + shift) % 2], SM_MASKS[(iN + iL + shift) % 3], SM_CLAMPS[(iN + 2 * iL + shift) % 3]))
    return out


SOFTMAX = _softmax_cases()


def sid(c):
    return "%s-n%d-L%d-m%d-%s-%s" % (c.entry, c.N, c.L, c.M, c.mask, CLAMP_NAME[c.clamp])


# ------------------------------------------------------------------------------------------------------- references and emulation
def split16(x):
    """the HL8 split of the kernels (hl_split) and of ops.hl8_pack: saturate, hi = fp16(x), lo = fp16(x - hi); both as fp32"""
    xs = x.float().clamp(-65504.0, 65504.0)
    hi = xs.half()
    return hi.float(), (xs - hi.float()).half().float()


def emu_product(a, w, inf):
    if inf == "f16":
        return a.float() @ w.float().t()
    ah, al = split16(a)
    wh, wl = split16(w)
    return (ah @ wl.t() + al @ wh.t()) + ah @ wh.t()


def round_out(v, outf):
    if outf == "f16":
        return v.half().float()
    if outf == "hl8":
        hi, lo = split16(v)
        return hi + lo
    return v


def emu_gemm(a, w, bias, resid, act, alpha, osc, inf, outf):
    """the format choice only: split operands, three fp32 products, the epilogue in fp32, the output rounding"""
    v = emu_product(a, w, inf) * torch.tensor(alpha, dtype=torch.float32)
    if bias is not None:
        v = v + bias.float()
    if act == 1:
        v = torch.nn.functional.gelu(v)
    elif act == 2:
        v = torch.relu(v)
    elif act == 3:
        v = v / (1.0 + torch.exp(-1.702 * v))
    if resid is not None:
        v = v + resid.float()
    return round_out(v * osc, outf)


def ref_out(want, outf):
    """what a correct kernel stores for the float64 value: HL8 saturates at +-65504, fp16 overflows to +-inf beyond 65520"""
    if outf == "hl8":
        return want.clamp(-65504.0, 65504.0)
    if outf == "f16":
        return torch.where(want.abs() >= 65520.0, torch.sign(want) * math.inf, want)
    return want


def loops_gemm(a, w, bias, resid, act, alpha, osc):
    """the epilogue formula written out: one loop iteration per (m, n, k), numpy float64"""
    a, w = a.double().numpy(), w.double().numpy()
    out = np.zeros((a.shape[0], w.shape[0]))
    for m in range(a.shape[0]):
        for n in range(w.shape[0]):
            s = 0.0
            for k in range(a.shape[1]):
                s += a[m, k] * w[n, k]
            y = alpha * s + (0.0 if bias is None else float(bias[n]))
            if act == 1:
                y = 0.5 * y * (1.0 + math.erf(y / math.sqrt(2.0)))
            elif act == 2:
                y = max(y, 0.0)
            elif act == 3:
                y = y / (1.0 + math.exp(-1.702 * y)) if y > -400 else 0.0
            out[m, n] = (y + (0.0 if resid is None else float(resid[m, n]))) * osc
    return torch.from_numpy(out)


def _logits(a, w, cb, alpha, clamp, ft):
    s = torch.einsum("bhmk,bhnk->bhmn", a.to(ft), w.to(ft)) * alpha
    if cb is not None:
        s = s + cb.to(ft)[:, :, None, :]
    if clamp > 0:
        s = s.clamp(-clamp, clamp)
    return s


def _valid(mask, B, N, L):
    v = torch.zeros(B, N, dtype=torch.bool)
    v[:, :L] = True if mask is None else mask.bool()
    return v


def ref_softmax(a, w, cb, mask, L, clamp, alpha):
    """float64: a (B, H, M, K), w (B, H, N, K), cb (B, H, N) | None, mask (B, L) | None -> P (B, H, M, N)"""
    s = _logits(a, w, cb, alpha, clamp, torch.float64)
    s = s.masked_fill(~_valid(mask, a.shape[0], w.shape[2], L)[:, None, None, :], -math.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    tot = p.sum(-1, keepdim=True)
    return torch.where(tot > 0, p / tot, torch.zeros_like(p))


def loops_softmax(a, w, cb, mask, L, clamp, alpha):
    a, w = a.double().numpy(), w.double().numpy()
    B, H, M, K = a.shape
    N = w.shape[2]
    out = np.zeros((B, H, M, N))
    for b, h, m in itertools.product(range(B), range(H), range(M)):
        s = []
        for n in range(L):
            if mask is not None and not bool(mask[b, n]):
                continue
            x = alpha * sum(a[b, h, m, k] * w[b, h, n, k] for k in range(K)) + (0.0 if cb is None else float(cb[b, h, n]))
            s.append((n, min(max(x, -clamp), clamp) if clamp > 0 else x))
        if s:
            top = max(x for _, x in s)
            tot = sum(math.exp(x - top) for _, x in s)
            for n, x in s:
                out[b, h, m, n] = math.exp(x - top) / tot
    return torch.from_numpy(out)


def emu_softmax(a, w, cb, mask, L, clamp, alpha):
    """fp32 emulation of the softmax epilogue: split product, fp32 logits, exp(x - max), division by the fp32 sum, HL8 rounding"""
    B, H, M, K = a.shape
    N = w.shape[2]
    s = torch.stack([torch.stack([emu_product(a[b, h], w[b, h], "hl8") for h in range(H)]) for b in range(B)]) * torch.tensor(alpha, dtype=torch.float32)
    if cb is not None:
        s = s + cb.float()[:, :, None, :]
    if clamp > 0:
        s = s.clamp(-clamp, clamp)
    s = s.masked_fill(~_valid(mask, B, N, L)[:, None, None, :], -math.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    tot = p.sum(-1, keepdim=True)
    return round_out(torch.where(tot > 0, p * (1.0 / tot), torch.zeros_like(p)), "hl8")


def block_err(got, ref):
    """max over the 32 x 32 blocks of max|got - ref| / max|ref|; an all-zero reference block must be exactly zero; non-finite entries
    (an fp16 overflow) must agree exactly and are left out"""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    assert got.shape == ref.shape
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), "non-finite values (an element the kernel did not write reads NaN)"
    if not bool(fin.all()):
        assert torch.equal(got[~fin], ref[~fin])
        got, ref = torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, ref, torch.zeros_like(ref))
    M, N = ref.shape
    Mp, Np = -(-M // 32) * 32, -(-N // 32) * 32
    d, r = torch.zeros(Mp, Np, dtype=torch.float64), torch.zeros(Mp, Np, dtype=torch.float64)
    d[:M, :N] = (got - ref).abs()
    r[:M, :N] = ref.abs()
    d, r = d.view(Mp // 32, 32, Np // 32, 32).amax((1, 3)), r.view(Mp // 32, 32, Np // 32, 32).amax((1, 3))
    dead = r == 0
    assert bool((d[dead] == 0).all()), "a block whose reference is all zero must be exactly zero"
    return float((d[~dead] / r[~dead]).max()) if bool((~dead).any()) else 0.0


# ------------------------------------------------------------------------------------------------------------------- problems
Problem = collections.namedtuple("Problem", "tab a_row a w bias resid out_row want")


@functools.lru_cache(maxsize=None)
def tile_problem(c):
    """the CPU side of a tile-kernel case: operand table (fp32; fp16-rounded for plain operands), row maps, float64 reference `want`
    in PRODUCT row order; resid is in OUTPUT row order where there is a row map"""
    g = gen("tile-" + gid(c) + c.group)
    rows = {None: c.M, "id": c.M, "perm": c.M + 40, "rep": 50}[c.gather]
    tab = torch.randn(rows, c.K, generator=g) * (2.0 if c.mag == 1.0 else c.mag)
    w = torch.randn(c.N, c.K, generator=g) * (c.K ** -0.5 if c.mag == 1.0 else c.mag)
    if c.inf == "f16":
        tab, w = tab.half().float(), w.half().float()
    a_row = {None: None, "id": torch.arange(c.M), "perm": torch.randperm(rows, generator=g)[:c.M],
             "rep": torch.randint(0, rows, (c.M,), generator=g)}[c.gather]
    bias = None if c.bias is None else torch.randn(c.N, generator=g)
    if c.bias == "ext":
        bias[8:15] = torch.tensor(EXTREMES)
        zr = torch.tensor(ZERO_ROWS)
        tab[zr if a_row is None else a_row[zr]] = 0.0
    if c.over:
        bias[40], bias[41] = OVER, -OVER
    a = tab if a_row is None else tab[a_row]
    out_row, R = None, c.M
    if c.out_row:
        R = c.M + 5
        out_row = torch.randperm(R, generator=g)[:c.M]
        out_row[torch.randperm(c.M, generator=g)[:c.M // 4]] = -1
    resid = torch.randn(R, c.N, generator=g) if c.res else None
    r_rows = resid if (resid is None or out_row is None) else resid[out_row.clamp_min(0)]
    want = ref_epilogue(a, w, bias, r_rows, c.act, c.alpha, c.osc)
    return Problem(tab, None if a_row is None else a_row.int(), a, w, bias, resid, None if out_row is None else out_row.int(), want)


def tile_emulation(c):
    p = tile_problem(c)
    r_rows = p.resid if (p.resid is None or p.out_row is None) else p.resid[p.out_row.long().clamp_min(0)]
    return emu_gemm(p.a, p.w, p.bias, r_rows, c.act, c.alpha, c.osc, c.inf, c.outf)


def live_rows(p):
    return slice(None) if p.out_row is None else p.out_row >= 0


BProblem = collections.namedtuple("BProblem", "a w bias resid want")


@functools.lru_cache(maxsize=None)
def batched_problem(c):
    """a (NO, NI, M, K), w (NO, NI, N, K) with the shared operand repeated (the device copy uses a zero stride), want (NO, NI, M, N)"""
    g = gen("batched-" + bid(c))
    a = torch.randn(NO, 1 if c.share == "a" else NI, c.M, c.K, generator=g).expand(NO, NI, c.M, c.K) * 2.0
    w = torch.randn(1 if c.share == "w" else NO, NI, c.N, c.K, generator=g).expand(NO, NI, c.N, c.K) * c.K ** -0.5
    bias = torch.randn(c.N, generator=g) if c.resid else None
    resid = torch.randn(NO, NI, c.M, c.N, generator=g) if c.resid == "res" else None
    want = 0.25 * torch.einsum("oimk,oink->oimn", a.double(), w.double())
    if bias is not None:
        want = want + bias.double()
    if resid is not None:
        want = want + resid.double()
    return BProblem(a, w, bias, resid, want)


def batched_emulation(c):
    p = batched_problem(c)
    return torch.stack([torch.stack([emu_gemm(p.a[o, i], p.w[o, i], p.bias, None if p.resid is None else p.resid[o, i], 0, 0.25, 1.0, "hl8", c.outf)
                                     for i in range(NI)]) for o in range(NO)])


VProblem = collections.namedtuple("VProblem", "x weight bias cols wmat want")
CONV_B = 2


@functools.lru_cache(maxsize=None)
def conv_problem(c):
    """x (B, C, H, W), weight (N, C, 3, 3); cols = the im2col rows (B H W, 9 C) in (dy, dx, channel) order, wmat (N, 9 C) the weight in the
    same order (what the entry takes); want (B H W, N) float64 from F.conv2d"""
    g = gen("conv-" + vid(c))
    H, W = c.hw
    x = torch.randn(CONV_B, c.C, H, W, generator=g) * 2.0
    weight = torch.randn(c.N, c.C, 3, 3, generator=g) * (9 * c.C) ** -0.5
    bias = torch.randn(c.N, generator=g) * 0.3
    want = torch.nn.functional.conv2d(x.double(), weight.double(), bias.double(), padding=1)
    if c.relu:
        want = torch.relu(want)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1)                     # (B, H + 2, W + 2, C)
    cols = torch.cat([xp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], dim=-1).reshape(CONV_B * H * W, 9 * c.C)
    wmat = weight.permute(0, 2, 3, 1).reshape(c.N, 9 * c.C).contiguous()
    return VProblem(x, weight, bias, cols, wmat, want.permute(0, 2, 3, 1).reshape(CONV_B * H * W, c.N))


def conv_emulation(c):
    p = conv_problem(c)
    return emu_gemm(p.cols, p.wmat, p.bias, None, 2 if c.relu else 0, 1.0, 1.0, "hl8", c.outf)


SProblem = collections.namedtuple("SProblem", "a w cb mask want")


@functools.lru_cache(maxsize=None)
def softmax_problem(c):
    """a (NO, NI, M, K) (softmax_bias: shared by the inner items, as the folded fusion attention shares the visual stream), w (NO, NI, N, K),
    cb (NO, NI, N) with one column per item that moves the row maximum, mask (NO, L) uint8 | None"""
    g = gen("softmax-" + sid(c))
    a = torch.randn(NO, NI, c.M, SM_K, generator=g) * 2.0
    cb = None
    if c.entry == "softmax_bias":
        a = a[:, :1].expand(NO, NI, c.M, SM_K)
        cb = torch.randn(NO, NI, c.N, generator=g) * 0.5
        cb[:, :, torch.randint(0, c.L, (1,), generator=g)] = 4.0
    w = torch.randn(NO, NI, c.N, SM_K, generator=g) * SM_K ** -0.5
    mask = None
    if c.mask != "none":
        mask = (torch.rand(NO, c.L, generator=g) > 0.3).to(torch.uint8)
        mask[torch.arange(NO), torch.randint(0, c.L, (NO,), generator=g)] = 1
        if c.mask == "item":
            mask[1] = 0
    return SProblem(a, w, cb, mask, ref_softmax(a, w, cb, mask, c.L, c.clamp, SM_ALPHA))


def softmax_emulation(c):
    p = softmax_problem(c)
    return emu_softmax(p.a, p.w, p.cb, p.mask, c.L, c.clamp, SM_ALPHA)


WRAPPER_MNK = {"matmul_nt_batched": (3, 37, 13, 32), "gemm_split_k-nk1": (1, 40, 264, 128), "gemm_split_k-nk4": (4, 40, 264, 128)}
CONVT = dict(B=2, H=3, W=5, Cin=32, Cout=16)


@functools.lru_cache(maxsize=None)
def wrapper_problem(name):
    g = gen("wrapper-" + name)
    if name.startswith("convt"):
        x = torch.randn(CONVT["B"], CONVT["Cin"], CONVT["H"], CONVT["W"], generator=g) * 2.0
        weight = torch.randn(CONVT["Cin"], CONVT["Cout"], 2, 2, generator=g) * CONVT["Cin"] ** -0.5
        bias = torch.randn(CONVT["Cout"], generator=g) if name == "convt-bias" else None
        want = torch.nn.functional.conv_transpose2d(x.double(), weight.double(), None if bias is None else bias.double(), stride=2)
        return x, weight, bias, want.permute(0, 2, 3, 1)
    B, M, N, K = WRAPPER_MNK[name]
    if name == "matmul_nt_batched":
        a, w = torch.randn(B, M, K, generator=g) * 2.0, torch.randn(B, N, K, generator=g) * K ** -0.5
        return a, w, 0.5, 0.5 * torch.einsum("bmk,bnk->bmn", a.double(), w.double())
    a, w = torch.randn(M, K, generator=g) * 2.0, torch.randn(N, K, generator=g) * K ** -0.5
    return a, w, B, a.double() @ w.double().t()


def wrapper_emulations():
    out = []
    a, w, alpha, want = wrapper_problem("matmul_nt_batched")
    out.append(("matmul_nt_batched", torch.stack([emu_gemm(a[b], w[b], None, None, 0, alpha, 1.0, "hl8", "f32") for b in range(a.shape[0])]), want))
    for nk in (1, 4):
        a, w, _, want = wrapper_problem("gemm_split_k-nk%d" % nk)
        Kc = a.shape[1] // nk
        parts = [emu_product(a[:, k * Kc:(k + 1) * Kc], w[:, k * Kc:(k + 1) * Kc], "hl8") for k in range(nk)]
        out.append(("gemm_split_k-nk%d" % nk, torch.stack(parts).sum(0), want))
    for name in ("convt-bias", "convt-nobias"):
        x, weight, bias, want = wrapper_problem(name)
        rows = x.permute(0, 2, 3, 1).reshape(-1, CONVT["Cin"])
        got = torch.zeros(CONVT["B"], 2 * CONVT["H"], 2 * CONVT["W"], CONVT["Cout"])
        for i, j in itertools.product(range(2), range(2)):
            y = emu_gemm(rows, weight[:, :, i, j].t().contiguous(), bias, None, 0, 1.0, 1.0, "hl8", "f32")
            got[:, i::2, j::2] = y.view(CONVT["B"], CONVT["H"], CONVT["W"], CONVT["Cout"])
        out.append((name, got, want))
    return out


# ------------------------------------------------------------------------------------------------------------------- CPU tests
def test_matrix_reaches_every_line():
    """every launch line is the launch_line of a case, tile-kernel lines in both operand formats; the named neighbours stay off their kernel"""
    lines = collections.Counter(line_of(c) for c in TILE_CASES)
    lines.update(launch_line("batched", N=c.N) for c in BATCHED)
    lines.update(launch_line("bresid", N=c.N) for c in BRESID)
    lines.update(launch_line("conv", N=c.N, in_fmt=c.inf) for c in CONV)
    lines.update(launch_line(c.entry) for c in SOFTMAX)
    assert set(lines) == set(ALL_LINES), (set(ALL_LINES) - set(lines), set(lines) - set(ALL_LINES))
    for group, cases, want in (("small", SMALL, "small"), ("wide16", WIDE16, "wide16"), ("plain", PLAIN, "plain"), ("big", BIG_GATHER, "big256"),
                               ("k256", THIN, "k256")):
        assert all(line_of(c).startswith(want) for c in cases), group
    for c in BIG_DIRECT:
        assert line_of(c) == "%s/%s" % (BIG_DIRECT_LINE[c.M], c.inf)
    assert all(not line_of(c).startswith("k256") for c in THIN_NEIGHBOURS)
    for line, (N, inf, gather) in EPI_LINES.items():
        mine = [c for c in EPILOGUE if (c.N, c.inf, c.gather) == (N, inf, gather)]
        assert all(line_of(c) == line for c in mine)
        assert {(c.outf, c.act, c.res) for c in mine} >= set(itertools.product(("f32", "f16", "hl8"), (0, 1, 2, 3), (False, True)))
        assert any(c.bias is None for c in mine) and {c.outf for c in mine if c.over} == {"hl8", "f16"}
    assert {line_of(c) for c in SUBNORMAL} == {"small/hl8", "big256/hl8", "big256/f32", "wide16/hl8", "k256/hl8"}
    assert {line_of(c) for c in ROW_MAP} == {"small/hl8", "big256/hl8"} and {c.outf for c in ROW_MAP} == {"f32", "hl8"}
    # the axes of the small matrix, the stage counts of the big one, group_m with a short last group
    assert {c.M for c in SMALL} == {1, 63, 65, 129} and {c.N for c in SMALL} == {8, 128, 136, 264} and {c.K for c in SMALL} == {32, 64, 96, 128, 256}
    assert {c.K for c in BIG_GATHER if c.N == 264} == {32, 64, 96} and {c.gather for c in BIG_GATHER} == {"id", "perm", "rep"}
    assert -(-1288 // 256) == 6 > 4 and -(-2305 // 256) == 10 and 10 % 8 != 0
    assert {(c.M, c.N) for c in THIN} == set(itertools.product((8192, 8193, 8319), (384, 416))) and (416 // 32) % 2 == 1
    assert {(c.N, c.outf) for c in BATCHED} == set(itertools.product((264, 320, 640), ("f32", "hl8")))
    assert {c.M for c in BATCHED} == {1, 257} and {c.K for c in BATCHED} == {32, 96} and {c.share for c in BATCHED} == {"a", "w"}
    assert {(c.C, c.N) for c in CONV} == set(itertools.product((32, 64), (264, 320))) and {(c.inf, c.outf) for c in CONV} == set(itertools.product(("hl8", "f32"), repeat=2))
    for entry in ("softmax", "softmax_bias"):
        mine = [c for c in SOFTMAX if c.entry == entry]
        assert {(c.N, c.L) for c in mine} == {(N, L) for N in (8, 136, 256) for L in (1, N - 3, N)}
        for N in (8, 136, 256):
            assert {c.mask for c in mine if c.N == N} == set(SM_MASKS) and {c.clamp for c in mine if c.N == N} == set(SM_CLAMPS)
            assert {c.M for c in mine if c.N == N} == {1, 257}
    assert all((-(-M // 256) * NI) % 8 != 0 for M in (1, 257))          # VAR 8 tile map: a block count that is no multiple of 8


def test_mirror_is_pinned_to_the_source():
    """the literals launch_line copies are still in gemm.hip: a changed threshold fails here instead of moving cases to another kernel"""
    with open(os.path.join(ROOT, "hipie_amd", "csrc", "gemm.hip")) as f:
        src = f.read()
    for lit in ("96L", "N >= 384", "M >= 8192", "N % 32 == 0", "N % 320 == 0", "small_ok && a_row == nullptr", "K == 256",
                "alpha == 1.f && oscale == 1.f", "ldw * 2 == 1024", "((M + 255) / 256)"):
        assert lit in src, lit


def test_references_agree():
    """the torch float64 references and the loop forms agree to 1e-12 on tiny inputs with every epilogue switch and mask kind"""
    g = gen("agree")
    a, w = torch.randn(5, 32, generator=g) * 2.0, torch.randn(8, 32, generator=g) * 32 ** -0.5
    bias = torch.randn(8, generator=g)
    bias[:7] = torch.tensor(EXTREMES)
    a[1] = 0.0
    resid = torch.randn(5, 8, generator=g)
    for act, res, b, alpha, osc in ((0, None, None, 1.0, 1.0), (1, resid, bias, 0.5, 4.0), (2, None, bias, 0.5, 1.0), (3, resid, bias, 1.0, 4.0)):
        want, got = ref_epilogue(a, w, b, res, act, alpha, osc), loops_gemm(a, w, b, res, act, alpha, osc)
        assert float((want - got).abs().max()) <= 1e-12 * float(want.abs().max()), act
    for c in (_S("softmax", 8, 5, 1, "holes", CLAMP_BIND), _S("softmax_bias", 8, 8, 1, "item", 0.0), _S("softmax_bias", 8, 1, 1, "none", 50000.0)):
        p = softmax_problem(c)
        got = loops_softmax(p.a, p.w, p.cb, p.mask, c.L, c.clamp, SM_ALPHA)
        assert float((p.want - got).abs().max()) <= 1e-12


def test_im2col_is_the_convolution():
    """the im2col rows and weight order the emulation (and the raw entry's weight operand) use give F.conv2d"""
    for c in CONV[:2]:
        p = conv_problem(c)
        y = p.cols.double() @ p.wmat.double().t() + p.bias.double()
        y = torch.relu(y) if c.relu else y
        assert float((y - p.want).abs().max()) <= 1e-12 * float(p.want.abs().max())


def test_inputs_have_their_properties():
    """planted rows and columns are where the tests look for them; the binding clamp binds, the 50000 one does not, the masked item exists"""
    for c in EPILOGUE:
        p = tile_problem(c)
        if c.bias == "ext":
            assert torch.equal(p.bias[8:15], torch.tensor(EXTREMES)) and int(p.a[list(ZERO_ROWS)].abs().sum()) == 0
            pre = c.alpha * (p.a.double() @ p.w.double().t()) + p.bias.double()
            assert torch.equal(pre[list(ZERO_ROWS)], p.bias.double().expand(4, -1))
        if c.over:
            assert float(p.want[:, 40].min()) > 65520 and float(p.want[:, 41].max()) < -65520
        assert bool(torch.isfinite(p.want).all())
    for c in ROW_MAP + [c for c in THIN_NEIGHBOURS if c.out_row]:
        p = tile_problem(c)
        live = p.out_row[p.out_row >= 0]
        assert int((p.out_row < 0).sum()) == c.M // 4 and live.unique().numel() == live.numel() and int(live.max()) < c.M + 5
    for c in SOFTMAX:
        p = softmax_problem(c)
        free = _logits(p.a, p.w, p.cb, SM_ALPHA, 0.0, torch.float64)
        changed = float((free.abs() > c.clamp).double().mean()) if c.clamp > 0 else 0.0
        assert changed >= BIND_SHARE if c.clamp == CLAMP_BIND else changed == 0.0, (sid(c), changed)
        if c.mask == "item":
            assert int(p.mask[1].sum()) == 0 and int(p.mask[0].sum()) > 0 and int(torch.count_nonzero(p.want[1])) == 0
        if c.mask == "holes":
            assert bool((p.mask.sum(1) > 0).all())
        if p.cb is not None and c.L > 1:                        # the column bias moves the row maximum
            assert float((free.argmax(-1) != _logits(p.a, p.w, None, SM_ALPHA, 0.0, torch.float64).argmax(-1)).double().mean()) > 0.2
        sums = p.want.sum(-1)
        assert bool(((sums - 1).abs() < 1e-12).logical_or(sums == 0).all())


def emulation_groups(group):
    """(group, output format) -> list of (id, emulation, reference) for the cases of one group; all groups = every case of every matrix"""
    groups = collections.defaultdict(list)
    for c in (c for c in TILE_CASES if c.group == group):
        p = tile_problem(c)
        groups[c.group, c.outf].append((gid(c), lambda c=c: tile_emulation(c), ref_out(p.want, c.outf)))
    for c in {"batched": BATCHED, "bresid": BRESID}.get(group, []):
        groups[group, c.outf].append((bid(c), lambda c=c: batched_emulation(c), batched_problem(c).want))
    for c in CONV if group == "conv" else []:
        groups["conv", c.outf].append((vid(c), lambda c=c: conv_emulation(c), conv_problem(c).want))
    for c in SOFTMAX if group == "softmax" else []:
        groups["softmax", "hl8"].append((sid(c), lambda c=c: softmax_emulation(c), softmax_problem(c).want))
    return groups


EMU_GROUPS = ["small", "big", "wide16", "plain", "epilogue", "rowmap", "k256", "subnormal", "batched", "bresid", "conv", "wrappers", "softmax"]


@pytest.mark.parametrize("group", EMU_GROUPS)
def test_emulation_within_bound(group):
    """the bounds are attainable: the format choice alone stays within half of each (fp16: one rounding + 1.5e-6) on every case, and
    EMULATION_ERR is what it says.  The softmax group has no project bound: its entry defines SOFTMAX_BOUND"""
    if group == "wrappers":
        items = {("wrappers", "f32"): [(n, lambda e=e: e, w) for n, e, w in wrapper_emulations()]}
    else:
        items = {k: v for k, v in emulation_groups(group).items() if k[0] == group}
    assert items
    for (grp, outf), cases in sorted(items.items()):
        worst = 0.0
        for name, emu, want in cases:
            e = block_err(emu(), want)
            print("emulation %s %s %s: %.3e" % (grp, outf, name, e))
            if grp != "softmax":
                assert e <= (SUBNORMAL_BOUND / 2 if grp == "subnormal" else EMU_BOUND[outf]), (name, e)
            worst = max(worst, e)
        print("emulation worst %s %s: %.3e" % (grp, outf, worst))
        rec = EMULATION_ERR[grp, outf]
        assert 0.5 * rec <= worst <= rec, (grp, outf, worst, rec)
    if group == "softmax":
        assert SOFTMAX_BOUND == 4 * EMULATION_ERR["softmax", "hl8"]


# --------------------------------------------------------------------------------------------------------------------- GPU
def poisoned(shape, dtype):
    """free a NaN-filled device block: the allocator hands the most recently freed block of a size to the next torch.empty of that
    size, so an element the kernel does not write reads NaN"""
    block = torch.full(shape, math.nan, dtype=dtype, device=DEV)
    del block


def planes(t):
    """HL8 (..., 2N) fp16 -> (hi, lo) fp32 planes (..., N)"""
    pl = t.float().reshape(*t.shape[:-1], t.shape[-1] // 16, 2, 8)
    return pl[..., 0, :].reshape(*t.shape[:-1], -1), pl[..., 1, :].reshape(*t.shape[:-1], -1)


def value_of(out, outf):
    """device output -> CPU fp32 values; an HL8 output also has to satisfy the plane condition |lo| <= |hi| 2^-11 + 2^-24"""
    out = out.cpu()
    if outf != "hl8":
        return out.float()
    hi, lo = planes(out)
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -11 + 2.0 ** -24).all()), "HL8 planes: lo is not the remainder of hi"
    return hi + lo


def report(line, name, e, bound):
    print("block_err %s %s: %.3e (bound %.1e)" % (line, name, e, bound))
    assert e < bound, (line, name, e)


def run_tile(c, outf=None):
    """one ops.gemm call for case c -> (values (rows, N) fp32 on the CPU in OUTPUT row order, raw output tensor on the CPU)"""
    from hipie_amd import ops
    outf = outf or c.outf
    p = tile_problem(c)
    fmt = {"f32": ops.F32, "f16": ops.F16, "hl8": ops.HL8}[outf]
    width = {"f32": c.N, "f16": c.N, "hl8": 2 * c.N}[outf]
    odt = torch.float32 if outf == "f32" else torch.float16
    if c.inf == "f16":
        A, W = p.tab.half().to(DEV), p.w.half().to(DEV)
    else:
        W = ops.hl8_pack(p.w).to(DEV)
        src = p.tab if c.inf == "f32" else ops.hl8_pack(p.tab)
        if c.strided:                                            # a column block of a wider tensor: row stride > row length, 128-byte offset
            wide = torch.zeros(src.shape[0], src.shape[1] + (64 if c.inf == "f32" else 128), dtype=src.dtype, device=DEV)
            off = 32 if c.inf == "f32" else 64
            A = wide[:, off:off + src.shape[1]]
            A.copy_(src)
        else:
            A = src.to(DEV)
    if c.wide_w:                                                 # weight rows of a wider tensor: ops.gemm takes dense weights only, so the raw entry
        from hipie_amd import _lib
        assert c.inf == "hl8" and not (c.res or c.out_row or c.gather or c.strided)
        ww = torch.zeros(c.N, 2 * c.K + 64, dtype=torch.float16, device=DEV)
        ww[:, :2 * c.K] = W
        out, b = torch.full((c.M, width), math.nan, dtype=odt, device=DEV), p.bias.to(DEV)
        rc = _lib.load().hipie_gemm(A.data_ptr(), A.stride(0), ww.data_ptr(), ww.stride(0), b.data_ptr(), None, 0,
                                    out.data_ptr(), width, None, c.M, c.N, c.K, ops.HL8, fmt, c.act, c.alpha, c.osc, ops._stream())
        _lib.check(rc, "hipie_gemm")
        return out.cpu()
    kw = dict(out_fmt=fmt, act=c.act, alpha=c.alpha, oscale=c.osc, split=c.inf != "f16")
    bias = None if p.bias is None else p.bias.to(DEV)
    if p.a_row is not None:
        kw["a_row"] = p.a_row.to(DEV)
    if p.out_row is not None:
        R = c.M + 5
        resid = None if p.resid is None else p.resid.to(DEV)
        out = resid if c.inplace else torch.full((R, width), SENTINEL, dtype=odt, device=DEV)
        before = out.clone()
        ops.gemm(A, W, bias, resid, out=out, out_row=p.out_row.to(DEV), **kw)
        dead = torch.ones(R, dtype=torch.bool)
        dead[p.out_row[p.out_row >= 0].long()] = False
        assert torch.equal(out.cpu()[dead], before.cpu()[dead]), "a row no product row maps to was written"
        return out.cpu()[p.out_row.long().clamp_min(0)]
    resid = None if p.resid is None else p.resid.to(DEV)
    if c.strided:                                                # strided output rows inside a sentinel frame
        pad = torch.full((c.M + 3, width + 8), SENTINEL, dtype=odt, device=DEV)
        ops.gemm(A, W, bias, resid, out=pad[1:c.M + 1, :width], **kw)
        pad = pad.cpu()
        assert bool((pad[0] == SENTINEL).all()) and bool((pad[c.M + 1:] == SENTINEL).all()) and bool((pad[:, width:] == SENTINEL).all())
        return pad[1:c.M + 1, :width]
    poisoned((c.M, width), odt)
    out = ops.gemm(A, W, bias, resid, **kw)
    assert out.shape == (c.M, width) and out.dtype == odt
    return out.cpu()


def check_tile(c):
    p = tile_problem(c)
    raw = run_tile(c)
    live = live_rows(p)
    e = block_err(value_of(raw, c.outf)[live], ref_out(p.want, c.outf)[live])
    report(line_of(c), gid(c), e, bound_of(c))
    return raw


@gpu
@pytest.mark.parametrize("c", SMALL, ids=gid)
def test_small(c):
    check_tile(c)


@gpu
@pytest.mark.parametrize("c", BIG_DIRECT, ids=gid)
def test_big_direct(c):
    check_tile(c)


@gpu
@pytest.mark.parametrize("c", BIG_GATHER, ids=gid)
def test_big_gather(c):
    check_tile(c)


@gpu
@pytest.mark.parametrize("c", WIDE16, ids=gid)
def test_wide16(c):
    check_tile(c)


@gpu
@pytest.mark.parametrize("c", PLAIN, ids=gid)
def test_plain(c):
    check_tile(c)


@gpu
@pytest.mark.parametrize("c", SUBNORMAL, ids=lambda c: line_of(c).replace("/", "_") + "-" + gid(c))
def test_subnormal_lo_halves(c):
    check_tile(c)


@gpu
@pytest.mark.parametrize("c", EPILOGUE, ids=lambda c: line_of(c).replace("/", "_") + "-" + gid(c))
def test_epilogue(c):
    raw = check_tile(c)
    if c.over and c.outf == "hl8":                               # saturation: hi = +-65504, lo finite
        hi, lo = planes(raw)
        assert bool((hi[:, 40] == 65504.0).all()) and bool((hi[:, 41] == -65504.0).all()) and bool(torch.isfinite(lo).all())
    if c.over and c.outf == "f16":                               # the fp16 output is .half() of the fp32 output of the same call
        assert torch.equal(raw, run_tile(c, "f32").half()) and bool(torch.isinf(raw[:, 40:42]).all())


@gpu
@pytest.mark.parametrize("c", ROW_MAP, ids=lambda c: line_of(c).replace("/", "_") + "-" + gid(c))
def test_row_map(c):
    check_tile(c)


@gpu
@pytest.mark.parametrize("c", THIN + THIN_NEIGHBOURS, ids=gid)
def test_thin_k(c):
    check_tile(c)


def hl8_dev(t):
    from hipie_amd import ops
    return ops.hl8_pack(t).to(DEV)


def framed(lead, M, width, dtype):
    """an output buffer (*lead, M + 1, width + 8) full of the sentinel: item (o, i) owns [o, i, :M, :width]; row stride and item strides"""
    buf = torch.full(tuple(lead) + (M + 1, width + 8), SENTINEL, dtype=dtype, device=DEV)
    ldo = width + 8
    return buf, ldo, NI * (M + 1) * ldo, (M + 1) * ldo


def check_frame(buf, M, width):
    assert bool((buf[..., M:, :] == SENTINEL).all()) and bool((buf[..., width:] == SENTINEL).all()), "written outside the batch item"


def batched_operands(p, c):
    """device HL8 operands with distinct outer / inner strides; the shared one has a zero stride"""
    K2 = 2 * c.K
    if c.share == "a":
        A = hl8_dev(p.a[:, 0])                                   # (NO, M, 2K): the inner items share A
        a_str = (K2, c.M * K2, 0)
    else:
        A = hl8_dev(p.a).permute(0, 2, 1, 3).reshape(NO, c.M, NI * K2).contiguous()
        a_str = (NI * K2, c.M * NI * K2, K2)                     # inner item i = column block i of a wider row
    if c.share == "w":
        W = hl8_dev(p.w[0])                                      # (NI, N, 2K): the outer items share W
        w_str = (K2, 0, c.N * K2)
    else:
        W = hl8_dev(p.w)
        w_str = (K2, NI * c.N * K2, c.N * K2)
    return A, a_str, W, w_str


@gpu
@pytest.mark.parametrize("c", BATCHED, ids=bid)
def test_batched(c):
    from hipie_amd import _lib, ops
    lib, p = _lib.load(), batched_problem(c)
    A, (lda, a_o, a_i), W, (ldw, w_o, w_i) = batched_operands(p, c)
    width = c.N if c.outf == "f32" else 2 * c.N
    buf, ldo, o_o, o_i = framed((NO, NI), c.M, width, torch.float32 if c.outf == "f32" else torch.float16)
    rc = lib.hipie_gemm_batched(A.data_ptr(), lda, a_o, a_i, W.data_ptr(), ldw, w_o, w_i, buf.data_ptr(), ldo, o_o, o_i, NO, NI, c.M, c.N, c.K,
                                ops.F32 if c.outf == "f32" else ops.HL8, 0.25, ops._stream())
    _lib.check(rc, "hipie_gemm_batched")
    buf = buf.cpu()
    check_frame(buf, c.M, width)
    report(launch_line("batched", N=c.N), bid(c), block_err(value_of(buf[:, :, :c.M, :width], c.outf), p.want), BOUND[c.outf])


@gpu
@pytest.mark.parametrize("c", BRESID, ids=bid)
def test_batched_resid(c):
    from hipie_amd import _lib, ops
    lib, p = _lib.load(), batched_problem(c)
    A, (lda, a_o, a_i), W, (ldw, w_o, w_i) = batched_operands(p, c)
    buf, ldo, o_o, o_i = framed((NO, NI), c.M, c.N, torch.float32)
    bias = p.bias.to(DEV)
    r, ldr, r_o, r_i = None, 0, 0, 0
    if p.resid is not None:                                      # the residual has strides of its own: rows of N + 4, items of M + 2 rows
        r = torch.zeros(NO, NI, c.M + 2, c.N + 4, device=DEV)
        r[:, :, :c.M, :c.N] = p.resid.to(DEV)
        ldr, r_o, r_i = c.N + 4, NI * (c.M + 2) * (c.N + 4), (c.M + 2) * (c.N + 4)
    rc = lib.hipie_gemm_batched_resid(A.data_ptr(), lda, a_o, a_i, W.data_ptr(), ldw, w_o, w_i, bias.data_ptr(), None if r is None else r.data_ptr(),
                                      ldr, r_o, r_i, buf.data_ptr(), ldo, o_o, o_i, NO, NI, c.M, c.N, c.K, 0.25, ops._stream())
    _lib.check(rc, "hipie_gemm_batched_resid")
    buf = buf.cpu()
    check_frame(buf, c.M, c.N)
    report(launch_line("bresid", N=c.N), bid(c), block_err(buf[:, :, :c.M, :c.N], p.want), BOUND["f32"])


@gpu
def test_matmul_nt_batched():
    from hipie_amd import ops
    a, w, alpha, want = wrapper_problem("matmul_nt_batched")
    ad, wd = a.to(DEV), w.to(DEV)
    poisoned((a.shape[0], a.shape[1], -(-w.shape[1] // 8) * 8), torch.float32)
    got = ops.matmul_nt_batched(ad, wd, alpha)
    assert got.shape == want.shape
    report("batched256", "matmul_nt_batched", block_err(got.cpu(), want), BOUND["f32"])


@gpu
@pytest.mark.parametrize("nk", [1, 4])
def test_gemm_split_k(nk):
    from hipie_amd import ops
    a, w, _, want = wrapper_problem("gemm_split_k-nk%d" % nk)
    poisoned((nk, a.shape[0], w.shape[0]), torch.float32)
    got = ops.gemm_split_k(hl8_dev(a), hl8_dev(w), nk)
    report("batched256", "gemm_split_k-nk%d" % nk, block_err(got.cpu(), want), BOUND["f32"])


@gpu
@pytest.mark.parametrize("name", ["convt-bias", "convt-nobias"])
def test_convt2x2_split(name):
    from hipie_amd import ops
    x, weight, bias, want = wrapper_problem(name)
    rows = x.permute(0, 2, 3, 1).reshape(-1, CONVT["Cin"]).contiguous().to(DEV)
    owner = type("_Owner", (), {})()
    poisoned(tuple(want.shape), torch.float32)
    got = ops.convt2x2_split(rows, owner, "up", weight.to(DEV), None if bias is None else bias.to(DEV), CONVT["B"], CONVT["H"], CONVT["W"])
    assert got.shape == want.shape
    report("small/f32", name, block_err(got.cpu().reshape(-1, CONVT["Cout"]), want.reshape(-1, CONVT["Cout"])), BOUND["f32"])


@gpu
@pytest.mark.parametrize("c", CONV, ids=vid)
def test_conv3x3(c):
    """the raw entry on a zero-padded pixel grid with guard rows built here, as ops.conv3x3_split builds it (conv3x3_split_ok admits none
    of these maps: it asks for 16384 padded pixels and full 256-column tiles)"""
    from hipie_amd import _lib, ops
    lib, p = _lib.load(), conv_problem(c)
    H, W = c.hw
    Hp, Wp = H + 2, W + 2
    guard, rows = Wp + 1, CONV_B * Hp * Wp
    grid = torch.zeros(rows + 2 * guard, c.C)
    grid[guard:guard + rows].view(CONV_B, Hp, Wp, c.C)[:, 1:-1, 1:-1] = p.x.permute(0, 2, 3, 1)
    xin = (grid.to(DEV) if c.inf == "f32" else hl8_dev(grid))[guard:]
    wm, bias = hl8_dev(p.wmat), p.bias.to(DEV)
    width = c.N if c.outf == "f32" else 2 * c.N
    buf = torch.full((rows + 2, width + 8), SENTINEL, dtype=torch.float32 if c.outf == "f32" else torch.float16, device=DEV)
    rc = lib.hipie_conv3x3_split(xin.data_ptr(), c.C if c.inf == "f32" else 2 * c.C, wm.data_ptr(), bias.data_ptr(), buf.data_ptr(), width + 8, rows, Wp,
                                 c.C, c.N, ops.F32 if c.inf == "f32" else ops.HL8, ops.F32 if c.outf == "f32" else ops.HL8, 2 if c.relu else 0, ops._stream())
    _lib.check(rc, "hipie_conv3x3_split")
    buf = buf.cpu()
    assert bool((buf[rows:] == SENTINEL).all()) and bool((buf[:, width:] == SENTINEL).all())
    got = value_of(buf[:rows, :width], c.outf).view(CONV_B, Hp, Wp, c.N)[:, 1:-1, 1:-1].reshape(CONV_B * H * W, c.N)
    report(launch_line("conv", N=c.N, in_fmt=c.inf), vid(c), block_err(got, p.want), BOUND[c.outf])


@gpu
@pytest.mark.parametrize("c", SOFTMAX, ids=sid)
def test_softmax(c):
    from hipie_amd import _lib, ops
    lib, p = _lib.load(), softmax_problem(c)
    K2 = 2 * SM_K
    if c.entry == "softmax_bias":
        A, (lda, a_o, a_i) = hl8_dev(p.a[:, 0]), (K2, c.M * K2, 0)
    else:
        A, (lda, a_o, a_i) = hl8_dev(p.a).permute(0, 2, 1, 3).reshape(NO, c.M, NI * K2).contiguous(), (NI * K2, c.M * NI * K2, K2)
    W = hl8_dev(p.w)
    buf, ldo, o_o, o_i = framed((NO, NI), c.M, 2 * c.N, torch.float16)
    mask = None if p.mask is None else p.mask.contiguous().to(DEV)
    mp = None if mask is None else mask.data_ptr()
    if c.entry == "softmax_bias":
        cb = p.cb.contiguous().to(DEV)
        rc = lib.hipie_gemm_batched_softmax_bias(A.data_ptr(), lda, a_o, a_i, W.data_ptr(), K2, NI * c.N * K2, c.N * K2, buf.data_ptr(), ldo, o_o, o_i,
                                                 NO, NI, c.M, c.N, SM_K, mp, c.L, cb.data_ptr(), c.clamp, SM_ALPHA, ops._stream())
    else:
        rc = lib.hipie_gemm_batched_softmax(A.data_ptr(), lda, a_o, a_i, W.data_ptr(), K2, NI * c.N * K2, c.N * K2, buf.data_ptr(), ldo, o_o, o_i,
                                            NO, NI, c.M, c.N, SM_K, mp, c.L, c.clamp, SM_ALPHA, ops._stream())
    _lib.check(rc, "hipie_gemm_batched_" + c.entry)
    buf = buf.cpu()
    check_frame(buf, c.M, 2 * c.N)
    raw = buf[:, :, :c.M, :2 * c.N]
    got = value_of(raw, "hl8")
    report(c.entry, sid(c), block_err(got, p.want), SOFTMAX_BOUND)
    off = ~_valid(p.mask, NO, c.N, c.L)                          # masked and padded columns: exact zeros in both planes
    hi, lo = planes(raw)
    for b in range(NO):
        assert int(torch.count_nonzero(hi[b][..., off[b]])) == 0 and int(torch.count_nonzero(lo[b][..., off[b]])) == 0
    sums = got.double().sum(-1)
    alive = _valid(p.mask, NO, c.N, c.L).any(1)
    assert bool(((sums[alive] - 1).abs() < SOFTMAX_BOUND).all()) and int(torch.count_nonzero(got[~alive])) == 0
