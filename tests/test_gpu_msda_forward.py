"""MSDA forward (hipie_amd/csrc/msda.hip: ops.msda_fused / ops.ms_deform_attn_forward) against float64 references, over every dispatch
branch of the file:

  d32 map 2       msda_d32_kernel, Lq == S, dense level_start, every level a multiple of 4 rows x 8 columns (the encoder)
  map-2 fallback  Lq == S but a level does not divide, or level_start has gaps / trailing rows: the kernel takes map 1
  d32 map 1       msda_d32_kernel, Lq != S (the decoder; the unfused op with Lq != S)
  generic         msda_generic_kernel, D != 32
  f64             msda_f64_kernel (the unfused op in double)

References.  `ref_fused` upcasts the values the kernel actually reads (16-bit operands are rounded first) to float64, forms the sampling
locations (ops/modules/ms_deform_attn.py:99-114) and the softmax in float64 and calls oracle.ops.ms_deform_attn_core in float64.
`ref_loops` is a second, independent statement: plain per-sample loops in numpy float64 with the reference op's nested conditions; the
unmarked tests at the top check on the CPU that the two agree to 1e-12 on every exact-edge input.

Tolerances (header of tests/test_gpu_kernels.py, metric util.rel_err = max|diff| / max|ref|): fp32 2e-5; f16 1e-3 and bf16 8e-3 against
the reference fed the same rounded inputs; f64 1e-12.  The two geometries with levels above 64 pixels derive their fp32 bound from the
measured error of the oracle run in float32 (LARGE_GEOMETRY_F32_ORACLE_ERR below, docs/measurements.md); no bound comes from the kernel."""
import itertools

import numpy as np
import pytest
import torch

from oracle import ops as oo
from util import rel_err

torch.set_grad_enabled(False)
DEV = "cuda"
gpu = pytest.mark.gpu
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
TOL = {F32: 2e-5, F16: 1e-3, BF16: 8e-3, F64: 1e-12}
DT_CODE = {F32: 0, F16: 1, BF16: 2}
NAME = {F32: "f32", F16: "f16", BF16: "bf16", F64: "f64"}

# Error of oracle.ops.ms_deform_attn_core run in float32 (locations and softmax in float32 too) against ref_fused on the same inputs,
# measured on the CPU by `f32_oracle_error` below (test_recorded_f32_oracle_errors re-measures them), rel_err metric.  The kernel's fp32 bound on these geometries is
# max(2e-5, 4 x measured): the factor 4 covers a different summation order and expf.
LARGE_GEOMETRY_F32_ORACLE_ERR = {
    "bench_128": 3.07e-6,       # 128/64/32/16 levels, B = 2, query subset of test_msda_fused_full_scale_strided_aux: bound 2e-5 (4 x = 1.23e-5)
    "batch_256": 1.005e-5,      # 256/128/64/32 levels, ref_dim 4, last image of test_large_batch_offset: bound 4.02e-5
}


def large_geometry_f32_bound(name):
    return max(TOL[F32], 4 * LARGE_GEOMETRY_F32_ORACLE_ERR[name])


# --------------------------------------------------------------------------------------------------------------- references
def dense_lstart(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def level_rows(shapes, lstart):
    """rows of the (possibly gapped) value layout that hold the levels, in the packed order the oracle expects"""
    return torch.cat([torch.arange(int(lstart[l]), int(lstart[l]) + int(shapes[l, 0]) * int(shapes[l, 1])) for l in range(shapes.shape[0])])


def fused_locations(shapes, ref, off, dtype=F64):
    """ops/modules/ms_deform_attn.py:99-114: ref (B,Lq,L,2|4), off (B,Lq,M,L,P,2) -> sampling locations (B,Lq,M,L,P,2)"""
    ref, off = ref.to(dtype), off.to(dtype)
    P = off.shape[4]
    if ref.shape[-1] == 2:
        norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(dtype)
        return ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    return ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5


def ref_fused(value, shapes, lstart, ref, off, logits, queries=None, dtype=F64):
    """float64 reference of ops.msda_fused from the values the kernel reads.  `queries`: compare a subset of the queries only (the op is
    independent per query).  dtype=float32 runs the same formulation in float32 (used to measure the oracle's own fp32 error)."""
    shapes, lstart = shapes.cpu(), lstart.cpu()
    if queries is not None:
        ref, off, logits = ref[:, queries], off[:, queries], logits[:, queries]
    ref, off, logits = ref.cpu(), off.cpu(), logits.cpu()
    B, Lq, M, L, P, _ = off.shape
    v = value[:, level_rows(shapes, lstart).to(value.device)].cpu().to(dtype)
    loc = fused_locations(shapes, ref, off, dtype)
    attn = torch.softmax(logits.to(dtype), -1).view(B, Lq, M, L, P)
    return oo.ms_deform_attn_core(v, shapes, loc, attn)


def ref_unfused(value, shapes, lstart, loc, attn):
    shapes, lstart = shapes.cpu(), lstart.cpu()
    v = value[:, level_rows(shapes, lstart).to(value.device)].cpu().double()
    return oo.ms_deform_attn_core(v, shapes, loc.cpu().double(), attn.cpu().double())


def ref_loops(value, shapes, lstart, loc, attn):
    """The op written straight from its formula: one loop iteration per (image, query, head, level, point), numpy float64, the reference
    op's nested conditions (a sample counts when -1 < h, w < size; each corner counts when it lies inside the map)."""
    v = value.cpu().double().numpy()
    loc, attn = loc.cpu().double().numpy(), attn.cpu().double().numpy()
    B, S, M, D = v.shape
    _, Lq, _, L, P, _ = loc.shape
    out = np.zeros((B, Lq, M, D))
    for b, q, m, l, p in itertools.product(range(B), range(Lq), range(M), range(L), range(P)):
        H, W, base = int(shapes[l, 0]), int(shapes[l, 1]), int(lstart[l])
        h_im = loc[b, q, m, l, p, 1] * H - 0.5
        w_im = loc[b, q, m, l, p, 0] * W - 0.5
        if h_im > -1 and w_im > -1 and h_im < H and w_im < W:
            h_low, w_low = int(np.floor(h_im)), int(np.floor(w_im))
            h_high, w_high = h_low + 1, w_low + 1
            lh, lw = h_im - h_low, w_im - w_low
            hh, hw = 1 - lh, 1 - lw
            v1 = v2 = v3 = v4 = np.zeros(D)
            if h_low >= 0 and w_low >= 0:
                v1 = v[b, base + h_low * W + w_low, m]
            if h_low >= 0 and w_high <= W - 1:
                v2 = v[b, base + h_low * W + w_high, m]
            if h_high <= H - 1 and w_low >= 0:
                v3 = v[b, base + h_high * W + w_low, m]
            if h_high <= H - 1 and w_high <= W - 1:
                v4 = v[b, base + h_high * W + w_high, m]
            out[b, q, m] += (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4) * attn[b, q, m, l, p]
    return torch.from_numpy(out).reshape(B, Lq, M * D)


# ------------------------------------------------------------------------------------------------------------ exact-edge inputs
EDGE_SHAPES = torch.tensor([(1, 1), (1, 8), (8, 1), (4, 8)])       # powers of two: pixel coordinate = loc * size - 0.5 is exact in fp32
EDGE_PAD = 16                                                       # rows behind the last level (random data: a read past a level shows)


def edge_coords(n):
    """pixel coordinates of one axis of size n: on and next to every threshold of the zero padding, and far outside"""
    return [-1.0, -1.0 + 2.0 ** -10, -0.5, 0.0, 0.5, n - 1.0, n - 0.5, n - 2.0 ** -10, float(n), 1e6, -1e6]


def edge_pixels(P):
    """(Lq = 121, L, P, 2) pixel coordinates (w_im, h_im): query i * 11 + j takes row coordinate i and column coordinate j of every
    level's own list; the second point of a level takes them the other way round."""
    L, n = EDGE_SHAPES.shape[0], len(edge_coords(1))
    pix = torch.zeros(n * n, L, P, 2, dtype=F64)
    for l in range(L):
        ch, cw = edge_coords(int(EDGE_SHAPES[l, 0])), edge_coords(int(EDGE_SHAPES[l, 1]))
        for i, j in itertools.product(range(n), range(n)):
            for p in range(P):
                a, b = (i, j) if p % 2 == 0 else (j, i)
                pix[i * n + j, l, p, 0], pix[i * n + j, l, p, 1] = cw[b], ch[a]
    return pix


def edge_case(D, M=2, P=1, seed=21):
    """value with EDGE_PAD trailing rows, dense level_start, sampling locations (1,121,M,L,P,2) whose pixel coordinates are exactly the
    edge coordinates (dyadic rationals: exact in fp32 and in the kernel's arithmetic), attention weights in [0.5, 1)"""
    g = torch.Generator().manual_seed(seed)
    L = EDGE_SHAPES.shape[0]
    S = int(EDGE_SHAPES.prod(1).sum()) + EDGE_PAD
    value = torch.randn(1, S, M, D, generator=g, dtype=F64)
    pix = edge_pixels(P)
    size = torch.stack([EDGE_SHAPES[:, 1], EDGE_SHAPES[:, 0]], -1).double()       # (L, 2) as (W, H)
    loc = ((pix + 0.5) / size[None, :, None, :])[None, :, None].expand(1, -1, M, -1, -1, -1).contiguous()
    attn = torch.rand(1, pix.shape[0], M, L, P, generator=g, dtype=F64) * 0.5 + 0.5
    return value, EDGE_SHAPES, dense_lstart(EDGE_SHAPES), loc, attn


def edge_case_fused(D, ref_dim, M=2, seed=22):
    """the same pixel coordinates through the fused op: dyadic ref and off such that ref + off / size (ref_dim 2, P = 1) or
    ref_xy + off / P * ref_wh * 0.5 (ref_dim 4, P = 2, ref_wh = 2 / size) is exact in fp32; random logits"""
    g = torch.Generator().manual_seed(seed)
    P = 1 if ref_dim == 2 else 2
    L = EDGE_SHAPES.shape[0]
    S = int(EDGE_SHAPES.prod(1).sum()) + EDGE_PAD
    value = torch.randn(1, S, M, D, generator=g)
    pix = edge_pixels(P)                                                           # (Lq, L, P, 2)
    Lq = pix.shape[0]
    size = torch.stack([EDGE_SHAPES[:, 1], EDGE_SHAPES[:, 0]], -1).double()       # (L, 2) as (W, H)
    ref = torch.full((1, Lq, L, ref_dim), 0.5, dtype=F64)                          # level centre
    off = pix + 0.5 - 0.5 * size[None, :, None, :]                                 # pixels from the centre
    if ref_dim == 4:
        ref[..., 2:] = 2.0 / size
        off = off * P
    off = off[None, :, None].expand(1, -1, M, -1, -1, -1).contiguous()
    assert torch.equal(off.float().double(), off) and torch.equal(ref.float().double(), ref)       # exact in fp32
    logits = torch.randn(1, Lq, M, L * P, generator=g)
    return value, EDGE_SHAPES, dense_lstart(EDGE_SHAPES), ref.float(), off.float(), logits


# ------------------------------------------------------------------------------- CPU: the references against each other (no GPU)
def test_references_agree_on_unfused_edge_inputs():
    for P in (1, 2):
        value, shapes, lstart, loc, attn = edge_case(D=4, P=P)
        want = ref_loops(value, shapes, lstart, loc, attn)
        assert rel_err(ref_unfused(value, shapes, lstart, loc, attn), want) < 1e-12
        # the pixel coordinates come out exactly: every threshold is really hit
        h_im = loc[0, :, 0, 3, 0, 1] * 4 - 0.5
        assert sorted(set(h_im.tolist())) == sorted(edge_coords(4))
        assert torch.equal(loc.float().double(), loc)


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_references_agree_on_fused_edge_inputs(ref_dim):
    value, shapes, lstart, ref, off, logits = edge_case_fused(D=4, ref_dim=ref_dim)
    B, Lq, M, L, P, _ = off.shape
    loc = fused_locations(shapes, ref, off)
    attn = torch.softmax(logits.double(), -1).view(B, Lq, M, L, P)
    want = ref_loops(value, shapes, lstart, loc, attn)
    assert rel_err(ref_fused(value, shapes, lstart, ref, off, logits), want) < 1e-12
    w_im = (loc[0, :, 0, 3, 0, 0] * 8 - 0.5).tolist()
    assert sorted(set(w_im)) == sorted(edge_coords(8))
    # the same arithmetic in fp32, in the kernel's order, lands on the same coordinates
    loc32 = fused_locations(shapes, ref, off, F32)
    assert torch.equal(loc32.double(), loc)


def test_references_agree_on_a_gapped_layout():
    g = torch.Generator().manual_seed(23)
    shapes = torch.tensor([(3, 5), (2, 2), (1, 3)])
    lstart = dense_lstart(shapes) + torch.tensor([2, 9, 13])
    S = int(lstart[-1]) + 3 + 4
    value = torch.randn(2, S, 3, 4, generator=g, dtype=F64)
    ref, off, logits = torch.rand(2, 9, 3, 4, generator=g), torch.randn(2, 9, 3, 3, 2, 2, generator=g), torch.randn(2, 9, 3, 6, generator=g)
    loc = fused_locations(shapes, ref, off)
    attn = torch.softmax(logits.double(), -1).view(2, 9, 3, 3, 2)
    want = ref_loops(value, shapes, lstart, loc, attn)
    assert rel_err(ref_fused(value, shapes, lstart, ref, off, logits), want) < 1e-12
    sub = torch.tensor([7, 0, 3])
    assert rel_err(ref_fused(value, shapes, lstart, ref, off, logits, queries=sub), want[:, sub]) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ GPU helpers
def make_inputs(shapes, B, Lq, M, D, P, ref_dim, seed, gap=None, trailing=0):
    """fp32 inputs on the CPU.  gap: rows left unused in front of level l (a list, or one number for every level but the first)"""
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor(shapes, dtype=torch.long)
    L = shapes.shape[0]
    lstart = dense_lstart(shapes)
    if gap is not None:
        gaps = torch.as_tensor(gap if isinstance(gap, (list, tuple)) else [0] + [gap] * (L - 1))
        lstart = lstart + gaps.cumsum(0)
    S = int(lstart[-1] + shapes[-1].prod()) + trailing
    Lq = S + int(Lq) if isinstance(Lq, str) else int(Lq)       # "+1" / "-1" / "+0": relative to S
    value = torch.randn(B, S, M, D, generator=g)
    if ref_dim == 2:
        ref = torch.rand(B, Lq, L, 2, generator=g)
    else:
        ref = torch.cat([torch.rand(B, Lq, L, 2, generator=g), torch.rand(B, Lq, L, 2, generator=g) * 0.5 + 0.1], -1)
    off = torch.randn(B, Lq, M, L, P, 2, generator=g) * 2      # a good share of the points falls outside the maps
    logits = torch.randn(B, Lq, M, L * P, generator=g)
    return value, shapes, lstart, ref, off, logits


F32S = "f32 strided"          # aux form: fp32 column blocks of one projection tensor (the model's call when its GEMM emits fp32)
AUX_FORMS = [F32, F32S, F16, BF16]
aux_id = lambda a: "aux_" + ("f32s" if a == F32S else NAME[a])


def aux_on_device(off, logits, adt):
    """dense fp32 offsets / logits, or the two column blocks of ONE projection tensor (fp32 / f16 / bf16) read in place through its row
    stride, which is how modeling/transformer.py passes them"""
    if adt == F32:
        return off.to(DEV), logits.to(DEV)
    B, Lq, M, L, P, _ = off.shape
    proj = torch.cat([off.flatten(2), logits.flatten(2)], -1).to(F32 if adt == F32S else adt).to(DEV)
    no = M * L * P * 2
    o, lg = proj[..., :no].unflatten(-1, (M, L, P, 2)), proj[..., no:].unflatten(-1, (M, L * P))
    assert not o.is_contiguous() or Lq * B == 1
    return o, lg


def check_fused(value, shapes, lstart, ref, off, logits, vdt=F32, adt=F32, tol=None):
    """run ops.msda_fused on the given dtypes and compare with ref_fused fed what the kernel read; returns the output"""
    from hipie_amd import ops
    v = value.to(vdt).to(DEV)
    o, lg = aux_on_device(off, logits, adt)
    got = ops.msda_fused(v, shapes.to(DEV), lstart.to(DEV), ref.to(DEV), o, lg)
    assert got.dtype == vdt and tuple(got.shape) == (value.shape[0], off.shape[1], value.shape[2] * value.shape[3])
    want = ref_fused(v, shapes, lstart, ref, o, lg)
    err = rel_err(got.float().cpu(), want)
    print("msda_fused %s/%s ref_dim %d: rel_err %.3e" % (NAME[vdt], aux_id(adt), ref.shape[-1], err))
    assert err < (TOL[vdt] if tol is None else tol), err
    return got


def fused_into(out, value, shapes, lstart, ref, off, logits):
    """hipie_msda_fused_forward_strided straight on the library, writing into a buffer the caller has filled: an unwritten row shows"""
    from hipie_amd import _lib
    lib = _lib.load()
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = off.shape
    assert value.is_contiguous() and out.is_contiguous() and shapes.dtype == lstart.dtype == torch.int64
    return lib.hipie_msda_fused_forward_strided(value.data_ptr(), 0, shapes.data_ptr(), lstart.data_ptr(), ref.data_ptr(), off.data_ptr(),
                                                logits.data_ptr(), out.data_ptr(), B, S, M, D, L, Lq, P, ref.shape[-1], DT_CODE[value.dtype],
                                                DT_CODE[off.dtype], off.stride(1), logits.stride(1), torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------- tiled map
PYR_SQUARE = [(32, 32), (16, 16), (8, 8), (4, 8)]      # S = 1376, every level a multiple of 4 x 8
PYR_RECT = [(24, 40), (12, 24), (8, 8)]                # S = 1312


@gpu
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("adt", AUX_FORMS, ids=aux_id)
@pytest.mark.parametrize("vdt", [F32, F16, BF16], ids=lambda d: "val_" + NAME[d])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pyr", [PYR_SQUARE, PYR_RECT], ids=["square", "rect"])
def test_tiled_map(pyr, B, vdt, adt, ref_dim):
    """msda_d32_kernel<T, A, FUSED>, map 2 (Lq == S, dense level_start, tileable levels): T = value dtype, A = aux dtype (fp32 dense, and
    fp32 / f16 / bf16 as strided column blocks of one projection tensor: MSDeformAttn.forward in the encoder under every precision
    policy), both reference-point forms."""
    value, shapes, lstart, ref, off, logits = make_inputs(pyr, B, "+0", 8, 32, 4, ref_dim, seed=100 + B)
    assert off.shape[1] == value.shape[1] and all(h % 4 == 0 and w % 8 == 0 for h, w in pyr)
    check_fused(value, shapes, lstart, ref, off, logits, vdt, adt)


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(16, 32), (4, 8), (32, 64)])
def test_tiled_map_identity(hw, B):
    """map 2, fp32: one level, P = 1, zero offsets, every query's reference point on its own pixel centre.  The bilinear weight of that
    pixel is exactly 1 and the other three are exactly 0 (the level sizes are powers of two, so (j + 0.5) / W * W - 0.5 == j in fp32
    whether or not the compiler contracts it into an fma), so the output IS the value tensor.  (Both the inputs and the output row of a group follow
    from the decoded query index, so a wrong tile decode shows as rows that no tile writes, not as rows with another query's result: the
    NaN-filled buffer of test_tiled_map_eligibility[dense_control] catches that deterministically, this test names the rows.)"""
    from hipie_amd import ops
    H, W = hw
    S, M, D = H * W, 8, 32
    g = torch.Generator().manual_seed(31)
    value = torch.randn(B, S, M, D, generator=g)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ref = torch.stack([(xs.flatten().float() + 0.5) / W, (ys.flatten().float() + 0.5) / H], -1)      # fp32 arithmetic as the caller would do it
    assert torch.equal(ref[:, 0] * W - 0.5, xs.flatten().float()) and torch.equal(ref[:, 1] * H - 0.5, ys.flatten().float())
    ref = ref.view(1, S, 1, 2).expand(B, -1, -1, -1).contiguous()
    off, logits = torch.zeros(B, S, M, 1, 1, 2), torch.randn(B, S, M, 1, generator=g)
    shapes = torch.tensor([hw])
    got = ops.msda_fused(value.to(DEV), shapes.to(DEV), dense_lstart(shapes).to(DEV), ref.to(DEV), off.to(DEV), logits.to(DEV)).cpu()
    want = value.view(B, S, M * D)
    if not torch.equal(got, want):
        bad = (got != want).any(-1).flatten().nonzero().flatten()
        q = int(bad[0])
        src = (value.view(B * S, M * D) == got.view(B * S, M * D)[q]).all(-1).nonzero().flatten().tolist()
        pytest.fail("%d of %d queries differ; first wrong query: image %d, pixel %d (row %d, column %d); its output equals value row(s) %s"
                    % (bad.numel(), B * S, q // S, q % S, (q % S) // W, (q % S) % W, src[:4]))


@gpu
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("adt", AUX_FORMS, ids=aux_id)
@pytest.mark.parametrize("vdt", [F32, F16, BF16], ids=lambda d: "val_" + NAME[d])
@pytest.mark.parametrize("layout", ["dense", "column_block"])
def test_decoder_form(layout, vdt, adt, ref_dim):
    """msda_d32_kernel<T, A, FUSED>, map 1 (Lq = 300 != S): MSDeformAttn.forward_projected in the decoders -- value dense or the middle
    column block of a 3x wider projection output sampled in place, every value / aux dtype pair, both reference-point forms."""
    from hipie_amd import ops
    M, D = 8, 32
    value, shapes, lstart, ref, off, logits = make_inputs(PYR_SQUARE, 2, 300, M, D, 4, ref_dim, seed=111)
    if layout == "dense":
        check_fused(value, shapes, lstart, ref, off, logits, vdt, adt)
        return
    B, S = value.shape[:2]
    wide = torch.randn(B, S, 3 * M * D, generator=torch.Generator().manual_seed(112)).to(vdt).to(DEV)
    wide[:, :, M * D:2 * M * D] = value.to(vdt).reshape(B, S, M * D).to(DEV)
    block = wide[:, :, M * D:2 * M * D].unflatten(-1, (M, D))
    assert not block.is_contiguous()
    o, lg = aux_on_device(off, logits, adt)
    got = ops.msda_fused(block, shapes.to(DEV), lstart.to(DEV), ref.to(DEV), o, lg)
    assert rel_err(got.float().cpu(), ref_fused(block, shapes, lstart, ref, o, lg)) < TOL[vdt]


# ------------------------------------------------------------------------------------------------------- eligibility boundaries
PYR_TILE = [(8, 16), (4, 8), (4, 8)]                   # tileable, 128 + 32 + 32 = 192 pixels

BOUNDARY = {
    # name: (pyramid, Lq relative to S, gap, trailing rows)                          branch reached
    "level_does_not_divide": ([(16, 16), (8, 8), (4, 4)], "+0", None, 0),           # map-2 fallback (4 x 4 level)
    "rows_do_not_divide": ([(8, 8), (6, 8)], "+0", None, 0),                        # map-2 fallback (6 rows)
    "lq_is_s_minus_1": (PYR_TILE, "-1", None, 0),                                   # d32 map 1
    "lq_is_s_plus_1": (PYR_TILE, "+1", None, 0),                                    # d32 map 1
    "gaps_of_32": (PYR_TILE, "+0", 32, 0),                                          # map-2 fallback (level_start not dense)
    "gaps_of_5": (PYR_TILE, "+0", 5, 0),                                            # map-2 fallback
    "gaps_of_64_and_7": (PYR_TILE, "+0", [0, 64, 7], 0),                            # map-2 fallback
    "first_level_offset_32": (PYR_TILE, "+0", [32, 0, 0], 0),                       # map-2 fallback (rows in front of level 0)
    "trailing_32_rows": (PYR_TILE, "+0", None, 32),                                 # map-2 fallback (levels do not fill [0, Lq))
    "trailing_7_rows": (PYR_TILE, "+0", None, 7),                                   # map-2 fallback
    "dense_control": (PYR_TILE, "+0", None, 0),                                     # d32 map 2
}


@gpu
@pytest.mark.parametrize("vdt", [F32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_tiled_map_eligibility(name, vdt):
    """Around the conditions of map 2.  The output buffer is filled with NaN before the library call, so a query the kernel does not
    compute (a gap row that belongs to no tile) cannot pass; every query is compared with the reference, and ops.msda_fused must give
    the same bits."""
    from hipie_amd import ops
    pyr, dlq, gap, trailing = BOUNDARY[name]
    B, M, D, P = 2, 8, 32, 4
    value, shapes, lstart, ref, off, logits = make_inputs(pyr, B, dlq, M, D, P, 2, seed=41, gap=gap, trailing=trailing)
    S, Lq = value.shape[1], off.shape[1]
    assert Lq == S + int(dlq)
    dv = [t.to(DEV) for t in (value.to(vdt), shapes, lstart, ref, off, logits)]
    out = torch.full((B, Lq, M * D), float("nan"), dtype=vdt, device=DEV)
    guard = torch.full((64, M * D), 7.0, dtype=vdt, device=DEV)                     # allocated right behind: stays untouched
    assert fused_into(out, *dv) == 0
    torch.cuda.synchronize()
    unwritten = torch.isnan(out.float()).any(-1).flatten().nonzero().flatten().cpu()
    assert unwritten.numel() == 0, "%d queries never written, first %s" % (unwritten.numel(), unwritten[:8].tolist())
    err = rel_err(out.float().cpu(), ref_fused(*dv))
    print("%s %s: rel_err %.3e" % (name, NAME[vdt], err))
    assert err < TOL[vdt], err
    assert torch.equal(ops.msda_fused(*dv), out)
    assert bool((guard == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- ragged groups
RAGGED_PYR = [(6, 5), (4, 3), (2, 2), (1, 3)]
RAGGED_BQ = [(1, 1), (1, 7), (1, 31), (3, 11), (1, 257)]          # B * Lq = 1, 7, 31, 33, 257


@gpu
@pytest.mark.parametrize("LP", [(1, 1), (1, 4), (3, 4), (4, 4), (3, 8), (4, 8)], ids=lambda lp: "L%dP%d" % lp)
@pytest.mark.parametrize("M", [1, 5, 8, 16])
def test_ragged_groups(M, LP):
    """Group and softmax shapes away from L*P = 16, M = 8.  D = 32: msda_d32_kernel map 1 (publish_records strides the L*P points over 8
    lanes: with L*P = 1, 4, 12 some lanes hold no point; M sets how the workgroups divide the queries; B * Lq below, at and above the 32
    queries of a workgroup).  D = 16, 64: msda_generic_kernel.  Fused (both ref_dim; aux fp32 dense, f16 / bf16 / fp32 strided in turn)
    and unfused."""
    from hipie_amd import ops
    L, P = LP
    pyr = RAGGED_PYR[:L]
    k = 0
    for (B, Lq), D in itertools.product(RAGGED_BQ, (32, 16, 64)):
        ref_dim, adt = (2, 4)[k % 2], (F32, F16, BF16, F32S)[k % 3 if k % 5 else 3]
        k += 1
        value, shapes, lstart, ref, off, logits = make_inputs(pyr, B, Lq, M, D, P, ref_dim, seed=200 + k)
        check_fused(value, shapes, lstart, ref, off, logits, F32, adt)
        loc = fused_locations(shapes, ref, off, F32)
        attn = torch.softmax(logits, -1).view(B, Lq, M, L, P)
        got = ops.ms_deform_attn_forward(value.to(DEV), shapes.to(DEV), lstart.to(DEV), loc.to(DEV), attn.to(DEV))
        assert rel_err(got.cpu(), ref_unfused(value, shapes, lstart, loc, attn)) < TOL[F32]


@gpu
@pytest.mark.parametrize("D", [32, 16])
def test_fused_refuses_more_than_32_points(D):
    """L*P = 32 is the stated maximum of the fused softmax (covered above); 33 raises the library's error and writes nothing."""
    from hipie_amd import ops, _lib
    value, shapes, lstart, ref, off, logits = make_inputs(RAGGED_PYR[:3], 1, 9, 2, D, 11, 2, seed=51)
    dv = [t.to(DEV) for t in (value, shapes, lstart, ref, off, logits)]
    with pytest.raises(RuntimeError, match=r"L\*P=33 > 32"):
        ops.msda_fused(*dv)
    out = torch.full((1, 9, 2 * D), -3.0, device=DEV)
    assert fused_into(out, *dv) == -22 and b"L*P=33" in _lib.load().hipie_last_error()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


# ------------------------------------------------------------------------------------------------------------------ exact edges
EDGE_PATHS = {"d32_f32": (32, F32), "d32_f16": (32, F16), "d32_bf16": (32, BF16), "generic_f32": (12, F32), "generic_bf16": (12, BF16),
              "f64_d32": (32, F64), "f64_d6": (6, F64)}


@gpu
@pytest.mark.parametrize("path", sorted(EDGE_PATHS))
def test_exact_edges_unfused(path):
    """Every pair of {-1, -1 + 2^-10, -0.5, 0, 0.5, H-1, H-0.5, H - 2^-10, H, +/-1e6} as pixel coordinates on 1 x 1, 1 x 8, 8 x 1 and 4 x 8
    levels, exact in fp32, through ops.ms_deform_attn_forward: point_record's branch-free clamp-and-zero form (msda_d32_kernel, map 1,
    unfused), the nested ifs of msda_generic_kernel, and msda_f64_kernel, each against the oracle AND the per-sample loops."""
    from hipie_amd import ops
    D, dt = EDGE_PATHS[path]
    for P in (1, 2):
        value, shapes, lstart, loc, attn = edge_case(D, P=P)
        adt = F64 if dt == F64 else F32
        v = value.to(dt).to(DEV)
        got = ops.ms_deform_attn_forward(v, shapes.to(DEV), lstart.to(DEV), loc.to(adt).to(DEV), attn.to(adt).to(DEV))
        assert got.dtype == dt
        attn_read = attn.to(adt)
        for want in (ref_unfused(v, shapes, lstart, loc, attn_read), ref_loops(v, shapes, lstart, loc, attn_read)):
            err = rel_err(got.cpu().double(), want)
            print("edges %s P=%d: rel_err %.3e" % (path, P, err))
            assert err < TOL[dt], err
        # a sample on or outside -1 / H contributes exactly nothing: queries with every point outside are exactly zero
        outside = (ref_loops(torch.ones_like(value), shapes, lstart, loc, torch.ones_like(attn)) == 0).all(-1).flatten()
        assert outside.sum() > 0 and float(got.view(-1, got.shape[-1])[outside.to(DEV)].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("D", [32, 12])
def test_exact_edges_fused(D, ref_dim):
    """the same pixel coordinates through ops.msda_fused with dyadic ref and off (msda_d32_kernel map 1 / msda_generic_kernel, FUSED,
    ref_dim 2 with P = 1 and ref_dim 4 with P = 2): fp32 value and 16-bit values, against the oracle and the loops"""
    value, shapes, lstart, ref, off, logits = edge_case_fused(D, ref_dim)
    B, Lq, M, L, P, _ = off.shape
    for vdt in (F32, F16, BF16):
        got = check_fused(value, shapes, lstart, ref, off, logits, vdt, F32)
        attn = torch.softmax(logits.double(), -1).view(B, Lq, M, L, P)
        want = ref_loops(value.to(vdt), shapes, lstart, fused_locations(shapes, ref, off), attn)
        assert rel_err(got.float().cpu(), want) < TOL[vdt]


# ---------------------------------------------------------------------------------------------------------------------- softmax
def _softmax_logits(kind, shape, g):
    n = shape[-1]
    base = torch.randn(shape, generator=g)
    if kind == "all_equal":
        return torch.zeros(shape)
    if kind == "all_equal_at_200":                     # exp(200) overflows fp32: only the max subtraction keeps this finite
        return torch.full(shape, 200.0)
    if kind == "one_dominant":
        base[..., 3 % n] += 80.0
        return base
    if kind == "spread_80":
        return (torch.rand(shape, generator=g) * 2 - 1) * 80.0
    if kind == "spread_80_shifted":                    # the same spread around +120
        return (torch.rand(shape, generator=g) * 2 - 1) * 80.0 + 120.0
    if kind == "minus_1e4":
        base[..., ::2] = -1e4
        return base
    if kind == "f16_near_6e4":
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        return sign * (6e4 + torch.rand(shape, generator=g) * 64)          # fp16 spacing there is 32: ties and near ties at the top
    raise KeyError(kind)


@gpu
@pytest.mark.parametrize("D", [32, 16])
@pytest.mark.parametrize("kind", ["all_equal", "all_equal_at_200", "one_dominant", "spread_80", "spread_80_shifted", "minus_1e4", "f16_near_6e4"])
def test_softmax_extremes(kind, D):
    """the in-kernel softmax (publish_records / msda_generic_kernel, FUSED) on logits a naive exp would overflow or flush"""
    value, shapes, lstart, ref, off, _ = make_inputs([(8, 8), (4, 4), (2, 2)], 2, 45, 8, D, 4, 2, seed=61)
    logits = _softmax_logits(kind, (2, 45, 8, 12), torch.Generator().manual_seed(62))
    adt = F16 if kind.startswith("f16") else F32
    got = check_fused(value, shapes, lstart, ref, off * 0.25, logits, F32, adt)
    assert torch.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------- strided value
@gpu
@pytest.mark.parametrize("form", ["map2", "map1", "generic"])
@pytest.mark.parametrize("vdt", [F16, BF16], ids=lambda d: NAME[d])
def test_strided_value_16bit(vdt, form):
    """16-bit value as the middle column block of a 3x wider projection output (the decoder's one value GEMM for all layers), sampled in
    place through its row stride: the same bits as the dense call, and both within the dtype's bound of the reference.  Aux 16-bit
    strided as the model passes it; ref_dim 4 on the decoder forms."""
    from hipie_amd import ops
    M, D = (8, 32) if form != "generic" else (4, 16)
    ref_dim = 2 if form == "map2" else 4
    value, shapes, lstart, ref, off, logits = make_inputs(PYR_TILE, 2, "+0" if form == "map2" else 77, M, D, 4, ref_dim, seed=71)
    dense = check_fused(value, shapes, lstart, ref, off, logits, vdt, vdt)
    B, S = value.shape[:2]
    wide = torch.randn(B, S, 3 * M * D, generator=torch.Generator().manual_seed(72)).to(vdt).to(DEV)
    wide[:, :, M * D:2 * M * D] = value.to(vdt).reshape(B, S, M * D).to(DEV)
    block = wide[:, :, M * D:2 * M * D].unflatten(-1, (M, D))
    assert not block.is_contiguous()
    o, lg = aux_on_device(off, logits, vdt)
    got = ops.msda_fused(block, shapes.to(DEV), lstart.to(DEV), ref.to(DEV), o, lg)
    assert torch.equal(got, dense)
    assert rel_err(got.float().cpu(), ref_fused(block, shapes, lstart, ref, o, lg)) < TOL[vdt]


# ----------------------------------------------------------------------------------------------------------- large batch offset
def large_batch_inputs():
    """the last image's inputs of test_large_batch_offset (CPU, seeded): 256/128/64/32 levels, decoder-sized Lq, ref_dim 4"""
    g = torch.Generator().manual_seed(81)
    shapes = torch.tensor([(256, 256), (128, 128), (64, 64), (32, 32)])
    S, M, D, Lq = int(shapes.prod(1).sum()), 8, 32, 300
    value = torch.randn(1, S, M, D, generator=g).bfloat16()
    ref = torch.cat([torch.rand(1, Lq, 4, 2, generator=g), torch.rand(1, Lq, 4, 2, generator=g) * 0.5 + 0.1], -1)
    proj = (torch.randn(1, Lq, 384, generator=g)).bfloat16()
    return value, shapes, dense_lstart(shapes), ref, proj


@gpu
def test_large_batch_offset():
    """B * S * M * D > 2^31 elements (bf16, B = 100 images of S = 87040 pixels, 4.46 GB): the kernel keeps 32-bit sample offsets inside an
    image and a 64-bit image base.  msda_d32_kernel<bf16, bf16, FUSED> map 1, ref_dim 4.  The last image's output equals a B = 1 call on
    that image's slice bit for bit, and agrees with the reference.

    Bounds.  The levels exceed 64 pixels, so the fp32 bound is derived: the oracle in float32 against ref_fused on the last image's inputs
    measures 1.005e-5 (LARGE_GEOMETRY_F32_ORACLE_ERR["batch_256"]) -> max(2e-5, 4 x 1.005e-5) = 4.02e-5.  That is far below the bf16 bound
    of 8e-3 (reference fed the same rounded inputs), which therefore stands for the bf16 batch; the last image is also run alone with
    the same numbers as an fp32 value and fp32 aux (msda_d32_kernel<float, float, FUSED> map 1) against the 4.02e-5."""
    from hipie_amd import ops
    value1, shapes, lstart, ref1, proj1 = large_batch_inputs()
    B, (_, S, M, D), Lq = 100, value1.shape, ref1.shape[1]
    assert B * S * M * D > 2 ** 31 and S * M * D < 2 ** 31
    need = B * S * M * D * 2 + (1 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB available" % (need / 2 ** 30, free / 2 ** 30))
    value = torch.empty(B, S, M, D, dtype=BF16, device=DEV)
    value.normal_()                                                # the other images: generated on the device
    value[B - 1] = value1[0].to(DEV)
    gg = torch.Generator().manual_seed(82)
    ref = torch.rand(B, Lq, 4, 4, generator=gg).to(DEV)
    proj = torch.randn(B, Lq, 384, generator=gg).bfloat16().to(DEV)
    ref[B - 1], proj[B - 1] = ref1[0].to(DEV), proj1[0].to(DEV)
    off, lg = proj[..., :256].unflatten(-1, (M, 4, 4, 2)), proj[..., 256:].unflatten(-1, (M, 16))
    ss, ls = shapes.to(DEV), lstart.to(DEV)
    full = ops.msda_fused(value, ss, ls, ref, off, lg)
    last = ops.msda_fused(value[B - 1:], ss, ls, ref[B - 1:].contiguous(), off[B - 1:], lg[B - 1:])
    assert torch.equal(full[B - 1:], last)
    first = ops.msda_fused(value[:1], ss, ls, ref[:1].contiguous(), off[:1], lg[:1])
    assert torch.equal(full[:1], first)
    want = ref_fused(value[B - 1:], shapes, lstart, ref[B - 1:], off[B - 1:], lg[B - 1:])
    err = rel_err(full[B - 1:].float().cpu(), want)
    print("large batch, last image: rel_err %.3e" % err)
    assert err < max(TOL[BF16], large_geometry_f32_bound("batch_256")), err
    last32 = ops.msda_fused(value[B - 1:].float(), ss, ls, ref[B - 1:].contiguous(), off[B - 1:].float().contiguous(), lg[B - 1:].float().contiguous())
    err = rel_err(last32.cpu(), want)
    print("large batch geometry, last image in fp32: rel_err %.3e" % err)
    assert err < large_geometry_f32_bound("batch_256"), err
    del value, full
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ benchmark geometry (used by test_gpu_kernels.py)
def full_scale_inputs():
    """inputs of test_gpu_kernels.test_msda_fused_full_scale_strided_aux (CPU, seeded): 128/64/32/16 levels, B = 2, queries = pixels,
    bf16 value, one bf16 projection tensor holding offsets and logits, ref_dim 2"""
    gen = torch.Generator().manual_seed(3)
    B, M, D, L, P = 2, 8, 32, 4, 4
    shapes = torch.tensor([(128, 128), (64, 64), (32, 32), (16, 16)])
    S = int(shapes.prod(1).sum())
    value = torch.randn(B, S, M, D, generator=gen).bfloat16()
    proj = (torch.randn(B, S, 384, generator=gen) * 0.5).bfloat16()
    ref = torch.rand(B, S, L, 2, generator=gen)
    return value, shapes, dense_lstart(shapes), ref, proj


def bench_geometry_queries(shapes, n_random=4000, seed=91):
    """first and last 8 x 4 tile of every level plus n_random random queries of a pyramid whose queries are its pixels"""
    lstart = dense_lstart(shapes)
    idx = []
    for l in range(shapes.shape[0]):
        H, W, base = int(shapes[l, 0]), int(shapes[l, 1]), int(lstart[l])
        for y0, x0 in ((0, 0), (H - 4, W - 8)):
            idx += [base + (y0 + dy) * W + x0 + dx for dy in range(4) for dx in range(8)]
    S = int(shapes.prod(1).sum())
    rnd = torch.randperm(S, generator=torch.Generator().manual_seed(seed))[:n_random]
    return torch.unique(torch.cat([torch.tensor(idx), rnd]))


def f32_oracle_error(name):
    """oracle run in float32 (locations, softmax and sampling) against ref_fused on the inputs of a large geometry; CPU only"""
    if name == "bench_128":
        value, shapes, lstart, ref, proj = full_scale_inputs()
        q = bench_geometry_queries(shapes)
    else:
        value, shapes, lstart, ref, proj = large_batch_inputs()
        q = None
    off, lg = proj[..., :256].unflatten(-1, (8, 4, 4, 2)), proj[..., 256:].unflatten(-1, (8, 16))
    args = (value, shapes, lstart, ref, off, lg)
    return rel_err(ref_fused(*args, queries=q, dtype=F32), ref_fused(*args, queries=q))


@pytest.mark.parametrize("name", sorted(LARGE_GEOMETRY_F32_ORACLE_ERR))
def test_recorded_f32_oracle_errors(name):
    """the figures the large-geometry bounds are derived from are what the oracle measures (CPU; exp and summation order may differ a
    little between hosts, hence a window and not equality)"""
    err = f32_oracle_error(name)
    print("%s: oracle in float32 against float64: %.3e" % (name, err))
    assert 0.5 * LARGE_GEOMETRY_F32_ORACLE_ERR[name] <= err <= 1.5 * LARGE_GEOMETRY_F32_ORACLE_ERR[name]
