"""GPU: every hand-written HIP kernel, called through the C ABI, against the oracle on the same seeded inputs and
against the reference-generated golden fixtures.  Tolerances are written next to each check:
  fp32 kernels (MSDA f32, dynamic mask, einsum precision 0/1): <= 2e-5 relative to the output scale;
  16-bit MFMA kernels: vs the oracle fed the SAME 16-bit-rounded inputs 1e-3 (fp16) / 8e-3 (bf16) -- the residual is the
  rounding of P and of the output to 16 bit; vs the fp32 golden 2e-3 (fp16) / 2e-2 (bf16).
Per-branch float64 conformance files exist for csrc/msda.hip (tests/test_gpu_msda_forward.py) and for the 16-bit flash attention family,
csrc/flash_attn.hip and csrc/bi_xattn.hip (tests/test_gpu_flash_attn.py: ops.flash_attn, vit_attn, vit_attn_fused, bi_xattn), for
vit_attn.hip (vit_attn_rel) and vit_attn_split.hip (tests/test_gpu_vit_attn.py) and for attn_f32.hip and attn_split.hip
(tests/test_gpu_small_attn.py).  The training attention kernels have no such file yet; the attention tests below are all they have."""
import pytest
import torch

import _synth
from oracle import ops as oo
from util import Golden, rel_err
from test_oracle_golden import msda_case, vit_attn_case, bi_case, dyn_case

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


def test_selftest_mfma_layout():
    from hipie_amd import ops
    g = torch.Generator().manual_seed(1)
    A = torch.randn(32, 16, generator=g).bfloat16()
    B = torch.randn(16, 32, generator=g).bfloat16()
    D = ops.selftest(0, A.to(DEV).view(torch.int16), B.to(DEV).view(torch.int16)).cpu().view(32, 32)
    ref = A.float() @ B.float()      # asymmetric operands: a transposed C/D map cannot pass
    assert rel_err(D, ref) < 1e-5


def test_selftest_tr_read():
    from hipie_amd import ops
    tile = torch.arange(256, dtype=torch.float32).view(8, 32)
    out = ops.selftest(1, tile.bfloat16().to(DEV).view(torch.int16)).cpu().view(64, 4)
    for lane in range(64):
        l16, g1, hi = lane & 15, (lane >> 4) & 1, lane >> 5
        for j in range(4):
            assert out[lane, j] == tile[4 * hi + j, 16 * g1 + l16], (lane, j)


def _lsi(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def test_msda_reference_recipe_float():
    """the reference's own check (ops/test.py:52-66): fp32 op vs pytorch core, rtol 1e-2 atol 1e-3 there; here 1e-6."""
    from hipie_amd import ops
    g = Golden("msda")
    shapes = g["ref_float_shapes"]
    out = ops.ms_deform_attn_forward(g["ref_float_value"].to(DEV), shapes.to(DEV), _lsi(shapes).to(DEV),
                                     g["ref_float_loc"].to(DEV), g["ref_float_attn"].to(DEV), 2).cpu()
    assert torch.allclose(out, g["ref_float_out"], rtol=1e-2, atol=1e-3)
    assert rel_err(out, g["ref_float_out"]) < 1e-6


def test_msda_reference_recipe_double():
    """the double instantiation of the op (ops/test.py:36-49 check_forward_equal_with_pytorch_double): f64 in, f64 out, 1e-12."""
    from hipie_amd import ops
    g = Golden("msda")
    shapes = g["ref_double_shapes"]
    f64 = torch.float64                                        # the fixture stores the inputs as they were generated; the op runs in double
    out = ops.ms_deform_attn_forward(g["ref_double_value"].to(f64).to(DEV), shapes.to(DEV), _lsi(shapes).to(DEV),
                                     g["ref_double_loc"].to(f64).to(DEV), g["ref_double_attn"].to(f64).to(DEV), 2).cpu()
    assert out.dtype == torch.float64
    assert rel_err(out, g["ref_double_out"]) < 1e-12


@pytest.mark.parametrize("tag", ["hot_enc", "hot_dec", "hot_rect"])
def test_msda_hot_geometry(tag):
    from hipie_amd import ops
    g = Golden("msda")
    value, shapes, loc, attn = msda_case(g, tag)
    out = ops.ms_deform_attn_forward(value.to(DEV), shapes.to(DEV), _lsi(shapes).to(DEV), loc.to(DEV), attn.to(DEV)).cpu()
    assert rel_err(g.like(tag + "_out", out), g[tag + "_out"]) < 2e-5          # vs reference golden
    assert rel_err(out, oo.ms_deform_attn_core(value, shapes, loc, attn)) < 2e-5   # vs oracle, full tensor
    for dt, tol in ((torch.float16, 1e-3), (torch.bfloat16, 8e-3)):
        o16 = ops.ms_deform_attn_forward(value.to(DEV).to(dt), shapes.to(DEV), _lsi(shapes).to(DEV), loc.to(DEV), attn.to(DEV))
        ref16 = oo.ms_deform_attn_core(value.to(dt).float(), shapes, loc, attn)
        assert rel_err(o16.float().cpu(), ref16) < tol


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_msda_fused(ref_dim):
    """fused sampling-location + softmax variant == MSDeformAttn.forward lines 99-114 followed by the op."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(5)
    B, Lq, M, D, L, P = 2, 77, 8, 32, 4, 4
    shapes = torch.tensor([(12, 20), (6, 10), (3, 5), (2, 3)])
    S = int(shapes.prod(1).sum())
    value = torch.randn(B, S, M, D, generator=gen)
    off = torch.randn(B, Lq, M, L, P, 2, generator=gen) * 2
    logit = torch.randn(B, Lq, M, L * P, generator=gen)
    ref = torch.rand(B, Lq, L, ref_dim, generator=gen)
    aw = torch.softmax(logit, -1).view(B, Lq, M, L, P)
    if ref_dim == 2:
        norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).float()
        loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    else:
        loc = ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5
    want = oo.ms_deform_attn_core(value, shapes, loc, aw)
    got = ops.msda_fused(value.to(DEV), shapes.to(DEV), _lsi(shapes).to(DEV), ref.to(DEV), off.to(DEV), logit.to(DEV)).cpu()
    assert rel_err(got, want) < 2e-5
    # the value tensor as the middle column block of a 3x wider projection output (one GEMM for all decoder layers): same bits
    wide = torch.randn(B, S, 3 * M * D, generator=gen).to(DEV)
    wide[:, :, M * D:2 * M * D] = value.reshape(B, S, M * D).to(DEV)
    block = wide[:, :, M * D:2 * M * D].unflatten(-1, (M, D))
    assert not block.is_contiguous()
    got2 = ops.msda_fused(block, shapes.to(DEV), _lsi(shapes).to(DEV), ref.to(DEV), off.to(DEV), logit.to(DEV)).cpu()
    assert torch.equal(got2, got)


def test_msda_generic_head_dim():
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(6)
    shapes = torch.tensor([(6, 4), (3, 2)])
    S = int(shapes.prod(1).sum())
    for D in (2, 30, 71):
        value = torch.rand(1, S, 2, D, generator=gen)
        loc = torch.rand(1, 5, 2, 2, 2, 2, generator=gen)
        attn = torch.rand(1, 5, 2, 2, 2, generator=gen)
        got = ops.ms_deform_attn_forward(value.to(DEV), shapes.to(DEV), _lsi(shapes).to(DEV), loc.to(DEV), attn.to(DEV)).cpu()
        assert rel_err(got, oo.ms_deform_attn_core(value, shapes, loc, attn)) < 2e-6


@pytest.mark.parametrize("prec,tol", [(0, 2e-6), (1, 3e-5), (2, 1e-2)])
@pytest.mark.parametrize("shape", [(2, 300, 256, 64, 64), (1, 37, 64, 24, 40), (1, 330, 32, 8, 8), (1, 5, 16, 3, 50), (2, 300, 80, 20, 13)])
def test_mask_einsum(prec, tol, shape):
    from hipie_amd import ops
    B, Q, C, H, W = shape
    gen = torch.Generator().manual_seed(7)
    e = torch.randn(B, Q, C, generator=gen)
    f = torch.randn(B, C, H, W, generator=gen)
    want = oo.mask_einsum(e, f)
    got = ops.mask_einsum(e.to(DEV), f.to(DEV), precision=prec).cpu()
    assert rel_err(got, want) < tol
    if prec == 1:
        got16 = ops.mask_einsum(e.to(DEV), f.to(DEV), precision=1, out_dtype=torch.bfloat16).float().cpu()
        assert rel_err(got16, want) < 8e-3
    if prec in (1, 2):          # the workspace-free entry point; then a constant per query row (the folded 1x1 convolution's emb . b)
        plain = ops.mask_einsum(e.to(DEV), f.to(DEV), precision=prec, workspace=False).cpu()
        assert rel_err(plain, want) < tol
        rb = torch.randn(B, Q, generator=gen) * 3
        gotb = ops.mask_einsum(e.to(DEV), f.to(DEV), precision=prec, row_bias=rb.to(DEV)).cpu()
        assert rel_err(gotb, want + rb[:, :, None, None]) < tol
    else:
        with pytest.raises(RuntimeError):
            ops.mask_einsum(e.to(DEV), f.to(DEV), precision=0, row_bias=torch.zeros(B, Q, device=DEV))


@pytest.mark.parametrize("dt,split,tol", [(torch.float16, True, 6e-4), (torch.float16, False, 1e-3), (torch.bfloat16, True, 4e-3)])
@pytest.mark.parametrize("shape", [(2, 300, 256, 64, 64), (1, 37, 64, 24, 40), (1, 320, 32, 8, 8), (1, 5, 16, 2, 4)])
def test_mask_einsum16(dt, split, tol, shape):
    """hipie_mask_einsum16 (16-bit features, transposed product, 16-byte stores) vs the fp32 einsum of the SAME 16-bit-rounded
    features: the residual is the rounding of the embedding (hi + lo: ~2^-22, hi only: 2^-12) and of the 16-bit output."""
    from hipie_amd import ops
    B, Q, C, H, W = shape
    gen = torch.Generator().manual_seed(Q + C)
    emb = torch.randn(B, Q, C, generator=gen)
    feat = torch.randn(B, C, H, W, generator=gen).to(dt)
    want = torch.einsum("bqc,bchw->bqhw", emb, feat.float())
    got = ops.mask_einsum16(emb.to(DEV), feat.to(DEV), split=split)
    assert got.dtype == dt and got.shape == want.shape
    assert rel_err(got.float().cpu(), want) < tol
    got32 = ops.mask_einsum16(emb.to(DEV), feat.to(DEV), split=split, out_dtype=torch.float32)
    assert rel_err(got32.cpu(), want) < (3e-6 if split and dt == torch.float16 else 1e-4 if split else tol)
    rb = torch.randn(B, Q, generator=gen)                             # the folded bias of the mask_features head's last conv
    gotb = ops.mask_einsum16(emb.to(DEV), feat.to(DEV), split=split, out_dtype=torch.float32, row_bias=rb.to(DEV))
    assert rel_err(gotb.cpu(), want + rb[:, :, None, None]) < (3e-6 if split and dt == torch.float16 else 1e-4 if split else tol)


@pytest.mark.parametrize("name", ["sq", "rect"])
def test_dynamic_mask(name):
    from hipie_amd import ops
    g = Golden("dynamic_mask")
    c, feats, refs, params = dyn_case(g, name)
    got = ops.dynamic_mask(feats.to(DEV), refs[0].contiguous().to(DEV), params[0].contiguous().to(DEV), c["Q"], stride=8, up=2).cpu()
    got = got.view(1, c["B"] * c["Q"], 2 * c["H"], 2 * c["W"])
    assert rel_err(g.like(name + "_out", got), g[name + "_out"]) < 2e-5
    want = oo.dynamic_mask(feats, refs, params, [c["Q"]] * c["B"], stride=8, up=2)
    assert rel_err(got, want) < 2e-5


def _dynamic_mask16_emulation(feats, refs, params, Q, stride, dt):
    """the oracle's formulation with hipie_dynamic_mask16's roundings: features, layer weights and hidden activations in `dt`,
    coordinate weights hi + lo, fp32 (here fp64) accumulation and bias / reference-point terms."""
    B, C, H, W = feats.shape
    rd = lambda t: t.to(dt).double()
    p = params.reshape(-1, 169).double()
    n_all = p.shape[0]
    w0, w1, w2 = p[:, :80].reshape(n_all, 8, 10), p[:, 80:144].reshape(n_all, 8, 8), p[:, 144:152].reshape(n_all, 1, 8)
    b0, b1, b2 = p[:, 152:160], p[:, 160:168], p[:, 168:169]
    xs = (torch.arange(0, W * stride, stride) + stride // 2).double()
    ys = (torch.arange(0, H * stride, stride) + stride // 2).double()
    r = refs.reshape(-1, 2).double()
    wxy = rd(w0[:, :, :2].float()) + rd((w0[:, :, :2].float() - w0[:, :, :2].float().to(dt).float()))      # hi + lo
    f = rd(feats).reshape(B, C, H * W)[torch.arange(n_all) // Q]
    pix = torch.stack([xs.view(1, W).expand(H, W).reshape(-1), ys.view(H, 1).expand(H, W).reshape(-1)])     # (2, HW)
    c1 = b0 + w0[:, :, 0] * r[:, :1] + w0[:, :, 1] * r[:, 1:]
    h1 = torch.relu(c1[:, :, None] - wxy @ pix[None] + rd(w0[:, :, 2:].float()) @ f)
    h2 = torch.relu(rd(w1.float()) @ rd(h1.float()) + b1[:, :, None])
    y = rd(w2.float()) @ rd(h2.float()) + b2[:, :, None]
    return oo.aligned_bilinear(y.reshape(n_all, 1, H, W).float(), 2).reshape(n_all, 2 * H, 2 * W)


@pytest.mark.parametrize("dt,tol", [(torch.float16, 3e-3), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("name", ["sq", "rect"])
def test_dynamic_mask16_golden(name, dt, tol):
    """the matrix-pipe variant against the reference's fp32 output (golden) within the 16-bit operand tolerance."""
    from hipie_amd import ops
    g = Golden("dynamic_mask")
    c, feats, refs, params = dyn_case(g, name)
    if c["W"] % 4:
        pytest.skip("hipie_dynamic_mask16 needs W % 4 == 0")
    got = ops.dynamic_mask(feats.to(DEV), refs[0].contiguous().to(DEV), params[0].contiguous().to(DEV), c["Q"], stride=8, up=2,
                           mlp_dtype=dt).cpu()
    got = got.view(1, c["B"] * c["Q"], 2 * c["H"], 2 * c["W"])
    assert rel_err(g.like(name + "_out", got), g[name + "_out"]) < tol


@pytest.mark.parametrize("name", ["sq", "rect"])
def test_dynamic_mask_split_golden(name):
    """the split form of the matrix-pipe kernel (weights and activations as fp16 pairs, three products per layer: what the split policy
    runs) against the reference's fp32 output and the oracle at the fp32 kernel's own tolerance class."""
    from hipie_amd import ops
    g = Golden("dynamic_mask")
    c, feats, refs, params = dyn_case(g, name)
    if c["W"] % 4:
        pytest.skip("hipie_dynamic_mask16 needs W % 4 == 0")
    got = ops.dynamic_mask(feats.to(DEV), refs[0].contiguous().to(DEV), params[0].contiguous().to(DEV), c["Q"], stride=8, up=2,
                           mlp_dtype="split").cpu()
    got = got.view(1, c["B"] * c["Q"], 2 * c["H"], 2 * c["W"])
    e = rel_err(g.like(name + "_out", got), g[name + "_out"])
    print("dynamic_mask split %s: %.2e" % (name, e))
    assert e < 2e-5


@pytest.mark.parametrize("B,Q,H,W", [(2, 9, 16, 32), (1, 6, 37, 168), (3, 5, 20, 44), (1, 910, 8, 128)])
def test_dynamic_mask_split_ragged_vs_fp32_kernel(B, Q, H, W):
    """ragged shapes (Q % 4 != 0, W % 32 != 0, H % 16 != 0): the split matrix-pipe form against the fp32 VALU kernel and the oracle"""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + Q + 7)
    feats = torch.randn(B, 8, H, W, generator=gen)
    refs = torch.rand(B * Q, 2, generator=gen) * torch.tensor([8.0 * W, 8.0 * H])
    params = torch.randn(B * Q, 169, generator=gen) * 0.3
    params[:, 0:80:10] *= 0.01
    params[:, 1:80:10] *= 0.01
    got = ops.dynamic_mask(feats.to(DEV), refs.to(DEV), params.to(DEV), Q, stride=8, up=2, mlp_dtype="split").cpu()
    ref = ops.dynamic_mask(feats.to(DEV), refs.to(DEV), params.to(DEV), Q, stride=8, up=2).cpu()
    full = oo.dynamic_mask(feats, refs[None], params[None], [Q] * B, stride=8, up=2)[0]
    e1, e2 = rel_err(got, ref), rel_err(got, full)
    print("dynamic_mask split %dx%dx%dx%d: vs fp32 kernel %.2e, vs oracle %.2e" % (B, Q, H, W, e1, e2))
    assert e1 < 2e-5 and e2 < 2e-5          # the tolerance class of the fp32 kernels of this library


@pytest.mark.parametrize("B,Q,H,W,dt,odt", [(2, 9, 16, 32, torch.float16, torch.float32), (1, 6, 37, 168, torch.float16, torch.float16),
                                            (3, 5, 20, 44, torch.bfloat16, torch.float32), (1, 910, 8, 128, torch.float16, torch.float32)])
def test_dynamic_mask16_matches_rounded_formulation(B, Q, H, W, dt, odt):
    """ragged shapes (Q % 4 != 0, W % 32 != 0, H % 16 != 0) against the same arithmetic written with torch (same operand
    roundings, wide accumulation): pins every lane / k-slot map of the three chained MFMA layers."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + Q)
    feats = torch.randn(B, 8, H, W, generator=gen)
    refs = torch.rand(B * Q, 2, generator=gen) * torch.tensor([8.0 * W, 8.0 * H])
    params = torch.randn(B * Q, 169, generator=gen) * 0.3
    params[:, 0:80:10] *= 0.01                                   # coordinate weights: the inputs are ~1000 pixels
    params[:, 1:80:10] *= 0.01
    got = ops.dynamic_mask(feats.to(DEV), refs.to(DEV), params.to(DEV), Q, stride=8, up=2, out_dtype=odt, mlp_dtype=dt).float().cpu()
    want = _dynamic_mask16_emulation(feats, refs, params, Q, 8, dt)
    # a hidden activation that lands on a rounding boundary may round the other way (fp32 vs wide accumulation): 1 ulp of dt
    tol = (2e-3 if dt == torch.float16 else 1.5e-2) if odt == torch.float32 else 3e-3
    assert rel_err(got, want) < tol
    full = oo.dynamic_mask(feats, refs[None], params[None], [Q] * B, stride=8, up=2)[0]
    assert rel_err(got, full) < (6e-3 if dt == torch.float16 else 4e-2)


def _vit_qkv(c, sd, x):
    import torch.nn.functional as F
    B, H, W, C = x.shape
    qkv = F.linear(x, sd["qkv.weight"], sd["qkv.bias"]).reshape(B, H * W, 3 * C)
    return qkv


@pytest.mark.parametrize("dt,tol_same,tol_gold", [(torch.float16, 1e-3, 2e-3), (torch.bfloat16, 8e-3, 2e-2)])
@pytest.mark.parametrize("name", ["window14", "global16", "global64", "global_rect"])
def test_vit_attention(name, dt, tol_same, tol_gold):
    """hipie_vit_attn (windowed 14x14, global with interpolated table, the real 64x64 grid, a non-square grid)."""
    import torch.nn.functional as F
    from hipie_amd import ops
    g = Golden("vit_attn")
    c, sd, x = vit_attn_case(g, name)
    B, H, W, C = x.shape
    heads = c["heads"]
    hd = C // heads
    qkv = _vit_qkv(c, sd, x).to(dt)                                   # the 16-bit operands the kernel sees
    q, k, v = qkv.float().reshape(B, H * W, 3, heads, hd).permute(2, 0, 3, 1, 4).reshape(3, B * heads, H * W, hd).unbind(0)
    Rh = oo.get_rel_pos(H, H, sd["rel_pos_h"])
    Rw = oo.get_rel_pos(W, W, sd["rel_pos_w"])
    rq = q.reshape(B * heads, H, W, hd)
    rel_h = torch.einsum("bhwc,hkc->bkhw", rq, Rh).reshape(B * heads, H, H * W).contiguous()       # key-row major
    rel_w = torch.einsum("bhwc,wkc->bhwk", rq, Rw).reshape(B * heads, H * W, W).contiguous()
    got = ops.vit_attn(qkv.to(DEV), rel_h.to(DEV), rel_w.to(DEV), (H, W), heads, hd ** -0.5).float().cpu()
    want = oo.vit_attention_core(q, k, v, sd["rel_pos_h"], sd["rel_pos_w"], (H, W), hd ** -0.5)
    want = want.view(B, heads, H * W, hd).permute(0, 2, 1, 3).reshape(B, H * W, C)
    assert rel_err(got, want) < tol_same
    out = F.linear(got, sd["proj.weight"], sd["proj.bias"]).view(B, H, W, C)
    assert rel_err(g.like(name + "_out", out), g[name + "_out"]) < tol_gold


@pytest.mark.parametrize("dt,tol_same,tol_gold", [(torch.float16, 1e-3, 2e-3), (torch.bfloat16, 8e-3, 2e-2)])
def test_vit_attention_fused_relpos(dt, tol_same, tol_gold):
    """hipie_vit_attn_fused (rel-pos bias computed in the kernel from the tables) on the real 64x64 grid: against the oracle
    on the same 16-bit operands and tables, and against the reference golden."""
    import torch.nn.functional as F
    from hipie_amd import ops
    g = Golden("vit_attn")
    c, sd, x = vit_attn_case(g, "global64")
    B, H, W, C = x.shape
    heads = c["heads"]
    hd = C // heads
    assert ops.vit_attn_fused_ok((H, W), hd)
    qkv = _vit_qkv(c, sd, x).to(dt)
    q, k, v = qkv.float().reshape(B, H * W, 3, heads, hd).permute(2, 0, 3, 1, 4).reshape(3, B * heads, H * W, hd).unbind(0)
    th, tw = sd["rel_pos_h"].to(dt), sd["rel_pos_w"].to(dt)           # (2*64-1, hd): no re-interpolation needed
    got = ops.vit_attn_fused(qkv.to(DEV), th.to(DEV).contiguous(), tw.to(DEV).contiguous(), (H, W), heads, hd ** -0.5).float().cpu()
    want = oo.vit_attention_core(q, k, v, th.float(), tw.float(), (H, W), hd ** -0.5)
    want = want.view(B, heads, H * W, hd).permute(0, 2, 1, 3).reshape(B, H * W, C)
    assert rel_err(got, want) < tol_same
    out = F.linear(got, sd["proj.weight"], sd["proj.bias"]).view(B, H, W, C)
    assert rel_err(g.like("global64_out", out), g["global64_out"]) < tol_gold


def _fold_rel(qkv32, tab_h32, tab_w32, heads, hd, dt):
    """operands of hipie_vit_attn_rel from fp32 qkv / (re-interpolated) tables: q rows * scale*log2(e), tables / scale, rounded
    ONCE to the 16-bit type; plus the fp32 (q, k, v, tables) those 16-bit operands stand for (what the oracle is fed)."""
    from hipie_amd import ops
    scale = hd ** -0.5
    c1 = scale * ops.LOG2E
    C = heads * hd
    f = qkv32.clone()
    f[..., :C] *= c1
    f = f.to(dt)
    th, tw = (tab_h32 / scale).to(dt).contiguous(), (tab_w32 / scale).to(dt).contiguous()
    B, N = f.shape[:2]
    q, k, v = f.float().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).reshape(3, B * heads, N, hd).unbind(0)
    return f, th, tw, q / c1, k, v, th.float() * scale, tw.float() * scale


@pytest.mark.parametrize("dt,fast,tol_same,tol_gold", [(torch.float16, False, 1e-3, 2e-3), (torch.float16, True, 1.5e-3, 2e-3),
                                                        (torch.bfloat16, True, 8e-3, 2e-2)])
@pytest.mark.parametrize("name", ["window14", "global16", "global64", "global_rect", "global84"])
def test_vit_attention_rel(name, dt, fast, tol_same, tol_gold):
    """hipie_vit_attn_rel (bias computed in the kernel, pre-scaled q, two key rows per tile for the 14x14 windows) on the
    reference-generated cases: windowed 14x14, a 16x16 grid with interpolated tables, the real 64x64 grid, a 12x20 grid
    whose 32-query blocks wrap grid rows.  vs the oracle on the same 16-bit operands, and vs the reference golden."""
    import torch.nn.functional as F
    from hipie_amd import ops
    from hipie_amd.modeling.vit import resize_rel_pos
    g = Golden("vit_attn")
    c, sd, x = vit_attn_case(g, name)
    B, H, W, C = x.shape
    heads = c["heads"]
    hd = C // heads
    assert ops.vit_attn_rel_ok((H, W), hd)
    f, th, tw, q, k, v, th32, tw32 = _fold_rel(_vit_qkv(c, sd, x), resize_rel_pos(H, sd["rel_pos_h"]), resize_rel_pos(W, sd["rel_pos_w"]),
                                               heads, hd, dt)
    got = ops.vit_attn_rel(f.to(DEV), th.to(DEV), tw.to(DEV), (H, W), heads, fast=fast).float().cpu()
    want = oo.vit_attention_core(q, k, v, th32, tw32, (H, W), hd ** -0.5)
    want = want.view(B, heads, H * W, hd).permute(0, 2, 1, 3).reshape(B, H * W, C)
    assert rel_err(got, want) < tol_same
    out = F.linear(got, sd["proj.weight"], sd["proj.bias"]).view(B, H, W, C)
    assert rel_err(g.like(name + "_out", out), g[name + "_out"]) < tol_gold


@pytest.mark.parametrize("B,gh,gw,heads,hd,dt,fast", [
    (1, 64, 64, 16, 80, torch.float16, False),        # the ViT-H global block at 1024^2 (BASELINE configs[2,3])
    (1, 64, 64, 16, 80, torch.bfloat16, True),
    (1, 84, 84, 4, 80, torch.float16, True),          # 1344^2 (BASELINE configs[4]): 84-wide grid, 3 key blocks, 8-wave workgroups
    (2, 40, 64, 8, 64, torch.float16, True),          # ViT-B/L head dim, fewer rows than columns, batch/head swizzle on
    (3, 14, 14, 5, 80, torch.float16, False),         # windows: 7-wave workgroups, odd batch*heads (no swizzle)
    (2, 7, 14, 2, 80, torch.float16, True),           # odd number of key rows with two rows per tile (ragged last tile)
    (1, 33, 50, 3, 64, torch.float16, False)])
def test_vit_attention_rel_against_materialised_scores(B, gh, gw, heads, hd, dt, fast):
    """the reference's own formulation with the (N x N) score tensor materialised in fp32 on the device
    (backbone/vit.py:72-80 + utils.py:96-125) on random operands, at the full-size geometries."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(21 + gh + gw)
    N, C = gh * gw, heads * hd
    scale = hd ** -0.5
    f, th, tw, q, k, v, th32, tw32 = _fold_rel(torch.randn(B, N, 3 * C, generator=gen) * 0.8, torch.randn(2 * gh - 1, hd, generator=gen) * 0.2,
                                               torch.randn(2 * gw - 1, hd, generator=gen) * 0.2, heads, hd, dt)
    q, k, v = (t.to(DEV).view(B, heads, N, hd) for t in (q, k, v))
    idx_h = torch.arange(gh, device=DEV)[:, None] - torch.arange(gh, device=DEV)[None, :] + gh - 1
    idx_w = torch.arange(gw, device=DEV)[:, None] - torch.arange(gw, device=DEV)[None, :] + gw - 1
    Rh, Rw = th32.to(DEV)[idx_h], tw32.to(DEV)[idx_w]
    rq = q.reshape(B, heads, gh, gw, hd)
    rel_h = torch.einsum("bmhwc,hkc->bmhwk", rq, Rh)
    rel_w = torch.einsum("bmhwc,wkc->bmhwk", rq, Rw)
    attn = (q * scale) @ k.transpose(-2, -1)
    attn = (attn.view(B, heads, gh, gw, gh, gw) + rel_h[..., :, None] + rel_w[..., None, :]).view(B, heads, N, N)
    want = (attn.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, N, C)
    got = ops.vit_attn_rel(f.to(DEV), th.to(DEV), tw.to(DEV), (gh, gw), heads, fast=fast).float()
    assert rel_err(got.cpu(), want.cpu()) < (8e-3 if dt == torch.bfloat16 else 1.5e-3 if fast else 1e-3)


@pytest.mark.parametrize("B,gh,heads,hd", [(2, 48, 8, 64), (1, 64, 16, 80), (3, 5, 3, 80)])
def test_vit_attention_fused_equals_unfused(B, gh, heads, hd):
    """fused prologue == hipie_vit_relpos + hipie_vit_attn on random data: batch/head swizzle on and off, fewer rows than 64."""
    from hipie_amd import ops
    gw = 64
    gen = torch.Generator().manual_seed(gh * 7 + hd)
    qkv = (torch.randn(B, gh * gw, 3 * heads * hd, generator=gen) * 0.7).bfloat16().to(DEV)
    th = (torch.randn(2 * gh - 1, hd, generator=gen) * 0.3).bfloat16().to(DEV)
    tw = (torch.randn(2 * gw - 1, hd, generator=gen) * 0.3).bfloat16().to(DEV)
    rel_h, rel_w = ops.vit_relpos(qkv, th, tw, (gh, gw), heads)
    a = ops.vit_attn(qkv, rel_h, rel_w, (gh, gw), heads, hd ** -0.5).float()
    b = ops.vit_attn_fused(qkv, th, tw, (gh, gw), heads, hd ** -0.5).float()
    assert rel_err(b.cpu(), a.cpu()) < 4e-3                            # both round P to bf16; the biases agree to fp32 rounding


def test_vit_attention_fused_rejects_other_grids():
    from hipie_amd import ops
    from hipie_amd._lib import HipieLibraryError
    qkv = torch.zeros(1, 14 * 14, 3 * 80, dtype=torch.bfloat16, device=DEV)
    t = torch.zeros(27, 80, dtype=torch.bfloat16, device=DEV)
    with pytest.raises((HipieLibraryError, RuntimeError)):
        ops.vit_attn_fused(qkv, t, t, (14, 14), 1, 80 ** -0.5)


@pytest.mark.parametrize("dt,tol", [(torch.float16, 1.5e-3), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("name", ["L20", "L600_pad", "clamp"])
def test_bi_xattn(name, dt, tol):
    """hipie_bi_xattn vs the oracle core on the same 16-bit-rounded projections (incl. the +-5e4 clamp case)."""
    import torch.nn.functional as F
    from hipie_amd import ops
    g = Golden("bi_attn")
    c, sd, v, l, mask = bi_case(g, name)
    B, Nv, L, Hh, hd = c["B"], c["Nv"], c["L"], 8, 256
    vn = F.layer_norm(v, (256,), sd["layer_norm_v.weight"], sd["layer_norm_v.bias"])
    ln_ = F.layer_norm(l, (768,), sd["layer_norm_l.weight"], sd["layer_norm_l.bias"])
    q = (F.linear(vn, sd["attn.v_proj.weight"], sd["attn.v_proj.bias"]) * hd ** -0.5).to(dt)
    k = F.linear(ln_, sd["attn.l_proj.weight"], sd["attn.l_proj.bias"]).to(dt)
    vv = F.linear(vn, sd["attn.values_v_proj.weight"], sd["attn.values_v_proj.bias"]).to(dt)
    vl = F.linear(ln_, sd["attn.values_l_proj.weight"], sd["attn.values_l_proj.bias"]).to(dt)
    if dt == torch.float16 and name == "clamp":
        pytest.skip("3000x scaled activations overflow fp16 (the clamp case is a bf16/fp32-range case)")

    def split(t, n):
        return t.float().view(B, n, Hh, hd).transpose(1, 2).reshape(B * Hh, n, hd)
    wv, wl = oo.bi_attention_core(split(q, Nv), split(k, L), split(vv, Nv), split(vl, L), mask)
    wv = wv.view(B, Hh, Nv, hd).transpose(1, 2).reshape(B, Nv, Hh * hd)
    wl = wl.view(B, Hh, L, hd).transpose(1, 2).reshape(B, L, Hh * hd)
    ov, ol = ops.bi_xattn(q.view(B, Nv, Hh, hd).to(DEV), k.view(B, L, Hh, hd).to(DEV), vv.view(B, Nv, Hh, hd).to(DEV),
                          vl.view(B, L, Hh, hd).to(DEV), mask.to(DEV))
    assert rel_err(ov.float().cpu(), wv) < tol
    assert rel_err(ol.float().cpu(), wl) < tol


@pytest.mark.parametrize("hd,nq,nk", [(80, 200, 333), (64, 1500, 640), (32, 77, 64), (256, 130, 100)])
def test_flash_attn_generic(hd, nq, nk):
    """hipie_flash_attn without bias: ragged tails, every head dim, strided q/k/v views against dense copies."""
    import os
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(9)
    qkv = torch.randn(2, max(nq, nk), 3, 4, hd, generator=gen).half().to(DEV)
    q, k, v = qkv[:, :nq, 0], qkv[:, :nk, 1], qkv[:, :nk, 2]            # strided views, head_dim contiguous
    a = ops.flash_attn(q, k, v, hd ** -0.5)
    b = ops.flash_attn(q.contiguous(), k.contiguous(), v.contiguous(), hd ** -0.5)      # the same numbers from dense operands
    assert rel_err(a.float().cpu(), b.float().cpu()) < 1e-6
    ref = torch.nn.functional.scaled_dot_product_attention(q.float().cpu().transpose(1, 2), k.float().cpu().transpose(1, 2),
                                                           v.float().cpu().transpose(1, 2)).transpose(1, 2).reshape(2, nq, 4 * hd)
    assert rel_err(a.float().cpu(), ref) < 1e-3


@pytest.mark.parametrize("C,rows", [(1280, 1000), (256, 4099), (160, 37), (2048, 5), (4, 1), (8, 3), (252, 5), (260, 7)])
def test_add_layernorm(C, rows):
    """hipie_add_layernorm vs torch fp32: fp32 in/out 2e-6; 16-bit storage within its rounding.  The last four are the widths of the
    backward's SHAPES: a tail vector only (4, 8), the longest tail (252), one full vector and a one-lane tail (260)."""
    import torch.nn.functional as F
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(rows, C, generator=gen) * 3
    d = torch.randn(rows, C, generator=gen)
    w = 1 + 0.1 * torch.randn(C, generator=gen)
    b = 0.1 * torch.randn(C, generator=gen)
    want_res = x + d
    want = F.layer_norm(want_res, (C,), w, b, 1e-6)
    res, out = ops.add_layernorm(x.to(DEV), d.to(DEV), w.to(DEV), b.to(DEV), 1e-6, torch.float32)
    assert rel_err(res.cpu(), want_res) < 1e-6 and rel_err(out.cpu(), want) < 2e-6
    _, out0 = ops.add_layernorm(x.to(DEV), None, w.to(DEV), b.to(DEV), 1e-6, torch.float32)
    assert rel_err(out0.cpu(), F.layer_norm(x, (C,), w, b, 1e-6)) < 2e-6
    xb, db = x.bfloat16(), d.half()
    res, out = ops.add_layernorm(xb.to(DEV), db.to(DEV), w.to(DEV), b.to(DEV), 1e-6, torch.float16)
    s = xb.float() + db.float()
    assert rel_err(res.float().cpu(), s) < 8e-3
    assert rel_err(out.float().cpu(), F.layer_norm(s, (C,), w, b, 1e-6)) < 2e-3


@pytest.mark.parametrize("B,H,W,ws", [(2, 9, 11, 4), (1, 64, 64, 14), (2, 28, 14, 14)])
def test_add_layernorm_window_row_maps(B, H, W, ws):
    """hipie_add_layernorm_rows: LN written straight into the zero-padded window layout == window_partition(LN(x + d)),
    and the residual add reading the window layout == x + window_unpartition(y) (hipie/backbone/utils.py:16-60)."""
    import torch.nn.functional as F
    from hipie_amd import ops
    from hipie_amd.modeling.vit import window_partition, window_row_maps, window_unpartition
    C = 160
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, C, generator=gen) * 2
    d = torch.randn(B, H, W, C, generator=gen)
    w = 1 + 0.1 * torch.randn(C, generator=gen)
    b = 0.1 * torch.randn(C, generator=gen)
    out_src, delta_row, nwin = window_row_maps(B, H, W, ws, DEV)
    res, out = ops.add_layernorm(x.to(DEV), d.to(DEV), w.to(DEV), b.to(DEV), 1e-6, torch.float32, out_src=out_src)
    want, pad_hw = window_partition(F.layer_norm(x + d, (C,), w, b, 1e-6), ws)
    assert out.shape[0] == nwin * ws * ws
    assert rel_err(res.cpu(), x + d) < 1e-6
    assert rel_err(out.cpu().view_as(want), want) < 2e-6
    assert (out.cpu().view_as(want)[want == 0] == 0).all()                 # pad rows are exact zeros
    ywin = torch.randn(nwin, ws, ws, C, generator=gen)
    res2, out2 = ops.add_layernorm(x.to(DEV), ywin.reshape(-1, C).to(DEV), w.to(DEV), b.to(DEV), 1e-6, torch.float32,
                                   delta_row=delta_row)
    s = x + window_unpartition(ywin, ws, pad_hw, (H, W))
    assert rel_err(res2.cpu(), s) < 1e-6
    assert rel_err(out2.cpu(), F.layer_norm(s, (C,), w, b, 1e-6)) < 2e-6


@pytest.mark.parametrize("name", ["window14", "global16", "global64", "global_rect"])
def test_vit_relpos_tables(name):
    """hipie_vit_relpos == the reference's two einsums over get_rel_pos (fp32) on the same 16-bit q and tables."""
    from hipie_amd import ops
    from hipie_amd.modeling.vit import resize_rel_pos
    g = Golden("vit_attn")
    c, sd, x = vit_attn_case(g, name)
    B, H, W, C = x.shape
    heads = c["heads"]
    hd = C // heads
    for dt, tol in ((torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)):
        qkv = _vit_qkv(c, sd, x).to(dt)
        th = resize_rel_pos(H, sd["rel_pos_h"]).to(dt).contiguous()
        tw = resize_rel_pos(W, sd["rel_pos_w"]).to(dt).contiguous()
        q = qkv.float().reshape(B, H * W, 3, heads, hd)[:, :, 0].permute(0, 2, 1, 3).reshape(B * heads, H, W, hd)
        Rh = oo.get_rel_pos(H, H, th.float())
        Rw = oo.get_rel_pos(W, W, tw.float())
        want_h = torch.einsum("bhwc,hkc->bkhw", q, Rh).reshape(B * heads, H, H * W)
        want_w = torch.einsum("bhwc,wkc->bhwk", q, Rw).reshape(B * heads, H * W, W)
        rh, rw = ops.vit_relpos(qkv.to(DEV), th.to(DEV), tw.to(DEV), (H, W), heads)
        assert rel_err(rh.cpu(), want_h) < 1e-5 and rel_err(rw.cpu(), want_w) < 1e-5    # fp32 accumulate of exact products


def test_msda_fused_full_scale_strided_aux():
    """BASELINE-size geometry (Nv = 21760 @1024^2, batch 2), 16-bit value and a single strided bf16 projection tensor for
    offsets + logits: the strided 16-bit aux gives what dense fp32 aux of the same numbers gives, the op is linear in `value`, and (msda_d32_kernel
    map 2 at the production size) it agrees with the float64 reference on the first and last tile of every level plus ~4000 random
    queries -- bf16 as called, and with the same numbers as an fp32 value, where the bound is tight enough to see a misplaced sample.

    fp32 bound on this geometry (levels above 64 pixels: fp32 rounding of a location is ~1e-5 pixel): the oracle run in float32 against
    ref_fused on these inputs and queries measures 3.07e-6 (test_gpu_msda_forward.LARGE_GEOMETRY_F32_ORACLE_ERR, docs/measurements.md), so
    max(2e-5, 4 x 3.07e-6) = 2e-5."""
    from hipie_amd import ops
    from test_gpu_msda_forward import full_scale_inputs, bench_geometry_queries, ref_fused, large_geometry_f32_bound
    M, L, P = 8, 4, 4
    value, shapes, lstart, ref, proj = (t.to(DEV) for t in full_scale_inputs())       # seed 3, the inputs this test has always used
    off = proj[..., :256].unflatten(-1, (M, L, P, 2))
    lg = proj[..., 256:].unflatten(-1, (M, L * P))
    ss, ls = shapes, lstart
    a = ops.msda_fused(value, ss, ls, ref, off, lg)
    b = ops.msda_fused(value, ss, ls, ref, off.float().contiguous(), lg.float().contiguous())   # dense fp32 aux, same numbers
    assert rel_err(a.float().cpu(), b.float().cpu()) < 1e-6
    c = ops.msda_fused((2 * value.float()).bfloat16(), ss, ls, ref, off, lg)                     # linearity in value
    assert rel_err(c.float().cpu(), 2 * a.float().cpu()) < 1e-2
    assert torch.isfinite(a.float()).all()
    # against the float64 reference on a query subset (the op is independent per query)
    q = bench_geometry_queries(shapes.cpu())
    want = ref_fused(value, shapes, lstart, ref, off, lg, queries=q)
    for name, got in (("bf16 value, strided bf16 aux", a), ("bf16 value, dense fp32 aux", b)):
        err = rel_err(got[:, q.to(DEV)].float().cpu(), want)
        print("full scale, %s: rel_err %.3e over %d queries" % (name, err, q.numel()))
        assert err < max(8e-3, large_geometry_f32_bound("bench_128")), (name, err)
    f = ops.msda_fused(value.float(), ss, ls, ref, off.float().contiguous(), lg.float().contiguous())
    err = rel_err(f[:, q.to(DEV)].cpu(), want)
    print("full scale, fp32 value and aux: rel_err %.3e" % err)
    assert err < large_geometry_f32_bound("bench_128"), err


@pytest.mark.parametrize("form", ["decoder", "encoder"])
def test_msda_fused_beside_gemms(form):
    """hipie_msda_fused on a side stream while gemm_kernel<256> (the K = 256 projections of the encoder layers) fills the chip on the
    main stream: 50 rounds x 4 launches, every output EQUAL to the kernel run alone.  Until round 6 this failed in ~25 % of the launches
    (pairs of adjacent (query, head) groups = lanes 48-63 of a wave): a gfx950 erratum of packed fp32 VALU instructions with a swapped
    second source (tools/ubench/pk_f32_hazard.hip) -- msda.hip is now built without them and
    tests/test_isa_hazards.py keeps the form out of every file.  The stateless, stream-parameterised ABI (include/hipie_mi355.h) promises
    exactly this: a kernel's results do not depend on what runs beside it."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(0)
    B, S, Q = 8, 21760, 300
    shapes = torch.tensor([[128, 128], [64, 64], [32, 32], [16, 16]], device=DEV)
    lstart = _lsi(shapes.cpu()).to(DEV)
    val = torch.randn(B, S, 8, 32, generator=gen).to(DEV)
    if form == "decoder":
        ref = (torch.rand(B, Q, 4, 4, generator=gen) * 0.5 + 0.25).to(DEV)
        off, lg = torch.randn(B, Q, 8, 4, 4, 2, generator=gen).to(DEV), torch.randn(B, Q, 8, 16, generator=gen).to(DEV)
    else:
        ref = torch.rand(B, S, 4, 2, generator=gen).to(DEV)
        off, lg = torch.randn(B, S, 8, 4, 4, 2, generator=gen).to(DEV), torch.randn(B, S, 8, 16, generator=gen).to(DEV)
    x = torch.randn(B * S, 256, generator=gen).to(DEV)
    w = ops.hl8_pack(torch.randn(256, 256, generator=gen) * 0.06).to(DEV)
    fn = lambda: ops.msda_fused(val, shapes, lstart, ref, off, lg)
    want = fn().clone()
    torch.cuda.synchronize()
    side, main = torch.cuda.Stream(), torch.cuda.current_stream()
    bad = 0
    for it in range(50 if form == "decoder" else 12):
        side.wait_stream(main)
        for _ in range(3):
            ops.gemm(x, w, None, split=True, out_fmt=ops.F32)
        with torch.cuda.stream(side):
            outs = [fn() for _ in range(4)]
        main.wait_stream(side)
        torch.cuda.synchronize()
        bad += sum(int(not torch.equal(o, want)) for o in outs)
    assert bad == 0, "%d launches beside gemm_kernel<256> differ from the kernel run alone" % bad


def test_mask_einsum_full_size_against_library_gemm():
    """BASELINE-size contraction (300 queries x 256 channels x 256^2 pixels, batch 2): exact-fp32 MFMA path against an fp32
    library GEMM on the same device, and linearity of the bf16x3 path."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(8)
    emb = torch.randn(2, 300, 256, generator=gen).to(DEV)
    feat = torch.randn(2, 256, 256, 256, generator=gen).to(DEV)
    want = torch.bmm(emb, feat.flatten(2)).view(2, 300, 256, 256)
    got = ops.mask_einsum(emb, feat, precision=0)
    assert rel_err(got.cpu(), want.cpu()) < 2e-6
    a = ops.mask_einsum(emb, feat, precision=1)
    assert rel_err(a.cpu(), want.cpu()) < 3e-5
    b = ops.mask_einsum(3.0 * emb, feat, precision=1)
    assert rel_err(b.cpu(), 3.0 * a.cpu()) < 3e-5


def test_vit_attention_full_grid_against_materialised_scores():
    """the real global-attention geometry (64x64 tokens, 16 heads x 80) against the reference's own formulation with the
    (N x N) score tensor materialised in fp32 on the device (backbone/vit.py:72-80 + utils.py:96-125), fused and unfused."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(21)
    B, gh, gw, heads, hd = 1, 64, 64, 16, 80
    N, C = gh * gw, heads * hd
    qkv = (torch.randn(B, N, 3 * C, generator=gen) * 0.8).half().to(DEV)
    th = (torch.randn(2 * gh - 1, hd, generator=gen) * 0.2).half().to(DEV)
    tw = (torch.randn(2 * gw - 1, hd, generator=gen) * 0.2).half().to(DEV)
    q, k, v = qkv.float().view(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)        # (B, heads, N, hd)
    idx_h = torch.arange(gh, device=DEV)[:, None] - torch.arange(gh, device=DEV)[None, :] + gh - 1
    idx_w = torch.arange(gw, device=DEV)[:, None] - torch.arange(gw, device=DEV)[None, :] + gw - 1
    Rh, Rw = th.float()[idx_h], tw.float()[idx_w]                                          # (gh, gh, hd), (gw, gw, hd)
    rq = q.reshape(B, heads, gh, gw, hd)
    rel_h = torch.einsum("bmhwc,hkc->bmhwk", rq, Rh)
    rel_w = torch.einsum("bmhwc,wkc->bmhwk", rq, Rw)
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
    attn = (attn.view(B, heads, gh, gw, gh, gw) + rel_h[..., :, None] + rel_w[..., None, :]).view(B, heads, N, N)
    want = (attn.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, N, C)
    fused = ops.vit_attn_fused(qkv, th, tw, (gh, gw), heads, hd ** -0.5).float()
    assert rel_err(fused.cpu(), want.cpu()) < 1e-3
    bh, bw = ops.vit_relpos(qkv, th, tw, (gh, gw), heads)
    unfused = ops.vit_attn(qkv, bh, bw, (gh, gw), heads, hd ** -0.5).float()
    assert rel_err(unfused.cpu(), want.cpu()) < 1e-3


def test_glue_sine_embed_and_box_refine():
    """hipie_sine_embed / hipie_box_refine against the product's own eager restatements of get_sine_pos_embed
    (deformable_transformer_dino.py:636-670) and of sigmoid(delta + inverse_sigmoid(ref)), fp32, incl. a row-strided view."""
    from hipie_amd import ops
    from hipie_amd.modeling.transformer import get_sine_pos_embed, inverse_sigmoid
    gen = torch.Generator().manual_seed(5)
    ref = torch.rand(3, 37, 4, 4, generator=gen).to(DEV)
    for view in (ref[:, :, 0, :], ref[:, :, 0, :].contiguous(), ref[:, :, 0, :2].contiguous()):
        want = get_sine_pos_embed(view)
        got = ops.sine_embed(view)
        assert got.shape == want.shape and rel_err(got.cpu(), want.cpu()) < 2e-6
    half = ops.sine_embed(ref[:, :, 0, :], out_dtype=torch.float16)
    assert rel_err(half.float().cpu(), get_sine_pos_embed(ref[:, :, 0, :]).cpu()) < 6e-4
    r = torch.rand(2, 50, 4, generator=gen)
    r[0, 0] = torch.tensor([0.0, 1.0, 1e-7, 1.0 - 1e-7])                       # the clamps of inverse_sigmoid
    d = torch.randn(2, 50, 4, generator=gen)
    want = (d + inverse_sigmoid(r)).sigmoid()
    assert rel_err(ops.box_refine(d.to(DEV), r.to(DEV)).cpu(), want) < 2e-6
    assert rel_err(ops.box_refine(d.half().to(DEV), r.to(DEV)).cpu(), (d.half().float() + inverse_sigmoid(r)).sigmoid()) < 2e-6


def test_empty_inputs_are_handled():
    from hipie_amd import ops
    keep, count = ops.batched_nms(torch.zeros(2, 0, 4, device=DEV), torch.zeros(2, 0, device=DEV),
                                  torch.zeros(2, 0, dtype=torch.long, device=DEV), 0.7)
    assert keep.shape == (2, 0) and count.tolist() == [0, 0]
    m = ops.mask_finalize(torch.zeros(4, 8, 8, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), 4, (32, 32), (32, 32), 0.5)
    assert m.shape == (0, 32, 32)
    shapes = torch.tensor([(4, 4)], device=DEV)
    out = ops.msda_fused(torch.zeros(1, 16, 8, 32, device=DEV), shapes, torch.zeros(1, dtype=torch.long, device=DEV),
                         torch.zeros(1, 0, 1, 2, device=DEV), torch.zeros(1, 0, 8, 1, 4, 2, device=DEV),
                         torch.zeros(1, 0, 8, 4, device=DEV))
    assert out.shape == (1, 0, 256)


@pytest.mark.parametrize("dt,ddt", [(torch.float16, torch.float16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("shape", [(3, 301, 256), (5, 8), (5, 260), (5, 2048)], ids=lambda s: "x".join(map(str, s)))
def test_decoder_glue_layernorm_dec_and_add_cast(shape, dt, ddt):
    """hipie_add_layernorm_dec / hipie_add_cast against the eager chain they replace in the decoder layers; 256 is the decoders' width,
    8 is a tail vector only, 260 one full vector and a one-lane tail, 2048 the widest row."""
    import torch.nn.functional as F
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(11)
    C = shape[-1]
    x = torch.randn(*shape, generator=gen).to(DEV)
    delta = torch.randn(*shape, generator=gen).to(DEV).to(ddt)
    qp = torch.randn(*shape, generator=gen).to(DEV).to(dt)
    w, b = torch.randn(C, generator=gen).to(DEV), torch.randn(C, generator=gen).to(DEV)
    want = F.layer_norm(x + delta.float(), (C,), w, b, 1e-5)
    n32, n16, s16 = ops.add_layernorm_dec(x, delta, w, b, 1e-5, dt, want16=True, addend=qp)
    assert rel_err(n32.cpu(), want.cpu()) < 2e-6
    assert torch.equal(n16, n32.to(dt))
    assert torch.equal(s16, (n32 + qp.float()).to(dt))
    n32b, none16, nones = ops.add_layernorm_dec(x, delta, w, b, 1e-5, dt)
    assert none16 is None and nones is None and torch.equal(n32b, n32)
    assert torch.equal(ops.add_cast(x, qp), (x + qp.float()).to(dt))


@pytest.mark.parametrize("C", [8, 260, 1280])
def test_layernorm_forward_kernels_agree(C):
    """For fp32 x and delta the two forward kernels give the same fp32 bits, and the backward recomputes the forward's xhat: for ONE row
    and gy = 1, dgamma = 0 + 1 * xhat is the backward's xhat, and with gamma = 1, beta = 0 the forward's output is its own.  (dx for
    gy = 1 / gamma is a rounding residue, not exact zero: docs/measurements.md.)"""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(C)
    x, d = (torch.randn(5, C, generator=gen) * 3).to(DEV), torch.randn(5, C, generator=gen).to(DEV)
    w, b = (1 + 0.1 * torch.randn(C, generator=gen)).to(DEV), (0.1 * torch.randn(C, generator=gen)).to(DEV)
    for eps in (1e-6, 1e-5):
        s, n = ops.add_layernorm(x, d, w, b, eps, torch.float32)
        assert torch.equal(ops.add_layernorm_dec(x, d, w, b, eps, torch.float16)[0], n)
        one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        xhat = ops.add_layernorm(s, None, one, zero, eps, torch.float32)[1]
        for r in range(s.shape[0]):
            dgamma = ops.layernorm_backward(s[r:r + 1], one[None], w, eps)[1]
            assert torch.equal(dgamma, xhat[r]), (eps, r)


@pytest.mark.parametrize("nq", [910, 300])
def test_decoder_self_attention_at_query_counts(nq):
    """the decoder self-attention (nn.MultiheadAttention semantics, q = k = tgt + pos, v = tgt; deformable_transformer_dino.py
    :435-436) on hipie_flash_attn at the two query counts of the path -- 910 (900 + 10 background queries, DINO decoder) and
    300 (MaskDINO decoder) -- against the oracle's fp32 formulation.  fp16 operands: 1e-3."""
    import oracle.model as om
    from hipie_amd.modeling.transformer import MultiheadAttention
    torch.manual_seed(nq)
    m = MultiheadAttention(256, 8, torch.float16).to(DEV)
    m.in_proj_bias.data.normal_(0, 0.1)
    x_v = torch.randn(2, nq, 256)
    x_qk = x_v + torch.randn(2, nq, 256)
    sd = {"sa." + k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    want = om.mha(x_qk, x_v, sd, "sa.")
    got = m(x_qk.to(DEV), x_v.to(DEV)).float().cpu()
    assert rel_err(got, want) < 1e-3
    # the 16-bit policy's weights (the fused decoder path): within the fp16 operand tolerance
    m16 = MultiheadAttention(256, 8, torch.float16).to(DEV)
    m16.load_state_dict(m.state_dict())
    m16.in_proj_weight.data = m16.in_proj_weight.data.half()
    m16.in_proj_bias.data = m16.in_proj_bias.data.half()
    m16.out_proj.weight.data = m16.out_proj.weight.data.half()
    m16.out_proj.bias.data = m16.out_proj.bias.data.half()
    got16 = m16(x_qk.to(DEV).half(), x_v.to(DEV).half()).float().cpu()
    assert rel_err(got16, want) < 4e-3


def test_decoder_layer_fast_path_matches_oracle():
    """DeformableTransformerDecoderLayer.forward16 (fp32 stream, 16-bit GEMMs, fused LayerNorm outputs, value block of a batched
    projection) against the oracle's decoder_layer in fp32, 300 queries, 4 levels."""
    import oracle.model as om
    from hipie_amd.modeling.transformer import (DeformableTransformerDecoderLayer, batched_decoder_values, cast_head, level_tensors)
    torch.manual_seed(5)
    dt = torch.float16
    layers = torch.nn.ModuleList([DeformableTransformerDecoderLayer(256, 512, 4, 8, 4, dt, dt) for _ in range(3)]).to(DEV)
    for l in layers:
        for p in l.parameters():
            if p.dim() == 1:
                p.data.normal_(0, 0.1)
        l.cross_attn.sampling_offsets.weight.data.normal_(0, 0.05)
        l.cross_attn.attention_weights.weight.data.normal_(0, 0.2)
        for n in (l.norm1, l.norm2, l.norm3):
            n.weight.data.fill_(1.0).add_(0.05 * torch.randn(256, device=DEV))
    sd32 = [{k: v.detach().float().cpu().clone() for k, v in l.state_dict().items()} for l in layers]
    cast_head(layers, dt, dt)
    shapes = [(16, 24), (8, 12), (4, 6), (2, 3)]
    S = sum(h * w for h, w in shapes)
    B, Q = 2, 300
    src = torch.randn(B, S, 256)
    tgt, qpos = torch.randn(B, Q, 256), torch.randn(B, Q, 256) * 0.5
    refs = torch.rand(B, Q, 4, 4) * 0.5 + 0.25
    ss, ls = level_tensors(shapes, torch.device(DEV))
    values = batched_decoder_values(layers, layers, src.to(DEV).to(dt), None)
    lid = 1                                                                            # a middle column block of the batched GEMM
    t32, t16 = layers[lid].forward16(tgt.to(DEV), tgt.to(DEV).to(dt), qpos.to(DEV).to(dt), refs.to(DEV), values[lid], ss, ls)
    sd = {"l." + k: v for k, v in sd32[lid].items()}
    want = om.decoder_layer(tgt, qpos.to(dt).float(), refs, src, shapes, None, sd, "l.")
    assert rel_err(t32.float().cpu(), want) < 4e-3
    assert torch.equal(t16, t32.to(dt))


@pytest.mark.parametrize("shape,nhwc,dt,odt,relu,pre", [((2, 256, 16, 24), True, torch.float16, torch.float16, False, False),
                                                         ((3, 256, 33, 17), True, torch.float32, torch.float32, True, True),
                                                         ((2, 256, 32, 32), False, torch.float16, torch.float16, True, True),
                                                         ((1, 256, 128, 128), False, torch.float32, torch.float32, False, False),
                                                         ((2, 256, 8, 8), True, torch.bfloat16, torch.float32, True, False)])
def test_group_norm(shape, nhwc, dt, odt, relu, pre):
    """hipie_group_norm vs torch (fp32 reference of the same op) in both memory formats, with the fused pre-bias and ReLU."""
    import torch.nn.functional as F
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=gen) * 2 + 0.5).to(dt)
    w, b = 1 + 0.2 * torch.randn(256, generator=gen), 0.2 * torch.randn(256, generator=gen)
    pb = torch.randn(256, generator=gen) if pre else None
    xin = x.to(DEV)
    if nhwc:
        xin = xin.contiguous(memory_format=torch.channels_last)
    got = ops.group_norm(xin, 32, w.to(DEV), b.to(DEV), 1e-5, relu=relu, prebias=None if pb is None else pb.to(DEV), out_dtype=odt)
    assert got.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    xr = x.float() + (0 if pb is None else pb.view(1, -1, 1, 1))
    want = F.group_norm(xr, 32, w, b, 1e-5)
    if relu:
        want = F.relu(want)
    tol = 2e-5 if odt == torch.float32 else 1.5e-3
    assert rel_err(got.float().cpu(), want) < tol


@pytest.mark.parametrize("L,nv,nvalid,dt,tol", [(194, 1300, 194, torch.float16, 1.5e-3), (194, 777, 150, torch.bfloat16, 1e-2),
                                                (100, 300, 100, torch.float16, 1.5e-3), (224, 2000, 201, torch.float16, 1.5e-3),
                                                (65, 256, 3, torch.float16, 1.5e-3)])
def test_bi_xattn_short_text_kernel(L, nv, nvalid, dt, tol):
    """the image -> text kernel for one short text (64 < L <= 224, head dim 256: the 80-class caption is 194 tokens): ragged
    query tiles (nv % 256 != 0, several tiles per workgroup), padded text rows, a partial text mask, both block counts; against
    the oracle's BiMultiHeadAttention core on the same 16-bit operands.  The text -> image half of the call runs the generic
    kernel and is checked in the same breath."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(L * 7 + nv)
    B, Hh, hd = 2, 2, 256
    q = (torch.randn(B, nv, Hh, hd, generator=gen) * 0.25).to(dt)
    k = (torch.randn(B, L, Hh, hd, generator=gen) * 0.25).to(dt)
    vv = torch.randn(B, nv, Hh, hd, generator=gen).to(dt)
    vl = torch.randn(B, L, Hh, hd, generator=gen).to(dt)
    mask = torch.zeros(B, L, dtype=torch.int64)
    mask[0, :nvalid] = 1
    mask[1, :max(1, nvalid // 2)] = 1

    def split(t, n):
        return t.float().transpose(1, 2).reshape(B * Hh, n, hd)
    wv, wl = oo.bi_attention_core(split(q, nv), split(k, L), split(vv, nv), split(vl, L), mask)
    wv = wv.view(B, Hh, nv, hd).transpose(1, 2).reshape(B, nv, Hh * hd)
    wl = wl.view(B, Hh, L, hd).transpose(1, 2).reshape(B, L, Hh * hd)
    ov, ol = ops.bi_xattn(q.to(DEV), k.to(DEV), vv.to(DEV), vl.to(DEV), mask.to(DEV))
    assert rel_err(ov.float().cpu(), wv) < tol
    assert rel_err(ol.float().cpu(), wl) < tol


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_add_layernorm_sum(dt):
    """hipie_add_layernorm_sum: LayerNorm(x + delta) and LayerNorm(x + delta) + addend from one launch."""
    import torch.nn.functional as F
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 777, 256, generator=gen).to(DEV).to(dt)
    d = torch.randn(2, 777, 256, generator=gen).to(DEV).to(dt)
    pos = torch.randn(2, 777, 256, generator=gen).to(DEV).to(dt)
    w, b = torch.randn(256, generator=gen).to(DEV), torch.randn(256, generator=gen).to(DEV)
    n, s = ops.add_layernorm_sum(x, d, w, b, 1e-5, pos)
    want = F.layer_norm(x.float() + d.float(), (256,), w, b, 1e-5)
    tol = 2e-6 if dt == torch.float32 else 1e-3
    assert rel_err(n.float().cpu(), want.cpu()) < tol
    assert rel_err(s.float().cpu(), (want + pos.float()).cpu()) < tol
    assert torch.equal(n, ops.add_layernorm(x, d, w, b, 1e-5, dt, want_res=False)[1])


def test_add_layernorm_optional_arguments_do_not_carry_over():
    """the row maps of hipie_add_layernorm_rows and the addend of hipie_add_layernorm_sum belong to their own call: the plain call
    after them gives, bit for bit, what it gave before them (tolerances of the mapped / summed results as in test_add_layernorm)."""
    import torch.nn.functional as F
    from hipie_amd import ops
    C, rows = 160, 37
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(rows, C, generator=gen) * 3).to(DEV)
    d = torch.randn(rows, C, generator=gen).to(DEV)
    pos = torch.randn(rows, C, generator=gen).to(DEV)
    w = (1 + 0.1 * torch.randn(C, generator=gen)).to(DEV)
    b = (0.1 * torch.randn(C, generator=gen)).to(DEV)
    want = F.layer_norm((x + d).cpu(), (C,), w.cpu(), b.cpu(), 1e-6)
    before = ops.add_layernorm(x, d, w, b, 1e-6, torch.float32)[1].clone()
    assert rel_err(before.cpu(), want) < 2e-6
    perm = torch.randperm(rows, generator=gen)
    out_src = torch.cat((perm[:5], torch.tensor([-1]), perm[5:])).to(torch.int32)       # every row once, one padding row
    res, mapped = ops.add_layernorm(x, d, w, b, 1e-6, torch.float32, out_src=out_src.to(DEV))
    want_mapped = torch.cat((want[perm[:5]], torch.zeros(1, C), want[perm[5:]]))
    assert rel_err(res.cpu(), (x + d).cpu()) < 1e-6 and rel_err(mapped.cpu(), want_mapped) < 2e-6
    assert (mapped[5] == 0).all()
    n, s = ops.add_layernorm_sum(x, d, w, b, 1e-6, pos)
    assert rel_err(n.cpu(), want) < 2e-6 and rel_err(s.cpu(), want + pos.cpu()) < 2e-6
    after = ops.add_layernorm(x, d, w, b, 1e-6, torch.float32)[1]
    assert torch.equal(after, before)


@pytest.mark.parametrize("dt,tol", [(torch.float32, 5e-6), (torch.float16, 2e-3)])
def test_decoder_heads_fused(dt, tol):
    """hipie_ref_point_mlp / hipie_box_head against the chains they replace: get_sine_pos_embed -> ref_point_head (oracle's
    sine_embed_4 + mlp) and bbox_embed -> sigmoid(. + inverse_sigmoid(ref)), at 300 and 910 queries (ragged last row block)."""
    import oracle.model as om
    from hipie_amd import ops
    from hipie_amd.modeling.transformer import MLP, cast_head
    torch.manual_seed(21)
    rp = MLP(512, 256, 256, 2).to(DEV)
    bb = MLP(256, 256, 4, 3).to(DEV)
    for m in (rp, bb):
        for p in m.parameters():
            if p.dim() == 1:
                p.data.normal_(0, 0.1)
    sd = {"rp." + k: v.detach().float().cpu() for k, v in rp.state_dict().items()}
    sd.update({"bb." + k: v.detach().float().cpu() for k, v in bb.state_dict().items()})
    if dt != torch.float32:
        cast_head(rp, dt, dt)
    for nq in (300, 910 + 3):
        ref = torch.rand(2, nq, 4) * 0.8 + 0.1
        wide = torch.rand(2, nq, 4, 4)                      # the (B, Q, levels, 4) tensor whose level-0 slice is the sine input
        wide[:, :, 0, :] = ref
        want_q = om.mlp(om.sine_embed_4(ref), sd, "rp.", 2)
        got_q = ops.ref_point_mlp(wide.to(DEV)[:, :, 0, :], rp)
        assert got_q.dtype == dt and rel_err(got_q.float().cpu(), want_q) < tol
        x = torch.randn(2, nq, 256)
        want_b = torch.sigmoid(om.mlp(x, sd, "bb.", 3) + om.inverse_sigmoid(ref))
        got_b = ops.box_head(x.to(DEV), ref.to(DEV), bb)
        assert rel_err(got_b.cpu(), want_b) < 5e-6


# ------------------------------------------------------------------------------------------------ split-fp16 ("HL8") kernels
@pytest.mark.parametrize("name", ["window14", "global16", "global64", "global_rect", "global84", "global128"])
def test_vit_attention_split_golden(name):
    """hipie_vit_attn_split on the reference-generated cases, fed the UNROUNDED fp32 qkv / tables as HL8 pairs: vs the fp32 oracle
    (the only 16-bit rounding left is the probability operand: 3e-4) and, through the projection, vs the reference golden."""
    import torch.nn.functional as F
    from hipie_amd import ops
    from hipie_amd.modeling.vit import resize_rel_pos
    g = Golden("vit_attn")
    c, sd, x = vit_attn_case(g, name)
    B, H, W, C = x.shape
    heads = c["heads"]
    hd = C // heads
    assert ops.vit_attn_split_ok((H, W), hd)
    scale = hd ** -0.5
    c1 = scale * ops.LOG2E
    qkv32 = _vit_qkv(c, sd, x)
    f = qkv32.clone()
    f[..., :C] *= c1
    th32, tw32 = resize_rel_pos(H, sd["rel_pos_h"]), resize_rel_pos(W, sd["rel_pos_w"])
    got = ops.vit_attn_split(ops.hl8_pack(f).to(DEV), ops.hl8_pack(th32 / scale).to(DEV), ops.hl8_pack(tw32 / scale).to(DEV), (H, W), heads)
    got = ops.hl8_unpack(got).cpu()
    q, k, v = qkv32.reshape(B, H * W, 3, heads, hd).permute(2, 0, 3, 1, 4).reshape(3, B * heads, H * W, hd).unbind(0)
    want = oo.vit_attention_core(q, k, v, th32, tw32, (H, W), scale)
    want = want.view(B, heads, H * W, hd).permute(0, 2, 1, 3).reshape(B, H * W, C)
    e1 = rel_err(got, want)
    out = F.linear(got, sd["proj.weight"], sd["proj.bias"]).view(B, H, W, C)
    e2 = rel_err(g.like(name + "_out", out), g[name + "_out"])
    print("vit_attn_split %s: vs fp32 oracle %.2e, vs golden (after proj) %.2e" % (name, e1, e2))
    assert e1 < 1.5e-4 and e2 < 2e-4


@pytest.mark.parametrize("B,gh,gw,heads,hd", [
    (1, 64, 64, 16, 80),         # the ViT-H global block at 1024^2
    (2, 40, 64, 8, 64),          # ViT-B/L head dim, fewer rows than columns, batch/head swizzle on
    (3, 14, 14, 5, 80),          # windows: 7-wave workgroups, odd batch*heads (no swizzle)
    (2, 7, 14, 2, 80),           # odd number of key rows with two rows per tile (ragged last tile)
    (1, 33, 50, 3, 64),
    (1, 84, 84, 2, 80),          # the 1344-pixel configuration: 96-slot tiles, bias_h recomputed per chunk of 16 key rows
    (2, 37, 70, 4, 64),          # wider than 64, token count not a multiple of the 256-query workgroup, chunk boundary inside
    (1, 70, 64, 1, 80),          # 64 wide, more than 64 rows: the 4-wave two-block variant
    (1, 64, 128, 2, 80),         # a 1024 x 2048 image: wider than 96 -> the TRANSPOSED walk (key tile = a column of the grid)
    (2, 40, 100, 2, 64),         # transposed, ragged everything
    (1, 90, 112, 1, 80)])        # transposed onto the 96-slot tiles (height in (64, 96])
def test_vit_attention_split_against_materialised_scores(B, gh, gw, heads, hd):
    """the reference's own formulation with the (N x N) score tensor materialised in fp64 on the device, random fp32 operands with
    LARGE logits (|q.k| up to ~25: a single-fp16 q or k would move the probabilities by 1e-2)."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(21 + gh + gw)
    N, C = gh * gw, heads * hd
    scale = hd ** -0.5
    c1 = scale * ops.LOG2E
    qkv = torch.randn(B, N, 3 * C, generator=gen) * 1.6
    th32, tw32 = torch.randn(2 * gh - 1, hd, generator=gen) * 0.2, torch.randn(2 * gw - 1, hd, generator=gen) * 0.2
    f = qkv.clone()
    f[..., :C] *= c1
    q, k, v = (t.to(DEV).double().view(B, heads, N, hd) for t in qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4))
    idx_h = torch.arange(gh, device=DEV)[:, None] - torch.arange(gh, device=DEV)[None, :] + gh - 1
    idx_w = torch.arange(gw, device=DEV)[:, None] - torch.arange(gw, device=DEV)[None, :] + gw - 1
    Rh, Rw = th32.to(DEV).double()[idx_h], tw32.to(DEV).double()[idx_w]
    rq = q.reshape(B, heads, gh, gw, hd)
    rel_h = torch.einsum("bmhwc,hkc->bmhwk", rq, Rh)
    rel_w = torch.einsum("bmhwc,wkc->bmhwk", rq, Rw)
    attn = (q * scale) @ k.transpose(-2, -1)
    attn = (attn.view(B, heads, gh, gw, gh, gw) + rel_h[..., :, None] + rel_w[..., None, :]).view(B, heads, N, N)
    want = (attn.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, N, C)
    got = ops.hl8_unpack(ops.vit_attn_split(ops.hl8_pack(f).to(DEV), ops.hl8_pack(th32 / scale).to(DEV), ops.hl8_pack(tw32 / scale).to(DEV),
                                            (gh, gw), heads))
    e = rel_err(got.cpu(), want.float().cpu())
    print("vit_attn_split %dx%d hd %d: %.2e" % (gh, gw, hd, e))
    assert e < 4e-4


def test_layernorm_hl8_outputs():
    """hipie_add_layernorm / _rows / _dec with HIPIE_HL8 outputs == the fp32 outputs split by hl8_pack (bit for bit)."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 9, 9, 160, generator=gen) * 3).to(DEV)
    d = torch.randn(2, 9, 9, 160, generator=gen).to(DEV)
    w, b = (1 + 0.1 * torch.randn(160, generator=gen)).to(DEV), (0.1 * torch.randn(160, generator=gen)).to(DEV)
    r32, n32 = ops.add_layernorm(x, d, w, b, 1e-6, torch.float32)
    r, n = ops.add_layernorm(x, d, w, b, 1e-6, "hl8")
    assert torch.equal(r, r32) and n.shape == (2, 9, 9, 320) and torch.equal(n, ops.hl8_pack(n32))
    # window row maps (zero rows for the padding) with the HL8 output
    from hipie_amd.modeling.vit import window_row_maps
    out_src, delta_row, nwin = window_row_maps(2, 9, 9, 7, x.device)
    _, nw32 = ops.add_layernorm(x, d, w, b, 1e-6, torch.float32, out_src=out_src)
    _, nw = ops.add_layernorm(x, d, w, b, 1e-6, "hl8", out_src=out_src)
    assert torch.equal(nw, ops.hl8_pack(nw32))
    # decoder form: fp32 + HL8 + (n + addend) as HL8
    xs, ds = x.view(-1, 160).contiguous(), d.view(-1, 160).contiguous()
    add32 = torch.randn(xs.shape, generator=gen).to(DEV)
    o32, n16, s16 = ops.add_layernorm_dec(xs, ds, w, b, 1e-5, "hl8", want16=True, addend=ops.hl8_pack(add32))
    assert torch.equal(n16, ops.hl8_pack(o32))
    assert torch.equal(s16, ops.hl8_pack(o32 + ops.hl8_unpack(ops.hl8_pack(add32))))


@pytest.mark.parametrize("nhwc", [False, True])
def test_group_norm_large_mean(nhwc):
    """|mean| >> std (a large convolution bias folded in as pre-bias): the shifted sums keep the variance; E[x^2] - mean^2 in fp32
    would lose it (mean 300, std 0.05: relative spacing of fp32 at 9e4 is 8e-3 >> var 2.5e-3)."""
    import torch.nn.functional as F
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 256, 24, 40, generator=gen) * 0.05
    pb = 300.0 + torch.randn(256, generator=gen) * 0.01
    w, b = 1 + 0.2 * torch.randn(256, generator=gen), 0.2 * torch.randn(256, generator=gen)
    xin = x.to(DEV)
    if nhwc:
        xin = xin.contiguous(memory_format=torch.channels_last)
    got = ops.group_norm(xin, 32, w.to(DEV), b.to(DEV), 1e-5, prebias=pb.to(DEV))
    want = F.group_norm(x.double() + pb.double().view(1, -1, 1, 1), 32, w.double(), b.double(), 1e-5).float()
    assert rel_err(got.float().cpu(), want) < 2e-4


@pytest.mark.parametrize("shape,odt", [((2, 256, 32, 40), torch.float32), ((1, 256, 64, 64), torch.float16), ((3, 64, 8, 8), torch.float32)])
def test_group_norm_channels_last_in_nchw_out(shape, odt):
    """channels_last = 2 (the mask_features head: maskdino_encoder.py:289-292 feeds the mask contraction pixel-fastest): the same values as
    the channels-last pass followed by `.contiguous()`, bit for bit, as a dense NCHW tensor; H*W % 64 != 0 keeps the input's layout."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(sum(shape))
    C = shape[1]
    x = (torch.randn(shape, generator=gen) * 2 + 0.5).to(DEV).contiguous(memory_format=torch.channels_last)
    w, b = (1 + 0.2 * torch.randn(C, generator=gen)).to(DEV), (0.2 * torch.randn(C, generator=gen)).to(DEV)
    pb = torch.randn(C, generator=gen).to(DEV)
    want = ops.group_norm(x, C // 8, w, b, 1e-5, relu=True, prebias=pb, out_dtype=odt)
    got = ops.group_norm(x, C // 8, w, b, 1e-5, relu=True, prebias=pb, out_dtype=odt, out_nchw=True)
    assert got.is_contiguous() and want.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got, want.contiguous())
    odd = x[:, :, :5, :7].contiguous(memory_format=torch.channels_last)            # 35 pixels: not a multiple of 64
    assert ops.group_norm(odd, C // 8, w, b, 1e-5, out_nchw=True).is_contiguous(memory_format=torch.channels_last)


def test_msda_fused_tiny_dense_heads():
    """dense value with M * D not a multiple of 8 (the reference's own unit shapes, ops/test.py: M = 2, D = 2) through the fused op."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(9)
    B, M, D, L, P, Lq = 1, 2, 2, 2, 2, 3
    shapes = torch.tensor([(6, 4), (3, 2)], dtype=torch.long)
    S = int(shapes.prod(1).sum())
    value = torch.rand(B, S, M, D, generator=gen)
    ref = torch.rand(B, Lq, L, 2, generator=gen)
    off = torch.randn(B, Lq, M, L, P, 2, generator=gen)
    logits = torch.randn(B, Lq, M, L * P, generator=gen)
    loc = ref[:, :, None, :, None, :] + off / torch.stack([shapes[:, 1], shapes[:, 0]], -1)[None, None, None, :, None, :].float()
    attn = torch.softmax(logits, -1).view(B, Lq, M, L, P)
    want = oo.ms_deform_attn_core(value, shapes, loc, attn)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    got = ops.msda_fused(value.to(DEV), shapes.to(DEV), lsi.to(DEV), ref.to(DEV), off.to(DEV), logits.to(DEV))
    assert rel_err(got.cpu(), want) < 2e-5


def test_msda_fused_value_stride_does_not_carry_over():
    """the value row stride of a strided call belongs to that call: a dense call after it gives, bit for bit, what it gave before it,
    and the strided call (value = a column block of a tensor twice as wide) what the dense one gives on a contiguous copy."""
    from hipie_amd import ops
    gen = torch.Generator().manual_seed(13)
    B, M, D, L, P, Lq = 1, 2, 32, 2, 2, 8
    shapes = torch.tensor([(4, 4), (2, 2)], dtype=torch.long)
    S = int(shapes.prod(1).sum())
    value = torch.rand(B, S, M, D, generator=gen).to(DEV)
    wide = torch.rand(B, S, 2 * M * D, generator=gen).to(DEV)
    block = wide[..., M * D:].unflatten(-1, (M, D))                  # row stride 2 * M * D
    assert not block.is_contiguous() and block.stride(1) == 2 * M * D
    ref = torch.rand(B, Lq, L, 2, generator=gen).to(DEV)
    off = torch.randn(B, Lq, M, L, P, 2, generator=gen).to(DEV)
    logits = torch.randn(B, Lq, M, L * P, generator=gen).to(DEV)
    ss, ls = shapes.to(DEV), _lsi(shapes).to(DEV)
    before = ops.msda_fused(value, ss, ls, ref, off, logits).clone()
    strided = ops.msda_fused(block, ss, ls, ref, off, logits)
    after = ops.msda_fused(value, ss, ls, ref, off, logits)
    assert torch.equal(after, before)
    assert torch.equal(strided, ops.msda_fused(block.contiguous(), ss, ls, ref, off, logits))
    assert not torch.equal(strided, before)                          # different values: a carried-over stride would show


def test_hl8_saturates_instead_of_nan():
    """values beyond the fp16 range: hi saturates at 65504 and lo stays finite (an inf hi would make lo = x - inf a NaN)."""
    from hipie_amd import ops
    x = torch.tensor([[1e6, -3e5, 65504.0, 70000.0, 1.0, -2.0, 0.0, 123.456]], device=DEV)
    h = ops.to_hl8(x)
    assert torch.isfinite(h.float()).all()
    back = ops.hl8_unpack(h)[0].cpu()
    assert back[0] == 65504.0 and back[1] == -65504.0 and back[3] == 65504.0 and abs(float(back[7]) - 123.456) < 1e-4
    assert torch.equal(h, ops.hl8_pack(x))


# --------------------------------------------------------------------------- top-k
@pytest.mark.gpu
@pytest.mark.parametrize("rows,n,k", [(8, 21760, 900), (8, 21760, 300), (2, 340, 20), (1, 72000, 100), (3, 1000, 1000), (2, 1025, 1024),
                                      (1, 5, 5), (4, 37485, 900)])
def test_topk_matches_torch(rows, n, k):
    """hipie_topk vs torch.topk (CPU): identical values, identical indices (distinct scores), descending order."""
    from hipie_amd import ops
    g = torch.Generator().manual_seed(rows * 7 + n + k)
    x = torch.randn(rows, n, generator=g) * 3.0
    x[0, : min(n, 7)] = torch.tensor([float("inf"), -float("inf"), 0.0, -0.0, 1e-38, -1e-38, 65504.0])[: min(n, 7)]
    want_v, want_i = torch.topk(x, k, dim=1)
    idx, val = ops.topk(x.cuda(), k, want_values=True)
    torch.cuda.synchronize()
    assert torch.equal(val.cpu(), want_v)
    distinct = torch.ones(rows, k, dtype=torch.bool)
    distinct[:, 1:] &= want_v[:, 1:] != want_v[:, :-1]
    distinct[:, :-1] &= want_v[:, 1:] != want_v[:, :-1]
    assert torch.equal(idx.cpu()[distinct], want_i[distinct])
    assert torch.equal(torch.gather(x, 1, idx.cpu()), want_v)


@pytest.mark.gpu
def test_topk_ties_take_the_lowest_indices_in_order():
    from hipie_amd import ops
    x = torch.zeros(2, 5000)
    x[0, 100:110] = 1.0                      # 10 above, the remaining 20 winners come from the tie at 0 -> indices 0..19
    x[1] = 2.5                               # a constant row: indices 0..k-1
    idx = ops.topk(x.cuda(), 30).cpu()
    assert idx[0].tolist() == list(range(100, 110)) + list(range(20))
    assert idx[1].tolist() == list(range(30))
    # a strided view (row stride > n) and NaN as the largest value, as torch orders it
    y = torch.randn(4, 3000, generator=torch.Generator().manual_seed(77))
    y[2, 17] = float("nan")
    yv = y.cuda()[:, :2000]
    got = ops.topk(yv, 50).cpu()
    want = torch.topk(y[:, :2000], 50, dim=1)[1]
    assert torch.equal(got, want)
    # canonical keys: a NEGATIVE-signed NaN (0 * -inf) is still the largest value; -0.0 ties with +0.0 and the tie goes to the lower index
    z = -torch.rand(2, 1500, generator=torch.Generator().manual_seed(78)) - 1.0
    z[0, 700] = float("nan")
    z[0, 700] = -z[0, 700].abs() if False else torch.tensor(float("nan")).copysign(torch.tensor(-1.0))
    z[1, 40], z[1, 20], z[1, 30] = 0.0, -0.0, 0.0
    got = ops.topk(z.cuda(), 4).cpu()
    assert got[0, 0].item() == 700
    assert got[1, :3].tolist() == [20, 30, 40]


@pytest.mark.gpu
def test_topk_replays_in_a_hip_graph():
    """the property torch.topk lacks here: 200 replays of a captured selection on changing scores."""
    from hipie_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(8, 21760, device="cuda", generator=gen)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.topk(x, 900)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            idx = ops.topk(x, 900)
    for it in range(200):
        x.copy_(torch.randn(8, 21760, device="cuda", generator=gen))
        gr.replay()
        if it % 50 == 49:
            torch.cuda.synchronize()
            want_v = torch.topk(x.cpu(), 900, dim=1)[0]            # values, not indices: equal scores may be ordered differently
            assert torch.equal(torch.gather(x.cpu(), 1, idx.cpu()), want_v)
    with pytest.raises(RuntimeError):
        ops.topk(x, 1025)


# --------------------------------------------------------------------------- MSDA backward (the plugin's second entry point)
def _msda_bwd_case(case):
    g = Golden("msda_bwd")
    tag, D = [(t, d) for n, t, d in g.meta["cases"] if n == case][0]
    return g, _synth.msda_bwd_inputs(tag, D)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["recipe30", "recipe32", "recipe64", "recipe71", "recipe1025", "hot"])
def test_msda_backward_golden(case):
    """hipie_msda_backward vs the gradients of the reference's own differentiable formulation (tests/golden/msda_bwd.npz: F.grid_sample +
    autograd in double): the f64 instantiation to 1e-11, the f32 one to fp32 rounding.  Channel counts of ops/test.py:97-98."""
    from hipie_amd import ops
    g, (value, shapes, loc, attn, gout) = _msda_bwd_case(case)
    sh, ls = shapes.to(DEV), _lsi(shapes).to(DEV)
    gv, gl, ga = ops.ms_deform_attn_backward(value.to(DEV), sh, ls, loc.to(DEV), attn.to(DEV), gout.to(DEV), 2)
    assert gv.dtype == torch.float64
    assert rel_err(gv.cpu(), g[case + "_gvalue"]) < 1e-11
    assert rel_err(gl.cpu(), g[case + "_gloc"]) < 1e-10
    assert rel_err(ga.cpu(), g[case + "_gattn"]) < 1e-11
    f = torch.float32
    gv, gl, ga = ops.ms_deform_attn_backward(value.to(f).to(DEV), sh, ls, loc.to(f).to(DEV), attn.to(f).to(DEV), gout.to(f).to(DEV), 2)
    assert gv.dtype == f
    # f32: the inputs themselves are rounded (a location moves by 2^-24 * size pixels), the sums over D run in fp32
    assert rel_err(gv.cpu(), g[case + "_gvalue"]) < 2e-6
    assert rel_err(gl.cpu(), g[case + "_gloc"]) < 2e-5
    assert rel_err(ga.cpu(), g[case + "_gattn"]) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [30, 32, 64, 71])
def test_msda_gradcheck_reference_recipe(channels):
    """ops/test.py:69-85 check_gradient_numerical: torch.autograd.gradcheck of MSDeformAttnFunction in double on the recipe's shapes --
    here the Function of hipie_amd.msda_shim (the reference's own Function runs on the same two entry points via install())."""
    from torch.autograd import gradcheck
    from hipie_amd.msda_shim import MSDeformAttnFunction
    N, M, Lq, L, P = 1, 2, 2, 2, 2
    shapes = torch.as_tensor([(6, 4), (3, 2)], dtype=torch.long, device=DEV)
    S = int(shapes.prod(1).sum())
    torch.manual_seed(3)
    value = (torch.rand(N, S, M, channels, device=DEV) * 0.01).double().requires_grad_(True)
    loc = torch.rand(N, Lq, M, L, P, 2, device=DEV).double().requires_grad_(True)
    attn = torch.rand(N, Lq, M, L, P, device=DEV) + 1e-5
    attn = (attn / attn.sum(-1, keepdim=True).sum(-2, keepdim=True)).double().requires_grad_(True)
    with torch.enable_grad():
        assert gradcheck(MSDeformAttnFunction.apply, (value, shapes, _lsi(shapes), loc, attn, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [2048, 3096])
def test_msda_backward_wide_channels_vs_oracle_autograd(channels):
    """the two largest channel counts of ops/test.py (a numerical gradcheck over 1.8e5 inputs would take minutes): analytic gradients vs
    autograd through the oracle's formulation, double."""
    from hipie_amd import ops
    value, shapes, loc, attn, gout = _synth.msda_bwd_inputs("recipe", channels)
    with torch.enable_grad():
        v, l, a = value.clone().requires_grad_(True), loc.clone().requires_grad_(True), attn.clone().requires_grad_(True)
        want = torch.autograd.grad(oo.ms_deform_attn_core(v, shapes, l, a), (v, l, a), gout)
    got = ops.ms_deform_attn_backward(value.to(DEV), shapes.to(DEV), _lsi(shapes).to(DEV), loc.to(DEV), attn.to(DEV), gout.to(DEV), 2)
    for w, x in zip(want, got):
        assert rel_err(x.cpu(), w) < 1e-10


@pytest.mark.gpu
def test_msda_backward_through_the_reference_module_name_and_contended_pixels():
    """(a) MultiScaleDeformableAttention.ms_deform_attn_backward as the reference's MSDeformAttnFunction.backward calls it (positional
    arguments, a 3-tuple back); (b) every query samples the SAME point: all grad_value contributions meet on four pixels (atomics),
    and the training geometry Lq = 21760 x 8 heads finishes; (c) nothing requires_grad-related leaks into the inference op."""
    import sys
    from hipie_amd import msda_shim, ops
    msda_shim.install()
    import MultiScaleDeformableAttention as MSDA
    try:
        B, M, D, L, P, Lq = 1, 8, 32, 4, 4, 21760
        shapes = torch.as_tensor([(128, 128), (64, 64), (32, 32), (16, 16)], dtype=torch.long, device=DEV)
        S = int(shapes.prod(1).sum())
        g = torch.Generator(device="cuda").manual_seed(5)
        # double: 87040 equal addends meet on each of four pixels per level -- in fp32 that running sum rounds every add the same way
        # (5437.3 instead of 5440, as any fp32 accumulation in arrival order would); the f64 atomics are exact to 1e-12
        value = torch.randn(B, S, M, D, device=DEV, generator=g, dtype=torch.float64)
        loc = torch.full((B, Lq, M, L, P, 2), 0.3, device=DEV, dtype=torch.float64)
        attn = torch.full((B, Lq, M, L, P), 1.0 / (L * P), device=DEV, dtype=torch.float64)
        gout = torch.ones(B, Lq, M * D, device=DEV, dtype=torch.float64)
        res = MSDA.ms_deform_attn_backward(value, shapes, _lsi(shapes), loc, attn, gout, 64)
        assert isinstance(res, tuple) and len(res) == 3
        gv, gl, ga = res
        torch.cuda.synchronize()
        # each level: the bilinear weights of the one sampled point sum to 1 -> sum of grad_value over the level = Lq * P * A per (head, channel)
        start = 0
        for (H, W) in shapes.tolist():
            tot = gv[0, start:start + H * W].sum(0)
            assert torch.allclose(tot, torch.full_like(tot, Lq * P / (L * P)), rtol=1e-10)
            assert int((gv[0, start:start + H * W].abs().sum((1, 2)) > 0).sum()) <= 4
            start += H * W
        # all queries are identical: so are their location / weight gradients
        assert torch.equal(gl[0, 0], gl[0, -1]) and torch.equal(ga[0, 0], ga[0, -1])
        fwd = ops.ms_deform_attn_forward(value, shapes, _lsi(shapes), loc, attn, 64)
        assert rel_err(ga.sum((3, 4)).reshape(B, Lq, M).cpu() * 1.0, (fwd.view(B, Lq, M, D).sum(-1) * (L * P)).cpu()) < 1e-10
    finally:
        sys.modules.pop("MultiScaleDeformableAttention")


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["four_levels", "three_levels", "gapped_layout", "few_queries"])
def test_msda_backward_d32_geometries(geom):
    """hipie_msda_backward at the production head width (D = 32, fp32) against autograd through the oracle's formulation in double:
    pyramids of 4 and 3 levels with sampling points outside the maps, level_start with gaps between the levels (the gap rows of
    grad_value stay zero), and fewer queries than one workgroup holds.  (The same cases qualified the LDS-accumulating variant of
    profiles/r05_msda_bwd_lds_study.txt, which was correct and slower.)"""
    from hipie_amd import ops
    M, D, P = 8, 32, 4
    shapes = {"four_levels": [(40, 40), (20, 20), (10, 10), (5, 5)], "three_levels": [(60, 80), (30, 40), (15, 20)],
              "gapped_layout": [(16, 16), (8, 8), (4, 4)], "few_queries": [(24, 24), (12, 12), (6, 6), (3, 3)]}[geom]
    B, Lq = (2, 7) if geom == "few_queries" else (2, 3001)
    L = len(shapes)
    sh = torch.as_tensor(shapes, dtype=torch.long)
    ls = _lsi(sh)
    S = int(sh.prod(1).sum())
    if geom == "gapped_layout":
        ls = ls + torch.arange(L) * 5                   # 5 unused rows between the levels
        S += 5 * L
    g = torch.Generator().manual_seed(11)
    value = torch.randn(B, S, M, D, generator=g, dtype=torch.float64)
    loc = torch.rand(B, Lq, M, L, P, 2, generator=g, dtype=torch.float64) * 1.2 - 0.1        # some points outside the maps
    attn = torch.softmax(torch.randn(B, Lq, M, L * P, generator=g, dtype=torch.float64), -1).view(B, Lq, M, L, P)
    gout = torch.randn(B, Lq, M * D, generator=g, dtype=torch.float64)
    # the oracle's formulation works on the packed layout: pick the levels' rows out of the (possibly gapped) value
    rows = torch.cat([torch.arange(int(ls[l]), int(ls[l]) + shapes[l][0] * shapes[l][1]) for l in range(L)])
    with torch.enable_grad():
        v, l_, a = value.clone().requires_grad_(True), loc.clone().requires_grad_(True), attn.clone().requires_grad_(True)
        want = torch.autograd.grad(oo.ms_deform_attn_core(v[:, rows], sh, l_, a), (v, l_, a), gout)
    f = torch.float32
    got = ops.ms_deform_attn_backward(value.to(f).to(DEV), sh.to(DEV), ls.to(DEV), loc.to(f).to(DEV), attn.to(f).to(DEV), gout.to(f).to(DEV), 64)
    for w, x, tol in zip(want, got, (3e-6, 2e-5, 2e-5)):
        assert rel_err(x.cpu(), w) < tol
    if geom == "gapped_layout":
        gap = torch.ones(S, dtype=torch.bool)
        gap[rows] = False
        assert float(got[0][:, gap.to(DEV)].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["heads5", "heads16_batch3", "tall_image", "all_outside", "one_pixel_hot"])
def test_msda_backward_gather_form_against_the_atomic_kernel_and_autograd(case):
    """hipie_msda_backward_ws (round 6: corners binned by destination in LDS counters, every (pixel, head) row of grad_value summed in registers
    and stored once) against hipie_msda_backward (floating-point atomics) on the same inputs, and against autograd through the oracle's
    formulation in double.  Cases: head counts that do not / do follow the one-head-per-XCD group map (5; 16 with 3 images: 48 planes -> 5 query
    slices), more pixel rows per image than the LDS of a CU holds (S = 41650 > 40960: the entry runs the atomic kernel and says nothing), every
    sampling point outside the maps (all gradients zero, grad_value still fully written), every query sampling the same pixel (one
    destination list of B*Lq*L*P... records per head)."""
    from hipie_amd import _lib, ops
    lib = _lib.load()
    M, D, P = {"heads5": (5, 32, 4), "heads16_batch3": (16, 32, 2)}.get(case, (8, 32, 4))
    shapes = {"tall_image": [(280, 112), (140, 56), (70, 28), (35, 14)]}.get(case, [(24, 32), (12, 16), (6, 8)])
    B, Lq = {"heads16_batch3": (3, 517), "tall_image": (1, 700)}.get(case, (2, 1203))
    L = len(shapes)
    sh = torch.as_tensor(shapes, dtype=torch.long)
    ls = _lsi(sh)
    S = int(sh.prod(1).sum())
    g = torch.Generator().manual_seed(len(case))
    value = torch.randn(B, S, M, D, generator=g, dtype=torch.float64)
    # sampling points from 1.5 pixels outside the maps to 1.5 pixels outside on the other side, kept 0.05 pixel away from the pixel
    # boundaries (where grad_sampling_loc jumps and an fp32 rounding of the location would pick the other side)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)[None, None, None, :, None, :]
    raw = torch.rand(B, Lq, M, L, P, 2, generator=g, dtype=torch.float64) * (wh + 3) - 2.0
    if case == "all_outside":
        raw = raw + 2 * wh
    if case == "one_pixel_hot":
        raw = torch.floor(wh / 2) + torch.rand(raw.shape, generator=g, dtype=torch.float64)
    pix = torch.floor(raw) + 0.05 + 0.9 * (raw - torch.floor(raw))
    loc = (pix + 0.5) / wh
    attn = torch.softmax(torch.randn(B, Lq, M, L * P, generator=g, dtype=torch.float64), -1).view(B, Lq, M, L, P)
    gout = torch.randn(B, Lq, M * D, generator=g, dtype=torch.float64)
    with torch.enable_grad():
        v, l_, a = value.clone().requires_grad_(True), loc.clone().requires_grad_(True), attn.clone().requires_grad_(True)
        want = torch.autograd.grad(oo.ms_deform_attn_core(v, sh, l_, a), (v, l_, a), gout)
    f = torch.float32
    dv, dsh, dls, dloc, dattn, dgo = (value.to(f).to(DEV), sh.to(DEV), ls.to(DEV), loc.to(f).to(DEV), attn.to(f).to(DEV), gout.to(f).to(DEV))
    need = int(lib.hipie_msda_backward_workspace(B, S, M, L, Lq, P))
    assert need >= B * Lq * M * L * P * 4 * 8
    got = ops.ms_deform_attn_backward(dv, dsh, dls, dloc, dattn, dgo, 64)
    ref = [torch.full_like(dv, float("nan")), torch.empty_like(dloc), torch.empty_like(dattn)]
    rc = lib.hipie_msda_backward(dv.data_ptr(), dsh.data_ptr(), dls.data_ptr(), dloc.data_ptr(), dattn.data_ptr(), dgo.data_ptr(), ref[0].data_ptr(),
                                 ref[1].data_ptr(), ref[2].data_ptr(), B, S, M, D, L, Lq, P, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    # fp32 locations on a 280-pixel axis carry 280 * 2^-24 = 1.7e-5 pixel of rounding into the bilinear weights
    tols = (3e-5, 2e-4, 2e-4) if case == "tall_image" else (3e-6, 2e-5, 2e-5)
    for w, x, r, tol in zip(want, got, ref, tols):
        scale = float(w.abs().max())
        if scale == 0.0:
            assert float(x.abs().max()) == 0.0 and float(r.abs().max()) == 0.0
        else:
            assert rel_err(x.cpu(), w) < tol and rel_err(r.cpu(), w) < tol
            assert float((x - r).abs().max()) <= 2e-5 * scale
    # a workspace that is too small is refused with the size that is needed (the atomic-only forms ignore the workspace)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    out = [torch.empty_like(dv), torch.empty_like(dloc), torch.empty_like(dattn)]
    rc = lib.hipie_msda_backward_ws(dv.data_ptr(), dsh.data_ptr(), dls.data_ptr(), dloc.data_ptr(), dattn.data_ptr(), dgo.data_ptr(), out[0].data_ptr(),
                                    out[1].data_ptr(), out[2].data_ptr(), B, S, M, D, L, Lq, P, 0, ws.data_ptr(), 1024, torch.cuda.current_stream().cuda_stream)
    if case == "tall_image":
        assert rc == 0 and S > 40960
        torch.cuda.synchronize()
        assert rel_err(out[0].cpu(), want[0]) < tols[0]
    else:
        assert rc != 0 and b"needed" in lib.hipie_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("B,Q,C,H,W,bias", [(2, 300, 256, 64, 64, True), (1, 37, 256, 25, 38, False), (2, 1100, 256, 32, 32, True), (1, 5, 64, 3, 7, False)])
def test_mask_einsum_backward_vs_autograd(B, Q, C, H, W, bias):
    """row f-4: the backward of the mask contraction (hipie_amd.training.functions.MaskEinsumFunction: forward hipie_mask_einsum, backward
    two hipie_gemm_batched products) against torch.autograd of the einsum in double -- the formulation of the oracle's mask head
    (oracle/model.py: einsum("bqc,bchw->bqhw")).  Ragged H x W (950 pixels: K padded to 960, N to 952), Q not a multiple of 32."""
    from hipie_amd.training.functions import mask_einsum
    g = torch.Generator().manual_seed(B * 1000 + Q)
    e = torch.randn(B, Q, C, generator=g, dtype=torch.float64)
    f = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    rb = torch.randn(B, Q, generator=g, dtype=torch.float64) if bias else None
    go = torch.randn(B, Q, H, W, generator=g, dtype=torch.float64)
    with torch.enable_grad():
        leaves = [t.clone().requires_grad_(True) for t in (e, f)] + ([rb.clone().requires_grad_(True)] if bias else [])
        ref = torch.einsum("bqc,bchw->bqhw", leaves[0], leaves[1])
        if bias:
            ref = ref + leaves[2][:, :, None, None]
        want = torch.autograd.grad(ref, leaves, go)
        dl = [t.float().to(DEV).requires_grad_(True) for t in (e, f)] + ([rb.float().to(DEV).requires_grad_(True)] if bias else [])
        out = mask_einsum(dl[0], dl[1], dl[2] if bias else None)
        got = torch.autograd.grad(out, dl, go.float().to(DEV))
    assert rel_err(out.detach().cpu(), ref.detach()) < 3e-5          # the forward's own bound (three bf16 products)
    for w, x in zip(want, got):
        assert x.dtype == torch.float32 and rel_err(x.cpu(), w) < 3e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,Q,H,W,up", [(2, 37, 32, 32, 2), (1, 40, 9, 6, 2), (1, 2100, 2, 2, 2), (2, 5, 9, 6, 2), (1, 11, 16, 24, 1), (3, 1, 1, 2, 2),
                                        (1, 300, 40, 56, 2)])
def test_dynamic_mask_backward_vs_oracle_autograd(B, Q, H, W, up):
    """row f-4: hipie_dynamic_mask_backward (through hipie_amd.training.functions.DynamicMaskFunction) against torch.autograd of the
    oracle's dynamic_mask in double (oracle/ops.py: relative coordinates, three per-instance 1x1 layers, aligned_bilinear).  Ragged
    pixel counts (54, 2 pixels: partly dead workgroups; the forward needs an even W), one instance, instance chunks of 1 and of 3 instances, up = 1.
    The last case evaluates 10.7 M ReLUs: a handful of pre-activations within fp32 rounding of 0 take the other branch than in double
    and move the few gradient elements they feed by one (instance, pixel) term -- that case is held to the bound on 99 % of the
    elements and to 5e-2 everywhere (a wrong kernel is off everywhere); the small cases are held to it on every element."""
    from hipie_amd.training.functions import dynamic_mask
    g = torch.Generator().manual_seed(H * 100 + Q)
    feats = torch.randn(B, 8, H, W, generator=g, dtype=torch.float64)
    refs = torch.rand(B * Q, 2, generator=g, dtype=torch.float64) * torch.tensor([8.0 * W, 8.0 * H], dtype=torch.float64)
    params = torch.randn(B * Q, 169, generator=g, dtype=torch.float64) * 0.3
    params[:, :80].view(-1, 8, 10)[:, :, :2] *= 0.02                  # coordinate weights: inputs of ~100 pixels
    go = torch.randn(B * Q, up * H, up * W, generator=g, dtype=torch.float64)
    with torch.enable_grad():
        leaves = [t.clone().requires_grad_(True) for t in (feats, refs, params)]
        ref = oo.dynamic_mask(leaves[0], leaves[1][None], leaves[2][None], [Q] * B, stride=8, up=up)[0]
        want = torch.autograd.grad(ref, leaves, go)
        dl = [t.float().to(DEV).requires_grad_(True) for t in (feats, refs, params)]
        out = dynamic_mask(dl[0], dl[1], dl[2], Q, 8, up)
        got = torch.autograd.grad(out, dl, go.float().to(DEV))
    assert rel_err(out.detach().cpu(), ref.detach()) < 1e-5
    big = B * Q * H * W > 500000
    for w, x, name in zip(want, got, ("feats", "refs", "params")):
        assert x.dtype == torch.float32 and x.shape == w.shape
        err = (x.cpu().double() - w).abs() / w.abs().max()
        if big:
            assert float(err.flatten().kthvalue(max(1, int(0.99 * err.numel()))).values) < 2e-5, name
            assert float(err.max()) < 5e-2, name
        else:
            assert float(err.max()) < 2e-5, name


@pytest.mark.gpu
@pytest.mark.parametrize("Nk,L", [(21760, 194), (1000, 37), (333, 7)])
def test_flash_attn_reads_keys_from_hl8_hi_halves(Nk, L):
    """HIPIE_K_HL8_HI: the text -> image direction of the fusion takes its keys from the hi halves of the HL8 visual projection in place
    (8-element chunks 16 elements apart) -- bit-identical to the same call on a strided copy of those halves, full and ragged last tile."""
    from hipie_amd import ops
    B, H, hd = 2, 8, 256
    g = torch.Generator().manual_seed(Nk)
    x = (torch.randn(B, Nk, H * hd, generator=g) * 0.05).to(DEV)
    hl8 = ops.to_hl8(x)
    hi = hl8.view(B * Nk, H * hd // 8, 2, 8)[:, :, 0, :].reshape(B, Nk, H, hd)
    assert torch.equal(hi, x.half().view(B, Nk, H, hd))
    q = (torch.randn(B, L, H, hd, generator=g) * 0.5).half().to(DEV)
    v = torch.randn(B, Nk, H, hd, generator=g).half().to(DEV)
    a = ops.flash_attn(q, hi, v, 1.0, clamp=50000.0, out_f32=True)
    b = ops.flash_attn(q, hl8, v, 1.0, clamp=50000.0, out_f32=True, k_hl8=True)
    assert torch.equal(a, b)
    ref = torch.softmax(torch.einsum("blhd,bnhd->bhln", q.float(), hi.float()), -1)
    ref = torch.einsum("bhln,bnhd->blhd", ref, v.float()).reshape(B, L, H * hd)
    assert rel_err(b.cpu(), ref.cpu()) < 2e-3


# --------------------------------------------------------------------------- exact fp32 small attention
# (workload-like shapes, one whole-tensor metric; the launch lines, tile edges, masked prefixes and the online-softmax rescale of these two
# kernels are walked per 32-query block against float64 in tests/test_gpu_small_attn.py)
@pytest.mark.gpu
@pytest.mark.parametrize("B,Nq,Nk,H,hd,masked", [(2, 194, 194, 12, 64, True), (3, 910, 910, 8, 32, False), (2, 300, 300, 8, 32, False),
                                                 (1, 5, 37, 2, 64, True), (2, 512, 512, 12, 64, True)])
@pytest.mark.parametrize("which", ["attn_f32", "attn_split"])
def test_attn_f32_exact(B, Nq, Nk, H, hd, masked, which):
    """hipie_attn_f32 (exact fp32 FMA chains) and hipie_attn_split (the same attention on the matrix pipe from fp16 PAIRS, what the split
    policy runs for BERT / the decoders' query self-attention) vs softmax attention in double; q / k / v are column blocks of ONE projection
    output, large logits (|s| up to ~30), a padded tail and one fully masked sequence.  Same bound for both."""
    from hipie_amd import ops
    attn = getattr(ops, which)
    g = torch.Generator().manual_seed(B * 1000 + Nq + hd)
    C = H * hd
    qkv = torch.randn(B, Nk, 3 * C, generator=g) * 1.5
    q, k, v = (qkv[:, :, i * C:(i + 1) * C].view(B, Nk, H, hd) for i in range(3))
    q = q[:, :Nq]
    mask = None
    if masked:
        mask = torch.ones(B, Nk, dtype=torch.bool)
        mask[0, Nk - Nk // 3:] = False
        if B > 1:
            mask[1, 1::2] = False
    scale = hd ** -0.5
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    want = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v.double()).reshape(B, Nq, C)
    dev = qkv.to(DEV)
    qd, kd, vd = (dev[:, :, i * C:(i + 1) * C].view(B, Nk, H, hd) for i in range(3))
    got = attn(qd[:, :Nq], kd, vd, scale, key_mask=None if mask is None else mask.to(DEV))
    e = rel_err(got.cpu(), want.float())
    print("%s %dx%d hd %d: %.2e" % (which, Nq, Nk, hd, e))
    # fp32 scores of magnitude ~40 (log2 domain) carry 4e-6 of rounding into the exponent: the same bound as any fp32 evaluation
    assert got.dtype == torch.float32 and e < 1e-5
    if masked:                                     # a sequence with every key masked: zeros, not NaN
        m2 = mask.clone()
        m2[0] = False
        got2 = attn(qd[:, :Nq], kd, vd, scale, key_mask=m2.to(DEV))
        assert torch.isfinite(got2).all() and float(got2[0].abs().max()) == 0.0


# --------------------------------------------------------------------------- split image -> text fusion attention
@pytest.mark.gpu
@pytest.mark.parametrize("B,Nv,L,heads,hd", [(2, 1000, 30, 8, 256), (1, 21760, 194, 8, 256), (2, 300, 257, 2, 64)])
def test_bi_i2t_split(B, Nv, L, heads, hd):
    """ops.bi_i2t_split (batched split GEMM -> masked softmax -> batched split GEMM) vs the reference formulation of the image -> text
    direction (fuse_helper.py:77-121: clamp, mask as -9e15 / +1, softmax over the text tokens, bmm with the text values) in double;
    logits of magnitude ~20 (a single-fp16 q or k would move the probabilities by 1e-2), ragged text lengths."""
    from hipie_amd import ops
    g = torch.Generator().manual_seed(L + Nv)
    E = heads * hd
    q = torch.randn(B, Nv, E, generator=g) * 0.9
    k = torch.randn(B, L, E, generator=g) * 0.9
    vl = torch.randn(B, L, E, generator=g)
    mask = torch.ones(B, L, dtype=torch.bool)
    mask[0, L - L // 4:] = False
    qd, kd, vd = (t.double().view(B, -1, heads, hd) for t in (q, k, vl))
    w = torch.einsum("bnhd,blhd->bhnl", qd, kd).clamp(-50000, 50000)
    am = mask.long()[:, None, None, :].expand(B, 1, Nv, L).clone()
    am = am.masked_fill(am == 0, int(-9e15))
    want = torch.einsum("bhnl,blhd->bnhd", (w + am).softmax(-1), vd).reshape(B, Nv, E)
    got = ops.bi_i2t_split(ops.to_hl8(q.to(DEV)), k.to(DEV), vl.to(DEV), mask.to(DEV), heads)
    e = rel_err(got.cpu(), want.float())
    print("bi_i2t_split Nv=%d L=%d: %.2e" % (Nv, L, e))
    assert got.shape == (B, Nv, E) and e < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nv,L,heads,hd,C", [(2, 1000, 30, 8, 256, 256), (1, 21760, 194, 8, 256, 256), (2, 300, 256, 2, 64, 256)])
def test_bi_i2t_folded(B, Nv, L, heads, hd, C):
    """ops.bi_i2t_folded -- the image -> text direction with the visual-side projections folded into the text side (one batched split GEMM with
    the masked softmax and the per-column logit bias in its epilogue, one batched GEMM with bias + residual) -- against the reference order of
    operations in double (fuse_helper.py:62-139: v_proj * scale, q . k, clamp, -9e15 mask, softmax over the text tokens, bmm with the text
    values, out_v_proj); logits of magnitude ~20, a partly masked text, the residual in the epilogue."""
    from hipie_amd import ops
    g = torch.Generator().manual_seed(L + Nv)
    E = heads * hd
    x = torch.randn(B, Nv, C, generator=g)
    wq = torch.randn(E, C, generator=g) * (0.9 / C ** 0.5)
    bq = torch.randn(E, generator=g) * 0.3
    k = torch.randn(B, L, E, generator=g) * 0.9
    vl = torch.randn(B, L, E, generator=g)
    wo = torch.randn(C, E, generator=g) * E ** -0.5
    bo = torch.randn(C, generator=g)
    resid = torch.randn(B, Nv, C, generator=g)
    mask = torch.ones(B, L, dtype=torch.bool)
    mask[0, L - L // 4:] = False
    xd, kd, vd = x.double(), k.double().view(B, L, heads, hd), vl.double().view(B, L, heads, hd)
    qd = (xd @ wq.double().t() + bq.double()).view(B, Nv, heads, hd)
    w = torch.einsum("bnhd,blhd->bhnl", qd, kd).clamp(-50000, 50000)
    am = mask.long()[:, None, None, :].expand(B, 1, Nv, L).clone()
    am = am.masked_fill(am == 0, int(-9e15))
    attn = torch.einsum("bhnl,blhd->bnhd", (w + am).softmax(-1), vd).reshape(B, Nv, E)
    want = attn @ wo.double().t() + bo.double() + resid.double()
    kh = k.to(DEV).view(B, L, heads, hd).permute(0, 2, 1, 3)
    M = torch.matmul(kh, wq.to(DEV).view(1, heads, hd, C))
    cb = (kh * bq.to(DEV).view(1, heads, 1, hd)).sum(-1)
    got = ops.bi_i2t_folded(ops.to_hl8(x.to(DEV)), M.contiguous(), cb.contiguous(), vl.to(DEV), mask.to(DEV), heads, wo.to(DEV), bo.to(DEV),
                            resid=resid.to(DEV))
    e = rel_err(got.cpu(), want.float())
    print("bi_i2t_folded Nv=%d L=%d: %.2e" % (Nv, L, e))
    assert got.shape == (B, Nv, C) and e < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("L,n_keys", [(40, None), (194, None), (300, 150)])
def test_bi_attention_folded_matches_the_projected_form(L, n_keys):
    """BiMultiHeadAttention in the split policy: the folded form (no visual projection of width embed_dim: transformer._forward_folded) against
    the projected form (q / values projections of every visual token, ops.bi_i2t_split + the flash kernel) on the same module: the visual update
    at fp32 class (2e-5), the text update at the fp16-operand class of that direction (2e-3); a text with trailing masked tokens and n_keys."""
    import hipie_amd.modeling.transformer as T
    from hipie_amd import ops
    torch.manual_seed(L)
    m = T.BiMultiHeadAttention(256, 768, 2048, 8, torch.float16).cuda()
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.03)
    T.set_split(m)
    B, Nv = 2, 3000
    v = torch.randn(B, Nv, 256, device="cuda")
    l = torch.randn(B, L, 768, device="cuda")
    mask = torch.ones(B, L, dtype=torch.uint8, device="cuda")
    if n_keys:
        mask[:, n_keys:] = 0
    mask[1, (n_keys or L) - 7:] = 0
    gamma = torch.rand(256, device="cuda") + 0.5
    assert ops.bi_i2t_folded_ok(v, L, n_keys)
    fv, fl = m(v, l, attention_mask_l=mask, gamma_v=gamma, n_keys=n_keys, resid_v=v)
    assert m.resid_fused
    keep = ops.bi_i2t_folded_ok
    ops.bi_i2t_folded_ok = lambda *a: False
    try:
        pv, pl = m(v, l, attention_mask_l=mask, gamma_v=gamma, n_keys=n_keys, resid_v=v)
    finally:
        ops.bi_i2t_folded_ok = keep
    ev, el = rel_err((fv - v).cpu(), (pv - v).cpu()), rel_err(fl.cpu(), pl.cpu())
    print("folded vs projected, L=%d: visual update %.2e, text update %.2e" % (L, ev, el))
    assert ev < 2e-5 and el < 2e-3
