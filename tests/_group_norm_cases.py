"""shared by test_group_norm_bwd_cpu.py and test_gpu_group_norm_bwd.py: inputs of the training GroupNorm (+ ReLU) node, its backward in
float64 as csrc/groupnorm_bwd.hip states it (the ReLU mask is an INPUT: the GPU tests take it from the kernel forward's own y > 0), torch's
own graph, and the smallest parameter set that runs the 4 + 7 conv + GN blocks of net.backbone_and_projections / net.maskdino_pixel_decoder.
Everything is drawn in fp32, so a float64 copy holds fp32-representable values."""
import torch
import torch.nn.functional as F

EPS = 1e-5


def inputs(B, groups, HW, seed=0, offset=0.0):
    """x, dy (B, 8 groups, HW / 4, 4), gamma, beta (8 groups) in fp32"""
    g = torch.Generator().manual_seed(seed * 7919 + B * 131 + groups * 17 + HW)
    C = 8 * groups
    x = torch.randn(B, C, HW // 4, 4, generator=g) * 1.5 + 0.3 + offset
    dy = torch.randn(B, C, HW // 4, 4, generator=g)
    gamma = torch.randn(C, generator=g) * 0.5 + 1.0
    beta = torch.randn(C, generator=g) * 0.5
    return x, dy, gamma, beta


def pre_activation64(x, gamma, beta, groups, eps=EPS):
    """xhat * gamma + beta in float64, (xhat, mean, rstd) beside it; mean / rstd (B, groups)"""
    B, C = x.shape[:2]
    xg = x.double().reshape(B, groups, -1)
    mean = xg.mean(-1)
    rstd = (xg.var(-1, unbiased=False) + eps).rsqrt()
    xh = ((xg - mean[..., None]) * rstd[..., None]).reshape(x.shape)
    return xh * gamma.double().view(1, C, 1, 1) + beta.double().view(1, C, 1, 1), xh, mean, rstd


def backward64(x, dy, gamma, beta, groups, eps, mask):
    """(dx, dgamma, dbeta) in float64: g = dy * mask (mask None: 1), n = 8 HW, s1 = sum_group gamma g, s2 = sum_group gamma g xhat,
    dx = rstd (gamma g - (s1 + xhat s2) / n), dgamma = sum g xhat, dbeta = sum g"""
    B, C = x.shape[:2]
    _, xh, _, rstd = pre_activation64(x, gamma, beta, groups, eps)
    g = dy.double() if mask is None else dy.double() * mask.to(torch.float64)
    gg = g * gamma.double().view(1, C, 1, 1)
    n = x[0].numel() // groups
    s1 = gg.reshape(B, groups, -1).sum(-1)
    s2 = (gg * xh).reshape(B, groups, -1).sum(-1)
    per_c = lambda t: t.repeat_interleave(C // groups, 1).view(B, C, 1, 1)          # noqa: E731
    dx = per_c(rstd) * (gg - (per_c(s1) + xh * per_c(s2)) / n)
    return dx, (g * xh).sum((0, 2, 3)), g.sum((0, 2, 3))


def torch_graph(x, dy, gamma, beta, groups, eps, relu, dtype, dev="cpu"):
    """(y, dx, dgamma, dbeta) of F.group_norm (+ F.relu) under autograd in `dtype`"""
    x_, w_, b_ = (t.detach().to(dev, dtype).requires_grad_(True) for t in (x, gamma, beta))
    with torch.enable_grad():
        y = F.group_norm(x_, groups, w_, b_, eps)
        if relu:
            y = F.relu(y)
        grads = torch.autograd.grad(y, (x_, w_, b_), dy.detach().to(dev, dtype))
    return (y.detach(),) + tuple(grads)


def separated_case(B, groups, HW, margin=1e-3):
    """inputs whose pre-activations all stay `margin` away from zero (the ReLU mask is then the same in every precision): the first seed
    that gives them"""
    for seed in range(200):
        x, dy, gamma, beta = inputs(B, groups, HW, seed)
        if float(pre_activation64(x, gamma, beta, groups)[0].abs().min()) >= margin:
            return x, dy, gamma, beta
    raise AssertionError("no separated case")


class TorchGroupNorms:
    """a plain-torch stand-in for net.HipBackendGroupNorms that records its calls"""

    def __init__(self):
        self.calls = []

    def group_norm(self, x, groups, weight, bias, eps, relu):
        self.calls.append((tuple(x.shape), groups, eps, relu))
        y = F.group_norm(x, groups, weight, bias, eps)
        return F.relu(y) if relu else y


def wiring_case(seed=3, C=32, cin=(6, 5, 4)):
    """(feats {res3, res4, res5}, padding mask, sd, cfg) for net.backbone_and_projections (with net.vit_backbone replaced by `feats`) and
    net.maskdino_pixel_decoder without encoder layers: the 4 + 7 conv + GroupNorm(32) blocks at C channels on 8 x 8 / 4 x 4 / 2 x 2 maps"""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=0.3):
        return (torch.randn(*shape, generator=g) * scale).requires_grad_(True)
    feats = {n: rnd(2, c, s, s, scale=1.0) for n, c, s in zip(("res3", "res4", "res5"), cin, (8, 4, 2))}
    sd = {}
    for p in ("detr.detr.", "detr.mask_dino.pixel_decoder."):
        for i, c in enumerate(cin + (cin[2],)):
            k = 3 if i == 3 else 1
            sd.update({"%sinput_proj.%d.0.weight" % (p, i): rnd(C, c, k, k), "%sinput_proj.%d.0.bias" % (p, i): rnd(C),
                       "%sinput_proj.%d.1.weight" % (p, i): rnd(C, scale=1.0), "%sinput_proj.%d.1.bias" % (p, i): rnd(C)})
    p = "detr.mask_dino.pixel_decoder."
    sd.update({p + "transformer.level_embed": rnd(4, 256), p + "adapter_1.weight": rnd(C, cin[0], 1, 1), p + "adapter_1.norm.weight": rnd(C, scale=1.0),
               p + "adapter_1.norm.bias": rnd(C), p + "layer_1.weight": rnd(C, C, 3, 3), p + "layer_1.norm.weight": rnd(C, scale=1.0),
               p + "layer_1.norm.bias": rnd(C), p + "mask_features.0.weight": rnd(C, C, 2, 2), p + "mask_features.0.bias": rnd(C),
               p + "mask_features.1.weight": rnd(C, scale=1.0), p + "mask_features.1.bias": rnd(C),
               p + "mask_features.3.weight": rnd(8, C, 1, 1), p + "mask_features.3.bias": rnd(8)})
    pad = torch.zeros(2, 64, 64, dtype=torch.bool)
    pad[1, :, 48:] = True
    return feats, pad, sd, dict(backbone="vit", hidden_dim=C, md_enc_layers=0)
