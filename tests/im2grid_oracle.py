"""TEST INFRASTRUCTURE ONLY -- CPU oracle of the Im2Grid baseline ("Baseline methods/Im2Grid/models.py":238-386), an independent
torch composition from oracle/modet_torch.py's encoder, mode_transformer, warp, upsample2, ncc_loss and grad3d_loss plus the
positional-encoding layer restated here.  Pure functions over a name -> tensor dict, differentiable through autograd, in fp64
(the reference for every bound) or fp32 (the ATen yardstick: what the same composition loses in single precision).

The embedding is formed in fp64 whatever the dtype of the run and cast once: the reference forms it in fp32 even inside a
``.double()`` model (``pos.type(torch.FloatTensor)``), which tests/golden/REPORT_im2grid.txt records as a ~1e-7 deviation."""
import math

import torch
import torch.nn.functional as F

from oracle import modet_torch as orc


def embedding(D, H, W, dtype=torch.float64):
    """(D,H,W,6): [cos t_d, sin t_d, cos t_h, sin t_h, cos t_w, sin t_w], t_p = p * pi / (n - 1), computed in fp64"""
    out = torch.zeros(D, H, W, 6, dtype=torch.float64)
    for a, n in enumerate((D, H, W)):
        t = torch.arange(n, dtype=torch.float64) * (math.pi / (n - 1))
        shape = [1, 1, 1]
        shape[a] = n
        out[..., 2 * a] = t.cos().reshape(shape)
        out[..., 2 * a + 1] = t.sin().reshape(shape)
    return out.to(dtype)


def posenc_cl(x, Wt, b, alpha):
    """channels-last (B,D,H,W,Cin) -> (B,D,H,W,6): Linear + alpha * embedding"""
    return F.linear(x, Wt, b) + alpha * embedding(*x.shape[1:4], dtype=x.dtype)


def posenc(p, name, feat):
    """(B,C,D,H,W) -> (B,D,H,W,6) with the parameters ``name.proj.weight | proj.bias | alpha`` of p"""
    return posenc_cl(feat.permute(0, 2, 3, 4, 1), p[name + ".proj.weight"], p[name + ".proj.bias"], p[name + ".alpha"])


def cotr(q, k):
    """the coordinate translator: one head over all channels, no bias, no scale -> (B,3,D,H,W)"""
    return orc.mode_transformer(q, k, torch.zeros(1, 27, dtype=q.dtype), 1, 1.0)


def im2grid_forward(p, moving, fixed, taps=None):
    """Im2grid.forward (models.py:352-386) -> (y_moved, flow)"""
    M = orc.encoder(p, moving)
    Fx = orc.encoder(p, fixed)

    def level(lvl, Mf):
        q, k = posenc(p, f"peblock{lvl}", Fx[lvl - 1]), posenc(p, f"peblock{lvl}", Mf)
        w = cotr(q, k)
        if taps is not None:
            taps[f"q{lvl}"], taps[f"k{lvl}"], taps[f"w{lvl}"] = q, k, w
        return w

    flow = orc.upsample2(2 * level(5, M[4]))
    for lvl in (4, 3, 2):
        w = level(lvl, orc.warp(M[lvl - 1], flow))
        flow = orc.upsample2(2 * (orc.warp(flow, w) + w))
    w = level(1, orc.warp(M[0], flow))
    flow = orc.warp(flow, w) + w
    return orc.warp(moving, flow), flow


def train_loss(p, moving, fixed, weights=(1.0, 1.0)):
    """NCC + Grad3d('l2') of one training iteration ("Baseline methods/Im2Grid/train.py") -> (loss, sim, reg, y_moved, flow)"""
    y_moved, flow = im2grid_forward(p, moving, fixed)
    sim, reg = orc.ncc_loss(fixed, y_moved), orc.grad3d_loss(flow)
    return weights[0] * sim + weights[1] * reg, sim, reg, y_moved, flow


def make_weights(channels=4, in_channel=1, seed=7, dtype=torch.float64):
    """seeded NON-zero parameters with the reference's names (the reference initialises the layer to zero weight, alpha = 1, where
    every q equals every k): fp32-representable values, so a fixture and a model hold the same numbers"""
    g = torch.Generator().manual_seed(seed)
    c, p = channels, {}
    convs = [("encoder.conv0.0", in_channel, c), ("encoder.conv0.1", c, 2 * c), ("encoder.conv0.2", 2 * c, 2 * c)]
    for lvl in range(1, 5):
        convs += [(f"encoder.conv{lvl}.1", 2 ** lvl * c, 2 ** (lvl + 1) * c), (f"encoder.conv{lvl}.2", 2 ** (lvl + 1) * c, 2 ** (lvl + 1) * c)]
    for name, cin, cout in convs:
        p[name + ".main.weight"] = torch.randn(cout, cin, 3, 3, 3, generator=g) * (1.0 / math.sqrt(27 * cin))
        p[name + ".main.bias"] = torch.randn(cout, generator=g) * 0.1
    for lvl in range(1, 6):
        cin = 2 ** lvl * c
        p[f"peblock{lvl}.proj.weight"] = torch.randn(6, cin, generator=g) * (1.5 / math.sqrt(cin))
        p[f"peblock{lvl}.proj.bias"] = torch.randn(6, generator=g) * 0.2
        p[f"peblock{lvl}.alpha"] = torch.tensor([0.6 + 0.15 * lvl])
    return {k: v.float().to(dtype) for k, v in p.items()}


def value_and_grads(p, moving, fixed, dtype):
    """one evaluation in ``dtype`` -> (loss, sim, reg, y_moved, flow, {name: gradient}), everything detached"""
    q = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
    loss, sim, reg, y, flow = train_loss(q, moving.to(dtype), fixed.to(dtype))
    names = sorted(q)
    grads = torch.autograd.grad(loss, [q[n] for n in names], allow_unused=True)
    return (loss.detach(), sim.detach(), reg.detach(), y.detach(), flow.detach(),
            {n: (torch.zeros_like(q[n]) if g is None else g.detach()) for n, g in zip(names, grads)})
