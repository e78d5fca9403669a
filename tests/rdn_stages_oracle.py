"""TEST INFRASTRUCTURE ONLY -- CPU oracle of the trilinear resize (include/modet_hip_resize.h) and of RDN with recursive stages and
its weight-shared forms ("Baseline methods/RDN/models.py":217-525, :617-704): tests/rdn_oracle.py's encoder and estimator,
oracle/modet_torch.py's warp and upsample2, tests/vecint_oracle.py's scaling and squaring, and a ``resize`` written from the
header's index rule (not from F.interpolate, which tests/test_cpu_rdn_stages.py compares it with).  Pure functions over a name ->
tensor dict, differentiable through autograd, in fp64 (the reference for every bound) or fp32 (the ATen yardstick).

The cases of tests/test_gpu_resize.py and tests/test_gpu_resize_guard.py live here, so that both build the same tensors."""
import functools

import numpy as np
import torch

from oracle import modet_torch as orc
from tests import rdn_oracle as rdn
from tests import vecint_oracle as vio

# ------------------------------------------------------------------------------------------------ the operator
# case number of the issue's table -> (B, (Di, Hi, Wi), (Do, Ho, Wo), C, scale)
OP_CASES = {
    1: (1, (9, 13, 33), (5, 4, 2), 3, 0.5),         # the ratios are the integers 2, 4 and 32: out = 0.5 x[::2, ::4, ::32]
    2: (2, (16, 24, 16), (8, 12, 8), 3, 0.5),       # the pyramid's 1/2 level at the golden shape
    3: (1, (16, 24, 16), (2, 3, 2), 3, 0.125),      # its 1/8 level
    4: (1, (7, 9, 11), (3, 4, 5), 1, 1.0),          # one channel, odd sizes
    5: (1, (3, 4, 5), (7, 9, 11), 4, 2.0),          # the 16-byte path, upsampling, a non-integer ratio
    6: (2, (5, 1, 6), (1, 4, 6), 8, -1.5),          # So = 1, Si = 1 and identity, one axis each
    7: (1, (2, 2, 2), (9, 9, 9), 3, 1.0),           # an input index in nine stencils per axis
    8: (1, (6, 6, 6), (6, 6, 6), 3, 0.25),          # identity: out = 0.25 x
    9: (1, (40, 48, 40), (20, 24, 20), 3, 0.5),     # several workgroups and a partial last one
    10: (1, (4, 6, 8), (8, 12, 16), 6, 2.0),        # C = 6: the scalar path (run once more on a view offset by one float)
}
YARD_CASES = (1, 2, 3, 4, 5, 6, 7)                  # the yardstick's cases, frozen
# (B, (D, H, W)) of the pyramid cases
PYRAMID_CASES = {1: (1, (16, 24, 16)), 2: (2, (8, 8, 8)), 3: (1, (9, 11, 33)), 4: (1, (40, 48, 40))}
PYRAMID = ((2, 0.5), (4, 0.25), (8, 0.125))


def axis_cells(Si, So, dtype):
    """(i0, i1, l) of every output index of one axis, by the header's rule: r and c in fp32 when dtype is fp32 (what the kernel
    does), in fp64 otherwise (the reference for every bound)"""
    ft = np.float32 if dtype == torch.float32 else np.float64
    r = ft(Si - 1) / ft(So - 1) if So > 1 else ft(0)
    c = (r * np.arange(So).astype(ft)).astype(ft)
    i0 = np.minimum(c.astype(np.int64), Si - 1)
    i1 = np.minimum(i0 + 1, Si - 1)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy((c - i0.astype(ft)).astype(ft)).to(dtype)


def resize(x, size, scale=1.0):
    """scale * the trilinear resize of channels-last x (B,D,H,W,C) onto ``size``, axis by axis: y = (1 - l) x[i0] + l x[i1]"""
    y = x
    for ax, So in zip((1, 2, 3), size):
        i0, i1, l = axis_cells(y.shape[ax], int(So), x.dtype)
        shape = [1] * 5
        shape[ax] = -1
        l = l.reshape(shape)
        y = (1 - l) * y.index_select(ax, i0) + l * y.index_select(ax, i1)
    return scale * y


def flow_pyramid(flow):
    """the three rescaled downsamplings of a channels-last field, sized as nnf.interpolate(scale_factor=) sizes them"""
    return tuple(resize(flow, tuple(s // f for s in flow.shape[1:4]), sc) for f, sc in PYRAMID)


def op_value_and_grad(x, gy, size, scale, dtype):
    """{out, d_x} of ``resize`` in ``dtype`` for the cotangent gy, detached"""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    y = resize(xr, size, scale)
    (dx,) = torch.autograd.grad(y, [xr], gy.to(dtype))
    return {"out": y.detach(), "d_x": dx}


@functools.lru_cache(maxsize=None)
def case_tensors(n, seed=None):
    """(x, gy) of case n in fp32, unit variance, seeded"""
    B, si, so, C, _ = OP_CASES[n]
    g = torch.Generator().manual_seed(2000 + n if seed is None else seed)
    return torch.randn((B,) + si + (C,), generator=g), torch.randn((B,) + so + (C,), generator=g)


@functools.lru_cache(maxsize=None)
def pyramid_tensors(n, seed=None):
    """(x, gy2, gy4, gy8, add) of pyramid case n in fp32"""
    B, s = PYRAMID_CASES[n]
    g = torch.Generator().manual_seed(3000 + n if seed is None else seed)
    x = torch.randn((B,) + s + (3,), generator=g)
    gys = tuple(torch.randn((B,) + tuple(v // f for v in s) + (3,), generator=g) for f, _ in PYRAMID)
    return (x,) + gys + (torch.randn(x.shape, generator=g),)


# ------------------------------------------------------------------------------------------------ the network
def _cl(t):
    return t.permute(0, 2, 3, 4, 1)


def _planar(t):
    return t.permute(0, 4, 1, 2, 3)


def staged_forward(p, moving, fixed, stages, levels=(1, 1, 1, 1), diff=False, share=False, int_steps=7):
    """RDN / RDN_diff / RDN_share / RDN_diff_share .forward -> (y_moved, flow_out, [stage field per stage]); planar tensors"""
    M, Fx = rdn.encoder(p, moving), rdn.encoder(p, fixed)
    integ = (lambda w: vio.vecint(w, int_steps)) if diff else (lambda w: w)
    flow, fields = None, []
    for i in range(stages):
        if i == 0:
            Fm = M
        else:
            f2, f4, f8 = (_planar(f) for f in flow_pyramid(_cl(flow)))
            Fm = [orc.warp(M[0], flow), orc.warp(M[1], f2), orc.warp(M[2], f4), orc.warp(M[3], f8)]
        sflow = sv = None
        for lvl in (3, 2, 1, 0):
            name = f"est{lvl}" if share else f"est{lvl}.{i}"
            if sflow is not None:
                sflow = orc.upsample2(2 * sflow)
                sv = orc.upsample2(2 * sv) if diff else None
            for j in range(levels[lvl]):
                if sflow is None:
                    w = rdn.estimator(p, name, Fx[lvl], Fm[lvl])
                    sflow, sv = integ(w), (w if diff else None)
                    continue
                w = rdn.estimator(p, name, Fx[lvl], orc.warp(Fm[lvl], sflow))
                sv = orc.warp(sv, w) + w if diff else None
                w = integ(w)
                sflow = orc.warp(sflow, w) + w
        flow = sflow if i == 0 else orc.warp(flow, sflow) + sflow
        fields.append(sv if diff else sflow)
    flow_out = orc.upsample2(2 * flow)
    return orc.warp(moving, flow_out), flow_out, fields


def train_loss(p, moving, fixed, stages, levels=(1, 1, 1, 1), diff=False, share=False, int_steps=7):
    """NCC(y_moved) + sum over stages of Grad3d(stage field), as "Baseline methods/RDN/train.py":104-130 forms it
    -> (loss, sim, reg, y_moved, flow_out, fields)"""
    y_moved, flow_out, fields = staged_forward(p, moving, fixed, stages, levels, diff, share, int_steps)
    sim = orc.ncc_loss(fixed, y_moved)
    reg = orc.grad3d_loss(fields[0])
    for f in fields[1:]:
        reg = reg + orc.grad3d_loss(f)
    return sim + reg, sim, reg, y_moved, flow_out, fields


def make_weights(stages, share, seed=11, channels=4, dtype=torch.float64):
    """tests/rdn_oracle.py's make_weights under the staged names: the encoder as it is; unshared, stage s of level l gets the
    estimator of seed + 100 s (stage 0 IS rdn_oracle's, so one stage is the one-stage network); shared, ``estL.conv.*`` is stage 0's"""
    p = {}
    for s in range(1 if share else stages):
        q = rdn.make_weights(seed + 100 * s, channels, dtype=dtype)
        for k, v in q.items():
            if k.startswith("encoder."):
                if s == 0:
                    p[k] = v
            elif share:
                p[k.replace(".0.conv.", ".conv.")] = v
            else:
                p[k.replace(".0.conv.", ".%d.conv." % s)] = v
    return p


def value_and_grads(p, moving, fixed, dtype, stages, levels=(1, 1, 1, 1), diff=False, share=False, int_steps=7):
    """one evaluation in ``dtype`` -> (loss, sim, reg, y_moved, flow_out, [stage fields], {name: gradient}), everything detached"""
    q = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
    loss, sim, reg, y, flow, fields = train_loss(q, moving.to(dtype), fixed.to(dtype), stages, levels, diff, share, int_steps)
    names = sorted(q)
    grads = torch.autograd.grad(loss, [q[n] for n in names], allow_unused=True)
    return (loss.detach(), sim.detach(), reg.detach(), y.detach(), flow.detach(), [f.detach() for f in fields],
            {n: (torch.zeros_like(q[n]) if g is None else g.detach()) for n, g in zip(names, grads)})


# the four golden runs: tag -> (the reference's class, stages, levels finest first, diff, share)
RUNS = {
    "rdn_s2": ("RDN", 2, (1, 1, 1, 2), False, False),
    "share_s3": ("RDN_share", 3, (1, 1, 1, 1), False, True),
    "diff_s2": ("RDN_diff", 2, (1, 1, 1, 1), True, False),
    "diff_share_s2": ("RDN_diff_share", 2, (1, 1, 2, 1), True, True),
}
