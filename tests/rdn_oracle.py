"""TEST INFRASTRUCTURE ONLY -- CPU oracle of the stride-2 convolution layer and of the RDN baseline ("Baseline methods/RDN/
models.py":172-214, :323-525), an independent torch composition: F.conv3d for both kinds of convolution, oracle/modet_torch.py's
warp, upsample2, ncc_loss and grad3d_loss, tests/vecint_oracle.py's scaling and squaring.  Pure functions over a name -> tensor
dict, differentiable through autograd, in fp64 (the reference for every bound) or fp32 (the ATen yardstick: what the same
composition loses in single precision).  nn.Conv3d in fp64 IS the reference's layer, so the op needs no committed fixture.

The cases of tests/test_gpu_convs2.py and tests/test_gpu_convs2_guard.py live here, so that both build the same tensors."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import modet_torch as orc
from tests import vecint_oracle as vio

# case number of the issue's table -> (B, (D, H, W), Cin, Cout, slope); slope None = no activation
OP_CASES = {
    1: (2, (3, 5, 7), 1, 16, 0.2),          # all dimensions odd, high-end padding, the image layer
    2: (1, (8, 6, 20), 16, 32, 0.2),        # all dimensions even
    3: (1, (2, 2, 2), 64, 128, 0.2),        # one output voxel, deepest K
    4: (1, (1, 1, 1), 4, 8, None),          # only the centre tap is data
    5: (2, (5, 4, 9), 8, 4, 0.0),           # ReLU, Cout < Cin
    6: (1, (9, 17, 33), 4, 8, 0.1),         # several workgroups and a partial last one in each of the three kernels
    7: (1, (4, 4, 6), 256, 256, 0.2),       # the channel limit
    # (N = B Do Ho Wo output voxels; the weight gradient makes S = ceil(N / V) partial rows, V = 256, 512 or 1024 by Cout)
    8: (2, (9, 17, 33), 1, 8, None),        # Cin = 1 without an activation; N = 1530: S = 6
    9: (1, (16, 18, 20), 8, 128, 0.2),      # V = 512 with N = 720: two splits, the last one partial
    10: (2, (17, 20, 24), 4, 256, 0.2),     # V = 1024 with N = 2160: three splits, the last one partial, across the batch boundary
    11: (1, (20, 22, 30), 4, 4, 0.1),       # N = 1650: S = 7
}
MASKED_FROM = 8            # cases from this number on zero the cotangent near y = 0 (cases 1 .. 7 keep the tensors they always had)
MASK_BELOW = 1e-5          # |y| in fp64 below which the two precisions may take different LeakyReLU branches (tests/rcn_oracle.py's)
MASK_CAP = 0.01            # at most this share of a case's outputs may lose its cotangent


def out_shape(D, H, W):
    return tuple((n - 1) // 2 + 1 for n in (D, H, W))


def f32_slope(slope):
    """the slope as the kernel receives it: rounded to fp32 once (0.2 and 0.1 are not fp32 numbers), whatever the run's dtype"""
    return None if slope is None else float(torch.tensor(slope, dtype=torch.float32))


def conv_s2_cl(x, w, b, slope):
    """channels-last (B,D,H,W,Cin) -> (B,Do,Ho,Wo,Cout): F.conv3d(stride=2, padding=1), then LeakyReLU(slope) unless slope is None"""
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, b, stride=2, padding=1)
    if slope is not None:
        s = f32_slope(slope)
        y = torch.where(y > 0, y, y * s)
    return y.permute(0, 2, 3, 4, 1)


def op_value_and_grads(x, w, b, gy, slope, dtype):
    """{y, d_x, d_w, d_b} of the layer in ``dtype`` for the cotangent gy, detached, channels-last"""
    o = [t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w, b)]
    y = conv_s2_cl(o[0], o[1], o[2], slope)
    dx, dw, db = torch.autograd.grad(y, o, gy.to(dtype))
    return {"y": y.detach(), "d_x": dx, "d_w": dw, "d_b": db}


@functools.lru_cache(maxsize=None)
def spec_tensors(spec, seed, kind="randn", mask=False):
    """(x, w, b, gy, masked share) of a layer (B, (D, H, W), Cin, Cout, slope) that need not be in OP_CASES, as case_tensors
    describes them; mask: zero the cotangent where |y| < MASK_BELOW in fp64 (an fp32 / fp64 LeakyReLU branch flip there is no
    kernel error)"""
    B, (D, H, W), Cin, Cout, slope = spec
    g = torch.Generator().manual_seed(seed)
    Do, Ho, Wo = out_shape(D, H, W)
    shapes = ((B, D, H, W, Cin), (Cout, Cin, 3, 3, 3), (Cout,), (B, Do, Ho, Wo, Cout))
    if kind == "int":
        return tuple(torch.randint(-3, 4, s, generator=g).float() for s in shapes) + (0.0,)
    x, w, b, gy = (torch.randn(s, generator=g) for s in shapes)
    w, b = w * (1.0 / math.sqrt(27 * Cin)), b * 0.1
    masked = 0.0
    if mask and slope is not None:
        near = conv_s2_cl(x.double(), w.double(), b.double(), slope).abs() < MASK_BELOW
        masked = float(near.double().mean())
        gy = torch.where(near, torch.zeros_like(gy), gy).contiguous()      # (near has the permuted strides of y: where() follows them)
    return x, w, b, gy, masked


def case_tensors(n, kind="randn", seed=None):
    """(x, w, b, gy) of case n in fp32.  kind 'randn': unit-variance data, weights scaled by 1/sqrt(27 Cin), from case MASKED_FROM
    on the cotangent zeroed where |y| < MASK_BELOW in fp64; 'int': integers in [-3, 3], every product and partial sum exactly
    representable in fp32"""
    return spec_tensors(OP_CASES[n], 1000 + n if seed is None else seed, kind, n >= MASKED_FROM)[:4]


def masked_share(n, seed=None):
    """the share of case n's outputs whose cotangent case_tensors zeroed (at most MASK_CAP: tests/test_cpu_rdn.py)"""
    return spec_tensors(OP_CASES[n], 1000 + n if seed is None else seed, "randn", n >= MASKED_FROM)[4]


# ------------------------------------------------------------------------------------------------ the network
def encoder(p, x):
    """four ConvBlock(., ., 3, 2, 1) with LeakyReLU(0.2), planar (B,C,D,H,W) -> [c, 2c, 4c, 8c] features at 1/2 .. 1/16"""
    out = []
    for i in range(4):
        x = F.leaky_relu(F.conv3d(x, p[f"encoder.conv{i}.main.weight"], p[f"encoder.conv{i}.main.bias"], stride=2, padding=1), 0.2)
        out.append(x)
    return out


def estimator(p, name, fixed_fm, moving_fm):
    x = torch.cat([fixed_fm, moving_fm], dim=1)
    for i in (0, 1, 2):
        x = F.conv3d(x, p[f"{name}.conv.{i}.weight"], p[f"{name}.conv.{i}.bias"], padding=1)
    x = F.leaky_relu(x, 0.1)
    return F.conv3d(x, p[f"{name}.conv.4.weight"], p[f"{name}.conv.4.bias"], padding=1)


def rdn_forward(p, moving, fixed, levels=(1, 1, 1, 1), diff=False, int_steps=7):
    """RDN.forward / RDN_diff.forward with one stage -> (y_moved, flow_out, stage flow | stage velocity)"""
    M, Fx = encoder(p, moving), encoder(p, fixed)
    integ = (lambda w: vio.vecint(w, int_steps)) if diff else (lambda w: w)
    sflow = sv = None
    for lvl in (3, 2, 1, 0):
        name = f"est{lvl}.0"
        if sflow is not None:
            sflow = orc.upsample2(2 * sflow)
            sv = orc.upsample2(2 * sv) if diff else None
        for j in range(levels[lvl]):
            if sflow is None:
                w = estimator(p, name, Fx[lvl], M[lvl])
                sflow, sv = integ(w), (w if diff else None)
                continue
            w = estimator(p, name, Fx[lvl], orc.warp(M[lvl], sflow))
            sv = orc.warp(sv, w) + w if diff else None
            w = integ(w)
            sflow = orc.warp(sflow, w) + w
    flow_out = orc.upsample2(2 * sflow)
    return orc.warp(moving, flow_out), flow_out, (sv if diff else sflow)


def train_loss(p, moving, fixed, levels=(1, 1, 1, 1), diff=False, int_steps=7):
    """NCC(y_moved) + Grad3d(stage field) as "Baseline methods/RDN/train.py":104-130 forms it at one stage
    -> (loss, sim, reg, y_moved, flow_out, stage field)"""
    y_moved, flow_out, s = rdn_forward(p, moving, fixed, levels, diff, int_steps)
    sim, reg = orc.ncc_loss(fixed, y_moved), orc.grad3d_loss(s)
    return sim + reg, sim, reg, y_moved, flow_out, s


def make_weights(seed=11, channels=4, in_channel=1, dtype=torch.float64):
    """seeded parameters with the reference's names, fp32-representable.  The flow convolutions are NON-zero (the reference starts
    them at Normal(0, 1e-5), where every w vanishes) and scaled so that each level's w stays of the order of a voxel"""
    g = torch.Generator().manual_seed(seed)
    c, p = channels, {}
    for i, (cin, cout) in enumerate([(in_channel, c), (c, 2 * c), (2 * c, 4 * c), (4 * c, 8 * c)]):
        p[f"encoder.conv{i}.main.weight"] = torch.randn(cout, cin, 3, 3, 3, generator=g) * (1.4 / math.sqrt(27 * cin))
        p[f"encoder.conv{i}.main.bias"] = torch.randn(cout, generator=g) * 0.1
    for lvl in range(4):
        w = 2 * 2 ** lvl * c
        for i in (0, 1, 2):
            p[f"est{lvl}.0.conv.{i}.weight"] = torch.randn(w, w, 3, 3, 3, generator=g) * (1.0 / math.sqrt(27 * w))
            p[f"est{lvl}.0.conv.{i}.bias"] = torch.randn(w, generator=g) * 0.05
        p[f"est{lvl}.0.conv.4.weight"] = torch.randn(3, w, 3, 3, 3, generator=g) * (0.6 / math.sqrt(27 * w))
        p[f"est{lvl}.0.conv.4.bias"] = torch.randn(3, generator=g) * 0.05
    return {k: v.float().to(dtype) for k, v in p.items()}


def value_and_grads(p, moving, fixed, dtype, levels=(1, 1, 1, 1), diff=False, int_steps=7):
    """one evaluation in ``dtype`` -> (loss, sim, reg, y_moved, flow_out, stage field, {name: gradient}), everything detached"""
    q = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
    loss, sim, reg, y, flow, s = train_loss(q, moving.to(dtype), fixed.to(dtype), levels, diff, int_steps)
    names = sorted(q)
    grads = torch.autograd.grad(loss, [q[n] for n in names], allow_unused=True)
    return (loss.detach(), sim.detach(), reg.detach(), y.detach(), flow.detach(), s.detach(),
            {n: (torch.zeros_like(q[n]) if g is None else g.detach()) for n, g in zip(names, grads)})


# the four golden runs: tag -> (levels, diff)
RUNS = {"rdn": ((2, 1, 1, 2), False), "rdn_diff": ((1, 1, 1, 1), True)}
