"""The flow regularisers of include/modet_hip_reg.h restated in torch, for any dtype, from the header's stencil formulae (shifted
slices, one explicit expression per derivative):

  itv, gradient_l2, gradient_l1, bending     fp64 = the yardstick's zero (equal to the reference's classes on the goldens of
                                             tests/golden/op_reg.npz); fp32 = the ATen composition whose own error against fp64
                                             sets the GPU parity bound
  KINDS                                      name (as train.py's --reg has it) -> function
  value_and_grad                             (loss, d loss / d flow) on a host copy

A flow is (B,C,D,H,W) planar."""
import torch

EPS = 1e-6


def _shift(f, lo, oz, oy, ox):
    """f[p + (oz, oy, ox)] for all p at least ``lo`` from every face"""
    D, H, W = f.shape[2:]
    return f[:, :, lo + oz:D - lo + oz, lo + oy:H - lo + oy, lo + ox:W - lo + ox]


def _off(*terms):
    """sum of k * e_a over the (k, a) given"""
    o = [0, 0, 0]
    for k, a in terms:
        o[a] += k
    return o


def itv(f):
    p = f[:, :, 1:, 1:, 1:]
    dz, dy, dx = p - f[:, :, :-1, 1:, 1:], p - f[:, :, 1:, :-1, 1:], p - f[:, :, 1:, 1:, :-1]
    return torch.sqrt(dz * dz + dy * dy + dx * dx + EPS).mean() / 3


def _central(f):
    return [(_shift(f, 1, *_off((1, a))) - _shift(f, 1, *_off((-1, a)))) / 2 for a in range(3)]


def gradient_l2(f):
    gz, gy, gx = _central(f)
    return (gz * gz + gy * gy + gx * gx).mean() / 3


def gradient_l1(f):
    gz, gy, gx = _central(f)
    return (gz.abs() + gy.abs() + gx.abs()).mean() / 3


def bending(f):
    c = _shift(f, 2, 0, 0, 0)
    total = 0
    for a in range(3):
        s = (_shift(f, 2, *_off((2, a))) - 2 * c + _shift(f, 2, *_off((-2, a)))) / 4
        total = total + s * s
    for a in range(3):
        for b in range(a + 1, 3):
            s = (_shift(f, 2, *_off((1, a), (1, b))) - _shift(f, 2, *_off((1, a), (-1, b)))
                 - _shift(f, 2, *_off((-1, a), (1, b))) + _shift(f, 2, *_off((-1, a), (-1, b)))) / 4
            total = total + 2 * (s * s)
    return total.mean()


KINDS = {"itv": itv, "gradient-l2": gradient_l2, "gradient-l1": gradient_l1, "bending": bending}
MIN_SIZE = {"itv": 2, "gradient-l2": 3, "gradient-l1": 3, "bending": 5}


def value_and_grad(fn, flow, dtype):
    """(loss, d loss / d flow) of ``fn`` on a host copy of ``flow`` in ``dtype``"""
    f = flow.detach().cpu().to(dtype).requires_grad_(True)
    loss = fn(f)
    (g,) = torch.autograd.grad(loss, [f])
    return loss.detach(), g
