"""The SSIM3D loss restated in torch (include/modet_hip_ssim.h has the definition), for any dtype:

  ssim_loss              fp64 = the yardstick's zero (equal to the reference's class on the goldens of tests/golden/op_ssim.npz);
                         fp32 = the ATen composition (five dense conv3d) whose own error against fp64 sets the GPU parity bound
  value_and_grads        (loss, d loss / d a, d loss / d b) on host copies

The 3-D window is built from the fp32 1-D taps by two fp32 matrix products, as the reference builds it, and only then cast to the
images' dtype."""
from math import exp

import torch
import torch.nn.functional as F

SIGMA = 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps(window_size):
    g = torch.tensor([exp(-(i - window_size // 2) ** 2 / float(2 * SIGMA ** 2)) for i in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def window(window_size, like):
    """(1, 1, w, w, w) in ``like``'s dtype and device"""
    t = taps(window_size).unsqueeze(1)
    w2 = t.mm(t.t())
    w3 = t.mm(w2.reshape(1, -1)).reshape(1, 1, window_size, window_size, window_size)
    return w3.to(device=like.device, dtype=like.dtype)


def ssim_loss(a, b, window_size=11):
    """a = img1, b = img2, (B,1,D,H,W)"""
    w, p = window(window_size, a), window_size // 2
    g = lambda v: F.conv3d(v, w, padding=p)      # noqa: E731
    mu1, mu2 = g(a), g(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = g(a * a) - mu1_sq, g(b * b) - mu2_sq, g(a * b) - mu1_mu2
    ssim = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return 1 - ssim.mean()


def value_and_grads(fn, a, b, dtype, **kw):
    """(loss, d loss / d a, d loss / d b) of ``fn`` on host copies of a and b in ``dtype``"""
    a = a.detach().cpu().to(dtype).requires_grad_(True)
    b = b.detach().cpu().to(dtype).requires_grad_(True)
    loss = fn(a, b, **kw)
    ga, gb = torch.autograd.grad(loss, [a, b])
    return loss.detach(), ga, gb
