"""The two mutual-information losses restated in torch (include/modet_hip_mi.h has the definition), for any dtype:

  mi_loss / lmi_loss     fp64 = the yardstick's zero (equal to the reference's classes on the goldens of tests/golden/op_mi.npz);
                         fp32 on the CPU = the ATen composition whose own error against fp64 sets the GPU parity bound
  value_and_grads        (loss, d loss / d a, d loss / d b) of either on host copies

The bin centres are the fp32 values of torch.linspace whatever the dtype, as in the reference, whose centre tensor stays fp32."""
import numpy as np
import torch
import torch.nn.functional as F

BINS = 32


def _bins(minval, maxval, sigma_ratio, like):
    centres = torch.linspace(minval, maxval, BINS, dtype=torch.float32).to(device=like.device, dtype=like.dtype)
    sigma = np.mean(np.diff(np.linspace(minval, maxval, num=BINS))) * sigma_ratio
    return centres, 1.0 / (2.0 * sigma ** 2)


def _parzen(x, centres, preterm):
    """x (P, n) -> the normalised window weights (P, n, 32)"""
    w = torch.exp(-preterm * torch.square(x.unsqueeze(-1) - centres))
    return w / w.sum(dim=-1, keepdim=True)


def _mi(xa, xb, centres, preterm):
    """mutual information of each row pair of xa, xb (P, n) -> (P,)"""
    ia, ib = _parzen(xa, centres, preterm), _parzen(xb, centres, preterm)
    n = xa.shape[1]
    pab = torch.bmm(ia.transpose(1, 2), ib) / n
    pa, pb = ia.mean(dim=1, keepdim=True), ib.mean(dim=1, keepdim=True)
    papb = torch.bmm(pa.transpose(1, 2), pb) + 1e-6             # (an outer product as a bmm, rows then columns summed: the
    return (pab * torch.log(pab / papb + 1e-6)).sum(dim=1).sum(dim=1)      # reference's order, which the one-voxel case feels)


def mi_loss(a, b, sigma_ratio=1, minval=0.0, maxval=1.0):
    """a = y_true, b = y_pred, (B,1,D,H,W)"""
    centres, preterm = _bins(minval, maxval, sigma_ratio, a)
    xa, xb = (torch.clamp(t, 0.0, maxval).reshape(t.shape[0], -1) for t in (a, b))
    return -_mi(xa, xb, centres, preterm).mean()


def _patches(x, p):
    """(B,1,D,H,W), zero-padded to multiples of p (the smaller half on the low side) -> (patches, p^3)"""
    pad = []
    for n in reversed(x.shape[2:]):
        r = -n % p
        pad += [r // 2, r - r // 2]
    x = F.pad(x, pad, "constant", 0)
    B, _, D, H, W = x.shape
    x = x.reshape(B, D // p, p, H // p, p, W // p, p).permute(0, 1, 3, 5, 2, 4, 6)
    return x.reshape(-1, p ** 3)


def lmi_loss(a, b, sigma_ratio=1, minval=0.0, maxval=1.0, patch_size=5):
    centres, preterm = _bins(minval, maxval, sigma_ratio, a)
    xa, xb = (_patches(torch.clamp(t, 0.0, maxval), patch_size) for t in (a, b))
    return -_mi(xa, xb, centres, preterm).mean()


def value_and_grads(fn, a, b, dtype, **kw):
    """(loss, d loss / d a, d loss / d b) of ``fn`` on host copies of a and b in ``dtype``"""
    a = a.detach().cpu().to(dtype).requires_grad_(True)
    b = b.detach().cpu().to(dtype).requires_grad_(True)
    loss = fn(a, b, **kw)
    ga, gb = torch.autograd.grad(loss, [a, b])
    return loss.detach(), ga, gb
