"""The MIND-SSC descriptor and the MIND loss (Heinrich et al., MICCAI 2013) restated in pure torch, twice:

  mind_ssc / mind_loss            GATHER form, straight from the definition in include/modet_hip_losses.h: every neighbour
                                  access is an index_select through clamped coordinates.  Run in float64 it is the oracle of
                                  the HIP kernels (tests/golden/make_goldens_mind.py checks it against the reference's class).
  mind_ssc_aten / mind_loss_aten  the ATen COMPOSITION a framework user writes (replication pads, dilated one-hot conv3d,
                                  avg_pool3d, clamp with host-side bounds).  Run in float32 it is the arithmetic class the HIP
                                  path is measured against (its own error against float64 sets the parity bound) and the timing
                                  baseline of tools/bench_mind.py.

Images are (B,1,D,H,W).  Descriptors come out in the reference's channel order (PERM applied)."""
import torch
import torch.nn.functional as F

NEIGHBOURS = ((0, 1, 1), (1, 1, 0), (1, 0, 1), (1, 1, 2), (2, 1, 1), (1, 2, 1))
PAIRS = tuple((i, j) for i in range(6) for j in range(6)
              if i > j and sum((a - b) ** 2 for a, b in zip(NEIGHBOURS[i], NEIGHBOURS[j])) == 2)
PERM = (6, 8, 1, 11, 2, 10, 0, 7, 9, 4, 5, 3)
RADIUS, DILATION = 2, 2
assert PAIRS == ((1, 0), (2, 0), (2, 1), (3, 0), (3, 2), (4, 1), (4, 2), (4, 3), (5, 0), (5, 1), (5, 3), (5, 4))


def shifted(t, off):
    """s[..., p] = t[..., clamp(p + off)] over the last three axes"""
    for ax, o in zip((-3, -2, -1), off):
        if o:
            n = t.shape[ax]
            t = t.index_select(ax, (torch.arange(n) + o).clamp_(0, n - 1).to(t.device))
    return t


def _tail(ssd, g_scale=(0.001, 1000.0)):
    m = ssd - ssd.min(1, keepdim=True)[0]
    v = m.mean(1, keepdim=True)
    g = float(v.detach().mean())                              # a constant: nothing flows through it
    vc = v.clamp(g * g_scale[0], g * g_scale[1])
    return torch.exp(-(m / vc))[:, list(PERM)]


def mind_ssc(img):
    if img.dim() != 5 or img.shape[1] != 1:
        raise RuntimeError("mind_ssc: expects a (B,1,D,H,W) image")
    x = img[:, 0]
    s = [shifted(x, [DILATION * (c - 1) for c in nb]) for nb in NEIGHBOURS]
    d2 = torch.stack([(s[i] - s[j]) ** 2 for i, j in PAIRS], 1)
    for ax in range(3):                              # the 5^3 box, one axis at a time, clamped in the d^2 field
        acc = 0
        for o in range(-RADIUS, RADIUS + 1):
            off = [0, 0, 0]
            off[ax] = o
            acc = acc + shifted(d2, off)
        d2 = acc
    return _tail(d2 / float((2 * RADIUS + 1) ** 3))


def mind_loss(a, b):
    return ((mind_ssc(a) - mind_ssc(b)) ** 2).mean()


def _one_hot_kernels(dtype, device):
    w1 = torch.zeros(12, 1, 3, 3, 3, dtype=dtype, device=device)
    w2 = torch.zeros_like(w1)
    for c, (i, j) in enumerate(PAIRS):
        w1[(c, 0) + NEIGHBOURS[i]] = 1
        w2[(c, 0) + NEIGHBOURS[j]] = 1
    return w1, w2


def mind_ssc_aten(img):
    w1, w2 = _one_hot_kernels(img.dtype, img.device)
    p = F.pad(img, (DILATION,) * 6, mode="replicate")
    d = F.conv3d(p, w1, dilation=DILATION) - F.conv3d(p, w2, dilation=DILATION)
    ssd = F.avg_pool3d(F.pad(d * d, (RADIUS,) * 6, mode="replicate"), 2 * RADIUS + 1, stride=1)
    return _tail(ssd)


def mind_loss_aten(a, b):
    return ((mind_ssc_aten(a) - mind_ssc_aten(b)) ** 2).mean()


def value_and_grads(fn, a, b, dtype):
    """(loss, d loss / d a, d loss / d b) of ``fn`` on host copies of a and b in ``dtype``"""
    a = a.detach().cpu().to(dtype).requires_grad_(True)
    b = b.detach().cpu().to(dtype).requires_grad_(True)
    loss = fn(a, b)
    ga, gb = torch.autograd.grad(loss, [a, b])
    return loss.detach(), ga, gb
