"""TEST INFRASTRUCTURE ONLY -- the label-overlap (soft Dice) term of include/modet_hip_segdice.h as the ATen composition it
replaces: the one-hot moving labels (channels 1..L), warped trilinearly by ``oracle.modet_torch.warp``, the per-label sums against
the one-hot fixed labels, the loss; d_flow from autograd.  Runs wherever its tensors live, in the dtype asked for (fp64 on the CPU
is the reference of the tests, fp32 on the GPU the yardstick of their bounds), and the inputs the tests share.

``one_hot`` is written as a comparison with 1..L: the same channels for labels in 0..L, and defined (all zero) for the hostile
values the kernels must ignore (negative, above L), where torch's one_hot raises."""
import torch

from oracle import modet_torch as orc

EPS = 1e-5                       # dice_val_VOI's (reference utils.py:104)
SHAPES = [(1, 5, 6, 7), (2, 4, 5, 9), (1, 1, 3, 70), (1, 16, 16, 16)]      # (B, D, H, W)
LABELS = [1, 5, 54, 256]


def one_hot(lab, L, dtype):
    """(B,1,D,H,W) integer labels -> (B,L,D,H,W): channel l-1 is [lab == l], l in 1..L"""
    ids = torch.arange(1, L + 1, device=lab.device, dtype=torch.int64).view(1, L, 1, 1, 1)
    return (lab.to(torch.int64) == ids).to(dtype)


def table_and_loss(mov_lab, flow, fix_lab, L, dtype=torch.float64):
    """((B,3,L+1) table [I, P, T] with column 0 = 0, loss) in ``dtype``; differentiable in ``flow`` (planar (B,3,D,H,W))"""
    warped = orc.warp(one_hot(mov_lab, L, dtype), flow.to(dtype))
    fixed = one_hot(fix_lab, L, dtype)
    I, P, T = (fixed * warped).sum((2, 3, 4)), warped.sum((2, 3, 4)), fixed.sum((2, 3, 4))
    dsc = 2 * I / (P + T + EPS)
    table = torch.stack([I, P, T], 1)
    table = torch.cat([torch.zeros_like(table[..., :1]), table], -1)
    return table, 1 - dsc.mean()


def value_and_grad(mov_lab, flow, fix_lab, L, dtype=torch.float64):
    """(table, loss, d loss / d flow), detached"""
    f = flow.detach().to(dtype).requires_grad_(True)
    table, loss = table_and_loss(mov_lab, f, fix_lab, L, dtype)
    (g,) = torch.autograd.grad(loss, [f])
    return table.detach(), loss.detach(), g


def hostile(L):
    """label values that count in no sum: background, the int16 extremes and the first value above the range"""
    return [0, -32768, 32767, L + 1]


def absent_label(L):
    """the label that neither map of ``make_labels`` holds (with one label there is none to spare: None)"""
    return None if L == 1 else L // 2 + 1


def make_labels(shape, L, seed, noise=0.3):
    """(mov_lab, fix_lab) (B,1,D,H,W) int16.  Both maps of a batch item have the same four regions (the halves of z times the
    halves of y, so a region's rows are whole) with labels drawn from 1..L without ``absent_label(L)`` -- the warped moving labels
    overlap the fixed ones --, then ``noise`` of each map's voxels is redrawn at random from the valid labels and the ``hostile``
    values, and every hostile value is forced into both maps"""
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    valid = torch.tensor([l for l in range(1, L + 1) if l != absent_label(L)], dtype=torch.int64)
    pool = torch.cat([valid, torch.tensor(hostile(L), dtype=torch.int64)])
    z = (torch.arange(D) * 2 // D).view(D, 1, 1)
    y = (torch.arange(H) * 2 // H).view(1, H, 1)
    region = (z * 2 + y).expand(D, H, W)
    maps = ([], [])
    for _b in range(B):
        names = valid[torch.randint(len(valid), (4,), generator=gen)]
        for per in maps:
            lab = names[region]
            redraw = torch.rand((D, H, W), generator=gen) < noise
            lab = torch.where(redraw, pool[torch.randint(len(pool), (D, H, W), generator=gen)], lab)
            flat = lab.reshape(-1).clone()
            at = torch.randperm(flat.numel(), generator=gen)[:4]
            flat[at] = torch.tensor(hostile(L), dtype=torch.int64)
            per.append(flat.reshape(D, H, W))
    return tuple(torch.stack(per)[:, None].to(torch.int16).contiguous() for per in maps)


def lattice_flow(shape, seed):
    """planar (B,3,D,H,W) fp32 flow on the 1/16 grid: integer part in [-3, 3], fraction k / 16 with k in 1..15 -- p = v + flow is
    exact in fp32 and fp64 alike, never an integer (no kink), and near every face some voxels land wholly, some partly outside"""
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    whole = torch.randint(-3, 4, (B, 3, D, H, W), generator=gen)
    frac = torch.randint(1, 16, (B, 3, D, H, W), generator=gen)
    return (whole.double() + frac.double() / 16).float()


def integer_flow(shape, seed):
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (B, 3, D, H, W), generator=gen).float()


def general_flow(shape, seed):
    """a flow that is not dyadic: integer part in [-3, 3], fractional part uniform in [0.01, 0.99]"""
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    whole = torch.randint(-3, 4, (B, 3, D, H, W), generator=gen).double()
    frac = 0.01 + 0.98 * torch.rand((B, 3, D, H, W), generator=gen, dtype=torch.float64)
    return (whole + frac).float()


def positions(flow):
    """p = v + flow in fp64, (B,3,D,H,W)"""
    B, _, D, H, W = flow.shape
    g = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")).double()
    return flow.double().cpu() + g


def cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def planar(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()
