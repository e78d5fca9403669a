"""Scaling and squaring of a velocity field (the reference's VecInt, ModeT/models.py:70-87), restated in torch on direct voxel
coordinates with a dtype argument: the fp64 yardstick of the HIP kernels and, run in fp32, the ATen composition whose own error
sets the parity bound.  Equal to the reference's class in fp64 to rounding (tests/golden/REPORT_vecint.txt).

The cases of tests/test_cpu_vecint.py and tests/test_gpu_vecint.py live here too, so that the golden maker, the CPU and the GPU
tests build the same fields."""
import torch

from oracle import modet_torch as orc

# case -> (kind, B, shape, amp, nsteps, seed, in goldens)
CASES = {
    "n7_5x6x7_B2": ("randn", 2, (5, 6, 7), 2.0, 7, 71, True),
    "n3_4x5x67": ("randn", 1, (4, 5, 67), 3.0, 3, 71, True),
    "n1_6x6x6": ("randn", 1, (6, 6, 6), 1.5, 1, 71, True),
    "out_n3_6x7x9": ("randn", 1, (6, 7, 9), 12.0, 3, 71, True),
    "bounded_n7_8x12x16": ("tanh", 1, (8, 12, 16), 1.0, 7, 76, True),
    "mixed_n7_8x12x16": ("tanh", 1, (8, 12, 16), 8.0, 7, 73, False),
    "n2_12x20x28_B2": ("randn", 2, (12, 20, 28), 4.0, 2, 78, False),
}
COTANGENT_SEED = 5


def case_field(tag):
    """the planar (B,3,D,H,W) fp64 field of a case: randn in fp32 from the seeded generator, widened, times amp (tanh first for the
    'tanh' kind, so that max |field| <= amp)"""
    kind, B, shape, amp, _, seed, _ = CASES[tag]
    f = torch.randn((B, 3) + tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float32).double()
    return (torch.tanh(f) if kind == "tanh" else f) * amp


def cotangent(shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(COTANGENT_SEED), dtype=torch.float64)


def vecint(w, nsteps, rec=None):
    """VecInt(nsteps)(w) of a planar (B,3,D,H,W) field in voxels.  ``rec`` (a list) receives, per step, the sample coordinates
    p + v_k[p] as a (B,3,D,H,W) tensor."""
    v = w * (1.0 / (2 ** nsteps))
    for _ in range(nsteps):
        if rec is not None:
            B, _, D, H, W = v.shape
            grid = torch.stack(torch.meshgrid([torch.arange(s, dtype=v.dtype) for s in (D, H, W)], indexing="ij")).unsqueeze(0)
            rec.append((grid + v).detach())
        v = v + orc.warp(v, v)
    return v


def value_and_grad(w, nsteps, dtype, cot=None):
    """(out, d_w) in ``dtype`` for the cotangent ``cot`` (default: the seeded one), both detached"""
    w = w.to(dtype).clone().requires_grad_(True)
    out = vecint(w, nsteps)
    cot = cotangent(out.shape) if cot is None else cot
    (g,) = torch.autograd.grad(out, [w], cot.to(dtype))
    return out.detach(), g.detach()


def margin_and_coord_error(w, nsteps):
    """(margin, e_coord): the smallest distance of any sample coordinate from an integer over all steps, voxels and axes in
    fp64, and the largest difference between those coordinates evaluated in fp32 and in fp64.  Trilinear sampling has a slope
    kink at integer coordinates: an fp32 evaluation on the other side of one differs by a second difference of the field, not by
    rounding, so a parity case needs margin well above e_coord."""
    r64, r32 = [], []
    vecint(w.double(), nsteps, r64)
    vecint(w.float(), nsteps, r32)
    if not r64:
        return float("inf"), 0.0
    margin = min(float((c - torch.round(c)).abs().min()) for c in r64)
    e = max(float((a.double() - b).abs().max()) for a, b in zip(r32, r64))
    return margin, e


def modet_forward_diff(p, moving, fixed, int_steps=7, num_heads=(8, 4, 2, 1, 1), head_dim=6, scale=1.0):
    """oracle.modet_torch.modet_forward's level sequence with every level's field integrated before it is composed, as the
    reference's RDN_diff does (Baseline methods/RDN/models.py:268-310) -> (y_moved, flow)"""
    sc = scale if scale else head_dim ** -0.5
    M = orc.encoder(p, moving)
    Fx = orc.encoder(p, fixed)

    def level(lvl, Ff, Mf):
        heads = num_heads[5 - lvl]
        q = orc.projection(p, f"projblock{lvl}", Ff)
        k = orc.projection(p, f"projblock{lvl}", Mf)
        w = orc.mode_transformer(q, k, p[f"mdt{lvl}.rpb"], heads, sc)
        if lvl >= 3:
            w = orc.cwm(p, f"cwm{lvl}", w, heads)
        return vecint(w, int_steps)

    flow = level(5, Fx[4], M[4])
    w = level(4, Fx[3], orc.warp(M[3], flow))
    flow = orc.warp(orc.upsample2(2 * flow), w) + w
    w = level(3, Fx[2], orc.warp(M[2], flow))
    flow = orc.warp(orc.upsample2(2 * flow), w) + w
    w = level(2, Fx[1], orc.warp(M[1], flow))
    flow = orc.upsample2(2 * (orc.warp(flow, w) + w))
    w = level(1, Fx[0], orc.warp(M[0], flow))
    flow = orc.warp(flow, w) + w
    return orc.warp(moving, flow), flow
