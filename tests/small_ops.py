"""Cases, seeded tensors and references for the small "plumbing" kernels: pooling (csrc/norm_act.hip), upsample x2 and layout
(csrc/warp.hip), the one-head CWM tail, the flat kernels (scale, LeakyReLU backward) and Adam with AMSGrad.  Host only.

Method.  Most of these operations are permutations, single roundings or sums in a fixed order, so their reference is the same
arithmetic in ATen-CPU fp32 and the comparison is ``same``: equal shape, dtype and values, no tolerance.  Where a kernel
interpolates or divides (upsample, Adam) the reference is ATen fp64 and the bound is A = 4 times the error ATen fp32 makes on
the same inputs (``within``: the per-op rule of tests/test_gpu_deconv.py and tests/test_gpu_resize.py).
tests/test_cpu_small_ops.py proves the premises on the host and shows that both comparisons reject a wrong reference;
tests/test_gpu_small_ops.py holds the kernels to them.

All volumes are channels-last (B,D,H,W,C) float32 unless a name says otherwise."""
import functools
import itertools

import torch
import torch.nn.functional as F

A = 4.0
# flat_grid (csrc/common.h) caps a flat launch at 4096 workgroups of 256 threads: a kernel with more work items than FLAT_CAP
# takes a second trip of its grid-stride loop
FLAT_CAP = 4096 * 256
FLAT_N = (1, 255, 257, FLAT_CAP + 257)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gauss(seed, *shape):
    return torch.randn(*shape, generator=gen(seed))


def ints(seed, *shape, amp=8):
    """small integers in [-amp, amp] as float32: every sum of a few of them, in any order, is exact"""
    return torch.randint(-amp, amp + 1, shape, generator=gen(seed)).float()


def data(kind, seed, *shape):
    return ints(seed, *shape) if kind == "int" else gauss(seed, *shape)


def same(got, want):
    """THE bit comparison of the GPU tests: equal dtype, shape and values (host copies; no tolerance)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def within(e_hip, e_f32, a=A):
    """THE tolerance rule of the GPU tests: an error against fp64 of at most ``a`` times ATen fp32's own"""
    return e_hip <= a * e_f32


# ------------------------------------------------------------------------------------------------ layout, scale, LeakyReLU'
# (B, C, (D, H, W)): V = D*H*W is no multiple of 256; the last case has B*V = FLAT_CAP + 257 work items
LAYOUT_CASES = tuple((B, C, s) for C in (2, 3, 8, 27) for B, s in ((2, (4, 5, 9)), (1, (1, 1, 255)))) + ((1, 3, (1, 1, FLAT_CAP + 257)),)
SCALES = (0.37, -2.0, 0.0)


def to_cl_ref(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def to_ncdhw_ref(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def lrelu_inputs(n):
    """(dy, y): y holds +0.0 and -0.0 (from n = 2 on) between positive and negative values"""
    dy, y = gauss(300 + n % 1000, n), gauss(301 + n % 1000, n)
    i = torch.arange(n)
    y[i % 5 == 0] = 0.0
    y[i % 5 == 1] = -0.0
    return dy, y


def lrelu_bwd_ref(dy, y):
    return dy * torch.where(y > 0, torch.tensor(1.0), torch.tensor(0.1))


# ------------------------------------------------------------------------------------------------ pooling
POOL_C = (4, 8, 12, 32)
POOL_SHAPES = ((2, 2, 2), (2, 4, 6), (6, 10, 14))          # x's (D, H, W)
POOL_B = (1, 3)
POOL_FWD_BIG = (1, 64, 128, 132, 32)                       # x: B*d*h*w*C/4 = 1 081 344 > FLAT_CAP
POOL_BWD_BIG = (1, 32, 64, 66, 32)                         # x: B*D*H*W*C/4 = 1 081 344 > FLAT_CAP
POOL_ORDER = tuple(itertools.product((0, 1), repeat=3))    # (dz, dy, dx), the kernel's order
SUBSETS = tuple(s for s in itertools.product((True, False), repeat=3) if any(s))     # which of (gy, ga, gb) arrive: seven
FUSED_C = (4, 8, 16)
FUSED_SHAPES = ((4, 6, 10), (8, 12, 20))


def pool_ref(x, order=POOL_ORDER, factor=0.125):
    """avgpool2_fwd_kernel's arithmetic in CPU fp32: the eight strided slices added to zero one by one, then one multiply"""
    s = torch.zeros_like(x[:, ::2, ::2, ::2])
    for dz, dy, dx in order:
        s = s + x[:, dz::2, dy::2, dx::2]
    return s * factor


def unpool(gy):
    return gy.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)


def pool_bwd_ref(gy, add=None):
    """avgpool2_bwd_kernel's arithmetic: multiply, then add the addend where there is one"""
    r = 0.125 * unpool(gy)
    return r if add is None else r + add


def tee_split_bwd_ref(gy, ga, gb, Bh, shape):
    """d_x of pool_tee_split for the cotangents that arrive (None: absent)"""
    zero = torch.zeros(shape)
    if gy is None:
        return torch.cat((zero[:Bh] if ga is None else ga, zero[Bh:] if gb is None else gb))
    u = 0.125 * unpool(gy)
    return torch.cat((u[:Bh] if ga is None else u[:Bh] + ga, u[Bh:] if gb is None else u[Bh:] + gb))


def pool_shape(shape):
    B, D, H, W, C = shape
    return (B, D // 2, H // 2, W // 2, C)


# ------------------------------------------------------------------------------------------------ upsample x2
UP_N = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33)
UP_N_SEP = (182, 183)                                      # batch 2n: B*d*h*w = 2 n^2 >= 65 536, the three-pass form's minimum
UP_N_YARD = tuple(range(2, 10))                            # the frozen yardstick set of the matrix test
SEP_MIN = 65536


def axis_shape(axis, n):
    s = [1, 1, 1]
    s[axis] = n
    return tuple(s)


def onehot_inputs(axis, n):
    """(n, d, h, w, 1): input i = e_i along ``axis``, the other two axes have size 1"""
    x = torch.zeros((n,) + axis_shape(axis, n) + (1,))
    for i in range(n):
        x[(i,) + tuple(i if a == axis else 0 for a in range(3)) + (0,)] = 1.0
    return x


def onehot_cotangents(axis, n):
    """(2n, 2d, 2h, 2w, 1): cotangent j = e_j along ``axis`` at fine (0, 0) of the other two axes"""
    g = torch.zeros((2 * n,) + tuple(2 * s for s in axis_shape(axis, n)) + (1,))
    for j in range(2 * n):
        g[(j,) + tuple(j if a == axis else 0 for a in range(3)) + (0,)] = 1.0
    return g


def matrix_from_fwd(y, axis, factor=2.0):
    """the (2n x n) weight matrix from upsample2(onehot_inputs, factor): W[j, i] = y[i] at fine j of ``axis``, (0, 0) elsewhere"""
    y = y.detach().cpu().movedim(1 + axis, 1)               # (n, 2n, 2, 2, 1) whatever the axis
    return (y[:, :, 0, 0, 0] / factor).t().contiguous()


def matrix_from_bwd(dx, axis, factor=2.0):
    """the same matrix from the backward on onehot_cotangents: W[j, i] = d_x[j] at coarse i"""
    dx = dx.detach().cpu().movedim(1 + axis, 1)             # (2n, n, 1, 1, 1)
    return (dx[:, :, 0, 0, 0] / factor).contiguous()


@functools.lru_cache(maxsize=None)
def aten_matrix(n, dtype):
    """F.interpolate(scale_factor=2, trilinear, align_corners=True) on the one-hot batch: its (2n x n) matrix in ``dtype``"""
    x = onehot_inputs(0, n).to(dtype).permute(0, 4, 1, 2, 3)
    y = F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True)
    return y[:, 0, :, 0, 0].t().contiguous()


def matrix_err(W, n):
    """max |W - W64|; the matrix's largest entry is 1, so this is the relative error of tests.util.rel_err too"""
    return float((W.double() - aten_matrix(n, torch.float64)).abs().max())


@functools.lru_cache(maxsize=None)
def matrix_yardstick():
    """the worst ATen-fp32 matrix error over the frozen set UP_N_YARD"""
    return max(matrix_err(aten_matrix(n, torch.float32), n) for n in UP_N_YARD)


def matrix_bound(n):
    return A * max(matrix_err(aten_matrix(n, torch.float32), n), matrix_yardstick())


def rows_are_two_adjacent(W):
    """every row: at most two non-zeros, adjacent"""
    for row in W:
        nz = torch.nonzero(row).flatten().tolist()
        if len(nz) > 2 or (len(nz) == 2 and nz[1] - nz[0] != 1):
            return False
    return True


UP_SHAPES = ((1, 1, 1), (1, 5, 3), (2, 2, 2), (3, 1, 4), (5, 7, 9), (8, 9, 17))
UP_C = (1, 2, 3, 4, 6, 8)                                  # pick_cpt: 1 (C = 1, 2), 3 (C = 3, 6: G = 1, 2), 4 (C = 4, 8: G = 1, 2)
UP_B = (1, 2)
UP_SCALES = (1.0, 2.0)
UP_CASES = tuple(itertools.product(UP_SHAPES, UP_C, UP_B, UP_SCALES))
# the yardstick is frozen to the cases of the first three shapes listed; a later case may use its own ATen-fp32 error instead
UP_YARD_CASES = tuple(c for c in UP_CASES if c[0] in UP_SHAPES[:3])
UP_SEP_CASES = tuple(itertools.product(((1, 256, 256), (256, 2, 128), (148, 148, 3)), (1, 3, 4), (1,), (2.0,)))
UP_FWD_BIG = ((32, 32, 33), 16, 1, 2.0)                    # B*8*d*h*w*G = 1 081 344 > FLAT_CAP
UP_BWD_BIG = ((16, 32, 33), 32, 1, 2.0)                    # B*d*h*w*G = 135 168 > 131 072 = 4096 workgroups of 32 groups
UP_QUANTITIES = ("out", "d_x")


def up_seed(case):
    (d, h, w), C, B, scale = case
    return 7 + d * 1009 + h * 101 + w * 11 + C * 5 + B


@functools.lru_cache(maxsize=None)
def up_tensors(case):
    """(x, gy) of a case, seeded by its shape; read-only.  The batch of two holds the batch of one as its first sample."""
    (d, h, w), C, B, scale = case
    s = up_seed(((d, h, w), C, 0, 0.0))
    x, gy = gauss(s, 2, d, h, w, C), gauss(s + 1, 2, 2 * d, 2 * h, 2 * w, C)
    return x[:B].contiguous(), gy[:B].contiguous()


def up_aten(x, gy, scale, dtype):
    """{out, d_x} of scale * F.interpolate(x2, trilinear, align_corners=True) in ``dtype`` on the CPU, channels-last"""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    y = scale * F.interpolate(xr.permute(0, 4, 1, 2, 3), scale_factor=2, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
    (dx,) = torch.autograd.grad(y, [xr], gy.to(dtype))
    return {"out": y.detach().contiguous(), "d_x": dx}


def rel_err(got, ref):
    """tests.util.rel_err (kept here so that this module imports nothing of the GPU side)"""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    return float((got - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def up_reference(case):
    """fp64 results of a case: computed once, shared, never modified"""
    return up_aten(*up_tensors(case), case[3], torch.float64)


@functools.lru_cache(maxsize=None)
def up_own(case):
    got, ref = up_aten(*up_tensors(case), case[3], torch.float32), up_reference(case)
    return {q: rel_err(got[q], ref[q]) for q in UP_QUANTITIES}


@functools.lru_cache(maxsize=None)
def up_yardstick():
    return {q: max(up_own(c)[q] for c in UP_YARD_CASES) for q in UP_QUANTITIES}


def up_bound(case):
    yard = up_yardstick()
    if case in UP_YARD_CASES:
        return {q: A * yard[q] for q in UP_QUANTITIES}
    own = up_own(case)
    return {q: A * max(yard[q], own[q]) for q in UP_QUANTITIES}


# ------------------------------------------------------------------------------------------------ Adam with AMSGrad
ADAM_N = (1, 255, 257, 1027)
ADAM_N_BIG = FLAT_CAP + 257
ADAM_QUANTITIES = ("p", "m", "v", "vmax")
ADAM_STEPS = 4
# four steps each, the state carried over, the second step's gradient 10 x smaller so that vmax keeps the old maximum
ADAM_CASES = {
    "unit": dict(gstd=1.0, lr=1e-4, step0=1, grad_scale=0.37, p0=False),
    "eps": dict(gstd=1e-8, lr=1e-4, step0=1, grad_scale=1.0, p0=False),          # eps = 1e-8 dominates the denominator
    "late": dict(gstd=1.0, lr=1e-4, step0=100000, grad_scale=1.0, p0=False),     # both bias corrections at 1
    "p0": dict(gstd=1.0, lr=1e-4, step0=1, grad_scale=1.0, p0=True),             # non-zero p: measured on p alone
}


@functools.lru_cache(maxsize=None)
def adam_tensors(name, n):
    """(p0, [g of each step]) in fp32; read-only"""
    c = ADAM_CASES[name]
    s = 900 + 17 * sorted(ADAM_CASES).index(name) + n % 4099
    p0 = gauss(s, n) if c["p0"] else torch.zeros(n)
    gs = [gauss(s + 1 + k, n) * (c["gstd"] * (0.1 if k == 1 else 1.0)) for k in range(ADAM_STEPS)]
    return p0, gs


def adam_run(name, n, dtype, step_fn=None):
    """the states {p, m, v, vmax} after each of the four steps of oracle.modet_torch.adam_amsgrad_step in ``dtype``, the
    gradients multiplied by grad_scale beforehand (in ``dtype``)"""
    from oracle import modet_torch as orc
    step_fn = step_fn or orc.adam_amsgrad_step
    c = ADAM_CASES[name]
    p0, gs = adam_tensors(name, n)
    par = {"w": p0.to(dtype).clone()}
    st = {"w": tuple(torch.zeros(n, dtype=dtype) for _ in range(3))}
    out = []
    for k, g in enumerate(gs):
        step_fn(par, {"w": g.to(dtype) * c["grad_scale"]}, st, c["lr"], c["step0"] + k)
        out.append({"p": par["w"].clone(), "m": st["w"][0].clone(), "v": st["w"][1].clone(), "vmax": st["w"][2].clone()})
    return out


@functools.lru_cache(maxsize=None)
def adam_reference(name, n):
    return adam_run(name, n, torch.float64)


def adam_errors(states, name, n):
    """{(quantity, step index): rel_err against the fp64 reference}"""
    ref = adam_reference(name, n)
    return {(q, k): rel_err(states[k][q], ref[k][q]) for k in range(ADAM_STEPS) for q in ADAM_QUANTITIES}


@functools.lru_cache(maxsize=None)
def adam_own(name, n):
    """ATen fp32's own errors in one run"""
    return adam_errors(adam_run(name, n, torch.float32), name, n)


@functools.lru_cache(maxsize=None)
def adam_yardstick(name, n):
    """ATen fp32's error of a quantity after a step IN THE CASE: the largest over the case's sizes ADAM_N (and n itself).  The
    kernel is elementwise, so a size is a sample of the same arithmetic, and the error of a single element is a draw between 0 and
    an ulp: at n = 1 ATen's own figure measures the draw (2.7e-16 on m after the first step of `eps`), not the arithmetic class."""
    runs = [adam_own(name, k) for k in sorted(set(ADAM_N) | {n})]
    return {key: max(r[key] for r in runs) for key in runs[0]}


# Quantities on which the kernel is measured BEYOND A x ATen fp32 (an open finding), case -> quantity -> A.
# modet_adam_amsgrad_step takes its betas as fp32 and forms 1.f - beta in the kernel: 1.f - 0.999f is 1.3e-5 below 0.001 and
# 1.f - 0.9f is 2.4e-7 above 0.1, so v and vmax sit 1.3e-5 and m 2.4e-7 from fp64; p follows only where the bias corrections,
# formed from the same rounded betas, no longer cancel it (`late`).  Each is pinned at 1.35 x its own measured worst
# e_hip / e_f32 over the sizes and steps (tests.util.GRAD_A_OPEN's convention), so that it cannot grow unseen; every other
# quantity is held to A.
ADAM_A_OPEN = {
    "unit": {"v": 100.0, "vmax": 100.0},                        # measured 74.0
    "eps": {"m": 7.4, "v": 198.0, "vmax": 198.0},               # measured 5.5, 146.4
    "late": {"p": 49.1, "v": 216.0, "vmax": 216.0},             # measured 36.4, 159.9, 160.1
}


def adam_a(name, q):
    return ADAM_A_OPEN.get(name, {}).get(q, A)


def adam_measured(name):
    """the quantities a case is measured on"""
    return ("p",) if ADAM_CASES[name]["p0"] else ADAM_QUANTITIES
