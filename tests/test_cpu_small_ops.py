"""Host-only proof of the premises tests/test_gpu_small_ops.py rests on (cases and references: tests/small_ops.py):

  * the pool reference -- eight strided slices added to zero in (dz, dy, dx) order, one multiply by 1/8 -- IS AvgPool3d(2): on
    small-integer data it equals fp64 F.avg_pool3d bit for bit, in any order of the additions; on Gaussian data it lies within
    2 ulp of the maximum of fp64's, and another order gives other bits.  So the integer cases pin the values, the Gaussian cases
    the order;
  * the one-hot reading of the upsample matrix recovers ATen's own matrix exactly, along every axis, forward and backward;
    ATen fp32's matrix error, the yardstick, is never zero from n = 2 on;
  * the Adam reference equals torch.optim.Adam(amsgrad=True) in fp64, and no ATen-fp32 yardstick of a measured quantity is zero;
  * the cases reach the edges their comments name (second trips, the three-pass form's minimum, every channel width);
  * a deliberately wrong reference fails the GPU tests' own comparison functions, ``same`` and ``within``, on host tensors."""
import math
import os
import random

import pytest
import torch
import torch.nn.functional as F

from tests import small_ops as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_SHAPES = tuple((B,) + s + (C,) for C in so.POOL_C for s in so.POOL_SHAPES for B in so.POOL_B)


def pool64(x):
    return F.avg_pool3d(x.double().permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1).contiguous()


def pool64_bwd(shape, gy, add=None):
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(pool64(x), [x], gy.double())
    return dx if add is None else dx + add.double()


# ------------------------------------------------------------------------------------------------ pooling
def test_pool_reference_is_avg_pool3d_exactly_on_integers():
    for shape in POOL_SHAPES:
        x, gy, add = so.ints(1, *shape), so.ints(2, *so.pool_shape(shape)), so.ints(3, *shape)
        assert torch.equal(so.pool_ref(x).double(), pool64(x)), shape
        assert torch.equal(so.pool_bwd_ref(gy).double(), pool64_bwd(shape, gy)), shape
        assert torch.equal(so.pool_bwd_ref(gy, add).double(), pool64_bwd(shape, gy, add)), shape


def test_pool_reference_is_within_two_ulp_of_the_maximum_on_gaussian_data():
    for shape in POOL_SHAPES:
        x = so.gauss(4, *shape)
        want = pool64(x)
        top = float(want.abs().max())
        ulp = 2.0 ** (math.floor(math.log2(top)) - 23)
        err = float((so.pool_ref(x).double() - want).abs().max())
        assert err <= 2.0 * ulp, (shape, err, ulp)


def test_integer_data_gives_the_same_bits_in_any_order_and_gaussian_data_does_not():
    rng = random.Random(5)
    orders = [so.POOL_ORDER[::-1]] + [tuple(rng.sample(so.POOL_ORDER, 8)) for _ in range(12)]
    shape = (3, 6, 10, 14, 8)
    xi, xg = so.ints(6, *shape), so.gauss(7, *shape)
    want_i, want_g = so.pool_ref(xi), so.pool_ref(xg)
    assert all(so.same(so.pool_ref(xi, order=o), want_i) for o in orders)
    assert any(not so.same(so.pool_ref(xg, order=o), want_g) for o in orders)
    # a pairwise tree, the other natural order of a kernel
    a = [xi[:, dz::2, dy::2, dx::2] for dz, dy, dx in so.POOL_ORDER]
    assert so.same((((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) * 0.125, want_i)


@pytest.mark.parametrize("kind", ("int", "gauss"))
def test_wrong_pool_references_fail_the_comparison(kind):
    shape, Bh = (4, 2, 4, 6, 8), 2
    x, gy, g = so.data(kind, 8, *shape), so.data(kind, 9, *so.pool_shape(shape)), so.data(kind, 10, *shape)
    ga, gb = g[:Bh], g[Bh:]
    assert so.same(so.pool_ref(x), so.pool_ref(x.clone()))
    assert not so.same(so.pool_ref(x, factor=0.25), so.pool_ref(x))                             # 1/4 instead of 1/8
    assert not so.same(so.pool_ref(x).flip(3), so.pool_ref(x))                                  # x mirrored
    assert not so.same(so.pool_bwd_ref(gy), so.pool_bwd_ref(gy, g))                             # the addend dropped
    assert not so.same(0.25 * so.unpool(gy) + g, so.pool_bwd_ref(gy, g))
    want = so.tee_split_bwd_ref(gy, ga, gb, Bh, shape)
    assert so.same(want, so.pool_bwd_ref(gy, g))
    assert not so.same(so.tee_split_bwd_ref(gy, gb, ga, Bh, shape), want)                       # the two halves swapped
    assert not so.same(so.tee_split_bwd_ref(gy, g[:1], g[1:], 1, shape)[:Bh], so.tee_split_bwd_ref(gy, g[:1], None, 1, shape)[:Bh])
    # a half whose gradient is absent gets exactly the unpooled share, not zero and not the other half's gradient
    only_a = so.tee_split_bwd_ref(gy, ga, None, Bh, shape)
    assert so.same(only_a[Bh:], 0.125 * so.unpool(gy)[Bh:]) and not so.same(only_a, want)
    assert so.same(so.tee_split_bwd_ref(None, ga, None, Bh, shape)[Bh:], torch.zeros(shape)[Bh:])
    assert so.same(so.tee_split_bwd_ref(None, ga, gb, Bh, shape), g)


def test_comparison_sees_dtype_shape_and_a_single_ulp():
    x = so.gauss(11, 257)
    y = x.clone()
    y[200] = torch.nextafter(y[200], torch.tensor(10.0))
    assert so.same(x, x.clone()) and not so.same(x, y)
    assert not so.same(x, x.double()) and not so.same(x, x.view(1, 257))
    assert so.within(4e-8, 1e-8) and not so.within(4.1e-8, 1e-8) and not so.within(1e-30, 0.0)


# ------------------------------------------------------------------------------------------------ flat kernels, layout
def test_flat_and_layout_cases_reach_their_edges():
    assert so.FLAT_CAP == 2 ** 20 and so.FLAT_N[-1] == 2 ** 20 + 257
    assert "g > 256 * 16" in open(os.path.join(ROOT, "smilecode_amd", "csrc", "common.h")).read()      # flat_grid's cap
    assert {c[1] for c in so.LAYOUT_CASES} == {2, 3, 8, 27}
    vols = [c[0] * math.prod(c[2]) for c in so.LAYOUT_CASES]
    assert all(math.prod(c[2]) % 256 for c in so.LAYOUT_CASES) and max(vols) == so.FLAT_CAP + 257
    for n in so.FLAT_N[1:]:
        dy, y = so.lrelu_inputs(n)
        sign = torch.signbit(y)
        assert ((y == 0) & ~sign).any() and ((y == 0) & sign).any() and (y > 0).any() and (y < 0).any()
        ref = so.lrelu_bwd_ref(dy, y)
        assert ref.dtype == torch.float32 and so.same(ref[y == 0], dy[y == 0] * torch.tensor(0.1))     # LeakyReLU'(+-0) = slope
        assert so.same(ref[y > 0], dy[y > 0])
    B, D, H, W, C = so.POOL_FWD_BIG
    assert B * (D // 2) * (H // 2) * (W // 2) * (C // 4) > so.FLAT_CAP
    assert math.prod(so.POOL_BWD_BIG) // 4 > so.FLAT_CAP
    assert len(so.SUBSETS) == 7 and len(set(so.SUBSETS)) == 7


def test_layout_references_are_inverse_permutations():
    x = so.gauss(12, 2, 3, 4, 5, 9)
    y = so.to_cl_ref(x)
    assert y.is_contiguous() and tuple(y.shape) == (2, 4, 5, 9, 3) and so.same(so.to_ncdhw_ref(y), x)
    assert float(y[1, 2, 3, 4, 1]) == float(x[1, 1, 2, 3, 4])
    assert not so.same(x.permute(0, 2, 3, 4, 1).reshape(2, 4, 5, 9, 3).transpose(1, 2).reshape(2, 4, 5, 9, 3), y)


# ------------------------------------------------------------------------------------------------ upsample x2
def aten_up(x, dtype, gy=None):
    xr = x.to(dtype).clone().requires_grad_(True)
    y = 2.0 * F.interpolate(xr.permute(0, 4, 1, 2, 3), scale_factor=2, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
    if gy is None:
        return y.detach()
    return torch.autograd.grad(y, [xr], gy.to(dtype))[0]


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8, 17))
def test_one_hot_reading_recovers_atens_matrix_along_every_axis(n):
    want = so.aten_matrix(n, torch.float64)
    assert tuple(want.shape) == (2 * n, n) and so.rows_are_two_adjacent(want)
    assert float((want.sum(1) - 1).abs().max()) < 1e-15
    for axis in range(3):
        x, g = so.onehot_inputs(axis, n), so.onehot_cotangents(axis, n)
        assert tuple(x.shape) == (n,) + so.axis_shape(axis, n) + (1,) and float(x.sum()) == n
        assert tuple(g.shape) == (2 * n,) + tuple(2 * s for s in so.axis_shape(axis, n)) + (1,) and float(g.sum()) == 2 * n
        assert so.same(so.matrix_from_fwd(aten_up(x, torch.float64), axis), want), axis
        bwd_x = torch.zeros((2 * n,) + so.axis_shape(axis, n) + (1,))
        assert so.same(so.matrix_from_bwd(aten_up(bwd_x, torch.float64, g), axis), want), axis
    if n == 1:
        assert so.same(want, torch.ones(2, 1, dtype=torch.float64))
    else:                                                                 # a matrix shifted by one index fails both comparisons
        shifted = torch.roll(want, 1, 1)
        assert not so.same(shifted, want)
        assert not so.within(so.matrix_err(shifted, n), so.matrix_err(so.aten_matrix(n, torch.float32), n) + so.matrix_yardstick())
        assert not so.rows_are_two_adjacent(want + torch.roll(want, 2, 1)) or n < 4


def test_upsample_matrix_yardstick_is_never_zero():
    errs = {n: so.matrix_err(so.aten_matrix(n, torch.float32), n) for n in so.UP_N + so.UP_N_SEP}
    assert errs[1] == 0.0 and all(e > 0 for n, e in errs.items() if n >= 2), errs
    assert 1e-8 < errs[2] < 1e-7 and 1e-6 < errs[182] < 1e-4              # (4e-8 at n = 2, 1e-5 at n = 182)
    assert so.matrix_yardstick() >= max(errs[n] for n in so.UP_N_YARD if n in errs) > 0
    assert all(so.matrix_bound(n) >= so.A * so.matrix_yardstick() for n in errs)
    assert all(2 * n * n >= so.SEP_MIN for n in so.UP_N_SEP) and all(2 * n * n < so.SEP_MIN for n in so.UP_N)
    assert "< 65536) return 0" in open(os.path.join(ROOT, "smilecode_amd", "csrc", "warp.hip")).read()


def test_upsample_cases_reach_every_width_and_the_three_pass_form():
    def cpt(C):
        return 4 if C % 4 == 0 else (3 if C % 3 == 0 else 1)
    assert {cpt(C) for C in so.UP_C} == {1, 3, 4} and {(cpt(C), C // cpt(C) > 1) for C in so.UP_C} >= {(3, True), (4, True), (1, True)}
    assert len(so.UP_CASES) == 144 and len(so.UP_YARD_CASES) == 72
    for (d, h, w), C, B, scale in so.UP_SEP_CASES:
        assert B * d * h * w >= so.SEP_MIN and min(d, h, w) in (1, 2, 3)
    inner = {((4 * h * w * C) % 4 == 0, (2 * w * C) % 4 == 0) for (d, h, w), C, B, s in so.UP_SEP_CASES}
    assert (True, False) in inner and (True, True) in inner                # both V4 branches of the rows kernel
    (d, h, w), C, B, s = so.UP_FWD_BIG
    assert B * 8 * d * h * w * (C // 4) > so.FLAT_CAP
    (d, h, w), C, B, s = so.UP_BWD_BIG
    assert B * d * h * w * (C // 4) > so.FLAT_CAP // 8 and B * d * h * w < so.SEP_MIN
    x1, g1 = so.up_tensors(((5, 7, 9), 3, 1, 2.0))
    x2, g2 = so.up_tensors(((5, 7, 9), 3, 2, 1.0))
    assert so.same(x2[:1], x1) and so.same(g2[:1], g1) and not so.same(x2[1:], x1)


def test_upsample_rule_on_the_host():
    """ATen fp32 passes its own rule; a result scaled by 1 + 1e-5, or with the two samples swapped, does not"""
    yard = so.up_yardstick()
    assert yard["out"] > 0 and yard["d_x"] > 0
    for case in (((1, 5, 3), 3, 2, 2.0), ((5, 7, 9), 4, 2, 1.0), ((8, 9, 17), 8, 1, 2.0)):
        x, gy = so.up_tensors(case)
        got, ref, bound = so.up_aten(x, gy, case[3], torch.float32), so.up_reference(case), so.up_bound(case)
        for q in so.UP_QUANTITIES:
            assert so.rel_err(got[q], ref[q]) <= bound[q]
            assert so.rel_err(got[q] * (1 + 1e-5), ref[q]) > bound[q]
            if case[2] == 2:
                assert so.rel_err(got[q].flip(0), ref[q]) > bound[q]


# ------------------------------------------------------------------------------------------------ Adam with AMSGrad
@pytest.mark.parametrize("name", sorted(so.ADAM_CASES))
def test_adam_reference_is_torch_optim_adam_in_fp64(name):
    n, c = 257, so.ADAM_CASES[name]
    p0, gs = so.adam_tensors(name, n)
    ref = so.adam_reference(name, n)
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([p], lr=c["lr"], amsgrad=True)
    if c["step0"] > 1:                                                    # a state that has seen step0 - 1 steps of zero gradient
        p.grad = torch.zeros_like(p)
        opt.step()
        opt.state[p]["step"] = torch.tensor(float(c["step0"] - 1))
        assert float(p.detach().sub(p0.double()).abs().max()) == 0.0
    for k, g in enumerate(gs):
        p.grad = g.double() * c["grad_scale"]
        opt.step()
        st = opt.state[p]
        for q, got in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"]), ("vmax", st["max_exp_avg_sq"])):
            assert so.rel_err(got, ref[k][q]) < 1e-13, (name, k, q)
    if not c["p0"]:                                                       # p from zero: p after the first step IS the step
        assert float(ref[0]["p"].abs().max()) < 4 * c["lr"] and float(ref[0]["p"].abs().min()) > 0


def test_adam_yardsticks_are_not_zero_and_vmax_keeps_the_old_maximum():
    for name in so.ADAM_CASES:
        for n in so.ADAM_N:
            yard, own = so.adam_yardstick(name, n), so.adam_own(name, n)
            assert all(own[(q, k)] > 0 for q in so.adam_measured(name) for k in range(so.ADAM_STEPS)), (name, n, own)
            assert all(own[key] <= yard[key] < 1e-6 for key in yard), (name, n)
            assert yard == so.adam_yardstick(name, 1027)                   # one yardstick per case
        ref = so.adam_reference(name, 1027)
        keeps = int((ref[1]["vmax"] > ref[1]["v"]).sum())                  # the second step's gradient is 10 x smaller:
        assert 100 < keeps < 927, keeps                                    # both branches of the maximum are taken
    assert so.ADAM_N_BIG > so.FLAT_CAP
    # eps dominates the denominator of the `eps` case, the bias corrections of `late` are 1
    r = so.adam_reference("eps", 1027)[0]
    assert float((r["vmax"].sqrt() / math.sqrt(1 - 0.999)).max()) < 5 * 1e-8
    assert 1 - 0.9 ** so.ADAM_CASES["late"]["step0"] == 1.0 and 1 - 0.999 ** so.ADAM_CASES["late"]["step0"] == 1.0


def test_open_adam_pins_are_few_and_above_the_rule():
    for name, pins in so.ADAM_A_OPEN.items():
        assert name in so.ADAM_CASES and set(pins) <= set(so.adam_measured(name)) and all(a > so.A for a in pins.values())
    assert so.adam_a("p0", "p") == so.A and so.adam_a("unit", "p") == so.A and so.adam_a("late", "m") == so.A
    # v is wrong by 1 - 0.999f against 0.001, whatever the data: 1.3e-5
    import numpy as np
    assert abs(float(np.float32(1) - np.float32(0.999)) / 0.001 - 1) == pytest.approx(1.29e-5, rel=0.01)


def _adam_eps_inside_sqrt(params, grads, state, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    for n, w in params.items():
        m, v, vmax = state[n]
        m.mul_(beta1).add_(grads[n], alpha=1 - beta1)
        v.mul_(beta2).addcmul_(grads[n], grads[n], value=1 - beta2)
        torch.maximum(vmax, v, out=vmax)
        w.addcdiv_(m, (vmax / bc2 + eps).sqrt(), value=-lr / bc1)


def _adam_without_amsgrad(params, grads, state, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    for n, w in params.items():
        m, v, vmax = state[n]
        m.mul_(beta1).add_(grads[n], alpha=1 - beta1)
        v.mul_(beta2).addcmul_(grads[n], grads[n], value=1 - beta2)
        vmax.copy_(v)
        w.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(eps), value=-lr / bc1)


def _adam_without_bias_correction(params, grads, state, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    from oracle import modet_torch as orc
    orc.adam_amsgrad_step(params, grads, state, lr * (1 - beta1 ** step), step, beta1, beta2, eps)


def _beyond(states, name, n):
    errs, yard = so.adam_errors(states, name, n), so.adam_yardstick(name, n)
    return {q for (q, k), e in errs.items() if q in so.adam_measured(name) and not so.within(e, yard[(q, k)])}


def test_wrong_adam_fails_the_rule():
    n = 1027
    for name in so.ADAM_CASES:
        assert not _beyond(so.adam_run(name, n, torch.float32), name, n)                      # ATen fp32 passes its own rule
        assert "p" in _beyond(so.adam_run(name, n, torch.float32, _adam_without_bias_correction), name, n) or name == "late", name
        # without the running maximum the denominators of the second step differ by a part in a thousand: seen from p = 0
        assert "p" in _beyond(so.adam_run(name, n, torch.float32, _adam_without_amsgrad), name, n) or name == "p0", name
    # eps inside the square root: seen where eps matters
    assert "p" in _beyond(so.adam_run("eps", n, torch.float32, _adam_eps_inside_sqrt), "eps", n)
    # grad_scale forgotten, or applied twice: m and v see it (p, a ratio of the two, does not)
    from oracle import modet_torch as orc
    c = so.ADAM_CASES["unit"]
    for wrong in (1.0, c["grad_scale"] ** 2):
        p0, gs = so.adam_tensors("unit", n)
        par, st, out = {"w": p0.clone()}, {"w": tuple(torch.zeros(n) for _ in range(3))}, []
        for k, g in enumerate(gs):
            orc.adam_amsgrad_step(par, {"w": g * wrong}, st, c["lr"], c["step0"] + k)
            out.append({"p": par["w"].clone(), "m": st["w"][0].clone(), "v": st["w"][1].clone(), "vmax": st["w"][2].clone()})
        assert {"m", "v", "vmax"} <= _beyond(out, "unit", n), wrong
