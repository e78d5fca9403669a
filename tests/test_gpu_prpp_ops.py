"""-m gpu: the PR++ family's kernels (csrc/prpp.hip) through smilecode_amd.ops against the same operators in ATen fp64 on the CPU
(tests/prpp_oracle.py), measured in units of the error ATen fp32 makes on the CPU.

THE RULE (tests/test_gpu_pcnet_ops.py's): per operator and quantity, HIP's error against fp64 is at most A = 4 times the LARGEST
ATen-fp32 error of that quantity over the operator's cases.  An error is max|got - ref| / max|ref|.  Every measured figure goes to
the parity report (tests.util.note_many) before it is asserted.  Where an operator only moves or selects numbers (the decoder
input, ReLU, the stack's outer slices) or its arithmetic is exact on the chosen data (integer cotangents, the half-integer
lattice of the composition) the assertion is equality of bits, with ATen or with fp64."""
import functools

import pytest
import torch

from tests import prpp_oracle as orc
from tests.util import note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0


def errors(got, ref, quantities):
    return {q: rel_err(got[q], ref[q]) for q in quantities}


_YARD = {}


def yardstick(op, quantities, cases, run):
    """quantity -> the largest ATen-fp32 error over the operator's cases"""
    if op not in _YARD:
        worst = {q: 0.0 for q in quantities}
        for n in cases:
            e = errors(run(n, torch.float32), run(n, torch.float64), quantities)
            worst = {q: max(worst[q], e[q]) for q in quantities}
        note_many({"prpp.%s.aten_f32.%s" % (op, q): v for q, v in worst.items()})
        _YARD[op] = worst
    return _YARD[op]


def check(op, n, got, ref, yard, quantities):
    errs = errors(got, ref, quantities)
    note_many({"prpp.%s[case%s].%s.e_hip" % (op, n, q): e for q, e in errs.items()})
    for q in quantities:
        assert got[q].shape == ref[q].shape and float(ref[q].abs().max()) > 0, (op, n, q)
        assert errs[q] <= A * yard[q], "%s case %s %s: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (op, n, q, errs[q], A * yard[q], A)


def bits(a, b):
    """equal as numbers everywhere and of one shape (a +0 against a -0 passes: ATen's own CPU and GPU ReLU differ there)"""
    return a.shape == b.shape and torch.equal(a.detach().cpu().double(), b.detach().cpu().double())


# ------------------------------------------------------------------------------------------------ upsample_nearest_cat
def upcat_hip(x, skip, gy, want_x=True, want_skip=True):
    from smilecode_amd import ops
    xg, sg = x.cuda().requires_grad_(want_x), skip.cuda().requires_grad_(want_skip)
    y = ops.upsample_nearest_cat(xg, sg)
    leaves = [t for t, wnt in ((xg, want_x), (sg, want_skip)) if wnt]
    grads = torch.autograd.grad(y, leaves, gy.cuda())
    out = {"out": y.detach()}
    out.update(dict(zip([k for k, wnt in (("d_x", want_x), ("d_skip", want_skip)) if wnt], grads)))
    return out


@pytest.mark.parametrize("n", sorted(orc.UPCAT_CASES))
def test_upcat_forward_is_atens_bits_and_integer_backward_is_fp64s(n):
    x, skip, gy = orc.upcat_tensors(n)
    got = upcat_hip(x, skip, gy)
    assert bits(got["out"], orc.upsample_nearest_cat(x, skip))
    x, skip, gy = orc.upcat_tensors(n, integer=True)                  # sums of eight small integers: exact in fp32
    got = upcat_hip(x, skip, gy)
    ref = orc.value_and_grads(orc.upsample_nearest_cat, {"x": x, "skip": skip}, gy, torch.float64)
    for q in ("out", "d_x", "d_skip"):
        assert bits(got[q], ref[q]) and float(ref[q].abs().max()) > 0, (n, q)
    only = upcat_hip(x, skip, gy, want_x=False)                       # a call that wants only d_skip
    assert set(only) == {"out", "d_skip"} and bits(only["d_skip"], ref["d_skip"])
    only = upcat_hip(x, skip, gy, want_skip=False)
    assert set(only) == {"out", "d_x"} and bits(only["d_x"], ref["d_x"])


def test_upcat_random_backward_within_the_rule():
    """d_x on random data: a sum of eight floats in the kernel's fixed order against fp64"""
    def run(n, dtype):
        x, skip, gy = orc.upcat_tensors(n)
        return orc.value_and_grads(orc.upsample_nearest_cat, {"x": x, "skip": skip}, gy, dtype)
    yard = yardstick("upcat", ("d_x",), sorted(orc.UPCAT_CASES), run)
    for n in sorted(orc.UPCAT_CASES):
        check("upcat", n, upcat_hip(*orc.upcat_tensors(n)), run(n, torch.float64), yard, ("d_x",))


# ------------------------------------------------------------------------------------------------ relu, relu_add
@pytest.mark.parametrize("n", orc.RELU_SIZES)
def test_relu_and_relu_add_are_atens_bits(n):
    """forward and backward against ATen on the same fp32 data, exact +0 and -0 included: the gradient at 0 is 0.  The cotangent is
    zeroed where |t| < RELU_EPS (the planted zeros only: the share is recorded and, at n = 1027, below 1 %) for the comparison
    with fp64, and left alone for the comparison with ATen's own backward"""
    from smilecode_amd import ops
    x, t, gy = orc.relu_tensors(n)
    near = t.abs() < orc.RELU_EPS
    note_many({"prpp.relu[n%d].masked_share" % n: float(near.float().mean())})
    if n >= 1027:
        assert float(near.float().mean()) < 0.01
    for masked in (False, True):
        g = torch.where(near, torch.zeros_like(gy), gy) if masked else gy
        dtype = torch.float64 if masked else torch.float32
        tg = t.cuda().requires_grad_(True)
        y = ops.relu(tg)
        (dt,) = torch.autograd.grad(y, [tg], g.cuda())
        ref = orc.value_and_grads(orc.relu, {"t": t}, g, dtype)
        assert bits(y, ref["out"]) and bits(dt, ref["d_t"])
        assert n < 3 or (float(dt[1]) == 0.0 and float(dt[2]) == 0.0)
        xg, tg = x.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
        s = ops.relu_add(xg, tg)
        dx, dt = torch.autograd.grad(s, [xg, tg], g.cuda())
        ref = orc.value_and_grads(orc.relu_add, {"x": x, "t": t}, g, torch.float32)      # (x + relu(t) rounds: fp32 against fp32)
        assert bits(s, ref["out"]) and bits(dx, ref["d_x"]) and bits(dt, ref["d_t"])
    tg = t.cuda().requires_grad_(True)                                # relu_add with a gradient for t only
    (dt,) = torch.autograd.grad(ops.relu_add(x.cuda(), tg), [tg], gy.cuda())
    assert bits(dt, orc.value_and_grads(orc.relu_add, {"x": x, "t": t}, gy, torch.float32)["d_t"])


def test_relu_passes_a_nan_and_in_place_calls_agree():
    from smilecode_amd import _lib, ops
    t = torch.tensor([float("nan"), -1.0, 2.0, -0.0, 0.5], device="cuda")
    y = ops.relu(t)
    assert bool(torch.isnan(y[0])) and y[1:].tolist() == [0.0, 2.0, 0.0, 0.5]
    buf = t.clone()
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().modet_prpp_relu_fwd(buf.data_ptr(), buf.data_ptr(), 5, s), "relu in place")
    assert torch.equal(buf[1:], y[1:])


# ------------------------------------------------------------------------------------------------ corr_stack
STACK_Q = ("corr", "d_mov", "d_fix")


@functools.lru_cache(maxsize=None)
def stack_oracle(n, dtype):
    mov, fix, gy = orc.stack_tensors(n)
    r = orc.value_and_grads(orc.corr_stack, {"mov": mov, "fix": fix}, gy, dtype)
    C = mov.shape[-1]
    r["corr"] = r["out"][..., C:C + 27]
    return r


def stack_hip(mov, fix, gy):
    from smilecode_amd import ops
    mg, fg = mov.cuda().requires_grad_(True), fix.cuda().requires_grad_(True)
    y = ops.corr_stack(mg, fg)
    dm, df = torch.autograd.grad(y, [mg, fg], gy.cuda())
    C = mov.shape[-1]
    return {"out": y.detach(), "corr": y.detach()[..., C:C + 27], "d_mov": dm, "d_fix": df}


@pytest.mark.parametrize("n", sorted(orc.STACK_CASES))
def test_stack_against_fp64_in_units_of_aten_fp32(n):
    """the outer slices are the inputs' bits; the middle slice is ops.correlation3d's (the same kernels: equal bits, and within
    the rule of oracle.modet_torch's correlation in fp64); the gradients of a random cotangent over ALL 2C + 27 channels; two runs
    give the same bits"""
    from smilecode_amd import ops
    mov, fix, gy = orc.stack_tensors(n)
    C = mov.shape[-1]
    got = stack_hip(mov, fix, gy)
    assert tuple(got["out"].shape) == tuple(mov.shape[:-1]) + (2 * C + 27,)
    assert torch.equal(got["out"][..., :C].cpu(), mov) and torch.equal(got["out"][..., C + 27:].cpu(), fix)
    planar = ops.correlation3d(mov.cuda(), fix.cuda())
    same = torch.equal(planar.permute(0, 2, 3, 4, 1), got["corr"])
    note_many({"prpp.stack[case%d].corr_equals_correlation3d_bits" % n: float(same)})
    yard = yardstick("stack", STACK_Q, sorted(orc.STACK_CASES), stack_oracle)
    ref = stack_oracle(n, torch.float64)
    check("stack", n, got, ref, yard, STACK_Q)
    assert same or rel_err(planar.permute(0, 2, 3, 4, 1), ref["corr"]) <= A * yard["corr"]
    again = stack_hip(mov, fix, gy)
    assert all(torch.equal(got[q], again[q]) for q in got)


def test_stack_batch_of_two_is_two_batches_of_one_and_outputs_are_optional():
    mov, fix, gy = orc.stack_tensors(2)
    both = stack_hip(mov, fix, gy)
    for b in range(2):
        one = stack_hip(mov[b:b + 1], fix[b:b + 1], gy[b:b + 1])
        assert all(torch.equal(both[q][b:b + 1], one[q]) for q in both), b
    from smilecode_amd import ops
    mg = mov.cuda().requires_grad_(True)
    (dm,) = torch.autograd.grad(ops.corr_stack(mg, fix.cuda()), [mg], gy.cuda())
    fg = fix.cuda().requires_grad_(True)
    (df,) = torch.autograd.grad(ops.corr_stack(mov.cuda(), fg), [fg], gy.cuda())
    assert torch.equal(dm, both["d_mov"]) and torch.equal(df, both["d_fix"])


# ------------------------------------------------------------------------------------------------ compose_cross
COMPOSE_Q = ("out", "d_src", "d_w")
COMPOSE_RULE_CASES = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def compose_oracle(n, dtype):
    src, w, gy = orc.compose_tensors(n)
    return orc.value_and_grads(orc.compose, {"src": src, "w": w}, gy, dtype)


def compose_hip(src, w, gy, want_src=True, want_w=True):
    from smilecode_amd import ops
    sg, wg = src.cuda().requires_grad_(want_src), w.cuda().requires_grad_(want_w)
    y = ops.compose_cross(sg, wg)
    leaves = [t for t, wnt in ((sg, want_src), (wg, want_w)) if wnt]
    grads = torch.autograd.grad(y, leaves, gy.cuda())
    out = {"out": y.detach()}
    out.update(dict(zip([k for k, wnt in (("d_src", want_src), ("d_w", want_w)) if wnt], grads)))
    return out


@pytest.mark.parametrize("n", COMPOSE_RULE_CASES)
def test_compose_against_fp64_in_units_of_aten_fp32(n):
    """fields of +-3 fine voxels: every face of the coarse grid has samples outside (asserted).  Two runs give the same bits, a
    batch of two the bits of two calls, d_src included"""
    src, w, gy = orc.compose_tensors(n)
    share = orc.outside_share(w, src.shape[1:4])
    note_many({"prpp.compose[case%d].outside_share" % n: share})
    assert share > 0.2
    got = compose_hip(src, w, gy)
    check("compose", n, got, compose_oracle(n, torch.float64), yardstick("compose", COMPOSE_Q, COMPOSE_RULE_CASES, compose_oracle), COMPOSE_Q)
    again = compose_hip(src, w, gy)
    assert all(torch.equal(got[q], again[q]) for q in got)
    for b in range(src.shape[0]):
        one = compose_hip(src[b:b + 1], w[b:b + 1], gy[b:b + 1])
        assert all(torch.equal(got[q][b:b + 1], one[q]) for q in got), b
    assert torch.equal(compose_hip(src, w, gy, want_w=False)["d_src"], got["d_src"])
    assert torch.equal(compose_hip(src, w, gy, want_src=False)["d_w"], got["d_w"])


def test_compose_on_the_half_integer_lattice_is_fp64s_bits():
    """3 x 5 x 9 -> 5 x 9 x 17 (the ratio is exactly 1/2 per axis), w on the half-integer lattice, integer src and cotangent: the
    output and both gradients are exact in fp32; the lattice holds a sample exactly on the last coarse node and one exactly one
    cell outside (tests/test_cpu_prpp.py)"""
    src, w, gy = orc.compose_exact_tensors()
    got = compose_hip(src, w, gy)
    ref = orc.value_and_grads(orc.compose, {"src": src, "w": w}, gy, torch.float64)
    for q in COMPOSE_Q:
        assert bits(got[q], ref[q]) and float(ref[q].abs().max()) > 0, q


def test_compose_on_equal_grids_is_warp_add_flow():
    """Sf = Sc: the ratio is exactly 1 and the kernel follows modet_warp_fwd's arithmetic; recorded whether the bits are equal,
    else held to the rule"""
    from smilecode_amd import ops
    src, w, gy = orc.compose_tensors(4)
    got = compose_hip(src, w, gy)
    sg, wg = src.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = ops.warp(sg, wg, add_flow=True)
    ds, dw = torch.autograd.grad(y, [sg, wg], gy.cuda())
    same = {"out": torch.equal(got["out"], y), "d_src": torch.equal(got["d_src"], ds), "d_w": torch.equal(got["d_w"], dw)}
    note_many({"prpp.compose[equal grids].%s_equals_warp_bits" % q: float(v) for q, v in same.items()})
    assert same["out"], "the forward follows warp_fwd_kernel instruction for instruction"
    yard = yardstick("compose", COMPOSE_Q, COMPOSE_RULE_CASES, compose_oracle)
    ref = compose_oracle(4, torch.float64)
    own = errors(compose_oracle(4, torch.float32), ref, COMPOSE_Q)
    for q, other in (("d_src", ds), ("d_w", dw)):
        assert same[q] or rel_err(got[q], ref[q]) <= A * max(yard[q], own[q]), q
        assert rel_err(other, ref[q]) <= A * max(yard[q], own[q]), q


def test_compose_is_not_upsample_then_warp_on_the_gpu_either():
    from smilecode_amd import ops
    src, w, _ = orc.compose_tensors(1)
    a = ops.compose_cross(src.cuda(), w.cuda())
    b = ops.warp(ops.upsample2(src.cuda(), 1.0), w.cuda(), add_flow=True)
    assert float((a - b).abs().max()) > 1e-2


def test_wrappers_refuse_by_name():
    from smilecode_amd import ops
    z = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    for bad, word in ((lambda: ops.upsample_nearest_cat(z(1, 2, 2, 2, 4), z(1, 4, 4, 5, 4)), "upsample_nearest_cat"),
                      (lambda: ops.upsample_nearest_cat(z(1, 2, 2, 2, 4), z(1, 4, 4, 4)), "upsample_nearest_cat"),
                      (lambda: ops.relu(z(0)), "relu"), (lambda: ops.relu_add(z(4), z(5)), "relu_add"),
                      (lambda: ops.corr_stack(z(1, 2, 2, 2, 6), z(1, 2, 2, 2, 6)), "corr_stack"),
                      (lambda: ops.corr_stack(z(1, 2, 2, 2, 8), z(1, 2, 2, 3, 8)), "corr_stack"),
                      (lambda: ops.corr_stack(z(1, 2, 2, 2, 132), z(1, 2, 2, 2, 132)), "corr_stack"),
                      (lambda: ops.compose_cross(z(1, 2, 2, 2, 3), z(1, 4, 1, 4, 3)), "compose_cross"),
                      (lambda: ops.compose_cross(z(1, 2, 2, 2, 3), z(2, 4, 4, 4, 3)), "compose_cross"),
                      (lambda: ops.compose_cross(z(1, 2, 2, 2, 4), z(1, 4, 4, 4, 3)), "compose_cross")):
        with pytest.raises(RuntimeError, match=word):
            bad()
