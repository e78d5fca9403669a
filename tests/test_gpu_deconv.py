"""-m gpu: the stride-2 4x4x4 transposed-convolution kernels (csrc/deconv.hip) on the MI355X against the layer in ATen fp64
(tests/rcn_oracle.py: F.conv_transpose3d(stride=2, padding=1) + LeakyReLU, the reference's layer), measured in units of the error
the same layer makes in ATen fp32 on the CPU.

THE RULE (tests/test_gpu_convs2.py's): per quantity, HIP's error against fp64 is at most A = 4 times the LARGEST ATen-fp32 error of
that quantity over the cases of this file.  An error is max|got - ref| / max|ref|.  Every measured figure goes to the parity
report (tests.util.note_many) before it is asserted.

TILES.  The forward works on tiles of 4x8x8 (up to 4 output channels), 4x4x8 (up to 8) or 4x4x4 input voxels, the data gradient on
4x4x8 (up to 8 input channels) or 4x4x4.  Case 6 (9x17x33, 8 -> 4) gives the forward 3x3x5 tiles and the data gradient 3x5x5, the
last one partial in every axis; cases 2 and 4 run the 4x4x4 tiles with 8 and 4 channel-group rows of workgroups."""
import functools

import pytest
import torch

from tests import rcn_oracle as orc
from tests.util import note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
QUANTITIES = ("y", "d_x", "d_w", "d_b")
CASES = tuple(sorted(orc.OP_CASES))


def quantities(n):
    return tuple(q for q in QUANTITIES if q != "d_b" or orc.OP_CASES[n][4])


@functools.lru_cache(maxsize=None)
def oracle(n, kind="randn"):
    """(tensors, fp64 results) of a case: computed once, shared, never modified"""
    t = orc.case_tensors(n, kind)
    return t, orc.op_value_and_grads(*t, orc.OP_CASES[n][5], torch.float64)


@functools.lru_cache(maxsize=None)
def aten_yardstick():
    """quantity -> the largest ATen-fp32 (CPU) error over the file's cases"""
    worst = {q: 0.0 for q in QUANTITIES}
    for n in CASES:
        t, ref = oracle(n)
        got = orc.op_value_and_grads(*t, orc.OP_CASES[n][5], torch.float32)
        for q in quantities(n):
            worst[q] = max(worst[q], rel_err(got[q], ref[q]))
    note_many({"deconv.aten_f32.%s" % q: v for q, v in worst.items()})
    return worst


def hip(x, w, b, gy, slope, x_grad=True):
    from smilecode_amd import ops
    x, w, gy = (t.cuda() for t in (x, w, gy))
    b = None if b is None else b.cuda().requires_grad_(True)
    x.requires_grad_(x_grad); w.requires_grad_(True)
    y = ops.conv_transpose3d_k4s2(x, w, b, slope)
    grads = list(torch.autograd.grad(y, ([x] if x_grad else []) + [w] + ([] if b is None else [b]), gy))
    return {"y": y.detach(), "d_x": grads.pop(0) if x_grad else None, "d_w": grads[0], "d_b": None if b is None else grads[1]}


@pytest.mark.parametrize("n", CASES)
def test_layer_against_fp64_in_units_of_aten_fp32(n):
    (t, ref), yard = oracle(n), aten_yardstick()
    got = hip(*t, orc.OP_CASES[n][5])
    errs = {q: rel_err(got[q], ref[q]) for q in quantities(n)}
    note_many({"deconv[case%d].%s.e_hip" % (n, q): e for q, e in errs.items()})
    for q in quantities(n):
        assert got[q].shape == ref[q].shape
        assert errs[q] <= A * yard[q], "case %d %s: e_hip %.3e, largest ATen fp32 error %.3e (A = %g)" % (n, q, errs[q], yard[q], A)


@pytest.mark.parametrize("n", (1, 3, 4, 6))
def test_integer_data_equals_fp64_bit_for_bit(n):
    """x, w, b, d_y integers in [-3, 3]: every product and sum is exactly representable (at most 64 * 128 * 9 in the data gradient,
    5 049 * 9 in case 6's weight gradient, all below 2^24), so whatever the summation order the four results ARE the fp64 ones (the
    slope enters once, as fl(P + slope * Q) of two exact integer sums)"""
    t, ref = oracle(n, "int")
    got = hip(*t, orc.OP_CASES[n][5])
    for q in quantities(n):
        assert torch.equal(got[q].cpu().double(), ref[q].float().double()), (n, q, float((got[q].cpu().double() - ref[q]).abs().max()))
        assert float(ref[q].abs().max()) > 0


@pytest.mark.parametrize("n", (3, 4, 6))
def test_delta_weights_pick_single_input_voxels(n):
    """w[c, c, k] = 1: y[2 i - 1 + k] == x[i] exactly and 0 where no input maps; d_x is the transpose of that.  k = (1,1,1): the
    even output voxels; k = (0,0,0): output 2 i - 1, which input 0 of an axis does not reach"""
    from smilecode_amd import ops
    B, (D, H, W), Cin, Cout, _, _ = orc.OP_CASES[n]
    C = min(Cin, Cout)
    x, _, _, gy = orc.case_tensors(n)
    for tap in ((1, 1, 1), (0, 0, 0)):
        w = torch.zeros(Cin, Cout, 4, 4, 4)
        for c in range(C):
            w[c, c][tap] = 1.0
        xg = x.cuda().requires_grad_(True)
        y = ops.conv_transpose3d_k4s2(xg, w.cuda(), None, None)
        (dx,) = torch.autograd.grad(y, [xg], gy.cuda())
        want, wdx = torch.zeros(B, 2 * D, 2 * H, 2 * W, Cout), torch.zeros_like(x)
        if tap == (1, 1, 1):
            want[:, ::2, ::2, ::2, :C] = x[..., :C]
            wdx[..., :C] = gy[:, ::2, ::2, ::2, :C]
        else:
            want[:, 1:-1:2, 1:-1:2, 1:-1:2, :C] = x[:, 1:, 1:, 1:, :C]          # output 2 i - 1 for i = 1 .. n - 1 per axis
            wdx[:, 1:, 1:, 1:, :C] = gy[:, 1:-1:2, 1:-1:2, 1:-1:2, :C]
        assert torch.equal(y.detach().cpu(), want), (n, tap)
        assert torch.equal(dx.cpu(), wdx), (n, tap)


@pytest.mark.parametrize("n", (1, 5, 6))
def test_two_runs_are_bit_identical_and_a_batch_equals_its_samples(n):
    t = orc.case_tensors(n)
    B, slope = orc.OP_CASES[n][0], orc.OP_CASES[n][5]
    if B == 1:                                                   # case 6 has one sample: stack it with a second, seeded one
        u = orc.case_tensors(n, seed=77)
        t = (torch.cat((t[0], u[0])), t[1], t[2], torch.cat((t[3], u[3])))
    a, b = hip(*t, slope), hip(*t, slope)
    for q in quantities(n):
        assert torch.equal(a[q], b[q]), (n, q)
    for i in range(2):
        one = hip(t[0][i:i + 1], t[1], t[2], t[3][i:i + 1], slope)
        assert torch.equal(one["y"], a["y"][i:i + 1]) and torch.equal(one["d_x"], a["d_x"][i:i + 1]), (n, i)


def test_an_input_without_a_gradient_launches_no_data_gradient():
    from smilecode_amd import ops
    t, slope = orc.case_tensors(1), orc.OP_CASES[1][5]
    full = hip(*t, slope)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        none = hip(*t, slope, x_grad=False)
    finally:
        ops.set_kernel_timer(None)
    tags = [r[0] for r in timer.records]
    assert tags == ["deconv_fwd[8->4]", "deconv_bwd_weight[8->4]"], tags
    assert torch.equal(none["d_w"], full["d_w"]) and torch.equal(none["d_b"], full["d_b"]) and torch.equal(none["y"], full["y"])


def test_wrapper_refusals_name_the_argument():
    from smilecode_amd import ops
    x, w, b = torch.zeros(1, 2, 2, 2, 4).cuda(), torch.zeros(4, 8, 4, 4, 4).cuda(), torch.zeros(8).cuda()
    for args, word in (((x, w[:2].contiguous(), b), "weight"), ((x, w, b[:4].contiguous()), "bias"),
                       ((x, w[..., :3].contiguous(), b), "weight"), ((x[0], w, b), "x must be"), ((x, w, b, -0.1), "slope"),
                       ((x.cpu(), w, b), "GPU"), ((x[:0], w, b), "empty")):
        with pytest.raises(RuntimeError, match=word):
            ops.conv_transpose3d_k4s2(*args)
    assert ops.conv_transpose3d_k4s2_out_shape(3, 4, 5) == (6, 8, 10)
