"""-m gpu: the stride-2 4x4x4 transposed-convolution kernels (csrc/deconv.hip) on the MI355X against the layer in ATen fp64
(tests/rcn_oracle.py: F.conv_transpose3d(stride=2, padding=1) + LeakyReLU, the reference's layer), measured in units of the error
the same layer makes in ATen fp32 on the CPU.

THE RULE (tests/test_gpu_convs2.py's): per quantity, HIP's error against fp64 is at most A = 4 times the LARGEST ATen-fp32 error of
that quantity over cases 1 .. 7 of this file (YARD_CASES: the yardstick is frozen to them, a later case cannot raise it).  A case
from 8 on and a combination of the sweep may use A times its OWN ATen-fp32 error instead where that is larger (case 13's d_w sums
67 240 voxels: ATen's own error there, 2.0e-6, is beyond what the small cases show).  An error is max|got - ref| / max|ref|.  Every
measured figure, HIP's and ATen's, goes to the parity report (tests.util.note_many) before it is asserted.

TILES.  The forward works on tiles of 4x8x8 (up to 4 output channels), 4x4x8 (up to 8) or 4x4x4 input voxels, the data gradient on
4x4x8 (up to 8 input channels) or 4x4x4; either stages 16 input / 4 output channels at a time, and loads and stores rows of x / y
as 16-byte vectors where Cin / Cout is a multiple of 4 (VX / VY) and channel by channel otherwise.  The weight gradient cuts the
N input voxels into S = ceil(N / max(256, ceil(N / 256))) splits and sums their rows four at a time.  The 13 cases: 1 .. 7 are the
network's shapes and the smallest ones (case 6, 9x17x33, 8 -> 4: 3x3x5 forward and 3x5x5 data-gradient tiles, the last one partial
in every axis; cases 2 and 4: the 4x4x4 tiles with 8 and 4 channel-group rows of workgroups, one tile each).  8: the 4x4x8 forward
tile over 3x3x2 tiles, S = 5.  9: an activation with a Cout tail beside 16-byte rows of x, chunks of 16 + 4, the 4x4x4
data-gradient tile over 2x2x4 tiles with its second LDS half, S = 7 with a split across the batch boundary.  10: the network's
Deconv2 (35 -> 8: chunks of 16 + 16 + 3, 9 input-channel groups over 3 rows of workgroups).  11 and 12: the 4x4x4 forward tile over
2x2x3 tiles, a last chunk of 8, with and without a Cout tail.  13: S = 256 rows, the last split of 175 voxels, 11x5x6 tiles of
4x8x8.  The sweep (test_every_variant_...) launches each of the 12 + 16 + 8 instantiations the host code can choose."""
import functools

import pytest
import torch

from tests import rcn_oracle as orc
from tests.util import note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
QUANTITIES = ("y", "d_x", "d_w", "d_b")
CASES = tuple(sorted(orc.OP_CASES))
YARD_CASES = (1, 2, 3, 4, 5, 6, 7)         # the yardstick's cases, frozen
NEW_CASES = tuple(n for n in CASES if n not in YARD_CASES)


def quantities(n):
    return tuple(q for q in QUANTITIES if q != "d_b" or orc.OP_CASES[n][4])


@functools.lru_cache(maxsize=None)
def oracle(n, kind="randn"):
    """(tensors, fp64 results) of a case: computed once, shared, never modified"""
    t = orc.case_tensors(n, kind)
    return t, orc.op_value_and_grads(*t, orc.OP_CASES[n][5], torch.float64)


@functools.lru_cache(maxsize=None)
def aten_yardstick():
    """quantity -> the largest ATen-fp32 (CPU) error over YARD_CASES"""
    worst = {q: 0.0 for q in QUANTITIES}
    for n in YARD_CASES:
        t, ref = oracle(n)
        got = orc.op_value_and_grads(*t, orc.OP_CASES[n][5], torch.float32)
        for q in quantities(n):
            worst[q] = max(worst[q], rel_err(got[q], ref[q]))
    note_many({"deconv.aten_f32.%s" % q: v for q, v in worst.items()})
    return worst


def own_aten(key, t, ref, slope):
    """quantity -> the ATen-fp32 (CPU) error of these tensors themselves, noted as deconv.aten_f32[<key>].<quantity>"""
    got = orc.op_value_and_grads(*t, slope, torch.float32)
    own = {q: rel_err(got[q], ref[q]) for q in QUANTITIES if ref[q] is not None}
    note_many({"deconv.aten_f32[%s].%s" % (key, q): v for q, v in own.items()})
    return own


@functools.lru_cache(maxsize=None)
def allowed(n):
    """quantity -> the error case n may show: A x the frozen yardstick, for a case from 8 on A x its own ATen error if larger"""
    yard = aten_yardstick()
    if n in YARD_CASES:
        return {q: A * yard[q] for q in quantities(n)}
    own = own_aten("case%d" % n, *oracle(n), orc.OP_CASES[n][5])
    return {q: A * max(yard[q], own[q]) for q in quantities(n)}


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
    (t, ref), bound = oracle(n), allowed(n)
    got = hip(*t, orc.OP_CASES[n][5])
    errs = {q: rel_err(got[q], ref[q]) for q in quantities(n)}
    note_many({"deconv[case%d].%s.e_hip" % (n, q): e for q, e in errs.items()})
    for q in quantities(n):
        assert got[q].shape == ref[q].shape
        assert errs[q] <= bound[q], "case %d %s: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (n, q, errs[q], bound[q], A)


@pytest.mark.parametrize("n", (1, 3, 4, 6) + NEW_CASES)
def test_integer_data_equals_fp64_bit_for_bit(n):
    """x, w, b, d_y integers in [-3, 3]: every product and sum is exactly representable (at most 64 * 128 * 9 in the data gradient,
    67 240 * 9 in case 13's weight gradient, all below 2^24), so whatever the summation order the four results ARE the fp64 ones
    (the slope enters once, as fl(P + slope * Q) of two exact integer sums)"""
    t, ref = oracle(n, "int")
    got = hip(*t, orc.OP_CASES[n][5])
    for q in quantities(n):
        assert torch.equal(got[q].cpu().double(), ref[q].float().double()), (n, q, float((got[q].cpu().double() - ref[q]).abs().max()))
        assert float(ref[q].abs().max()) > 0


@pytest.mark.parametrize("n", (3, 4, 6, 8, 11, 12))
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


@pytest.mark.parametrize("n", (1, 5, 6, 9))
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


@pytest.mark.parametrize("Cin,Cout", [(ci, co) for ci in orc.SWEEP_CIN for co in orc.SWEEP_COUT])
def test_every_variant_the_host_can_launch_against_fp64(Cin, Cout):
    """One sample of 5x9x9 voxels with a bias, with and without LeakyReLU(0.1), at every (Cin, Cout) of the product below: integer
    data bit for bit as in test_integer_data_equals_fp64_bit_for_bit, then unit-variance data under THE RULE with the combination's
    own ATen-fp32 error.  The grid gives the three tile shapes 2x2x2, 2x3x2 and 2x3x3 tiles: a seam and a partial tile in every
    axis.  What the host code (csrc/deconv.hip) chooses, VX = Cin % 4 == 0, VY = Cout % 4 == 0:

        Cin   data-gradient tile  VX   forward chunks      |   Cout   forward tile  VY
          3   4x4x8               no   3                   |      3   4x8x8         no
          8   4x4x8               yes  8                   |      4   4x8x8         yes
         12   4x4x4               yes  12                  |      6   4x4x8         no
         27   4x4x4               no   16 + 11             |      8   4x4x8         yes
                                                           |     12   4x4x4         yes
                                                           |     13   4x4x4         no

        forward          <tile, VX, VY>:       3 tiles (Cout) x 2 VX (Cin) x 2 VY (Cout)                        = 12, each launched
        data gradient    <tile, ACT, VX, VY>:  4 (tile, VX) pairs (Cin) x 2 ACT (slope) x 2 VY (Cout)           = 16, each launched
        weight gradient  <ACT, VX, VY>:        2 ACT (slope) x 2 VX (Cin) x 2 VY (Cout)                         =  8, each launched

    e.g. deconv_fwd_kernel<4,4,4,false,false> is (27, 13) and (3, 13); deconv_bwd_data_kernel<4,4,8,true,true,false> is Cin = 8,
    Cout in (3, 6, 13) with the slope; deconv_bwd_weight_kernel<true,false,false> is Cin in (3, 27), Cout in (3, 6, 13) with the slope."""
    yard = aten_yardstick()
    for slope in orc.SWEEP_SLOPES:
        spec, seed = orc.sweep_spec(Cin, Cout, slope)
        key = "sweep %d->%d,%s" % (Cin, Cout, slope)
        t = orc.spec_tensors(spec, seed, "int")[:4]
        ref, got = orc.op_value_and_grads(*t, slope, torch.float64), hip(*t, slope)
        for q in QUANTITIES:
            assert torch.equal(got[q].cpu().double(), ref[q].float().double()), (key, q, float((got[q].cpu().double() - ref[q]).abs().max()))
            assert float(ref[q].abs().max()) > 0
        t = orc.spec_tensors(spec, seed)[:4]
        ref, got = orc.op_value_and_grads(*t, slope, torch.float64), hip(*t, slope)
        own = own_aten(key, t, ref, slope)
        errs = {q: rel_err(got[q], ref[q]) for q in QUANTITIES}
        note_many({"deconv[%s].%s.e_hip" % (key, q): e for q, e in errs.items()})
        for q in QUANTITIES:
            bound = A * max(yard[q], own[q])
            assert got[q].shape == ref[q].shape
            assert errs[q] <= bound, "%s %s: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (key, q, errs[q], bound, A)


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
