"""-m gpu: the stride-2 convolution kernels (csrc/convs2.hip) and the channel concatenation on the MI355X against the layer in ATen
fp64 (tests/rdn_oracle.py: F.conv3d(stride=2, padding=1) + LeakyReLU, the reference's own layer), measured in units of the error
the same layer makes in ATen fp32 on the CPU.

THE RULE (tests/test_gpu_im2grid.py's and tests/test_gpu_vecint.py's): per quantity, HIP's error against fp64 is at most A = 4 times
the LARGEST ATen-fp32 error of that quantity over cases 1 .. 7 of this file (YARD_CASES: the yardstick is frozen to them, a later
case cannot raise it).  A case from 8 on may use A times its OWN ATen-fp32 error instead where that is larger (case 10's d_w and
d_b sum 2 160 voxels: ATen's own errors there, 1.9e-6 and 1.5e-6, are beyond what the small cases show).  An error is
max|got - ref| / max|ref|.  Every measured figure, HIP's and ATen's, goes to the parity report (tests.util.note_many) before it is
asserted.

TILES.  The kernels are flat launches of 256 threads without a grid cap: the forward has one thread per (output voxel, 4 output
channels), the data gradient one per (input voxel, 4 input channels), the weight gradient 256 (tap, 4 ci, 4 co) items per workgroup
and one workgroup row per V = 256, 512 (Cout > 64) or 1024 (Cout > 128) output voxels; its S = ceil(N / V) rows are summed four
at a time.  The 11 cases: 1 .. 7 are the network's shapes and the smallest ones (case 6, 9x17x33, 4 -> 8: 765 output and 5 049
input voxels, gives the three kernels 6, 20 and 3 workgroups, the last one partial in each -- there are no per-axis tiles, so "a
partial tile in every axis" is the partial last workgroup of a flat index whose three axes are all odd); S is 1 or 3 in all of them.
8: Cin = 1 without an activation (convs2_bwd_data_kernel<1,false>, convs2_bwd_weight_kernel<1,false>), S = 6.  9: V = 512 with two
rows, the last one of 208 voxels.  10: V = 1024 with three rows, the second across the batch boundary, the last one of 112 voxels.
11: S = 7.  With tests/test_gpu_deconv.py's 5, 7 and 256 the column sum runs one round of four and a tail of 1, 2 and 3 rows, and
64 rounds without a tail."""
import functools

import pytest
import torch

from tests import rdn_oracle as orc
from tests.util import note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
QUANTITIES = ("y", "d_x", "d_w", "d_b")
CASES = tuple(sorted(orc.OP_CASES))
YARD_CASES = (1, 2, 3, 4, 5, 6, 7)         # the yardstick's cases, frozen
NEW_CASES = tuple(n for n in CASES if n not in YARD_CASES)


@functools.lru_cache(maxsize=None)
def oracle(n, kind="randn"):
    """(tensors, fp64 results) of a case: computed once, shared, never modified"""
    t = orc.case_tensors(n, kind)
    return t, orc.op_value_and_grads(*t, orc.OP_CASES[n][4], torch.float64)


@functools.lru_cache(maxsize=None)
def aten_yardstick():
    """quantity -> the largest ATen-fp32 (CPU) error over YARD_CASES"""
    worst = {q: 0.0 for q in QUANTITIES}
    for n in YARD_CASES:
        t, ref = oracle(n)
        got = orc.op_value_and_grads(*t, orc.OP_CASES[n][4], torch.float32)
        for q in QUANTITIES:
            worst[q] = max(worst[q], rel_err(got[q], ref[q]))
    note_many({"convs2.aten_f32.%s" % q: v for q, v in worst.items()})
    return worst


@functools.lru_cache(maxsize=None)
def allowed(n):
    """quantity -> the error case n may show: A x the frozen yardstick, for a case from 8 on A x its own ATen-fp32 (CPU) error if
    that is larger (noted as convs2.aten_f32[case<n>].<quantity>)"""
    yard = aten_yardstick()
    if n in YARD_CASES:
        return {q: A * yard[q] for q in QUANTITIES}
    t, ref = oracle(n)
    got = orc.op_value_and_grads(*t, orc.OP_CASES[n][4], torch.float32)
    own = {q: rel_err(got[q], ref[q]) for q in QUANTITIES}
    note_many({"convs2.aten_f32[case%d].%s" % (n, q): v for q, v in own.items()})
    return {q: A * max(yard[q], own[q]) for q in QUANTITIES}


def hip(x, w, b, gy, slope, x_grad=True):
    from smilecode_amd import ops
    x, w, b, gy = (t.cuda() for t in (x, w, b, gy))
    x.requires_grad_(x_grad); w.requires_grad_(True); b.requires_grad_(True)
    y = ops.conv3d_s2(x, w, b, slope)
    grads = torch.autograd.grad(y, ([x] if x_grad else []) + [w, b], gy)
    return {"y": y.detach(), "d_x": grads[0] if x_grad else None, "d_w": grads[-2], "d_b": grads[-1]}


@pytest.mark.parametrize("n", CASES)
def test_layer_against_fp64_in_units_of_aten_fp32(n):
    (t, ref), bound = oracle(n), allowed(n)
    got = hip(*t, orc.OP_CASES[n][4])
    errs = {q: rel_err(got[q], ref[q]) for q in QUANTITIES}
    note_many({"convs2[case%d].%s.e_hip" % (n, q): e for q, e in errs.items()})
    for q in QUANTITIES:
        assert got[q].shape == ref[q].shape
        assert errs[q] <= bound[q], "case %d %s: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (n, q, errs[q], bound[q], A)


@pytest.mark.parametrize("n", (1, 2, 5, 6) + NEW_CASES)
def test_integer_data_equals_fp64_bit_for_bit(n):
    """x, w, b, d_y integers in [-3, 3]: every product and sum is exactly representable (at most 27 * 256 * 9 in case 10's data
    gradient and 2 160 * 9 in its weight gradient, all below 2^24), so whatever the summation order the four results ARE the fp64
    ones (the slope enters once, as fl(P + slope * Q) of two exact integer sums)"""
    t, ref = oracle(n, "int")
    got = hip(*t, orc.OP_CASES[n][4])
    for q in QUANTITIES:
        assert torch.equal(got[q].cpu().double(), ref[q].float().double()), (n, q, float((got[q].cpu().double() - ref[q]).abs().max()))
        assert float(ref[q].abs().max()) > 0


@pytest.mark.parametrize("n", (2, 5, 6, 8))
def test_delta_weights_pick_single_input_voxels(n):
    """centre tap + identity channels: y[o] == x[2o], d_x == d_y at even indices and 0 elsewhere; tap (0,0,0): y[o] == x[2o - 1],
    0 where that is padding"""
    from smilecode_amd import ops
    B, (D, H, W), Cin, Cout, _ = orc.OP_CASES[n]
    C = min(Cin, Cout)
    x, _, _, gy = orc.case_tensors(n)
    Do, Ho, Wo = orc.out_shape(D, H, W)
    for tap in ((1, 1, 1), (0, 0, 0)):
        w = torch.zeros(Cout, Cin, 3, 3, 3)
        for c in range(C):
            w[c, c][tap] = 1.0
        xg = x.cuda().requires_grad_(True)
        y = ops.conv3d_s2(xg, w.cuda(), None, None)
        (dx,) = torch.autograd.grad(y, [xg], gy.cuda())
        want = torch.zeros(B, Do, Ho, Wo, Cout)
        wdx = torch.zeros_like(x)
        if tap == (1, 1, 1):
            want[..., :C] = x[:, ::2, ::2, ::2, :C]
            wdx[:, ::2, ::2, ::2, :C] = gy[..., :C]
        else:
            odd = (slice(None), slice(1, 2 * Do - 2, 2), slice(1, 2 * Ho - 2, 2), slice(1, 2 * Wo - 2, 2), slice(0, C))
            want[:, 1:, 1:, 1:, :C] = x[odd]                      # x[2o - 1] for o = 1 .. Do - 1 per axis
            wdx[odd] = gy[:, 1:, 1:, 1:, :C]
        assert torch.equal(y.detach().cpu(), want), (n, tap)
        assert torch.equal(dx.cpu(), wdx), (n, tap)


@pytest.mark.parametrize("n", (1, 5, 6, 10))
def test_two_runs_are_bit_identical_and_a_batch_equals_its_samples(n):
    t = orc.case_tensors(n)
    B, slope = orc.OP_CASES[n][0], orc.OP_CASES[n][4]
    if B == 1:                                                   # case 6 has one sample: stack it with a second, seeded one
        u = orc.case_tensors(n, seed=77)
        t = (torch.cat((t[0], u[0])), t[1], t[2], torch.cat((t[3], u[3])))
    a, b = hip(*t, slope), hip(*t, slope)
    for q in QUANTITIES:
        assert torch.equal(a[q], b[q]), (n, q)
    for i in range(2):
        one = hip(t[0][i:i + 1], t[1], t[2], t[3][i:i + 1], slope)
        assert torch.equal(one["y"], a["y"][i:i + 1]) and torch.equal(one["d_x"], a["d_x"][i:i + 1]), (n, i)


def test_an_input_without_a_gradient_launches_no_data_gradient():
    from smilecode_amd import ops
    t, slope = orc.case_tensors(1), orc.OP_CASES[1][4]
    full = hip(*t, slope)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        none = hip(*t, slope, x_grad=False)
    finally:
        ops.set_kernel_timer(None)
    tags = [r[0] for r in timer.records]
    assert tags == ["convs2_fwd[1->16]", "convs2_bwd_weight[1->16]"], tags
    assert torch.equal(none["d_w"], full["d_w"]) and torch.equal(none["d_b"], full["d_b"]) and torch.equal(none["y"], full["y"])


def test_raw_image_range():
    """the 1 -> 16 layer on an image scaled by 60 000: within the same yardstick (no reduced-precision form, no range assumption)"""
    x, w, b, gy = orc.case_tensors(1)
    x, slope = x * 60000.0, orc.OP_CASES[1][4]
    ref, yard = orc.op_value_and_grads(x, w, b, gy, slope, torch.float64), aten_yardstick()
    got = hip(x, w, b, gy, slope)
    errs = {q: rel_err(got[q], ref[q]) for q in QUANTITIES}
    note_many({"convs2[raw_image].%s.e_hip" % q: e for q, e in errs.items()})
    assert float(ref["y"].abs().max()) > 1e4 and bool(torch.isfinite(got["y"]).all())
    for q in QUANTITIES:
        assert errs[q] <= A * yard[q], "raw image %s: e_hip %.3e, largest ATen fp32 error %.3e" % (q, errs[q], yard[q])


def test_no_bias_and_no_activation_forms():
    from smilecode_amd import ops
    x, w, b, gy = orc.case_tensors(6)
    xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = ops.conv3d_s2(xg, wg)
    dx, dw = torch.autograd.grad(y, [xg, wg], gy.cuda())
    ref = orc.op_value_and_grads(x, w, torch.zeros_like(b), gy, None, torch.float64)
    yard = aten_yardstick()
    for q, g_ in (("y", y), ("d_x", dx), ("d_w", dw)):
        assert rel_err(g_, ref[q]) <= A * yard[q], q


@pytest.mark.parametrize("shape,C1,C2", [((1, 3, 5, 7), 8, 16), ((2, 1, 3, 3), 3, 5), ((1, 7, 9, 11), 4, 6), ((37,), 1, 2)])
def test_cat_channels_equals_torch_cat_and_its_split(shape, C1, C2):
    from smilecode_amd import ops
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(shape + (C1,), generator=g).cuda(), torch.randn(shape + (C2,), generator=g).cuda()
    go = torch.randn(shape + (C1 + C2,), generator=g).cuda()
    a.requires_grad_(True); b.requires_grad_(True)
    out = ops.cat_channels(a, b)
    assert torch.equal(out.detach(), torch.cat((a.detach(), b.detach()), -1))
    da, db = torch.autograd.grad(out, [a, b], go)
    assert torch.equal(da, go[..., :C1]) and torch.equal(db, go[..., C1:])
    b2 = b.detach()                                              # one side without a gradient: the other is still split out
    (da2,) = torch.autograd.grad(ops.cat_channels(a, b2), [a], go)
    assert torch.equal(da2, da)


def test_wrapper_refusals_name_the_argument():
    from smilecode_amd import ops
    x, w, b = torch.zeros(1, 4, 4, 4, 4).cuda(), torch.zeros(8, 4, 3, 3, 3).cuda(), torch.zeros(8).cuda()
    for args, word in (((x[..., :2].contiguous(), w[:, :2].contiguous(), b), "x has 2 channels"),
                       ((x, w[:6].contiguous(), b[:6].contiguous()), "6 output channels"),
                       ((x, w, b[:4].contiguous()), "bias"), ((x, w[:, :1].contiguous(), b), "weight"),
                       ((x[0], w, b), "x must be"), ((x, w, b, -0.1), "slope"), ((x.cpu(), w, b), "GPU")):
        with pytest.raises(RuntimeError, match=word):
            ops.conv3d_s2(*args)
    with pytest.raises(RuntimeError, match="cat_channels"):
        ops.cat_channels(x, x[:, :2].contiguous())
