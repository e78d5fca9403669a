"""-m gpu: the trilinear resize kernels (csrc/resize.hip) on the MI355X against F.interpolate(mode='trilinear', align_corners=True)
times the scale in ATen fp64, measured in units of the error the same composition makes in ATen fp32 on the CPU.

THE RULE (tests/test_gpu_deconv.py's): per quantity (out, d_x), HIP's error against fp64 is at most A = 4 times the LARGEST
ATen-fp32 error of that quantity over cases 1 .. 7 of tests/rdn_stages_oracle.py OP_CASES (YARD_CASES: the yardstick is frozen to
them, a later case cannot raise it).  A case from 8 on and a pyramid case may use A times its OWN ATen-fp32 error instead where
that is larger.  An error is max|got - ref| / max|ref|.  The operator is linear with fixed weights: no masking is needed.  Every
measured figure, HIP's and ATen's, goes to the parity report (tests.util.note_many) before it is asserted."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import rdn_stages_oracle as orc
from tests.util import note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
QUANTITIES = ("out", "d_x")
CASES = tuple(sorted(orc.OP_CASES))
PCASES = tuple(sorted(orc.PYRAMID_CASES))


def aten(x, gy, size, scale, dtype):
    """{out, d_x} of scale * F.interpolate in ``dtype`` on the CPU, channels-last"""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    y = scale * F.interpolate(xr.permute(0, 4, 1, 2, 3), size=size, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
    (dx,) = torch.autograd.grad(y, [xr], gy.to(dtype))
    return {"out": y.detach().contiguous(), "d_x": dx}


@functools.lru_cache(maxsize=None)
def reference(n):
    """(tensors, fp64 results) of a case: computed once, shared, never modified"""
    t = orc.case_tensors(n)
    return t, aten(*t, orc.OP_CASES[n][2], orc.OP_CASES[n][4], torch.float64)


@functools.lru_cache(maxsize=None)
def aten_yardstick():
    worst = {q: 0.0 for q in QUANTITIES}
    for n in orc.YARD_CASES:
        t, ref = reference(n)
        got = aten(*t, orc.OP_CASES[n][2], orc.OP_CASES[n][4], torch.float32)
        for q in QUANTITIES:
            worst[q] = max(worst[q], rel_err(got[q], ref[q]))
    note_many({"resize.aten_f32.%s" % q: v for q, v in worst.items()})
    return worst


@functools.lru_cache(maxsize=None)
def allowed(n):
    yard = aten_yardstick()
    if n in orc.YARD_CASES:
        return {q: A * yard[q] for q in QUANTITIES}
    t, ref = reference(n)
    got = aten(*t, orc.OP_CASES[n][2], orc.OP_CASES[n][4], torch.float32)
    own = {q: rel_err(got[q], ref[q]) for q in QUANTITIES}
    note_many({"resize.aten_f32[case%d].%s" % (n, q): v for q, v in own.items()})
    return {q: A * max(yard[q], own[q]) for q in QUANTITIES}


def hip(x, gy, size, scale):
    from smilecode_amd import ops
    x, gy = x.cuda().requires_grad_(True), gy.cuda()
    y = ops.resize(x, size, scale)
    (dx,) = torch.autograd.grad(y, [x], gy)
    return {"out": y.detach(), "d_x": dx}


@pytest.mark.parametrize("n", CASES)
def test_resize_against_fp64_in_units_of_aten_fp32(n):
    (t, ref), bound = reference(n), allowed(n)
    got = hip(*t, orc.OP_CASES[n][2], orc.OP_CASES[n][4])
    errs = {q: rel_err(got[q], ref[q]) for q in QUANTITIES}
    note_many({"resize[case%d].%s.e_hip" % (n, q): e for q, e in errs.items()})
    for q in QUANTITIES:
        assert got[q].shape == ref[q].shape
        assert errs[q] <= bound[q], "case %d %s: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (n, q, errs[q], bound[q], A)


def test_integer_ratios_pick_voxels_bit_for_bit():
    """case 1: the ratios are 2, 4 and 32, every l is 0: out = 0.5 x[::2, ::4, ::32], d_x = 0.5 gy there and exactly 0 elsewhere"""
    x, gy = orc.case_tensors(1)
    got = hip(x, gy, (5, 4, 2), 0.5)
    assert torch.equal(got["out"].cpu(), 0.5 * x[:, ::2, ::4, ::32])
    want = torch.zeros_like(x)
    want[:, ::2, ::4, ::32] = 0.5 * gy
    assert torch.equal(got["d_x"].cpu(), want)


def test_identity_only_scales_bit_for_bit():
    x, gy = orc.case_tensors(8)
    got = hip(x, gy, (6, 6, 6), 0.25)
    assert torch.equal(got["out"].cpu(), 0.25 * x) and torch.equal(got["d_x"].cpu(), 0.25 * gy)


def test_scalar_path_on_a_view_offset_by_one_float():
    """case 10 (C = 6: never 16-byte rows) once more with x, out and both gradients' sources 4 bytes off a 16-byte boundary, and
    case 5 (C = 4) there too: the library must take the scalar path and give the aligned run's bits"""
    from smilecode_amd import _lib
    L = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    for n in (10, 5):
        B, si, so, C, scale = orc.OP_CASES[n]
        x, gy = orc.case_tensors(n)
        want = hip(x, gy, so, scale)

        def off(t):
            buf = torch.zeros(t.numel() + 1, device="cuda")
            v = buf[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
            return v
        xo, gyo, yo, dxo = off(x), off(gy), off(torch.zeros_like(gy)), off(torch.zeros_like(x))
        _lib.check(L.modet_resize_fwd(xo.data_ptr(), yo.data_ptr(), B, *si, *so, C, scale, s), "resize fwd")
        _lib.check(L.modet_resize_bwd(gyo.data_ptr(), dxo.data_ptr(), B, *si, *so, C, scale, s), "resize bwd")
        assert torch.equal(yo, want["out"]) and torch.equal(dxo, want["d_x"]), n


@pytest.mark.parametrize("n", CASES)
def test_two_runs_are_bit_identical_and_a_batch_equals_its_samples(n):
    B, si, so, C, scale = orc.OP_CASES[n]
    x, gy = orc.case_tensors(n)
    if B == 1:                                                   # one sample: stack it with a second, seeded one
        u = orc.case_tensors(n, seed=77 + n)
        x, gy = torch.cat((x, u[0])), torch.cat((gy, u[1]))
    a, b = hip(x, gy, so, scale), hip(x, gy, so, scale)
    for q in QUANTITIES:
        assert torch.equal(a[q], b[q]), (n, q)
    for i in range(2):
        one = hip(x[i:i + 1], gy[i:i + 1], so, scale)
        assert torch.equal(one["out"], a["out"][i:i + 1]) and torch.equal(one["d_x"], a["d_x"][i:i + 1]), (n, i)


# ------------------------------------------------------------------------------------------------ the pyramid
def _ptr(t):
    return None if t is None else t.data_ptr()


def pyramid_fwd(x, want=(True, True, True), fill=None):
    """the C ABI directly: outputs not wanted are passed as NULL; ``fill``: the value the buffers hold before the call"""
    from smilecode_amd import _lib, ops
    B, D, H, W, _ = x.shape
    ys = [torch.full((B,) + s + (3,), fill, device="cuda") if fill is not None else torch.empty((B,) + s + (3,), device="cuda")
          for s in ops.flow_pyramid_sizes(D, H, W)]
    _lib.check(_lib.load().modet_resize_pyramid_fwd(x.data_ptr(), *(_ptr(y) if w else None for y, w in zip(ys, want)), B, D, H, W,
                                                    torch.cuda.current_stream().cuda_stream), "pyramid fwd")
    return ys


def pyramid_bwd(shape, gys, add=None, into=None):
    from smilecode_amd import _lib
    B, D, H, W, _ = shape
    dx = torch.empty(shape, device="cuda") if into is None else into
    _lib.check(_lib.load().modet_resize_pyramid_bwd(_ptr(gys[0]), _ptr(gys[1]), _ptr(gys[2]), _ptr(add), dx.data_ptr(), B, D, H, W,
                                                    torch.cuda.current_stream().cuda_stream), "pyramid bwd")
    return dx


@functools.lru_cache(maxsize=None)
def pyramid_reference(n):
    """fp64 and fp32 ATen gradients of the three rescaled downsamplings, summed: (d_x fp64, its ATen-fp32 error)"""
    x, g2, g4, g8, _ = orc.pyramid_tensors(n)
    out = {}
    for dtype in (torch.float64, torch.float32):
        total = None
        for gy, (f, sc) in zip((g2, g4, g8), orc.PYRAMID):
            d = aten(x, gy, tuple(gy.shape[1:4]), sc, dtype)["d_x"]
            total = d if total is None else total + d
        out[dtype] = total
    return out[torch.float64], rel_err(out[torch.float32], out[torch.float64])


@pytest.mark.parametrize("n", PCASES)
def test_pyramid_outputs_hold_the_bits_of_the_single_call(n):
    from smilecode_amd import ops
    x = orc.pyramid_tensors(n)[0].cuda()
    ys = pyramid_fwd(x)
    for y, (f, sc) in zip(ys, orc.PYRAMID):
        assert torch.equal(y, ops.resize(x, tuple(y.shape[1:4]), sc)), (n, f)
    again = pyramid_fwd(x)
    assert all(torch.equal(a, b) for a, b in zip(ys, again))
    via_op = ops.flow_pyramid(x)
    assert all(torch.equal(a, b) for a, b in zip(ys, via_op))
    # a NULL output is left unwritten, the others are what they were
    for skip in range(3):
        part = pyramid_fwd(x, want=tuple(i != skip for i in range(3)), fill=7.0)
        for i in range(3):
            assert torch.equal(part[i], torch.full_like(part[i], 7.0) if i == skip else ys[i]), (n, skip, i)


@pytest.mark.parametrize("n", PCASES)
def test_pyramid_backward(n):
    from smilecode_amd import ops
    x, g2, g4, g8, add = (t.cuda() for t in orc.pyramid_tensors(n))
    gys = (g2, g4, g8)
    ref, own = pyramid_reference(n)
    bound = A * max(aten_yardstick()["d_x"], own)
    dx = pyramid_bwd(x.shape, gys)
    e = rel_err(dx, ref)
    ref_add = ref + orc.pyramid_tensors(n)[4].double()
    dx_add = pyramid_bwd(x.shape, gys, add=add)
    aliased = add.clone()
    pyramid_bwd(x.shape, gys, add=aliased, into=aliased)                 # d_x_add aliases d_x
    e_add = rel_err(dx_add, ref_add)
    note_many({"resize.pyramid[case%d].aten_f32.d_x" % n: own, "resize.pyramid[case%d].d_x.e_hip" % n: e,
               "resize.pyramid[case%d].d_x_add.e_hip" % n: e_add})
    assert e <= bound, "pyramid %d d_x: e_hip %.3e, bound %.3e" % (n, e, bound)
    assert e_add <= bound, "pyramid %d d_x with d_x_add: e_hip %.3e, bound %.3e" % (n, e_add, bound)
    assert torch.equal(aliased, dx_add)
    # a single cotangent and no d_x_add: the bits of modet_resize_bwd
    for i, (gy, (f, sc)) in enumerate(zip(gys, orc.PYRAMID)):
        only = pyramid_bwd(x.shape, tuple(g if j == i else None for j, g in enumerate(gys)))
        xr = x.clone().requires_grad_(True)
        (single,) = torch.autograd.grad(ops.resize(xr, tuple(gy.shape[1:4]), sc), [xr], gy)
        assert torch.equal(only, single), (n, f)
    # the autograd node: all three cotangents in one launch, and only the ones that arrive
    xr = x.clone().requires_grad_(True)
    (d_all,) = torch.autograd.grad(ops.flow_pyramid(xr), [xr], gys)
    assert torch.equal(d_all, dx)
    xr = x.clone().requires_grad_(True)
    f2, f4, f8 = ops.flow_pyramid(xr)
    (d_4,) = torch.autograd.grad([f4], [xr], [g4])
    assert torch.equal(d_4, pyramid_bwd(x.shape, (None, g4, None)))
    assert torch.equal(pyramid_bwd(x.shape, gys), dx)                   # two runs, the same bits


def test_pyramid_batch_of_two_equals_two_batches_of_one():
    x, g2, g4, g8, _ = (t.cuda() for t in orc.pyramid_tensors(2))       # B = 2, down to 1 x 1 x 1
    ys, dx = pyramid_fwd(x), pyramid_bwd(x.shape, (g2, g4, g8))
    assert tuple(ys[2].shape) == (2, 1, 1, 1, 3)
    for i in range(2):
        one = pyramid_fwd(x[i:i + 1].contiguous())
        assert all(torch.equal(a, b[i:i + 1]) for a, b in zip(one, ys)), i
        d1 = pyramid_bwd((1,) + tuple(x.shape[1:]), tuple(g[i:i + 1].contiguous() for g in (g2, g4, g8)))
        assert torch.equal(d1, dx[i:i + 1]), i


def test_calls_captured_into_a_graph_replay_equal_to_eager():
    from smilecode_amd import ops
    x, gy = (t.cuda() for t in orc.case_tensors(2))
    px, g2, g4, g8, _ = (t.cuda() for t in orc.pyramid_tensors(1))
    so, scale = orc.OP_CASES[2][2], orc.OP_CASES[2][4]

    def run():
        xr, pr = x.clone().requires_grad_(True), px.clone().requires_grad_(True)
        y = ops.resize(xr, so, scale)
        fs = ops.flow_pyramid(pr)
        dx, dp = torch.autograd.grad([y, *fs], [xr, pr], [gy, g2, g4, g8])
        return [y.detach(), dx, dp] + [f.detach() for f in fs]

    eager = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                            # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for _ in range(2):
        for t in captured:
            t.fill_(-3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))


def test_wrapper_refusals_name_the_argument():
    from smilecode_amd import ops
    x = torch.zeros(1, 8, 8, 8, 3).cuda()
    for fn, word in ((lambda: ops.resize(x.cpu(), (4, 4, 4)), "GPU"), (lambda: ops.resize(x, (4, 4)), "size"),
                     (lambda: ops.resize(x[:0], (4, 4, 4)), "empty"), (lambda: ops.flow_pyramid(x[:, :7].contiguous()), "at least 8"),
                     (lambda: ops.flow_pyramid(torch.zeros(1, 8, 8, 8, 4).cuda()), "3 channels")):
        with pytest.raises(RuntimeError, match=word):
            fn()
