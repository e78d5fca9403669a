"""-m gpu: WHAT the pool, upsample, layout, scale, CWM-tail and Adam kernels compute at their edges (tests/test_gpu_guard.py pins
WHERE they read and write).  Cases, seeded tensors and references: tests/small_ops.py; their premises: tests/test_cpu_small_ops.py.

No tolerance here is tuned to a kernel.  A comparison is either ``so.same`` (equal bits, against the same arithmetic in ATen-CPU
fp32) or ``so.within``: an error against ATen fp64 of at most A = 4 times the error ATen fp32 makes on the same inputs, the per-op
rule of tests/test_gpu_deconv.py and tests/test_gpu_resize.py.  The one 1e-5 figure is test_upsample_backward_separable's
(tests/test_gpu_ops.py); the Adam quantities measured beyond A are an open finding, each pinned at 1.35 x its measured ratio
(so.ADAM_A_OPEN).  Every measured figure, HIP's and ATen's, goes to the parity report before it is asserted."""
import pytest
import torch

from tests import guard
from tests import small_ops as so
from tests.util import note_many

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from smilecode_amd import ops as o
    return o


@pytest.fixture(scope="module")
def abi():
    """(library, check, stream) for the entry points no wrapper reaches with these arguments"""
    from smilecode_amd import _lib
    return _lib.load(), _lib.check, (lambda: torch.cuda.current_stream().cuda_stream)


def grad(outs, x, gs):
    """d_x for the (output, cotangent) pairs whose cotangent is not None; the graph is kept for the next subset"""
    pairs = [(o, g) for o, g in zip(outs, gs) if g is not None]
    (dx,) = torch.autograd.grad([o for o, _ in pairs], [x], [g for _, g in pairs], retain_graph=True)
    return dx


# ------------------------------------------------------------------------------------------------ 1. layout, scale, LeakyReLU'
@pytest.mark.parametrize("case", so.LAYOUT_CASES, ids=lambda c: "B%d_C%d_%dx%dx%d" % (c[0], c[1], *c[2]))
def test_layout_kernels_are_the_permutation(ops, case):
    B, C, s = case
    x, g = so.gauss(11, B, C, *s), so.gauss(12, B, *s, C)
    xd = x.cuda().requires_grad_(True)
    y = ops.to_channels_last(xd)
    assert so.same(y, so.to_cl_ref(x))
    (dx,) = torch.autograd.grad(y, [xd], g.cuda())                       # the backward is modet_cl_to_ncdhw
    assert so.same(dx, so.to_ncdhw_ref(g))
    gd = g.cuda().requires_grad_(True)
    z = ops.to_ncdhw(gd)
    assert so.same(z, so.to_ncdhw_ref(g))
    (dg,) = torch.autograd.grad(z, [gd], x.cuda())                       # ... and modet_ncdhw_to_cl
    assert so.same(dg, so.to_cl_ref(x))


def test_layout_of_one_channel_is_a_view(ops):
    x = so.gauss(13, 2, 1, 4, 5, 9).cuda()
    y = ops.to_channels_last(x)
    assert y.data_ptr() == x.data_ptr() and tuple(y.shape) == (2, 4, 5, 9, 1) and so.same(y, so.to_cl_ref(x.cpu()))
    z = ops.to_ncdhw(y)
    assert z.data_ptr() == x.data_ptr() and so.same(z, x)


@pytest.mark.parametrize("n", so.FLAT_N)
def test_scale_by_is_one_fp32_multiply(ops, n):
    x = so.gauss(20 + n % 1000, n)
    for s in so.SCALES:
        s32 = torch.tensor(s, dtype=torch.float32)
        assert so.same(ops._scale_by(x.cuda(), s32.cuda()), x * s32), s


@pytest.mark.parametrize("n", so.FLAT_N)
def test_lrelu_backward_bits(abi, n):
    L, check, stream = abi
    dy, y = so.lrelu_inputs(n)
    dyd, yd, dx = dy.cuda(), y.cuda(), torch.empty(n, device="cuda")
    check(L.modet_lrelu_bwd(dyd.data_ptr(), yd.data_ptr(), dx.data_ptr(), n, stream()), "lrelu_bwd")
    assert so.same(dx, so.lrelu_bwd_ref(dy, y))


def test_conv3d_with_activation_runs_lrelu_backward(ops, monkeypatch):
    from smilecode_amd import _lib
    px = guard.LibProxy(_lib.load())
    monkeypatch.setattr(_lib, "_lib", px)
    x = so.gauss(30, 1, 4, 6, 8, 8).cuda().requires_grad_(True)
    w = (0.1 * so.gauss(31, 8, 8, 3, 3, 3)).cuda().requires_grad_(True)
    b = (0.1 * so.gauss(32, 8)).cuda().requires_grad_(True)
    y = ops.conv3d(x, w, b, act=True)
    assert "modet_lrelu_bwd" not in px.names()
    torch.autograd.grad(y, [x, w, b], so.gauss(33, *y.shape).cuda())
    assert "modet_lrelu_bwd" in px.names()


# ------------------------------------------------------------------------------------------------ 2. pooling
def _pool_case(ops, kind, shape, seed):
    x, gy = so.data(kind, seed, *shape), so.data(kind, seed + 1, *so.pool_shape(shape))
    xd = x.cuda().requires_grad_(True)
    y = ops.avgpool2(xd)
    assert so.same(y, so.pool_ref(x)), ("forward", kind, shape)
    (dx,) = torch.autograd.grad(y, [xd], gy.cuda())
    assert so.same(dx, so.pool_bwd_ref(gy)), ("backward", kind, shape)


@pytest.mark.parametrize("kind", ("int", "gauss"))
@pytest.mark.parametrize("C", so.POOL_C)
def test_avgpool2_bits(ops, C, kind):
    for s in so.POOL_SHAPES:
        for B in so.POOL_B:
            _pool_case(ops, kind, (B,) + s + (C,), 40 + C + B)


def test_avgpool2_forward_second_trip(ops):
    x = so.gauss(50, *so.POOL_FWD_BIG)
    assert x.numel() // 8 // 4 > so.FLAT_CAP
    assert so.same(ops.avgpool2(x.cuda()), so.pool_ref(x))


def test_avgpool2_backward_second_trip(ops):
    assert torch.Size(so.POOL_BWD_BIG).numel() // 4 > so.FLAT_CAP
    gy = so.gauss(51, *so.pool_shape(so.POOL_BWD_BIG))
    xd = torch.zeros(so.POOL_BWD_BIG, device="cuda").requires_grad_(True)
    (dx,) = torch.autograd.grad(ops.avgpool2(xd), [xd], gy.cuda())
    assert so.same(dx, so.pool_bwd_ref(gy))


@pytest.mark.parametrize("kind", ("int", "gauss"))
def test_pool_tee_bits(ops, kind):
    for C, s, B in ((4, (2, 2, 2), 1), (12, (2, 4, 6), 3), (8, (6, 10, 14), 3)):
        shape = (B,) + s + (C,)
        x, gy, gx = so.data(kind, 60, *shape), so.data(kind, 61, *so.pool_shape(shape)), so.data(kind, 62, *shape)
        xd = x.cuda().requires_grad_(True)
        y, t = ops.pool_tee(xd)
        assert so.same(y, so.pool_ref(x)) and so.same(t, x) and t.data_ptr() == xd.data_ptr()
        assert so.same(grad((y, t), xd, (gy.cuda(), None)), so.pool_bwd_ref(gy))
        assert so.same(grad((y, t), xd, (None, gx.cuda())), gx)                       # returned untouched
        assert so.same(grad((y, t), xd, (gy.cuda(), gx.cuda())), so.pool_bwd_ref(gy, gx))


def _cotangents(kind, seed, shape, Bh, subset):
    gy, g = so.data(kind, seed, *so.pool_shape(shape)), so.data(kind, seed + 1, *shape)
    return tuple(t if on else None for t, on in zip((gy, g[:Bh].contiguous(), g[Bh:].contiguous()), subset))


@pytest.mark.parametrize("kind", ("int", "gauss"))
@pytest.mark.parametrize("Bh", (1, 2, 3))
def test_pool_tee_split_bits(ops, Bh, kind):
    shape = (4, 2, 4, 6, 8)
    x = so.data(kind, 70, *shape)
    xd = x.cuda().requires_grad_(True)
    outs = ops.pool_tee_split(xd, Bh)
    assert so.same(outs[0], so.pool_ref(x)) and so.same(outs[1], x[:Bh]) and so.same(outs[2], x[Bh:])
    for subset in so.SUBSETS:
        gs = _cotangents(kind, 71, shape, Bh, subset)
        dx = grad(outs, xd, tuple(None if g is None else g.cuda() for g in gs))
        assert so.same(dx, so.tee_split_bwd_ref(*gs, Bh, shape)), subset


@pytest.mark.parametrize("C", so.FUSED_C)
def test_fused_instnorm_pool_split_is_the_two_node_form(ops, C):
    for s in so.FUSED_SHAPES:
        shape = (4,) + s + (C,)
        x = so.gauss(80 + C, *shape)
        for Bh in (1, 2, 3):
            xa, xb = x.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
            fused = ops.instnorm_lrelu_pool_tee_split(xa, None, Bh)
            two = ops.pool_tee_split(ops.instnorm_lrelu(xb), Bh)
            for name, a, b in zip(("pooled", "first half", "second half"), fused, two):
                assert so.same(a, b), (name, shape, Bh)
            for subset in so.SUBSETS:
                gs = tuple(None if g is None else g.cuda() for g in _cotangents("gauss", 81, shape, Bh, subset))
                assert so.same(grad(fused, xa, gs), grad(two, xb, gs)), ("d_x", shape, Bh, subset)


# ------------------------------------------------------------------------------------------------ 3. upsample x2
def _fwd_matrix(ops, axis, n):
    return so.matrix_from_fwd(ops.upsample2(so.onehot_inputs(axis, n).cuda(), 2.0), axis)


def _bwd_direct(abi, gy, shape, scale):
    L, check, stream = abi
    B, d, h, w, C = shape
    gy, dx = gy.cuda(), torch.empty(shape, device="cuda")
    check(L.modet_upsample2_bwd(gy.data_ptr(), dx.data_ptr(), B, d, h, w, C, scale, stream()), "modet_upsample2_bwd")
    return dx


def _bwd_sep(abi, gy, shape, scale):
    L, check, stream = abi
    B, d, h, w, C = shape
    nb = L.modet_upsample2_bwd_sep_ws_bytes(B, d, h, w, C)
    assert nb > 0 and B * d * h * w >= so.SEP_MIN
    gy, dx, ws = gy.cuda(), torch.empty(shape, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda")
    check(L.modet_upsample2_bwd_sep(gy.data_ptr(), dx.data_ptr(), ws.data_ptr(), nb, B, d, h, w, C, scale, stream()), "modet_upsample2_bwd_sep")
    return dx


def _check_matrix(W, n, what):
    assert so.rows_are_two_adjacent(W), what
    assert float(W.min()) >= 0.0 and float(W.max()) <= 1.0, what
    if n == 1:
        assert so.same(W, torch.ones(2, 1)), what


@pytest.mark.parametrize("n", so.UP_N + so.UP_N_SEP)
def test_upsample_kernels_share_one_weight_matrix(ops, abi, n):
    """(a) the forward, the direct gather and (large n) the three-pass backward: one matrix, bit for bit; (b) against fp64"""
    rep, worst = {}, 0.0
    for axis in range(3):
        shape = (2 * n,) + so.axis_shape(axis, n) + (1,)
        gy = so.onehot_cotangents(axis, n)
        Wf = _fwd_matrix(ops, axis, n)
        Wb = so.matrix_from_bwd(_bwd_direct(abi, gy, shape, 2.0), axis)
        _check_matrix(Wf, n, ("forward", axis))
        assert so.same(Wf, Wb), ("forward vs direct gather", axis, int((Wf != Wb).sum()), float((Wf - Wb).abs().max()))
        if n in so.UP_N_SEP:
            Ws = so.matrix_from_bwd(_bwd_sep(abi, gy, shape, 2.0), axis)
            assert so.same(Wf, Ws), ("forward vs three-pass", axis, int((Wf != Ws).sum()), float((Wf - Ws).abs().max()))
        else:
            # the autograd node takes the direct gather below the three-pass form's minimum
            assert 2 * n * n < so.SEP_MIN
            x2 = torch.zeros(shape, device="cuda").requires_grad_(True)
            (dx,) = torch.autograd.grad(ops.upsample2(x2, 2.0), [x2], gy.cuda())
            assert so.same(so.matrix_from_bwd(dx, axis), Wf), ("autograd", axis)
        e = so.matrix_err(Wf, n)
        rep["small_ops.upsample.matrix[n%d,axis%d].e_hip" % (n, axis)] = e
        worst = max(worst, e)
    e_f32, bound = so.matrix_err(so.aten_matrix(n, torch.float32), n), so.matrix_bound(n)
    rep["small_ops.upsample.matrix[n%d].aten_f32" % n] = e_f32
    rep["small_ops.upsample.matrix.aten_f32_frozen"] = so.matrix_yardstick()
    note_many(rep)
    assert worst <= bound, "n = %d: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (n, worst, bound, so.A)


def _hip_up(ops, x, gy, scale):
    xd = x.cuda().requires_grad_(True)
    y = ops.upsample2(xd, scale)
    (dx,) = torch.autograd.grad(y, [xd], gy.cuda())
    return {"out": y.detach(), "d_x": dx}


def _held_to_fp64(tag, case, got):
    ref, bound, own = so.up_reference(case), so.up_bound(case), so.up_own(case)
    errs = {q: so.rel_err(got[q], ref[q]) for q in got}
    rep = {"small_ops.upsample[%s].%s.e_hip" % (tag, q): e for q, e in errs.items()}
    rep.update({"small_ops.upsample[%s].%s.aten_f32" % (tag, q): own[q] for q in got})
    rep.update({"small_ops.upsample.aten_f32_frozen.%s" % q: v for q, v in so.up_yardstick().items()})
    note_many(rep)
    for q in got:
        assert got[q].shape == ref[q].shape
        assert errs[q] <= bound[q], "%s %s: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (tag, q, errs[q], bound[q], so.A)


def _tag(case):
    (d, h, w), C, B, scale = case
    return "%dx%dx%d_C%d_B%d_s%g" % (d, h, w, C, B, scale)


@pytest.mark.parametrize("shape", so.UP_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_upsample_against_fp64_in_units_of_aten_fp32(ops, shape):
    for case in so.UP_CASES:
        if case[0] != shape:
            continue
        x, gy = so.up_tensors(case)
        got = _hip_up(ops, x, gy, case[3])
        _held_to_fp64(_tag(case), case, got)
        again = _hip_up(ops, x, gy, case[3])
        assert all(so.same(got[q], again[q]) for q in got), ("two runs", case)
        if case[2] == 2:                                                 # a batch of two equals its two samples
            for i in range(2):
                one = _hip_up(ops, x[i:i + 1].contiguous(), gy[i:i + 1].contiguous(), case[3])
                assert all(so.same(one[q], got[q][i:i + 1]) for q in got), ("sample", i, case)
    if shape == (1, 1, 1):                                               # both ratios are 0: the voxel, eight times, scaled
        x, gy = so.up_tensors((shape, 3, 2, 2.0))
        got = _hip_up(ops, x, gy, 2.0)
        assert so.same(got["out"], (2.0 * x).expand(2, 2, 2, 2, 3).contiguous())


@pytest.mark.parametrize("case", so.UP_SEP_CASES, ids=_tag)
def test_upsample_three_pass_backward_with_a_thin_axis(ops, abi, case):
    (d, h, w), C, B, scale = case
    x, gy = so.up_tensors(case)
    assert abi[0].modet_upsample2_bwd_sep_ws_bytes(B, d, h, w, C) > 0      # the autograd node takes the three-pass form
    got = _hip_up(ops, x, gy, scale)
    _held_to_fp64(_tag(case), case, got)
    direct = _bwd_direct(abi, gy, (B, d, h, w, C), scale)
    diff, big = float((direct - got["d_x"]).abs().max()), max(1.0, float(direct.abs().max()))
    note_many({"small_ops.upsample[%s].sep_vs_direct" % _tag(case): diff / big})
    assert diff <= 1e-5 * big
    assert so.same(_bwd_sep(abi, gy, (B, d, h, w, C), scale), got["d_x"])


def test_upsample_forward_second_trip(ops):
    case = so.UP_FWD_BIG
    (d, h, w), C, B, scale = case
    assert B * 8 * d * h * w * (C // 4) > so.FLAT_CAP
    x, gy = so.up_tensors(case)
    _held_to_fp64(_tag(case), case, {"out": ops.upsample2(x.cuda(), scale)})


def test_upsample_direct_backward_second_trip(abi):
    case = so.UP_BWD_BIG
    (d, h, w), C, B, scale = case
    assert B * d * h * w * (C // 4) > so.FLAT_CAP // 8
    x, gy = so.up_tensors(case)
    _held_to_fp64(_tag(case), case, {"d_x": _bwd_direct(abi, gy, (B, d, h, w, C), scale)})


# ------------------------------------------------------------------------------------------------ 4. CWM tail with one head
@pytest.mark.parametrize("N", so.FLAT_N)
def test_cwm_tail_with_one_head_doubles(ops, N):
    x, lg, dout = so.gauss(90, N, 3), 5.0 * so.gauss(91, N, 1), so.gauss(92, N, 3)
    xd, ld = x.cuda().requires_grad_(True), lg.cuda().requires_grad_(True)
    out = ops.cwm_tail(xd, ld)
    assert so.same(out, 2.0 * x)
    dx, dl = torch.autograd.grad(out, [xd, ld], dout.cuda())
    assert so.same(dx, 2.0 * dout) and so.same(dl, torch.zeros(N, 1))


# ------------------------------------------------------------------------------------------------ 5. Adam with AMSGrad
def _hip_adam(ops, name, n, grads=None, grad_scale=None, lr=None, upto=None):
    c = so.ADAM_CASES[name]
    p0, gs = so.adam_tensors(name, n)
    gs = gs if grads is None else grads
    p, m, v, vm = p0.cuda().clone(), torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    out = []
    for k, g in enumerate(gs[:upto]):
        ops.adam_amsgrad_step_(p, g.cuda(), m, v, vm, c["lr"] if lr is None else lr, c["step0"] + k,
                               grad_scale=c["grad_scale"] if grad_scale is None else grad_scale)
        out.append({"p": p.clone(), "m": m.clone(), "v": v.clone(), "vmax": vm.clone()})
    return out


def _adam_rule(ops, name, n):
    got = _hip_adam(ops, name, n)
    errs, yard, own = so.adam_errors(got, name, n), so.adam_yardstick(name, n), so.adam_own(name, n)
    rep = {}
    for (q, k), e in errs.items():
        rep["small_ops.adam[%s,n%d].%s.step%d.e_hip" % (name, n, q, k)] = e
        rep["small_ops.adam[%s,n%d].%s.step%d.aten_f32" % (name, n, q, k)] = own[(q, k)]
        rep["small_ops.adam[%s].%s.step%d.aten_f32_of_the_case" % (name, q, k)] = yard[(q, k)]
    for q in so.adam_measured(name):
        rep["small_ops.adam[%s,n%d].%s.worst_e_hip_over_e_f32" % (name, n, q)] = max(errs[(q, k)] / yard[(q, k)] for k in range(so.ADAM_STEPS))
    note_many(rep)
    bad = [(q, k) for (q, k) in errs if q in so.adam_measured(name) and not so.within(errs[(q, k)], yard[(q, k)], so.adam_a(name, q))]
    assert not bad, "%s, n = %d: beyond A x ATen fp32's error in " % (name, n) + "; ".join(
        "%s after step %d: e_hip %.3e, e_f32 %.3e (A = %g)" % (q, k, errs[(q, k)], yard[(q, k)], so.adam_a(name, q)) for q, k in bad)
    for k in range(1, so.ADAM_STEPS):                                    # AMSGrad's maximum on the kernel's own v
        assert so.same(got[k]["vmax"], torch.maximum(got[k - 1]["vmax"], got[k]["v"])), (name, n, k)
    assert so.same(got[0]["vmax"], got[0]["v"])
    assert not so.same(got[1]["vmax"], got[1]["v"]) or n == 1            # the second step keeps the old maximum somewhere


@pytest.mark.parametrize("n", so.ADAM_N)
@pytest.mark.parametrize("name", sorted(so.ADAM_CASES))
def test_adam_against_fp64_in_units_of_aten_fp32(ops, name, n):
    _adam_rule(ops, name, n)


def test_adam_second_trip(ops):
    _adam_rule(ops, "unit", so.ADAM_N_BIG)


@pytest.mark.parametrize("n", so.ADAM_N)
def test_adam_grad_scale_is_the_fp32_multiply(ops, n):
    """grad_scale = 0.37 against gradients multiplied by 0.37 in fp32 beforehand and grad_scale = 1: the same bits"""
    s = so.ADAM_CASES["unit"]["grad_scale"]
    pre = [g * torch.tensor(s, dtype=torch.float32) for g in so.adam_tensors("unit", n)[1]]
    a, b = _hip_adam(ops, "unit", n), _hip_adam(ops, "unit", n, grads=pre, grad_scale=1.0)
    for k in range(so.ADAM_STEPS):
        assert all(so.same(a[k][q], b[k][q]) for q in so.ADAM_QUANTITIES), k


@pytest.mark.parametrize("n", so.ADAM_N)
def test_adam_with_zero_learning_rate_leaves_p(ops, n):
    p0 = so.adam_tensors("p0", n)[0]
    frozen, moving = _hip_adam(ops, "p0", n, lr=0.0), _hip_adam(ops, "p0", n)
    for k in range(so.ADAM_STEPS):
        assert so.same(frozen[k]["p"], p0), k
        assert all(so.same(frozen[k][q], moving[k][q]) for q in ("m", "v", "vmax")), k     # the state still advances
        assert float(frozen[k]["m"].abs().max()) > 0 and float(frozen[k]["v"].max()) > 0
        assert not so.same(moving[k]["p"], p0)


@pytest.mark.parametrize("n", so.ADAM_N)
def test_adam_with_zero_gradient_from_zero_state(ops, n):
    for name in ("unit", "p0"):
        p0 = so.adam_tensors(name, n)[0]
        got = _hip_adam(ops, name, n, grads=[torch.zeros(n)] * 2)
        for st in got:
            assert so.same(st["p"], p0) and all(so.same(st[q], torch.zeros(n)) for q in ("m", "v", "vmax"))
