"""-m gpu: the PCNet family's kernels (csrc/pcnet.hip) through smilecode_amd.ops against the same operators in ATen fp64 on the CPU
(tests/pcnet_oracle.py), measured in units of the error ATen fp32 makes on the CPU.

THE RULE (tests/test_gpu_deconv.py's): per operator and quantity, HIP's error against fp64 is at most A = 4 times the LARGEST
ATen-fp32 error of that quantity over the operator's frozen yardstick cases; a later case may use A times its OWN ATen-fp32 error
where that is larger.  An error is max|got - ref| / max|ref|.  Every measured figure goes to the parity report (tests.util.note_many)
before it is asserted.

THE ARGMAX CONDITION.  nff_fuse sends the max pool's gradient to ONE voxel per (sample, channel); where fp32 and fp64 pick
different voxels a comparison measures nothing.  Every nff case therefore plants its maxima (pcnet_oracle.nff_tensors: the winning
voxel is 1.5 x the runner-up), and the test asserts, per case, that the smallest relative gap between the two largest values of a
channel is at least 100 x ATen fp32's own relative error on the pooled tensor (the concatenation)."""
import functools

import pytest
import torch

from tests import pcnet_oracle as orc
from tests.util import note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0


def bounds(op, quantities, yard_cases, run, n):
    """quantity -> allowed error of case n: A x the frozen yardstick, and for a case outside it A x its own ATen error if larger"""
    yard = yardstick(op, quantities, yard_cases, run)
    if n in yard_cases:
        return {q: A * yard[q] for q in quantities}
    own = errors(run(n, torch.float32), run(n, torch.float64), quantities)
    note_many({"pcnet.%s.aten_f32[case%d].%s" % (op, n, q): v for q, v in own.items()})
    return {q: A * max(yard[q], own[q]) for q in quantities}


def errors(got, ref, quantities):
    return {q: rel_err(got[q], ref[q]) for q in quantities}


_YARD = {}


def yardstick(op, quantities, yard_cases, run):
    if op not in _YARD:
        worst = {q: 0.0 for q in quantities}
        for n in yard_cases:
            e = errors(run(n, torch.float32), run(n, torch.float64), quantities)
            worst = {q: max(worst[q], e[q]) for q in quantities}
        note_many({"pcnet.%s.aten_f32.%s" % (op, q): v for q, v in worst.items()})
        _YARD[op] = worst
    return _YARD[op]


def check(op, n, got, ref, bound, quantities):
    errs = errors(got, ref, quantities)
    note_many({"pcnet.%s[case%s].%s.e_hip" % (op, n, q): e for q, e in errs.items()})
    for q in quantities:
        assert got[q].shape == ref[q].shape and float(ref[q].abs().max()) > 0, (op, n, q)
        assert errs[q] <= bound[q], "%s case %s %s: e_hip %.3e, A x ATen fp32's error %.3e (A = %g)" % (op, n, q, errs[q], bound[q], A)


# ------------------------------------------------------------------------------------------------ upsample_pow2
UP_Q = ("out", "d_x")
UP_YARD = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def up_oracle(n, dtype):
    x, gy = orc.up_tensors(n)
    f = orc.UP_CASES[n][2]
    return orc.value_and_grads(lambda t: orc.upsample_pow2(t, f), {"x": x}, gy, dtype)


def up_hip(x, gy, f, ld=3, off=0, fill=None):
    from smilecode_amd import ops
    xg = x.cuda().requires_grad_(True)
    out = None
    if ld != 3 or fill is not None:
        B, d, h, w, _ = x.shape
        out = torch.full((B, f * d, f * h, f * w, ld), 7.0 if fill is None else fill, device="cuda")
    y = ops.upsample_pow2(xg, f, out, off)
    g = torch.zeros_like(y)
    g[..., off:off + 3] = gy.cuda()
    (dx,) = torch.autograd.grad(y, [xg], g)
    return {"out": y.detach()[..., off:off + 3], "d_x": dx, "row": y.detach()}


@pytest.mark.parametrize("n", sorted(orc.UP_CASES))
def test_upsample_against_fp64_in_units_of_aten_fp32(n):
    x, gy = orc.up_tensors(n)
    got = up_hip(x, gy, orc.UP_CASES[n][2])
    check("upsample", n, got, up_oracle(n, torch.float64), bounds("upsample", UP_Q, UP_YARD, up_oracle, n), UP_Q)


@pytest.mark.parametrize("ld,off", [(3, 0), (6, 0), (6, 3), (9, 0), (9, 3), (9, 6)])
def test_upsample_into_a_slice_leaves_the_rows_other_channels_untouched(ld, off):
    """the same bits as the plain call in channels [off, off + 3); every other channel of the row keeps its fill, and the gradient
    is read from the same slice (the other channels of d_y hold 0 here, NaN in the second run: neither is read)"""
    x, gy = orc.up_tensors(2)
    plain, got = up_hip(x, gy, 4), up_hip(x, gy, 4, ld, off, fill=7.0)
    assert torch.equal(got["out"], plain["out"]) and torch.equal(got["d_x"], plain["d_x"])
    keep = [c for c in range(ld) if not off <= c < off + 3]
    assert bool((got["row"][..., keep] == 7.0).all())
    from smilecode_amd import ops
    xg = x.cuda().requires_grad_(True)
    y = ops.upsample_pow2(xg, 4, torch.zeros(1, 8, 12, 20, ld, device="cuda"), off)
    g = torch.full_like(y, float("nan"))
    g[..., off:off + 3] = gy.cuda()
    assert torch.equal(torch.autograd.grad(y, [xg], g)[0], plain["d_x"])


def test_three_upsamplings_chain_through_one_buffer():
    """DFIBlock's cat(up8(p3), up4(p2), up2(p1)) in one 9-channel buffer: values and all three gradients equal the separate calls"""
    from smilecode_amd import ops
    g = orc.gen(7150)
    ps = [torch.randn(2, 2 * s, 3 * s, 2 * s, 3, generator=g) for s in (1, 2, 4)]
    gy = torch.randn(2, 16, 24, 16, 9, generator=g).cuda()
    leaves = [p.cuda().requires_grad_(True) for p in ps]
    buf = torch.empty(2, 16, 24, 16, 9, device="cuda")
    for i, (p, f) in enumerate(zip(leaves, (8, 4, 2))):
        buf = ops.upsample_pow2(p, f, buf, 3 * i)
    grads = torch.autograd.grad(buf, leaves, gy)
    for i, (p, f) in enumerate(zip(ps, (8, 4, 2))):
        one = up_hip(p, gy[..., 3 * i:3 * i + 3].cpu(), f)
        assert torch.equal(buf.detach()[..., 3 * i:3 * i + 3], one["out"]) and torch.equal(grads[i], one["d_x"]), i


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5))
def test_upsample_corners_are_the_inputs_corners(n):
    x, gy = orc.up_tensors(n)
    y = up_hip(x, gy, orc.UP_CASES[n][2])["out"].cpu()
    for cz in (0, -1):
        for cy in (0, -1):
            for cx in (0, -1):
                assert torch.equal(y[:, cz, cy, cx], x[:, cz, cy, cx])


@pytest.mark.parametrize("f", (2, 4, 8))
def test_upsample_delta_gradients_are_the_interpolation_weights(f):
    """d_y = 1 at one fine voxel, channel 1: d_x holds that voxel's weights, products of (1 - t, t) per axis with t = r / (f n - 1)
    from the integer remainder r -- eight of them for an interior voxel, four on the face o_z = 0 (t = 0 there: the far corners get
    exact zeros).  Each weight is a product of three factors that are each within half an ulp of the exact one (t is one
    correctly rounded division, 1 - t one subtraction of it: 2 roundings at most) and two multiplications: 8 roundings of 2^-24,
    so every weight is within 9 x 2^-24 of the fp64 product, and so is their sum of 1 (the 8 weights sum to at most 1)."""
    from smilecode_amd import ops
    B, (d, h, w) = 1, (2, 3, 5)
    x = torch.zeros(B, d, h, w, 3, device="cuda", requires_grad=True)
    for o in ((1, f + 1, 2 * f + 1), (0, f + 1, 2 * f + 1)):
        y = ops.upsample_pow2(x, f)
        g = torch.zeros_like(y)
        g[(0,) + o + (1,)] = 1.0
        (dx,) = torch.autograd.grad(y, [x], g)
        dx = dx.cpu().double()
        want = torch.zeros(d, h, w, dtype=torch.float64)
        axes = []
        for oi, n in zip(o, (d, h, w)):
            q, r = divmod(oi * (n - 1), f * n - 1)
            axes.append(((q, 1.0 - r / (f * n - 1)), (min(q + 1, n - 1), r / (f * n - 1))))
        for iz, wz in axes[0]:
            for iy, wy in axes[1]:
                for ix, wx in axes[2]:
                    want[iz, iy, ix] += wz * wy * wx
        assert int((want > 0).sum()) == (8 if o[0] else 4)
        assert float(dx[0, ..., 0].abs().max()) == 0.0 and float(dx[0, ..., 2].abs().max()) == 0.0
        assert bool((dx[0, ..., 1][want == 0] == 0).all())
        assert float((dx[0, ..., 1] - want).abs().max()) <= 9 * 2.0 ** -24
        assert abs(float(dx[0, ..., 1].sum()) - 1.0) <= 9 * 2.0 ** -24


def test_upsample_by_4_is_not_twice_by_2():
    from smilecode_amd import ops
    x = orc.up_tensors(1)[0].cuda()
    four, twice = ops.upsample_pow2(x, 4), ops.upsample_pow2(ops.upsample_pow2(x, 2), 2)
    assert four.shape == twice.shape and float((four - twice).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ dfi_gate
DFI_Q = ("out", "d_x", "d_logits")
DFI_YARD = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def dfi_oracle(n, dtype):
    x, lg, gy = orc.dfi_tensors(n)
    return orc.value_and_grads(orc.dfi_gate, {"x": x, "logits": lg}, gy, dtype)


def dfi_hip(x, lg, gy):
    from smilecode_amd import ops
    xg, lgg = x.cuda().requires_grad_(True), lg.cuda().requires_grad_(True)
    y = ops.dfi_gate(xg, lgg)
    dx, dl = torch.autograd.grad(y, [xg, lgg], gy.cuda())
    return {"out": y.detach(), "d_x": dx, "d_logits": dl}


@pytest.mark.parametrize("n", sorted(orc.DFI_CASES))
def test_dfi_gate_against_fp64_in_units_of_aten_fp32(n):
    check("dfi_gate", n, dfi_hip(*orc.dfi_tensors(n)), dfi_oracle(n, torch.float64), bounds("dfi_gate", DFI_Q, DFI_YARD, dfi_oracle, n), DFI_Q)


@pytest.mark.parametrize("n", sorted(orc.DFI_CASES))
def test_dfi_gate_zero_logits_halve_the_sum_bit_for_bit(n):
    """sigmoid(0) is exactly 0.5 and x holds integers in [-8, 8]: every product and sum is exact"""
    x, lg, gy = orc.dfi_tensors(n)
    x = torch.randint(-8, 9, x.shape, generator=orc.gen(7250 + n)).float()
    got = dfi_hip(x, torch.zeros_like(lg), gy)
    nf = orc.DFI_CASES[n][2]
    assert torch.equal(got["out"].cpu(), 0.5 * x.reshape(*x.shape[:-1], nf, 3).sum(-2))
    assert torch.equal(got["d_x"].cpu(), (0.5 * gy).repeat(1, 1, 1, 1, nf))


@pytest.mark.parametrize("n", sorted(orc.DFI_CASES))
def test_dfi_gate_saturated_logits_give_finite_gradients(n):
    x, lg, gy = orc.dfi_tensors(n)
    sat = torch.where(lg > 0, torch.full_like(lg, 30.0), torch.full_like(lg, -30.0))
    sat.view(-1)[:4] = torch.tensor([100.0, -100.0, 1000.0, -1000.0])
    got, ref = dfi_hip(x, sat, gy), orc.value_and_grads(orc.dfi_gate, {"x": x, "logits": sat}, gy, torch.float64)
    for q in DFI_Q:
        assert bool(torch.isfinite(got[q]).all()), q
    # 1 / (1 + exp(-30)) is 1 to fp32 and exp(-30) itself is far below 2^-24 of anything here: the values are x or 0 to an ulp
    assert rel_err(got["out"], ref["out"]) <= 2.0 ** -22 and rel_err(got["d_x"], ref["d_x"]) <= 2.0 ** -22
    assert float(got["d_logits"].abs().max()) <= 1e-11 * float(gy.abs().max() * x.abs().max())


# ------------------------------------------------------------------------------------------------ nff_fuse
NFF_Q = ("out", "d_t0", "d_t1", "d_t2", "d_logits", "d_W1", "d_W2")


@functools.lru_cache(maxsize=None)
def nff_oracle(n, dtype, plant="max"):
    *t, gy = orc.nff_tensors(n, plant=plant)
    return orc.value_and_grads(orc.nff_fuse, dict(zip(orc.NFF_NAMES, t)), gy, dtype)


def nff_oracle_max(n, dtype):
    return nff_oracle(n, dtype)


def nff_hip(t0, t1, t2, lg, W1, W2, gy, wrt=orc.NFF_NAMES):
    from smilecode_amd import ops
    t = {k: v.cuda().requires_grad_(k in wrt) for k, v in zip(orc.NFF_NAMES, (t0, t1, t2, lg, W1, W2))}
    y = ops.nff_fuse(*t.values())
    names = [k for k in t if k in wrt]
    g = torch.autograd.grad(y, [t[k] for k in names], gy.cuda())
    out = {"out": y.detach()}
    out.update({"d_" + k: v for k, v in zip(names, g)})
    return out


def assert_argmax_condition(n, plant="max"):
    """the smallest gap of the case (a planted tie's own channel excepted) is at least 100 x ATen fp32's relative error on cat"""
    t0, t1, t2, lg = orc.nff_tensors(n, plant=plant)[:4]
    gaps = orc.nff_gaps(t0, t1, t2, lg)
    if plant == "tie":
        assert float(gaps[:, 0].abs().max()) == 0.0
        gaps = gaps[:, 1:]
    e_cat = rel_err(orc.nff_cat(t0, t1, t2, lg), orc.nff_cat(*(t.double() for t in (t0, t1, t2, lg))))
    note_many({"pcnet.nff[case%d,%s].min_gap" % (n, plant): float(gaps.min()), "pcnet.nff[case%d,%s].aten_f32_cat" % (n, plant): e_cat})
    assert float(gaps.min()) >= 100.0 * e_cat, (n, float(gaps.min()), e_cat)


@pytest.mark.parametrize("n", sorted(orc.NFF_CASES))
def test_nff_fuse_against_fp64_in_units_of_aten_fp32(n):
    assert_argmax_condition(n)
    check("nff_fuse", n, nff_hip(*orc.nff_tensors(n)), nff_oracle(n, torch.float64),
          bounds("nff_fuse", NFF_Q, orc.NFF_YARD, nff_oracle_max, n), NFF_Q)


def test_nff_second_samples_maxima_are_at_other_voxels():
    """B = 2 measures the per-sample index arithmetic only if the two samples' winners differ"""
    for n in (2, 3, 5, 6):
        t0, t1, t2, lg = orc.nff_tensors(n)[:4]
        cat = orc.nff_cat(*(t.double() for t in (t0, t1, t2, lg)))
        at = cat.reshape(2, cat.shape[1], -1).argmax(-1)
        assert float((at[0] != at[1]).double().mean()) > 0.5, n


@pytest.mark.parametrize("n", (3, 6))
def test_nff_maxima_at_the_first_and_the_last_voxel(n):
    assert_argmax_condition(n, "ends")
    t = orc.nff_tensors(n, plant="ends")
    cat = orc.nff_cat(*(v.double() for v in t[:4]))
    at = cat.reshape(cat.shape[0], cat.shape[1], -1).argmax(-1)
    assert bool((at[:, 0] == 0).all()) and bool((at[:, 1] == cat[0, 0].numel() - 1).all())
    ref = nff_oracle(n, torch.float64, "ends")
    own = errors(nff_oracle(n, torch.float32, "ends"), ref, NFF_Q)
    yard = yardstick("nff_fuse", NFF_Q, orc.NFF_YARD, nff_oracle_max)
    check("nff_fuse", "%d,ends" % n, nff_hip(*t), ref, {q: A * max(yard[q], own[q]) for q in NFF_Q}, NFF_Q)


@pytest.mark.parametrize("n", (3, 6))
def test_nff_planted_tie_sends_the_gradient_to_the_lower_index(n):
    """two voxels of channel 0 hold the same maximum bit for bit: the fp64 oracle (ATen's adaptive_max_pool3d) sends the pooled
    gradient to the first, and so must the kernels -- d_t0 at the second voxel carries no max-pool term"""
    assert_argmax_condition(n, "tie")
    t = orc.nff_tensors(n, plant="tie")
    V = t[0][0, ..., 0].numel()
    lo, hi = orc.TIE_AT(V)
    cat = orc.nff_cat(*(v.double() for v in t[:4])).reshape(t[0].shape[0], -1, V)
    assert bool((cat[:, 0, lo] == cat[:, 0, hi]).all()) and bool((cat[:, 0].argmax(-1) == lo).all())
    ref, got = nff_oracle(n, torch.float64, "tie"), nff_hip(*t)
    own = errors(nff_oracle(n, torch.float32, "tie"), ref, NFF_Q)
    yard = yardstick("nff_fuse", NFF_Q, orc.NFF_YARD, nff_oracle_max)
    check("nff_fuse", "%d,tie" % n, got, ref, {q: A * max(yard[q], own[q]) for q in NFF_Q}, NFF_Q)
    B, C = t[0].shape[0], t[0].shape[-1]
    d64, dhip = ref["d_t0"].reshape(B, V, C), got["d_t0"].cpu().reshape(B, V, C)
    # the max-pool term lands on one of the two voxels only: HIP agrees with the oracle at both
    assert float((dhip[:, lo, 0].double() - d64[:, lo, 0]).abs().max()) <= 1e-4 * float(d64.abs().max())
    assert float((dhip[:, hi, 0].double() - d64[:, hi, 0]).abs().max()) <= 1e-4 * float(d64.abs().max())


def test_nff_inputs_without_a_gradient_launch_no_gradient_work():
    from smilecode_amd import ops
    t = orc.nff_tensors(3)
    full = nff_hip(*t)

    def tags(wrt):
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            got = nff_hip(*t, wrt=wrt)
        finally:
            ops.set_kernel_timer(None)
        return [r[0] for r in timer.records], got

    fwd = ["nff_pool[C4]", "nff_gate_fwd[C4]", "nff_apply_fwd[C4]"]
    names, got = tags(("W1", "W2"))
    assert names == fwd + ["nff_apply_bwd_gate[C4]", "nff_gate_bwd[C4]"], names
    assert torch.equal(got["d_W1"], full["d_W1"]) and torch.equal(got["d_W2"], full["d_W2"])
    names, got = tags(("t1",))
    assert names == fwd + ["nff_apply_bwd_gate[C4]", "nff_gate_bwd[C4]", "nff_apply_bwd[C4]"], names
    assert torch.equal(got["d_t1"], full["d_t1"]) and set(got) == {"out", "d_t1"}


# ------------------------------------------------------------------------------------------------ residual_add
@pytest.mark.parametrize("n", (1, 2, 3, 4, 1021, 4098, 4099))
def test_residual_add_with_every_tail(n):
    from smilecode_amd import ops
    g = orc.gen(7400 + n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ag, bg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    s = ops.residual_add(ag, bg)
    assert torch.equal(s.detach().cpu(), a + b)
    gs = torch.randn(n, generator=g).cuda()
    da, db = torch.autograd.grad(s, [ag, bg], gs)
    assert torch.equal(da, gs) and torch.equal(db, gs)


# ------------------------------------------------------------------------------------------------ all of them
def _pair(case_tensors, n):
    """the case's tensors with a batch of two (a one-sample case is stacked with a second, seeded one; weights are shared)"""
    t = case_tensors(n)
    if t[0].shape[0] == 2:
        return t
    u = case_tensors(n, seed=99)
    return tuple(a if a.dim() == 2 else torch.cat((a, b)) for a, b in zip(t, u))


@pytest.mark.parametrize("op,n", [("up", 3), ("up", 5), ("up", 6), ("dfi", 1), ("dfi", 3), ("nff", 2), ("nff", 4), ("nff", 5), ("nff", 6)])
def test_two_runs_are_bit_identical_and_a_batch_equals_its_samples(op, n):
    if op == "up":
        f = orc.UP_CASES[n][2]
        t, run, per_sample = _pair(orc.up_tensors, n), lambda *a: up_hip(*a, f), UP_Q
    elif op == "dfi":
        t, run, per_sample = _pair(orc.dfi_tensors, n), dfi_hip, DFI_Q
    else:
        t, run, per_sample = _pair(orc.nff_tensors, n), nff_hip, NFF_Q[:5]            # d_W1 / d_W2 are sums over the batch
    a, b = run(*t), run(*t)
    for q in a:
        assert torch.equal(a[q], b[q]), (op, n, q)
    for i in range(2):
        one = run(*(v if v.dim() == 2 else v[i:i + 1] for v in t))
        for q in per_sample:
            assert torch.equal(one[q], a[q][i:i + 1]), (op, n, q, i)


def test_wrapper_refusals_name_the_argument():
    from smilecode_amd import ops
    z = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    x = z(1, 2, 3, 5, 3)
    for bad, word in ((lambda: ops.upsample_pow2(x, 3), "f must be"), (lambda: ops.upsample_pow2(z(1, 1, 3, 5, 3), 2), "axis of 1"),
                      (lambda: ops.upsample_pow2(z(1, 2, 3, 5, 4), 2), "3 channels"), (lambda: ops.upsample_pow2(x[0], 2), "x must be"),
                      (lambda: ops.upsample_pow2(x, 2, z(1, 4, 6, 10, 6), 4), "offset"), (lambda: ops.upsample_pow2(x, 2, None, 3), "offset"),
                      (lambda: ops.upsample_pow2(x, 2, z(1, 4, 6, 10, 5)), "out"), (lambda: ops.upsample_pow2(x, 2, z(1, 4, 6, 9, 6)), "out"),
                      (lambda: ops.upsample_pow2(x.cpu(), 2), "GPU"),
                      (lambda: ops.dfi_gate(z(2, 5, 4), z(2, 5, 4)), "x "), (lambda: ops.dfi_gate(z(2, 5, 6), z(2, 5, 3)), "logits"),
                      (lambda: ops.dfi_gate(z(0, 6), z(0, 6)), "empty"),
                      (lambda: ops.residual_add(z(4), z(5)), "b "), (lambda: ops.residual_add(z(0), z(0)), "empty")):
        with pytest.raises(RuntimeError, match=word):
            bad()
    t, lg, W1, W2 = z(1, 2, 3, 2, 8), z(1, 2, 3, 2, 3), z(3, 24), z(24, 3)
    f = ops.nff_fuse
    for bad, word in ((lambda: f(t, t[..., :4].contiguous(), t, lg, W1, W2), "t1"), (lambda: f(t, t, t[:, :1].contiguous(), lg, W1, W2), "t2"),
                      (lambda: f(t, t, t, z(1, 2, 3, 2, 4), W1, W2), "logits"), (lambda: f(t, t, t, lg, z(2, 24), W2), "W1"),
                      (lambda: f(t, t, t, lg, W1, z(24, 2)), "W2"), (lambda: f(t[0], t, t, lg, W1, W2), "t0 must be"),
                      (lambda: f(z(1, 2, 3, 2, 6), z(1, 2, 3, 2, 6), z(1, 2, 3, 2, 6), lg, z(2, 18), z(18, 2)), "multiple of 4"),
                      (lambda: f(t.double(), t, t, lg, W1, W2), "float32")):
        with pytest.raises(RuntimeError, match=word):
            bad()
