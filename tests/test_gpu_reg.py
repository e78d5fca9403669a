"""-m gpu: the flow regularisers of csrc/reg.hip against fp64 (the reference's recorded results of tests/golden/op_reg.npz, and the
restatement of tests/reg_oracle.py for the larger flows), in both layouts; zero and constant flows; bit-reproducibility; hipGraph
capture of a step with the term, the seeded against the autograd path, and the end-to-end parameter gradients against the fp64
oracle model.

The parity bound is not a chosen number (as in tests/test_gpu_ssim.py): every (case, kind) is also evaluated with the restatement
in fp32 on the CPU, the ATen composition, whose own error against fp64 is measured; the HIP result has to stay within A = 4 times
the LARGEST such error over this file's cases, per quantity (another summation order plus one noisy ATen sample).  Where the fp64
value is exactly 0 (the zero flow) only an exact 0 is within a relative bound: the error is 0 for one and infinite otherwise.
The errors of every case are in the report.  The shapes put every voxel in bending's 4-voxel shell (5^3, 6 x 7 x 9), have a first
interior voxel (9^3), rows longer than a wave in either layout (37, 67), more than one workgroup (12 x 20 x 28 x 2, 32 x 48 x 32)
and the minimum sizes of every kind."""
import functools

import numpy as np
import pytest
import torch

from tests import reg_oracle
from tests.util import gold, grad_yardstick, note_many

pytestmark = pytest.mark.gpu

A = 4.0
ALL = ("itv", "gradient-l2", "gradient-l1", "bending")
GOLDEN = ("noise2x3x5x5x5", "noise1x3x6x7x9", "noise1x3x9x9x9", "smooth1x3x8x10x37", "slab1x3x7x8x9", "zero1x3x6x6x6", "itv2x2x2x3x4",
          "itv1x1x4x5x6")
# restatement-only cases: (shape, batch, kinds), standard normal flows
SYNTH = {"rand12x20x28_B2": ((12, 20, 28), 2, ALL), "rand3x27x67": ((3, 27, 67), 1, ("itv",)),
         "rand5x27x67": ((5, 27, 67), 1, ALL[1:]), "rand32x48x32": ((32, 48, 32), 1, ALL)}
QUANTITIES = ("loss", "grad")


def _inputs(tag):
    """(planar flow on the host, kinds)"""
    if tag in GOLDEN:
        g = gold("op_reg.npz")
        return torch.from_numpy(g[tag + ".f"]), [str(k) for k in g[tag + ".kinds"]]
    shape, batch, kinds = SYNTH[tag]
    gen = torch.Generator().manual_seed(67)
    return torch.randn((batch, 3) + shape, generator=gen), list(kinds)


def _fp64(tag, kind, f):
    if tag in GOLDEN:
        g = gold("op_reg.npz")
        return tuple(torch.from_numpy(np.ascontiguousarray(g["%s.%s.%s" % (tag, kind, q)])).double() for q in ("loss", "grad"))
    return reg_oracle.value_and_grad(reg_oracle.KINDS[kind], f, torch.float64)


def _rel(err, ref):
    return 0.0 if err == 0.0 else (err / ref if ref > 0.0 else float("inf"))


def _errors(loss, grad, ref):
    l64, g64 = ref
    return {"loss": _rel(abs(float(loss.detach()) - float(l64)), abs(float(l64))),
            "grad": _rel(float((grad.double().cpu() - g64).abs().max()), float(g64.abs().max()))}


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _measured():
    """(case, kind) -> {"aten": errors of the fp32 ATen composition on the CPU, "hip": errors of the HIP path (planar), "cl": the
    largest difference between the channels-last gradient and the planar one}, each against fp64: loss relative, gradient
    max|err| over all elements / max|g64|"""
    from smilecode_amd import ops
    out = {}
    for tag in GOLDEN + tuple(SYNTH):
        f, kinds = _inputs(tag)
        for kind in kinds:
            ref = _fp64(tag, kind, f)
            aten = _errors(*reg_oracle.value_and_grad(reg_oracle.KINDS[kind], f, torch.float32), ref)
            fd = f.cuda().requires_grad_(True)
            loss = ops.reg_loss(fd, kind)
            (grad,) = torch.autograd.grad(loss, [fd])
            assert loss.shape == () and grad.shape == f.shape
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), (tag, kind)
            assert torch.equal(ops.reg_loss(fd.detach(), kind), loss), (tag, kind)           # d_f = NULL: the same value bits
            r = {"aten": aten, "hip": _errors(loss, grad, ref), "cl": None}
            if f.shape[1] == 3:
                # the same element runs the same arithmetic whatever the layout: equal bit for bit after the permute
                l_cl, g_cl = ops.reg_value_and_grad_cl(_cl(fd.detach()), kind)
                assert g_cl.shape == _cl(fd).shape
                assert torch.equal(l_cl, loss), (tag, kind, float(l_cl), float(loss))
                r["cl"] = float((g_cl.permute(0, 4, 1, 2, 3) - grad).abs().max())
            out[(tag, kind)] = r
    rep = {}
    for (tag, kind), r in out.items():
        for who in ("aten", "hip"):
            for q, v in r[who].items():
                rep[f"reg[{tag}.{kind}].{q}.e_{who}"] = v if np.isfinite(v) else 1e30
                print(f"reg[{tag}.{kind}] {q}: {who} {v:.3e}")
    note_many(rep)
    return out


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_parity_with_fp64_within_four_times_aten_fp32(quantity):
    m = _measured()
    assert len(m) == 6 * 4 + 2 + 4 + 1 + 3 + 4
    bound = A * max(r["aten"][quantity] for r in m.values())
    note_many({f"reg.bound.{quantity}": bound})
    print(f"bound for {quantity}: {bound:.3e}")
    assert 0.0 < bound < float("inf")
    bad = {k: r["hip"][quantity] for k, r in m.items() if not r["hip"][quantity] <= bound}
    assert not bad, f"{quantity}: HIP error beyond {A:g} x the largest ATen fp32 error ({bound:.3e}): {bad}"


def test_channels_last_gradient_equals_the_planar_one_bit_for_bit():
    m = _measured()
    seen = {k: r["cl"] for k, r in m.items() if r["cl"] is not None}
    assert len(seen) == 6 * 4 + 4 + 1 + 3 + 4          # every case of three channels
    assert not {k: v for k, v in seen.items() if v != 0.0}


@pytest.mark.parametrize("shape", [(1, 3, 6, 6, 6), (2, 3, 9, 10, 37)])
def test_zero_flow(shape):
    """iTV keeps the reference's 1e-6 under the root: loss 1e-3 / 3 (within one ulp of its fp32 value), gradient exactly 0; the
    other kinds are exactly 0 with a gradient of exactly 0"""
    from smilecode_amd import ops
    f = torch.zeros(shape, device="cuda")
    want = np.float32(1e-3 / 3)
    for kind in ALL:
        fr = f.clone().requires_grad_(True)
        lp = ops.reg_loss(fr, kind)
        (gp,) = torch.autograd.grad(lp, [fr])
        lc, gc = ops.reg_value_and_grad_cl(_cl(f), kind)
        assert torch.equal(lp, lc), kind
        for loss, grad in ((lp, gp), (lc, gc)):
            assert grad.shape[0] == shape[0] and not bool(grad.any()), kind
            if kind == "itv":
                got = np.float32(float(loss.detach()))
                assert abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1, (float(got), float(want))
            else:
                assert float(loss) == 0.0, kind


def test_adding_a_constant_leaves_the_gradient_bits_alone():
    """every term is made of differences: on a small-integer-valued flow a power of two is added without rounding, the
    differences are the same numbers and so is every gradient bit"""
    from smilecode_amd import ops
    gen = torch.Generator().manual_seed(5)
    f = torch.randint(-8, 9, (2, 3, 9, 11, 37), generator=gen).float().cuda()
    for kind in ALL:
        for c in (64.0, -1024.0):
            l0, g0 = ops.reg_value_and_grad_cl(_cl(f), kind)
            l1, g1 = ops.reg_value_and_grad_cl(_cl(f + c), kind)
            assert torch.equal(g0, g1) and torch.equal(l0, l1), (kind, c)
            fa, fb = f.clone().requires_grad_(True), (f + c).requires_grad_(True)
            (ga,) = torch.autograd.grad(ops.reg_loss(fa, kind), [fa])
            (gb,) = torch.autograd.grad(ops.reg_loss(fb, kind), [fb])
            assert torch.equal(ga, gb) and float(ga.abs().max()) > 0.0, (kind, c)


@pytest.mark.parametrize("tag", ["rand12x20x28_B2", "noise1x3x9x9x9", "smooth1x3x8x10x37"])
def test_loss_and_gradient_are_bit_reproducible(tag):
    from smilecode_amd import ops
    f, kinds = _inputs(tag)
    f = _cl(f.cuda())
    for kind in kinds:
        l1, g1 = ops.reg_value_and_grad_cl(f, kind)
        junk = torch.rand(1 << 22, device="cuda")                 # another allocation pattern for the second run's workspace
        l2, g2 = ops.reg_value_and_grad_cl(f, kind)
        del junk
        assert torch.equal(l1, l2) and torch.equal(g1, g2), kind
        l3, g3 = ops.reg_value_and_grad_cl(f, kind, grad_scale=0.37)   # the loss term's weight scales the gradient, not the value
        assert torch.equal(l3, l1), kind
        assert float((g3 - 0.37 * g1).abs().max()) <= 2e-6 * float(g1.abs().max()), kind
        assert float(g1.abs().max()) > 0.0
        l4, none = ops._reg_launch(f, kind, ops._reg_args("reg_loss", f, kind, True), True, False)      # d_f = NULL
        assert none is None and torch.equal(l4.reshape(()), l1), kind


def _model(shape):
    from smilecode_amd import models, synth
    m = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(m, synth.make_weights(24))
    return m


def _pair(shape):
    from smilecode_amd import synth
    mov, fix = synth.make_pair(shape, 24)
    return torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda()


def _term(kind):
    from smilecode_amd import losses
    return losses.Grad3DiTV() if kind == "itv" else losses.DisplacementRegularizer(kind)


@pytest.mark.parametrize("kind", ["bending", "itv"])
def test_hip_graph_capture_of_a_step_with_the_term(kind):
    """no host read-back is left in the term: the step captures (a sync inside a capture is an error), and its replays give the
    eager step's loss and flat gradient"""
    from smilecode_amd.engine import Trainer
    shape = (32, 48, 32)
    mov, fix = _pair(shape)
    eager = Trainer(_model(shape), reg=_term(kind))
    assert eager._seedable()
    le = eager._fwd_bwd(mov, fix)
    ge = eager.fp.grad.clone()
    assert bool(torch.isfinite(ge).all()) and float(ge.abs().max()) > 0.0
    tr = Trainer(_model(shape), reg=_term(kind)).capture(mov, fix)
    assert tr._graph is not None
    for _ in range(3):
        tr.fp.grad.fill_(float("nan"))
        tr._graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tr.fp.grad, ge), float((tr.fp.grad - ge).abs().max())
        assert all(torch.equal(x, y) for x, y in zip(tr._static_out, le))


@pytest.mark.parametrize("kind", ["bending", "itv"])
def test_seeded_step_equals_the_autograd_path(kind):
    from smilecode_amd.engine import Trainer
    shape = (32, 48, 32)
    mov, fix = _pair(shape)
    res = {}
    for seeded in (True, False):
        tr = Trainer(_model(shape), reg=_term(kind))
        tr.seed_backward = seeded
        assert tr._seedable() == seeded
        out = tr._fwd_bwd(mov, fix)
        res[seeded] = (tr.fp.grad.clone(), [float(v) for v in out])
    (ga, la), (gb, lb) = res[True], res[False]
    assert la[2] == lb[2], "the term's value"
    assert abs(la[0] - lb[0]) <= 2e-6 * abs(lb[0]) and abs(la[1] - lb[1]) <= 2e-6 * abs(lb[1]), (la, lb)
    assert torch.equal(ga, gb), float((ga - gb).abs().max())
    # a weighted term: the weight enters the kernel instead of a multiplication behind it
    res = {}
    for seeded in (True, False):
        tr = Trainer(_model(shape), weights=(0.7, 2.5), reg=_term(kind))
        tr.seed_backward = seeded
        tr._fwd_bwd(mov, fix)
        res[seeded] = tr.fp.grad.clone()
    gerr = float((res[True] - res[False]).abs().max() / res[False].abs().max())
    note_many({f"reg.seeded_step[{kind}].grad_relerr_weights_0.7_2.5": gerr})
    assert gerr < 2e-6, gerr


def test_end_to_end_gradient_against_the_fp64_oracle():
    """the product step with NCC + bending against the CPU oracle model in fp64 with the fp64 restatement as its regulariser; per
    parameter tensor HIP stays within tests/util.py's yardstick: GRAD_A x the error of the same oracle in ATen fp32 (the worst of
    F32_RUNS runs) + GRAD_FLOOR"""
    from oracle import modet_torch as orc
    from smilecode_amd import synth
    from smilecode_amd.engine import Trainer
    from tests.util import F32_RUNS, f32_inputs
    shape = (32, 48, 32)
    weights = synth.make_weights(24)
    mov, fix = synth.make_pair(shape, 24)
    model = _model(shape)
    tr = Trainer(model, reg=_term("bending"))
    loss, sim, reg = tr._fwd_bwd(torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda())
    torch.cuda.synchronize()
    names = [n for n, _ in model.named_parameters()]

    def oracle(m, f, dtype):
        p = {n: torch.from_numpy(v).to(dtype).requires_grad_(True) for n, v in weights.items()}
        y, flow = orc.modet_forward(p, m.to(dtype), f.to(dtype), (8, 4, 2, 1, 1), 6, 1.0)
        so, ro = orc.ncc_loss(f.to(dtype), y), reg_oracle.bending(flow)
        gs = torch.autograd.grad(so + ro, [p[n] for n in names], allow_unused=True)
        return float((so + ro).detach()), float(ro.detach()), {n: (g if g is not None else torch.zeros_like(p[n])).detach() for n, g in zip(names, gs)}

    lo, ro, g64 = oracle(torch.from_numpy(mov), torch.from_numpy(fix), torch.float64)
    g32 = [oracle(*f32_inputs((mov, fix), r), torch.float32)[2] for r in range(F32_RUNS)]
    grad = tr.fp.grad
    ghip = {n: grad[off:off + k] for n, (off, k) in zip(names, tr.fp.offsets)}
    el, er = abs(float(loss) - lo), abs(float(reg) - ro)
    note_many({"reg.e2e.loss_err": el, "reg.e2e.reg_err": er})
    print(f"bending: |loss err| {el:.2e} (loss {lo:.4f}, term {ro:.6f})")
    assert el < 2e-4 and er < 2e-4, (el, er)              # the bounds of __graft_entry__.smoke()
    grad_yardstick("reg.e2e", g64, g32, ghip, a={})
