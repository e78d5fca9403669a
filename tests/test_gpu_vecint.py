"""-m gpu: the scaling-and-squaring integration of csrc/vecint.hip against fp64 (the reference's recorded results of
tests/golden/op_vecint.npz, and the restatement of tests/vecint_oracle.py for the two larger fields); exact cases; the inference
form, the planar module, bit-reproducibility, hipGraph capture; and ModeT(diff=True) against the fp64 oracle model.

The parity bound is not a chosen number (as in tests/test_gpu_reg.py): every case is also evaluated with the restatement in fp32
on the CPU, the ATen composition, whose own error against fp64 is measured; the HIP result has to stay within A = 4 times the
LARGEST such error over this file's cases, per quantity (another summation order plus one noisy ATen sample).  The composition of
existing launches (ops.warp seven times) has to sit within the same bound: that shows the bound is fair.  The fields keep clear
of the kinks of trilinear sampling (tests/test_cpu_vecint.py asserts the margin)."""
import functools

import numpy as np
import pytest
import torch

from tests import vecint_oracle as vo
from tests.util import gold, grad_yardstick, note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
# (case, bound): bounded twice (every step on the gather path, every step on the scatter path), mixed with steps 0-4 gathered
RUNS = [(t, 0.0) for t in vo.CASES if not t.startswith(("bounded", "mixed"))] + [
    ("bounded_n7_8x12x16", 1.0), ("bounded_n7_8x12x16", 0.0), ("mixed_n7_8x12x16", 8.0)]
QUANTITIES = ("out", "grad")


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _pl(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


@functools.lru_cache(maxsize=None)
def _fp64(tag):
    """(out, grad) in fp64: the reference's own where recorded, else the restatement; computed once and shared"""
    if vo.CASES[tag][6]:
        g = gold("op_vecint.npz")
        return tuple(torch.from_numpy(np.ascontiguousarray(g["%s.%s" % (tag, q)])) for q in QUANTITIES)
    return vo.value_and_grad(vo.case_field(tag), vo.CASES[tag][4], torch.float64)


def _errors(out, grad, ref):
    return {"out": rel_err(out, ref[0]), "grad": rel_err(grad, ref[1])}


def _hip(w_cl, nsteps, bound, cot_cl):
    from smilecode_amd import ops
    w = w_cl.clone().requires_grad_(True)
    out = ops.vecint(w, nsteps, bound)
    (g,) = torch.autograd.grad(out, [w], cot_cl)
    return out.detach(), g


def _composed(w_cl, nsteps, bound, cot_cl):
    """the composition of existing launches: the scale, then ops.warp(v, v, add_flow=True) nsteps times"""
    from smilecode_amd import ops
    w = w_cl.clone().requires_grad_(True)
    v = w * (1.0 / 2 ** nsteps)
    for k in range(nsteps):
        v = ops.warp(v, v, 0, True, 1 if (bound > 0 and bound * 2.0 ** (k - nsteps) <= 1.0) else 0)
    (g,) = torch.autograd.grad(v, [w], cot_cl)
    return v.detach(), g


@functools.lru_cache(maxsize=None)
def _measured():
    """(case, bound) -> {"aten", "hip", "composed"}: errors against fp64, each max|err| / max|ref|"""
    out = {}
    for tag, bound in RUNS:
        nsteps = vo.CASES[tag][4]
        w = vo.case_field(tag)
        ref = _fp64(tag)
        cot = vo.cotangent(w.shape)
        aten = _errors(*vo.value_and_grad(w, nsteps, torch.float32), ref)
        w_cl, cot_cl = _cl(w.float()).cuda(), _cl(cot.float()).cuda()
        o, g = _hip(w_cl, nsteps, bound, cot_cl)
        assert o.shape == w_cl.shape and g.shape == w_cl.shape
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(g).all()), (tag, bound)
        oc, gc = _composed(w_cl, nsteps, bound, cot_cl)
        out[(tag, bound)] = {"aten": aten, "hip": _errors(_pl(o), _pl(g), ref), "composed": _errors(_pl(oc), _pl(gc), ref),
                             "fwd_equals_composed": bool(torch.equal(o, oc))}
    rep = {}
    for (tag, bound), r in out.items():
        for who in ("aten", "hip", "composed"):
            for q, v in r[who].items():
                rep[f"vecint[{tag},bound={bound:g}].{q}.e_{who}"] = v
                print(f"vecint[{tag},bound={bound:g}] {q}: {who} {v:.3e}")
    note_many(rep)
    return out


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_parity_with_fp64_within_four_times_aten_fp32(quantity):
    m = _measured()
    assert len(m) == 8
    bound = A * max(r["aten"][quantity] for r in m.values())
    note_many({f"vecint.bound.{quantity}": bound})
    print(f"bound for {quantity}: {bound:.3e}")
    assert 0.0 < bound < float("inf")
    bad = {k: r["hip"][quantity] for k, r in m.items() if not r["hip"][quantity] <= bound}
    assert not bad, f"{quantity}: HIP error beyond {A:g} x the largest ATen fp32 error ({bound:.3e}): {bad}"
    fair = {k: r["composed"][quantity] for k, r in m.items() if not r["composed"][quantity] <= bound}
    assert not fair, f"{quantity}: the composition of existing launches is beyond the bound ({bound:.3e}) itself: {fair}"


def test_forward_equals_the_composed_launches_bit_for_bit():
    """the header's statement: a step is modet_warp_fwd with src = flow and add_flow = 1, the scale a power of two"""
    assert all(r["fwd_equals_composed"] for r in _measured().values())


def _grid_cotangent(shape, seed=9):
    """a cotangent on a 2^-10 grid: the scatter path sums in fixed point (2^-40 of the power of two above max |g| per unit),
    which holds such values -- and their doubles, step after step -- without rounding"""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randint(-4096, 4097, shape, generator=gen).float() / 1024.0).cuda()


@pytest.mark.parametrize("bound", [1.0, 0.0, 16.0])
@pytest.mark.parametrize("shape,nsteps", [((2, 5, 6, 7, 3), 7), ((1, 8, 12, 37, 3), 3)])
def test_zero_field_is_exact(shape, nsteps, bound):
    """out is exactly 0; every step doubles the cotangent (identity + the one neighbour of weight 1) and step 0 halves it nsteps
    times: d_vec equals the cotangent bit for bit, on the gather path (bound 1), the scatter path (0) and both (16)"""
    cot = _grid_cotangent(shape)
    out, g = _hip(torch.zeros(shape, device="cuda"), nsteps, bound, cot)
    assert not bool(out.any())
    assert torch.equal(g, cot), float((g - cot).abs().max())


@pytest.mark.parametrize("bound", [1.0, 0.0])
def test_no_steps_returns_the_input_and_the_cotangent_bits(bound):
    w = _cl(vo.case_field("n3_4x5x67").float()).cuda()
    cot = _cl(vo.cotangent((1, 3, 4, 5, 67)).float()).cuda()
    out, g = _hip(w, 0, bound, cot)
    assert torch.equal(out, w) and torch.equal(g, cot)


@pytest.mark.parametrize("tag", ["n7_5x6x7_B2", "n2_12x20x28_B2", "n1_6x6x6"])
def test_inference_form_equals_the_saving_form_bit_for_bit(tag):
    """steps = NULL (the steps alternate between out and a scratch field) against the form that keeps every step's input"""
    from smilecode_amd import ops
    nsteps = vo.CASES[tag][4]
    w = _cl(vo.case_field(tag).float()).cuda()
    with torch.no_grad():
        a = ops.vecint(w, nsteps)
    b = ops.vecint(w.clone().requires_grad_(True), nsteps)
    assert not a.requires_grad and b.requires_grad
    assert torch.equal(a, b.detach())
    o1, s1 = ops._vecint_fwd(w, nsteps, False)
    o2, s2 = ops._vecint_fwd(w, nsteps, True)
    assert s1 is None and (s2 is None) == (nsteps < 2) and torch.equal(o1, o2) and torch.equal(o1, a)
    if s2 is not None:
        assert s2.shape == (nsteps - 1,) + tuple(w.shape)


def test_planar_module_equals_the_channels_last_op():
    from smilecode_amd import models, ops
    tag = "n3_4x5x67"
    w = vo.case_field(tag).float().cuda()
    m = models.VecInt(vo.CASES[tag][2], 3).cuda()
    assert not list(m.parameters())
    wp = w.clone().requires_grad_(True)
    out = m(wp)
    assert out.shape == w.shape
    wc = _cl(w).requires_grad_(True)
    ref = ops.vecint(wc, 3)
    assert torch.equal(out.detach(), _pl(ref.detach()))
    cot = vo.cotangent(w.shape).float().cuda()
    (gp,) = torch.autograd.grad(out, [wp], cot)
    (gc,) = torch.autograd.grad(ref, [wc], _cl(cot))
    assert torch.equal(gp, _pl(gc))


@pytest.mark.parametrize("tag,bound", [("bounded_n7_8x12x16", 1.0), ("bounded_n7_8x12x16", 0.0), ("mixed_n7_8x12x16", 8.0),
                                       ("n2_12x20x28_B2", 0.0)])
def test_two_runs_are_bit_identical(tag, bound):
    nsteps = vo.CASES[tag][4]
    w = _cl(vo.case_field(tag).float()).cuda()
    cot = _cl(vo.cotangent(vo.case_field(tag).shape).float()).cuda()
    o1, g1 = _hip(w, nsteps, bound, cot)
    junk = torch.rand(1 << 22, device="cuda")                 # another allocation pattern for the second run's buffers
    o2, g2 = _hip(w, nsteps, bound, cot)
    del junk
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    assert float(g1.abs().max()) > 0.0


@pytest.mark.parametrize("bound", [1.0, 0.0])
def test_hip_graph_of_forward_and_backward_replays_the_eager_bits(bound):
    from smilecode_amd import ops
    tag = "bounded_n7_8x12x16"
    w = _cl(vo.case_field(tag).float()).cuda().requires_grad_(True)
    cot = _cl(vo.cotangent(vo.case_field(tag).shape).float()).cuda()
    oe, ge = _hip(w.detach(), 7, bound, cot)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture (allocator, library load)
        (gw,) = torch.autograd.grad(ops.vecint(w, 7, bound), [w], cot)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.vecint(w, 7, bound)
        (g,) = torch.autograd.grad(out, [w], cot)
    for _ in range(2):
        out.detach().fill_(float("nan"))
        g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), oe) and torch.equal(g, ge)


# ------------------------------------------------------------------------------------------------ the model
SHAPE = (32, 48, 32)


def _model(diff=True, **kw):
    from smilecode_amd import models, synth
    m = models.ModeT(SHAPE, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0, diff=diff, int_steps=7, **kw).cuda()
    models.load_numpy_weights(m, synth.make_weights(24))
    return m


def _pair():
    from smilecode_amd import synth
    mov, fix = synth.make_pair(SHAPE, 24)
    return torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda()


def test_diff_model_against_the_fp64_oracle():
    """the flow of ModeT(diff=True, int_steps=7) within 4 x the error the same restatement makes in fp32 on the CPU; the
    parameter gradients of NCC + Grad3d through tests/util.py's yardstick"""
    from oracle import modet_torch as orc
    from smilecode_amd import synth
    from smilecode_amd.engine import Trainer
    from tests.util import F32_RUNS, f32_inputs
    weights = synth.make_weights(24)
    mov, fix = synth.make_pair(SHAPE, 24)
    model = _model()
    tr = Trainer(model)
    tr._fwd_bwd(torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda())
    with torch.no_grad():
        _, flow = model(torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda())
    torch.cuda.synchronize()
    names = [n for n, _ in model.named_parameters()]

    def oracle(m, f, dtype):
        p = {n: torch.from_numpy(v).to(dtype).requires_grad_(True) for n, v in weights.items()}
        y, fl = vo.modet_forward_diff(p, m.to(dtype), f.to(dtype), 7)
        loss = orc.ncc_loss(f.to(dtype), y) + orc.grad3d_loss(fl)
        gs = torch.autograd.grad(loss, [p[n] for n in names], allow_unused=True)
        return fl.detach(), {n: (g if g is not None else torch.zeros_like(p[n])).detach() for n, g in zip(names, gs)}

    f64, g64 = oracle(torch.from_numpy(mov), torch.from_numpy(fix), torch.float64)
    r32 = [oracle(*f32_inputs((mov, fix), r), torch.float32) for r in range(F32_RUNS)]
    e_f32, e_hip = rel_err(r32[0][0], f64), rel_err(flow, f64)
    note_many({"vecint.e2e.flow.e_f32": e_f32, "vecint.e2e.flow.e_hip": e_hip})
    print(f"diff flow: e_f32 {e_f32:.3e}, e_hip {e_hip:.3e}")
    assert e_hip <= A * e_f32, (e_hip, e_f32)
    grad = tr.fp.grad
    ghip = {n: grad[off:off + k] for n, (off, k) in zip(names, tr.fp.offsets)}
    grad_yardstick("vecint.e2e", g64, [g for _, g in r32], ghip)


def test_captured_trainer_step_equals_the_eager_step():
    from smilecode_amd.engine import Trainer
    mov, fix = _pair()
    eager = Trainer(_model())
    le = eager._fwd_bwd(mov, fix)
    ge = eager.fp.grad.clone()
    assert bool(torch.isfinite(ge).all()) and float(ge.abs().max()) > 0.0
    tr = Trainer(_model()).capture(mov, fix)
    assert tr._graph is not None
    for _ in range(2):
        tr.fp.grad.fill_(float("nan"))
        tr._graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tr.fp.grad, ge), float((tr.fp.grad - ge).abs().max())
        assert all(torch.equal(x, y) for x, y in zip(tr._static_out, le))


def test_bf16_activations_compose_with_diff():
    mov, fix = _pair()
    with torch.no_grad():
        y, flow = _model(act_dtype=torch.bfloat16)(mov, fix)
    assert flow.shape == (1, 3) + SHAPE and bool(torch.isfinite(flow).all()) and bool(torch.isfinite(y).all())
    assert float(flow.abs().max()) > 0.0
