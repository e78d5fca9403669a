"""-m gpu: the MIND-SSC descriptor, loss and gradient of csrc/mind.hip against fp64 (the reference's recorded results of
tests/golden/op_mind.npz, and the restatement of tests/mind_oracle.py for the larger volumes), bit-reproducibility, hipGraph
capture of a step with the term, the seeded against the autograd path, and one end-to-end gradient against the fp64 oracle model.

The parity bound is not a chosen number: every case is also evaluated with the ATen composition (tests/mind_oracle.py
mind_loss_aten) in fp32 on the CPU, whose own error against fp64 is measured; the HIP result has to stay within
A = 4 times the LARGEST such error over this file's cases, per quantity (another order of the 125-term box sum and of the
12-channel mean rounds differently, and one ATen sample is itself noisy)."""
import functools

import numpy as np
import pytest
import torch

from tests import mind_oracle
from tests.util import gold, note_many

pytestmark = pytest.mark.gpu

A = 4.0
GOLDEN = ("pair16", "pair12x20x28", "noise2x10x12x14", "tiny3x4x5")
SYNTH = {"pair32x48x32": ((32, 48, 32), 24, 1), "pair48x64x48": ((48, 64, 48), 24, 1), "pair64x64x64": ((64, 64, 64), 24, 1),
         "pair20x24x36_B2": ((20, 24, 36), 40, 2)}


def _inputs(tag):
    if tag in GOLDEN:
        g = gold("op_mind.npz")
        return torch.from_numpy(g[tag + ".a"]), torch.from_numpy(g[tag + ".b"])
    from smilecode_amd import synth
    shape, seed, batch = SYNTH[tag]
    mov, fix = synth.make_pair(shape, seed, batch)
    return torch.from_numpy(mov), torch.from_numpy(fix)


def _fp64(tag, a, b):
    """(loss, da, db, descriptor of a on the planes zs, zs) in fp64"""
    if tag in GOLDEN:
        g = gold("op_mind.npz")
        T = lambda k: torch.from_numpy(np.ascontiguousarray(g[tag + k])).double()      # noqa: E731
        return T(".loss"), T(".da"), T(".db"), T(".mind_a"), [int(z) for z in g[tag + ".mind_a_z"]]
    loss, da, db = mind_oracle.value_and_grads(mind_oracle.mind_loss, a, b, torch.float64)
    return loss, da, db, mind_oracle.mind_ssc(a.double()), list(range(a.shape[2]))


def _errors(loss, da, db, desc, ref):
    l64, da64, db64, d64, zs = ref
    return {"loss": abs(float(loss) - float(l64)) / abs(float(l64)),
            "grad_a": float((da.double().cpu() - da64).abs().max()) / float(da64.abs().max()),
            "grad_b": float((db.double().cpu() - db64).abs().max()) / float(db64.abs().max()),
            "descriptor": float((desc.double().cpu()[:, :, zs] - d64).abs().max())}


@functools.lru_cache(maxsize=None)
def _measured():
    """case -> {"aten": errors of the fp32 ATen composition on the CPU, "hip": errors of the HIP path}, each against fp64:
    loss relative, gradients max|err| over ALL voxels / max|g64|, descriptor max|err| (its values lie in [0, 1])"""
    from smilecode_amd import ops
    out = {}
    for tag in GOLDEN + tuple(SYNTH):
        a, b = _inputs(tag)
        ref = _fp64(tag, a, b)
        l32, da32, db32 = mind_oracle.value_and_grads(mind_oracle.mind_loss_aten, a, b, torch.float32)
        aten = _errors(l32, da32, db32, mind_oracle.mind_ssc_aten(a.float()), ref)
        ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        loss = ops.mind_loss(ad, bd)
        da, db = torch.autograd.grad(loss, [ad, bd])
        # each argument alone takes the other branch of the autograd node: same kernel, same bits
        (da1,) = torch.autograd.grad(ops.mind_loss(ad, bd.detach()), [ad])
        (db1,) = torch.autograd.grad(ops.mind_loss(ad.detach(), bd), [bd])
        assert torch.equal(da1, da) and torch.equal(db1, db), tag
        desc = ops.mind_ssc(ad.detach())
        assert desc.shape == (a.shape[0], 12) + tuple(a.shape[2:])
        assert all(bool(torch.isfinite(t).all()) for t in (loss, da, db, desc)), tag
        out[tag] = {"aten": aten, "hip": _errors(loss, da, db, desc, ref)}
    rep = {}
    for tag, r in out.items():
        for who in ("aten", "hip"):
            for q, v in r[who].items():
                rep[f"mind[{tag}].{q}.e_{who}"] = v
                print(f"mind[{tag}] {q}: {who} {v:.3e}")
    note_many(rep)
    return out


def _bound(quantities):
    m = _measured()
    return A * max(m[tag]["aten"][q] for tag in m for q in quantities)


@pytest.mark.parametrize("quantity", ["descriptor", "loss", "gradient"])
def test_parity_with_fp64_within_four_times_aten_fp32(quantity):
    qs = ("grad_a", "grad_b") if quantity == "gradient" else (quantity,)
    m, bound = _measured(), _bound(qs)
    note_many({f"mind.bound.{quantity}": bound})
    print(f"bound for {quantity}: {bound:.3e}")
    assert bound > 0.0
    bad = {(tag, q): m[tag]["hip"][q] for tag in m for q in qs if not m[tag]["hip"][q] <= bound}
    assert not bad, f"{quantity}: HIP error beyond {A:g} x the largest ATen fp32 error ({bound:.3e}): {bad}"


@pytest.mark.parametrize("tag", ["pair20x24x36_B2", "pair32x48x32", "tiny3x4x5"])
def test_loss_and_gradient_are_bit_reproducible(tag):
    from smilecode_amd import ops
    a, b = (t.cuda() for t in _inputs(tag))
    l1, g1 = ops.mind_value_and_grad(a, b)
    junk = torch.rand(1 << 22, device="cuda")                 # another allocation pattern for the second run's workspace
    l2, g2 = ops.mind_value_and_grad(a, b)
    d1, d2 = ops.mind_ssc(a), ops.mind_ssc(a)
    del junk
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(d1, d2)
    l3, g3 = ops.mind_value_and_grad(a, b, 0.37)              # the loss term's weight scales the gradient, not the value
    assert torch.equal(l3, l1)
    assert float((g3 - 0.37 * g1).abs().max()) <= 2e-6 * float(g1.abs().max())    # (a handful of fp32 roundings apart)
    # the loss is symmetric: the swapped call sums the same squares in the same order
    l4, _ = ops.mind_value_and_grad(b, a)
    assert torch.equal(l4, l1)


def _model(shape):
    from smilecode_amd import models, synth
    m = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(m, synth.make_weights(24))
    return m


def _pair(shape):
    from smilecode_amd import synth
    mov, fix = synth.make_pair(shape, 24)
    return torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda()


def test_step_with_a_mind_term_is_bit_reproducible():
    from smilecode_amd.engine import Trainer
    from smilecode_amd.losses import MIND_loss
    shape = (32, 48, 32)
    mov, fix = _pair(shape)
    a, b = Trainer(_model(shape), sim=MIND_loss()), Trainer(_model(shape), sim=MIND_loss())
    assert a._seedable()
    o1 = a._fwd_bwd(mov, fix)
    g1 = a.fp.grad.clone()
    o2 = a._fwd_bwd(mov, fix)
    assert torch.equal(a.fp.grad, g1) and all(torch.equal(x, y) for x, y in zip(o1, o2)), "two steps of one trainer differ"
    b._fwd_bwd(mov, fix)
    assert torch.equal(b.fp.grad, g1), "two trainers differ"
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0.0


def test_hip_graph_capture_of_a_step_with_a_mind_term():
    """no host read-back is left in the term: the step captures (a sync inside a capture is an error), and its replays give the
    eager step's loss and flat gradient"""
    from smilecode_amd.engine import Trainer
    from smilecode_amd.losses import MIND_loss
    shape = (32, 48, 32)
    mov, fix = _pair(shape)
    eager = Trainer(_model(shape), sim=MIND_loss())
    le = eager._fwd_bwd(mov, fix)
    ge = eager.fp.grad.clone()
    tr = Trainer(_model(shape), sim=MIND_loss()).capture(mov, fix)
    assert tr._graph is not None
    for _ in range(3):
        tr.fp.grad.fill_(float("nan"))
        tr._graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tr.fp.grad, ge), float((tr.fp.grad - ge).abs().max())
        assert all(torch.equal(x, y) for x, y in zip(tr._static_out, le))
    # and through train_step, against an eager trainer
    l1, l2 = eager.train_step(mov, fix), tr.train_step(mov, fix)
    assert float(l1[0]) == float(l2[0]) and float(l1[1]) == float(l2[1])
    assert torch.equal(eager.fp.flat, tr.fp.flat)


def test_seeded_step_equals_the_autograd_path_with_a_mind_term():
    from smilecode_amd.engine import Trainer
    from smilecode_amd.losses import MIND_loss
    shape = (32, 48, 32)
    mov, fix = _pair(shape)
    res = {}
    for seeded in (True, False):
        tr = Trainer(_model(shape), sim=MIND_loss())
        tr.seed_backward = seeded
        assert tr._seedable() == seeded
        out = tr._fwd_bwd(mov, fix)
        res[seeded] = (tr.fp.grad.clone(), [float(v) for v in out])
    (ga, la), (gb, lb) = res[True], res[False]
    assert la[1] == lb[1], "MIND value"
    assert abs(la[0] - lb[0]) <= 2e-6 * abs(lb[0]) and abs(la[2] - lb[2]) <= 2e-6 * abs(lb[2]), (la, lb)
    assert torch.equal(ga, gb), float((ga - gb).abs().max())
    # a weighted term: the weight enters the kernel instead of a multiplication behind it
    res = {}
    for seeded in (True, False):
        tr = Trainer(_model(shape), weights=(0.7, 2.5), sim=MIND_loss())
        tr.seed_backward = seeded
        tr._fwd_bwd(mov, fix)
        res[seeded] = tr.fp.grad.clone()
    gerr = float((res[True] - res[False]).abs().max() / res[False].abs().max())
    note_many({"mind.seeded_step.grad_relerr_weights_0.7_2.5": gerr})
    assert gerr < 2e-6, gerr


def test_end_to_end_gradient_with_a_mind_term_against_the_fp64_oracle():
    """the product step with sim = MIND_loss against the CPU oracle model in fp64 with the MIND restatement as its similarity
    term; bounds: those of __graft_entry__.smoke() (|loss err| < 2e-4, every parameter tensor within 5e-3 of its maximum)"""
    from oracle import modet_torch as orc
    from smilecode_amd import synth
    from smilecode_amd.engine import Trainer
    from smilecode_amd.losses import MIND_loss
    shape = (32, 48, 32)
    weights = synth.make_weights(24)
    mov, fix = synth.make_pair(shape, 24)
    model = _model(shape)
    tr = Trainer(model, sim=MIND_loss())
    loss, sim, reg = tr._fwd_bwd(torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda())
    torch.cuda.synchronize()
    p = {n: torch.from_numpy(v).double().requires_grad_(True) for n, v in weights.items()}
    m64, f64 = torch.from_numpy(mov).double(), torch.from_numpy(fix).double()
    y, flow = orc.modet_forward(p, m64, f64, (8, 4, 2, 1, 1), 6, 1.0)
    so, ro = mind_oracle.mind_loss(f64, y), orc.grad3d_loss(flow)
    lo = so + ro
    names = [n for n, _ in model.named_parameters()]
    ref = {n: (g if g is not None else torch.zeros_like(p[n]))
           for n, g in zip(names, torch.autograd.grad(lo, [p[n] for n in names], allow_unused=True))}
    el, es = abs(float(loss) - float(lo.detach())), abs(float(sim) - float(so.detach()))
    grad = tr.fp.grad.double().cpu()
    eg, worst, rep = 0.0, "", {}
    for i, n in enumerate(names):
        off, k = tr.fp.offsets[i]
        r = ref[n].reshape(-1)
        gmax = float(r.abs().max())
        if gmax < 1e-8:                 # a conv bias under InstanceNorm: analytically zero, rounding noise on both sides
            continue
        e = float((grad[off:off + k] - r).abs().max()) / gmax
        rep[f"mind.e2e.{n}.e_hip"] = e
        if e > eg:
            eg, worst = e, n
    rep.update({"mind.e2e.loss_err": el, "mind.e2e.sim_err": es, "mind.e2e.worst_grad_err": eg})
    note_many(rep)
    print(f"|loss err| {el:.2e} (loss {float(lo):.4f}, MIND {float(so):.4f}), worst parameter-gradient err {eg:.2e} ({worst})")
    assert np.isfinite(eg) and el < 2e-4 and es < 2e-4 and eg < 5e-3, (el, es, eg, worst)
