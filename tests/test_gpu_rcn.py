"""-m gpu: the VTN and RCN networks (models.VTN, models.RCN) on the MI355X at 64 x 64 x 128 with channels = 4 against the reference's
golden vectors (fp64, tests/golden/make_goldens_rcn.py), measured in units of the error the same composition makes in ATen fp32 on
the CPU (tests/rcn_oracle.py run in single precision).

THE RULE for the outputs (tests/test_gpu_rdn.py's): HIP's error against the golden is at most A = 4 times the largest error of
F32_RUNS ATen-fp32 runs (tests.util.f32_inputs).  The parameter gradients go through tests.util.grad_yardstick.  An error is
max|got - ref| / max|ref|.  Every measured figure goes to the parity report before it is asserted."""
import functools
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import rcn_oracle as orc
from tests.util import F32_RUNS, GOLD, f32_inputs, gold, grad_yardstick, note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
SHAPE, CHANNELS, NPZ = orc.GOLD_SHAPE, orc.GOLD_CHANNELS, "e2e_rcn_64x64x128.npz"
RUNS = [(run, B) for run in orc.RUNS for B in (1, 2)]
IDS = ["%s-B%d" % rb for rb in RUNS]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _load(m, p):
    from smilecode_amd import models
    models.load_numpy_weights(m, {n: v.float().numpy() for n, v in p.items()})
    return m


def _model(run="rcn", **kw):
    from smilecode_amd import models
    n, fm = orc.RUNS[run]
    if n == 0:
        m = models.VTN(SHAPE, flow_multiplier=fm, channels=CHANNELS, warp=True, **kw)
    else:
        m = models.RCN(SHAPE, flow_multiplier=fm, channels=CHANNELS, n_cascade=n, **kw)
    return _load(m.cuda(), orc.golden_weights(run))


def _pair(B):
    mov, fix = orc.golden_pair()
    return mov[:B].cuda(), fix[:B].cuda()


@functools.lru_cache(maxsize=None)
def _oracle(run, B):
    """(fp64 run, the F32_RUNS fp32 runs) of the oracle's loss and gradients on the golden pair, computed once per case"""
    mov, fix = (t[:B] for t in orc.golden_pair())
    p, (n, fm) = orc.golden_weights(run), orc.RUNS[run]
    runs = []
    for r in range(F32_RUNS):
        m, f = f32_inputs((mov, fix), r)
        runs.append(orc.value_and_grads(p, m, f, n, torch.float32, fm))
    return orc.value_and_grads(p, mov, fix, n, torch.float64, fm), runs


@functools.lru_cache(maxsize=None)
def _oracle_outputs(run, B):
    """the outputs (loss, moved, flow, subflows) of the F32_RUNS fp32 runs alone: forward passes without a tape (an evaluation
    with gradients costs three times as much on the CPU, and the forward test of a case needs none)"""
    mov, fix = (t[:B] for t in orc.golden_pair())
    p, (n, fm) = orc.golden_weights(run), orc.RUNS[run]
    p32 = {k: v.float() for k, v in p.items()}
    with torch.no_grad():
        return [orc.train_loss(p32, *f32_inputs((mov, fix), r), n, fm) for r in range(F32_RUNS)]


def _outputs(model, mov, fix):
    """(moved, flow, [subflows]) of either network in its training form"""
    out = model(mov, fix)
    return out[0], out[1], (list(out[2:]) if len(out) > 2 else [out[1]])


@pytest.mark.parametrize("run,B", RUNS, ids=IDS)
def test_forward_against_the_golden(run, B):
    g, tag = gold(NPZ), "%s.B%d" % (run, B)
    stride = int(g["stride"])
    runs = _oracle_outputs(run, B)
    kw = {"return_subflows": True} if run == "rcn" else {}
    model, (mov, fix) = _model(run, **kw), _pair(B)
    with torch.no_grad():
        moved, flow, subs = _outputs(model, mov, fix)
        moved2, flow2 = _model(run)(mov, fix)                          # the inference contract: two outputs, the same bits
    assert tuple(moved.shape) == (B, 1) + SHAPE and tuple(flow.shape) == (B, 3) + SHAPE and len(subs) == max(orc.RUNS[run][0], 1)
    assert torch.equal(moved, moved2) and torch.equal(flow, flow2)
    named = [("flow", flow, lambda r: r[2]), ("moved", moved, lambda r: r[1])]
    named += [("subflow%d" % i, w, (lambda r, i=i: r[3][i])) for i, w in enumerate(subs)]
    rep = {}
    for name, got, pick in named:
        ref = T(g["%s.%s" % (tag, name)])
        rep["rcn[%s].%s.e_hip" % (tag, name)] = rel_err(got.reshape(-1)[::stride], ref)
        rep["rcn[%s].%s.e_f32" % (tag, name)] = max(rel_err(pick(r).reshape(-1)[::stride], ref) for r in runs)
    note_many(rep)
    for name, _, _ in named:
        e_hip, e_f32 = rep["rcn[%s].%s.e_hip" % (tag, name)], rep["rcn[%s].%s.e_f32" % (tag, name)]
        assert e_hip <= A * e_f32, "%s %s: e_hip %.3e, ATen fp32 %.3e (A = %g)" % (tag, name, e_hip, e_f32, A)


def _reference_loss(fix, moved, subs):
    """NCC(moved) + Grad3d('l2') of every subflow ("Baseline methods/RCN/train.py":106-130)"""
    from smilecode_amd import losses
    loss = losses.NCC_vxm()(fix, moved)
    for w in subs:
        loss = loss + losses.Grad3d(penalty="l2")(w, fix)
    return loss


@pytest.mark.parametrize("run,B", [("rcn", 1)], ids=["rcn-B1"])
def test_parameter_gradients_against_the_yardstick(run, B):
    """the reference's loss on the training outputs: the tensors the golden holds against the reference, the rest against the
    oracle in fp64 (recomputed here), all through grad_yardstick.  One case, RCN at B = 1: the yardstick is four evaluations of the
    oracle with gradients on the CPU, and they are this test's time (measured inside the whole suite: 27 s here, 21 s for the bare
    VTN, which is why that case is not run: RCN's two cascades are two VTNs with every layer of the class).  The batch is covered
    by the layer's B = 2 cases (tests/test_gpu_deconv.py), by the B = 2 outputs above and by the trainer tests below, and the
    VTN and B = 2 golden gradients by tests/test_cpu_rcn.py"""
    g, tag = gold(NPZ), "%s.B%d" % (run, B)
    (loss64, _, _, _, g64), runs = _oracle(run, B)
    g64 = dict(g64)
    n_gold = 0
    for n in g64:
        key = "%s.grad.%s" % (tag, n)
        if key in g.files:
            g64[n] = T(g[key])
            n_gold += 1
    assert n_gold == 28 * max(orc.RUNS[run][0], 1)
    kw = {"return_subflows": True} if run == "rcn" else {}
    model, (mov, fix) = _model(run, **kw), _pair(B)
    moved, flow, subs = _outputs(model, mov, fix)
    loss = _reference_loss(fix, moved, subs)
    note_many({"rcn[%s].loss_abs_err" % tag: abs(float(loss.detach()) - float(g[tag + ".loss"][0]))})
    loss.backward()
    ghip = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(ghip) == sorted(g64) and all(v is not None for v in ghip.values())
    grad_yardstick("rcn[%s]" % tag, g64, [r[4] for r in runs], ghip)


def test_eight_channels_against_the_oracle():
    """channels = 8, the widest configuration, at 64^3 with one cascade: 256 -> 256 through the stride-1 kernels, Pred5 on 259 input
    channels, Deconv5 256 -> 128 and Deconv4 259 -> 64, outputs and every parameter gradient against the oracle in fp64 (no golden of
    this configuration is committed), by the file's rules"""
    from smilecode_amd import models
    shape, tag = (64, 64, 64), "rcn[c8,64^3]"
    mov, fix = (t[:1, :, :64, :64, :64].contiguous() for t in orc.golden_pair())
    p = orc.make_weights(8, 1, mov, fix, 2.0)
    ref = orc.value_and_grads(p, mov, fix, 1, torch.float64, 2.0)
    runs = [orc.value_and_grads(p, *f32_inputs((mov, fix), r), 1, torch.float32, 2.0) for r in range(F32_RUNS)]
    assert orc.SUBFLOW_RANGE[0] <= float(ref[3][0].abs().max()) <= orc.SUBFLOW_RANGE[1]
    m = _load(models.RCN(shape, flow_multiplier=2.0, channels=8, n_cascade=1, return_subflows=True).cuda(), p)
    moved, flow, sub = m(mov.cuda(), fix.cuda())
    rep = {}
    for name, got, pick in (("flow", flow, lambda r: r[2]), ("moved", moved, lambda r: r[1]), ("subflow0", sub, lambda r: r[3][0])):
        rep["%s.%s.e_hip" % (tag, name)] = rel_err(got, pick(ref))
        rep["%s.%s.e_f32" % (tag, name)] = max(rel_err(pick(r), pick(ref)) for r in runs)
    note_many(rep)
    for name in ("flow", "moved", "subflow0"):
        assert rep["%s.%s.e_hip" % (tag, name)] <= A * rep["%s.%s.e_f32" % (tag, name)], (name, rep)
    _reference_loss(fix.cuda(), moved, [sub]).backward()
    grad_yardstick(tag, ref[4], [r[4] for r in runs], {n: q.grad for n, q in m.named_parameters()})


def _rel_l2_per_tensor(tr_a, tr_b):
    out = []
    for (off, n), p in zip(tr_a.fp.offsets, tr_a.fp.params):
        a, b = tr_a.fp.flat[off:off + n].double(), tr_b.fp.flat[off:off + n].double()
        out.append((float((a - b).norm()), float(a.norm())))
    return out


def _trainable(run="rcn"):
    return _model(run, **({"return_subflows": True} if run == "rcn" else {}))


def test_trainer_loss_is_the_reference_loss():
    """NCC on moved plus the regulariser on EVERY subflow (not on the composed flow), in both of the step's loss paths"""
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(1)
    tr = Trainer(_trainable())
    with torch.no_grad():
        moved, flow, subs = _outputs(tr.model, mov, fix)
        want = _reference_loss(fix, moved, subs)
        loss, sim, reg = tr.loss(mov, fix)
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want)) and float(reg) > 0      # (the sums associate differently)
    assert abs(float(reg) - sum(float(_reference_loss(fix, moved, [w])) - float(_reference_loss(fix, moved, [])) for w in subs)) < 1e-5
    (sl, ssim, sreg), roots, seeds = tr._seeded_loss(mov, fix)
    assert len(roots) == len(seeds) == 3 and all(r.shape == s.shape for r, s in zip(roots, seeds))
    assert abs(float(sl) - float(want)) <= 1e-6 * abs(float(want))


@pytest.mark.parametrize("B", [1, 2])
def test_trainer_capture_verifies_and_follows_the_eager_steps(B):
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(B)
    a, b = Trainer(_trainable()), Trainer(_trainable())
    b.capture(mov, fix, verify=True)                                   # raises if a replay does not reproduce the eager gradients
    assert b._graph is not None and torch.equal(a.fp.flat, b.fp.flat)
    for _ in range(3):
        la, lb = a.train_step(mov, fix), b.train_step(mov, fix)
    assert bool(torch.isfinite(la[0])) and abs(float(la[0]) - float(lb[0])) < 1e-5
    rel, floor_frac = a._verify_tolerance()
    per = _rel_l2_per_tensor(a, b)
    floor = floor_frac * max(n for _, n in per)
    note_many({"rcn[B%d].graph_vs_eager_worst_rel_l2_after_3_steps" % B: max(d / max(n, 1e-30) for d, n in per)})
    assert all(d <= rel * n + floor for d, n in per), [i for i, (d, n) in enumerate(per) if d > rel * n + floor]
    assert float((a.fp.flat - Trainer(_trainable()).fp.flat).abs().max()) > 1e-5, "three steps moved the parameters"


@pytest.mark.parametrize("run", sorted(orc.RUNS))
def test_deterministic_step_is_bit_reproducible(run):
    from smilecode_amd import ops
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(2)
    prev = ops.set_deterministic(True)
    try:
        a, b = Trainer(_trainable(run)), Trainer(_trainable(run))
        a._fwd_bwd(mov, fix)
        g1 = a.fp.grad.clone()
        a._fwd_bwd(mov, fix)
        assert torch.equal(a.fp.grad, g1), "two eager steps of one trainer differ"
        b._fwd_bwd(mov, fix)
        assert torch.equal(b.fp.grad, g1), "two trainers differ"
        assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    finally:
        ops.set_deterministic(prev)


def test_overlapped_allreduce_is_refused():
    from smilecode_amd.engine import Trainer
    with pytest.raises(RuntimeError, match="ModeT's three bucket"):
        Trainer(_trainable(), overlap_allreduce=True)


@pytest.mark.parametrize("run,cls", [("vtn", "VTN"), ("rcn", "RCN")])
def test_state_dict_round_trip_through_a_reference_format_dict(run, cls):
    want = json.load(open(os.path.join(GOLD, "rcn_state_dict.json")))[cls]
    src = _model(run, legacy_grid_buffers=True)
    sd = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    assert {k: list(v.shape) for k, v in sd.items()} == want              # what the reference's load_state_dict(strict=True) needs
    assert torch.equal(sd["transformer.grid"][0, 2, 0, 0, :], torch.arange(128.0))
    dst = _model(run)
    with torch.no_grad():
        for p in dst.parameters():
            p.zero_()
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mov, fix = _pair(1)
    with torch.no_grad():
        ya, fa = src(mov, fix)
        yb, fb = dst(mov, fix)
    assert torch.equal(fa, fb) and torch.equal(ya, yb) and float(fa.abs().max()) > 0.1


def test_train_and_infer_scripts_with_the_model_switch(tmp_path):
    from smilecode_amd import infer, train
    extra = ["--model", "rcn", "--cascades", "2", "--channels", "4"]
    out, stdout = str(tmp_path), sys.stdout
    try:
        train.main(["--synthetic", "4", "--img-size", "64,64,64", "--max-epoch", "1", "--out", out] + extra)
    finally:
        sys.stdout = stdout
    name = "RCN_ncc_1_reg_1_lr_0.0001_54r"
    exp = os.path.join(out, "experiments", name)
    ck = glob.glob(glob.escape(exp) + "/dsc*.pth.tar")
    assert os.path.isdir(exp) and len(ck) == 1 and os.listdir(os.path.join(out, "experiments")) == [name]
    sd = torch.load(ck[0], map_location="cpu")
    assert set(sd) == {"epoch", "state_dict", "best_dsc", "optimizer"} and "vtn.1.Pred0.upconv.weight" in sd["state_dict"]
    assert float(sd["optimizer"]["state"][0]["step"]) == 12.0           # 4 subjects: 12 ordered pairs, one step each
    log = open(os.path.join(out, "logs", name, "logfile.log")).read()
    assert "Iter 12 of 12 loss" in log and "Img Sim:" in log
    d = infer.main(["--synthetic", "2", "--img-size", "64,64,64", "--model-dir", exp + "/"] + extra)
    assert 0.0 <= d <= 1.0
