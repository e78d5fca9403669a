"""-m gpu: the RDN network (models.RDN, diff off and on) on the MI355X at 32 x 48 x 32 with channels = 4 against the reference's golden
vectors (fp64, tests/golden/make_goldens_rdn.py), measured in units of the error the same composition makes in ATen fp32 on the CPU
(tests/rdn_oracle.py run in single precision).

THE RULE for the outputs (tests/test_gpu_im2grid.py's): HIP's error against the golden is at most A = 4 times the largest error of
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

from tests import rdn_oracle as orc
from tests.util import F32_RUNS, GOLD, f32_inputs, gold, grad_yardstick, note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
SHAPE, CHANNELS = (32, 48, 32), 4
RUNS = [(run, B) for run in orc.RUNS for B in (1, 2)]
IDS = ["%s-B%d" % rb for rb in RUNS]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _weights_np():
    return {n: v.float().numpy() for n, v in orc.make_weights(channels=CHANNELS).items()}


def _model(run="rdn", **kw):
    from smilecode_amd import models
    levels, diff = orc.RUNS[run]
    m = models.RDN(SHAPE, channels=CHANNELS, level_recursion=list(levels), diff=diff, **kw).cuda()
    models.load_numpy_weights(m, _weights_np())
    return m


def _pair(B):
    g = gold("e2e_rdn_32x48x32.npz")
    return T(g["moving"][:B]).cuda(), T(g["fixed"][:B]).cuda()


@functools.lru_cache(maxsize=None)
def _oracle(run, B):
    """(fp64 run, the F32_RUNS fp32 runs) of the oracle on the golden pair: computed once per case, shared by the forward and the
    gradient test"""
    g = gold("e2e_rdn_32x48x32.npz")
    mov, fix = T(g["moving"][:B]), T(g["fixed"][:B])
    p = orc.make_weights(channels=CHANNELS)
    levels, diff = orc.RUNS[run]
    runs = []
    for r in range(F32_RUNS):
        m, f = f32_inputs((mov, fix), r)
        runs.append(orc.value_and_grads(p, m, f, torch.float32, levels, diff))
    return orc.value_and_grads(p, mov, fix, torch.float64, levels, diff), runs


@pytest.mark.parametrize("run,B", RUNS, ids=IDS)
def test_forward_against_the_golden(run, B):
    g, tag = gold("e2e_rdn_32x48x32.npz"), "%s.B%d" % (run, B)
    stride = int(g["stride"])
    _, runs = _oracle(run, B)
    model, (mov, fix) = _model(run, return_stage_flows=True), _pair(B)
    with torch.no_grad():
        y, flow, stage = model(mov, fix)
        y2, flow2 = _model(run)(mov, fix)                              # the inference contract: two outputs, the same bits
    assert tuple(y.shape) == (B, 1) + SHAPE and tuple(flow.shape) == (B, 3) + SHAPE
    assert tuple(stage.shape) == (B, 3) + tuple(s // 2 for s in SHAPE)
    assert torch.equal(y, y2) and torch.equal(flow, flow2)
    rep = {}
    for name, got, idx in (("flow_out", flow, 4), ("y_moved", y, 3), ("stage", stage, 5)):
        ref = T(g["%s.%s" % (tag, name)])
        rep["rdn[%s].%s.e_hip" % (tag, name)] = rel_err(got.reshape(-1)[::stride], ref)
        rep["rdn[%s].%s.e_f32" % (tag, name)] = max(rel_err(r[idx].reshape(-1)[::stride], ref) for r in runs)
    note_many(rep)
    for name in ("flow_out", "y_moved", "stage"):
        e_hip, e_f32 = rep["rdn[%s].%s.e_hip" % (tag, name)], rep["rdn[%s].%s.e_f32" % (tag, name)]
        assert e_hip <= A * e_f32, "%s %s: e_hip %.3e, ATen fp32 %.3e (A = %g)" % (tag, name, e_hip, e_f32, A)


@pytest.mark.parametrize("run,B", RUNS, ids=IDS)
def test_parameter_gradients_against_the_yardstick(run, B):
    """the reference's loss at one stage, NCC(y_moved) + Grad3d(stage field) on the return_stage_flows=True outputs: the tensors the
    golden holds against the reference, the rest against the oracle in fp64 (recomputed here), all through grad_yardstick"""
    from smilecode_amd import losses
    g, tag = gold("e2e_rdn_32x48x32.npz"), "%s.B%d" % (run, B)
    (loss64, _, _, _, _, _, g64), runs = _oracle(run, B)
    g64 = dict(g64)
    n_gold = 0
    for n in g64:
        key = "%s.grad.%s" % (tag, n)
        if key in g.files:
            g64[n] = T(g[key])
            n_gold += 1
    assert n_gold >= 24
    model, (mov, fix) = _model(run, return_stage_flows=True), _pair(B)
    y, flow, stage = model(mov, fix)
    loss = losses.NCC_vxm()(fix, y) + losses.Grad3d(penalty="l2")(stage, fix)
    note_many({"rdn[%s].loss_abs_err" % tag: abs(float(loss.detach()) - float(g[tag + ".loss"][0]))})
    loss.backward()
    ghip = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(ghip) == sorted(g64) and all(v is not None for v in ghip.values())
    grad_yardstick("rdn[%s]" % tag, g64, [r[6] for r in runs], ghip)


def test_default_channel_count_against_the_oracle():
    """channels = 16, the reference's default, at 32 x 32 x 32: Estimator widths 32, 64, 128 and 256 through the stride-1 kernels and
    the encoder's 1 -> 16 .. 64 -> 128 layers, outputs and every parameter gradient against the oracle in fp64 (no golden of this
    configuration is committed), by the file's rules"""
    from smilecode_amd import losses, models, synth
    shape, tag = (32, 32, 32), "rdn[c16,32^3]"
    mov, fix = (T(a) for a in synth.make_pair(shape, 24, batch=1))
    p = orc.make_weights(channels=16)
    ref = orc.value_and_grads(p, mov, fix, torch.float64)
    runs = [orc.value_and_grads(p, *f32_inputs((mov, fix), r), torch.float32) for r in range(F32_RUNS)]
    m = models.RDN(shape, channels=16, return_stage_flows=True).cuda()
    models.load_numpy_weights(m, {n: v.float().numpy() for n, v in p.items()})
    y, flow, stage = m(mov.cuda(), fix.cuda())
    rep = {}
    for name, got, idx in (("flow_out", flow, 4), ("y_moved", y, 3), ("stage", stage, 5)):
        rep["%s.%s.e_hip" % (tag, name)] = rel_err(got, ref[idx])
        rep["%s.%s.e_f32" % (tag, name)] = max(rel_err(r[idx], ref[idx]) for r in runs)
    note_many(rep)
    for name in ("flow_out", "y_moved", "stage"):
        assert rep["%s.%s.e_hip" % (tag, name)] <= A * rep["%s.%s.e_f32" % (tag, name)], (name, rep)
    loss = losses.NCC_vxm()(fix.cuda(), y) + losses.Grad3d(penalty="l2")(stage, fix.cuda())
    loss.backward()
    grad_yardstick(tag, ref[6], [r[6] for r in runs], {n: q.grad for n, q in m.named_parameters()})


def _rel_l2_per_tensor(tr_a, tr_b):
    out = []
    for (off, n), p in zip(tr_a.fp.offsets, tr_a.fp.params):
        a, b = tr_a.fp.flat[off:off + n].double(), tr_b.fp.flat[off:off + n].double()
        out.append((float((a - b).norm()), float(a.norm())))
    return out


@pytest.mark.parametrize("B", [1, 2])
def test_trainer_capture_verifies_and_follows_the_eager_steps(B):
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(B)
    a, b = Trainer(_model()), Trainer(_model())
    b.capture(mov, fix, verify=True)                                   # raises if a replay does not reproduce the eager gradients
    assert b._graph is not None and torch.equal(a.fp.flat, b.fp.flat)
    for _ in range(3):
        la, lb = a.train_step(mov, fix), b.train_step(mov, fix)
    assert bool(torch.isfinite(la[0])) and abs(float(la[0]) - float(lb[0])) < 1e-5
    rel, floor_frac = a._verify_tolerance()
    per = _rel_l2_per_tensor(a, b)
    floor = floor_frac * max(n for _, n in per)
    note_many({"rdn[B%d].graph_vs_eager_worst_rel_l2_after_3_steps" % B: max(d / max(n, 1e-30) for d, n in per)})
    assert all(d <= rel * n + floor for d, n in per), [i for i, (d, n) in enumerate(per) if d > rel * n + floor]
    assert float((a.fp.flat - Trainer(_model()).fp.flat).abs().max()) > 1e-5, "three steps moved the parameters"


@pytest.mark.parametrize("run", sorted(orc.RUNS))
def test_deterministic_step_is_bit_reproducible(run):
    from smilecode_amd import ops
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(2)
    prev = ops.set_deterministic(True)
    try:
        a, b = Trainer(_model(run)), Trainer(_model(run))
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
        Trainer(_model(), overlap_allreduce=True)


@pytest.mark.parametrize("run,cls", [("rdn", "RDN"), ("rdn_diff", "RDN_diff")])
def test_state_dict_round_trip_through_a_reference_format_dict(run, cls):
    want = json.load(open(os.path.join(GOLD, "rdn_state_dict.json")))[cls]
    src = _model(run, legacy_grid_buffers=True)
    sd = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    assert {k: list(v.shape) for k, v in sd.items()} == want              # what the reference's load_state_dict(strict=True) needs
    assert torch.equal(sd["transformer.1.grid"][0, 1, 0, :, 0], torch.arange(24.0))
    if run == "rdn_diff":
        assert torch.equal(sd["integrate.2.transformer.grid"][0, 2, 0, 0, :], torch.arange(8.0))
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


@pytest.mark.parametrize("diff", [False, True], ids=["plain", "diff"])
def test_train_and_infer_scripts_with_the_model_switch(tmp_path, diff):
    from smilecode_amd import infer, train
    extra = ["--model", "rdn", "--channels", "4", "--levels", "1,1,1,2"] + (["--diff"] if diff else [])
    out, stdout = str(tmp_path), sys.stdout
    try:
        train.main(["--synthetic", "4", "--img-size", "32,48,32", "--max-epoch", "1", "--out", out] + extra)
    finally:
        sys.stdout = stdout
    name = "RDN(1, 1112)_ncc_1_diffusion_1_lr_0.0001" + ("_diff7" if diff else "")
    exp = os.path.join(out, "experiments", name)
    ck = glob.glob(glob.escape(exp) + "/dsc*.pth.tar")
    assert os.path.isdir(exp) and len(ck) == 1 and os.listdir(os.path.join(out, "experiments")) == [name]
    sd = torch.load(ck[0], map_location="cpu")
    assert set(sd) == {"epoch", "state_dict", "best_dsc", "optimizer"} and "est3.0.conv.4.weight" in sd["state_dict"]
    assert float(sd["optimizer"]["state"][0]["step"]) == 12.0           # 4 subjects: 12 ordered pairs, one step each
    log = open(os.path.join(out, "logs", name, "logfile.log")).read()
    assert "Iter 12 of 12 loss" in log and "Img Sim:" in log
    d = infer.main(["--synthetic", "2", "--img-size", "32,48,32", "--model-dir", exp + "/"] + extra)
    assert 0.0 <= d <= 1.0
