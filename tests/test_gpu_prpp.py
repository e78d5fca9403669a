"""-m gpu: the PR++ network (models.PRNetplusplus) on the MI355X at 32 x 48 x 32 with first_channel = 4 against the reference's golden
vectors (fp64, tests/golden/make_goldens_prpp.py), measured in units of the error the same composition makes in ATen fp32 on the
CPU (tests/prpp_oracle.py run in single precision).

THE RULE for the outputs (tests/test_gpu_pcnet.py's): HIP's error against the golden is at most A = 4 times the largest error of
F32_RUNS ATen-fp32 runs (tests.util.f32_inputs).  The parameter gradients go through tests.util.grad_yardstick.  An error is
max|got - ref| / max|ref|.  Every measured figure goes to the parity report before it is asserted.  The golden weights give every
block a field of 0.25 .. 1.5 voxels of its own grid (tests/golden/REPORT_prpp.txt, tests/test_cpu_prpp.py): with the reference's
N(0, 1e-5) flow layers every warp and composition would be the identity."""
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import prpp_oracle as orc
from tests.util import F32_RUNS, GOLD, f32_inputs, gold, grad_yardstick, note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
SHAPE, CHANNELS, NPZ = orc.GOLD_SHAPE, orc.GOLD_CHANNELS, "e2e_prpp_32x48x32.npz"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _load(m, p):
    from smilecode_amd import models
    models.load_numpy_weights(m, {n: v.float().numpy() for n, v in p.items()})
    return m


def _model(**kw):
    from smilecode_amd import models
    return _load(models.PRNetplusplus(SHAPE, first_channel=CHANNELS, **kw).cuda(), orc.golden_weights())


def _pair(B):
    mov, fix = orc.golden_pair()
    return mov[:B].cuda(), fix[:B].cuda()


@functools.lru_cache(maxsize=None)
def _oracle_outputs(B):
    """(loss, moved, flow) of the F32_RUNS fp32 runs: forward passes without a tape"""
    mov, fix = (t[:B] for t in orc.golden_pair())
    p32 = {k: v.float() for k, v in orc.golden_weights().items()}
    with torch.no_grad():
        return [orc.train_loss(p32, *f32_inputs((mov, fix), r)) for r in range(F32_RUNS)]


def _reference_loss(fix, moved, flow):
    """NCC(moved) + Grad3d('l2')(flow) ("Baseline methods/PR++/train.py":98-126)"""
    from smilecode_amd import losses
    return losses.NCC_vxm()(fix, moved) + losses.Grad3d(penalty="l2")(flow, fix)


@pytest.mark.parametrize("B", [1, 2])
def test_forward_against_the_golden(B):
    g, tag = gold(NPZ), "B%d" % B
    stride = int(g["stride"])
    runs = _oracle_outputs(B)
    model, (mov, fix) = _model(), _pair(B)
    with torch.no_grad():
        moved, flow = model(mov, fix)
        moved_cl, flow_cl = model.forward_cl(mov, fix)
    assert tuple(moved.shape) == (B, 1) + SHAPE and tuple(flow.shape) == (B, 3) + SHAPE
    assert torch.equal(flow_cl.permute(0, 4, 1, 2, 3), flow) and torch.equal(moved_cl.permute(0, 4, 1, 2, 3), moved)
    rep = {}
    for name, got, pick in (("flow", flow, lambda r: r[2]), ("moved", moved, lambda r: r[1])):
        ref = T(g["%s.%s" % (tag, name)])
        rep["prpp[%s].%s.e_hip" % (tag, name)] = rel_err(got.reshape(-1)[::stride], ref)
        rep["prpp[%s].%s.e_f32" % (tag, name)] = max(rel_err(pick(r).reshape(-1)[::stride], ref) for r in runs)
    note_many(rep)
    for name in ("flow", "moved"):
        e_hip, e_f32 = rep["prpp[%s].%s.e_hip" % (tag, name)], rep["prpp[%s].%s.e_f32" % (tag, name)]
        assert e_hip <= A * e_f32, "%s %s: e_hip %.3e, ATen fp32 %.3e (A = %g)" % (tag, name, e_hip, e_f32, A)


def _case(tag, shape, channels, grads):
    """a configuration without a committed golden against the oracle in fp64, by the file's rules: the weights are scaled on the
    pair of that shape so that every block's field is of the order of a voxel (asserted: inside half .. twice FIELD_RANGE);
    ``grads``: also every parameter gradient of the reference's loss through grad_yardstick"""
    from smilecode_amd import models
    mov, fix = (t[:1] for t in orc.golden_pair(shape))
    p = orc.golden_weights(channels, shape)
    taps = {}
    if grads:
        ref = orc.net_value_and_grads(p, mov, fix, torch.float64, taps)
        runs = [orc.net_value_and_grads(p, *f32_inputs((mov, fix), r), torch.float32) for r in range(F32_RUNS)]
    else:
        p32 = {k: v.float() for k, v in p.items()}
        with torch.no_grad():
            ref = orc.train_loss(p, mov.double(), fix.double(), taps=taps)
            runs = [orc.train_loss(p32, *f32_inputs((mov, fix), r)) for r in range(F32_RUNS)]
    cond = orc.field_conditions(taps)
    note_many({"%s.max_w%d" % (tag, k): a for k, (a, _) in cond.items()})
    assert all(orc.FIELD_RANGE[0] / 2 <= a <= 2 * orc.FIELD_RANGE[1] for a, _ in cond.values()), cond
    m = _load(models.PRNetplusplus(shape, first_channel=channels).cuda(), p)
    with torch.set_grad_enabled(grads):
        moved, flow = m(mov.cuda(), fix.cuda())
    rep = {}
    for name, got, k in (("flow", flow, 2), ("moved", moved, 1)):
        rep["%s.%s.e_hip" % (tag, name)] = rel_err(got, ref[k])
        rep["%s.%s.e_f32" % (tag, name)] = max(rel_err(r[k], ref[k]) for r in runs)
    note_many(rep)
    for name in ("flow", "moved"):
        assert rep["%s.%s.e_hip" % (tag, name)] <= A * rep["%s.%s.e_f32" % (tag, name)], (name, rep)
    if not grads:
        return
    loss = _reference_loss(fix.cuda(), moved, flow)
    note_many({"%s.loss_abs_err" % tag: abs(float(loss.detach()) - float(ref[0]))})
    loss.backward()
    ghip = {n: q.grad for n, q in m.named_parameters()}
    assert sorted(ghip) == sorted(ref[3]) and all(v is not None for v in ghip.values())
    grad_yardstick(tag, ref[3], [r[3] for r in runs], ghip)


def test_parameter_gradients_against_the_yardstick():
    """B = 1 at 16 x 32 x 16 with first_channel = 4 (a 2 x 4 x 2 grid at 1/8: the smallest legal size at which that grid is not
    degenerate), every parameter gradient against the oracle in fp64; the golden's own gradients (the reference's, B = 1 and
    B = 2) are pinned on the CPU, against the oracle (tests/test_cpu_prpp.py)"""
    _case("prpp[16x32x16]", (16, 32, 16), CHANNELS, grads=True)


def test_eight_channels_against_the_oracle():
    """first_channel = 8 at 32^3, the outputs: rows of 43 / 59 / 91 floats through the stride-1 kernels"""
    _case("prpp[c8,32^3]", (32, 32, 32), 8, grads=False)


def test_eight_channel_rows_through_the_data_gradients():
    """first_channel = 8 at 32^3: one backward pass through the 43- / 59- / 91-channel convolutions' data gradients, finite and
    not zero, and the same bits twice in deterministic mode"""
    from smilecode_amd import models, ops
    shape = (32, 32, 32)
    mov, fix = (t[:1].cuda() for t in orc.golden_pair(shape))
    m = _load(models.PRNetplusplus(shape, first_channel=8).cuda(), orc.golden_weights(8, shape))
    prev = ops.set_deterministic(True)
    try:
        got = []
        for _ in range(2):
            m.zero_grad()
            moved, flow = m(mov, fix)
            _reference_loss(fix, moved, flow).backward()
            got.append({n: q.grad.clone() for n, q in m.named_parameters()})
    finally:
        ops.set_deterministic(prev)
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in got[0].values())
    assert all(torch.equal(got[0][n], got[1][n]) for n in got[0])


def test_every_convolution_weight_is_a_parameter_itself(monkeypatch):
    """a train step packs every stride-1 convolution weight up front from the address it had in the pass before
    (ops.StepContext.prepacked), so no temporary -- a concatenated or sliced copy -- may reach a convolution as its weight, and
    with [moving; fixed] as one batch every weight is the operand of exactly one convolution per pass"""
    from smilecode_amd import ops
    model, (mov, fix) = _model(), _pair(1)
    params = {id(p): n for n, p in model.named_parameters()}
    seen = []
    for name in ("conv3d", "conv3d_s2"):
        real = getattr(ops, name)

        def spy(*a, _real=real, _name=name, **k):
            seen.append((_name, params.get(id(a[1]))))
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    model(mov, fix)
    assert all(n is not None for _, n in seen), seen
    names = [n for _, n in seen]
    assert len(names) == len(set(names)) == 10 + 5 * 5 and sum(k == "conv3d_s2" for k, _ in seen) == 4
    assert sorted(names) == sorted(n for n in params.values() if n.endswith(".weight"))


def test_trainer_loss_is_the_reference_loss():
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(1)
    tr = Trainer(_model())
    with torch.no_grad():
        moved, flow = tr.model(mov, fix)
        want = _reference_loss(fix, moved, flow)
        loss, sim, reg = tr.loss(mov, fix)
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want)) and float(reg) > 0


@pytest.mark.parametrize("B", [1, 2])
def test_trainer_capture_verifies_and_three_captured_steps_equal_three_eager_steps(B):
    from smilecode_amd import ops
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(B)
    prev = ops.set_deterministic(True)
    try:
        a, b = Trainer(_model()), Trainer(_model())
        b.capture(mov, fix, verify=True)                               # raises if a replay does not reproduce the eager gradients
        assert b._graph is not None and torch.equal(a.fp.flat, b.fp.flat)
        for _ in range(3):
            la, lb = a.train_step(mov, fix), b.train_step(mov, fix)
        assert bool(torch.isfinite(la[0])) and float(la[0]) == float(lb[0])
        assert torch.equal(a.fp.flat, b.fp.flat), "three captured steps differ from three eager steps"
        assert float((a.fp.flat - Trainer(_model()).fp.flat).abs().max()) > 1e-5, "three steps moved the parameters"
    finally:
        ops.set_deterministic(prev)


def test_deterministic_step_is_bit_reproducible():
    from smilecode_amd import ops
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(2)
    prev = ops.set_deterministic(True)
    try:
        a, b = Trainer(_model()), Trainer(_model())
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


def test_state_dict_round_trip_through_a_reference_format_dict():
    want = json.load(open(os.path.join(GOLD, "prpp_state_dict.json")))["PRNetplusplus(32x48x32, first_channel=4)"]
    src = _model(legacy_grid_buffers=True)
    sd = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    assert {k: list(v.shape) for k, v in sd.items()} == want              # what the reference's load_state_dict(strict=True) needs
    assert torch.equal(sd["transformers.0.grid"][0, 1, 0, :, 0], torch.arange(48.0))
    dst = _model()
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
    """fresh child processes, each under a time limit"""
    extra = ["--model", "prpp", "--channels", "4", "--img-size", "32,48,32"]
    out = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "smilecode_amd.train", "--synthetic", "4", "--max-epoch", "1", "--out", out] + extra, cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    name = "PRNetplusplus_ncc_1_reg_1_lr_0.0001_54r"
    exp = os.path.join(out, "experiments", name)
    ck = glob.glob(glob.escape(exp) + "/dsc*.pth.tar")
    assert os.path.isdir(exp) and len(ck) == 1 and os.listdir(os.path.join(out, "experiments")) == [name]
    sd = torch.load(ck[0], map_location="cpu")
    assert set(sd) == {"epoch", "state_dict", "best_dsc", "optimizer"} and "prblock2.conv1.0.weight" in sd["state_dict"]
    assert float(sd["optimizer"]["state"][0]["step"]) == 12.0           # 4 subjects: 12 ordered pairs, one step each
    log = open(os.path.join(out, "logs", name, "logfile.log")).read()
    assert "Iter 12 of 12 loss" in log and "Img Sim:" in log
    r = subprocess.run([sys.executable, "-m", "smilecode_amd.infer", "--synthetic", "4", "--model-dir", exp + "/"] + extra, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "dice" in (r.stdout + r.stderr).lower() or "dsc" in (r.stdout + r.stderr).lower()
