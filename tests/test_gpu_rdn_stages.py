"""-m gpu: RDN with recursive stages and its weight-shared forms (models.RDNStages, models.RDN_share, models.ResizeTransform) on the
MI355X at 32 x 48 x 32 with channels = 4 against the reference's golden vectors (fp64, tests/golden/make_goldens_rdn_stages.py),
measured in units of the error the same composition makes in ATen fp32 on the CPU (tests/rdn_stages_oracle.py in single precision).

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
import torch.nn.functional as F

from tests import rdn_stages_oracle as orc
from tests.util import F32_RUNS, GOLD, f32_inputs, gold, grad_yardstick, note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
SHAPE, CHANNELS = (32, 48, 32), 4
GOLDEN = "e2e_rdn_stages_32x48x32.npz"
RUNS = [(run, B) for run in orc.RUNS for B in (1, 2)]
IDS = ["%s-B%d" % rb for rb in RUNS]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _weights_np(stages, share):
    return {n: v.float().numpy() for n, v in orc.make_weights(stages, share, channels=CHANNELS).items()}


def _model(run="rdn_s2", **kw):
    from smilecode_amd import models
    _, stages, levels, diff, share = orc.RUNS[run]
    m = models.RDNStages(SHAPE, channels=CHANNELS, stage_recursion=stages, level_recursion=list(levels), diff=diff, share=share, **kw).cuda()
    models.load_numpy_weights(m, _weights_np(stages, share))
    return m


def _pair(B):
    g = gold("e2e_rdn_32x48x32.npz")                                   # the pair the staged goldens were computed on
    return T(g["moving"][:B]).cuda(), T(g["fixed"][:B]).cuda()


@functools.lru_cache(maxsize=None)
def _oracle(run, B):
    """(fp64 run, the F32_RUNS fp32 runs) of the oracle on the golden pair: computed once per case, shared by the forward and the
    gradient test"""
    g = gold("e2e_rdn_32x48x32.npz")
    mov, fix = T(g["moving"][:B]), T(g["fixed"][:B])
    _, stages, levels, diff, share = orc.RUNS[run]
    p = orc.make_weights(stages, share, channels=CHANNELS)
    runs = []
    for r in range(F32_RUNS):
        m, f = f32_inputs((mov, fix), r)
        runs.append(orc.value_and_grads(p, m, f, torch.float32, stages, levels, diff, share))
    return orc.value_and_grads(p, mov, fix, torch.float64, stages, levels, diff, share), runs


@pytest.mark.parametrize("run,B", RUNS, ids=IDS)
def test_forward_against_the_golden(run, B):
    g, tag = gold(GOLDEN), "%s.B%d" % (run, B)
    stride, stages = int(g["stride"]), orc.RUNS[run][1]
    _, runs = _oracle(run, B)
    model, (mov, fix) = _model(run, return_stage_flows=True), _pair(B)
    with torch.no_grad():
        outs = model(mov, fix)
        y2, flow2 = _model(run)(mov, fix)                              # the inference contract: two outputs, the same bits
    assert len(outs) == 2 + stages                                     # as the reference
    y, flow, fields = outs[0], outs[1], outs[2:]
    assert tuple(y.shape) == (B, 1) + SHAPE and tuple(flow.shape) == (B, 3) + SHAPE
    assert all(tuple(f.shape) == (B, 3) + tuple(s // 2 for s in SHAPE) for f in fields)
    assert torch.equal(y, y2) and torch.equal(flow, flow2)
    named = [("flow_out", flow, lambda r: r[4]), ("y_moved", y, lambda r: r[3])]
    named += [("stage%d" % i, fields[i], (lambda r, i=i: r[5][i])) for i in range(stages)]
    rep = {}
    for name, got, pick in named:
        ref = T(g["%s.%s" % (tag, name)])
        rep["rdn_stages[%s].%s.e_hip" % (tag, name)] = rel_err(got.reshape(-1)[::stride], ref)
        rep["rdn_stages[%s].%s.e_f32" % (tag, name)] = max(rel_err(pick(r).reshape(-1)[::stride], ref) for r in runs)
    note_many(rep)
    for name, _, _ in named:
        e_hip, e_f32 = rep["rdn_stages[%s].%s.e_hip" % (tag, name)], rep["rdn_stages[%s].%s.e_f32" % (tag, name)]
        assert e_hip <= A * e_f32, "%s %s: e_hip %.3e, ATen fp32 %.3e (A = %g)" % (tag, name, e_hip, e_f32, A)


@pytest.mark.parametrize("run,B", RUNS, ids=IDS)
def test_parameter_gradients_against_the_yardstick(run, B):
    """the reference's loss, NCC(y_moved) + the sum of Grad3d over the stage fields, on the return_stage_flows=True outputs: the
    tensors the golden holds against the reference, the rest against the oracle in fp64, all through grad_yardstick.  With
    share=True an Estimator's gradient is the sum over the stages that reuse it."""
    from smilecode_amd import losses
    g, tag = gold(GOLDEN), "%s.B%d" % (run, B)
    (loss64, _, _, _, _, _, g64), runs = _oracle(run, B)
    g64 = dict(g64)
    n_gold = 0
    for n in g64:
        key = "%s.grad.%s" % (tag, n)
        if key in g.files:
            g64[n] = T(g[key])
            n_gold += 1
    assert n_gold >= 20
    model, (mov, fix) = _model(run, return_stage_flows=True), _pair(B)
    outs = model(mov, fix)
    reg = losses.Grad3d(penalty="l2")
    loss = losses.NCC_vxm()(fix, outs[0]) + sum(reg(f, fix) for f in outs[2:])
    note_many({"rdn_stages[%s].loss_abs_err" % tag: abs(float(loss.detach()) - float(g[tag + ".loss"][0]))})
    loss.backward()
    ghip = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(ghip) == sorted(g64) and all(v is not None for v in ghip.values())
    grad_yardstick("rdn_stages[%s]" % tag, g64, [r[6] for r in runs], ghip)


@pytest.mark.parametrize("diff", [False, True], ids=["plain", "diff"])
def test_one_unshared_stage_is_rdn_bit_for_bit(diff):
    """the same kernels in the same order: outputs and every parameter gradient of the one-stage loss"""
    from smilecode_amd import losses, models, ops
    from tests import rdn_oracle
    w = {n: v.float().numpy() for n, v in rdn_oracle.make_weights(channels=CHANNELS).items()}
    mov, fix = _pair(2)
    prev = ops.set_deterministic(True)                                 # (the warp scatter's atomic order is not part of the claim)
    try:
        res = []
        for cls in (models.RDN, models.RDNStages):
            m = cls(SHAPE, channels=CHANNELS, level_recursion=[2, 1, 1, 2], diff=diff, return_stage_flows=True).cuda()
            models.load_numpy_weights(m, w)
            y, flow, stage = m(mov, fix)
            (losses.NCC_vxm()(fix, y) + losses.Grad3d(penalty="l2")(stage, fix)).backward()
            res.append((y.detach(), flow.detach(), stage.detach(), {n: p.grad for n, p in m.named_parameters()}))
    finally:
        ops.set_deterministic(prev)
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert sorted(a[3]) == sorted(b[3])
    for n in a[3]:
        assert torch.equal(a[3][n], b[3][n]), n
    assert float(a[1].abs().max()) > 0.5


def _rel_l2_per_tensor(tr_a, tr_b):
    out = []
    for (off, n), p in zip(tr_a.fp.offsets, tr_a.fp.params):
        a, b = tr_a.fp.flat[off:off + n].double(), tr_b.fp.flat[off:off + n].double()
        out.append((float((a - b).norm()), float(a.norm())))
    return out


@pytest.mark.parametrize("run", ["rdn_s2", "diff_share_s2"])
def test_trainer_capture_verifies_and_follows_the_eager_steps(run):
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(1)
    make = lambda: _model(run, return_stage_flows=True)               # noqa: E731  (the regulariser sits on every stage field)
    a, b = Trainer(make()), Trainer(make())
    b.capture(mov, fix, verify=True)                                   # raises if a replay does not reproduce the eager gradients
    assert b._graph is not None and torch.equal(a.fp.flat, b.fp.flat)
    for _ in range(3):
        la, lb = a.train_step(mov, fix), b.train_step(mov, fix)
    assert bool(torch.isfinite(la[0])) and abs(float(la[0]) - float(lb[0])) < 1e-5
    rel, floor_frac = a._verify_tolerance()
    per = _rel_l2_per_tensor(a, b)
    floor = floor_frac * max(n for _, n in per)
    note_many({"rdn_stages[%s].graph_vs_eager_worst_rel_l2_after_3_steps" % run: max(d / max(n, 1e-30) for d, n in per)})
    assert all(d <= rel * n + floor for d, n in per), [i for i, (d, n) in enumerate(per) if d > rel * n + floor]
    assert float((a.fp.flat - Trainer(make()).fp.flat).abs().max()) > 1e-5, "three steps moved the parameters"


def test_trainer_loss_is_the_staged_loss():
    """engine.Trainer puts the regulariser on every stage field (reg_on_subflows), not on flow_out: its value is the golden's"""
    from smilecode_amd.engine import Trainer
    g = gold(GOLDEN)
    mov, fix = _pair(2)
    tr = Trainer(_model("share_s3", return_stage_flows=True))
    loss, sim, reg = tr._fwd_bwd(mov, fix)
    want = g["share_s3.B2.loss"]
    assert abs(float(loss) - want[0]) < 2e-4 and abs(float(sim) - want[1]) < 2e-4 and abs(float(reg) - want[2]) < 2e-4
    with pytest.raises(RuntimeError, match="regularises its subflows"):
        Trainer(_model("share_s3"))._fwd_bwd(mov, fix)


@pytest.mark.parametrize("run", sorted(orc.RUNS))
def test_deterministic_step_is_bit_reproducible(run):
    from smilecode_amd import ops
    from smilecode_amd.engine import Trainer
    mov, fix = _pair(2)
    prev = ops.set_deterministic(True)
    try:
        a, b = Trainer(_model(run, return_stage_flows=True)), Trainer(_model(run, return_stage_flows=True))
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
        Trainer(_model(return_stage_flows=True), overlap_allreduce=True)


@pytest.mark.parametrize("factor,shape", [(0.5, (9, 11, 33)), (2, (3, 4, 5)), (0.25, (16, 24, 16))])
def test_resize_transform_against_the_reference_module(factor, shape):
    """the reference's ResizeTransform.forward restated on ATen in fp64 (interpolate then scale for factor < 1, scale then
    interpolate for factor > 1); HIP within A = 4 x the same composition in ATen fp32, value and input gradient"""
    from smilecode_amd import models
    g = torch.Generator().manual_seed(17)
    x = torch.randn((2, 3) + shape, generator=g)

    def ref(x, dtype):
        xr = x.to(dtype).clone().requires_grad_(True)
        if factor < 1:
            y = factor * F.interpolate(xr, align_corners=True, scale_factor=factor, mode="trilinear")
        else:
            y = F.interpolate(factor * xr, align_corners=True, scale_factor=factor, mode="trilinear")
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(18)).to(dtype)
        (dx,) = torch.autograd.grad(y, [xr], gy)
        return y.detach(), dx, gy
    y64, dx64, gy = ref(x, torch.float64)
    y32, dx32, _ = ref(x, torch.float32)
    xg = x.cuda().requires_grad_(True)
    m = models.ResizeTransform(factor, 3)
    y = m(xg)
    (dx,) = torch.autograd.grad(y, [xg], gy.float().cuda())
    assert tuple(y.shape) == tuple(y64.shape)
    rep = {"e_hip.out": rel_err(y, y64), "e_f32.out": rel_err(y32, y64), "e_hip.d_x": rel_err(dx, dx64), "e_f32.d_x": rel_err(dx32, dx64)}
    note_many({"resize_transform[%g].%s" % (factor, k): v for k, v in rep.items()})
    assert rep["e_hip.out"] <= A * rep["e_f32.out"] and rep["e_hip.d_x"] <= A * rep["e_f32.d_x"], rep
    y_cl = m.forward_cl(xg.detach().permute(0, 2, 3, 4, 1).contiguous())
    assert torch.equal(y_cl.permute(0, 4, 1, 2, 3), y.detach())


@pytest.mark.parametrize("run,cls", [("rdn_s2", "RDN"), ("share_s3", "RDN_share"), ("diff_s2", "RDN_diff"), ("diff_share_s2", "RDN_diff_share")])
def test_state_dict_round_trip_through_a_reference_format_dict(run, cls):
    want = json.load(open(os.path.join(GOLD, "rdn_stages_state_dict.json")))[cls]
    src = _model(run, legacy_grid_buffers=True)
    sd = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    assert {k: list(v.shape) for k, v in sd.items()} == want              # what the reference's load_state_dict(strict=True) needs
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


def test_train_and_infer_scripts_with_stages_and_share(tmp_path):
    from smilecode_amd import infer, train
    extra = ["--model", "rdn", "--stages", "2", "--share", "--channels", "4", "--levels", "1,1,1,1"]
    out, stdout = str(tmp_path), sys.stdout
    try:
        train.main(["--synthetic", "4", "--img-size", "32,48,32", "--max-epoch", "1", "--out", out] + extra)
    finally:
        sys.stdout = stdout
    name = "RDN_share(2, 1111)_ncc_1_diffusion_1_lr_0.0001"
    exp = os.path.join(out, "experiments", name)
    ck = glob.glob(glob.escape(exp) + "/dsc*.pth.tar")
    assert os.path.isdir(exp) and len(ck) == 1 and os.listdir(os.path.join(out, "experiments")) == [name]
    sd = torch.load(ck[0], map_location="cpu")
    assert set(sd) == {"epoch", "state_dict", "best_dsc", "optimizer"}
    assert "est3.conv.4.weight" in sd["state_dict"] and "est3.0.conv.4.weight" not in sd["state_dict"]
    assert float(sd["optimizer"]["state"][0]["step"]) == 12.0           # 4 subjects: 12 ordered pairs, one step each
    log = open(os.path.join(out, "logs", name, "logfile.log")).read()
    assert "Iter 12 of 12 loss" in log and "Img Sim:" in log
    d = infer.main(["--synthetic", "2", "--img-size", "32,48,32", "--model-dir", exp + "/"] + extra)
    assert 0.0 <= d <= 1.0
