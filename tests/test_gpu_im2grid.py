"""-m gpu: the positional-encoding kernels and the Im2Grid network on the MI355X against the reference's golden vectors (fp64,
tests/golden/make_goldens_im2grid.py), measured in units of the error the same composition makes in ATen fp32 on the CPU
(tests/im2grid_oracle.py run in single precision).

THE RULE (tests/test_gpu_vecint.py's, and its reason): per quantity, HIP's error against the fp64 golden is at most A = 4 times the
LARGEST ATen-fp32 error over the cases of this file -- another summation order plus one noisy ATen sample.  An error is
max|got - ref| / max|ref|.  Every measured figure goes to the parity report (tests.util.note_many) before it is asserted."""
import functools
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import im2grid_oracle as orc
from tests.util import F32_RUNS, GOLD, f32_inputs, gold, grad_yardstick, note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
OP_CASES = ("b2_2x3x5_c8", "b1_7x6x19_c16", "b1_3x5x17_c32", "b2_4x7x9_c64", "b1_2x3x4_c128")
QUANTITIES = ("y", "d_x", "d_W", "d_b", "d_alpha")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _case(tag):
    g, gx = gold("op_posenc.npz"), gold("op_posenc_dx.npz")
    c = {n: T(g["%s.%s" % (tag, n)]) for n in ("x1", "x2", "gy1", "gy2", "Wt", "b", "alpha", "y1", "y2", "dW", "db", "dalpha",
                                             "dW_single", "db_single", "dalpha_single")}
    c["dx1"], c["dx2"] = T(gx[tag + ".dx1"]), T(gx[tag + ".dx2"])
    return c


def _golden(c, pair):
    if pair:
        return {"y": torch.stack((c["y1"], c["y2"])), "d_x": torch.stack((c["dx1"], c["dx2"])), "d_W": c["dW"], "d_b": c["db"],
                "d_alpha": c["dalpha"]}
    return {"y": c["y1"], "d_x": c["dx1"], "d_W": c["dW_single"], "d_b": c["db_single"], "d_alpha": c["dalpha_single"]}


def _aten32(c, pair):
    """the ATen composition in fp32 on the CPU"""
    o = [c[n].clone().requires_grad_(True) for n in ("x1", "x2", "Wt", "b", "alpha")]
    y1 = orc.posenc_cl(o[0], o[2], o[3], o[4])
    if not pair:
        dx, dW, db, da = torch.autograd.grad(y1, [o[0], o[2], o[3], o[4]], c["gy1"])
        return {"y": y1.detach(), "d_x": dx, "d_W": dW, "d_b": db, "d_alpha": da}
    y2 = orc.posenc_cl(o[1], o[2], o[3], o[4])
    dx1, dx2, dW, db, da = torch.autograd.grad([y1, y2], o, [c["gy1"], c["gy2"]])
    return {"y": torch.stack((y1, y2)).detach(), "d_x": torch.stack((dx1, dx2)), "d_W": dW, "d_b": db, "d_alpha": da}


@functools.lru_cache(maxsize=None)
def aten_yardstick():
    """quantity -> the largest ATen-fp32 error over the file's cases, both forms (computed once, shared by every op test)"""
    worst = {q: 0.0 for q in QUANTITIES}
    for tag in OP_CASES:
        c = _case(tag)
        for pair in (True, False):
            got, ref = _aten32(c, pair), _golden(c, pair)
            for q in QUANTITIES:
                worst[q] = max(worst[q], rel_err(got[q], ref[q]))
    note_many({"posenc.aten_f32.%s" % q: v for q, v in worst.items()})
    return worst


def _hip(c, pair, Wt=None, b=None):
    from smilecode_amd import ops
    d = {n: c[n].cuda() for n in ("x1", "x2", "gy1", "gy2", "Wt", "b", "alpha")}
    if Wt is not None:
        d["Wt"], d["b"] = Wt.cuda(), b.cuda()
    for n in ("x1", "x2", "Wt", "b", "alpha"):
        d[n].requires_grad_(True)
    tab = ops.posenc_table(*d["x1"].shape[1:4], device="cuda")
    if not pair:
        y1 = ops.posenc(d["x1"], d["Wt"], d["b"], d["alpha"], tab)
        dx, dW, db, da = torch.autograd.grad(y1, [d["x1"], d["Wt"], d["b"], d["alpha"]], d["gy1"])
        return {"y": y1.detach(), "d_x": dx, "d_W": dW, "d_b": db, "d_alpha": da}
    y1, y2 = ops.posenc_pair(d["x1"], d["x2"], d["Wt"], d["b"], d["alpha"], tab)
    dx1, dx2, dW, db, da = torch.autograd.grad([y1, y2], [d[n] for n in ("x1", "x2", "Wt", "b", "alpha")], [d["gy1"], d["gy2"]])
    return {"y": torch.stack((y1, y2)).detach(), "d_x": torch.stack((dx1, dx2)), "d_W": dW, "d_b": db, "d_alpha": da}


@pytest.mark.parametrize("pair", [True, False], ids=["pair", "single"])
@pytest.mark.parametrize("tag", OP_CASES)
def test_layer_against_the_golden_in_units_of_aten_fp32(tag, pair):
    c, yard = _case(tag), aten_yardstick()
    got, ref = _hip(c, pair), _golden(c, pair)
    errs = {q: rel_err(got[q], ref[q]) for q in QUANTITIES}
    form = "pair" if pair else "single"
    note_many({"posenc[%s,%s].%s.e_hip" % (tag, form, q): e for q, e in errs.items()})
    for q in QUANTITIES:
        assert got[q].numel() == ref[q].numel()
        assert errs[q] <= A * yard[q], "%s %s %s: e_hip %.3e, largest ATen fp32 error %.3e (A = %g)" % (tag, form, q, errs[q], yard[q], A)


@pytest.mark.parametrize("tag", OP_CASES)
def test_zero_projection_gives_alpha_times_the_table_bit_for_bit(tag):
    """Wt = 0 and bias = 0: y = fl(alpha * tab) at every voxel of every batch entry -- the axis order, the table offsets and the
    batch stride, without a tolerance"""
    from smilecode_amd import ops
    c = _case(tag)
    B, D, H, W, Cin = c["x1"].shape
    got = _hip(c, True, Wt=torch.zeros(6, Cin), b=torch.zeros(6))["y"].cpu()
    tab, alpha = ops.posenc_table(D, H, W), c["alpha"]
    assert float(alpha) != 1.0
    at = alpha * tab                                                    # fp32 * fp32, rounded once
    want = torch.empty(D, H, W, 6)
    want[..., 0:2] = at[:D].reshape(D, 1, 1, 2)
    want[..., 2:4] = at[D:D + H].reshape(1, H, 1, 2)
    want[..., 4:6] = at[D + H:].reshape(1, 1, W, 2)
    for u in range(2):
        for bi in range(B):
            assert torch.equal(got[u, bi], want), (tag, u, bi, float((got[u, bi] - want).abs().max()))


@pytest.mark.parametrize("tag", OP_CASES)
def test_pair_equals_two_single_calls_and_two_runs_are_bit_identical(tag):
    from smilecode_amd import ops
    c = _case(tag)
    pair, again = _hip(c, True), _hip(c, True)
    for q in QUANTITIES:
        assert torch.equal(pair[q], again[q]), (tag, q)
    single = _hip(c, False)
    assert torch.equal(pair["y"][0], single["y"]) and torch.equal(pair["d_x"][0], single["d_x"])
    d = {n: c[n].cuda() for n in ("x2", "gy2", "Wt", "b", "alpha")}
    d["x2"].requires_grad_(True)
    tab = ops.posenc_table(*d["x2"].shape[1:4], device="cuda")
    y2 = ops.posenc(d["x2"], d["Wt"], d["b"], d["alpha"], tab)
    (dx2,) = torch.autograd.grad(y2, [d["x2"]], d["gy2"])
    assert torch.equal(pair["y"][1], y2.detach()) and torch.equal(pair["d_x"][1], dx2)
    with torch.no_grad():                                               # without a gradient: the same forward launch
        y1n, y2n = ops.posenc_pair(c["x1"].cuda(), d["x2"].detach(), d["Wt"], d["b"], d["alpha"], tab)
    assert torch.equal(y1n, pair["y"][0]) and torch.equal(y2n, pair["y"][1])


def test_layer_beyond_one_grid_pass():
    """64 x 96 x 96 voxels of 8 channels: more workgroup tiles than either grid cap (csrc/posenc.hip STREAM_GRID, PARAM_GRID), so
    every kernel strides.  No golden of that size is committed: the reference here is the same composition in ATen fp64 on the
    GPU, the yardstick the same in ATen fp32, the rule the file's (A x the ATen-fp32 error of this case)."""
    import torch.nn.functional as F
    from smilecode_amd import ops
    gen = torch.Generator().manual_seed(91)
    B, D, H, W, Cin = 1, 64, 96, 96, 8
    x1, x2 = (torch.randn(B, D, H, W, Cin, generator=gen).cuda() for _ in range(2))
    gy1, gy2 = (torch.randn(B, D, H, W, 6, generator=gen).cuda() for _ in range(2))
    Wt, b, alpha = (torch.randn(6, Cin, generator=gen) / Cin ** 0.5).cuda(), torch.randn(6, generator=gen).cuda(), torch.tensor([1.3]).cuda()
    emb = orc.embedding(D, H, W).cuda()

    def aten(dtype):
        o = [t.to(dtype).requires_grad_(True) for t in (x1, x2, Wt, b, alpha)]
        ys = [F.linear(o[i], o[2], o[3]) + o[4] * emb.to(dtype) for i in (0, 1)]
        return [ys[0].detach(), ys[1].detach()] + list(torch.autograd.grad(ys, o, [gy1.to(dtype), gy2.to(dtype)]))

    ref, f32 = aten(torch.float64), aten(torch.float32)
    o = [t.clone().requires_grad_(True) for t in (x1, x2, Wt, b, alpha)]
    ys = ops.posenc_pair(*o, ops.posenc_table(D, H, W, device="cuda"))
    got = [ys[0].detach(), ys[1].detach()] + list(torch.autograd.grad(list(ys), o, [gy1, gy2]))
    names = ("y1", "y2", "d_x1", "d_x2", "d_W", "d_b", "d_alpha")
    rep = {}
    for n, g_, r_, f_ in zip(names, got, ref, f32):
        rep["posenc[64x96x96].%s.e_hip" % n], rep["posenc[64x96x96].%s.e_f32" % n] = rel_err(g_, r_), rel_err(f_, r_)
    note_many(rep)
    for n in names:
        assert rep["posenc[64x96x96].%s.e_hip" % n] <= A * rep["posenc[64x96x96].%s.e_f32" % n], (n, rep)


def test_module_forward_and_pair_use_the_table_of_the_grid():
    from smilecode_amd import models
    c = _case(OP_CASES[2])
    pe = models.PositionalEncodingLayer(32).cuda()
    with torch.no_grad():
        pe.proj.weight.copy_(c["Wt"]); pe.proj.bias.copy_(c["b"]); pe.alpha.copy_(c["alpha"])
    x1, x2 = c["x1"].cuda(), c["x2"].cuda()
    q, k = pe.forward_pair(x1, x2)
    assert pe.grid_shape == (3, 5, 17) and torch.equal(pe(x1), q) and torch.equal(pe(x2), k)
    assert rel_err(q, c["y1"]) <= A * aten_yardstick()["y"]
    small = x1[:, :2, :3, :4].contiguous()                              # another grid: the table follows
    assert pe(small).shape == (1, 2, 3, 4, 6) and pe.grid_shape == (2, 3, 4)
    assert sorted(pe.state_dict()) == ["alpha", "proj.bias", "proj.weight"]


def test_attention_at_the_width_of_the_layer():
    """one head, C = 6, scale 1, zero bias without a gradient (what CoTr hands the kernel) against oracle.mode_transformer in fp64,
    forward and both gradients, each within A x the same function's ATen-fp32 error"""
    from oracle import modet_torch as mt
    from smilecode_amd import models
    gen = torch.Generator().manual_seed(66)
    shape = (2, 5, 6, 19, 6)
    q, k = torch.randn(shape, generator=gen) * 0.8, torch.randn(shape, generator=gen) * 0.8
    gy = torch.randn((2, 3, 5, 6, 19), generator=gen)

    def run(dtype):
        a, b = q.to(dtype).requires_grad_(True), k.to(dtype).requires_grad_(True)
        out = mt.mode_transformer(a, b, torch.zeros(1, 27, dtype=dtype), 1, 1.0)
        return (out.detach(),) + torch.autograd.grad(out, [a, b], gy.to(dtype))

    ref, f32 = run(torch.float64), run(torch.float32)
    a, b = q.cuda().requires_grad_(True), k.cuda().requires_grad_(True)
    out = models.CoTr().cuda()(a, b)
    assert out.shape == (2, 3, 5, 6, 19)
    got = (out.detach(),) + torch.autograd.grad(out, [a, b], gy.cuda())
    rep = {}
    for name, g_, r_, f_ in zip(("out", "d_q", "d_k"), got, ref, f32):
        rep["cotr6.%s.e_hip" % name], rep["cotr6.%s.e_f32" % name] = rel_err(g_, r_), rel_err(f_, r_)
    note_many(rep)
    for name in ("out", "d_q", "d_k"):
        assert rep["cotr6.%s.e_hip" % name] <= A * rep["cotr6.%s.e_f32" % name], (name, rep)


# ------------------------------------------------------------------------------------------------ end to end, 32 x 48 x 32
SHAPE = (32, 48, 32)


def _weights_np():
    return {n: v.float().numpy() for n, v in orc.make_weights().items()}


def _model():
    from smilecode_amd import models
    m = models.Im2grid(SHAPE).cuda()
    models.load_numpy_weights(m, _weights_np())
    return m


def _pair(B):
    g = gold("e2e_im2grid_32x48x32.npz")
    return T(g["moving"][:B]).cuda(), T(g["fixed"][:B]).cuda()


@functools.lru_cache(maxsize=None)
def _oracle(B):
    """(fp64 run, the F32_RUNS fp32 runs) of the oracle on the golden pair: computed once per batch size, shared by the forward and
    the gradient test (the first of the two pays: 2-3 s of CPU alone, 7-10 s while the suite's background oracle jobs hold the CPUs)"""
    g = gold("e2e_im2grid_32x48x32.npz")
    mov, fix = T(g["moving"][:B]), T(g["fixed"][:B])
    p = orc.make_weights()
    runs = []
    for r in range(F32_RUNS):
        m, f = f32_inputs((mov, fix), r)
        runs.append(orc.value_and_grads(p, m, f, torch.float32))
    return orc.value_and_grads(p, mov, fix, torch.float64), runs


@pytest.mark.parametrize("B", [1, 2])
def test_forward_against_the_golden(B):
    g, tag = gold("e2e_im2grid_32x48x32.npz"), "B%d" % B
    stride = int(g["stride"])
    _, runs = _oracle(B)
    model, (mov, fix) = _model(), _pair(B)
    with torch.no_grad():
        y, flow = model(mov, fix)
    assert tuple(y.shape) == (B, 1) + SHAPE and tuple(flow.shape) == (B, 3) + SHAPE
    rep = {}
    for name, got, idx in (("flow", flow, 4), ("y_moved", y, 3)):
        ref = T(g["%s.%s" % (tag, name)])
        rep["im2grid[%s].%s.e_hip" % (tag, name)] = rel_err(got.reshape(-1)[::stride], ref)
        rep["im2grid[%s].%s.e_f32" % (tag, name)] = max(rel_err(r[idx].reshape(-1)[::stride], ref) for r in runs)
    note_many(rep)
    for name in ("flow", "y_moved"):
        e_hip, e_f32 = rep["im2grid[%s].%s.e_hip" % (tag, name)], rep["im2grid[%s].%s.e_f32" % (tag, name)]
        assert e_hip <= A * e_f32, "%s %s: e_hip %.3e, ATen fp32 %.3e (A = %g)" % (tag, name, e_hip, e_f32, A)


@pytest.mark.parametrize("B", [1, 2])
def test_parameter_gradients_against_the_yardstick(B):
    """NCC + Grad3d: the fifteen peblock gradients against the reference's golden, the encoder's against the oracle in fp64
    (recomputed here: they do not fit a committed file), all through tests.util.grad_yardstick"""
    from smilecode_amd import losses
    g, tag = gold("e2e_im2grid_32x48x32.npz"), "B%d" % B
    (loss64, _, _, _, _, g64), runs = _oracle(B)
    g64 = dict(g64)
    for n in g64:
        if n.startswith("peblock"):
            g64[n] = T(g["%s.grad.%s" % (tag, n)])
    model, (mov, fix) = _model(), _pair(B)
    y, flow = model(mov, fix)
    loss = losses.NCC_vxm()(fix, y) + losses.Grad3d(penalty="l2")(flow, fix)
    note_many({"im2grid[%s].loss_abs_err" % tag: abs(float(loss.detach()) - float(g[tag + ".loss"][0]))})
    loss.backward()
    ghip = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(ghip) == sorted(g64) and all(v is not None for v in ghip.values())
    grad_yardstick("im2grid[%s]" % tag, g64, [r[5] for r in runs], ghip)


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
    note_many({"im2grid[B%d].graph_vs_eager_worst_rel_l2_after_3_steps" % B: max(d / max(n, 1e-30) for d, n in per)})
    assert all(d <= rel * n + floor for d, n in per), [i for i, (d, n) in enumerate(per) if d > rel * n + floor]
    assert float((a.fp.flat - Trainer(_model()).fp.flat).abs().max()) > 1e-5, "three steps moved the parameters"


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


def test_state_dict_round_trip_through_a_reference_format_dict():
    from smilecode_amd import models
    want = json.load(open(os.path.join(GOLD, "im2grid_state_dict.json")))
    src = models.Im2grid(SHAPE, legacy_grid_buffers=True).cuda()
    models.load_numpy_weights(src, _weights_np())
    sd = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    assert {k: list(v.shape) for k, v in sd.items()} == want              # what the reference's load_state_dict(strict=True) needs
    assert torch.equal(sd["transformer.1.grid"][0, 1, 0, :, 0], torch.arange(24.0))
    dst = models.Im2grid(SHAPE).cuda()
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mov, fix = _pair(1)
    with torch.no_grad():
        ya, fa = src(mov, fix)
        yb, fb = dst(mov, fix)
    assert torch.equal(fa, fb) and torch.equal(ya, yb)


def test_train_and_infer_scripts_with_the_model_switch(tmp_path):
    from smilecode_amd import infer, train
    d = infer.main(["--synthetic", "4", "--img-size", "32,48,32", "--model", "im2grid"])
    assert 0.0 <= d <= 1.0
    out, stdout = str(tmp_path), sys.stdout
    try:
        train.main(["--synthetic", "3", "--img-size", "32,48,32", "--max-epoch", "1", "--max-iters", "2", "--out", out, "--model", "im2grid"])
    finally:
        sys.stdout = stdout
    exp = os.path.join(out, "experiments", "Im2Grid_ncc_1_reg_1_lr_0.0001_54r")
    ck = glob.glob(exp + "/dsc*.pth.tar")
    assert os.path.isdir(exp) and len(ck) == 1 and os.listdir(os.path.join(out, "experiments")) == ["Im2Grid_ncc_1_reg_1_lr_0.0001_54r"]
    sd = torch.load(ck[0], map_location="cpu")
    assert set(sd) == {"epoch", "state_dict", "best_dsc", "optimizer"} and "peblock5.alpha" in sd["state_dict"]
    assert float(sd["optimizer"]["state"][0]["step"]) == 2.0
    log = open(os.path.join(out, "logs", "Im2Grid_ncc_1_reg_1_lr_0.0001_54r", "logfile.log")).read()
    assert "Iter 2 of 2 loss" in log and "Img Sim:" in log
    d = infer.main(["--synthetic", "2", "--img-size", "32,48,32", "--model", "im2grid", "--model-dir", exp + "/", "--surface"])
    assert 0.0 <= d <= 1.0
