"""The RDN network and its stride-2 convolution family without a GPU: the oracle against the reference's recorded results, the
header of the family against its ctypes table and the library's exports, the output-size rule and the workspace sizes, every
refusal before a launch, the state-dict keys of both forms, and the --model rdn switch of train.py / infer.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import guard, rdn_oracle as orc
from tests.guard_family import check_family_table, check_header_is_c99
from tests.util import GOLD, digest, gold

NAMES = {"modet_convs2_ws_bytes", "modet_convs2_fwd", "modet_convs2_bwd_data", "modet_convs2_bwd_weight", "modet_cat_channels2_fwd",
         "modet_cat_channels2_bwd"}


def recorded():
    """tests/golden/REPORT_rdn.txt: quantity -> (max|oracle - reference|, max|reference|) as the generator measured them"""
    out = {}
    for line in open(os.path.join(GOLD, "REPORT_rdn.txt")):
        if line.startswith("#") or not line.strip():
            continue
        name, err, mag = line.rstrip("\n").split("\t")
        out[name] = (float(err), float(mag))
    return out


def within_recorded(name, got, want, rec):
    """10 x the recorded deviation (another summation order or thread count).  Where the generator measured 0 another order of an
    n-term fp64 sum moves the result by at most n * 2^-53 * sum|terms|; the longest sums here, the loss and the first layer's
    gradients, have 2 x 49 152 terms, each below the result's recorded maximum"""
    err, mag = rec[name]
    dev = float((got.double() - want.double()).abs().max())
    bound = max(10.0 * err, 98304 * 2.0 ** -53 * mag)
    assert dev <= bound, (name, dev, err, bound)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def e2e_oracle(run, B):
    g = gold("e2e_rdn_32x48x32.npz")
    levels, diff = orc.RUNS[run]
    return orc.value_and_grads(orc.make_weights(channels=int(g["channels"])), T(g["moving"][:B]), T(g["fixed"][:B]), torch.float64, levels, diff)


@pytest.mark.parametrize("run,B", [(r, b) for r in orc.RUNS for b in (1, 2)])
def test_oracle_network_equals_the_reference_golden(run, B):
    g, rec, tag = gold("e2e_rdn_32x48x32.npz"), recorded(), "%s.B%d" % (run, B)
    stride = int(g["stride"])
    loss, sim, reg, y, flow, stage, grads = e2e_oracle(run, B)
    within_recorded("e2e[%s] flow_out" % tag, flow.reshape(-1)[::stride], T(g[tag + ".flow_out"]), rec)
    within_recorded("e2e[%s] y_moved" % tag, y.reshape(-1)[::stride], T(g[tag + ".y_moved"]), rec)
    within_recorded("e2e[%s] stage" % tag, stage.reshape(-1)[::stride], T(g[tag + ".stage"]), rec)
    within_recorded("e2e[%s] loss" % tag, loss, T(g[tag + ".loss"])[0], rec)
    kept = sorted(n for n in grads if "%s.grad.%s" % (tag, n) in g.files)
    want = sorted(n for n in grads if n.startswith(("encoder.", "est0.")) or n.endswith(".bias"))
    assert kept == [n for n in want if not (B == 1 and n == "encoder.conv3.main.weight")] and len(kept) >= 27
    for n in kept:
        within_recorded("e2e[%s] grad %s" % (tag, n), grads[n], T(g["%s.grad.%s" % (tag, n)]), rec)
    # the fields are of the order of a voxel (make_weights scales the flow convolutions for that), and nothing is analytically zero
    assert 0.3 < float(g[tag + ".flow_out_absmax"]) < 8.0 and 0.1 < float(g[tag + ".stage_absmax"]) < 4.0
    assert all(float(v.abs().max()) > 1e-6 for v in grads.values())


def test_oracle_layer_runs_in_fp32_and_follows_the_padding_rule():
    """the ATen yardstick of the GPU tests stays near fp64; with delta weights the layer picks x[2o] (centre tap) and x[2o - 1]"""
    x, w, b, gy = orc.case_tensors(6)
    slope = orc.OP_CASES[6][4]
    r32, r64 = orc.op_value_and_grads(x, w, b, gy, slope, torch.float32), orc.op_value_and_grads(x, w, b, gy, slope, torch.float64)
    for q in ("y", "d_x", "d_w", "d_b"):
        assert r32[q].dtype == torch.float32 and 0 < float((r32[q].double() - r64[q]).abs().max()) < 1e-4 * float(r64[q].abs().max())
    assert r64["y"].shape == (1, 5, 9, 17, 8) and r64["d_x"].shape == x.shape
    wd = torch.zeros_like(w)
    for c in range(4):
        wd[c, c, 1, 1, 1] = 1.0
    y = orc.conv_s2_cl(x, wd, None, None)
    assert torch.equal(y[..., :4], x[:, ::2, ::2, ::2]) and float(y[..., 4:].abs().max()) == 0
    xi, wi, bi, gi = orc.case_tensors(5, "int")
    ri = orc.op_value_and_grads(xi, wi, bi, gi, 0.0, torch.float64)
    assert all(torch.equal(v, v.round()) for v in ri.values())          # ReLU on integers: integer results


def test_masked_share_of_every_case_is_below_the_cap():
    """cases 1 .. 7 keep every cotangent (their tensors are pinned below); from case MASKED_FROM on the outputs within MASK_BELOW of
    zero lose theirs: 1 of case 11's 6 600, about 1e-5 of the larger cases'"""
    from tests import rcn_oracle
    assert (orc.MASK_BELOW, orc.MASK_CAP) == (rcn_oracle.MASK_BELOW, rcn_oracle.MASK_CAP) and orc.MASK_CAP == 0.01
    for n, case in orc.OP_CASES.items():
        share = orc.masked_share(n)
        assert 0.0 <= share <= orc.MASK_CAP, (n, share)
        assert share == 0.0 or (case[4] is not None and n >= orc.MASKED_FROM), n
        if n >= orc.MASKED_FROM and case[4] is not None:
            x, w, b, gy = orc.case_tensors(n)
            near = orc.conv_s2_cl(x.double(), w.double(), b.double(), case[4]).abs() < orc.MASK_BELOW
            assert float(gy[near].abs().sum()) == 0.0 and float(near.double().mean()) == share, n


def test_tensors_of_cases_1_to_7_are_what_they_always_were():
    """goldens, guard files and the frozen yardstick of tests/test_gpu_convs2.py rest on these tensors: a checksum taken before
    the case table grew and tensor construction moved into spec_tensors"""
    assert digest(t for n in range(1, 8) for kind in ("randn", "int") for t in orc.case_tensors(n, kind)) == \
        "19c4a1fba2ff79fa2ee2c1b303fb948a00b379bbff447a055f454dedd410e59e"


def test_new_cases_launch_what_they_are_named_for():
    """the arithmetic behind the comments of OP_CASES 8 .. 11: the weight gradient's row counts and the last split"""
    rows = {}
    for n, (B, (D, H, W), _, cout, _) in orc.OP_CASES.items():
        Do, Ho, Wo = orc.out_shape(D, H, W)
        N, V = B * Do * Ho * Wo, (256 if cout <= 64 else 512 if cout <= 128 else 1024)
        rows[n] = (V, -(-N // V), N - (-(-N // V) - 1) * V)
    assert {n: rows[n] for n in (8, 9, 10, 11)} == {8: (256, 6, 250), 9: (512, 2, 208), 10: (1024, 3, 112), 11: (256, 7, 114)}
    assert all(rows[n][1] in (1, 3) for n in range(1, 8))              # (what cases 1 .. 7 gave the column sum)
    for n in range(8, 12):                                             # integer data: results far below 2^24
        res = orc.op_value_and_grads(*orc.case_tensors(n, "int"), orc.OP_CASES[n][4], torch.float64)
        assert max(float(v.abs().max()) for v in res.values()) < 4e3, n


def test_output_size_rule_for_odd_and_even_dimensions():
    from smilecode_amd import ops
    for n, want in ((1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (8, 4), (9, 5), (17, 9), (33, 17), (160, 80), (192, 96)):
        assert ops.conv3d_s2_out_shape(n, n, n) == (want,) * 3 == orc.out_shape(n, n, n)
        assert torch.nn.functional.conv3d(torch.zeros(1, 1, n, 1, 1), torch.zeros(1, 1, 3, 3, 3), stride=2, padding=1).shape[2] == want
    assert ops.conv3d_s2_out_shape(3, 5, 8) == (2, 3, 4)


# ------------------------------------------------------------------------------------------------ the family
def test_convs2_header_table_and_exports_agree():
    from smilecode_amd import build
    lib = check_family_table("convs2", NAMES, sorted(NAMES - {"modet_convs2_ws_bytes"}))
    assert lib.modet_hip_version() >= 446
    assert "convs2.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "convs2.hip"))


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("convs2", tmp_path, "return modet_convs2_ws_bytes(0, 0, 0, 0, 0, MODET_CONVS2_MAX_CHANNELS, MODET_CONVS2_PASS_FWD) != 0;")


def test_workspace_sizes_and_zero_for_refused_shapes():
    from smilecode_amd import _lib
    lib = _lib.load()
    for n, (B, (D, H, W), cin, cout, _) in orc.OP_CASES.items():
        Do, Ho, Wo = orc.out_shape(D, H, W)
        N, V = B * Do * Ho * Wo, (256 if cout <= 64 else 512 if cout <= 128 else 1024)
        assert lib.modet_convs2_ws_bytes(B, D, H, W, cin, cout, 0) == 27 * cin * cout * 4 == lib.modet_convs2_ws_bytes(B, D, H, W, cin, cout, 1)
        assert lib.modet_convs2_ws_bytes(B, D, H, W, cin, cout, 2) == 2 * -(-N // V) * (27 * cin * cout + cout) * 4, n
    # the RDN encoder at full size with channels = 16: every layer is covered
    for (D, H, W), cin, cout in (((160, 192, 160), 1, 16), ((80, 96, 80), 16, 32), ((40, 48, 40), 32, 64), ((20, 24, 20), 64, 128)):
        assert all(lib.modet_convs2_ws_bytes(2, D, H, W, cin, cout, k) > 0 for k in range(3))
    for bad in ((0, 8, 8, 8, 4, 8), (1, 0, 8, 8, 4, 8), (1, 8, -1, 8, 4, 8), (1, 8, 8, 0, 4, 8), (1, 8, 8, 8, 2, 8), (1, 8, 8, 8, 3, 8),
                (1, 8, 8, 8, 6, 8), (1, 8, 8, 8, 0, 8), (1, 8, 8, 8, 260, 8), (1, 8, 8, 8, 4, 2), (1, 8, 8, 8, 4, 6), (1, 8, 8, 8, 4, 0),
                (1, 8, 8, 8, 4, 260), (1, 8, 8, 8, 4, -4), (1, 1024, 1024, 1024, 4, 8), (8, 1024, 1024, 256, 1, 16)):
        for k in range(3):
            assert lib.modet_convs2_ws_bytes(*bad, k) == 0, (bad, k)
    assert lib.modet_convs2_ws_bytes(1, 8, 8, 8, 4, 8, 3) == 0 and lib.modet_convs2_ws_bytes(1, 8, 8, 8, 4, 8, -1) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL required pointers, refused channel counts, empty axes, a bad activation code or slope, a misaligned tensor and a short
    or misaligned workspace come back as the error codes of modet_hip.h from the host checks (no pointer is dereferenced there)"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL, 16-byte aligned value that is never dereferenced
    NULL, DIM, UNSUP, WS = -1, -2, -3, -4
    ok = (1, 8, 8, 8, 4, 8)

    def size(k, dims):
        return lib.modet_convs2_ws_bytes(*dims, k) or lib.modet_convs2_ws_bytes(*ok, k)

    def fwd(x=p, w=p, b=p, y=p, ws=p, nb=None, dims=ok, act=1, slope=0.2):
        return lib.modet_convs2_fwd(x, w, b, y, ws, size(0, dims) if nb is None else nb, *dims, act, slope, None)

    def bwd_data(dy=p, y=p, w=p, dx=p, ws=p, nb=None, dims=ok, act=1, slope=0.2):
        return lib.modet_convs2_bwd_data(dy, y, w, dx, ws, size(1, dims) if nb is None else nb, *dims, act, slope, None)

    def bwd_weight(x=p, dy=p, y=p, dw=p, db=p, ws=p, nb=None, dims=ok, act=1, slope=0.2):
        return lib.modet_convs2_bwd_weight(x, dy, y, dw, db, ws, size(2, dims) if nb is None else nb, *dims, act, slope, None)

    for k in ("x", "w", "y", "ws"):
        assert fwd(**{k: None}) == NULL, k
    for k in ("dy", "y", "w", "dx", "ws"):
        assert bwd_data(**{k: None}) == NULL, k
    for k in ("x", "dy", "y", "dw", "ws"):
        assert bwd_weight(**{k: None}) == NULL, k
    for i, fn in enumerate((fwd, bwd_data, bwd_weight)):
        for dims in ((0, 8, 8, 8, 4, 8), (1, 0, 8, 8, 4, 8), (1, 8, 8, -3, 4, 8), (1, 1024, 1024, 1024, 4, 8)):
            assert fn(dims=dims) == DIM, (fn.__name__, dims)
        for dims in ((1, 8, 8, 8, 2, 8), (1, 8, 8, 8, 6, 8), (1, 8, 8, 8, 0, 8), (1, 8, 8, 8, 260, 8), (1, 8, 8, 8, 4, 6), (1, 8, 8, 8, 4, 260)):
            assert fn(dims=dims) == UNSUP, (fn.__name__, dims)
        assert fn(act=2) == UNSUP and fn(act=-1) == UNSUP and fn(slope=-0.1) == UNSUP and fn(slope=float("nan")) == UNSUP
        full = lib.modet_convs2_ws_bytes(*ok, i)
        assert fn(nb=full - 1) == WS and fn(nb=0) == WS and fn(ws=p + 4) == WS and fn(ws=p + 8) == WS
    assert fwd(x=p + 4) == UNSUP and fwd(y=p + 8) == UNSUP and bwd_data(dx=p + 4) == UNSUP and bwd_weight(dy=p + 4) == UNSUP
    cat = lambda a=p, b=p, o=p, N=8, C1=4, C2=8: lib.modet_cat_channels2_fwd(a, b, o, N, C1, C2, None)      # noqa: E731
    split = lambda o=p, a=p, b=p, N=8, C1=4, C2=8: lib.modet_cat_channels2_bwd(o, a, b, N, C1, C2, None)    # noqa: E731
    assert cat(a=None) == cat(b=None) == cat(o=None) == NULL and split(o=None) == NULL and split(a=None, b=None) == NULL
    assert cat(N=0) == cat(C1=0) == cat(C2=-1) == split(N=-5) == DIM and cat(N=1 << 28) == DIM and split(N=1 << 40) == DIM
    assert cat(a=p + 4) == UNSUP and split(b=p + 8) == UNSUP and cat(a=p + 2, C1=3) == UNSUP


class _Fake:
    """what ops._chk looks at, for the dtype refusals on a machine without a GPU"""
    is_cuda, data16 = True, None

    def __init__(self, dtype):
        self.dtype = dtype

    def is_contiguous(self):
        return True


def test_ops_check_arguments_before_the_launch(monkeypatch):
    """with tensors that claim to be on the GPU the argument checks still fire first: the library is never reached"""
    from smilecode_amd import _lib, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["convs2"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    x, w, b = torch.zeros(1, 4, 5, 6, 8), torch.zeros(16, 8, 3, 3, 3), torch.zeros(16)
    for fn in (lambda: ops.conv3d_s2(x, w, b, 0.2), lambda: ops.cat_channels(x, x)):
        with pytest.raises(RuntimeError, match="GPU"):             # no CPU fallback: a host tensor is an error, not a slow path
            fn()
    with pytest.raises(RuntimeError, match="float32"):
        ops._convs2_args("conv3d_s2", _Fake(torch.float64), w, b, None)
    handle = _Fake(torch.float32)
    handle.data16 = object()
    with pytest.raises(RuntimeError, match="bf16 feature handle"):
        ops._convs2_args("conv3d_s2", handle, w, b, None)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    bad = [
        (lambda: ops.conv3d_s2(x[0], w, b), r"x must be a channels-last \(B,D,H,W,C\)"),
        (lambda: ops.conv3d_s2(x, w[0], b), "weight must be"),
        (lambda: ops.conv3d_s2(x, torch.zeros(16, 4, 3, 3, 3), b), "weight .* does not match"),
        (lambda: ops.conv3d_s2(x, torch.zeros(16, 8, 3, 3, 1), b), "weight .* does not match"),
        (lambda: ops.conv3d_s2(x, w, torch.zeros(8)), "bias .* does not match"),
        (lambda: ops.conv3d_s2(x, w, b, -0.2), "slope must be"),
        (lambda: ops.conv3d_s2(x, w, b, True), "slope must be"),
        (lambda: ops.conv3d_s2(x, w, b, "0.2"), "slope must be"),
        (lambda: ops.conv3d_s2(torch.zeros(1, 4, 5, 6, 6), torch.zeros(16, 6, 3, 3, 3), b), "x has 6 channels"),
        (lambda: ops.conv3d_s2(torch.zeros(1, 4, 5, 6, 260), torch.zeros(16, 260, 3, 3, 3), b), "x has 260 channels"),
        (lambda: ops.conv3d_s2(x, torch.zeros(6, 8, 3, 3, 3), torch.zeros(6)), "weight has 6 output channels"),
        (lambda: ops.conv3d_s2(x, torch.zeros(260, 8, 3, 3, 3), torch.zeros(260)), "weight has 260 output channels"),
        (lambda: ops.conv3d_s2(torch.zeros(0, 4, 5, 6, 8), w, b), "is empty"),
        (lambda: ops.cat_channels(x, x[0]), "must agree in every dimension but the last"),
        (lambda: ops.cat_channels(x, torch.zeros(1, 4, 5, 7, 8)), "must agree in every dimension but the last"),
        (lambda: ops.cat_channels(x, torch.zeros(1, 4, 5, 6, 0)), "is empty"),
    ]
    for fn, match in bad:
        with pytest.raises(RuntimeError, match=match):
            fn()
    assert not [n for n, _ in px.records if guard.is_launching(n)]


# ------------------------------------------------------------------------------------------------ the modules
def test_state_dict_keys_and_shapes_equal_the_reference():
    from smilecode_amd import models
    want = json.load(open(os.path.join(GOLD, "rdn_state_dict.json")))
    for cls, diff in (("RDN", False), ("RDN_diff", True)):
        legacy = {k: list(v.shape) for k, v in models.RDN((32, 48, 32), channels=4, diff=diff, legacy_grid_buffers=True).state_dict().items()}
        assert legacy == want[cls], cls
        m = models.RDN((32, 48, 32), channels=4, diff=diff)
        plain = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert plain == {k: v for k, v in want[cls].items() if not k.endswith(".grid")}          # as ModeT: dropped unless asked for
        assert {k.split(".conv.")[1].split(".")[0] for k in plain if k.startswith("est")} == {"0", "1", "2", "4"}
        ref_format = {k: torch.randn(v) for k, v in want[cls].items()}
        assert m.load_state_dict(ref_format, strict=True).missing_keys == []
        assert torch.equal(m.est2[0].conv[4].bias.detach(), ref_format["est2.0.conv.4.bias"])
        assert torch.equal(m.encoder.conv1.main.weight.detach(), ref_format["encoder.conv1.main.weight"])
    assert sum(k.startswith("integrate.") for k in want["RDN_diff"]) == 5 and not any(k.startswith("integrate.") for k in want["RDN"])
    # the reference's initial values of the flow convolution: Normal(0, 1e-5) weights, zero bias
    m = models.RDN((32, 32, 32), channels=4)
    for est in (m.est0[0], m.est1[0], m.est2[0], m.est3[0]):
        w = est.conv[4].weight.detach()
        assert float(est.conv[4].bias.detach().abs().max()) == 0 and 0 < float(w.abs().max()) < 1e-4 and 2e-6 < float(w.std()) < 5e-5
    assert m.encoder.conv0.alpha == 0.2 and m.stages == 1 and m.levels == [1, 1, 1, 1] and m.channels == 4 and m.inshape == (32, 32, 32)


def test_rdn_refuses_what_it_cannot_run():
    from smilecode_amd import engine, models
    for shape, match in (((32, 40, 32), "multiple of 16"), ((16, 32, 32), "at least 32"), ((32, 32), "expected"), ((32, 32, 0), "at least 32")):
        with pytest.raises(RuntimeError, match="inshape.*" + match):
            models.RDN(shape, channels=4)
    with pytest.raises(RuntimeError, match="stage_recursion = 2.*ResizeTransform"):
        models.RDN((32, 32, 32), channels=4, stage_recursion=2)
    with pytest.raises(RuntimeError, match="stage_recursion"):
        models.RDN((32, 32, 32), channels=4, stage_recursion=0)
    with pytest.raises(RuntimeError, match="act_dtype"):
        models.RDN((32, 32, 32), channels=4, act_dtype=torch.bfloat16)
    for kw, match in ((dict(channels=3), "channels = 3"), (dict(channels=6), "channels = 6"), (dict(channels=32), "channels = 32"),
                      (dict(channels=4, in_channel=2), "in_channel = 2"), (dict(channels=0), "channels = 0"),
                      (dict(channels=4, level_recursion=[1, 1, 1]), "level_recursion"), (dict(channels=4, level_recursion=[1, 0, 1, 1]), "level_recursion"),
                      (dict(channels=4, diff=True, int_steps=13), "nsteps")):
        with pytest.raises(RuntimeError, match=match):
            models.RDN((32, 32, 32), **kw)
    m = models.RDN((32, 32, 32), channels=4)
    v = torch.zeros(1, 1, 32, 32, 40)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        m(v, v)
    with pytest.raises(RuntimeError, match="same shape"):
        m(v, torch.zeros(1, 1, 32, 32, 32))
    with pytest.raises(RuntimeError, match="ModeT's three bucket"):
        engine.Trainer(m, overlap_allreduce=True)
    assert hasattr(m, "forward_cl") and m.stage_buckets is False and not hasattr(m, "integrate")
    assert len(models.RDN((32, 32, 32), channels=4, diff=True).integrate) == 5
    assert models.rdn_unsupported_config(1, 16) is None and models.rdn_unsupported_config(4, 8) is None


# ------------------------------------------------------------------------------------------------ train.py / infer.py
def test_model_switch_of_the_scripts(capsys):
    from smilecode_amd import infer, train
    ap = train.make_parser()
    a = ap.parse_args(["--model", "rdn"])
    assert a.channels == 16 and a.levels == "1,1,1,1" and train.check_model_args(ap, a) is a
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 1]) == "RDN(1, 1111)_ncc_1_diffusion_1_lr_0.0001/"        # RDN/train.py:51
    a = ap.parse_args(["--model", "rdn", "--levels", "4,3,2,1", "--diff", "--int-steps", "5", "--sim", "mind", "--reg", "bending", "--reg-weight", "0.5"])
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 0.5]) == "RDN(1, 4321)_mind_1_diffusion_bending_0.5_lr_0.0001_diff5/"
    m = train.make_model(ap.parse_args(["--model", "rdn", "--channels", "4", "--levels", "2,1,1,2", "--diff"]), (32, 32, 32))
    assert type(m).__name__ == "RDN" and m.levels == [2, 1, 1, 2] and m.diff and m.channels == 4
    ip = infer.make_parser()
    b = ip.parse_args(["--model", "rdn", "--channels", "4", "--levels", "1,1,1,2"])
    assert train.check_model_args(ip, b) is b and train.make_model(b, (32, 32, 32)).levels == [1, 1, 1, 2]
    for parser, argv in ((ap, ["--model", "rdn", "--overlap-allreduce"]), (ap, ["--model", "rdn", "--levels", "1,1,1"]),
                         (ap, ["--model", "rdn", "--levels", "1,0,1,1"]), (ip, ["--model", "rdn", "--levels", "a,b,c,d"])):
        with pytest.raises(SystemExit) as e:
            train.check_model_args(parser, parser.parse_args(argv))
        assert e.value.code == 2
    assert "--levels" in capsys.readouterr().err
    # the other networks' names do not change
    assert train.save_dir_name(ap.parse_args([]), [8, 4, 2, 1, 1], 6, [1, 1]) == "modet-heads(84211)-rpe_headim_6_ncc_1_reg_1_lr_0.0001_54r/"
    assert train.save_dir_name(ap.parse_args(["--model", "im2grid"]), [8, 4, 2, 1, 1], 6, [1, 1]) == "Im2Grid_ncc_1_reg_1_lr_0.0001_54r/"
