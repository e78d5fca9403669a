"""The RCN / VTN network and its transposed-convolution family without a GPU: the oracle against the reference's recorded results,
the layer in fp32 and its two forms, the header of the family against its ctypes table and the library's exports, the workspace
sizes, every refusal before a launch, the state-dict keys, and the --model rcn switch of train.py / infer.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import guard, rcn_oracle as orc
from tests.guard_family import check_family_table, check_header_is_c99
from tests.util import GOLD, digest, gold

NAMES = {"modet_deconv4s2_ws_bytes", "modet_deconv4s2_fwd", "modet_deconv4s2_bwd_data", "modet_deconv4s2_bwd_weight"}
NPZ = "e2e_rcn_64x64x128.npz"


def recorded():
    """tests/golden/REPORT_rcn.txt: quantity -> (max|oracle - reference|, max|reference|) as the generator measured them"""
    out = {}
    for line in open(os.path.join(GOLD, "REPORT_rcn.txt")):
        if line.startswith("#") or not line.strip():
            continue
        name, err, mag = line.rstrip("\n").split("\t")
        out[name] = (float(err), float(mag))
    return out


def within_recorded(name, got, want, rec):
    """10 x the recorded deviation (another summation order or thread count).  Where the generator measured 0 another order of an
    n-term fp64 sum moves the result by at most n * 2^-53 * sum|terms|; the longest sums here, the loss and the first layer's
    gradients, have 2 x 524 288 terms, each below the result's recorded maximum"""
    err, mag = rec[name]
    dev = float((got.double() - want.double()).abs().max())
    bound = max(10.0 * err, 1048576 * 2.0 ** -53 * mag)
    assert dev <= bound, (name, dev, err, bound)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def e2e_oracle(run, B):
    n, fm = orc.RUNS[run]
    mov, fix = orc.golden_pair()
    return orc.value_and_grads(orc.golden_weights(run), mov[:B], fix[:B], n, torch.float64, fm)


def test_the_seeded_pair_is_the_generators():
    g = gold(NPZ)
    mov, fix = orc.golden_pair()
    stride = int(g["stride"])
    assert tuple(mov.shape) == (2, 1) + orc.GOLD_SHAPE == tuple(fix.shape) and tuple(g["shape"]) == orc.GOLD_SHAPE
    assert torch.equal(mov.reshape(-1)[::stride], T(g["moving"])) and torch.equal(fix.reshape(-1)[::stride], T(g["fixed"]))
    assert float(mov.double().sum()) == float(g["pair_sum"][0]) and float(fix.double().sum()) == float(g["pair_sum"][1])


@pytest.mark.parametrize("run,B", [("vtn", 1), ("rcn", 2)])
def test_oracle_network_equals_the_reference_golden(run, B):
    """(one batch size per network here: an fp64 evaluation takes seconds on the CPU; the generator's report covers all four)"""
    g, rec, tag = gold(NPZ), recorded(), "%s.B%d" % (run, B)
    stride = int(g["stride"])
    loss, moved, flow, subs, grads = e2e_oracle(run, B)
    named = [("flow", flow), ("moved", moved)] + [("subflow%d" % i, w) for i, w in enumerate(subs)]
    for name, got in named:
        within_recorded("e2e[%s] %s" % (tag, name), got.reshape(-1)[::stride], T(g["%s.%s" % (tag, name)]), rec)
    within_recorded("e2e[%s] loss" % tag, loss, T(g[tag + ".loss"])[0], rec)
    kept = sorted(n for n in grads if "%s.grad.%s" % (tag, n) in g.files)
    # per VTN: 20 biases (10 encoder, Pred6 .. Pred2, Deconv5 .. Deconv1), 5 Upsamp weights, Deconv1, Pred0 and conv1's weight
    assert len(kept) == max(orc.RUNS[run][0], 1) * 28
    for n in kept:
        within_recorded("e2e[%s] grad %s" % (tag, n), grads[n], T(g["%s.grad.%s" % (tag, n)]), rec)
    # THE CONDITION of make_weights: every cascade's subflow is of the order of a voxel, and nothing is analytically zero
    for i, w in enumerate(subs):
        assert orc.SUBFLOW_RANGE[0] <= float(w.abs().max()) <= orc.SUBFLOW_RANGE[1], (tag, i, float(w.abs().max()))
        assert orc.SUBFLOW_RANGE[0] <= float(g["%s.subflow%d_absmax" % (tag, i)]) <= orc.SUBFLOW_RANGE[1]
    assert all(float(v.abs().max()) > 1e-9 for v in grads.values())


def test_report_records_the_subflow_range_of_every_run():
    rec = recorded()
    rng = {k: v for k, v in rec.items() if k.startswith("range[")}
    assert len(rng) == 2 * 1 + 2 * 2                                   # vtn: one flow, rcn: two subflows, B = 1 and 2
    assert all(orc.SUBFLOW_RANGE[0] <= v[1] <= orc.SUBFLOW_RANGE[1] for v in rng.values())
    assert all(v[0] <= 1e-9 * max(v[1], 1.0) for k, v in rec.items() if k.startswith("e2e["))      # the oracle IS the reference


def test_oracle_layer_runs_in_fp32_and_both_forms_are_equal():
    """the ATen yardstick of the GPU tests stays near fp64; the reference's crop form and the padding = 1 form are the same
    function; the index rule of the header, written out, gives the same numbers"""
    x, w, b, gy = orc.case_tensors(6)
    slope = orc.OP_CASES[6][5]
    r32, r64 = orc.op_value_and_grads(x, w, b, gy, slope, torch.float32), orc.op_value_and_grads(x, w, b, gy, slope, torch.float64)
    for q in ("y", "d_x", "d_w", "d_b"):
        assert r32[q].dtype == torch.float32 and 0 < float((r32[q].double() - r64[q]).abs().max()) < 1e-4 * float(r64[q].abs().max())
    assert r64["y"].shape == (1, 18, 34, 66, 4) and r64["d_x"].shape == x.shape
    for n in orc.OP_CASES:
        x, w, b, _ = (None if t is None else t.double() for t in orc.case_tensors(n))
        s = orc.OP_CASES[n][5]
        assert float((orc.deconv_cl(x, w, b, s) - orc.deconv_crop_cl(x, w, b, s)).abs().max()) == 0.0, n
    xi, wi, bi, _ = (None if t is None else t.double() for t in orc.case_tensors(3, "int"))
    assert torch.equal(orc.deconv_by_rule(xi, wi, bi), orc.deconv_cl(xi, wi, bi, None))
    xi, wi, bi, _ = (t.double() for t in orc.case_tensors(1, "int"))
    assert torch.equal(orc.deconv_by_rule(xi, wi, bi), orc.deconv_cl(xi, wi, bi, None))


def test_masked_share_of_every_case_is_below_the_cap():
    for n, case in orc.OP_CASES.items():
        share = orc.masked_share(n)
        assert 0.0 <= share <= orc.MASK_CAP, (n, share)
        assert share == 0.0 or case[5] is not None
    for cin in orc.SWEEP_CIN:                               # the variant sweep of tests/test_gpu_deconv.py, at its own seeds
        for cout in orc.SWEEP_COUT:
            for slope in orc.SWEEP_SLOPES:
                share = orc.spec_tensors(*orc.sweep_spec(cin, cout, slope))[4]
                assert 0.0 <= share <= orc.MASK_CAP and (share == 0.0 or slope is not None), (cin, cout, slope, share)
    seeds = [orc.sweep_spec(ci, co, s)[1] for ci in orc.SWEEP_CIN for co in orc.SWEEP_COUT for s in orc.SWEEP_SLOPES]
    assert len(set(seeds)) == 48 and not set(seeds) & {3000 + n for n in orc.OP_CASES}


def test_tensors_of_cases_1_to_7_are_what_they_always_were():
    """goldens, guard files and the frozen yardstick of tests/test_gpu_deconv.py rest on these tensors: a checksum taken before
    the case table grew and tensor construction moved into spec_tensors"""
    assert digest(t for n in range(1, 8) for kind in ("randn", "int") for t in orc.case_tensors(n, kind)) == \
        "b5d675798a369486a1b7c3d1882303ec5e7a5209a3c2dd4cef566891c5e70abd"


def test_new_cases_launch_what_they_are_named_for():
    """the arithmetic behind the comments of OP_CASES 8 .. 13: the weight gradient's row counts and the last split"""
    rows = {}
    for n, (B, (D, H, W), _, _, _, _) in orc.OP_CASES.items():
        N = B * D * H * W
        V = max(256, -(-N // 256))
        rows[n] = (-(-N // V), N - (-(-N // V) - 1) * V)
    assert {n: rows[n][0] for n in (8, 9, 13)} == {8: 5, 9: 7, 13: 256} and rows[13][1] == 175
    assert all(rows[n][0] in (1, 2, 20) for n in range(1, 8))          # (what cases 1 .. 7 gave the column sum)
    for n in range(8, 14):                                             # integer data: results far below 2^24
        res = orc.op_value_and_grads(*orc.case_tensors(n, "int"), orc.OP_CASES[n][5], torch.float64)
        assert max(float(v.abs().max()) for v in res.values() if v is not None) < 4e3, n


def test_out_shape_rule():
    from smilecode_amd import ops
    for n in (1, 2, 3, 5, 96):
        assert ops.conv_transpose3d_k4s2_out_shape(n, n, n) == (2 * n,) * 3 == orc.out_shape(n, n, n)
        y = torch.nn.functional.conv_transpose3d(torch.zeros(1, 1, n, 1, 1), torch.zeros(1, 1, 4, 4, 4), stride=2, padding=1)
        assert y.shape[2] == 2 * n
    assert ops.conv_transpose3d_k4s2_out_shape(3, 5, 8) == (6, 10, 16)


# ------------------------------------------------------------------------------------------------ the family
def test_deconv_header_table_and_exports_agree():
    from smilecode_amd import build
    lib = check_family_table("deconv", NAMES, sorted(NAMES - {"modet_deconv4s2_ws_bytes"}))
    assert lib.modet_hip_version() == 447
    assert "deconv.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "deconv.hip"))


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("deconv", tmp_path,
                        "return modet_deconv4s2_ws_bytes(0, 0, 0, 0, 0, MODET_DECONV_MAX_CHANNELS, MODET_DECONV_PASS_FWD) != 0;")


def test_workspace_sizes_and_zero_for_refused_shapes():
    from smilecode_amd import _lib
    lib = _lib.load()
    p4 = lambda c: (c + 3) // 4 * 4          # noqa: E731
    for n, (B, (D, H, W), cin, cout, _, _) in orc.OP_CASES.items():
        N = B * D * H * W
        V = max(256, -(-N // 256))
        packed = 64 * p4(cin) * p4(cout) * 4
        assert lib.modet_deconv4s2_ws_bytes(B, D, H, W, cin, cout, 0) == packed == lib.modet_deconv4s2_ws_bytes(B, D, H, W, cin, cout, 1)
        assert lib.modet_deconv4s2_ws_bytes(B, D, H, W, cin, cout, 2) == 2 * -(-N // V) * (64 * p4(cin) * p4(cout) + p4(cout)) * 4, n
    # every transposed convolution of VTN at 192^3 with channels = 8, and every count from 1 to 1024 on either side
    for g, cin, cout in ((3, 256, 128), (3, 3, 3), (6, 259, 64), (12, 131, 32), (24, 67, 16), (48, 35, 8), (96, 19, 3), (48, 3, 3)):
        assert all(lib.modet_deconv4s2_ws_bytes(2, g, g, g, cin, cout, k) > 0 for k in range(3))
    for c in (1, 2, 3, 5, 7, 1023, 1024):
        assert lib.modet_deconv4s2_ws_bytes(1, 2, 2, 2, c, 1, 0) > 0 and lib.modet_deconv4s2_ws_bytes(1, 2, 2, 2, 1, c, 1) > 0
    for bad in ((0, 8, 8, 8, 4, 8), (1, 0, 8, 8, 4, 8), (1, 8, -1, 8, 4, 8), (1, 8, 8, 0, 4, 8), (1, 8, 8, 8, 0, 8), (1, 8, 8, 8, 1025, 8),
                (1, 8, 8, 8, 4, 0), (1, 8, 8, 8, 4, 1025), (1, 8, 8, 8, 4, -4), (1, 1024, 1024, 1024, 1, 1), (1, 512, 512, 512, 4, 8),
                (2, 512, 512, 512, 8, 1)):
        for k in range(3):
            assert lib.modet_deconv4s2_ws_bytes(*bad, k) == 0, (bad, k)
    assert lib.modet_deconv4s2_ws_bytes(1, 8, 8, 8, 4, 8, 3) == 0 and lib.modet_deconv4s2_ws_bytes(1, 8, 8, 8, 4, 8, -1) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL required pointers, refused channel counts, empty axes, a bad activation code or slope, a misaligned tensor and a short
    or misaligned workspace come back as the error codes of modet_hip.h from the host checks (no pointer is dereferenced there)"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL, 16-byte aligned value that is never dereferenced
    NULL, DIM, UNSUP, WS = -1, -2, -3, -4
    ok = (1, 8, 8, 8, 4, 8)

    def size(k, dims):
        return lib.modet_deconv4s2_ws_bytes(*dims, k) or lib.modet_deconv4s2_ws_bytes(*ok, k)

    def fwd(x=p, w=p, b=p, y=p, ws=p, nb=None, dims=ok, act=1, slope=0.1):
        return lib.modet_deconv4s2_fwd(x, w, b, y, ws, size(0, dims) if nb is None else nb, *dims, act, slope, None)

    def bwd_data(dy=p, y=p, w=p, dx=p, ws=p, nb=None, dims=ok, act=1, slope=0.1):
        return lib.modet_deconv4s2_bwd_data(dy, y, w, dx, ws, size(1, dims) if nb is None else nb, *dims, act, slope, None)

    def bwd_weight(x=p, dy=p, y=p, dw=p, db=p, ws=p, nb=None, dims=ok, act=1, slope=0.1):
        return lib.modet_deconv4s2_bwd_weight(x, dy, y, dw, db, ws, size(2, dims) if nb is None else nb, *dims, act, slope, None)

    for k in ("x", "w", "y", "ws"):
        assert fwd(**{k: None}) == NULL, k
    for k in ("dy", "y", "w", "dx", "ws"):
        assert bwd_data(**{k: None}) == NULL, k
    for k in ("x", "dy", "y", "dw", "ws"):
        assert bwd_weight(**{k: None}) == NULL, k
    for i, fn in enumerate((fwd, bwd_data, bwd_weight)):
        for dims in ((0, 8, 8, 8, 4, 8), (1, 0, 8, 8, 4, 8), (1, 8, 8, -3, 4, 8), (1, 8, 8, 8, 0, 8), (1, 8, 8, 8, 4, 0), (1, 512, 512, 512, 4, 8)):
            assert fn(dims=dims) == DIM, (fn.__name__, dims)
        for dims in ((1, 8, 8, 8, 1025, 8), (1, 8, 8, 8, 4, 1028)):
            assert fn(dims=dims) == UNSUP, (fn.__name__, dims)
        assert fn(act=2) == UNSUP and fn(act=-1) == UNSUP and fn(slope=-0.1) == UNSUP and fn(slope=float("nan")) == UNSUP
        full = lib.modet_deconv4s2_ws_bytes(*ok, i)
        assert fn(nb=full - 1) == WS and fn(nb=0) == WS and fn(ws=p + 4) == WS and fn(ws=p + 8) == WS
    assert fwd(x=p + 4) == UNSUP and fwd(y=p + 8) == UNSUP and bwd_data(dx=p + 4) == UNSUP and bwd_weight(dy=p + 4) == UNSUP
    # a count that is no multiple of 4 asks its tensor for 4-byte alignment only
    odd = (1, 8, 8, 8, 3, 3)
    assert fwd(x=p + 4, y=p + 8, dims=odd, ws=None) == NULL and fwd(x=p + 2, dims=odd) == UNSUP


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
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["deconv"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    f = ops.conv_transpose3d_k4s2
    x, w, b = torch.zeros(1, 2, 3, 4, 8), torch.zeros(8, 16, 4, 4, 4), torch.zeros(16)
    with pytest.raises(RuntimeError, match="GPU"):                 # no CPU fallback: a host tensor is an error, not a slow path
        f(x, w, b, 0.1)
    with pytest.raises(RuntimeError, match="float32"):
        ops._deconv_args("conv_transpose3d_k4s2", _Fake(torch.float64), w, b, None)
    handle = _Fake(torch.float32)
    handle.data16 = object()
    with pytest.raises(RuntimeError, match="bf16 feature handle"):
        ops._deconv_args("conv_transpose3d_k4s2", handle, w, b, None)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    bad = [
        (lambda: f(x[0], w, b), r"x must be a channels-last \(B,D,H,W,C\)"),
        (lambda: f(x, w[0], b), "weight must be"),
        (lambda: f(x, torch.zeros(4, 16, 4, 4, 4), b), "weight .* does not match"),
        (lambda: f(x, torch.zeros(16, 8, 4, 4, 4), b), "weight .* does not match"),           # nn.Conv3d's order
        (lambda: f(x, torch.zeros(8, 16, 3, 3, 3), b), "weight .* does not match"),
        (lambda: f(x, w, torch.zeros(8)), "bias .* does not match"),
        (lambda: f(x, w, b, -0.1), "slope must be"),
        (lambda: f(x, w, b, True), "slope must be"),
        (lambda: f(x, w, b, "0.1"), "slope must be"),
        (lambda: f(torch.zeros(1, 2, 3, 4, 1028), torch.zeros(1028, 16, 4, 4, 4), b), "x has 1028 channels"),
        (lambda: f(x, torch.zeros(8, 1028, 4, 4, 4), torch.zeros(1028)), "weight has 1028 output channels"),
        (lambda: f(torch.zeros(0, 2, 3, 4, 8), w, b), "is empty"),
        (lambda: f(torch.zeros(1, 512, 512, 512, 8), w, b), "2\\^31 elements"),
    ]
    for fn, match in bad:
        with pytest.raises(RuntimeError, match=match):
            fn()
    assert not [n for n, _ in px.records if guard.is_launching(n)]


# ------------------------------------------------------------------------------------------------ the modules
def test_state_dict_keys_and_shapes_equal_the_reference():
    from smilecode_amd import models
    want = json.load(open(os.path.join(GOLD, "rcn_state_dict.json")))
    shape = orc.GOLD_SHAPE
    for cls, make in (("VTN", lambda **kw: models.VTN(shape, channels=4, **kw)),
                      ("RCN", lambda **kw: models.RCN(shape, channels=4, n_cascade=2, return_subflows=True, **kw)),
                      ("RCN_test", lambda **kw: models.RCN(shape, channels=4, n_cascade=2, **kw))):
        legacy = {k: list(v.shape) for k, v in make(legacy_grid_buffers=True).state_dict().items()}
        assert legacy == want[cls], cls
        assert list(legacy) == list(want[cls]) or sorted(legacy) == sorted(want[cls])
        m = make()
        plain = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert plain == {k: v for k, v in want[cls].items() if not k.endswith(".grid")}          # as ModeT: dropped unless asked for
        ref_format = {k: torch.randn(v) for k, v in want[cls].items()}
        assert m.load_state_dict(ref_format, strict=True).missing_keys == []
    assert want["RCN"] == want["RCN_test"] and "vtn.1.encoder.conv3.0.main.weight" in want["RCN"]
    assert want["VTN"]["Deconv4.upconv.weight"] == [16 * 4 * 2 + 3, 8 * 4, 4, 4, 4] and "Upsamp6to5.upconv.bias" not in want["VTN"]
    assert {k: v for k, v in want["VTN"].items() if not k.endswith(".grid")} == {k: list(v) for k, v in orc.vtn_shapes(4).items()}
    # the reference's initial values: Pred0 starts as Normal(0, 1e-5); the other layers as nn.ConvTranspose3d does, whose fan-in
    # comes from weight.size(1) = Cout
    m = models.VTN(shape, channels=4)
    w = m.Pred0.upconv.weight.detach()
    assert m.Pred0.upconv.bias is None and 0 < float(w.abs().max()) < 1e-4 and 2e-6 < float(w.std()) < 5e-5
    for layer, cout in ((m.Deconv5, 64), (m.Deconv1, 4), (m.Upsamp3to2, 3)):
        bound = 1.0 / (cout * 64) ** 0.5
        wmax = float(layer.upconv.weight.detach().abs().max())
        assert 0.8 * bound < wmax <= bound, (cout, wmax, bound)
        if layer.upconv.bias is not None:
            assert float(layer.upconv.bias.detach().abs().max()) <= bound
    assert m.encoder.conv1.alpha == 0.1 and m.Deconv5.alpha == 0.1 and m.channels == 4 and m.inshape == shape and m.step == 7
    assert "encoder._wpad" not in m.state_dict() and tuple(m.encoder._wpad.shape) == (4, 54)


def test_rcn_refuses_what_it_cannot_run():
    from smilecode_amd import engine, models
    for cls in (models.VTN, models.RCN):
        name = cls.__name__
        for shape in ((160, 192, 160), (64, 64, 96), (32, 64, 64), (64, 64, 0)):
            with pytest.raises(RuntimeError, match=name + ": inshape.*multiple of 64.*reference itself raises in torch.cat"):
                cls(shape, channels=4)
        with pytest.raises(RuntimeError, match=name + r": inshape: \(D, H, W\) expected"):
            cls((64, 64), channels=4)
        with pytest.raises(RuntimeError, match=name + ": channels = 16.*reference's default of 16 is not built"):
            cls((64, 64, 64))                                            # the reference's default channel count
        for kw, match in ((dict(channels=3), "channels = 3"), (dict(channels=6), "channels = 6"), (dict(channels=12), "channels = 12"),
                          (dict(channels=32), "channels = 32"), (dict(channels=0), "channels = 0"),
                          (dict(channels=4, in_channel=1), "in_channel = 1"), (dict(channels=4, in_channel=4), "in_channel = 4"),
                          (dict(channels=4, act_dtype=torch.bfloat16), "act_dtype")):
            with pytest.raises(RuntimeError, match=name + ": " + match):
                cls((64, 64, 64), **kw)
    for n in (0, -1, True, 2.0):
        with pytest.raises(RuntimeError, match="n_cascade"):
            models.RCN((64, 64, 64), channels=4, n_cascade=n)
    with pytest.raises(RuntimeError, match="kernel 4 and stride 2"):
        models.UpConvBlock(3, 3, kernel_size=3, stride=2)
    with pytest.raises(RuntimeError, match="kernel 4 and stride 2"):
        models.UpConvLeakyReLU(3, 3, 4, 1)
    assert models.rcn_unsupported_config(2, 4) is None and models.rcn_unsupported_config(2, 8) is None
    m = models.RCN((64, 64, 64), channels=4, n_cascade=1)
    v = torch.zeros(1, 1, 64, 64, 96)
    with pytest.raises(RuntimeError, match="RCN.forward: .*multiple of 64"):
        m(v, v)
    with pytest.raises(RuntimeError, match="same shape"):
        m(v, torch.zeros(1, 1, 64, 64, 64))
    with pytest.raises(RuntimeError, match="VTN.forward: .*multiple of 64"):
        models.VTN((64, 64, 64), channels=4)(v, v)
    with pytest.raises(RuntimeError, match="ModeT's three bucket"):
        engine.Trainer(m, overlap_allreduce=True)
    assert hasattr(m, "forward_cl") and m.stage_buckets is False and m.reg_on_subflows is True and m.n == 1
    for other in (models.ModeT, models.Im2grid, models.RDN, models.VTN):
        assert not getattr(other, "reg_on_subflows", False)             # the attribute is RCN's only


def test_trainer_asks_for_the_subflows():
    """the two-output (inference) form has nothing for the regulariser: refused by name before anything runs"""
    from smilecode_amd import engine, models
    tr = engine.Trainer.__new__(engine.Trainer)
    tr.model = models.RCN((64, 64, 64), channels=4, n_cascade=1)
    with pytest.raises(RuntimeError, match="return_subflows=True"):
        tr._reg_fields((torch.zeros(1), torch.zeros(1)))
    a, b, c, d = (torch.zeros(1) for _ in range(4))
    assert [id(t) for t in tr._reg_fields((a, b, c, d))] == [id(c), id(d)]
    tr.model = object()
    assert [id(t) for t in tr._reg_fields((a, b))] == [id(b)]


# ------------------------------------------------------------------------------------------------ train.py / infer.py
def test_model_switch_of_the_scripts(capsys):
    from smilecode_amd import infer, train
    ap = train.make_parser()
    a = ap.parse_args(["--model", "rcn"])
    assert a.channels == 16 and a.cascades == 10 and train.check_model_args(ap, a) is a
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 1]) == "RCN_ncc_1_reg_1_lr_0.0001_54r/"                # RCN/train.py:50
    a = ap.parse_args(["--model", "rcn", "--sim", "mind", "--reg", "bending", "--reg-weight", "0.5"])
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 0.5]) == "RCN_mind_1_reg_bending_0.5_lr_0.0001_54r/"
    args = ap.parse_args(["--model", "rcn", "--channels", "4", "--cascades", "2"])
    m = train.make_model(args, (64, 64, 64), training=True)
    assert type(m).__name__ == "RCN" and m.n == 2 and m.channels == 4 and m.return_subflows and m.vtn[1].flow_multiplier == 2
    ip = infer.make_parser()
    b = ip.parse_args(["--model", "rcn", "--channels", "8", "--cascades", "1"])
    mi = train.make_model(train.check_model_args(ip, b), (64, 64, 64))
    assert mi.n == 1 and mi.channels == 8 and not mi.return_subflows                                             # the two-output form
    for parser, argv in ((ap, ["--model", "rcn", "--overlap-allreduce"]), (ap, ["--model", "rcn", "--diff"]),
                         (ap, ["--model", "rcn", "--cascades", "0"]), (ip, ["--model", "rcn", "--diff"])):
        with pytest.raises(SystemExit) as e:
            train.check_model_args(parser, parser.parse_args(argv))
        assert e.value.code == 2
    assert "--cascades" in capsys.readouterr().err
    # the other networks' names do not change
    assert train.save_dir_name(ap.parse_args([]), [8, 4, 2, 1, 1], 6, [1, 1]) == "modet-heads(84211)-rpe_headim_6_ncc_1_reg_1_lr_0.0001_54r/"
    assert train.save_dir_name(ap.parse_args(["--model", "rdn"]), [8, 4, 2, 1, 1], 6, [1, 1]) == "RDN(1, 1111)_ncc_1_diffusion_1_lr_0.0001/"
