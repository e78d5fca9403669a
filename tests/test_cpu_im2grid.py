"""The Im2Grid network and its positional-encoding family without a GPU: the oracle against the reference's recorded results, the
header of the family against its ctypes table and the library's exports, the workspace size, every refusal before a launch, the
state-dict keys, and the --model switch of train.py / infer.py."""
import argparse
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import guard, im2grid_oracle as orc
from tests.guard_family import check_family_table, check_header_is_c99
from tests.util import GOLD, gold

OP_CASES = ("b2_2x3x5_c8", "b1_7x6x19_c16", "b1_3x5x17_c32", "b2_4x7x9_c64", "b1_2x3x4_c128")
NAMES = {"modet_posenc_ws_bytes", "modet_posenc_fwd_pair", "modet_posenc_bwd_data_pair", "modet_posenc_bwd_params_pair"}


def recorded():
    """tests/golden/REPORT_im2grid.txt: quantity -> (max|oracle - reference|, max|reference|) as the generator measured them"""
    out = {}
    for line in open(os.path.join(GOLD, "REPORT_im2grid.txt")):
        if line.startswith("#") or not line.strip():
            continue
        name, err, mag = line.rstrip("\n").split("\t")
        out[name] = (float(err), float(mag))
    return out


def within_recorded(name, got, want, rec):
    """10 x the recorded deviation (another summation order).  Where the generator measured 0 -- the oracle and the reference
    were the same fp64 operations in the same order there -- another order of an n-term fp64 sum moves the result by at most
    n * 2^-53 * sum|terms|; every sum here has fewer than 4096 terms, each below the result's recorded maximum."""
    err, mag = rec[name]
    dev = float((got.double() - want.double()).abs().max())
    bound = max(10.0 * err, 4096 * 2.0 ** -53 * mag)
    assert dev <= bound, (name, dev, err, bound)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("tag", OP_CASES)
def test_oracle_layer_equals_the_reference_golden(tag):
    g, gx, rec = gold("op_posenc.npz"), gold("op_posenc_dx.npz"), recorded()
    o = [T(g[tag + "." + n]).double().requires_grad_(True) for n in ("x1", "x2", "Wt", "b", "alpha")]
    gy1, gy2 = T(g[tag + ".gy1"]).double(), T(g[tag + ".gy2"]).double()
    y1, y2 = orc.posenc_cl(o[0], o[2], o[3], o[4]), orc.posenc_cl(o[1], o[2], o[3], o[4])
    dx1, dx2, dW, db, da = torch.autograd.grad([y1, y2], o, [gy1, gy2])
    assert y1.shape == tuple(g[tag + ".x1"].shape[:-1]) + (6,) and float(g[tag + ".alpha"][0]) != 1.0 and np.abs(g[tag + ".Wt"]).min() > 0
    within_recorded("op[%s] y" % tag, torch.stack((y1, y2)).detach(), torch.stack((T(g[tag + ".y1"]), T(g[tag + ".y2"]))), rec)
    within_recorded("op[%s] d_x" % tag, torch.stack((dx1, dx2)), torch.stack((T(gx[tag + ".dx1"]), T(gx[tag + ".dx2"]))), rec)
    within_recorded("op[%s] d_W" % tag, dW, T(g[tag + ".dW"]), rec)
    within_recorded("op[%s] d_b" % tag, db, T(g[tag + ".db"]), rec)
    within_recorded("op[%s] d_alpha" % tag, da, T(g[tag + ".dalpha"]), rec)
    # the embedding deviation is recorded, not hidden: the reference forms it in fp32
    assert rec["op[%s] y" % tag][0] > 1e-9 and rec["op[%s] d_x" % tag][0] < 1e-12


@functools.lru_cache(maxsize=None)
def e2e_oracle(B):
    g = gold("e2e_im2grid_32x48x32.npz")
    return orc.value_and_grads(orc.make_weights(), T(g["moving"][:B]), T(g["fixed"][:B]), torch.float64)


@pytest.mark.parametrize("B", [1, 2])
def test_oracle_network_equals_the_reference_golden(B):
    g, rec, tag = gold("e2e_im2grid_32x48x32.npz"), recorded(), "B%d" % B
    stride = int(g["stride"])
    loss, sim, reg, y, flow, grads = e2e_oracle(B)
    within_recorded("e2e[%s] flow" % tag, flow.reshape(-1)[::stride], T(g[tag + ".flow"]), rec)
    within_recorded("e2e[%s] y_moved" % tag, y.reshape(-1)[::stride], T(g[tag + ".y_moved"]), rec)
    within_recorded("e2e[%s] loss" % tag, loss, T(g[tag + ".loss"])[0], rec)
    small = sorted(n for n in grads if n.startswith("peblock"))
    assert len(small) == 15
    for n in small:
        within_recorded("e2e[%s] grad %s" % (tag, n), grads[n], T(g["%s.grad.%s" % (tag, n)]), rec)
    p = orc.make_weights()
    for n in small:                                         # the fixture's weights are the oracle's: seeded, NON-zero, alpha != 1
        assert np.array_equal(g["weight." + n], p[n].float().numpy()) and float(p[n].abs().min()) > 0
        assert "alpha" not in n or float(p[n]) != 1.0


def test_oracle_runs_in_fp32_too():
    """the ATen yardstick of the GPU tests: the same composition in single precision stays near the fp64 one"""
    g = gold("op_posenc.npz")
    tag = OP_CASES[1]
    a = [T(g[tag + "." + n]) for n in ("x1", "Wt", "b", "alpha")]
    y32, y64 = orc.posenc_cl(*a), orc.posenc_cl(*(t.double() for t in a))
    assert y32.dtype == torch.float32 and 0 < float((y32.double() - y64).abs().max()) < 1e-5
    e = orc.embedding(3, 4, 5)
    assert e.shape == (3, 4, 5, 6) and float(e[0, 0, 0, 0]) == 1.0 and float(e[2, 0, 0, 0]) == -1.0 and float(e[0, 3, 0, 2]) == -1.0
    assert float(e[0, 0, 4, 4]) == -1.0 and abs(float(e[1, 0, 0, 1]) - 1.0) < 1e-15 and abs(float(e[0, 0, 2, 5]) - 1.0) < 1e-15


# ------------------------------------------------------------------------------------------------ the family
def test_posenc_header_table_and_exports_agree():
    lib = check_family_table("posenc", NAMES, sorted(NAMES - {"modet_posenc_ws_bytes"}))
    assert lib.modet_hip_version() >= 445


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("posenc", tmp_path, "return modet_posenc_ws_bytes(0, 0, 0, 0, 0, MODET_POSENC_DIM) != 0;")


def test_workspace_is_zero_for_uncovered_shapes():
    from smilecode_amd import _lib
    lib = _lib.load()
    for cin in (4, 8, 16, 32, 64, 128, 12, 100):
        nb = lib.modet_posenc_ws_bytes(1, 160, 192, 160, cin, 6)
        assert 0 < nb <= 2 * 1024 * (6 * cin + 7) * 4 and nb % 16 == 0 and nb == lib.modet_posenc_ws_bytes(1, 160, 192, 160, cin, 6), cin
        assert 0 < lib.modet_posenc_ws_bytes(2, 2, 2, 2, cin, 6) <= nb
    for bad in ((0, 8, 8, 8, 8, 6), (-1, 8, 8, 8, 8, 6), (1, 1, 8, 8, 8, 6), (1, 8, 1, 8, 8, 6), (1, 8, 8, 1, 8, 6), (1, 8, 8, 0, 8, 6),
                (1, 8, 8, 8, 0, 6), (1, 8, 8, 8, 6, 6), (1, 8, 8, 8, 132, 6), (1, 8, 8, 8, -8, 6), (1, 8, 8, 8, 8, 5), (1, 8, 8, 8, 8, 12),
                (1, 8, 8, 8, 8, 0), (1, 2048, 2048, 2048, 8, 6), (1, 1000, 500, 37, 8, 6), (4, 1024, 1024, 512, 8, 6)):
        assert lib.modet_posenc_ws_bytes(*bad) == 0, bad


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """other widths, NULL required pointers, one pointer of a NULL-together pair, axes below 2 and a short or misaligned workspace
    come back as the error codes of modet_hip.h from the host checks (the pointers are never dereferenced on these paths)"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL value that is never dereferenced
    NULL, DIM, UNSUP, WS = -1, -2, -3, -4
    ok = (1, 8, 8, 8, 8, 6)

    def fwd(x1=p, x2=p, Wt=p, b=p, alpha=p, tab=p, y1=p, y2=p, dims=ok):
        return lib.modet_posenc_fwd_pair(x1, x2, Wt, b, alpha, tab, y1, y2, *dims, None)

    def bwd_data(dy1=p, dy2=p, Wt=p, dx1=p, dx2=p, dims=ok):
        return lib.modet_posenc_bwd_data_pair(dy1, dy2, Wt, dx1, dx2, *dims, None)

    def bwd_params(x1=p, dy1=p, x2=p, dy2=p, tab=p, dW=p, db=p, da=p, ws=p, nb=None, dims=ok):
        size = lib.modet_posenc_ws_bytes(*ok) if nb is None else nb
        return lib.modet_posenc_bwd_params_pair(x1, dy1, x2, dy2, tab, dW, db, da, ws, size, *dims, None)

    for k in ("x1", "Wt", "b", "alpha", "tab", "y1"):
        assert fwd(**{k: None}) == NULL, k
    assert fwd(x2=None) == NULL and fwd(y2=None) == NULL                  # x2 and y2 are NULL together
    for k in ("Wt", "dy1", "dy2"):
        assert bwd_data(**{k: None}) == NULL, k
    assert bwd_data(dx1=None, dx2=None) == NULL                            # one of the two data gradients is wanted
    for k in ("x1", "dy1", "tab", "dW", "db", "da", "ws"):
        assert bwd_params(**{k: None}) == NULL, k
    assert bwd_params(x2=None) == NULL and bwd_params(dy2=None) == NULL
    for fn in (fwd, bwd_data, bwd_params):
        for dims in ((0, 8, 8, 8, 8, 6), (1, 1, 8, 8, 8, 6), (1, 8, 1, 8, 8, 6), (1, 8, 8, 1, 8, 6), (1, 8, 8, -3, 8, 6),
                     (1, 2048, 2048, 2048, 8, 6)):
            assert fn(dims=dims) == DIM, (fn.__name__, dims)
        for dims in ((1, 8, 8, 8, 8, 12), (1, 8, 8, 8, 8, 5), (1, 8, 8, 8, 8, 0), (1, 8, 8, 8, 6, 6), (1, 8, 8, 8, 0, 6), (1, 8, 8, 8, 132, 6),
                     (1, 1000, 500, 37, 8, 6)):
            assert fn(dims=dims) == UNSUP, (fn.__name__, dims)
    full = lib.modet_posenc_ws_bytes(*ok)
    assert bwd_params(nb=full - 1) == WS and bwd_params(nb=0) == WS
    assert bwd_params(ws=p + 4) == WS and bwd_params(ws=p + 8) == WS


class _Fake:
    """what ops._chk looks at, for the dtype refusals on a machine without a GPU"""
    is_cuda, data16 = True, None

    def __init__(self, dtype):
        self.dtype = dtype

    def is_contiguous(self):
        return True


def test_ops_check_arguments_before_the_launch(monkeypatch):
    """with tensors that claim to be on the GPU the argument checks still fire first: the library is never reached"""
    from smilecode_amd import _lib, models, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["posenc"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    x, W, b, al = torch.zeros(1, 4, 5, 6, 8), torch.zeros(6, 8), torch.zeros(6), torch.ones(1)
    tab = ops.posenc_table(4, 5, 6)
    assert tab.shape == (15, 2) and tab.dtype == torch.float32
    for fn in (lambda: ops.posenc(x, W, b, al, tab), lambda: ops.posenc_pair(x, x, W, b, al, tab)):
        with pytest.raises(RuntimeError, match="GPU"):             # no CPU fallback: a host tensor is an error, not a slow path
            fn()
    with pytest.raises(RuntimeError, match="float32"):
        ops._posenc_args("posenc", _Fake(torch.float64), None, W, b, al, tab)
    with pytest.raises(RuntimeError, match="float32"):
        ops._posenc_args("posenc", _Fake(torch.bfloat16), None, W, b, al, tab)
    handle = _Fake(torch.float32)
    handle.data16 = object()
    with pytest.raises(RuntimeError, match="bf16 feature handle"):
        ops._posenc_args("posenc_pair", x, handle, W, b, al, tab)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    bad = [
        (lambda: ops.posenc(x[0], W, b, al, tab), r"\(B,D,H,W,C\)"),
        (lambda: ops.posenc_pair(x, torch.zeros(1, 4, 5, 7, 8), W, b, al, tab), "does not match"),
        (lambda: ops.posenc_pair(x, torch.zeros(2, 4, 5, 6, 8), W, b, al, tab), "does not match"),
        (lambda: ops.posenc_pair(x, None, W, b, al, tab), "x2 is missing"),
        (lambda: ops.posenc(x, torch.zeros(12, 8), torch.zeros(12), al, tab), "dim = 6 only"),
        (lambda: ops.posenc(x, torch.zeros(6, 16), b, al, tab), "does not match"),
        (lambda: ops.posenc(x, W, torch.zeros(5), al, tab), "does not match"),
        (lambda: ops.posenc(x, W, b, torch.ones(2), tab), "does not match"),
        (lambda: ops.posenc(x, W, b, al, ops.posenc_table(4, 5, 7)), "does not match"),
        (lambda: ops.posenc(torch.zeros(1, 1, 5, 6, 8), W, b, al, tab), "at least 2 voxels"),
        (lambda: ops.posenc(torch.zeros(0, 4, 5, 6, 8), W, b, al, tab), "at least 2 voxels"),
        (lambda: ops.posenc(torch.zeros(1, 4, 5, 6, 6), torch.zeros(6, 6), b, al, tab), "multiple of 4"),
        (lambda: ops.posenc(torch.zeros(1, 4, 5, 6, 132), torch.zeros(6, 132), b, al, tab), "multiple of 4"),
        (lambda: ops.posenc_table(4, 1, 6), "at least 2 voxels"),
        (lambda: models.PositionalEncodingLayer(8, dim=12), "dim = 12"),
        (lambda: models.PositionalEncodingLayer(8)(x[0]), r"\(B,D,H,W,C\)"),
    ]
    for fn, match in bad:
        with pytest.raises(RuntimeError, match=match):
            fn()
    assert not [n for n, _ in px.records if guard.is_launching(n)]


def test_table_is_fp64_rounded_once_and_laid_out_as_the_header_says():
    from smilecode_amd import ops
    D, H, W = 5, 2, 12
    tab = ops.posenc_table(D, H, W)
    for off, n in ((0, D), (D, H), (D + H, W)):
        t = np.arange(n, dtype=np.float64) * (np.pi / (n - 1))
        assert np.array_equal(tab[off:off + n, 0].numpy(), np.cos(t).astype(np.float32))
        assert np.array_equal(tab[off:off + n, 1].numpy(), np.sin(t).astype(np.float32))
    assert float(tab[0, 0]) == 1.0 and float(tab[D - 1, 0]) == -1.0 and float(tab[D + 1, 0]) == -1.0


# ------------------------------------------------------------------------------------------------ the modules
def test_state_dict_keys_and_shapes_equal_the_reference():
    from smilecode_amd import models
    want = json.load(open(os.path.join(GOLD, "im2grid_state_dict.json")))
    assert {k for k in want if k.startswith("peblock")} == {"peblock%d.%s" % (i, s) for i in range(1, 6) for s in ("proj.weight", "proj.bias", "alpha")}
    legacy = {k: list(v.shape) for k, v in models.Im2grid((32, 48, 32), legacy_grid_buffers=True).state_dict().items()}
    assert legacy == want
    m = models.Im2grid((32, 48, 32))
    plain = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert plain == {k: v for k, v in want.items() if not k.startswith("transformer.")}          # as ModeT: dropped unless asked for
    # the reference's initial values, and a round trip through a reference-format dict, strict
    for i in range(1, 6):
        pe = getattr(m, "peblock%d" % i)
        assert float(pe.proj.weight.detach().abs().max()) == 0 and float(pe.proj.bias.detach().abs().max()) == 0
        assert float(pe.alpha.detach()) == 1.0
        assert pe.tab.shape == (sum(s // 2 ** (i - 1) for s in (32, 48, 32)), 2) and "tab" not in dict(pe.state_dict())
    ref_format = {k: torch.randn(v) for k, v in want.items()}
    assert m.load_state_dict(ref_format, strict=True).missing_keys == []
    assert torch.equal(m.peblock3.alpha.detach(), ref_format["peblock3.alpha"]) and torch.equal(m.cotr.grid, ref_format["cotr.grid"])


def test_im2grid_refuses_what_it_cannot_run():
    from smilecode_amd import engine, models
    for shape, match in (((32, 40, 32), "multiple of 16"), ((16, 32, 32), "at least 32"), ((32, 32), "expected"), ((32, 32, 0), "at least 32")):
        with pytest.raises(RuntimeError, match=match):
            models.Im2grid(shape)
    with pytest.raises(RuntimeError, match="act_dtype"):
        models.Im2grid((32, 32, 32), act_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="diff=True"):
        models.Im2grid((32, 32, 32), diff=True)
    with pytest.raises(RuntimeError, match="channels"):
        models.Im2grid((32, 32, 32), channels=5)
    m = models.Im2grid((32, 32, 32))
    v = torch.zeros(1, 1, 32, 32, 40)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        m(v, v)
    with pytest.raises(RuntimeError, match="same shape"):
        m(v, torch.zeros(1, 1, 32, 32, 32))
    with pytest.raises(RuntimeError, match="ModeT's three bucket"):
        engine.Trainer(m, overlap_allreduce=True)
    assert hasattr(m, "forward_cl") and m.flow_multiplier == 1.0 and m.channels == 4 and m.inshape == (32, 32, 32)


# ------------------------------------------------------------------------------------------------ train.py / infer.py
def test_model_switch_of_the_scripts(capsys):
    from smilecode_amd import infer, train
    ap = train.make_parser()
    assert ap.parse_args([]).model == "modet" and infer.make_parser().parse_args([]).model == "modet"
    a = ap.parse_args(["--model", "im2grid"])
    assert a.model == "im2grid" and train.check_model_args(ap, a) is a
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 1]) == "Im2Grid_ncc_1_reg_1_lr_0.0001_54r/"      # Im2Grid/train.py:49
    a = ap.parse_args(["--model", "im2grid", "--sim", "mind", "--reg", "bending", "--reg-weight", "0.5", "--lr", "0.001"])
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 0.5]) == "Im2Grid_mind_1_reg_bending_0.5_lr_0.001_54r/"
    a = ap.parse_args(["--model", "im2grid", "--reg", "itv"])
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 1]) == "Im2Grid_ncc_1_reg_itv_1_lr_0.0001_54r/"
    for parser, argv in ((ap, ["--model", "im2grid", "--diff"]), (ap, ["--model", "im2grid", "--overlap-allreduce"]),
                         (infer.make_parser(), ["--model", "im2grid", "--diff"]), (ap, ["--model", "voxelmorph"])):
        with pytest.raises(SystemExit) as e:
            train.check_model_args(parser, parser.parse_args(argv))
        assert e.value.code == 2
    assert "ModeT's" in capsys.readouterr().err
    assert type(train.make_model(ap.parse_args(["--model", "im2grid"]), (32, 32, 32))).__name__ == "Im2grid"


def test_modet_directory_names_are_unchanged():
    """the names the parent revision gave, literally, with and without --model modet"""
    from smilecode_amd import train
    ap = train.make_parser()
    table = [
        ([], [1, 1], "modet-heads(84211)-rpe_headim_6_ncc_1_reg_1_lr_0.0001_54r/"),
        (["--lr", "0.001"], [1, 1], "modet-heads(84211)-rpe_headim_6_ncc_1_reg_1_lr_0.001_54r/"),
        (["--sim", "mind"], [1, 1], "modet-heads(84211)-rpe_headim_6_mind_1_reg_1_lr_0.0001_54r/"),
        (["--sim", "mi", "--reg", "bending"], [1, 1], "modet-heads(84211)-rpe_headim_6_mi_1_reg_bending_1_lr_0.0001_54r/"),
        (["--reg-weight", "0.5"], [1, 0.5], "modet-heads(84211)-rpe_headim_6_ncc_1_reg_grad3d_0.5_lr_0.0001_54r/"),
        (["--sim", "ssim", "--reg", "itv", "--reg-weight", "2"], [1, 2.0], "modet-heads(84211)-rpe_headim_6_ssim_1_reg_itv_2.0_lr_0.0001_54r/"),
        (["--diff"], [1, 1], "modet-heads(84211)-rpe_headim_6_ncc_1_reg_1_lr_0.0001_54r_diff7/"),
        (["--diff", "--int-steps", "5", "--sim", "lmi"], [1, 1], "modet-heads(84211)-rpe_headim_6_lmi_1_reg_1_lr_0.0001_54r_diff5/"),
    ]
    for argv, weights, want in table:
        for extra in ([], ["--model", "modet"]):
            assert train.save_dir_name(ap.parse_args(argv + extra), [8, 4, 2, 1, 1], 6, weights) == want, argv
    old = argparse.Namespace(sim="ncc", reg="grad3d", lr=0.0001)            # a namespace from before the switch
    assert train.save_dir_name(old, [8, 4, 2, 1, 1], 6, [1, 1]) == table[0][2]
