"""RDN with recursive stages, its weight-shared forms and the resize family without a GPU: the header of the family against its
ctypes table and the library's exports, the oracle's resize against F.interpolate, the staged oracle against the reference's
recorded results, the state-dict keys of the four classes, every refusal before a launch, and --stages / --share of the scripts."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import guard, rdn_oracle, rdn_stages_oracle as orc
from tests.guard_family import check_family_table, check_header_is_c99
from tests.util import GOLD, gold

NAMES = {"modet_resize_fwd", "modet_resize_bwd", "modet_resize_pyramid_fwd", "modet_resize_pyramid_bwd"}
GOLDEN = "e2e_rdn_stages_32x48x32.npz"
SHAPE = (32, 48, 32)
# the reference's class -> what builds it here
CLASSES = {"RDN": dict(stage_recursion=2), "RDN_diff": dict(stage_recursion=2, diff=True),
           "RDN_share": dict(stage_recursion=3, share=True), "RDN_diff_share": dict(stage_recursion=2, share=True, diff=True)}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def recorded():
    """tests/golden/REPORT_rdn_stages.txt: quantity -> (max|oracle - reference|, max|reference|) as the generator measured them"""
    out = {}
    for line in open(os.path.join(GOLD, "REPORT_rdn_stages.txt")):
        if line.startswith("#") or not line.strip():
            continue
        name, err, mag = line.rstrip("\n").split("\t")
        out[name] = (float(err), float(mag))
    return out


def within_recorded(name, got, want, rec):
    """tests/test_cpu_rdn.py's rule: 10 x the recorded deviation, or where that is 0 the movement of a 2 x 49 152-term fp64 sum"""
    err, mag = rec[name]
    dev = float((got.double() - want.double()).abs().max())
    bound = max(10.0 * err, 98304 * 2.0 ** -53 * mag)
    assert dev <= bound, (name, dev, err, bound)


# ------------------------------------------------------------------------------------------------ the family
def test_resize_header_table_and_exports_agree():
    from smilecode_amd import build
    lib = check_family_table("resize", NAMES, sorted(NAMES))
    assert lib.modet_hip_version() == 447
    assert "resize.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "resize.hip"))


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("resize", tmp_path, "return modet_resize_fwd(0, 0, 1, 1, 1, 1, 1, 1, 1, MODET_RESIZE_MAX_C, 1.0f, 0) != "
                        "MODET_RESIZE_PYRAMID_MIN;")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL pointers and refused sizes come back as the error codes of modet_hip.h from the host checks (nothing is dereferenced)"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p, NULL, DIM = 4096, -1, -2
    ok = (1, 4, 5, 6, 2, 3, 9, 3)

    def one(fn, a=p, b=p, dims=ok, scale=1.0):
        return fn(a, b, *dims, scale, None)

    for fn in (lib.modet_resize_fwd, lib.modet_resize_bwd):
        assert one(fn, a=None) == NULL and one(fn, b=None) == NULL
        for i in range(8):
            for bad in (0, -1):
                assert one(fn, dims=ok[:i] + (bad,) + ok[i + 1:]) == DIM, (fn.__name__, i, bad)
        assert one(fn, dims=(65536,) + ok[1:]) == DIM and one(fn, dims=ok[:7] + (257,)) == DIM
        assert one(fn, scale=float("nan")) == DIM and one(fn, scale=float("inf")) == DIM
    pf, pb = lib.modet_resize_pyramid_fwd, lib.modet_resize_pyramid_bwd
    assert pf(None, p, p, p, 1, 8, 8, 8, None) == NULL and pf(p, None, None, None, 1, 8, 8, 8, None) == NULL
    assert pb(p, p, p, None, None, 1, 8, 8, 8, None) == NULL and pb(None, None, None, p, p, 1, 8, 8, 8, None) == NULL
    for dims in ((0, 8, 8, 8), (65536, 8, 8, 8), (1, 7, 8, 8), (1, 8, 7, 8), (1, 8, 8, 7), (1, 8, 8, -8)):
        assert pf(p, p, None, None, *dims, None) == DIM and pb(None, p, None, None, p, *dims, None) == DIM, dims


class _Fake:
    """what ops._chk looks at, for the dtype refusals on a machine without a GPU"""
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype

    def is_contiguous(self):
        return True


def test_ops_check_arguments_before_the_launch(monkeypatch):
    from smilecode_amd import _lib, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["resize"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    x = torch.zeros(1, 8, 9, 10, 3)
    for fn in (lambda: ops.resize(x, (4, 4, 4)), lambda: ops.flow_pyramid(x)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()
    with pytest.raises(RuntimeError, match="float32"):
        ops._resize_args("resize", _Fake(torch.float64), (4, 4, 4), 1.0)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    bad = [
        (lambda: ops.resize(x[0], (4, 4, 4)), r"x must be a channels-last \(B,D,H,W,C\)"),
        (lambda: ops.resize(x, (4, 4)), "size .* three positive integers"),
        (lambda: ops.resize(x, (4, 0, 4)), "size .* three positive integers"),
        (lambda: ops.resize(x, (4, 2.5, 4)), "size .* three positive integers"),
        (lambda: ops.resize(x[:0], (4, 4, 4)), "is empty"),
        (lambda: ops.resize(torch.zeros(1, 2, 2, 2, 257), (4, 4, 4)), "1 to 256 channels"),
        (lambda: ops.resize(x, (4, 4, 4), float("nan")), "scale"),
        (lambda: ops.flow_pyramid(x[0]), r"flow must be a channels-last \(B,D,H,W,C\)"),
        (lambda: ops.flow_pyramid(torch.zeros(1, 8, 8, 8, 4)), "3 channels"),
        (lambda: ops.flow_pyramid(torch.zeros(1, 8, 7, 8, 3)), "at least 8 voxels"),
    ]
    for fn, match in bad:
        with pytest.raises(RuntimeError, match=match):
            fn()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    assert ops.flow_pyramid_sizes(80, 96, 80) == ((40, 48, 40), (20, 24, 20), (10, 12, 10))
    assert ops.flow_pyramid_sizes(9, 11, 33) == ((4, 5, 16), (2, 2, 8), (1, 1, 4))


# ------------------------------------------------------------------------------------------------ the oracle
def _interp(x, size, scale):
    return scale * F.interpolate(x.permute(0, 4, 1, 2, 3), size=size, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)


def test_oracle_resize_equals_interpolate_in_fp64():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 7, 9, 33, 3, generator=g, dtype=torch.float64)
    assert float((orc.resize(x, (3, 4, 5)) - _interp(x, (3, 4, 5), 1.0)).abs().max()) <= 1e-14
    for n, (B, si, so, C, scale) in orc.OP_CASES.items():
        if n == 9:
            continue                                                   # (the largest one: nothing the others lack on the CPU)
        x, gy = (t.double() for t in orc.case_tensors(n))
        res = orc.op_value_and_grad(x, gy, so, scale, torch.float64)
        xr = x.clone().requires_grad_(True)
        y = _interp(xr, so, scale)
        (dx,) = torch.autograd.grad(y, [xr], gy)
        assert float((res["out"] - y.detach()).abs().max()) <= 1e-14 * max(1.0, abs(scale)), n
        assert float((res["d_x"] - dx).abs().max()) <= 1e-13 * max(1.0, abs(scale)), n
    # nnf.interpolate(scale_factor=) sizes its output floor(S * factor): the pyramid's sizes
    f = torch.zeros(1, 3, 9, 11, 33)
    for k, want in ((0.5, (4, 5, 16)), (0.25, (2, 2, 8)), (0.125, (1, 1, 4))):
        assert tuple(F.interpolate(f, scale_factor=k, mode="trilinear", align_corners=True).shape[2:]) == want
    assert [tuple(t.shape[1:4]) for t in orc.flow_pyramid(f.permute(0, 2, 3, 4, 1))] == [(4, 5, 16), (2, 2, 8), (1, 1, 4)]


def test_exact_cases_of_the_oracle():
    """integer ratios pick voxels; an identity resize only scales: in fp32 too, where the kernel is held to the same"""
    x, gy = orc.case_tensors(1)
    res = orc.op_value_and_grad(x, gy, (5, 4, 2), 0.5, torch.float32)
    assert torch.equal(res["out"], 0.5 * x[:, ::2, ::4, ::32])
    want = torch.zeros_like(x)
    want[:, ::2, ::4, ::32] = 0.5 * gy
    assert torch.equal(res["d_x"], want)
    x, gy = orc.case_tensors(8)
    assert torch.equal(orc.op_value_and_grad(x, gy, (6, 6, 6), 0.25, torch.float32)["out"], 0.25 * x)


def test_an_input_index_lies_in_as_many_stencils_as_the_header_says():
    def most(Si, So):
        i0, i1, _ = orc.axis_cells(Si, So, torch.float32)
        return max(int(((i0 == q) | (i1 == q)).sum()) for q in range(Si))
    assert [most(*p) for p in ((16, 8), (16, 2), (24, 3), (80, 10), (96, 12), (7, 3), (33, 2))] == [1] * 7
    assert most(6, 6) == 2 and most(2, 9) == 9


def test_gather_window_of_the_header_never_misses_a_stencil():
    """the backward's window of output indices around q / r, [(q - 1) / r - 1, (q + 1) / r + 2] in fp32 with the inverse ratio
    rounded once (everything when r = 0), holds every output whose cell names input index q"""
    f = np.float32
    sizes = list(range(1, 25)) + [33, 48, 80, 96, 160, 1000]
    for Si in sizes:
        for So in sizes:
            i0, i1, _ = (t.numpy() for t in orc.axis_cells(Si, So, torch.float32))
            r = f(Si - 1) / f(So - 1) if So > 1 else f(0)
            if not r > 0:
                continue                                               # the kernel then walks every output index
            inv = f(1) / r
            q = np.arange(Si).astype(f)
            lo = np.clip((q - f(1)) * inv - f(1), 0, 2e9).astype(np.int64)
            hi = np.minimum(np.clip((q + f(1)) * inv + f(2), 0, 2e9).astype(np.int64), So - 1)
            for idx in (i0, i1):                                       # output p names input idx[p]: p must lie in that input's window
                p = np.arange(So)
                assert bool(((lo[idx] <= p) & (p <= hi[idx])).all()), (Si, So)


@functools.lru_cache(maxsize=None)
def e2e_oracle(run, B):
    g = gold("e2e_rdn_32x48x32.npz")
    _, stages, levels, diff, share = orc.RUNS[run]
    p = orc.make_weights(stages, share, channels=int(gold(GOLDEN)["channels"]))
    return orc.value_and_grads(p, T(g["moving"][:B]), T(g["fixed"][:B]), torch.float64, stages, levels, diff, share)


@pytest.mark.parametrize("run,B", [(r, b) for r in orc.RUNS for b in (1, 2)])
def test_staged_oracle_equals_the_reference_golden(run, B):
    g, rec, tag = gold(GOLDEN), recorded(), "%s.B%d" % (run, B)
    stride, stages = int(g["stride"]), orc.RUNS[run][1]
    loss, sim, reg, y, flow, fields, grads = e2e_oracle(run, B)
    within_recorded("e2e[%s] flow_out" % tag, flow.reshape(-1)[::stride], T(g[tag + ".flow_out"]), rec)
    within_recorded("e2e[%s] y_moved" % tag, y.reshape(-1)[::stride], T(g[tag + ".y_moved"]), rec)
    assert len(fields) == stages
    for i, f in enumerate(fields):
        within_recorded("e2e[%s] stage%d" % (tag, i), f.reshape(-1)[::stride], T(g["%s.stage%d" % (tag, i)]), rec)
    within_recorded("e2e[%s] loss" % tag, loss, T(g[tag + ".loss"])[0], rec)
    kept = sorted(n for n in grads if "%s.grad.%s" % (tag, n) in g.files)
    assert len(kept) >= 20 + 4 * (1 if orc.RUNS[run][4] else stages)
    for n in kept:
        within_recorded("e2e[%s] grad %s" % (tag, n), grads[n], T(g["%s.grad.%s" % (tag, n)]), rec)
    # every later stage carries signal: its field is of the order of a voxel, and no gradient is analytically zero
    assert 0.3 < float(g[tag + ".flow_out_absmax"]) < 8.0
    assert all(0.1 < float(g["%s.stage%d_absmax" % (tag, i)]) < 4.0 for i in range(stages))
    assert all(float(v.abs().max()) > 1e-6 for v in grads.values())


def test_one_stage_of_the_staged_oracle_is_the_one_stage_oracle():
    g = gold("e2e_rdn_32x48x32.npz")
    mov, fix = T(g["moving"][:1]).double(), T(g["fixed"][:1]).double()
    p = orc.make_weights(1, False, channels=4)
    assert sorted(p) == sorted(rdn_oracle.make_weights(channels=4))
    a = orc.staged_forward(p, mov, fix, 1, (2, 1, 1, 2))
    b = rdn_oracle.rdn_forward(p, mov, fix, (2, 1, 1, 2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][0], b[2])


# ------------------------------------------------------------------------------------------------ the modules
def test_state_dict_keys_and_shapes_equal_the_reference():
    from smilecode_amd import models
    want = json.load(open(os.path.join(GOLD, "rdn_stages_state_dict.json")))
    assert sorted(want) == sorted(CLASSES)
    for cls, kw in CLASSES.items():
        legacy = {k: list(v.shape) for k, v in models.RDNStages(SHAPE, channels=4, legacy_grid_buffers=True, **kw).state_dict().items()}
        assert legacy == want[cls], cls
        m = models.RDNStages(SHAPE, channels=4, **kw)
        plain = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert plain == {k: v for k, v in want[cls].items() if not k.endswith(".grid")}
        shared = bool(kw.get("share"))
        assert ("est3.conv.4.weight" in plain) == shared and ("est3.%d.conv.4.weight" % (kw["stage_recursion"] - 1) in plain) != shared
        # a strict round trip through a reference-format dict
        ref_format = {k: torch.randn(v) for k, v in want[cls].items()}
        res = m.load_state_dict(ref_format, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        est2 = m.est2 if shared else m.est2[kw["stage_recursion"] - 1]
        key = "est2.conv.4.bias" if shared else "est2.%d.conv.4.bias" % (kw["stage_recursion"] - 1)
        assert torch.equal(est2.conv[4].bias.detach(), ref_format[key])
        back = m.state_dict()
        assert all(torch.equal(back[k], ref_format[k]) for k in back)
    m = models.RDN_share(SHAPE, channels=4, stage_recursion=3, diff=True)
    assert isinstance(m, models.RDNStages) and m.share and m.stages == 3
    assert sorted(m.state_dict()) == sorted(models.RDNStages(SHAPE, channels=4, stage_recursion=2, share=True, diff=True).state_dict())
    assert m.reg_on_subflows is True and m.stage_buckets is False and hasattr(m, "forward_cl")
    one = models.RDNStages(SHAPE, channels=4)
    assert sorted(one.state_dict()) == sorted(models.RDN(SHAPE, channels=4).state_dict())


def test_every_refusal_names_its_argument():
    from smilecode_amd import engine, models
    with pytest.raises(RuntimeError, match="stage_recursion = 2.*ResizeTransform") as e:
        models.RDN((32, 32, 32), channels=4, stage_recursion=2)              # models.RDN keeps refusing, and says where to go
    assert "RDNStages" in str(e.value)
    for cls in (models.RDNStages, models.RDN_share):
        for shape, match in (((32, 40, 32), "multiple of 16"), ((16, 32, 32), "at least 32"), ((32, 32), "expected")):
            with pytest.raises(RuntimeError, match=cls.__name__ + ": inshape.*" + match):
                cls(shape, channels=4)
        for bad in (0, -1, 2.0, True, "2"):
            with pytest.raises(RuntimeError, match="stage_recursion"):
                cls((32, 32, 32), channels=4, stage_recursion=bad)
        with pytest.raises(RuntimeError, match="act_dtype"):
            cls((32, 32, 32), channels=4, act_dtype=torch.bfloat16)
        for kw, match in ((dict(channels=3), "channels = 3"), (dict(channels=32), "channels = 32"), (dict(channels=4, in_channel=2), "in_channel = 2"),
                          (dict(channels=4, level_recursion=[1, 1, 1]), "level_recursion"), (dict(channels=4, diff=True, int_steps=13), "nsteps")):
            with pytest.raises(RuntimeError, match=match):
                cls((32, 32, 32), stage_recursion=2, **kw)
    m = models.RDNStages((32, 32, 32), channels=4, stage_recursion=2, return_stage_flows=True)
    v = torch.zeros(1, 1, 32, 32, 40)
    with pytest.raises(RuntimeError, match="RDNStages.forward: .*multiple of 16"):
        m(v, v)
    with pytest.raises(RuntimeError, match="same shape"):
        m(v, torch.zeros(1, 1, 32, 32, 32))
    with pytest.raises(RuntimeError, match="ModeT's three bucket"):
        engine.Trainer(m, overlap_allreduce=True)
    # ResizeTransform
    for kw, match in ((dict(factor=0.5, ndims=2), "ndims = 2"), (dict(factor=0), "factor = 0"), (dict(factor=-2), "factor = -2"),
                      (dict(factor=float("nan")), "factor"), (dict(factor="2"), "factor")):
        with pytest.raises(RuntimeError, match="ResizeTransform: " + match):
            models.ResizeTransform(**kw)
    with pytest.raises(RuntimeError, match="leaves a size of 0"):
        models.ResizeTransform(0.125)(torch.zeros(1, 3, 8, 7, 8))
    x = torch.zeros(1, 3, 4, 4, 4)
    assert models.ResizeTransform(1)(x) is x and models.ResizeTransform(1.0, 3).forward_cl(x) is x
    assert models.ResizeTransform(0.5)._size((9, 11, 33)) == (4, 5, 16) and models.ResizeTransform(2)._size((3, 4, 5)) == (6, 8, 10)


# ------------------------------------------------------------------------------------------------ train.py / infer.py
def test_stages_and_share_of_the_scripts(capsys):
    from smilecode_amd import infer, train
    ap, ip = train.make_parser(), infer.make_parser()
    a = ap.parse_args(["--model", "rdn"])
    assert a.stages == 1 and a.share is False and type(train.make_model(a, (32, 32, 32), training=True)).__name__ == "RDN"
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 1]) == "RDN(1, 1111)_ncc_1_diffusion_1_lr_0.0001/"
    a = train.check_model_args(ap, ap.parse_args(["--model", "rdn", "--stages", "4", "--levels", "4,4,4,4", "--channels", "4"]))
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 1]) == "RDN(4, 4444)_ncc_1_diffusion_1_lr_0.0001/"               # RDN/train.py:51
    m = train.make_model(a, (32, 32, 32), training=True)
    assert type(m).__name__ == "RDNStages" and m.stages == 4 and m.levels == [4, 4, 4, 4] and m.return_stage_flows and not m.share
    assert not train.make_model(a, (32, 32, 32)).return_stage_flows
    a = ap.parse_args(["--model", "rdn", "--stages", "2", "--share", "--diff", "--channels", "4"])
    assert train.save_dir_name(a, [8, 4, 2, 1, 1], 6, [1, 1]) == "RDN_share(2, 1111)_ncc_1_diffusion_1_lr_0.0001_diff7/"
    m = train.make_model(a, (32, 32, 32))
    assert type(m).__name__ == "RDNStages" and m.share and m.diff and m.stages == 2
    a = ap.parse_args(["--model", "rdn", "--share", "--channels", "4"])                  # one stage, shared keys: still the staged class
    assert type(train.make_model(a, (32, 32, 32))).__name__ == "RDNStages"
    b = ip.parse_args(["--model", "rdn", "--stages", "2", "--share", "--channels", "4"])
    assert train.check_model_args(ip, b) is b and train.make_model(b, (32, 32, 32)).share
    for parser, argv in ((ap, ["--stages", "2"]), (ap, ["--model", "rcn", "--share"]), (ip, ["--model", "pcnet", "--stages", "3"]),
                         (ip, ["--model", "im2grid", "--share"]), (ap, ["--model", "rdn", "--stages", "0"]),
                         (ap, ["--model", "rdn", "--stages", "2", "--overlap-allreduce"])):
        with pytest.raises(SystemExit) as e:
            train.check_model_args(parser, parser.parse_args(argv))
        assert e.value.code == 2
    assert "--stages" in capsys.readouterr().err
