"""No GPU: the restatement of tests/vecint_oracle.py against the reference's recorded fp64 results, the kink margin of every
parity case, the sixth header / table / export agreement, host-side answers of modet_vecint_ws_bytes, the argument checks of
ops.vecint in front of the library, and the public signatures (VecInt, ModeT(diff=...), the train and infer parsers)."""
import inspect

import numpy as np
import pytest
import torch

from tests.guard_family import check_family_table, check_header_is_c99
from tests import guard
from tests import vecint_oracle as vo
from tests.util import gold


@pytest.mark.parametrize("tag", [t for t, c in vo.CASES.items() if c[6]])
def test_restatement_equals_the_reference_in_fp64(tag):
    g = gold("op_vecint.npz")
    out, grad = vo.value_and_grad(vo.case_field(tag), vo.CASES[tag][4], torch.float64)
    for got, q in ((out, "out"), (grad, "grad")):
        ref = torch.from_numpy(np.ascontiguousarray(g["%s.%s" % (tag, q)]))
        assert ref.dtype == torch.float64 and ref.shape == got.shape
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (tag, q)


def test_goldens_hold_exactly_the_golden_cases():
    g = gold("op_vecint.npz")
    assert sorted(g.files) == sorted("%s.%s" % (t, q) for t, c in vo.CASES.items() if c[6] for q in ("out", "grad"))
    assert len(vo.CASES) == 7 and sum(c[6] for c in vo.CASES.values()) == 5


@pytest.mark.parametrize("tag", sorted(vo.CASES))
def test_fields_keep_clear_of_the_kinks(tag):
    """margin >= 4 x e_coord: no fp32 evaluation of a sample coordinate lands on the other side of an integer"""
    kind, B, shape, amp, nsteps, seed, _ = vo.CASES[tag]
    w = vo.case_field(tag)
    assert w.shape == (B, 3) + shape and w.dtype == torch.float64
    if kind == "tanh":
        assert float(w.abs().max()) <= amp
    margin, e_coord = vo.margin_and_coord_error(w, nsteps)
    print(f"{tag}: margin {margin:.3e}, e_coord {e_coord:.3e}")
    assert e_coord > 0.0 and margin >= 4.0 * e_coord, (tag, margin, e_coord)


def test_case_bounds_split_the_steps_as_the_tests_say():
    """bounded with bound 1: every step gathered; mixed with bound 8: steps 0-4 gathered, 5 and 6 scattered"""
    from smilecode_amd import ops
    assert ops._vecint_general_steps(7, 1.0) == 0 and ops._vecint_general_steps(7, 8.0) == 2
    assert ops._vecint_general_steps(7, 0.0) == 7 and ops._vecint_general_steps(0, 0.0) == 0
    assert ops._vecint_general_steps(3, 16.0) == 3 and ops._vecint_general_steps(7, 16.0) == 3


def test_vecint_header_table_and_exports_agree():
    """every name include/modet_hip_vecint.h declares has a signature in _lib.FAMILIES["vecint"] and is exported by the library,
    the table holds nothing else and shares no name with another family (tests/guard_family.py)"""
    check_family_table("vecint", {"modet_vecint_fwd", "modet_vecint_ws_bytes", "modet_vecint_bwd"}, ["modet_vecint_bwd", "modet_vecint_fwd"])
    from smilecode_amd import _lib, build, ops
    assert "MODET_VECINT_MAX_STEPS = %d" % ops.VECINT_MAX_STEPS in open(_lib.FAMILIES["vecint"][0]).read()
    assert "vecint.hip" in build.SOURCES


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("vecint", tmp_path, "return modet_vecint_ws_bytes(0, 0, 0, 0, MODET_VECINT_MAX_STEPS, 0.f) != 0;")


def test_workspace_size_answers_on_the_host():
    """0 where every step is bounded and for bad arguments; otherwise the scattered sum, v_0 where step 0 is general, and the
    scatter's own workspace"""
    from smilecode_amd import _lib
    L = _lib.load()
    q = L.modet_vecint_ws_bytes
    shape = (1, 16, 24, 16)
    field = 16 * 24 * 16 * 12
    assert q(*shape, 7, 1.0) == 0 and q(*shape, 7, 0.5) == 0 and q(*shape, 0, 0.0) == 0 and q(*shape, 1, 2.0) == 0
    tiles = L.modet_warp_bwd_dsrc_tiles_ws_bytes(*shape, 3)
    assert tiles > 0
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731
    assert q(*shape, 7, 0.0) == 2 * up(field) + up(tiles)             # step 0 general: v_0 is materialised
    assert q(*shape, 7, 8.0) == up(field) + up(tiles)                 # steps 5 and 6 general
    assert q(*shape, 7, 8.0) == q(*shape, 7, 128.0) == q(*shape, 1, 2.5) - up(field)
    big = (1, 8, 8, 1032)                                             # an axis beyond the tile path's 1024: the fixed-point scatter
    assert L.modet_warp_bwd_dsrc_tiles_ws_bytes(*big, 3) == 0
    assert q(*big, 2, 0.0) == 2 * up(8 * 8 * 1032 * 12) + up(L.modet_warp_bwd_det_ws_bytes(*big, 3))
    for bad in ((0, 4, 4, 4, 7, 0.0), (1, 0, 4, 4, 7, 0.0), (1, 4, 4, -1, 7, 0.0), (1, 4, 4, 4, -1, 0.0), (1, 4, 4, 4, 13, 0.0),
                (1, 4, 4, 4, 7, -1.0), (1, 4, 4, 4, 7, float("nan")), (1, 4, 4, 4, 7, float("inf")), (1, 1024, 1024, 1024, 7, 0.0),
                (1, 1024, 1024, 683, 7, 0.0)):
        assert q(*bad) == 0, bad
    assert q(1, 1024, 1024, 682, 7, 0.0) > 0                          # 3 * 2^20 * 682 < 2^31 <= 3 * 2^20 * 683


class _Fake:
    """a tensor that claims to live on the GPU (the checks in front of the library look at nothing else first)"""
    is_cuda = True

    def __init__(self, dtype, contiguous=True):
        self.dtype, self._c = dtype, contiguous

    def is_contiguous(self):
        return self._c


def test_ops_check_arguments_before_the_launch(monkeypatch):
    """every refusal of ops.vecint fires before the library is reached"""
    from smilecode_amd import _lib, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["vecint"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    with pytest.raises(RuntimeError, match="float32"):
        ops.vecint(_Fake(torch.float64))
    with pytest.raises(RuntimeError, match="float32"):
        ops.vecint(_Fake(torch.bfloat16))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.vecint(_Fake(torch.float32, contiguous=False))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vecint(torch.zeros(1, 4, 4, 4, 3))
    for n in (-1, 13, 2.0, "7", True, None):
        with pytest.raises(RuntimeError, match="nsteps"):
            ops.vecint(_Fake(torch.float64), n)          # (nsteps and bound are looked at before the tensor)
    for b in (-1.0, -1e-30, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="bound"):
            ops.vecint(_Fake(torch.float64), 7, b)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    for shape in ((4, 4, 4, 3), (1, 1, 4, 4, 4, 3)):
        with pytest.raises(RuntimeError, match=r"\(B,D,H,W,C\)"):
            ops.vecint(torch.zeros(shape))
    for shape in ((1, 3, 4, 4, 4), (1, 4, 4, 4, 2), (1, 4, 4, 4, 4)):
        with pytest.raises(RuntimeError, match=r"\(B,D,H,W,3\)"):
            ops.vecint(torch.zeros(shape))
    for shape in ((0, 4, 4, 4, 3), (1, 4, 0, 4, 3)):
        with pytest.raises(RuntimeError, match="non-empty"):
            ops.vecint(torch.zeros(shape))
    assert not [n for n, _ in px.records if guard.is_launching(n)]


def test_public_signatures_and_defaults():
    from smilecode_amd import models
    sig = inspect.signature(models.VecInt.__init__)
    assert list(sig.parameters) == ["self", "inshape", "nsteps", "legacy_grid_buffers"]
    assert sig.parameters["nsteps"].default == 7 and sig.parameters["legacy_grid_buffers"].default is False
    m = models.VecInt((8, 8, 8))
    assert m.nsteps == 7 and m.scale == 1.0 / 128 and not list(m.parameters()) and not m.state_dict()
    assert isinstance(m.transformer, models.SpatialTransformer) and hasattr(m, "forward_cl")
    sd = models.VecInt((4, 5, 6), 3, legacy_grid_buffers=True).state_dict()
    assert list(sd) == ["transformer.grid"] and sd["transformer.grid"].shape == (1, 3, 4, 5, 6)
    for bad in (-1, 13, 2.5):
        with pytest.raises(RuntimeError, match="nsteps"):
            models.VecInt((8, 8, 8), bad)
    for cls, scale in ((models.ModeT, None), (models.ModeT_cu, 1)):
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-2:] == ["diff", "int_steps"] and p["diff"].default is False and p["int_steps"].default == 7
        assert p["scale"].default == scale
        assert list(p)[:10] == ["self", "inshape", "in_channel", "channels", "head_dim", "num_heads", "scale", "legacy_grid_buffers",
                                "act_dtype", "fused_attention"]


def test_train_and_infer_parsers_and_the_directory_name():
    from smilecode_amd import infer, train
    heads, hd = [8, 4, 2, 1, 1], 6
    a = train.make_parser().parse_args([])
    assert a.diff is False and a.int_steps == 7
    old = "modet-heads(84211)-rpe_headim_6_ncc_1_reg_1_lr_0.0001_54r/"
    assert train.save_dir_name(a, heads, hd, [1, 1]) == old           # unchanged without --diff
    b = train.make_parser().parse_args(["--diff"])
    c = train.make_parser().parse_args(["--diff", "--int-steps", "5"])
    assert b.diff is True and b.int_steps == 7 and c.int_steps == 5
    names = {train.save_dir_name(x, heads, hd, [1, 1]) for x in (a, b, c)}
    assert len(names) == 3 and all(n.endswith("/") for n in names)
    d = train.make_parser().parse_args(["--int-steps", "5"])          # without --diff the step count names nothing
    assert train.save_dir_name(d, heads, hd, [1, 1]) == old
    i = infer.make_parser().parse_args([])
    assert i.diff is False and i.int_steps == 7
    i = infer.make_parser().parse_args(["--diff", "--int-steps", "4"])
    assert i.diff is True and i.int_steps == 4
