"""The flow regularisers (Grad3DiTV, DisplacementRegularizer) without a GPU: the torch restatement against the reference's recorded
results, the header of the family against its ctypes table and the library's exports, the workspace size, the refusals, the
argument checks, the trainer's ``reg`` argument and train.py's flags."""
import os

import numpy as np
import pytest
import torch

from tests.guard_family import check_family_table, check_header_is_c99
from tests import guard, reg_oracle
from tests.util import gold

ALL = ("itv", "gradient-l2", "gradient-l1", "bending")
CASES = {"noise2x3x5x5x5": ((2, 3, 5, 5, 5), ALL), "noise1x3x6x7x9": ((1, 3, 6, 7, 9), ALL), "noise1x3x9x9x9": ((1, 3, 9, 9, 9), ALL),
         "smooth1x3x8x10x37": ((1, 3, 8, 10, 37), ALL), "slab1x3x7x8x9": ((1, 3, 7, 8, 9), ALL), "zero1x3x6x6x6": ((1, 3, 6, 6, 6), ALL),
         "itv2x2x2x3x4": ((2, 2, 2, 3, 4), ("itv",)), "itv1x1x4x5x6": ((1, 1, 4, 5, 6), ("itv",))}
KIND_ID = {"itv": 0, "gradient-l2": 1, "gradient-l1": 2, "bending": 3}
MIN = {"itv": 2, "gradient-l2": 3, "gradient-l1": 3, "bending": 5}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_equals_the_reference_golden(tag):
    """tests/reg_oracle.py in fp64 against what the reference's classes returned for the same flow
    (tests/golden/make_goldens_reg.py): loss within 1e-13 absolute, gradient within 1e-13 of its maximum
    (tests/golden/REPORT_reg.txt has the measured differences, at most 3e-17)"""
    g = gold("op_reg.npz")
    f = T(g[tag + ".f"])
    for kind in g[tag + ".kinds"]:
        k = "%s.%s" % (tag, kind)
        loss, grad = reg_oracle.value_and_grad(reg_oracle.KINDS[str(kind)], f, torch.float64)
        want, ref = float(g[k + ".loss"]), T(g[k + ".grad"])
        assert abs(float(loss) - want) <= 1e-13, (k, float(loss), want)
        assert grad.shape == ref.shape == f.shape
        assert float((grad - ref).abs().max()) <= 1e-13 * float(ref.abs().max()), k


def test_goldens_hold_the_cases_the_gpu_tests_rely_on():
    g = gold("op_reg.npz")
    for tag, (shape, kinds) in CASES.items():
        assert g[tag + ".f"].shape == shape and g[tag + ".f"].dtype == np.float32, tag
        assert tuple(str(k) for k in g[tag + ".kinds"]) == kinds, tag
        for kind in kinds:
            assert g["%s.%s.loss" % (tag, kind)].dtype == np.float64 and g["%s.%s.grad" % (tag, kind)].dtype == np.float64
            assert g["%s.%s.grad" % (tag, kind)].shape == shape
    # bending's minimum holds one stencil point per channel; 9^3 is the first shape with a voxel at least 4 from every face
    assert min(CASES["noise2x3x5x5x5"][0][2:]) == 5 and all(n - 8 == 1 for n in CASES["noise1x3x9x9x9"][0][2:])
    # the slab's constant block: central differences of exactly 0 (the l1 kink) and iTV norms of exactly sqrt(1e-6)
    s = g["slab1x3x7x8x9.f"].astype(np.float64)
    gz = (s[:, :, 2:, 1:-1, 1:-1] - s[:, :, :-2, 1:-1, 1:-1]) / 2
    assert int((gz == 0).sum()) >= 3 * 2 * 2 * 2
    p = s[:, :, 1:, 1:, 1:]
    n2 = (p - s[:, :, :-1, 1:, 1:]) ** 2 + (p - s[:, :, 1:, :-1, 1:]) ** 2 + (p - s[:, :, 1:, 1:, :-1]) ** 2
    assert int((n2 == 0).sum()) == 3 * 3 * 3 * 3
    assert not g["zero1x3x6x6x6.f"].any() and float(g["zero1x3x6x6x6.itv.loss"]) == pytest.approx(1e-3 / 3, rel=1e-12)
    assert not g["zero1x3x6x6x6.itv.grad"].any() and float(g["zero1x3x6x6x6.bending.loss"]) == 0.0
    sm = g["smooth1x3x8x10x37.f"]
    assert 1.5 < float(np.abs(sm).max()) < 4.0 and sm.shape[-1] > 32
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "op_reg.npz")) < (1 << 20)


def test_reg_header_table_and_exports_agree():
    """every name include/modet_hip_reg.h declares has a signature in _lib.FAMILIES["reg"] and is exported by the library, the
    table holds nothing else and shares no name with another family (tests/guard_family.py)"""
    check_family_table("reg", {"modet_reg_ws_bytes", "modet_reg_fwd_bwd"}, ["modet_reg_fwd_bwd"])
    from smilecode_amd import _lib
    txt = open(_lib.FAMILIES["reg"][0]).read()
    for name, value in KIND_ID.items():
        assert "MODET_REG_%s = %d" % (name.upper().replace("-", "_"), value) in txt
    from smilecode_amd import ops
    assert ops.REG_KINDS == KIND_ID and ops.REG_MIN_SIZE == MIN == reg_oracle.MIN_SIZE


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("reg", tmp_path, "return modet_reg_ws_bytes(MODET_REG_BENDING, 0, 0, 0, 0, 0) != 0;")


def test_workspace_holds_partials_only_and_is_a_function_of_kind_and_shape():
    """the header's bound: one double per workgroup, at most 2048 of them -- far below the flow's own 12 B per voxel + 1 MiB"""
    from smilecode_amd import _lib
    lib = _lib.load()
    for kind in range(4):
        full = lib.modet_reg_ws_bytes(kind, 1, 3, 160, 192, 160)
        assert 0 < full <= 2048 * 8 < 12 * 160 * 192 * 160 + (1 << 20), kind
        assert full == lib.modet_reg_ws_bytes(kind, 1, 3, 160, 192, 160)
        m = list(MIN.values())[kind]
        assert 8 <= lib.modet_reg_ws_bytes(kind, 1, 3, m, m, m) <= 2048 * 8, kind
        assert 0 < lib.modet_reg_ws_bytes(kind, 2, 3, 7, 9, 37) <= 2048 * 8, kind
        for bad in ((1, 3, m - 1, 9, 9), (1, 3, 9, m - 1, 9), (1, 3, 9, 9, m - 1), (0, 3, 9, 9, 9), (1, 0, 9, 9, 9), (-1, 3, 9, 9, 9),
                    (1, 3, 2048, 2048, 2048)):
            assert lib.modet_reg_ws_bytes(kind, *bad) == 0, (kind, bad)
        for C in (1, 2, 4):                                    # the displacement kinds take 3 channels, iTV any
            assert (lib.modet_reg_ws_bytes(kind, 1, C, 9, 9, 9) > 0) == (kind == 0), (kind, C)
    for kind in (-1, 4, 17):
        assert lib.modet_reg_ws_bytes(kind, 1, 3, 9, 9, 9) == 0, kind


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """NULL pointers, sizes below a kind's minimum, wrong channel counts, unknown kinds and a short or misaligned workspace come
    back as error codes from the host checks (no device is touched: the pointers are never dereferenced on these paths); d_f may
    be NULL.  The layout is not an argument of modet_reg_ws_bytes, so channels-last with C != 3 is refused here."""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL value that is never dereferenced

    def reg(f=p, loss=p, ws=p, nb=1 << 20, kind=3, dims=(1, 3, 9, 9, 9), cl=0):
        return lib.modet_reg_fwd_bwd(f, loss, None, ws, nb, kind, *dims, cl, 1.0, None)

    for k in ("f", "loss", "ws"):
        assert reg(**{k: None}) == -1, k
    for kind in range(4):
        m = list(MIN.values())[kind]
        for dims in ((0, 3, 9, 9, 9), (1, 3, m - 1, 9, 9), (1, 3, 9, m - 1, 9), (1, 3, 9, 9, m - 1), (1, 3, 9, -2, 9), (1, 0, 9, 9, 9),
                     (1, 3, 2048, 2048, 2048)):
            assert reg(kind=kind, dims=dims) == -2, (kind, dims)
        for C in (1, 2, 4):
            assert reg(kind=kind, dims=(1, C, 9, 9, 9), cl=1) == -2, (kind, C)
            if kind:
                assert reg(kind=kind, dims=(1, C, 9, 9, 9)) == -2, (kind, C)
        full = lib.modet_reg_ws_bytes(kind, 1, 3, 9, 9, 9)
        assert reg(kind=kind, nb=full - 1) == -4 and reg(kind=kind, nb=0) == -4
        assert reg(kind=kind, ws=p + 4) == -4 and reg(kind=kind, ws=p + 2) == -4      # the workspace begins with doubles
    for kind in (-1, 4, 99):
        assert reg(kind=kind) == -3, kind


def test_loss_classes_refuse_what_they_cannot_compute():
    from smilecode_amd import losses, ops
    assert losses.DisplacementRegularizer("bending").energy_type == "bending"
    for bad in ("bend", "gradient", "l2", None, 3, "itv"):
        with pytest.raises(RuntimeError, match="energy_type"):
            losses.DisplacementRegularizer(bad)
    itv = losses.Grad3DiTV()
    terms = [("Grad3DiTV", itv, "itv")] + [("DisplacementRegularizer", losses.DisplacementRegularizer(k), k) for k in ALL[1:]]
    for name, m, kind in terms:
        for bad in (torch.zeros(3, 9, 9, 9), torch.zeros(9, 9, 9), torch.zeros(1, 1, 3, 9, 9, 9)):                # rank
            with pytest.raises(RuntimeError, match=name):
                m(bad, None)
        n = MIN[kind]
        for shape in ((1, 3, n - 1, 9, 9), (1, 3, 9, n - 1, 9), (1, 3, 9, 9, n - 1), (0, 3, 9, 9, 9)):           # too-small axes
            with pytest.raises(RuntimeError, match=name):
                m(torch.zeros(shape), None)
        if kind != "itv":
            for C in (1, 2, 4):                                                                                   # channels
                with pytest.raises(RuntimeError, match=r"\(B,3,D,H,W\)"):
                    m(torch.zeros(1, C, 9, 9, 9), None)
        with pytest.raises(RuntimeError, match="GPU"):          # no CPU fallback: a host tensor is an error, not a slow path
            m(torch.zeros(1, 3, 9, 9, 9), None)
        with pytest.raises(RuntimeError, match="GPU"):
            ops.reg_loss(torch.zeros(1, 3, 9, 9, 9), kind)
        with pytest.raises(RuntimeError, match="GPU"):
            ops.reg_value_and_grad_cl(torch.zeros(1, 9, 9, 9, 3), kind)
    with pytest.raises(RuntimeError, match="GPU"):
        itv(torch.zeros(1, 2, 2, 2, 2))                         # (two channels at the minimum sizes pass the class's own checks)


class _Fake:
    """what ops._chk looks at, for the dtype refusal on a machine without a GPU"""
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype

    def is_contiguous(self):
        return True


def test_ops_check_arguments_before_the_launch(monkeypatch):
    """with tensors that claim to be on the GPU the argument checks still fire first: the library is never reached"""
    from smilecode_amd import _lib, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["reg"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    with pytest.raises(RuntimeError, match="float32"):         # (the dtype is looked at before the shape is)
        ops._reg_args("reg_loss", _Fake(torch.float64), "bending", False)
    with pytest.raises(RuntimeError, match="unknown kind"):     # (and the kind before the tensor)
        ops._reg_args("reg_loss", _Fake(torch.float64), "bend", False)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    for kind in ALL:
        n = MIN[kind]
        for fn, mk in ((ops.reg_loss, lambda B, C, D, H, W: torch.zeros(B, C, D, H, W)),
                       (ops.reg_value_and_grad_cl, lambda B, C, D, H, W: torch.zeros(B, D, H, W, C))):
            for shape in ((1, 3, n - 1, 9, 9), (1, 3, 9, n - 1, 9), (1, 3, 9, 9, n - 1), (0, 3, 9, 9, 9)):
                with pytest.raises(RuntimeError, match="needs a non-empty flow"):
                    fn(mk(*shape), kind)
            with pytest.raises(RuntimeError, match="expects a"):
                fn(torch.zeros(3, 9, 9, 9), kind)
            with pytest.raises(RuntimeError, match="unknown kind"):
                fn(mk(1, 3, 9, 9, 9), "grad3d")
        for C in (1, 2, 4):
            with pytest.raises(RuntimeError, match=r"channels-last \(B,D,H,W,3\)"):      # also: a planar flow handed to the _cl form
                ops.reg_value_and_grad_cl(torch.zeros(1, 9, 9, 9, C), kind)
            if kind != "itv":
                with pytest.raises(RuntimeError, match="3 channels"):
                    ops.reg_loss(torch.zeros(1, C, 9, 9, 9), kind)
        with pytest.raises(RuntimeError, match=r"channels-last \(B,D,H,W,3\)"):
            ops.reg_value_and_grad_cl(torch.zeros(1, 3, 9, 9, 9), kind)
    assert not [n for n, _ in px.records if guard.is_launching(n)]


def test_trainer_takes_a_regulariser_and_seeds_the_backward_for_the_exact_types():
    """``Trainer(model)`` keeps Grad3d('l2'); the new terms hand out value and gradient, so the step seeds its backward with them;
    exact types only: a subclass keeps the autograd expression"""
    from smilecode_amd import engine, losses

    class WithCl(torch.nn.Linear):
        def forward_cl(self, a, b):
            raise AssertionError("not called here")

    tr = engine.Trainer(WithCl(3, 2))
    assert type(tr.reg) is losses.Grad3d and tr.reg.penalty == "l2" and tr.reg.loss_mult is None and tr._seedable()
    assert not engine.Trainer(WithCl(3, 2), reg=losses.Grad3d("l2", loss_mult=2.0))._seedable()
    for reg in (losses.Grad3DiTV(), losses.DisplacementRegularizer("bending"), losses.DisplacementRegularizer("gradient-l2"),
                losses.DisplacementRegularizer("gradient-l1")):
        tr = engine.Trainer(WithCl(3, 2), reg=reg, sim=losses.MutualInformation())
        assert tr.reg is reg and tr._seedable()
        tr.seed_backward = False
        assert not tr._seedable()
        assert not engine.Trainer(torch.nn.Linear(3, 2), reg=reg)._seedable()

    class SubI(losses.Grad3DiTV):
        pass

    class SubD(losses.DisplacementRegularizer):
        pass
    assert not engine.Trainer(WithCl(3, 2), reg=SubI())._seedable()
    assert not engine.Trainer(WithCl(3, 2), reg=SubD("bending"))._seedable()


def test_train_flags_and_directory_name():
    from smilecode_amd import train
    heads, hd = [8, 4, 2, 1, 1], 6
    a = train.make_parser().parse_args([])
    assert a.reg == "grad3d" and a.reg_weight == 1
    old = "modet-heads({}{}{}{}{})-rpe_headim_{}_{}_{}_reg_{}_lr_{}_54r/".format(*heads, hd, "ncc", 1, 1, 0.0001)
    assert train.save_dir_name(a, heads, hd, [1, 1]) == old
    names = {old}
    for kind in ("grad3d", "itv", "gradient-l2", "gradient-l1", "bending"):
        a = train.make_parser().parse_args(["--sim", "mi", "--reg", kind, "--reg-weight", "0.5"])
        assert a.reg == kind and a.reg_weight == 0.5
        name = train.save_dir_name(a, heads, hd, [1, a.reg_weight])
        assert kind in name and "0.5" in name and "_mi_" in name
        names.add(name)
    a = train.make_parser().parse_args(["--reg", "bending"])
    names.add(train.save_dir_name(a, heads, hd, [1, 1]))
    assert len(names) == 7
    with pytest.raises(SystemExit):
        train.make_parser().parse_args(["--reg", "tv"])
