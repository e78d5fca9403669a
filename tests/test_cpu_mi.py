"""The mutual-information losses without a GPU: the torch restatement against the reference's recorded results, the header of
the family against its ctypes table and the library's exports, the workspace sizes, the refusals and the argument checks."""
import numpy as np
import pytest
import torch

from tests.guard_family import check_family_table
from tests import guard, mi_oracle
from tests.util import gold

CASES = ("pair16", "pair12x20x28", "noise2x10x12x14", "tiny3x5x7", "one1x1x1", "wide6x7x9")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def terms(g, tag):
    """(name, oracle function, keyword arguments) of every loss recorded for the case"""
    sr, lo, hi = (float(v) for v in g[tag + ".params"])
    kw = {"sigma_ratio": sr, "minval": lo, "maxval": hi}
    out = [("mi", mi_oracle.mi_loss, kw)]
    return out + [("lmi%d" % p, mi_oracle.lmi_loss, dict(kw, patch_size=int(p))) for p in g[tag + ".patches"]]


@pytest.mark.parametrize("tag", CASES)
def test_restatement_equals_the_reference_golden(tag):
    """tests/mi_oracle.py in fp64 against what the reference's two classes returned for the same images
    (tests/golden/make_goldens_mi.py): loss within 1e-13 relative, gradients within 1e-12 of their maximum"""
    g = gold("op_mi.npz")
    a, b = T(g[tag + ".a"]), T(g[tag + ".b"])
    seen = set()
    for name, fn, kw in terms(g, tag):
        k = "%s.%s" % (tag, name)
        loss, da, db = mi_oracle.value_and_grads(fn, a, b, torch.float64, **kw)
        want = float(g[k + ".loss"])
        assert abs(float(loss) - want) <= 1e-13 * abs(want), (k, float(loss), want)
        for got, ref in ((da, T(g[k + ".da"])), (db, T(g[k + ".db"]))):
            assert got.shape == ref.shape == a.shape
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), k
        seen.add(name)
    assert {"mi", "lmi5"} <= seen


def test_goldens_hold_the_cases_the_gpu_tests_rely_on():
    g = gold("op_mi.npz")
    patches = set()
    for tag in CASES:
        patches |= {int(p) for p in g[tag + ".patches"]}
    assert patches == {3, 4, 5, 7}
    a, b = g["noise2x10x12x14.a"], g["noise2x10x12x14.b"]
    assert (a < 0).any() and (a > 1).any() and (b < 0).any() and (b > 1).any(), "both clamp ends cut"
    assert g["tiny3x5x7.a"].size % 2 == 1 and g["one1x1x1.a"].size == 1
    assert tuple(g["wide6x7x9.params"]) == (0.5, 0.0, 2.0)
    # the clamp's gradient rule in the recorded gradients: zero outside [0, maxval], alive inside
    db = g["noise2x10x12x14.mi.db"]
    assert (db[(b < 0) | (b > 1)] == 0).all() and (db[(b >= 0) & (b <= 1)] != 0).all()


def test_mi_header_table_and_exports_agree():
    """every name include/modet_hip_mi.h declares has a signature in _lib.FAMILIES["mi"] and is exported by the library, the
    table holds nothing else and shares no name with another family (tests/guard_family.py)"""
    check_family_table("mi", {"modet_mi_ws_bytes", "modet_mi_fwd_bwd", "modet_lmi_fwd_bwd"}, ["modet_lmi_fwd_bwd", "modet_mi_fwd_bwd"])


def test_workspace_holds_nothing_per_voxel_and_bin():
    """at the workload's shape either form's workspace is smaller than ONE volume; bad arguments give 0"""
    from smilecode_amd import _lib
    lib = _lib.load()
    n = 160 * 192 * 160
    for patch in (0, 5):
        assert 0 < lib.modet_mi_ws_bytes(1, 160, 192, 160, patch) < 4 * n, patch
    assert lib.modet_mi_ws_bytes(1, 1, 1, 1, 0) > 0 and lib.modet_mi_ws_bytes(1, 1, 1, 1, 16) > 0
    assert lib.modet_mi_ws_bytes(2, 3, 5, 7, 3) == 2 * 1 * 2 * 3 * 4          # one float per patch
    for bad in ((0, 8, 8, 8, 0), (1, 0, 8, 8, 0), (1, 8, -1, 8, 5), (1, 8, 8, 0, 5), (1, 8, 8, 8, -1), (1, 8, 8, 8, 17),
                (1, 2048, 2048, 2048, 0)):
        assert lib.modet_mi_ws_bytes(*bad) == 0, bad


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL pointers, non-positive dims, unsupported parameters and a short workspace come back as error codes from the host
    checks (no device is touched: the pointers are never dereferenced on these paths); d_a and d_b may be NULL"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL value that is never dereferenced
    nan = float("nan")

    def mi(a=p, b=p, loss=p, ws=p, nb=None, dims=(1, 8, 8, 8), bins=32, lo=0.0, hi=1.0, sr=1.0, patch=None):
        size = lib.modet_mi_ws_bytes(1, 8, 8, 8, patch or 0) if nb is None else nb
        if patch is None:
            return lib.modet_mi_fwd_bwd(a, b, loss, None, None, ws, size, *dims, bins, lo, hi, sr, 1.0, None)
        return lib.modet_lmi_fwd_bwd(a, b, loss, None, None, ws, size, *dims, bins, lo, hi, sr, patch, 1.0, None)

    for patch in (None, 5):
        for k in ("a", "b", "loss", "ws"):
            assert mi(patch=patch, **{k: None}) == -1, (patch, k)
        for dims in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -2, 8), (1, 8, 8, 0)):
            assert mi(patch=patch, dims=dims) == -2, (patch, dims)
        for kw in ({"bins": 16}, {"bins": 64}, {"hi": 0.0}, {"hi": -1.0}, {"lo": 1.0}, {"lo": 2.0}, {"sr": 0.0}, {"sr": -1.0},
                   {"hi": nan}, {"sr": nan}):
            assert mi(patch=patch, **kw) == -3, (patch, kw)
        full = lib.modet_mi_ws_bytes(1, 8, 8, 8, patch or 0)
        assert mi(patch=patch, nb=full - 1) == -4 and mi(patch=patch, nb=0) == -4
    for patch in (0, -1, 17):
        assert mi(patch=patch, nb=1 << 20) == -3, patch
    # the global workspace begins with doubles, the local one holds floats: a misaligned pointer is refused like a short one
    assert mi(ws=p + 4) == -4 and mi(patch=5, ws=p + 2) == -4


def test_loss_classes_refuse_what_they_cannot_compute():
    from smilecode_amd import losses, ops
    for cls in (losses.MutualInformation, losses.localMutualInformation):
        m = cls()
        assert (m.sigma_ratio, m.minval, m.maxval, m.num_bins) == (1, 0.0, 1.0, 32)
        for kw in ({"num_bin": 16}, {"maxval": 0.0}, {"minval": 1.0, "maxval": 1.0}, {"sigma_ratio": 0}, {"sigma_ratio": -1.0}):
            with pytest.raises(RuntimeError, match=cls.__name__):
                cls(**kw)
        v = torch.zeros(1, 1, 4, 5, 6)
        for bad in (torch.zeros(4, 5, 6), torch.zeros(1, 4, 5, 6), torch.zeros(1, 2, 4, 5, 6), torch.zeros(1, 1, 0, 5, 6)):
            with pytest.raises(RuntimeError, match=cls.__name__):
                m(bad, bad)
            with pytest.raises(RuntimeError, match=cls.__name__):
                m(v, bad)
        with pytest.raises(RuntimeError, match="differ in shape"):
            m(v, torch.zeros(1, 1, 4, 5, 7))
        with pytest.raises(RuntimeError, match="GPU"):              # no CPU fallback: a host tensor is an error, not a slow path
            m(v, v)
    assert losses.localMutualInformation().patch_size == 5 and losses.localMutualInformation(patch_size=7).patch_size == 7
    for bad in (0, 17, -5, 2.5):
        with pytest.raises(RuntimeError, match="patch_size"):
            losses.localMutualInformation(patch_size=bad)
    v = torch.zeros(1, 1, 4, 5, 6)
    for fn in (ops.mi_loss, ops.lmi_loss, ops.mi_value_and_grad, ops.lmi_value_and_grad):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(v, v)


def test_ops_check_parameters_before_the_launch(monkeypatch):
    """with tensors that claim to be on the GPU the parameter checks still fire first: the library is never reached"""
    from smilecode_amd import _lib, ops
    monkeypatch.setattr(_lib, "_lib", guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["mi"][1], segments=lambda: [], refuse=True))
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    v = torch.zeros(1, 1, 4, 5, 6)
    for fn in (ops.mi_loss, ops.lmi_loss, ops.mi_value_and_grad, ops.lmi_value_and_grad):
        for kw in ({"num_bin": 16}, {"maxval": 0.0}, {"minval": 2.0}, {"sigma_ratio": 0.0}):
            with pytest.raises(RuntimeError, match="num_bin|maxval"):
                fn(v, v, **kw)
        with pytest.raises(RuntimeError, match="does not match"):
            fn(v, torch.zeros(1, 1, 4, 5, 7))
        with pytest.raises(RuntimeError, match=r"\(B,1,D,H,W\)"):
            fn(torch.zeros(1, 2, 4, 5, 6), torch.zeros(1, 2, 4, 5, 6))
    for fn in (ops.lmi_loss, ops.lmi_value_and_grad):
        for bad in (0, 17, 2.5):
            with pytest.raises(RuntimeError, match="patch_size"):
                fn(v, v, patch_size=bad)


def test_trainer_seeds_the_backward_for_the_two_terms():
    """both classes are terms whose kernels hand out value and gradient, so the step seeds its backward with them; exact types
    only: a subclass keeps the autograd expression"""
    from smilecode_amd import engine, losses

    class WithCl(torch.nn.Linear):
        def forward_cl(self, a, b):
            raise AssertionError("not called here")

    for cls in (losses.MutualInformation, losses.localMutualInformation):
        tr = engine.Trainer(WithCl(3, 2), sim=cls())
        assert type(tr.sim) is cls and tr._seedable()
        tr.seed_backward = False
        assert not tr._seedable()

        class Sub(cls):
            pass
        assert not engine.Trainer(WithCl(3, 2), sim=Sub())._seedable()
        assert not engine.Trainer(torch.nn.Linear(3, 2), sim=cls())._seedable()
