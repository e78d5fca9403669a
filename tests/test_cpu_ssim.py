"""The SSIM3D loss without a GPU: the torch restatement against the reference's recorded results, the header of the family
against its ctypes table and the library's exports, the workspace size, the refusals and the argument checks."""

import numpy as np
import pytest
import torch

from tests.guard_family import check_family_table, check_header_is_c99
from tests import guard, ssim_oracle
from tests.util import gold

CASES = {"pair16": (11,), "noise2x6x10x14": (11, 3, 5, 7), "tiny3x5x7": (11, 3, 5, 7), "one1x1x1": (11, 3), "wide6x7x9": (11, 5)}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_equals_the_reference_golden(tag):
    """tests/ssim_oracle.py in fp64 against what the reference's class returned for the same images
    (tests/golden/make_goldens_ssim.py): both sides are the same fp64 operations; loss within 1e-13 absolute, gradients within
    1e-13 of their maximum (tests/golden/REPORT_ssim.txt has the measured differences, at most 7e-18)"""
    g = gold("op_ssim.npz")
    a, b = T(g[tag + ".a"]), T(g[tag + ".b"])
    for w in g[tag + ".windows"]:
        k = "%s.w%d" % (tag, int(w))
        loss, da, db = ssim_oracle.value_and_grads(ssim_oracle.ssim_loss, a, b, torch.float64, window_size=int(w))
        want = float(g[k + ".loss"])
        assert abs(float(loss) - want) <= 1e-13, (k, float(loss), want)
        for got, ref in ((da, T(g[k + ".da"])), (db, T(g[k + ".db"]))):
            assert got.shape == ref.shape == a.shape
            assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max()), k


def test_goldens_hold_the_cases_the_gpu_tests_rely_on():
    g = gold("op_ssim.npz")
    for tag, windows in CASES.items():
        assert tuple(int(w) for w in g[tag + ".windows"]) == windows, tag
        for w in windows:
            for q in ("loss", "da", "db"):
                assert g["%s.w%d.%s" % (tag, w, q)].dtype == np.float64
    assert g["pair16.a"].shape == (1, 1, 16, 16, 16) and g["noise2x6x10x14.a"].shape == (2, 1, 6, 10, 14)
    assert g["tiny3x5x7.a"].shape == (1, 1, 3, 5, 7) and g["one1x1x1.a"].size == 1 and g["wide6x7x9.a"].shape == (1, 1, 6, 7, 9)
    a = g["noise2x6x10x14.a"]
    assert (a < 0).any() and (a > 1).any() and g["wide6x7x9.b"].max() > 2.0


def test_ssim_header_table_and_exports_agree():
    """every name include/modet_hip_ssim.h declares has a signature in _lib.FAMILIES["ssim"] and is exported by the library,
    the table holds nothing else and shares no name with another family (tests/guard_family.py)"""
    check_family_table("ssim", {"modet_ssim_ws_bytes", "modet_ssim_fwd_bwd"}, ["modet_ssim_fwd_bwd"])


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("ssim", tmp_path, "return modet_ssim_ws_bytes(0, 0, 0, 0, 0) != 0;")


def test_workspace_is_at_most_five_volumes_and_a_function_of_shape_and_window():
    from smilecode_amd import _lib
    lib = _lib.load()
    n = 160 * 192 * 160
    full = lib.modet_ssim_ws_bytes(1, 160, 192, 160, 11)
    assert 0 < full <= 5 * 4 * n + (1 << 20)
    assert full == lib.modet_ssim_ws_bytes(1, 160, 192, 160, 11)
    for w in (1, 3, 5, 7, 9, 11):
        assert 4 * 4 <= lib.modet_ssim_ws_bytes(1, 1, 1, 1, w) <= 5 * 4 + 64, w
        assert 0 < lib.modet_ssim_ws_bytes(2, 3, 5, 7, w) <= 5 * 4 * 210 + (1 << 20), w
    for bad in ((0, 8, 8, 8, 11), (1, 0, 8, 8, 11), (1, 8, -1, 8, 11), (1, 8, 8, 0, 11), (1, 8, 8, 8, 0), (1, 8, 8, 8, -1),
                (1, 8, 8, 8, 2), (1, 8, 8, 8, 10), (1, 8, 8, 8, 12), (1, 8, 8, 8, 13), (1, 2048, 2048, 2048, 11)):
        assert lib.modet_ssim_ws_bytes(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """NULL pointers, non-positive dims, unsupported windows and a short or misaligned workspace come back as error codes from
    the host checks (no device is touched: the pointers are never dereferenced on these paths); d_a and d_b may be NULL"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL value that is never dereferenced

    def ssim(a=p, b=p, loss=p, ws=p, nb=None, dims=(1, 8, 8, 8), window=11):
        size = lib.modet_ssim_ws_bytes(1, 8, 8, 8, 11) if nb is None else nb
        return lib.modet_ssim_fwd_bwd(a, b, loss, None, None, ws, size, *dims, window, 1.0, None)

    for k in ("a", "b", "loss", "ws"):
        assert ssim(**{k: None}) == -1, k
    for dims in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -2, 8), (1, 8, 8, 0), (1, 2048, 2048, 2048)):
        assert ssim(dims=dims, nb=1 << 40) == -2, dims
    for window in (0, -1, 2, 4, 10, 12, 13, 111):
        assert ssim(window=window, nb=1 << 30) == -3, window
    full = lib.modet_ssim_ws_bytes(1, 8, 8, 8, 11)
    assert ssim(nb=full - 1) == -4 and ssim(nb=0) == -4
    assert ssim(ws=p + 4) == -4 and ssim(ws=p + 2) == -4          # the workspace begins with doubles


def test_loss_class_refuses_what_it_cannot_compute():
    from smilecode_amd import losses, ops
    m = losses.SSIM3D()
    assert (m.window_size, m.size_average, m.channel) == (11, True, 1) and losses.SSIM3D(window_size=7).window_size == 7
    assert ops.SSIM_MAX_WINDOW == 11
    with pytest.raises(RuntimeError, match="size_average"):
        losses.SSIM3D(size_average=False)
    for bad in (0, 2, 10, 12, 13, -3, 2.5):
        with pytest.raises(RuntimeError, match="window_size"):
            losses.SSIM3D(window_size=bad)
    v = torch.zeros(1, 1, 4, 5, 6)
    for bad in (torch.zeros(4, 5, 6), torch.zeros(1, 4, 5, 6), torch.zeros(1, 2, 4, 5, 6), torch.zeros(1, 1, 0, 5, 6)):
        for name, fn in (("SSIM3D", m), ("ssim3D", losses.ssim3D)):
            with pytest.raises(RuntimeError, match=name):
                fn(bad, bad)
            with pytest.raises(RuntimeError, match=name):
                fn(v, bad)
    with pytest.raises(RuntimeError, match="differ in shape"):
        m(v, torch.zeros(1, 1, 4, 5, 7))
    with pytest.raises(RuntimeError, match="size_average"):
        losses.ssim3D(v, v, size_average=False)
    with pytest.raises(RuntimeError, match="window_size"):
        losses.ssim3D(v, v, window_size=4)
    for fn in (m, losses.ssim3D, ops.ssim_loss, ops.ssim_value_and_grad):
        with pytest.raises(RuntimeError, match="GPU"):          # no CPU fallback: a host tensor is an error, not a slow path
            fn(v, v)


def test_ops_check_arguments_before_the_launch(monkeypatch):
    """with tensors that claim to be on the GPU the argument checks still fire first: the library is never reached"""
    from smilecode_amd import _lib, losses, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["ssim"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    v = torch.zeros(1, 1, 4, 5, 6)
    with pytest.raises(RuntimeError, match="float32"):         # (the dtype is looked at before the shape is)
        ops._ssim_args("ssim_loss", _Fake(torch.float64), _Fake(torch.float64), 11)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    for fn in (ops.ssim_loss, ops.ssim_value_and_grad, losses.ssim3D):
        for bad in (0, 2, 10, 12, 13, 2.5):
            with pytest.raises(RuntimeError, match="window_size"):
                fn(v, v, window_size=bad)
    for fn in (ops.ssim_loss, ops.ssim_value_and_grad):
        with pytest.raises(RuntimeError, match="does not match"):
            fn(v, torch.zeros(1, 1, 4, 5, 7))
        with pytest.raises(RuntimeError, match="does not match"):
            fn(v, torch.zeros(2, 1, 4, 5, 6))
        with pytest.raises(RuntimeError, match=r"\(B,1,D,H,W\)"):
            fn(torch.zeros(1, 2, 4, 5, 6), torch.zeros(1, 2, 4, 5, 6))
        with pytest.raises(RuntimeError, match=r"\(B,1,D,H,W\)"):
            fn(torch.zeros(4, 5, 6), torch.zeros(4, 5, 6))
        with pytest.raises(RuntimeError, match=r"\(B,1,D,H,W\)"):
            fn(torch.zeros(1, 1, 0, 5, 6), torch.zeros(1, 1, 0, 5, 6))
    assert not [n for n, _ in px.records if guard.is_launching(n)]


class _Fake:
    """what ops._chk looks at, for the dtype refusal on a machine without a GPU"""
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype

    def is_contiguous(self):
        return True


def test_trainer_seeds_the_backward_for_the_term():
    """the kernel hands out value and gradient, so the step seeds its backward with them; exact type only: a subclass keeps the
    autograd expression"""
    from smilecode_amd import engine, losses

    class WithCl(torch.nn.Linear):
        def forward_cl(self, a, b):
            raise AssertionError("not called here")

    tr = engine.Trainer(WithCl(3, 2), sim=losses.SSIM3D())
    assert type(tr.sim) is losses.SSIM3D and tr._seedable()
    tr.seed_backward = False
    assert not tr._seedable()

    class Sub(losses.SSIM3D):
        pass
    assert not engine.Trainer(WithCl(3, 2), sim=Sub())._seedable()
    assert not engine.Trainer(torch.nn.Linear(3, 2), sim=losses.SSIM3D())._seedable()
