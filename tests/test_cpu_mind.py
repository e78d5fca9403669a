"""MIND-SSC without a GPU: the fp64 restatement against the reference's recorded results, the loss family's header against its
ctypes table and the library's exports, and the argument checks of losses.MIND_loss."""
import numpy as np
import pytest
import torch

from tests.guard_family import check_family_table
from tests import mind_oracle
from tests.util import gold

CASES = ("pair16", "pair12x20x28", "noise2x10x12x14", "tiny3x4x5")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize("tag", CASES)
def test_restatement_equals_the_reference_golden(tag):
    """tests/mind_oracle.py (gather form, fp64) against what the reference's MIND_loss returned for the same images
    (tests/golden/make_goldens_mind.py): loss, descriptor and both gradients to fp64 rounding"""
    g = gold("op_mind.npz")
    a, b = T(g[tag + ".a"]), T(g[tag + ".b"])
    loss, da, db = mind_oracle.value_and_grads(mind_oracle.mind_loss, a, b, torch.float64)
    want = float(g[tag + ".loss"])
    assert abs(float(loss) - want) <= 1e-13 * abs(want), (float(loss), want)
    for got, ref in ((da, T(g[tag + ".da"])), (db, T(g[tag + ".db"]))):
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    zs = [int(z) for z in g[tag + ".mind_a_z"]]
    desc = mind_oracle.mind_ssc(a)[:, :, zs]
    ref = T(g[tag + ".mind_a"])
    assert desc.shape == ref.shape and desc.shape[1] == 12
    assert float((desc - ref).abs().max()) <= 1e-12


def test_aten_composition_equals_the_gather_form_in_fp64():
    """the two restatements are the same function: the fp32 run of the composition is the yardstick of the GPU parity test"""
    g = gold("op_mind.npz")
    for tag in ("noise2x10x12x14", "tiny3x4x5"):
        a, b = T(g[tag + ".a"]), T(g[tag + ".b"])
        l1, da1, db1 = mind_oracle.value_and_grads(mind_oracle.mind_loss, a, b, torch.float64)
        l2, da2, db2 = mind_oracle.value_and_grads(mind_oracle.mind_loss_aten, a, b, torch.float64)
        assert abs(float(l1) - float(l2)) <= 1e-13 * abs(float(l1))
        assert float((da1 - da2).abs().max()) <= 1e-12 * float(da1.abs().max())
        assert float((db1 - db2).abs().max()) <= 1e-12 * float(db1.abs().max())


def test_loss_header_table_and_exports_agree():
    """every name include/modet_hip_losses.h declares has a signature in _lib.FAMILIES["mind"] and is exported by the library, and
    the table holds nothing else and shares no name with another family (tests/guard_family.py)"""
    lib = check_family_table("mind", {"modet_mind_ws_bytes", "modet_mind_descriptor", "modet_mind_fwd_bwd"},
                             ["modet_mind_descriptor", "modet_mind_fwd_bwd"])
    # host-side answers (no device needed): 12 volumes per image + partials; bad arguments give 0
    n = 160 * 192 * 160
    assert lib.modet_mind_ws_bytes(1, 160, 192, 160, 1) >= 12 * n * 4
    assert 2 * 12 * n * 4 <= lib.modet_mind_ws_bytes(1, 160, 192, 160, 2) < 2 * 12 * n * 4 + (1 << 20)
    assert lib.modet_mind_ws_bytes(1, 3, 4, 5, 2) > 0
    for bad in ((0, 8, 8, 8, 1), (1, 0, 8, 8, 1), (1, 8, -1, 8, 2), (1, 8, 8, 0, 2), (1, 8, 8, 8, 0), (1, 8, 8, 8, 3)):
        assert lib.modet_mind_ws_bytes(*bad) == 0, bad


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL pointers, non-positive dims, another radius or dilation and a short workspace come back as error codes from the host
    checks (no device is touched: the pointers are never dereferenced on these paths)"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL value that is never dereferenced
    nb = lib.modet_mind_ws_bytes(1, 8, 8, 8, 2)
    assert lib.modet_mind_fwd_bwd(None, p, p, p, p, nb, 1, 8, 8, 8, 2, 2, 1.0, None) == -1
    assert lib.modet_mind_fwd_bwd(p, p, None, p, p, nb, 1, 8, 8, 8, 2, 2, 1.0, None) == -1
    assert lib.modet_mind_fwd_bwd(p, p, p, p, None, nb, 1, 8, 8, 8, 2, 2, 1.0, None) == -1
    assert lib.modet_mind_fwd_bwd(p, p, p, p, p, nb, 1, 0, 8, 8, 2, 2, 1.0, None) == -2
    assert lib.modet_mind_fwd_bwd(p, p, p, p, p, nb, 1, 8, 8, 8, 1, 2, 1.0, None) == -3
    assert lib.modet_mind_fwd_bwd(p, p, p, p, p, nb, 1, 8, 8, 8, 2, 1, 1.0, None) == -3
    assert lib.modet_mind_fwd_bwd(p, p, p, p, p, nb - 1, 1, 8, 8, 8, 2, 2, 1.0, None) == -4
    nb1 = lib.modet_mind_ws_bytes(1, 8, 8, 8, 1)
    assert lib.modet_mind_descriptor(p, None, p, nb1, 1, 8, 8, 8, 2, 2, None) == -1
    assert lib.modet_mind_descriptor(p, p, p, nb1, 1, 8, 8, -3, 2, 2, None) == -2
    assert lib.modet_mind_descriptor(p, p, p, nb1, 1, 8, 8, 8, 3, 2, None) == -3
    assert lib.modet_mind_descriptor(p, p, p, nb1 - 1, 1, 8, 8, 8, 2, 2, None) == -4


def test_mind_loss_refuses_what_it_cannot_compute():
    from smilecode_amd import losses, ops
    m = losses.MIND_loss(win=[9, 9, 9])
    assert m.win == [9, 9, 9]
    v = torch.zeros(1, 1, 4, 5, 6)
    for bad in (torch.zeros(4, 5, 6), torch.zeros(1, 4, 5, 6), torch.zeros(1, 2, 4, 5, 6), torch.zeros(1, 1, 0, 5, 6)):
        with pytest.raises(RuntimeError, match="MIND_loss"):
            m(bad, bad)
        with pytest.raises(RuntimeError, match="MIND_loss"):
            m(v, bad)
    with pytest.raises(RuntimeError, match="differ in shape"):
        m(v, torch.zeros(1, 1, 4, 5, 7))
    with pytest.raises(RuntimeError, match="differ in shape"):
        m(torch.zeros(2, 1, 4, 5, 6), v)
    with pytest.raises(RuntimeError, match="GPU"):              # no CPU fallback: a host tensor is an error, not a slow path
        m(v, v)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mind_ssc(v)


def test_trainer_seeds_the_backward_for_a_mind_term():
    """engine.Trainer(sim=...): None keeps NCC_vxm; MIND_loss is a term whose kernel hands out value and gradient, so the step
    seeds its backward with it; a subclass or an unknown module keeps the autograd expression"""
    from smilecode_amd import engine, losses

    class WithCl(torch.nn.Linear):
        def forward_cl(self, a, b):
            raise AssertionError("not called here")

    assert type(engine.Trainer(WithCl(3, 2)).sim) is losses.NCC_vxm
    tr = engine.Trainer(WithCl(3, 2), sim=losses.MIND_loss())
    assert type(tr.sim) is losses.MIND_loss and tr._seedable()
    tr.seed_backward = False
    assert not tr._seedable()
    tr.seed_backward = True
    tr.reg = losses.Grad3d(penalty="l2", loss_mult=2)
    assert not tr._seedable()

    class Sub(losses.MIND_loss):
        pass
    assert not engine.Trainer(WithCl(3, 2), sim=Sub())._seedable()
    assert not engine.Trainer(WithCl(3, 2), sim=torch.nn.MSELoss())._seedable()
    assert not engine.Trainer(torch.nn.Linear(3, 2), sim=losses.MIND_loss())._seedable()
