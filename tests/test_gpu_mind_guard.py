"""-m gpu: WHERE the MIND kernels read and write -- tests/test_gpu_guard.py's four assertions over the loss family's own table
(_lib.FAMILIES["mind"], include/modet_hip_losses.h).  Every caller-supplied tensor sits between guard bands (tests/guard.py),
workspaces are exactly modet_mind_ws_bytes(...) bytes, outputs and workspaces are poisoned, and the library is reached through a
recording proxy over the new table.  Per case: no band is damaged, every result is finite, the results equal an unguarded run
bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits.  Shapes have odd
dimensions, one smaller than the stencil's reach.  The coverage condition of the core table is restated over the new one."""
import pytest
import torch

from tests import guard
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("mind")
px = H.fixture()


def abi_case(shape, B):
    """the C ABI directly, exact workspaces: descriptor; loss + gradient; the value alone (d_b = NULL)"""
    def case(g):
        from smilecode_amd import _lib
        L, gen = _lib.load(), torch.Generator().manual_seed(31)
        D, H, W = shape
        a, b = g(torch.rand(B, 1, D, H, W, generator=gen)), g(torch.rand(B, 1, D, H, W, generator=gen))
        n1, n2 = L.modet_mind_ws_bytes(B, D, H, W, 1), L.modet_mind_ws_bytes(B, D, H, W, 2)
        assert 0 < n1 < n2
        desc, ws = g.empty((B, 12, D, H, W)), g.ws(n1)
        _lib.check(L.modet_mind_descriptor(a.data_ptr(), desc.data_ptr(), ws.data_ptr(), n1, B, D, H, W, 2, 2, stream()), "descriptor")
        loss, d_b, ws2 = g.empty(1), g.empty(b.shape), g.ws(n2)
        _lib.check(L.modet_mind_fwd_bwd(a.data_ptr(), b.data_ptr(), loss.data_ptr(), d_b.data_ptr(), ws2.data_ptr(), n2, B, D, H, W,
                                        2, 2, 0.37, stream()), "fwd_bwd")
        loss0, ws3 = g.empty(1), g.ws(n2)
        _lib.check(L.modet_mind_fwd_bwd(a.data_ptr(), b.data_ptr(), loss0.data_ptr(), None, ws3.data_ptr(), n2, B, D, H, W,
                                        2, 2, 1.0, stream()), "fwd")
        return dict(desc=desc, loss=loss, d_b=d_b, loss_nograd=loss0)
    return case


def ops_case(shape, B):
    """the package's own wrappers under GuardedAlloc: their outputs, saved gradients and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import losses, ops
        gen = torch.Generator().manual_seed(32)
        D, H, W = shape
        a = g(torch.rand(B, 1, D, H, W, generator=gen)).requires_grad_(True)
        b = g(torch.rand(B, 1, D, H, W, generator=gen)).requires_grad_(True)
        m = losses.MIND_loss()
        loss = m(a, b)
        da, db = torch.autograd.grad(loss, [a, b])
        lv, dv = ops.mind_value_and_grad(a.detach(), b.detach(), 2.5)
        return dict(loss=loss, da=da, db=db, desc=m.MINDSSC(a.detach()), loss_vg=lv, d_vg=dv)
    return case


CASES = {
    "abi[7x9x37]": abi_case((7, 9, 37), 1),
    "abi[9x17x33,B2]": abi_case((9, 17, 33), 2),
    "abi[3x1x5]": abi_case((3, 1, 5), 1),
    "abi[1x2x3,B2]": abi_case((1, 2, 3), 2),
    "ops[11x13x35,B2]": ops_case((11, 13, 35), 2),
    "ops[5x3x7]": ops_case((5, 3, 7), 1),
}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_mind_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_entry_points_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import losses, ops
    px.refuse = True
    v = torch.rand(1, 1, 4, 5, 6, device="cuda")
    for bad in (lambda: ops.mind_loss(v, v[..., :5].contiguous()), lambda: ops.mind_ssc(v[:, 0]), lambda: ops.mind_ssc(v, 3, 2),
                lambda: ops.mind_ssc(v, 2, 1), lambda: ops.mind_loss(v.double(), v.double()),
                lambda: ops.mind_value_and_grad(v, torch.rand(2, 1, 4, 5, 6, device="cuda")),
                lambda: losses.MIND_loss()(v, torch.rand(1, 1, 4, 5, 7, device="cuda"))):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_every_launching_mind_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the loss family's table: every launching name of
    _lib.FAMILIES["mind"] was called at least once with every device pointer inside a guarded buffer, and no case handed the library
    a device pointer outside one.  Cases deselected from this session are run here, guarded once."""
    # both forms of the loss call were seen: with a gradient buffer and with NULL (pointer arguments: a, b, loss, d_b, ws, stream)
    H.check_coverage(px, CASES, {"modet_mind_descriptor": ((), ()), "modet_mind_fwd_bwd": ((3,), ())})
