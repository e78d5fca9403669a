"""-m gpu: WHERE the mutual-information kernels read and write -- tests/test_gpu_mind_guard.py's assertions over the family's own
table (_lib.FAMILIES["mi"], include/modet_hip_mi.h).  Every caller-supplied tensor sits between guard bands (tests/guard.py),
workspaces are exactly modet_mi_ws_bytes(...) bytes, outputs and workspaces are poisoned, and the library is reached through a
recording proxy over the new table.  Per case: no band is damaged, every result is finite, the results equal an unguarded run
bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits.  Shapes have odd
dimensions, voxel counts that are no multiple of the 32-voxel gradient tile or the 64-voxel histogram step, one volume of more
than a workgroup's 4096 voxels (9x17x33 = 5049), and volumes smaller than one patch."""
import pytest
import torch

from tests import guard
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("mi")
px = H.fixture()


def abi_case(shape, B):
    """the C ABI directly, exact workspaces: the global form and the local form at patch sizes 5 and 3, each with both
    gradients, with d_b alone, with d_a alone and with neither"""
    def case(g):
        from smilecode_amd import _lib
        L, gen = _lib.load(), torch.Generator().manual_seed(31)
        D, H, W = shape
        # values from -0.1 to 1.1: both clamp ends cut
        a = g(torch.rand(B, 1, D, H, W, generator=gen) * 1.2 - 0.1)
        b = g(torch.rand(B, 1, D, H, W, generator=gen) * 1.2 - 0.1)
        out = {}
        for patch in (0, 5, 3):
            nb = L.modet_mi_ws_bytes(B, D, H, W, patch)
            assert nb > 0
            for want_a, want_b in ((True, True), (False, True), (True, False), (False, False)):
                loss, ws = g.empty(1), g.ws(nb)
                d_a = g.empty(a.shape) if want_a else None
                d_b = g.empty(b.shape) if want_b else None
                pa, pb = (None if d_a is None else d_a.data_ptr()), (None if d_b is None else d_b.data_ptr())
                if patch == 0:
                    rc = L.modet_mi_fwd_bwd(a.data_ptr(), b.data_ptr(), loss.data_ptr(), pa, pb, ws.data_ptr(), nb, B, D, H, W, 32,
                                            0.0, 1.0, 1.0, 0.37, stream())
                else:
                    rc = L.modet_lmi_fwd_bwd(a.data_ptr(), b.data_ptr(), loss.data_ptr(), pa, pb, ws.data_ptr(), nb, B, D, H, W, 32,
                                             0.0, 1.0, 1.0, patch, 0.37, stream())
                _lib.check(rc, "mi patch %d" % patch)
                k = "p%d.%d%d." % (patch, want_a, want_b)
                out[k + "loss"] = loss
                if want_a:
                    out[k + "d_a"] = d_a
                if want_b:
                    out[k + "d_b"] = d_b
        return out
    return case


def ops_case(shape, B):
    """the package's own wrappers under GuardedAlloc: their outputs, saved gradients and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import losses, ops
        gen = torch.Generator().manual_seed(32)
        D, H, W = shape
        a = g(torch.rand(B, 1, D, H, W, generator=gen)).requires_grad_(True)
        b = g(torch.rand(B, 1, D, H, W, generator=gen)).requires_grad_(True)
        out = {}
        for name, m in (("mi", losses.MutualInformation()), ("lmi", losses.localMutualInformation()),
                        ("lmi4w", losses.localMutualInformation(sigma_ratio=0.5, maxval=2.0, patch_size=4))):
            loss = m(a, b)
            out[name + ".da"], out[name + ".db"] = torch.autograd.grad(loss, [a, b])
            out[name + ".loss"] = loss
            (out[name + ".db_alone"],) = torch.autograd.grad(m(a.detach(), b), [b])
        out["mi.loss_vg"], out["mi.d_vg"] = ops.mi_value_and_grad(a.detach(), b.detach(), grad_scale=2.5)
        out["lmi.loss_vg"], out["lmi.d_vg"] = ops.lmi_value_and_grad(a.detach(), b.detach(), patch_size=7, grad_scale=2.5)
        return out
    return case


CASES = {
    "abi[7x9x37]": abi_case((7, 9, 37), 1),
    "abi[9x17x33,B2]": abi_case((9, 17, 33), 2),
    "abi[3x1x5]": abi_case((3, 1, 5), 1),
    "abi[1x2x3,B2]": abi_case((1, 2, 3), 2),
    "abi[1x1x1]": abi_case((1, 1, 1), 1),
    "ops[11x13x35,B2]": ops_case((11, 13, 35), 2),
    "ops[5x3x7]": ops_case((5, 3, 7), 1),
}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_mi_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_entry_points_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import losses, ops
    px.refuse = True
    v = torch.rand(1, 1, 4, 5, 6, device="cuda")
    w = torch.rand(1, 1, 4, 5, 7, device="cuda")
    for bad in (lambda: ops.mi_loss(v, v[..., :5].contiguous()), lambda: ops.lmi_loss(v, w), lambda: ops.mi_loss(v[:, 0], v[:, 0]),
                lambda: ops.mi_loss(v.double(), v.double()), lambda: ops.lmi_loss(v.double(), v.double()),
                lambda: ops.mi_loss(v, v, num_bin=16), lambda: ops.mi_loss(v, v, maxval=0.0), lambda: ops.mi_loss(v, v, minval=1.0),
                lambda: ops.lmi_loss(v, v, sigma_ratio=0.0), lambda: ops.lmi_loss(v, v, patch_size=0),
                lambda: ops.lmi_loss(v, v, patch_size=17), lambda: ops.lmi_value_and_grad(v, v, patch_size=32),
                lambda: ops.mi_value_and_grad(v, torch.rand(2, 1, 4, 5, 6, device="cuda")),
                lambda: ops.lmi_value_and_grad(v, w), lambda: ops.mi_value_and_grad(v, v, num_bin=64),
                lambda: losses.MutualInformation()(v, w), lambda: losses.localMutualInformation()(v, w)):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_every_launching_mi_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table: every launching name of _lib.FAMILIES["mi"] was
    called at least once with every device pointer inside a guarded buffer, and no case handed the library a device pointer
    outside one.  Cases deselected from this session are run here, guarded once."""
    # each gradient buffer was seen present and absent, for both entry points (pointer arguments: a, b, loss, d_a, d_b, ws, stream)
    H.check_coverage(px, CASES, {n: ((3, 4), (0, 1, 2, 5)) for n in ("modet_lmi_fwd_bwd", "modet_mi_fwd_bwd")})
