"""-m gpu: WHERE the SSIM3D kernels read and write -- tests/test_gpu_mi_guard.py's assertions over the family's own table
(_lib.FAMILIES["ssim"], include/modet_hip_ssim.h).  Every caller-supplied tensor sits between guard bands (tests/guard.py),
workspaces are exactly modet_ssim_ws_bytes(...) bytes, outputs and workspaces are poisoned, and the library is reached through a
recording proxy over the new table.  Per case: no band is damaged, every result is finite, the results equal an unguarded run
bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits.  Shapes have odd
dimensions, axes shorter than the window and than its halo, rows longer than the 32-voxel tile (37, 67, 35) and more rows than
its 16 (27), so partial tiles sit on every side."""
import pytest
import torch

from tests import guard
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("ssim")
px = H.fixture()


def abi_case(shape, B):
    """the C ABI directly, exact workspaces: windows 11 and 3, each with both gradients, with d_b alone, with d_a alone and with
    neither"""
    def case(g):
        from smilecode_amd import _lib
        L, gen = _lib.load(), torch.Generator().manual_seed(31)
        D, H, W = shape
        a = g(torch.rand(B, 1, D, H, W, generator=gen) * 1.2 - 0.1)
        b = g(torch.rand(B, 1, D, H, W, generator=gen) * 1.2 - 0.1)
        out = {}
        for window in (11, 3):
            nb = L.modet_ssim_ws_bytes(B, D, H, W, window)
            assert nb > 0
            for want_a, want_b in ((True, True), (False, True), (True, False), (False, False)):
                loss, ws = g.empty(1), g.ws(nb)
                d_a = g.empty(a.shape) if want_a else None
                d_b = g.empty(b.shape) if want_b else None
                pa, pb = (None if d_a is None else d_a.data_ptr()), (None if d_b is None else d_b.data_ptr())
                rc = L.modet_ssim_fwd_bwd(a.data_ptr(), b.data_ptr(), loss.data_ptr(), pa, pb, ws.data_ptr(), nb, B, D, H, W, window,
                                          0.37, stream())
                _lib.check(rc, "ssim window %d" % window)
                k = "w%d.%d%d." % (window, want_a, want_b)
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
        for name, m in (("w11", losses.SSIM3D()), ("w5", losses.SSIM3D(window_size=5))):
            loss = m(a, b)
            out[name + ".da"], out[name + ".db"] = torch.autograd.grad(loss, [a, b])
            out[name + ".loss"] = loss
            (out[name + ".db_alone"],) = torch.autograd.grad(m(a.detach(), b), [b])
        out["sim"] = losses.ssim3D(a.detach(), b.detach(), window_size=7)
        out["loss_vg"], out["d_vg"] = ops.ssim_value_and_grad(a.detach(), b.detach(), grad_scale=2.5)
        out["w9.loss_vg"], out["w9.d_vg"] = ops.ssim_value_and_grad(a.detach(), b.detach(), window_size=9, grad_scale=2.5)
        return out
    return case


CASES = {
    "abi[7x9x37]": abi_case((7, 9, 37), 1),
    "abi[9x27x67,B2]": abi_case((9, 27, 67), 2),
    "abi[3x1x5]": abi_case((3, 1, 5), 1),
    "abi[1x2x3,B2]": abi_case((1, 2, 3), 2),
    "abi[1x1x1]": abi_case((1, 1, 1), 1),
    "ops[11x13x35,B2]": ops_case((11, 13, 35), 2),
    "ops[5x3x7]": ops_case((5, 3, 7), 1),
}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_ssim_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_entry_points_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import losses, ops
    px.refuse = True
    v = torch.rand(1, 1, 4, 5, 6, device="cuda")
    w = torch.rand(1, 1, 4, 5, 7, device="cuda")
    for bad in (lambda: ops.ssim_loss(v, v[..., :5].contiguous()), lambda: ops.ssim_loss(v, w), lambda: ops.ssim_loss(v[:, 0], v[:, 0]),
                lambda: ops.ssim_loss(v.double(), v.double()), lambda: ops.ssim_value_and_grad(v.half(), v.half()),
                lambda: ops.ssim_loss(v, v, window_size=4), lambda: ops.ssim_loss(v, v, window_size=13),
                lambda: ops.ssim_loss(v, v, window_size=0), lambda: ops.ssim_value_and_grad(v, v, window_size=10),
                lambda: ops.ssim_value_and_grad(v, torch.rand(2, 1, 4, 5, 6, device="cuda")),
                lambda: ops.ssim_value_and_grad(v, w), lambda: ops.ssim_loss(v.expand(1, 2, 4, 5, 6).contiguous(), v.expand(1, 2, 4, 5, 6).contiguous()),
                lambda: ops.ssim_loss(v[:, :, :0], v[:, :, :0]),
                lambda: losses.SSIM3D()(v, w), lambda: losses.ssim3D(v, w), lambda: losses.ssim3D(v, v, size_average=False),
                lambda: losses.ssim3D(v, v, window_size=6), lambda: losses.SSIM3D()(v.double(), v.double())):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_every_launching_ssim_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table: every launching name of _lib.FAMILIES["ssim"] was
    called at least once with every device pointer inside a guarded buffer, and no case handed the library a device pointer
    outside one.  Cases deselected from this session are run here, guarded once."""
    # each gradient buffer was seen present and absent (pointer arguments: a, b, loss, d_a, d_b, ws, stream)
    H.check_coverage(px, CASES, {"modet_ssim_fwd_bwd": ((3, 4), (0, 1, 2, 5))})
