"""-m gpu: WHERE the flow-regulariser kernels read and write -- tests/test_gpu_ssim_guard.py's assertions over the family's own table
(_lib.FAMILIES["reg"], include/modet_hip_reg.h).  Every caller-supplied tensor sits between guard bands (tests/guard.py),
workspaces are exactly modet_reg_ws_bytes(...) bytes, outputs and workspaces are poisoned, and the library is reached through a
recording proxy over the new table.  Per case: no band is damaged, every result is finite, the results equal an unguarded run
bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits.  The stencils reach 1, 2 and
4 voxels along every axis, so the shapes are each kind's minimum (where every neighbour but the voxel itself is outside), odd
sizes with every voxel in bending's shell (5^3, 7 x 9 x 37) and one with interior voxels and rows longer than a wave (9 x 27 x 67),
in both layouts, with the gradient present and absent."""
import pytest
import torch

from tests import guard
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("reg")
px = H.fixture()


def abi_case(kind, shape, B, C=3):
    """the C ABI directly, exact workspaces: planar and (C = 3) channels-last, each with and without d_f"""
    def case(g):
        from smilecode_amd import _lib, ops
        L, gen = _lib.load(), torch.Generator().manual_seed(31)
        D, H, W = shape
        planar = torch.randn(B, C, D, H, W, generator=gen)
        kid = ops.REG_KINDS[kind]
        nb = L.modet_reg_ws_bytes(kid, B, C, D, H, W)
        assert nb > 0
        out = {}
        for cl in ((0, 1) if C == 3 else (0,)):
            f = g(planar.permute(0, 2, 3, 4, 1).contiguous() if cl else planar)
            for want in (True, False):
                loss, ws = g.empty(1), g.ws(nb)
                d_f = g.empty(f.shape) if want else None
                rc = L.modet_reg_fwd_bwd(f.data_ptr(), loss.data_ptr(), None if d_f is None else d_f.data_ptr(), ws.data_ptr(), nb, kid,
                                         B, C, D, H, W, cl, 0.37, stream())
                _lib.check(rc, "reg %s" % kind)
                k = "cl%d.%d." % (cl, want)
                out[k + "loss"] = loss
                if want:
                    out[k + "d_f"] = d_f
        return out
    return case


def ops_case(shape, B):
    """the package's own wrappers under GuardedAlloc: their outputs, saved gradients and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import losses, ops
        gen = torch.Generator().manual_seed(32)
        D, H, W = shape
        planar = torch.randn(B, 3, D, H, W, generator=gen)
        f = g(planar).requires_grad_(True)
        f_cl = g(planar.permute(0, 2, 3, 4, 1).contiguous())
        out = {}
        terms = [("itv", losses.Grad3DiTV())] + [(k, losses.DisplacementRegularizer(k)) for k in ALL[1:]]
        for kind, m in terms:
            loss = m(f, None)
            (out[kind + ".df"],) = torch.autograd.grad(loss, [f])
            out[kind + ".loss"] = loss
            out[kind + ".loss_nograd"] = m(f.detach(), None)
            out[kind + ".loss_vg"], out[kind + ".d_vg"] = ops.reg_value_and_grad_cl(f_cl, kind, grad_scale=2.5)
        return out
    return case


ALL = ("itv", "gradient-l2", "gradient-l1", "bending")
SHAPES = {"itv": [((5, 5, 5), 2), ((7, 9, 37), 1), ((9, 27, 67), 2), ((2, 2, 2), 1), ((2, 3, 35), 1)],
          "gradient-l2": [((5, 5, 5), 2), ((7, 9, 37), 1), ((9, 27, 67), 2), ((3, 3, 3), 1)],
          "gradient-l1": [((5, 5, 5), 2), ((7, 9, 37), 1), ((9, 27, 67), 2), ((3, 3, 3), 1)],
          "bending": [((5, 5, 5), 2), ((7, 9, 37), 1), ((9, 27, 67), 2)]}
CASES = {"abi[%s,%dx%dx%d,B%d]" % ((kind,) + shape + (B,)): abi_case(kind, shape, B) for kind in ALL for shape, B in SHAPES[kind]}
CASES["abi[itv,C2,2x3x35,B2]"] = abi_case("itv", (2, 3, 35), 2, C=2)
CASES["ops[11x13x35,B2]"] = ops_case((11, 13, 35), 2)
CASES["ops[5x6x7]"] = ops_case((5, 6, 7), 1)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_reg_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_entry_points_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import losses, ops
    px.refuse = True
    v = torch.rand(1, 3, 9, 9, 9, device="cuda")
    v_cl = v.permute(0, 2, 3, 4, 1).contiguous()
    bend, itv = losses.DisplacementRegularizer("bending"), losses.Grad3DiTV()
    for bad in (lambda: ops.reg_loss(v, "bend"), lambda: ops.reg_loss(v[0], "bending"), lambda: ops.reg_loss(v.double(), "bending"),
                lambda: ops.reg_loss(v.half(), "itv"), lambda: ops.reg_loss(v.permute(0, 1, 4, 3, 2), "gradient-l2"),
                lambda: ops.reg_loss(v[:, :2].contiguous(), "bending"), lambda: ops.reg_loss(v[:, :2].contiguous(), "gradient-l1"),
                lambda: ops.reg_loss(v[:, :, :4].contiguous(), "bending"), lambda: ops.reg_loss(v[..., :2].contiguous(), "gradient-l2"),
                lambda: ops.reg_loss(v[:, :, :, :1].contiguous(), "itv"), lambda: ops.reg_loss(v[:0], "itv"),
                lambda: ops.reg_value_and_grad_cl(v, "bending"), lambda: ops.reg_value_and_grad_cl(v, "itv"),
                lambda: ops.reg_value_and_grad_cl(v_cl[..., :2].contiguous(), "itv"), lambda: ops.reg_value_and_grad_cl(v_cl, "tv"),
                lambda: ops.reg_value_and_grad_cl(v_cl[:, :4].contiguous(), "bending"), lambda: ops.reg_value_and_grad_cl(v_cl.double(), "itv"),
                lambda: ops.reg_value_and_grad_cl(v_cl[:, ::2], "gradient-l2"),
                lambda: bend(v[:, :2].contiguous(), None), lambda: bend(v[:, :, :, :4].contiguous(), None), lambda: bend(v[0], None),
                lambda: bend(v.double(), None), lambda: itv(v[..., :1].contiguous(), None), lambda: itv(v[0], None), lambda: itv(v.half(), None)):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_every_launching_reg_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table: every launching name of _lib.FAMILIES["reg"] was
    called at least once with every device pointer inside a guarded buffer, and no case handed the library a device pointer
    outside one.  Cases deselected from this session are run here, guarded once."""
    # the gradient buffer was seen present and absent (pointer arguments: f, loss, d_f, ws, stream)
    H.check_coverage(px, CASES, {"modet_reg_fwd_bwd": ((2,), (0, 1, 3))})
