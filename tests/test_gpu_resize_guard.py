"""-m gpu: WHERE the resize kernels read and write -- tests/test_gpu_deconv_guard.py's assertions over the family's own table
(_lib.FAMILIES["resize"], include/modet_hip_resize.h).  Every caller-supplied tensor sits between guard bands (tests/guard.py),
outputs are poisoned, and the library is reached through a recording proxy over the new table.  Per case: no band is damaged, every
result is finite, the results equal an unguarded run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and
poison gives the same bits.  The shapes: cases 1, 5, 6 and 7 of tests/test_gpu_resize.py (the largest ratio, whose last stencil ends
on the last input voxel; the 16-byte rows while upsampling; axes of one voxel on either side; the widest gather window, clamped at
both ends) and pyramid cases 2 and 3 (down to one voxel per sample; odd sizes, whose last input planes no output of the coarser
levels reads), with every output and cotangent once absent."""
import pytest
import torch

from tests import guard
from tests import rdn_stages_oracle as orc
from tests.guard_family import DIM, NULL, Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("resize")
px = H.fixture()


def _p(t):
    return None if t is None else t.data_ptr()


def abi_case(n):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, si, so, C, scale = orc.OP_CASES[n]
        x, gy = (g(t) for t in orc.case_tensors(n))
        y, dx = g.empty(gy.shape), g.empty(x.shape)
        _lib.check(L.modet_resize_fwd(_p(x), _p(y), B, *si, *so, C, scale, stream()), "resize fwd")
        _lib.check(L.modet_resize_bwd(_p(gy), _p(dx), B, *si, *so, C, scale, stream()), "resize bwd")
        return {"y": y, "d_x": dx}
    return case


def ops_case(n):
    def case(g):
        from smilecode_amd import ops
        B, si, so, C, scale = orc.OP_CASES[n]
        x, gy = (g(t) for t in orc.case_tensors(n, seed=5000 + n))
        x.requires_grad_(True)
        y = ops.resize(x, so, scale)
        (dx,) = torch.autograd.grad(y, [x], gy)
        return {"y": y, "d_x": dx}
    return case


def pyramid_abi_case(n, keep, add):
    """keep: which of the three outputs / cotangents are passed; add: None, 'own' (a tensor of its own) or 'alias' (d_x itself)"""
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, (D, Hh, W) = orc.PYRAMID_CASES[n]
        t = orc.pyramid_tensors(n)
        x = g(t[0])
        gys = [g(t[1 + i]) if keep[i] else None for i in range(3)]
        ys = [g.empty(t[1 + i].shape) if keep[i] else None for i in range(3)]
        _lib.check(L.modet_resize_pyramid_fwd(_p(x), *(_p(y) for y in ys), B, D, Hh, W, stream()), "pyramid fwd")
        if add == "alias":
            dx = g(t[4])
            a = dx
        else:
            dx, a = g.empty(x.shape), (g(t[4]) if add == "own" else None)
        _lib.check(L.modet_resize_pyramid_bwd(*(_p(v) for v in gys), _p(a), _p(dx), B, D, Hh, W, stream()), "pyramid bwd")
        out = {"y%d" % (2 << i): y for i, y in enumerate(ys) if y is not None}
        out["d_x"] = dx
        return out
    return case


def pyramid_ops_case(n):
    def case(g):
        from smilecode_amd import ops
        t = orc.pyramid_tensors(n, seed=6000 + n)
        x = g(t[0]).requires_grad_(True)
        fs = ops.flow_pyramid(x)
        (dx,) = torch.autograd.grad(fs, [x], [g(v) for v in t[1:4]])
        return {"f2": fs[0], "f4": fs[1], "f8": fs[2], "d_x": dx}
    return case


CASES = {}
for _n in (1, 5, 6, 7):
    CASES["abi[case%d]" % _n] = abi_case(_n)
    CASES["ops[case%d]" % _n] = ops_case(_n)
CASES["pyramid abi[case2,all]"] = pyramid_abi_case(2, (True, True, True), None)
CASES["pyramid abi[case3,all,add]"] = pyramid_abi_case(3, (True, True, True), "own")
CASES["pyramid abi[case3,all,alias]"] = pyramid_abi_case(3, (True, True, True), "alias")
CASES["pyramid abi[case3,only 2]"] = pyramid_abi_case(3, (True, False, False), None)
CASES["pyramid abi[case3,only 4]"] = pyramid_abi_case(3, (False, True, False), "own")
CASES["pyramid abi[case2,only 8]"] = pyramid_abi_case(2, (False, False, True), None)
CASES["pyramid ops[case2]"] = pyramid_ops_case(2)
CASES["pyramid ops[case3]"] = pyramid_ops_case(3)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_resize_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_wrappers_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import ops
    px.refuse = True
    x = torch.rand(1, 8, 8, 8, 3, device="cuda")
    for bad in (lambda: ops.resize(x.double(), (4, 4, 4)), lambda: ops.resize(x[0], (4, 4, 4)), lambda: ops.resize(x.cpu(), (4, 4, 4)),
                lambda: ops.resize(x.permute(0, 3, 2, 1, 4), (4, 4, 4)), lambda: ops.resize(x, (4, 4, 0)), lambda: ops.resize(x, (4, 4)),
                lambda: ops.resize(x[:0], (4, 4, 4)), lambda: ops.resize(x, (4, 4, 4), float("inf")),
                lambda: ops.flow_pyramid(x[..., :2].contiguous()), lambda: ops.flow_pyramid(x[:, :, :7].contiguous()),
                lambda: ops.flow_pyramid(x.double()), lambda: ops.flow_pyramid(x[0])):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, sizes and channel counts outside the kernels' are answered with the library's error codes before any launch:
    the outputs keep their fill"""
    from smilecode_amd import _lib
    L = _lib.load()
    x = torch.zeros(1, 8, 8, 8, 3, device="cuda")
    outs = [torch.full((1, n, n, n, 3), 7.0, device="cuda") for n in (4, 2, 1, 8)]
    y2, y4, y8, dx = outs
    p, s = x.data_ptr(), stream()
    assert L.modet_resize_fwd(None, _p(y2), 1, 8, 8, 8, 4, 4, 4, 3, 1.0, s) == NULL
    assert L.modet_resize_fwd(p, None, 1, 8, 8, 8, 4, 4, 4, 3, 1.0, s) == NULL
    assert L.modet_resize_bwd(_p(y2), None, 1, 8, 8, 8, 4, 4, 4, 3, 1.0, s) == NULL
    for dims in ((0, 8, 8, 8, 4, 4, 4, 3), (1, 8, 8, 8, 4, 0, 4, 3), (1, 8, 8, 8, 4, 4, 4, 0), (1, 8, 8, 8, 4, 4, 4, 257),
                 (65536, 8, 8, 8, 4, 4, 4, 3), (1, 8, -8, 8, 4, 4, 4, 3)):
        assert L.modet_resize_fwd(p, _p(y2), *dims, 1.0, s) == DIM and L.modet_resize_bwd(_p(y2), _p(dx), *dims, 1.0, s) == DIM, dims
    assert L.modet_resize_fwd(p, _p(y2), 1, 8, 8, 8, 4, 4, 4, 3, float("nan"), s) == DIM
    assert L.modet_resize_pyramid_fwd(p, None, None, None, 1, 8, 8, 8, s) == NULL
    assert L.modet_resize_pyramid_fwd(None, _p(y2), _p(y4), _p(y8), 1, 8, 8, 8, s) == NULL
    assert L.modet_resize_pyramid_bwd(None, None, None, p, _p(dx), 1, 8, 8, 8, s) == NULL
    assert L.modet_resize_pyramid_bwd(_p(y2), _p(y4), _p(y8), None, None, 1, 8, 8, 8, s) == NULL
    for dims in ((1, 7, 8, 8), (1, 8, 8, 4), (0, 8, 8, 8), (65536, 8, 8, 8)):
        assert L.modet_resize_pyramid_fwd(p, _p(y2), _p(y4), _p(y8), *dims, s) == DIM, dims
        assert L.modet_resize_pyramid_bwd(_p(y2), _p(y4), _p(y8), None, _p(dx), *dims, s) == DIM, dims
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)                      # nothing was launched


def test_every_launching_resize_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table; the NULL-able pointers -- the pyramid's three
    outputs, its three cotangents and d_x_add -- were seen both present and absent"""
    H.check_coverage(px, CASES, {
        "modet_resize_fwd": ((), (0, 1)),                               # x y | stream
        "modet_resize_bwd": ((), (0, 1)),                               # d_y d_x | stream
        "modet_resize_pyramid_fwd": ((1, 2, 3), (0,)),                  # x y2 y4 y8 | stream
        "modet_resize_pyramid_bwd": ((0, 1, 2, 3), (4,)),               # d_y2 d_y4 d_y8 d_x_add d_x | stream
    })
