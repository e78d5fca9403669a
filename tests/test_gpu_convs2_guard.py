"""-m gpu: WHERE the stride-2 convolution kernels and the channel concatenation read and write -- tests/test_gpu_posenc_guard.py's
assertions over the family's own table (_lib.FAMILIES["convs2"], include/modet_hip_convs2.h).  Every caller-supplied tensor sits
between guard bands (tests/guard.py), every workspace is exactly modet_convs2_ws_bytes(..., pass) bytes, outputs and workspaces are
poisoned, and the library is reached through a recording proxy over the new table.  Per case: no band is damaged, every result is
finite, the results equal an unguarded run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives
the same bits.  The shapes: cases 1, 3, 4 and 6 of tests/test_gpu_convs2.py (odd axes with high-end padding and Cin = 1, one
output voxel at 64 -> 128, a single input voxel without activation, several workgroups with a partial last one)."""
import pytest
import torch

from tests import guard
from tests import rdn_oracle as orc
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("convs2")
px = H.fixture()


def abi_case(n, bias=True):
    """the C ABI directly, exact workspaces: forward, data gradient, weight gradient"""
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, (D_, H_, W_), Cin, Cout, slope = orc.OP_CASES[n]
        x, w, b, gy = (g(t) for t in orc.case_tensors(n))
        b = b if bias else None
        act, sl = int(slope is not None), float(slope or 0.0)
        dims = (B, D_, H_, W_, Cin, Cout)
        y, dx, dw = g.empty(gy.shape), g.empty(x.shape), g.empty(w.shape)
        db = g.empty((Cout,)) if bias else None
        p = lambda v: None if v is None else v.data_ptr()      # noqa: E731
        nbs = [L.modet_convs2_ws_bytes(*dims, k) for k in range(3)]
        assert min(nbs) > 0
        ws = [g.ws(nb) for nb in nbs]
        _lib.check(L.modet_convs2_fwd(p(x), p(w), p(b), p(y), p(ws[0]), nbs[0], *dims, act, sl, stream()), "convs2 fwd")
        ya = y if act else None
        _lib.check(L.modet_convs2_bwd_data(p(gy), p(ya), p(w), p(dx), p(ws[1]), nbs[1], *dims, act, sl, stream()), "convs2 bwd data")
        _lib.check(L.modet_convs2_bwd_weight(p(x), p(gy), p(ya), p(dw), p(db), p(ws[2]), nbs[2], *dims, act, sl, stream()), "convs2 bwd weight")
        out = {"y": y, "d_x": dx, "d_w": dw}
        if bias:
            out["d_b"] = db
        return out
    return case


def ops_case(n, bias=True):
    """the package's own wrapper under GuardedAlloc: outputs, gradients and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import ops
        slope = orc.OP_CASES[n][4]
        x, w, b, gy = (g(t) for t in orc.case_tensors(n, seed=2000 + n))
        leaves = [t.requires_grad_(True) for t in ((x, w, b) if bias else (x, w))]
        y = ops.conv3d_s2(x, w, b if bias else None, slope)
        grads = torch.autograd.grad(y, leaves, gy)
        out = {"y": y}
        out.update({"g%d" % i: v for i, v in enumerate(grads)})
        return out
    return case


def cat_abi_case(shape, C1, C2, want=(True, True)):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        gen = torch.Generator().manual_seed(31 + C1)
        a, b = g(torch.randn(shape + (C1,), generator=gen)), g(torch.randn(shape + (C2,), generator=gen))
        go = g(torch.randn(shape + (C1 + C2,), generator=gen))
        N = a.numel() // C1
        out = g.empty(go.shape)
        da, db = (g.empty(a.shape) if want[0] else None), (g.empty(b.shape) if want[1] else None)
        p = lambda v: None if v is None else v.data_ptr()      # noqa: E731
        _lib.check(L.modet_cat_channels2_fwd(p(a), p(b), p(out), N, C1, C2, stream()), "cat fwd")
        _lib.check(L.modet_cat_channels2_bwd(p(go), p(da), p(db), N, C1, C2, stream()), "cat bwd")
        res = {"out": out}
        res.update({k: v for k, v in (("d_a", da), ("d_b", db)) if v is not None})
        return res
    return case


def cat_ops_case(shape, C1, C2):
    def case(g):
        from smilecode_amd import ops
        gen = torch.Generator().manual_seed(32 + C1)
        a, b = g(torch.randn(shape + (C1,), generator=gen)), g(torch.randn(shape + (C2,), generator=gen))
        go = g(torch.randn(shape + (C1 + C2,), generator=gen))
        a.requires_grad_(True); b.requires_grad_(True)
        out = ops.cat_channels(a, b)
        da, db = torch.autograd.grad(out, [a, b], go)
        return {"out": out, "d_a": da, "d_b": db}
    return case


CASES = {}
for _n in (1, 3, 4, 6):
    CASES["abi[case%d]" % _n] = abi_case(_n)
    CASES["ops[case%d]" % _n] = ops_case(_n)
CASES["abi[case6,no bias]"] = abi_case(6, bias=False)
CASES["ops[case1,no bias]"] = ops_case(1, bias=False)
CASES["cat abi[3x5x7,8+16]"] = cat_abi_case((1, 3, 5, 7), 8, 16)
CASES["cat abi[3x3x3,3+5]"] = cat_abi_case((2, 3, 3, 3), 3, 5)
CASES["cat abi[3x5x7,4+12,d_a only]"] = cat_abi_case((1, 3, 5, 7), 4, 12, want=(True, False))
CASES["cat abi[3x3x3,1+2,d_b only]"] = cat_abi_case((1, 3, 3, 3), 1, 2, want=(False, True))
CASES["cat ops[7x9x11,4+6]"] = cat_ops_case((1, 7, 9, 11), 4, 6)
CASES["cat ops[3x5x7,16+8]"] = cat_ops_case((2, 3, 5, 7), 16, 8)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_convs2_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_wrappers_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import models, ops
    px.refuse = True
    x, w, b = torch.rand(1, 4, 5, 6, 8, device="cuda"), torch.rand(16, 8, 3, 3, 3, device="cuda"), torch.rand(16, device="cuda")
    for bad in (lambda: ops.conv3d_s2(x.double(), w, b), lambda: ops.conv3d_s2(x[0], w, b), lambda: ops.conv3d_s2(x.cpu(), w, b),
                lambda: ops.conv3d_s2(x.permute(0, 3, 2, 1, 4), w, b), lambda: ops.conv3d_s2(x, w[:, :4].contiguous(), b),
                lambda: ops.conv3d_s2(x, w, b[:8].contiguous()), lambda: ops.conv3d_s2(x, w[:6].contiguous(), b[:6].contiguous()),
                lambda: ops.conv3d_s2(x[..., :6].contiguous(), w[:, :6].contiguous(), b), lambda: ops.conv3d_s2(x, w, b, -1.0),
                lambda: ops.conv3d_s2(x, w, b, "relu"), lambda: ops.conv3d_s2(x[:0], w, b), lambda: ops.cat_channels(x, x[:, :2].contiguous()),
                lambda: ops.cat_channels(x, x.double()), lambda: ops.cat_channels(x, x[..., :0].contiguous()),
                lambda: models.RDN((32, 32, 24)), lambda: models.RDN((32, 32, 32), stage_recursion=2),
                lambda: models.RDN((32, 32, 32), channels=6), lambda: models.RDN((32, 32, 32), channels=4).cuda()(x, x)):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, channel counts outside the kernels', empty axes, a negative slope, a misaligned tensor and a short or misaligned
    workspace are answered with the library's error codes before any launch: the outputs keep their fill"""
    from smilecode_amd import _lib
    L = _lib.load()
    dims = (1, 4, 4, 4, 4, 8)
    x, w, b = torch.zeros(1, 4, 4, 4, 4, device="cuda"), torch.zeros(8, 4, 3, 3, 3, device="cuda"), torch.zeros(8, device="cuda")
    y, gy = torch.full((1, 2, 2, 2, 8), 7.0, device="cuda"), torch.ones(1, 2, 2, 2, 8, device="cuda")
    dx, dw, db = torch.full_like(x, 7.0), torch.full_like(w, 7.0), torch.full_like(b, 7.0)
    P, st = (lambda t: t.data_ptr()), stream()
    NULL, DIM, UNSUP, WS = -1, -2, -3, -4
    nb = [L.modet_convs2_ws_bytes(*dims, k) for k in range(3)]
    assert nb[0] == nb[1] == 27 * 4 * 8 * 4 and nb[2] == 2 * (27 * 4 * 8 + 8) * 4
    assert L.modet_convs2_ws_bytes(*dims, 3) == 0 and L.modet_convs2_ws_bytes(1, 4, 4, 4, 2, 8, 0) == 0
    assert L.modet_convs2_ws_bytes(1, 4, 4, 4, 4, 260, 0) == 0 and L.modet_convs2_ws_bytes(1, 0, 4, 4, 4, 8, 0) == 0
    assert L.modet_convs2_ws_bytes(1, 1024, 1024, 1024, 4, 8, 0) == 0                      # x of 2^32 elements
    ws = torch.empty(max(nb) + 32, dtype=torch.uint8, device="cuda")
    tail = (1, 0.2, st)
    assert L.modet_convs2_fwd(None, P(w), P(b), P(y), P(ws), nb[0], *dims, *tail) == NULL
    assert L.modet_convs2_fwd(P(x), P(w), P(b), None, P(ws), nb[0], *dims, *tail) == NULL
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), None, nb[0], *dims, *tail) == NULL
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), P(ws), nb[0] - 1, *dims, *tail) == WS
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), P(ws) + 4, nb[0], *dims, *tail) == WS
    assert L.modet_convs2_fwd(P(x) + 4, P(w), P(b), P(y), P(ws), nb[0], *dims, *tail) == UNSUP
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], 1, 4, 4, 4, 3, 8, *tail) == UNSUP
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], 1, 4, 4, 4, 4, 6, *tail) == UNSUP
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], 1, 4, 0, 4, 4, 8, *tail) == DIM
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], *dims, 1, -0.5, st) == UNSUP
    assert L.modet_convs2_fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], *dims, 2, 0.2, st) == UNSUP
    assert L.modet_convs2_bwd_data(P(gy), None, P(w), P(dx), P(ws), nb[1], *dims, *tail) == NULL      # act == 1 needs y
    assert L.modet_convs2_bwd_data(P(gy), P(y), P(w), None, P(ws), nb[1], *dims, *tail) == NULL
    assert L.modet_convs2_bwd_data(P(gy), P(y), P(w), P(dx), P(ws), nb[1] - 4, *dims, *tail) == WS
    assert L.modet_convs2_bwd_weight(P(x), P(gy), None, P(dw), P(db), P(ws), nb[2], *dims, *tail) == NULL
    assert L.modet_convs2_bwd_weight(P(x), P(gy), P(y), None, P(db), P(ws), nb[2], *dims, *tail) == NULL
    assert L.modet_convs2_bwd_weight(P(x), P(gy), P(y), P(dw), P(db), P(ws), nb[2] - 4, *dims, *tail) == WS
    assert L.modet_convs2_bwd_weight(P(x), P(gy), P(y), P(dw), P(db), P(ws) + 8, nb[2], *dims, *tail) == WS
    assert L.modet_cat_channels2_fwd(P(x), None, P(dx), 64, 4, 4, st) == NULL
    assert L.modet_cat_channels2_fwd(P(x), P(x), P(dx), 0, 4, 4, st) == DIM
    assert L.modet_cat_channels2_fwd(P(x), P(x), P(dx), 8, 4, 0, st) == DIM
    assert L.modet_cat_channels2_fwd(P(x), P(x), P(dx), 1 << 29, 4, 4, st) == DIM
    assert L.modet_cat_channels2_bwd(P(x), None, None, 8, 4, 4, st) == NULL
    assert L.modet_cat_channels2_bwd(P(x) + 4, P(dx), None, 8, 4, 4, st) == UNSUP
    torch.cuda.synchronize()
    for t in (y, dx, dw, db):
        assert bool((t == 7.0).all())                                   # nothing was launched


def test_every_launching_convs2_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table; the NULL-able pointers -- the forward's bias, y
    of both backward entry points (absent without an activation), the weight gradient's d_b and either output of the
    concatenation's split -- were seen both present and absent"""
    H.check_coverage(px, CASES, {
        "modet_convs2_fwd": ((2,), (0, 1, 3, 4)),                       # x w bias y ws | stream
        "modet_convs2_bwd_data": ((1,), (0, 2, 3, 4)),                  # d_y y w d_x ws | stream
        "modet_convs2_bwd_weight": ((2, 4), (0, 1, 3, 5)),              # x d_y y d_w d_b ws | stream
        "modet_cat_channels2_fwd": ((), (0, 1, 2)),                     # a b out | stream
        "modet_cat_channels2_bwd": ((1, 2), (0,)),                      # d_out d_a d_b | stream
    })
